// RUNGEMM, frame-staged kernels for the mask layer (the last decoder layer: N = 16 output columns, no BatchNorm statistics) and for its input gradient.
//
// Both launches run with nothing beside them in the step and moved every operand byte many times on the kernels they had (profiles/thin_mask_notes.md):
// the forward (phase-merged transposed conv, K = 2 frames x 3 positions x 64 channels) sent every input position L2 -> LDS six times on rungemm_kernel
// and filled half of a 32-wide MFMA tile; the input gradient (K = 2 frames x 5 positions x 8 channels, 64 columns to two destinations) is bound by its
// stores and reached them through a 2 KB per-wave transpose on rundirect_kernel.  Here
//   * the weights live in registers for the life of a wave, as the A operand of v_mfma_f32_16x16x32_bf16 (rows = output columns): 12 K steps x 4 VGPRs
//     for the forward, 3 K steps x 4 column tiles x 4 VGPRs for the gradient.  The accumulator of a 16-position block is 4 registers per column tile and
//     a lane holds CONSECUTIVE output channels of ONE position, so the results leave as 16-byte stores without an LDS transpose;
//   * forward: a workgroup owns a run of consecutive output frames (batch items back to back) and keeps the two input frames an output frame needs in a
//     ring of three LDS slots (positions -1 .. Fo of both sources, channels side by side, XOR-swizzled 16-byte chunks; positions -1 and Fo are zero).  The
//     third slot is being filled by LDS-DMA while a frame is multiplied: every input frame is fetched ONCE per workgroup (plus one at the start of its
//     run).  A frame outside [0, Tin) - the frame before an item's first, the frame behind its last - is fetched from the zero page: no branch around
//     a load, and the frame behind an item's last one is the frame before the next item's first one, so the ring carries over batch boundaries;
//   * input gradient: one tap of one position is one 16-byte chunk of the upstream gradient; the B fragments come straight from global memory (the 32 MB
//     tensor stays in L2, no LDS), one block of chunks in flight ahead of the block being multiplied.  The weight rows are permuted so that the two column
//     tiles of a 32-channel group give a lane 8 consecutive channels: a wave stores 16 positions x 64 bytes = 1 KB contiguous per destination;
//   * persistent grids (resident workgroups); no flag, wait or atomic between workgroups - every output element has one writer.
// Same descriptors as the kernels replaced and the same order of the runs in k; the 16-column MFMA groups the sums differently and the zero padding of
// the runs is skipped, so equality of the bits is not promised (measured equal on the benchmark shapes, profiles/thin_mask_notes.md).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "sefd_desc.h"
#include "tuning.h"
#include "dev_common.h"
#include "launch_common.h"
#include "thin_common.h"

namespace sefd {

namespace {

constexpr int kMaskFo = 128;                    // output positions per frame the forward kernel is built for (4 waves x 2 blocks of 16)
constexpr int64_t kThinMaskMinRows = 262144;    // default rule: smaller launches stay on the kernels they had

__device__ __forceinline__ int fdivm(int x, uint32_t m, uint32_t s) { return m ? (int)(__umulhi((uint32_t)x, m) >> s) : x; }

// ------------------------------------------------------------------------------------------------------------ forward
// C: channels per source (two sources).  LDS image of a frame: [Fo + 2 positions][2 C channels] bf16, position index = input bin + 1, the 16-byte chunk c
// of position p stored at chunk c ^ swz(p): the 16 lanes of one ds_read_b128 group (16 different positions, one or two chunk columns) spread over the
// 64 banks (CDNA4: 256-byte bank lines) without a padded pitch - conflict-free for the first tap, a few 2-way pairs for the other two
// (profiles/thin_mask_notes.md) - and three slots stay under a third of the CU's LDS.
template <int C>
struct MaskFwdGeom {
  static constexpr int CH = 2 * C / 8;          // 16-byte chunks per position
  static constexpr int PB = CH * 16;            // bytes per position
  static constexpr int SLOT = (kMaskFo + 2) * PB;
  static constexpr int CPT = C / 8;             // chunks per tap of one source
  static constexpr int KS = 12 * C / 32;        // K steps of 32: 2 sources x 2 frames x 3 taps x C channels
  static constexpr int NIT = kMaskFo * CH / 256;   // LDS-DMA instructions per thread per frame
  static constexpr int RPL = 256 / PB;          // positions per bank line
  static_assert(C % 16 == 0 && C <= 32 && NIT >= 1, "instantiated channel counts");
  __host__ __device__ static constexpr int swz(int pos) { return (pos / RPL) & (CH - 1); }
};

}  // namespace

template <int C>
__global__ __launch_bounds__(256) void thin_mask_fwd_kernel(const RunGemm d, const ArenaBases ab) {
  using G = MaskFwdGeom<C>;
  constexpr int CH = G::CH, PB = G::PB, SLOT = G::SLOT, CPT = G::CPT, KS = G::KS, NIT = G::NIT;
  __shared__ __attribute__((aligned(16))) char smem[3 * SLOT];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, q = lane >> 4;

  // ---- this workgroup's run of output frames g = b * Tout + u
  const int Tout = d.Tout, Tin = d.Tin[0];
  const int64_t nframes = d.M / kMaskFo;
  const int g0 = (int)((int64_t)blockIdx.x * nframes / gridDim.x), g1 = (int)((int64_t)(blockIdx.x + 1) * nframes / gridDim.x);
  if (g0 >= g1) return;

  const uint16_t* x0 = reinterpret_cast<const uint16_t*>(rp(ab, d.x[0]));
  const uint16_t* x1 = reinterpret_cast<const uint16_t*>(rp(ab, d.x[1]));
  const uint16_t* zp = reinterpret_cast<const uint16_t*>(rp(ab, d.zero));
  const uint16_t* w = reinterpret_cast<const uint16_t*>(rp(ab, d.w));
  uint16_t* y = reinterpret_cast<uint16_t*>(rp(ab, d.y));

  // ---- weights (A operand: row = output column li, k = 8 q .. + 7 of every K step) and the LDS offsets of the matching B fragments, once
  const int ko0 = d.seg[0].koff, ko1 = d.seg[1].koff, ko2 = d.seg[2].koff, ko3 = d.seg[3].koff;
  uint4 wreg[KS];
  int aoff[KS];
  bool akw[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    int tg, cc;                                  // tap counted over the four runs (run = tg / 3: source, frame), chunk inside the tap
    if constexpr (CPT >= 4) { tg = ks / (CPT / 4); cc = (ks % (CPT / 4)) * 4 + q; }
    else { const int ci = ks * 4 + q; tg = ci / CPT; cc = ci % CPT; }
    const int sg = tg / 3, tap = tg - 3 * sg;
    const int ko = sg == 0 ? ko0 : sg == 1 ? ko1 : sg == 2 ? ko2 : ko3;
    wreg[ks] = *reinterpret_cast<const uint4*>(w + (int64_t)li * d.ldw + ko + tap * C + cc * 8);
    const int pos = wid * 32 + li + tap;         // LDS position of tap `tap` of output position wid * 32 + li (input bin f - 1 + tap)
    aoff[ks] = pos * PB + ((((sg >> 1) * CPT + cc) ^ G::swz(pos)) << 4);
    akw[ks] = (sg & 1) != 0;                     // second run of a source: the frame before
  }
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (d.bias.arena >= 0) {
    const float* bp = reinterpret_cast<const float*>(rp(ab, d.bias));
#pragma unroll
    for (int e = 0; e < 4; ++e) bias4[e] = bp[4 * q + e];
  }

  // ---- this thread's share of a frame's LDS-DMA: chunks L = it * 256 + tid of positions 1 .. Fo, swizzle applied on the source side
  int eoff[NIT];
  bool esrc[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int L = it * 256 + tid, pos = 1 + L / CH, c = (L % CH) ^ G::swz(pos);
    esrc[it] = c >= CPT;
    eoff[it] = (pos - 1) * C + (c % CPT) * 8;
  }
  const uint32_t lbase = lds_addr(smem) + PB + wid * 1024;
  const int64_t bs0 = d.bstride[0], bs1 = d.bstride[1];
  const int ts0 = d.tstride[0], ts1 = d.tstride[1], ba0 = d.base[0], ba1 = d.base[1];
  auto issue_frame = [&](int b, int u, bool valid, int slot) {
    const uint16_t* f0 = x0 + (int64_t)b * bs0 + ba0 + (int64_t)u * ts0;
    const uint16_t* f1 = x1 + (int64_t)b * bs1 + ba1 + (int64_t)u * ts1;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const uint16_t* src = valid ? (esrc[it] ? f1 : f0) + eoff[it] : zp;
      dma16(src, lbase + slot + it * 4096);
    }
  };
  // positions 0 and Fo + 1 of every slot: zero, never written again
  if (tid < 6 * CH) {
    const int slot = tid / (2 * CH), r = tid % (2 * CH);
    *reinterpret_cast<uint4*>(smem + slot * SLOT + (r < CH ? 0 : (kMaskFo + 1) * PB) + (r % CH) * 16) = make_uint4(0, 0, 0, 0);
  }

  int cb = g0 / Tout, cu = g0 - cb * Tout;
  int sp = 0, sc = SLOT, sn = 2 * SLOT;          // slots of the frame before, this frame, the next frame
  issue_frame(cb, cu - 1, cu > 0 && cu - 1 < Tin, sp);
  issue_frame(cb, cu, cu < Tin, sc);
  int nb = cb, nu = cu + 1;
  if (nu == Tout) { nu = 0; ++nb; }
  const int f0 = wid * 32 + li;
  const bool odd = (q & 1) != 0;

  for (int g = g0; g < g1; ++g) {
    wait_vm<0>();                                // this thread's chunks of frame g (and of everything before it) have landed
    lds_barrier();                               // ... everyone's; and nobody reads slot `sn` (the frame before frame g - 1) any more
    if (g + 1 < g1) issue_frame(nb, nu, nu < Tin, sn);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    uint4 a0[KS], a1[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const char* p = smem + (akw[ks] ? sp : sc) + aoff[ks];
      a0[ks] = *reinterpret_cast<const uint4*>(p);
      a1[ks] = *reinterpret_cast<const uint4*>(p + 16 * PB);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wreg[ks]), __builtin_bit_cast(bf16x8, a0[ks]), acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wreg[ks]), __builtin_bit_cast(bf16x8, a1[ks]), acc1, 0, 0, 0);
    }
    settle(acc0, acc1);
    // lane (position li, q): columns 4 q .. + 3 of positions f0 (acc0) and f0 + 16 (acc1).  The lanes q and q ^ 1 trade halves: the even one leaves with
    // columns 4 q .. + 7 of position f0, the odd one with columns 4 (q - 1) .. + 7 of position f0 + 16 - whole 8-channel output positions
    // (the bias is added to the finished sum, as rungemm_kernel does: with the same order of the runs in k the two kernels then round alike)
    acc0 += bias4; acc1 += bias4;
    const uint32_t X0 = pack_bf16x2(acc0[0], acc0[1]), X1 = pack_bf16x2(acc0[2], acc0[3]);
    const uint32_t Y0 = pack_bf16x2(acc1[0], acc1[1]), Y1 = pack_bf16x2(acc1[2], acc1[3]);
    const uint32_t r0 = (uint32_t)__shfl_xor((int)(odd ? X0 : Y0), 16), r1 = (uint32_t)__shfl_xor((int)(odd ? X1 : Y1), 16);
    const uint4 out = odd ? make_uint4(r0, r1, Y0, Y1) : make_uint4(X0, X1, r0, r1);
    const int f = odd ? f0 + 16 : f0, n0 = odd ? 4 * (q - 1) : 4 * q;
    *reinterpret_cast<uint4*>(y + (int64_t)cb * d.y_bstride + (int64_t)cu * d.y_tstride + (int64_t)f * d.y_fstride + d.y_off + n0) = out;
    cb = nb; cu = nu;
    if (++nu == Tout) { nu = 0; ++nb; }
    const int t = sp; sp = sc; sc = sn; sn = t;
  }
}

// ------------------------------------------------------------------------------------------------------------ input gradient
// NT: 16-column tiles (N = 16 NT).  Column tiles 2 p and 2 p + 1 cover columns 32 p .. + 31: MFMA row r of tile 2 p + h is column 32 p + 8 (r / 4) + 4 h
// + r % 4, so that lane (position, q) ends with columns 32 p + 8 q .. + 7 in its two accumulators.
template <int NT>
__global__ __launch_bounds__(256) void thin_mask_dgrad_kernel(const RunGemm d, const ArenaBases ab) {
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, q = lane >> 4;
  const uint16_t* x = reinterpret_cast<const uint16_t*>(rp(ab, d.x[0]));
  const uint16_t* zp = reinterpret_cast<const uint16_t*>(rp(ab, d.zero));
  const uint16_t* w = reinterpret_cast<const uint16_t*>(rp(ab, d.w));
  uint16_t* y = reinterpret_cast<uint16_t*>(rp(ab, d.y));
  uint16_t* y2 = d.n2 > 0 ? reinterpret_cast<uint16_t*>(rp(ab, d.y2)) - d.n2 : y;       // second destination of the columns n >= n2
  const int n2 = d.n2 > 0 ? d.n2 : 0x7fffffff;

  // ---- K step ks, lane group q: the 16-byte chunk c = 4 ks + q of the 10 (2 runs x 5 taps of 8 channels); chunks 10, 11 are zero
  const int dt0 = d.seg[0].dt, dt1 = d.seg[1].dt, of0 = d.seg[0].off, of1 = d.seg[1].off, ko0 = d.seg[0].koff, ko1 = d.seg[1].koff;
  const int ts = d.tstride[0], Tin = d.Tin[0], rowlen = d.rowlen[0], fs = d.fstride[0];
  int cdt[3], crel[3], coff[3];
  bool cok[3];
  uint4 wreg[NT][3];
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    const int c = ks * 4 + q, kw = c >= 5 ? 1 : 0, tap = c - 5 * kw;
    cok[ks] = c < 10;
    cdt[ks] = kw ? dt1 : dt0;
    crel[ks] = (kw ? of1 : of0) + tap * 8;
    coff[ks] = cdt[ks] * ts + crel[ks];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = 32 * (t >> 1) + 8 * (li >> 2) + 4 * (t & 1) + (li & 3);
      const uint16_t* wp = cok[ks] ? w + (int64_t)n * d.ldw + (kw ? ko1 : ko0) + tap * 8 : zp;
      wreg[t][ks] = *reinterpret_cast<const uint4*>(wp);
    }
  }

  // ---- this workgroup's range of 16-row blocks; its waves take them in turn
  const int nblk = (d.M + 15) >> 4;
  const int bs = (int)((int64_t)blockIdx.x * nblk / gridDim.x), be = (int)((int64_t)(blockIdx.x + 1) * nblk / gridDim.x);
  const int TF = d.Tout * d.Fo;
  // the three chunks of row blk * 16 + li (every load is issued: an invalid chunk, or a block past the end, reads the zero page); returns the row's
  // output offset, -1 for no row
  auto load = [&](int blk, uint4 (&a)[3]) -> int64_t {
    const int m = blk * 16 + li;
    const bool rv = blk < be && m < d.M;
    const int mm = rv ? m : 0;
    const int b = fdivm(mm, d.div_tf_m, d.div_tf_s), rem = mm - b * TF;
    const int u = fdivm(rem, d.div_fo_m, d.div_fo_s), f = rem - u * d.Fo;
    const uint16_t* row = x + (int64_t)b * d.bstride[0] + d.base[0] + (int64_t)u * ts + f * fs;
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      const int tt = u + cdt[ks], r = f * fs + crel[ks];
      const bool ok = rv && cok[ks] && tt >= 0 && tt < Tin && r >= 0 && r + 8 <= rowlen;
      a[ks] = *reinterpret_cast<const uint4*>(ok ? row + coff[ks] : zp);
    }
    return rv ? (int64_t)b * d.y_bstride + (int64_t)u * d.y_tstride + (int64_t)f * d.y_fstride + d.y_off : -1;
  };

  int blk = bs + wid;
  if (blk >= be) return;
  uint4 a[3];
  int64_t yo = load(blk, a);
  for (; blk < be; blk += 4) {
    uint4 an[3];
    const int64_t yon = load(blk + 4, an);
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 3; ++ks)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wreg[t][ks]), __builtin_bit_cast(bf16x8, a[ks]), acc[t], 0, 0, 0);
    if constexpr (NT == 4) settle(acc[0], acc[1], acc[2], acc[3]); else settle(acc[0], acc[1]);
#pragma unroll
    for (int p = 0; p < NT / 2; ++p) {
      const uint4 out = make_uint4(pack_bf16x2(acc[2 * p][0], acc[2 * p][1]), pack_bf16x2(acc[2 * p][2], acc[2 * p][3]),
                                   pack_bf16x2(acc[2 * p + 1][0], acc[2 * p + 1][1]), pack_bf16x2(acc[2 * p + 1][2], acc[2 * p + 1][3]));
      const int n0 = 32 * p + 8 * q;
      if (yo >= 0) *reinterpret_cast<uint4*>((n0 >= n2 ? y2 : y) + yo + n0) = out;
    }
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) a[ks] = an[ks];
    yo = yon;
  }
}

// ------------------------------------------------------------------------------------------------------------ selection
namespace {

// What both forms share: thin_common.h's plain bf16 launch, without statistics, in whole frames.
bool mask_common(const RunGemm& d) {
  if (!thin_plain_bf16(d)) return false;
  return d.stats.arena < 0 && d.zero.arena >= 0 && d.M > 0 && d.Tout > 0 && d.Fo > 0 && (int64_t)d.M % ((int64_t)d.Tout * d.Fo) == 0;
}

// Forward: the phase-merged transposed conv of a layer without statistics - two sources of C channels each, runs (source 0 frame u, frame u - 1, source 1
// frame u, frame u - 1) of 3 positions from bin f - 1, 16 output columns ([phase][8 channels]).  Returns C, 0: not this form or a C that is not built.
int mask_fwd_form(const RunGemm& d) {
  if (!mask_common(d) || d.N != 16 || d.n2 != 0 || d.Fo != kMaskFo || d.nseg != 4 || d.x[1].arena < 0) return 0;
  const int C = d.fstride[0];
  if (C <= 0 || C % 8 != 0 || d.fstride[1] != C || d.Tin[0] != d.Tin[1] || d.Tout <= d.Tin[0]) return 0;
  for (int s = 0; s < 2; ++s)
    if (d.rowlen[s] != d.Fo * C || d.tstride[s] % 8 != 0 || d.base[s] % 8 != 0 || d.bstride[s] % 8 != 0) return 0;
  for (int sg = 0; sg < 4; ++sg) {
    const Seg& s = d.seg[sg];
    if (s.src != (sg >> 1) || s.dt != -(sg & 1) || s.off != -C || s.len != 3 * C || s.koff % 8 != 0 || s.koff < 0 || s.koff + s.len > d.ldw) return 0;
  }
  return (C == 32 || C == 16) ? C : 0;           // the instantiated channel counts
}

// Input gradient: one source of 8 buffer channels per position, two runs (frames) of 5 positions, 32 or 64 columns, optionally split over two
// destinations at a multiple of 8.  Returns the number of 16-column tiles, 0: not this form.
int mask_dgrad_form(const RunGemm& d) {
  if (!mask_common(d) || d.nseg != 2 || d.bias.arena >= 0 || (d.N != 32 && d.N != 64)) return 0;
  if (d.n2 != 0 && (d.n2 < 0 || d.n2 % 8 != 0 || d.n2 >= d.N || d.y2.arena < 0)) return 0;
  if (d.fstride[0] % 8 != 0 || d.tstride[0] % 8 != 0 || d.base[0] % 8 != 0 || d.bstride[0] % 8 != 0 || d.rowlen[0] % 8 != 0) return 0;
  for (int sg = 0; sg < 2; ++sg) {
    const Seg& s = d.seg[sg];
    if (s.src != 0 || s.len != 40 || s.off % 8 != 0 || s.koff % 8 != 0 || s.koff < 0 || s.koff + s.len > d.ldw) return 0;
  }
  return d.N / 16;
}

// The instantiated forms.  fwd: the forward with key = C channels per source; else the input gradient with key = 16-column tiles.
struct MaskRow { bool fwd; int key; GemmKernel kern; int fallback; };      // fallback: resident workgroups per CU without a device
constexpr MaskRow kMaskRows[] = {
    {true, 32, &thin_mask_fwd_kernel<32>, 3},
    {true, 16, &thin_mask_fwd_kernel<16>, 6},
    {false, 4, &thin_mask_dgrad_kernel<4>, 4},
    {false, 2, &thin_mask_dgrad_kernel<2>, 4},
};
constexpr int kMaskForms = sizeof(kMaskRows) / sizeof(kMaskRows[0]);
std::atomic<int> g_mask_resident[kMaskForms];

// Row of kMaskRows that runs `d`, -1: neither form
int mask_form(const RunGemm& d) {
  const int cf = mask_fwd_form(d), nt = cf ? 0 : mask_dgrad_form(d);
  if (!cf && !nt) return -1;
  for (int i = 0; i < kMaskForms; ++i)
    if (kMaskRows[i].fwd == (cf != 0) && kMaskRows[i].key == (cf ? cf : nt)) return i;
  return -1;
}

}  // namespace

// Knobs, read per launch (launch_common.h): THIN_MASK with the default rule "launches of at least kThinMaskMinRows rows", THIN_MASK_GRID.
// A workgroup's units: frames (forward); blocks of 16 rows, four waves a workgroup (input gradient).
bool thin_mask_choose(const RunGemm& d, KernelChoice* c) {
  const int mode = (int)tune_int("THIN_MASK", 1);
  if (mode <= 0) return false;
  const int form = mask_form(d);
  if (form < 0 || !knob_takes(mode, d.M >= kThinMaskMinRows)) return false;
  const MaskRow& r = kMaskRows[form];
  const int64_t units = r.fwd ? d.M / kMaskFo : (((int64_t)d.M + 15) / 16 + 3) / 4;
  *c = KernelChoice{kFamThinMask, form, cap_grid(knob_grid(tune_int("THIN_MASK_GRID", 0), resident_wgs_per_cu(g_mask_resident[form], r.kern, 256, r.fallback)), units)};
  return true;
}

void thin_mask_launch(const RunGemm& d, const KernelChoice& c, const ArenaBases& ab, hipStream_t st) {
  hipLaunchKernelGGL(kMaskRows[c.form].kern, dim3(c.grid), dim3(256), 0, st, d, ab);
}

}  // namespace sefd
