// RUNGEMM, frame-staged kernels for the thin layers next to the mask layer, in two forms (profiles/thin_stage_notes.md).  The strided form (the second encoder
// layer's forward conv, the second-to-last decoder layer's input gradient) has its own heading further down.  First the phase-merged form,
// the kernel for the thin phase-merged launches with N = C output columns: the second-to-last decoder layer's forward conv (dec4: two
// sources of C channels, frames u and u - 1, BatchNorm statistics rows in the epilogue) and the second encoder layer's input gradient (enc1: one source,
// frames u + 1 and u, no statistics).  It is thin_mask_fwd_kernel's form (thin_mask.hip) with more output columns than one wave can hold weights for:
//   * the output columns are split over the waves of a workgroup.  A wave keeps the weights of ONE 16-column tile in registers for its life, as the A
//     operand of v_mfma_f32_16x16x32_bf16 (rows = output columns): K / 32 steps x 4 VGPRs - 96 at K = 768.  A 32 x 32 x 16 tile would halve the LDS bytes
//     per FLOP but needs 192 weight registers per wave: two waves per SIMD where the LDS ring allows three, and no room for the B fragments in flight;
//   * every wave multiplies its column tile with ALL the positions of a frame (C = 64: four waves x four 16-position blocks; C = 32: two column tiles x
//     two halves of the frame), reading the B fragments from the LDS image of the frame: [Fo + 2 positions][sources x C channels] bf16, position index =
//     input bin + 1, positions 0 and Fo + 1 zero, the 16-byte chunk c of position p at chunk c ^ swz(p) - no padded pitch, a ring of three slots is under
//     a third of the CU's LDS;
//   * a workgroup owns a run of consecutive output frames g = b * Tout + u and walks them in ascending order.  Output frame u reads input frames u + hi
//     and u + hi - 1 (hi = 0 for the decoder, 1 for the encoder gradient): the ring holds them while the third slot is filled by LDS-DMA with the frame the
//     next step needs.  A frame outside [0, Tin) comes from the zero page by pointer select.  Where the zero frame behind an item's last frame is also
//     the frame before the next item's first one (decoder: Tout = Tin + 1) the ring carries over the batch boundary as it is; where it is not (encoder
//     gradient: the next item starts with two frames the ring does not hold) the walk takes one step without output per item, which only loads;
//   * a lane's accumulator is 4 consecutive columns of one position; the lanes q and q ^ 1 trade halves of two position blocks and leave with 8
//     consecutive columns of one position: 16-byte stores without an LDS transpose;
//   * statistics (d.stats): row m / 128 = two consecutive output frames (Fo = 64) holds the sum and the sum of squares of the fp32 result (accumulator +
//     bias) before it is rounded.  Every workgroup's run starts at an even frame, so a row has ONE writer, and inside a row the sums are formed in the
//     order of the kernels replaced (chain32 below): the partial rows keep their bits, whatever the grid;
//   * persistent grid (resident workgroups); no flag, wait or atomic between workgroups.
// Same descriptors as the kernels replaced, the same order of the runs in k, the bias added to the finished sum and the statistics in their order: outputs
// and partial rows are bit-equal to theirs on every shape tested (tests/test_gpu_thin_stage.py asserts it on two small plans; the 16-column MFMA and the
// skipped zero padding of the runs changed no rounding).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "sefd_desc.h"
#include "tuning.h"
#include "dev_common.h"
#include "launch_common.h"
#include "thin_common.h"

namespace sefd {

namespace {

constexpr int kStageFo = 64;                     // output positions per frame the kernel is built for
constexpr int kStage64Fo = 32;                   // ... of the strided form at 64 channels (thin_stage64_choose)
constexpr int64_t kThinStageMinRows = 262144;    // default rule: smaller launches stay on the kernels they had

// Statistics in the order of the kernels replaced (rungemm_persist.hip, rungemm_kernel), so that the partial rows - and with them every step of a training
// run - keep their bits: a 128-row statistics block is four groups of 32 rows; in a group a column has two chains (rows 4 hh + 8 k + r, k and r
// ascending, hh = 0 / 1) that start at 0.f and add one value / fuse one square after the other; a group's sum is chain 0 + chain 1, the block's the groups'
// sums added in ascending order to 0.f.  Here a group is two 16-position blocks (a, b) with one row per lane li, so a chain walks the lanes 4 hh .. + 3,
// 8 + 4 hh .. + 3 of block a and then of block b: the running value moves from lane to lane by DPP row shifts (all q rows of the wave in step).  The
// group's sum and sum of squares arrive in lane li == 11; the other lanes hold values nobody reads.
__device__ __forceinline__ void chain32(float a, float b, float& t1, float& t2) {
  constexpr int SHR1 = 0x111, SHR5 = 0x115, SHL11 = 0x10B, SHL4 = 0x104;     // row_shr:n lane i <- lane i - n; row_shl:n lane i <- lane i + n
  float s = 0.f + a, r = __builtin_fmaf(a, a, 0.f);
#pragma unroll
  for (int k = 0; k < 3; ++k) { s = dpp_f<SHR1>(s) + a; r = __builtin_fmaf(a, a, dpp_f<SHR1>(r)); }
  s = dpp_f<SHR5>(s) + a; r = __builtin_fmaf(a, a, dpp_f<SHR5>(r));          // lanes 8, 12 go on from lanes 3, 7
#pragma unroll
  for (int k = 0; k < 3; ++k) { s = dpp_f<SHR1>(s) + a; r = __builtin_fmaf(a, a, dpp_f<SHR1>(r)); }
  s = dpp_f<SHL11>(s) + b; r = __builtin_fmaf(b, b, dpp_f<SHL11>(r));        // lanes 0, 4 of block b go on from lanes 11, 15
#pragma unroll
  for (int k = 0; k < 3; ++k) { s = dpp_f<SHR1>(s) + b; r = __builtin_fmaf(b, b, dpp_f<SHR1>(r)); }
  s = dpp_f<SHR5>(s) + b; r = __builtin_fmaf(b, b, dpp_f<SHR5>(r));
#pragma unroll
  for (int k = 0; k < 3; ++k) { s = dpp_f<SHR1>(s) + b; r = __builtin_fmaf(b, b, dpp_f<SHR1>(r)); }
  t1 = s + dpp_f<SHL4>(s);                                                    // lane 11: chain 0 + chain 1 (lane 15)
  t2 = r + dpp_f<SHL4>(r);
}
__device__ __forceinline__ void chain32(const f32x4& a, const f32x4& b, f32x4& t1, f32x4& t2) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { float x, y; chain32(a[e], b[e], x, y); t1[e] = x; t2[e] = y; }
}

// C: channels per source and output columns; NSRC: sources
template <int C, int NSRC>
struct StageGeom {
  static constexpr int CH = NSRC * C / 8;        // 16-byte chunks per position
  static constexpr int PB = CH * 16;             // bytes per position
  static constexpr int SLOT = (kStageFo + 2) * PB;
  static constexpr int CPT = C / 8;              // chunks per tap of one source
  static constexpr int HS = C / 32;              // K steps of 32 per tap
  static constexpr int NSEG = 2 * NSRC;          // runs: (source, frame)
  static constexpr int KS = NSEG * 3 * HS;       // K steps
  static constexpr int NIT = kStageFo * CH / 256;   // LDS-DMA instructions per thread per frame
  static constexpr int RPL = PB >= 256 ? 1 : 256 / PB;   // positions per bank line
  static constexpr int NT = C / 16;              // 16-column tiles
  static constexpr int NPG = 4 / NT;             // position groups: waves that share a column tile
  static constexpr int NB = kStageFo / 16 / NPG; // 16-position blocks per wave
  static constexpr int RED = NPG > 1 ? 2 * 4 * 2 * 4 * 16 : 0;   // bytes of the statistics hand-over between the waves of a column tile: [frame of the row][wave][sum, squares][q] x 16
  static_assert((C == 64 || C == 32) && (NSRC == 1 || NSRC == 2) && NIT >= 1 && NB % 2 == 0 && NT * NPG == 4 && (NPG == 1 || NB == 2), "instantiated forms");
  __host__ __device__ static constexpr int swz(int pos) { return (pos / RPL) & (CH - 1); }
};

}  // namespace

// (three waves per SIMD: what the LDS ring of the two-source form allows - 168 registers hold its 96 of weights)
template <int C, int NSRC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void thin_stage_pm_kernel(const RunGemm d, const ArenaBases ab) {
  using G = StageGeom<C, NSRC>;
  constexpr int CH = G::CH, PB = G::PB, SLOT = G::SLOT, CPT = G::CPT, HS = G::HS, NSEG = G::NSEG, KS = G::KS, NIT = G::NIT, NT = G::NT, NB = G::NB;
  __shared__ __attribute__((aligned(16))) char smem[3 * SLOT + G::RED];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, q = lane >> 4;
  const int ct = wid % NT, pg = wid / NT;        // this wave's column tile and position group

  // ---- this workgroup's run of output frames g = b * Tout + u, whole statistics rows (two frames)
  const int Tout = d.Tout, Tin = d.Tin[0];
  const int nframes = (int)(d.M / kStageFo), nrows = (nframes + 1) >> 1;
  const int g0 = 2 * (int)((int64_t)blockIdx.x * nrows / gridDim.x);
  int g1 = 2 * (int)((int64_t)(blockIdx.x + 1) * nrows / gridDim.x);
  if (g1 > nframes) g1 = nframes;
  if (g0 >= g1) return;

  const uint16_t* x0 = reinterpret_cast<const uint16_t*>(rp(ab, d.x[0]));
  const uint16_t* x1 = NSRC > 1 ? reinterpret_cast<const uint16_t*>(rp(ab, d.x[1])) : x0;
  const uint16_t* zp = reinterpret_cast<const uint16_t*>(rp(ab, d.zero));
  const uint16_t* w = reinterpret_cast<const uint16_t*>(rp(ab, d.w));
  uint16_t* y = reinterpret_cast<uint16_t*>(rp(ab, d.y));
  float* part = d.stats.arena >= 0 ? reinterpret_cast<float*>(rp(ab, d.stats)) : nullptr;

  // ---- the two frames of an output frame: u + hi (slot `sc`) and u + hi - 1 (slot `sp`)
  const int hi = d.seg[0].dt > d.seg[1].dt ? d.seg[0].dt : d.seg[1].dt;
  bool alo[NSEG];
#pragma unroll
  for (int sg = 0; sg < NSEG; ++sg) alo[sg] = d.seg[sg].dt != hi;
  // the zero frame behind an item's last output frame serves as the frame before the next item's first one; else: one loading step per item
  const int ustart = (hi == 0 && Tout - 1 >= Tin) ? 0 : -1;

  // ---- weights (A operand: row = output column 16 ct + li, k = 8 q .. + 7 of every K step) and the LDS offsets of the matching B fragments, once
  uint4 wreg[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int tg = ks / HS, half = ks % HS, sg = tg / 3, tap = tg - 3 * sg;
    wreg[ks] = *reinterpret_cast<const uint4*>(w + (int64_t)(16 * ct + li) * d.ldw + d.seg[sg].koff + tap * C + (half * 4 + q) * 8);
  }
  // offset of tap `tap` of output position pg * 16 NB + li (input bin f - 1 + tap) with chunk q; the chunk of (source s, half) is this XOR a constant,
  // because the swizzle is an XOR and a position's bytes start at a multiple of PB
  int abase[3];
#pragma unroll
  for (int tap = 0; tap < 3; ++tap) {
    const int pos = pg * 16 * NB + li + tap;
    abase[tap] = pos * PB + ((q ^ G::swz(pos)) << 4);
  }
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (d.bias.arena >= 0) {
    const float* bp = reinterpret_cast<const float*>(rp(ab, d.bias));
#pragma unroll
    for (int e = 0; e < 4; ++e) bias4[e] = bp[16 * ct + 4 * q + e];
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
  const int64_t bs0 = d.bstride[0], bs1 = d.bstride[NSRC - 1];
  const int ts0 = d.tstride[0], ts1 = d.tstride[NSRC - 1], ba0 = d.base[0], ba1 = d.base[NSRC - 1];
  auto issue_frame = [&](int b, int t, int slot) {
    const bool valid = t >= 0 && t < Tin;
    const uint16_t* f0 = x0 + (int64_t)b * bs0 + ba0 + (int64_t)t * ts0;
    const uint16_t* f1 = x1 + (int64_t)b * bs1 + ba1 + (int64_t)t * ts1;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const uint16_t* src = valid ? (esrc[it] ? f1 : f0) + eoff[it] : zp;
      dma16(src, lbase + slot + it * 4096);
    }
  };
  // positions 0 and Fo + 1 of every slot: zero, never written again
  if (tid < 6 * CH) {
    const int slot = tid / (2 * CH), r = tid % (2 * CH);
    *reinterpret_cast<uint4*>(smem + slot * SLOT + (r < CH ? 0 : (kStageFo + 1) * PB) + (r % CH) * 16) = make_uint4(0, 0, 0, 0);
  }

  int cb = g0 / Tout, cu = g0 - cb * Tout;
  int sp = 0, sc = SLOT, sn = 2 * SLOT;          // slots of frame u + hi - 1, of frame u + hi, of the next step's frame
  issue_frame(cb, cu + hi - 1, sp);
  issue_frame(cb, cu + hi, sc);
  int nb = cb, nu = cu + 1;
  if (nu == Tout) { nu = ustart; ++nb; }
  const bool odd = (q & 1) != 0;
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;      // statistics of this lane's 4 columns over the row so far
  int left = g1 - g0;                            // output frames to go
  // the weights have landed: a wait the compiler sees, so that it does not carry their pending loads into the loop and count the LDS-DMAs and the
  // stores of a frame against them (vmcnt(0), expcnt and lgkmcnt left alone)
  __builtin_amdgcn_s_waitcnt(0x0F70);

  while (left > 0) {
    wait_vm<0>();                                // this thread's chunks of the newest frame (and of everything before it) have landed
    lds_barrier();                               // ... everyone's; and nobody reads slot `sn` any more
    const bool out = cu >= 0;                    // (a step with cu = -1 only moves the ring on to the next item's first two frames)
    if (left - (out ? 1 : 0) > 0) issue_frame(nb, nu + hi, sn);
    if (out) {
      const int g = g1 - left;
      f32x4 acc[NB];
#pragma unroll
      for (int blk = 0; blk < NB; ++blk) acc[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
      // the B fragments of K step ks + 1 are read while step ks is multiplied.  (Slot bases are multiples of PB: the XOR that selects source and half
      // commutes with them, and is not hoisted out of the frame loop into twelve registers of offsets.)
      auto frag = [&](int ks, uint4 (&b)[NB]) {
        const int tg = ks / HS, half = ks % HS, sg = tg / 3, tap = tg - 3 * sg;
        const int off = ((alo[sg] ? sp : sc) + abase[tap]) ^ ((((sg >> 1) * CPT + half * 4)) << 4);
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) b[blk] = *reinterpret_cast<const uint4*>(smem + off + blk * 16 * PB);
      };
      uint4 bf[2][NB];
      frag(0, bf[0]);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks + 1 < KS) frag(ks + 1, bf[(ks + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);       // (the scheduler otherwise sinks the reads to their uses to save registers: two in flight per wave)
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
          acc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wreg[ks]), __builtin_bit_cast(bf16x8, bf[ks & 1][blk]), acc[blk], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (NB == 4) settle(acc[0], acc[1], acc[2], acc[3]); else settle(acc[0], acc[1]);
      // the bias is added to the finished sum, as rungemm_kernel does
#pragma unroll
      for (int blk = 0; blk < NB; ++blk) acc[blk] += bias4;

      if (part) {
        // (order: see chain32.  A wave's pair of blocks is one 32-row group; the sums sit in lane li == 11)
        const int fr = (g - g0) & 1;
        const bool rowend = fr != 0 || left == 1;  // the row's last frame (the launch's last row may be a single frame)
        float* prow = part + (int64_t)(g >> 1) * 2 * d.Npad + 16 * ct + 4 * q;
        if constexpr (G::NPG == 1) {
          if (fr == 0) { s1 = f32x4{0.f, 0.f, 0.f, 0.f}; s2 = s1; }
#pragma unroll
          for (int j = 0; j < NB / 2; ++j) {
            f32x4 t1, t2;
            chain32(acc[2 * j], acc[2 * j + 1], t1, t2);
            s1 += t1; s2 += t2;
          }
          if (rowend && li == 11) {
            *reinterpret_cast<f32x4*>(prow) = s1;
            *reinterpret_cast<f32x4*>(prow + d.Npad) = s2;
          }
        } else {
          // the waves of a column tile own one group each: they meet in LDS at the end of the row and are added in the order (frame, group) to 0.f.
          // The area is written again behind at least one frame barrier, which the readers reach with their reads retired
          f32x4* red = reinterpret_cast<f32x4*>(smem + 3 * SLOT);
          f32x4 t1, t2;
          chain32(acc[0], acc[1], t1, t2);
          if (li == 11) { red[((fr * 4 + wid) * 2 + 0) * 4 + q] = t1; red[((fr * 4 + wid) * 2 + 1) * 4 + q] = t2; }
          if (rowend) {
            lds_barrier();
            if (pg == 0 && li == 11) {
              f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1;
              for (int f = 0; f <= fr; ++f)
#pragma unroll
                for (int h = 0; h < G::NPG; ++h) { a1 += red[((f * 4 + ct + h * NT) * 2 + 0) * 4 + q]; a2 += red[((f * 4 + ct + h * NT) * 2 + 1) * 4 + q]; }
              *reinterpret_cast<f32x4*>(prow) = a1;
              *reinterpret_cast<f32x4*>(prow + d.Npad) = a2;
            }
          }
        }
      }

      // lane (position li, q): columns 16 ct + 4 q .. + 3 of the positions of its blocks.  Per pair of blocks the lanes q and q ^ 1 trade halves: the even
      // one leaves with columns 4 q .. + 7 of the first block's position, the odd one with columns 4 (q - 1) .. + 7 of the second block's
      uint16_t* yrow = y + (int64_t)cb * d.y_bstride + (int64_t)cu * d.y_tstride + d.y_off + 16 * ct + (odd ? 4 * (q - 1) : 4 * q);
#pragma unroll
      for (int j = 0; j < NB / 2; ++j) {
        const f32x4 &A = acc[2 * j], &B = acc[2 * j + 1];
        const uint32_t X0 = pack_bf16x2(A[0], A[1]), X1 = pack_bf16x2(A[2], A[3]);
        const uint32_t Y0 = pack_bf16x2(B[0], B[1]), Y1 = pack_bf16x2(B[2], B[3]);
        const uint32_t r0 = (uint32_t)__shfl_xor((int)(odd ? X0 : Y0), 16), r1 = (uint32_t)__shfl_xor((int)(odd ? X1 : Y1), 16);
        const uint4 o4 = odd ? make_uint4(r0, r1, Y0, Y1) : make_uint4(X0, X1, r0, r1);
        const int f = pg * 16 * NB + 16 * (2 * j + (odd ? 1 : 0)) + li;
        *reinterpret_cast<uint4*>(yrow + (int64_t)f * d.y_fstride) = o4;
      }
      --left;
    }
    cb = nb; cu = nu;
    if (++nu == Tout) { nu = ustart; ++nb; }
    const int t = sp; sp = sc; sc = sn; sn = t;
  }
}

// ------------------------------------------------------------------------------------------------------------ strided form
// The second encoder layer's forward conv (enc1: statistics, bias) and the input gradient of the second-to-last decoder layer (dec4: 32 NCP columns split
// at n2 over two destinations): one source of C channels, two runs (frames u + hi, u + hi - 1) of 5 positions from input position 2 f - 2, 64 output
// positions per frame from 128 input positions.  thin_mask_dgrad_kernel's arithmetic (a tap of C = 32 channels is one K step, the weight rows permuted
// so that the two column tiles of a 32-column pair give a lane 8 consecutive columns: 16-byte stores without an exchange) on the frame walk above: at
// this size the operand of the forward no longer sits in L2, so the frames are staged in LDS and each is fetched once per workgroup.
//   * LDS image of a frame: the even and the odd input positions in two planes of [Fo + 2 rows][C channels] (row = (position + 2) / 2, rows 0 and Fo + 1
//     zero), so that the 16 output positions of a block read 16 CONSECUTIVE rows of one plane for every tap (a stride of two positions would use half
//     the banks); chunk c of row r at c ^ swz(r);
//   * wave w: column pair w % NCP, position group w / NCP: half a frame (two blocks of 16 positions), the whole frame at NCP = 4.  At NCP = 1 (the
//     small plans' forward) the waves 2 and 3 only load;
//   * FO, the output positions per frame, is a parameter of the geometry.  <64, 4, 32> is the next class up (profiles/thin_stage64_notes.md; selected by
//     thin_stage64_choose under a knob of its own): 64 channels, 128 columns, K = 640 - the third encoder layer's forward conv and the two input gradients
//     of the third-to-last decoder layer.  Four waves x 32 columns hold the 160 KB of weights in 160 registers each (two workgroups per CU); per wave and
//     frame the MFMAs (80) and the fragment reads (40) are those of <32, 4, 64>.  A statistics row is four frames there.
namespace {

// FO: output positions per frame (2 FO input positions).  At C = 64, FO = 32 (the third encoder layer's forward conv, the third-to-last decoder layer's
// input gradients: 128 columns, K = 640) a wave holds 160 registers of weights and a frame is ONE 32-row statistics group; the statistics then go
// through an fp32 tile of the frame in LDS (TILE, see the kernel).
template <int C, int NCP, int FO>
struct StrideGeom {
  static constexpr int CPT = C / 8;              // 16-byte chunks per position
  static constexpr int PB = CPT * 16;            // bytes per position
  static constexpr int PLANE = (FO + 2) * PB;
  static constexpr int SLOT = 2 * PLANE;
  static constexpr int KS = 2 * 5 * C / 32;      // K steps: 2 runs x 5 taps x C channels
  static constexpr int NIT = 2 * FO * CPT / 256;
  static constexpr int RPL = 256 / PB;           // rows per bank line
  static constexpr int FPR = 128 / FO;           // frames per statistics row
  static constexpr int NPH = NCP == 4 ? 1 : 2;         // position groups: waves that share a column pair, one 32-row statistics group each (a whole frame at NPH = 1)
  static constexpr int NB = FO / 16 / NPH;       // 16-position blocks per wave
  static constexpr int RED = NPH > 1 ? 2 * 4 * 2 * 8 * 16 : 0;   // statistics hand-over: [frame of the row][wave][sum, squares][q][h] x 16 bytes
  static constexpr bool TILE = FO == 32;         // statistics chains walked by one lane per (column, chain) over the frame's fp32 tile in LDS
  static constexpr int TP = 32 * NCP + 4;        // ... its pitch in floats: the two chains of a column start 4 rows apart, 16 banks apart
  static constexpr int TILEB = TILE ? 32 * TP * 4 : 0;
  static_assert((!TILE || FPR == 4) && ((FO == 64 && (C == 32 || C == 16) && (NCP == 1 || NCP == 2 || NCP == 4)) || (FO == 32 && C == 64 && NCP == 4)) && NIT >= 1 &&
                (2 * 5 * C) % 32 == 0 && NB % 2 == 0 && (!TILE || (NPH == 1 && NB == 2)), "instantiated forms");
  __host__ __device__ static constexpr int swz(int row) { return (row / RPL) & (CPT - 1); }
};

}  // namespace

template <int C, int NCP, int FO = kStageFo>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NCP == 4 ? 2 : 3))) void thin_stage_st_kernel(const RunGemm d, const ArenaBases ab) {
  using G = StrideGeom<C, NCP, FO>;
  constexpr int CPT = G::CPT, PB = G::PB, PLANE = G::PLANE, SLOT = G::SLOT, KS = G::KS, NIT = G::NIT, NB = G::NB, FPR = G::FPR;
  __shared__ __attribute__((aligned(16))) char smem[3 * SLOT + G::RED + G::TILEB];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, q = lane >> 4;
  const int cp = wid % NCP, ph = wid / NCP;      // this wave's column pair and position group
  const bool active = ph < G::NPH;               // (wave-uniform)

  const int Tout = d.Tout, Tin = d.Tin[0];
  const int nframes = (int)(d.M / FO), nrows = (nframes + FPR - 1) / FPR;
  const int g0 = FPR * (int)((int64_t)blockIdx.x * nrows / gridDim.x);
  int g1 = FPR * (int)((int64_t)(blockIdx.x + 1) * nrows / gridDim.x);
  if (g1 > nframes) g1 = nframes;
  if (g0 >= g1) return;

  const uint16_t* x0 = reinterpret_cast<const uint16_t*>(rp(ab, d.x[0]));
  const uint16_t* zp = reinterpret_cast<const uint16_t*>(rp(ab, d.zero));
  const uint16_t* w = reinterpret_cast<const uint16_t*>(rp(ab, d.w));
  uint16_t* y = reinterpret_cast<uint16_t*>(rp(ab, d.y));
  uint16_t* y2 = d.n2 > 0 ? reinterpret_cast<uint16_t*>(rp(ab, d.y2)) - d.n2 : y;       // second destination of the columns n >= n2
  const int n2 = d.n2 > 0 ? d.n2 : 0x7fffffff;
  float* part = d.stats.arena >= 0 ? reinterpret_cast<float*>(rp(ab, d.stats)) : nullptr;

  const int hi = d.seg[0].dt > d.seg[1].dt ? d.seg[0].dt : d.seg[1].dt;
  const bool lo0 = d.seg[0].dt != hi, lo1 = d.seg[1].dt != hi;
  const int ustart = (hi == 0 && Tout - 1 >= Tin) ? 0 : -1;

  // ---- K step ks, lane group q: the 16-byte chunk 4 ks + q of the 2 runs x 5 taps x CPT.  Weights of the two column tiles of the pair (MFMA row r of
  // tile h is column 32 cp + 8 (r / 4) + 4 h + r % 4) and the LDS offset of the matching B fragment, once
  uint4 wreg[2][KS];
  int koff[KS];
  bool klo[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    int run, tap, cc;
    if constexpr (CPT == 4) { run = ks / 5; tap = ks % 5; cc = q; }
    else { const int cid = 4 * ks + q; run = cid / (5 * CPT); tap = (cid - run * 5 * CPT) / CPT; cc = cid % CPT; }
    klo[ks] = run ? lo1 : lo0;
    const int ko = run ? d.seg[1].koff : d.seg[0].koff;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int n = 32 * cp + 8 * (li >> 2) + 4 * h + (li & 3);
      wreg[h][ks] = *reinterpret_cast<const uint4*>(w + (int64_t)n * d.ldw + ko + tap * C + cc * 8);
    }
    const int row = ph * 16 * NB + li + (tap >> 1);      // input position 2 f - 2 + tap: plane tap & 1, row f + tap / 2
    koff[ks] = (tap & 1) * PLANE + row * PB + ((cc ^ G::swz(row)) << 4);
  }
  f32x4 bias4[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if (d.bias.arena >= 0) {
    const float* bp = reinterpret_cast<const float*>(rp(ab, d.bias));
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) bias4[h][e] = bp[32 * cp + 8 * q + 4 * h + e];
  }

  // ---- this thread's share of a frame's LDS-DMA: chunk L = it * 256 + tid of the two planes' rows 1 .. Fo, swizzle and de-interleave on the source side
  int eoff[NIT], edst[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int L = it * 256 + tid, plane = L / (FO * CPT), within = L % (FO * CPT), row = 1 + within / CPT, c = (within % CPT) ^ G::swz(row);
    eoff[it] = (2 * (row - 1) + plane) * C + c * 8;
    const int L0 = it * 256 + wid * 64;
    edst[it] = (L0 / (FO * CPT)) * PLANE + PB + (L0 % (FO * CPT)) * 16;
  }
  const uint32_t lbase = lds_addr(smem);
  const int64_t bs0 = d.bstride[0];
  const int ts0 = d.tstride[0], ba0 = d.base[0];
  auto issue_frame = [&](int b, int t, int slot) {
    const bool valid = t >= 0 && t < Tin;
    const uint16_t* f0 = x0 + (int64_t)b * bs0 + ba0 + (int64_t)t * ts0;
#pragma unroll
    for (int it = 0; it < NIT; ++it) dma16(valid ? f0 + eoff[it] : zp, lbase + slot + edst[it]);
  };
  // rows 0 and Fo + 1 of both planes of every slot: zero, never written again
  if (tid < 12 * CPT) {
    const int r = tid / CPT, slot = r / 4, plane = (r >> 1) & 1, last = r & 1;
    *reinterpret_cast<uint4*>(smem + slot * SLOT + plane * PLANE + (last ? (FO + 1) * PB : 0) + (tid % CPT) * 16) = make_uint4(0, 0, 0, 0);
  }

  int cb = g0 / Tout, cu = g0 - cb * Tout;
  int sp = 0, sc = SLOT, sn = 2 * SLOT;
  issue_frame(cb, cu + hi - 1, sp);
  issue_frame(cb, cu + hi, sc);
  int nb = cb, nu = cu + 1;
  if (nu == Tout) { nu = ustart; ++nb; }
  f32x4 s1[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, s2[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  int left = g1 - g0;
  __builtin_amdgcn_s_waitcnt(0x0F70);            // the weights have landed (see thin_stage_pm_kernel)

  while (left > 0) {
    wait_vm<0>();
    lds_barrier();
    const bool out = cu >= 0;
    if (left - (out ? 1 : 0) > 0) issue_frame(nb, nu + hi, sn);
    if (out) {
      const int g = g1 - left;
      f32x4 acc[2][NB];
#pragma unroll
      for (int blk = 0; blk < NB; ++blk) acc[0][blk] = acc[1][blk] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (active) {
      // the B fragments of K step ks + 1 are read while step ks is multiplied (scheduling barriers: see thin_stage_pm_kernel)
      auto frag = [&](int ks, uint4 (&b)[NB]) {
        const int off = (klo[ks] ? sp : sc) + koff[ks];
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) b[blk] = *reinterpret_cast<const uint4*>(smem + off + blk * 16 * PB);
      };
      uint4 bf[2][NB];
      frag(0, bf[0]);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks + 1 < KS) frag(ks + 1, bf[(ks + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
          const bf16x8 bfr = __builtin_bit_cast(bf16x8, bf[ks & 1][blk]);
          acc[0][blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wreg[0][ks]), bfr, acc[0][blk], 0, 0, 0);
          acc[1][blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wreg[1][ks]), bfr, acc[1][blk], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // the bias is added to the finished sum (the compiler pads the MFMA results for this add; the inline assembly below reads the add's)
#pragma unroll
      for (int blk = 0; blk < NB; ++blk) { acc[0][blk] += bias4[0]; acc[1][blk] += bias4[1]; }
      }

      if constexpr (G::TILE) {
        // One lane per (column, chain) over the frame's fp32 tile in LDS: 16 dependent add / fma steps where the DPP walk below takes 16 for each of a
        // lane's 8 values.  The order is the 128-column kernels' (rungemm_persist_kernel<128>: two waves of 64 rows per column): chain hh of a column
        // starts at 0.f and walks the rows 4 hh + 8 k + r of TWO consecutive frames without a restart; the pair is chain 0 + chain 1; the row is its two
        // pairs added in ascending order to 0.f (a missing pair or frame of the launch's last row adds nothing, as rows beyond M add nothing there).
        // The tile is written again behind the next frame's barrier, which the readers reach with their reads retired
        if (part) {
          float* tile = reinterpret_cast<float*>(smem + 3 * SLOT + G::RED);
#pragma unroll
          for (int blk = 0; blk < NB; ++blk)
#pragma unroll
            for (int h = 0; h < 2; ++h) *reinterpret_cast<f32x4*>(tile + (16 * blk + li) * G::TP + 32 * cp + 8 * q + 4 * h) = acc[h][blk];
          lds_barrier();
          const int fr = (g - g0) % FPR, col = tid >> 1, hh = tid & 1;
          if (fr == 0) { s1[0][0] = 0.f; s2[0][0] = 0.f; }
          if ((fr & 1) == 0) { s1[0][1] = 0.f; s2[0][1] = 0.f; }
          float s = s1[0][1], r = s2[0][1];      // this lane's chain over the pair of frames so far
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const float v = tile[(4 * hh + 8 * k + rr) * G::TP + col];
              s = s + v;
              r = __builtin_fmaf(v, v, r);
            }
          s1[0][1] = s; s2[0][1] = r;
          const bool rowend = fr == FPR - 1 || left == 1;
          if ((fr & 1) != 0 || rowend) {
            s1[0][0] += s + dpp_f<0xB1>(s);      // quad_perm [1, 0, 3, 2]: the other chain of the column
            s2[0][0] += r + dpp_f<0xB1>(r);
          }
          if (rowend && hh == 0) {
            float* prow = part + (int64_t)(g / FPR) * 2 * d.Npad + col;
            prow[0] = s1[0][0];
            prow[d.Npad] = s2[0][0];
          }
        }
      } else if (part) {
        // (order: see chain32.  A wave's pair of blocks is one 32-row group; the sums sit in lane li == 11)
        const int fr = (g - g0) & 1;
        const bool rowend = fr != 0 || left == 1;
        float* prow = part + (int64_t)(g >> 1) * 2 * d.Npad + 32 * cp + 8 * q;
        if constexpr (G::NPH == 1) {
          if (fr == 0) { s1[0] = s1[1] = s2[0] = s2[1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
          for (int j = 0; j < NB / 2; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              f32x4 t1, t2;
              chain32(acc[h][2 * j], acc[h][2 * j + 1], t1, t2);
              s1[h] += t1; s2[h] += t2;
            }
          if (rowend && li == 11) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              *reinterpret_cast<f32x4*>(prow + 4 * h) = s1[h];
              *reinterpret_cast<f32x4*>(prow + d.Npad + 4 * h) = s2[h];
            }
          }
        } else {
          // the waves of a column pair own one group each: they meet in LDS at the end of the row and are added in the order (frame, group) to 0.f
          f32x4* red = reinterpret_cast<f32x4*>(smem + 3 * SLOT);
          if (active) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              f32x4 t1, t2;
              chain32(acc[h][0], acc[h][1], t1, t2);
              if (li == 11) { red[((fr * 4 + wid) * 2 + 0) * 8 + q * 2 + h] = t1; red[((fr * 4 + wid) * 2 + 1) * 8 + q * 2 + h] = t2; }
            }
          }
          if (rowend) {
            lds_barrier();
            if (ph == 0 && li == 11) {
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1;
                for (int f = 0; f <= fr; ++f)
#pragma unroll
                  for (int hh = 0; hh < G::NPH; ++hh) {
                    a1 += red[((f * 4 + cp + hh * NCP) * 2 + 0) * 8 + q * 2 + h];
                    a2 += red[((f * 4 + cp + hh * NCP) * 2 + 1) * 8 + q * 2 + h];
                  }
                *reinterpret_cast<f32x4*>(prow + 4 * h) = a1;
                *reinterpret_cast<f32x4*>(prow + d.Npad + 4 * h) = a2;
              }
            }
          }
        }
      }

      const int n0 = 32 * cp + 8 * q;
      uint16_t* yrow = (n0 >= n2 ? y2 : y) + (int64_t)cb * d.y_bstride + (int64_t)cu * d.y_tstride + d.y_off + n0;
#pragma unroll
      for (int blk = 0; blk < NB; ++blk) {
        const uint4 o4 = make_uint4(pack_bf16x2(acc[0][blk][0], acc[0][blk][1]), pack_bf16x2(acc[0][blk][2], acc[0][blk][3]),
                                    pack_bf16x2(acc[1][blk][0], acc[1][blk][1]), pack_bf16x2(acc[1][blk][2], acc[1][blk][3]));
        const int f = 16 * (ph * NB + blk) + li;
        if (active) *reinterpret_cast<uint4*>(yrow + (int64_t)f * d.y_fstride) = o4;
      }
      --left;
    }
    cb = nb; cu = nu;
    if (++nu == Tout) { nu = ustart; ++nb; }
    const int t = sp; sp = sc; sc = sn; sn = t;
  }
}

// ------------------------------------------------------------------------------------------------------------ selection
namespace {

// The instantiated forms.  strided: the strided form with n = NCP pairs of 32 columns, else the phase-merged form with n = NSRC sources; C channels
// per source and position; fo output positions per frame.  The last row is a family of its own (thin_stage64_choose).
struct StageRow { bool strided; int C, n, fo; GemmKernel kern; int fallback; };      // fallback: resident workgroups per CU without a device
constexpr StageRow kStageRows[] = {
    {false, 64, 2, kStageFo, &thin_stage_pm_kernel<64, 2>, 2},
    {false, 64, 1, kStageFo, &thin_stage_pm_kernel<64, 1>, 2},
    {false, 32, 2, kStageFo, &thin_stage_pm_kernel<32, 2>, 4},
    {false, 32, 1, kStageFo, &thin_stage_pm_kernel<32, 1>, 4},
    {true, 32, 2, kStageFo, &thin_stage_st_kernel<32, 2>, 3},
    {true, 32, 4, kStageFo, &thin_stage_st_kernel<32, 4>, 2},
    {true, 16, 1, kStageFo, &thin_stage_st_kernel<16, 1>, 4},
    {true, 16, 2, kStageFo, &thin_stage_st_kernel<16, 2>, 4},
    {true, 64, 4, kStage64Fo, &thin_stage_st_kernel<64, 4, kStage64Fo>, 2},
};
constexpr int kStageForms = sizeof(kStageRows) / sizeof(kStageRows[0]);
std::atomic<int> g_stage_resident[kStageForms];

// Row of kStageRows with these parameters, -1: a form that is not built
int stage_row(bool strided, int C, int n, int fo) {
  for (int i = 0; i < kStageForms; ++i)
    if (kStageRows[i].strided == strided && kStageRows[i].C == C && kStageRows[i].n == n && kStageRows[i].fo == fo) return i;
  return -1;
}

// What all forms share: thin_common.h's plain bf16 launch (bias, optional statistics), Fo = `fo`, whole frames.
bool stage_common(const RunGemm& d, int fo = kStageFo) {
  if (!thin_plain_bf16(d)) return false;
  if (d.zero.arena < 0 || d.M <= 0 || d.Tout <= 0 || d.Fo != fo || (int64_t)d.M % ((int64_t)d.Tout * d.Fo) != 0 || d.x[0].arena < 0) return false;
  if (d.n2 != 0 && (d.n2 < 0 || d.n2 % 8 != 0 || d.n2 >= d.N || d.y2.arena < 0)) return false;
  if (d.stats.arena >= 0 && (d.Npad != d.N || d.n2 != 0 || d.stats.off % 16 != 0)) return false;   // every column of a statistics row is written
  return d.Tin[0] > 0 && d.tstride[0] % 8 == 0 && d.base[0] % 8 == 0 && d.bstride[0] % 8 == 0;
}

// the runs of source sg / 2 are its frames u + hi and u + hi - 1 (hi = 0 or 1, either order) of `len` elements from `off`
bool stage_runs(const RunGemm& d, int nsrc, int off, int len) {
  if (d.nseg != 2 * nsrc) return false;
  const int hi = d.seg[0].dt > d.seg[1].dt ? d.seg[0].dt : d.seg[1].dt;
  if (hi != 0 && hi != 1) return false;
  for (int sg = 0; sg < 2 * nsrc; ++sg) {
    const Seg& s = d.seg[sg];
    if (s.src != (sg >> 1) || (s.dt != hi && s.dt != hi - 1) || s.off != off || s.len != len || s.koff % 8 != 0 || s.koff < 0 || s.koff + s.len > d.ldw) return false;
    if ((sg & 1) && s.dt == d.seg[sg - 1].dt) return false;
  }
  return true;
}

// The phase-merged form with N = C: one or two sources of C channels per position, per source two runs of 3 positions from bin f - 1.
// Returns its row, -1: not this form or a (C, sources) that is not built.
int stage_pm_form(const RunGemm& d) {
  if (!stage_common(d) || d.n2 != 0) return -1;
  const int nsrc = d.x[1].arena >= 0 ? 2 : 1, C = d.fstride[0];
  const int row = stage_row(false, C, nsrc, kStageFo);
  if (row < 0 || d.N != C) return -1;
  for (int s = 0; s < nsrc; ++s)
    if (d.fstride[s] != C || d.rowlen[s] != d.Fo * C || d.Tin[s] != d.Tin[0] || d.tstride[s] % 8 != 0 || d.base[s] % 8 != 0 || d.bstride[s] % 8 != 0) return -1;
  return stage_runs(d, nsrc, -C, 3 * C) ? row : -1;
}

// The strided form: one source of C channels per position, 2 Fo positions per frame, two runs of 5 positions from position 2 f - 2, 32 NCP columns,
// with statistics rows (the encoder forward) or split over two destinations (the decoder's merged input gradient).
// Returns its row, -1: not this form or a (C, NCP) that is not built.
int stage_st_form(const RunGemm& d) {
  if (!stage_common(d) || d.x[1].arena >= 0 || d.fstride[0] % 2 != 0 || d.N % 32 != 0) return -1;
  const int C = d.fstride[0] / 2;
  const int row = stage_row(true, C, d.N / 32, kStageFo);
  if (row < 0 || d.rowlen[0] != 2 * d.Fo * C) return -1;
  if (d.stats.arena < 0 && d.n2 == 0) return -1;     // the forward with its statistics rows or the two-destination gradient: what was measured
  return stage_runs(d, 1, -2 * C, 5 * C) ? row : -1;
}

// Row of either form at Fo = 64, -1: neither
int stage_form(const RunGemm& d) {
  const int pm = stage_pm_form(d);
  return pm >= 0 ? pm : stage_st_form(d);
}

// The strided form at 64 channels and 32 output positions per frame, 128 columns (thin_stage_st_kernel<64, 4, 32>): the third encoder layer's forward
// conv (bias, statistics rows) and the input gradients of the third-to-last decoder layer, one launch per destination (no statistics; a second
// destination at n2 costs the kernel nothing and is allowed).  Field by field, as stage_st_form; no flag but the two alignment flags.
// Returns its row, -1: not this form.
int stage64_form(const RunGemm& d) {
  if (!stage_common(d, kStage64Fo) || (d.flags & ~(kRunAligned | kRunYAligned)) != 0 || d.x[1].arena >= 0) return -1;
  constexpr int C = 64;
  if (d.fstride[0] != 2 * C || d.N != 128 || d.Npad != 128 || d.rowlen[0] != 2 * d.Fo * C) return -1;
  if (d.stats.arena < 0 && d.bias.arena >= 0) return -1;         // the two epilogues built and measured: bias + statistics, or neither
  return stage_runs(d, 1, -2 * C, 5 * C) ? stage_row(true, C, 4, kStage64Fo) : -1;
}

// Row that runs `d` under its family's knob at `mode` (launch_common.h; default rule: launches of at least kThinStageMinRows rows), -1: not taken
int stage_takes(const RunGemm& d, int mode, int (*form_of)(const RunGemm&)) {
  if (mode <= 0) return -1;
  const int form = form_of(d);
  return form >= 0 && knob_takes(mode, d.M >= kThinStageMinRows) ? form : -1;
}

// ... and its choice with the family's grid knob at `forced`.  The unit of a workgroup's run is a statistics row: 128 / fo frames.
KernelChoice stage_choice(const RunGemm& d, int family, int form, int64_t forced) {
  const StageRow& r = kStageRows[form];
  const int fpr = 128 / r.fo;
  return KernelChoice{family, form, cap_grid(knob_grid(forced, resident_wgs_per_cu(g_stage_resident[form], r.kern, 256, r.fallback)), (d.M / r.fo + fpr - 1) / fpr)};
}

}  // namespace

// Knobs, read per launch: THIN_STAGE, THIN_STAGE_GRID
bool thin_stage_choose(const RunGemm& d, KernelChoice* c) {
  const int form = stage_takes(d, (int)tune_int("THIN_STAGE", 1), stage_form);
  if (form >= 0) *c = stage_choice(d, kFamThinStage, form, tune_int("THIN_STAGE_GRID", 0));
  return form >= 0;
}
// The 64-channel strided form: knobs of its own, THIN_STAGE64 and THIN_STAGE64_GRID.  THIN_STAGE and THIN_MASK do not switch it.
bool thin_stage64_choose(const RunGemm& d, KernelChoice* c) {
  const int form = stage_takes(d, (int)tune_int("THIN_STAGE64", 1), stage64_form);
  if (form >= 0) *c = stage_choice(d, kFamThinStage64, form, tune_int("THIN_STAGE64_GRID", 0));
  return form >= 0;
}

// Both families: the choice's form is the row
void thin_stage_launch(const RunGemm& d, const KernelChoice& c, const ArenaBases& ab, hipStream_t st) {
  hipLaunchKernelGGL(kStageRows[c.form].kern, dim3(c.grid), dim3(256), 0, st, d, ab);
}

}  // namespace sefd
