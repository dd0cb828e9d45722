// WGRAD, frame-staged kernel for the thin layers next to the mask layer (profiles/thin_wgrad_notes.md): the weight gradients of the mask layer and of the
// second-to-last decoder layer in their swapped form (one launch per source: the runs go over dy, the dense operand is the source activation) and of the
// second encoder layer (the forward descriptor: the runs go over the first layer's output, the dense operand is dz).  All have one form: ONE run source of
// CRUN channels per position and 2 Fo positions per frame, two runs (frames u + hi and u + hi - 1) of 5 positions from position 2 f - 2, and a dense
// operand of Fo positions x N channels per frame.  wgrad_bf16_dma_kernel fetches the im2col-expanded rows of the run operand for every 32 rows and k tile
// (every element about five times) and the dense operand once per k tile; here
//   * a workgroup owns one row split and ALL ldw columns: grid = d.nsplit, the 32-row steps [step0, step1) exactly as wgrad_bf16_dma_kernel defines them;
//   * it walks the frames its steps touch in ascending order and keeps them in an LDS ring filled by LDS-DMA: slot of visit (b, u) = the run frame u + hi in
//     thin_stage_st_kernel's layout (even and odd positions in two planes of [Fo + 2 rows][CRUN channels], rows 0 and Fo + 1 zero) and the dense frame u
//     ([Fo positions][N channels]).  Step (b, u, h) multiplies rows 32 h .. + 31 of the dense frame with the rows of the current slot (the run with dt = hi)
//     and of the slot before it (dt = hi - 1).  Each element of either operand is fetched once per workgroup, plus one run frame in front of its first step;
//     an item starts with a visit u = -1 that only loads.  Frames outside [0, Tin) come from the zero page by pointer select;
//   * the arithmetic is the parent's: one v_mfma_f32_16x16x32_bf16 per 16 x 16 tile and 32-row step, steps in ascending order into an accumulator that starts
//     at +0, the rows of a step in tr_frag_swz's k slots (ds_read_b64_tr_b16 of rows 4 g + q and 16 + 4 g + q for lane group g).  Accumulators stay in
//     registers for the whole split.  16-column blocks of k that are padding only are not multiplied; their zeros are written;
//   * no flag, wait or atomic between workgroups.
// Every byte of every partial block [split][Npad][ldw] equals what wgrad_bf16_dma_kernel writes (tests/test_gpu_thin_wgrad.py).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "sefd_desc.h"
#include "tuning.h"
#include "dev_common.h"
#include "launch_common.h"
#include "thin_common.h"

namespace sefd {

namespace {

constexpr int64_t kThinWgradMinRows = 262144;    // default rule: smaller launches stay on the kernels they had (the threshold of thin_mask / thin_stage)

typedef __attribute__((ext_vector_type(4))) short s16x4;
struct Frag8 { s16x4 lo, hi; };

// CRUN: channels per position of the run operand; N: channels of the dense operand = rows of the packed gradient
template <int CRUN, int N>
struct WgGeom {
  static constexpr int FO = CRUN == 8 ? 128 : 64;          // GEMM rows per frame (the mask layer has twice the bins)
  static constexpr int SPF = FO / kWgRows;                 // 32-row steps per frame
  static constexpr int CPT = CRUN / 8;                     // 16-byte chunks per position of the run operand
  static constexpr int RPB = CRUN * 2;                     // bytes per plane row
  static constexpr int PLANE = (FO + 2) * RPB;
  static constexpr int RUNB = 2 * PLANE;
  static constexpr int DCH = N / 8;                        // chunks per position of the dense operand
  static constexpr int DPB = N * 2;
  static constexpr int SLOT = RUNB + FO * DPB;
  static constexpr int SEGLEN = 5 * CRUN;
  static constexpr int SEGPAD = (SEGLEN + 63) / 64 * 64;   // layout_segs: a run starts a 64-column tile
  static constexpr int LDW = 2 * SEGPAD;
  static constexpr int KBS = (SEGLEN + 15) / 16;           // 16-column blocks of a run that hold data: 10, 5, 3 (the last of 3 is half padding)
  static constexpr int PADC = SEGPAD - 16 * KBS;           // columns of a run behind them
  static constexpr int WPS = N == 64 ? 2 : 1;              // waves that share a run
  static constexpr int NWN = 4 / (2 * WPS);                // waves along n
  static constexpr int NT = N / 16 / NWN;                  // 16-row tiles of the gradient per wave
  static constexpr int KB = KBS / WPS;                     // blocks per wave
  static constexpr int NIT_R = 2 * FO * CPT / 256;         // LDS-DMA instructions per thread and visit: run frame
  static constexpr int NIT_D = FO * DCH / 256;             // ... dense frame
  static constexpr int NI = NIT_R + NIT_D;
  // ring slots: the two a step reads and S - 2 in flight.  <32, 64>: one workgroup per CU at the planner's 256 splits, 16.6 KB per visit - three visits in
  // flight are 50 KB per CU, above the 26 KB that 4.5 TB/s x 1.5 us / 256 CUs ask for.  <8, 32>: 1 024 splits, four workgroups per CU of one visit
  // (12.4 KB) in flight each.  <16, 32>: 512 splits
  static constexpr int S = CRUN == 32 ? 5 : CRUN == 16 ? 4 : 3;
  static_assert((N == 64 || N == 32) && (CRUN == 32 || CRUN == 16 || CRUN == 8) && KBS % WPS == 0 && NIT_R >= 1 && NIT_D >= 1 && NT >= 1, "instantiated forms");
  static_assert((FO * CPT) % 64 == 0 && (FO * DCH) % 64 == 0, "a wave's 64 chunks stay inside one plane");
  // 32-byte pieces of a row are XOR-ed with row bits so that the 8 rows a 32-lane half of ds_read_b64_tr_b16 reads fall on 8 different 32-byte
  // bank groups (by hand, cdna_hip_programming.md section 2): rows of 128 bytes take (row >> 1) & 3, rows of 64 bytes (row >> 2) & 1, shorter rows nothing
  __host__ __device__ static constexpr int swz_run(int row) { return CPT == 4 ? ((row >> 2) & 1) << 1 : 0; }
  __host__ __device__ static constexpr int swz_den(int pos) { return DCH == 8 ? ((pos >> 1) & 3) << 1 : ((pos >> 2) & 1) << 1; }
};

__device__ __forceinline__ bf16x8 tr_pair(const char* smem, int lo, int hi) {
  Frag8 f;
  f.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(smem + lo));
  f.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(smem + hi));
  return __builtin_bit_cast(bf16x8, f);
}

}  // namespace

template <int CRUN, int N>
__global__ __launch_bounds__(256) void thin_wgrad_kernel(const RunGemm d, const ArenaBases ab) {
  using G = WgGeom<CRUN, N>;
  constexpr int FO = G::FO, SPF = G::SPF, CPT = G::CPT, RPB = G::RPB, PLANE = G::PLANE, RUNB = G::RUNB, DCH = G::DCH, DPB = G::DPB, SLOT = G::SLOT;
  constexpr int NT = G::NT, KB = G::KB, NIT_R = G::NIT_R, NIT_D = G::NIT_D, NI = G::NI, S = G::S, LDW = G::LDW;
  __shared__ __attribute__((aligned(16))) char smem[S * SLOT];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, q = lane >> 4;
  const int split = blockIdx.x;
  float* part = reinterpret_cast<float*>(rp(ab, d.w)) + (int64_t)split * N * LDW;

  // ---- this split's steps, as wgrad_bf16_dma_kernel walks them: per batch item, spb steps of 32 rows (Tout * Fo is a multiple of 32: no ragged step)
  const int Tout = d.Tout, Tin = d.Tin[0];
  const int spb = Tout * SPF;
  const int nsteps_total = (int)(d.M / ((int64_t)Tout * FO)) * spb;
  const int per = (nsteps_total + d.nsplit - 1) / d.nsplit;
  const int64_t s0 = (int64_t)split * per;
  const int step0 = (int)(s0 < nsteps_total ? s0 : nsteps_total);
  const int step1 = nsteps_total < step0 + per ? nsteps_total : step0 + per;

  const int wn = wid % G::NWN, wk = wid / G::NWN;
  const int sg = wk / G::WPS, blk0 = (wk % G::WPS) * KB;   // this wave's run and its first block
  const int kcol0 = d.seg[sg].koff + 16 * blk0;

  f32x4 acc[NT][KB];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < KB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (step0 < step1) {
    const uint16_t* x0 = reinterpret_cast<const uint16_t*>(rp(ab, d.x[0]));
    const uint16_t* dy = reinterpret_cast<const uint16_t*>(rp(ab, d.y));
    const uint16_t* zp = reinterpret_cast<const uint16_t*>(rp(ab, d.zero));
    const int hi = d.seg[0].dt > d.seg[1].dt ? d.seg[0].dt : d.seg[1].dt;
    const bool lo_run = d.seg[sg].dt != hi;                // this wave's run reads the slot before the current one

    // ---- fragment offsets inside a slot, once.  Lane (q, li) supplies row 4 q + (li >> 2) (and + 16) of the step, columns 4 (li & 3) .. + 3 of the block
    const int r0 = 4 * q + (li >> 2), c4 = 4 * (li & 3);
    int doff[NT][2], koff[KB][2], kstep[KB];               // kstep: bytes from a step's rows to the next step's (0 for a lane that reads padding)
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int pos = r0 + 16 * h, col = 16 * (wn * NT + a) + c4;
        doff[a][h] = RUNB + pos * DPB + (((col >> 3) ^ G::swz_den(pos)) << 4) + (col & 7) * 2;
      }
#pragma unroll
    for (int b = 0; b < KB; ++b)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = 16 * (blk0 + b) + c4;                 // column inside the run: tap j / CRUN (input position 2 f - 2 + tap), channel j % CRUN
        const int tap = j / CRUN, ch = j % CRUN;
        const int row = r0 + 16 * h + (tap >> 1);           // plane tap & 1, row f + tap / 2
        // (a padding column - the second half of a run's last block where 5 CRUN is no multiple of 16 - reads the zero row 0 of plane 0 at every step)
        const bool data = 16 * G::KBS == G::SEGLEN || j < G::SEGLEN;
        koff[b][h] = data ? (tap & 1) * PLANE + row * RPB + (((ch >> 3) ^ G::swz_run(row)) << 4) + (ch & 7) * 2 : 0;
        kstep[b] = data ? kWgRows * RPB : 0;
      }

    // ---- this thread's share of a visit's LDS-DMA: chunk L = it * 256 + tid; swizzle and de-interleave on the source side
    int roff[NIT_R], rdst[NIT_R], yoff[NIT_D], ydst[NIT_D];
#pragma unroll
    for (int it = 0; it < NIT_R; ++it) {
      const int L = it * 256 + tid, plane = L / (FO * CPT), within = L % (FO * CPT), row = 1 + within / CPT, c = (within % CPT) ^ G::swz_run(row);
      roff[it] = (2 * (row - 1) + plane) * CRUN + c * 8;
      const int L0 = it * 256 + wid * 64;
      rdst[it] = (L0 / (FO * CPT)) * PLANE + RPB + (L0 % (FO * CPT)) * 16;
    }
#pragma unroll
    for (int it = 0; it < NIT_D; ++it) {
      const int L = it * 256 + tid, pos = L / DCH, c = (L % DCH) ^ G::swz_den(pos);
      yoff[it] = pos * d.y_fstride + c * 8;
      ydst[it] = RUNB + (it * 256 + wid * 64) * 16;
    }
    const uint32_t lbase = lds_addr(smem);
    const int64_t bs0 = d.bstride[0], ybs = d.y_bstride;
    const int ts0 = d.tstride[0], ba0 = d.base[0], yts = d.y_tstride, yo = d.y_off;

    // ---- the visits: item b, frame u = -1 .. Tout - 1 (u = -1 only loads the run frame hi - 1).  The first visit is the one in front of the first step's
    // frame (its run frame is that step's lower one; its dense frame is not read), the last the last step's frame
    const int b0 = step0 / spb, u0 = (step0 - b0 * spb) / SPF;
    const int b1 = (step1 - 1) / spb, u1 = (step1 - 1 - b1 * spb) / SPF;
    const int nv = (b1 - b0) * (Tout + 1) + u1 - u0 + 2;
    int ib = b0, iu = u0 - 1, iv = 0, islot = 0;            // issue pointer
    auto issue = [&]() {
      const bool in = iv < nv;
      const int t = iu + hi;
      const bool rv = in && t >= 0 && t < Tin, dv = in && iu >= 0 && iv > 0;
      const uint16_t* fr = x0 + (int64_t)ib * bs0 + ba0 + (int64_t)t * ts0;
      const uint16_t* fd = dy + (int64_t)ib * ybs + (int64_t)iu * yts + yo;
      const uint32_t sl = lbase + islot * SLOT;
#pragma unroll
      for (int it = 0; it < NIT_R; ++it) dma16(rv ? fr + roff[it] : zp, sl + rdst[it]);
#pragma unroll
      for (int it = 0; it < NIT_D; ++it) dma16(dv ? fd + yoff[it] : zp, sl + ydst[it]);
      ++iv;
      if (++iu == Tout) { iu = -1; ++ib; }
      islot = islot + 1 == S ? 0 : islot + 1;
    };
    // rows 0 and Fo + 1 of both planes of every slot: zero, never written again
    for (int i = tid; i < S * 4 * CPT; i += 256) {
      const int r = i / CPT, slot = r / 4, plane = (r >> 1) & 1, last = r & 1;
      *reinterpret_cast<uint4*>(smem + slot * SLOT + plane * PLANE + (last ? (FO + 1) * RPB : 0) + (i % CPT) * 16) = make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < S - 2; ++i) issue();

    int cb = b0, cu = u0 - 1, cur = 0, prev = (S - 1) * SLOT;   // the visit multiplied, its slot and the slot before it (byte offsets)
    for (int v = 0; v < nv; ++v) {
      wait_vm<(S - 3) * NI>();                             // this thread's chunks of visit v have landed (S - 3 newer visits may stay in flight)
      lds_barrier();                                       // ... everyone's; and nobody reads the slot of visit v - 2 any more
      issue();                                             // visit v + S - 2 into that slot (behind the last visit: the zero page, so that the count holds)
      if (cu >= 0) {
        const int sbase = cb * spb + cu * SPF;
        const int rslot = lo_run ? prev : cur;
#pragma unroll
        for (int h = 0; h < SPF; ++h) {
          const int s = sbase + h;
          if (s >= step0 && s < step1) {                   // (workgroup-uniform)
            bf16x8 af[NT], bfr[KB];
#pragma unroll
            for (int a = 0; a < NT; ++a) af[a] = tr_pair(smem, cur + doff[a][0] + h * kWgRows * DPB, cur + doff[a][1] + h * kWgRows * DPB);
#pragma unroll
            for (int b = 0; b < KB; ++b) bfr[b] = tr_pair(smem, rslot + koff[b][0] + h * kstep[b], rslot + koff[b][1] + h * kstep[b]);
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
              for (int b = 0; b < KB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
          }
        }
      }
      if (++cu == Tout) { cu = -1; ++cb; }
      prev = cur;
      cur = cur + SLOT == S * SLOT ? 0 : cur + SLOT;
    }
    wait_vm<0>();                                          // the visits issued behind the last one
  }

  // ---- the whole [N][ldw] block of the split: accumulators, and zeros in the padding columns of both runs
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < KB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = 16 * (wn * NT + a) + 4 * q + r;
        part[(int64_t)n * LDW + kcol0 + 16 * b + li] = acc[a][b][r];
      }
  if constexpr (G::PADC > 0) {
    for (int i = tid; i < N * 2 * G::PADC; i += 256) {
      const int n = i / (2 * G::PADC), c = i % (2 * G::PADC), s = c / G::PADC;
      part[(int64_t)n * LDW + d.seg[s].koff + 16 * G::KBS + c % G::PADC] = 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ selection
namespace {

// The instantiated forms: C channels per position of the run operand, N channels of the dense operand
struct WgRow { int C, N; GemmKernel kern; };
constexpr WgRow kThinWgRows[] = {{32, 64, &thin_wgrad_kernel<32, 64>}, {16, 32, &thin_wgrad_kernel<16, 32>}, {8, 32, &thin_wgrad_kernel<8, 32>}};
constexpr int kThinWgForms = sizeof(kThinWgRows) / sizeof(kThinWgRows[0]);

// The form: aligned bf16 WGRAD without a ones run, one run source of C channels per position and 2 Fo positions per frame, two runs (frames u + hi and
// u + hi - 1, either order) of 5 positions from position 2 f - 2 in layout_segs' columns, a dense operand of N = Npad channels.
// Returns the row of kThinWgRows, -1: not this form or a (C, N) that is not built.
int wgrad_thin_form(const RunGemm& d) {
  if (d.xdt != DT_BF16 || d.ydt != DT_BF16 || !(d.flags & kRunAligned)) return -1;
  if (d.flags & ~(kRunAligned | kRunYAligned)) return -1;   // nothing else: no wide tile, ones MFMA, rank form, first layer, fused BatchNorm backward
  if (d.zero.arena < 0 || d.x[0].arena < 0 || d.x[1].arena >= 0 || d.y.arena < 0 || d.w.arena < 0 || d.nseg != 2 || d.nsplit < 1) return -1;
  if (d.fstride[0] % 2 != 0 || d.N != d.Npad) return -1;
  const int C = d.fstride[0] / 2, N = d.N;
  int row = -1;
  for (int i = 0; i < kThinWgForms; ++i)
    if (kThinWgRows[i].C == C && kThinWgRows[i].N == N) row = i;
  if (row < 0) return -1;
  const int Fo = C == 8 ? 128 : 64;
  if (d.Fo != Fo || d.Tout <= 0 || d.M <= 0 || (int64_t)d.M % ((int64_t)d.Tout * Fo) != 0 || d.Tin[0] <= 0) return -1;
  if (d.rowlen[0] != 2 * Fo * C || d.tstride[0] % 8 != 0 || d.base[0] % 8 != 0 || d.bstride[0] % 8 != 0 || d.x[0].off % 16 != 0) return -1;
  if (!y_strides_aligned(d) || d.y_fstride < N || d.y.off % 16 != 0) return -1;
  const int hi = d.seg[0].dt > d.seg[1].dt ? d.seg[0].dt : d.seg[1].dt, lo = d.seg[0].dt < d.seg[1].dt ? d.seg[0].dt : d.seg[1].dt;
  if (lo != hi - 1) return -1;
  const int pad = (5 * C + 63) / 64 * 64;
  for (int s = 0; s < 2; ++s)
    if (d.seg[s].src != 0 || d.seg[s].off != -2 * C || d.seg[s].len != 5 * C || d.seg[s].koff != s * pad) return -1;
  if (d.ldw != 2 * pad) return -1;
  return row;
}

}  // namespace

// Knob, read per launch (launch_common.h): THIN_WGRAD with the default rule "launches of a built form with at least kThinWgradMinRows rows".  The grid is
// d.nsplit (WG_NSPLIT varies it).
bool thin_wgrad_choose(const RunGemm& d, KernelChoice* c) {
  const int mode = (int)tune_int("THIN_WGRAD", 1);
  if (mode <= 0) return false;
  const int form = wgrad_thin_form(d);
  if (form < 0 || !knob_takes(mode, d.M >= kThinWgradMinRows)) return false;
  *c = KernelChoice{kWgFamThin, form, d.nsplit};
  return true;
}

void thin_wgrad_launch(const RunGemm& d, const KernelChoice& c, const ArenaBases& ab, hipStream_t st) {
  hipLaunchKernelGGL(kThinWgRows[c.form].kern, dim3((unsigned)c.grid), dim3(256), 0, st, d, ab);
}

}  // namespace sefd
