// RUNGEMM, persistent form of the 128-row LDS-DMA kernel of rungemm.hip for the N <= 128 bf16 conv layers and their input gradients.
//
// rungemm_kernel lives for ONE output tile: row decode, run entry and the weight pointers, the first DMAs into an empty ring, the K loop, then an
// epilogue of four workgroup barriers that stages the tile through the ring's LDS - so nothing of a next tile can be in flight behind it.  Here
//   * workgroup b walks the tiles b, b + gridDim, ... (XCD-aware order, as before); the grid is what is resident: min(tiles, workgroups per CU x CUs);
//   * begin_tile(next) - row decode, enter_run(0), weight pointers, the first ring stage - is issued right behind the K loop of the current tile
//     and BEFORE its epilogue; the ring stage index carries over from tile to tile;
//   * the epilogue stays in registers (bias, ReLU, bf16, QuadT / OctW of dev_common.h, 16-byte stores, as in cgemm256.hip): it touches no ring
//     byte.  Only the per-column statistics of the WM_ waves that share a column meet in a small LDS area behind the ring: one barrier per tile.
// Same two-stage ring, fragment reads, MFMA order and statistics order as rungemm_kernel: outputs and partial rows are bit-identical.
// Waits: with two stages every K tile's top is `s_waitcnt vmcnt(0)`, as in rungemm_kernel (wait_stage<NL, 2>); behind an epilogue that wait also
// covers the tile's stores, which are younger than the DMAs of begin_tile - it can only wait for more than it needs, never for less.
// No workgroup waits for another one and no loop depends on memory: every loop is bounded by the tile count.
#include <hip/hip_runtime.h>
#include "sefd_desc.h"
#include "tuning.h"
#include "dev_common.h"
#include "launch_common.h"

namespace sefd {

namespace {

__device__ __forceinline__ int fdivp(int x, uint32_t m, uint32_t s) { return m ? (int)(__umulhi((uint32_t)x, m) >> s) : x; }

__device__ __forceinline__ int xcd_remap_p(int bid, int nwg) {       // rungemm.hip xcd_remap
  const int xcd = bid & 7, local = bid >> 3;
  const int q = nwg >> 3, r = nwg & 7;
  const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return start + local;
}

constexpr int persist_lds_bytes(int BN) { return 2 * (kBM + BN) * 128 + (BN == 128 ? 2 : 4) * BN * 8; }

}  // namespace

template <int BN>
__global__ __launch_bounds__(256) void rungemm_persist_kernel(const RunGemm d, const ArenaBases ab) {
  typedef uint16_t TA;
  constexpr int VEC = 8, BK = 64, BM = kBM, NW = 4, S = 2;
  constexpr int PR = NW * 8;                   // rows per load pass (8 threads per 128-byte row)
  constexpr int RP = BM / PR;
  constexpr int WN_ = BN == 128 ? 2 : 1;
  constexpr int WM_ = NW / WN_;
  constexpr int MI = BM / (32 * WM_);
  constexpr int NI = BN / (32 * WN_);
  constexpr int BPASS = BN / PR;
  constexpr int TILE_BYTES = (BM + BN) * 128;
  constexpr int RING = S * TILE_BYTES;
  static_assert(RING + WM_ * BN * 8 == persist_lds_bytes(BN), "LDS budget the launcher counts with");
  // one array: the ring, then the statistics area [WM_][BN][2] (a second __shared__ object beside a DMA ring can cost a vmcnt(0) per fragment read)
  __shared__ __attribute__((aligned(16))) char smem[RING + WM_ * BN * 8];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nn = d.Npad / BN;
  const int nm = (d.M + BM - 1) / BM;
  const int total = nm * nn;
  const int TF = d.Tout * d.Fo;
  // the run table is read through the kernarg segment (the descriptor is the first argument): indexing the by-value copy with a run-time run
  // id costs a private-segment object
  const auto* dk = (const __attribute__((address_space(4))) RunGemm*)__builtin_amdgcn_kernarg_segment_ptr();
  int ntiles = 0;
  for (int s = 0; s < d.nseg; ++s) ntiles += (dk->seg[s].len + BK - 1) / BK;

  const TA* x0 = reinterpret_cast<const TA*>(rp(ab, d.x[0]));
  const TA* x1 = d.x[1].arena >= 0 ? reinterpret_cast<const TA*>(rp(ab, d.x[1])) : x0;
  const TA* w = reinterpret_cast<const TA*>(rp(ab, d.w));
  const TA* zp = reinterpret_cast<const TA*>(rp(ab, d.zero));
  const int Tin0 = d.Tin[0], Tin1 = d.Tin[1], fs0 = d.fstride[0], fs1 = d.fstride[1], rl0 = d.rowlen[0], rl1 = d.rowlen[1];
  const int64_t ts0 = d.tstride[0], ts1 = d.tstride[1];

  // ---- load roles: chunk column c, rows r0 + 32p; the swizzle sits on the SOURCE chunk (the DMA destination is lane-linear)
  const int c = tid & 7, r0 = tid >> 3;
  const int csrc = c ^ ((r0 >> 1) & 7);
  const uint32_t lbase = lds_addr(smem) + wid * 1024;
  // ---- fragment roles
  const int wm0 = (wid / WN_) * (MI * 32), wn0 = (wid % WN_) * (NI * 32);
  const int rsw = ((lane & 31) >> 1) & 7;
  int chs[4];
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) chs[kc] = ((2 * kc + (lane >> 5)) ^ rsw) * 16;
  const int arow = (wm0 + (lane & 31)) * 128, brow = (wn0 + (lane & 31)) * 128;

  // ---- epilogue constants
  const float* biasp = d.bias.arena >= 0 ? reinterpret_cast<const float*>(rp(ab, d.bias)) : nullptr;
  uint16_t* yb = reinterpret_cast<uint16_t*>(rp(ab, d.y));
  const int n2 = d.n2 > 0 ? d.n2 : 0x7fffffff;                    // 8-column chunks from n2 on leave for the second destination, at column n - n2
  uint16_t* yb2 = d.n2 > 0 ? reinterpret_cast<uint16_t*>(rp(ab, d.y2)) - d.n2 : yb;
  const bool want_stats = d.stats.arena >= 0;
  const bool relu = (d.flags & kRunRelu) != 0;
  // dense output rows (conv outputs: frames and batch items follow each other without gaps): row offset = m * pitch + off, no (b, u, fo) decode
  const bool ylin = d.y_tstride == d.Fo * d.y_fstride && d.y_bstride == (int64_t)d.Tout * d.y_tstride;
  float* stat = reinterpret_cast<float*>(smem + RING);

  // ---- DMA state of the tile being loaded: set up, and its first ring stage issued, before the previous tile's epilogue
  int ld_ntile = 0, ld_mtile = 0;
  int64_t rb0[RP], rb1[RP];
  int ru[RP], rfo[RP];
  bool rv[RP];
  const TA* wrow[BPASS];
  const TA* rptr[RP];
  int jlo[RP], jhi[RP];
  int seg = 0, k0 = 0, seglen = 0, wseg = 0;
  int issued = 0, istage = 0, cstage = 0;                          // ring positions: they carry over from tile to tile
  auto enter_run = [&](int sgi) {
    Seg sg;
    sg.src = dk->seg[sgi].src; sg.dt = dk->seg[sgi].dt; sg.off = dk->seg[sgi].off; sg.len = dk->seg[sgi].len; sg.koff = dk->seg[sgi].koff;
    seglen = sg.len;
    wseg = sg.koff;
#pragma unroll
    for (int p = 0; p < RP; ++p) {
      int lo = 0, hi = 0;
      const TA* ptr = x0;
      if (sg.src >= 0 && rv[p]) {
        const int s = sg.src;
        const int tt = ru[p] + sg.dt;
        if (tt >= 0 && tt < (s ? Tin1 : Tin0)) {
          const int rr = sg.off + rfo[p] * (s ? fs1 : fs0);
          lo = rr < 0 ? -rr : 0;
          hi = min(sg.len, (s ? rl1 : rl0) - rr);
          ptr = (s ? x1 : x0) + (s ? rb1[p] : rb0[p]) + (int64_t)tt * (s ? ts1 : ts0) + rr;
          if ((reinterpret_cast<uintptr_t>(ptr) & 15) != 0) { lo |= 0x40000000; }   // unaligned run: never with kRunAligned; reads the zero page
        }
      }
      rptr[p] = ptr; jlo[p] = lo; jhi[p] = hi;
    }
  };
  auto issue_next = [&]() {
    const uint32_t A = lbase + istage * TILE_BYTES, B = A + BM * 128;
    const int j0 = k0 + csrc * VEC;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int p = 0; p < RP; ++p) {
        if ((p & 3) != q) continue;
        const TA* src = (j0 >= jlo[p] && j0 + VEC <= jhi[p]) ? rptr[p] + j0 : zp;
        dma16(src, A + p * (PR * 128));
      }
#pragma unroll
      for (int p = 0; p < BPASS; ++p) {
        if ((p & 3) != q) continue;
        dma16(wrow[p] + wseg + k0, B + p * (PR * 128));
      }
    }
    istage ^= 1;
    ++issued;
    k0 += BK;
    if (k0 >= seglen && issued < ntiles) { k0 = 0; ++seg; enter_run(seg); }
  };
  // Called with the ring where the previous tile's K loop left it: istage == cstage, the stage that the LAST K tile was read from is cstage ^ 1,
  // so the first stage of tile t goes where the last-but-one K tile sat - every wave is past that one (it passed the last K tile's barrier).
  auto begin_tile = [&](int t) {
    const int swz = xcd_remap_p(t, total);
    ld_ntile = swz % nn; ld_mtile = swz / nn;
#pragma unroll
    for (int p = 0; p < RP; ++p) {
      const int m = ld_mtile * BM + r0 + PR * p;
      rv[p] = m < d.M;
      const int mm = rv[p] ? m : 0;
      const int b = fdivp(mm, d.div_tf_m, d.div_tf_s), rem = mm - b * TF;
      ru[p] = fdivp(rem, d.div_fo_m, d.div_fo_s);
      rfo[p] = rem - ru[p] * d.Fo;
      rb0[p] = (int64_t)b * d.bstride[0] + d.base[0];
      rb1[p] = (int64_t)b * d.bstride[1] + d.base[1];
    }
#pragma unroll
    for (int p = 0; p < BPASS; ++p) wrow[p] = w + (int64_t)(ld_ntile * BN + r0 + PR * p) * d.ldw + csrc * VEC;
    seg = 0; k0 = 0; issued = 0;
    enter_run(0);
    if (issued < ntiles) issue_next();
  };

  if ((int)blockIdx.x < total) begin_tile(blockIdx.x);
  for (int t = blockIdx.x; t < total; t += gridDim.x) {
    const int ntile = ld_ntile, mtile = ld_mtile;
    // the bias is needed in the epilogue only, but an ordinary load whose first use sits behind begin_tile(next) would make the compiler wait there
    // for everything in flight - the next tile's DMAs included.  Loaded and pinned here, its wait falls together with the K loop's first one.
    float bv[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = ntile * BN + wn0 + j * 32 + (lane & 31);
      bv[j] = (biasp && n < d.N) ? biasp[n] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) asm volatile("" : "+v"(bv[j]));

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    for (int kt = 0; kt < ntiles; ++kt) {
      wait_vm<0>();                                    // K tile kt has landed (this thread's part); behind an epilogue: and its stores
      lds_barrier();                                   // ... everyone's part; and the stage of K tile kt - 1 (or of the previous tile's last one) is free
      const char* As = smem + cstage * TILE_BYTES;
      const char* Bs = As + BM * 128;
      if (issued < ntiles) issue_next();
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        uint4 af[MI], bf[NI];
#pragma unroll
        for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const uint4*>(As + arow + i * 4096 + chs[kc]);
#pragma unroll
        for (int j = 0; j < NI; ++j) bf[j] = *reinterpret_cast<const uint4*>(Bs + brow + j * 4096 + chs[kc]);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i]), __builtin_bit_cast(bf16x8, bf[j]), acc[i][j], 0, 0, 0);
      }
      cstage ^= 1;
    }
    if (t + (int)gridDim.x < total) begin_tile(t + gridDim.x);

    // ---- epilogue, in registers: bias / ReLU / statistics on the accumulators as they sit (one column per lane, rows i -> q -> r as in
    // rungemm_kernel), then the quad transpose and the lane-pair widening of dev_common.h: two 16-byte stores per lane and 32 x 32 block
    const QuadT qt(lane);
    const OctW ow(lane);
    float s1[NI], s2[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) s1[j] = s2[j] = 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row0 = mtile * BM + wm0 + i * 32;
      int64_t ro[4];                                   // output offsets of this lane's 4 rows after the transpose (-1: beyond M)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = row0 + 8 * q + 4 * (lane >> 5) + (lane & 3);
        ro[q] = -1;
        if (m < d.M) {
          if (ylin) ro[q] = (int64_t)m * d.y_fstride + d.y_off;
          else {
            const int b = fdivp(m, d.div_tf_m, d.div_tf_s), rem = m - b * TF, u = fdivp(rem, d.div_fo_m, d.div_fo_s), fo = rem - u * d.Fo;
            ro[q] = (int64_t)b * d.y_bstride + (int64_t)u * d.y_tstride + (int64_t)fo * d.y_fstride + d.y_off;
          }
        }
      }
      const bool full = row0 + 32 <= d.M;
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int n = ntile * BN + wn0 + j * 32 + (lane & 31);
        const bool nok = n < d.N;
        float v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          v[e] = acc[i][j][e] + bv[j];
          if (relu) v[e] = fmaxf(v[e], 0.f);
        }
        // sum of squares: an explicit fused chain.  Written as s2 += v * v, the first two squares of a chain that starts at zero may be contracted
        // either way round (fma(v0, v0, v1 * v1) or fma(v1, v1, v0 * v0)): rungemm_kernel's build rounds v0 * v0 first and fuses every later term
        if (want_stats && nok) {
          if (full) {
#pragma unroll
            for (int e = 0; e < 16; ++e) { s1[j] += v[e]; s2[j] = __builtin_fmaf(v[e], v[e], s2[j]); }
          } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
              if (row0 + row < d.M) { s1[j] += v[e]; s2[j] = __builtin_fmaf(v[e], v[e], s2[j]); }
            }
          }
        }
        uint2 pk[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) pk[q] = qt.pack(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        uint4 wide[2];
        ow.widen(pk, wide);
        const int n8 = (ntile * BN + wn0 + j * 32 + (lane & 28)) & ~7;     // N % 8 == 0 (kRunYAligned): 8 columns are all valid or all padding
        uint16_t* dst = n8 >= n2 ? yb2 : yb;                               // the destination is chosen per 8-column chunk
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t r = ow.hi4 ? ro[2 * h + 1] : ro[2 * h];
          if (r >= 0 && n8 < d.N) *reinterpret_cast<uint4*>(dst + r + n8) = wide[h];
        }
      }
    }
    if (want_stats) {
      // the WM_ waves of a column meet in LDS, summed in ascending wave order from 0.f (rungemm_kernel's order).  The area is reused by the next
      // tile only behind at least one K-tile barrier, which the readers below reach with their reads retired (lds_barrier waits lgkmcnt(0)).
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const float t1 = s1[j] + __shfl_xor(s1[j], 32), t2 = s2[j] + __shfl_xor(s2[j], 32);
        const int nl = wn0 + j * 32 + (lane & 31);
        if (lane < 32) {
          stat[((wid / WN_) * BN + nl) * 2 + 0] = t1;
          stat[((wid / WN_) * BN + nl) * 2 + 1] = t2;
        }
      }
      lds_barrier();
      if (tid < BN) {
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int wmi = 0; wmi < WM_; ++wmi) { a1 += stat[(wmi * BN + tid) * 2 + 0]; a2 += stat[(wmi * BN + tid) * 2 + 1]; }
        float* part = reinterpret_cast<float*>(rp(ab, d.stats));    // one row of partials per kBM output rows: row mtile
        part[((int64_t)mtile * 2 + 0) * d.Npad + ntile * BN + tid] = a1;
        part[((int64_t)mtile * 2 + 1) * d.Npad + ntile * BN + tid] = a2;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ selection
// What the descriptor must show (everything else stays on rungemm_kernel): bf16 in and out through the LDS-DMA loader, whole 16-byte output
// chunks, no accumulate, no BatchNorm-backward epilogue.
static bool persist_form(const RunGemm& d) {
  if (d.xdt != DT_BF16 || d.ydt != DT_BF16) return false;
  if (!(d.flags & kRunAligned) || !(d.flags & kRunYAligned)) return false;
  if (d.flags & (kRunAccum | kRunBnBwd | kRunWTile32 | kRunEnc0 | kRunDyFromBn)) return false;
  if (d.n2 > 0 && d.n2 % 8 != 0) return false;
  return d.nseg > 0 && d.M > 0;
}

// The instantiated tile widths (bn_of); a row's residency is the occupancy query's, never more than the LDS admits - which is also the value without a device
struct PersistRow { int bn; GemmKernel kern; };
static constexpr PersistRow kPersistRows[] = {{128, &rungemm_persist_kernel<128>}, {64, &rungemm_persist_kernel<64>}, {32, &rungemm_persist_kernel<32>}};
static std::atomic<int> g_persist_resident[3];

// Knobs, read per launch (launch_common.h): RG_PERSIST 0 off, 1 the default rule, 2 every launch of the form above, 3 the default rule for launches
// with statistics only; RG_PERSIST_GRID.  A workgroup's units are the 128-row tiles.
bool rungemm_persist_choose(const RunGemm& d, KernelChoice* c) {
  const int mode = (int)tune_int("RG_PERSIST", 1);
  if (mode <= 0 || !persist_form(d)) return false;
  const int bn = bn_of(d.N), form = bn == 128 ? 0 : bn == 64 ? 1 : 2;
  const int64_t tiles = (int64_t)((d.M + kBM - 1) / kBM) * (d.Npad / bn);
  const int cap = (160 * 1024) / persist_lds_bytes(bn);
  const int64_t grid = knob_grid(tune_int("RG_PERSIST_GRID", 0), resident_wgs_per_cu(g_persist_resident[form], kPersistRows[form].kern, 256, cap, cap));
  if (mode != 2) {
    // default rule: a launch must fill the grid at least twice, or the workgroups' second tiles - where the overlap is - do not exist; and the
    // 32-wide tile stays on rungemm_kernel: its epilogue is a quarter of the 128-wide one's, and the mask layer (N = 16, 15 488 tiles) measured
    // 187 -> 198 us alone in the persistent form (profiles/rungemm_persist_notes.md)
    if (tiles < 2 * grid || bn < 64) return false;
    if (mode == 3 && d.stats.arena < 0) return false;  // measurement arm: the forward layers (they carry statistics) only
  }
  *c = KernelChoice{kFamPersist, form, cap_grid(grid, tiles)};
  return true;
}

void rungemm_persist_launch(const RunGemm& d, const KernelChoice& c, const ArenaBases& ab, hipStream_t st) {
  hipLaunchKernelGGL(kPersistRows[c.form].kern, dim3(c.grid), dim3(256), 0, st, d, ab);
}

}  // namespace sefd
