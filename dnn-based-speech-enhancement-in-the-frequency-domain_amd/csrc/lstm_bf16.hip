// bf16 variant of the persistent LSTM recurrence (see kernels.hip for the fp32 parity version and the design notes).
// v_mfma_f32_16x16x32_bf16: A[i=l&15][k=8*(l>>4)+e], B[k=8*(l>>4)+e][j=l&15], D[row=4*(l>>4)+r][col=l&15], fp32 accumulate.
// Arithmetic contract of bf16 mode: the recurrent operands (h_{t-1}, W_hh, and dgates_t in the backward) are rounded to
// bf16; gate pre-activations from the input GEMM, the cell state and all gate math stay fp32.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "sefd_desc.h"
#include "tuning.h"
#include "dev_common.h"

// No implicit mul+add contraction in this file: with it the compiler fused the cell update `f*c + i*g` differently for the two
// packed row pairs of a lane (one v_pk_fma, one v_pk_mul + v_pk_add), so a sequence's result depended on which of the 16 MFMA
// tile rows it sat in - 1e-7 in c, a flipped bf16 ulp in h a few frames later, 2e-3 at the output: eval-mode batch independence
// failed in bf16 (tests/test_gpu_model.py::test_bf16_full_shape_properties_at_bench_size).  Fused operations are written out.
#pragma clang fp contract(off)

namespace sefd {

__device__ __forceinline__ uint32_t pack2(float a, float b) { return pack_bf16x2(a, b); }

// Gate math on pairs of cells: the non-transcendental half of a sigmoid / tanh / cell update compiles to packed fp32
// (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32, two lanes-worth per issue slot); v_exp_f32 / v_rcp_f32 stay scalar.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 exp2_2(f32x2 x) { return f32x2{__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)}; }
__device__ __forceinline__ f32x2 rcp_2(f32x2 x) { return f32x2{__builtin_amdgcn_rcpf(x.x), __builtin_amdgcn_rcpf(x.y)}; }
__device__ __forceinline__ f32x2 sigmoid2(f32x2 x) { return rcp_2(exp2_2(x * -1.4426950408889634f) + 1.f); }
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 tanh2(f32x2 x) { return fma2(rcp_2(exp2_2(x * 2.8853900817779268f) + 1.f), f32x2{-2.f, -2.f}, f32x2{1.f, 1.f}); }

// H is a compile-time constant (32 / 64 / 96 / 128): with run-time trip counts hipcc guards every MFMA with a branch and
// drains the software-prefetched loads before the matrix section, which serialises the 483-step loop.
// RPW = sequences per workgroup.  16: every row of the 16-row MFMA tile is a sequence, a lane owns 4 cells (rows 4*kq .. 4*kq+3).
// 4: the sequences sit in tile rows 0, 4, 8, 12 and a lane owns ONE cell (row 4*kq): the step loop is bound by the gate math a lane
// issues (5 exp + 5 rcp per cell at quarter rate), not by the MFMAs, and the recurrence of a DCCRN step (B = 32, 4 groups) fills 8 of
// 256 CUs - four times the workgroups, a quarter of the per-step issue (forward LSTM of the default step: 1.03 -> ~0.4 ms exposed).
// The per-element arithmetic is the same in both variants (same operations in the same order), only the packing differs.
// DIR: some group of the launch walks the frames backwards (LstmRec::rev_mask, the reverse direction of a bidirectional layer): logical step s of a
// reversed group is physical frame T - 1 - s and its predecessor the frame after it.  Steps, the LDS double buffer and the prefetch ring are counted in
// logical steps; only the addresses of gx, h, c and the saved gates run the other way (the prefetch clamp of the last logical step is then frame 0).
// Such a launch covers the whole sequence (the launcher refuses t0 / t1).  With DIR = false the strides below are the compile-time constants they were.
template <int HMAX, int RPW, bool DIR>
__global__ __launch_bounds__(HMAX * 4) void lstm_fwd_bf16_kernel(const LstmRec d, const ArenaBases ab) {
  extern __shared__ __attribute__((aligned(16))) uint16_t ldsh[];
  constexpr int H = HMAX;
  const int T = d.T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = blockIdx.y, b0 = blockIdx.x * RPW;
  const bool rev = DIR && ((d.rev_mask >> g) & 1);
  constexpr int NR = RPW == 16 ? 4 : 1;            // cells per lane
  const float* whh = reinterpret_cast<const float*>(rp(ab, d.whh[g % d.nset]));
  const float* gx = reinterpret_cast<const float*>(rp(ab, d.gx)) + d.gx_goff[g];
  uint16_t* hout = reinterpret_cast<uint16_t*>(rp(ab, d.h));
  float* gates = reinterpret_cast<float*>(rp(ab, d.gates));
  float* cs = reinterpret_cast<float*>(rp(ab, d.c));
  constexpr int hs = H + 8;                       // LDS row stride in bf16 elements (16-byte aligned rows, rotating 16-B slots)
  constexpr int KS = H / 32;
  const int unit = 16 * w + (lane & 15);
  const int kq = lane >> 4;

  uint4 wreg[4][HMAX / 32];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int ks = 0; ks < HMAX / 32; ++ks) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (ks < KS) {
        const float* p = whh + (int64_t)(q * H + unit) * H + 32 * ks + 8 * kq;
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        v = make_uint4(pack2(a.x, a.y), pack2(a.z, a.w), pack2(b.x, b.y), pack2(b.z, b.w));
      }
      wreg[q][ks] = v;
    }
  for (int i = threadIdx.x; i < 2 * 16 * hs; i += blockDim.x) ldsh[i] = 0;
  __syncthreads();
  const int tb = d.t0, te = d.t1 > 0 ? d.t1 : T;         // this launch covers frames [tb, te); tb > 0 resumes from the saved state

  bool rvalid[NR];
  int64_t rowbt[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int b = RPW == 16 ? b0 + 4 * kq + r : b0 + kq;
    rvalid[r] = b < d.B;
    rowbt[r] = (int64_t)(rvalid[r] ? b : 0) * T;
  }
  float c[NR] = {};
  // The step loop is issue-bound (two waves per SIMD, ~300 instructions per step before this layout): the four gates of a
  // (row, unit) cell are adjacent in gx and in the saved gates (sefd_desc.h gate_col), so a lane moves a cell with ONE 16-byte
  // load and ONE 16-byte store, addresses advance by constants, and the two-step prefetch ring is unrolled (no copies).
  const int64_t GBT = (int64_t)d.B * T;
  const float* gxp[NR];                          // gx of (row r, this unit), current prefetch position
  int64_t so[NR];                               // (g*GBT + row*T + t) * H + unit : element offset of the cell in h / c, x4 in gates
  const int f0 = rev ? T - 1 : tb;              // physical frame of the first step
  const int64_t hstep = rev ? -H : H;           // one logical step in h / c
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    gxp[r] = gx + (rowbt[r] + f0) * d.gx_ld + gate_col(0, unit);     // rows >= B alias row 0 (in either direction), never stored
    so[r] = ((int64_t)g * GBT + rowbt[r] + f0) * H + unit;
    if (tb > 0) {                                                    // h[tb-1] into the LDS buffer step tb reads, c[tb-1] into registers
      c[r] = cs[so[r] - H];
      ldsh[(tb & 1) * 16 * hs + (4 * kq + r) * hs + unit] = hout[so[r] - H];
    }
  }
  if (tb > 0) __syncthreads();
  const int64_t gx_ld = rev ? -(int64_t)d.gx_ld : (int64_t)d.gx_ld;    // one logical step in gx
  auto load_gx = [&](int t, float4 (&dst)[NR]) {                        // t is clamped: the last two prefetches re-read step T-1
    const int64_t inc = t < T - 1 ? gx_ld : 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) { dst[r] = *reinterpret_cast<const float4*>(gxp[r]); gxp[r] += inc; }
  };
  auto step = [&](int t, const float4 (&cur)[NR], float4 (&pre)[NR]) {
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NR; ++r) { acc[0][r] = cur[r].x; acc[1][r] = cur[r].y; acc[2][r] = cur[r].z; acc[3][r] = cur[r].w; }
    load_gx(t + 2, pre);                        // gate pre-activations two steps ahead: one step does not cover an HBM round trip
    const int hp = (t & 1) * 16 * hs;           // LDS offsets, not pointers: keeps the accesses in the LDS address space (ds_*, not flat_*)
    if (t > 0) {
#pragma unroll
      for (int ks = 0; ks < HMAX / 32; ++ks) {
        if (ks < KS) {
          const uint4 a = *reinterpret_cast<const uint4*>(&ldsh[hp + (lane & 15) * hs + 32 * ks + 8 * kq]);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, wreg[q][ks]), acc[q], 0, 0, 0);
        }
      }
    }
    const int hn = ((t + 1) & 1) * 16 * hs;
    if constexpr (RPW == 16) {
#pragma unroll
    for (int rp2 = 0; rp2 < 4; rp2 += 2) {
      const f32x2 ig = sigmoid2(f32x2{acc[0][rp2], acc[0][rp2 + 1]}), fg = sigmoid2(f32x2{acc[1][rp2], acc[1][rp2 + 1]});
      const f32x2 gg = tanh2(f32x2{acc[2][rp2], acc[2][rp2 + 1]}), og = sigmoid2(f32x2{acc[3][rp2], acc[3][rp2 + 1]});
      const f32x2 cn = fma2(fg, f32x2{c[rp2], c[rp2 + 1]}, ig * gg);
      const f32x2 hv = og * tanh2(cn);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int r = rp2 + k;
        c[r] = cn[k];
        const uint16_t hb = f2bf(hv[k]);
        ldsh[hn + (4 * kq + r) * hs + unit] = hb;
        if (rvalid[r]) {
          hout[so[r]] = hb;
          *reinterpret_cast<float4*>(gates + so[r] * 4) = make_float4(ig[k], fg[k], gg[k], og[k]);
          cs[so[r]] = cn[k];
        }
        so[r] += hstep;
      }
    }
    } else {
      const f32x2 s = sigmoid2(f32x2{acc[0][0], acc[1][0]});                                                   // i, f
      const f32x2 v = rcp_2(exp2_2(f32x2{acc[2][0], acc[3][0]} * f32x2{2.8853900817779268f, -1.4426950408889634f}) + 1.f);
      const float gg = __builtin_fmaf(v.x, -2.f, 1.f), og = v.y;                                               // tanh(g), sigmoid(o): tanh2 / sigmoid2 written out
      const float cn = __builtin_fmaf(s.y, c[0], s.x * gg);
      const float hv = og * __builtin_fmaf(__builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(cn * 2.8853900817779268f) + 1.f), -2.f, 1.f);
      c[0] = cn;
      const uint16_t hb = f2bf(hv);
      ldsh[hn + 4 * kq * hs + unit] = hb;
      if (rvalid[0]) {
        hout[so[0]] = hb;
        *reinterpret_cast<float4*>(gates + so[0] * 4) = make_float4(s.x, s.y, gg, og);
        cs[so[0]] = cn;
      }
      so[0] += hstep;
    }
    lds_barrier();
  };
  float4 b0v[NR], b1v[NR], b2v[NR];
  load_gx(tb, b0v);
  load_gx(tb + 1, b1v);
  int t = tb;
  for (; t + 3 <= te; t += 3) {
    step(t, b0v, b2v);
    step(t + 1, b1v, b0v);
    step(t + 2, b2v, b1v);
  }
  if (t < te) { step(t, b0v, b2v); ++t; }
  if (t < te) { step(t, b1v, b0v); ++t; }
}

// RPW as in the forward kernel.  4: the sequences sit in rows 0, 4, 8, 12 of the dgates tile (A operand), so the accumulator row a lane
// reads back (row 4*kq of dh_{t-1} = dgates_t . W_hh) is the ONE cell whose gate gradients it forms: a quarter of the loads and of the
// gate math per lane and four times the workgroups (DCCRN step: 8 -> 32 of 256 CUs).  Same operations in the same order per element.
// DIR as in the forward kernel: the backward of a reversed group walks the physical frames 0 -> T - 1 and hands dh to frame t + 1.  `t` below stays the
// logical step (T - 1 down to 0, so the three-frame rotation and its tails are the same); the fetch and store positions move the other way.
template <int HMAX, int RPW, bool DIR>
__global__ __launch_bounds__(HMAX * 4) void lstm_bwd_bf16_kernel(const LstmRec d, const ArenaBases ab) {
  extern __shared__ __attribute__((aligned(16))) uint16_t ldsh[];
  constexpr int H = HMAX;
  const int T = d.T;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = blockIdx.y, b0 = blockIdx.x * RPW;
  const bool rev = DIR && ((d.rev_mask >> g) & 1);
  constexpr int NR = RPW == 16 ? 4 : 1;            // cells per lane
  const float* whh = reinterpret_cast<const float*>(rp(ab, d.whh[g % d.nset]));
  const float* gates = reinterpret_cast<const float*>(rp(ab, d.gates));
  const float* cs = reinterpret_cast<const float*>(rp(ab, d.c));
  const float* dh = reinterpret_cast<const float*>(rp(ab, d.dh));
  uint16_t* dgo = reinterpret_cast<uint16_t*>(rp(ab, d.dgates));
  constexpr int gs = 4 * H + 8;
  const int unit = 16 * w + (lane & 15);
  const int kq = lane >> 4;
  constexpr int KS = 4 * H / 32;

  // B[k = gate column][j = unit] = W_hh[torch row of that column][unit]; the LDS tile (and dgates in memory) use the
  // unit-major gate-column order of sefd_desc.h, the parameter keeps PyTorch's gate-major rows
  uint4 wreg[HMAX / 8];
#pragma unroll
  for (int ks = 0; ks < HMAX / 8; ++ks) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ks < KS) {
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = whh[(int64_t)gate_torch_row(32 * ks + 8 * kq + e, H) * H + unit];
      v = make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7]));
    }
    wreg[ks] = v;
  }
  if constexpr (RPW != 16) {                     // tile rows that hold no sequence are multiplied too (results unused): keep them finite
    for (int i = threadIdx.x; i < 16 * gs; i += blockDim.x) ldsh[i] = 0;
    __syncthreads();
  }
  bool rvalid[NR];
  int64_t fo[NR];                               // fetch position: (g*GBT + row*T + t) * H + unit
  const int64_t GBT = (int64_t)d.B * T;
  const int fl = rev ? 0 : T - 1;               // physical frame of the last logical step, where the walk starts
  const int64_t hback = rev ? -H : H;           // one logical step back in h / c / dh
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int b = RPW == 16 ? b0 + 4 * kq + r : b0 + kq;
    rvalid[r] = b < d.B;
    fo[r] = ((int64_t)g * GBT + (int64_t)(rvalid[r] ? b : 0) * T + fl) * H + unit;   // rows >= B alias row 0 (in either direction), results unused
  }
  // dgates_t leave through the LDS tile with 16-byte stores: H/2 chunks per sequence; RPW 16: 2 chunks per thread (tile rows w', w'+8),
  // RPW 4: threads 0 .. 2H-1 move one chunk each (tile rows 0, 4, 8, 12)
  constexpr int CPR = H / 2;
  constexpr int ND = RPW == 16 ? 2 : 1;
  const int crow = threadIdx.x / CPR, cc8 = threadIdx.x % CPR;
  uint16_t* dptr[ND];
  bool dvalid[ND];
  int drow[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    const int b = RPW == 16 ? b0 + crow + 8 * i : b0 + crow;
    drow[i] = RPW == 16 ? crow + 8 * i : 4 * (crow & 3);
    dvalid[i] = b < d.B && (RPW == 16 || crow < 4);
    dptr[i] = dgo + d.gx_goff[g] + ((int64_t)(dvalid[i] ? b : 0) * T + fl) * d.gx_ld + cc8 * 8;
  }
  const int64_t gx_ld = rev ? -(int64_t)d.gx_ld : (int64_t)d.gx_ld;    // one logical step back in dgates

  float dcarry[NR] = {};
  f32x4 dhrec = {0.f, 0.f, 0.f, 0.f};
  // software prefetch ring, two steps of look-ahead (one step does not cover an HBM round trip); unrolled, no copies
  struct Sav { float4 g[NR]; float cp[NR], dh[NR]; };
  auto fetch = [&](int t_, Sav& s) {            // reads the current position, then steps back one logical step (stays at step 0)
    const int64_t back = t_ > 0 ? hback : 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      s.g[r] = *reinterpret_cast<const float4*>(gates + fo[r] * 4);
      s.cp[r] = cs[fo[r] - back];
      s.dh[r] = dh[fo[r]];
      fo[r] -= back;
    }
  };
  float pct[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) pct[r] = cs[fo[r]];
  auto step = [&](int t, const Sav& cur, Sav& pre) {
    fetch(t - 2, pre);
    if constexpr (RPW == 16) {
#pragma unroll
    for (int rp2 = 0; rp2 < 4; rp2 += 2) {
      const f32x2 ig = {cur.g[rp2].x, cur.g[rp2 + 1].x}, fg = {cur.g[rp2].y, cur.g[rp2 + 1].y};
      const f32x2 gg = {cur.g[rp2].z, cur.g[rp2 + 1].z}, og = {cur.g[rp2].w, cur.g[rp2 + 1].w};
      const f32x2 ct = {pct[rp2], pct[rp2 + 1]};
      const f32x2 cp = t > 0 ? f32x2{cur.cp[rp2], cur.cp[rp2 + 1]} : f32x2{0.f, 0.f};
      const f32x2 dht = f32x2{cur.dh[rp2], cur.dh[rp2 + 1]} + f32x2{dhrec[rp2], dhrec[rp2 + 1]};
      const f32x2 tc = tanh2(ct);
      f32x2 dog = dht * tc * og * (1.f - og);
      const f32x2 dc = dht * og * (1.f - tc * tc) + f32x2{dcarry[rp2], dcarry[rp2 + 1]};
      f32x2 di = dc * gg * ig * (1.f - ig);
      f32x2 df = dc * cp * fg * (1.f - fg);
      f32x2 dg = dc * ig * (1.f - gg * gg);
      const f32x2 dcn = dc * fg;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int r = rp2 + k;
        const bool v = rvalid[r];                 // rows beyond the batch alias row 0: their gradients are forced to zero
        dcarry[r] = v ? dcn[k] : 0.f;
        pct[r] = cur.cp[r];                       // c_{t-1} is the cell state of the next (earlier) step
        *reinterpret_cast<uint2*>(ldsh + (4 * kq + r) * gs + gate_col(0, unit)) =
            v ? make_uint2(pack2(di[k], df[k]), pack2(dg[k], dog[k])) : make_uint2(0u, 0u);
      }
    }
    } else {                                      // the same expressions, one cell
      const float ig = cur.g[0].x, fg = cur.g[0].y, gg = cur.g[0].z, og = cur.g[0].w;
      const float cp = t > 0 ? cur.cp[0] : 0.f;
      const float dht = cur.dh[0] + dhrec[0];
      const float tc = __builtin_fmaf(__builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(pct[0] * 2.8853900817779268f) + 1.f), -2.f, 1.f);
      const float dog = dht * tc * og * (1.f - og);
      const float dc = dht * og * (1.f - tc * tc) + dcarry[0];
      const float di = dc * gg * ig * (1.f - ig);
      const float df = dc * cp * fg * (1.f - fg);
      const float dg = dc * ig * (1.f - gg * gg);
      const bool v = rvalid[0];
      dcarry[0] = v ? dc * fg : 0.f;
      pct[0] = cur.cp[0];
      *reinterpret_cast<uint2*>(ldsh + 4 * kq * gs + gate_col(0, unit)) = v ? make_uint2(pack2(di, df), pack2(dg, dog)) : make_uint2(0u, 0u);
    }
    lds_barrier();
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      if (dvalid[i]) *reinterpret_cast<uint4*>(dptr[i]) = *reinterpret_cast<const uint4*>(ldsh + drow[i] * gs + cc8 * 8);
      dptr[i] -= gx_ld;
    }
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    if (t > 0) {
#pragma unroll
      for (int ks = 0; ks < HMAX / 8; ks += 2) {
        if (ks < KS) {
          const uint4 x0 = *reinterpret_cast<const uint4*>(ldsh + (lane & 15) * gs + 32 * ks + 8 * kq);
          const uint4 x1 = *reinterpret_cast<const uint4*>(ldsh + (lane & 15) * gs + 32 * (ks + 1) + 8 * kq);
          a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x0), __builtin_bit_cast(bf16x8, wreg[ks]), a0, 0, 0, 0);
          a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x1), __builtin_bit_cast(bf16x8, wreg[ks + 1]), a1, 0, 0, 0);
        }
      }
    }
    dhrec = a0 + a1;
    lds_barrier();
  };
  Sav s0, s1, s2;
  fetch(T - 1, s0);
  fetch(T - 2, s1);
  int t = T - 1;
  for (; t >= 2; t -= 3) {
    step(t, s0, s2);
    step(t - 1, s1, s0);
    step(t - 2, s2, s1);
  }
  if (t >= 0) { step(t, s0, s2); --t; }
  if (t >= 0) { step(t, s1, s0); --t; }
}

template <int HMAX, bool DIR>
static void launch_t(const LstmRec& d, const ArenaBases& ab, hipStream_t st, bool fwd) {
  dim3 grid((d.B + 15) / 16, d.G);
  dim3 block(64 * (d.H / 16));
  // LSTM_RPW = 4 / 16 forces a variant for both directions, LSTM_RPW_BWD for the backward alone (read per launch: the per-op test
  // runs both variants in one process)
  const int rpw_both = (int)tune_int("LSTM_RPW", 0);
  const int rpw_env = fwd ? rpw_both : (int)tune_int("LSTM_RPW_BWD", rpw_both);
  const bool spread = rpw_env ? rpw_env == 4 : (int64_t)((d.B + 3) / 4) * d.G <= 1024;      // one cell per lane while the chip has CUs to spare
  if (fwd && spread) hipLaunchKernelGGL((lstm_fwd_bf16_kernel<HMAX, 4, DIR>), dim3((d.B + 3) / 4, d.G), block, 2 * 16 * (d.H + 8) * sizeof(uint16_t), st, d, ab);
  else if (fwd) hipLaunchKernelGGL((lstm_fwd_bf16_kernel<HMAX, 16, DIR>), grid, block, 2 * 16 * (d.H + 8) * sizeof(uint16_t), st, d, ab);
  else if (spread) hipLaunchKernelGGL((lstm_bwd_bf16_kernel<HMAX, 4, DIR>), dim3((d.B + 3) / 4, d.G), block, 16 * (4 * d.H + 8) * sizeof(uint16_t), st, d, ab);
  else hipLaunchKernelGGL((lstm_bwd_bf16_kernel<HMAX, 16, DIR>), grid, block, 16 * (4 * d.H + 8) * sizeof(uint16_t), st, d, ab);
}

template <bool DIR>
static void launch_h(const LstmRec& d, const ArenaBases& ab, hipStream_t st, bool fwd) {
  switch (d.H) {          // planner guarantees H % 32 == 0, H <= 128 and gdt == bf16 in bf16 mode
    case 32: launch_t<32, DIR>(d, ab, st, fwd); break;
    case 64: launch_t<64, DIR>(d, ab, st, fwd); break;
    case 96: launch_t<96, DIR>(d, ab, st, fwd); break;
    default: launch_t<128, DIR>(d, ab, st, fwd); break;
  }
}

__global__ void lstm_bf16_refuse_kernel(int* host_word, int* dev_word) { set_status(host_word, dev_word); }

void launch_lstm_bf16(const LstmRec& d, const ArenaBases& ab, hipStream_t st, bool fwd) {
  // a reversed group resumes from no saved state: its launch covers the whole sequence (t0 = t1 = 0), of at most 4 groups (gx_goff).  Anything else is
  // not launched; the plan's status word says so, as the cluster launcher does (lstm_cluster.hip).  The DIR instantiations run only when a group is reversed
  const int mask = lstm_rev_groups(d);
  if (mask != 0 && (d.t0 != 0 || d.t1 != 0 || d.G > 4)) {
    hipLaunchKernelGGL(lstm_bf16_refuse_kernel, dim3(1), dim3(1), 0, st, ab.status, ab.dstatus);
    return;
  }
  if (mask != 0) launch_h<true>(d, ab, st, fwd);
  else launch_h<false>(d, ab, st, fwd);
}

}  // namespace sefd
