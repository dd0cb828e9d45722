// BaseModel on its own (tools_for_model.py:801-1185): `unfold` and the seven norms as streaming kernels on tensors in the REFERENCE's layout,
// fp32 [rows][F][T] with the frames contiguous (the fsn_* kernels of fsn.hip do the same arithmetic on the FullSubNet plan's time-major buffers
// with the sub-band gather fused in; they cannot be called on a tensor).
//
// Lanes run along T: a thread owns one "unit" of frames - 4 consecutive frames read and written as one 16-byte access when T % 4 == 0 and every
// base pointer is 16-byte aligned, one frame otherwise (same values, lower bandwidth) - and walks down the bins.  A workgroup is 64 units x 4 waves,
// the waves interleave over the bins of one of FS bin ranges; grid = (rows, unit tiles, FS).  Offsets are 64-bit, statistics are double.
//
//   forward   reduce: per (row, range, frame) sum of x (and of x^2 for the layer norm)            -> partials (scratch)
//             scan  : one workgroup per row, 256 frames per chunk: adds the ranges in order, then a workgroup scan of the affine maps
//                     mu_t = A_t mu_{t-1} + B_t (a cumulative sum is A = 1) with the chunk's carry -> ws [rows][T] { mean, std } (double)
//             apply : y = x * mul_t + add_t
//   backward  reduce: per (row, range, frame) sum of g x (and of g for the layer norm)            -> partials
//             scan  : the adjoint recurrences / suffix sums, frames last to first                  -> coef [rows][T] { mul, add, xc } (scratch)
//             apply : dx = g * mul_t + add_t + x * xc_t   (sband, t >= L: add_t goes to bin F / 2 - 1 alone)
// The two offline norms take their statistics over all F * T values of a row: reduce over NS segments, one thread per row adds them in order.
// No atomics, no waits between workgroups, every sum in a fixed order: results are bit-identical from run to run, and a row's result depends on
// that row alone.  The partials and the backward's coefficients live in the caller's ws behind the statistics: the entry points only enqueue.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/sefd.h"
#include "dev_common.h"

namespace sefd {
namespace {

constexpr double kEpsF32 = 1.1920928955078125e-07;        // np.finfo(np.float32).eps: tools_for_model.py:798 (kNormEps of fsn.hip)
constexpr int kChunk = 256;                               // frames per scan step = threads of the scan workgroup
constexpr int kMaxFS = 16, kBinsPerRange = 32;            // bin ranges of the reduce / apply grids
constexpr int kSegment = 2048, kMaxNS = 256;              // values per workgroup of the offline kernels

enum { K_OFF_LAPLACE = 0, K_CUM_LAPLACE = 1, K_OFF_GAUSS = 2, K_CUM_LAYER = 3, K_FORGET = 4, K_SBAND = 5, K_HYBRID = 6 };

struct NormArgs {
  int kind, rows, F, T, L, FS, fper, NS;
  int64_t N, seg;              // offline: values per row, values per segment (a multiple of 4)
  double alpha;                // (L - 1) / (L + 1)
};

// The forgetting factor of frame t (tools_for_model.py:898-903, 932-938, 969-972).  Warm-up frames t < L: torch.min(torch.tensor([(t - 1) / (t + 1),
// alpha])) is a float32 tensor whatever the input's dtype, and `1 - alp` is taken in float32; later frames use the Python doubles.
__device__ __forceinline__ double forget_a(int t, int L, double alpha, double& one_minus) {
  if (t < L) {
    const double r = (double)(t - 1) / (double)(t + 1);
    const float af = (float)(r < alpha ? r : alpha);
    one_minus = (double)(1.f - af);
    return (double)af;
  }
  one_minus = 1.0 - alpha;
  return alpha;
}
__device__ __forceinline__ double norm_eps(int kind) { return kind == K_CUM_LAPLACE ? kEpsF32 : 1e-10; }

template <int V> struct Vec;
template <> struct Vec<1> {
  static __device__ __forceinline__ void ld(const float* p, float (&v)[1]) { v[0] = *p; }
  static __device__ __forceinline__ void st(float* p, const float (&v)[1]) { *p = v[0]; }
};
template <> struct Vec<4> {
  static __device__ __forceinline__ void ld(const float* p, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  }
  static __device__ __forceinline__ void st(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// ---------------------------------------------------------------------------------------------- per-frame sums over the bins
// NCH = 1: sum of a (forward: x; backward: g x).  NCH = 2: also the sum of x^2 (forward) / of g (backward).  part [rows][FS][NCH][T] double.
template <int V, int NCH, bool BWD>
__global__ __launch_bounds__(256) void bm_reduce_kernel(const NormArgs a, const float* __restrict__ x, const float* __restrict__ g, double* __restrict__ part) {
  __shared__ double sh[3][64][NCH * V];
  const int row = blockIdx.x, sp = blockIdx.z, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int U = a.T / V, u = blockIdx.y * 64 + lane;
  const int f0 = sp * a.fper, f1 = min(a.F, f0 + a.fper);
  double acc[NCH * V];
#pragma unroll
  for (int i = 0; i < NCH * V; ++i) acc[i] = 0;
  if (u < U) {
    for (int f = f0 + w; f < f1; f += 4) {
      const int64_t o = ((int64_t)row * a.F + f) * a.T + (int64_t)u * V;
      float xv[V], gv[V];
      Vec<V>::ld(x + o, xv);
      if (BWD) Vec<V>::ld(g + o, gv);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (BWD) {
          acc[v] += (double)gv[v] * xv[v];
          if (NCH == 2) acc[V + v] += gv[v];
        } else {
          acc[v] += xv[v];
          if (NCH == 2) acc[V + v] += (double)xv[v] * xv[v];
        }
      }
    }
  }
  if (w > 0) {
#pragma unroll
    for (int i = 0; i < NCH * V; ++i) sh[w - 1][lane][i] = acc[i];
  }
  __syncthreads();
  if (w == 0 && u < U) {
#pragma unroll
    for (int i = 0; i < NCH * V; ++i) {
      const double s = ((acc[i] + sh[0][lane][i]) + sh[1][lane][i]) + sh[2][lane][i];
      const int c = i / V, v = i - c * V;
      part[(((int64_t)row * a.FS + sp) * NCH + c) * a.T + (int64_t)u * V + v] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------- the scan over the frames
// Inclusive scan over the 256 threads of { affine map (A, B), two plain sums }, continued from `carry` (the state after the previous chunk).
// Thread i composes the maps of threads 0 .. i in order: 6 shuffle steps inside the wave, then the aggregates of the waves in front of it.
struct ScanVal { double A, B, s1, s2; };
__device__ __forceinline__ void block_scan(ScanVal& v, double (&carry)[3], ScanVal* wsh, double* csh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double Ap = __shfl_up(v.A, o), Bp = __shfl_up(v.B, o), p1 = __shfl_up(v.s1, o), p2 = __shfl_up(v.s2, o);
    if (lane >= o) { v.B = v.A * Bp + v.B; v.A = v.A * Ap; v.s1 += p1; v.s2 += p2; }
  }
  __syncthreads();                                  // the previous chunk's readers of wsh / csh are done
  if (lane == 63) wsh[w] = v;
  __syncthreads();
  double mu = carry[0], c1 = carry[1], c2 = carry[2];
  for (int k = 0; k < w; ++k) { mu = wsh[k].A * mu + wsh[k].B; c1 += wsh[k].s1; c2 += wsh[k].s2; }
  v.B = v.A * mu + v.B;                             // from here on: B = the state after this frame, s1 / s2 = the running sums
  v.s1 += c1; v.s2 += c2;
  if (threadIdx.x == kChunk - 1) { csh[0] = v.B; csh[1] = v.s1; csh[2] = v.s2; }
  __syncthreads();
  carry[0] = csh[0]; carry[1] = csh[1]; carry[2] = csh[2];
}

// forward: ws [rows][T][2] = { mean_t, std_t (layer norm; 0 otherwise) }
__global__ __launch_bounds__(kChunk) void bm_scan_fwd_kernel(const NormArgs a, const float* __restrict__ x, const double* __restrict__ part, double* __restrict__ stat) {
  __shared__ ScanVal wsh[4];
  __shared__ double csh[3];
  const int row = blockIdx.x, nch = a.kind == K_CUM_LAYER ? 2 : 1;
  double carry[3] = {0, 0, 0};
  for (int c0 = 0; c0 < a.T; c0 += kChunk) {
    const int t = c0 + threadIdx.x;
    const bool ok = t < a.T;
    ScanVal v{1.0, 0.0, 0.0, 0.0};
    if (ok) {
      double s = 0, q = 0;
      for (int sp = 0; sp < a.FS; ++sp) {
        const int64_t o = (((int64_t)row * a.FS + sp) * nch) * a.T + t;
        s += part[o];
        if (nch == 2) q += part[o + a.T];
      }
      v.s1 = s; v.s2 = q;
      if (a.kind >= K_FORGET) {
        double om;
        const double al = forget_a(t, a.L, a.alpha, om);
        if (a.kind == K_SBAND && t >= a.L) { v.A = al; v.B = om * (double)x[((int64_t)row * a.F + (a.F / 2 - 1)) * a.T + t]; }
        else if (a.kind == K_HYBRID && t >= a.L) { v.A = 0.0; v.B = 0.0; }
        else { v.A = al; v.B = om * (s / (double)a.F); }
      }
    }
    block_scan(v, carry, wsh, csh);
    if (ok) {
      const double n = (double)a.F * (double)(t + 1);
      double m, sd = 0.0;
      if (a.kind == K_CUM_LAPLACE) m = v.s1 / n;
      else if (a.kind == K_CUM_LAYER) { m = v.s1 / n; sd = sqrt((v.s2 - 2.0 * m * v.s1) / n + m * m + kEpsF32); }
      else if (a.kind == K_HYBRID) m = t < a.L ? v.B : v.s1 / n;
      else m = v.B;
      stat[((int64_t)row * a.T + t) * 2] = m;
      stat[((int64_t)row * a.T + t) * 2 + 1] = sd;
    }
  }
}

// backward, frames last to first (thread i of a chunk owns frame T - 1 - (c0 + i)).  With den_t the forward's denominator and S_t = sum_f g x / den_t^2:
//   cumulative_laplace : dx = g / den_t - sum_{u >= t} S_u / n_u                                                n_u = F (u + 1)
//   forgetting         : lam_t = -S_t + a_{t+1} lam_{t+1};  dx = g / den_t + (1 - a_t) lam_t / F
//   sband_forgetting   : the same; for t >= L the term (1 - alpha) lam_t goes to bin F / 2 - 1 alone
//   hybrid             : lam runs among the warm-up frames only (nothing enters lam_{L-1} from later frames); every frame also gets
//                        - sum_{u >= max(t, L)} S_u / n_u
//   cumulative_layer   : dx = g / sd_t - sum_{u >= t} [ G_u / (n_u sd_u) + (x - m_u) Sy_u / (n_u sd_u^2) ],  G = sum_f g, Sy = sum_f g y
// coef [rows][T][3] = { mul, add, xc }: dx = g mul + add + x xc.
__global__ __launch_bounds__(kChunk) void bm_scan_bwd_kernel(const NormArgs a, const double* __restrict__ part, const double* __restrict__ stat, double* __restrict__ coef) {
  __shared__ ScanVal wsh[4];
  __shared__ double csh[3];
  const int row = blockIdx.x, nch = a.kind == K_CUM_LAYER ? 2 : 1;
  double carry[3] = {0, 0, 0};
  for (int c0 = 0; c0 < a.T; c0 += kChunk) {
    const int i = c0 + threadIdx.x, t = a.T - 1 - i;
    const bool ok = i < a.T;
    ScanVal v{1.0, 0.0, 0.0, 0.0};
    double m = 0, sd = 1, mul = 0, om_t = 0;
    const double n = (double)a.F * (double)(t + 1);
    if (ok) {
      double p0 = 0, p1 = 0;
      for (int sp = 0; sp < a.FS; ++sp) {
        const int64_t o = (((int64_t)row * a.FS + sp) * nch) * a.T + t;
        p0 += part[o];
        if (nch == 2) p1 += part[o + a.T];
      }
      m = stat[((int64_t)row * a.T + t) * 2];
      sd = stat[((int64_t)row * a.T + t) * 2 + 1];
      if (a.kind == K_CUM_LAYER) {
        const double Sy = (p0 - m * p1) / sd, bb = Sy / (n * sd * sd);
        mul = 1.0 / sd;
        v.B = p1 / (n * sd); v.s1 = bb; v.s2 = bb * m;                       // A = 1: three suffix sums
      } else {
        const double den = m + norm_eps(a.kind), S = p0 / (den * den);
        mul = 1.0 / den;
        if (a.kind == K_CUM_LAPLACE) {
          v.s1 = S / n;
        } else {
          double om_next;
          const double a_next = forget_a(t + 1, a.L, a.alpha, om_next);
          (void)forget_a(t, a.L, a.alpha, om_t);
          if (a.kind == K_HYBRID) {
            if (t >= a.L) { v.A = 0.0; v.B = 0.0; v.s1 = S / n; }
            else { v.A = t + 1 < a.L ? a_next : 0.0; v.B = -S; }
          } else {
            v.A = a_next; v.B = -S;
          }
        }
      }
    }
    block_scan(v, carry, wsh, csh);
    if (ok) {
      double add, xc = 0.0;
      if (a.kind == K_CUM_LAYER) { add = v.s2 - v.B; xc = -v.s1; }
      else if (a.kind == K_CUM_LAPLACE) add = -v.s1;
      else if (a.kind == K_HYBRID) add = (t < a.L ? om_t * v.B / (double)a.F : 0.0) - v.s1;
      else if (a.kind == K_SBAND && t >= a.L) add = om_t * v.B;              // to bin F / 2 - 1 alone (bm_apply_kernel)
      else add = om_t * v.B / (double)a.F;
      double* c = coef + ((int64_t)row * a.T + t) * 3;
      c[0] = mul; c[1] = add; c[2] = xc;
    }
  }
}

// ---------------------------------------------------------------------------------------------- apply
// forward: out = x mul + add from ws;  backward: out = g mul + add + x xc from coef (p = g)
template <int V, bool BWD>
__global__ __launch_bounds__(256) void bm_apply_kernel(const NormArgs a, const float* __restrict__ p, const float* __restrict__ x, const double* __restrict__ cf,
                                                      float* __restrict__ out) {
  const int row = blockIdx.x, sp = blockIdx.z, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int U = a.T / V, u = blockIdx.y * 64 + lane;
  if (u >= U) return;
  const int f0 = sp * a.fper, f1 = min(a.F, f0 + a.fper);
  double mul[V], add[V], xc[V], addbin[V];
  bool anyx = false;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int t = u * V + v;
    addbin[v] = 0.0; xc[v] = 0.0;
    if (BWD) {
      const double* c = cf + ((int64_t)row * a.T + t) * 3;
      mul[v] = c[0]; add[v] = c[1]; xc[v] = c[2];
      if (a.kind == K_SBAND && t >= a.L) { addbin[v] = add[v]; add[v] = 0.0; }
    } else {
      const double m = cf[((int64_t)row * a.T + t) * 2], sd = cf[((int64_t)row * a.T + t) * 2 + 1];
      if (a.kind == K_CUM_LAYER) { mul[v] = 1.0 / sd; add[v] = -m / sd; }
      else { mul[v] = 1.0 / (m + norm_eps(a.kind)); add[v] = 0.0; }
    }
  }
  anyx = BWD && a.kind == K_CUM_LAYER;
  const int bin = a.kind == K_SBAND ? a.F / 2 - 1 : -1;
  for (int f = f0 + w; f < f1; f += 4) {
    const int64_t o = ((int64_t)row * a.F + f) * a.T + (int64_t)u * V;
    float pv[V], xv[V], ov[V];
    Vec<V>::ld(p + o, pv);
    if (anyx) Vec<V>::ld(x + o, xv);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      double r = (double)pv[v] * mul[v] + add[v];
      if (f == bin) r += addbin[v];
      if (anyx) r += (double)xv[v] * xc[v];
      ov[v] = (float)r;
    }
    Vec<V>::st(out + o, ov);
  }
}

// ---------------------------------------------------------------------------------------------- offline norms: rows of N values
__device__ __forceinline__ double block_sum256(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
// part [rows][NS][2]: forward { sum x, sum x^2 }, backward { sum g x, sum g }.  A thread takes whole quads of values in both forms (V = 1 loads the
// four one by one and stops at the row's end), so the order of every sum - and the result, bit for bit - does not depend on the alignment.
template <int V, bool BWD>
__global__ __launch_bounds__(256) void bm_off_reduce_kernel(const NormArgs a, const float* __restrict__ x, const float* __restrict__ g, double* __restrict__ part) {
  __shared__ double sh[4];
  const int row = blockIdx.x, sp = blockIdx.y;
  const int64_t n0 = sp * a.seg, n1 = n0 + a.seg < a.N ? n0 + a.seg : a.N, base = (int64_t)row * a.N;
  double c0 = 0, c1 = 0;
  for (int64_t i = n0 + (int64_t)threadIdx.x * 4; i < n1; i += 256 * 4) {
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f};
    if (V == 4) {
      Vec<4>::ld(x + base + i, xv);
      if (BWD) Vec<4>::ld(g + base + i, gv);
    } else {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (i + v < n1) { xv[v] = x[base + i + v]; if (BWD) gv[v] = g[base + i + v]; }
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (V == 4 || i + v < n1) {
        if (BWD) { c0 += (double)gv[v] * xv[v]; c1 += gv[v]; }
        else { c0 += xv[v]; c1 += (double)xv[v] * xv[v]; }
      }
    }
  }
  c0 = block_sum256(c0, sh);
  c1 = block_sum256(c1, sh);
  if (threadIdx.x == 0) { part[((int64_t)row * a.NS + sp) * 2] = c0; part[((int64_t)row * a.NS + sp) * 2 + 1] = c1; }
}
// one thread per row.  forward: ws [rows][2] = { mean, unbiased std }.  backward: coef [rows][3] with
//   offline_laplace  : dx = g / den - sum(g x) / (den^2 N)                                   den = mean + 1e-5
//   offline_gaussian : dx = (g - G / N) / D - y Sy / ((N - 1) sd)      D = sd + 1e-5, y = (x - mean) / D, Sy = sum g y, G = sum g
template <bool BWD>
__global__ __launch_bounds__(64) void bm_off_final_kernel(const NormArgs a, const double* __restrict__ part, const double* __restrict__ stat_in, double* __restrict__ out) {
  const int row = blockIdx.x * 64 + threadIdx.x;
  if (row >= a.rows) return;
  double c0 = 0, c1 = 0;
  for (int sp = 0; sp < a.NS; ++sp) { c0 += part[((int64_t)row * a.NS + sp) * 2]; c1 += part[((int64_t)row * a.NS + sp) * 2 + 1]; }
  const double N = (double)a.N;
  if (!BWD) {
    const double mu = c0 / N;
    double sd = 0.0;
    if (a.kind == K_OFF_GAUSS) { const double var = (c1 - N * mu * mu) / (N - 1.0); sd = sqrt(var > 0 ? var : 0.0); }
    out[(int64_t)row * 2] = mu; out[(int64_t)row * 2 + 1] = sd;
  } else {
    const double mu = stat_in[(int64_t)row * 2], sd = stat_in[(int64_t)row * 2 + 1];
    double mul, add, xc = 0.0;
    if (a.kind == K_OFF_LAPLACE) {
      const double den = mu + 1e-5;
      mul = 1.0 / den; add = -c0 / (den * den * N);
    } else {
      // (a constant row has sd = 0: the division gives inf / NaN gradients, as the backward of torch.std does in the reference)
      const double D = sd + 1e-5, Sy = (c0 - mu * c1) / D, k = Sy / (D * (N - 1.0) * sd);
      mul = 1.0 / D; add = -c1 / (N * D) + mu * k; xc = -k;
    }
    out[(int64_t)row * 3] = mul; out[(int64_t)row * 3 + 1] = add; out[(int64_t)row * 3 + 2] = xc;
  }
}
template <int V, bool BWD>
__global__ __launch_bounds__(256) void bm_off_apply_kernel(const NormArgs a, const float* __restrict__ p, const float* __restrict__ x, const double* __restrict__ cf,
                                                          float* __restrict__ out) {
  const int row = blockIdx.x, sp = blockIdx.y;
  const int64_t n0 = sp * a.seg, n1 = n0 + a.seg < a.N ? n0 + a.seg : a.N, base = (int64_t)row * a.N;
  double mul, add, xc = 0.0;
  if (BWD) { mul = cf[(int64_t)row * 3]; add = cf[(int64_t)row * 3 + 1]; xc = cf[(int64_t)row * 3 + 2]; }
  else {
    const double mu = cf[(int64_t)row * 2], sd = cf[(int64_t)row * 2 + 1];
    if (a.kind == K_OFF_LAPLACE) { mul = 1.0 / (mu + 1e-5); add = 0.0; }
    else { mul = 1.0 / (sd + 1e-5); add = -mu * mul; }
  }
  const bool anyx = BWD && a.kind == K_OFF_GAUSS;
  for (int64_t i = n0 + (int64_t)threadIdx.x * V; i < n1; i += 256 * V) {
    float pv[V], xv[V], ov[V];
    Vec<V>::ld(p + base + i, pv);
    if (anyx) Vec<V>::ld(x + base + i, xv);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      double r = (double)pv[v] * mul + add;
      if (anyx) r += (double)xv[v] * xc;
      ov[v] = (float)r;
    }
    Vec<V>::st(out + base + i, ov);
  }
}

// ---------------------------------------------------------------------------------------------- unfold
// out [B][F][C][K][T], K = 2 n + 1: out[b, f, c, k, :] = x[b, c, reflect(f - n + k), :] - a gather of whole T-rows, one unit per thread
template <int V>
__global__ __launch_bounds__(256) void bm_unfold_fwd_kernel(const float* __restrict__ x, int B, int C, int F, int T, int n, float* __restrict__ out) {
  const int K = 2 * n + 1, U = T / V;
  const int64_t total = (int64_t)B * F * C * K * U;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int u = (int)(i % U);
    int64_t r = i / U;                                    // output row ((b F + f) C + c) K + k
    const int k = (int)(r % K); r /= K;
    const int c = (int)(r % C); r /= C;
    const int f = (int)(r % F);
    const int64_t b = r / F;
    int j = f - n + k;
    j = j < 0 ? -j : (j >= F ? 2 * (F - 1) - j : j);
    float v[V];
    Vec<V>::ld(x + ((b * C + c) * F + j) * T + (int64_t)u * V, v);
    Vec<V>::st(out + (i / U) * T + (int64_t)u * V, v);
  }
}
// The transposed gather written as a gather: dx[b, c, j, :] = sum of the g[b, f, c, k, :] with reflect(f - n + k) == j, in a fixed order - k ascending;
// per k the un-reflected position p = j (f = j + n - k), then the low mirror p = -j, then the high mirror p = 2 (F - 1) - j.  n < F: one fold at most.
template <int V>
__global__ __launch_bounds__(256) void bm_unfold_bwd_kernel(const float* __restrict__ g, int B, int C, int F, int T, int n, float* __restrict__ dx) {
  const int K = 2 * n + 1, U = T / V;
  const int64_t total = (int64_t)B * C * F * U;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int u = (int)(i % U);
    int64_t r = i / U;                                    // input row (b C + c) F + j
    const int j = (int)(r % F); r /= F;
    const int c = (int)(r % C);
    const int64_t b = r / C;
    double s[V];
#pragma unroll
    for (int v = 0; v < V; ++v) s[v] = 0.0;
    for (int k = 0; k < K; ++k) {
      const int o = n - k;
      const int cand[3] = {j + o, o - j, 2 * (F - 1) - j + o};
      const bool use[3] = {true, j > 0, j < F - 1};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int f = cand[q];
        if (use[q] && f >= 0 && f < F) {
          float gv[V];
          Vec<V>::ld(g + ((((b * F + f) * C + c) * K) + k) * T + (int64_t)u * V, gv);
#pragma unroll
          for (int v = 0; v < V; ++v) s[v] += gv[v];
        }
      }
    }
    float sv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) sv[v] = (float)s[v];
    Vec<V>::st(dx + (i / U) * T + (int64_t)u * V, sv);
  }
}

// ---------------------------------------------------------------------------------------------- host side
bool offline(int kind) { return kind == K_OFF_LAPLACE || kind == K_OFF_GAUSS; }

bool norm_args(int kind, int rows, int F, int T, int L, NormArgs& a) {
  if (kind < 0 || kind > K_HYBRID || rows < 1 || F < 1 || T < 1) return false;
  if (kind >= K_FORGET && L < 1) return false;
  if (kind == K_SBAND && F < 2) return false;
  const int64_t N = (int64_t)F * T;
  if (kind == K_OFF_GAUSS && N < 2) return false;
  a.kind = kind; a.rows = rows; a.F = F; a.T = T; a.L = kind >= K_FORGET ? L : 0;
  a.alpha = kind >= K_FORGET ? ((double)L - 1.0) / ((double)L + 1.0) : 0.0;
  const int64_t fs = ((int64_t)F + kBinsPerRange - 1) / kBinsPerRange;      // (the offline kinds pass F up to 2^31 - 1)
  a.FS = (int)(fs < kMaxFS ? fs : kMaxFS);
  a.fper = (int)(((int64_t)F + a.FS - 1) / a.FS);
  a.FS = (int)(((int64_t)F + a.fper - 1) / a.fper);       // no empty range
  a.N = N;
  int64_t ns = (N + kSegment - 1) / kSegment;
  if (ns > kMaxNS) ns = kMaxNS;
  a.seg = ((N + ns - 1) / ns + 3) / 4 * 4;
  a.NS = (int)((N + a.seg - 1) / a.seg);
  return true;
}
// ws, in doubles: the statistics (forward writes, backward reads), then the pair's scratch: the partial sums (each pass writes its own) and the
// backward's coefficients
struct WsLayout { int64_t stat, part, coef; int64_t total() const { return stat + part + coef; } };
WsLayout ws_layout(const NormArgs& a) {
  if (offline(a.kind)) return WsLayout{(int64_t)a.rows * 2, (int64_t)a.rows * a.NS * 2, (int64_t)a.rows * 3};
  const int nch = a.kind == K_CUM_LAYER ? 2 : 1;
  return WsLayout{(int64_t)a.rows * a.T * 2, (int64_t)a.rows * a.FS * nch * a.T, (int64_t)a.rows * a.T * 3};
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace sefd

extern "C" {
using namespace sefd;

int64_t sefd_norm_ws_floats(int32_t kind, int32_t rows, int32_t F, int32_t T) {
  NormArgs a;
  if (!norm_args(kind, rows, F, T, 1, a)) return -1;
  return 2 * ws_layout(a).total();
}

int32_t sefd_norm_forward(int32_t kind, const float* x, int32_t rows, int32_t F, int32_t T, int32_t sample_len, float* ws, float* y, void* stream) {
  NormArgs a;
  if (!x || !y || !ws || (reinterpret_cast<uintptr_t>(ws) & 7) || !norm_args(kind, rows, F, T, sample_len, a)) return -1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* stat = reinterpret_cast<double*>(ws);
  if (offline(kind)) {
    double* part = stat + ws_layout(a).stat;
    const bool v4 = a.N % 4 == 0 && aligned16(x) && aligned16(y);
    const dim3 grid(rows, a.NS);
    if (v4) hipLaunchKernelGGL((bm_off_reduce_kernel<4, false>), grid, dim3(256), 0, st, a, x, nullptr, part);
    else hipLaunchKernelGGL((bm_off_reduce_kernel<1, false>), grid, dim3(256), 0, st, a, x, nullptr, part);
    hipLaunchKernelGGL((bm_off_final_kernel<false>), dim3((rows + 63) / 64), dim3(64), 0, st, a, part, nullptr, stat);
    if (v4) hipLaunchKernelGGL((bm_off_apply_kernel<4, false>), grid, dim3(256), 0, st, a, x, nullptr, stat, y);
    else hipLaunchKernelGGL((bm_off_apply_kernel<1, false>), grid, dim3(256), 0, st, a, x, nullptr, stat, y);
    return hipGetLastError() == hipSuccess ? 0 : -2;
  }
  const int nch = kind == K_CUM_LAYER ? 2 : 1;
  double* part = stat + ws_layout(a).stat;
  const bool v4 = T % 4 == 0 && aligned16(x) && aligned16(y);
  const int U = v4 ? T / 4 : T;
  const dim3 grid(rows, (U + 63) / 64, a.FS);
  if (nch == 2) {
    if (v4) hipLaunchKernelGGL((bm_reduce_kernel<4, 2, false>), grid, dim3(256), 0, st, a, x, nullptr, part);
    else hipLaunchKernelGGL((bm_reduce_kernel<1, 2, false>), grid, dim3(256), 0, st, a, x, nullptr, part);
  } else {
    if (v4) hipLaunchKernelGGL((bm_reduce_kernel<4, 1, false>), grid, dim3(256), 0, st, a, x, nullptr, part);
    else hipLaunchKernelGGL((bm_reduce_kernel<1, 1, false>), grid, dim3(256), 0, st, a, x, nullptr, part);
  }
  hipLaunchKernelGGL(bm_scan_fwd_kernel, dim3(rows), dim3(kChunk), 0, st, a, x, part, stat);
  if (v4) hipLaunchKernelGGL((bm_apply_kernel<4, false>), grid, dim3(256), 0, st, a, x, nullptr, stat, y);
  else hipLaunchKernelGGL((bm_apply_kernel<1, false>), grid, dim3(256), 0, st, a, x, nullptr, stat, y);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int32_t sefd_norm_backward(int32_t kind, const float* x, const float* grad_y, int32_t rows, int32_t F, int32_t T, int32_t sample_len, const float* ws,
                           float* grad_x, void* stream) {
  NormArgs a;
  if (!x || !grad_y || !grad_x || !ws || (reinterpret_cast<uintptr_t>(ws) & 7) || !norm_args(kind, rows, F, T, sample_len, a)) return -1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // ws is const for the statistics' sake; what follows them is the scratch of this forward / backward pair, and the backward overwrites it
  const double* stat = reinterpret_cast<const double*>(ws);
  const WsLayout lay = ws_layout(a);
  double* part = const_cast<double*>(stat) + lay.stat;
  double* coef = part + lay.part;
  if (offline(kind)) {
    const bool v4 = a.N % 4 == 0 && aligned16(x) && aligned16(grad_y) && aligned16(grad_x);
    const dim3 grid(rows, a.NS);
    if (v4) hipLaunchKernelGGL((bm_off_reduce_kernel<4, true>), grid, dim3(256), 0, st, a, x, grad_y, part);
    else hipLaunchKernelGGL((bm_off_reduce_kernel<1, true>), grid, dim3(256), 0, st, a, x, grad_y, part);
    hipLaunchKernelGGL((bm_off_final_kernel<true>), dim3((rows + 63) / 64), dim3(64), 0, st, a, part, stat, coef);
    if (v4) hipLaunchKernelGGL((bm_off_apply_kernel<4, true>), grid, dim3(256), 0, st, a, grad_y, x, coef, grad_x);
    else hipLaunchKernelGGL((bm_off_apply_kernel<1, true>), grid, dim3(256), 0, st, a, grad_y, x, coef, grad_x);
    return hipGetLastError() == hipSuccess ? 0 : -2;
  }
  const int nch = kind == K_CUM_LAYER ? 2 : 1;
  const bool v4 = T % 4 == 0 && aligned16(x) && aligned16(grad_y) && aligned16(grad_x);
  const int U = v4 ? T / 4 : T;
  const dim3 grid(rows, (U + 63) / 64, a.FS);
  if (nch == 2) {
    if (v4) hipLaunchKernelGGL((bm_reduce_kernel<4, 2, true>), grid, dim3(256), 0, st, a, x, grad_y, part);
    else hipLaunchKernelGGL((bm_reduce_kernel<1, 2, true>), grid, dim3(256), 0, st, a, x, grad_y, part);
  } else {
    if (v4) hipLaunchKernelGGL((bm_reduce_kernel<4, 1, true>), grid, dim3(256), 0, st, a, x, grad_y, part);
    else hipLaunchKernelGGL((bm_reduce_kernel<1, 1, true>), grid, dim3(256), 0, st, a, x, grad_y, part);
  }
  hipLaunchKernelGGL(bm_scan_bwd_kernel, dim3(rows), dim3(kChunk), 0, st, a, part, stat, coef);
  if (v4) hipLaunchKernelGGL((bm_apply_kernel<4, true>), grid, dim3(256), 0, st, a, grad_y, x, coef, grad_x);
  else hipLaunchKernelGGL((bm_apply_kernel<1, true>), grid, dim3(256), 0, st, a, grad_y, x, coef, grad_x);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

static int unfold_grid(int64_t total) {
  const int64_t n = (total + 255) / 256;
  return (int)(n < 1 ? 1 : (n > 16384 ? 16384 : n));
}
int32_t sefd_unfold_forward(const float* x, int32_t B, int32_t C, int32_t F, int32_t T, int32_t n, float* out, void* stream) {
  if (!x || !out || B < 1 || C < 1 || F < 1 || T < 1 || n < 0 || n >= F) return -1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool v4 = T % 4 == 0 && aligned16(x) && aligned16(out);
  const int64_t total = (int64_t)B * F * C * (2 * n + 1) * (v4 ? T / 4 : T);
  if (v4) hipLaunchKernelGGL((bm_unfold_fwd_kernel<4>), dim3(unfold_grid(total)), dim3(256), 0, st, x, B, C, F, T, n, out);
  else hipLaunchKernelGGL((bm_unfold_fwd_kernel<1>), dim3(unfold_grid(total)), dim3(256), 0, st, x, B, C, F, T, n, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
int32_t sefd_unfold_backward(const float* grad_out, int32_t B, int32_t C, int32_t F, int32_t T, int32_t n, float* grad_x, void* stream) {
  if (!grad_out || !grad_x || B < 1 || C < 1 || F < 1 || T < 1 || n < 0 || n >= F) return -1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool v4 = T % 4 == 0 && aligned16(grad_out) && aligned16(grad_x);
  const int64_t total = (int64_t)B * C * F * (v4 ? T / 4 : T);
  if (v4) hipLaunchKernelGGL((bm_unfold_bwd_kernel<4>), dim3(unfold_grid(total)), dim3(256), 0, st, grad_out, B, C, F, T, n, grad_x);
  else hipLaunchKernelGGL((bm_unfold_bwd_kernel<1>), dim3(unfold_grid(total)), dim3(256), 0, st, grad_out, B, C, F, T, n, grad_x);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
}  // extern "C"
