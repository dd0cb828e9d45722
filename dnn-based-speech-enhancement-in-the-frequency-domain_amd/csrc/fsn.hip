// FullSubNet glue kernels (reference models.py:626-672, tools_for_model.py:806-837, 997-1011): everything around the
// per-time-step LSTM GEMMs is HBM-bound element-wise / gather work on time-major tensors.
#include <hip/hip_runtime.h>
#include "sefd_desc.h"
#include "dev_common.h"

namespace sefd {

constexpr float kNormEps = 1.1920928955078125e-07f;    // EPSILON = np.finfo(np.float32).eps (tools_for_model.py: cumulative norms)

static inline int gridn(int64_t n, int cap = 16384) { int64_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > cap ? cap : g)); }
#define GSL(i, n) for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// ---------------------------------------------------------------------------------------------- LSTM cell (one time step)
// element offset of (row r, buffer k) and the gate-column helper for both layouts of LstmCell
struct CellAddr {
  int64_t o[5];
};
__device__ __forceinline__ CellAddr cell_addr(const LstmCell& d, int64_t r) {
  CellAddr a;
  if (d.G > 0) {
    const int g = (int)(r / d.Bg);
    const int64_t b = r - (int64_t)g * d.Bg;
#pragma unroll
    for (int k = 0; k < 5; ++k) a.o[k] = d.go[k][g] + b * d.rs[k];
  } else {
    a.o[0] = r * 4 * d.H; a.o[1] = r * d.H; a.o[2] = r * d.H; a.o[3] = r * d.H; a.o[4] = r * 4 * d.H;
  }
  return a;
}
__device__ __forceinline__ int cell_col(const LstmCell& d, int q, int j) { return d.unit_major ? gate_col(q, j) : q * d.H + j; }

__global__ __launch_bounds__(256) void cell_fwd_kernel(const LstmCell d, const ArenaBases ab) {
  float* g = reinterpret_cast<float*>(rp(ab, d.gates));
  const float* cp = d.first ? nullptr : reinterpret_cast<const float*>(rp(ab, d.c_prev));
  float* c = reinterpret_cast<float*>(rp(ab, d.c));
  char* h = rp(ab, d.h);
  const int H = d.H;
  GSL(i, d.rows * H) {
    const int64_t r = i / H;
    const int j = (int)(i - r * H);
    const CellAddr a = cell_addr(d, r);
    float* gr = g + a.o[0];
    const int ci = cell_col(d, 0, j), cf = cell_col(d, 1, j), cg = cell_col(d, 2, j), co = cell_col(d, 3, j);
    const float ig = sigmoidf_(gr[ci]), fg = sigmoidf_(gr[cf]), gg = tanhf_(gr[cg]), og = sigmoidf_(gr[co]);
    const float cn = fg * (cp ? cp[a.o[1] + j] : 0.f) + ig * gg;
    gr[ci] = ig; gr[cf] = fg; gr[cg] = gg; gr[co] = og;
    c[a.o[1] + j] = cn;
    st_elem(h, d.hdt, a.o[2] + j, og * tanhf_(cn));
  }
}

// GRU cell, one time step (LstmCell kind 1)
__global__ __launch_bounds__(256) void gru_fwd_kernel(const LstmCell d, const ArenaBases ab) {
  float* g = reinterpret_cast<float*>(rp(ab, d.gates));
  const float* gh = reinterpret_cast<const float*>(rp(ab, d.gh));
  const char* hp = d.first ? nullptr : rp(ab, d.c_prev);
  char* h = rp(ab, d.h);
  const int H = d.H;
  GSL(i, d.rows * H) {
    const int64_t r = i / H;
    const int j = (int)(i - r * H);
    float* gr = g + r * 4 * H;
    const float* hr = gh + r * 3 * H;
    const float rg = sigmoidf_(gr[j] + hr[j]), zg = sigmoidf_(gr[H + j] + hr[H + j]);
    const float hn = hr[2 * H + j];
    const float ng = tanhf_(gr[2 * H + j] + rg * hn);
    const float hprev = hp ? ld_elem(hp, d.hdt, r * H + j) : 0.f;
    gr[j] = rg; gr[H + j] = zg; gr[2 * H + j] = ng; gr[3 * H + j] = hn;
    st_elem(h, d.hdt, r * H + j, (1.f - zg) * ng + zg * hprev);
  }
}
__global__ __launch_bounds__(256) void gru_bwd_kernel(const LstmCell d, const ArenaBases ab) {
  const float* g = reinterpret_cast<const float*>(rp(ab, d.gates));
  const char* hp = d.c_prev.arena >= 0 ? rp(ab, d.c_prev) : nullptr;
  const float* dh = reinterpret_cast<const float*>(rp(ab, d.dh));
  float* dhp = d.dc.arena >= 0 ? reinterpret_cast<float*>(rp(ab, d.dc)) : nullptr;
  char* dgi = rp(ab, d.dgates);
  char* dgh = rp(ab, d.gh);
  const int H = d.H;
  GSL(i, d.rows * H) {
    const int64_t r = i / H;
    const int j = (int)(i - r * H);
    const float* gr = g + r * 4 * H;
    const float rg = gr[j], zg = gr[H + j], ng = gr[2 * H + j], hn = gr[3 * H + j];
    const float hprev = hp ? ld_elem(hp, d.hdt, r * H + j) : 0.f;
    const float dht = dh[r * H + j];
    const float dn = dht * (1.f - zg) * (1.f - ng * ng);
    const float dz = dht * (hprev - ng) * zg * (1.f - zg);
    const float dr = dn * hn * rg * (1.f - rg);
    st_elem(dgi, d.gdt, r * 3 * H + j, dr); st_elem(dgi, d.gdt, r * 3 * H + H + j, dz); st_elem(dgi, d.gdt, r * 3 * H + 2 * H + j, dn);
    st_elem(dgh, d.gdt, r * 3 * H + j, dr); st_elem(dgh, d.gdt, r * 3 * H + H + j, dz); st_elem(dgh, d.gdt, r * 3 * H + 2 * H + j, dn * rg);
    if (dhp) dhp[r * H + j] += dht * zg;
  }
}

__global__ __launch_bounds__(256) void cell_bwd_kernel(const LstmCell d, const ArenaBases ab) {
  const float* g = reinterpret_cast<const float*>(rp(ab, d.gates));
  const float* cp = d.c_prev.arena >= 0 ? reinterpret_cast<const float*>(rp(ab, d.c_prev)) : nullptr;
  const float* c = reinterpret_cast<const float*>(rp(ab, d.c));
  const float* dh = reinterpret_cast<const float*>(rp(ab, d.dh));
  float* dc = reinterpret_cast<float*>(rp(ab, d.dc));
  char* dg = rp(ab, d.dgates);
  const int H = d.H;
  GSL(i, d.rows * H) {
    const int64_t r = i / H;
    const int j = (int)(i - r * H);
    const CellAddr a = cell_addr(d, r);
    const float* gr = g + a.o[0];
    const int ci = cell_col(d, 0, j), cf = cell_col(d, 1, j), cg = cell_col(d, 2, j), co = cell_col(d, 3, j);
    const float ig = gr[ci], fg = gr[cf], gg = gr[cg], og = gr[co];
    const float tc = tanhf_(c[a.o[1] + j]);
    const float dht = dh[a.o[3] + j];
    const float dcv = dht * og * (1.f - tc * tc) + (d.first ? 0.f : dc[i]);
    st_elem(dg, d.gdt, a.o[4] + ci, dcv * gg * ig * (1.f - ig));
    st_elem(dg, d.gdt, a.o[4] + cf, dcv * (cp ? cp[a.o[1] + j] : 0.f) * fg * (1.f - fg));
    st_elem(dg, d.gdt, a.o[4] + cg, dcv * ig * (1.f - gg * gg));
    st_elem(dg, d.gdt, a.o[4] + co, dht * tc * og * (1.f - og));
    dc[i] = dcv * fg;
  }
}

// ---------------------------------------------------------------------------------------------- dropout
__device__ __forceinline__ float keep_scale(const Dropout& d, const uint32_t* seed, int64_t i) { return drop_scale(seed[0], seed[1], d.layer, d.keep, i); }
__global__ __launch_bounds__(256) void dropout_kernel(const Dropout d, const ArenaBases ab) {   // forward and backward are the same map
  const char* x = rp(ab, d.x);
  char* y = rp(ab, d.y);
  const uint32_t* seed = reinterpret_cast<const uint32_t*>(rp(ab, d.seed));
  GSL(i, d.n) st_elem(y, d.dt, i, ld_elem(x, d.dt, i) * keep_scale(d, seed, i));
}

// ---------------------------------------------------------------------------------------------- input / normalisation
__global__ __launch_bounds__(256) void fsn_in_kernel(const Fsn d, const ArenaBases ab) {       // one workgroup per (b, f-chunk)
  const float* in = reinterpret_cast<const float*>(rp(ab, d.in));       // [B][F][T]
  float* mt = reinterpret_cast<float*>(rp(ab, d.out));                 // [TP][B][F]
  float* sums = reinterpret_cast<float*>(rp(ab, d.sums));              // [B][F]  partial sums (one per (b, f))
  const int b = blockIdx.y;
  for (int f = blockIdx.x; f < d.F; f += gridDim.x) {
    float s = 0.f;
    for (int t = threadIdx.x; t < d.TP; t += 256) {
      const float v = t < d.T ? in[((int64_t)b * d.F + f) * d.T + t] : 0.f;
      mt[((int64_t)t * d.B + b) * d.F + f] = v;
      s += v;
    }
    __shared__ float red[4];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[b * d.F + f] = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void fsn_scale_kernel(const Fsn d, const ArenaBases ab) {
  const float* mt = reinterpret_cast<const float*>(rp(ab, d.in));
  char* out = rp(ab, d.out);                                             // [TP][B][FP]
  const float* mu = reinterpret_cast<const float*>(rp(ab, d.sums));     // [B] means (finalised)
  GSL(i, (int64_t)d.TP * d.B * d.FP) {
    const int f = (int)(i % d.FP);
    const int64_t tb = i / d.FP;
    const int b = (int)(tb % d.B);
    float v = 0.f;
    if (f < d.F) {
      const float x = mt[tb * d.F + f];
      if (d.mode == 0) v = x / (mu[b] + 1e-5f);
      else {
        const float* stt = reinterpret_cast<const float*>(rp(ab, d.stat));
        if (d.mode == 2) v = (x - stt[b]) / (stt[d.B + b] + 1e-5f);
        else if (d.mode == 1) v = x / (stt[tb * 2] + kNormEps);
        else v = (x - stt[tb * 2]) / stt[tb * 2 + 1];
      }
    }
    st_elem(out, d.dt, i, v);
  }
}
// means: sums [B][nper] -> aux2[B] = sum / count
// one wave per batch item: lane l adds partials l, l + 64, ... in double, then a fixed-order butterfly (one thread per item walking the 257
// partials was a chain of 257 dependent loads: 60 us per launch, three launches per step on the critical path)
__global__ __launch_bounds__(64) void fsn_mean_kernel(const Fsn d, const ArenaBases ab, double count, int nper) {
  const float* sums = reinterpret_cast<const float*>(rp(ab, d.sums));
  float* mu = reinterpret_cast<float*>(rp(ab, d.aux2));
  const int b = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (int f = lane; f < nper; f += 64) s += sums[b * nper + f];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) mu[b] = (float)(s / count);
}

__device__ __forceinline__ int reflect_idx(int f, int F) { return f < 0 ? -f : (f >= F ? 2 * (F - 1) - f : f); }

// un-normalised sub-band input element (tools_for_model.py:806-837 + models.py:649-655), k < NB: neighbour f - n + k of the magnitude,
// k = NB + j: neighbour f - nf + j of the full-band output (nf = 0: the bin itself)
__device__ __forceinline__ float sb_raw(const Fsn& d, const float* mt, const float* fbo, int t, int b, int f, int k) {
  const int n = (d.NB - 1) / 2;
  if (k < d.NB) return mt[((int64_t)t * d.B + b) * d.F + reflect_idx(f - n + k, d.F)];
  return fbo[((int64_t)t * d.B + b) * d.FP + reflect_idx(f - (fsn_nfb(d) >> 1) + (k - d.NB), d.F)];
}
__global__ __launch_bounds__(256) void fsn_sbsum_kernel(const Fsn d, const ArenaBases ab) {    // grid (F, B): sums[b][f] over (k, t)
  const float* mt = reinterpret_cast<const float*>(rp(ab, d.in));
  const float* fbo = reinterpret_cast<const float*>(rp(ab, d.aux));
  float* sums = reinterpret_cast<float*>(rp(ab, d.sums));
  const int f = blockIdx.x, b = blockIdx.y, W = fsn_w(d);
  float s = 0.f;
  for (int i = threadIdx.x; i < d.TP * W; i += 256) s += sb_raw(d, mt, fbo, i / W, b, f, i % W);
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) sums[b * d.F + f] = red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void fsn_sbbuild_kernel(const Fsn d, const ArenaBases ab) {
  const float* mt = reinterpret_cast<const float*>(rp(ab, d.in));
  const float* fbo = reinterpret_cast<const float*>(rp(ab, d.aux));
  const float* mu = reinterpret_cast<const float*>(rp(ab, d.sums));
  char* out = rp(ab, d.out);                                            // [TP][B*F][WP], columns W..WP-1 zero
  const int W = fsn_w(d), WP = fsn_wp(d);
  if (d.mode == 0 && d.dt == DT_BF16 && (int64_t)d.TP * d.B * d.F * (WP / 8) < (1LL << 31) && !(W == WP && fsn_nfb(d) == 1)) {
    // any other width: the same 16-byte chunks over rows stored WP = roundup(W, 8) wide, the full-band window reflect-indexed, pad columns zero
    const unsigned CH = (unsigned)WP / 8, n8 = (unsigned)d.TP * d.B * d.F * CH;
    const int nn = (d.NB - 1) / 2, nf = fsn_nfb(d) >> 1;
    for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < n8; j += gridDim.x * 256u) {
      const unsigned c = j % CH, r = j / CH;
      const unsigned f = r % (unsigned)d.F, tb = r / (unsigned)d.F, b = tb % (unsigned)d.B;
      const float den = mu[b] + 1e-5f;
      const float* mrow = mt + (int64_t)tb * d.F;
      const float* frow = fbo + (int64_t)tb * d.FP;
      uint32_t pk[4];
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        float x[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int k = (int)(8 * c) + e + u;
          x[u] = k < d.NB ? mrow[reflect_idx((int)f - nn + k, d.F)] : k < W ? frow[reflect_idx((int)f - nf + (k - d.NB), d.F)] : 0.f;
        }
        pk[e >> 1] = (uint32_t)f2bf(x[0] / den) | ((uint32_t)f2bf(x[1] / den) << 16);
      }
      *reinterpret_cast<uint4*>(out + ((int64_t)r * WP + 8 * c) * 2) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    }
    return;
  }
  if (d.mode == 0 && d.dt == DT_BF16 && W == WP && (int64_t)d.TP * d.B * d.F * (W / 8) < (1LL << 31)) {
    // the default norm in bf16 plans (round 6): a thread forms 8 consecutive features of a row and stores them as ONE 16-byte chunk, its index split with
    // 32-bit divisions once per chunk (one thread per element: four 64-bit divisions and a 2-byte store each - 250 us for 203 MB at B = 64; same values)
    const unsigned CH = (unsigned)W / 8, n8 = (unsigned)d.TP * d.B * d.F * CH;
    const int nn = (d.NB - 1) / 2;
    for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < n8; j += gridDim.x * 256u) {
      const unsigned c = j % CH, r = j / CH;
      const unsigned f = r % (unsigned)d.F, tb = r / (unsigned)d.F, b = tb % (unsigned)d.B;
      const float den = mu[b] + 1e-5f;
      const float* mrow = mt + (int64_t)tb * d.F;
      uint32_t pk[4];
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        float x[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int k = (int)(8 * c) + e + u;
          x[u] = k < d.NB ? mrow[reflect_idx((int)f - nn + k, d.F)] : fbo[(int64_t)tb * d.FP + f];
        }
        pk[e >> 1] = (uint32_t)f2bf(x[0] / den) | ((uint32_t)f2bf(x[1] / den) << 16);
      }
      *reinterpret_cast<uint4*>(out + ((int64_t)r * W + 8 * c) * 2) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    }
    return;
  }
  GSL(i, (int64_t)d.TP * d.B * d.F * WP) {
    const int k = (int)(i % WP);
    const int64_t r = i / WP;
    if (k >= W) { st_elem(out, d.dt, i, 0.f); continue; }
    const int f = (int)(r % d.F);
    const int64_t tb = r / d.F;
    const int b = (int)(tb % d.B), t = (int)(tb / d.B);
    const float x = sb_raw(d, mt, fbo, t, b, f, k);
    float v;
    if (d.mode == 0) v = x / (mu[b] + 1e-5f);
    else {
      const float* stt = reinterpret_cast<const float*>(rp(ab, d.stat));
      if (d.mode == 2) v = (x - stt[b]) / (stt[d.B + b] + 1e-5f);
      else if (d.mode == 1) v = x / (stt[r * 2] + kNormEps);
      else v = (x - stt[r * 2]) / stt[r * 2 + 1];
    }
    st_elem(out, d.dt, i, v);
  }
}
// output activation of a SequenceModel head (tools_for_model.py:766-775, 792-793) and its derivative at the pre-activation x; fp32
__device__ __forceinline__ float head_act(int act, float x) {
  return act == 1 ? fmaxf(x, 0.f) : act == 2 ? tanhf(x) : act == 3 ? fminf(fmaxf(x, 0.f), 6.f) : x;
}
__device__ __forceinline__ float head_act_grad(int act, float x, float g) {
  if (act == 1) return x > 0.f ? g : 0.f;
  if (act == 2) { const float y = tanhf(x); return g * (1.f - y * y); }
  if (act == 3) return (x > 0.f && x < 6.f) ? g : 0.f;
  return g;
}
__device__ __forceinline__ float head_act_grad_y(int act, float y, float g) {        // the same from the activation's OUTPUT y
  if (act == 1) return y > 0.f ? g : 0.f;
  if (act == 2) return g * (1.f - y * y);
  if (act == 3) return (y > 0.f && y < 6.f) ? g : 0.f;
  return g;
}
__global__ __launch_bounds__(256) void fsn_out_kernel(const Fsn d, const ArenaBases ab) {      // crm [B][F][T][2] <- act(sbo [TP][B*F][2])
  const float* sbo = reinterpret_cast<const float*>(rp(ab, d.in));
  float* crm = reinterpret_cast<float*>(rp(ab, d.out));
  const int act = fsn_sbact(d);
  GSL(i, (int64_t)d.B * d.F * d.T * 2) {
    const int cch = (int)(i & 1);
    const int64_t q = i >> 1;
    const int t = (int)(q % d.T);
    const int64_t bf = q / d.T;
    const float v = sbo[(((int64_t)(t + d.LA)) * d.B * d.F + bf) * 2 + cch];
    crm[i] = act ? head_act(act, v) : v;
  }
}
// in-place Tanh / ReLU6 on the full-band head's output [TP][B][FP] (act(0) = 0: the pad columns stay zero)
__global__ __launch_bounds__(256) void fsn_act_kernel(const Fsn d, const ArenaBases ab) {
  float* y = reinterpret_cast<float*>(rp(ab, d.out));
  GSL(i, (int64_t)d.TP * d.B * d.FP) y[i] = head_act(d.act, y[i]);
}
__global__ __launch_bounds__(256) void fsn_out_bwd_kernel(const Fsn d, const ArenaBases ab) {  // d_sbo [TP][B*F][2] (dtype dt) <- grad_crm
  const float* g = reinterpret_cast<const float*>(rp(ab, d.in));
  char* ds = rp(ab, d.out);
  const int act = fsn_sbact(d);
  const float* pre = act ? reinterpret_cast<const float*>(rp(ab, d.aux)) : nullptr;     // sbo, the head's pre-activation: same [TP][B*F][2] layout
  GSL(i, (int64_t)d.TP * d.B * d.F * 2) {
    const int cch = (int)(i & 1);
    const int64_t q = i >> 1;
    const int64_t bf = q % ((int64_t)d.B * d.F);
    const int t = (int)(q / ((int64_t)d.B * d.F));
    float v = t >= d.LA ? g[(bf * d.T + (t - d.LA)) * 2 + cch] : 0.f;
    if (act && t >= d.LA) v = head_act_grad(act, pre[i], v);
    st_elem(ds, d.dt, i, v);
  }
}
// S[b][f] = sum_{k,t} d_sbin * sbin   (in = d_sbin fp32 [TP][B*F][W], aux = sbin dtype dt)
__global__ __launch_bounds__(256) void fsn_sbbwd_sum_kernel(const Fsn d, const ArenaBases ab) {
  const float* dsb = reinterpret_cast<const float*>(rp(ab, d.in));
  const char* sb = rp(ab, d.aux);
  float* sums = reinterpret_cast<float*>(rp(ab, d.sums));
  const int f = blockIdx.x, b = blockIdx.y, W = fsn_w(d), WP = fsn_wp(d);
  float s = 0.f;
  for (int i = threadIdx.x; i < d.TP * W; i += 256) {
    const int t = i / W, k = i % W;
    const int64_t o = (((int64_t)t * d.B + b) * d.F + f) * WP + k;
    s += dsb[o] * ld_elem(sb, d.dt, o);
  }
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) sums[b * d.F + f] = red[0] + red[1] + red[2] + red[3];
}
// d_fb_pre [TP][B][FP] (dtype dt) = relu'(fbo) * ( d_sbin[..][NB] / (mu+eps) - S_b / (N (mu+eps)) )     aux = fbo, aux2 = mu_sb, sums = S_b (mean form)
__global__ __launch_bounds__(256) void fsn_sbbwd_apply_kernel(const Fsn d, const ArenaBases ab) {
  const float* dsb = reinterpret_cast<const float*>(rp(ab, d.in));
  const float* fbo = reinterpret_cast<const float*>(rp(ab, d.aux));
  const float* mu = reinterpret_cast<const float*>(rp(ab, d.aux2));
  const float* Sm = reinterpret_cast<const float*>(rp(ab, d.sums));     // S_b / N  (finalised as a "mean")
  char* out = rp(ab, d.out);
  const int W = fsn_wp(d);
  GSL(i, (int64_t)d.TP * d.B * d.FP) {
    const int f = (int)(i % d.FP);
    const int64_t tb = i / d.FP;
    const int b = (int)(tb % d.B);
    float v = 0.f;
    if (f < d.F) {
      if (d.mode == 0) {
        const float den = mu[b] + 1e-5f;
        v = dsb[(tb * d.F + f) * W + d.NB] / den - Sm[b] / den;
      } else {
        v = dsb[tb * d.F + f];                                   // FSN_NORMBWD already went through the normalisation
      }
      const float y = fbo[i];
      if (d.act == 1) v = y > 0.f ? v : 0.f;                     // ReLU
      else if (d.act == 2) v *= (1.f - y * y);                   // Tanh
      else if (d.act == 3) v = (y > 0.f && y < 6.f) ? v : 0.f;   // ReLU6
    }
    st_elem(out, d.dt, i, v);
  }
}
// fb_num_neighbors > 0: the transpose of the reflect gather.  Column NB + j of sub-band row f holds fb_out[reflect(f - nf + j)], so the gradient of
// full-band bin g is the sum over the (f, j) with reflect(f - nf + j) == g: per j the regular source f = g + nf - j and, near the two edges, the
// mirrored ones (p = -g, p = 2 (F - 1) - g).  One workgroup per (t, b): the NFB gradient columns of its F rows go to LDS with consecutive lanes
// on consecutive addresses (runs of NFB floats; mode 0 reads them out of d_sb_in at stride WP, modes 1-3 from FSN_NORMBWD's dense [F][NFB]), then
// one thread per bin adds its sources in a fixed order (j ascending; regular, low mirror, high mirror): no atomics, bit-reproducible.
// mode 0 also applies the mean's term, once per source: d_fb[g] = (sum - cnt S_b / N) / (mu + eps).
__global__ __launch_bounds__(256) void fsn_sbbwd_gather_kernel(const Fsn d, const ArenaBases ab) {
  extern __shared__ float col[];                                          // [F][NFB]
  const float* src = reinterpret_cast<const float*>(rp(ab, d.in));
  const float* fbo = reinterpret_cast<const float*>(rp(ab, d.aux));
  char* out = rp(ab, d.out);
  const int NFB = fsn_nfb(d), nf = NFB >> 1, F = d.F;
  const int ld = d.mode == 0 ? fsn_wp(d) : NFB, c0 = d.mode == 0 ? d.NB : 0;
  const int64_t tb = blockIdx.x;
  const int b = (int)(tb % d.B);
  const float* rows = src + tb * F * ld + c0;
  for (int i = threadIdx.x; i < F * NFB; i += 256) {
    const int f = i / NFB, j = i - f * NFB;
    col[i] = rows[(int64_t)f * ld + j];
  }
  __syncthreads();
  for (int g = threadIdx.x; g < d.FP; g += 256) {
    float v = 0.f;
    if (g < F) {
      float s = 0.f;
      int cnt = 0;
      for (int j = 0; j < NFB; ++j) {
        const int o = nf - j;                                             // source row f = p + o for the un-reflected position p
        int f = g + o;
        if (f >= 0 && f < F) { s += col[f * NFB + j]; ++cnt; }
        f = o - g;
        if (g > 0 && f >= 0) { s += col[f * NFB + j]; ++cnt; }
        f = 2 * (F - 1) - g + o;
        if (g < F - 1 && f < F) { s += col[f * NFB + j]; ++cnt; }
      }
      if (d.mode == 0) {
        const float* mu = reinterpret_cast<const float*>(rp(ab, d.aux2));
        const float* Sm = reinterpret_cast<const float*>(rp(ab, d.sums));
        const float den = mu[b] + 1e-5f;
        v = s / den - (float)cnt * Sm[b] / den;
      } else {
        v = s;
      }
      v = head_act_grad_y(d.act, fbo[tb * d.FP + g], v);
    }
    st_elem(out, d.dt, tb * d.FP + g, v);
  }
}

// ---------------------------------------------------------------------------------------------- other norm_type choices
// block sum of doubles for 64- or 256-thread blocks (result valid in every thread)
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int nw = blockDim.x >> 6;
  if (nw == 1) return v;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0;
  for (int i = 0; i < nw; ++i) t += sh[i];
  return t;
}
// value j of frame t of row (b, f): src 0 -> mag_t[t][b][j] (f unused), src 1 -> the un-normalised sub-band input
__device__ __forceinline__ float norm_val(const Fsn& d, const float* mt, const float* fbo, int t, int b, int f, int j) {
  return d.src ? sb_raw(d, mt, fbo, t, b, f, j) : mt[((int64_t)t * d.B + b) * d.F + j];
}
// mode 2: one workgroup per utterance, (mean, unbiased std) over all its values (torch.mean / torch.std, tools_for_model.py:1047-1061)
__global__ __launch_bounds__(256) void fsn_normstat_utt_kernel(const Fsn d, const ArenaBases ab) {
  const float* mt = reinterpret_cast<const float*>(rp(ab, d.in));
  const float* fbo = d.src ? reinterpret_cast<const float*>(rp(ab, d.aux)) : nullptr;
  float* st = reinterpret_cast<float*>(rp(ab, d.stat));
  __shared__ double sh[4];
  const int b = blockIdx.x, W = d.src ? fsn_w(d) : d.F, nf = d.src ? d.F : 1;
  const int64_t n = (int64_t)d.TP * nf * W;
  double s = 0, q = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const int j = (int)(i % W);
    const int64_t r = i / W;
    const float x = norm_val(d, mt, fbo, (int)(r / nf), b, (int)(r % nf), j);
    s += x; q += (double)x * x;
  }
  s = block_sum(s, sh); q = block_sum(q, sh);
  if (threadIdx.x == 0) {
    const double mu = s / n, var = (q - n * mu * mu) / (n - 1);
    st[b] = (float)mu;
    st[d.B + b] = (float)sqrt(var > 0 ? var : 0.0);
  }
}
// modes 1 / 3: one workgroup per row (grid (F or 1, B)), frames in order: running mean and sqrt(running variance + eps) (:1014-1044, 1064-1104)
__global__ void fsn_normstat_cum_kernel(const Fsn d, const ArenaBases ab) {
  const float* mt = reinterpret_cast<const float*>(rp(ab, d.in));
  const float* fbo = d.src ? reinterpret_cast<const float*>(rp(ab, d.aux)) : nullptr;
  float* st = reinterpret_cast<float*>(rp(ab, d.stat));
  __shared__ double sh[4];
  const int f = blockIdx.x, b = blockIdx.y, W = d.src ? fsn_w(d) : d.F;
  const int64_t rows = d.src ? (int64_t)d.B * d.F : d.B, row = d.src ? (int64_t)b * d.F + f : b;
  double cs = 0, cq = 0;
  for (int t = 0; t < d.TP; ++t) {
    double s = 0, q = 0;
    for (int j = threadIdx.x; j < W; j += blockDim.x) { const float x = norm_val(d, mt, fbo, t, b, f, j); s += x; q += (double)x * x; }
    cs += block_sum(s, sh); cq += block_sum(q, sh);
    if (threadIdx.x == 0) {
      const double n = (double)W * (t + 1), m = cs / n;
      st[((int64_t)t * rows + row) * 2] = (float)m;
      st[((int64_t)t * rows + row) * 2 + 1] = d.mode == 3 ? (float)sqrt((cq - 2 * m * cs) / n + m * m + (double)kNormEps) : 0.f;
    }
  }
}
// backward of the sub-band normalisation w.r.t. its full-band column k = NB.  in = d_sbin fp32 [TP][B*F][W], aux2 = sb_in (dtype dt),
// aux = fbo (raw full-band output, fp32 [TP][B][FP]), stat as above, out = fp32 [TP][B][F].
// modes 1 / 3, one wave per row, frames last to first (suffix sums of the statistics' gradients):
//   cumulative_laplace : dx_t = g_t / (m_t + eps) - sum_{u >= t} S_u / ((m_u + eps) n_u)                          S_u = sum_k g y at frame u
//   cumulative_layer   : dx_t = g_t / sd_t - sum_{u >= t} [ G_u / (n_u sd_u) + (x_t - m_u) S_u / (n_u sd_u^2) ]   G_u = sum_k g
__global__ __launch_bounds__(64) void fsn_normbwd_cum_kernel(const Fsn d, const ArenaBases ab) {
  const float* dsb = reinterpret_cast<const float*>(rp(ab, d.in));
  const char* sb = rp(ab, d.aux2);
  const float* fbo = reinterpret_cast<const float*>(rp(ab, d.aux));
  const float* st = reinterpret_cast<const float*>(rp(ab, d.stat));
  float* out = reinterpret_cast<float*>(rp(ab, d.out));
  const int f = blockIdx.x, b = blockIdx.y, W = fsn_w(d), WP = fsn_wp(d), NFB = fsn_nfb(d), k = threadIdx.x;
  const int64_t rows = (int64_t)d.B * d.F, row = (int64_t)b * d.F + f;
  const int fsrc = reflect_idx(f - (NFB >> 1) + k, d.F);          // lane k < NFB owns full-band column k: out [TP][B][F][NFB]
  double accA = 0, accB = 0, accBM = 0;
  for (int t = d.TP - 1; t >= 0; --t) {
    const int64_t o = ((int64_t)t * rows + row) * WP;
    const float g = k < W ? dsb[o + k] : 0.f, y = k < W ? ld_elem(sb, d.dt, o + k) : 0.f;
    double G = g, S = (double)g * y;
    if (k + 64 < W) { const float g2 = dsb[o + k + 64]; G += g2; S += (double)g2 * ld_elem(sb, d.dt, o + k + 64); }   // W <= 126
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) { G += __shfl_xor(G, sft); S += __shfl_xor(S, sft); }
    // G, S are the same in every lane after the butterfly: each lane keeps the row's suffix sums
    const double m = st[((int64_t)t * rows + row) * 2], sd = st[((int64_t)t * rows + row) * 2 + 1], n = (double)W * (t + 1);
    double v = 0;
    if (d.mode == 1) {
      const double den = m + (double)kNormEps;
      accA += S / (den * n);
      if (k < NFB) v = (double)dsb[o + d.NB + k] / den - accA;
    } else {
      const double bb = S / (n * sd * sd);
      accA += G / (n * sd); accB += bb; accBM += bb * m;
      if (k < NFB) v = (double)dsb[o + d.NB + k] / sd - accA - (double)fbo[((int64_t)t * d.B + b) * d.FP + fsrc] * accB + accBM;
    }
    if (k < NFB) out[(((int64_t)t * d.B + b) * d.F + f) * NFB + k] = (float)v;
  }
}
// mode 2 (offline_gaussian_norm): dx = (g - G_b / N) / (sd_b + 1e-5) - y S_b / ((N - 1) sd_b);  sums[2][B][F] partial (S, G) per (b, f)
__global__ __launch_bounds__(256) void fsn_normbwd_utt_part_kernel(const Fsn d, const ArenaBases ab) {
  const float* dsb = reinterpret_cast<const float*>(rp(ab, d.in));
  const char* sb = rp(ab, d.aux2);
  float* part = reinterpret_cast<float*>(rp(ab, d.sums));
  __shared__ double sh[4];
  const int f = blockIdx.x, b = blockIdx.y, W = fsn_w(d), WP = fsn_wp(d);
  double S = 0, G = 0;
  for (int i = threadIdx.x; i < d.TP * W; i += 256) {
    const int64_t o = (((int64_t)(i / W) * d.B + b) * d.F + f) * WP + i % W;
    const float g = dsb[o];
    G += g; S += (double)g * ld_elem(sb, d.dt, o);
  }
  S = block_sum(S, sh); G = block_sum(G, sh);
  if (threadIdx.x == 0) { part[b * d.F + f] = (float)S; part[(d.B + b) * d.F + f] = (float)G; }
}
__global__ __launch_bounds__(256) void fsn_normbwd_utt_kernel(const Fsn d, const ArenaBases ab) {
  const float* dsb = reinterpret_cast<const float*>(rp(ab, d.in));
  const char* sb = rp(ab, d.aux2);
  const float* part = reinterpret_cast<const float*>(rp(ab, d.sums));
  const float* st = reinterpret_cast<const float*>(rp(ab, d.stat));
  float* out = reinterpret_cast<float*>(rp(ab, d.out));
  __shared__ double tot[2];
  const int b = blockIdx.y, W = fsn_w(d), WP = fsn_wp(d), NFB = fsn_nfb(d);
  if (threadIdx.x < 2) {                                        // serial sum of F partials: deterministic, tiny
    double s = 0;
    for (int f = 0; f < d.F; ++f) s += part[(threadIdx.x * d.B + b) * d.F + f];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
  const double N = (double)d.F * W * d.TP, sdv = st[d.B + b], sden = sdv + 1e-5;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < (int64_t)d.TP * d.F * NFB; i += (int64_t)gridDim.x * 256) {   // out [TP][B][F][NFB]
    const int j = (int)(i % NFB);
    const int f = (int)((i / NFB) % d.F), t = (int)(i / ((int64_t)NFB * d.F));
    const int64_t o = (((int64_t)t * d.B + b) * d.F + f) * WP + d.NB + j;
    out[(((int64_t)t * d.B + b) * d.F + f) * NFB + j] = (float)((dsb[o] - tot[1] / N) / sden - (double)ld_elem(sb, d.dt, o) * tot[0] / ((N - 1) * sdv));
  }
}

__global__ __launch_bounds__(256) void reflectpad_kernel(const ReflectPad d, const ArenaBases ab) {
  const float* src = reinterpret_cast<const float*>(rp(ab, d.src));
  float* dst = reinterpret_cast<float*>(rp(ab, d.dst));
  const int Lp = d.L + 2 * d.pad;
  GSL(i, (int64_t)d.B * Lp) {
    const int64_t b = i / Lp;
    int j = (int)(i - b * Lp) - d.pad;
    j = j < 0 ? -j : (j >= d.L ? 2 * (d.L - 1) - j : j);
    dst[i] = src[b * d.L + j];
  }
}

void launch_fsn(const Op& op, const ArenaBases& ab, hipStream_t st) {
  switch (op.kind) {
    case OP_STFT_FFT: launch_stft_fft(op.fft, ab, st); break;
    case OP_ISTFT_FFT: launch_istft_fft(op.ifft, ab, st); break;
    case OP_IFFT_OLA: launch_ifft_ola(op.iola, ab, st); break;
    case OP_OLA_FOLD: launch_ola_fold(op.ola, ab, st); break;
    case OP_SPECOUT_ADJ: launch_specout_adj(op.so, ab, st); break;
    case OP_REFLECTPAD: hipLaunchKernelGGL(reflectpad_kernel, dim3(gridn((int64_t)op.rpad.B * (op.rpad.L + 2 * op.rpad.pad))), dim3(256), 0, st, op.rpad, ab); break;
    case OP_CELL_FWD:
      if (op.cell.kind == 1) hipLaunchKernelGGL(gru_fwd_kernel, dim3(gridn(op.cell.rows * op.cell.H)), dim3(256), 0, st, op.cell, ab);
      else hipLaunchKernelGGL(cell_fwd_kernel, dim3(gridn(op.cell.rows * op.cell.H)), dim3(256), 0, st, op.cell, ab);
      break;
    case OP_CELL_BWD:
      if (op.cell.kind == 1) hipLaunchKernelGGL(gru_bwd_kernel, dim3(gridn(op.cell.rows * op.cell.H)), dim3(256), 0, st, op.cell, ab);
      else hipLaunchKernelGGL(cell_bwd_kernel, dim3(gridn(op.cell.rows * op.cell.H)), dim3(256), 0, st, op.cell, ab);
      break;
    case OP_DROPOUT_FWD:
    case OP_DROPOUT_BWD: hipLaunchKernelGGL(dropout_kernel, dim3(gridn(op.drop.n)), dim3(256), 0, st, op.drop, ab); break;
    case OP_FSN_IN: {
      const Fsn& d = op.fsn;
      hipLaunchKernelGGL(fsn_in_kernel, dim3(d.F, d.B), dim3(256), 0, st, d, ab);
      hipLaunchKernelGGL(fsn_mean_kernel, dim3(d.B), dim3(64), 0, st, d, ab, (double)d.F * d.TP, d.F);
      break;
    }
    case OP_FSN_SCALE: hipLaunchKernelGGL(fsn_scale_kernel, dim3(gridn((int64_t)op.fsn.TP * op.fsn.B * op.fsn.FP)), dim3(256), 0, st, op.fsn, ab); break;
    case OP_FSN_SBSUM: {
      const Fsn& d = op.fsn;
      hipLaunchKernelGGL(fsn_sbsum_kernel, dim3(d.F, d.B), dim3(256), 0, st, d, ab);
      hipLaunchKernelGGL(fsn_mean_kernel, dim3(d.B), dim3(64), 0, st, d, ab, (double)d.F * d.TP * fsn_w(d), d.F);
      break;
    }
    case OP_FSN_SBBUILD: hipLaunchKernelGGL(fsn_sbbuild_kernel, dim3(gridn((int64_t)op.fsn.TP * op.fsn.B * op.fsn.F * fsn_wp(op.fsn))), dim3(256), 0, st, op.fsn, ab); break;
    case OP_FSN_OUT: hipLaunchKernelGGL(fsn_out_kernel, dim3(gridn((int64_t)op.fsn.B * op.fsn.F * op.fsn.T * 2)), dim3(256), 0, st, op.fsn, ab); break;
    case OP_FSN_OUT_BWD: hipLaunchKernelGGL(fsn_out_bwd_kernel, dim3(gridn((int64_t)op.fsn.TP * op.fsn.B * op.fsn.F * 2)), dim3(256), 0, st, op.fsn, ab); break;
    case OP_FSN_SBBWD_SUM: {
      const Fsn& d = op.fsn;
      hipLaunchKernelGGL(fsn_sbbwd_sum_kernel, dim3(d.F, d.B), dim3(256), 0, st, d, ab);
      hipLaunchKernelGGL(fsn_mean_kernel, dim3(d.B), dim3(64), 0, st, d, ab, (double)d.F * d.TP * fsn_w(d), d.F);
      break;
    }
    case OP_FSN_NORMSTAT: {
      const Fsn& d = op.fsn;
      if (d.mode == 2) hipLaunchKernelGGL(fsn_normstat_utt_kernel, dim3(d.B), dim3(256), 0, st, d, ab);
      else if (d.src) hipLaunchKernelGGL(fsn_normstat_cum_kernel, dim3(d.F, d.B), dim3(64), 0, st, d, ab);
      else hipLaunchKernelGGL(fsn_normstat_cum_kernel, dim3(1, d.B), dim3(256), 0, st, d, ab);
      break;
    }
    case OP_FSN_NORMBWD: {
      const Fsn& d = op.fsn;
      if (d.mode == 2) {
        hipLaunchKernelGGL(fsn_normbwd_utt_part_kernel, dim3(d.F, d.B), dim3(256), 0, st, d, ab);
        hipLaunchKernelGGL(fsn_normbwd_utt_kernel, dim3(64, d.B), dim3(256), 0, st, d, ab);
      } else {
        hipLaunchKernelGGL(fsn_normbwd_cum_kernel, dim3(d.F, d.B), dim3(64), 0, st, d, ab);
      }
      break;
    }
    case OP_FSN_SBBWD_APPLY:
      if (fsn_nfb(op.fsn) > 1) hipLaunchKernelGGL(fsn_sbbwd_gather_kernel, dim3(op.fsn.TP * op.fsn.B), dim3(256), (size_t)op.fsn.F * fsn_nfb(op.fsn) * 4, st, op.fsn, ab);
      else hipLaunchKernelGGL(fsn_sbbwd_apply_kernel, dim3(gridn((int64_t)op.fsn.TP * op.fsn.B * op.fsn.FP)), dim3(256), 0, st, op.fsn, ab);
      break;
    case OP_FSN_ACT: hipLaunchKernelGGL(fsn_act_kernel, dim3(gridn((int64_t)op.fsn.TP * op.fsn.B * op.fsn.FP)), dim3(256), 0, st, op.fsn, ab); break;
    default: break;
  }
}

// ---------------------------------------------------------------------------------------------- training targets
// trainer.py:100-104: noisy_mag = |noisy| ; cIRM = compress(complex ratio mask)   (tools_for_model.py:683-717), interleaved complex in.
__global__ __launch_bounds__(256) void fsn_targets_kernel(const float* noisy, const float* clean, int64_t n, float* mag, float* phase, float* cirm) {
  GSL(i, n) {
    const float nr = noisy[2 * i], ni = noisy[2 * i + 1];
    if (mag) mag[i] = sqrtf(nr * nr + ni * ni);
    if (phase) phase[i] = atan2f(ni, nr);
    if (cirm) {
      const float cr = clean[2 * i], ci = clean[2 * i + 1];
      const float den = nr * nr + ni * ni + 1.1920929e-07f;          // np.finfo(np.float32).eps
      float m[2] = {(nr * cr + ni * ci) / den, (nr * ci - ni * cr) / den};
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float v = m[e] <= -100.f ? -100.f : m[e];
        const float ex = expf(-0.1f * v);
        cirm[2 * i + e] = 10.f * (1.f - ex) / (1.f + ex);
      }
    }
  }
}

// Backward of fsn_targets_kernel: one pass over the interleaved complex inputs; the gradient of noisy and / or clean (whichever pointer is given),
// each element written once.  Cotangents that are null count as zero.
//   mag, phase:  d re = g_m re / m - g_p (im / m) / m,  d im = g_m im / m + g_p (re / m) / m;  m == 0: both 0 (torch: NaN) - ConvSTFT's rule
//   cIRM: h_e = g_e f'(v_e), f'(v) = K C 2 e^{-Cv} / (1 + e^{-Cv})^2 (0 on the clamped arm v <= -100), v = (a, b) / den, a = nr cr + ni ci, b = nr ci - ni cr:
//     d cr = (h_0 nr - h_1 ni) / den, d ci = (h_0 ni + h_1 nr) / den,
//     d nr = (h_0 cr + h_1 ci) / den - 2 nr (h_0 v_0 + h_1 v_1) / den,  d ni = (h_0 ci - h_1 cr) / den - 2 ni (h_0 v_0 + h_1 v_1) / den
__global__ __launch_bounds__(256) void fsn_targets_bwd_kernel(const float* noisy, const float* clean, int64_t n, const float* g_mag, const float* g_phase,
                                                              const float* g_cirm, float* d_noisy, float* d_clean) {
  GSL(i, n) {
    const float nr = noisy[2 * i], ni = noisy[2 * i + 1];
    float dr = 0.f, di = 0.f;
    if (g_mag || g_phase) {
      const float m = sqrtf(nr * nr + ni * ni);
      if (m != 0.f) {
        const float gm = g_mag ? g_mag[i] : 0.f, gp = g_phase ? g_phase[i] : 0.f;
        dr = gm * nr / m - gp * (ni / m) / m;
        di = gm * ni / m + gp * (nr / m) / m;
      }
    }
    if (g_cirm) {
      const float cr = clean[2 * i], ci = clean[2 * i + 1];
      const float den = nr * nr + ni * ni + 1.1920929e-07f;          // np.finfo(np.float32).eps
      const float v[2] = {(nr * cr + ni * ci) / den, (nr * ci - ni * cr) / den};
      float h[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float ex = expf(-0.1f * v[e]), q = 1.f + ex;
        h[e] = v[e] <= -100.f ? 0.f : g_cirm[2 * i + e] * (2.f * ex / (q * q));       // K C = 1
      }
      if (d_clean) {
        d_clean[2 * i] = (h[0] * nr - h[1] * ni) / den;
        d_clean[2 * i + 1] = (h[0] * ni + h[1] * nr) / den;
      }
      const float hv = 2.f * (h[0] * v[0] + h[1] * v[1]);
      dr += (h[0] * cr + h[1] * ci - nr * hv) / den;
      di += (h[0] * ci - h[1] * cr - ni * hv) / den;
    }
    if (d_noisy) { d_noisy[2 * i] = dr; d_noisy[2 * i + 1] = di; }
  }
}

}  // namespace sefd

extern "C" int32_t sefd_fsn_targets_backward(const float* noisy_c64, const float* clean_c64, int64_t n, const float* g_mag, const float* g_phase, const float* g_cirm,
                                             float* d_noisy, float* d_clean, void* stream) {
  using namespace sefd;
  if (!noisy_c64 || n < 0 || (g_cirm && !clean_c64) || (d_clean && !g_cirm) || (!d_noisy && !d_clean)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(fsn_targets_bwd_kernel, dim3(gridn(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), noisy_c64, clean_c64, n, g_mag, g_phase, g_cirm,
                     d_noisy, d_clean);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int32_t sefd_fsn_targets(const float* noisy_c64, const float* clean_c64, int64_t n, float* mag, float* phase, float* cirm, void* stream) {
  using namespace sefd;
  hipLaunchKernelGGL(fsn_targets_kernel, dim3(gridn(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), noisy_c64, clean_c64, n, mag, phase, cirm);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
