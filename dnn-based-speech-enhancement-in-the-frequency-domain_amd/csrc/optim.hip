// Grouped optimizer step on the flat fp32 buffers (include/sefd.h, "Grouped optimizer step"): Adam / AdamW with L2 or decoupled weight decay,
// amsgrad, up to 8 parameter groups, frozen parameters and global-norm clipping.
//   sefd_grad_norm   two launches: fp64 partial sums of squares per workgroup, then one workgroup adds them in index order -> { norm, coef }
//   sefd_optim_step  one launch over the chunk table; reads grad, never writes it (the clip is the factor coef)
// Both are streaming kernels: one workgroup of 256 threads per chunk of at most SEFD_OPTIM_CHUNK = 4 * 256 elements, one float4 per thread and
// buffer where the chunk sits on 16-byte lines, single floats in front of the first line and behind the last whole one.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include "../../include/sefd.h"

namespace {
constexpr int kChunk = SEFD_OPTIM_CHUNK;
static_assert(kChunk == 4 * 256, "one float4 per thread of a 256-thread workgroup");
// Workgroups of one sefd_optim_step launch.  Measured (tools/optim_bench.py, 3.7 M and 5.6 M elements): a workgroup per chunk is fastest - with 1024
// or 2048 workgroups walking the table, or with 2048- / 4096-element chunks, the same update takes 7 % to 24 % longer.  Past this many chunks
// (8.4 M elements in full chunks) the grid-stride loop takes over.
constexpr int kMaxGrid = 8192;
constexpr int kNormGrid = 1024;                      // partial sums of sefd_grad_norm: more of them only lengthen the finalize

struct GroupK {                                      // what the kernel needs of a sefd_optim_group, formed on the host in double
  float step_size, bc2_sqrt, b1, b2, eps, wd, lrwd;  // lr / bc1, sqrt(bc2), ..., lr * wd (decoupled)
  uint32_t flags;
};
struct GroupsK { GroupK g[SEFD_OPTIM_MAX_GROUPS]; };

// The split of a chunk that starts at address `a`: [0, head) single floats, nvec float4 from head on, the rest single floats again.
__device__ __forceinline__ void split_chunk(const void* a, int count, int vec_ok, int& head, int& nvec) {
  head = vec_ok ? (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(a) & 15u)) & 15u) >> 2 : count;
  if (head > count) head = count;
  nvec = (count - head) >> 2;
}
__device__ __forceinline__ bool chunk_ok(const sefd_optim_chunk& ch, int64_t n) {
  return ch.begin >= 0 && ch.count >= 1 && ch.count <= kChunk && ch.begin <= n - ch.count;
}

// Sum over the 256 threads in a fixed order (xor butterfly inside each wave, then the four waves in index order); the result is valid in thread 0.
__device__ __forceinline__ double block_sum(double x) {
  __shared__ double sh[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* g, int64_t n, const sefd_optim_chunk* table, int64_t nchunks, int vec_ok,
                                                           double* part) {
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    int64_t begin;
    int count;
    if (table) {
      const sefd_optim_chunk ch = table[c];
      if (!chunk_ok(ch, n)) continue;
      begin = ch.begin; count = ch.count;
    } else {
      begin = c * kChunk;
      count = (int)(n - begin < kChunk ? n - begin : kChunk);
    }
    const float* q = g + begin;
    int head, nvec;
    split_chunk(q, count, vec_ok, head, nvec);
    if (t < nvec) {
      const float4 x = *reinterpret_cast<const float4*>(q + head + 4 * t);
      acc += (double)x.x * (double)x.x;
      acc += (double)x.y * (double)x.y;
      acc += (double)x.z * (double)x.z;
      acc += (double)x.w * (double)x.w;
    }
    const int tail0 = head + 4 * nvec, ns = head + (count - tail0);
    for (int k = t; k < ns; k += 256) {
      const double x = q[k < head ? k : tail0 + (k - head)];
      acc += x * x;
    }
  }
  const double s = block_sum(acc);
  if (t == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void norm_finalize_kernel(const double* part, int nparts, float gscale, float max_norm, float* out) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += part[i];
  const double s = block_sum(acc);
  if (threadIdx.x == 0) {
    const double norm = fabs((double)gscale) * sqrt(s);
    const float nf = (float)norm;
    const double c = (double)max_norm / (norm + 1e-6);
    out[0] = nf;
    out[1] = (nf - nf == 0.f) ? (float)(c < 1.0 ? c : 1.0) : __builtin_nanf("");     // nf - nf: 0 for a finite norm, NaN for Inf and NaN
  }
}

__device__ __forceinline__ void update_one(float& p, float g, float& m, float& v, float& vm, const GroupK& h, float gs, float coef, bool ams) {
  float gi = g * gs * coef;
  if (h.wd != 0.f) {
    if (h.flags & SEFD_OPTIM_DECOUPLED) p = fmaf(-h.lrwd, p, p);     // p *= 1 - lr * wd in one rounding: the factor itself is no fp32 number
    else gi += h.wd * p;
  }
  const float mi = h.b1 * m + (1.f - h.b1) * gi;
  const float vi = h.b2 * v + (1.f - h.b2) * gi * gi;
  m = mi; v = vi;
  float d = vi;
  if (ams) { vm = fmaxf(vm, vi); d = vm; }
  p -= h.step_size * (mi / (sqrtf(d) / h.bc2_sqrt + h.eps));
}

__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   float* __restrict__ vmax, int64_t n, GroupsK hp, int ngroups,
                                                   const sefd_optim_chunk* __restrict__ table, int nchunks, int vec_ok, float gscale, const float* coef_p,
                                                   const int32_t* skip, const float* skip_nan) {
  // the three skips of a whole step, all before the first write (adam_kernel's two, and a clip coefficient that is NaN: a non-finite gradient norm)
  if (skip_nan) { const float q = *skip_nan; if (q != q) return; }
  if (skip && __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
  float coef = 1.f;
  if (coef_p) { coef = *coef_p; if (coef != coef) return; }
  const int t = threadIdx.x;
  sefd_optim_chunk next = table[blockIdx.x];                                       // grid <= nchunks
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const sefd_optim_chunk ch = next;
    if (c + (int)gridDim.x < nchunks) next = table[c + gridDim.x];                // the next descriptor travels under this chunk's loads
    if (!chunk_ok(ch, n) || ch.group < 0 || ch.group >= ngroups) continue;       // the host refused such a table already; never write outside [0, n)
    const GroupK h = hp.g[ch.group];
    const bool ams = (h.flags & SEFD_OPTIM_AMSGRAD) != 0 && vmax != nullptr;
    const int64_t b = ch.begin;
    int head, nvec;
    split_chunk(p + b, ch.count, vec_ok, head, nvec);
    if (t < nvec) {
      const int64_t i = b + head + 4 * t;
      float4 pi = *reinterpret_cast<const float4*>(p + i), mi = *reinterpret_cast<const float4*>(m + i), vi = *reinterpret_cast<const float4*>(v + i);
      const float4 gi = *reinterpret_cast<const float4*>(g + i);
      float4 xi = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ams) xi = *reinterpret_cast<const float4*>(vmax + i);
      update_one(pi.x, gi.x, mi.x, vi.x, xi.x, h, gscale, coef, ams);
      update_one(pi.y, gi.y, mi.y, vi.y, xi.y, h, gscale, coef, ams);
      update_one(pi.z, gi.z, mi.z, vi.z, xi.z, h, gscale, coef, ams);
      update_one(pi.w, gi.w, mi.w, vi.w, xi.w, h, gscale, coef, ams);
      *reinterpret_cast<float4*>(m + i) = mi;
      *reinterpret_cast<float4*>(v + i) = vi;
      if (ams) *reinterpret_cast<float4*>(vmax + i) = xi;
      *reinterpret_cast<float4*>(p + i) = pi;
    }
    const int tail0 = head + 4 * nvec, ns = head + (ch.count - tail0);
    for (int k = t; k < ns; k += 256) {
      const int64_t i = b + (k < head ? k : tail0 + (k - head));
      float pi = p[i], mi = m[i], vi = v[i], xi = ams ? vmax[i] : 0.f;
      update_one(pi, g[i], mi, vi, xi, h, gscale, coef, ams);
      m[i] = mi; v[i] = vi;
      if (ams) vmax[i] = xi;
      p[i] = pi;
    }
  }
}

// Host check of the table the kernels are about to walk: every chunk inside [0, n), its length within the chunk size, its group known.
bool table_ok(const sefd_optim_chunk* tab, int32_t nchunks, int64_t n, int32_t ngroups) {
  for (int32_t c = 0; c < nchunks; ++c) {
    const sefd_optim_chunk& ch = tab[c];
    if (ch.begin < 0 || ch.count < 1 || ch.count > kChunk || ch.begin > n - ch.count) return false;
    if (ngroups > 0 && (ch.group < 0 || ch.group >= ngroups)) return false;
  }
  return true;
}
int alike16(std::initializer_list<const void*> ps) {
  uintptr_t first = 0;
  bool have = false;
  for (const void* q : ps) {
    if (!q) continue;
    const uintptr_t a = reinterpret_cast<uintptr_t>(q) & 15u;
    if (a & 3u) return -1;                            // not even a float boundary
    if (!have) { first = a; have = true; }
    else if (a != first) return 0;
  }
  return 1;
}
// Workgroups for `work` chunks: all of them up to kMaxGrid, beyond that the smallest grid that needs no more trips through the grid-stride loop
// than kMaxGrid would - every workgroup then makes the same number of trips (the last few one fewer), and none idles through a ragged last one.
int even_grid(int64_t work) {
  if (work <= kMaxGrid) return (int)work;
  const int64_t trips = (work + kMaxGrid - 1) / kMaxGrid;
  return (int)((work + trips - 1) / trips);
}
int64_t norm_blocks(int64_t n) {
  const int64_t b = (n + kChunk - 1) / kChunk;
  return b < 1 ? 1 : (b < kNormGrid ? b : kNormGrid);
}
}  // namespace

extern "C" {
int64_t sefd_grad_norm_ws_floats(int64_t n) { return 2 * norm_blocks(n); }

int32_t sefd_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, const sefd_optim_chunk* table_host,
                       const sefd_optim_chunk* table_dev, int32_t nchunks, float* ws, float* out, void* stream) {
  if (!grad || !ws || !out || n < 1 || !(max_norm >= 0.f) || (table_host == nullptr) != (table_dev == nullptr)) return -1;
  if ((reinterpret_cast<uintptr_t>(ws) & 7u) || (reinterpret_cast<uintptr_t>(grad) & 3u) || (reinterpret_cast<uintptr_t>(out) & 3u)) return -1;
  if (table_host && (nchunks < 1 || !table_ok(table_host, nchunks, n, 0))) return -1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t work = table_host ? (int64_t)nchunks : (n + kChunk - 1) / kChunk;
  const int64_t cap = norm_blocks(n);
  const int grid = (int)(work < cap ? work : cap);
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(grid), dim3(256), 0, st, grad, n, table_dev, work, 1, part);
  hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(256), 0, st, part, grid, grad_scale, max_norm, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int32_t sefd_optim_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n, int32_t step,
                        const sefd_optim_group* groups, int32_t ngroups, const sefd_optim_chunk* table_host, const sefd_optim_chunk* table_dev,
                        int32_t nchunks, float grad_scale, const float* coef, const int32_t* skip_if_set, const float* skip_if_nan, void* stream) {
  if (n < 1 || step < 1 || ngroups < 1 || ngroups > SEFD_OPTIM_MAX_GROUPS || !param || !grad || !exp_avg || !exp_avg_sq || !groups || !table_host ||
      !table_dev || nchunks < 1)
    return -1;
  const int vec_ok = alike16({param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq});
  if (vec_ok < 0 || !table_ok(table_host, nchunks, n, ngroups)) return -1;
  GroupsK hp = {};
  for (int32_t i = 0; i < ngroups; ++i) {
    const sefd_optim_group& s = groups[i];
    if ((s.flags & SEFD_OPTIM_AMSGRAD) && !max_exp_avg_sq) return -1;
    const double bc1 = 1.0 - std::pow((double)s.beta1, step), bc2 = 1.0 - std::pow((double)s.beta2, step);
    hp.g[i] = GroupK{(float)(s.lr / bc1), (float)std::sqrt(bc2), s.beta1, s.beta2, s.eps, s.weight_decay,
                     (float)((double)s.lr * (double)s.weight_decay), s.flags};
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int grid = even_grid(nchunks);
  hipLaunchKernelGGL(optim_kernel, dim3(grid), dim3(256), 0, st, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, hp, ngroups, table_dev, nchunks,
                     vec_ok, grad_scale, coef, skip_if_set, skip_if_nan);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
}  // extern "C"
