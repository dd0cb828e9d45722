// STOI (Taal et al., IEEE TASLP 2011, with the framing conventions of pystoi 0.3.3) of a batch of clean / estimated pairs on the device: the
// host scorer's stoi_one (csrc_host/scorers.cpp) restated stage by stage, its quirks included.  Inputs are fp32; everything after the load
// is fp64 (a measuring instrument: a few hundred MFLOP per batch).
//
//   resample   fs -> 10 kHz, resample_poly with the Kaiser-windowed sinc of csrc_host/stoi_tables.h: one thread per output sample sums its
//              polyphase taps in the host's order.  Skipped at fs == 10 kHz (the later stages then read the fp32 input).
//   energy     one wave per 256-sample Hann frame of the clean signal (hop 128, frames start while i < n - 256: strict, so a signal with
//              n - 256 a multiple of 128 loses its last frame): e = 20 log10(sqrt(sum (w x)^2) + eps).
//   select     one workgroup per utterance: the maximum e, keep a frame iff emax - 40 - e < 0, and the list of the kept frames in order
//              (ballot + popcount prefix counts, no atomics).  K kept frames.
//   bands      one wave per frame g < K - 1 of the compacted signal.  The compacted signal (overlap-add of the kept, windowed frames, length
//              (K - 1) 128 + 256) is not stored: sample t is the sum of at most two kept frames, t / 128 - 1 first, gathered where it is
//              needed.  Windowed again, zero-padded to 512, one radix-2 FFT per signal in LDS (not packed into one complex transform: a zero
//              signal must give exact zeros, as it does on the host), then sqrt of the |X|^2 sums over the bins of the 15 one-third octave bands.
//   correlate  one workgroup per utterance: per segment of 30 frames and band the norm-ratio scaling, the clip, mean removal and the
//              correlation; the J * 15 terms are summed in a fixed order (strided per thread, fixed shuffle tree).  Fewer than 30 frames: 1e-5.
//
// Frame counts are data dependent: grids are sized for "every frame kept" and read K from device memory; the host enqueues the five launches
// and the table copy on the caller's stream and never waits.  No floating-point atomics: results are bit-identical from run to run, and an
// utterance's score does not depend on the rest of its batch.
#include <hip/hip_runtime.h>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include "../../include/sefd.h"
#include "../csrc_host/stoi_tables.h"

namespace {
using namespace sefd_stoi;
constexpr int kHop = kFrame / 2;
constexpr int kMaxRatio = 1024;                     // largest up / down factor (after reduction) the resampler takes

struct StoiParams {
  int32_t L, resampled, up, down, pre, n_taps;
  int32_t nf, nfs;                                  // frames of the 10 kHz signal; row stride of the band envelopes (nf - 1)
  int64_t pre_remove, n;                            // n: samples per utterance at 10 kHz
  int32_t lo[kBands], hi[kBands];
  double clip;
  const double* win;                                // [256]
  const double2* tw;                                // [256]: exp(-2 pi i k / 512)
  const double* taps;                               // [n_taps], unit DC gain
  double* xr; double* yr;                           // [B][n] resampled clean / estimate
  double* e;                                        // [B][nf]
  int32_t* kept;                                    // [B][nf]: the kept frames, ascending
  int32_t* K;                                       // [B]
  double* xt; double* yt;                           // [B][15][nfs] band envelopes
};

// Host-side constants of one sample rate, built once and kept for the life of the process (so the asynchronous copy never outlives them).
struct Table {
  int n_taps = 0;
  std::vector<double> blob;                         // window [256], twiddles [256][2], taps [n_taps]
};

const Table* table_for(int fs) {
  static std::mutex mu;
  static std::map<int, std::unique_ptr<Table>> cache;
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find(fs);
  if (it != cache.end()) return it->second.get();
  auto t = std::make_unique<Table>();
  t->blob = hann_inner(kFrame);
  for (int k = 0; k < kNfft / 2; ++k) {
    t->blob.push_back(std::cos(2.0 * kPi * k / kNfft));
    t->blob.push_back(-std::sin(2.0 * kPi * k / kNfft));
  }
  if (fs != kFs) {
    const std::vector<double> h = resample_window(kFs, fs);
    t->n_taps = (int)h.size();
    t->blob.insert(t->blob.end(), h.begin(), h.end());
  }
  const Table* r = t.get();
  cache.emplace(fs, std::move(t));
  return r;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// fixed-order sum over the 256 threads of a workgroup; every thread gets the total
__device__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// sample i of utterance b at 10 kHz: the resampled signal, or the fp32 input itself at fs == 10 kHz
__device__ __forceinline__ double sample(const double* r, const float* in, const StoiParams& p, int b, int64_t i) {
  return p.resampled ? r[(int64_t)b * p.n + i] : (double)in[(int64_t)b * p.L + i];
}

__global__ __launch_bounds__(256) void stoi_resample_kernel(const float* __restrict__ clean, const float* __restrict__ est, const StoiParams p) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= p.n) return;
  const int b = blockIdx.y;
  const float* x = (blockIdx.z ? est : clean) + (int64_t)b * p.L;
  double* y = (blockIdx.z ? p.yr : p.xr) + (int64_t)b * p.n;
  // tap i = i0 - j up of source sample j, 0 <= i < n_taps, 0 <= j < L (scorers.cpp resample_poly)
  const int64_t i0 = (o + p.pre_remove) * p.down - p.pre;
  double acc = 0.0;
  if (i0 >= 0) {
    int64_t jhi = i0 / p.up;
    if (jhi > p.L - 1) jhi = p.L - 1;
    int64_t jlo = (i0 - (p.n_taps - 1) + p.up - 1) / p.up;
    if (jlo < 0) jlo = 0;
    for (int64_t j = jlo; j <= jhi; ++j) acc += p.taps[i0 - j * p.up] * (double)x[j];
  }
  y[o] = acc * p.up;
}

__global__ __launch_bounds__(64) void stoi_energy_kernel(const float* __restrict__ clean, const StoiParams p) {
  const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int64_t base = (int64_t)f * kHop;
  double s = 0.0;
  for (int j = lane; j < kFrame; j += 64) {
    const double v = p.win[j] * sample(p.xr, clean, p, b, base + j);
    s += v * v;
  }
  s = wave_sum(s);
  if (lane == 0) p.e[(int64_t)b * p.nf + f] = 20.0 * log10(sqrt(s) + kEps);
}

__global__ __launch_bounds__(256) void stoi_select_kernel(const StoiParams p) {
  __shared__ double shmax[4];
  __shared__ int wcnt[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nf = p.nf;
  const double* e = p.e + (int64_t)b * nf;
  int32_t* kept = p.kept + (int64_t)b * nf;
  double emax = -1e300;
  for (int f = tid; f < nf; f += 256) emax = fmax(emax, e[f]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) emax = fmax(emax, __shfl_xor(emax, o));
  if (lane == 0) shmax[w] = emax;
  __syncthreads();
  emax = fmax(fmax(shmax[0], shmax[1]), fmax(shmax[2], shmax[3]));
  int running = 0;
  for (int base = 0; base < nf; base += 256) {
    const int f = base + tid;
    const bool keep = f < nf && (emax - kDynRange - e[f] < 0);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wcnt[w] = __popcll(mask);
    __syncthreads();
    int off = running;
    for (int i = 0; i < w; ++i) off += wcnt[i];
    if (keep) kept[off + __popcll(mask & ((1ull << lane) - 1ull))] = f;
    running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  if (tid == 0) p.K[b] = running;
}

__global__ __launch_bounds__(64) void stoi_bands_kernel(const float* __restrict__ clean, const float* __restrict__ est, const StoiParams p) {
  __shared__ double2 zx[kNfft], zy[kNfft];
  const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int K = p.K[b];
  if (g >= K - 1) return;                           // the whole wave leaves: frames of the compacted signal start while i < (K - 1) 128
  const int32_t* kept = p.kept + (int64_t)b * p.nf;
  for (int j = lane; j < kNfft; j += 64) {
    double vx = 0.0, vy = 0.0;
    if (j < kFrame) {
      // compacted sample t = 128 g + j lies in the kept frames k - 1 (second half) and k (first half), k = t / 128; added in that order
      const int k = g + (j >> 7), jj = j & (kHop - 1);
      if (k >= 1) {
        const int64_t i = (int64_t)kept[k - 1] * kHop + jj + kHop;
        const double w = p.win[jj + kHop];
        vx += w * sample(p.xr, clean, p, b, i);
        vy += w * sample(p.yr, est, p, b, i);
      }
      if (k < K) {
        const int64_t i = (int64_t)kept[k] * kHop + jj;
        const double w = p.win[jj];
        vx += w * sample(p.xr, clean, p, b, i);
        vy += w * sample(p.yr, est, p, b, i);
      }
      vx *= p.win[j];
      vy *= p.win[j];
    }
    const int r = (int)(__builtin_bitreverse32((uint32_t)j) >> 23);          // 9 bits
    zx[r] = make_double2(vx, 0.0);
    zy[r] = make_double2(vy, 0.0);
  }
  __syncthreads();
  for (int h = 1; h < kNfft; h <<= 1) {
    const int stride = kNfft / 2 / h;
    for (int j = lane; j < kNfft / 2; j += 64) {
      const int pos = j & (h - 1), i0 = ((j - pos) << 1) + pos, i1 = i0 + h;
      const double2 w = p.tw[pos * stride];                                   // W_2h^pos = W_512^(pos 256 / h)
      const double2 ax = zx[i0], bx = zx[i1], ay = zy[i0], by = zy[i1];
      const double2 tx = make_double2(bx.x * w.x - bx.y * w.y, bx.x * w.y + bx.y * w.x);
      const double2 ty = make_double2(by.x * w.x - by.y * w.y, by.x * w.y + by.y * w.x);
      zx[i0] = make_double2(ax.x + tx.x, ax.y + tx.y);
      zx[i1] = make_double2(ax.x - tx.x, ax.y - tx.y);
      zy[i0] = make_double2(ay.x + ty.x, ay.y + ty.y);
      zy[i1] = make_double2(ay.x - ty.x, ay.y - ty.y);
    }
    __syncthreads();
  }
  if (lane < kBands) {
    double sx = 0.0, sy = 0.0;
    for (int k = p.lo[lane]; k < p.hi[lane]; ++k) {
      sx += zx[k].x * zx[k].x + zx[k].y * zx[k].y;
      sy += zy[k].x * zy[k].x + zy[k].y * zy[k].y;
    }
    const int64_t o = ((int64_t)b * kBands + lane) * p.nfs + g;
    p.xt[o] = sqrt(sx);
    p.yt[o] = sqrt(sy);
  }
}

__global__ __launch_bounds__(256) void stoi_correlate_kernel(const StoiParams p, double* __restrict__ out) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  const int nfr = p.nf > 0 ? p.K[b] - 1 : 0;       // frames of the compacted signal
  if (nfr < kSeg) {
    if (threadIdx.x == 0) out[b] = 1e-5;
    return;
  }
  const int J = nfr - kSeg + 1, terms = J * kBands;
  double acc = 0.0;
  for (int idx = threadIdx.x; idx < terms; idx += 256) {
    const int band = idx / J, m = idx - band * J;
    const double* xs = p.xt + ((int64_t)b * kBands + band) * p.nfs + m;
    const double* ys = p.yt + ((int64_t)b * kBands + band) * p.nfs + m;
    double x[kSeg], yp[kSeg];
    double nx = 0.0, ny = 0.0;
#pragma unroll
    for (int i = 0; i < kSeg; ++i) { x[i] = xs[i]; yp[i] = ys[i]; nx += x[i] * x[i]; ny += yp[i] * yp[i]; }
    const double c = sqrt(nx) / (sqrt(ny) + kEps);
    double xm = 0.0, ym = 0.0;
#pragma unroll
    for (int i = 0; i < kSeg; ++i) { yp[i] = fmin(yp[i] * c, x[i] * p.clip); xm += x[i]; ym += yp[i]; }
    xm /= kSeg; ym /= kSeg;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int i = 0; i < kSeg; ++i) { const double a = x[i] - xm, q = yp[i] - ym; sxx += a * a; syy += q * q; sxy += a * q; }
    acc += sxy / ((sqrt(sxx) + kEps) * (sqrt(syy) + kEps));
  }
  const double total = block_sum(acc, sh);
  if (threadIdx.x == 0) out[b] = total / ((double)J * kBands);
}

struct Geometry {
  int resampled, n_taps;
  PolyphaseGeometry pg;
  int64_t n, nf, nfs;
  int64_t at_xr, at_yr, at_e, at_kept, at_K, at_xt, at_yt, bytes;
};

// Validation and workspace layout: pure host arithmetic (no table is built, no GPU touched)
int32_t geometry(int32_t B, int32_t L, int32_t fs, Geometry* g) {
  if (B < 1 || B > 65535 || L < 1 || fs < 1) return -1;
  if (L > SEFD_STOI_MAX_SAMPLES) return -3;
  g->resampled = fs != kFs;
  g->n_taps = 0;
  g->n = L;
  if (g->resampled) {
    int up = kFs, down = fs;
    reduce_ratio(up, down);
    if (up > kMaxRatio || down > kMaxRatio) return -4;
    g->n_taps = 2 * (int)resample_half_len(kFs, fs) + 1;
    g->pg = polyphase_geometry(L, kFs, fs, g->n_taps);
    g->n = g->pg.n_out;
    if (g->n > SEFD_STOI_MAX_SAMPLES) return -3;
  }
  g->nf = g->n > kFrame ? (g->n - kFrame + kHop - 1) / kHop : 0;
  g->nfs = g->nf > 0 ? g->nf - 1 : 0;
  auto pad = [](int64_t v) { return (v + 255) & ~(int64_t)255; };
  int64_t at = pad((int64_t)(kFrame + kNfft + g->n_taps) * 8);
  const int64_t sig = g->resampled ? pad((int64_t)B * g->n * 8) : 0;
  g->at_xr = at; at += sig;
  g->at_yr = at; at += sig;
  g->at_e = at; at += pad((int64_t)B * g->nf * 8);
  g->at_kept = at; at += pad((int64_t)B * g->nf * 4);
  g->at_K = at; at += pad((int64_t)B * 4);
  g->at_xt = at; at += pad((int64_t)B * kBands * g->nfs * 8);
  g->at_yt = at; at += pad((int64_t)B * kBands * g->nfs * 8);
  g->bytes = at;
  return 0;
}
}  // namespace

extern "C" int64_t sefd_stoi_ws_bytes(int32_t B, int32_t L, int32_t fs) {
  Geometry g;
  const int32_t rc = geometry(B, L, fs, &g);
  return rc != 0 ? rc : g.bytes;
}

extern "C" int32_t sefd_stoi_gpu(const float* clean, const float* est, int32_t B, int32_t L, int32_t fs, void* ws, double* out, void* stream) {
  if (!clean || !est || !ws || !out) return -1;
  Geometry g;
  const int32_t rc = geometry(B, L, fs, &g);
  if (rc != 0) return rc;
  const Table& t = *table_for(fs);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  if (hipMemcpyAsync(base, t.blob.data(), t.blob.size() * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) return -2;
  StoiParams p;
  p.L = L; p.resampled = g.resampled; p.n_taps = g.n_taps;
  p.up = g.resampled ? g.pg.up : 1; p.down = g.resampled ? g.pg.down : 1; p.pre = g.resampled ? g.pg.pre : 0;
  p.pre_remove = g.resampled ? g.pg.pre_remove : 0;
  p.n = g.n; p.nf = (int32_t)g.nf; p.nfs = (int32_t)g.nfs;
  thirdoct_bins(p.lo, p.hi);
  p.clip = 1.0 + std::pow(10.0, -kBeta / 20.0);
  const double* tb = reinterpret_cast<const double*>(base);
  p.win = tb;
  p.tw = reinterpret_cast<const double2*>(tb + kFrame);
  p.taps = tb + kFrame + kNfft;
  p.xr = reinterpret_cast<double*>(base + g.at_xr);
  p.yr = reinterpret_cast<double*>(base + g.at_yr);
  p.e = reinterpret_cast<double*>(base + g.at_e);
  p.kept = reinterpret_cast<int32_t*>(base + g.at_kept);
  p.K = reinterpret_cast<int32_t*>(base + g.at_K);
  p.xt = reinterpret_cast<double*>(base + g.at_xt);
  p.yt = reinterpret_cast<double*>(base + g.at_yt);
  const unsigned uB = (unsigned)B;
  if (g.resampled)
    hipLaunchKernelGGL(stoi_resample_kernel, dim3((unsigned)((g.n + 255) / 256), uB, 2), dim3(256), 0, st, clean, est, p);
  if (g.nf > 0) hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)g.nf, uB), dim3(64), 0, st, clean, p);
  hipLaunchKernelGGL(stoi_select_kernel, dim3(uB), dim3(256), 0, st, p);
  if (g.nfs >= kSeg) hipLaunchKernelGGL(stoi_bands_kernel, dim3((unsigned)g.nfs, uB), dim3(64), 0, st, clean, est, p);
  hipLaunchKernelGGL(stoi_correlate_kernel, dim3(uB), dim3(256), 0, st, p, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
