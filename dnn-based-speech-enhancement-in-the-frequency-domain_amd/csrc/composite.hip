// Frame analysis of the composite measure (Hu & Loizou 2006: CSIG / CBAK / COVL; reference composite.m:151-562 run through Octave by
// tools_for_estimate.py:24-33): per 30 ms frame with a quarter-frame hop, for a batch of clean / processed pairs on the device,
//   WSS    n_fft-point power spectrum -> 25 Klatt critical bands (sparse filter table built by the host) -> slopes, nearest peaks, weights;
//   LLR    autocorrelation lags 0..P -> Levinson -> log(A_p R_c A_p' / A_c R_c A_c');
//   segSNR 10 log10(Es / (En + eps) + eps) clamped to [-10, 35];
// then per utterance the 95 % trimmed means of WSS and LLR and the plain mean of segSNR.
//
// Stage 1: ONE wave (a 64-thread workgroup) per (frame, utterance).  Everything is fp64: the samples + eps, the window, the autocorrelation,
// Levinson and the quadratic forms (frames of digital silence are otherwise singular), and the FFT - a complex M = n_fft / 2 point radix-2
// transform of the even / odd packed real frame in the wave's LDS, bit-reversed load, in-place passes, then the real-FFT split.  The FFT is
// a few tens of kFLOP per frame: fp64 costs nothing here and keeps the band energies exact down to the 1e-10 floor.
// Stage 2: one workgroup per utterance.  The trimmed mean is the mean of the k = round(0.95 n) smallest frame values: a radix selection of
// the k-th smallest (8 passes of 8-bit digits over order-preserving keys, LDS histograms) gives the threshold t, then
// (sum of the values below t + (k - their count) t) / k.  Sums run in a fixed order (strided per thread, fixed shuffle tree), so results
// are bit-identical run to run and an utterance's numbers do not depend on the rest of its batch.
#include <hip/hip_runtime.h>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include "../../include/sefd.h"

namespace {
constexpr int kBands = 25;
constexpr int kMaxOrder = 16;
constexpr double kEps = 2.220446049250313080847e-16;       // MATLAB eps = 2^-52

struct CompParams {
  int32_t L, win, skip, nf, M, logM, P;
  int32_t band_lo[kBands], band_cnt[kBands], band_off[kBands];
  const double* window;     // [win]
  const double2* tw;        // [M]: (cos, -sin)(2 pi k / n_fft)
  const double* filt;       // sparse band weights, band i at band_off[i], band_cnt[i] bins from bin band_lo[i]
  double* fr;               // [3][B][nf] per-frame llr, wss, segsnr
  int64_t plane;            // B * nf
};

// Host-side constants of one sample rate, built once and kept for the life of the process (so the asynchronous copy never outlives them).
struct Table {
  int win = 0, skip = 0, nfft = 0, P = 0;
  int lo[kBands], cnt[kBands], off[kBands];
  std::vector<double> blob;  // window [win], pad to even, tw [2 M], filt [...]
  size_t tw_at = 0, filt_at = 0;
};

int matlab_round(double x) { return (int)std::copysign(std::floor(std::fabs(x) + 0.5), x); }

const Table* table_for(int fs) {
  static std::mutex mu;
  static std::map<int, std::unique_ptr<Table>> cache;
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find(fs);
  if (it != cache.end()) return it->second.get();
  // Klatt's critical bands (centre frequency, bandwidth), Hz, as published for the WSS measure
  static const double cent[kBands] = {50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38,
                                      1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
  static const double bwid[kBands] = {70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914,
                                      140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136};
  auto t = std::make_unique<Table>();
  t->win = matlab_round(30.0 * fs / 1000.0);
  t->skip = t->win / 4;
  int nfft = 1;
  while (nfft < 2 * t->win) nfft <<= 1;
  t->nfft = nfft;
  t->P = fs < 10000 ? 10 : 16;
  const int half = nfft / 2;
  std::vector<double>& v = t->blob;
  for (int n = 1; n <= t->win; ++n) v.push_back(0.5 * (1.0 - std::cos(2.0 * M_PI * n / (t->win + 1))));
  if (v.size() & 1) v.push_back(0.0);
  t->tw_at = v.size();
  for (int k = 0; k < half; ++k) {
    v.push_back(std::cos(2.0 * M_PI * k / nfft));
    v.push_back(-std::sin(2.0 * M_PI * k / nfft));
  }
  t->filt_at = v.size();
  const double max_freq = fs / 2.0, min_factor = std::exp(-30.0 / (2.0 * 2.303));
  for (int i = 0; i < kBands; ++i) {
    const double f0 = std::floor(cent[i] / max_freq * half), bw = bwid[i] / max_freq * half;
    const double norm = std::log(bwid[0]) - std::log(bwid[i]);
    int lo = -1, hi = -1;
    for (int j = 0; j < half; ++j) {
      const double d = (j - f0) / bw;
      const double g = std::exp(-11.0 * (d * d) + norm);
      if (g > min_factor) { if (lo < 0) lo = j; hi = j; }
    }
    t->lo[i] = lo < 0 ? 0 : lo;
    t->cnt[i] = lo < 0 ? 0 : hi - lo + 1;
    t->off[i] = (int)(v.size() - t->filt_at);
    for (int j = t->lo[i]; j < t->lo[i] + t->cnt[i]; ++j) {       // the Gaussian is unimodal: [lo, hi] holds every bin above the factor
      const double d = (j - f0) / bw;
      const double g = std::exp(-11.0 * (d * d) + norm);
      v.push_back(g > min_factor ? g : 0.0);
    }
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
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// Levinson-Durbin on lags r[0..P] (composite.m lpcoeff): returns A = [1, -a] in A[0..P].
__device__ void levinson(const double* r, int P, double* A) {
  double a[kMaxOrder], prev[kMaxOrder];
  double E = r[0];
  for (int i = 0; i < P; ++i) {
    double s = 0.0;
    for (int j = 0; j < i; ++j) s += a[j] * r[i - j];
    const double k = (r[i + 1] - s) / E;
    for (int j = 0; j < i; ++j) prev[j] = a[j];
    for (int j = 0; j < i; ++j) a[j] = prev[j] - k * prev[i - 1 - j];
    a[i] = k;
    E = (1.0 - k * k) * E;
  }
  A[0] = 1.0;
  for (int j = 0; j < P; ++j) A[j + 1] = -a[j];
}
__device__ double quad_form(const double* A, const double* r, int P) {
  double q = 0.0;
  for (int i = 0; i <= P; ++i) {
    double s = 0.0;
    for (int j = 0; j <= P; ++j) s += r[i > j ? i - j : j - i] * A[j];
    q += A[i] * s;
  }
  return q;
}

// Nearest peak of band i (0..23): right while the slope is > 0 (reporting the band before the first non-positive slope), else left while it
// is <= 0 (a search that runs off band 0 takes band 0).
__device__ double loc_peak(const double* E, int i) {
  if (E[i + 1] - E[i] > 0) {
    int n = i;
    while (n < kBands - 1 && E[n + 1] - E[n] > 0) ++n;
    return E[n - 1];
  }
  int n = i;
  while (n >= 0 && E[n + 1] - E[n] <= 0) --n;
  return E[n + 1];
}

// The 25 band energies (dB) of one windowed frame -> Eb[0..24].  z: this wave's M complex doubles of LDS.
__device__ void band_energies(const float* src, const CompParams& p, double2* z, double* Eb, int lane) {
  const int M = p.M;
  for (int m = lane; m < M; m += 64) {
    const int n0 = 2 * m, n1 = 2 * m + 1;
    const double re = n0 < p.win ? ((double)src[n0] + kEps) * p.window[n0] : 0.0;
    const double im = n1 < p.win ? ((double)src[n1] + kEps) * p.window[n1] : 0.0;
    z[__builtin_bitreverse32((uint32_t)m) >> (32 - p.logM)] = make_double2(re, im);
  }
  __syncthreads();
  for (int h = 1; h < M; h <<= 1) {
    const int stride = M / h;
    for (int j = lane; j < M / 2; j += 64) {
      const int pos = j & (h - 1), i0 = ((j - pos) << 1) + pos, i1 = i0 + h;
      const double2 a = z[i0], t = cmul(z[i1], p.tw[pos * stride]);       // W_M^pos/(2h) = W_nfft^(pos M / h)
      z[i0] = make_double2(a.x + t.x, a.y + t.y);
      z[i1] = make_double2(a.x - t.x, a.y - t.y);
    }
    __syncthreads();
  }
  if (lane < kBands) {
    // real-FFT split: X[k] = (Z[k] + conj Z[M-k]) / 2 - i W^k (Z[k] - conj Z[M-k]) / 2, bins 0..n_fft/2 - 1
    double e = 0.0;
    const int lo = p.band_lo[lane], cnt = p.band_cnt[lane];
    const double* f = p.filt + p.band_off[lane];
    for (int q = 0; q < cnt; ++q) {
      const int k = lo + q;
      const double2 a = z[k], b = z[(M - k) & (M - 1)];
      const double2 ev = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
      const double2 od = make_double2(0.5 * (a.x - b.x), 0.5 * (a.y + b.y));      // (Z[k] - conj Z[M-k]) / 2
      const double2 w = p.tw[k];
      const double2 wo = cmul(w, od);
      const double xr = ev.x + wo.y, xi = ev.y - wo.x;                              // ev - i (w od)
      e += (xr * xr + xi * xi) * f[q];
    }
    Eb[lane] = 10.0 * log10(fmax(e, 1e-10));
  }
  __syncthreads();
}

__global__ __launch_bounds__(64) void composite_frame_kernel(const float* __restrict__ clean, const float* __restrict__ enh, const CompParams p) {
  extern __shared__ double2 lds[];                            // M complex doubles; stage (a) uses it as the two frames, 2 win <= 2 M doubles
  __shared__ double Ebc[kBands], Ebp[kBands];
  const int f = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int64_t base = (int64_t)b * p.L + (int64_t)f * p.skip;
  const float* c = clean + base;
  const float* e = enh + base;
  double* xc = reinterpret_cast<double*>(lds);
  double* xp = xc + p.win;
  // (a) windowed frames of x + eps, frame energies, autocorrelation lags
  double es = 0.0, en = 0.0;
  for (int n = lane; n < p.win; n += 64) {
    const double w = p.window[n];
    const double a = ((double)c[n] + kEps) * w, q = ((double)e[n] + kEps) * w, d = a - q;
    xc[n] = a; xp[n] = q;
    es += a * a; en += d * d;
  }
  __syncthreads();
  double rc[kMaxOrder + 1], rp[kMaxOrder + 1];
#pragma unroll
  for (int k = 0; k <= kMaxOrder; ++k) {
    double sc = 0.0, sp = 0.0;
    if (k <= p.P)
      for (int n = lane; n < p.win - k; n += 64) { sc += xc[n] * xc[n + k]; sp += xp[n] * xp[n + k]; }
    rc[k] = wave_sum(sc);
    rp[k] = wave_sum(sp);
  }
  es = wave_sum(es);
  en = wave_sum(en);
  __syncthreads();                                            // frames done: the LDS becomes the FFT buffer
  const int64_t o = (int64_t)b * p.nf + f;
  if (lane == 0) {
    const double s = 10.0 * log10(es / (en + kEps) + kEps);
    p.fr[2 * p.plane + o] = fmin(fmax(s, -10.0), 35.0);
  } else if (lane == 1) {
    double Ac[kMaxOrder + 1], Ap[kMaxOrder + 1];
    levinson(rc, p.P, Ac);
    levinson(rp, p.P, Ap);
    p.fr[o] = log(quad_form(Ap, rc, p.P) / quad_form(Ac, rc, p.P));
  }
  // (b) WSS
  band_energies(c, p, lds, Ebc, lane);
  band_energies(e, p, lds, Ebp, lane);
  double num = 0.0, den = 0.0;
  if (lane < kBands - 1) {
    double mc = Ebc[0], mp = Ebp[0];
    for (int i = 1; i < kBands; ++i) { mc = fmax(mc, Ebc[i]); mp = fmax(mp, Ebp[i]); }
    const double wc = 20.0 / (20.0 + mc - Ebc[lane]) * (1.0 / (1.0 + loc_peak(Ebc, lane) - Ebc[lane]));
    const double wp = 20.0 / (20.0 + mp - Ebp[lane]) * (1.0 / (1.0 + loc_peak(Ebp, lane) - Ebp[lane]));
    const double w = (wc + wp) / 2.0, d = (Ebc[lane + 1] - Ebc[lane]) - (Ebp[lane + 1] - Ebp[lane]);
    num = w * d * d;
    den = w;
  }
  num = wave_sum(num);
  den = wave_sum(den);
  if (lane == 0) p.fr[p.plane + o] = num / den;
}

__device__ __forceinline__ uint64_t okey(double v) {        // order-preserving map of doubles onto unsigned integers
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(uint64_t key) {
  return __longlong_as_double((long long)((key >> 63) ? (key & 0x7fffffffffffffffull) : ~key));
}

// fixed-order sum over the 256 threads of a workgroup; every thread gets the total
__device__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// mean of the k = round(0.95 n) smallest of v[0..n)
__device__ double trimmed_mean(const double* v, int n, unsigned* hist, double* sh, uint64_t* sel) {
  const int k = (int)round(0.95 * n);
  uint64_t prefix = 0;
  int rem = k;
  for (int shift = 56; shift >= 0; shift -= 8) {
    const uint64_t hi = shift == 56 ? 0ull : (~0ull << (shift + 8));
    for (int i = threadIdx.x; i < 256; i += 256) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
      const uint64_t key = okey(v[i]);
      if ((key & hi) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int cum = 0, d = 0;
      for (; d < 255 && cum + (int)hist[d] < rem; ++d) cum += (int)hist[d];
      sel[0] = prefix | ((uint64_t)d << shift);
      sel[1] = (uint64_t)(rem - cum);
    }
    __syncthreads();
    prefix = sel[0];
    rem = (int)sel[1];
    __syncthreads();
  }
  const double t = key_value(prefix);                        // the k-th smallest value: ties with it fill the rest of the k
  double s = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double x = v[i];
    if (okey(x) < prefix) { s += x; cnt += 1.0; }
  }
  s = block_sum(s, sh);
  cnt = block_sum(cnt, sh);
  return (s + ((double)k - cnt) * t) / (double)k;
}

__global__ __launch_bounds__(256) void composite_reduce_kernel(const CompParams p, double* out) {
  __shared__ unsigned hist[256];
  __shared__ double sh[4];
  __shared__ uint64_t sel[2];
  const int b = blockIdx.x, n = p.nf;
  const double* llr = p.fr + (int64_t)b * n;
  const double* wss = p.fr + p.plane + (int64_t)b * n;
  const double* seg = p.fr + 2 * p.plane + (int64_t)b * n;
  double r_llr, r_wss, r_seg;
  if (n == 0) {
    r_llr = r_wss = r_seg = __longlong_as_double(0x7ff8000000000000ll);    // the mean of no frames
  } else {
    r_llr = trimmed_mean(llr, n, hist, sh, sel);
    r_wss = trimmed_mean(wss, n, hist, sh, sel);
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += seg[i];
    r_seg = block_sum(s, sh) / n;
  }
  if (threadIdx.x == 0) {
    out[3 * b + 0] = r_llr;
    out[3 * b + 1] = r_wss;
    out[3 * b + 2] = r_seg;
  }
}

struct Geometry { const Table* t; int64_t nf; size_t table_bytes; };

int32_t geometry(int32_t B, int32_t L, int32_t fs, Geometry* g) {
  if (B <= 0 || B > 65535 || L <= 0 || fs <= 0) return -1;
  const int win = matlab_round(30.0 * fs / 1000.0);
  int nfft = 1;
  while (nfft < 2 * win) nfft <<= 1;
  if (nfft < 256 || nfft > 4096) return -4;                  // 4.3 .. 68.2 kHz
  if (L < win) return -1;
  g->t = table_for(fs);
  const double x = std::floor((double)L / g->t->skip - (double)win / g->t->skip);
  g->nf = x > 0 ? (int64_t)x : 0;
  if (g->nf > SEFD_COMPOSITE_MAX_FRAMES) return -3;
  g->table_bytes = (g->t->blob.size() * sizeof(double) + 255) & ~(size_t)255;
  return 0;
}
}  // namespace

extern "C" int64_t sefd_composite_ws_bytes(int32_t B, int32_t L, int32_t fs) {
  Geometry g;
  const int32_t rc = geometry(B, L, fs, &g);
  if (rc != 0) return rc;
  return (int64_t)g.table_bytes + 3 * (int64_t)B * g.nf * (int64_t)sizeof(double);
}

extern "C" int32_t sefd_composite_frames(const float* clean, const float* enhanced, int32_t B, int32_t L, int32_t fs, void* ws, double* out,
                                         void* stream) {
  if (!clean || !enhanced || !ws || !out) return -1;
  Geometry g;
  const int32_t rc = geometry(B, L, fs, &g);
  if (rc != 0) return rc;
  const Table& t = *g.t;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  if (hipMemcpyAsync(base, t.blob.data(), t.blob.size() * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) return -2;
  CompParams p;
  p.L = L; p.win = t.win; p.skip = t.skip; p.nf = (int32_t)g.nf; p.M = t.nfft / 2; p.P = t.P;
  p.logM = 0;
  while ((1 << p.logM) < p.M) ++p.logM;
  for (int i = 0; i < kBands; ++i) { p.band_lo[i] = t.lo[i]; p.band_cnt[i] = t.cnt[i]; p.band_off[i] = t.off[i]; }
  const double* tb = reinterpret_cast<const double*>(base);
  p.window = tb;
  p.tw = reinterpret_cast<const double2*>(tb + t.tw_at);
  p.filt = tb + t.filt_at;
  p.fr = reinterpret_cast<double*>(base + g.table_bytes);
  p.plane = (int64_t)B * g.nf;
  if (g.nf > 0)
    hipLaunchKernelGGL(composite_frame_kernel, dim3((unsigned)g.nf, (unsigned)B), dim3(64), (size_t)p.M * sizeof(double2), st, clean, enhanced, p);
  hipLaunchKernelGGL(composite_reduce_kernel, dim3((unsigned)B), dim3(256), 0, st, p, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
