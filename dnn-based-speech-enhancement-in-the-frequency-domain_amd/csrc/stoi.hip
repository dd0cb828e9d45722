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
//
// Extended STOI (Jensen & Taal 2016; sefd_stoi_gpu_ex, flags bit 0) replaces the correlate stage: one wave per 30-frame segment normalises the
// 15 x 30 clean and estimate matrices by row (band over time) and then by column (frame over bands), mean removed and divided by (norm + eps),
// and writes sum(x_n y_n) / 30; one workgroup per utterance then averages the segments in a fixed order.
//
// Backward (sefd_stoi_backward, after a forward with flags bit 1): the gradient with respect to the estimate, the clean signal, the frame
// selection and the resampling filter held constant.  The stages in reverse, every one a gather (no atomics, bit-identical from run to run):
//   segments   d score / d yt of every segment on its own: STOI one thread per (band, segment) through the clip, the norm-ratio scale c and the
//              normalisation; ESTOI one wave per segment through both normalisations.  450 doubles per segment.
//   gather     one thread per envelope element sums its up to 30 segments in ascending order.
//   bands      one wave per compacted frame: the estimate's spectrum Y again, G[k] = sum over the bands of k of g_yt Y[k] / yt, the
//              inverse-direction 512-point transform of G (the forward's radix-2 loop with conjugate twiddles), real part times the window.
//   uncompact  one thread per 10 kHz sample: its at most two original frames, each (if kept at position k, by the select stage's inverse map)
//              its window weight times the compacted-sample gradient, itself the sum over the at most two compacted frames g < K - 1 there.
//   resample   the transpose of the resampler, one thread per input sample; at 10 kHz the uncompact stage stores the fp32 result itself.
// Zero rule: where a square root or a norm under a division is exactly 0, the gradient through that term is 0 (torch would give NaN).
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
constexpr int kSegElems = kBands * kSeg;
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
  // extended score and backward (sefd_stoi_gpu_ex); null / 0 in the plain scorer
  int32_t nseg;                                     // segments per utterance when every frame is kept: nfs - 29, or 0
  int32_t* inv;                                     // [B][nf]: position of frame f among the kept ones, or -1
  double* seg;                                      // [B][nseg] ESTOI score of every segment
  double* gyt;                                      // [B][15][nfs] d loss / d yt
  double* segg;                                     // [B][nseg][15][30] the same of every segment on its own
  double* gf;                                       // [B][nfs][256] d loss / d compacted sample, frame by frame
  double* gy;                                       // [B][n] d loss / d sample at 10 kHz (resampled rates)
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
    const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));
    if (keep) kept[pos] = f;
    if (p.inv && f < nf) p.inv[(int64_t)b * nf + f] = keep ? pos : -1;
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

// ---- extended STOI: one wave per segment m of utterance b.  Rows first (lanes 0..14 the clean bands, 15..29 the estimate's), then columns
// (lanes 0..29 the clean frames, 30..59 the estimate's), each sum in index order.  kBwd: the cotangent of the segment's 15 x 30 estimate
// envelopes, scaled by grad_out[b] / J, goes to p.segg instead of the score to p.seg.
template <bool kBwd>
__global__ __launch_bounds__(64) void stoi_estoi_segment_kernel(const StoiParams p, const double* __restrict__ grad_out) {
  __shared__ double xs[kBands][kSeg + 1], ys[kBands][kSeg + 1], yc[kBands][kSeg + 1], gs[kBands][kSeg + 1];
  __shared__ double rown[kBands], coln[kSeg], part[kSeg];
  const int m = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int nfr = p.K[b] - 1;
  if (m > nfr - kSeg) return;                        // the whole wave leaves: segments start at m <= nfr - 30
  for (int idx = lane; idx < kSegElems; idx += 64) {
    const int band = idx / kSeg, t = idx - band * kSeg;
    const int64_t o = ((int64_t)b * kBands + band) * p.nfs + m + t;
    xs[band][t] = p.xt[o];
    ys[band][t] = p.yt[o];
  }
  __syncthreads();
  if (lane < 2 * kBands) {
    double (*a)[kSeg + 1] = lane < kBands ? xs : ys;
    const int r = lane < kBands ? lane : lane - kBands;
    double mean = 0.0, nn = 0.0;
    for (int t = 0; t < kSeg; ++t) mean += a[r][t];
    mean /= kSeg;
    for (int t = 0; t < kSeg; ++t) { const double v = a[r][t] - mean; a[r][t] = v; nn += v * v; }
    const double N = sqrt(nn);
    if (kBwd && lane >= kBands) {
      rown[r] = N;
      for (int t = 0; t < kSeg; ++t) yc[r][t] = a[r][t];
    }
    for (int t = 0; t < kSeg; ++t) a[r][t] = a[r][t] / (N + kEps);
  }
  __syncthreads();
  if (lane < 2 * kSeg) {
    const bool est = lane >= kSeg;
    double (*a)[kSeg + 1] = est ? ys : xs;
    const int t = est ? lane - kSeg : lane;
    double mean = 0.0, nn = 0.0;
    for (int k = 0; k < kBands; ++k) mean += a[k][t];
    mean /= kBands;
    for (int k = 0; k < kBands; ++k) { const double v = a[k][t] - mean; a[k][t] = v; nn += v * v; }
    const double N = sqrt(nn);
    if (kBwd && est) {
      coln[t] = N;                                   // ys keeps the centred column: the backward needs it, not the normalised one
    } else {
      for (int k = 0; k < kBands; ++k) a[k][t] = a[k][t] / (N + kEps);
    }
  }
  __syncthreads();
  if (!kBwd) {
    if (lane < kSeg) {
      double s = 0.0;
      for (int k = 0; k < kBands; ++k) s += xs[k][lane] * ys[k][lane];
      part[lane] = s;
    }
    __syncthreads();
    if (lane == 0) {
      double tot = 0.0;
      for (int t = 0; t < kSeg; ++t) tot += part[t];
      p.seg[(int64_t)b * p.nseg + m] = tot / kSeg;
    }
    return;
  }
  // z = cc / (N + eps), N = |cc|:  g_cc = g_z / (N + eps) - cc (g_z . cc) / ((N + eps)^2 N), the second term 0 at N == 0; then the mean's
  const double sc = grad_out[b] / ((double)(nfr - kSeg + 1) * kSeg);
  if (lane < kSeg) {
    const int t = lane;
    const double N = coln[t], D = N + kEps;
    double dot = 0.0, mean = 0.0;
    for (int k = 0; k < kBands; ++k) dot += xs[k][t] * sc * ys[k][t];
    const double kk = N > 0.0 ? dot / (D * D * N) : 0.0;
    for (int k = 0; k < kBands; ++k) { const double g = xs[k][t] * sc / D - kk * ys[k][t]; gs[k][t] = g; mean += g; }
    mean /= kBands;
    for (int k = 0; k < kBands; ++k) gs[k][t] -= mean;
  }
  __syncthreads();
  if (lane < kBands) {
    const int r = lane;
    const double N = rown[r], D = N + kEps;
    double dot = 0.0, mean = 0.0;
    for (int t = 0; t < kSeg; ++t) dot += gs[r][t] * yc[r][t];
    const double kk = N > 0.0 ? dot / (D * D * N) : 0.0;
    for (int t = 0; t < kSeg; ++t) { const double g = gs[r][t] / D - kk * yc[r][t]; gs[r][t] = g; mean += g; }
    mean /= kSeg;
    for (int t = 0; t < kSeg; ++t) gs[r][t] -= mean;
  }
  __syncthreads();
  double* dst = p.segg + ((int64_t)b * p.nseg + m) * kSegElems;
  for (int idx = lane; idx < kSegElems; idx += 64) dst[idx] = gs[idx / kSeg][idx % kSeg];
}

__global__ __launch_bounds__(256) void stoi_estoi_mean_kernel(const StoiParams p, double* __restrict__ out) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  const int nfr = p.nf > 0 ? p.K[b] - 1 : 0;
  if (nfr < kSeg) {
    if (threadIdx.x == 0) out[b] = 1e-5;
    return;
  }
  const int J = nfr - kSeg + 1;
  double acc = 0.0;
  for (int m = threadIdx.x; m < J; m += 256) acc += p.seg[(int64_t)b * p.nseg + m];
  const double total = block_sum(acc, sh);
  if (threadIdx.x == 0) out[b] = total / (double)J;
}

// ---- backward of stoi_correlate_kernel, one thread per (band, segment) as there: the cotangent of the segment's 30 estimate envelopes, scaled
// by grad_out[b] / (15 J).  d = sxy / (A Q), A = sqrt(sxx) + eps, Q = sqrt(syy) + eps, q = yp - mean(yp), yp = min(c y, clip x),
// c = |x| / (|y| + eps).  A clipped entry passes nothing directly; c depends on every y.
__global__ __launch_bounds__(256) void stoi_correlate_bwd_kernel(const StoiParams p, const double* __restrict__ grad_out) {
  const int b = blockIdx.y;
  const int nfr = p.K[b] - 1;
  if (nfr < kSeg) return;
  const int J = nfr - kSeg + 1, terms = J * kBands;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= terms) return;
  const int band = idx / J, m = idx - band * J;
  const double* xs = p.xt + ((int64_t)b * kBands + band) * p.nfs + m;
  const double* ys = p.yt + ((int64_t)b * kBands + band) * p.nfs + m;
  double x[kSeg], y[kSeg], q[kSeg];
  double nx = 0.0, ny = 0.0;
#pragma unroll
  for (int i = 0; i < kSeg; ++i) { x[i] = xs[i]; y[i] = ys[i]; nx += x[i] * x[i]; ny += y[i] * y[i]; }
  const double snx = sqrt(nx), sny = sqrt(ny), den = sny + kEps, c = snx / den;
  uint32_t open = 0;                                 // bit i: entry i is on the c y arm of the clip
  double xm = 0.0, ym = 0.0;
#pragma unroll
  for (int i = 0; i < kSeg; ++i) {
    const double u = y[i] * c, v = x[i] * p.clip;
    if (u <= v) open |= 1u << i;
    q[i] = fmin(u, v);
    xm += x[i]; ym += q[i];
  }
  xm /= kSeg; ym /= kSeg;
  double sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
  for (int i = 0; i < kSeg; ++i) { x[i] -= xm; q[i] -= ym; sxx += x[i] * x[i]; syy += q[i] * q[i]; sxy += x[i] * q[i]; }
  const double ssyy = sqrt(syy), A = sqrt(sxx) + kEps, Q = ssyy + kEps;
  const double k1 = 1.0 / (A * Q), k2 = ssyy > 0.0 ? sxy / (A * Q * Q * ssyy) : 0.0;
  double gmean = 0.0;
#pragma unroll
  for (int i = 0; i < kSeg; ++i) { q[i] = x[i] * k1 - q[i] * k2; gmean += q[i]; }     // q: now d / d q, then d / d yp
  gmean /= kSeg;
  double dc = 0.0;
#pragma unroll
  for (int i = 0; i < kSeg; ++i) {
    q[i] = (open >> i & 1u) ? q[i] - gmean : 0.0;
    dc += q[i] * y[i];
  }
  const double kc = sny > 0.0 ? -dc * snx / (den * den * sny) : 0.0;                    // d / d c times d c / d y_i = kc y_i
  const double sc = grad_out[b] / ((double)J * kBands);
  double* dst = p.segg + ((int64_t)b * p.nseg + m) * kSegElems + band * kSeg;
#pragma unroll
  for (int i = 0; i < kSeg; ++i) dst[i] = (c * q[i] + kc * y[i]) * sc;
}

// one thread per envelope element (band, frame f < nfr): its segments m = max(0, f - 29) .. min(J - 1, f), ascending
__global__ __launch_bounds__(256) void stoi_gather_segments_kernel(const StoiParams p) {
  const int b = blockIdx.y;
  const int nfr = p.K[b] - 1;
  if (nfr < kSeg) return;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= kBands * p.nfs) return;
  const int band = idx / p.nfs, f = idx - band * p.nfs;
  if (f >= nfr) return;
  const int J = nfr - kSeg + 1;
  const int mlo = f - (kSeg - 1) > 0 ? f - (kSeg - 1) : 0, mhi = f < J - 1 ? f : J - 1;
  const double* src = p.segg + (int64_t)b * p.nseg * kSegElems + band * kSeg;
  double acc = 0.0;
  for (int m = mlo; m <= mhi; ++m) acc += src[(int64_t)m * kSegElems + (f - m)];
  p.gyt[((int64_t)b * kBands + band) * p.nfs + f] = acc;
}

// one wave per frame g < K - 1 of the compacted estimate: d loss / d (its 256 compacted samples), through this frame alone
__global__ __launch_bounds__(64) void stoi_bands_bwd_kernel(const StoiParams p) {
  __shared__ double2 zy[kNfft], zg[kNfft];
  __shared__ double coef[kBands];
  const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int K = p.K[b];
  if (K - 1 < kSeg || g >= K - 1) return;
  const int32_t* kept = p.kept + (int64_t)b * p.nf;
  const double* yr = p.yr + (int64_t)b * p.n;
  for (int j = lane; j < kNfft; j += 64) {
    double vy = 0.0;
    if (j < kFrame) {                                // as stoi_bands_kernel gathers it
      const int k = g + (j >> 7), jj = j & (kHop - 1);
      if (k >= 1) vy += p.win[jj + kHop] * yr[(int64_t)kept[k - 1] * kHop + jj + kHop];
      if (k < K) vy += p.win[jj] * yr[(int64_t)kept[k] * kHop + jj];
      vy *= p.win[j];
    }
    zy[(int)(__builtin_bitreverse32((uint32_t)j) >> 23)] = make_double2(vy, 0.0);
  }
  if (lane < kBands) {
    const int64_t o = ((int64_t)b * kBands + lane) * p.nfs + g;
    const double yt = p.yt[o];
    coef[lane] = yt > 0.0 ? p.gyt[o] / yt : 0.0;     // sqrt at 0: no gradient
  }
  __syncthreads();
  for (int h = 1; h < kNfft; h <<= 1) {
    const int stride = kNfft / 2 / h;
    for (int j = lane; j < kNfft / 2; j += 64) {
      const int pos = j & (h - 1), i0 = ((j - pos) << 1) + pos, i1 = i0 + h;
      const double2 w = p.tw[pos * stride];
      const double2 a = zy[i0], c = zy[i1];
      const double2 t = make_double2(c.x * w.x - c.y * w.y, c.x * w.y + c.y * w.x);
      zy[i0] = make_double2(a.x + t.x, a.y + t.y);
      zy[i1] = make_double2(a.x - t.x, a.y - t.y);
    }
    __syncthreads();
  }
  for (int k = lane; k < kNfft; k += 64) {
    double cf = 0.0;
    for (int band = 0; band < kBands; ++band)
      if (k >= p.lo[band] && k < p.hi[band]) cf += coef[band];
    zg[(int)(__builtin_bitreverse32((uint32_t)k) >> 23)] = make_double2(cf * zy[k].x, cf * zy[k].y);
  }
  __syncthreads();
  for (int h = 1; h < kNfft; h <<= 1) {              // the same loop with conjugate twiddles: sum_k G[k] e^{+2 pi i jk / 512}
    const int stride = kNfft / 2 / h;
    for (int j = lane; j < kNfft / 2; j += 64) {
      const int pos = j & (h - 1), i0 = ((j - pos) << 1) + pos, i1 = i0 + h;
      const double2 w = p.tw[pos * stride];
      const double2 a = zg[i0], c = zg[i1];
      const double2 t = make_double2(c.x * w.x + c.y * w.y, c.y * w.x - c.x * w.y);
      zg[i0] = make_double2(a.x + t.x, a.y + t.y);
      zg[i1] = make_double2(a.x - t.x, a.y - t.y);
    }
    __syncthreads();
  }
  double* dst = p.gf + ((int64_t)b * p.nfs + g) * kFrame;
  for (int j = lane; j < kFrame; j += 64) dst[j] = p.win[j] * zg[j].x;
}

// one thread per sample i of the 10 kHz estimate: frames f = i / 128 - 1 and i / 128, each kept at position k or dropped
__global__ __launch_bounds__(256) void stoi_uncompact_kernel(const StoiParams p, float* __restrict__ grad_est) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const int b = blockIdx.y;
  const int K = p.K[b];
  double acc = 0.0;
  if (K - 1 >= kSeg) {
    const int f1 = (int)(i >> 7);
    for (int f = f1 - 1; f <= f1; ++f) {
      if (f < 0 || f >= p.nf) continue;
      const int k = p.inv[(int64_t)b * p.nf + f];
      if (k < 0) continue;
      const int jj = (int)(i - (int64_t)f * kHop), h = k + (jj >> 7), r = jj & (kHop - 1);
      double gc = 0.0;                               // compacted sample 128 k + jj lies in the compacted frames h - 1 and h
      if (h >= 1 && h - 1 < K - 1) gc += p.gf[((int64_t)b * p.nfs + h - 1) * kFrame + r + kHop];
      if (h < K - 1) gc += p.gf[((int64_t)b * p.nfs + h) * kFrame + r];
      acc += p.win[jj] * gc;
    }
  }
  if (p.resampled) p.gy[(int64_t)b * p.n + i] = acc;
  else grad_est[(int64_t)b * p.L + i] = (float)acc;
}

// transpose of stoi_resample_kernel: input sample j gathers the outputs o whose tap (o + pre_remove) down - pre - j up lies in [0, n_taps)
__global__ __launch_bounds__(256) void stoi_resample_adjoint_kernel(const StoiParams p, float* __restrict__ grad_est) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= p.L) return;
  const int b = blockIdx.y;
  const int64_t first = j * p.up + p.pre;            // (o + pre_remove) down runs from `first` to first + n_taps - 1
  int64_t olo = (first + p.down - 1) / p.down - p.pre_remove, ohi = (first + p.n_taps - 1) / p.down - p.pre_remove;
  if (olo < 0) olo = 0;
  if (ohi > p.n - 1) ohi = p.n - 1;
  const double* gy = p.gy + (int64_t)b * p.n;
  double acc = 0.0;
  for (int64_t o = olo; o <= ohi; ++o) acc += p.taps[(o + p.pre_remove) * p.down - first] * gy[o];
  grad_est[(int64_t)b * p.L + j] = (float)(acc * p.up);
}

// the estimate as fp64 for the backward at fs == 10 kHz, where the forward reads the fp32 input itself
__global__ __launch_bounds__(256) void stoi_keep_estimate_kernel(const float* __restrict__ est, const StoiParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < p.n) p.yr[(int64_t)blockIdx.y * p.n + i] = (double)est[(int64_t)blockIdx.y * p.L + i];
}


constexpr int32_t kFlagExtended = 1, kFlagKeep = 2;

struct Geometry {
  int resampled, n_taps;
  PolyphaseGeometry pg;
  int64_t n, nf, nfs, nseg;
  int64_t at_xr, at_yr, at_e, at_kept, at_K, at_xt, at_yt, at_seg, at_inv, at_gyt, at_segg, at_gf, at_gy, bytes;
};

// Validation and workspace layout: pure host arithmetic (no table is built, no GPU touched).  flags == 0 is the layout of the plain scorer;
// the extended score appends its per-segment scores, the keep bit what the backward reads and writes.
int32_t geometry(int32_t B, int32_t L, int32_t fs, int32_t flags, Geometry* g) {
  if (B < 1 || B > 65535 || L < 1 || fs < 1 || (flags & ~(kFlagExtended | kFlagKeep))) return -1;
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
  g->nseg = g->nfs >= kSeg ? g->nfs - kSeg + 1 : 0;
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
  g->at_seg = at;
  if (flags & kFlagExtended) at += pad((int64_t)B * g->nseg * 8);
  g->at_inv = g->at_gyt = g->at_segg = g->at_gf = g->at_gy = at;
  if (flags & kFlagKeep) {
    g->at_inv = at; at += pad((int64_t)B * g->nf * 4);
    g->at_gyt = at; at += pad((int64_t)B * kBands * g->nfs * 8);
    g->at_segg = at; at += pad((int64_t)B * g->nseg * kSegElems * 8);
    g->at_gf = at; at += pad((int64_t)B * g->nfs * kFrame * 8);
    g->at_gy = at; at += pad((int64_t)B * g->n * 8);       // resampled: d / d 10 kHz sample; 10 kHz: the estimate as fp64
  }
  g->bytes = at;
  return 0;
}

StoiParams params(const Geometry& g, int32_t L, int32_t flags, char* base) {
  StoiParams p;
  p.L = L; p.resampled = g.resampled; p.n_taps = g.n_taps;
  p.up = g.resampled ? g.pg.up : 1; p.down = g.resampled ? g.pg.down : 1; p.pre = g.resampled ? g.pg.pre : 0;
  p.pre_remove = g.resampled ? g.pg.pre_remove : 0;
  p.n = g.n; p.nf = (int32_t)g.nf; p.nfs = (int32_t)g.nfs; p.nseg = (int32_t)g.nseg;
  thirdoct_bins(p.lo, p.hi);
  p.clip = 1.0 + std::pow(10.0, -kBeta / 20.0);
  const double* tb = reinterpret_cast<const double*>(base);
  p.win = tb;
  p.tw = reinterpret_cast<const double2*>(tb + kFrame);
  p.taps = tb + kFrame + kNfft;
  const bool keep = flags & kFlagKeep;
  p.xr = reinterpret_cast<double*>(base + g.at_xr);
  p.yr = reinterpret_cast<double*>(base + (keep && !g.resampled ? g.at_gy : g.at_yr));
  p.e = reinterpret_cast<double*>(base + g.at_e);
  p.kept = reinterpret_cast<int32_t*>(base + g.at_kept);
  p.K = reinterpret_cast<int32_t*>(base + g.at_K);
  p.xt = reinterpret_cast<double*>(base + g.at_xt);
  p.yt = reinterpret_cast<double*>(base + g.at_yt);
  p.seg = flags & kFlagExtended ? reinterpret_cast<double*>(base + g.at_seg) : nullptr;
  p.inv = keep ? reinterpret_cast<int32_t*>(base + g.at_inv) : nullptr;
  p.gyt = keep ? reinterpret_cast<double*>(base + g.at_gyt) : nullptr;
  p.segg = keep ? reinterpret_cast<double*>(base + g.at_segg) : nullptr;
  p.gf = keep ? reinterpret_cast<double*>(base + g.at_gf) : nullptr;
  p.gy = keep && g.resampled ? reinterpret_cast<double*>(base + g.at_gy) : nullptr;
  return p;
}

int32_t forward(const float* clean, const float* est, int32_t B, int32_t L, int32_t fs, int32_t flags, void* ws, double* out, void* stream) {
  if (!clean || !est || !ws || !out) return -1;
  Geometry g;
  const int32_t rc = geometry(B, L, fs, flags, &g);
  if (rc != 0) return rc;
  const Table& t = *table_for(fs);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  if (hipMemcpyAsync(base, t.blob.data(), t.blob.size() * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) return -2;
  const StoiParams p = params(g, L, flags, base);
  const unsigned uB = (unsigned)B;
  if (g.resampled)
    hipLaunchKernelGGL(stoi_resample_kernel, dim3((unsigned)((g.n + 255) / 256), uB, 2), dim3(256), 0, st, clean, est, p);
  else if (flags & kFlagKeep)
    hipLaunchKernelGGL(stoi_keep_estimate_kernel, dim3((unsigned)((g.n + 255) / 256), uB), dim3(256), 0, st, est, p);
  if (g.nf > 0) hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)g.nf, uB), dim3(64), 0, st, clean, p);
  hipLaunchKernelGGL(stoi_select_kernel, dim3(uB), dim3(256), 0, st, p);
  if (g.nfs >= kSeg) hipLaunchKernelGGL(stoi_bands_kernel, dim3((unsigned)g.nfs, uB), dim3(64), 0, st, clean, est, p);
  if (flags & kFlagExtended) {
    if (g.nseg > 0)
      hipLaunchKernelGGL(stoi_estoi_segment_kernel<false>, dim3((unsigned)g.nseg, uB), dim3(64), 0, st, p, (const double*)nullptr);
    hipLaunchKernelGGL(stoi_estoi_mean_kernel, dim3(uB), dim3(256), 0, st, p, out);
  } else {
    hipLaunchKernelGGL(stoi_correlate_kernel, dim3(uB), dim3(256), 0, st, p, out);
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
}  // namespace

extern "C" int64_t sefd_stoi_ws_bytes(int32_t B, int32_t L, int32_t fs) { return sefd_stoi_ws_bytes_ex(B, L, fs, 0); }

extern "C" int64_t sefd_stoi_ws_bytes_ex(int32_t B, int32_t L, int32_t fs, int32_t flags) {
  Geometry g;
  const int32_t rc = geometry(B, L, fs, flags, &g);
  return rc != 0 ? rc : g.bytes;
}

extern "C" int32_t sefd_stoi_gpu(const float* clean, const float* est, int32_t B, int32_t L, int32_t fs, void* ws, double* out, void* stream) {
  return forward(clean, est, B, L, fs, 0, ws, out, stream);
}

extern "C" int32_t sefd_stoi_gpu_ex(const float* clean, const float* est, int32_t B, int32_t L, int32_t fs, int32_t flags, void* ws, double* out,
                                    void* stream) {
  return forward(clean, est, B, L, fs, flags, ws, out, stream);
}

extern "C" int32_t sefd_stoi_backward(int32_t B, int32_t L, int32_t fs, int32_t flags, void* ws, const double* grad_out, float* grad_est,
                                      void* stream) {
  if (!ws || !grad_out || !grad_est || !(flags & kFlagKeep)) return -1;
  Geometry g;
  const int32_t rc = geometry(B, L, fs, flags, &g);
  if (rc != 0) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const StoiParams p = params(g, L, flags, static_cast<char*>(ws));
  const unsigned uB = (unsigned)B;
  if (g.nseg > 0) {
    if (flags & kFlagExtended)
      hipLaunchKernelGGL(stoi_estoi_segment_kernel<true>, dim3((unsigned)g.nseg, uB), dim3(64), 0, st, p, grad_out);
    else
      hipLaunchKernelGGL(stoi_correlate_bwd_kernel, dim3((unsigned)((g.nseg * kBands + 255) / 256), uB), dim3(256), 0, st, p, grad_out);
    hipLaunchKernelGGL(stoi_gather_segments_kernel, dim3((unsigned)((g.nfs * kBands + 255) / 256), uB), dim3(256), 0, st, p);
    hipLaunchKernelGGL(stoi_bands_bwd_kernel, dim3((unsigned)g.nfs, uB), dim3(64), 0, st, p);
  }
  hipLaunchKernelGGL(stoi_uncompact_kernel, dim3((unsigned)((g.n + 255) / 256), uB), dim3(256), 0, st, p, grad_est);
  if (g.resampled)
    hipLaunchKernelGGL(stoi_resample_adjoint_kernel, dim3((unsigned)((L + 255) / 256), uB), dim3(256), 0, st, p, grad_est);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
