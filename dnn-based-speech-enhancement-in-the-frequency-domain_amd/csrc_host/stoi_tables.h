// Constants of the STOI scorers, shared by the host scorer (scorers.cpp, g++) and the launcher of the device scorer (csrc/stoi.hip, hipcc
// host side): the Kaiser-windowed sinc of the resampler, its polyphase alignment, and the one-third octave band edges.  Host code only,
// double precision; one statement of each so the two scorers cannot drift apart.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace sefd_stoi {

constexpr int kFs = 10000, kFrame = 256, kNfft = 512, kBands = 15, kSeg = 30;
constexpr double kMinFreq = 150.0, kBeta = -15.0, kDynRange = 40.0;
constexpr double kPi = 3.14159265358979323846;
constexpr double kEps = 2.220446049250313e-16;

inline double bessel_i0(double x) {                // series of the modified Bessel function (np.kaiser uses i0)
  double s = 1.0, t = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 200; ++k) { t *= q / ((double)k * k); s += t; if (t < 1e-18 * s) break; }
  return s;
}

inline void reduce_ratio(int& p, int& q) {
  int a = p, b = q;
  while (b) { const int t = a % b; a = b; b = t; }
  p /= a; q /= a;
}

// Half length L of the low-pass for the rational factor p / q (2 L + 1 taps): 60 dB rejection, 10 % roll-off.  As a double, so that a
// caller can refuse a ratio whose filter would be absurdly long before anything of that size is built.
inline double resample_half_len(int p, int q) {
  reduce_ratio(p, q);
  const double fc = 1.0 / (2.0 * std::max(p, q)), roll = fc / 10.0, rej = 60.0;
  return std::ceil((rej - 8.0) / (28.714 * roll));
}

// Octave-style `resample` low-pass (Kaiser-windowed sinc, 60 dB, 10 % roll-off), unit DC gain
inline std::vector<double> resample_window(int p, int q) {
  reduce_ratio(p, q);
  const double fc = 1.0 / (2.0 * std::max(p, q)), roll = fc / 10.0, rej = 60.0;
  const int L = (int)std::ceil((rej - 8.0) / (28.714 * roll));
  const double beta = 0.1102 * (rej - 8.7);
  std::vector<double> h(2 * L + 1);
  double sum = 0;
  for (int i = 0; i <= 2 * L; ++i) {
    const double t = i - L, a = 2.0 * fc * t;
    const double sinc = a == 0.0 ? 1.0 : std::sin(kPi * a) / (kPi * a);
    const double r = 2.0 * i / (2.0 * L) - 1.0;
    h[i] = 2.0 * p * fc * sinc * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / bessel_i0(beta);
    sum += h[i];
  }
  for (double& v : h) v /= sum;
  return h;
}

// scipy.signal.resample_poly's alignment of upfirdn(h * up, x, up, down) for a filter of n_taps taps (up / down already reduced):
// output sample o reads the up-sampled stream at (o + pre_remove) * down - pre, and there are ceil(n_in * up / down) outputs.
struct PolyphaseGeometry { int up, down, pre; int64_t pre_remove, n_out; };
inline PolyphaseGeometry polyphase_geometry(int64_t n_in, int up, int down, int n_taps) {
  reduce_ratio(up, down);
  PolyphaseGeometry g;
  g.up = up; g.down = down;
  int64_t n_out = n_in * up;
  g.n_out = n_out / down + (n_out % down ? 1 : 0);
  const int half = (n_taps - 1) / 2;
  g.pre = down - half % down;
  g.pre_remove = (half + g.pre) / down;
  return g;
}

inline std::vector<double> hann_inner(int n) {      // np.hanning(n + 2)[1:-1]
  std::vector<double> w(n);
  for (int i = 0; i < n; ++i) w[i] = 0.5 - 0.5 * std::cos(2.0 * kPi * (i + 1) / (n + 1));
  return w;
}

// FFT bins [lo, hi) of the kBands one-third octave bands from kMinFreq at kFs / kNfft (pystoi's thirdoct: nearest bin to either edge)
inline void thirdoct_bins(int* lo, int* hi) {
  for (int b = 0; b < kBands; ++b) {
    const double fl = kMinFreq * std::pow(2.0, (2.0 * b - 1.0) / 6.0), fh = kMinFreq * std::pow(2.0, (2.0 * b + 1.0) / 6.0);
    double bl = 1e300, bh = 1e300;
    for (int k = 0; k <= kNfft / 2; ++k) {
      const double f = (double)kFs * k / kNfft;
      if ((f - fl) * (f - fl) < bl) { bl = (f - fl) * (f - fl); lo[b] = k; }
      if ((f - fh) * (f - fh) < bh) { bh = (f - fh) * (f - fh); hi[b] = k; }
    }
  }
}

}  // namespace sefd_stoi
