// Planners: model configuration -> op list over channels-last buffers (DCCRN: models.py:15-284 of the reference).
//
// Layout decisions (MI355X-first, not the reference's NCHW):
//   * every activation is channels-last  [B][T(+1)][F][C]  so that each A-row of the implicit GEMM is a few contiguous
//     runs (all 5 frequency taps x C channels of one frame are ONE run) -> 16-byte coalesced loads, no im2col;
//   * a complex conv is one real GEMM with the block weight [[Wr,-Wi],[Wi,Wr]] (same MACs as the reference's 4 convs);
//   * the transposed conv is two dense sub-pixel GEMMs (even / odd output rows), never a scatter;
//   * complex_cat / chunk / permute / reshape glue of the reference (23 % of its CPU step) is index arithmetic in the
//     run descriptors: the skip connection is a second source pointer, the LSTM feature order c*D+d is a weight permutation;
//   * decoder buffers keep the extra frame that `out[..., 1:]` drops, because BatchNorm statistics include it.
//
// This header: what every planner shares - the front-end geometry (Stft) and the Builder (arenas, parameter tables, op list, GEMM
// descriptors, the conv stack, the recurrent block, weight gradients and their UNPACK).  The planners: plan_dccrn.cpp, plan_crn.cpp,
// plan_fsn.cpp, plan_seq.cpp, plan_clstm.cpp, plan_frontend.cpp; the post-pass over a finished plan and build_plan(): plan.cpp.
#pragma once
#include "plan.h"
#include "tuning.h"

#include <algorithm>
#include <array>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace sefd {

constexpr double kPi = 3.14159265358979323846;
inline int64_t rup(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// Runs of a RUNGEMM / WGRAD are whole, 16-byte aligned chunks (then the kernels use the LDS-DMA loaders).  Arena buffers are
// 256-byte aligned, so only element offsets matter.  WGRAD: the upstream-gradient operand must be chunk aligned as well.
inline bool runs_aligned(const RunGemm& g, bool is_wgrad) {
  const int vec = 16 / esize(g.xdt);
  bool ok = true;
  for (int s = 0; s < g.nseg && ok; ++s) {
    const Seg& sg = g.seg[s];
    if (sg.src < 0) { ok = is_wgrad; continue; }          // the ones run exists only in WGRAD
    const int q = sg.src;
    ok = sg.off % vec == 0 && sg.len % vec == 0 && g.fstride[q] % vec == 0 && g.base[q] % vec == 0 && g.rowlen[q] % vec == 0 &&
         g.tstride[q] % vec == 0 && g.bstride[q] % vec == 0 && (g.x[q].off % 16) == 0;
  }
  if (is_wgrad)
    ok = ok && g.xdt == DT_BF16 && g.ydt == DT_BF16 && g.N % 8 == 0 && g.y_off % 8 == 0 && g.y_fstride % 8 == 0 && g.y_tstride % 8 == 0 &&
         g.y_bstride % 8 == 0 && (g.y.off % 16) == 0;
  return ok;
}

// ConvSTFT / ConviSTFT window sample j (tools_for_model.py:17-20)
inline double window_value(const ModelConfig& cfg, int j, int W) {
  if (cfg.window == 1) return 1.0;
  if (cfg.window == 2 && cfg.window_values) return cfg.window_values[j];
  return 0.5 - 0.5 * std::cos(2.0 * kPi * j / W);
}

// ConvSTFT / ConviSTFT front end of the DCCRN, CRN and front-end plans (tools_for_model.py:16-61): frame geometry, window, bases
struct Stft {
  int B = 0, L = 0, W = 0, hop = 0, NFFT = 0, trim = 0, T = 0, NF = 0, NS = 0, SW = 0, Lp = 0;
  std::vector<double> win;
  std::vector<double> Kinv;                                // synthesis basis [part][k][j] (Builder::synthesis)
  Ptr c_coff = Ptr{-1, 0, 0};                              // OLA normaliser: sum of the squared windows over the frames covering a sample
  Stft() = default;
  explicit Stft(const ModelConfig& cfg) : B(cfg.B), L(cfg.L), W(cfg.win_len), hop(cfg.hop), NFFT(cfg.fft_len) {
    trim = W - hop;
    T = (L + 2 * trim - W) / hop + 1;
    NF = NFFT / 2 + 1; NS = NF + 1; SW = NS * 2;             // spectrum rows: NS (re, im) pairs, slot 0 unused (aligned bins)
    Lp = (T - 1) * hop + W;
    win.resize(W);
    for (int j = 0; j < W; ++j) win[j] = window_value(cfg, j, W);    // win_type None: np.ones (tools_for_model.py:17-18)
  }
  // analysis basis (tools_for_model.py:16-33): K[part*NF+k][j] = w[j]*{cos,-sin}(2 pi k j / NFFT), without the window
  double Kun(int part, int k, int j) const {
    const double ang = 2.0 * kPi * (double)(((int64_t)k * j) % NFFT) / NFFT;
    return part == 0 ? std::cos(ang) : -std::sin(ang);
  }
};

// signed 1-based flat element `idx` of parameter p (the entries of PACK tables and of the Coef / Bias functions)
inline int32_t pe(const ParamInfo& p, int64_t idx, int sign = 1) { return (int32_t)(sign * (p.off + idx + 1)); }

struct Builder {
  Plan* P;
  ModelConfig c;
  int64_t ws_off = 0;
  int64_t io_off = 0;
  std::map<std::string, int> pidx, sidx;

  // gradient partial region (allocated at the end) and the inverse (unpack) table
  int64_t gp_off = 0;                                     // floats
  struct Fix { int op; int64_t rel; int which; };         // which: 0 -> op.g.w, 1 -> op.unpack.part, 2 -> op.mask.colsum
  std::vector<Fix> fixes;
  std::vector<std::vector<int32_t>> inv;                  // per trainable element: signed (gp-relative position + 1)
  std::vector<char> zero_grad;                            // elements without any contribution that UNPACK still writes (an exact 0)

  Ptr mk(int arena, int64_t off) { Ptr p; p.arena = arena; p.pad_ = 0; p.off = off; return p; }
  Ptr none() { return mk(A_NONE, 0); }

  Ptr ws(const std::string& name, int64_t elems, int dt) {
    const int64_t bytes = rup(elems * esize(dt), 256);
    Ptr p = mk(A_WS, ws_off);
    P->bufs[name] = BufInfo{ws_off, elems * esize(dt), dt};
    ws_off += bytes;
    return p;
  }
  Ptr io(const std::string& name, int64_t elems) {
    Ptr p = mk(A_IO, io_off);
    P->bufs["io." + name] = BufInfo{io_off, elems * 4, DT_F32};
    io_off += rup(elems * 4, 256);
    return p;
  }
  Ptr cst(const void* data, int64_t bytes) {
    const int64_t off = rup((int64_t)P->consts.size(), 256);
    P->consts.resize(off + bytes);
    std::memcpy(P->consts.data() + off, data, bytes);
    return mk(A_CONST, off);
  }
  void add_param(const std::string& name, std::vector<int64_t> shape, bool trainable) {
    ParamInfo pi;
    pi.name = name;
    pi.shape = shape;
    pi.numel = 1;
    for (auto s : shape) pi.numel *= s;
    auto& vec = trainable ? P->params : P->state;
    pi.arena = trainable ? A_PARAM : A_STATE;
    pi.off = vec.empty() ? 0 : vec.back().off + vec.back().numel;
    (trainable ? pidx : sidx)[name] = (int)vec.size();
    vec.push_back(pi);
  }
  const ParamInfo& par(const std::string& n) const {
    auto it = pidx.find(n);
    if (it == pidx.end()) { P->error = "missing param " + n; static ParamInfo z; return z; }
    return P->params[it->second];
  }
  Ptr pptr(const std::string& n, int arena = A_PARAM) { return mk(arena, par(n).off * 4); }
  Ptr sptr(const std::string& n) { return mk(A_STATE, P->state[sidx.at(n)].off * 4); }

  int wg_rounds = 1;                                       // see wgrad(): row splits sized for this many dispatch rounds
  int cur_lane = 0;
  int cur_hold = 0;                                        // lane-1 ops pushed while set wait for the NEXT recurrence launch (kOpHold)
  Op& push(std::vector<Op>& v, int kind, int tag) {
    Op op;
    std::memset(&op, 0, sizeof(op));
    op.kind = kind;
    op.tag = tag;
    op.lane = cur_lane;
    if (cur_lane == 1 && cur_hold) op.join = kOpHold;
    v.push_back(op);
    return v.back();
  }

  static RunGemm gemm0() {
    RunGemm g;
    std::memset(&g, 0, sizeof(g));
    g.x[0].arena = g.x[1].arena = g.w.arena = g.bias.arena = g.y.arena = g.stats.arena = g.y2.arena = g.bnb_dz1.arena = g.bnb_totals.arena = A_NONE;
    g.nsplit = 1;
    return g;
  }
  // lay out run segments: assigns koff (padded to the K-tile of the operand dtype) and ldw
  static void layout_segs(RunGemm& g) {
    const int bk = bk_of(g.xdt);
    int k = 0;
    for (int s = 0; s < g.nseg; ++s) { g.seg[s].koff = k; k += (int)rup(g.seg[s].len, bk); }
    g.ldw = k;
    g.Npad = (int)rup(g.N, bn_of(g.N));
  }
  // Dense batch-major GEMM over the rows [B][T][rowlen] of x (DCCRN / CRN: B, T of the front end): columns [off, off + len) of every row
  // times an [N][len] matrix.  Anything else a site needs (a row index f, kRunAccum, a second source) it sets afterwards
  RunGemm rows_gemm(Ptr x, int xdt, int rowlen, int off, int len, int N, int ydt) const {
    RunGemm g = gemm0();
    g.x[0] = x; g.xdt = xdt; g.ydt = ydt;
    g.bstride[0] = (int64_t)fe.T * rowlen; g.tstride[0] = rowlen; g.rowlen[0] = rowlen; g.Tin[0] = fe.T;
    g.M = fe.B * fe.T; g.Tout = fe.T; g.Fo = 1;
    g.nseg = 1; g.seg[0] = Seg{0, 0, off, len, 0};
    g.N = N;
    layout_segs(g);
    return g;
  }
  // ... reading D slices `pitch` apart instead (the [D][Cl] rows of the encoder output): `len` columns from `off` of every slice
  static void rows_slices(RunGemm& g, int D, int pitch, int off, int len) {
    if (D > kMaxSeg) { std::fprintf(stderr, "sefd planner: rows_slices over %d > kMaxSeg runs (slice_chunks)\n", D); std::abort(); }
    g.nseg = D;
    for (int dd = 0; dd < D; ++dd) g.seg[dd] = Seg{0, 0, dd * pitch + off, len, 0};
    layout_segs(g);
  }
  // A descriptor holds kMaxSeg runs, so a recurrent input GEMM reads the D channel slices kMaxSeg at a time: slice_chunks(D) GEMMs, every one
  // after the first adding onto the first one's output (kRunAccum, no bias)
  static int slice_chunks(int D) { return (D + kMaxSeg - 1) / kMaxSeg; }
  // ... writing columns [yoff, yoff + N) of the rows [B][T][ld] of y
  void rows_out(RunGemm& g, Ptr y, int ld, int yoff = 0) const {
    g.y = y; g.y_bstride = (int64_t)fe.T * ld; g.y_tstride = ld; g.y_off = yoff;
  }

  using Coef = std::function<int32_t(int n, int seg, int j)>;   // signed 1-based flat param element, 0 = structural zero

  // PACK op for the weights of `g` (fills g.w), optional bias table (width 2) -> g.bias
  void pack_weights(std::vector<Op>& ops, RunGemm& g, const Coef& coef, const std::string& name, int tag,
                    const std::function<void(int n, int32_t out[2])>* bias = nullptr) {
    std::vector<int32_t> tab((size_t)g.Npad * g.ldw, 0);
    for (int n = 0; n < g.N; ++n)
      for (int s = 0; s < g.nseg; ++s)
        if (g.seg[s].src >= 0)
          for (int j = 0; j < g.seg[s].len; ++j) tab[(size_t)n * g.ldw + g.seg[s].koff + j] = coef(n, s, j);
    g.w = ws("w." + name, (int64_t)tab.size(), g.xdt);
    Op& op = push(ops, OP_PACK, tag);
    op.pack.tab = cst(tab.data(), (int64_t)tab.size() * 4);
    op.pack.src = mk(A_PARAM, 0);
    op.pack.dst = g.w;
    op.pack.n = (int64_t)tab.size();
    op.pack.ddt = g.xdt;
    op.pack.width = 1;
    if (bias) {
      std::vector<int32_t> bt((size_t)g.N * 2, 0);
      for (int n = 0; n < g.N; ++n) (*bias)(n, &bt[(size_t)n * 2]);
      g.bias = ws("b." + name, g.N, DT_F32);
      Op& ob = push(ops, OP_PACK, tag);
      ob.pack.tab = cst(bt.data(), (int64_t)bt.size() * 4);
      ob.pack.src = mk(A_PARAM, 0);
      ob.pack.dst = g.bias;
      ob.pack.n = g.N;
      ob.pack.ddt = DT_F32;
      ob.pack.width = 2;
    }
  }

  // Fused FFT STFT (stft_fft.hip) for fft_len == 512: frame t reads src[t*hop - off + j] * win[j], j < W.  Returns false
  // (caller plans the framing GEMM instead) for other transform sizes.
  bool stft_fft(std::vector<Op>& ops, int tag, Ptr src, Ptr spec, int B, int L, int T, int hop, int off, int NFFT,
                const std::vector<double>& win) {
    if (NFFT != 512 || (int)win.size() > 512 || tune_has("STFT_GEMM")) return false;
    if (fft_tw.arena < 0) {
      std::vector<float> tw(1024);
      for (int k = 0; k < 512; ++k) { tw[2 * k] = (float)std::cos(2.0 * kPi * k / 512.0); tw[2 * k + 1] = (float)std::sin(2.0 * kPi * k / 512.0); }
      fft_tw = cst(tw.data(), 4096);
    }
    std::vector<float> wf(512, 0.f);
    for (size_t j = 0; j < win.size(); ++j) wf[j] = (float)win[j];
    Op& op = push(ops, OP_STFT_FFT, tag);
    op.fft.src = src; op.fft.spec = spec; op.fft.tw = fft_tw; op.fft.win = cst(wf.data(), 2048);
    op.fft.B = B; op.fft.L = L; op.fft.T = T; op.fft.hop = hop; op.fft.off = off; op.fft.lp_dt = 0;
    op.fft.corr = none(); op.fft.scale = 1.f; op.fft.lp = none(); op.fft.pair = fft_pair();
    return true;
  }
  // two frames per transform in the bf16 plans only (stft_fft.hip); STFT_PAIR=0 / 1 forces one form (A/B runs)
  int fft_pair() const { return tune_int("STFT_PAIR", c.act_dtype == DT_BF16) != 0; }
  Ptr fft_tw = Ptr{-1, 0, 0};
  Ptr fft_corr = Ptr{-1, 0, 0};
  // rank-2 correction of the closed-form pinv synthesis basis: cE/cO[part][k] = sum over even/odd j < W of the
  // un-windowed analysis basis, divided by (NFFT/2 + number of such j)
  Ptr istft_corr(int W) {
    if (fft_corr.arena >= 0) return fft_corr;
    std::vector<float> c(4 * 257, 0.f);
    const double ne = (W + 1) / 2, no = W / 2;
    for (int part = 0; part < 2; ++part)
      for (int k = 0; k <= 256; ++k) {
        double se = 0, so = 0;
        for (int m = 0; m < W; ++m) {
          const double ang = 2.0 * kPi * (double)(((int64_t)k * m) % 512) / 512.0;
          (m % 2 == 0 ? se : so) += part == 0 ? std::cos(ang) : -std::sin(ang);
        }
        c[(0 * 2 + part) * 257 + k] = (float)(se / (256.0 + ne));
        c[(1 * 2 + part) * 257 + k] = (float)(so / (256.0 + no));
      }
    fft_corr = cst(c.data(), (int64_t)c.size() * 4);
    return fft_corr;
  }
  Ptr win512(const std::vector<double>& win) {
    std::vector<float> wf(512, 0.f);
    for (size_t j = 0; j < win.size(); ++j) wf[j] = (float)win[j];
    return cst(wf.data(), 2048);
  }
  // iSTFT synthesis est -> frames as an inverse FFT (istft_fft_kernel); false: plan the synthesis GEMM instead
  bool istft_fft(std::vector<Op>& ops, int tag, Ptr est, Ptr frames, int64_t nframes, int NFFT, const std::vector<double>& win) {
    if (NFFT != 512 || (int)win.size() > 512 || tune_has("STFT_GEMM")) return false;
    if (fft_tw.arena < 0) return false;                      // the STFT helper creates the twiddle table first
    Op& op = push(ops, OP_ISTFT_FFT, tag);
    op.ifft.est = est; op.ifft.frames = frames; op.ifft.tw = fft_tw; op.ifft.win = win512(win); op.ifft.corr = istft_corr((int)win.size());
    op.ifft.nframes = nframes; op.ifft.W = (int)win.size();
    return true;
  }
  // its backward: d est = Kinv . (frames of the padded waveform gradient) = the analysis transform with the same correction
  bool istft_bwd_fft(std::vector<Op>& ops, int tag, Ptr dpad, Ptr dest, int B, int Lp, int T, int hop, int NFFT, const std::vector<double>& win) {
    if (NFFT != 512 || (int)win.size() > 512 || tune_has("STFT_GEMM") || fft_tw.arena < 0) return false;
    Op& op = push(ops, OP_STFT_FFT, tag);
    op.fft.src = dpad; op.fft.spec = dest; op.fft.tw = fft_tw; op.fft.win = win512(win);
    op.fft.B = B; op.fft.L = Lp; op.fft.T = T; op.fft.hop = hop; op.fft.off = 0; op.fft.lp_dt = 0;
    op.fft.corr = istft_corr((int)win.size()); op.fft.scale = 1.f / 256.f; op.fft.lp = none(); op.fft.pair = fft_pair();
    return true;
  }

  // ---- the ConvSTFT front end (fe) and its inverse
  Stft fe;
  Ptr ana_w = Ptr{-1, 0, 0};                               // analysis GEMM weights (shared by every STFT of the plan)
  // synthesis basis = pinv(K_unwindowed)^T * w, closed form: K^T K = (NFFT/2) I + E, E[n][m] = [n-m even]
  //   pinv(K)[j][r] = (K[r][j] - sum_{m == j mod 2} K[r][m] / (NFFT/2 + |{m == j mod 2}|)) / (NFFT/2)
  // and the OLA normaliser (constant c_coff)
  void synthesis() {
    const int W = fe.W, NF = fe.NF, NFFT = fe.NFFT;
    fe.Kinv.assign((size_t)2 * NF * W, 0.0);
    const double ne = (W + 1) / 2, no = W / 2;
    for (int part = 0; part < 2; ++part)
      for (int k = 0; k < NF; ++k) {
        double se = 0, so = 0;
        for (int m = 0; m < W; ++m) (m % 2 == 0 ? se : so) += fe.Kun(part, k, m);
        for (int j = 0; j < W; ++j) {
          const double corr = (j % 2 == 0) ? se / (NFFT / 2.0 + ne) : so / (NFFT / 2.0 + no);
          fe.Kinv[((size_t)part * NF + k) * W + j] = (fe.Kun(part, k, j) - corr) / (NFFT / 2.0) * fe.win[j];
        }
      }
    std::vector<float> coff(fe.Lp, 0.f), w2(W);
    for (int j = 0; j < W; ++j) { const float wf = (float)fe.win[j]; w2[j] = wf * wf; }
    for (int t = 0; t < fe.T; ++t)
      for (int j = 0; j < W; ++j) coff[t * fe.hop + j] += w2[j];
    fe.c_coff = cst(coff.data(), (int64_t)coff.size() * 4);
  }
  // constant (fp32) weights of a single-run GEMM: w[n][j] = val(n, j)
  void const_weights(RunGemm& g, const std::function<double(int n, int j)>& val) {
    std::vector<float> wt((size_t)g.Npad * g.ldw, 0.f);
    for (int nn = 0; nn < g.N; ++nn)
      for (int j = 0; j < g.seg[0].len; ++j) wt[(size_t)nn * g.ldw + j] = (float)val(nn, j);
    g.w = cst(wt.data(), (int64_t)wt.size() * 4);
  }
  // STFT (ConvSTFT.forward, tools_for_model.py:54-61) wav [B][L] -> spec [B*T][SW]: the fused FFT, else the framing GEMM.  True: FFT
  bool stft_fwd(std::vector<Op>& ops, int tag, Ptr wav, Ptr spec) {
    if (stft_fft(ops, tag, wav, spec, fe.B, fe.L, fe.T, fe.hop, fe.trim, fe.NFFT, fe.win)) return true;
    RunGemm g = gemm0();
    g.x[0] = wav; g.xdt = DT_F32; g.ydt = DT_F32;
    g.bstride[0] = fe.L; g.rowlen[0] = fe.L; g.fstride[0] = fe.hop; g.Tin[0] = 1;
    g.M = fe.B * fe.T; g.Tout = 1; g.Fo = fe.T;
    g.nseg = 1; g.seg[0] = Seg{0, 0, -fe.trim, fe.W, 0};
    g.N = fe.SW;
    layout_segs(g);
    if (ana_w.arena < 0) {
      const_weights(g, [&](int nn, int j) { return nn < 2 ? 0.0 : fe.Kun(nn & 1, nn / 2 - 1, j) * fe.win[j]; });
      ana_w = g.w;
    }
    g.w = ana_w;
    g.y = spec; g.y_bstride = (int64_t)fe.T * fe.SW; g.y_fstride = fe.SW;
    push(ops, OP_RUNGEMM, tag).g = g;
    return false;
  }
  // iSTFT (ConviSTFT.forward) est [B*T][SW] -> frames [B*T][W] (inverse FFT, else the synthesis GEMM), then the overlap-add into wav
  Ola istft_ola(std::vector<Op>& ops, Ptr est, Ptr frames, Ptr wav) {
    const int64_t BT = (int64_t)fe.B * fe.T;
    if (!istft_fft(ops, 501, est, frames, BT, fe.NFFT, fe.win)) {
      RunGemm g = gemm0();
      g.x[0] = est; g.xdt = DT_F32; g.ydt = DT_F32;
      g.bstride[0] = (int64_t)fe.T * fe.SW; g.tstride[0] = fe.SW; g.rowlen[0] = fe.SW; g.Tin[0] = fe.T;
      g.M = (int)BT; g.Tout = fe.T; g.Fo = 1;
      g.nseg = 1; g.seg[0] = Seg{0, 0, 0, fe.SW, 0};
      g.N = fe.W;
      layout_segs(g);
      const int NF = fe.NF, W = fe.W;
      const_weights(g, [&](int nn, int j) { return j < 2 ? 0.0 : fe.Kinv[((size_t)(j & 1) * NF + (j / 2 - 1)) * W + nn]; });
      g.y = frames; g.y_bstride = (int64_t)fe.T * W; g.y_tstride = W;
      push(ops, OP_RUNGEMM, 501).g = g;
    }
    Ola ola;
    std::memset(&ola, 0, sizeof(ola));
    ola.frames = frames; ola.wav = wav; ola.coff = fe.c_coff; ola.dwav = ola.dpad = none();
    ola.B = fe.B; ola.T = fe.T; ola.L = fe.L; ola.win = fe.W; ola.hop = fe.hop; ola.trim = fe.trim;
    if (fe.Lp - 2 * fe.trim < fe.L) ola.Lout = fe.Lp - 2 * fe.trim;      // ConviSTFT's `[..., trim:-trim]` of the frames' span (tools_for_model.py:111)
    push(ops, OP_OLA_FWD, 502).ola = ola;
    return ola;
  }
  // their backward: the overlap-add's (dwav -> dpad), then the iSTFT's (dpad -> the returned dest [B*T][SW])
  Ptr istft_ola_bwd(std::vector<Op>& ops, const Ola& ola, Ptr dwav) {
    const int64_t BT = (int64_t)fe.B * fe.T;
    Ptr dpad = ws("dpad", (int64_t)fe.B * fe.Lp, DT_F32);
    Ptr dest = ws("dest", BT * fe.SW, DT_F32);
    Ola o = ola;
    o.dwav = dwav; o.dpad = dpad;
    push(ops, OP_OLA_BWD, 502).ola = o;
    if (!istft_bwd_fft(ops, 501, dpad, dest, fe.B, fe.Lp, fe.T, fe.hop, fe.NFFT, fe.win)) {
      RunGemm g = gemm0();
      g.x[0] = dpad; g.xdt = DT_F32; g.ydt = DT_F32;
      g.bstride[0] = fe.Lp; g.rowlen[0] = fe.Lp; g.fstride[0] = fe.hop; g.Tin[0] = 1;
      g.M = (int)BT; g.Tout = 1; g.Fo = fe.T;
      g.nseg = 1; g.seg[0] = Seg{0, 0, 0, fe.W, 0};
      g.N = fe.SW;
      layout_segs(g);
      const int NF = fe.NF, W = fe.W;
      const_weights(g, [&](int nn, int j) { return nn < 2 ? 0.0 : fe.Kinv[((size_t)(nn & 1) * NF + (nn / 2 - 1)) * W + j]; });
      g.y = dest; g.y_bstride = (int64_t)fe.T * fe.SW; g.y_fstride = fe.SW;
      push(ops, OP_RUNGEMM, 501).g = g;
    }
    return dest;
  }

  // ---- the conv stack shared by the DCCRN (complex convs as block-real GEMMs) and CRN (real convs) planners
  using Bias = std::function<void(int n, int32_t out[2])>;
  struct ActSrc { Ptr p; int64_t bstride; int tstride, base, C; };      // channels-last activation: batch / frame strides, first element, channels
  // one conv layer: forward descriptor(s) (decoder: one per sub-pixel phase) with their coefficient and bias functions, activations
  // (y conv output, z BatchNorm + PReLU output, mi its statistics), C channels, Fq frequency bins, R BatchNorm rows; gradient buffers
  struct ConvLayer { RunGemm f[2]; Coef coef[2]; Bias bias; Ptr y, z, mi, dy, dz, dskip; int C, Fq; int64_t R; };

  // BatchNorm2d + PReLU forward of a conv layer (parameters <pp>.1 / <pp>.2): y -> z.  Training: batch statistics from nblk partial rows
  // of pitch Cpad in `part` (nsub > 0: each row holds nsub sub-pixel phases substride columns apart)
  // more than kBnMaxC channels: refused - bn.hip's LDS arrays hold no more (every launch of the layer would write past them)
  bool bn_fits(const std::string& pp, int C) {
    if (C <= kBnMaxC) return true;
    if (P->error.empty())
      P->error = "BatchNorm2d: at most " + std::to_string(kBnMaxC) + " channels per layer (bn.hip stages a layer's parameters in LDS): " + pp + " has " + std::to_string(C);
    return false;
  }
  void bn_fwd(std::vector<Op>& ops, int tag, const std::string& pp, const ConvLayer& Ly, Ptr part, int nblk, int Cpad, int nsub, int substride) {
    if (!bn_fits(pp, Ly.C)) return;
    Op& op = push(ops, OP_BN_FINALIZE, tag);
    op.bnf.part = part; op.bnf.mean_invstd = Ly.mi;
    op.bnf.running_mean = sptr(pp + ".1.running_mean"); op.bnf.running_var = sptr(pp + ".1.running_var");
    op.bnf.nblk = c.training ? nblk : -1; op.bnf.C = Ly.C; op.bnf.Cpad = Cpad; op.bnf.count = (double)Ly.R;
    op.bnf.nsub = nsub; op.bnf.substride = substride;
    op.bnf.eps = 1e-5f; op.bnf.momentum = 0.1f;
    Op& oa = push(ops, OP_BN_APPLY, tag);
    oa.bna.y = Ly.y; oa.bna.z = Ly.z; oa.bna.mean_invstd = Ly.mi;
    oa.bna.gamma = pptr(pp + ".1.weight"); oa.bna.beta = pptr(pp + ".1.bias"); oa.bna.slope = pptr(pp + ".2.weight");
    oa.bna.R = Ly.R; oa.bna.C = Ly.C; oa.bna.dt = c.act_dtype;
  }
  // Encoder conv (kernel KS x 2 over (frequency, time), frequency stride 2, frames t-1 and t) over the channels-last input x (coef / bias
  // map its channels to parameters, zero for pad channels): packed weights, RUNGEMM into <nm>.y, then with `bn` BatchNorm + PReLU into
  // <nm>.z.  enc0: DCCRN's first layer reading the fp32 spectrum itself (kRunEnc0, enc0.hip)
  ConvLayer enc_conv(std::vector<Op>& ops, int tag, const std::string& nm, const std::string& pp, const ActSrc& x, int Fi, int Fo, int Co,
                     const Coef& coef, const Bias& bias, bool bn, bool enc0) {
    const int adt = c.act_dtype, KS = c.kernel_size, T = fe.T;
    ConvLayer Ly{};
    RunGemm g = gemm0();
    g.x[0] = x.p;
    g.xdt = enc0 ? DT_F32 : adt;
    g.ydt = adt;
    if (enc0) g.flags |= kRunEnc0;
    g.bstride[0] = x.bstride; g.tstride[0] = x.tstride; g.base[0] = x.base;
    g.rowlen[0] = Fi * x.C; g.fstride[0] = 2 * x.C; g.Tin[0] = T;
    g.M = fe.B * T * Fo; g.Tout = T; g.Fo = Fo;
    g.nseg = 2;
    g.seg[0] = Seg{0, -1, -2 * x.C, KS * x.C, 0};   // kw = 0 : frame t-1
    g.seg[1] = Seg{0, 0, -2 * x.C, KS * x.C, 0};    // kw = 1 : frame t
    g.N = Co;
    layout_segs(g);
    pack_weights(ops, g, coef, nm, tag, &bias);
    Ly.C = Co; Ly.Fq = Fo; Ly.R = (int64_t)fe.B * T * Fo;
    Ly.y = ws(nm + ".y", Ly.R * Co, adt);
    Ly.z = ws(nm + ".z", Ly.R * Co, adt);
    Ly.mi = ws(nm + ".mi", 2 * Co, DT_F32);
    const int nblk = (int)((g.M + kBM - 1) / kBM);
    Ptr part = ws(nm + ".stat", (int64_t)nblk * 2 * g.Npad, DT_F32);
    g.y = Ly.y; g.y_bstride = (int64_t)T * Fo * Co; g.y_tstride = Fo * Co; g.y_fstride = Co; g.y_off = 0;
    g.stats = c.training && bn ? part : none();
    push(ops, OP_RUNGEMM, tag).g = g;
    if (bn) bn_fwd(ops, tag, pp, Ly, part, nblk, g.Npad, 0, 0);
    Ly.f[0] = g; Ly.coef[0] = coef; Ly.bias = bias;
    return Ly;
  }
  // Decoder transposed conv (kernel KS x 2, frequency stride 2; Ly.y keeps the extra frame that `[..., 1:]` drops) as two sub-pixel phase
  // GEMMs over src[0] (previous layer) and, with skips, src[1]: phase 0 = output bins 2f (taps kh = 4, 2, 0 over input bins f-1, f, f+1),
  // phase 1 = bins 2f+1 (kh = 3, 1 over bins f, f+1).  wcoef(n, source, channel, kh, kw); N output columns ([phase][N] per input bin);
  // stats: BatchNorm partial rows, nblk1 per phase (none: no statistics).  pack = false: descriptors and coefficients only
  using WCoef = std::function<int32_t(int n, int s, int cc, int kh, int kw)>;
  void dec_phases(std::vector<Op>& ops, int tag, const std::string& nm, ConvLayer& Ly, const std::array<ActSrc, 2>& src, int Fi, int N,
                  const WCoef& wcoef, Ptr stats, int nblk1, bool pack) {
    const int adt = c.act_dtype, T = fe.T, Fo = 2 * Fi, nsrc = c.skip ? 2 : 1;
    for (int par = 0; par < 2; ++par) {
      RunGemm g = gemm0();
      g.xdt = adt; g.ydt = adt;
      g.nseg = 0;
      const int ntap = par == 0 ? 3 : 2;
      for (int s = 0; s < nsrc; ++s) {
        g.x[s] = src[s].p; g.bstride[s] = src[s].bstride; g.tstride[s] = src[s].tstride; g.base[s] = src[s].base;
        g.rowlen[s] = Fi * src[s].C; g.fstride[s] = src[s].C; g.Tin[s] = T;
        for (int kw = 0; kw < 2; ++kw) g.seg[g.nseg++] = Seg{s, -kw, par == 0 ? -src[s].C : 0, ntap * src[s].C, 0};
      }
      g.M = fe.B * (T + 1) * Fi; g.Tout = T + 1; g.Fo = Fi;
      g.N = N;
      layout_segs(g);
      const int c0 = src[0].C, c1 = src[1].C;
      Coef coef = [=](int nn, int sg, int j) -> int32_t {
        const int s = sg / 2, kw = sg % 2;
        const int Cs = s == 0 ? c0 : c1;
        const int jj = j / Cs, cc = j % Cs;
        return wcoef(nn, s, cc, par == 0 ? 4 - 2 * jj : 3 - 2 * jj, kw);
      };
      Ly.coef[par] = coef;
      if (!pack) { Ly.f[par] = g; continue; }
      pack_weights(ops, g, coef, nm + ".p" + std::to_string(par), tag, par == 0 ? &Ly.bias : nullptr);
      if (par == 1) g.bias = Ly.f[0].bias;
      g.y = Ly.y; g.y_bstride = (int64_t)(T + 1) * Fo * N; g.y_tstride = Fo * N; g.y_fstride = 2 * N; g.y_off = par * N;
      if (stats.arena >= 0) g.stats = mk(A_WS, stats.off + (int64_t)par * nblk1 * 2 * g.Npad * 4);
      push(ops, OP_RUNGEMM, tag).g = g;
      Ly.f[par] = g;
    }
  }
  // gradient buffers of the conv stack (the mask layer's dy has mask_ch channels)
  void conv_grads(std::vector<ConvLayer>& enc, std::vector<ConvLayer>& dec, int mask_ch) {
    const int n = (int)enc.size(), adt = c.act_dtype, B = fe.B, T = fe.T;
    for (int d = 0; d < n; ++d) {
      const int Co = d == n - 1 ? mask_ch : dec[d].C, Fo = dec[d].Fq;
      dec[d].dy = ws("dec" + std::to_string(d) + ".dy", (int64_t)B * (T + 1) * Fo * Co, adt);
      if (d != n - 1) dec[d].dz = ws("dec" + std::to_string(d) + ".dz", (int64_t)B * T * Fo * Co, adt);
    }
    for (int i = 0; i < n; ++i) {
      const int64_t e = (int64_t)B * T * enc[i].Fq * enc[i].C;
      enc[i].dy = ws("enc" + std::to_string(i) + ".dy", e, adt);
      enc[i].dz = ws("enc" + std::to_string(i) + ".dz", e, adt);
      if (c.skip) enc[i].dskip = ws("enc" + std::to_string(i) + ".dskip", e, adt);
    }
  }
  // DCCRN: BatchNorm backward partial rows left by the epilogues of the GEMMs that produce a layer's dz (kRunBnBwd)
  struct BnbAcc { Ptr part; int rows = 0, cap = 0, ldp = 0; bool on = false; Ptr y, mi; std::string pp; };
  // BatchNorm2d + PReLU backward of a conv layer: dz0 (+ dz1, the skip connection's) -> dy and the parameter gradients; rpb rows per
  // batch item, the first `skip` of them not in dz.  DCCRN only: cbn = ComplexBatchNorm (mi = its coefficient table), fused = the
  // producers' epilogues wrote the partial rows, no_apply = no BN_BWD_APPLY.  Returns the BN_BWD_FINALIZE descriptor.
  BnBwdApply bn_bwd(std::vector<Op>& R, int tag, Ptr y, Ptr dz0, Ptr dz1, Ptr mi, const std::string& pp, int C, int64_t Rr, int64_t rpb,
                    int skip, Ptr dy, const std::string& nm, bool cbn, const BnbAcc* fused, bool no_apply) {
    const int adt = c.act_dtype;
    int64_t rpbk = std::max<int64_t>(64, (Rr + 2047) / 2048);
    const int nblk = (int)((Rr + rpbk - 1) / rpbk);
    BnBwdApply a;
    std::memset(&a, 0, sizeof(a));
    if (cbn) {
      const int h = C / 2;
      CbnBwd cb;
      std::memset(&cb, 0, sizeof(cb));
      cb.y = y; cb.dz0 = dz0; cb.dz1 = dz1; cb.dy = dy; cb.coef = mi;
      cb.coefb = ws(nm + ".ccoefb", 9 * h, DT_F32);
      cb.part = ws(nm + ".cbnpart", (int64_t)nblk * 7 * h, DT_F32);
      const char* wn[3] = {"Wrr", "Wri", "Wii"};
      for (int q = 0; q < 3; ++q) { cb.W[q] = pptr(pp + ".1." + wn[q]); cb.dW[q] = pptr(pp + ".1." + wn[q], A_GRAD); }
      cb.dB[0] = pptr(pp + ".1.Br", A_GRAD); cb.dB[1] = pptr(pp + ".1.Bi", A_GRAD);
      cb.slope = pptr(pp + ".2.weight"); cb.dslope = pptr(pp + ".2.weight", A_GRAD);
      cb.R = Rr; cb.rpb = rpb; cb.C = C; cb.dt = adt; cb.nblk = nblk; cb.rows_per_blk = (int)rpbk; cb.skip = skip; cb.count = (double)Rr;
      push(R, OP_CBN_BWD_REDUCE, tag).cbb = cb;
      push(R, OP_CBN_BWD_FINALIZE, tag).cbb = cb;
      push(R, OP_CBN_BWD_APPLY, tag).cbb = cb;
      return a;
    }
    if (!bn_fits(pp, C)) return a;
    BnBwdReduce r;
    std::memset(&r, 0, sizeof(r));
    r.y = y; r.dz0 = dz0; r.dz1 = dz1; r.mean_invstd = mi;
    r.gamma = pptr(pp + ".1.weight"); r.beta = pptr(pp + ".1.bias"); r.slope = pptr(pp + ".2.weight");
    r.R = Rr; r.C = C; r.dt = adt; r.nblk = nblk; r.rows_per_blk = (int)rpbk; r.rpb = rpb; r.skip = skip;
    if (fused && fused->on) {                   // the producers' epilogues wrote the partial rows
      r.part = fused->part; r.nblk = fused->rows; r.ldp = fused->ldp;
    } else {
      r.part = ws(nm + ".bnpart", (int64_t)nblk * 3 * C, DT_F32);
      push(R, OP_BN_BWD_REDUCE, tag).bnr = r;
    }
    a.r = r; a.totals = ws(nm + ".bntot", 3 * C, DT_F32); a.dy = dy;
    a.dgamma = pptr(pp + ".1.weight", A_GRAD); a.dbeta = pptr(pp + ".1.bias", A_GRAD); a.dslope = pptr(pp + ".2.weight", A_GRAD);
    a.count = (double)Rr;
    push(R, OP_BN_BWD_FINALIZE, tag).bnb = a;
    if (!no_apply) push(R, OP_BN_BWD_APPLY, tag).bnb = a;
    return a;
  }
  // Input gradient of decoder source s (Cs channels) as a conv over Ly.dy [B][T+1][Fo][Co] (Co: its buffer channels), read off the
  // forward phases' coefficients: dx[ci,f,t] = sum W[ci,co,kh,kw] dy[co, 2f+kh-2, t+kw] into dx [B][T][Fi][Cs].  Packed unless `pack` is
  // false; not pushed
  RunGemm dec_dgrad(std::vector<Op>& ops, int tag, const std::string& nm, const ConvLayer& Ly, int Co, int Fi, int s, int Cs, Ptr dx,
                    Coef& coef, bool pack) {
    const int adt = c.act_dtype, KS = c.kernel_size, T = fe.T, Fo = 2 * Fi;
    RunGemm g = gemm0();
    g.x[0] = Ly.dy; g.xdt = adt; g.ydt = adt;
    g.bstride[0] = (int64_t)(T + 1) * Fo * Co; g.tstride[0] = Fo * Co; g.base[0] = 0; g.rowlen[0] = Fo * Co; g.fstride[0] = 2 * Co; g.Tin[0] = T + 1;
    g.M = fe.B * T * Fi; g.Tout = T; g.Fo = Fi;
    g.nseg = 2;
    g.seg[0] = Seg{0, 0, -2 * Co, KS * Co, 0};    // kw = 0 : buffer frame u = t
    g.seg[1] = Seg{0, 1, -2 * Co, KS * Co, 0};    // kw = 1 : buffer frame u = t + 1
    g.N = Cs;
    layout_segs(g);
    // d y[co] / d x[(s,cc)] is the forward coefficient of phase (kh odd) at tap jj: look it up in the forward tables
    const Coef f0 = Ly.coef[0], f1 = Ly.coef[1];
    coef = [=](int nn, int sg, int j) -> int32_t {
      const int kw = sg, kh = j / Co, co = j % Co;
      const int par = kh & 1;
      const int jj = par == 0 ? (4 - kh) / 2 : (3 - kh) / 2;
      return (par == 0 ? f0 : f1)(co, s * 2 + kw, jj * Cs + nn);
    };
    if (pack) pack_weights(ops, g, coef, nm + ".dg" + std::to_string(s), tag);
    g.y = dx; g.y_bstride = (int64_t)T * Fi * Cs; g.y_tstride = Fi * Cs; g.y_fstride = Cs; g.y_off = 0;
    return g;
  }
  // Input gradient of encoder layer Ly (Ci input channels, Fi input bins): dx[ci,f,t] = sum W[co,ci,kh,kw] dy[co,(f+2-kh)/2, t+1-kw] as
  // sub-pixel phase `par` over Ly.dy [B][T][Fo][Co], writing bins 2f+par of dx [B][T][Fi][Ci].  Packed, not pushed
  RunGemm enc_dgrad(std::vector<Op>& ops, int tag, const std::string& nm, const ConvLayer& Ly, int Ci, int Fi, int par, Ptr dx) {
    const int adt = c.act_dtype, T = fe.T, Co = Ly.C, Fo = Ly.Fq;
    RunGemm g = gemm0();
    g.x[0] = Ly.dy; g.xdt = adt; g.ydt = adt;
    g.bstride[0] = (int64_t)T * Fo * Co; g.tstride[0] = Fo * Co; g.rowlen[0] = Fo * Co; g.fstride[0] = Co; g.Tin[0] = T;
    g.M = fe.B * T * Fo; g.Tout = T; g.Fo = Fo;           // Fi/2 == Fo output rows per phase
    const int ntap = par == 0 ? 3 : 2;
    g.nseg = 2;
    g.seg[0] = Seg{0, 1, par == 0 ? -Co : 0, ntap * Co, 0};   // kw = 0 : frame t+1
    g.seg[1] = Seg{0, 0, par == 0 ? -Co : 0, ntap * Co, 0};   // kw = 1 : frame t
    g.N = Ci;
    layout_segs(g);
    const Coef cf = Ly.coef[0];
    Coef coef = [=](int nn, int sg, int j) -> int32_t {
      const int kw = sg, jj = j / Co, co = j % Co;
      const int kh = par == 0 ? 4 - 2 * jj : 3 - 2 * jj;
      return cf(co, kw, kh * Ci + nn);
    };
    pack_weights(ops, g, coef, nm + ".dg" + std::to_string(par), tag);
    g.y = dx; g.y_bstride = (int64_t)T * Fi * Ci; g.y_tstride = Fi * Ci; g.y_fstride = 2 * Ci; g.y_off = par * Ci;
    return g;
  }

  // ---- the recurrent block shared by DCCRN with cfg.lstm == 'real' (two layers) and CRN (one): nn.LSTM layers over the encoder output
  // [B][T][D][Cl] in the reference's feature order c*D + d (models.py:214-218; a weight permutation here), then a Linear into the decoder input
  struct Rnn { int D = 0, Cl = 0, H = 0; bool stepped = false; } rnn;   // stepped: one GEMM + one cell launch per frame instead of the persistent kernels
  // what the backward of a layer needs from its forward: buffers, the input GEMM with its coefficient and bias functions, W_hh
  // (gxc / cgxc: the input GEMM per chunk of channel slices with its coefficient function - one chunk unless layer 0 reads more than kMaxSeg slices)
  struct RealLstm { std::string nm; int l; RunGemm gx; Coef cgx; Bias bgx; Ptr gxb, h, gates, cst; const ParamInfo* Whh; std::vector<RunGemm> gxc; std::vector<Coef> cgxc; };
  void real_cell(LstmCell& cl, const RealLstm& Lr, int t, bool fwd, Ptr dh, Ptr dcb, Ptr dgates) {
    const int adt = c.act_dtype, H = rnn.H, T = fe.T;
    cl.gates = mk(A_WS, Lr.gxb.off + (int64_t)t * 4 * H * 4);
    cl.c = mk(A_WS, Lr.cst.off + (int64_t)t * H * 4);
    cl.c_prev = t > 0 ? mk(A_WS, Lr.cst.off + (int64_t)(t - 1) * H * 4) : none();
    cl.h = fwd ? mk(A_WS, Lr.h.off + (int64_t)t * H * esize(adt)) : none();
    cl.dh = fwd ? none() : mk(A_WS, dh.off + (int64_t)t * H * 4);
    cl.dc = fwd ? none() : dcb;
    cl.dgates = fwd ? none() : mk(A_WS, dgates.off + (int64_t)t * 4 * H * esize(adt));
    cl.rows = fe.B; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = fwd ? t == 0 : t == T - 1;
    cl.G = 1; cl.Bg = fe.B; cl.unit_major = 1;
    cl.rs[0] = (int64_t)T * 4 * H; cl.rs[1] = cl.rs[2] = cl.rs[3] = (int64_t)T * H; cl.rs[4] = (int64_t)T * 4 * H;
  }
  // the persistent recurrence of a layer (backward: with dh and dgates)
  void real_rec(LstmRec& r, const RealLstm& Lr, Ptr dh, Ptr dgates, int gdt) {
    std::memset(&r, 0, sizeof(r));
    r.gx = Lr.gxb; r.whh[0] = r.whh[1] = pptr(Lr.Whh->name);
    r.h = Lr.h; r.gates = Lr.gates; r.c = Lr.cst; r.dh = dh; r.dgates = dgates;
    r.gx_ld = 4 * rnn.H; r.G = 1; r.nset = 1; r.B = fe.B; r.T = fe.T; r.H = rnn.H; r.hdt = c.act_dtype; r.gdt = gdt;
  }
  // Forward of layer l (parameters enhance.*_l<l>, buffers and packs <nm>.*) over x: the encoder output (l == 0) or the layer below's h.
  // gdt: gate dtype of the forward recurrence descriptor
  RealLstm real_lstm_fwd(std::vector<Op>& ops, const std::string& nm, int l, Ptr x, int gdt) {
    const int adt = c.act_dtype, B = fe.B, T = fe.T, D = rnn.D, Cl = rnn.Cl, H = rnn.H, tag = 200 + l;
    const int64_t BT = (int64_t)B * T;
    const std::string sl = std::to_string(l);
    const ParamInfo *Wih = &par("enhance.weight_ih_l" + sl), *Whh = &par("enhance.weight_hh_l" + sl);
    const ParamInfo *bih = &par("enhance.bias_ih_l" + sl), *bhh = &par("enhance.bias_hh_l" + sl);
    RealLstm Lr;
    Lr.nm = nm; Lr.l = l; Lr.Whh = Whh;
    Lr.gxb = ws(nm + ".gx", BT * 4 * H, DT_F32);
    Lr.h = ws(nm + ".h", BT * H, adt);
    Lr.gates = ws(nm + ".gates", BT * 4 * H, DT_F32);
    Lr.cst = ws(nm + ".c", BT * H, DT_F32);
    const int I = l == 0 ? D * Cl : H;
    Lr.cgx = [=](int nn, int sg, int j) -> int32_t { return pe(*Wih, (int64_t)gate_torch_row(nn, H) * I + (l == 0 ? j * D + sg : j), 1); };
    Lr.bgx = [=](int nn, int32_t* o) { o[0] = pe(*bih, gate_torch_row(nn, H), 1); o[1] = pe(*bhh, gate_torch_row(nn, H), 1); };
    for (int ck = 0; ck < (l == 0 ? slice_chunks(D) : 1); ++ck) {
      const int d0 = ck * kMaxSeg;
      RunGemm g = rows_gemm(x, adt, I, 0, I, 4 * H, DT_F32);
      if (l == 0) rows_slices(g, std::min(kMaxSeg, D - d0), Cl, d0 * Cl, Cl);
      const Coef cf = Lr.cgx;
      const Coef cc = ck == 0 ? cf : Coef([=](int nn, int sg, int j) -> int32_t { return cf(nn, sg + d0, j); });
      pack_weights(ops, g, cc, nm + ".ih" + (ck ? "_" + std::to_string(ck) : ""), tag, ck == 0 ? &Lr.bgx : nullptr);
      if (ck) g.flags |= kRunAccum;
      rows_out(g, Lr.gxb, 4 * H);
      push(ops, OP_RUNGEMM, tag).g = g;
      Lr.gxc.push_back(g); Lr.cgxc.push_back(cc);
    }
    Lr.gx = Lr.gxc[0];
    if (!rnn.stepped) {
      real_rec(push(ops, OP_LSTM_FWD, tag).lstm, Lr, none(), none(), gdt);
      return Lr;
    }
    // per frame: gx[t] += h[t-1] . W_hh^T over the B rows of that frame, then the cell (gx is overwritten in place by the gates i,f,g,o)
    RunGemm hg = gemm0();
    hg.x[0] = Lr.h; hg.xdt = adt; hg.ydt = DT_F32;
    hg.fstride[0] = T * H; hg.rowlen[0] = (int)(BT * H); hg.Tin[0] = 1;
    hg.M = B; hg.Tout = 1; hg.Fo = B;
    hg.nseg = 1; hg.seg[0] = Seg{0, 0, 0, H, 0};
    hg.N = 4 * H;
    layout_segs(hg);
    Coef chh = [=](int nn, int sg, int j) -> int32_t { return pe(*Whh, (int64_t)gate_torch_row(nn, H) * H + j, 1); };
    pack_weights(ops, hg, chh, nm + ".hh", tag);
    hg.y = Lr.gxb; hg.y_fstride = T * 4 * H; hg.flags = kRunAccum;
    for (int t = 0; t < T; ++t) {
      if (t > 0) {
        RunGemm q = hg;
        q.base[0] = (t - 1) * H;
        q.y_off = t * 4 * H;
        push(ops, OP_RUNGEMM, tag).g = q;
      }
      real_cell(push(ops, OP_CELL_FWD, tag).cell, Lr, t, true, none(), none(), none());
    }
    return Lr;
  }
  // Its backward from dh [B][T][H] (fp32): dgates, both weight gradients, and the input gradient - layer 0: D channel slices of the
  // encoder-output gradient dx [B][T][D][Cl] (act dtype); upper layers: the dh of the layer below (fp32)
  void real_lstm_bwd(std::vector<Op>& ops, const RealLstm& Lr, Ptr dh, Ptr dx) {
    const int adt = c.act_dtype, B = fe.B, T = fe.T, D = rnn.D, Cl = rnn.Cl, H = rnn.H, l = Lr.l, tag = 200 + l;
    const int64_t BT = (int64_t)B * T;
    const ParamInfo* Whh = Lr.Whh;
    Ptr dgates = ws(Lr.nm + ".dgates", BT * 4 * H, adt);
    if (!rnn.stepped) {
      real_rec(push(ops, OP_LSTM_BWD, tag).lstm, Lr, dh, dgates, adt);
    } else {
      // per frame, last to first: cell backward (dgates[t], carry dc), then dh[t-1] += dgates[t] . W_hh
      Ptr dcb = ws(Lr.nm + ".dc", (int64_t)B * H, DT_F32);
      RunGemm rb = gemm0();
      rb.x[0] = dgates; rb.xdt = adt; rb.ydt = DT_F32;
      rb.fstride[0] = T * 4 * H; rb.rowlen[0] = (int)(BT * 4 * H); rb.Tin[0] = 1;
      rb.M = B; rb.Tout = 1; rb.Fo = B;
      rb.nseg = 1; rb.seg[0] = Seg{0, 0, 0, 4 * H, 0};
      rb.N = H;
      layout_segs(rb);
      Coef cT = [=](int nn, int sg, int j) -> int32_t { return pe(*Whh, (int64_t)gate_torch_row(j, H) * H + nn, 1); };
      pack_weights(ops, rb, cT, Lr.nm + ".hhT", tag);
      rb.y = dh; rb.y_fstride = T * H; rb.flags = kRunAccum;
      for (int t = T - 1; t >= 0; --t) {
        real_cell(push(ops, OP_CELL_BWD, tag).cell, Lr, t, false, dh, dcb, dgates);
        if (t > 0) {
          RunGemm q = rb;
          q.base[0] = t * 4 * H;
          q.y_off = (t - 1) * H;
          push(ops, OP_RUNGEMM, tag).g = q;
        }
      }
    }
    for (size_t ck = 0; ck < Lr.gxc.size(); ++ck) {
      RunGemm fw = Lr.gxc[ck];
      fw.ydt = adt;                       // WGRAD reads dy = dgates (act dtype), not the fp32 gx the forward wrote
      fw.flags &= ~kRunAccum;
      wgrad(ops, fw, dgates, Lr.cgxc[ck], tag, ck == 0 ? &Lr.bgx : nullptr);
    }
    RunGemm f = rows_gemm(Lr.h, adt, H, 0, H, 4 * H, adt);      // W_hh: dW[n][k] = sum_t dgates[t][n] * h[t-1][k]
    f.seg[0].dt = -1;
    rows_out(f, dgates, 4 * H);
    Coef chh = [=](int nn, int sg, int j) -> int32_t { return pe(*Whh, (int64_t)gate_torch_row(nn, H) * H + j, 1); };
    wgrad(ops, f, dgates, chh, tag, nullptr);
    const Coef cf = Lr.cgx;
    for (int q = 0; q < (l == 0 ? D : 1); ++q) {
      RunGemm g = rows_gemm(dgates, adt, 4 * H, 0, 4 * H, l == 0 ? Cl : H, l == 0 ? adt : DT_F32);
      Coef coef = [=](int nn, int sg, int j) -> int32_t { return cf(j, q, nn); };
      pack_weights(ops, g, coef, Lr.nm + ".dx" + std::to_string(q), tag);
      if (l == 0) rows_out(g, dx, D * Cl, q * Cl); else rows_out(g, dx, H);
      push(ops, OP_RUNGEMM, tag).g = g;
    }
  }
  // The Linear behind the recurrent block (`tranform`; DCCRN's complex stack: r_trans / i_trans as one block matrix) over the K columns of
  // x, writing the decoder input [B][T][D][Cl] directly: its coefficient and bias functions, then the forward descriptor
  struct Proj { Coef coef; Bias bias; RunGemm g; };
  Proj tranform() {
    const ParamInfo *Wt = &par("tranform.weight"), *bt = &par("tranform.bias");
    const int D = rnn.D, Cl = rnn.Cl, H = rnn.H;
    Proj p;
    p.coef = [=](int nn, int s, int j) -> int32_t { const int dd = nn / Cl, cc = nn % Cl; return pe(*Wt, (int64_t)(cc * D + dd) * H + j, 1); };
    p.bias = [=](int nn, int32_t* o) { const int dd = nn / Cl, cc = nn % Cl; o[0] = pe(*bt, cc * D + dd, 1); o[1] = 0; };
    return p;
  }
  void proj_fwd(std::vector<Op>& ops, Proj& p, Ptr x, int K, Ptr decin) {
    const int adt = c.act_dtype, N = rnn.D * rnn.Cl;
    p.g = rows_gemm(x, adt, K, 0, K, N, adt);
    pack_weights(ops, p.g, p.coef, "proj", 300, &p.bias);
    rows_out(p.g, decin, N);
    push(ops, OP_RUNGEMM, 300).g = p.g;
  }
  // its backward: the weight gradient on the weight-gradient lane, and dx [B][T][K] (fp32) = d_decin . W
  void proj_bwd(std::vector<Op>& ops, const Proj& p, Ptr d_decin, Ptr dx) {
    const int N = rnn.D * rnn.Cl, K = p.g.rowlen[0];
    cur_lane = 1;
    wgrad(ops, p.g, d_decin, p.coef, 300, &p.bias);
    cur_lane = 0;
    RunGemm g = rows_gemm(d_decin, c.act_dtype, N, 0, N, K, DT_F32);
    const Coef cf = p.coef;
    Coef coef = [=](int nn, int sg, int j) -> int32_t { return cf(j, 0, nn); };
    pack_weights(ops, g, coef, "proj.dg", 300);
    rows_out(g, dx, K);
    push(ops, OP_RUNGEMM, 300).g = g;
  }

  // WGRAD for the layer whose forward descriptor is `f` (same A runs + a ones run) against upstream gradient `dy`.
  void wgrad(std::vector<Op>& ops, const RunGemm& f, Ptr dy, const Coef& coef, int tag,
             const std::function<void(int n, int32_t out[2])>* bias) {
    if (bias && f.nseg >= kMaxSeg) {
      // kMaxSeg data runs (a recurrent input GEMM over kMaxSeg channel slices) leave no room for the ones run: the bias gradient comes from a
      // GEMM of its own over the same rows (the form of the mask layer's bias-only pass)
      wgrad(ops, f, dy, coef, tag, nullptr);
      RunGemm fb = f;
      fb.nseg = 0;
      const Coef none_coef = [](int, int, int) -> int32_t { return 0; };
      wgrad(ops, fb, dy, none_coef, tag, bias);
      return;
    }
    RunGemm g = f;            // operands keep the forward dtype: fp32 -> 32x32x2 fp32 MFMA, bf16 -> transposing 16x16x32 bf16 MFMA
    if (bias) {
      Seg& o = g.seg[g.nseg++];
      o.src = -1; o.dt = 0; o.off = 0; o.len = 1; o.koff = 0;
    }
    layout_segs(g);
    g.y = dy;
    g.bias = none();
    g.stats = none();
    // Row splits: every workgroup of a WGRAD launch does the same amount of work, so the grid is sized to fill the
    // co-resident slots of the 256 CUs in ONE wave of workgroups and never spill a few stragglers into a second one
    // (sized for the 4-stage ring: 64 KiB (128-wide n tile) or 48 KiB (64-wide) of LDS, 2 or 3 workgroups per CU; the shipped
    //  3-stage ring needs 48 / 36 KiB, so the same grids still fit in one wave with room for the other stream's kernels).
    const bool narrow = runs_aligned(g, true);       // thin layers: 32 / 16 wide n tiles (aligned bf16 kernel only)
    int tn = narrow ? wgrad_tn(g.xdt, g.N, g.Npad) : (g.xdt == DT_BF16 && g.Npad >= 128) ? 128 : kWgTN;
    // the layers that carry the FLOPs: 256 x 256 tile of the 8-wave kernel.  WG256=0 keeps the 128 x 128 tile; WG256_MINM
    // lowers the row threshold (tests run the wide kernel on small cases)
    const bool wide_on = tune_on("WG256");
    const int64_t wide_minm = tune_int("WG256_MINM", 32768);
    int tk = kWgTK;
    if (narrow && wide_on && g.Npad % 256 == 0 && g.ldw >= 384 && g.M >= wide_minm) { tn = 256; tk = 256; g.flags |= kRunWgWide; }
    else if (narrow && wide_on && g.Npad == 128 && g.ldw >= 1024 && g.M >= wide_minm) { tn = 128; tk = 512; g.flags |= kRunWgWide; }
    // a bias ones run that would open a k tile of its own (the data columns fill whole 256-wide tiles): the kernel forms the bias with a constant ones
    // operand in the workgroups of k tile 0 instead (kRunOnesMfma, rungemm.hip); ONES_MFMA=0 keeps the run a DMA'd column
    if ((g.flags & kRunWgWide) && tn == 256 && bias && g.nseg >= 2 && g.seg[g.nseg - 1].src < 0 && g.seg[g.nseg - 1].koff == g.ldw - 64 &&
        (g.ldw - 64) % 256 == 0 && tune_on("ONES_MFMA"))
      g.flags |= kRunOnesMfma;
    const int64_t ldk = (g.flags & kRunOnesMfma) ? g.ldw - 64 : g.ldw;    // columns the k tiles cover
    // wg_rounds > 1 (FullSubNet): that many dispatch rounds of shorter workgroups - the launch shares the chip with a recurrence whose
    // second round leaves 2/3 of the CUs idle, and a workgroup that needs the whole kernel's duration on its CU cannot use such a hole
    // (DCCRN in 2, 3, 4 rounds, all or only the wide-tile weight-gradient GEMMs: no gain, profiles/r05_tuning_notes.md - one round unless the model asks)
    // Wide-tile launches of SHORT workgroups (at most 10 tiles, fewer than 8192 rows per workgroup at 256 slots) fill 224 CUs, not 256: beside them the
    // main stream's 160 KB-LDS GEMMs need whole CUs, and 220 instead of 250 workgroups leave every XCD four - DCCRN default 10.60 -> 10.50 ms per step
    // (slots 160 / 192 / 208 / 216 / 224 / 232 / 240 / 248: 10.59 / 10.55 / 10.53 / 10.50 / 10.50 / 10.61 / 10.61 / 10.59, profiles/r05_tuning_notes.md);
    // DCCRN-large's launches (20 / 40 tiles, or 5 tiles of 19 000-row workgroups) LOSE 0.3-0.7 ms that way and keep 256.
    const int tiles_w = std::max(1, (int)(rup(std::min(g.N, g.Npad), tn) / tn * rup(ldk, tk) / tk));
    const bool short_wg = wg_rounds <= 1 && tiles_w <= 10 && (int64_t)g.M * tiles_w < (int64_t)8192 * 256;
    const int wide_slots = short_wg ? 224 : 256;
    // the first encoder layer's kernel on the spectrum (enc0.hip; 21 KB of LDS and <= 124 registers: up to 4 workgroups per CU).  Row splits
    // 512 / 768 / 1024 / 2048: 10.267 / 10.282 / 10.285 / 10.315 ms per step (three alternating runs each): the launch is not grid-bound, fewer partials fold faster
    const int enc0_slots = (int)tune_int("ENC0_WG_SLOTS", 512);
    const int slots = ((g.flags & kRunEnc0) ? enc0_slots : g.xdt == DT_BF16 ? ((g.flags & kRunWgWide) ? wide_slots : (tn == 128 ? 512 : tn == 64 ? 768 : 1024)) : 768) * std::max(1, wg_rounds);
    const int tiles = (int)(rup(std::min(g.N, g.Npad), tn) / tn * rup(ldk, tk) / tk);   // tiles that hold real rows
    const int steps = (int)((g.M + kWgRows - 1) / kWgRows);
    int ns = std::max(1, slots / tiles);
    ns = std::max(1, std::min(ns, std::max(1, steps / 4)));
    // N <= 4 outputs over a contiguous array (FullSubNet's sub-band head): the streaming kernel, one workgroup per row split, 0.48 ms per step ahead of the tiled
    // kernels (profiles/r06_tuning_notes.md); WGRANK_MINM: fewest rows, tests lower it
    if (wgrad_rank_form(g) && g.M >= tune_int("WGRANK_MINM", 65536)) {
      g.flags |= kRunRank;
      ns = std::max(1, std::min(1024, steps / 4));
    }
    // WG_NSPLIT = n > 0 (tests): min(n, steps) row splits for EVERY weight gradient of the plan, whatever its kernel - 1: one workgroup per tile walks every
    // row of every batch item; a huge n: one 32-row step per split.  The partial sums and the SPLITSUM table below are sized from it.  0 / unset: the rule above
    const int64_t ns_forced = tune_int("WG_NSPLIT", 0);
    if (ns_forced > 0) ns = (int)std::max<int64_t>(1, std::min<int64_t>(ns_forced, steps));
    g.nsplit = ns;
    const int64_t sz = (int64_t)g.Npad * g.ldw;
    const int64_t rel = gp_off;
    gp_off += sz * ns;
    Op& op = push(ops, OP_WGRAD, tag);
    op.g = g;
    fixes.push_back(Fix{(int)ops.size() - 1, rel, 0});
    if (ns > 1) split_sum(ops, rel, sz, ns, tag);
    // inverse table
    for (int n = 0; n < g.N; ++n) {
      for (int s = 0; s < g.nseg; ++s) {
        if (g.seg[s].src >= 0) {
          for (int j = 0; j < g.seg[s].len; ++j) {
            const int32_t t = coef(n, s, j);
            if (t == 0) continue;
            const int64_t pos = rel + (int64_t)n * g.ldw + g.seg[s].koff + j + 1;
            assert(pos < (1LL << 31));
            inv[std::abs(t) - 1].push_back((int32_t)(t > 0 ? pos : -pos));
          }
        } else if (bias) {
          int32_t bt[2] = {0, 0};
          (*bias)(n, bt);
          const int64_t pos = rel + (int64_t)n * g.ldw + g.seg[s].koff + 1;
          for (int e = 0; e < 2; ++e)
            if (bt[e] != 0) inv[std::abs(bt[e]) - 1].push_back((int32_t)(bt[e] > 0 ? pos : -pos));
        }
      }
    }
  }

  // Split sums: nothing reads a weight gradient's partial sums before the UNPACK that gathers them, so the folds of ALL weight gradients
  // planned since the last UNPACK wait in `pending_sums` and become ONE table-driven SPLITSUM launch in front of it (43 launches of
  // 6-20 us on the weight-gradient lane before: 0.37 ms per step).  SPLITSUM_MULTI=0 plans one SPLITSUM behind every WGRAD again.
  struct SumSeg { int64_t rel, n, ns; };
  std::vector<SumSeg> pending_sums;
  void split_sum(std::vector<Op>& ops, int64_t rel, int64_t n, int64_t ns, int tag) {
    if (tune_on("SPLITSUM_MULTI")) { pending_sums.push_back(SumSeg{rel, n, ns}); return; }
    Op& os = push(ops, OP_SPLITSUM, tag);
    os.unpack.n = n;
    os.unpack.sstride = n;
    os.unpack.nsplit = (int32_t)ns;
    os.unpack.start = os.unpack.ent = os.unpack.dst = none();
    fixes.push_back(Fix{(int)ops.size() - 1, rel, 1});
  }
  // side = true: the launch rides the weight-gradient lane behind the WGRADs it folds (a pure HBM stream next to the other lane's GEMMs);
  // false: main stream, which first waits for the weight-gradient lane (the fold in front of an UNPACK)
  void flush_sums(std::vector<Op>& ops, int tag, bool side = false, bool join = true) {
    if (pending_sums.empty()) return;
    std::vector<int64_t> tab;
    int64_t nmax = 0;
    for (const SumSeg& sg : pending_sums) { tab.push_back(sg.rel); tab.push_back(sg.n); tab.push_back(sg.ns); nmax = std::max(nmax, sg.n); }
    const int save = cur_lane;
    cur_lane = side ? 1 : 0;
    Op& os = push(ops, OP_SPLITSUM, tag);
    cur_lane = save;
    os.join = (side || !join) ? 0 : 1;                     // the partial sums come from the weight-gradient lane (join = false: from the main stream)
    os.unpack.start = cst(tab.data(), (int64_t)tab.size() * 8);     // int64 [nseg][3]: offset from the partial-sum base, elements, splits
    os.unpack.ent = os.unpack.dst = none();
    os.unpack.n = nmax;
    os.unpack.sstride = 0;
    os.unpack.nsplit = 0;
    os.unpack.nseg = (int32_t)pending_sums.size();
    fixes.push_back(Fix{(int)ops.size() - 1, 0, 1});
    pending_sums.clear();
  }

  int64_t unpack_lo = 0;                                   // flat gradient elements below this are already unpacked (FullSubNet's first bucket)
  int64_t unpack_hi = -1;                                  // (set by unpack_range: elements [unpack_hi, end) are already done)
  // UNPACK of the flat gradient elements [lo, hi): every weight gradient GEMM that contributes to them must have been planned.
  // The partial-sum base is not known yet (finish_unpack allocates it): recorded as a fix-up.
  void unpack_range(std::vector<Op>& ops, int64_t lo, int64_t hi, int tag, bool nojoin = false) {
    flush_sums(ops, tag, false, !nojoin);
    const int64_t n = hi - lo;
    std::vector<int32_t> start(n + 1, 0), ent;
    for (int64_t j = 0; j < n; ++j) {
      start[j] = (int32_t)ent.size();
      for (auto e : inv[lo + j]) ent.push_back(e);
      if (inv[lo + j].empty() && (size_t)(lo + j) < zero_grad.size() && zero_grad[lo + j]) ent.push_back(0);   // entry 0 adds nothing: writes 0
    }
    start[n] = (int32_t)ent.size();
    if (ent.empty()) ent.push_back(0);
    Op& op = push(ops, OP_UNPACK, tag);
    op.unpack.start = cst(start.data(), (int64_t)start.size() * 4);
    op.unpack.ent = cst(ent.data(), (int64_t)ent.size() * 4);
    op.unpack.part = none();
    op.unpack.dst = mk(A_GRAD, lo * 4);
    op.unpack.n = n;
    op.unpack.sstride = 0;
    op.unpack.nsplit = 1;
    if (nojoin) op.join = kOpNoJoin;
    fixes.push_back(Fix{(int)ops.size() - 1, 0, 1});
  }
  void finish_unpack(std::vector<Op>& ops) {
    const int64_t n = unpack_hi >= 0 ? unpack_hi : (int64_t)inv.size();
    unpack_range(ops, unpack_lo, n, 999);
    Ptr base = ws("gradpart", std::max<int64_t>(gp_off, 1), DT_F32);
    for (auto& f : fixes) {
      Ptr p = mk(A_WS, base.off + f.rel * 4);
      if (f.which == 0) ops[f.op].g.w = p; else if (f.which == 1) ops[f.op].unpack.part = p; else ops[f.op].mask.colsum = p;
    }
  }
};

void finalize_rungemms(Builder& b, Plan* P);
void finish_plan(Builder& b, Plan* P, int64_t nparam, int64_t nstate);

Plan* build_frontend_plan(const ModelConfig& cfg);
Plan* build_fsn_plan(const ModelConfig& cfg);
Plan* build_seq_plan(const ModelConfig& cfg);
Plan* build_torchstft_plan(const ModelConfig& cfg);
Plan* build_torchistft_plan(const ModelConfig& cfg);
Plan* build_torchstft_adj_plan(const ModelConfig& cfg);
Plan* build_torchistft_adj_plan(const ModelConfig& cfg);
Plan* build_convstft_plan(const ModelConfig& cfg);
Plan* build_convistft_plan(const ModelConfig& cfg);
Plan* build_convlayer_plan(const ModelConfig& cfg);
Plan* build_cbn_plan(const ModelConfig& cfg);
Plan* build_clstm_plan(const ModelConfig& cfg);

}  // namespace sefd
