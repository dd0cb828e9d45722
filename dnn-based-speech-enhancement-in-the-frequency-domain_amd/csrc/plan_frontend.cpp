// Front-end planners: the ConvSTFT front end on its own, torch.stft and torch.istft, and ConvSTFT / ConviSTFT as differentiable modules.
#include "plan_builder.h"

namespace sefd {

// Front end only (model 2): ConvSTFT 'complex' of io.wav in the reference layout -> io.out_real / io.out_imag [B][NF][T].
// Used by DCCRN.loss for the clean spectrum of the LMS loss (models.py:306-309).
Plan* build_frontend_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  Builder b;
  b.P = P;
  b.c = cfg;
  b.fe = Stft(cfg);
  const int B = cfg.B, T = b.fe.T, NF = b.fe.NF;
  P->T = T;
  P->NF = NF;
  Ptr io_wav = b.io("wav", (int64_t)B * cfg.L);
  Ptr io_or = b.io("out_real", (int64_t)B * NF * T);
  Ptr io_oi = b.io("out_imag", (int64_t)B * NF * T);
  Ptr spec = b.ws("spec", (int64_t)B * T * b.fe.SW, DT_F32);
  b.stft_fwd(P->fwd, 1, io_wav, spec);
  SpecOut so;
  std::memset(&so, 0, sizeof(so));
  so.est = spec; so.out_real = io_or; so.out_imag = io_oi; so.B = B; so.T = T; so.NF = NF;
  b.push(P->fwd, OP_SPECOUT_FWD, 2).so = so;
  finish_plan(b, P, 0, 0);
  return P;
}

// =================================================================================================================
// torch.stft front end of FullSubNet (model 4; tools_for_model.py:628-648): centre / reflect padding, hop = cfg.hop,
// periodic Hann(win_len) zero-padded to fft_len in the middle.  io.wav [B][L] -> io.spec = complex64 image [B][NF][T][2].
Plan* build_torchstft_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  Builder b;
  b.P = P;
  b.c = cfg;
  const int B = cfg.B, L = cfg.L, W = cfg.win_len, hop = cfg.hop, NFFT = cfg.fft_len;
  const int pad = NFFT / 2, Lp = L + 2 * pad;
  const int NF = NFFT / 2 + 1, NS = NF + 1, SW = NS * 2;
  P->NF = NF;
  // one sentence per limit: the message names the one that was hit
  if (hop <= 0 || hop % 4 != 0) {
    P->error = "torch.stft plan: hop " + std::to_string(hop) + " is not a positive multiple of 4 (a limit of this planner's frame GEMM, whose rows start "
               "hop samples apart; torch.stft has no such limit)";
    return P;
  }
  if (W <= 0 || W > NFFT) {                                   // win[left + j] below would be written in front of the table
    P->error = "torch.stft plan: win_len " + std::to_string(W) + " must lie in 1 .. fft_len = " + std::to_string(NFFT);
    return P;
  }
  if (pad >= L) {
    P->error = "torch.stft plan: a clip of " + std::to_string(L) + " samples is not longer than fft_len/2 = " + std::to_string(pad) + ", which reflect padding needs";
    return P;
  }
  const int T = 1 + L / hop;
  P->T = T;
  Ptr io_wav = b.io("wav", (int64_t)B * L);
  Ptr io_spec = b.io("spec", (int64_t)B * NF * T * 2);
  Ptr wpad = b.ws("wpad", (int64_t)B * Lp, DT_F32);
  Ptr spec = b.ws("spec", (int64_t)B * T * SW, DT_F32);
  { Op& op = b.push(P->fwd, OP_REFLECTPAD, 1); op.rpad.src = io_wav; op.rpad.dst = wpad; op.rpad.B = B; op.rpad.L = L; op.rpad.pad = pad; }
  std::vector<double> win(NFFT, 0.0);
  const int left = (NFFT - W) / 2;
  for (int j = 0; j < W; ++j) win[left + j] = 0.5 - 0.5 * std::cos(2.0 * kPi * j / W);
  RunGemm g = Builder::gemm0();
  g.x[0] = wpad; g.xdt = DT_F32; g.ydt = DT_F32;
  g.bstride[0] = Lp; g.rowlen[0] = Lp; g.fstride[0] = hop; g.Tin[0] = 1;
  g.M = B * T; g.Tout = 1; g.Fo = T;
  g.nseg = 1;
  g.N = SW;
  g.y = spec; g.y_bstride = (int64_t)T * SW; g.y_fstride = SW;
  // The sum over a frame's fft_len samples runs in chunks of kChunk, every chunk a GEMM of its own that adds onto the one before (kRunAccum).
  // One fp32 accumulator walking all the products rounds at the size of the growing partial sum: 6e-7 of the largest bin at fft_len 512, where
  // float32 torch.stft stays at 1.5e-7; partial sums over 128 samples, added up, keep this GEMM below 3e-7 (tests/test_gpu_frontend_edges.py).
  constexpr int kChunk = 128;
  for (int k0 = 0; k0 < NFFT; k0 += kChunk) {
    RunGemm q = g;
    const int len = std::min(kChunk, NFFT - k0);
    q.seg[0] = Seg{0, 0, k0, len, 0};
    Builder::layout_segs(q);
    std::vector<float> wt((size_t)q.Npad * q.ldw, 0.f);
    for (int nn = 2; nn < q.N; ++nn)
      for (int j = k0; j < k0 + len; ++j) {
        const double ang = 2.0 * kPi * (double)(((int64_t)(nn / 2 - 1) * j) % NFFT) / NFFT;
        wt[(size_t)nn * q.ldw + (j - k0)] = (float)(((nn & 1) == 0 ? std::cos(ang) : -std::sin(ang)) * win[j]);
      }
    q.w = b.cst(wt.data(), (int64_t)wt.size() * 4);
    if (k0 > 0) q.flags |= kRunAccum;
    b.push(P->fwd, OP_RUNGEMM, 2).g = q;
  }
  SpecOut so;
  std::memset(&so, 0, sizeof(so));
  so.est = spec; so.out_real = io_spec; so.out_imag = b.none(); so.B = B; so.T = T; so.NF = NF; so.mode = 3;
  b.push(P->fwd, OP_SPECOUT_FWD, 3).so = so;
  finish_plan(b, P, 0, 0);
  return P;
}

// =================================================================================================================
// torch.istft(n_fft, hop, win_length, hann_window(win_length), center=True, length=L) - the inverse front end of FullSubNet's
// validation path (tools_for_model.py:651-680, called at trainer.py:341-345).  IO: spec [B][NF][T][2] (memory image of the
// complex [B, NF, T] tensor, or the reference's real-pair [B, NF, T, 2]) -> wav [B][L].  Same two kernels as the ConviSTFT path:
// the inverse-FFT frame kernel (its rank-2 "correction" table set to the irfft's half weights of the DC and Nyquist bins:
//   irfft(X)[j] = (S[j] - Re X[0] / 2 - (-1)^j Re X[N/2] / 2) / (N/2),  S[j] = Re sum_{k <= N/2} X[k] e^{2 pi i k j / N})
// and the overlap-add kernel with the window-envelope normaliser, without the clamp.
Plan* build_torchistft_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  Builder b;
  b.P = P;
  b.c = cfg;
  const int B = cfg.B, L = cfg.L, W = cfg.win_len, hop = cfg.hop, NFFT = cfg.fft_len;
  const int pad = NFFT / 2;
  const int NF = NFFT / 2 + 1, NS = NF + 1, SW = NS * 2;
  P->NF = NF;
  // one sentence per limit: the message names the one that was hit
  if (NFFT != 512) {
    P->error = "torch.istft plan: fft_len " + std::to_string(NFFT) + " is not 512, the only size the inverse-FFT frame kernel is built for";
    return P;
  }
  if (W <= 0 || W > NFFT) {
    P->error = "torch.istft plan: win_len " + std::to_string(W) + " must lie in 1 .. fft_len = " + std::to_string(NFFT);
    return P;
  }
  if (hop <= 0) { P->error = "torch.istft plan: hop " + std::to_string(hop) + " is not positive"; return P; }
  if (pad >= L) {
    P->error = "torch.istft plan: length " + std::to_string(L) + " is not above fft_len/2 = " + std::to_string(pad) + " (no torch.stft has such a clip)";
    return P;
  }
  const int T = 1 + L / hop;
  P->T = T;
  Ptr io_spec = b.io("spec", (int64_t)B * NF * T * 2);
  Ptr io_wav = b.io("wav", (int64_t)B * L);
  Ptr est = b.ws("est", (int64_t)B * T * SW, DT_F32);
  Ptr frames = b.ws("frames", (int64_t)B * T * NFFT, DT_F32);
  std::vector<double> win(NFFT, 0.0);
  const int left = (NFFT - W) / 2;
  for (int j = 0; j < W; ++j) win[left + j] = 0.5 - 0.5 * std::cos(2.0 * kPi * j / W);
  { Op& op = b.push(P->fwd, OP_MEMSET, 1); op.ms.dst = est; op.ms.bytes = (int64_t)B * T * SW * 4; }       // slot 0 of every frame stays 0
  SpecOut so;
  std::memset(&so, 0, sizeof(so));
  so.est = est; so.out_real = io_spec; so.out_imag = b.none(); so.B = B; so.T = T; so.NF = NF; so.mode = 3; so.accumulate = 0;
  b.push(P->fwd, OP_SPECOUT_BWD, 2).so = so;
  {
    std::vector<float> tw(1024);
    for (int k = 0; k < 512; ++k) { tw[2 * k] = (float)std::cos(2.0 * kPi * k / 512.0); tw[2 * k + 1] = (float)std::sin(2.0 * kPi * k / 512.0); }
    std::vector<float> c(4 * 257, 0.f);                  // [even | odd][re | im][k]
    c[(0 * 2 + 0) * 257 + 0] = 0.5f; c[(0 * 2 + 0) * 257 + 256] = 0.5f;
    c[(1 * 2 + 0) * 257 + 0] = 0.5f; c[(1 * 2 + 0) * 257 + 256] = -0.5f;
    Op& op = b.push(P->fwd, OP_ISTFT_FFT, 3);
    op.ifft.est = est; op.ifft.frames = frames; op.ifft.tw = b.cst(tw.data(), 4096); op.ifft.win = b.win512(win);
    op.ifft.corr = b.cst(c.data(), (int64_t)c.size() * 4); op.ifft.nframes = (int64_t)B * T; op.ifft.W = NFFT;
  }
  // Window envelope in double, and torch.istft's own test on it: the overlap-add divides by the envelope alone, so a clip that reaches a sample
  // where it is (next to) zero has no inverse - torch raises there ("window overlap add min"), and so does this plan.  A clip that runs past
  // the last frame is zero from there on (torch pads it): Ola::Lout, as for ConviSTFT.
  const int Lp = (T - 1) * hop + NFFT;
  const int Lcov = std::min(L, Lp - pad);
  std::vector<double> env64(Lp, 0.0);
  for (int t = 0; t < T; ++t)
    for (int j = 0; j < NFFT; ++j) env64[t * hop + j] += win[j] * win[j];
  for (int p = pad; p < pad + Lcov; ++p)
    if (env64[p] <= 1e-11) {
      P->error = "torch.istft plan: at length " + std::to_string(L) + " the clip reaches sample " + std::to_string(p - pad) + ", where the overlap-add envelope of the " +
                 std::to_string(W) + "-sample Hann window at hop " + std::to_string(hop) + " over " + std::to_string(T) + " frames is " + std::to_string(env64[p]) +
                 " (not above 1e-11): torch.istft refuses this length too";
      return P;
    }
  std::vector<float> env(env64.begin(), env64.end());
  Ola ola;
  std::memset(&ola, 0, sizeof(ola));
  ola.frames = frames; ola.wav = io_wav; ola.coff = b.cst(env.data(), (int64_t)env.size() * 4); ola.dwav = ola.dpad = b.none();
  ola.B = B; ola.T = T; ola.L = L; ola.win = NFFT; ola.hop = hop; ola.trim = pad; ola.noclamp = 1; ola.Lout = Lcov < L ? Lcov : 0;
  b.push(P->fwd, OP_OLA_FWD, 4).ola = ola;
  finish_plan(b, P, 0, 0);
  return P;
}

// =================================================================================================================
// ConvSTFT (model 7) and ConviSTFT (model 8) on their own (tools_for_model.py:36-112): each a forward and a backward phase.
// kernel_num[0] = feature type: 0 'complex' (the concatenated [B][2 NF][T] tensor), 1 anything else ((mags, phase), [B][NF][T] each).
namespace {

// One sentence per limit; true when the geometry was refused.
bool convstft_refuse(Plan* P, const char* who, const ModelConfig& cfg) {
  const int W = cfg.win_len, hop = cfg.hop, NFFT = cfg.fft_len;
  const std::string pre = std::string(who) + " plan: ";
  if (W < 1 || NFFT < 2 || NFFT % 2 != 0) { P->error = pre + "win_len " + std::to_string(W) + " / fft_len " + std::to_string(NFFT) + " must be positive and fft_len even"; return true; }
  if (W > NFFT) { P->error = pre + "win_len " + std::to_string(W) + " is above fft_len " + std::to_string(NFFT) + " (the analysis basis has fft_len rows only)"; return true; }
  if (hop <= 0 || hop > W) { P->error = pre + "hop " + std::to_string(hop) + " must lie in 1 .. win_len = " + std::to_string(W); return true; }
  if (cfg.B < 1) { P->error = pre + "batch " + std::to_string(cfg.B) + " is not positive"; return true; }
  return false;
}

// Frames per workgroup of the fused inverse-FFT + overlap-add kernel: 16, halved until the staged frames (halo included) fit 40 KiB of LDS
// beside the kernel's 22 KiB of transform slices and twiddles (64 KiB per workgroup).  0: they do not fit (take the two-launch composition).
int ifft_ola_fpw(int W, int hop) {
  const int halo = (W + hop - 1) / hop - 1;
  for (int fpw = 16; fpw >= 4; fpw /= 2)
    if ((int64_t)(halo + fpw) * W * 4 <= 40 * 1024) return fpw;
  return 0;
}

// est [B*T][SW] -> out [B][Lout], fft_len == 512: the fused kernel, on the knob CONVSTFT_FUSE and if its stage fits.  False: not planned - the caller plans the
// two-launch composition, which measured faster (profiles/convstft_bench.json) and is the default.
bool ifft_ola(Builder& b, std::vector<Op>& ops, int tag, Ptr est, Ptr out, int Lout, bool synth) {
  const Stft& fe = b.fe;
  const int fpw = ifft_ola_fpw(fe.W, fe.hop);
  if (fe.NFFT != 512 || tune_has("STFT_GEMM") || !tune_has("CONVSTFT_FUSE") || fpw == 0) return false;
  Op& op = b.push(ops, OP_IFFT_OLA, tag);
  IfftOla& d = op.iola;
  d.est = est; d.out = out; d.tw = b.fft_tw; d.win = b.win512(fe.win);
  d.corr = synth ? b.istft_corr(fe.W) : b.none();
  d.coff = synth ? fe.c_coff : b.none();
  d.B = fe.B; d.T = fe.T; d.W = fe.W; d.hop = fe.hop; d.trim = fe.trim; d.Lout = Lout;
  d.fpw = fpw; d.halo = (fe.W + fe.hop - 1) / fe.hop - 1;
  d.scale = synth ? 1.f / 256.f : 1.f;
  return true;
}

void fft_twiddles(Builder& b) {
  if (b.fft_tw.arena >= 0) return;
  std::vector<float> tw(1024);
  for (int k = 0; k < 512; ++k) { tw[2 * k] = (float)std::cos(2.0 * kPi * k / 512.0); tw[2 * k + 1] = (float)std::sin(2.0 * kPi * k / 512.0); }
  b.fft_tw = b.cst(tw.data(), 4096);
}

SpecConv specconv(Builder& b, int mode, Ptr spec, Ptr a, Ptr bb) {
  SpecConv c;
  std::memset(&c, 0, sizeof(c));
  c.spec = spec; c.a = a; c.b = bb; c.dspec = c.ga = c.gb = b.none();
  c.B = b.fe.B; c.T = b.fe.T; c.NF = b.fe.NF; c.mode = mode;
  return c;
}

}  // namespace

// ConvSTFT: io.wav [B][L] -> io.out [B][2 NF][T] ('complex') or io.mags, io.phase [B][NF][T]; backward io.grad_out / io.grad_mags, io.grad_phase -> io.grad_wav.
// Backward = the adjoint of the analysis transform: d wav[b][p] = sum_t win[j] Re sum_k (g_re + i g_im)[k, t] e^{+2 pi i k j / fft_len}, j = p + trim - t hop:
// the synthesis transform without its rank-2 correction, overlap-added without a normaliser.
Plan* build_convstft_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  P->T = 0; P->NF = cfg.fft_len / 2 + 1;
  if (convstft_refuse(P, "ConvSTFT", cfg)) return P;
  Builder b;
  b.P = P;
  b.c = cfg;
  b.fe = Stft(cfg);
  const Stft& fe = b.fe;
  const int B = cfg.B, L = cfg.L, T = fe.T, NF = fe.NF, W = fe.W;
  if (L < 1 || L + 2 * fe.trim < W || T < 1) {
    P->error = "ConvSTFT plan: a clip of " + std::to_string(L) + " samples gives no frame (T < 1) at win_len " + std::to_string(W) + ", hop " + std::to_string(fe.hop);
    return P;
  }
  P->T = T;
  const bool polar = cfg.kernel_num[0] != 0;
  const int64_t BT = (int64_t)B * T;
  Ptr io_wav = b.io("wav", (int64_t)B * L);
  Ptr o_a, o_b = b.none(), g_a, g_b = b.none();
  if (polar) {
    o_a = b.io("mags", BT * NF); o_b = b.io("phase", BT * NF);
    g_a = b.io("grad_mags", BT * NF); g_b = b.io("grad_phase", BT * NF);
  } else {
    o_a = b.io("out", BT * 2 * NF); g_a = b.io("grad_out", BT * 2 * NF);
  }
  Ptr io_gw = b.io("grad_wav", (int64_t)B * L);
  Ptr spec = b.ws("spec", BT * fe.SW, DT_F32);
  Ptr gspec = b.ws("gspec", BT * fe.SW, DT_F32);
  b.stft_fwd(P->fwd, 1, io_wav, spec);
  b.push(P->fwd, OP_SPECCONV, 2).sc = specconv(b, polar ? 2 : 0, spec, o_a, o_b);
  {
    SpecConv c = specconv(b, polar ? 3 : 1, polar ? spec : gspec, g_a, g_b);
    c.dspec = polar ? gspec : b.none();
    b.push(P->bwd, OP_SPECCONV, 2).sc = c;
  }
  fft_twiddles(b);
  if (!ifft_ola(b, P->bwd, 1, gspec, io_gw, L, false)) {
    // the composition: frames [B*T][W] in HBM, then the overlap-add with a normaliser table of ones (its division is then exact)
    Ptr frames = b.ws("frames", BT * W, DT_F32);
    if (fe.NFFT == 512 && !tune_has("STFT_GEMM")) {
      std::vector<double> w256(fe.win);
      for (double& v : w256) v *= 256.0;                      // the frame kernel's fixed 1/256 (a power of two: exact)
      std::vector<float> zc(4 * 257, 0.f);
      Op& op = b.push(P->bwd, OP_ISTFT_FFT, 1);
      op.ifft.est = gspec; op.ifft.frames = frames; op.ifft.tw = b.fft_tw; op.ifft.win = b.win512(w256);
      op.ifft.corr = b.cst(zc.data(), (int64_t)zc.size() * 4); op.ifft.nframes = BT; op.ifft.W = W;
    } else {
      RunGemm g = Builder::gemm0();                           // the transpose of the framing GEMM
      g.x[0] = gspec; g.xdt = DT_F32; g.ydt = DT_F32;
      g.bstride[0] = (int64_t)T * fe.SW; g.tstride[0] = fe.SW; g.rowlen[0] = fe.SW; g.Tin[0] = T;
      g.M = (int)BT; g.Tout = T; g.Fo = 1;
      g.nseg = 1; g.seg[0] = Seg{0, 0, 0, fe.SW, 0};
      g.N = W;
      Builder::layout_segs(g);
      b.const_weights(g, [&](int nn, int j) { return j < 2 ? 0.0 : fe.Kun(j & 1, j / 2 - 1, nn) * fe.win[nn]; });
      g.y = frames; g.y_bstride = (int64_t)T * W; g.y_tstride = W;
      b.push(P->bwd, OP_RUNGEMM, 1).g = g;
    }
    std::vector<float> ones((size_t)std::max(fe.Lp, L + fe.trim), 1.f);
    Ola ola;
    std::memset(&ola, 0, sizeof(ola));
    ola.frames = frames; ola.wav = io_gw; ola.coff = b.cst(ones.data(), (int64_t)ones.size() * 4); ola.dwav = ola.dpad = b.none();
    ola.B = B; ola.T = T; ola.L = L; ola.win = W; ola.hop = fe.hop; ola.trim = fe.trim; ola.noclamp = 1;
    b.push(P->bwd, OP_OLA_FWD, 1).ola = ola;
  }
  finish_plan(b, P, 0, 0);
  return P;
}

// =================================================================================================================
// The backward passes of models 4 and 5 as plans of their own (models 12 and 13), so that the forward plans keep their bytes.  Neither reads
// anything a forward run left behind: any number of forwards of one shape may precede their backwards.  fft_len == 512 only (the FFT frame
// kernels); whatever the forward twin refuses is refused here with the twin's sentence.
namespace {

// The forward twin's verdict on this geometry: its error sentence ("" = accepted) and its frame count.
std::string twin_verdict(const ModelConfig& cfg, int model, int* T) {
  ModelConfig fc = cfg;
  fc.model = model;
  Plan* F = model == 4 ? build_torchstft_plan(fc) : build_torchistft_plan(fc);
  const std::string err = F->error;
  *T = F->T;
  delete F;
  return err;
}

std::vector<double> centred_hann(int W, int NFFT) {
  std::vector<double> win(NFFT, 0.0);
  const int left = (NFFT - W) / 2;
  for (int j = 0; j < W; ++j) win[left + j] = 0.5 - 0.5 * std::cos(2.0 * kPi * j / W);
  return win;
}

}  // namespace

// torch.stft's backward (model 12).  io.grad_spec [B][NF][T][2], the complex cotangent g = dL/dRe + i dL/dIm -> io.grad_wav [B][L]:
//   dxp[q] = sum_t w[j] Re sum_{k <= N/2} g[k, t] e^{+2 pi i k j / N},  j = q - t hop      (no half weights, no 1 / N, no normaliser)
//   dx[i]  = dxp[i + pad] + [1 <= i <= pad] dxp[pad - i] + [L-1-pad <= i <= L-2] dxp[pad + 2 (L-1) - i]
// The transform is the inverse-FFT frame kernel with a zero correction table and the window times 256 (as ConvSTFT's backward); the overlap-add
// and the fold are one gather (OP_OLA_FOLD): no [B][L + N] intermediate.
Plan* build_torchstft_adj_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  const int B = cfg.B, L = cfg.L, W = cfg.win_len, hop = cfg.hop, NFFT = cfg.fft_len;
  const int NF = NFFT / 2 + 1, SW = (NF + 1) * 2;
  P->NF = NF;
  int T = 0;
  P->error = twin_verdict(cfg, 4, &T);
  if (!P->error.empty()) return P;
  if (NFFT != 512) {
    P->error = "torch.stft backward plan: fft_len " + std::to_string(NFFT) + " is not 512, the only size the inverse-FFT frame kernel is built for";
    return P;
  }
  P->T = T;
  Builder b;
  b.P = P;
  b.c = cfg;
  const int64_t BT = (int64_t)B * T;
  Ptr io_gs = b.io("grad_spec", BT * NF * 2);
  Ptr io_gw = b.io("grad_wav", (int64_t)B * L);
  Ptr gspec = b.ws("gspec", BT * SW, DT_F32);
  Ptr frames = b.ws("frames", BT * NFFT, DT_F32);
  SpecOut so;
  std::memset(&so, 0, sizeof(so));
  so.est = gspec; so.out_real = io_gs; so.out_imag = b.none(); so.B = B; so.T = T; so.NF = NF; so.mode = 3; so.accumulate = 0;
  b.push(P->fwd, OP_SPECOUT_BWD, 1).so = so;
  fft_twiddles(b);
  {
    std::vector<double> w256 = centred_hann(W, NFFT);
    for (double& v : w256) v *= 256.0;                        // the frame kernel's fixed 1/256 (a power of two: exact)
    std::vector<float> zc(4 * 257, 0.f);
    Op& op = b.push(P->fwd, OP_ISTFT_FFT, 2);
    op.ifft.est = gspec; op.ifft.frames = frames; op.ifft.tw = b.fft_tw; op.ifft.win = b.win512(w256);
    op.ifft.corr = b.cst(zc.data(), (int64_t)zc.size() * 4); op.ifft.nframes = BT; op.ifft.W = NFFT;
  }
  Ola ola;
  std::memset(&ola, 0, sizeof(ola));
  ola.frames = frames; ola.wav = io_gw; ola.coff = ola.dwav = ola.dpad = b.none();
  ola.B = B; ola.T = T; ola.L = L; ola.win = NFFT; ola.hop = hop; ola.trim = NFFT / 2; ola.noclamp = 1;
  b.push(P->fwd, OP_OLA_FOLD, 3).ola = ola;
  finish_plan(b, P, 0, 0);
  return P;
}

// torch.istft's backward (model 13).  io.grad_wav [B][L] -> io.grad_spec [B][NF][T][2], of y[p] = sum_t frames[t][p + pad - t hop] / env[p + pad]:
//   gy'[q] = gy[q - pad] / env[q] on the covered samples (zero past Ola::Lout),  gframes[t][j] = w[j] gy'[t hop + j],
//   gX[k, t] = (c_k / N) sum_j gframes[t][j] e^{-2 pi i k j / N},  c_0 = c_{N/2} = 1, else 2;  Im gX = 0 at DC and Nyquist
// OP_OLA_BWD (noclamp = 1) + OP_STFT_FFT, the pair DCCRN's backward runs, then the weighted transpose (OP_SPECOUT_ADJ).
Plan* build_torchistft_adj_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  const int B = cfg.B, L = cfg.L, W = cfg.win_len, hop = cfg.hop, NFFT = cfg.fft_len;
  const int pad = NFFT / 2, NF = NFFT / 2 + 1, SW = (NF + 1) * 2;
  P->NF = NF;
  int T = 0;
  P->error = twin_verdict(cfg, 5, &T);                        // fft_len != 512, the window, the hop, and the envelope test
  if (!P->error.empty()) return P;
  P->T = T;
  Builder b;
  b.P = P;
  b.c = cfg;
  const int64_t BT = (int64_t)B * T;
  const int Lp = (T - 1) * hop + NFFT;
  const int Lcov = std::min(L, Lp - pad);
  Ptr io_gw = b.io("grad_wav", (int64_t)B * L);
  Ptr io_gs = b.io("grad_spec", BT * NF * 2);
  Ptr dpad = b.ws("dpad", (int64_t)B * Lp, DT_F32);
  Ptr dest = b.ws("dest", BT * SW, DT_F32);
  const std::vector<double> win = centred_hann(W, NFFT);
  std::vector<double> env64(Lp, 0.0);                         // the forward plan's table
  for (int t = 0; t < T; ++t)
    for (int j = 0; j < NFFT; ++j) env64[t * hop + j] += win[j] * win[j];
  std::vector<float> renv(2 * (size_t)Lp, 0.f);               // 1 / env as a float pair (hi | lo): OLA_BWD with noclamp = 1 (sefd_desc.h)
  for (int p = pad; p < pad + Lcov; ++p) {                    // the twin has checked these: env > 1e-11
    const double r = 1.0 / env64[p];
    renv[p] = (float)r;
    renv[(size_t)Lp + p] = (float)(r - (double)renv[p]);
  }
  Ola ola;
  std::memset(&ola, 0, sizeof(ola));
  ola.frames = b.none(); ola.wav = io_gw; ola.coff = b.cst(renv.data(), (int64_t)renv.size() * 4); ola.dwav = io_gw; ola.dpad = dpad;
  ola.B = B; ola.T = T; ola.L = L; ola.win = NFFT; ola.hop = hop; ola.trim = pad; ola.noclamp = 1; ola.Lout = Lcov < L ? Lcov : 0;
  b.push(P->fwd, OP_OLA_BWD, 1).ola = ola;
  fft_twiddles(b);
  {
    Op& op = b.push(P->fwd, OP_STFT_FFT, 2);
    op.fft.src = dpad; op.fft.spec = dest; op.fft.tw = b.fft_tw; op.fft.win = b.win512(win);
    op.fft.B = B; op.fft.L = Lp; op.fft.T = T; op.fft.hop = hop; op.fft.off = 0; op.fft.lp_dt = 0;
    op.fft.corr = b.none(); op.fft.scale = 1.f; op.fft.lp = b.none(); op.fft.pair = b.fft_pair();
  }
  SpecOut so;
  std::memset(&so, 0, sizeof(so));
  so.est = dest; so.out_real = io_gs; so.out_imag = b.none(); so.B = B; so.T = T; so.NF = NF; so.mode = 3;
  b.push(P->fwd, OP_SPECOUT_ADJ, 3).so = so;
  finish_plan(b, P, 0, 0);
  return P;
}

// ConviSTFT: cfg.L = frames T (the FullSubNet convention).  io.in [B][2 NF][T] ('complex') or io.mags, io.phase [B][NF][T] -> io.wav [B][Lout],
// Lout = (T - 1) hop + win_len - 2 (win_len - hop); no clamp, division by coff + 1e-8.  Backward io.grad_wav -> io.grad_in / io.grad_mags, io.grad_phase.
Plan* build_convistft_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  P->T = 0; P->NF = cfg.fft_len / 2 + 1;
  if (convstft_refuse(P, "ConviSTFT", cfg)) return P;
  const int B = cfg.B, T = cfg.L, W = cfg.win_len, hop = cfg.hop, trim = W - hop;
  if (T < 1) { P->error = "ConviSTFT plan: " + std::to_string(T) + " frames (T < 1)"; return P; }
  const int64_t Lout64 = (int64_t)(T - 1) * hop + W - 2 * (int64_t)trim;
  if (Lout64 <= 0) {
    P->error = "ConviSTFT plan: " + std::to_string(T) + " frames at win_len " + std::to_string(W) + ", hop " + std::to_string(hop) + " leave Lout = " +
               std::to_string(Lout64) + " <= 0 samples after the trim (the reference returns an empty tensor)";
    return P;
  }
  const int Lout = (int)Lout64;
  ModelConfig fc = cfg;
  fc.L = Lout;                                                // the clip length whose ConvSTFT has exactly T frames
  Builder b;
  b.P = P;
  b.c = cfg;
  b.fe = Stft(fc);
  const Stft& fe = b.fe;
  const int NF = fe.NF;
  if (fe.T != T || fe.Lp - 2 * fe.trim != Lout) { P->error = "ConviSTFT plan: frame geometry"; return P; }
  P->T = T;
  b.synthesis();
  const bool polar = cfg.kernel_num[0] != 0;
  const int64_t BT = (int64_t)B * T;
  Ptr i_a, i_b = b.none(), g_a, g_b = b.none();
  if (polar) {
    i_a = b.io("mags", BT * NF); i_b = b.io("phase", BT * NF);
    g_a = b.io("grad_mags", BT * NF); g_b = b.io("grad_phase", BT * NF);
  } else {
    i_a = b.io("in", BT * 2 * NF); g_a = b.io("grad_in", BT * 2 * NF);
  }
  Ptr io_wav = b.io("wav", (int64_t)B * Lout);
  Ptr io_gw = b.io("grad_wav", (int64_t)B * Lout);
  Ptr est = b.ws("est", BT * fe.SW, DT_F32);
  b.push(P->fwd, OP_SPECCONV, 2).sc = specconv(b, polar ? 4 : 1, est, i_a, i_b);
  fft_twiddles(b);
  Ola ola;
  if (ifft_ola(b, P->fwd, 1, est, io_wav, Lout, true)) {
    std::memset(&ola, 0, sizeof(ola));
    ola.frames = b.none(); ola.wav = io_wav; ola.coff = fe.c_coff; ola.dwav = ola.dpad = b.none();
    ola.B = B; ola.T = T; ola.L = Lout; ola.win = W; ola.hop = hop; ola.trim = trim;
  } else {
    Ptr frames = b.ws("frames", BT * W, DT_F32);
    const size_t at = P->fwd.size();
    ola = b.istft_ola(P->fwd, est, frames, io_wav);
    for (size_t i = at; i < P->fwd.size(); ++i)
      if (P->fwd[i].kind == OP_OLA_FWD) P->fwd[i].ola.noclamp = 2;
  }
  ola.noclamp = 2;
  Ptr dest = b.istft_ola_bwd(P->bwd, ola, io_gw);
  {
    SpecConv c = specconv(b, polar ? 5 : 0, dest, polar ? i_a : g_a, polar ? i_b : b.none());
    if (polar) { c.ga = g_a; c.gb = g_b; }
    b.push(P->bwd, OP_SPECCONV, 2).sc = c;
  }
  finish_plan(b, P, 0, 0);
  return P;
}

}  // namespace sefd
