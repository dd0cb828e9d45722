#include "plan_builder.h"

namespace sefd {

// CRN (reference models.py:329-565): the real twin of DCCRN on magnitudes.  Same kernels, different planner:
// real convs with half the channels (C_in = 1 magnitudes), plain [prev, skip] concat, ONE-layer nn.LSTM + `tranform`
// Linear, mask = tanh(out) * |spec| re-attached to the noisy phase.  I/O: wav, tgt -> out_wav, out_real (= est_mags),
// out_imag (= target_mags).  Gradients flow from out_wav only (est_mags / target_mags feed nothing the reference can
// reach: CRN + perceptual crashes in the reference).
Plan* build_crn_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  Builder b;
  b.P = P;
  b.c = cfg;
  b.fe = Stft(cfg);
  const int n = cfg.n_layers;
  const int B = cfg.B, T = b.fe.T, NF = b.fe.NF, SW = b.fe.SW;
  const int adt = cfg.act_dtype;
  const int KS = cfg.kernel_size;
  const int MS = NF + 7, MO = 7;            // magnitude rows: bin k at element k + 7 -> bin 1 is 16-byte aligned in fp32 and bf16
  P->T = T;
  P->NF = NF;
  // models.py:506-532: 'Direct(None make)' (mask_mode 4) = spectral mapping, every other cfg.masking_mode = the tanh magnitude mask
  if (KS != 5 || n < 1 || n > 7) { P->error = "CRN: unsupported configuration"; return P; }
  const bool direct = cfg.mask_mode == 4;
  std::vector<int> ch(n + 1), Fe(n + 1);
  ch[0] = 1;
  for (int i = 0; i < n; ++i) ch[i + 1] = cfg.kernel_num[i] / 2;
  Fe[0] = NF - 1;
  for (int i = 0; i < n; ++i) Fe[i + 1] = Fe[i] / 2;
  const int D = Fe[n], Cl = ch[n];
  const int H = cfg.rnn_units / 2;
  const int hid = D * Cl;                    // must equal cfg.rnn_input_size
  for (int i = 1; i <= n; ++i)
    if (ch[i] % 8 != 0) { P->error = "channel counts must be multiples of 8"; return P; }
  if (H % 16 != 0 || H > 128 || (adt == DT_BF16 && H % 32 != 0)) { P->error = "rnn_units/2 must be a multiple of 16 (32 for bf16) and <= 128"; return P; }
  if (Fe[n] < 1 || (Fe[0] % (1 << n)) != 0) { P->error = "fft_len/2 must be divisible by 2^n_layers"; return P; }

  for (int i = 0; i < n; ++i) {
    const std::string p = "encoder." + std::to_string(i);
    b.add_param(p + ".0.conv.weight", {ch[i + 1], ch[i], KS, 2}, true);
    b.add_param(p + ".0.conv.bias", {ch[i + 1]}, true);
    b.add_param(p + ".1.weight", {ch[i + 1]}, true);
    b.add_param(p + ".1.bias", {ch[i + 1]}, true);
    b.add_param(p + ".1.running_mean", {ch[i + 1]}, false);
    b.add_param(p + ".1.running_var", {ch[i + 1]}, false);
    b.add_param(p + ".2.weight", {1}, true);
  }
  for (int d = 0; d < n; ++d) {
    const int idx = n - d;
    const int cin = ch[idx] * (cfg.skip ? 2 : 1), cout = ch[idx - 1];
    const std::string p = "decoder." + std::to_string(d);
    b.add_param(p + ".0.conv.weight", {cin, cout, KS, 2}, true);
    b.add_param(p + ".0.conv.bias", {cout}, true);
    if (idx != 1) {
      b.add_param(p + ".1.weight", {cout}, true);
      b.add_param(p + ".1.bias", {cout}, true);
      b.add_param(p + ".1.running_mean", {cout}, false);
      b.add_param(p + ".1.running_var", {cout}, false);
      b.add_param(p + ".2.weight", {1}, true);
    }
  }
  b.add_param("enhance.weight_ih_l0", {4 * H, hid}, true);
  b.add_param("enhance.weight_hh_l0", {4 * H, H}, true);
  b.add_param("enhance.bias_ih_l0", {4 * H}, true);
  b.add_param("enhance.bias_hh_l0", {4 * H}, true);
  b.add_param("tranform.weight", {hid, H}, true);
  b.add_param("tranform.bias", {hid}, true);
  const int64_t nparam = P->params.back().off + P->params.back().numel;
  const int64_t nstate = P->state.empty() ? 0 : P->state.back().off + P->state.back().numel;
  b.inv.resize(nparam);

  Ptr io_wav = b.io("wav", (int64_t)B * cfg.L);
  Ptr io_out = b.io("out_wav", (int64_t)B * cfg.L);
  Ptr io_or = b.io("out_real", (int64_t)B * NF * T);      // est_mags
  Ptr io_oi = b.io("out_imag", (int64_t)B * NF * T);      // target_mags
  Ptr io_gw = b.io("grad_wav", (int64_t)B * cfg.L);
  Ptr io_gr = b.io("grad_real", (int64_t)B * NF * T);     // gradient w.r.t. est_mags (crn_direct_train's loss lives there)
  b.io("grad_imag", (int64_t)B * NF * T);
  Ptr io_tgt = b.io("tgt", (int64_t)B * cfg.L);
  b.synthesis();
  std::vector<Op>& F = P->fwd;
  std::vector<Op>& R = P->bwd;
  const int64_t BT = (int64_t)B * T;

  // ---- STFT of the noisy input and of the target (CRN.forward always does both, models.py:468, 505; both take the same form)
  Ptr spec = b.ws("spec", BT * SW, DT_F32);
  Ptr spec_t = b.ws("spec_t", BT * SW, DT_F32);
  b.stft_fwd(F, 1, io_wav, spec);
  b.stft_fwd(F, 2, io_tgt, spec_t);
  Ptr mags = b.ws("mags", BT * MS, adt);
  {
    Op& op = b.push(F, OP_MAGS, 3);
    op.mags.spec = spec; op.mags.mags = mags; op.mags.frames = BT; op.mags.NF = NF; op.mags.MS = MS; op.mags.MO = MO; op.mags.dt = adt;
  }

  // ---- encoder (RealConv2d, tools_for_model.py:341-386)
  std::vector<Builder::ConvLayer> enc(n), dec(n);
  Builder::ActSrc x{mags, (int64_t)T * MS, MS, MO + 1, 1};
  for (int i = 0; i < n; ++i) {
    const int Ci = ch[i], Co = ch[i + 1], Fo = Fe[i + 1];
    const std::string pp = "encoder." + std::to_string(i);
    const ParamInfo &Wc = b.par(pp + ".0.conv.weight"), &bc = b.par(pp + ".0.conv.bias");
    Builder::Coef coef = [=](int nn, int s, int j) -> int32_t {
      const int kw = s, kh = j / Ci, ci = j % Ci;
      return pe(Wc, (((int64_t)nn * Ci + ci) * KS + kh) * 2 + kw, 1);
    };
    Builder::Bias bias = [=](int nn, int32_t* o) { o[0] = pe(bc, nn, 1); o[1] = 0; };
    enc[i] = b.enc_conv(F, 100 + i, "enc" + std::to_string(i), pp, x, Fe[i], Fo, Co, coef, bias, true, false);
    x = Builder::ActSrc{enc[i].z, (int64_t)T * Fo * Co, Fo * Co, 0, Co};
  }

  // ---- single-layer LSTM + Linear (models.py:391-398, 483-486); feature order c*D + d
  b.rnn = Builder::Rnn{D, Cl, H, false};
  const Builder::RealLstm lstm = b.real_lstm_fwd(F, "lstm", 0, enc[n - 1].z, adt);
  Ptr decin = b.ws("decin", BT * D * Cl, adt);
  Builder::Proj proj = b.tranform();
  b.proj_fwd(F, proj, lstm.h, H, decin);

  // ---- decoder (RealConvTranspose2d, tools_for_model.py:389-425; torch.cat([out, enc], 1) skips)
  std::array<Builder::ActSrc, 2> src{Builder::ActSrc{decin, (int64_t)T * D * Cl, D * Cl, 0, Cl}, Builder::ActSrc{}};
  for (int d = 0; d < n; ++d) {
    const int idx = n - d;
    const int C0 = ch[idx], C1 = cfg.skip ? ch[idx] : 0, Co = ch[idx - 1];
    const int Fi = Fe[idx], Fo = 2 * Fi;
    const bool last = (idx == 1);
    const std::string nm = "dec" + std::to_string(d);
    const std::string pp = "decoder." + std::to_string(d);
    const ParamInfo &Wc = b.par(pp + ".0.conv.weight"), &bc = b.par(pp + ".0.conv.bias");
    Builder::ConvLayer& Ly = dec[d];
    Ly.C = Co; Ly.Fq = Fo; Ly.R = (int64_t)B * (T + 1) * Fo;
    Ly.y = b.ws(nm + ".y", Ly.R * Co, adt);
    if (!last) { Ly.z = b.ws(nm + ".z", Ly.R * Co, adt); Ly.mi = b.ws(nm + ".mi", 2 * Co, DT_F32); }
    Builder::WCoef wcoef = [=](int nn, int s, int cc, int kh, int kw) -> int32_t {
      const int rc = s == 0 ? cc : C0 + cc;
      return pe(Wc, (((int64_t)rc * Co + nn) * KS + kh) * 2 + kw, 1);
    };
    Ly.bias = [=](int nn, int32_t* o) { o[0] = pe(bc, nn, 1); o[1] = 0; };
    const int nblk1 = (int)(((int64_t)B * (T + 1) * Fi + kBM - 1) / kBM);
    const int npad_stat = (int)rup(Co, bn_of(Co));
    Ptr part = last ? b.none() : b.ws(nm + ".stat", (int64_t)2 * nblk1 * 2 * npad_stat, DT_F32);
    src[1] = Builder::ActSrc{enc[idx - 1].z, (int64_t)T * Fi * C1, Fi * C1, 0, C1};
    b.dec_phases(F, 400 + d, nm, Ly, src, Fi, Co, wcoef, !last && cfg.training ? part : b.none(), nblk1, true);
    if (!last) {
      b.bn_fwd(F, 400 + d, pp, Ly, part, 2 * nblk1, npad_stat, 0, 0);
      src[0] = Builder::ActSrc{Ly.z, (int64_t)(T + 1) * Fo * Co, Fo * Co, Fo * Co, Co};   // frames 1..T of the T+1 buffer
    }
  }

  // ---- mask, iSTFT, outputs (models.py:519-532)
  Ptr est = b.ws("est", BT * SW, DT_F32);
  Ptr estm = b.ws("estm", BT * NF, DT_F32);
  Ptr frames = b.ws("frames", BT * b.fe.W, DT_F32);
  Mask mk;
  std::memset(&mk, 0, sizeof(mk));
  {
    const int Fo = Fe[0];
    mk.spec = spec; mk.mask = dec[n - 1].y; mk.est = est; mk.estm = estm; mk.dest = mk.dmask = mk.destm = b.none();
    mk.frames = BT; mk.NF = NF; mk.mode = direct ? 5 : 3; mk.mdt = adt; mk.mch = 1;
    mk.mask_fstride = Fo; mk.mask_bstride = (int64_t)(T + 1) * Fo; mk.mask_base = Fo; mk.T = T;
    b.push(F, OP_MASK_FWD, 500).mask = mk;
  }
  const Ola ola = b.istft_ola(F, est, frames, io_out);
  {
    SpecOut so;
    std::memset(&so, 0, sizeof(so));
    so.est = estm; so.out_real = io_or; so.out_imag = b.none(); so.B = B; so.T = T; so.NF = NF; so.mode = 2;
    b.push(F, OP_SPECOUT_FWD, 503).so = so;
    so.est = spec_t; so.out_real = io_oi; so.mode = 1;
    b.push(F, OP_SPECOUT_FWD, 504).so = so;
  }

  // =================================================================================================== backward
  if (cfg.training) {
    Ptr dest = b.istft_ola_bwd(R, ola, io_gw);
    b.conv_grads(enc, dec, ch[0]);
    Ptr d_decin = b.ws("decin.d", BT * D * Cl, adt);
    {
      Ptr d_estm = b.ws("destm", BT * NF, DT_F32);       // io.grad_real [B][NF][T] -> [B*T][NF]
      SpecOut s2;
      std::memset(&s2, 0, sizeof(s2));
      s2.est = d_estm; s2.out_real = io_gr; s2.out_imag = b.none(); s2.B = B; s2.T = T; s2.NF = NF; s2.mode = 2;
      b.push(R, OP_SPECOUT_BWD, 503).so = s2;
      Mask m2 = mk;
      m2.dest = dest; m2.dmask = dec[n - 1].dy; m2.destm = d_estm;
      b.push(R, OP_MASK_BWD, 500).mask = m2;
    }
    for (int d = n - 1; d >= 0; --d) {
      const int idx = n - d;
      const int C0 = ch[idx], C1 = cfg.skip ? ch[idx] : 0;
      const std::string nm = "dec" + std::to_string(d);
      Builder::ConvLayer& Ly = dec[d];
      if (idx != 1)
        b.bn_bwd(R, 400 + d, Ly.y, Ly.dz, b.none(), Ly.mi, "decoder." + std::to_string(d), Ly.C, Ly.R, (int64_t)(T + 1) * Ly.Fq, Ly.Fq, Ly.dy, nm,
                 false, nullptr, false);
      b.cur_lane = 1;                           // weight gradients of the decoder: nothing downstream needs them before UNPACK
      for (int par = 0; par < 2; ++par) b.wgrad(R, Ly.f[par], Ly.dy, Ly.coef[par], 400 + d, &Ly.bias);
      b.cur_lane = 0;
      for (int s = 0; s < (cfg.skip ? 2 : 1); ++s) {
        Builder::Coef coef;
        const RunGemm g = b.dec_dgrad(R, 400 + d, nm, Ly, Ly.C, Fe[idx], s, s == 0 ? C0 : C1, s == 0 ? (d > 0 ? dec[d - 1].dz : d_decin) : enc[idx - 1].dskip,
                                      coef, true);
        b.push(R, OP_RUNGEMM, 400 + d).g = g;
      }
    }
    // projection + LSTM backward
    Ptr dh = b.ws("lstm.dh", BT * H, DT_F32);
    b.proj_bwd(R, proj, d_decin, dh);
    b.real_lstm_bwd(R, lstm, dh, enc[n - 1].dz);
    for (int i = n - 1; i >= 0; --i) {
      const std::string nm = "enc" + std::to_string(i);
      Builder::ConvLayer& Ly = enc[i];
      b.bn_bwd(R, 100 + i, Ly.y, Ly.dz, cfg.skip ? Ly.dskip : b.none(), Ly.mi, "encoder." + std::to_string(i), Ly.C, Ly.R, (int64_t)T * Ly.Fq, 0,
               Ly.dy, nm, false, nullptr, false);
      b.wgrad(R, Ly.f[0], Ly.dy, Ly.coef[0], 100 + i, &Ly.bias);
      for (int par = 0; i > 0 && par < 2; ++par) {
        const RunGemm g = b.enc_dgrad(R, 100 + i, nm, Ly, ch[i], Fe[i], par, enc[i - 1].dz);
        b.push(R, OP_RUNGEMM, 100 + i).g = g;
      }
    }
    b.finish_unpack(R);
  }
  finish_plan(b, P, nparam, nstate);
  return P;
}

}  // namespace sefd
