// The DCCRN planner (reference models.py:15-284).
#include "plan_builder.h"

namespace sefd {

Plan* build_dccrn_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  Builder b;
  b.P = P;
  b.c = cfg;
  b.fe = Stft(cfg);
  const int n = cfg.n_layers;
  const int B = cfg.B, L = cfg.L, W = cfg.win_len, T = b.fe.T, NF = b.fe.NF, NS = b.fe.NS, SW = b.fe.SW;
  const int adt = cfg.act_dtype;
  const int KS = cfg.kernel_size;
  P->T = T;
  P->NF = NF;
  if (cfg.model != 0 || KS != 5 || n < 1 || n > 7) { P->error = "unsupported configuration"; return P; }
  const bool cx = cfg.lstm_complex != 0;     // cfg.lstm: 'complex' (NavieComplexLSTM stack) or 'real' (nn.LSTM(2 layers) + tranform, models.py:96-105)
  std::vector<int> ch(n + 1), Fe(n + 1);
  ch[0] = 2;
  for (int i = 0; i < n; ++i) ch[i + 1] = cfg.kernel_num[i];
  Fe[0] = NF - 1;
  for (int i = 0; i < n; ++i) Fe[i + 1] = Fe[i] / 2;
  const int D = Fe[n];                       // hidden_dim (models.py:81)
  const int H = cfg.lstm_complex ? cfg.rnn_units / 2 : cfg.rnn_units;   // per-part hidden size of the complex LSTM / hidden size of the real one
  const int NL = cfg.rnn_layers;
  const int Cl = ch[n];                      // channels entering the LSTM
  for (int i = 1; i <= n; ++i)
    if (ch[i] % 8 != 0 && !(i == 0)) { P->error = "channel counts must be multiples of 8"; return P; }
  // H <= 128: persistent recurrence kernels (W_hh resident in the VGPRs of one CU).  Larger H (DCCRN-large: rnn_units 512):
  // bf16 mode runs the cluster kernels of lstm_cluster.hip (W_hh spread over H/64 CUs, h handed over in memory every step);
  // fp32 mode and odd sizes fall back to one GEMM + one cell launch per time step on the same buffers.
  const bool cluster_ok = adt == DT_BF16 && H > 128 && H <= 512 && H % 64 == 0;
  const bool stepped = (H > 128 && !cluster_ok) || tune_has("LSTM_STEPPED");
  // all weight gradients ride the second stream (after the fork they run next to the encoder's dgrad / BatchNorm chain and
  // fill the tails of its kernels: 14.42 -> 14.30 ms/step); LANE_ALL=0 keeps only the decoder's there
  const bool lane_all = tune_on("LANE_ALL");
  if (H % 16 != 0 || (adt == DT_BF16 && H % 32 != 0)) { P->error = "rnn_units/2 must be a multiple of 16 (32 for bf16)"; return P; }
  if (Fe[n] < 1 || (Fe[0] % (1 << n)) != 0) { P->error = "fft_len/2 must be divisible by 2^n_layers"; return P; }

  // ------------------------------------------------------------------ parameters (reference registration order)
  const bool cbn = cfg.use_cbn != 0;
  // SyncBN for ComplexBatchNorm is built on request (cbn_sync, which models.py sets for GradientExchange(sync_bn=True)); bn_world alone keeps
  // refusing it, as it did before the CBN finalize kernels had their SyncBN modes
  if (cbn && cfg.bn_world > 1 && !cfg.cbn_sync) { P->error = "ComplexBatchNorm SyncBN plans need cbn_sync = 1"; return P; }
  // the normalisation + PReLU behind a conv: nn.BatchNorm2d(C) or ComplexBatchNorm(C) (tools_for_model.py:441-467: 5 parameters and 5 buffers of C / 2)
  auto add_norm = [&](const std::string& p, int C) {
    if (cbn) {
      for (const char* w : {"Wrr", "Wri", "Wii", "Br", "Bi"}) b.add_param(p + ".1." + w, {C / 2}, true);
      for (const char* w : {"RMr", "RMi", "RVrr", "RVri", "RVii"}) b.add_param(p + ".1." + w, {C / 2}, false);
    } else {
      b.add_param(p + ".1.weight", {C}, true);
      b.add_param(p + ".1.bias", {C}, true);
      b.add_param(p + ".1.running_mean", {C}, false);
      b.add_param(p + ".1.running_var", {C}, false);
    }
    b.add_param(p + ".2.weight", {1}, true);
  };
  // forward of that layer: y [Rr][C] -> z
  auto cbn_fwd = [&](int tag, const std::string& pp, const std::string& nm, Ptr y, Ptr z, int C, int64_t Rr) -> Ptr {
    if ((C / 2) % 4 != 0) { P->error = "ComplexBatchNorm: channel pairs per layer must be a multiple of 4"; return b.none(); }
    if (C / 2 > 1024) { P->error = "ComplexBatchNorm: at most 1024 channel pairs per layer (cbn.hip reduces a row of pairs in one workgroup)"; return b.none(); }
    CbnFwd c;
    std::memset(&c, 0, sizeof(c));
    const int h = C / 2;
    const int64_t rpbk = std::max<int64_t>(64, (Rr + 2047) / 2048);
    c.y = y; c.z = z; c.R = Rr; c.C = C; c.dt = adt; c.nblk = (int)((Rr + rpbk - 1) / rpbk); c.rows_per_blk = (int)rpbk;
    c.training = cfg.training; c.count = (double)Rr; c.eps = 1e-5f; c.momentum = 0.1f;
    c.part = cfg.training ? b.ws(nm + ".cstat", (int64_t)c.nblk * 5 * h, DT_F32) : b.none();
    c.coef = b.ws(nm + ".ccoef", 14 * h, DT_F32);
    const char* wn[3] = {"Wrr", "Wri", "Wii"};
    const char* rvn[3] = {"RVrr", "RVri", "RVii"};
    for (int q = 0; q < 3; ++q) { c.W[q] = b.pptr(pp + ".1." + wn[q]); c.RV[q] = b.sptr(pp + ".1." + rvn[q]); }
    c.Bv[0] = b.pptr(pp + ".1.Br"); c.Bv[1] = b.pptr(pp + ".1.Bi");
    c.RM[0] = b.sptr(pp + ".1.RMr"); c.RM[1] = b.sptr(pp + ".1.RMi");
    c.slope = b.pptr(pp + ".2.weight");
    if (cfg.training) b.push(P->fwd, OP_CBN_STATS, tag).cbf = c;
    b.push(P->fwd, OP_CBN_FINALIZE, tag).cbf = c;
    b.push(P->fwd, OP_CBN_APPLY, tag).cbf = c;
    return c.coef;
  };
  for (int i = 0; i < n; ++i) {
    const std::string p = "encoder." + std::to_string(i);
    for (const char* part : {"real_conv", "imag_conv"}) {
      b.add_param(p + ".0." + part + ".weight", {ch[i + 1] / 2, ch[i] / 2, KS, 2}, true);
      b.add_param(p + ".0." + part + ".bias", {ch[i + 1] / 2}, true);
    }
    add_norm(p, ch[i + 1]);
  }
  for (int d = 0; d < n; ++d) {
    const int idx = n - d;
    const int cin = ch[idx] * (cfg.skip ? 2 : 1), cout = ch[idx - 1];
    const std::string p = "decoder." + std::to_string(d);
    for (const char* part : {"real_conv", "imag_conv"}) {
      b.add_param(p + ".0." + part + ".weight", {cin / 2, cout / 2, KS, 2}, true);
      b.add_param(p + ".0." + part + ".bias", {cout / 2}, true);
    }
    if (idx != 1) add_norm(p, cout);
  }
  const int hid = D * Cl;                    // LSTM feature size real+imag
  if (!cx) {                                  // nn.LSTM(hid, rnn_units, num_layers=2) then nn.Linear(rnn_units, hid)
    for (int l = 0; l < 2; ++l) {
      const std::string sl = std::to_string(l);
      b.add_param("enhance.weight_ih_l" + sl, {4 * H, l == 0 ? hid : H}, true);
      b.add_param("enhance.weight_hh_l" + sl, {4 * H, H}, true);
      b.add_param("enhance.bias_ih_l" + sl, {4 * H}, true);
      b.add_param("enhance.bias_hh_l" + sl, {4 * H}, true);
    }
    b.add_param("tranform.weight", {hid, H}, true);
    b.add_param("tranform.bias", {hid}, true);
  }
  for (int l = 0; l < (cx ? NL : 0); ++l) {
    const int I = (l == 0 ? hid : cfg.rnn_units) / 2;
    const std::string p = "enhance." + std::to_string(l);
    for (const char* part : {"real_lstm", "imag_lstm"}) {
      b.add_param(p + "." + part + ".weight_ih_l0", {4 * H, I}, true);
      b.add_param(p + "." + part + ".weight_hh_l0", {4 * H, H}, true);
      b.add_param(p + "." + part + ".bias_ih_l0", {4 * H}, true);
      b.add_param(p + "." + part + ".bias_hh_l0", {4 * H}, true);
    }
    if (l == NL - 1)
      for (const char* part : {"r_trans", "i_trans"}) {
        b.add_param(p + "." + part + ".weight", {hid / 2, H}, true);
        b.add_param(p + "." + part + ".bias", {hid / 2}, true);
      }
  }
  const int64_t nparam = P->params.back().off + P->params.back().numel;
  const int64_t nstate = P->state.empty() ? 0 : P->state.back().off + P->state.back().numel;
  b.inv.resize(nparam);

  // ------------------------------------------------------------------ I/O block
  Ptr io_wav = b.io("wav", (int64_t)B * L);
  Ptr io_out = b.io("out_wav", (int64_t)B * L);
  Ptr io_or = b.io("out_real", (int64_t)B * NF * T);
  Ptr io_oi = b.io("out_imag", (int64_t)B * NF * T);
  Ptr io_gw = b.io("grad_wav", (int64_t)B * L);
  Ptr io_gr = b.io("grad_real", (int64_t)B * NF * T);
  Ptr io_gi = b.io("grad_imag", (int64_t)B * NF * T);

  b.synthesis();

  std::vector<Op>& F = P->fwd;
  std::vector<Op>& R = P->bwd;

  // ------------------------------------------------------------------ STFT (ConvSTFT.forward, tools_for_model.py:54-61)
  Ptr spec = b.ws("spec", (int64_t)B * T * SW, DT_F32);
  Ptr spec_lp = spec;
  const bool spec_fft = b.stft_fwd(F, 1, io_wav, spec);
  // encoder input: spectrogram with the 2 channels padded to CP (aligned 16-byte runs for the thin first layer), act dtype
  const int CP = 8;
  // bf16 plans (round 6): the first layer reads the fp32 spectrum itself - no padded copy (64 MB written and read per step at B = 32), K = 20 instead of
  // 128 mostly-zero columns; kernels: enc0.hip.  ENC0_DIRECT=0: the padded copy and the generic kernels (A/B runs)
  const bool enc0_direct = adt == DT_BF16 && spec_fft && NS == 258 && KS == 5 && Fe[1] == 128 && (ch[1] == 16 || ch[1] == 32 || ch[1] == 64) &&
                           tune_on("ENC0_DIRECT");
  if (!enc0_direct) {
    spec_lp = b.ws("xin", (int64_t)B * T * NS * CP, adt);
    const bool fuse_pad = tune_on("SPECPAD_FUSE");
    if (spec_fft && fuse_pad && NS == 258) {      // the FFT kernel writes the padded copy beside the spectrogram (no SPECPAD pass: 48 us at B = 32)
      F.back().fft.lp = spec_lp; F.back().fft.lp_dt = adt;
    } else {
      Op& op = b.push(F, OP_SPECPAD, 1);
      op.mags.spec = spec; op.mags.mags = spec_lp; op.mags.frames = (int64_t)B * T; op.mags.NF = NS; op.mags.MS = CP; op.mags.MO = 0; op.mags.dt = adt;
    }
  }

  // ------------------------------------------------------------------ encoder
  std::vector<Builder::ConvLayer> enc(n), dec(n);
  const int C0b = enc0_direct ? 2 : CP;            // channels of the first layer's input BUFFER (padded, or the spectrum's (re, im) pairs)
  Builder::ActSrc x{enc0_direct ? spec : spec_lp, (int64_t)T * NS * C0b, NS * C0b, 2 * C0b, C0b};
  for (int i = 0; i < n; ++i) {
    const int Ci = ch[i], Co = ch[i + 1], Fo = Fe[i + 1], Cib = x.C;
    const std::string nm = "enc" + std::to_string(i);
    const std::string pp = "encoder." + std::to_string(i);
    const ParamInfo &Wr = b.par(pp + ".0.real_conv.weight"), &Wi = b.par(pp + ".0.imag_conv.weight");
    const ParamInfo &br = b.par(pp + ".0.real_conv.bias"), &bi = b.par(pp + ".0.imag_conv.bias");
    const int Ci2 = Ci / 2, Co2 = Co / 2;
    Builder::Coef coef = [=](int nn, int s, int j) -> int32_t {
      const int kw = s, kh = j / Cib, ci = j % Cib;
      if (ci >= Ci) return 0;                       // pad channel
      const bool oi = nn >= Co2, ii = ci >= Ci2;
      const int co2 = oi ? nn - Co2 : nn, ci2 = ii ? ci - Ci2 : ci;
      const int64_t idx = (((int64_t)co2 * Ci2 + ci2) * KS + kh) * 2 + kw;
      if (!oi) return ii ? pe(Wi, idx, -1) : pe(Wr, idx, 1);
      return ii ? pe(Wr, idx, 1) : pe(Wi, idx, 1);
    };
    Builder::Bias bias = [=](int nn, int32_t* o) {
      if (nn < Co2) { o[0] = pe(br, nn, 1); o[1] = pe(bi, nn, -1); }
      else { o[0] = pe(br, nn - Co2, 1); o[1] = pe(bi, nn - Co2, 1); }
    };
    enc[i] = b.enc_conv(F, 100 + i, nm, pp, x, Fe[i], Fo, Co, coef, bias, !cbn, i == 0 && enc0_direct);
    if (cbn) {
      enc[i].mi = cbn_fwd(100 + i, pp, nm, enc[i].y, enc[i].z, Co, enc[i].R);       // the layer's coefficient table takes the place of (mean, invstd)
      if (!P->error.empty()) return P;
    }
    x = Builder::ActSrc{enc[i].z, (int64_t)T * Fo * Co, Fo * Co, 0, Co};
  }

  // ------------------------------------------------------------------ complex LSTM stack (tools_for_model.py:141-181)
  const int64_t BT = (int64_t)B * T;
  // (gxc / cgxc: the input GEMM of a part per chunk of channel slices - one chunk unless layer 0 reads more than kMaxSeg slices, Builder::slice_chunks)
  struct Lstm { RunGemm gx[2]; Builder::Coef cgx[2]; Builder::Bias bgx; Ptr gxb, h, gates, cst, hc; RunGemm hh[2]; std::vector<RunGemm> gxc[2]; std::vector<Builder::Coef> cgxc[2]; };
  std::vector<Lstm> ls(NL);
  Ptr lin = enc[n - 1].z;
  b.rnn = Builder::Rnn{D, Cl, H, stepped};
  // ---- cfg.lstm == 'real': two stacked real LSTM layers over all D*Cl features (feature order c*D + d, models.py:214-218)
  Builder::RealLstm rl[2];
  for (int l = 0; l < (cx ? 0 : 2); ++l) {
    rl[l] = b.real_lstm_fwd(F, "lstm" + std::to_string(l), l, lin, DT_F32);
    lin = rl[l].h;
  }
  // ---- the complex stack: groups g4 = (part, parameter set); gx / dgates are [part][B*T][set][4H], h / c / dh [group][B*T][H]
  auto gx_goff = [=](int g4) { return (int64_t)(g4 / 2) * BT * 8 * H + (int64_t)(g4 % 2) * 4 * H; };
  // the persistent recurrence of layer l (backward: with dh and dgates)
  auto lstm_desc = [&](int l, Ptr dh, Ptr dgates, int gdt) {
    const std::string pp = "enhance." + std::to_string(l);
    LstmRec r;
    std::memset(&r, 0, sizeof(r));
    r.gx = ls[l].gxb;
    r.whh[0] = b.pptr(pp + ".real_lstm.weight_hh_l0"); r.whh[1] = b.pptr(pp + ".imag_lstm.weight_hh_l0");
    r.h = ls[l].h; r.gates = ls[l].gates; r.c = ls[l].cst; r.dh = dh; r.dgates = dgates;
    for (int g4 = 0; g4 < 4; ++g4) r.gx_goff[g4] = gx_goff(g4);
    r.gx_ld = 8 * H; r.G = 4; r.nset = 2; r.B = B; r.T = T; r.H = H; r.hdt = adt; r.gdt = gdt;
    return r;
  };
  // the cell launch of frame t of the stepped path, over the 4 groups
  auto complex_cell = [&](LstmCell& cl, int l, int t, bool fwd, Ptr dh, Ptr dcb, Ptr dgates) {
    cl.gates = b.mk(A_WS, ls[l].gxb.off + (int64_t)t * 8 * H * 4);
    cl.c = b.mk(A_WS, ls[l].cst.off + (int64_t)t * H * 4);
    cl.c_prev = t > 0 ? b.mk(A_WS, ls[l].cst.off + (int64_t)(t - 1) * H * 4) : b.none();
    cl.h = fwd ? b.mk(A_WS, ls[l].h.off + (int64_t)t * H * esize(adt)) : b.none();
    cl.dh = fwd ? b.none() : b.mk(A_WS, dh.off + (int64_t)t * H * 4);
    cl.dc = fwd ? b.none() : dcb;
    cl.dgates = fwd ? b.none() : b.mk(A_WS, dgates.off + (int64_t)t * 8 * H * esize(adt));
    cl.rows = 4 * B; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = fwd ? t == 0 : t == T - 1;
    cl.G = 4; cl.Bg = B; cl.unit_major = 1;
    cl.rs[0] = (int64_t)T * 8 * H; cl.rs[1] = cl.rs[2] = cl.rs[3] = (int64_t)T * H; cl.rs[4] = (int64_t)T * 8 * H;
    for (int g4 = 0; g4 < 4; ++g4) {
      cl.go[0][g4] = cl.go[4][g4] = gx_goff(g4);
      cl.go[1][g4] = cl.go[2][g4] = cl.go[3][g4] = (int64_t)g4 * BT * H;
    }
  };
  // Two complex layers, persistent bf16 kernels: the sequence is cut into chunks of frames and layer 1 (combine + input
  // GEMM + recurrence of a chunk, second HIP stream) runs while layer 0 already works on the next chunk - the two 483-step
  // recurrences (8 workgroups each, latency-bound) overlap instead of running back to back.  LSTM_CHUNKS=1 disables.
  // Measured (B = 32, T = 483): 1 chunk 14.08 ms/step, 2-6 chunks 13.84-13.94, 8: 13.94, 16: 14.50 -> 4.
  int nchunk = (int)tune_int("LSTM_CHUNKS", 4);
  if (!(cx && !stepped && adt == DT_BF16 && NL == 2) || nchunk < 2 || T < 8 * nchunk) nchunk = 1;
  const bool pipe = nchunk > 1;
  LstmRec pipe_rec[2];
  RunGemm pipe_gx1[2];
  for (int l = 0; l < (cx ? NL : 0); ++l) {
    const std::string nm = "lstm" + std::to_string(l);
    const std::string pp = "enhance." + std::to_string(l);
    const ParamInfo* Wih[2] = {&b.par(pp + ".real_lstm.weight_ih_l0"), &b.par(pp + ".imag_lstm.weight_ih_l0")};
    const ParamInfo* bih[2] = {&b.par(pp + ".real_lstm.bias_ih_l0"), &b.par(pp + ".imag_lstm.bias_ih_l0")};
    const ParamInfo* bhh[2] = {&b.par(pp + ".real_lstm.bias_hh_l0"), &b.par(pp + ".imag_lstm.bias_hh_l0")};
    const int I = (l == 0 ? hid : 2 * H) / 2;      // features per part
    const int rowlen = l == 0 ? D * Cl : 2 * H;
    ls[l].gxb = b.ws(nm + ".gx", 2 * BT * 8 * H, DT_F32);
    ls[l].h = b.ws(nm + ".h", 4 * BT * H, adt);
    ls[l].gates = b.ws(nm + ".gates", 4 * BT * 4 * H, DT_F32);
    ls[l].cst = b.ws(nm + ".c", 4 * BT * H, DT_F32);
    ls[l].hc = b.ws(nm + ".hc", BT * 2 * H, adt);
    Builder::Bias bias = [=](int nn, int32_t* o) {
      const int set = nn / (4 * H), gq = gate_torch_row(nn % (4 * H), H);
      o[0] = pe(*bih[set], gq, 1); o[1] = pe(*bhh[set], gq, 1);
    };
    ls[l].bgx = bias;
    const bool gx_merge = tune_on("GX_MERGE") && BT * 8 * H < (1LL << 31);
    const int nck = l == 0 ? Builder::slice_chunks(D) : 1;
    for (int p = 0; p < 2; ++p) {
      Builder::Coef coef = [=](int nn, int s, int j) -> int32_t {
        const int set = nn / (4 * H), gq = gate_torch_row(nn % (4 * H), H);
        const int feat = (l == 0) ? j * D + s : j;      // reference feature order c*D + d (models.py:203-206)
        return pe(*Wih[set], (int64_t)gq * I + feat, 1);
      };
      ls[l].cgx[p] = coef;
      for (int ck = 0; ck < nck; ++ck) {
        const int d0 = ck * kMaxSeg;
        RunGemm g = b.rows_gemm(lin, adt, rowlen, p * H, H, 8 * H, DT_F32);
        if (l == 0) Builder::rows_slices(g, std::min(kMaxSeg, D - d0), Cl, d0 * Cl + p * (Cl / 2), Cl / 2);
        const Builder::Coef cc = ck == 0 ? coef : Builder::Coef([=](int nn, int s, int j) -> int32_t { return coef(nn, s + d0, j); });
        b.pack_weights(F, g, cc, nm + ".ih" + std::to_string(p) + (ck ? "_" + std::to_string(ck) : ""), 200 + l, p == 0 && ck == 0 ? &bias : nullptr);
        if (p == 1 && ck == 0) g.bias = ls[l].gx[0].bias;
        if (ck) g.flags |= kRunAccum;
        b.rows_out(g, b.mk(A_WS, ls[l].gxb.off + (int64_t)p * BT * 8 * H * 4), 8 * H);
        if (ck == 0) ls[l].gx[p] = g;
        ls[l].gxc[p].push_back(g); ls[l].cgxc[p].push_back(cc);
        if (gx_merge) continue;
        if (pipe && l == 1) pipe_gx1[p] = g; else b.push(F, OP_RUNGEMM, 200 + l).g = g;
      }
    }
    for (int ck = 0; gx_merge && ck < nck; ++ck) {
      // both parts in ONE launch: the two GEMMs share their weights (W_ih of the real and the imag LSTM side by side) and differ only in the
      // input columns (part p) and the output slab - the part becomes the row index f of the run descriptor (rows (b, t, p))
      RunGemm g = ls[l].gxc[0][ck];
      g.Fo = 2; g.M = (int)(2 * BT);
      g.fstride[0] = l == 0 ? Cl / 2 : H;
      g.y_fstride = (int)(BT * 8 * H);
      if (pipe && l == 1) pipe_gx1[0] = g; else b.push(F, OP_RUNGEMM, 200 + l).g = g;
    }
    if (!stepped) {
      const LstmRec r = lstm_desc(l, b.none(), b.none(), DT_F32);
      if (pipe) pipe_rec[l] = r; else b.push(F, OP_LSTM_FWD, 200 + l).lstm = r;
    } else {
      // per time step: gx[t] += h[t-1] . W_hh^T (one GEMM per parameter set over the 2B rows (part, b)), then one cell launch
      // over the 4 groups; gx is overwritten in place by the gates i,f,g,o, which is what the backward cells read
      const ParamInfo* Whh[2] = {&b.par(pp + ".real_lstm.weight_hh_l0"), &b.par(pp + ".imag_lstm.weight_hh_l0")};
      for (int set = 0; set < 2; ++set) {
        RunGemm g = Builder::gemm0();
        g.x[0] = ls[l].h; g.xdt = adt; g.ydt = DT_F32;
        g.bstride[0] = 0; g.tstride[0] = 2 * BT * H; g.fstride[0] = T * H; g.rowlen[0] = (int)(BT * H); g.Tin[0] = 2;
        g.M = 2 * B; g.Tout = 2; g.Fo = B;
        g.nseg = 1; g.seg[0] = Seg{0, 0, 0, H, 0};
        g.N = 4 * H;
        Builder::layout_segs(g);
        const ParamInfo* Wp = Whh[set];
        Builder::Coef chh = [=](int nn, int sg, int j) -> int32_t { return pe(*Wp, (int64_t)gate_torch_row(nn, H) * H + j, 1); };
        b.pack_weights(F, g, chh, nm + ".hh" + std::to_string(set), 200 + l);
        g.y = ls[l].gxb; g.y_bstride = 0; g.y_tstride = (int)(BT * 8 * H); g.y_fstride = T * 8 * H; g.flags = kRunAccum;
        ls[l].hh[set] = g;
      }
      for (int t = 0; t < T; ++t) {
        if (t > 0)
          for (int set = 0; set < 2; ++set) {
            RunGemm g = ls[l].hh[set];
            g.base[0] = (int64_t)set * BT * H + (int64_t)(t - 1) * H;
            g.y_off = t * 8 * H + set * 4 * H;
            b.push(F, OP_RUNGEMM, 200 + l).g = g;
          }
        complex_cell(b.push(F, OP_CELL_FWD, 200 + l).cell, l, t, true, b.none(), b.none(), b.none());
      }
    }
    if (!pipe) {
      Op& op = b.push(F, OP_COMBINE_FWD, 200 + l);
      op.comb.h = ls[l].h; op.comb.out = ls[l].hc; op.comb.rows = BT; op.comb.H = H; op.comb.dt = adt; op.comb.T = T;
    }
    lin = ls[l].hc;
  }
  if (pipe) {
    for (int c = 0; c < nchunk; ++c) {
      const int t0 = (int)((int64_t)T * c / nchunk), t1 = (int)((int64_t)T * (c + 1) / nchunk), Tc = t1 - t0;
      {
        LstmRec r = pipe_rec[0];
        r.t0 = t0; r.t1 = t1;
        b.push(F, OP_LSTM_FWD, 200).lstm = r;
      }
      // lane 3 (third stream): the input GEMM of layer 1 for this chunk reads layer 0's chunk only, so it runs BESIDE layer 1's recurrence
      // over the previous chunk instead of queueing behind it on the second stream (round 4 timeline: 657 -> ~520 us for the LSTM block)
      b.cur_lane = 3;
      {
        Op& op = b.push(F, OP_COMBINE_FWD, 200);
        op.comb.h = ls[0].h; op.comb.out = ls[0].hc; op.comb.rows = BT; op.comb.H = H; op.comb.dt = adt;
        op.comb.T = T; op.comb.t0 = t0; op.comb.t1 = t1;
      }
      const bool gxm = pipe_gx1[0].Fo == 2;               // both parts in one launch (gx_merge)
      for (int p = 0; p < (gxm ? 1 : 2); ++p) {           // input GEMM of layer 1 for the frames of this chunk
        RunGemm g = pipe_gx1[p];
        g.M = B * Tc * (gxm ? 2 : 1); g.Tout = Tc; g.Tin[0] = Tc;
        g.base[0] += t0 * g.tstride[0];
        g.y_off += t0 * g.y_tstride;
        b.push(F, OP_RUNGEMM, 201).g = g;
      }
      b.cur_lane = 2;
      {
        LstmRec r = pipe_rec[1];
        r.t0 = t0; r.t1 = t1;
        b.push(F, OP_LSTM_FWD, 201).lstm = r;
      }
      b.cur_lane = 0;
    }
    Op& op = b.push(F, OP_COMBINE_FWD, 201);
    op.join = 1;                                           // the main stream needs layer 1's last chunk
    op.comb.h = ls[1].h; op.comb.out = ls[1].hc; op.comb.rows = BT; op.comb.H = H; op.comb.dt = adt; op.comb.T = T;
  }
  // projection r_trans / i_trans (tools_for_model.py:173-175) writing the decoder input [B][T][D][Cl] directly
  Ptr decin = b.ws("decin", BT * D * Cl, adt);
  Builder::Proj proj;
  if (!cx) {                                   // tranform: Linear(rnn_units -> D*Cl), output feature c*D + d -> decoder input [B][T][D][Cl]
    proj = b.tranform();
  } else {
    const std::string pp = "enhance." + std::to_string(NL - 1);
    const ParamInfo* Wt[2] = {&b.par(pp + ".r_trans.weight"), &b.par(pp + ".i_trans.weight")};
    const ParamInfo* bt[2] = {&b.par(pp + ".r_trans.bias"), &b.par(pp + ".i_trans.bias")};
    const int Ch = Cl / 2;
    proj.coef = [=](int nn, int s, int j) -> int32_t {
      const int dd = nn / Cl, rem = nn % Cl, p = rem / Ch, cc = rem % Ch;
      if ((j >= H) != (p == 1)) return 0;
      return pe(*Wt[p], (int64_t)(cc * D + dd) * H + (j - p * H), 1);
    };
    proj.bias = [=](int nn, int32_t* o) {
      const int dd = nn / Cl, rem = nn % Cl, p = rem / Ch, cc = rem % Ch;
      o[0] = pe(*bt[p], cc * D + dd, 1); o[1] = 0;
    };
  }
  b.proj_fwd(F, proj, lin, cx ? 2 * H : H, decin);

  // ------------------------------------------------------------------ decoder (models.py:222-226; sub-pixel phases)
  std::array<Builder::ActSrc, 2> src{Builder::ActSrc{decin, (int64_t)T * D * Cl, D * Cl, 0, Cl}, Builder::ActSrc{}};
  std::vector<std::array<Builder::ActSrc, 2>> dec_src(n);
  for (int d = 0; d < n; ++d) {
    const int idx = n - d;
    const int C0 = ch[idx], C1 = cfg.skip ? ch[idx] : 0, Co = ch[idx - 1];
    const int Fi = Fe[idx], Fo = 2 * Fi;
    const bool last = (idx == 1);
    const int Cob = last ? std::max(Co, CP) : Co;   // channels of the output BUFFER (mask layer: 2 -> 8, pad stays 0)
    const std::string nm = "dec" + std::to_string(d);
    const std::string pp = "decoder." + std::to_string(d);
    const ParamInfo &Wr = b.par(pp + ".0.real_conv.weight"), &Wi = b.par(pp + ".0.imag_conv.weight");
    const ParamInfo &br = b.par(pp + ".0.real_conv.bias"), &bi = b.par(pp + ".0.imag_conv.bias");
    const int Co2 = Co / 2;
    Builder::ConvLayer& Ly = dec[d];
    Ly.C = Co; Ly.Fq = Fo; Ly.R = (int64_t)B * (T + 1) * Fo;
    Ly.y = b.ws(nm + ".y", Ly.R * Cob, adt);
    if (!last) { Ly.z = b.ws(nm + ".z", Ly.R * Co, adt); Ly.mi = b.ws(nm + ".mi", 2 * Co, DT_F32); }
    // reference input-channel index (within the real or imag half) of channel c of source s (complex_cat order)
    auto refc = [=](int s, int cc, bool& imag) {
      const int Cs = s == 0 ? C0 : C1;
      imag = cc >= Cs / 2;
      const int q = imag ? cc - Cs / 2 : cc;
      return s == 0 ? q : C0 / 2 + q;
    };
    Builder::WCoef wcoef = [=](int nn, int s, int cc, int kh, int kw) -> int32_t {
      if (nn >= Co) return 0;                        // pad output channel
      bool ii;
      const int rc = refc(s, cc, ii);
      const bool oi = nn >= Co2;
      const int co2 = oi ? nn - Co2 : nn;
      const int64_t ix = (((int64_t)rc * Co2 + co2) * KS + kh) * 2 + kw;
      if (!oi) return ii ? pe(Wi, ix, -1) : pe(Wr, ix, 1);
      return ii ? pe(Wr, ix, 1) : pe(Wi, ix, 1);
    };
    Ly.bias = [=](int nn, int32_t* o) {
      if (nn >= Co) { o[0] = o[1] = 0; }
      else if (nn < Co2) { o[0] = pe(br, nn, 1); o[1] = pe(bi, nn, -1); }
      else { o[0] = pe(br, nn - Co2, 1); o[1] = pe(bi, nn - Co2, 1); }
    };
    const int nblk1 = (int)(((int64_t)B * (T + 1) * Fi + kBM - 1) / kBM);
    const int npad_stat = (int)rup(Co, bn_of(Co));
    Ptr part = last ? b.none() : b.ws(nm + ".stat", (int64_t)2 * nblk1 * 2 * npad_stat, DT_F32);
    const bool stats = !last && cfg.training && !cbn;
    // Thin layers (Cob <= PHASE_MERGE_MAXN, default 32: dec4 and the mask layer): ONE GEMM for both sub-pixel phases - the even
    // phase's runs (input bins f-1, f, f+1, two frames), 2 * Cob output columns [phase][channel] (= bins 2f and 2f+1 of the output row:
    // contiguous in the channels-last buffer), zero weights where the odd phase has no tap.  These layers are bound by streaming the
    // tap-expanded activation operand through L2 -> LDS, not by MFMAs: 20 % more MACs, the operand streamed once instead of twice.
    // The backward reads only the per-phase coefficient functions.
    const int merge_maxn = (int)tune_int("PHASE_MERGE_MAXN", 64);
    const bool merge = Cob <= merge_maxn && tune_on("WG_SWAP");
    src[1] = Builder::ActSrc{enc[idx - 1].z, (int64_t)T * Fi * C1, Fi * C1, 0, C1};
    dec_src[d] = src;
    b.dec_phases(F, 400 + d, nm, Ly, src, Fi, Cob, wcoef, stats ? part : b.none(), nblk1, !merge);
    int fin_nblk = 2 * nblk1, fin_cpad = npad_stat, fin_nsub = 0;
    if (merge) {
      RunGemm g = Ly.f[0];                      // the even phase's runs
      g.N = 2 * Cob;
      Builder::layout_segs(g);
      const Builder::Coef f0 = Ly.coef[0], f1 = Ly.coef[1];
      const Builder::Bias bias = Ly.bias;
      const int c0 = C0, c1 = C1, cob = Cob;
      Builder::Coef coef = [=](int nn, int sg, int j) -> int32_t {
        if (nn >= 2 * cob) return 0;
        if (nn < cob) return f0(nn, sg, j);
        const int Cs = sg / 2 == 0 ? c0 : c1;
        return j < Cs ? 0 : f1(nn - cob, sg, j - Cs);          // the odd phase's taps are bins f, f+1: one bin into the even phase's run
      };
      Builder::Bias bias2 = [=](int nn, int32_t* o) { if (nn >= 2 * cob) { o[0] = o[1] = 0; } else bias(nn % cob, o); };
      b.pack_weights(F, g, coef, nm + ".pm", 400 + d, &bias2);
      g.y = Ly.y; g.y_bstride = (int64_t)(T + 1) * Fo * Cob; g.y_tstride = Fo * Cob; g.y_fstride = 2 * Cob; g.y_off = 0;
      if (stats) {
        if ((int64_t)nblk1 * 2 * g.Npad > (int64_t)2 * nblk1 * 2 * npad_stat) { P->error = "merged sub-pixel GEMM: statistics pitch"; return P; }
        g.stats = part;
        fin_nblk = nblk1; fin_cpad = g.Npad; fin_nsub = 2;
      }
      b.push(F, OP_RUNGEMM, 400 + d).g = g;
    }
    if (last) continue;
    if (cbn) {
      Ly.mi = cbn_fwd(400 + d, pp, nm, Ly.y, Ly.z, Co, Ly.R);
      if (!P->error.empty()) return P;
    } else {
      b.bn_fwd(F, 400 + d, pp, Ly, part, fin_nblk, fin_cpad, fin_nsub, Cob);
    }
    src[0] = Builder::ActSrc{Ly.z, (int64_t)(T + 1) * Fo * Co, Fo * Co, Fo * Co, Co};   // frames 1..T of the T+1 buffer
  }

  // ------------------------------------------------------------------ mask, iSTFT, outputs (models.py:253-282)
  Ptr est = b.ws("est", BT * SW, DT_F32);
  Ptr frames = b.ws("frames", BT * W, DT_F32);
  Mask mk;
  std::memset(&mk, 0, sizeof(mk));
  {
    const int Fo = Fe[0], Co = std::max(2, CP);
    mk.spec = spec; mk.mask = dec[n - 1].y; mk.est = est; mk.dest = mk.dmask = b.none();
    mk.frames = BT; mk.NF = NF; mk.mode = cfg.mask_mode; mk.mdt = adt; mk.mch = Co; mk.estm = mk.destm = b.none();
    mk.mask_fstride = (int64_t)Fo * Co; mk.mask_bstride = (int64_t)(T + 1) * Fo * Co; mk.mask_base = (int64_t)Fo * Co; mk.T = T;
    b.push(F, OP_MASK_FWD, 500).mask = mk;
  }
  const Ola ola = b.istft_ola(F, est, frames, io_out);
  SpecOut so;
  std::memset(&so, 0, sizeof(so));
  so.est = est; so.out_real = io_or; so.out_imag = io_oi; so.B = B; so.T = T; so.NF = NF; so.accumulate = 0;
  b.push(F, OP_SPECOUT_FWD, 503).so = so;

  // =================================================================================================== backward
  if (cfg.training) {
    Ptr dest = b.istft_ola_bwd(R, ola, io_gw);
    {
      SpecOut s2 = so;
      s2.est = dest; s2.out_real = io_gr; s2.out_imag = io_gi; s2.accumulate = 1;
      b.push(R, OP_SPECOUT_BWD, 503).so = s2;
    }
    b.conv_grads(enc, dec, std::max(ch[0], CP));
    constexpr int kCsRows = 2048;                // workgroups of MASK_BWD when it also leaves the mask layer's bias-gradient shares
    const bool mask_colsum = tune_on("MASK_COLSUM") && CP >= 2 && CP <= 8 &&
                             tune_on("WG_SWAP");
    int mask_colsum_op = -1;
    Ptr d_decin = b.ws("decin.d", BT * D * Cl, adt);
    {
      Mask m2 = mk;
      m2.dest = dest; m2.dmask = dec[n - 1].dy;
      if (mask_colsum) { m2.colsum_rows = kCsRows; mask_colsum_op = (int)R.size(); }
      b.push(R, OP_MASK_BWD, 500).mask = m2;
    }
    // BatchNorm backward reductions in the epilogues of the GEMMs that PRODUCE the upstream gradient (kRunBnBwd): every dgrad GEMM
    // that writes (a component of) dz of a BatchNorm layer gets the layer's forward output and parameters and a range of partial rows;
    // BN_BWD_FINALIZE then adds all of them.  The separate reduce pass (two or three tensor reads per layer) is gone.  Not fused: the
    // last encoder layer (its dz arrives in channel slices from the LSTM input-gradient GEMMs).
    // Which layers: measured on the default model (profiles/r03_tuning_notes.md) the extra epilogue read costs the wide-tile kernel
    // (cgemm256, N % 256 == 0, compute-bound) 10-17 us per launch against 38-91 us for the pass it replaces, but it costs the thin
    // GEMMs (N <= 128: latency-bound tiles that stream at ~2 TB/s) 45-85 us per launch - more than the pass, which streams at 4-5 TB/s.
    // So by default only the layers whose producers all run on the wide-tile kernel are fused (bf16, C % 256 == 0).
    // BN_FUSE=0: none; BN_FUSE=2: every layer (the per-op tests run the epilogue of all three GEMM kernels that way).
    const int bn_fuse_mode = (int)tune_int("BN_FUSE", 1);
    const bool bn_fuse = bn_fuse_mode != 0 && !cbn;
    auto bn_fuse_layer = [&](int C, int64_t Rr) { return bn_fuse_mode == 2 || (adt == DT_BF16 && C % 256 == 0 && Rr >= 8192); };
    using BnbAcc = Builder::BnbAcc;
    std::vector<BnbAcc> bnb_dec(n), bnb_enc(n);
    auto bnb_init = [&](BnbAcc& a, const std::string& nm, Ptr y, Ptr mi, const std::string& pp, int C, int64_t Rr) {
      a.on = true; a.y = y; a.mi = mi; a.pp = pp;
      a.ldp = (int)rup(C, bn_of(C));
      a.cap = (int)(2 * ((Rr + kBM - 1) / kBM) + 16);
      a.part = b.ws(nm + ".bnpart", (int64_t)a.cap * 3 * a.ldp, DT_F32);
    };
    if (bn_fuse) {
      for (int d = 0; d + 1 < n; ++d) if (bn_fuse_layer(dec[d].C, dec[d].R)) bnb_init(bnb_dec[d], "dec" + std::to_string(d), dec[d].y, dec[d].mi, "decoder." + std::to_string(d), dec[d].C, dec[d].R);
      for (int i = 0; i + 1 < n; ++i) if (bn_fuse_layer(enc[i].C, enc[i].R)) bnb_init(bnb_enc[i], "enc" + std::to_string(i), enc[i].y, enc[i].mi, "encoder." + std::to_string(i), enc[i].C, enc[i].R);
    }
    // the GEMM `g` writes dz rows (b, u, fo) of that layer; (bs, ts, fs, off) address the same rows of the layer's forward output y
    auto bnb_attach = [&](RunGemm& g, BnbAcc& a, int64_t bs, int ts, int fs, int off) {
      if (!a.on) return;
      const int rows = (g.M + kBM - 1) / kBM;
      if (a.rows + rows > a.cap || g.Npad != a.ldp) { P->error = "BatchNorm backward partial rows: capacity / pitch"; return; }
      g.flags |= kRunBnBwd;
      g.bnb_y = a.y; g.bnb_mi = a.mi;
      g.bnb_gamma = b.pptr(a.pp + ".1.weight"); g.bnb_beta = b.pptr(a.pp + ".1.bias"); g.bnb_slope = b.pptr(a.pp + ".2.weight");
      g.bnb_bstride = bs; g.bnb_tstride = ts; g.bnb_fstride = fs; g.bnb_off = off;
      g.stats = b.mk(A_WS, a.part.off + (int64_t)a.rows * 3 * a.ldp * 4);
      a.rows += rows;
    };

    // ---- decoder backward
    for (int d = n - 1; d >= 0; --d) {
      const int idx = n - d;
      const int C0 = ch[idx], C1 = cfg.skip ? ch[idx] : 0;
      const int Fi = Fe[idx], Fo = 2 * Fi;
      const bool last = (idx == 1);
      const int Co = last ? std::max(ch[idx - 1], CP) : ch[idx - 1];     // buffer channels (pad rows of the mask layer carry zero weights)
      const std::string nm = "dec" + std::to_string(d);
      const std::string pp = "decoder." + std::to_string(d);
      if (!last)
        b.bn_bwd(R, 400 + d, dec[d].y, dec[d].dz, b.none(), dec[d].mi, pp, Co, dec[d].R, (int64_t)(T + 1) * Fo, Fo, dec[d].dy, nm, cbn, &bnb_dec[d], false);
      // Weight gradients.  Forward form (WG_SWAP=0): one WGRAD per sub-pixel phase, A = the forward runs (3 or 2 taps x C channels of
      // both sources, two frames: every input element is streamed through LDS ~5 times per phase pair), dense operand = dy.
      // Swapped form (default): the SAME tensor, contracted over INPUT pixels - dense operand = the source activation x_s (each element
      // read once), A = the runs of the input-gradient GEMM over dy (5 taps x Co channels, two frames): the tap expansion moves to the
      // operand with the FEWER channels (Co <= C_in / 2 in every decoder layer).  Mask layer: 3.0 GB -> 1.3 GB through LDS-DMA.
      // The bias gradient needs its own pass over dy then (ones run only) - planned for the mask layer; a conv bias in front of
      // BatchNorm has an identically zero gradient (the sum over all rows of the BatchNorm input gradient vanishes), which the reference
      // computes as rounding noise and this plan leaves at exactly 0.
      const bool wg_swap = tune_on("WG_SWAP");
      b.cur_lane = 1;                           // weight gradients of the decoder: nothing downstream needs them before UNPACK
      if (!wg_swap) for (int par = 0; par < 2; ++par) b.wgrad(R, dec[d].f[par], dec[d].dy, dec[d].coef[par], 400 + d, &dec[d].bias);
      else if (!last) {                          // conv biases in front of BatchNorm: UNPACK writes their exact zero
        b.zero_grad.resize(nparam, 0);
        for (const char* part : {".0.real_conv.bias", ".0.imag_conv.bias"}) {
          const ParamInfo& pb = b.par(pp + part);
          for (int64_t e = 0; e < pb.numel; ++e) b.zero_grad[pb.off + e] = 1;
        }
      } else if (mask_colsum_op >= 0) {
        // the mask layer's bias gradient = column sums of dmask: MASK_BWD's workgroups leave their shares in the partial-sum buffer
        // ([kCsRows][8] fp32), a SPLITSUM folds them to 128 rows and UNPACK adds those (a 110 us bias-only WGRAD pass over dmask before)
        const int64_t rel = b.gp_off;
        b.gp_off += (int64_t)kCsRows * 8;
        b.fixes.push_back(Builder::Fix{mask_colsum_op, rel, 2});
        b.split_sum(R, rel, 128 * 8, kCsRows / 128, 400 + d);
        for (int nn = 0; nn < Co; ++nn) {
          int32_t bt[2] = {0, 0};
          dec[d].bias(nn, bt);
          for (int r = 0; r < 128; ++r) {
            const int64_t pos = rel + (int64_t)r * 8 + nn + 1;
            for (int e = 0; e < 2; ++e)
              if (bt[e] != 0) b.inv[std::abs(bt[e]) - 1].push_back((int32_t)(bt[e] > 0 ? pos : -pos));
          }
        }
      } else {
        RunGemm fb = Builder::gemm0();           // all output rows (both phases), no activation run: wgrad() appends the ones run
        fb.xdt = adt; fb.ydt = adt;
        fb.M = B * (T + 1) * Fo; fb.Tout = T + 1; fb.Fo = Fo;
        fb.nseg = 0; fb.N = Co;
        fb.y_bstride = (int64_t)(T + 1) * Fo * Co; fb.y_tstride = Fo * Co; fb.y_fstride = Co; fb.y_off = 0;
        Builder::Coef none_coef = [](int, int, int) -> int32_t { return 0; };
        b.wgrad(R, fb, dec[d].dy, none_coef, 400 + d, &dec[d].bias);
      }
      b.cur_lane = 0;
      // input gradients: conv-form over dy [B][T+1][Fo][Co]; dx[ci,f,t] = sum W[ci,co,kh,kw] dy[co, 2f+kh-2, t+kw]
      const int nsrc = cfg.skip ? 2 : 1;
      // Thin layers: ONE GEMM over dy for the input gradients of both sources (previous layer's output | skip connection): the same runs
      // of dy, C0 + C1 output columns, the second half stored to the second destination (RunGemm::y2 / n2).  The A operand - what bounds
      // these layers - is streamed once instead of twice.  Not when a destination's BatchNorm sums ride in the epilogue (one layer per GEMM).
      const int dg_maxn = (int)tune_int("DGRAD_MERGE_MAXN", 128);
      const bool dg_merge = nsrc == 2 && C0 == C1 && C0 % 8 == 0 && C0 + C1 <= dg_maxn && !(d > 0 && bnb_dec[d - 1].on) && !bnb_enc[idx - 1].on;
      RunGemm dg_g[2];
      Builder::Coef dg_coef[2];
      for (int s = 0; s < nsrc; ++s) {
        const int Cs = s == 0 ? C0 : C1;
        Builder::Coef coef;
        RunGemm g = b.dec_dgrad(R, 400 + d, nm, dec[d], Co, Fi, s, Cs, s == 0 ? (d > 0 ? dec[d - 1].dz : d_decin) : enc[idx - 1].dskip, coef, !dg_merge);
        // dz of the previous decoder layer (its y keeps the frame that `[..., 1:]` drops: rows start one frame in) / of encoder layer idx-1
        if (s == 0 && d > 0) bnb_attach(g, bnb_dec[d - 1], (int64_t)(T + 1) * Fi * Cs, Fi * Cs, Cs, Fi * Cs);
        else if (s == 1) bnb_attach(g, bnb_enc[idx - 1], (int64_t)T * Fi * Cs, Fi * Cs, Cs, 0);
        if (!dg_merge) b.push(R, OP_RUNGEMM, 400 + d).g = g;
        dg_g[s] = g; dg_coef[s] = coef;
        if (wg_swap) {                           // weight gradient, swapped form: the runs of this GEMM against the source activation
          RunGemm fw = g;
          fw.flags = 0; fw.stats = b.none(); fw.bias = b.none(); fw.ydt = adt;
          const Builder::ActSrc& xs = dec_src[d][s];
          fw.y_bstride = xs.bstride; fw.y_tstride = xs.tstride; fw.y_fstride = xs.C; fw.y_off = xs.base;
          b.cur_lane = 1;
          b.wgrad(R, fw, xs.p, coef, 400 + d, nullptr);
          b.cur_lane = 0;
        }
      }
      if (dg_merge) {
        RunGemm g = dg_g[0];
        g.N = C0 + C1;
        Builder::layout_segs(g);
        const Builder::Coef f0 = dg_coef[0], f1 = dg_coef[1];
        const int c0 = C0;
        Builder::Coef coef = [=](int nn, int sg, int j) -> int32_t { return nn < c0 ? f0(nn, sg, j) : f1(nn - c0, sg, j); };
        b.pack_weights(R, g, coef, nm + ".dgm", 400 + d);
        g.y2 = dg_g[1].y; g.n2 = C0;
        b.push(R, OP_RUNGEMM, 400 + d).g = g;
      }
    }
    // ---- cfg.lstm == 'real': tranform, then the two LSTM layers last to first, then the gradient into the encoder output
    if (!cx) {
      Ptr dh[2] = {b.ws("lstm0.dh", BT * H, DT_F32), b.ws("lstm1.dh", BT * H, DT_F32)};
      b.proj_bwd(R, proj, d_decin, dh[1]);
      b.real_lstm_bwd(R, rl[1], dh[1], dh[0]);
      b.real_lstm_bwd(R, rl[0], dh[0], enc[n - 1].dz);
    }
    // ---- projection backward (the buffer is part of either plan's table)
    Ptr dhc_next = b.ws("dhc" + std::to_string(NL - 1), BT * 2 * H, DT_F32);
    if (cx) b.proj_bwd(R, proj, d_decin, dhc_next);
    // ---- LSTM backward
    for (int l = cx ? NL - 1 : -1; l >= 0; --l) {
      const std::string nm = "lstm" + std::to_string(l);
      const std::string pp = "enhance." + std::to_string(l);
      const ParamInfo* Whh[2] = {&b.par(pp + ".real_lstm.weight_hh_l0"), &b.par(pp + ".imag_lstm.weight_hh_l0")};
      Ptr dh = b.ws(nm + ".dh", 4 * BT * H, DT_F32);
      Ptr dgates = b.ws(nm + ".dgates", 2 * BT * 8 * H, adt);
      const int64_t dg_half = BT * 8 * H * esize(adt);
      {
        Op& op = b.push(R, OP_COMBINE_BWD, 200 + l);
        op.comb.h = dh; op.comb.out = dhc_next; op.comb.rows = BT; op.comb.H = H; op.comb.dt = DT_F32; op.comb.T = T;
      }
      if (!stepped) {
        b.push(R, OP_LSTM_BWD, 200 + l).lstm = lstm_desc(l, dh, dgates, adt);
      } else {
        // per time step, last to first: cell backward (dgates[t], carry dc), then dh[t-1] += dgates[t] . W_hh per parameter set
        Ptr dcb = b.ws(nm + ".dc", (int64_t)4 * B * H, DT_F32);
        RunGemm rb[2];
        for (int set = 0; set < 2; ++set) {
          RunGemm g = Builder::gemm0();
          g.x[0] = dgates; g.xdt = adt; g.ydt = DT_F32;
          g.bstride[0] = 0; g.tstride[0] = (int)(BT * 8 * H); g.fstride[0] = T * 8 * H; g.rowlen[0] = (int)(BT * 8 * H); g.Tin[0] = 2;
          g.M = 2 * B; g.Tout = 2; g.Fo = B;
          g.nseg = 1; g.seg[0] = Seg{0, 0, 0, 4 * H, 0};
          g.N = H;
          Builder::layout_segs(g);
          const ParamInfo* Wp = Whh[set];
          Builder::Coef cT = [=](int nn, int sg, int j) -> int32_t { return pe(*Wp, (int64_t)gate_torch_row(j, H) * H + nn, 1); };
          b.pack_weights(R, g, cT, nm + ".hhT" + std::to_string(set), 200 + l);
          g.y = dh; g.y_bstride = 0; g.y_tstride = (int)(2 * BT * H); g.y_fstride = T * H; g.flags = kRunAccum;
          rb[set] = g;
        }
        for (int t = T - 1; t >= 0; --t) {
          complex_cell(b.push(R, OP_CELL_BWD, 200 + l).cell, l, t, false, dh, dcb, dgates);
          if (t > 0)
            for (int set = 0; set < 2; ++set) {
              RunGemm g = rb[set];
              g.base[0] = (int64_t)t * 8 * H + (int64_t)set * 4 * H;
              g.y_off = (int)((int64_t)set * BT * H + (int64_t)(t - 1) * H);
              b.push(R, OP_RUNGEMM, 200 + l).g = g;
            }
        }
      }
      auto dyp = [&](int p) { return b.mk(A_WS, dgates.off + (int64_t)p * dg_half); };      // dgates of part p
      b.cur_lane = lane_all ? 1 : 0;
      for (int p = 0; p < 2; ++p)
        for (size_t ck = 0; ck < ls[l].gxc[p].size(); ++ck) {
          RunGemm fw = ls[l].gxc[p][ck];
          fw.ydt = adt;                     // WGRAD reads dy = dgates (act dtype), not the fp32 gx the forward wrote
          fw.flags &= ~kRunAccum;
          b.wgrad(R, fw, dyp(p), ls[l].cgxc[p][ck], 200 + l, ck == 0 ? &ls[l].bgx : nullptr);
        }
      for (int g4 = 0; g4 < 4; ++g4) {       // W_hh: dW[n][k] = sum_t dgates[g][t][n] * h[g][t-1][k]
        const int p = g4 / 2, set = g4 % 2;
        RunGemm f = b.rows_gemm(b.mk(A_WS, ls[l].h.off + (int64_t)g4 * BT * H * esize(adt)), adt, H, 0, H, 4 * H, adt);
        f.seg[0].dt = -1;
        b.rows_out(f, dyp(p), 8 * H, set * 4 * H);
        const ParamInfo* Wp = Whh[set];
        Builder::Coef coef = [=](int nn, int sg, int j) -> int32_t { return pe(*Wp, (int64_t)gate_torch_row(nn, H) * H + j, 1); };
        b.wgrad(R, f, dyp(p), coef, 200 + l, nullptr);
      }
      b.cur_lane = 0;
      // input gradient of the layer
      Ptr dx_full;
      if (l > 0) dx_full = b.ws("dhc" + std::to_string(l - 1), BT * 2 * H, DT_F32);
      // Layer 0 in bf16: ONE GEMM over both gate halves (two sources, K = 2 x 8H) with block weights - the half of the K range that
      // does not feed an output column is zero - writing the whole [D][Cl] row of d_encz contiguously, instead of 2 x D launches of
      // N = Cl / 2 (M = B*T rows only: 8 x 24 us of latency-bound tiles vs one wide-tile launch; twice the MACs, 65 GFLOP).
      const bool dx_merge = l == 0 && adt == DT_BF16 && (D * Cl) % 256 == 0 && (8 * H) % 64 == 0 &&
                            tune_on("DX_MERGE");
      if (dx_merge) {
        RunGemm g = b.rows_gemm(dyp(0), adt, 8 * H, 0, 8 * H, D * Cl, adt);
        g.x[1] = dyp(1); g.bstride[1] = g.bstride[0]; g.tstride[1] = 8 * H; g.rowlen[1] = 8 * H; g.Tin[1] = T;     // part 1: a second source
        g.nseg = 2; g.seg[1] = Seg{1, 0, 0, 8 * H, 0};
        Builder::layout_segs(g);
        const Builder::Coef cf0 = ls[l].cgx[0], cf1 = ls[l].cgx[1];
        const int Ch = Cl / 2;
        Builder::Coef coef = [=](int nn, int sg, int j) -> int32_t {
          const int q = nn / Cl, rem = nn % Cl, p = rem / Ch, c = rem % Ch;
          if (sg != p) return 0;
          return (p == 0 ? cf0 : cf1)(j, q, c);
        };
        b.pack_weights(R, g, coef, nm + ".dxm", 200 + l);
        b.rows_out(g, enc[n - 1].dz, D * Cl);
        b.push(R, OP_RUNGEMM, 200 + l).g = g;
      }
      for (int p = 0; p < (dx_merge ? 0 : 2); ++p) {
        const int nout = l == 0 ? D : 1;
        for (int q = 0; q < nout; ++q) {
          RunGemm g = b.rows_gemm(dyp(p), adt, 8 * H, 0, 8 * H, l == 0 ? Cl / 2 : H, l == 0 ? adt : DT_F32);
          const Builder::Coef cf = ls[l].cgx[p];
          Builder::Coef coef = [=](int nn, int sg, int j) -> int32_t { return l == 0 ? cf(j, q, nn) : cf(j, 0, nn); };
          b.pack_weights(R, g, coef, nm + ".dx" + std::to_string(p) + "_" + std::to_string(q), 200 + l);
          if (l == 0) b.rows_out(g, enc[n - 1].dz, D * Cl, q * Cl + p * (Cl / 2)); else b.rows_out(g, dx_full, 2 * H, p * H);
          b.push(R, OP_RUNGEMM, 200 + l).g = g;
        }
      }
      if (l > 0) dhc_next = dx_full;
    }
    // ---- data-parallel overlap: the gradients of decoder + LSTM (flat range [decoder.0 ..., end)) are complete here - every
    // weight gradient GEMM and BatchNorm parameter gradient that writes them has been planned above.  Their UNPACK goes here, so
    // a caller can start their all-reduce while the encoder backward still runs (sefd_plan_grad_bucket / sefd_plan_run_cb).
    // The folds of the decoder + LSTM weight gradients (3/4 of the 1.2 GB of partial sums of a step) go here, on the weight-gradient lane:
    // a bandwidth-bound pass beside the encoder's input-gradient GEMMs instead of in front of the final UNPACK on the main stream.
    if (tune_on("SPLITSUM_MID")) b.flush_sums(R, 997, true);
    // Without an exchange (one bucket) the same early UNPACK rides the weight-gradient lane (tag 997): the gather of 83 % of the parameters
    // leaves the tail of the main stream (79 us for all of them in front of Adam before); UNPACK_MID=0 keeps the single UNPACK.
    const bool unpack_mid = cfg.grad_buckets < 2 && tune_on("UNPACK_MID");
    if (cfg.grad_buckets >= 2 || unpack_mid) {
      const int64_t lo = b.par("decoder.0.0.real_conv.weight").off;
      b.flush_sums(R, 997, unpack_mid);                      // (nothing pending unless SPLITSUM_MID=0)
      if (unpack_mid) b.cur_lane = 1;
      b.unpack_range(R, lo, nparam, unpack_mid ? 997 : 998);
      b.cur_lane = 0;
      b.unpack_hi = lo;
      if (!unpack_mid) P->bucket_elem = lo;                  // (the op index is looked up after the op list is final)
    }
    // ---- encoder backward
    for (int i = n - 1; i >= 0; --i) {
      const int Ci = ch[i], Co = ch[i + 1], Fi = Fe[i], Fo = Fe[i + 1];
      const std::string nm = "enc" + std::to_string(i);
      const std::string pp = "encoder." + std::to_string(i);
      // First layer on the spectrum (enc0.hip): it has no input gradient, so its BatchNorm input gradient dy is read by the weight gradient alone -
      // BN_BWD_APPLY is not planned, the weight-gradient kernel takes dz through the BatchNorm + PReLU backward as it loads it (kRunDyFromBn) and runs on
      // the MAIN stream right behind BN_BWD_FINALIZE: apply (117 us) -> fold -> weight gradient (52 us) was the serial tail of the step.  ENC0_BNFUSE=0: off
      const bool dy_fused = i == 0 && (enc[0].f[0].flags & kRunEnc0) && enc0_accepts(enc[0].f[0], true) && !cbn &&    // (its weight gradient's form: sefd_desc.h)
                            tune_on("ENC0_BNFUSE");
      const BnBwdApply bnb = b.bn_bwd(R, 100 + i, enc[i].y, enc[i].dz, cfg.skip ? enc[i].dskip : b.none(), enc[i].mi, pp, Co, enc[i].R, (int64_t)T * Fo, 0,
                                      enc[i].dy, nm, cbn, &bnb_enc[i], dy_fused);
      // the folds of enc5 .. enc1 go in front of the LAST weight gradient on its lane (its input is the last thing the dgrad chain produces,
      // the lane usually waits for it): the fold in front of the final UNPACK then covers one thin layer
      if (i == 0 && lane_all && n > 1 && tune_on("SPLITSUM_MID")) b.flush_sums(R, 996, true);
      b.cur_lane = (lane_all && !dy_fused) ? 1 : 0;             // encoder weight gradients next to the dgrad chain
      // Every encoder conv bias sits in front of a training-mode BatchNorm: its gradient is identically zero (the sum over all rows of the
      // BatchNorm input gradient vanishes; the reference computes rounding noise there).  No bias "ones" run in these GEMMs - it cost a
      // whole 64-column K segment (enc0: 192 -> 128 columns, half the K tiles; enc3: 6 -> 5 wide tiles) - UNPACK writes the exact zero.
      const bool enc_bias_zero = tune_on("ENC_BIAS_ZERO");
      if (enc_bias_zero) {
        b.zero_grad.resize(nparam, 0);
        for (const char* part : {".0.real_conv.bias", ".0.imag_conv.bias"}) {
          const ParamInfo& pb = b.par(pp + part);
          for (int64_t e = 0; e < pb.numel; ++e) b.zero_grad[pb.off + e] = 1;
        }
      }
      b.wgrad(R, enc[i].f[0], dy_fused ? enc[i].dz : enc[i].dy, enc[i].coef[0], 100 + i, enc_bias_zero ? nullptr : &enc[i].bias);
      if (dy_fused) {
        for (size_t q = R.size(); q-- > 0;)
          if (R[q].kind == OP_WGRAD && R[q].tag == 100 + i) {
            RunGemm& g = R[q].g;
            g.flags |= kRunDyFromBn;
            g.bnb_dz1 = cfg.skip ? enc[i].dskip : b.none();
            g.bnb_y = enc[i].y; g.bnb_mi = enc[i].mi;
            g.bnb_gamma = b.pptr(pp + ".1.weight"); g.bnb_beta = b.pptr(pp + ".1.bias"); g.bnb_slope = b.pptr(pp + ".2.weight");
            g.bnb_bstride = g.y_bstride; g.bnb_tstride = g.y_tstride; g.bnb_fstride = g.y_fstride; g.bnb_off = g.y_off;
            // per-rank count: like every descriptor that carries a BatchNorm count, this one must be scaled by the SyncBN post-pass (finalize_rungemms)
            g.bnb_totals = bnb.totals; g.bnb_inv_count = (float)(1.0 / bnb.count);
            break;
          }
      }
      b.cur_lane = 0;
      if (i == 0) continue;
      // dx[ci,f,t] = sum W[co,ci,kh,kw] dy[co,(f+2-kh)/2, t+1-kw]  -> two sub-pixel phases over dy [B][T][Fo][Co]
      // thin layers: both phases in one GEMM over the even phase's runs (see the decoder forward), unless this layer's BatchNorm sums
      // ride in the epilogue (their partial rows have one column per channel)
      const int merge_maxn = (int)tune_int("PHASE_MERGE_MAXN", 64);
      if (Ci <= merge_maxn && !bnb_enc[i - 1].on) {
        RunGemm g = Builder::gemm0();
        g.x[0] = enc[i].dy; g.xdt = adt; g.ydt = adt;
        g.bstride[0] = (int64_t)T * Fo * Co; g.tstride[0] = Fo * Co; g.rowlen[0] = Fo * Co; g.fstride[0] = Co; g.Tin[0] = T;
        g.M = B * T * Fo; g.Tout = T; g.Fo = Fo;
        g.nseg = 2;
        g.seg[0] = Seg{0, 1, -Co, 3 * Co, 0};
        g.seg[1] = Seg{0, 0, -Co, 3 * Co, 0};
        g.N = 2 * Ci;
        Builder::layout_segs(g);
        const Builder::Coef cf = enc[i].coef[0];
        Builder::Coef coef = [=](int nn, int sg, int j) -> int32_t {
          const int kw = sg, jj = j / Co, co = j % Co, par = nn / Ci;
          if (par > 1 || (par == 1 && jj == 0)) return 0;
          const int kh = par == 0 ? 4 - 2 * jj : 5 - 2 * jj;
          return cf(co, kw, kh * Ci + nn % Ci);
        };
        b.pack_weights(R, g, coef, nm + ".dgm", 100 + i);
        g.y = enc[i - 1].dz; g.y_bstride = (int64_t)T * Fi * Ci; g.y_tstride = Fi * Ci; g.y_fstride = 2 * Ci; g.y_off = 0;
        b.push(R, OP_RUNGEMM, 100 + i).g = g;
        continue;
      }
      for (int par = 0; par < 2; ++par) {
        RunGemm g = b.enc_dgrad(R, 100 + i, nm, enc[i], Ci, Fi, par, enc[i - 1].dz);
        bnb_attach(g, bnb_enc[i - 1], (int64_t)T * Fi * Ci, Fi * Ci, 2 * Ci, par * Ci);      // rows of encoder layer i-1's output, this phase's bins
        b.push(R, OP_RUNGEMM, 100 + i).g = g;
      }
    }
    b.finish_unpack(R);
  }

  finish_plan(b, P, nparam, nstate);
  for (size_t k = 0; k < P->bwd.size(); ++k)
    if (P->bwd[k].kind == OP_UNPACK && P->bwd[k].tag == 998) P->bucket_op = (int32_t)k;
  return P;
}

}  // namespace sefd
