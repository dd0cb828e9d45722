#include "plan_builder.h"

namespace sefd {

// NavieComplexLSTM on its own (reference tools_for_model.py:141-181): one complex LSTM layer, optionally bidirectional, + r_trans / i_trans.  model == 11.
// Config fields reused: kernel_num = {I per part, H per part, P per part (0: no projection), bidirectional}; cfg.B = sequences, cfg.L = frames T.
// Plan boundary, batch-major fp32 (the layout of DCCRN's recurrent block, plan_dccrn.cpp): io.x [B][T][2 IP] (real part | imaginary part, IP = roundup(I, 8),
// pad columns zero) -> with a projection io.y [B][T][2 P] (real | imag); without one the combined outputs are the workspace buffer `hc` [D][B][T][2 H]
// (direction, real | imag) in the activation dtype.  Backward: io.grad_y, [B][T][2 P] or [D][B][T][2 H], -> A_GRAD and io.grad_x [B][T][2 IP].  The
// [T, B, .] permutes, the pad and the concatenations of halves stay with the caller.
//
// A direction d is one complex layer of DCCRN's stack on buffers of its own: the hoisted input GEMM per part with the two sets' W_ih side by side (unit-
// major gate columns, N = 8 H), gx / dgates [part][B*T][set][4H], h / c / dh [group = (part, set)][B*T][H], one LstmRec with G = 4, nset = 2, then
// OP_COMBINE_FWD/BWD.  Direction 1 walks the frames last to first: LstmRec::rev_mask = 0b1111, t0 = t1 = 0; its "previous" frame is t + 1.
// The recurrence is, chosen per plan by DCCRN's rules:
//   * persistent (H <= 128, H % 16 == 0 in fp32, H % 32 == 0 in bf16): kernels.hip / lstm_bf16.hip.  The reverse launch rides the second stream (lane 2):
//     a launch fills ceil(B / RPW) x 4 workgroups of 256 CUs and is latency bound, so the two directions run side by side and join before the combine;
//   * cluster (bf16, 128 < H <= 512, H % 64 == 0): lstm_cluster.hip, the two launches one after the other on the main stream - the workgroups of a
//     cluster launch wait for each other's frames, two such grids competing for CUs would only lengthen those waits;
//   * stepped (anything else, or knob LSTM_STEPPED): per frame one recurrent GEMM per set + one four-group cell launch; the reverse direction is the
//     same ops in the other frame order.
// The projection reads the directions' combined outputs as the two sources of ONE RUNGEMM (block matrix of r_trans / i_trans): no concatenated copy.
Plan* build_clstm_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  Builder b;
  b.P = P;
  b.c = cfg;
  const int B = cfg.B, T = cfg.L;
  const int I = cfg.kernel_num[0], H = cfg.kernel_num[1], Pp = cfg.kernel_num[2];
  const int D = cfg.kernel_num[3] ? 2 : 1;
  const int adt = cfg.act_dtype;
  P->T = T;
  P->NF = Pp > 0 ? Pp : D * H;
  if (I < 1 || H < 1 || Pp < 0 || T < 1 || B < 1) {
    P->error = "ComplexLSTM: input_size / 2, hidden_size / 2, projection_dim / 2, the number of frames and of sequences must be at least 1";
    return P;
  }
  if (H % 8) { P->error = "ComplexLSTM: hidden_size / 2 must be a multiple of 8"; return P; }
  const int IP = (int)rup(I, 8);
  const int64_t BT = (int64_t)B * T;
  if (BT * 8 * H >= (1LL << 31) || BT * 2 * IP >= (1LL << 31)) { P->error = "ComplexLSTM: sequences x frames x 8 x hidden_size / 2 must stay below 2^31"; return P; }
  b.fe.B = B; b.fe.T = T;                                  // rows_gemm / rows_out: rows (sequence, frame)

  const char* lstm_nm[2] = {"real_lstm", "imag_lstm"};    // parameter set 0 / 1
  auto sfx = [](int d) { return std::string(d ? "_l0_reverse" : "_l0"); };
  for (int set = 0; set < 2; ++set)
    for (int d = 0; d < D; ++d) {
      const std::string pp = std::string(lstm_nm[set]) + ".";
      b.add_param(pp + "weight_ih" + sfx(d), {4 * H, I}, true);
      b.add_param(pp + "weight_hh" + sfx(d), {4 * H, H}, true);
      b.add_param(pp + "bias_ih" + sfx(d), {4 * H}, true);
      b.add_param(pp + "bias_hh" + sfx(d), {4 * H}, true);
    }
  if (Pp > 0)
    for (const char* t : {"r_trans", "i_trans"}) {
      b.add_param(std::string(t) + ".weight", {Pp, D * H}, true);
      b.add_param(std::string(t) + ".bias", {Pp}, true);
    }
  const int64_t nparam = P->params.back().off + P->params.back().numel;
  b.inv.resize(nparam);
  const int NO = Pp > 0 ? 2 * Pp : 2 * H;                  // columns of a row of io.grad_y
  Ptr io_x = b.io("x", BT * 2 * IP);
  Ptr io_y = Pp > 0 ? b.io("y", BT * 2 * Pp) : b.none();
  Ptr io_gy = b.io("grad_y", (Pp > 0 ? 1 : D) * BT * NO);
  Ptr io_gx = b.io("grad_x", BT * 2 * IP);
  std::vector<Op>& F = P->fwd;
  std::vector<Op>& R = P->bwd;

  const bool cluster = adt == DT_BF16 && H > 128 && H <= 512 && H % 64 == 0;
  const bool persistent = H <= 128 && H % (adt == DT_BF16 ? 32 : 16) == 0;
  const bool stepped = !(cluster || persistent) || tune_has("LSTM_STEPPED");
  const bool side = D == 2 && !stepped && persistent;     // the reverse recurrence on the second stream

  auto at = [&](Ptr p, int64_t elems, int dt) { return b.mk(p.arena, p.off + elems * esize(dt)); };
  // fp32 -> activation dtype at the boundary of a bf16 plan: an fp32-operand GEMM with a constant identity matrix (exact: one product per output) whose
  // epilogue rounds to bf16, as plan_seq.cpp does; fp32 plans read the I/O block directly
  auto to_act = [&](std::vector<Op>& ops, Ptr src, int ld, const std::string& name, int tag) -> Ptr {
    if (adt == DT_F32) return src;
    Ptr dst = b.ws(name, BT * ld, adt);
    RunGemm g = b.rows_gemm(src, DT_F32, ld, 0, ld, ld, adt);
    b.const_weights(g, [](int n, int j) { return n == j ? 1.0 : 0.0; });
    b.rows_out(g, dst, ld);
    b.push(ops, OP_RUNGEMM, tag).g = g;
    return dst;
  };
  auto gx_goff = [=](int g4) { return (int64_t)(g4 / 2) * BT * 8 * H + (int64_t)(g4 % 2) * 4 * H; };

  struct Dir {
    const ParamInfo *Wih[2], *Whh[2], *bih[2], *bhh[2];
    Ptr gxb, h, gates, cst, hc, dh, dgates;
    RunGemm gx[2];
    Builder::Coef cgx;
    Builder::Bias bgx;
  };
  Dir ds[2];
  for (int d = 0; d < D; ++d)
    for (int set = 0; set < 2; ++set) {
      const std::string pp = std::string(lstm_nm[set]) + ".";
      ds[d].Wih[set] = &b.par(pp + "weight_ih" + sfx(d)); ds[d].Whh[set] = &b.par(pp + "weight_hh" + sfx(d));
      ds[d].bih[set] = &b.par(pp + "bias_ih" + sfx(d)); ds[d].bhh[set] = &b.par(pp + "bias_hh" + sfx(d));
    }
  // the recurrence of direction d (backward: with dh and dgates)
  auto lstm_desc = [&](int d, Ptr dh, Ptr dgates, int gdt) {
    const Dir& Q = ds[d];
    LstmRec r;
    std::memset(&r, 0, sizeof(r));
    r.gx = Q.gxb;
    r.whh[0] = b.mk(A_PARAM, Q.Whh[0]->off * 4); r.whh[1] = b.mk(A_PARAM, Q.Whh[1]->off * 4);
    r.h = Q.h; r.gates = Q.gates; r.c = Q.cst; r.dh = dh; r.dgates = dgates;
    for (int g4 = 0; g4 < 4; ++g4) r.gx_goff[g4] = gx_goff(g4);
    r.gx_ld = 8 * H; r.G = 4; r.nset = 2; r.B = B; r.T = T; r.H = H; r.hdt = adt; r.gdt = gdt;
    r.rev_mask = d ? 0xF : 0;                              // never chunked: t0 = t1 = 0
    return r;
  };
  // the cell launch of frame t of the stepped path over the 4 groups; tp: the direction's previous frame (-1: none, its first step)
  auto complex_cell = [&](LstmCell& cl, int d, int t, int tp, bool first, bool fwd) {
    const Dir& Q = ds[d];
    std::memset(&cl, 0, sizeof(cl));
    cl.gates = at(Q.gxb, (int64_t)t * 8 * H, DT_F32);
    cl.c = at(Q.cst, (int64_t)t * H, DT_F32);
    cl.c_prev = tp >= 0 ? at(Q.cst, (int64_t)tp * H, DT_F32) : b.none();
    cl.h = fwd ? at(Q.h, (int64_t)t * H, adt) : b.none();
    cl.dh = fwd ? b.none() : at(Q.dh, (int64_t)t * H, DT_F32);
    cl.dc = b.none();
    cl.dgates = fwd ? b.none() : at(Q.dgates, (int64_t)t * 8 * H, adt);
    cl.gh = b.none();
    cl.rows = 4 * B; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = first; cl.kind = 0;
    cl.G = 4; cl.Bg = B; cl.unit_major = 1;
    cl.rs[0] = (int64_t)T * 8 * H; cl.rs[1] = cl.rs[2] = cl.rs[3] = (int64_t)T * H; cl.rs[4] = (int64_t)T * 8 * H;
    for (int g4 = 0; g4 < 4; ++g4) {
      cl.go[0][g4] = cl.go[4][g4] = gx_goff(g4);
      cl.go[1][g4] = cl.go[2][g4] = cl.go[3][g4] = (int64_t)g4 * BT * H;
    }
  };

  // =================================================================================================== forward
  Ptr x_in = to_act(F, io_x, 2 * IP, "x_act", 90);
  Ptr hcall = b.ws("hc", D * BT * 2 * H, adt);
  for (int d = 0; d < D; ++d) {
    Dir& Q = ds[d];
    const int tag = 200 + d;
    const std::string dn = d ? "r" : "f";
    Q.gxb = b.ws("gx." + dn, 2 * BT * 8 * H, DT_F32);
    Q.h = b.ws("h." + dn, 4 * BT * H, adt);
    Q.gates = stepped ? Q.gxb : b.ws("gates." + dn, 4 * BT * 4 * H, DT_F32);     // stepped: i, f, g, o overwrite the pre-activations in place
    Q.cst = b.ws("c." + dn, 4 * BT * H, DT_F32);
    Q.hc = at(hcall, d * BT * 2 * H, adt);
    const ParamInfo *W0 = Q.Wih[0], *W1 = Q.Wih[1], *bi0 = Q.bih[0], *bi1 = Q.bih[1], *bh0 = Q.bhh[0], *bh1 = Q.bhh[1];
    Q.cgx = [=](int nn, int s, int j) -> int32_t {
      const int set = nn / (4 * H), gq = gate_torch_row(nn % (4 * H), H);
      return j < I ? pe(set ? *W1 : *W0, (int64_t)gq * I + j, 1) : 0;              // pad columns have no weight
    };
    Q.bgx = [=](int nn, int32_t* o) {
      const int set = nn / (4 * H), gq = gate_torch_row(nn % (4 * H), H);
      o[0] = pe(set ? *bi1 : *bi0, gq, 1); o[1] = pe(set ? *bh1 : *bh0, gq, 1);
    };
    // the two parts share the packed weights (the sets' W_ih side by side) and differ in the input columns and the output slab
    for (int p = 0; p < 2; ++p) {
      RunGemm g = b.rows_gemm(x_in, adt, 2 * IP, p * IP, IP, 8 * H, DT_F32);
      if (p == 0) b.pack_weights(F, g, Q.cgx, "ih." + dn, tag, &Q.bgx);
      else { g.w = Q.gx[0].w; g.bias = Q.gx[0].bias; }
      b.rows_out(g, at(Q.gxb, (int64_t)p * BT * 8 * H, DT_F32), 8 * H);
      Q.gx[p] = g;
      b.push(F, OP_RUNGEMM, tag).g = g;
    }
  }
  if (!stepped) {
    for (int d = D - 1; d >= 0; --d) {                     // the reverse launch first: the second stream starts while the main one goes on
      b.cur_lane = (side && d == 1) ? 2 : 0;
      b.push(F, OP_LSTM_FWD, 200 + d).lstm = lstm_desc(d, b.none(), b.none(), DT_F32);
      b.cur_lane = 0;
    }
  } else {
    for (int d = 0; d < D; ++d) {
      Dir& Q = ds[d];
      const int tag = 200 + d;
      const std::string dn = d ? "r" : "f";
      // per step: gx[t] += h[previous frame] . W_hh^T (one GEMM per parameter set over the 2B rows (part, sequence)), then one cell launch over the 4 groups
      RunGemm hh[2];
      for (int set = 0; set < 2; ++set) {
        RunGemm g = Builder::gemm0();
        g.x[0] = Q.h; g.xdt = adt; g.ydt = DT_F32;
        g.bstride[0] = 0; g.tstride[0] = (int)(2 * BT * H); g.fstride[0] = T * H; g.rowlen[0] = (int)(BT * H); g.Tin[0] = 2;
        g.M = 2 * B; g.Tout = 2; g.Fo = B;
        g.nseg = 1; g.seg[0] = Seg{0, 0, 0, H, 0};
        g.N = 4 * H;
        Builder::layout_segs(g);
        const ParamInfo* Wp = Q.Whh[set];
        Builder::Coef chh = [=](int nn, int sg, int j) -> int32_t { return pe(*Wp, (int64_t)gate_torch_row(nn, H) * H + j, 1); };
        b.pack_weights(F, g, chh, "hh" + std::to_string(set) + "." + dn, tag);
        g.y = Q.gxb; g.y_bstride = 0; g.y_tstride = (int)(BT * 8 * H); g.y_fstride = T * 8 * H; g.flags = kRunAccum;
        hh[set] = g;
      }
      for (int k = 0; k < T; ++k) {
        const int t = d ? T - 1 - k : k, tp = d ? t + 1 : t - 1;
        if (k > 0)
          for (int set = 0; set < 2; ++set) {
            RunGemm g = hh[set];
            g.base[0] = (int64_t)set * BT * H + (int64_t)tp * H;
            g.y_off = t * 8 * H + set * 4 * H;
            b.push(F, OP_RUNGEMM, tag).g = g;
          }
        complex_cell(b.push(F, OP_CELL_FWD, tag).cell, d, t, k > 0 ? tp : -1, k == 0, true);
      }
    }
  }
  for (int d = 0; d < D; ++d) {
    Op& op = b.push(F, OP_COMBINE_FWD, 200 + d);
    if (side && d == 1) op.join = 1;                       // the main stream needs the reverse recurrence
    op.comb.h = ds[d].h; op.comb.out = ds[d].hc; op.comb.rows = BT; op.comb.H = H; op.comb.dt = adt; op.comb.T = T;
  }
  // projection r_trans / i_trans (tools_for_model.py:173-175) over [real_fwd | real_rev] and [imag_fwd | imag_rev]: one GEMM, source s = direction s
  RunGemm projg;
  Builder::Coef cproj;
  Builder::Bias bproj;
  if (Pp > 0) {
    const ParamInfo* Wt[2] = {&b.par("r_trans.weight"), &b.par("i_trans.weight")};
    const ParamInfo* bt[2] = {&b.par("r_trans.bias"), &b.par("i_trans.bias")};
    const ParamInfo *Wt0 = Wt[0], *Wt1 = Wt[1], *bt0 = bt[0], *bt1 = bt[1];
    cproj = [=](int nn, int s, int j) -> int32_t {
      const int p = nn >= Pp ? 1 : 0, q = nn - p * Pp;
      if ((j >= H) != (p == 1)) return 0;
      return pe(p ? *Wt1 : *Wt0, (int64_t)q * D * H + s * H + (j - p * H), 1);
    };
    bproj = [=](int nn, int32_t* o) { const int p = nn >= Pp ? 1 : 0; o[0] = pe(p ? *bt1 : *bt0, nn - p * Pp, 1); o[1] = 0; };
    RunGemm g = b.rows_gemm(ds[0].hc, adt, 2 * H, 0, 2 * H, 2 * Pp, DT_F32);
    if (D == 2) {
      g.x[1] = ds[1].hc; g.bstride[1] = g.bstride[0]; g.tstride[1] = 2 * H; g.rowlen[1] = 2 * H; g.Tin[1] = T;
      g.nseg = 2; g.seg[1] = Seg{1, 0, 0, 2 * H, 0};
      Builder::layout_segs(g);
    }
    b.pack_weights(F, g, cproj, "proj", 300, &bproj);
    b.rows_out(g, io_y, 2 * Pp);
    b.push(F, OP_RUNGEMM, 300).g = g;
    projg = g;
  }

  // =================================================================================================== backward
  if (cfg.training) {
    Ptr dhc[2];                                            // gradient of a direction's combined output, fp32 [B*T][2H]
    if (Pp > 0) {
      Ptr dy = to_act(R, io_gy, 2 * Pp, "dy_act", 300);
      { RunGemm fw = projg; fw.ydt = adt; fw.flags = 0; b.wgrad(R, fw, dy, cproj, 300, &bproj); }
      for (int d = 0; d < D; ++d) {
        dhc[d] = b.ws(std::string("dhc.") + (d ? "r" : "f"), BT * 2 * H, DT_F32);
        RunGemm g = b.rows_gemm(dy, adt, 2 * Pp, 0, 2 * Pp, 2 * H, DT_F32);
        const Builder::Coef cf = cproj;
        Builder::Coef coef = [=](int nn, int sg, int j) -> int32_t { return cf(j, d, nn); };
        b.pack_weights(R, g, coef, std::string("proj.dg.") + (d ? "r" : "f"), 300);
        b.rows_out(g, dhc[d], 2 * H);
        b.push(R, OP_RUNGEMM, 300).g = g;
      }
    } else {
      for (int d = 0; d < D; ++d) dhc[d] = at(io_gy, d * BT * 2 * H, DT_F32);
    }
    for (int d = 0; d < D; ++d) {
      Dir& Q = ds[d];
      const std::string dn = d ? "r" : "f";
      Q.dh = b.ws("dh." + dn, 4 * BT * H, DT_F32);
      Q.dgates = b.ws("dgates." + dn, 2 * BT * 8 * H, adt);
      Op& op = b.push(R, OP_COMBINE_BWD, 200 + d);
      op.comb.h = Q.dh; op.comb.out = dhc[d]; op.comb.rows = BT; op.comb.H = H; op.comb.dt = DT_F32; op.comb.T = T;
    }
    if (!stepped) {
      for (int d = D - 1; d >= 0; --d) {
        b.cur_lane = (side && d == 1) ? 2 : 0;
        b.push(R, OP_LSTM_BWD, 200 + d).lstm = lstm_desc(d, ds[d].dh, ds[d].dgates, adt);
        b.cur_lane = 0;
      }
    } else {
      for (int d = 0; d < D; ++d) {
        Dir& Q = ds[d];
        const int tag = 200 + d;
        const std::string dn = d ? "r" : "f";
        // per step, the direction's last to its first: cell backward (dgates[t], carry dc), then dh[previous frame] += dgates[t] . W_hh per parameter set
        Ptr dcb = b.ws("dc." + dn, (int64_t)4 * B * H, DT_F32);
        RunGemm rb[2];
        for (int set = 0; set < 2; ++set) {
          RunGemm g = Builder::gemm0();
          g.x[0] = Q.dgates; g.xdt = adt; g.ydt = DT_F32;
          g.bstride[0] = 0; g.tstride[0] = (int)(BT * 8 * H); g.fstride[0] = T * 8 * H; g.rowlen[0] = (int)(BT * 8 * H); g.Tin[0] = 2;
          g.M = 2 * B; g.Tout = 2; g.Fo = B;
          g.nseg = 1; g.seg[0] = Seg{0, 0, 0, 4 * H, 0};
          g.N = H;
          Builder::layout_segs(g);
          const ParamInfo* Wp = Q.Whh[set];
          Builder::Coef cT = [=](int nn, int sg, int j) -> int32_t { return pe(*Wp, (int64_t)gate_torch_row(j, H) * H + nn, 1); };
          b.pack_weights(R, g, cT, "hhT" + std::to_string(set) + "." + dn, tag);
          g.y = Q.dh; g.y_bstride = 0; g.y_tstride = (int)(2 * BT * H); g.y_fstride = T * H; g.flags = kRunAccum;
          rb[set] = g;
        }
        for (int k = T - 1; k >= 0; --k) {
          const int t = d ? T - 1 - k : k, tp = d ? t + 1 : t - 1;
          LstmCell& cl = b.push(R, OP_CELL_BWD, tag).cell;
          complex_cell(cl, d, t, k > 0 ? tp : -1, k == T - 1, false);
          cl.dc = dcb;
          if (k > 0)
            for (int set = 0; set < 2; ++set) {
              RunGemm g = rb[set];
              g.base[0] = (int64_t)t * 8 * H + (int64_t)set * 4 * H;
              g.y_off = (int)((int64_t)set * BT * H + (int64_t)tp * H);
              b.push(R, OP_RUNGEMM, tag).g = g;
            }
        }
      }
    }
    const size_t after_rec = R.size();                     // the first op behind the recurrences waits for the second stream
    for (int d = 0; d < D; ++d) {
      Dir& Q = ds[d];
      const int tag = 200 + d;
      auto dyp = [&](int p) { return at(Q.dgates, (int64_t)p * BT * 8 * H, adt); };      // dgates of part p
      for (int p = 0; p < 2; ++p) {                        // W_ih and both biases: the forward descriptor of the part against its gate gradients
        RunGemm fw = Q.gx[p];
        fw.ydt = adt;
        fw.flags &= ~kRunAccum;
        b.wgrad(R, fw, dyp(p), Q.cgx, tag, &Q.bgx);
      }
      for (int g4 = 0; g4 < 4; ++g4) {                     // W_hh: dW[n][k] = sum_t dgates[g][t][n] * h[g][the direction's previous frame][k]
        const int p = g4 / 2, set = g4 % 2;
        RunGemm f = b.rows_gemm(at(Q.h, (int64_t)g4 * BT * H, adt), adt, H, 0, H, 4 * H, adt);
        f.seg[0].dt = d ? 1 : -1;
        b.rows_out(f, dyp(p), 8 * H, set * 4 * H);
        const ParamInfo* Wp = Q.Whh[set];
        Builder::Coef coef = [=](int nn, int sg, int j) -> int32_t { return pe(*Wp, (int64_t)gate_torch_row(nn, H) * H + j, 1); };
        b.wgrad(R, f, dyp(p), coef, tag, nullptr);
      }
    }
    if (side && after_rec < R.size()) R[after_rec].join = 1;
    // input gradient of part p: both directions (the two sources) and both sets (the 8H columns of a source) in one GEMM
    for (int p = 0; p < 2; ++p) {
      RunGemm g = b.rows_gemm(at(ds[0].dgates, (int64_t)p * BT * 8 * H, adt), adt, 8 * H, 0, 8 * H, IP, DT_F32);
      if (D == 2) {
        g.x[1] = at(ds[1].dgates, (int64_t)p * BT * 8 * H, adt); g.bstride[1] = g.bstride[0]; g.tstride[1] = 8 * H; g.rowlen[1] = 8 * H; g.Tin[1] = T;
        g.nseg = 2; g.seg[1] = Seg{1, 0, 0, 8 * H, 0};
        Builder::layout_segs(g);
      }
      const Builder::Coef c0 = ds[0].cgx, c1 = ds[D - 1].cgx;
      Builder::Coef coef = [=](int nn, int sg, int j) -> int32_t { return (sg ? c1 : c0)(j, 0, nn); };
      b.pack_weights(R, g, coef, "dx" + std::to_string(p), 200);
      b.rows_out(g, io_gx, 2 * IP, p * IP);
      b.push(R, OP_RUNGEMM, 200).g = g;
    }
    b.finish_unpack(R);
  }
  finish_plan(b, P, nparam, 0);
  return P;
}

}  // namespace sefd
