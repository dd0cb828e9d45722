#include "plan_builder.h"

namespace sefd {

// SequenceModel on its own (reference tools_for_model.py:726-795): nn.LSTM / nn.GRU of any depth, optionally bidirectional, + Linear.  model == 6.
// Config fields reused: kernel_num = {input size I, output size O, hidden H, num_layers, bidirectional, 0 LSTM / 1 GRU, dropout keep in 1/1000};
// cfg.B = sequences, cfg.L = frames T.  Plan boundary, time-major fp32: io.x [T][B][IP] (IP = roundup(I, 8), pad columns zero) -> io.y [T][B][O]
// (pre-activation); backward io.grad_y -> A_GRAD and io.grad_x [T][B][IP].  The [B, F, T] permutes and the output activation stay with the caller.
//
// A layer is D = 1 or 2 independent recurrences over the same rows.  Direction 1 is direction 0's op list with the frames visited last to first:
// its "previous" frame is t + 1.
// LSTM layers keep both directions' gate pre-activations in ONE fp32 slab [T][B][D * 4H] (direction d in columns [d * 4H, (d + 1) * 4H), gate columns
// unit-major, sefd_desc.h gate_col) and their gradients in one slab of the same shape in the activation dtype, so both directions share one hoisted input
// GEMM (N = D * 4H), one W_ih weight-gradient GEMM and one input-gradient GEMM.  The recurrence on those slabs is, chosen per plan like FullSubNet's
// full-band layers (plan_fsn.cpp):
//   * cluster (bf16, 128 < H <= 512, H % 64 == 0): both directions are the G = 2 groups of ONE launch of the cluster kernels (lstm_cluster.hip), group 1
//     reversed (LstmRec::rev_mask = 0b10), saved gates in a group-major buffer of their own;
//   * stepped (fp32, H <= 128, knob LSTM_STEPPED): per direction and frame one recurrent GEMM accumulating onto the direction's columns + one cell launch
//     in the strided form of LstmCell (row pitch D * 4H), gates overwritten in place.
// GRU layers are stepped on dense per-direction slabs (the GRU cell op addresses [rows][4H] / [rows][3H] only): per direction one hoisted input GEMM and
// one W_ih weight-gradient GEMM; the input gradient is still one GEMM per lower direction, its two sources the two directions' gate gradients.
// Layers above a bidirectional layer, and the head, read [h_fwd | h_rev] as the two sources of one RUNGEMM: no concatenated copy exists.
constexpr int kSeqMaxLayers = 8;

Plan* build_seq_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  Builder b;
  b.P = P;
  b.c = cfg;
  const int B = cfg.B, T = cfg.L;
  const int I = cfg.kernel_num[0], O = cfg.kernel_num[1], H = cfg.kernel_num[2], NL = cfg.kernel_num[3];
  const int D = cfg.kernel_num[4] ? 2 : 1;
  const bool gru = cfg.kernel_num[5] == 1;
  const float keep = cfg.training ? cfg.kernel_num[6] / 1000.f : 1.f;
  const int NG = gru ? 3 : 4;
  const int adt = cfg.act_dtype;
  const int IP = (int)rup(std::max(I, 1), 8);
  const int64_t rows = B;
  P->T = T;
  P->NF = O;
  if (NL < 1 || NL > kSeqMaxLayers) { P->error = "SequenceModel: num_layers must lie in 1 .. " + std::to_string(kSeqMaxLayers); return P; }
  if (H < 8 || H % 8) { P->error = "SequenceModel: hidden_size must be a multiple of 8"; return P; }
  if (I < 1 || O < 1 || T < 1 || B < 1) { P->error = "SequenceModel: input_size, output_size, the number of frames and of sequences must be at least 1"; return P; }
  if (cfg.kernel_num[5] < 0 || cfg.kernel_num[5] > 1) { P->error = "SequenceModel: sequence model must be 0 (LSTM) or 1 (GRU)"; return P; }
  if (!(keep > 0.f) || keep > 1.f) { P->error = "SequenceModel: dropout keep must lie in (0, 1]"; return P; }

  const std::string pp = "sequence_model.";
  auto sfx = [](int l, int d) { return "_l" + std::to_string(l) + (d ? "_reverse" : ""); };
  for (int l = 0; l < NL; ++l)
    for (int d = 0; d < D; ++d) {
      b.add_param(pp + "weight_ih" + sfx(l, d), {NG * H, l == 0 ? I : D * H}, true);
      b.add_param(pp + "weight_hh" + sfx(l, d), {NG * H, H}, true);
      b.add_param(pp + "bias_ih" + sfx(l, d), {NG * H}, true);
      b.add_param(pp + "bias_hh" + sfx(l, d), {NG * H}, true);
    }
  b.add_param("fc_output_layer.weight", {O, D * H}, true);
  b.add_param("fc_output_layer.bias", {O}, true);
  const int64_t nparam = P->params.back().off + P->params.back().numel;
  b.inv.resize(nparam);
  Ptr io_x = b.io("x", (int64_t)T * B * IP);
  Ptr io_y = b.io("y", (int64_t)T * B * O);
  Ptr io_gy = b.io("grad_y", (int64_t)T * B * O);
  Ptr io_gx = b.io("grad_x", (int64_t)T * B * IP);
  Ptr io_seed = b.io("seed", 2);
  std::vector<Op>& Fw = P->fwd;
  std::vector<Op>& R = P->bwd;

  const bool cluster = !gru && adt == DT_BF16 && H > 128 && H <= 512 && H % 64 == 0 && !tune_has("LSTM_STEPPED");
  const int GW = D * 4 * H;                              // LSTM: width of the directions' shared gate slab

  struct Src { Ptr p; int ld, off, len; };               // columns [off, off + len) of a time-major [T][rows][ld] array
  auto at = [&](Ptr p, int64_t elems, int dt) { return b.mk(p.arena, p.off + elems * esize(dt)); };
  // time-major GEMM over all frames: rows (t, r), one run per source
  auto seq_gemm = [&](const std::vector<Src>& src, int xdt, int N, int ydt) {
    RunGemm g = Builder::gemm0();
    g.xdt = xdt; g.ydt = ydt;
    g.nseg = (int)src.size();
    for (int s = 0; s < g.nseg; ++s) {
      g.x[s] = src[s].p;
      g.bstride[s] = 0; g.tstride[s] = (int)(rows * src[s].ld); g.base[s] = 0; g.rowlen[s] = (int)(rows * src[s].ld); g.fstride[s] = src[s].ld; g.Tin[s] = T;
      g.seg[s] = Seg{s, 0, src[s].off, src[s].len, 0};
    }
    g.M = (int)(T * rows); g.Tout = T; g.Fo = (int)rows;
    g.N = N;
    Builder::layout_segs(g);
    return g;
  };
  auto set_y = [&](RunGemm& g, Ptr y, int ld, int yoff) {
    g.y = y; g.y_bstride = 0; g.y_tstride = (int)(rows * ld); g.y_fstride = ld; g.y_off = yoff;
  };
  // one frame: rows (r), source slab [rows][feat] at x, result slab at y
  auto step_gemm = [&](Ptr x, int xdt, int feat, int N, Ptr y, int ld, int ydt, int flags) {
    RunGemm g = Builder::gemm0();
    g.x[0] = x; g.xdt = xdt; g.ydt = ydt;
    g.tstride[0] = 0; g.rowlen[0] = (int)(rows * feat); g.fstride[0] = feat; g.Tin[0] = 1;
    g.M = (int)rows; g.Tout = 1; g.Fo = (int)rows;
    g.nseg = 1; g.seg[0] = Seg{0, 0, 0, feat, 0};
    g.N = N;
    Builder::layout_segs(g);
    g.y = y; g.y_fstride = ld; g.flags = flags;
    return g;
  };
  // LSTM cell on the shared slabs: the strided form of LstmCell (one group of `rows` sequences, row pitch D * 4H for gates and gate gradients, the
  // direction's column offset folded into the base pointers), unit-major gate columns
  auto strided = [&](LstmCell& cl) {
    cl.G = 1; cl.Bg = (int)rows; cl.unit_major = 1;
    cl.rs[0] = GW; cl.rs[1] = H; cl.rs[2] = H; cl.rs[3] = H; cl.rs[4] = GW;
  };
  // fp32 -> activation dtype at the plan boundary of a bf16 plan: an fp32-operand GEMM with a constant identity matrix (exact: one product per output) whose
  // epilogue rounds to bf16 - no conversion op exists, and none is needed in fp32 plans, which read the I/O block directly
  auto to_act = [&](std::vector<Op>& ops, Ptr src, int ld, const std::string& name, int tag) -> Ptr {
    if (adt == DT_F32) return src;
    Ptr dst = b.ws(name, (int64_t)T * rows * ld, adt);
    RunGemm g = seq_gemm({Src{src, ld, 0, ld}}, DT_F32, ld, adt);
    b.const_weights(g, [](int n, int j) { return n == j ? 1.0 : 0.0; });
    set_y(g, dst, ld, 0);
    b.push(ops, OP_RUNGEMM, tag).g = g;
    return dst;
  };

  struct DirRt { const ParamInfo *Wih, *Whh, *bih, *bhh; Ptr gates, c, h, hd, gh, hzero; RunGemm gx; Builder::Coef cgx; std::function<void(int, int32_t*)> bgx, bhhf; };
  struct LayerRt { DirRt d[2]; int icols; Ptr gx, hall, call, gsav; RunGemm gxg; Builder::Coef cgx; std::function<void(int, int32_t*)> bgx; };
  std::vector<LayerRt> layers(NL);
  const int64_t slab = (int64_t)T * rows * H;            // elements of one direction's [T][rows][H] array

  // =================================================================================================== forward
  Ptr x_in = to_act(Fw, io_x, IP, "x_act", 90);
  std::vector<Src> cur = {Src{x_in, IP, 0, IP}};
  for (int l = 0; l < NL; ++l) {
    LayerRt& L = layers[l];
    const int tag = 100 + l;
    const std::string nm = "l" + std::to_string(l);
    L.icols = l == 0 ? I : D * H;
    const int icols = L.icols;
    for (int d = 0; d < D; ++d) {
      L.d[d].Wih = &b.par(pp + "weight_ih" + sfx(l, d)); L.d[d].Whh = &b.par(pp + "weight_hh" + sfx(l, d));
      L.d[d].bih = &b.par(pp + "bias_ih" + sfx(l, d)); L.d[d].bhh = &b.par(pp + "bias_hh" + sfx(l, d));
    }
    // column j of source run s = input feature s * H + j (layer 0: one run, the features beyond I are pad columns without a weight)
    auto in_feat = [=](int s, int j) -> int { return l == 0 ? (j < I ? j : -1) : s * H + j; };
    L.hall = b.ws(nm + ".h", D * slab, adt);
    if (!gru) L.call = b.ws(nm + ".c", D * slab, DT_F32);
    for (int d = 0; d < D; ++d) { L.d[d].h = at(L.hall, d * slab, adt); if (!gru) L.d[d].c = at(L.call, d * slab, DT_F32); }
    if (!gru) {
      // unit-major gate columns (sefd_desc.h gate_col), direction d in columns [d * 4H, (d + 1) * 4H) of the shared slab
      const ParamInfo *W0 = L.d[0].Wih, *W1 = L.d[D - 1].Wih, *bi0 = L.d[0].bih, *bi1 = L.d[D - 1].bih, *bh0 = L.d[0].bhh, *bh1 = L.d[D - 1].bhh;
      L.gx = b.ws(nm + ".gx", (int64_t)T * rows * GW, DT_F32);
      RunGemm g = seq_gemm(cur, adt, GW, DT_F32);
      L.cgx = [=](int nn, int s, int j) -> int32_t {
        const int f = in_feat(s, j);
        return f < 0 ? 0 : pe(nn < 4 * H ? *W0 : *W1, (int64_t)gate_torch_row(nn % (4 * H), H) * icols + f, 1);
      };
      L.bgx = [=](int nn, int32_t* o) { const int q = gate_torch_row(nn % (4 * H), H); o[0] = pe(nn < 4 * H ? *bi0 : *bi1, q, 1); o[1] = pe(nn < 4 * H ? *bh0 : *bh1, q, 1); };
      b.pack_weights(Fw, g, L.cgx, nm + ".ih", tag, &L.bgx);
      set_y(g, L.gx, GW, 0);
      b.push(Fw, OP_RUNGEMM, tag).g = g;
      L.gxg = g;
      if (cluster) {
        // one direction: the pre-activations are overwritten in place by i, f, g, o (as FullSubNet's G = 1 layers); two: the saved gates are a
        // group-major buffer of their own - a group's rows are not contiguous in the interleaved 8H slab
        L.gsav = D == 1 ? L.gx : b.ws(nm + ".gates", D * slab * 4, DT_F32);
        LstmRec r;
        std::memset(&r, 0, sizeof(r));
        r.gx = L.gx; r.gates = L.gsav;
        r.whh[0] = b.mk(A_PARAM, L.d[0].Whh->off * 4); r.whh[1] = b.mk(A_PARAM, L.d[D - 1].Whh->off * 4);
        r.h = L.hall; r.c = L.call; r.dh = r.dgates = b.none();
        r.gx_goff[0] = 0; r.gx_goff[1] = D == 2 ? 4 * H : 0;
        r.gx_ld = GW; r.G = D; r.nset = D; r.B = (int)rows; r.T = T; r.H = H; r.hdt = adt; r.gdt = DT_F32; r.tmajor = 1;
        r.rev_mask = D == 2 ? 2 : 0;                         // never chunked: t0 = t1 = 0
        b.push(Fw, OP_LSTM_FWD, tag).lstm = r;
      } else {
        for (int d = 0; d < D; ++d) {
          DirRt& Q = L.d[d];
          const std::string dn = nm + (d ? ".r" : ".f");
          const ParamInfo* Whh = Q.Whh;
          // recurrent weights, packed once per direction; step k of the direction is frame t, its previous frame tp (none at k == 0)
          RunGemm rec0 = step_gemm(Q.h, adt, H, 4 * H, at(L.gx, d * 4 * H, DT_F32), GW, DT_F32, kRunAccum);
          Builder::Coef chh = [=](int nn, int s, int j) -> int32_t { return pe(*Whh, (int64_t)gate_torch_row(nn, H) * H + j, 1); };
          b.pack_weights(Fw, rec0, chh, dn + ".hh", tag);
          for (int k = 0; k < T; ++k) {
            const int t = d ? T - 1 - k : k, tp = d ? t + 1 : t - 1;
            const Ptr gt = at(L.gx, (int64_t)t * rows * GW + d * 4 * H, DT_F32);
            if (k > 0) {
              RunGemm r = rec0;
              r.x[0] = at(Q.h, (int64_t)tp * rows * H, adt);
              r.y = gt;
              b.push(Fw, OP_RUNGEMM, tag).g = r;
            }
            LstmCell& cl = b.push(Fw, OP_CELL_FWD, tag).cell;
            std::memset(&cl, 0, sizeof(cl));
            cl.gates = gt;
            cl.h = at(Q.h, (int64_t)t * rows * H, adt);
            cl.c = at(Q.c, (int64_t)t * rows * H, DT_F32);
            cl.c_prev = k > 0 ? at(Q.c, (int64_t)tp * rows * H, DT_F32) : b.none();
            cl.dh = cl.dc = cl.dgates = cl.gh = b.none();
            cl.rows = rows; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = k == 0; cl.kind = 0;
            strided(cl);
          }
        }
      }
    } else {
      for (int d = 0; d < D; ++d) {
        DirRt& Q = L.d[d];
        const std::string dn = nm + (d ? ".r" : ".f");
        const ParamInfo *Wih = Q.Wih, *Whh = Q.Whh, *bih = Q.bih, *bhh = Q.bhh;
        Q.gates = b.ws(dn + ".gates", (int64_t)T * rows * 4 * H, DT_F32);
        RunGemm g = seq_gemm(cur, adt, 3 * H, DT_F32);
        Q.cgx = [=](int nn, int s, int j) -> int32_t { const int f = in_feat(s, j); return f < 0 ? 0 : pe(*Wih, (int64_t)nn * icols + f, 1); };
        Q.bgx = [=](int nn, int32_t* o) { o[0] = pe(*bih, nn, 1); o[1] = 0; };     // b_hh rides the recurrent GEMM: n = tanh(.. + r * (W_hn h + b_hn))
        b.pack_weights(Fw, g, Q.cgx, dn + ".ih", tag, &Q.bgx);
        set_y(g, Q.gates, 4 * H, 0);
        b.push(Fw, OP_RUNGEMM, tag).g = g;
        Q.gx = g;
        // per frame: gh = h_prev . W_hh^T + b_hh into one reused [rows][3H] buffer (the first step reads a zero slab), then the GRU cell
        Q.gh = b.ws(dn + ".gh", rows * 3 * H, DT_F32);
        Q.hzero = b.ws(dn + ".h0", rows * H, adt);
        { Op& m = b.push(Fw, OP_MEMSET, tag); m.ms.dst = Q.hzero; m.ms.bytes = rows * H * esize(adt); }
        RunGemm rec0 = step_gemm(Q.hzero, adt, H, 3 * H, Q.gh, 3 * H, DT_F32, 0);
        Builder::Coef chh = [=](int nn, int s, int j) -> int32_t { return pe(*Whh, (int64_t)nn * H + j, 1); };
        Q.bhhf = [=](int nn, int32_t* o) { o[0] = pe(*bhh, nn, 1); o[1] = 0; };
        b.pack_weights(Fw, rec0, chh, dn + ".hh", tag, &Q.bhhf);
        for (int k = 0; k < T; ++k) {
          const int t = d ? T - 1 - k : k, tp = d ? t + 1 : t - 1;
          const Ptr hprev = k > 0 ? at(Q.h, (int64_t)tp * rows * H, adt) : b.none();
          RunGemm r = rec0;
          if (k > 0) r.x[0] = hprev;
          b.push(Fw, OP_RUNGEMM, tag).g = r;
          LstmCell& cl = b.push(Fw, OP_CELL_FWD, tag).cell;
          std::memset(&cl, 0, sizeof(cl));
          cl.gates = at(Q.gates, (int64_t)t * rows * 4 * H, DT_F32);
          cl.h = at(Q.h, (int64_t)t * rows * H, adt);
          cl.dh = cl.dc = cl.dgates = cl.c = b.none();
          cl.rows = rows; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = k == 0;
          cl.kind = 1; cl.gh = Q.gh; cl.c_prev = hprev;
        }
      }
    }
    // inverted dropout on both directions' outputs of every layer but the last (nn.LSTM(dropout=...)); the mask id is distinct per (layer, direction)
    cur.clear();
    const bool drop = l < NL - 1 && keep < 1.f;
    Ptr hdall = drop ? b.ws(nm + ".hd", D * slab, adt) : L.hall;
    for (int d = 0; d < D; ++d) {
      L.d[d].hd = at(hdall, d * slab, adt);
      if (drop) {
        Op& op = b.push(Fw, OP_DROPOUT_FWD, tag);
        op.drop.x = L.d[d].h; op.drop.y = L.d[d].hd; op.drop.seed = io_seed; op.drop.n = slab; op.drop.keep = keep; op.drop.dt = adt; op.drop.layer = 2 * l + d;
      }
      cur.push_back(Src{L.d[d].hd, H, 0, H});
    }
  }
  // head (fc_output_layer): reads [h_fwd | h_rev] of the last layer, writes the pre-activation output
  const ParamInfo &Wf = b.par("fc_output_layer.weight"), &bf = b.par("fc_output_layer.bias");
  RunGemm fcg = seq_gemm(cur, adt, O, DT_F32);
  Builder::Coef cfc = [=, &Wf](int nn, int s, int j) -> int32_t { return pe(Wf, (int64_t)nn * D * H + s * H + j, 1); };
  std::function<void(int, int32_t*)> bfc = [=, &bf](int nn, int32_t* o) { o[0] = pe(bf, nn, 1); o[1] = 0; };
  b.pack_weights(Fw, fcg, cfc, "fc", 200, &bfc);
  set_y(fcg, io_y, O, 0);
  b.push(Fw, OP_RUNGEMM, 200).g = fcg;

  // =================================================================================================== backward
  if (cfg.training) {
    Ptr dy = to_act(R, io_gy, O, "dy_act", 200);
    { RunGemm fw = fcg; fw.ydt = adt; fw.flags = 0; b.wgrad(R, fw, dy, cfc, 200, &bfc); }
    Ptr dhall = b.ws("dh.top", D * slab, DT_F32);          // gradient of the layer's h, [D][T][rows][H] fp32; the recurrences accumulate onto it
    for (int d = 0; d < D; ++d) {
      RunGemm g = seq_gemm({Src{dy, O, 0, O}}, adt, H, DT_F32);
      Builder::Coef coef = [=, &Wf](int nn, int s, int j) -> int32_t { return pe(Wf, (int64_t)j * D * H + d * H + nn, 1); };
      b.pack_weights(R, g, coef, std::string("fc.dg") + (d ? ".r" : ".f"), 200);
      set_y(g, at(dhall, d * slab, DT_F32), H, 0);
      b.push(R, OP_RUNGEMM, 200).g = g;
    }
    for (int l = NL - 1; l >= 0; --l) {
      LayerRt& L = layers[l];
      const int tag = 100 + l;
      const std::string nm = "l" + std::to_string(l);
      std::vector<Src> dgsrc;                              // the gate gradients as GEMM sources (input gradient)
      Builder::Coef cdx;                                   // W_ih element of (input feature f, gate-gradient run s, column j), via cdx(f, s, j)
      if (!gru) {
        Ptr dgates = b.ws(nm + ".dgates", (int64_t)T * rows * GW, adt);
        if (cluster) {
          LstmRec r;
          std::memset(&r, 0, sizeof(r));
          r.gx = L.gx; r.gates = L.gsav; r.h = L.hall; r.c = L.call; r.dh = dhall; r.dgates = dgates;
          r.whh[0] = b.mk(A_PARAM, L.d[0].Whh->off * 4); r.whh[1] = b.mk(A_PARAM, L.d[D - 1].Whh->off * 4);
          r.gx_goff[0] = 0; r.gx_goff[1] = D == 2 ? 4 * H : 0;
          r.gx_ld = GW; r.G = D; r.nset = D; r.B = (int)rows; r.T = T; r.H = H; r.hdt = adt; r.gdt = adt; r.tmajor = 1;
          r.rev_mask = D == 2 ? 2 : 0;
          b.push(R, OP_LSTM_BWD, tag).lstm = r;
        } else {
          for (int d = 0; d < D; ++d) {
            DirRt& Q = L.d[d];
            const std::string dn = nm + (d ? ".r" : ".f");
            const ParamInfo* Whh = Q.Whh;
            const Ptr dh = at(dhall, d * slab, DT_F32);
            Ptr dc = b.ws(dn + ".dc", rows * H, DT_F32);
            // dh_prev += dgates_t . W_hh : packed transposed recurrent weights; the run is the direction's 4H columns of a D * 4H wide row
            RunGemm rb0 = step_gemm(at(dgates, d * 4 * H, adt), adt, GW, H, dh, H, DT_F32, kRunAccum);
            rb0.seg[0].len = 4 * H;
            Builder::layout_segs(rb0);
            Builder::Coef cT = [=](int nn, int s, int j) -> int32_t { return pe(*Whh, (int64_t)gate_torch_row(j, H) * H + nn, 1); };
            b.pack_weights(R, rb0, cT, dn + ".hhT", tag);
            for (int k = T - 1; k >= 0; --k) {             // this direction's steps, last to first
              const int t = d ? T - 1 - k : k, tp = d ? t + 1 : t - 1;
              const Ptr dgt = at(dgates, (int64_t)t * rows * GW + d * 4 * H, adt);
              LstmCell& cl = b.push(R, OP_CELL_BWD, tag).cell;
              std::memset(&cl, 0, sizeof(cl));
              cl.gates = at(L.gx, (int64_t)t * rows * GW + d * 4 * H, DT_F32);
              cl.h = cl.gh = b.none();
              cl.dh = at(dh, (int64_t)t * rows * H, DT_F32);
              cl.dgates = dgt;
              cl.c = at(Q.c, (int64_t)t * rows * H, DT_F32);
              cl.c_prev = k > 0 ? at(Q.c, (int64_t)tp * rows * H, DT_F32) : b.none();
              cl.dc = dc;
              cl.rows = rows; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = k == T - 1; cl.kind = 0;
              strided(cl);
              if (k > 0) {
                RunGemm r = rb0;
                r.x[0] = dgt;
                r.y = at(dh, (int64_t)tp * rows * H, DT_F32);
                b.push(R, OP_RUNGEMM, tag).g = r;
              }
            }
          }
        }
        // W_ih and both biases of both directions: ONE weight-gradient GEMM over the shared gate-gradient slab
        RunGemm fw = L.gxg;
        fw.ydt = adt; fw.flags = 0;
        set_y(fw, dgates, GW, 0);
        b.wgrad(R, fw, dgates, L.cgx, tag, &L.bgx);
        for (int d = 0; d < D; ++d) {
          const ParamInfo* Whh = L.d[d].Whh;
          RunGemm fh = seq_gemm({Src{L.d[d].h, H, 0, H}}, adt, 4 * H, adt);
          fh.seg[0].dt = d ? 1 : -1;                       // the direction's previous frame
          set_y(fh, dgates, GW, d * 4 * H);
          Builder::Coef chh = [=](int nn, int s, int j) -> int32_t { return pe(*Whh, (int64_t)gate_torch_row(nn, H) * H + j, 1); };
          b.wgrad(R, fh, dgates, chh, tag, nullptr);
        }
        dgsrc = {Src{dgates, GW, 0, GW}};
        const Builder::Coef cg = L.cgx;
        cdx = [=](int f, int s, int j) -> int32_t { return cg(j, f / H, f % H); };      // (run, column) of input feature f: layer 0 has one run
        if (l == 0) cdx = [=](int f, int s, int j) -> int32_t { return cg(j, 0, f); };
      } else {
        for (int d = 0; d < D; ++d) {
          DirRt& Q = L.d[d];
          const std::string dn = nm + (d ? ".r" : ".f");
          const ParamInfo* Whh = Q.Whh;
          const Ptr dh = at(dhall, d * slab, DT_F32);
          Ptr dgates = b.ws(dn + ".dgates", (int64_t)T * rows * 3 * H, adt);
          Ptr dgh = b.ws(dn + ".dgh", (int64_t)T * rows * 3 * H, adt);      // gradient of the recurrent pre-activations
          // dh_prev += dgh_t . W_hh : packed transposed recurrent weights
          RunGemm rb0 = step_gemm(dgh, adt, 3 * H, H, dh, H, DT_F32, kRunAccum);
          Builder::Coef cT = [=](int nn, int s, int j) -> int32_t { return pe(*Whh, (int64_t)j * H + nn, 1); };
          b.pack_weights(R, rb0, cT, dn + ".hhT", tag);
          for (int k = T - 1; k >= 0; --k) {               // this direction's steps, last to first
            const int t = d ? T - 1 - k : k, tp = d ? t + 1 : t - 1;
            LstmCell& cl = b.push(R, OP_CELL_BWD, tag).cell;
            std::memset(&cl, 0, sizeof(cl));
            cl.gates = at(Q.gates, (int64_t)t * rows * 4 * H, DT_F32);
            cl.h = cl.c = b.none();
            cl.dh = at(dh, (int64_t)t * rows * H, DT_F32);
            cl.dgates = at(dgates, (int64_t)t * rows * 3 * H, adt);
            cl.rows = rows; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = k == T - 1; cl.kind = 1;
            cl.c_prev = k > 0 ? at(Q.h, (int64_t)tp * rows * H, adt) : b.none();
            cl.dc = k > 0 ? at(dh, (int64_t)tp * rows * H, DT_F32) : b.none();
            cl.gh = at(dgh, (int64_t)t * rows * 3 * H, adt);
            if (k > 0) {
              RunGemm r = rb0;
              r.x[0] = at(dgh, (int64_t)t * rows * 3 * H, adt);
              r.y = at(dh, (int64_t)tp * rows * H, DT_F32);
              b.push(R, OP_RUNGEMM, tag).g = r;
            }
          }
          RunGemm fw = Q.gx;
          fw.ydt = adt; fw.flags = 0;
          set_y(fw, dgates, 3 * H, 0);                    // the gradient slab is 3H wide (the forward slab keeps a 4th block for W_hn h + b_hn)
          b.wgrad(R, fw, dgates, Q.cgx, tag, &Q.bgx);
          RunGemm fh = seq_gemm({Src{Q.h, H, 0, H}}, adt, 3 * H, adt);
          fh.seg[0].dt = d ? 1 : -1;                       // the direction's previous frame
          set_y(fh, dgh, 3 * H, 0);
          Builder::Coef chh = [=](int nn, int s, int j) -> int32_t { return pe(*Whh, (int64_t)nn * H + j, 1); };
          b.wgrad(R, fh, dgh, chh, tag, &Q.bhhf);         // b_hh belongs to this GEMM (bias "ones" run)
          dgsrc.push_back(Src{dgates, 3 * H, 0, 3 * H});
        }
        const Builder::Coef c0 = L.d[0].cgx, c1 = L.d[D - 1].cgx;
        cdx = [=](int f, int s, int j) -> int32_t { return (s == 0 ? c0 : c1)(j, f / H, f % H); };
        if (l == 0) cdx = [=](int f, int s, int j) -> int32_t { return (s == 0 ? c0 : c1)(j, 0, f); };
      }
      // input gradient: the layer below's [D][T][rows][H] (through its dropout), or the plan's grad_x; both directions' gate gradients in ONE GEMM
      if (l == 0) {
        RunGemm g = seq_gemm(dgsrc, adt, IP, DT_F32);
        const Builder::Coef cf = cdx;
        Builder::Coef coef = [=](int nn, int s, int j) -> int32_t { return cf(nn, s, j); };
        b.pack_weights(R, g, coef, nm + ".dx", tag);
        set_y(g, io_gx, IP, 0);
        b.push(R, OP_RUNGEMM, tag).g = g;
      } else {
        const bool drop = keep < 1.f;
        Ptr dlow = b.ws("dh." + std::to_string(l - 1), D * slab, DT_F32);
        Ptr dlowd = drop ? b.ws("dhd." + std::to_string(l - 1), D * slab, DT_F32) : dlow;
        for (int e = 0; e < D; ++e) {
          RunGemm g = seq_gemm(dgsrc, adt, H, DT_F32);
          const Builder::Coef cf = cdx;
          Builder::Coef coef = [=](int nn, int s, int j) -> int32_t { return cf(e * H + nn, s, j); };
          b.pack_weights(R, g, coef, nm + ".dx" + (e ? ".r" : ".f"), tag);
          set_y(g, at(dlowd, e * slab, DT_F32), H, 0);
          b.push(R, OP_RUNGEMM, tag).g = g;
          if (drop) {                                      // the same mask as the forward's, re-derived from the seed
            Op& op = b.push(R, OP_DROPOUT_BWD, tag - 1);
            op.drop.x = at(dlowd, e * slab, DT_F32); op.drop.y = at(dlow, e * slab, DT_F32); op.drop.seed = io_seed; op.drop.n = slab; op.drop.keep = keep;
            op.drop.dt = DT_F32; op.drop.layer = 2 * (l - 1) + e;
          }
        }
        dhall = dlow;
      }
    }
    b.finish_unpack(R);
  }
  finish_plan(b, P, nparam, 0);
  return P;
}

}  // namespace sefd
