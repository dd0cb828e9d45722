#include "plan_builder.h"

namespace sefd {

// FullSubNet (reference models.py:568-682; SequenceModel tools_for_model.py:726-795).  model == 3.
// Config fields reused: kernel_num = {sb_num_neighbors, fb_num_neighbors, look_ahead, fb_hidden, sb_hidden,
//                                     fb activation (0 none, 1 ReLU, 2 Tanh, 3 ReLU6), sb activation, dropout keep in 1/1000};
// T = frames of the input magnitude (passed in cfg.L as T, cfg.fft_len/2+1 = F).  I/O: io.mag [B][F][T] -> io.crm [B][F][T][2];
// backward: io.grad_crm -> A_GRAD.
// Every LSTM layer = one hoisted input GEMM over all T' steps + per step {recurrent GEMM accumulating onto the gate
// slab, cell kernel}; with B*257 = 8224 rows (B = 32) each step GEMM is a full-chip 8224 x 1536 x 384 problem.
Plan* build_fsn_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  Builder b;
  b.P = P;
  b.c = cfg;
  const int B = cfg.B, T = cfg.L, F = cfg.fft_len / 2 + 1;
  const int nsb = cfg.kernel_num[0], nfb = cfg.kernel_num[1], LA = cfg.kernel_num[2];
  const int Hf = cfg.kernel_num[3], Hs = cfg.kernel_num[4], actf = cfg.kernel_num[5], acts = cfg.kernel_num[6];
  const float keep = cfg.training ? cfg.kernel_num[7] / 1000.f : 1.f;
  const bool gru = cfg.kernel_num[8] == 1;        // cfg.sequence_model: nn.GRU instead of nn.LSTM (tools_for_model.py:739-756)
  const int nmode = cfg.kernel_num[9];            // cfg.norm_type (sefd_desc.h struct Fsn): 0 offline_laplace ... 3 cumulative_layer_norm
  if (nmode < 0 || nmode > 3) { P->error = "FullSubNet: unknown norm_type"; return P; }
  const int NG = gru ? 3 : 4;                     // gate blocks of the recurrent weights
  const int adt = cfg.act_dtype;
  // sub-band rows: NB magnitude neighbours + NFB full-band neighbours = W features, stored WP = roundup(W, 8) wide (sefd_desc.h struct Fsn)
  const int TP = T + LA, NB = 2 * nsb + 1, NFB = 2 * nfb + 1, W = NB + NFB, WP = (int)rup(W, 8);
  const int FP = (int)rup(F, 8);
  P->T = T;
  P->NF = F;
  if (nsb < 0 || nfb < 0 || nsb > kFsnMaxNeighbors || nfb > kFsnMaxNeighbors || F <= kFsnMaxNeighbors || (int64_t)F * NFB * 4 > 65536) {
    P->error = "FullSubNet: sb_num_neighbors and fb_num_neighbors must lie in 0 .. " + std::to_string(kFsnMaxNeighbors) + " (and below num_freqs; num_freqs * (2 fb_num_neighbors + 1) <= 16384)";
    return P;
  }
  if (actf < 0 || actf > 3 || acts < 0 || acts > 3) { P->error = "FullSubNet: unknown output activation"; return P; }
  if (Hf % 8 || Hs % 8) { P->error = "FullSubNet: hidden sizes must be multiples of 8"; return P; }
  struct Net { std::string name; int I, H, O; };
  Net nets[2] = {{"fb_model", F, Hf, F}, {"sb_model", W, Hs, 2}};
  for (auto& nt : nets) {
    for (int l = 0; l < 2; ++l) {
      const std::string p = nt.name + ".sequence_model.";
      b.add_param(p + "weight_ih_l" + std::to_string(l), {NG * nt.H, l == 0 ? nt.I : nt.H}, true);
      b.add_param(p + "weight_hh_l" + std::to_string(l), {NG * nt.H, nt.H}, true);
      b.add_param(p + "bias_ih_l" + std::to_string(l), {NG * nt.H}, true);
      b.add_param(p + "bias_hh_l" + std::to_string(l), {NG * nt.H}, true);
    }
    b.add_param(nt.name + ".fc_output_layer.weight", {nt.O, nt.H}, true);
    b.add_param(nt.name + ".fc_output_layer.bias", {nt.O}, true);
  }
  const int64_t nparam = P->params.back().off + P->params.back().numel;
  b.inv.resize(nparam);
  Ptr io_mag = b.io("mag", (int64_t)B * F * T);
  Ptr io_crm = b.io("crm", (int64_t)B * F * T * 2);
  Ptr io_gcrm = b.io("grad_crm", (int64_t)B * F * T * 2);
  Ptr io_seed = b.io("seed", 2);
  std::vector<Op>& Fw = P->fwd;
  std::vector<Op>& R = P->bwd;

  auto fsn0 = [&]() { Fsn f; std::memset(&f, 0, sizeof(f)); f.in = f.out = f.aux = f.aux2 = f.sums = f.stat = b.none();
                      f.B = B; f.F = F; f.T = T; f.TP = TP; f.FP = FP; f.NB = NB; f.LA = LA; f.dt = adt; f.act = actf; f.ext = fsn_ext(nfb, acts); return f; };
  // time-major GEMM over all steps: rows (t, r), source [TP][rows][feat]
  auto seq_gemm = [&](Ptr x, int xdt, int64_t rows, int feat, int off, int len, int N, int ydt) {
    RunGemm g = Builder::gemm0();
    g.x[0] = x; g.xdt = xdt; g.ydt = ydt;
    g.bstride[0] = 0; g.tstride[0] = (int)(rows * feat); g.base[0] = 0; g.rowlen[0] = (int)(rows * feat); g.fstride[0] = feat; g.Tin[0] = TP;
    g.M = (int)(TP * rows); g.Tout = TP; g.Fo = (int)rows;
    g.nseg = 1; g.seg[0] = Seg{0, 0, off, len, 0};
    g.N = N;
    Builder::layout_segs(g);
    return g;
  };
  auto set_y = [&](RunGemm& g, Ptr y, int64_t rows, int ld, int yoff) {
    g.y = y; g.y_bstride = 0; g.y_tstride = (int)(rows * ld); g.y_fstride = ld; g.y_off = yoff;
  };
  // one time step: rows (r), source slab [rows][feat] at step t
  auto step_gemm = [&](Ptr x, int xdt, int64_t rows, int feat, int t, int N, Ptr y, int ld, int64_t yslab_elems, int ydt, int flags) {
    RunGemm g = Builder::gemm0();
    g.x[0] = b.mk(A_WS, x.off + (int64_t)t * rows * feat * esize(xdt)); g.xdt = xdt; g.ydt = ydt;
    g.tstride[0] = 0; g.rowlen[0] = (int)(rows * feat); g.fstride[0] = feat; g.Tin[0] = 1;
    g.M = (int)rows; g.Tout = 1; g.Fo = (int)rows;
    g.nseg = 1; g.seg[0] = Seg{0, 0, 0, feat, 0};
    g.N = N;
    Builder::layout_segs(g);
    g.y = b.mk(A_WS, y.off + yslab_elems * esize(ydt)); g.y_fstride = ld; g.flags = flags;
    return g;
  };

  // ---- input: transpose, laplace norm (models.py:640-645)
  Ptr mag_t = b.ws("mag_t", (int64_t)TP * B * F, DT_F32);
  Ptr sum_fb = b.ws("sum_fb", (int64_t)B * F, DT_F32);
  Ptr mu_fb = b.ws("mu_fb", B, DT_F32);
  Ptr fb_in = b.ws("fb_in", (int64_t)TP * B * FP, adt);
  { Fsn f = fsn0(); f.in = io_mag; f.out = mag_t; f.sums = sum_fb; f.aux2 = mu_fb; b.push(Fw, OP_FSN_IN, 1).fsn = f; }
  Ptr st_fb = b.none(), st_sb = b.none();
  if (nmode == 2) { st_fb = b.ws("stat_fb", 2 * B, DT_F32); st_sb = b.ws("stat_sb", 2 * B, DT_F32); }
  else if (nmode) { st_fb = b.ws("stat_fb", (int64_t)TP * B * 2, DT_F32); st_sb = b.ws("stat_sb", (int64_t)TP * B * F * 2, DT_F32); }
  if (nmode) { Fsn f = fsn0(); f.in = mag_t; f.stat = st_fb; f.mode = nmode; f.src = 0; b.push(Fw, OP_FSN_NORMSTAT, 2).fsn = f; }
  { Fsn f = fsn0(); f.in = mag_t; f.out = fb_in; f.sums = mu_fb; f.mode = nmode; f.stat = st_fb; b.push(Fw, OP_FSN_SCALE, 2).fsn = f; }

  struct LayerRt { RunGemm gx; Builder::Coef cgx; std::function<void(int, int32_t*)> bgx; Ptr gates, c, h, hd, x; int xfeat, xlen, H; int64_t rows;
                   const ParamInfo* Whh; RunGemm rec; std::string nm; int lid; bool cluster, rowsk, xfuse, dropfused = false, dropbwd = false, headfuse = false; Ptr dyo, wo; int sdt, xf; int dhdt = DT_F32; Ptr hd_fused; Ptr gh, hzero; std::function<void(int, int32_t*)> bhh; };
  std::vector<LayerRt> layers;
  auto lstm_forward = [&](const std::string& netname, int l, int lid, Ptr x, int xfeat, int xlen, int64_t rows, int H, int tag) -> Ptr {
    LayerRt L;
    L.nm = netname + ".l" + std::to_string(l); L.lid = lid; L.x = x; L.xfeat = xfeat; L.xlen = xlen; L.rows = rows; L.H = H;
    const std::string pp = netname + ".sequence_model.";
    const ParamInfo &Wih = b.par(pp + "weight_ih_l" + std::to_string(l)), &Whh = b.par(pp + "weight_hh_l" + std::to_string(l));
    const ParamInfo &bih = b.par(pp + "bias_ih_l" + std::to_string(l)), &bhh = b.par(pp + "bias_hh_l" + std::to_string(l));
    L.Whh = &Whh;
    const int I = (int)Wih.shape[1];
    // thousands of rows (the sub-band model) in bf16: row-block kernels (lstm_rows.hip) on a packed bf16 copy of W_hh; their gate
    // slabs are bf16 too - at B * 257 rows those layers are bound by the HBM traffic of exactly these slabs (LSTM_SLAB32=1: fp32)
    const int64_t rows_min = tune_int("LSTM_ROWS_MIN", 1024);
    L.cluster = !gru && adt == DT_BF16 && H > 128 && H <= 512 && H % 64 == 0 && !tune_has("LSTM_STEPPED");
    L.rowsk = L.cluster && rows >= rows_min && (H == 256 || H == 384 || H == 512);
    L.sdt = (L.rowsk && !tune_has("LSTM_SLAB32")) ? DT_BF16 : DT_F32;
    L.gates = b.ws(L.nm + ".gates", (int64_t)TP * rows * 4 * H, L.sdt);
    L.c = b.ws(L.nm + ".c", (int64_t)TP * rows * H, DT_F32);
    L.h = b.ws(L.nm + ".h", (int64_t)TP * rows * H, adt);
    // bf16 mode, 128 < H <= 512: the whole recurrence is ONE launch of the cluster kernels (lstm_cluster.hip) on the time-major
    // slabs, gate columns unit-major (sefd_desc.h gate_col); otherwise one GEMM + one cell launch per frame, gate-major columns
    const bool um = L.cluster;
    RunGemm g = seq_gemm(x, adt, rows, xfeat, 0, xlen, NG * H, L.sdt);
    L.cgx = [=](int nn, int s, int j) -> int32_t { return j < I ? pe(Wih, (int64_t)(um ? gate_torch_row(nn, H) : nn) * I + j, 1) : 0; };
    if (gru) L.bgx = [=](int nn, int32_t* o) { o[0] = pe(bih, nn, 1); o[1] = 0; };     // b_hh rides the recurrent GEMM: n = tanh(.. + r * (W_hn h + b_hn))
    else L.bgx = [=](int nn, int32_t* o) { const int q = um ? gate_torch_row(nn, H) : nn; o[0] = pe(bih, q, 1); o[1] = pe(bhh, q, 1); };
    b.pack_weights(Fw, g, L.cgx, L.nm + ".ih", tag, &L.bgx);
    set_y(g, L.gates, rows, 4 * H, 0);
    // row-block kernels, 32 input features (the sub-band model's first layer): the input projection is fused into the recurrence (one more
    // k-step per frame) instead of writing and re-reading a [T x rows x 4H] pre-activation slab (8 GB at B = 64); LSTM_XFUSE=0 keeps the GEMM
    // ... and the layers above it (input = the layer below's h, H features): H/32 more k-steps per frame instead of an 8 GB slab + a GEMM
    const bool x32 = xlen == 32 && xfeat == 32 && g.ldw == 64, xh = xlen == H && xfeat == H && g.ldw == H;
    L.xfuse = L.rowsk && (x32 || xh) && g.Npad == 4 * H && tune_on("LSTM_XFUSE");
    if (L.xfuse) {
      // the packed W_ih re-ordered to MFMA B-fragment order ([4H][64] with K = 32 zero padded: in its first 4H x 32 slots)
      int32_t* tab = nullptr;
      for (auto it = Fw.rbegin(); it != Fw.rend(); ++it)
        if (it->kind == OP_PACK && it->pack.dst.arena == g.w.arena && it->pack.dst.off == g.w.off) { tab = reinterpret_cast<int32_t*>(P->consts.data() + it->pack.tab.off); break; }
      if (!tab) { P->error = "FullSubNet: packed W_ih not found"; return b.none(); }
      const int ldw = g.ldw, kf = x32 ? 32 : H;
      std::vector<int32_t> old(tab, tab + (size_t)4 * H * ldw);
      std::fill(tab, tab + (size_t)4 * H * ldw, 0);
      for (int c = 0; c < 4 * H; ++c)
        for (int k = 0; k < kf; ++k) tab[rows_wf_index(kf, c, k)] = old[(size_t)c * ldw + k];
      L.xf = kf;
    } else {
      b.push(Fw, OP_RUNGEMM, tag).g = g;
    }
    L.gx = g;
    if (L.cluster) {
      LstmRec r;
      std::memset(&r, 0, sizeof(r));
      r.gx = L.gates; r.gates = L.gates;                   // pre-activations are overwritten in place by i, f, g, o
      r.whh[0] = r.whh[1] = b.pptr(pp + "weight_hh_l" + std::to_string(l));
      r.h = L.h; r.c = L.c; r.dh = r.dgates = b.none();
      r.gx_ld = 4 * H; r.G = 1; r.nset = 1; r.B = (int)rows; r.T = TP; r.H = H; r.hdt = adt; r.gdt = DT_F32; r.tmajor = 1;
      // thousands of rows (the sub-band model): row-block kernels (lstm_rows.hip) on a packed bf16 copy of W_hh, rows = gate columns
      L.rec = Builder::gemm0();
      if (L.rowsk) {
        RunGemm pk = step_gemm(L.h, adt, rows, H, 0, 4 * H, L.gates, 4 * H, 0, DT_F32, 0);
        Builder::Coef chh = [=](int nn, int s, int j) -> int32_t { return pe(Whh, (int64_t)gate_torch_row(nn, H) * H + j, 1); };
        b.pack_weights(Fw, pk, chh, L.nm + ".hhpk", tag);
        if (pk.ldw != H || pk.Npad != 4 * H) { P->error = "FullSubNet: packed W_hh layout"; return b.none(); }
        {   // re-order the gather table into MFMA B-fragment order: one wave-load of the kernel = 1 KB contiguous (lstm_rows.hip)
          int32_t* tab = reinterpret_cast<int32_t*>(P->consts.data() + Fw.back().pack.tab.off);
          std::vector<int32_t> old(tab, tab + (size_t)4 * H * H);
          for (int c = 0; c < 4 * H; ++c)
            for (int k = 0; k < H; ++k) tab[rows_wf_index(H, c, k)] = old[(size_t)c * H + k];
        }
        r.impl = 1; r.wpk_f = pk.w; r.wpk_b = b.none(); r.gxdt = L.sdt;
        r.xin = r.wpk_x = r.bias = b.none();
        if (L.xfuse) { r.xin = x; r.wpk_x = g.w; r.bias = g.bias; r.xfeat = L.xf; }
        r.hd = r.seed = b.none();
        if (l == 0 && keep < 1.f && tune_on("LSTM_DROPFUSE")) {   // dropout applied while h_t is stored
          L.hd_fused = b.ws(L.nm + ".hd", (int64_t)TP * rows * H, adt);
          r.hd = L.hd_fused; r.seed = io_seed; r.keep = keep; r.drop_layer = lid;
          L.dropfused = true;
        }
      }
      b.push(Fw, OP_LSTM_FWD, tag).lstm = r;
    } else if (gru) {
      // per frame: gh = h_{t-1} . W_hh^T + b_hh into one reused [rows][3H] buffer (t = 0 reads a zero slab), then the GRU cell
      L.gh = b.ws(L.nm + ".gh", rows * 3 * H, DT_F32);
      L.hzero = b.ws(L.nm + ".h0", rows * H, adt);
      { Op& m = b.push(Fw, OP_MEMSET, tag); m.ms.dst = L.hzero; m.ms.bytes = rows * H * esize(adt); }
      RunGemm rec0 = step_gemm(L.hzero, adt, rows, H, 0, 3 * H, L.gh, 3 * H, 0, DT_F32, 0);
      Builder::Coef chh = [=](int nn, int s, int j) -> int32_t { return pe(Whh, (int64_t)nn * H + j, 1); };
      L.bhh = [=](int nn, int32_t* o) { o[0] = pe(bhh, nn, 1); o[1] = 0; };
      b.pack_weights(Fw, rec0, chh, L.nm + ".hh", tag, &L.bhh);
      L.rec = rec0;
      for (int t = 0; t < TP; ++t) {
        RunGemm r = rec0;
        if (t > 0) r.x[0] = b.mk(A_WS, L.h.off + (int64_t)(t - 1) * rows * H * esize(adt));
        b.push(Fw, OP_RUNGEMM, tag).g = r;
        LstmCell& cl = b.push(Fw, OP_CELL_FWD, tag).cell;
        std::memset(&cl, 0, sizeof(cl));
        cl.gates = b.mk(A_WS, L.gates.off + (int64_t)t * rows * 4 * H * 4);
        cl.gh = L.gh;
        cl.c = b.none();
        cl.c_prev = t > 0 ? b.mk(A_WS, L.h.off + (int64_t)(t - 1) * rows * H * esize(adt)) : b.none();
        cl.h = b.mk(A_WS, L.h.off + (int64_t)t * rows * H * esize(adt));
        cl.dh = cl.dc = cl.dgates = b.none();
        cl.rows = rows; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = t == 0; cl.kind = 1;
      }
    } else {
    // recurrent weights, packed once per step list
    RunGemm rec0 = step_gemm(L.h, adt, rows, H, 0, 4 * H, L.gates, 4 * H, 0, DT_F32, kRunAccum);
    Builder::Coef chh = [=](int nn, int s, int j) -> int32_t { return pe(Whh, (int64_t)nn * H + j, 1); };
    b.pack_weights(Fw, rec0, chh, L.nm + ".hh", tag);
    L.rec = rec0;
    for (int t = 0; t < TP; ++t) {
      if (t > 0) {
        RunGemm r = step_gemm(L.h, adt, rows, H, t - 1, 4 * H, L.gates, 4 * H, (int64_t)t * rows * 4 * H, DT_F32, kRunAccum);
        r.w = rec0.w;
        b.push(Fw, OP_RUNGEMM, tag).g = r;
      }
      Op& op = b.push(Fw, OP_CELL_FWD, tag);
      LstmCell& cl = op.cell;
      cl.kind = 0; cl.gh = b.none();
      cl.gates = b.mk(A_WS, L.gates.off + (int64_t)t * rows * 4 * H * 4);
      cl.c = b.mk(A_WS, L.c.off + (int64_t)t * rows * H * 4);
      cl.c_prev = t > 0 ? b.mk(A_WS, L.c.off + (int64_t)(t - 1) * rows * H * 4) : b.none();
      cl.h = b.mk(A_WS, L.h.off + (int64_t)t * rows * H * esize(adt));
      cl.dh = cl.dc = cl.dgates = b.none();
      cl.rows = rows; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = t == 0;
    }
    }
    L.hd = L.h;
    if (l == 0) {               // inter-layer dropout (nn.LSTM(dropout=0.8)): only after the first of the two layers
      L.hd = L.dropfused ? L.hd_fused : keep < 1.f ? b.ws(L.nm + ".hd", (int64_t)TP * rows * H, adt) : L.h;
      if (keep < 1.f && !L.dropfused) {
        Op& op = b.push(Fw, OP_DROPOUT_FWD, tag);
        op.drop.x = L.h; op.drop.y = L.hd; op.drop.seed = io_seed; op.drop.n = (int64_t)TP * rows * H; op.drop.keep = keep; op.drop.dt = adt; op.drop.layer = lid;
      }
    }
    layers.push_back(L);
    return L.hd;
  };
  struct FcRt { RunGemm g; Builder::Coef coef; std::function<void(int, int32_t*)> bias; };
  auto fc_forward = [&](const std::string& netname, Ptr x, int64_t rows, int H, int O, Ptr y, int ld, int flags, int tag) -> FcRt {
    const ParamInfo &Wf = b.par(netname + ".fc_output_layer.weight"), &bf = b.par(netname + ".fc_output_layer.bias");
    FcRt fc;
    fc.g = seq_gemm(x, adt, rows, H, 0, H, O, DT_F32);
    fc.coef = [=](int nn, int s, int j) -> int32_t { return pe(Wf, (int64_t)nn * H + j, 1); };
    fc.bias = [=](int nn, int32_t* o) { o[0] = pe(bf, nn, 1); o[1] = 0; };
    b.pack_weights(Fw, fc.g, fc.coef, netname + ".fc", tag, &fc.bias);
    set_y(fc.g, y, rows, ld, 0);
    fc.g.flags = flags;
    b.push(Fw, OP_RUNGEMM, tag).g = fc.g;
    return fc;
  };

  // ---- full-band model
  Ptr h0 = lstm_forward("fb_model", 0, 0, fb_in, FP, FP, B, Hf, 100);
  Ptr h1 = lstm_forward("fb_model", 1, 1, h0, Hf, Hf, B, Hf, 101);
  Ptr fbo = b.ws("fbo", (int64_t)TP * B * FP, DT_F32);
  { Op& m = b.push(Fw, OP_MEMSET, 102); m.ms.dst = fbo; m.ms.bytes = (int64_t)TP * B * FP * 4; }   // pad columns F..FP-1 stay 0
  FcRt fcf = fc_forward("fb_model", h1, B, Hf, F, fbo, FP, actf == 1 ? kRunRelu : 0, 102);
  if (actf > 1) { Fsn f = fsn0(); f.out = fbo; b.push(Fw, OP_FSN_ACT, 102).fsn = f; }     // Tanh / ReLU6 in place (ReLU: the GEMM's epilogue)

  // ---- sub-band input (models.py:647-665)
  const int64_t rs = (int64_t)B * F;
  Ptr sum_sb = b.ws("sum_sb", (int64_t)B * F, DT_F32);
  Ptr mu_sb = b.ws("mu_sb", B, DT_F32);
  Ptr sb_in = b.ws("sb_in", (int64_t)TP * rs * WP, adt);
  if (nmode == 0) { Fsn f = fsn0(); f.in = mag_t; f.aux = fbo; f.sums = sum_sb; f.aux2 = mu_sb; b.push(Fw, OP_FSN_SBSUM, 200).fsn = f; }
  else { Fsn f = fsn0(); f.in = mag_t; f.aux = fbo; f.stat = st_sb; f.mode = nmode; f.src = 1; b.push(Fw, OP_FSN_NORMSTAT, 200).fsn = f; }
  { Fsn f = fsn0(); f.in = mag_t; f.aux = fbo; f.sums = mu_sb; f.out = sb_in; f.mode = nmode; f.stat = st_sb; b.push(Fw, OP_FSN_SBBUILD, 201).fsn = f; }
  Ptr h2 = lstm_forward("sb_model", 0, 2, sb_in, WP, WP, rs, Hs, 202);     // W_ih packed with zero rows for the pad features (as FP pads F above)
  Ptr h3 = lstm_forward("sb_model", 1, 3, h2, Hs, Hs, rs, Hs, 203);
  Ptr sbo = b.ws("sbo", (int64_t)TP * rs * 2, DT_F32);
  FcRt fcs = fc_forward("sb_model", h3, rs, Hs, 2, sbo, 2, 0, 204);
  { Fsn f = fsn0(); f.in = sbo; f.out = io_crm; b.push(Fw, OP_FSN_OUT, 205).fsn = f; }

  // =================================================================================================== backward
  if (cfg.training) {
    // lane of the weight-gradient GEMMs: 1 = second stream (api.hip: issued behind the first recurrence kernel of the phase, joined in front of
    // the UNPACK); only when the recurrences are single launches (the per-frame GRU / fp32 formulation has no OP_LSTM_BWD to fork at)
    int wg_lane = (!gru && adt == DT_BF16 && tune_on("FSN_LANES")) ? 1 : 0;
    // data parallel (cfg.grad_buckets >= 2): the sub-band model's weight gradients keep the second lane busy for ~12 ms after the main stream
    // is through (profiles/r03_tuning_notes.md section 8) - the full-band model's gradients (the FRONT of the flat arena, 2/3 of it) are
    // therefore produced ON the main stream, folded and unpacked there without waiting for the lane, and their all-reduce (started by the
    // caller at that op: sefd_plan_grad_bucket_range) runs under the sub-band weight gradients; the sub-band range follows at the end
    const bool fsn_buckets = cfg.grad_buckets >= 2 && wg_lane == 1;
    // wg_hold: the weight gradients of the layer wait for the NEXT recurrence launch instead of starting beside the input-gradient GEMM in
    // between (two MFMA-bound GEMMs side by side ran 10 % slower than one after the other; beside the HBM-bound recurrence they fill its idle CUs)
    int wg_hold = 0;
    auto lstm_backward = [&](LayerRt& L, Ptr dh, bool need_dx, Ptr dx, int dx_ld, int dx_off, int dx_N, int dx_dt, int tag) {
      const int H = L.H;
      const int64_t rows = L.rows;
      Ptr dgates = b.ws(L.nm + ".dgates", (int64_t)TP * rows * NG * H, adt);
      const ParamInfo* Whh = L.Whh;
      const bool um = L.cluster;
      Ptr dgh = dgates;                                   // gradient of the recurrent pre-activations: the same slab for the LSTM
      if (gru) {
        dgh = b.ws(L.nm + ".dgh", (int64_t)TP * rows * 3 * H, adt);
        RunGemm rb0 = step_gemm(dgh, adt, rows, 3 * H, 0, H, dh, H, 0, DT_F32, kRunAccum);
        Builder::Coef cT = [=](int nn, int s, int j) -> int32_t { return pe(*Whh, (int64_t)j * H + nn, 1); };
        b.pack_weights(R, rb0, cT, L.nm + ".hhT", tag);
        for (int t = TP - 1; t >= 0; --t) {
          LstmCell& cl = b.push(R, OP_CELL_BWD, tag).cell;
          std::memset(&cl, 0, sizeof(cl));
          cl.gates = b.mk(A_WS, L.gates.off + (int64_t)t * rows * 4 * H * 4);
          cl.c = cl.h = b.none();
          cl.c_prev = t > 0 ? b.mk(A_WS, L.h.off + (int64_t)(t - 1) * rows * H * esize(adt)) : b.none();
          cl.dh = b.mk(A_WS, dh.off + (int64_t)t * rows * H * 4);
          cl.dc = t > 0 ? b.mk(A_WS, dh.off + (int64_t)(t - 1) * rows * H * 4) : b.none();
          cl.dgates = b.mk(A_WS, dgates.off + (int64_t)t * rows * 3 * H * esize(adt));
          cl.gh = b.mk(A_WS, dgh.off + (int64_t)t * rows * 3 * H * esize(adt));
          cl.rows = rows; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = t == TP - 1; cl.kind = 1;
          if (t > 0) {
            RunGemm r = step_gemm(dgh, adt, rows, 3 * H, t, H, dh, H, (int64_t)(t - 1) * rows * H, DT_F32, kRunAccum);
            r.w = rb0.w;
            b.push(R, OP_RUNGEMM, tag).g = r;
          }
        }
      } else if (L.cluster) {
        LstmRec r;
        std::memset(&r, 0, sizeof(r));
        r.gx = L.gates; r.gates = L.gates; r.h = L.h; r.c = L.c; r.dh = dh; r.dgates = dgates;
        r.whh[0] = r.whh[1] = b.mk(A_PARAM, Whh->off * 4);
        r.gx_ld = 4 * H; r.G = 1; r.nset = 1; r.B = (int)rows; r.T = TP; r.H = H; r.hdt = adt; r.gdt = adt; r.tmajor = 1;
        if (L.rowsk) {                                      // W_hh^T packed: row = hidden unit, column = gate column (unit-major)
          RunGemm pk = step_gemm(dgates, adt, rows, 4 * H, 0, H, dh, H, 0, DT_F32, 0);
          Builder::Coef cT = [=](int nn, int s, int j) -> int32_t { return pe(*Whh, (int64_t)gate_torch_row(j, H) * H + nn, 1); };
          b.pack_weights(R, pk, cT, L.nm + ".hhTpk", tag);
          if (pk.ldw != 4 * H || pk.Npad != H) { P->error = "FullSubNet: packed W_hh^T layout"; return; }
          {
            int32_t* tab = reinterpret_cast<int32_t*>(P->consts.data() + R.back().pack.tab.off);
            std::vector<int32_t> old(tab, tab + (size_t)4 * H * H);
            for (int n = 0; n < H; ++n)
              for (int k = 0; k < 4 * H; ++k) tab[rows_wb_index(H, n, k)] = old[(size_t)n * 4 * H + k];
          }
          r.impl = 1; r.wpk_b = pk.w; r.wpk_f = b.none(); r.gxdt = L.sdt;
          r.xin = r.wpk_x = r.bias = r.hd = r.seed = b.none();
          if (L.dropbwd) { r.seed = io_seed; r.keep = keep; r.drop_layer = L.lid; }
          r.dhdt = L.dhdt;
          r.dyo = r.wo = b.none();
          if (L.headfuse) { r.dyo = L.dyo; r.wo = L.wo; r.no = 2; }
        }
        b.push(R, OP_LSTM_BWD, tag).lstm = r;
      } else {
      Ptr dc = b.ws(L.nm + ".dc", rows * H, DT_F32);
      // dh_{t-1} += dgates_t . W_hh : packed transposed recurrent weights
      RunGemm rb0 = step_gemm(dgates, adt, rows, 4 * H, 0, H, dh, H, 0, DT_F32, kRunAccum);
      Builder::Coef cT = [=](int nn, int s, int j) -> int32_t { return pe(*Whh, (int64_t)j * H + nn, 1); };
      b.pack_weights(R, rb0, cT, L.nm + ".hhT", tag);
      for (int t = TP - 1; t >= 0; --t) {
        Op& op = b.push(R, OP_CELL_BWD, tag);
        LstmCell& cl = op.cell;
        cl.gates = b.mk(A_WS, L.gates.off + (int64_t)t * rows * 4 * H * 4);
        cl.c = b.mk(A_WS, L.c.off + (int64_t)t * rows * H * 4);
        cl.c_prev = t > 0 ? b.mk(A_WS, L.c.off + (int64_t)(t - 1) * rows * H * 4) : b.none();
        cl.h = b.none();
        cl.dh = b.mk(A_WS, dh.off + (int64_t)t * rows * H * 4);
        cl.dc = dc;
        cl.dgates = b.mk(A_WS, dgates.off + (int64_t)t * rows * 4 * H * esize(adt));
        cl.rows = rows; cl.H = H; cl.hdt = adt; cl.gdt = adt; cl.first = t == TP - 1;
        if (t > 0) {
          RunGemm r = step_gemm(dgates, adt, rows, 4 * H, t, H, dh, H, (int64_t)(t - 1) * rows * H, DT_F32, kRunAccum);
          r.w = rb0.w;
          b.push(R, OP_RUNGEMM, tag).g = r;
        }
      }
      }
      // weight gradients over all steps: nothing needs them before UNPACK - on the weight-gradient lane (second stream) they run beside the
      // input-gradient GEMM and the NEXT layer's recurrence (343 workgroups of 48 sequences on 256 CUs: its second round leaves 2/3 of the chip idle)
      b.cur_lane = wg_lane;
      b.cur_hold = wg_hold;
      b.wg_rounds = wg_lane ? 8 : 1;   // 3 -> 8 with the job-scheduled recurrences (r05 notes): 57.1 -> 56.6 ms
      RunGemm fw = L.gx;
      fw.ydt = adt;
      if (gru) set_y(fw, dgates, rows, NG * H, 0);        // the GRU's gradient slab is 3H wide (the forward slab keeps a 4th block for W_hn h + b_hn)
      Builder::Coef chh = [=](int nn, int s, int j) -> int32_t { return pe(*Whh, (int64_t)(um ? gate_torch_row(nn, H) : nn) * H + j, 1); };
      // A narrow input (the sub-band model's first layer: 32 features) next to H = 384 recurrent columns: [x_t | h_{t-1} | ones] is 64 + 384 + 64 =
      // 512 columns = exactly the two 256-wide k tiles the W_hh gradient alone occupies (its second tile half empty) - ONE weight-gradient GEMM
      // over dgates instead of two (the 1536 x 128 launch for W_ih and the bias, 1.6 ms at B = 64, and its pass over the 9.6 GB gate gradients are gone)
      const int xw = fw.nseg == 1 ? (int)rup(fw.seg[0].len, 64) : 0;
      const bool cat = !gru && L.rowsk && fw.nseg == 1 && fw.seg[0].src == 0 && xw == 64 && H % 64 == 0 && rup(xw + H + 64, 256) == rup(H, 256) &&
                       tune_on("FSN_WGCAT");
      // The upper layer: [h1_t | h2_{t-1}] = 2 H = 768 columns = three whole 256-wide k tiles in ONE GEMM over dgates (W_ih and W_hh apart: 384 (+ 64 ones)
      // and 384 columns = 2 + 2 tiles, a quarter of them padding, and two passes over the gate gradients); the bias comes from the ones MFMA of k tile 0
      const bool cat2 = !cat && !gru && L.rowsk && fw.nseg == 1 && fw.seg[0].src == 0 && fw.seg[0].len == H && fw.seg[0].dt == 0 && (2 * H) % 256 == 0 &&
                        tune_on("FSN_WGCAT2") && tune_on("ONES_MFMA");
      if (cat || cat2) {
        RunGemm fc = fw;
        fc.x[1] = L.h; fc.bstride[1] = 0; fc.tstride[1] = (int)(rows * H); fc.base[1] = 0; fc.rowlen[1] = (int)(rows * H); fc.fstride[1] = H; fc.Tin[1] = TP;
        fc.seg[fc.nseg++] = Seg{1, -1, 0, H, 0};           // h_{t-1}
        const Builder::Coef cgx = L.cgx;
        Builder::Coef cc = [=](int nn, int s, int j) -> int32_t { return s == 0 ? cgx(nn, 0, j) : chh(nn, 0, j); };
        b.wgrad(R, fc, dgates, cc, tag, &L.bgx);
      } else {
      b.wgrad(R, fw, dgates, L.cgx, tag, &L.bgx);
      RunGemm fh = seq_gemm(L.h, adt, rows, H, 0, H, NG * H, adt);
      fh.seg[0].dt = -1;                                   // h_{t-1}
      set_y(fh, dgh, rows, NG * H, 0);
      b.wgrad(R, fh, dgh, chh, tag, gru ? &L.bhh : nullptr);           // GRU: b_hh belongs to this GEMM (bias "ones" run)
      }
      b.cur_lane = 0;
      b.cur_hold = 0;
      b.wg_rounds = 1;
      if (need_dx) {
        RunGemm g = seq_gemm(dgates, adt, rows, NG * H, 0, NG * H, dx_N, dx_dt);
        const Builder::Coef cf = L.cgx;
        Builder::Coef coef = [=](int nn, int s, int j) -> int32_t { return cf(j, 0, nn); };
        b.pack_weights(R, g, coef, L.nm + ".dx", tag);
        set_y(g, dx, rows, dx_ld, dx_off);
        b.push(R, OP_RUNGEMM, tag).g = g;
      }
    };
    auto fc_backward = [&](FcRt& fc, Ptr dy, Ptr x, int64_t rows, int H, int O, int ld, Ptr dh, int tag, const std::string& nm, bool head_fused = false) {
      RunGemm fw = fc.g;
      fw.ydt = adt; fw.flags = 0;
      // the sub-band head's weight gradient (a 1.2 ms pass over h of the upper layer in front of the first recurrence): on the weight-gradient
      // lane it is held back and runs in the CUs the recurrence's second dispatch round leaves idle
      if (head_fused) b.cur_lane = wg_lane;
      b.wgrad(R, fw, dy, fc.coef, tag, &fc.bias);
      b.cur_lane = 0;
      if (head_fused) return;                             // the row-block LSTM backward forms dh = dy . W_fc itself (O = 2: a rank-2 update)
      RunGemm g = seq_gemm(dy, adt, rows, ld, 0, O, H, DT_F32);
      const Builder::Coef cf = fc.coef;
      Builder::Coef coef = [=](int nn, int s, int j) -> int32_t { return cf(j, 0, nn); };
      b.pack_weights(R, g, coef, nm + ".fc.dg", tag);
      set_y(g, dh, rows, H, 0);
      b.push(R, OP_RUNGEMM, tag).g = g;
    };
    auto dropout_bwd = [&](LayerRt& L, Ptr dxd, int tag) -> Ptr {      // gradient wrt the un-dropped h (fp32, in place semantics via a copy)
      if (!(keep < 1.f)) return dxd;
      if (L.dropfused) { L.dropbwd = true; return dxd; }               // the row-block backward kernel multiplies dh by the mask as it loads it
      Ptr dhu = b.ws(L.nm + ".dhu", (int64_t)TP * L.rows * L.H, DT_F32);
      Op& op = b.push(R, OP_DROPOUT_BWD, tag);
      op.drop.x = dxd; op.drop.y = dhu; op.drop.seed = io_seed; op.drop.n = (int64_t)TP * L.rows * L.H; op.drop.keep = keep; op.drop.dt = DT_F32; op.drop.layer = L.lid;
      return dhu;
    };
    LayerRt &Lf0 = layers[0], &Lf1 = layers[1], &Ls0 = layers[2], &Ls1 = layers[3];
    // sub-band head
    Ptr d_sbo = b.ws("d_sbo", (int64_t)TP * rs * 2, adt);
    { Fsn f = fsn0(); f.in = io_gcrm; f.out = d_sbo; if (acts) f.aux = sbo; b.push(R, OP_FSN_OUT_BWD, 205).fsn = f; }
    // sub-band head: 2 outputs.  With the row-block kernels the [T x rows x H] fp32 gradient of h (4 GB written by a K = 2 GEMM, read back
    // by the recurrence) is never materialised: the kernel computes dh = d_sbo[.., 0] W_fc[0] + d_sbo[.., 1] W_fc[1] as it needs it
    Ls1.headfuse = Ls1.rowsk && tune_on("LSTM_HEADFUSE");
    Ptr dh3 = Ls1.headfuse ? b.none() : b.ws("dh3", (int64_t)TP * rs * Hs, DT_F32);       // (not even allocated then: 4.6 GB at B = 64)
    if (Ls1.headfuse) { Ls1.dyo = d_sbo; Ls1.wo = b.pptr("sb_model.fc_output_layer.weight"); }
    fc_backward(fcs, d_sbo, h3, rs, Hs, 2, 2, dh3, 204, "sb_model", Ls1.headfuse);
    // the gradient slab between the two sub-band layers ([T x rows x H]: 4.8 GB in fp32 at B = 64, written by the input-gradient GEMM and read once by
    // the row-block backward of the layer below): bf16 like every other activation gradient of the bf16 plans when nothing but that kernel
    // reads it (the inter-layer dropout fused into it, or no dropout); FSN_DH16=0: fp32
    const bool dh16 = adt == DT_BF16 && Ls1.rowsk && Ls0.rowsk && (Ls0.dropfused || !(keep < 1.f)) && tune_on("FSN_DH16");
    Ptr dh2d = b.ws("dh2d", (int64_t)TP * rs * Hs, dh16 ? adt : DT_F32);
    // round 6: with the upper layer's ONE weight-gradient GEMM (cat2, 3 k tiles) starting beside the input-gradient GEMM is 0.12 ms per step better than
    // waiting for the lower layer's recurrence (54.15 vs 54.28 ms, twice, one box); FSN_HOLD=1 restores the hold
    wg_hold = tune_is("FSN_HOLD", 1);
    lstm_backward(Ls1, dh3, true, dh2d, Hs, 0, Hs, dh16 ? adt : DT_F32, 203);
    wg_hold = 0;
    if (dh16) Ls0.dhdt = adt;
    Ptr dh2 = dropout_bwd(Ls0, dh2d, 202);
    Ptr d_sbin = b.ws("d_sbin", (int64_t)TP * rs * WP, DT_F32);
    lstm_backward(Ls0, dh2, true, d_sbin, WP, 0, WP, DT_F32, 202);
    // through the normalised concat into the full-band output
    Ptr sumS = b.ws("sum_S", (int64_t)B * F, DT_F32);
    Ptr Sm = b.ws("Sm", B, DT_F32);
    Ptr d_fb = b.ws("d_fb", (int64_t)TP * B * FP, adt);
    if (nmode == 0) {
      { Fsn f = fsn0(); f.in = d_sbin; f.aux = sb_in; f.sums = sumS; f.aux2 = Sm; b.push(R, OP_FSN_SBBWD_SUM, 201).fsn = f; }
      { Fsn f = fsn0(); f.in = d_sbin; f.aux = fbo; f.aux2 = mu_sb; f.sums = Sm; f.out = d_fb; b.push(R, OP_FSN_SBBWD_APPLY, 200).fsn = f; }
    } else {
      Ptr dpre = b.ws("d_fb_pre", (int64_t)TP * B * F * NFB, DT_F32);    // one value per full-band column; FSN_SBBWD_APPLY gathers them per bin
      Ptr part = b.ws("normbwd_part", (int64_t)2 * B * F, DT_F32);
      { Fsn f = fsn0(); f.in = d_sbin; f.aux = fbo; f.aux2 = sb_in; f.stat = st_sb; f.sums = part; f.out = dpre; f.mode = nmode; f.src = 1;
        b.push(R, OP_FSN_NORMBWD, 201).fsn = f; }
      { Fsn f = fsn0(); f.in = dpre; f.aux = fbo; f.aux2 = mu_sb; f.sums = Sm; f.out = d_fb; f.mode = nmode; b.push(R, OP_FSN_SBBWD_APPLY, 200).fsn = f; }
    }
    if (fsn_buckets) b.flush_sums(R, 997, true);         // the sub-band folds: on the lane, behind the weight gradients they fold
    // full-band weight gradients (four 80 us launches): main stream.  Two gradient buckets need them there (no wait for the lane); since round 6 always: at
    // the end of the lane they ran 0.35 ms past the main stream, which idles beside the 8-workgroup cluster recurrences (profiles/r06_tuning_notes.md)
    wg_lane = 0;
    Ptr dh1 = b.ws("dh1", (int64_t)TP * B * Hf, DT_F32);
    fc_backward(fcf, d_fb, h1, B, Hf, F, FP, dh1, 102, "fb_model");
    Ptr dh0d = b.ws("dh0d", (int64_t)TP * B * Hf, DT_F32);
    lstm_backward(Lf1, dh1, true, dh0d, Hf, 0, Hf, DT_F32, 101);
    Ptr dh0 = dropout_bwd(Lf0, dh0d, 100);
    lstm_backward(Lf0, dh0, false, b.none(), 0, 0, 0, DT_F32, 100);
    if (fsn_buckets) {
      const int64_t sb_lo = b.par("sb_model.sequence_model.weight_ih_l0").off;
      b.unpack_range(R, 0, sb_lo, 998, true);             // folds + UNPACK of the full-band range: no wait for the lane
      b.unpack_lo = sb_lo;
      P->bucket_elem = 0; P->bucket_end = sb_lo;
    }
    b.finish_unpack(R);
  }
  finish_plan(b, P, nparam, 0);
  for (size_t k = 0; k < P->bwd.size(); ++k)
    if (P->bwd[k].kind == OP_UNPACK && P->bwd[k].tag == 998) P->bucket_op = (int32_t)k;
  return P;
}

}  // namespace sefd
