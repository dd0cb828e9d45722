#include "plan_builder.h"

namespace sefd {

// The conv layers and ComplexBatchNorm of the reference's tools_for_model.py on their own (models 9 and 10): ComplexConv2d / ComplexConvTranspose2d /
// RealConv2d / RealConvTranspose2d (tools_for_model.py:199-425) and ComplexBatchNorm (:430-607) as one-layer plans between two layout ops
// (OP_NCHW_CL, layout.hip) that take the reference's [B, C, F, T] tensors into the channels-last buffers every plan works in, and back.
//
// Model 9, cfg.B = batch, cfg.L = input frames T, kernel_num = {kind (0 ComplexConv2d, 1 ComplexConvTranspose2d, 2 RealConv2d, 3 RealConvTranspose2d),
// C_in, C_out, KH, KW, frequency stride, padding F, padding T, causal, output padding F, input bins F}.  io.x [B][C_in][F][T] -> io.y [B][C_out][Fo][To];
// backward io.grad_y -> io.grad_x and A_GRAD.  Channel counts are padded to multiples of 8 inside the plan (Cip, Cop) with zero coefficients.
//
// Strided conv (kinds 0, 2): output (fo, u) reads input bin fo s + kh - pf and frame u + kw - pt: ONE RUNGEMM with a run per time tap kw (dt = kw - pt)
// of KH * Cip elements at offset -pf * Cip, fstride = s * Cip; frames and bins outside the input read as zero by the descriptor's validity rule - the
// causal / symmetric time padding only decides To.  Its input gradient is the sub-pixel form: input bins fi = s g + q take the taps
// kh = r0 + s m (r0 = (q + pf) mod s) from output bins g + e0 - m (e0 = (q + pf - r0) / s): per phase q a run of nt = ceil((KH - r0) / s) output bins.
// Transposed conv (kinds 1, 3): output bin o = s f - pf + kh, frame u = t - pt + kw.  Phase p = (o + pf) mod s, o + pf = s g + p, takes the taps
// kh = p + s m from the input bins g - m: a run of nt = ceil((KH - p) / s) bins ending at g; rows g in [ceil((pf - p) / s), floor((Fo - 1 + pf - p) / s)]
// (output padding extends the range of the phase that owns the last bins).  Its input gradient is the strided conv over the cotangent.
// A phase without a tap (KH <= p) keeps one run of zero coefficients: its outputs are the bias / zero.
// Weight and bias gradients: Builder::wgrad over the forward descriptors (ones run), SPLITSUM + UNPACK into A_GRAD.
namespace {

struct Geo { int kind, Ci, Co, KH, KW, s, pf, pt, causal, opf, F, T, B, Cip, Cop, Fo, To; bool cplx, transposed; };

int cdiv_floor(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
int cdiv_ceil(int a, int b) { return -cdiv_floor(-a, b); }

}  // namespace

Plan* build_convlayer_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  P->T = 0; P->NF = 0;
  Geo q{};
  const int32_t* kn = cfg.kernel_num;
  q.kind = kn[0]; q.Ci = kn[1]; q.Co = kn[2]; q.KH = kn[3]; q.KW = kn[4]; q.s = kn[5]; q.pf = kn[6]; q.pt = kn[7]; q.causal = kn[8]; q.opf = kn[9]; q.F = kn[10];
  q.T = cfg.L; q.B = cfg.B;
  if (q.kind < 0 || q.kind > 3) { P->error = "ConvLayer: kind must be 0 .. 3"; return P; }
  q.cplx = q.kind < 2; q.transposed = (q.kind & 1) != 0;
  const char* names[4] = {"ComplexConv2d", "ComplexConvTranspose2d", "RealConv2d", "RealConvTranspose2d"};
  const std::string nm = names[q.kind];
  if (q.s < 1 || q.s > 2) { P->error = nm + ": the frequency stride must be 1 or 2"; return P; }
  if (q.KH < 1 || q.KH > 7) { P->error = nm + ": the frequency extent of the kernel must lie in 1 .. 7"; return P; }
  if (q.KW < 1 || q.KW > 4) { P->error = nm + ": the time extent of the kernel must lie in 1 .. 4 (a descriptor holds 8 runs over two sources)"; return P; }
  if (q.pf < 0 || q.pf >= q.KH || q.pt < 0 || q.pt >= q.KW) { P->error = nm + ": padding must be smaller than the kernel extent"; return P; }
  if (q.opf < 0 || q.opf >= q.s || (!q.transposed && q.opf)) { P->error = nm + ": output padding must be smaller than the stride"; return P; }
  if (q.Ci < 1 || q.Co < 1 || (q.cplx && ((q.Ci | q.Co) & 1))) { P->error = nm + ": the complex layers need even channel counts"; return P; }
  if (q.B < 1 || q.F < 1 || q.T < 1 || q.F > 65535) { P->error = nm + ": batch, bins and frames must be at least 1 (bins at most 65535)"; return P; }
  if (!q.transposed) {
    q.Fo = q.F + 2 * q.pf - q.KH >= 0 ? (q.F + 2 * q.pf - q.KH) / q.s + 1 : 0;
    q.To = q.T + (q.causal && q.pt ? q.pt : 2 * q.pt) - q.KW + 1;
  } else {
    q.Fo = (q.F - 1) * q.s - 2 * q.pf + q.KH + q.opf;
    q.To = q.T + q.KW - 1 - 2 * q.pt;
  }
  if (q.Fo < 1 || q.To < 1) {
    P->error = nm + " plan: " + std::to_string(q.F) + " bins x " + std::to_string(q.T) + " frames under kernel (" + std::to_string(q.KH) + ", " + std::to_string(q.KW) +
               "), stride (" + std::to_string(q.s) + ", 1), padding (" + std::to_string(q.pf) + ", " + std::to_string(q.pt) + ") leave " + std::to_string(q.Fo) +
               " output bins x " + std::to_string(q.To) + " output frames";
    return P;
  }
  if ((int64_t)q.B * q.To * q.Fo >= (1LL << 31) || (int64_t)q.B * q.T * q.F >= (1LL << 31)) { P->error = nm + ": more than 2^31 rows"; return P; }
  q.Cip = (int)rup(q.Ci, 8); q.Cop = (int)rup(q.Co, 8);
  P->T = q.To; P->NF = q.Fo;

  Builder b;
  b.P = P;
  b.c = cfg;
  const int adt = cfg.act_dtype;
  const int Ci2 = q.cplx ? q.Ci / 2 : q.Ci, Co2 = q.cplx ? q.Co / 2 : q.Co;
  // nn.Conv2d weight [out][in][KH][KW]; nn.ConvTranspose2d weight [in][out][KH][KW]
  const std::vector<int64_t> wshape = q.transposed ? std::vector<int64_t>{Ci2, Co2, q.KH, q.KW} : std::vector<int64_t>{Co2, Ci2, q.KH, q.KW};
  if (q.cplx) {
    for (const char* part : {"real_conv", "imag_conv"}) {
      b.add_param(std::string(part) + ".weight", wshape, true);
      b.add_param(std::string(part) + ".bias", {Co2}, true);
    }
  } else {
    b.add_param("conv.weight", wshape, true);
    b.add_param("conv.bias", {Co2}, true);
  }
  const int64_t nparam = P->params.back().off + P->params.back().numel;
  b.inv.resize(nparam);
  const ParamInfo* Wr = &b.par(q.cplx ? "real_conv.weight" : "conv.weight");
  const ParamInfo* Wi = q.cplx ? &b.par("imag_conv.weight") : nullptr;
  const ParamInfo* br = &b.par(q.cplx ? "real_conv.bias" : "conv.bias");
  const ParamInfo* bi = q.cplx ? &b.par("imag_conv.bias") : nullptr;

  const int B = q.B, F = q.F, T = q.T, Fo = q.Fo, To = q.To, Cip = q.Cip, Cop = q.Cop, KH = q.KH, KW = q.KW, s = q.s, pf = q.pf, pt = q.pt;
  Ptr io_x = b.io("x", (int64_t)B * q.Ci * F * T);
  Ptr io_y = b.io("y", (int64_t)B * q.Co * Fo * To);
  Ptr io_gy = b.io("grad_y", (int64_t)B * q.Co * Fo * To);
  Ptr io_gx = b.io("grad_x", (int64_t)B * q.Ci * F * T);
  Ptr x = b.ws("x", (int64_t)B * T * F * Cip, adt);
  Ptr y = b.ws("y", (int64_t)B * To * Fo * Cop, adt);
  Ptr dy = b.ws("dy", (int64_t)B * To * Fo * Cop, adt);
  Ptr dx = b.ws("dx", (int64_t)B * T * F * Cip, adt);

  auto layout = [&](std::vector<Op>& ops, int mode, Ptr nchw, Ptr cl, int C, int Cp, int Fq, int Tq) {
    NchwCl& d = b.push(ops, OP_NCHW_CL, 1).lay;
    d.nchw = nchw; d.cl = cl; d.B = B; d.C = C; d.Cpad = Cp; d.F = Fq; d.T = Tq; d.Tcl = Tq; d.t_off = 0; d.dt = adt; d.mode = mode;
  };

  // W[co][ci][kh][kw] of the block matrix [[Wr, -Wi], [Wi, Wr]] (complex) or of the conv itself (real): (output channel n, input channel c) of the padded
  // channel axes -> signed parameter element, 0 for a pad channel
  auto wel = [=](int n, int c, int kh, int kw) -> int32_t {
    if (n >= q.Co || c >= q.Ci || kh < 0 || kh >= KH) return 0;
    auto idx = [&](int co, int ci) -> int64_t {
      return q.transposed ? (((int64_t)ci * Co2 + co) * KH + kh) * KW + kw : (((int64_t)co * Ci2 + ci) * KH + kh) * KW + kw;
    };
    if (!q.cplx) return pe(*Wr, idx(n, c));
    const bool no = n >= Co2, ni = c >= Ci2;                 // imaginary output / input
    const int co = no ? n - Co2 : n, ci = ni ? c - Ci2 : c;
    if (!no) return ni ? pe(*Wi, idx(co, ci), -1) : pe(*Wr, idx(co, ci));       // real = Wr xr - Wi xi
    return ni ? pe(*Wr, idx(co, ci)) : pe(*Wi, idx(co, ci));                    // imag = Wi xr + Wr xi
  };
  Builder::Bias bias = [=](int n, int32_t* o) {
    o[0] = o[1] = 0;
    if (n >= q.Co) return;
    if (!q.cplx) { o[0] = pe(*br, n); return; }
    if (n < Co2) { o[0] = pe(*br, n); o[1] = pe(*bi, n, -1); }                  // b_r - b_i
    else { o[0] = pe(*br, n - Co2); o[1] = pe(*bi, n - Co2); }                  // b_r + b_i
  };

  // activation [B][Tq][Fq][C] as the single source of a GEMM
  auto src = [&](RunGemm& g, Ptr p, int Tq, int Fq, int C, int fstride) {
    g.x[0] = p; g.xdt = adt; g.ydt = adt;
    g.bstride[0] = (int64_t)Tq * Fq * C; g.tstride[0] = Fq * C; g.base[0] = 0; g.rowlen[0] = Fq * C; g.fstride[0] = fstride; g.Tin[0] = Tq;
  };
  auto dst = [&](RunGemm& g, Ptr p, int Tq, int Fq, int C, int fstride, int off) {
    g.y = p; g.y_bstride = (int64_t)Tq * Fq * C; g.y_tstride = Fq * C; g.y_fstride = fstride; g.y_off = off;
  };

  std::vector<RunGemm> fw;                                  // forward descriptors (one, or one per phase) and their coefficient functions
  std::vector<Builder::Coef> fc;
  std::vector<Op>& Fw = P->fwd;
  std::vector<Op>& R = P->bwd;
  layout(Fw, 0, io_x, x, q.Ci, Cip, F, T);
  if (!q.transposed) {
    RunGemm g = Builder::gemm0();
    src(g, x, T, F, Cip, s * Cip);
    g.M = B * To * Fo; g.Tout = To; g.Fo = Fo;
    g.nseg = KW;
    for (int kw = 0; kw < KW; ++kw) g.seg[kw] = Seg{0, kw - pt, -pf * Cip, KH * Cip, 0};
    g.N = Cop;
    Builder::layout_segs(g);
    Builder::Coef coef = [=](int n, int sg, int j) -> int32_t { return wel(n, j % Cip, j / Cip, sg); };
    b.pack_weights(Fw, g, coef, "conv", 2, &bias);
    dst(g, y, To, Fo, Cop, Cop, 0);
    b.push(Fw, OP_RUNGEMM, 2).g = g;
    fw.push_back(g); fc.push_back(coef);
  } else {
    Ptr bias_buf = b.none();
    for (int p = 0; p < s; ++p) {
      const int g0 = std::max(0, cdiv_ceil(pf - p, s)), g1 = cdiv_floor(Fo - 1 + pf - p, s);
      if (g1 < g0) continue;
      const int nt = p < KH ? (KH - p + s - 1) / s : 1;
      RunGemm g = Builder::gemm0();
      src(g, x, T, F, Cip, Cip);
      g.M = B * To * (g1 - g0 + 1); g.Tout = To; g.Fo = g1 - g0 + 1;
      g.nseg = KW;
      for (int kw = 0; kw < KW; ++kw) g.seg[kw] = Seg{0, pt - kw, (g0 - (nt - 1)) * Cip, nt * Cip, 0};
      g.N = Cop;
      Builder::layout_segs(g);
      Builder::Coef coef = [=](int n, int sg, int j) -> int32_t { return wel(n, j % Cip, p + s * (nt - 1 - j / Cip), sg); };
      b.pack_weights(Fw, g, coef, "conv.p" + std::to_string(p), 2, bias_buf.arena < 0 ? &bias : nullptr);
      if (bias_buf.arena < 0) bias_buf = g.bias; else g.bias = bias_buf;
      dst(g, y, To, Fo, Cop, s * Cop, (s * g0 + p - pf) * Cop);
      b.push(Fw, OP_RUNGEMM, 2).g = g;
      fw.push_back(g); fc.push_back(coef);
    }
  }
  layout(Fw, 1, io_y, y, q.Co, Cop, Fo, To);

  // ------------------------------------------------------------------------------------------------ backward
  layout(R, 2, io_gy, dy, q.Co, Cop, Fo, To);
  for (size_t i = 0; i < fw.size(); ++i) b.wgrad(R, fw[i], dy, fc[i], 2, &bias);
  if (!q.transposed) {
    // dx[ci, s g + ph, t] = sum W[co, ci, r0 + s m, kw] dy[co, g + e0 - m, t - kw + pt]
    for (int ph = 0; ph < s; ++ph) {
      const int G = (F - ph + s - 1) / s;
      if (G < 1) continue;
      const int r0 = (ph + pf) % s, e0 = (ph + pf - r0) / s;
      const int nt = r0 < KH ? (KH - r0 + s - 1) / s : 1;
      RunGemm g = Builder::gemm0();
      src(g, dy, To, Fo, Cop, Cop);
      g.M = B * T * G; g.Tout = T; g.Fo = G;
      g.nseg = KW;
      for (int kw = 0; kw < KW; ++kw) g.seg[kw] = Seg{0, pt - kw, (e0 - (nt - 1)) * Cop, nt * Cop, 0};
      g.N = Cip;
      Builder::layout_segs(g);
      Builder::Coef coef = [=](int n, int sg, int j) -> int32_t { return wel(j % Cop, n, r0 + s * (nt - 1 - j / Cop), sg); };
      b.pack_weights(R, g, coef, "conv.dg" + std::to_string(ph), 2);
      dst(g, dx, T, F, Cip, s * Cip, ph * Cip);
      b.push(R, OP_RUNGEMM, 2).g = g;
    }
  } else {
    // dx[ci, f, t] = sum W[ci, co, kh, kw] dy[co, s f - pf + kh, t - pt + kw]: a strided conv over the cotangent
    RunGemm g = Builder::gemm0();
    src(g, dy, To, Fo, Cop, s * Cop);
    g.M = B * T * F; g.Tout = T; g.Fo = F;
    g.nseg = KW;
    for (int kw = 0; kw < KW; ++kw) g.seg[kw] = Seg{0, kw - pt, -pf * Cop, KH * Cop, 0};
    g.N = Cip;
    Builder::layout_segs(g);
    Builder::Coef coef = [=](int n, int sg, int j) -> int32_t { return wel(j % Cop, n, j / Cop, sg); };
    b.pack_weights(R, g, coef, "conv.dg", 2);
    dst(g, dx, T, F, Cip, Cip, 0);
    b.push(R, OP_RUNGEMM, 2).g = g;
  }
  layout(R, 3, io_gx, dx, q.Ci, Cip, F, T);
  b.finish_unpack(R);
  finish_plan(b, P, nparam, 0);
  return P;
}

// ComplexBatchNorm on its own (model 10): cfg.B = batch, cfg.L = S = the product of the trailing dimensions (the rows of one batch item),
// kernel_num = {num_features C (real + imaginary), eps and momentum as float32 bit patterns}.  io.x [B][C][S] -> io.y; backward io.grad_y -> io.grad_x and
// A_GRAD.  The existing kernels (cbn.hip) run over the rows [B * S][C] with a constant PReLU slope of 1 (no activation); its gradient goes to scratch.
// cfg.training = 0: running statistics, buffers untouched; the backward's statistics terms vanish through an infinite row count (they are divided by it).
Plan* build_cbn_plan(const ModelConfig& cfg) {
  Plan* P = new Plan();
  P->cfg = cfg;
  P->T = cfg.L; P->NF = 1;
  const int B = cfg.B, S = cfg.L, C = cfg.kernel_num[0];
  float eps, momentum;
  std::memcpy(&eps, &cfg.kernel_num[1], 4);
  std::memcpy(&momentum, &cfg.kernel_num[2], 4);
  if (C < 8 || C % 8) { P->error = "ComplexBatchNorm: num_features must be a multiple of 8 (the kernels move 4 complex channels per lane)"; return P; }
  if (C / 2 > 1024) { P->error = "ComplexBatchNorm: at most 1024 channel pairs (cbn.hip reduces a row of pairs in one workgroup)"; return P; }
  if (B < 1 || S < 1 || (int64_t)B * S >= (1LL << 31)) { P->error = "ComplexBatchNorm: batch and trailing dimensions must be at least 1 (at most 2^31 rows)"; return P; }
  Builder b;
  b.P = P;
  b.c = cfg;
  const int adt = cfg.act_dtype, h = C / 2;
  const int64_t Rr = (int64_t)B * S;
  for (const char* w : {"Wrr", "Wri", "Wii", "Br", "Bi"}) b.add_param(w, {h}, true);
  for (const char* w : {"RMr", "RMi", "RVrr", "RVri", "RVii"}) b.add_param(w, {h}, false);
  const int64_t nparam = 5 * (int64_t)h, nstate = 5 * (int64_t)h;
  Ptr io_x = b.io("x", Rr * C);
  Ptr io_y = b.io("y", Rr * C);
  Ptr io_gy = b.io("grad_y", Rr * C);
  Ptr io_gx = b.io("grad_x", Rr * C);
  Ptr y = b.ws("y", Rr * C, adt), z = b.ws("z", Rr * C, adt), dz = b.ws("dz", Rr * C, adt), dy = b.ws("dy", Rr * C, adt);
  const float one = 1.f;
  Ptr slope = b.cst(&one, 4);
  Ptr dslope = b.ws("dslope", 1, DT_F32);
  auto layout = [&](std::vector<Op>& ops, int mode, Ptr nchw, Ptr cl) {
    NchwCl& d = b.push(ops, OP_NCHW_CL, 1).lay;
    d.nchw = nchw; d.cl = cl; d.B = B; d.C = C; d.Cpad = C; d.F = 1; d.T = S; d.Tcl = S; d.t_off = 0; d.dt = adt; d.mode = mode;
  };
  const int64_t rpbk = std::max<int64_t>(64, (Rr + 2047) / 2048);
  const int nblk = (int)((Rr + rpbk - 1) / rpbk);
  const char* wn[3] = {"Wrr", "Wri", "Wii"};
  const char* rvn[3] = {"RVrr", "RVri", "RVii"};
  CbnFwd c;
  std::memset(&c, 0, sizeof(c));
  c.y = y; c.z = z; c.R = Rr; c.C = C; c.dt = adt; c.nblk = nblk; c.rows_per_blk = (int)rpbk;
  c.training = cfg.training; c.count = (double)Rr; c.eps = eps; c.momentum = momentum;
  c.part = cfg.training ? b.ws("cstat", (int64_t)nblk * 5 * h, DT_F32) : b.none();
  c.coef = b.ws("ccoef", 14 * h, DT_F32);
  for (int k = 0; k < 3; ++k) { c.W[k] = b.pptr(wn[k]); c.RV[k] = b.sptr(rvn[k]); }
  c.Bv[0] = b.pptr("Br"); c.Bv[1] = b.pptr("Bi");
  c.RM[0] = b.sptr("RMr"); c.RM[1] = b.sptr("RMi");
  c.slope = slope; c.totals = b.none();
  layout(P->fwd, 0, io_x, y);
  if (cfg.training) b.push(P->fwd, OP_CBN_STATS, 2).cbf = c;
  b.push(P->fwd, OP_CBN_FINALIZE, 2).cbf = c;
  b.push(P->fwd, OP_CBN_APPLY, 2).cbf = c;
  layout(P->fwd, 1, io_y, z);

  CbnBwd cb;
  std::memset(&cb, 0, sizeof(cb));
  cb.y = y; cb.dz0 = dz; cb.dz1 = b.none(); cb.dy = dy; cb.coef = c.coef;
  cb.coefb = b.ws("ccoefb", 9 * h, DT_F32);
  cb.part = b.ws("cbnpart", (int64_t)nblk * 7 * h, DT_F32);
  for (int k = 0; k < 3; ++k) { cb.W[k] = b.pptr(wn[k]); cb.dW[k] = b.pptr(wn[k], A_GRAD); }
  cb.dB[0] = b.pptr("Br", A_GRAD); cb.dB[1] = b.pptr("Bi", A_GRAD);
  cb.slope = slope; cb.dslope = dslope; cb.totals = b.none();
  cb.R = Rr; cb.rpb = S; cb.C = C; cb.dt = adt; cb.nblk = nblk; cb.rows_per_blk = (int)rpbk; cb.skip = 0;
  cb.count = cfg.training ? (double)Rr : HUGE_VAL;
  layout(P->bwd, 2, io_gy, dz);
  b.push(P->bwd, OP_CBN_BWD_REDUCE, 2).cbb = cb;
  b.push(P->bwd, OP_CBN_BWD_FINALIZE, 2).cbb = cb;
  b.push(P->bwd, OP_CBN_BWD_APPLY, 2).cbb = cb;
  layout(P->bwd, 3, io_gx, dy);
  finish_plan(b, P, nparam, nstate);
  return P;
}

}  // namespace sefd
