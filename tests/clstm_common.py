"""Shared by tests/test_clstm_cpu.py, tests/test_gpu_clstm.py and tests/golden/make_clstm_golden.py (a plain module, not a conftest): the NavieComplexLSTM
cases, the formula weights keyed like the reference's state_dict, the closed-form inputs, a plain float64 reference (with a variant that rounds like a bf16
plan), the plan's batch-major boundary, and the comparisons at the project's bars (restated from tests/recurrence_cases.py, which restates
tests/test_gpu_model.py).

Nothing here is imported from the reference: the fixtures under tests/golden/ carry its results."""
import numpy as np
import torch

from oracle.weights import formula_state_dict, splitmix_uniform
from recurrence_cases import BF16_GRAD_L2, BF16_GRAD_WORST, BF16_OUT_L2, BF16_OUT_MAX, EMU_FACTOR, TOL, _RoundBF16  # noqa: F401
from util import rel_err, rel_l2, sub

# name: (input_size, hidden_size, projection_dim, bidirectional, B, T)
CASES = {
    "uni_h32_proj": (48, 64, 40, False, 3, 9),           # projection width 20, not a multiple of 8
    "bi_h32": (48, 64, None, True, 3, 9),                # two directions, no projection
    "bi_h128_proj": (80, 256, 96, True, 5, 10),          # DCCRN's H; B = 5 leaves a partial workgroup at 4 sequences per workgroup
    "bi_h192_proj": (80, 384, 96, True, 18, 10),         # cluster kernels in bf16, stepped in fp32
    "uni_h24": (48, 48, None, False, 3, 9),              # stepped in both dtypes
}
STRIDE = 211          # make_clstm_golden.py: sample(v, 211)
OP_LSTM_FWD, OP_LSTM_BWD, OP_CELL_FWD, OP_CELL_BWD = 9, 10, 23, 24          # sefd_desc.h OpKind


def sizes(case):
    """dict(I, H, P, D, B, T, O): per-part sizes, directions, and O = the width of each output."""
    isz, hsz, pdim, bi, B, T = case
    I, H, P, D = isz // 2, hsz // 2, (None if pdim is None else pdim // 2), (2 if bi else 1)
    return dict(I=I, H=H, P=P, D=D, B=B, T=T, O=P if P is not None else D * H)


def clstm_dict(case):
    isz, hsz, pdim, bi, _, _ = case
    return dict(input_size=isz, hidden_size=hsz, projection_dim=pdim, bidirectional=bi)


def torch_shapes(case):
    """{state_dict name: shape} of the reference's NavieComplexLSTM: torch's own nn.LSTM state_dict twice, then r_trans / i_trans."""
    s = sizes(case)
    shapes = {}
    for part in ("real_lstm", "imag_lstm"):
        rnn = torch.nn.LSTM(s["I"], s["H"], 1, bidirectional=s["D"] == 2, batch_first=False)
        shapes.update({f"{part}.{k}": tuple(v.shape) for k, v in rnn.state_dict().items()})
    if s["P"] is not None:
        for t in ("r_trans", "i_trans"):
            shapes[t + ".weight"] = (s["P"], s["D"] * s["H"])
            shapes[t + ".bias"] = (s["P"],)
    return shapes


def formula_params(case):
    return formula_state_dict(torch_shapes(case))


def inputs(case):
    """(x_real, x_imag [T, B, I], g_real, g_imag [T, B, O]): streams 1001 .. 1004 of oracle/weights.py, at scale 1."""
    s = sizes(case)
    T, B, I, O = s["T"], s["B"], s["I"], s["O"]
    mk = lambda idx, w: torch.from_numpy(splitmix_uniform(idx, T * B * w).astype(np.float32).reshape(T, B, w))
    return mk(1001, I), mk(1002, I), mk(1003, O), mk(1004, O)


def loss_of(out_r, out_i, g_r, g_i):
    return (out_r * g_r).mean() + (out_i * g_i).mean()


def loss_scale(out_r, out_i, g_r, g_i):
    """What an error of the loss is measured against: mean |out . g| over both outputs (the loss itself is a sum of terms of both signs)."""
    return float((out_r.double() * g_r.double()).abs().mean() + (out_i.double() * g_i.double()).abs().mean())


# ------------------------------------------------------------------------------------------------ the plain reference
class _RoundGradBF16(torch.autograd.Function):
    """Identity in the forward, the gradient rounded to bf16 (nearest even) in the backward."""

    @staticmethod
    def forward(ctx, v):
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def plain_forward(case, W, real, imag, bf16=False, hs=None):
    """tools_for_model.py:162-177 on differentiable tensors: W {state_dict name: tensor}, real / imag [T, B, I] -> (out_r, out_i) [T, B, O]; loops over
    parameter sets, directions and frames with torch's LSTM equations and gate order (i, f, g, o), each of the four LSTM calls from zero state.
    bf16: see plain_reference.  hs: dict that receives every hidden sequence as {(set, part, direction): [T, B, H]}."""
    s = sizes(case)
    H, D = s["H"], s["D"]
    T, B = real.shape[0], real.shape[1]
    dtype = real.dtype
    rnd = _RoundBF16.apply if bf16 else (lambda v: v)
    w = lambda name: rnd(W[name]) if W[name].dim() == 2 else W[name]

    def lstm(part, x, key):                                       # one nn.LSTM call: [T, B, I] -> [T, B, D * H]
        outs = []
        for d in range(D):
            sfx = "_l0" + ("_reverse" if d else "")
            wih, whh = w(f"{part}.weight_ih{sfx}"), w(f"{part}.weight_hh{sfx}")
            bih, bhh = W[f"{part}.bias_ih{sfx}"], W[f"{part}.bias_hh{sfx}"]
            h = torch.zeros(B, H, dtype=dtype)
            c = torch.zeros(B, H, dtype=dtype)
            seq = [None] * T
            for k in range(T):
                t = T - 1 - k if d else k
                a = x[t] @ wih.t() + bih + h @ whh.t() + bhh
                ai, af, ag, ao = a.split(H, 1)
                c = torch.sigmoid(af) * c + torch.sigmoid(ai) * torch.tanh(ag)
                h = rnd(torch.sigmoid(ao) * torch.tanh(c))
                seq[t] = h
            outs.append(torch.stack(seq))
            if hs is not None:
                hs[key + (d,)] = outs[-1].detach()
        return torch.cat(outs, 2)

    real, imag = rnd(real), rnd(imag)
    r2r, r2i = lstm("real_lstm", real, ("real_lstm", 0)), lstm("imag_lstm", real, ("imag_lstm", 0))
    i2r, i2i = lstm("real_lstm", imag, ("real_lstm", 1)), lstm("imag_lstm", imag, ("imag_lstm", 1))
    out_r, out_i = rnd(r2r - i2i), rnd(i2r + r2i)
    if s["P"] is not None:
        rg = _RoundGradBF16.apply if bf16 else (lambda v: v)
        out_r = rg(out_r @ w("r_trans.weight").t() + W["r_trans.bias"])
        out_i = rg(out_i @ w("i_trans.weight").t() + W["i_trans.bias"])
    return out_r, out_i


def plain_reference(case, P, xr, xi, gr, gi, dtype=torch.float64, bf16=False):
    """plain_forward, loss = mean(out_r g_r) + mean(out_i g_i), backward.  dtype: what everything is computed in.  bf16=True emulates the storage of a
    bf16 plan and nothing else: weight matrices and inputs rounded to bf16, h rounded to bf16 after every frame and the combined outputs once more
    (straight-through gradients), and the upstream gradient of the projection rounded to bf16 (a bf16 plan holds the operands of the projection's
    backward GEMMs in bf16; with this loss, linear in the outputs, the gradient of r_trans.bias / i_trans.bias depends on nothing else); biases, gates,
    cell state and every sum in `dtype`.
    Returns dict(out_r, out_i [T, B, O], loss, loss_scale, dxr, dxi, grads {state_dict name: grad}, h {(set, part, d): [T, B, H]})."""
    W = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    xs = [t.detach().to(dtype).clone().requires_grad_(True) for t in (xr, xi)]
    hs = {}
    out_r, out_i = plain_forward(case, W, xs[0], xs[1], bf16=bf16, hs=hs)
    loss = loss_of(out_r, out_i, gr.to(dtype), gi.to(dtype))
    names = list(W)
    g = torch.autograd.grad(loss, [W[k] for k in names] + xs)
    return dict(out_r=out_r.detach(), out_i=out_i.detach(), loss=float(loss.detach()), loss_scale=loss_scale(out_r.detach(), out_i.detach(), gr, gi),
                dxr=g[-2], dxi=g[-1], grads=dict(zip(names, g[:-2])), h=hs)


_refs = {}


def reference(name, dtype=torch.float64, bf16=False):
    """plain_reference of a case on its formula weights and inputs: computed once per process, shared by the tests that need it, never changed."""
    key = (name, dtype, bf16)
    if key not in _refs:
        _refs[key] = plain_reference(CASES[name], formula_params(CASES[name]), *inputs(CASES[name]), dtype=dtype, bf16=bf16)
    return _refs[key]


# ------------------------------------------------------------------------------------------------ the plan's boundary
def to_plan_x(case, xr, xi):
    """[T, B, I] x 2 -> io.x [B, T, 2 IP] (real | imaginary, zero pad columns)."""
    pad = -sizes(case)["I"] % 8
    f = torch.nn.functional.pad
    return torch.cat([f(xr, (0, pad)), f(xi, (0, pad))], 2).permute(1, 0, 2).contiguous()


def from_plan_y(case, plan, ar):
    """(out_r, out_i), each [T, B, O] fp32, from io.y or the combined-output buffer `hc`."""
    s = sizes(case)
    B, T, H, P, D = s["B"], s["T"], s["H"], s["P"], s["D"]
    if P is not None:
        y = plan.io(ar, "y", (B, T, 2 * P)).float().cpu()
        halves = (y[..., :P], y[..., P:])
    else:
        hc = plan.view(ar, "hc").view(D, B, T, 2 * H).float().cpu()
        halves = tuple(torch.cat([hc[d][..., p * H:(p + 1) * H] for d in range(D)], -1) for p in (0, 1))
    return tuple(h.permute(1, 0, 2).contiguous() for h in halves)


def to_plan_gy(case, gr, gi):
    """Gradients of the two outputs [T, B, O] -> io.grad_y ([B, T, 2 P], or [D, B, T, 2 H])."""
    s = sizes(case)
    H, P, D = s["H"], s["P"], s["D"]
    gr, gi = gr.permute(1, 0, 2), gi.permute(1, 0, 2)
    if P is not None:
        return torch.cat([gr, gi], 2).contiguous()
    return torch.stack([torch.cat([gr[..., d * H:(d + 1) * H], gi[..., d * H:(d + 1) * H]], 2) for d in range(D)]).contiguous()


def from_plan_gx(case, plan, ar):
    s = sizes(case)
    IP = s["I"] + (-s["I"] % 8)
    gx = plan.io(ar, "grad_x", (s["B"], s["T"], 2 * IP)).float().cpu().permute(1, 0, 2)
    return gx[..., :s["I"]].contiguous(), gx[..., IP:IP + s["I"]].contiguous()


# ------------------------------------------------------------------------------------------------ comparisons
def errors(ref, out_r, out_i, loss, dxr, dxi, grads):
    """Every figure the bars apply to against a reference dict(out_r, out_i, loss, dxr, dxi, grads): max-abs over max-abs and rel-L2 of the outputs
    and input gradients, the loss against the sum of the magnitudes of its terms' means (it is a sum with cancellation), per gradient tensor rel-L2."""
    e = {}
    for k, got in (("out_r", out_r), ("out_i", out_i), ("dxr", dxr), ("dxi", dxi)):
        e[k], e[k + "_l2"] = rel_err(got, ref[k]), rel_l2(got, ref[k])
    e["loss"] = abs(float(loss) - float(ref["loss"])) / float(ref["loss_scale"]) if "loss_scale" in ref else None
    e["grad"] = {k: rel_l2(grads[k], v) for k, v in ref["grads"].items()}
    e["grad_max"] = {k: rel_err(grads[k], v) for k, v in ref["grads"].items()}
    return e


def golden_ref(g):
    """A golden as the dict `errors` takes; the sampled gradients stay out of ref['grads'] (golden_errors adds them)."""
    return dict(out_r=g["g/out_r"], out_i=g["g/out_i"], loss=float(g["g/loss"]), loss_scale=float(g["g/meta/loss_scale"]), dxr=g["g/dxr"], dxi=g["g/dxi"],
                grads={k: torch.from_numpy(v) for k, v in sub(g, "g/grad").items()})


def golden_errors(g, out_r, out_i, loss, dxr, dxi, grads):
    e = errors(golden_ref(g), out_r, out_i, loss, dxr, dxi, grads)
    for k, v in sub(g, "g/grad_samp").items():
        e["grad"][k] = rel_l2(grads[k].reshape(-1)[::STRIDE], v)
        e["grad_max"][k] = rel_err(grads[k].reshape(-1)[::STRIDE], v)
    e["norm"] = {k: abs(float(grads[k].double().norm()) - float(v)) / float(v) for k, v in sub(g, "g/grad_norm").items()}
    return e


def assert_fp32(e, tol=TOL):
    for k in ("out_r", "out_i", "dxr", "dxi"):
        assert e[k] < tol, (k, e[k])
    assert e["loss"] is None or e["loss"] < tol, ("loss", e["loss"])
    for k, v in e["grad_max"].items():
        assert v < tol, ("grad", k, v)
    for k, v in e.get("norm", {}).items():
        assert v < tol, ("grad_norm", k, v)


def assert_bf16(e):
    """The project's bf16 bars: outputs rel-L2 < BF16_OUT_L2 and max-norm < BF16_OUT_MAX; gradients (the two input gradients are two more gradient
    tensors) rel-L2 median < BF16_GRAD_L2 and worst < BF16_GRAD_WORST."""
    for k in ("out_r", "out_i"):
        assert e[k + "_l2"] < BF16_OUT_L2 and e[k] < BF16_OUT_MAX, (k, e[k + "_l2"], e[k])
    gl = sorted(list(e["grad"].values()) + [e["dxr_l2"], e["dxi_l2"]])
    assert gl[len(gl) // 2] < BF16_GRAD_L2 and gl[-1] < BF16_GRAD_WORST, gl


def assert_bf16_against_emulation(e, emu):
    """bf16 results against fp64: outputs at the bf16 bars; the input gradients and every gradient tensor at EMU_FACTOR x the rel-L2 error the
    bf16-emulating reference itself has on that tensor, never above BF16_GRAD_L2."""
    for k in ("out_r", "out_i"):
        assert e[k + "_l2"] < BF16_OUT_L2 and e[k] < BF16_OUT_MAX, (k, e[k + "_l2"], e[k])
    for k, got, own in [("dxr", e["dxr_l2"], emu["dxr_l2"]), ("dxi", e["dxi_l2"], emu["dxi_l2"])] + [(k, v, emu["grad"][k]) for k, v in e["grad"].items()]:
        bar = min(EMU_FACTOR * own, BF16_GRAD_L2)
        assert got <= bar, (k, got, bar)


def emulation_errors(name):
    """The bf16-emulating reference against the fp64 one."""
    ref, emu = reference(name), reference(name, bf16=True)
    return errors(ref, emu["out_r"], emu["out_i"], emu["loss"], emu["dxr"], emu["dxi"], emu["grads"])


def lstm_launches(plan, abi):
    """[(phase, rev_mask, G, t0, t1)] of the OP_LSTM_FWD / OP_LSTM_BWD ops of a plan, in program order (abi: tests/golden/seqmodel_abi.json)."""
    import ctypes as C
    sz, u, off = abi["sefd_op_size"] // 4, abi["op_union_offset"], abi["lstm_rec_offsets"]
    out = []
    for ph, kind in ((0, OP_LSTM_FWD), (1, OP_LSTM_BWD)):
        n = plan.num_ops(ph)
        if not n:
            continue
        raw = np.ctypeslib.as_array((C.c_int32 * (n * sz)).from_address(plan.ops_ptr(ph))).reshape(n, sz)
        for row in raw[raw[:, 0] == kind]:
            f = {k: int(row[(u + o) // 4]) for k, o in off.items()}
            out.append((ph, f["rev_mask"], f["G"], f["t0"], f["t1"]))
    return out


def count_ops(plan, phase, kind):
    return int((plan.op_kinds(phase)[0] == kind).sum()) if plan.num_ops(phase) else 0
