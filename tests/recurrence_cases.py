"""Shared by tests/test_recurrence_cases_cpu.py and tests/test_gpu_recurrence_edges.py (a plain module, not a conftest): gate biases that
saturate the recurrences' non-linearities, a plain fp64 LSTM / GRU + Linear reference that hands out every gate pre-activation (and a variant of
it that rounds like a bf16 plan), and the case tables of both tiers.

The formula weights (oracle/weights.py) leave every gate pre-activation within about +-4, so sigmoid and tanh - written in the kernels as
rcp(1 + exp2(-1.4427 a)) and 1 - 2 rcp(exp2(2.885 a) + 1) - never reach the range where exp2 overflows to inf or the result flushes to zero, and
the backward factors s (1 - s) and 1 - t^2 are never exactly 0.  Scaling the recurrent weights does not get there (the recurrence turns chaotic and
the reference no longer agrees with its own fp32 run); an offset on the gate biases of selected units does, and leaves the gain unchanged."""
import re

import torch

from seqmodel_common import ACTS, formula_params, torch_shapes
from util import rel_err, rel_l2

# the project's bars (tests/test_gpu_model.py, restated here so that the CPU tier does not import a GPU suite; tests/test_gpu_recurrence_edges.py
# asserts that they are the same numbers)
TOL = 1e-3
BF16_OUT_L2, BF16_OUT_MAX, BF16_GRAD_L2, BF16_GRAD_WORST, BF16_LOSS = 2e-2, 5e-2, 8e-2, 0.35, 2e-2
EMU_FACTOR = 8            # simulator / kernels against fp64: at most 8 x what the bf16-emulating reference itself measures (and never above BF16_GRAD_L2)

# unit j of a layer gets the offset on gate block q (torch's order: LSTM i, f, g, o; GRU r, z, n) by j mod 16: {residue: ((q, sign), ...)}
HOT = {1: ((0, +1),), 2: ((1, +1),), 3: ((2, -1),), 5: ((3, -1),), 6: ((0, -1),), 7: ((1, -1),), 9: ((2, +1),), 10: ((3, +1),)}
# LSTM only: i = f = 1 and g = +-1, so the cell state is c_t = +-t and tanh(c) saturates as the frames go by
ACCUMULATE = {11: ((0, +1), (1, +1), (2, +1)), 12: ((0, +1), (1, +1), (2, -1))}
_BIAS_IH = re.compile(r"(.*)bias_ih_l(\d+)(_reverse)?$")


def hot_biases(P, offset=100.0, accumulate=False):
    """A copy of {state_dict name: tensor} with +-offset added to every `...bias_ih_l*` tensor (`_reverse` included): SequenceModel, DCCRN's
    enhance.*.{real,imag}_lstm and its lstm='real' stack, CRN's LSTM, FullSubNet's two models.  LSTM or GRU is read off the matching weight_hh
    ([4H, H] or [3H, H]); GRU has no fourth block, so its residues 5 and 10 get nothing."""
    out = {k: v.clone() for k, v in P.items()}
    for k, v in P.items():
        m = _BIAS_IH.match(k)
        if not m:
            continue
        whh = P[f"{m.group(1)}weight_hh_l{m.group(2)}{m.group(3) or ''}"]
        H = whh.shape[1]
        nq = whh.shape[0] // H
        assert nq in (3, 4) and tuple(v.shape) == (nq * H,), (k, tuple(v.shape), tuple(whh.shape))
        table = {**HOT, **ACCUMULATE} if accumulate and nq == 4 else HOT
        b = out[k].view(nq, H)
        for j in range(H):
            for q, sign in table.get(j % 16, ()):
                if q < nq:
                    b[q, j] += sign * offset
    return out


# ------------------------------------------------------------------------------------------------ the plain reference
class _RoundBF16(torch.autograd.Function):
    """Round to bf16 (nearest even) in the forward, identity in the backward (straight through)."""

    @staticmethod
    def forward(ctx, v):
        return v.to(torch.bfloat16).to(v.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def plain_reference(seq, I, O, H, NL, bi, act, P, x, tgt, dtype=torch.float64, bf16=False):
    """LSTM / GRU (torch's equations and gate order) + Linear + activation, written as loops over layers, directions and frames.
    x [B, I, T], tgt [B, O, T]; loss = mean((y - tgt)^2).  dtype: what everything is computed in (float64: the reference; float32: its own fp32 run).
    bf16=True emulates the storage of a bf16 plan and nothing else: weight matrices and x rounded to bf16, h rounded to bf16 after every frame with a
    straight-through gradient, biases, gates, cell state and every sum in `dtype`.
    Returns dict(y, loss, dx, grads {state_dict name: grad}, pre: every gate pre-activation as one flat tensor, cmax: largest |cell state|)."""
    rnd = _RoundBF16.apply if bf16 else (lambda v: v)
    W = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    w = lambda name: rnd(W[name]) if W[name].dim() == 2 else W[name]
    xd = x.detach().to(dtype).clone().requires_grad_(True)
    inp = rnd(xd).permute(2, 0, 1)                                       # [T, B, I]
    T, B = inp.shape[0], inp.shape[1]
    pre, cmax = [], 0.0
    for l in range(NL):
        outs = []
        for d in range(2 if bi else 1):
            sfx = f"_l{l}" + ("_reverse" if d else "")
            wih, whh = w("sequence_model.weight_ih" + sfx), w("sequence_model.weight_hh" + sfx)
            bih, bhh = W["sequence_model.bias_ih" + sfx], W["sequence_model.bias_hh" + sfx]
            h = torch.zeros(B, H, dtype=dtype)
            c = torch.zeros(B, H, dtype=dtype)
            hs = [None] * T
            for s in range(T):
                t = T - 1 - s if d else s
                gi = inp[t] @ wih.t() + bih
                gh = h @ whh.t() + bhh
                if seq == "LSTM":
                    a = gi + gh
                    pre.append(a.detach().reshape(-1))
                    ai, af, ag, ao = a.split(H, 1)
                    c = torch.sigmoid(af) * c + torch.sigmoid(ai) * torch.tanh(ag)
                    cmax = max(cmax, float(c.detach().abs().max()))
                    h = torch.sigmoid(ao) * torch.tanh(c)
                else:
                    ir, iz, in_ = gi.split(H, 1)
                    hr, hz, hn = gh.split(H, 1)
                    r = torch.sigmoid(ir + hr)
                    an = in_ + r * hn
                    pre.append(torch.cat([(ir + hr).detach(), (iz + hz).detach(), an.detach()], 1).reshape(-1))
                    z = torch.sigmoid(iz + hz)
                    h = (1 - z) * torch.tanh(an) + z * h
                h = rnd(h)
                hs[t] = h
            outs.append(torch.stack(hs))
        inp = torch.cat(outs, 2) if bi else outs[0]
    y = ACTS[act](inp @ w("fc_output_layer.weight").t() + W["fc_output_layer.bias"]).permute(1, 2, 0)      # [B, O, T]
    loss = ((y - tgt.detach().to(dtype)) ** 2).mean()
    names = list(W)
    g = torch.autograd.grad(loss, [W[k] for k in names] + [xd])
    return dict(y=y.detach(), loss=float(loss.detach()), dx=g[-1], grads=dict(zip(names, g[:-1])), pre=torch.cat(pre), cmax=cmax)


def errors_against(ref, y, loss, dx, grads):
    """The figures of seqmodel_common.golden_errors against a plain_reference result: y / dx max-norm and rel-L2, loss, and per gradient tensor
    the norm's relative error and the rel-L2 error."""
    return dict(y=rel_err(y, ref["y"]), y_l2=rel_l2(y, ref["y"]), dx=rel_err(dx, ref["dx"]), dx_l2=rel_l2(dx, ref["dx"]),
                loss=abs(float(loss) - ref["loss"]) / abs(ref["loss"]),
                norm={k: abs(float(grads[k].double().norm()) - float(v.double().norm())) / float(v.double().norm()) for k, v in ref["grads"].items() if float(v.norm()) > 0},
                grad={k: rel_l2(grads[k], v) for k, v in ref["grads"].items()})


def all_finite(y, loss, dx, grads):
    """Explicitly: a NaN must not pass through a max over a NaN comparison."""
    import math
    return math.isfinite(float(loss)) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())


# ------------------------------------------------------------------------------------------------ SequenceModel cases
I_, O_, ACT = 21, 5, "Tanh"


def seq_case(name):
    """name -> dict(seq, I, O, H, NL, bi, act, B, T, dtype)."""
    seq, H, NL, bi, B, T, dtype = SEQ_CASES[name]
    return dict(seq=seq, I=I_, O=O_, H=H, NL=NL, bi=bi, act=ACT, B=B, T=T, dtype=dtype)


# name: (sequence_model, H, layers, bidirectional, B, T, dtype)
SEQ_CASES = {
    # CPU tier, simulator against fp64 (fp32 at TOL; bf16 at the bf16 bars) - and, fp32 ones and the two T >= 10 cluster ones, GPU modules against fp64
    "f32_lstm_T67": ("LSTM", 64, 2, True, 3, 67, "fp32"),
    "f32_gru_T67": ("GRU", 64, 2, True, 3, 67, "fp32"),
    "bf16_h192_l1_bi": ("LSTM", 192, 1, True, 18, 10, "bf16"),          # one-launch BLSTM: reversed group, two row blocks (18 sequences > 16)
    "bf16_h192_l2_bi": ("LSTM", 192, 2, True, 18, 10, "bf16"),
    "bf16_h256_l2_bi": ("LSTM", 256, 2, True, 3, 4, "bf16"),
    "bf16_h512_l1_bi": ("LSTM", 512, 1, True, 2, 5, "bf16"),
    "bf16_h192_l3_uni": ("LSTM", 192, 3, False, 17, 10, "bf16"),
    # GPU tier only
    "f32_lstm_l3": ("LSTM", 64, 3, True, 3, 9, "fp32"),                 # cell kernels
    "f32_gru_l3": ("GRU", 64, 3, True, 3, 9, "fp32"),
    "bf16_h256_B1_T1": ("LSTM", 256, 1, True, 1, 1, "bf16"),
    "bf16_gru_l2": ("GRU", 64, 2, True, 3, 9, "bf16"),
    "bf16_h192_l2_bi_T67": ("LSTM", 192, 2, True, 18, 67, "bf16"),
    "bf16_h512_l1_bi_T10": ("LSTM", 512, 1, True, 2, 10, "bf16"),
}
CPU_SIM_CASES = ["f32_lstm_T67", "f32_gru_T67", "bf16_h192_l1_bi", "bf16_h192_l2_bi", "bf16_h256_l2_bi", "bf16_h512_l1_bi", "bf16_h192_l3_uni"]
# (case, knobs): every launch against the simulator on the GPU, plain and saturated
GPU_OP_CASES = [("f32_lstm_l3", ()), ("f32_gru_l3", ()), ("bf16_h192_l2_bi", ()), ("bf16_h256_B1_T1", ()), ("bf16_h512_l1_bi", ()), ("bf16_h192_l3_uni", ()),
                ("bf16_h192_l2_bi", (("LSTM_STEPPED", "1"),)), ("bf16_gru_l2", ())]
# modules against fp64 with accumulate=True (cell state +-T)
GPU_MODULE_CASES = ["f32_lstm_T67", "f32_gru_T67", "bf16_h192_l2_bi_T67", "bf16_h512_l1_bi_T10"]

_inputs, _refs = {}, {}


def head_scale(c, P, x):
    """The rule of test_gpu_seqmodel.edge_reference: the formula weights leave the head's pre-activations small, so the head is scaled by the smallest
    power of two at which its Tanh bends (at least 1 % of |y| beyond tanh(1)); 16 at H = 192, less for wider layers.  The recurrent features do not
    depend on the head, so they are computed once (torch's own modules in fp64)."""
    rnn = (torch.nn.LSTM if c["seq"] == "LSTM" else torch.nn.GRU)(c["I"], c["H"], c["NL"], batch_first=True, bidirectional=c["bi"]).double()
    rnn.load_state_dict({k[len("sequence_model."):]: v.double() for k, v in P.items() if k.startswith("sequence_model.")})
    with torch.no_grad():
        z = rnn(x.double().permute(0, 2, 1))[0] @ P["fc_output_layer.weight"].double().t() + P["fc_output_layer.bias"].double()
    for e in range(17):
        if float((z.abs() * 2.0 ** e > 1.0).double().mean()) >= 0.01:
            return 2.0 ** e
    raise AssertionError("no head scale up to 2^16 bends the Tanh")


def seq_inputs(name, hot, accumulate=False):
    """(case dict, P, x, tgt): formula weights (with saturating biases) and the head scaled by head_scale, x = 6 rand, tgt in (-1, 1), seed 11."""
    key = (name, hot, accumulate)
    if key not in _inputs:
        c = seq_case(name)
        gen = torch.Generator().manual_seed(11)
        x = 6 * torch.rand(c["B"], c["I"], c["T"], generator=gen)
        tgt = 2 * torch.rand(c["B"], c["O"], c["T"], generator=gen) - 1
        P = formula_params(torch_shapes(c["seq"], c["I"], c["O"], c["H"], c["NL"], c["bi"]))
        if hot:
            P = hot_biases(P, accumulate=accumulate)
        scale = head_scale(c, P, x)
        for leaf in ("weight", "bias"):
            P["fc_output_layer." + leaf] = P["fc_output_layer." + leaf] * scale
        c["head_scale"] = scale
        _inputs[key] = (c, P, x, tgt)
    return _inputs[key]


def seq_reference(name, hot, accumulate=False, dtype=torch.float64, bf16=False):
    """plain_reference of a case: computed once per process, shared by the tests that need it, never changed."""
    key = (name, hot, accumulate, dtype, bf16)
    if key not in _refs:
        c, P, x, tgt = seq_inputs(name, hot, accumulate)
        _refs[key] = plain_reference(c["seq"], c["I"], c["O"], c["H"], c["NL"], c["bi"], c["act"], P, x, tgt, dtype=dtype, bf16=bf16)
    return _refs[key]


def input_conditions(name, hot, accumulate=False):
    """What makes a saturated case a test, asserted from the reference alone.  Returns the figures."""
    c = seq_case(name)
    ref = seq_reference(name, hot, accumulate)
    a = ref["pre"].abs()
    fig = dict(beyond45=float((a > 45).double().mean()), beyond89=float((a > 89).double().mean()), within8=float((a <= 8).double().mean()), cmax=ref["cmax"])
    if hot:
        # 8 of the 64 (LSTM) / 6 of the 48 (GRU) gate blocks per 16 units carry the offset: 12.5 % by construction
        assert fig["beyond45"] >= 0.05 and fig["beyond89"] >= 0.05, (name, fig)
        # accumulate=True offsets 6 more of the 64 blocks, 14 / 64 = 21.9 % in all: 78.1 % is the most that can stay within +-8, so that case asks for 75 %
        assert fig["within8"] >= (0.75 if accumulate and c["seq"] == "LSTM" else 0.80), (name, fig)
    if hot and accumulate and c["seq"] == "LSTM":
        # c_t = +-t on residues 11 and 12: the cell state reaches T.  T = 67: beyond 45, where the kernels' tanh runs on an overflowed exp2;
        # T = 10: 1 - tanh(10) = 4e-9, below half an fp32 ulp of 1 - saturated all the same
        assert fig["cmax"] >= min(45.0, c["T"] - 1e-6), (name, fig)
    f32 = seq_reference(name, hot, accumulate, dtype=torch.float32)
    e32 = errors_against(ref, f32["y"], f32["loss"], f32["dx"], f32["grads"])
    fig["fp32_self"] = max([e32["y_l2"], e32["dx_l2"]] + list(e32["grad"].values()))
    assert fig["fp32_self"] <= 1e-4, (name, fig)
    if c["dtype"] == "bf16":
        emu = emulation_errors(name, hot, accumulate)
        fig["emu_y"], fig["emu_dx"], fig["emu_grad_worst"] = emu["y_l2"], emu["dx_l2"], max(emu["grad"].values())
        if hot:         # the bf16 storage itself must leave half of the budgets to the plan's own arithmetic
            assert emu["y_l2"] <= BF16_OUT_L2 / 2 and emu["dx_l2"] <= BF16_GRAD_L2 / 2 and fig["emu_grad_worst"] <= BF16_GRAD_L2 / 2, (name, fig)
    return fig


def emulation_errors(name, hot, accumulate=False):
    """The bf16-emulating reference against the fp64 one."""
    ref = seq_reference(name, hot, accumulate)
    emu = seq_reference(name, hot, accumulate, bf16=True)
    return errors_against(ref, emu["y"], emu["loss"], emu["dx"], emu["grads"])


def assert_bf16_against_emulation(e, emu, tag):
    """Outputs at the project's bf16 budgets; dx and every gradient tensor at EMU_FACTOR x the emulation's own rel-L2 figure of that tensor (the
    emulation rounds weights, inputs and h; a plan also stores gate slabs in bf16: unidirectional plans measure 0.5 .. 4.1 x), never above BF16_GRAD_L2."""
    assert e["y_l2"] < BF16_OUT_L2 and e["y"] < BF16_OUT_MAX and e["loss"] < BF16_LOSS, (tag, e["y_l2"], e["y"], e["loss"])
    for k, got in [("dx", e["dx_l2"])] + list(e["grad"].items()):
        bar = min(EMU_FACTOR * (emu["dx_l2"] if k == "dx" else emu["grad"][k]), BF16_GRAD_L2)
        assert got <= bar, (tag, k, got, bar)


# ------------------------------------------------------------------------------------------------ DCCRN / CRN / FullSubNet with saturated biases
SMALL_KN = (16, 32, 32, 64, 64, 64)
# CPU tier, through the hooked checkers of plan_check.py at their existing bars (offset 100 everywhere: no case needed a lower one)
DCCRN_CPU = [("complex", dict(kernel_num=SMALL_KN, rnn_units=128), 2, 3000), ("real", dict(kernel_num=SMALL_KN, rnn_units=64, lstm="real"), 2, 3000)]
CRN_CPU = [("crn", dict(kernel_num=SMALL_KN, rnn_units=128), 2, 3000)]
FSN_CPU = [("LSTM", "offline_laplace_norm"), ("GRU", "offline_laplace_norm")]
# GPU tier: one row of test_gpu_ops.test_every_op_against_host_simulator per recurrence variant (model, B, L, mode, kernel_num / hidden sizes, rnn_units,
# dtype), steered by that test's knobs (an L of 4001 is its marker for LSTM_RPW=16 beside the direct-operand kernels)
BIG_KN = (32, 64, 128, 256, 256, 256)
GPU_PLAN_ROWS = [("DCCRN", 3, 4000, "E", SMALL_KN, 128, "fp32"),           # kernels.hip persistent
                 ("DCCRN", 3, 4000, "R", SMALL_KN, 128, "bf16"),           # lstm_bf16.hip, 4 sequences per workgroup
                 ("DCCRN", 3, 4001, "R", SMALL_KN, 128, "bf16"),           # the same with LSTM_RPW=16
                 ("DCCRN", 2, 3400, "C", SMALL_KN, 128, "bf16"),           # chunked two-stream forward
                 ("DCCRN", 18, 2000, "C", SMALL_KN, 512, "bf16"),          # cluster, two row blocks
                 ("DCCRN", 1, 1600, "C", SMALL_KN, 1024, "bf16"),          # cluster, H = 512
                 ("DCCRN", 1, 1200, "C", SMALL_KN, 512, "fp32"),           # per-frame fp32
                 ("CRN", 2, 2400, "E", BIG_KN, 256, "bf16"),
                 ("FullSubNet", 2, 9, "E", (64, 32), 0, "bf16"),
                 ("FullSubNet", 2, 8, "GRU/offline_gaussian_norm", (64, 32), 0, "fp32"),
                 ("FullSubNet", 2, 9, "E", (256, 192), 0, "bf16"),
                 ("FullSubNet", 1, 10, "E", (512, 384), 0, "bf16"),        # LSTM_MT=3
                 ("FullSubNet", 1, 11, "E", (512, 384), 0, "bf16"),        # LSTM_ROWS_MIN=64: row-block kernels, fused projection, head, dropout at keep 0.2
                 ("FullSubNet", 1, 11, "E", (256, 256), 0, "bf16")]
