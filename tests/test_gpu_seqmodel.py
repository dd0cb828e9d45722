"""GPU: SequenceModel on its own - any depth, both directions, LSTM and GRU - against goldens captured from the real reference
(tests/golden/make_seqmodel_golden.py; pinned on the CPU by tests/test_seqmodel_cpu.py) and, at the edge shapes, against torch's own
nn.LSTM / nn.GRU + Linear in fp64 on the CPU.  Budgets are the project's own: TOL (fp32) and the named bf16 budgets of tests/test_gpu_model.py."""
import numpy as np
import pytest
import torch

from oracle.weights import fill_state_dict_
from seqmodel_common import CASES, assert_fp32, formula_params, golden_errors, torch_reference, torch_shapes
from test_gpu_model import BF16_GRAD_L2, BF16_GRAD_WORST, BF16_LOSS, BF16_OUT_L2, BF16_OUT_MAX, TOL
from util import knobs, load_golden, rel_err, rel_l2

pytestmark = pytest.mark.gpu
OP_LSTM_FWD, OP_LSTM_BWD = 9, 10          # sefd_desc.h OpKind


def make_model(seq, I, O, H, NL, bi, act, dtype="fp32", head_scale=1.0):
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models
    cfg.act_dtype = dtype
    try:
        m = models.SequenceModel(I, O, H, NL, bi, seq, act)
    finally:
        cfg.act_dtype = "fp32"
    fill_state_dict_(m)
    with torch.no_grad():                  # the factor the generator applied so that the head's activation clips (g/meta/head_scale)
        m.fc_output_layer.weight.mul_(head_scale)
        m.fc_output_layer.bias.mul_(head_scale)
    m = m.to("cuda").train()
    m.dropout_keep = 1.0
    return m


def step(m, x, tgt):
    """y = m(x); loss = mean((y - tgt)^2); backward.  Returns (y, loss, dx, {name: grad}) on the CPU."""
    x = x.cuda().requires_grad_(True)
    m.zero_grad()
    y = m(x)
    loss = ((y - tgt.cuda()) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), float(loss.detach()), x.grad.detach().cpu(), {k: p.grad.detach().cpu() for k, p in m.named_parameters()}


def the_plan(m):
    (plan, _), = [v for k, v in m._runtimes.items() if k[0] == "seq"]
    return plan


def lstm_launches(plan):
    return [int((plan.op_kinds(ph)[0] == kind).sum()) for ph, kind in ((0, OP_LSTM_FWD), (1, OP_LSTM_BWD))]


def bf16_record(e):
    vals = list(e["grad"].values())
    worst = max(e["grad"], key=e["grad"].get)
    return dict(y_rel_l2=e["y_l2"], y_rel_max=e["y"], dx_rel_l2=e.get("dx_l2"), loss_rel=e["loss"], grad_rel_l2_median=float(np.median(vals)),
                grad_rel_l2_worst=e["grad"][worst], worst=worst)


def assert_bf16(rec):
    assert rec["y_rel_l2"] < BF16_OUT_L2 and rec["y_rel_max"] < BF16_OUT_MAX and rec["loss_rel"] < BF16_LOSS, rec
    assert rec["grad_rel_l2_median"] < BF16_GRAD_L2 and rec["grad_rel_l2_worst"] < BF16_GRAD_WORST, rec
    assert rec["dx_rel_l2"] < BF16_GRAD_WORST, rec                    # the input gradient is one more gradient tensor


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_step_against_reference_golden(name):
    seq, I, O, H, NL, bi, act, B, T = CASES[name]
    g = load_golden("seqmodel_" + name)
    m = make_model(seq, I, O, H, NL, bi, act, "fp32", float(g["g/meta/head_scale"]))
    y, loss, dx, grads = step(m, torch.from_numpy(g["g/x"]), torch.from_numpy(g["g/tgt"]))
    e = golden_errors(g, y, loss, dx, grads)
    print(name, e)
    assert lstm_launches(the_plan(m)) == [0, 0]
    assert_fp32(e, TOL)


@pytest.mark.parametrize("stepped", [False, True])
@pytest.mark.parametrize("name", ["lstm_h192_l3_bi", "lstm_h256_l2_bi"])
def test_bf16_step_against_reference_golden(name, stepped):
    """stepped=False: every bidirectional layer is ONE launch of the direction-aware cluster kernels per phase; True (knob LSTM_STEPPED): the
    per-frame formulation in bf16.  Same budgets."""
    if stepped:
        knobs.set("LSTM_STEPPED", "1")
    seq, I, O, H, NL, bi, act, B, T = CASES[name]
    g = load_golden("seqmodel_" + name)
    m = make_model(seq, I, O, H, NL, bi, act, "bf16", float(g["g/meta/head_scale"]))
    y, loss, dx, grads = step(m, torch.from_numpy(g["g/x"]), torch.from_numpy(g["g/tgt"]))
    e = golden_errors(g, y, loss, dx, grads)
    e["dx_l2"] = rel_l2(dx, g["g/dx"])
    rec = bf16_record(e)
    print(name, "stepped" if stepped else "cluster", rec)
    plan = the_plan(m)
    assert lstm_launches(plan) == ([0, 0] if stepped else [NL, NL])
    assert plan.status() == 0
    assert_bf16(rec)


BASE = dict(seq="LSTM", I=21, O=5, H=192, NL=2, bi=True, act="Tanh", B=18, T=10)
EDGES = {"T1": dict(T=1), "T2": dict(T=2), "B1": dict(B=1), "I1": dict(I=1), "O1": dict(O=1), "L1_bi": dict(NL=1), "H512": dict(H=512),
         "gru_T1": dict(seq="GRU", T=1, H=64), "uni_B17": dict(bi=False, B=17, NL=3)}
_ref_cache = {}


def edge_reference(edge):
    """torch's own modules in fp64 on the CPU with the same formula weights: computed once per shape, shared by the fp32 and the bf16 test."""
    if edge not in _ref_cache:
        c = dict(BASE, **EDGES[edge])
        gen = torch.Generator().manual_seed(11)
        x = 6 * torch.rand(c["B"], c["I"], c["T"], generator=gen)
        tgt = 2 * torch.rand(c["B"], c["O"], c["T"], generator=gen) - 1
        # the formula weights leave the pre-activations small: the head is scaled, as in the goldens, by the smallest power of two at which the
        # Tanh bends (at least 1 % of the pre-activations beyond +-1, the head_stats rule of tests/golden/make_fsn_knobs_golden.py)
        shapes = torch_shapes(c["seq"], c["I"], c["O"], c["H"], c["NL"], c["bi"])
        for e in range(17):
            scale = float(2 ** e)
            ref = torch_reference(c["seq"], c["I"], c["O"], c["H"], c["NL"], c["bi"], c["act"], formula_params(shapes, scale), x, tgt)
            if float((ref[0].abs() > np.tanh(1.0)).double().mean()) >= 0.01:
                break
        else:
            raise AssertionError(f"{edge}: no head scale up to 2^16 bends the Tanh")
        _ref_cache[edge] = (c, x, tgt, scale, ref)
    return _ref_cache[edge]


def edge_errors(edge, dtype):
    c, x, tgt, scale, (ry, rloss, rdx, rgrads) = edge_reference(edge)
    m = make_model(c["seq"], c["I"], c["O"], c["H"], c["NL"], c["bi"], c["act"], dtype, scale)
    y, loss, dx, grads = step(m, x, tgt)
    e = dict(y=rel_err(y, ry), y_l2=rel_l2(y, ry), dx=rel_err(dx, rdx), dx_l2=rel_l2(dx, rdx), loss=abs(loss - rloss) / abs(rloss),
             norm={k: abs(float(grads[k].double().norm()) - float(v.norm())) / max(float(v.norm()), 1e-30) for k, v in rgrads.items() if float(v.norm()) > 0},
             grad={k: rel_l2(grads[k], v) for k, v in rgrads.items()})
    return c, the_plan(m), e


@pytest.mark.parametrize("edge", list(EDGES))
def test_edge_shapes_fp32(edge):
    c, plan, e = edge_errors(edge, "fp32")
    print(edge, e)
    assert_fp32(e, TOL)


@pytest.mark.parametrize("edge", [k for k in EDGES if dict(BASE, **EDGES[k])["H"] > 128 and dict(BASE, **EDGES[k])["seq"] == "LSTM"])
def test_edge_shapes_bf16_cluster(edge):
    c, plan, e = edge_errors(edge, "bf16")
    rec = bf16_record(e)
    print(edge, rec)
    assert lstm_launches(plan) == [c["NL"], c["NL"]] and plan.status() == 0
    assert_bf16(rec)


def test_bf16_bidirectional_cluster_is_bit_reproducible():
    seq, I, O, H, NL, bi, act, B, T = CASES["lstm_h192_l3_bi"]
    g = load_golden("seqmodel_lstm_h192_l3_bi")
    m = make_model(seq, I, O, H, NL, bi, act, "bf16", float(g["g/meta/head_scale"]))
    x, tgt = torch.from_numpy(g["g/x"]), torch.from_numpy(g["g/tgt"])
    flats, ys = [], []
    for _ in range(3):                                                # the third run: the plan is still usable, no spin budget ran out
        y, loss, dx, grads = step(m, x, tgt)
        flats.append(m._flat_grad.clone())
        ys.append((y, dx))
    plan = the_plan(m)
    assert lstm_launches(plan) == [NL, NL] and plan.status() == 0
    assert float(flats[0].abs().max()) > 0 and torch.equal(flats[0], flats[1]) and torch.equal(flats[0], flats[2])
    assert torch.equal(ys[0][0], ys[1][0]) and torch.equal(ys[0][1], ys[1][1])


@pytest.mark.parametrize("dtype,H", [("fp32", 64), ("bf16", 192)])
def test_training_smoke_with_dropout(dtype, H):
    from sefd_amd.optim import Adam
    m = make_model("LSTM", 21, 5, H, 3, True, None, dtype)
    m.dropout_keep = 0.2
    opt = Adam(m.parameters(), lr=1e-2)
    gen = torch.Generator().manual_seed(2)
    x = (6 * torch.rand(6, 21, 12, generator=gen)).cuda()
    tgt = (1.0 + 0.1 * torch.rand(6, 5, 12, generator=gen)).cuda()
    losses = []
    for _ in range(6):
        m.zero_grad()
        loss = ((m(x) - tgt) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(dtype, losses)
    assert all(np.isfinite(losses)) and min(losses[3:]) < losses[0], losses
    assert the_plan(m).status() == 0


def test_torch_optimizer_through_autograd():
    m = make_model("GRU", 21, 5, 64, 2, True, "ReLU")
    x = (6 * torch.rand(4, 21, 7, generator=torch.Generator().manual_seed(4))).cuda()
    y0 = m(x)                                                         # (flattens the parameters)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    before = m._flat_param.clone()
    (y0 ** 2).mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    opt.step()
    assert not torch.equal(before, m._flat_param)                     # the parameters are views of the flat arena the plan reads
    assert not torch.equal(m(x), y0)


def test_eval_mode_equals_train_mode_without_dropout():
    m = make_model("LSTM", 21, 5, 64, 3, True, "Tanh", head_scale=256.0)
    x = (6 * torch.rand(3, 21, 9, generator=torch.Generator().manual_seed(7))).cuda()
    with torch.no_grad():
        m.train()
        m.dropout_keep = 1.0
        y_train = m(x).clone()
        m.dropout_keep = 0.2
        y_drop = m(x).clone()
        m.eval()
        y_eval = m(x).clone()
    assert float(y_train.abs().max()) > 0 and torch.equal(y_train, y_eval) and not torch.equal(y_drop, y_train)
    assert tuple(y_eval.shape) == (3, 5, 9)


def test_cpu_tensor_is_rejected_not_silently_computed():
    m = make_model("LSTM", 21, 5, 64, 1, False, None)
    with pytest.raises(RuntimeError, match="cuda"):
        m(torch.zeros(2, 21, 4))


def test_stale_backward_is_refused():
    """A forward of the same shape between a forward and its backward overwrites the activations in the runtime's arena: that backward raises; a
    fresh forward and backward reach the input."""
    m = make_model("LSTM", 5, 3, 16, 1, False, None)
    x = torch.randn(2, 5, 3, generator=torch.Generator().manual_seed(3)).cuda().requires_grad_(True)
    y = m(x)
    m(x)
    with pytest.raises(RuntimeError, match="overwrote the activations"):
        (y ** 2).sum().backward()
    (m(x) ** 2).sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
