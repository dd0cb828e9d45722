"""GPU: NavieComplexLSTM on its own - the module against goldens captured from the real reference (tests/golden/make_clstm_golden.py; pinned on the CPU by
tests/test_clstm_cpu.py), every launch of its plans against the host simulator, the reverse walk of the persistent recurrence kernels bit for bit against
their forward walk, bit reproducibility across the two streams, stacked layers, and the module's modes.  Budgets are the project's own: TOL (fp32) and the
named bf16 budgets of tests/test_gpu_model.py (restated in tests/recurrence_cases.py)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import clstm_common as cc
from clstm_common import CASES, TOL
from plan_check import ops_device_vs_sim, report_path
from recurrence_cases import hot_biases
from simutil import PHASE_BWD, PHASE_FWD, Plan, fill_params, sim_run
from util import GOLDEN, knobs, load_golden

pytestmark = pytest.mark.gpu
ABI = json.load(open(os.path.join(GOLDEN, "seqmodel_abi.json")))


def make_module(case, dtype="fp32", P=None):
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models
    isz, hsz, pdim, bi, _, _ = case
    cfg.act_dtype = dtype
    try:
        m = models.NavieComplexLSTM(isz, hsz, projection_dim=pdim, bidirectional=bi)
    finally:
        cfg.act_dtype = "fp32"
    m.load_state_dict(cc.formula_params(case) if P is None else P)
    return m.to("cuda").train()


def step(m, xr, xi, gr, gi):
    """[out_r, out_i] = m([xr, xi]); loss = mean(out_r g_r) + mean(out_i g_i); backward.  Returns (out_r, out_i, loss, dxr, dxi, {name: grad}) on the CPU."""
    xr, xi = xr.cuda().requires_grad_(True), xi.cuda().requires_grad_(True)
    m.zero_grad()
    out_r, out_i = m([xr, xi])
    loss = cc.loss_of(out_r, out_i, gr.cuda(), gi.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return (out_r.detach().cpu(), out_i.detach().cpu(), float(loss.detach()), xr.grad.detach().cpu(), xi.grad.detach().cpu(),
            {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()})


def the_plan(m):
    (plan, _), = [v for k, v in m._runtimes.items() if k[0] == "clstm"]
    return plan


_report = {}


# ------------------------------------------------------------------------------------------------ 1. the module against the reference's golden
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_module_against_reference_golden(name, dtype):
    case = CASES[name]
    g = load_golden("clstm_" + name)
    m = make_module(case, dtype)
    res = step(m, *(torch.from_numpy(g["g/" + k]) for k in ("xr", "xi", "gr", "gi")))
    e = cc.golden_errors(g, *res)
    _report[f"{name}/{dtype}"] = e
    with open(report_path("clstm_gpu.json"), "w") as f:
        json.dump(_report, f, indent=1)
    print(name, dtype, {k: v for k, v in e.items() if not isinstance(v, dict)}, "worst grad l2", max(e["grad"].values()), max(e["grad"], key=e["grad"].get))
    assert the_plan(m).status() == 0
    assert all(bool(torch.isfinite(v).all()) for v in res[5].values())
    if dtype == "fp32":
        cc.assert_fp32(e)
    else:
        cc.assert_bf16(e)


# ------------------------------------------------------------------------------------------------ 2. every launch against the host simulator
@pytest.mark.parametrize("hot", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["bi_h32", "bi_h128_proj", "bi_h192_proj"])
def test_every_launch_against_host_simulator(name, dtype, hot):
    """plan_check.ops_device_vs_sim with the plan's own inputs (x, grad_y): every op of both phases on the device and on the host simulator from the
    SAME pre-op state, under the bars of tests/opcheck.py - buffers relative to the largest element of the buffer, every parameter gradient relative
    to the largest element of that tensor; hot: its per-element rule - and its stray-write detection."""
    case = CASES[name]
    s = cc.sizes(case)
    P = cc.formula_params(case)
    if hot:
        P = hot_biases(P)
        assert float((P["real_lstm.bias_ih_l0_reverse"] - cc.formula_params(case)["real_lstm.bias_ih_l0_reverse"]).abs().max()) == 100.0
    xr, xi, gr, gi = cc.inputs(case)
    n = s["T"] * s["B"] * s["O"]
    plan = Plan(s["B"], s["T"], model="ComplexLSTM", clstm=cc.clstm_dict(case), act_dtype=dtype)
    x, gy = cc.to_plan_x(case, xr, xi), cc.to_plan_gy(case, gr / n, gi / n)

    def seed(plan, dev):
        plan.io(dev, "x", tuple(x.shape)).copy_(x)
        plan.io(dev, "grad_y", tuple(gy.shape)).copy_(gy)
    lines, bad = ops_device_vs_sim(plan, P, "ComplexLSTM", s["B"], s["T"], dtype, per_element=hot, seed=seed,
                                   report=f"clstm_ops_{name}_{dtype}{'_hot' if hot else ''}.txt")
    assert not bad, "\n".join(bad)
    assert plan.status() == 0
    compared = lambda kind: [int(re.search(r"elems\s+(\d+)", l).group(1)) for l in lines if f" {kind} " in l]
    if dtype == "bf16" or s["H"] <= 128:       # persistent or cluster kernels: one launch per direction and phase, each compared
        assert len(compared("LSTM_FWD")) == 2 and len(compared("LSTM_BWD")) == 2 and min(compared("LSTM_FWD") + compared("LSTM_BWD")) > 0
        masks = [mk for _, mk, _, _, _ in cc.lstm_launches(plan, ABI)]
        assert masks == [0xF, 0, 0xF, 0]
    else:                                      # stepped: a cell launch per direction and frame
        assert len(compared("CELL_FWD")) == 2 * s["T"] and len(compared("CELL_BWD")) == 2 * s["T"] and min(compared("CELL_FWD") + compared("CELL_BWD")) > 0


# ------------------------------------------------------------------------------------------------ 3. the reverse walk itself
def mirrored_params(case):
    P = cc.formula_params(case)
    for k in list(P):
        if k.endswith("_reverse"):
            P[k] = P[k[:-len("_reverse")]].clone()
    return P


@pytest.mark.parametrize("dtype,H,rpw", [("bf16", 32, 4), ("bf16", 32, 16), ("bf16", 64, 4), ("bf16", 64, 16), ("bf16", 96, 4), ("bf16", 96, 16),
                                         ("bf16", 128, 4), ("bf16", 128, 16), ("fp32", 48, 0), ("fp32", 128, 0)])
def test_reverse_walk_is_the_forward_walk_on_flipped_time(dtype, H, rpw):
    """A bidirectional layer without projection whose `_reverse` tensors are copies of the forward ones.  Run A: inputs x, upstream gradient g.  Run B:
    inputs flip_t(x), upstream gradient with the halves of g swapped and flipped in time.  Then the reverse direction of A is the forward direction of B
    on the same numbers in the same order, so, BIT FOR BIT: the reverse half of each output of A is the time-flip of the forward half of B's, the saved
    hidden sequences and the gate gradients of the two recurrences are each other's time-flips, and - with the upstream gradient on one direction only
    (the other direction then adds exact zeros) - so are the input gradients.  rpw: LSTM_RPW and LSTM_RPW_BWD (bf16: both variants; fp32 has one)."""
    if rpw:
        knobs.set("LSTM_RPW", str(rpw))
        knobs.set("LSTM_RPW_BWD", str(rpw))
    I = 24
    base = (2 * I, 2 * H, None, True)
    m = make_module(base + (1, 1), dtype, mirrored_params(base + (1, 1)))
    for T in (1, 2, 3, 4, 5, 7, 10):
        for B in (1, 5, 18):
            case = base + (B, T)
            xr, xi, gr, gi = cc.inputs(case)
            gr[..., :H], gi[..., :H] = 0.0, 0.0                      # run A: upstream gradient on the reverse direction only
            swap = lambda g: torch.cat([g[..., H:], g[..., :H]], 2).flip(0)
            runs = []
            for ins in ((xr, xi, gr, gi), (xr.flip(0), xi.flip(0), swap(gr), swap(gi))):
                res = step(m, *ins)
                (plan, ar), = [v for k, v in m._runtimes.items() if k[:3] == ("clstm", B, T)]
                assert plan.status() == 0
                assert [mk for _, mk, _, _, _ in cc.lstm_launches(plan, ABI)] == [0xF, 0, 0xF, 0]
                bufs = {k: plan.view(ar, k).clone().cpu() for k in ("h.f", "h.r", "dgates.f", "dgates.r")}
                runs.append((res, bufs))
            (ra, ba), (rb, bb) = runs
            tag = (dtype, H, rpw, T, B)
            flip_h = lambda v: v.view(4, B, T, H).flip(2)
            flip_g = lambda v: v.view(2, B, T, 8 * H).flip(2)
            assert float(ba["h.r"].float().abs().max()) > 1e-3 and float(ba["dgates.r"].float().abs().max()) > 0, tag
            assert torch.equal(ba["h.r"].view(4, B, T, H), flip_h(bb["h.f"])), ("h", tag)
            assert torch.equal(ba["h.f"].view(4, B, T, H), flip_h(bb["h.r"])), ("h (forward of A = reverse of B)", tag)
            assert torch.equal(ba["dgates.r"].view(2, B, T, 8 * H), flip_g(bb["dgates.f"])), ("dgates", tag)
            for k in (0, 1):                                       # out_r, out_i
                assert torch.equal(ra[k][..., H:], rb[k][..., :H].flip(0)), ("output", k, tag)
                assert torch.equal(ra[k][..., :H], rb[k][..., H:].flip(0)), ("output (forward of A = reverse of B)", k, tag)
            for k in (3, 4):                                       # dxr, dxi
                assert float(ra[k].abs().max()) > 0 and torch.equal(ra[k], rb[k].flip(0)), ("input gradient", k, tag)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_launchers_refuse_a_chunked_reversed_launch(dtype):
    """A reversed group resumes from no saved state.  The planner never chunks one; a descriptor that is (t1 written into the plan's op list here) is not
    launched: the buffers stay untouched, the plan's status word is raised and the next run refuses, as the cluster launcher does."""
    import ctypes as C
    case = CASES["bi_h32"]
    s = cc.sizes(case)
    plan = Plan(s["B"], s["T"], model="ComplexLSTM", clstm=cc.clstm_dict(case), act_dtype=dtype)
    ar = plan.alloc_arenas("cuda")
    fill_params(plan, ar, cc.formula_params(case))
    x = cc.to_plan_x(case, *cc.inputs(case)[:2])
    plan.io(ar, "x", tuple(x.shape)).copy_(x)
    sz, u, off = ABI["sefd_op_size"] // 4, ABI["op_union_offset"], ABI["lstm_rec_offsets"]
    n = plan.num_ops(PHASE_FWD)
    raw = np.ctypeslib.as_array((C.c_int32 * (n * sz)).from_address(plan.ops_ptr(PHASE_FWD))).reshape(n, sz)
    rev, = [i for i in range(n) if raw[i, 0] == cc.OP_LSTM_FWD and raw[i, (u + off["rev_mask"]) // 4] == 0xF]
    plan.run(PHASE_FWD, ar, 0, 0, rev)                              # everything in front of the reverse recurrence
    raw[rev, (u + off["t1"]) // 4] = 5
    try:
        plan.run(PHASE_FWD, ar, 0, rev, rev + 1)
        torch.cuda.synchronize()
        assert plan.status() == 1
        assert float(plan.view(ar, "h.r").float().abs().max()) == 0.0 and float(plan.view(ar, "c.r").abs().max()) == 0.0
        with pytest.raises(RuntimeError, match="sefd_plan_run failed"):
            plan.run(PHASE_FWD, ar, 0, rev, rev + 1)
    finally:
        raw[rev, (u + off["t1"]) // 4] = 0
    assert plan.status(clear=True) == 1
    plan.run(PHASE_FWD, ar, 0, rev, rev + 1)                        # the planner's own descriptor runs
    torch.cuda.synchronize()
    assert plan.status() == 0 and float(plan.view(ar, "h.r").float().abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 4. bit reproducibility
def test_two_streams_are_bit_reproducible():
    """Forward + backward of bi_h128_proj in bf16, four times (the later ones replay the captured graph where that is on): identical bytes.  The two
    directions run on different streams; a missing join would show as a race."""
    case = CASES["bi_h128_proj"]
    m = make_module(case, "bf16")
    ins = cc.inputs(case)
    first = step(m, *ins)
    assert float(first[0].abs().max()) > 1e-3
    for _ in range(3):
        again = step(m, *ins)
        for a, b in zip(first[:2] + first[3:5], again[:2] + again[3:5]):
            assert torch.equal(a, b)
        assert first[2] == again[2]
        for k, v in first[5].items():
            assert torch.equal(v, again[5][k]), k
    assert the_plan(m).status() == 0


# ------------------------------------------------------------------------------------------------ 5. stacked layers
def test_stacked_layers_against_fp64():
    """nn.Sequential of two layers, as DCCRN stacks them (lists pass through), against the plain float64 reference; gradients reach the first layer's
    parameters and the inputs."""
    c0, c1 = (48, 64, None, False, 3, 9), (64, 64, 48, False, 3, 9)
    P0, P1 = cc.formula_params(c0), cc.formula_params(c1)
    net = torch.nn.Sequential(make_module(c0, "fp32", P0), make_module(c1, "fp32", P1))
    xr, xi, _, _ = cc.inputs(c0)
    _, _, gr, gi = cc.inputs(c1)
    out_r, out_i, loss, dxr, dxi, grads = step(net, xr, xi, gr, gi)
    W0 = {k: v.double().requires_grad_(True) for k, v in P0.items()}
    W1 = {k: v.double().requires_grad_(True) for k, v in P1.items()}
    xs = [xr.double().requires_grad_(True), xi.double().requires_grad_(True)]
    ref_r, ref_i = cc.plain_forward(c1, W1, *cc.plain_forward(c0, W0, *xs))
    ref_loss = cc.loss_of(ref_r, ref_i, gr.double(), gi.double())
    names = [("0." + k, W0[k]) for k in W0] + [("1." + k, W1[k]) for k in W1]
    g = torch.autograd.grad(ref_loss, [w for _, w in names] + xs)
    ref = dict(out_r=ref_r.detach(), out_i=ref_i.detach(), loss=float(ref_loss.detach()), loss_scale=cc.loss_scale(ref_r.detach(), ref_i.detach(), gr, gi),
               dxr=g[-2], dxi=g[-1], grads={k: v for (k, _), v in zip(names, g[:-2])})
    assert list(grads) == [k for k, _ in names]
    e = cc.errors(ref, out_r, out_i, loss, dxr, dxi, grads)
    print({k: v for k, v in e.items() if not isinstance(v, dict)}, max(e["grad_max"].values()))
    assert float(grads["0.real_lstm.weight_hh_l0"].abs().max()) > 0 and float(dxr.abs().max()) > 0
    cc.assert_fp32(e, TOL)


# ------------------------------------------------------------------------------------------------ 6. modes
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_no_grad_eval_and_the_stale_activation_guard(dtype):
    case = CASES["bi_h128_proj"]
    m = make_module(case, dtype)
    xr, xi, gr, gi = (t.cuda() for t in cc.inputs(case))
    train = [t.detach().clone() for t in m([xr, xi])]
    with torch.no_grad():
        ng = m([xr, xi])
    assert not ng[0].requires_grad and all(torch.equal(a, b) for a, b in zip(train, ng))
    m.eval()
    ev = m((xr, xi))                                              # a tuple is taken like a list
    assert all(torch.equal(a, b) for a, b in zip(train, ev))
    m.train()
    with pytest.raises(TypeError, match="list or tuple of two"):
        m(torch.cat([xr, xi], 2))
    xg = xr.clone().requires_grad_(True)
    out = m([xg, xi])
    m([xr, xi])                                                   # a second forward of the same shape before the backward
    with pytest.raises(RuntimeError, match="overwrote the activations"):
        cc.loss_of(out[0], out[1], gr, gi).backward()
    out = m([xg, xi])
    cc.loss_of(out[0], out[1], gr, gi).backward()
    assert float(xg.grad.abs().max()) > 0
