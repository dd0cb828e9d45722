"""CPU: NavieComplexLSTM on its own (tools_for_model.py:141-181) - constructor and state_dict, planner (csrc/plan_clstm.cpp: refusals, the path chosen per
size and dtype, the reversed launches) and, on the host simulator, every case of tests/golden/make_clstm_golden.py in fp32 and bf16 against the reference's
golden and against the plain float64 reference of tests/clstm_common.py, at the project's bars.

Every test here fails before this feature: the module had no forward, its bidirectional parameter set was the unidirectional one, and the planner had no
such model."""
import json
import os

import pytest
import torch

import clstm_common as cc
from clstm_common import CASES, TOL
from simutil import ARENA_GRAD, PHASE_BWD, PHASE_FWD, Plan, fill_params, read_params, sim_run
from util import GOLDEN, knobs, load_golden, rel_err

ABI = json.load(open(os.path.join(GOLDEN, "seqmodel_abi.json")))


def module(case):
    import sefd_amd  # noqa: F401
    from sefd_amd import models
    isz, hsz, pdim, bi, _, _ = case
    return models.NavieComplexLSTM(isz, hsz, projection_dim=pdim, bidirectional=bi)


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_is_the_reference(name):
    g = load_golden("clstm_" + name)
    want = [(str(k), tuple(int(v) for v in s if v)) for k, s in zip(g["g/meta/keys"], g["g/meta/shapes"])]
    assert len(want) in (8, 12, 16, 20)
    m = module(CASES[name])
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert want == list(cc.torch_shapes(CASES[name]).items())
    plan = Plan(CASES[name][4], CASES[name][5], model="ComplexLSTM", clstm=cc.clstm_dict(CASES[name]))
    assert [(k, s) for k, (_, s) in plan.params.items()] == want


def test_bidirectional_reference_checkpoint_loads():
    import sefd_amd  # noqa: F401
    from sefd_amd import models, tools_for_model
    assert tools_for_model.NavieComplexLSTM is models.NavieComplexLSTM
    g = load_golden("clstm_bi_h128_proj")
    sd = {str(k): torch.full(tuple(int(v) for v in s if v), 0.5) for k, s in zip(g["g/meta/keys"], g["g/meta/shapes"])}
    assert sum(k.endswith("_reverse") for k in sd) == 8 and sd["r_trans.weight"].shape == (48, 256)
    m = module(CASES["bi_h128_proj"])
    m.load_state_dict(sd)
    assert float(m.imag_lstm.weight_hh_l0_reverse.detach().min()) == 0.5
    # batch_first is accepted and ignored, as in the reference
    assert list(models.NavieComplexLSTM(48, 64, batch_first=True).state_dict()) == list(models.NavieComplexLSTM(48, 64).state_dict())


def test_dccrn_keeps_its_holders():
    import sefd_amd  # noqa: F401
    from sefd_amd import models
    m = models.DCCRN(rnn_units=64)
    assert all(isinstance(l, models.NavieComplexLSTM) and not l.bidirectional for l in m.enhance)
    assert [k for k in m.state_dict() if k.startswith("enhance.0.")] == ["enhance.0." + k for k in cc.torch_shapes((8, 64, None, False, 1, 1))]
    assert all(p._sefd_owner() is m for p in m.parameters())


def test_refusals_name_their_limit():
    ok = dict(input_size=48, hidden_size=64, projection_dim=40, bidirectional=True)
    with pytest.raises(ValueError, match="multiple of 8"):
        Plan(3, 9, model="ComplexLSTM", clstm=dict(ok, hidden_size=40))
    for k in ("input_size", "hidden_size", "projection_dim"):
        with pytest.raises(ValueError, match=f"{k} .* is odd"):
            Plan(3, 9, model="ComplexLSTM", clstm=dict(ok, **{k: ok[k] + 1}))
    for bad in (dict(input_size=0), dict(hidden_size=0), dict(projection_dim=0)):
        with pytest.raises(ValueError, match="at least 1"):
            Plan(3, 9, model="ComplexLSTM", clstm=dict(ok, **bad))
    for B, T in ((0, 9), (3, 0)):
        with pytest.raises(ValueError, match="at least 1"):
            Plan(B, T, model="ComplexLSTM", clstm=ok)
    m = module(CASES["bi_h32"])
    with pytest.raises(TypeError, match="list or tuple of two"):
        m(torch.zeros(9, 3, 48))
    with pytest.raises(RuntimeError, match="cuda"):
        m([torch.zeros(9, 3, 24), torch.zeros(9, 3, 24)])


# (case, dtype) -> the LstmRec launches [(phase, rev_mask, G, t0, t1)] in program order; [] = stepped
PERSISTENT = {("uni_h32_proj", "fp32"), ("uni_h32_proj", "bf16"), ("bi_h32", "fp32"), ("bi_h32", "bf16"), ("bi_h128_proj", "fp32"), ("bi_h128_proj", "bf16"),
              ("bi_h192_proj", "bf16")}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_path_per_plan(name, dtype):
    case = CASES[name]
    s = cc.sizes(case)
    plan = Plan(s["B"], s["T"], model="ComplexLSTM", clstm=cc.clstm_dict(case), act_dtype=dtype)
    got = cc.lstm_launches(plan, ABI)
    if (name, dtype) in PERSISTENT:
        # one launch per direction and phase, the reverse one first with all four groups reversed, never chunked
        dirs = [0xF, 0] if s["D"] == 2 else [0]
        assert got == [(ph, m, 4, 0, 0) for ph in (0, 1) for m in dirs], got
        assert cc.count_ops(plan, PHASE_FWD, cc.OP_CELL_FWD) == 0 and cc.count_ops(plan, PHASE_BWD, cc.OP_CELL_BWD) == 0
    else:
        assert got == []
        assert cc.count_ops(plan, PHASE_FWD, cc.OP_CELL_FWD) == s["D"] * s["T"] and cc.count_ops(plan, PHASE_BWD, cc.OP_CELL_BWD) == s["D"] * s["T"]
    knobs.set("LSTM_STEPPED", "1")
    plan = Plan(s["B"], s["T"], model="ComplexLSTM", clstm=cc.clstm_dict(case), act_dtype=dtype)
    assert cc.lstm_launches(plan, ABI) == [] and cc.count_ops(plan, PHASE_FWD, cc.OP_CELL_FWD) == s["D"] * s["T"]


def sim_step(case, dtype, P, xr, xi, gr, gi):
    """Forward, loss = mean(out_r g_r) + mean(out_i g_i), backward on the host simulator."""
    s = cc.sizes(case)
    plan = Plan(s["B"], s["T"], model="ComplexLSTM", clstm=cc.clstm_dict(case), act_dtype=dtype)
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, P)
    x = cc.to_plan_x(case, xr, xi)
    plan.io(ar, "x", tuple(x.shape)).copy_(x)
    sim_run(plan, PHASE_FWD, ar)
    out_r, out_i = cc.from_plan_y(case, plan, ar)
    n = out_r.numel()
    gy = cc.to_plan_gy(case, gr / n, gi / n)                      # d loss / d out
    plan.io(ar, "grad_y", tuple(gy.shape)).copy_(gy)
    sim_run(plan, PHASE_BWD, ar)
    dxr, dxi = cc.from_plan_gx(case, plan, ar)
    return plan, ar, (out_r, out_i, float(cc.loss_of(out_r, out_i, gr, gi)), dxr, dxi, read_params(plan, ar, ARENA_GRAD))


def check_against_golden_and_fp64(name, dtype):
    case = CASES[name]
    g = load_golden("clstm_" + name)
    assert float(g["g/meta/min_hh_effect"]) >= 0.05 and float(g["g/meta/flip_effect"]) >= 0.05      # the generator's conditions
    xr, xi, gr, gi = cc.inputs(case)
    for k, v in (("xr", xr), ("xi", xi), ("gr", gr), ("gi", gi)):
        assert torch.equal(torch.from_numpy(g["g/" + k]), v), k
    _, _, res = sim_step(case, dtype, cc.formula_params(case), xr, xi, gr, gi)
    eg = cc.golden_errors(g, *res)
    ef = cc.errors(cc.reference(name), *res)
    print(name, dtype, "golden", {k: v for k, v in eg.items() if not isinstance(v, dict)}, "worst grad", max(eg["grad"].values()))
    print(name, dtype, "fp64", {k: v for k, v in ef.items() if not isinstance(v, dict)}, "worst grad", max(ef["grad"].values()))
    if dtype == "fp32":
        cc.assert_fp32(eg)
        cc.assert_fp32(ef)
    else:
        cc.assert_bf16(eg)
        cc.assert_bf16_against_emulation(ef, cc.emulation_errors(name))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_host_simulator_against_golden_and_fp64(name, dtype):
    check_against_golden_and_fp64(name, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["bi_h32", "bi_h128_proj"])
def test_stepped_arm_is_held_to_the_same_numbers(name, dtype):
    knobs.set("LSTM_STEPPED", "1")
    check_against_golden_and_fp64(name, dtype)


def test_reference_restates_the_golden():
    """The plain float64 reference of clstm_common.py against the reference's own float32 results: the two yardsticks agree far below the bars."""
    for name in CASES:
        ref = cc.reference(name)
        e = cc.golden_errors(load_golden("clstm_" + name), ref["out_r"], ref["out_i"], ref["loss"], ref["dxr"], ref["dxi"], ref["grads"])
        cc.assert_fp32(e, 1e-5)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7])
def test_frame_count_tails(T, B, dtype):
    """bi_h32's sizes at the frame counts where the kernels' three-step rotations end differently (T mod 3, T < 3), one and several sequences."""
    case = CASES["bi_h32"][:4] + (B, T)
    P = cc.formula_params(case)
    ins = cc.inputs(case)
    _, _, res = sim_step(case, dtype, P, *ins)
    ref = cc.plain_reference(case, P, *ins)
    e = cc.errors(ref, *res)
    if dtype == "fp32":
        cc.assert_fp32(e)
    else:
        emu = cc.plain_reference(case, P, *ins, bf16=True)
        cc.assert_bf16_against_emulation(e, cc.errors(ref, emu["out_r"], emu["out_i"], emu["loss"], emu["dxr"], emu["dxi"], emu["grads"]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_frame_has_no_direction(dtype):
    """T = 1 with the reverse parameters copied from the forward ones: both directions compute the same hidden state, bit for bit."""
    case = CASES["bi_h32"][:4] + (5, 1)
    P = cc.formula_params(case)
    for k in list(P):
        if k.endswith("_reverse"):
            P[k] = P[k[:-len("_reverse")]].clone()
    plan, ar, res = sim_step(case, dtype, P, *cc.inputs(case))
    hf, hr = plan.view(ar, "h.f"), plan.view(ar, "h.r")
    assert float(hf.float().abs().max()) > 1e-3 and torch.equal(hf, hr)
    H = cc.sizes(case)["H"]
    assert torch.equal(res[0][..., :H], res[0][..., H:]) and torch.equal(res[1][..., :H], res[1][..., H:])
    assert rel_err(res[5]["real_lstm.weight_ih_l0"], res[5]["real_lstm.weight_ih_l0_reverse"]) > 0      # (different upstream gradients per direction)
