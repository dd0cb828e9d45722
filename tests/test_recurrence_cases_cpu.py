"""CPU: the recurrences at saturated gates and per direction (tests/recurrence_cases.py).  The plain fp64 reference is held to torch's own modules;
the conditions that make a saturated case a test are asserted from the reference alone; then the host simulator - fp32 and bf16 SequenceModel
plans, the bidirectional one-launch cluster plans included, plain and with saturating biases - against that reference, and DCCRN / CRN / FullSubNet
plans with saturating biases against their oracles through the checkers of plan_check.py at their existing bars."""
import json

import pytest
import torch

import recurrence_cases as rc
from oracle.weights import formula_state_dict
from plan_check import check_crn_plan_vs_oracle, check_dccrn_plan_vs_oracle, check_fsn_plan_vs_oracle, crn_config, dccrn_config, report_path
from seqmodel_common import assert_fp32, formula_params, seq_dict, torch_reference, torch_shapes
from simutil import Plan
from test_seqmodel_cpu import lstm_ops, sim_step
from util import rel_err

_report = {}


def record(key, value):
    _report[key] = value
    with open(report_path("recurrence_cases_cpu.json"), "w") as f:
        json.dump(_report, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------ the helpers themselves
def test_hot_biases_table():
    H = 32
    P = formula_params(torch_shapes("LSTM", 21, 5, H, 2, True))
    Q = rc.hot_biases(P)
    A = rc.hot_biases(P, offset=50.0, accumulate=True)
    touched = [k for k in P if not torch.equal(P[k], Q[k])]
    assert touched == [k for k in P if "bias_ih_l" in k] and len(touched) == 4 and any(k.endswith("_reverse") for k in touched)
    d = (Q["sequence_model.bias_ih_l1_reverse"] - P["sequence_model.bias_ih_l1_reverse"]).view(4, H)
    want = torch.zeros(4, H)
    for j in range(H):
        q, sgn = {1: (0, 1), 2: (1, 1), 3: (2, -1), 5: (3, -1), 6: (0, -1), 7: (1, -1), 9: (2, 1), 10: (3, 1)}.get(j % 16, (0, 0))
        want[q, j] += 100.0 * sgn
    assert torch.equal(d, want)
    da = (A["sequence_model.bias_ih_l0"] - P["sequence_model.bias_ih_l0"]).view(4, H)
    assert da[:, 11].tolist() == [50.0, 50.0, 50.0, 0.0] and da[:, 12].tolist() == [50.0, 50.0, -50.0, 0.0] and da[:, 27].tolist() == [50.0, 50.0, 50.0, 0.0]
    assert float(d[:, 11].abs().max()) == 0.0 and float(d[:, 0].abs().max()) == 0.0 and float(d[:, 4].abs().max()) == 0.0
    G = formula_params(torch_shapes("GRU", 21, 5, H, 1, False))
    dg = (rc.hot_biases(G, accumulate=True)["sequence_model.bias_ih_l0"] - G["sequence_model.bias_ih_l0"]).view(3, H)
    assert torch.equal(dg, want[:3])                                   # the same residues on r, z, n; no fourth block; accumulate is LSTM only
    assert P["sequence_model.bias_ih_l0"].abs().max() < 0.011          # the argument is not changed


def test_hot_biases_reaches_every_model():
    from oracle.crn import crn_state_shapes
    from oracle.dccrn import dccrn_state_shapes
    from oracle.fullsubnet import FSNConfig, fsn_state_shapes
    for shapes, n in ((dccrn_state_shapes(dccrn_config("E", rc.DCCRN_CPU[0][1])), 4), (dccrn_state_shapes(dccrn_config("E", rc.DCCRN_CPU[1][1])), 2),
                      (crn_state_shapes(crn_config(rc.CRN_CPU[0][1])), 1), (fsn_state_shapes(FSNConfig(fb_hidden=64, sb_hidden=32, sequence_model="GRU")), 4)):
        P = formula_state_dict(shapes)
        Q = rc.hot_biases(P)
        touched = [k for k in P if not torch.equal(P[k], Q[k])]
        assert len(touched) == n and all("bias_ih_l" in k for k in touched), touched
        assert all(abs(abs(float((Q[k] - P[k]).abs().max())) - 100.0) < 1e-5 for k in touched)


@pytest.mark.parametrize("seq,NL,bi,hot", [("LSTM", 2, True, False), ("GRU", 2, True, False), ("LSTM", 3, False, True), ("GRU", 1, True, True), ("LSTM", 1, True, True)])
def test_plain_reference_is_torch(seq, NL, bi, hot):
    I, O, H, B, T = 21, 5, 32, 3, 7
    P = formula_params(torch_shapes(seq, I, O, H, NL, bi), 16.0)
    if hot:
        P = rc.hot_biases(P, accumulate=True)
    gen = torch.Generator().manual_seed(11)
    x, tgt = 6 * torch.rand(B, I, T, generator=gen), 2 * torch.rand(B, O, T, generator=gen) - 1
    ry, rloss, rdx, rgrads = torch_reference(seq, I, O, H, NL, bi, "Tanh", P, x, tgt)
    ref = rc.plain_reference(seq, I, O, H, NL, bi, "Tanh", P, x, tgt)
    e = rc.errors_against(dict(y=ry, loss=rloss, dx=rdx, grads=rgrads), ref["y"], ref["loss"], ref["dx"], ref["grads"])
    worst = max([e["y"], e["dx"], e["loss"]] + list(e["grad"].values()))
    assert worst <= 1e-12 and rc.all_finite(ref["y"], ref["loss"], ref["dx"], ref["grads"]), e
    assert ref["pre"].numel() == T * B * H * NL * (2 if bi else 1) * (4 if seq == "LSTM" else 3)
    if hot and seq == "LSTM":
        assert abs(ref["cmax"] - T) < 1e-9                              # residues 11 / 12: c_t = +-t


def test_bf16_emulation_rounds_what_it_says():
    c, P, x, tgt = rc.seq_inputs("bf16_h256_l2_bi", False)
    emu = rc.seq_reference("bf16_h256_l2_bi", False, bf16=True)
    Pr = {k: (v.to(torch.bfloat16).float() if v.dim() == 2 else v) for k, v in P.items()}
    # the forward of the emulation is the plain reference on rounded weights and inputs, except for the rounding of h: close to it, not equal
    near = rc.plain_reference(c["seq"], c["I"], c["O"], c["H"], c["NL"], c["bi"], c["act"], Pr, x.to(torch.bfloat16).float(), tgt)
    assert 0 < rel_err(emu["y"], near["y"]) < 2e-2
    assert set(emu["grads"]) == set(P) and rc.all_finite(emu["y"], emu["loss"], emu["dx"], emu["grads"])


# ------------------------------------------------------------------------------------------------ conditions on the inputs, from the reference alone
@pytest.mark.parametrize("name", rc.CPU_SIM_CASES)
def test_saturated_inputs_meet_their_conditions(name):
    fig = rc.input_conditions(name, True)
    plain = rc.input_conditions(name, False)
    assert plain["beyond45"] == 0.0                                     # ... and without the offsets nothing comes near: what the suite had so far
    record(f"conditions/{name}", dict(hot=fig, plain=plain))


@pytest.mark.parametrize("name", rc.GPU_MODULE_CASES)
def test_accumulating_inputs_meet_their_conditions(name):
    """The module-level cases of the GPU tier (accumulate=True: cell state +-T), from the reference alone."""
    record(f"conditions_accumulate/{name}", rc.input_conditions(name, True, accumulate=True))


# ------------------------------------------------------------------------------------------------ simulator against fp64
@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hot"])
@pytest.mark.parametrize("name", rc.CPU_SIM_CASES)
def test_host_simulator_against_fp64(name, hot):
    """fp32 plans at TOL (measured 2 .. 3e-7); bf16 plans at the bf16 output budgets and, for dx and every gradient tensor, 8 x the bf16-emulating
    reference's own error on that tensor, never above BF16_GRAD_L2.  Before the simulator walked reversed groups backwards, the bidirectional
    cluster plans measured y 0.34 .. 0.87 (max-norm), dx 0.49 .. 0.79 and a worst gradient tensor of 0.21 .. 1.72 (rel-L2) here; now all of them sit
    within 0.9 .. 1.25 x the emulation's own figures."""
    c, P, x, tgt = rc.seq_inputs(name, hot)
    ref = rc.seq_reference(name, hot)
    plan = Plan(c["B"], c["T"], model="SequenceModel", seq=seq_dict(c["seq"], c["I"], c["O"], c["H"], c["NL"], c["bi"]), act_dtype=c["dtype"])
    y, loss, dx, grads, _ = sim_step(plan, P, x, tgt, c["act"])
    assert rc.all_finite(y, loss, dx, grads)
    e = rc.errors_against(ref, y, loss, dx, grads)
    tag = f"{name}/{'hot' if hot else 'plain'}"
    fig = dict(y=e["y"], y_l2=e["y_l2"], dx_l2=e["dx_l2"], loss=e["loss"], grad_worst=max(e["grad"].values()))
    print(tag, fig)
    if c["dtype"] == "fp32":
        record(f"sim/{tag}", fig)
        assert_fp32(e, rc.TOL)
        return
    cluster = c["H"] > 128
    assert lstm_ops(plan) == ([c["NL"], c["NL"]] if cluster else [0, 0])
    emu = rc.emulation_errors(name, hot)
    ratios = {"dx": e["dx_l2"] / emu["dx_l2"], **{k: v / emu["grad"][k] for k, v in e["grad"].items()}}
    fig.update(emu_dx_l2=emu["dx_l2"], emu_grad_worst=max(emu["grad"].values()), ratio_min=min(ratios.values()), ratio_max=max(ratios.values()),
               ratio_worst_tensor=max(ratios, key=ratios.get))
    record(f"sim/{tag}", fig)
    rc.assert_bf16_against_emulation(e, emu, tag)


# ------------------------------------------------------------------------------------------------ DCCRN / CRN / FullSubNet with saturated biases
@pytest.mark.parametrize("name,kw,B,L", rc.DCCRN_CPU, ids=[c[0] for c in rc.DCCRN_CPU])
def test_dccrn_plan_with_saturated_gates_against_oracle(name, kw, B, L):
    from oracle.dccrn import dccrn_state_shapes
    P = rc.hot_biases(formula_state_dict(dccrn_state_shapes(dccrn_config("E", kw))))
    rep = check_dccrn_plan_vs_oracle("E", "SI-SNR", kw, B, L, params=P)
    record(f"dccrn_hot/{name}", max((v, k) for k, v in rep.items()))


def test_crn_plan_with_saturated_gates_against_oracle():
    from oracle.crn import crn_state_shapes
    name, kw, B, L = rc.CRN_CPU[0]
    P = rc.hot_biases(formula_state_dict(crn_state_shapes(crn_config(kw))))
    rep = check_crn_plan_vs_oracle(kw, B, L, params=P)
    record(f"crn_hot/{name}", max((v, k) for k, v in rep.items()))


@pytest.mark.parametrize("seq,norm", rc.FSN_CPU)
def test_fsn_plan_with_saturated_gates_against_oracle(seq, norm):
    from oracle.fullsubnet import FSNConfig, fsn_state_shapes
    P = rc.hot_biases(formula_state_dict(fsn_state_shapes(FSNConfig(fb_hidden=128, sb_hidden=64, sequence_model=seq, norm_type=norm))))
    rep = check_fsn_plan_vs_oracle(seq, norm, params=P)
    record(f"fsn_hot/{seq}", max((v, k) for k, v in rep.items()))
