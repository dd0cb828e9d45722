"""GPU: the recurrence kernels per launch and at saturated gates (tests/recurrence_cases.py; pinned on the CPU by tests/test_recurrence_cases_cpu.py).

Every launch of SequenceModel plans - cell kernels in fp32 and bf16, GRU, the one-launch bidirectional cluster kernels with their reversed group -
and of DCCRN / CRN / FullSubNet plans, one per recurrence variant, against the host simulator from the same pre-op state, plain and with gate biases
of +-100 on selected units (sigmoid and tanh on an overflowed exp2, backward factors of exactly 0); the frame-count tails of the three-frame
rotation; and SequenceModel modules against the plain fp64 reference with cell states that grow to +-T."""
import json
import re

import pytest
import torch

import recurrence_cases as rc
import test_gpu_model as gm
from oracle.dccrn import dccrn_state_shapes
from oracle.weights import formula_state_dict
from plan_check import dccrn_config, ops_device_vs_sim, report_path
from plan_configs import BY_NAME, plan_kwargs
from seqmodel_common import assert_fp32, seq_dict
from test_gpu_ops import every_op_against_host_simulator
from test_gpu_seqmodel import assert_bf16, bf16_record, lstm_launches, step, the_plan
from util import knobs

pytestmark = pytest.mark.gpu
assert (rc.TOL, rc.BF16_OUT_L2, rc.BF16_OUT_MAX, rc.BF16_GRAD_L2, rc.BF16_GRAD_WORST, rc.BF16_LOSS) == \
    (gm.TOL, gm.BF16_OUT_L2, gm.BF16_OUT_MAX, gm.BF16_GRAD_L2, gm.BF16_GRAD_WORST, gm.BF16_LOSS)

_report = {}
_LINE = re.compile(r"phase (\d) op +(\d+) (\w+) +tag +-?\d+ elems +(\d+) err/tol ([0-9.einf+-]+)")


def record(key, value):
    _report[key] = value
    with open(report_path("recurrence_edges_gpu.json"), "w") as f:
        json.dump(_report, f, indent=1, sort_keys=True)


def summarise(lines):
    """Worst err/tol of the whole plan and of its recurrence launches, and how many launches of each recurrence kind compared elements."""
    worst, rec_worst, kinds = 0.0, 0.0, {}
    for ln in lines:
        m = _LINE.match(ln)
        assert m, ln
        kind, elems, e = m.group(3), int(m.group(4)), float(m.group(5))
        worst = max(worst, e)
        if kind in ("LSTM_FWD", "LSTM_BWD", "CELL_FWD", "CELL_BWD") and elems > 0:
            kinds[kind] = kinds.get(kind, 0) + 1
            rec_worst = max(rec_worst, e)
    return dict(worst_err_over_tol=worst, recurrence_worst_err_over_tol=rec_worst, recurrence_launches=kinds)


def has_recurrence(fig):
    k = fig["recurrence_launches"]
    return (k.get("LSTM_FWD", 0) > 0 and k.get("LSTM_BWD", 0) > 0) or (k.get("CELL_FWD", 0) > 0 and k.get("CELL_BWD", 0) > 0)


# ------------------------------------------------------------------------------------------------ SequenceModel plans, launch by launch
@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hot"])
@pytest.mark.parametrize("name,kn", rc.GPU_OP_CASES, ids=[n + "".join("-" + k for k, _ in kn) for n, kn in rc.GPU_OP_CASES])
def test_every_launch_of_a_sequence_model_plan_against_host_simulator(name, kn, hot):
    """Bars of plan_check.ops_device_vs_sim; with saturating biases its per-element rule."""
    from simutil import Plan
    c, P, x, tgt = rc.seq_inputs(name, hot)
    for k, v in kn:
        knobs.set(k, v)
    plan = Plan(c["B"], c["T"], model="SequenceModel", seq=seq_dict(c["seq"], c["I"], c["O"], c["H"], c["NL"], c["bi"]), act_dtype=c["dtype"])
    cluster = c["dtype"] == "bf16" and c["seq"] == "LSTM" and c["H"] > 128 and not kn
    assert lstm_launches(plan) == ([c["NL"], c["NL"]] if cluster else [0, 0])
    tag = f"{name}{''.join('_' + k for k, _ in kn)}_{'hot' if hot else 'plain'}"
    lines, bad = ops_device_vs_sim(plan, P, "SequenceModel", c["B"], c["T"], c["dtype"], per_element=hot, report=f"ops_report_seq_{tag}.txt")
    fig = summarise(lines)
    record(f"seq_ops/{tag}", fig)
    assert not bad, "\n".join(bad[:20])
    assert has_recurrence(fig) and ("LSTM_FWD" in fig["recurrence_launches"]) == cluster, fig


# ------------------------------------------------------------------------------------------------ DCCRN / CRN / FullSubNet plans with saturated biases
@pytest.mark.parametrize("i", range(len(rc.GPU_PLAN_ROWS)), ids=[f"{r[0]}-B{r[1]}-{r[2]}-{r[3].split('/')[0]}-{r[4][0]}-{r[5]}-{r[6]}" for r in rc.GPU_PLAN_ROWS])
def test_every_launch_of_a_saturated_plan_against_host_simulator(i):
    row = rc.GPU_PLAN_ROWS[i]
    lines = every_op_against_host_simulator(*row, params=rc.hot_biases, per_element=True, report_prefix=f"ops_report_hot{i:02d}")
    fig = summarise(lines)
    record(f"plan_ops_hot/{i:02d}_{row[0]}_B{row[1]}_{row[2]}_{row[3].split('/')[0]}_{row[5] or row[4][0]}_{row[6]}", fig)
    assert has_recurrence(fig), fig


def test_every_launch_of_the_saturated_real_lstm_plan_against_host_simulator():
    """cfg.lstm = 'real' on the odd-channel configuration (plan_configs 'lstm_real'), bf16."""
    from simutil import Plan
    e = BY_NAME["lstm_real"]
    kw = plan_kwargs(e, "bf16")
    P = rc.hot_biases(formula_state_dict(dccrn_state_shapes(dccrn_config("E", {k: v for k, v in kw.items() if k != "masking_mode"}))))
    assert sum(1 for k in P if "bias_ih_l" in k) == 2
    lines, bad = ops_device_vs_sim(Plan(e.B, e.L, **kw), P, e.model, e.B, e.L, "bf16", per_element=True, report="ops_report_hot_lstm_real_bf16.txt")
    fig = summarise(lines)
    record("plan_ops_hot/lstm_real_bf16", fig)
    assert not bad, "\n".join(bad[:20])
    assert has_recurrence(fig), fig


# ------------------------------------------------------------------------------------------------ frame-count tails
def shortest_clip():
    """The shortest clip the planner accepts for the small DCCRN (it refuses by ValueError)."""
    from simutil import Plan
    for L in range(1, 4000):
        try:
            Plan(2, L, masking_mode="E", kernel_num=rc.SMALL_KN, rnn_units=128)
            return L
        except ValueError:
            continue
    raise AssertionError("the planner accepts no clip below 4000 samples")


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hot"])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frame_count_tails_of_the_persistent_recurrences(dtype, k, hot):
    """Three clip lengths 100 samples (one hop) apart from the shortest one on: T mod 3 takes all three values, so the three-frame rotation of
    lstm_bf16.hip and the fp32 kernel's loop end in each of their tails."""
    from simutil import Plan
    L0 = shortest_clip()
    Ts = [Plan(2, L0 + 100 * j, masking_mode="E", kernel_num=rc.SMALL_KN, rnn_units=128).T for j in range(3)]
    assert sorted(t % 3 for t in Ts) == [0, 1, 2], Ts
    L = L0 + 100 * k
    lines = every_op_against_host_simulator("DCCRN", 2, L, "E", rc.SMALL_KN, 128, dtype, params=rc.hot_biases if hot else None, per_element=hot,
                                            report_prefix=f"ops_report_tail_{'hot' if hot else 'plain'}")
    fig = summarise(lines)
    fig["T"] = Ts[k]
    record(f"tails/{dtype}_L{L}_{'hot' if hot else 'plain'}", fig)
    assert fig["recurrence_launches"].get("LSTM_FWD", 0) > 0 and fig["recurrence_launches"].get("LSTM_BWD", 0) > 0, fig


# ------------------------------------------------------------------------------------------------ modules against fp64
def make_model(c, P):
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models
    cfg.act_dtype = c["dtype"]
    try:
        m = models.SequenceModel(c["I"], c["O"], c["H"], c["NL"], c["bi"], c["seq"], c["act"])
    finally:
        cfg.act_dtype = "fp32"
    m.load_state_dict({k: v.clone() for k, v in P.items()})
    m = m.to("cuda").train()
    m.dropout_keep = 1.0
    return m


@pytest.mark.parametrize("name", rc.GPU_MODULE_CASES)
def test_module_step_against_fp64_with_growing_cell_state(name):
    """accumulate=True: beside the saturated gates, units whose cell state is +-t, so tanh(c) saturates as the frames go by (T = 67: beyond 45).
    fp32 at TOL, bf16 at the project's bf16 budgets (test_gpu_seqmodel.assert_bf16)."""
    c, P, x, tgt = rc.seq_inputs(name, True, accumulate=True)
    ref = rc.seq_reference(name, True, accumulate=True)
    assert c["seq"] != "LSTM" or ref["cmax"] >= min(45.0, c["T"] - 1e-6)
    m = make_model(c, P)
    y, loss, dx, grads = step(m, x, tgt)
    assert rc.all_finite(y, loss, dx, grads), name
    assert set(grads) == set(ref["grads"])
    e = rc.errors_against(ref, y, loss, dx, grads)
    plan = the_plan(m)
    assert plan.status() == 0
    fig = dict(y=e["y"], y_l2=e["y_l2"], dx=e["dx"], dx_l2=e["dx_l2"], loss=e["loss"], grad_worst=max(e["grad"].values()),
               grad_worst_tensor=max(e["grad"], key=e["grad"].get), cmax=ref["cmax"])
    if c["dtype"] == "bf16":
        emu = rc.emulation_errors(name, True, accumulate=True)
        ratios = {"dx": e["dx_l2"] / emu["dx_l2"], **{k: v / emu["grad"][k] for k, v in e["grad"].items()}}
        fig.update(emu_dx_l2=emu["dx_l2"], emu_grad_worst=max(emu["grad"].values()), ratio_min=min(ratios.values()), ratio_max=max(ratios.values()))
    record(f"module/{name}", fig)
    print(name, fig)
    if c["dtype"] == "fp32":
        assert lstm_launches(plan) == [0, 0]
        assert_fp32(e, rc.TOL)
    else:
        assert lstm_launches(plan) == [c["NL"], c["NL"]]
        assert_bf16(bf16_record(e))
