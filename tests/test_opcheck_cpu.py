"""CPU: the comparison rule of the per-launch device-against-simulator tests (tests/opcheck.py) sees the faults it exists for.

The host simulator plays both sides.  A fault is planted in the copy that plays the device, after the op that writes the target tensor, and the
comparator's verdict is asserted.  The targets are the tensors the rule before the per-tensor split could not see: a parameter gradient whose largest
element lies below 1e-3 (the bar) of the largest gradient of the model.  Each plan first prints and asserts that precondition; for the dropped, scaled
and one-element faults the old arena-wide figure is computed as well and asserted to lie BELOW the old bar - the reason this file exists."""
import functools
import math

import pytest
import torch

import opcheck
from opcheck import GRAD, STATE, Table, compare_op
from simutil import PHASE_BWD, PHASE_FWD, Plan, fill_params, sim_run

SMALL_KN = (16, 32, 32, 64, 64, 64)
CHECK = (0, 2, 3, 5)                            # workspace, gradients, state, io: the arenas an op may write
BAR = 1e-3
OP_WGRAD = 2                                    # sefd_desc.h OpKind


def _dccrn(dtype):
    from oracle.dccrn import DCCRNConfig, dccrn_state_shapes
    from oracle.weights import formula_state_dict
    from plan_check import seed_inputs
    P = formula_state_dict(dccrn_state_shapes(DCCRNConfig(masking_mode="E", kernel_num=SMALL_KN, rnn_units=128)))
    B = 1
    for L in range(400, 4001, 100):             # the shortest clip the planner accepts (it refuses by ValueError)
        try:
            plan = Plan(B, L, masking_mode="E", kernel_num=SMALL_KN, rnn_units=128, act_dtype=dtype)
            break
        except ValueError:
            continue
    return plan, P, dtype, lambda plan, ar: seed_inputs(plan, ar, P, "DCCRN", B, L)


def _fsn():
    from oracle.fullsubnet import FSNConfig, fsn_state_shapes
    from oracle.weights import formula_state_dict
    from plan_check import seed_inputs
    P = formula_state_dict(fsn_state_shapes(FSNConfig(fb_hidden=64, sb_hidden=32)))
    plan = Plan(2, 8, model="FullSubNet", fsn=dict(fb_hidden=64, sb_hidden=32, keep=0.2))
    return plan, P, "fp32", lambda plan, ar: seed_inputs(plan, ar, P, "FullSubNet", 2, 8)


def _seq():
    from plan_check import seed_inputs
    from seqmodel_common import formula_params, seq_dict, torch_shapes
    shape = ("LSTM", 21, 5, 64, 2, True)
    P = formula_params(torch_shapes(*shape))
    plan = Plan(3, 9, model="SequenceModel", seq=seq_dict(*shape), act_dtype="fp32")
    return plan, P, "fp32", lambda plan, ar: seed_inputs(plan, ar, P, "SequenceModel", 3, 9)


def _clstm():
    import clstm_common as cc
    case = cc.CASES["bi_h32"]
    s = cc.sizes(case)
    xr, xi, gr, gi = cc.inputs(case)
    n = s["T"] * s["B"] * s["O"]
    x, gy = cc.to_plan_x(case, xr, xi), cc.to_plan_gy(case, gr / n, gi / n)
    plan = Plan(s["B"], s["T"], model="ComplexLSTM", clstm=cc.clstm_dict(case), act_dtype="fp32")

    def seed(plan, ar):
        plan.io(ar, "x", tuple(x.shape)).copy_(x)
        plan.io(ar, "grad_y", tuple(gy.shape)).copy_(gy)
    return plan, cc.formula_params(case), "fp32", seed


BUILD = {"dccrn_fp32": lambda: _dccrn("fp32"), "dccrn_bf16": lambda: _dccrn("bf16"), "fsn_64_32": _fsn, "seqmodel": _seq, "clstm": _clstm}
# The plans in which at least one trainable tensor's largest gradient lies below 1e-3 of the arena's (measured here, asserted by
# test_precondition): the others have no tensor the old rule could not see and serve the no-fault and stray cases only.
GAP_PLANS = ("dccrn_fp32", "dccrn_bf16", "fsn_64_32")
STATE_PLANS = ("dccrn_fp32", "dccrn_bf16")


def _fresh(plan, P, seed):
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, P)
    seed(plan, ar)
    return ar


def _excepted(name):
    return name.endswith("conv.bias") or name.endswith(".2.weight")


@functools.lru_cache(maxsize=None)
def walk(name):
    """Pass 1: both phases at once, for the final gradients and the targets.  Pass 2: op by op on two copies (simulator, "device"), the verdict on
    every op, and the arenas around the ops that the fault cases need."""
    plan, P, dtype, seed = BUILD[name]()
    table = opcheck.region_table(plan)
    ar = _fresh(plan, P, seed)
    sim_run(plan, PHASE_FWD, ar)
    sim_run(plan, PHASE_BWD, ar)
    grad, state = ar[GRAD].clone(), ar[STATE].clone()
    amax = float(grad.abs().max())
    ratios = sorted((float(grad[off:off + n].abs().max()) / amax, k) for k, off, n in table.tensors[GRAD])
    smax = float(state.abs().max()) if table.tensors[STATE] else 0.0
    sratios = sorted((float(state[off:off + n].abs().max()) / smax, k) for k, off, n in table.tensors[STATE] if k.endswith("running_mean"))
    res = dict(plan=plan, P=P, seed=seed, dtype=dtype, table=table, ratios=ratios, sratios=sratios, amax=amax, final_grad=grad, verdicts=[], snaps={})
    below = [(r, k) for r, k in ratios if 0.0 < r < BAR and not _excepted(k)]
    res["target"] = below[0][1] if below else None
    below2d = [(r, k) for r, k in below if len(plan.params[k][1]) >= 2]
    res["target2d"] = below2d[0][1] if below2d else None
    res["state_target"] = sratios[0][1] if sratios else None
    index = {a: {k: (off, n) for k, off, n in table.tensors[a]} for a in (GRAD, STATE)}
    watch = [(key, a, index[a][res[key]]) for key, a in (("target", GRAD), ("target2d", GRAD), ("state_target", STATE)) if res[key]]

    sim = _fresh(plan, P, seed)
    dev = [a.clone() for a in sim]
    for phase in (PHASE_FWD, PHASE_BWD):
        kinds, _ = plan.op_kinds(phase)
        for i in range(plan.num_ops(phase)):
            prev = {a: sim[a].clone() for a in CHECK}
            sim_run(plan, phase, sim, i, i + 1)
            sim_run(plan, phase, dev, i, i + 1)
            kind = int(kinds[i])
            res["verdicts"].append((phase, i, kind, compare_op(prev, sim, dev, table, kind, dtype)))
            snap = None
            for r in res["verdicts"][-1][3].rows:                                # the WGRAD launch with the smallest partial sums
                if kind == OP_WGRAD and r[0].startswith("gradpart+") and 0 < r[1] < res["snaps"].get("partials", dict(own=float("inf")))["own"]:
                    snap = dict(prev=prev, post={b: sim[b].clone() for b in CHECK}, kind=kind, op=(phase, i), own=r[1], row=r[0])
                    res["snaps"]["partials"] = snap
            for key, a, (off, n) in watch:                                       # the LAST op that writes the tensor: its value is then final
                if not torch.equal(sim[a][off:off + n], prev[a][off:off + n]):
                    snap = snap or dict(prev=prev, post={b: sim[b].clone() for b in CHECK}, kind=kind, op=(phase, i))
                    res["snaps"][key] = snap
            if dtype == "bf16" and "bf16" not in res["snaps"] and kind in (opcheck.OP_RUNGEMM, 6):      # an activation: a GEMM's or BN_APPLY's output
                for a, off, nb, dt, rname in table.regions:
                    if dt != opcheck.BF16 or nb <= 0:
                        continue
                    h8 = sim[a].view(torch.uint8)[off:off + nb]
                    if torch.equal(h8, prev[a].view(torch.uint8)[off:off + nb]):
                        continue
                    m = float(h8.view(torch.bfloat16).float().abs().max())
                    # four bf16 ulps of the largest element m are 4 * 2^-8 / (mantissa of m) of it: above the 1.6e-2 bar for a mantissa below 1.95
                    if m > 0 and 2 * math.frexp(m)[0] < 1.9:
                        res["snaps"]["bf16"] = dict(prev=prev, post={b: sim[b].clone() for b in CHECK}, kind=kind, op=(phase, i), region=(a, off, nb, rname), max=m)
                        break
            for a in CHECK:                                                      # as the GPU driver does: both sides go on from the device's state
                sim[a].copy_(dev[a])
    return res


def _faulted(snap):
    return {a: t.clone() for a, t in snap["post"].items()}


def _verdict(w, snap, dev, per_element=False):
    return compare_op(snap["prev"], snap["post"], dev, w["table"], snap["kind"], w["dtype"], per_element)


def _slice(w, arena, key):
    off, shape = (w["plan"].params if arena == GRAD else w["plan"].state)[key]
    n = 1
    for d in shape:
        n *= d
    return off, n, shape


def _old_rule(snap, dev, w):
    """(err, tol) of the rule before the split: the whole gradient arena relative to its largest element."""
    return opcheck.arena_max_error(snap["post"][GRAD], dev[GRAD]), opcheck.tolerance(0, "A_GRAD", snap["kind"], w["dtype"])


# ------------------------------------------------------------------------------------------------ the plans
@pytest.mark.parametrize("name", list(BUILD))
def test_precondition(name):
    w = walk(name)
    print(name, "largest gradient", w["amax"], "target", w["target"], "2-D target", w["target2d"], "state target", w["state_target"])
    for r, k in w["ratios"]:
        if r < 10 * BAR:
            print(f"   {r:.2e} {k}")
    for r, k in w["sratios"][:4]:
        print(f"   state {r:.2e} {k}")
    assert (w["target"] is not None) == (name in GAP_PLANS), w["ratios"][:8]
    if name in GAP_PLANS:
        assert w["target2d"] is not None and set(w["snaps"]) >= {"target", "target2d"}
        for key in ("target", "target2d"):                                       # the snapshot holds the final gradient of the target
            off, n, _ = _slice(w, GRAD, w[key])
            assert torch.equal(w["snaps"][key]["post"][GRAD][off:off + n], w["final_grad"][off:off + n])
    assert (w["state_target"] is not None) == (name in STATE_PLANS)


@pytest.mark.parametrize("name", list(BUILD))
def test_no_fault_every_op_of_both_phases(name):
    w = walk(name)
    plan = w["plan"]
    assert len(w["verdicts"]) == plan.num_ops(PHASE_FWD) + plan.num_ops(PHASE_BWD)
    misses = [(ph, i, kind, v.where) for ph, i, kind, v in w["verdicts"] if not (v.worst < 1.0)]
    stray = [(ph, i, kind, v.stray) for ph, i, kind, v in w["verdicts"] if v.stray]
    assert not misses and not stray, (misses, stray)
    seen = {r[0] for _, _, _, v in w["verdicts"] for r in v.rows}
    for k, off, n in w["table"].tensors[GRAD]:                                   # every tensor with a gradient was measured on its own
        assert ("A_GRAD:" + k in seen) == (float(w["final_grad"][off:off + n].abs().max()) > 0), k
    assert sum(v.elems for _, _, _, v in w["verdicts"]) > 0


# ------------------------------------------------------------------------------------------------ faults in a gradient tensor
def _plant(w, key, fault):
    """The arenas of the "device" with `fault(tensor view, pre-op tensor view)` applied to the target's gradient."""
    snap = w["snaps"][key]
    off, n, shape = _slice(w, GRAD, w[key])
    dev = _faulted(snap)
    fault(dev[GRAD][off:off + n], snap["prev"][GRAD][off:off + n], shape)
    return snap, dev


def _dropped(t, before, shape):
    t.copy_(before)


def _scaled(t, before, shape):
    t.mul_(1.01)


def _one_element(t, before, shape):
    t[t.numel() // 2] += 0.01 * float(t.abs().max())


def _last_row(t, before, shape):
    t.view(shape[0], -1)[-1].zero_()


def _last_column(t, before, shape):
    t.view(shape[0], -1)[:, -1].zero_()


def _nan(t, before, shape):
    t[t.numel() // 3] = float("nan")


@pytest.mark.parametrize("fault", [_dropped, _scaled, _one_element, _last_row, _last_column, _nan], ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("name", GAP_PLANS)
def test_fault_in_the_smallest_gradient_tensor_is_a_miss(name, fault):
    w = walk(name)
    key = "target2d" if fault in (_last_row, _last_column) else "target"
    snap, dev = _plant(w, key, fault)
    v = _verdict(w, snap, dev)
    old, old_tol = _old_rule(snap, dev, w)
    print(name, fault.__name__, w[key], "op", snap["op"], "per-tensor:", v.where, "err/tol", v.worst, "| arena-wide err", old, "tol", old_tol)
    assert not (v.worst < 1.0) and ("A_GRAD:" + w[key] + " ") in v.where, v
    assert v.stray == 0
    if fault in (_dropped, _scaled, _one_element):
        assert old < old_tol, (old, old_tol)                                    # the arena-wide rule passed this fault


# ------------------------------------------------------------------------------------------------ the launch that computes a small gradient
@pytest.mark.parametrize("fault", ["dropped", "scaled", "stray"])
@pytest.mark.parametrize("name", GAP_PLANS)
def test_fault_in_the_smallest_weight_gradient_launch_is_a_miss(name, fault):
    """The WGRAD launch whose partial sums are the smallest of the plan, inside the buffer that holds every launch's (`gradpart`)."""
    w = walk(name)
    snap = w["snaps"]["partials"]
    a, off, nb, _, _ = next(r for r in w["table"].regions if r[4] == opcheck.PARTIALS)
    view = lambda ar: ar[a].view(torch.uint8)[off:off + nb].view(torch.float32)
    pre, post = view(snap["prev"]), view(snap["post"])
    changed = post.view(torch.int32) != pre.view(torch.int32)
    ratio = snap["own"] / float(post.abs().max())
    print(name, fault, "op", snap["op"], snap["row"], "largest partial sum of the launch", snap["own"], "of the buffer's largest:", ratio)
    assert ratio < BAR
    dev = _faulted(snap)
    if fault == "dropped":
        view(dev)[changed] = pre[changed]
    elif fault == "scaled":
        view(dev)[changed] *= 1.01
    else:
        quiet = int(torch.argmax((~changed).to(torch.uint8)))                   # a partial sum of another launch
        view(dev)[quiet] += 1.0
    v = _verdict(w, snap, dev)
    old = opcheck.arena_max_error(post, view(dev))
    print("   per-launch:", v.where, "err/tol", v.worst, "stray", v.stray, "| buffer-wide err", old)
    if fault == "stray":
        assert 1 <= v.stray <= 4 and v.worst < 1.0
    else:
        assert not (v.worst < 1.0) and v.where.startswith(snap["row"] + " ") and v.stray == 0, v
        assert old < BAR


# ------------------------------------------------------------------------------------------------ state, stray writes
@pytest.mark.parametrize("name", STATE_PLANS)
def test_running_mean_off_by_one_percent_is_a_miss(name):
    w = walk(name)
    snap = w["snaps"]["state_target"]
    off, n, _ = _slice(w, STATE, w["state_target"])
    dev = _faulted(snap)
    dev[STATE][off:off + n].mul_(1.01)
    v = _verdict(w, snap, dev)
    old = opcheck.arena_max_error(snap["post"][STATE], dev[STATE])
    print(name, w["state_target"], w["sratios"][0][0], "per-tensor:", v.where, "| arena-wide err", old)
    assert not (v.worst < 1.0) and ("A_STATE:" + w["state_target"] + " ") in v.where, v
    assert old < BAR


@pytest.mark.parametrize("name", list(BUILD))
def test_one_float_in_a_tensor_the_op_leaves_alone_is_stray(name):
    """One float in a gradient tensor that the op does not write, at the first backward op that writes some gradient tensors and leaves others alone;
    a plan whose gradients all leave in ONE op: at the op in front of it, which writes none (the arena as a whole is then untouched)."""
    w = walk(name)
    plan, table = w["plan"], w["table"]
    sim = _fresh(plan, w["P"], w["seed"])
    sim_run(plan, PHASE_FWD, sim)
    kinds, _ = plan.op_kinds(PHASE_BWD)
    written = {i: sum(1 for r in v.rows if r[0].startswith("A_GRAD:")) for ph, i, kind, v in w["verdicts"] if ph == PHASE_BWD}
    some = [i for i, c in written.items() if 0 < c < len(table.tensors[GRAD])]
    last = some[0] if some else min(i for i, c in written.items() if c) - 1
    sim_run(plan, PHASE_BWD, sim, 0, last)
    prev = {a: sim[a].clone() for a in CHECK}
    sim_run(plan, PHASE_BWD, sim, last, last + 1)
    quiet = [(k, off, n) for k, off, n in table.tensors[GRAD] if torch.equal(sim[GRAD][off:off + n], prev[GRAD][off:off + n])]
    assert len(quiet) == len(table.tensors[GRAD]) - written[last] and quiet
    k, off, n = quiet[0]
    dev = {a: sim[a].clone() for a in CHECK}
    dev[GRAD][off + n - 1] += 1.0
    v = compare_op(prev, sim, dev, table, int(kinds[last]), w["dtype"])
    print(name, "op", last, "stray float in", k, v)
    assert 1 <= v.stray <= 4 and v.worst < 1.0


# ------------------------------------------------------------------------------------------------ bf16 activations: the existing bar keeps its meaning
def test_bf16_activation_one_ulp_passes_four_ulps_of_the_maximum_miss():
    w = walk("dccrn_bf16")
    snap = w["snaps"]["bf16"]
    a, off, nb, rname = snap["region"]
    ulp = 2.0 ** (math.frexp(snap["max"])[1] - 8)                               # bf16: 8 significant bits
    post = snap["post"][a].view(torch.uint8)[off:off + nb].view(torch.bfloat16)
    at = int(post.float().abs().argmax())
    sign = 1.0 if float(post[at]) > 0 else -1.0
    for ulps, miss in ((1, False), (4, True)):
        dev = _faulted(snap)
        t = dev[a].view(torch.uint8)[off:off + nb].view(torch.bfloat16)
        t[at] = float(post[at]) + sign * ulps * ulp
        assert abs(float(t[at]) - float(post[at])) == ulps * ulp                # representable: the move is exactly that many ulps
        v = _verdict(w, snap, dev)
        print(rname, "max", snap["max"], "ulps", ulps, v.where, "err/tol", v.worst)
        assert v.stray == 0 and (not (v.worst < 1.0)) == miss, v
        assert rname + " " in v.where


# ------------------------------------------------------------------------------------------------ the rule on a hand-made table
def _toy(grad_tensors, state_tensors=(), nfloat=16):
    table = Table(opcheck.arena_regions(4 * nfloat, 4 * nfloat), {GRAD: list(grad_tensors), STATE: list(state_tensors)})
    return table, {GRAD: torch.zeros(nfloat), STATE: torch.zeros(nfloat)}


def _clone(ar):
    return {a: t.clone() for a, t in ar.items()}


def test_padding_between_tensors_is_checked_like_an_untouched_tensor():
    table, prev = _toy([("a", 0, 4), ("b", 8, 4)])
    sim = _clone(prev)
    sim[GRAD][0:4] = torch.tensor([1.0, 2.0, 3.0, 4.0])
    for where in (5, 9, 14):                                                    # between a and b, in b (untouched), behind the last tensor
        dev = _clone(sim)
        dev[GRAD][where] = 1e-30
        v = compare_op(prev, sim, dev, table, 4, "fp32")
        assert v.stray > 0 and v.worst == 0.0, (where, v)
    v = compare_op(prev, sim, _clone(sim), table, 4, "fp32")
    assert v.stray == 0 and v.worst == 0.0 and v.elems == 4 and [r[0] for r in v.rows] == ["A_GRAD:a"]


def test_a_launch_the_device_dropped_errs_by_one():
    table, prev = _toy([("a", 0, 4), ("b", 4, 4)])
    prev[GRAD][4:8] = 1e3                                                       # a neighbour a million times larger
    sim = _clone(prev)
    sim[GRAD][0:4] = 1e-3
    v = compare_op(prev, sim, _clone(prev), table, 2, "fp32")
    assert abs(v.worst - 1.0 / 1e-3) < 1e-6 and v.where.startswith("A_GRAD:a ") and v.stray == 0
    assert opcheck.arena_max_error(sim[GRAD], prev[GRAD]) < 1e-3


def test_named_exceptions_widen_to_the_same_layer_only():
    names = ["encoder.0.0.real_conv.weight", "encoder.0.0.real_conv.bias", "encoder.0.1.weight", "encoder.0.2.weight", "decoder.5.0.real_conv.weight",
             "decoder.5.0.real_conv.bias", "enhance.0.real_lstm.weight_hh_l0"]
    table, prev = _toy([(k, 2 * i, 2) for i, k in enumerate(names)])
    sim = _clone(prev)
    vals = {"encoder.0.0.real_conv.weight": 1.0, "encoder.0.0.real_conv.bias": 1e-6, "encoder.0.1.weight": 1e-2, "encoder.0.2.weight": 1e-5,
            "decoder.5.0.real_conv.weight": 1.0, "decoder.5.0.real_conv.bias": 1e-6, "enhance.0.real_lstm.weight_hh_l0": 1e-6}
    for i, k in enumerate(names):
        sim[GRAD][2 * i:2 * i + 2] = vals[k]
    errs = {}
    for i, k in enumerate(names):
        dev = _clone(sim)
        dev[GRAD][2 * i] *= 1.5                                                # half of itself off
        v = compare_op(prev, sim, dev, table, 2, "fp32")
        errs[k] = v.worst * 1e-3
    assert abs(errs["encoder.0.0.real_conv.bias"] - 0.5e-6) < 1e-9             # bias in front of a norm: against the conv's weight gradient
    assert abs(errs["encoder.0.2.weight"] - 0.5e-5 / 1e-2) < 1e-9               # slope: against the layer's norm-weight gradient
    for k in ("encoder.0.0.real_conv.weight", "encoder.0.1.weight", "decoder.5.0.real_conv.weight", "decoder.5.0.real_conv.bias",
              "enhance.0.real_lstm.weight_hh_l0"):                              # everything else on its own (decoder.5: no norm behind the conv)
        assert abs(errs[k] - 0.5) < 1e-6, (k, errs[k])


def test_counts_compare_exactly_and_per_element_triggers_on_the_tensor():
    table, prev = _toy([("w", 0, 4)], [("bn.running_var", 0, 4), ("bn.num_batches_tracked", 4, 1)])
    sim = _clone(prev)
    sim[STATE][0:4] = 50.0
    sim[STATE][4] = 1.0
    dev = _clone(sim)
    dev[STATE][4] = 1.0 + 2e-4                                                  # inside 1e-3 of itself, and nothing beside the arena's 50
    v = compare_op(prev, sim, dev, table, 5, "fp32")
    assert v.worst == float("inf") and "num_batches_tracked" in v.where
    # per_element: the tensor's own maximum decides, not the arena's
    sim[GRAD][0:4] = torch.tensor([0.5, 0.01, 0.02, 0.03])
    dev = _clone(sim)
    dev[GRAD][1] += 4e-4                                                        # 8e-4 of the tensor's maximum
    assert compare_op(prev, sim, dev, table, 2, "fp32", per_element=True).worst < 1.0
    sim[GRAD][0] = 100.0
    dev = _clone(sim)
    dev[GRAD][1] += 4e-4
    dev[GRAD][0] += 0.05                                                        # 5e-4 of itself
    assert compare_op(prev, sim, dev, table, 2, "fp32", per_element=True).worst < 1.0        # floor 1 per element
    dev[GRAD][1] += 2e-3
    v = compare_op(prev, sim, dev, table, 2, "fp32", per_element=True)
    assert v.worst > 1.0 and v.where.startswith("A_GRAD:w ")
    assert compare_op(prev, sim, dev, table, 2, "fp32", per_element=False).worst < 1.0


def test_tolerances_per_dtype_and_op_kind():
    """The bars of the driver before the comparator moved here."""
    t = opcheck.tolerance
    assert (t(1, "enc0.y", 1, "bf16"), t(0, "enc0.y", 1, "fp32"), t(0, "A_GRAD", 2, "bf16")) == (1.6e-2, 1e-3, 1e-3)
    assert (t(0, "enc1.bnpart", 1, "bf16"), t(0, "enc1.bnpart", 1, "fp32"), t(0, "enc1.bnpart", 2, "bf16")) == (4e-3, 1e-3, 1e-3)
    assert (t(0, "c.f", 9, "bf16"), t(0, "A_GRAD", 10, "bf16"), t(0, "c.f", 9, "fp32"), t(1, "h.f", 9, "bf16")) == (4e-3, 4e-3, 1e-3, 1.6e-2)
    assert (t(0, "c.f", 23, "bf16"), t(0, "c.f", 24, "bf16")) == (1e-3, 1e-3)
