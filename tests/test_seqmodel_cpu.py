"""CPU: SequenceModel on its own (tools_for_model.py:726-795) - constructor, planner (csrc/plan_seq.cpp) and, on the host simulator, the fp32
plans of every golden case of tests/golden/make_seqmodel_golden.py at the project's fp32 bar (TOL of tests/test_gpu_model.py)."""
import json
import os

import numpy as np
import pytest
import torch

from seqmodel_common import ACTS, CASES, assert_fp32, formula_params, golden_errors, seq_dict, time_major, torch_shapes
from simutil import ARENA_GRAD, PHASE_BWD, PHASE_FWD, Plan, fill_params, read_params, sim_run
from util import GOLDEN, knobs, load_golden, rel_err

TOL = 1e-3                       # tests/test_gpu_model.py TOL (importing that module would need nothing from the GPU, but it is a GPU suite)
OP_LSTM_FWD, OP_LSTM_BWD, OP_DROPOUT_FWD, OP_DROPOUT_BWD = 9, 10, 25, 26        # sefd_desc.h OpKind
ABI = json.load(open(os.path.join(GOLDEN, "seqmodel_abi.json")))


def test_constructor_state_dict_and_plan():
    """Fails before this feature: the constructor raised NotImplementedError and the planner had no such model."""
    import sefd_amd  # noqa: F401
    from sefd_amd import models, tools_for_model
    m = models.SequenceModel(21, 5, 64, 3, True, "LSTM", "Tanh")
    ref = torch.nn.LSTM(21, 64, 3, batch_first=True, bidirectional=True)
    want = {"sequence_model." + k: tuple(v.shape) for k, v in ref.state_dict().items()}
    want.update({"fc_output_layer.weight": (5, 128), "fc_output_layer.bias": (5,)})
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want and list(m.state_dict()) == list(want)
    assert tools_for_model.SequenceModel is models.SequenceModel
    plan = Plan(3, 9, model="SequenceModel", seq=seq_dict("LSTM", 21, 5, 64, 3, True))
    assert {k: s for k, (_, s) in plan.params.items()} == want and list(plan.params) == list(want)
    with pytest.raises(NotImplementedError, match="Not implemented RNN"):
        models.SequenceModel(21, 5, 64, 1, False, "RNN")
    with pytest.raises(NotImplementedError, match="activation"):
        models.SequenceModel(21, 5, 64, 1, False, "LSTM", "Sigmoid")
    with pytest.raises(RuntimeError, match="cuda"):
        m(torch.zeros(1, 21, 4))


def test_dropin_module_is_the_same_class():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import tools_for_model, models; "
            "assert tools_for_model.SequenceModel is models.SequenceModel; print('same')") % os.path.join(root, "dropin")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert out.returncode == 0 and "same" in out.stdout, out.stderr


def test_fullsubnet_children_keep_their_state_dict():
    import sefd_amd  # noqa: F401
    from sefd_amd import models
    m = models.FullSubNet(fb_model_hidden_size=64, sb_model_hidden_size=32, weight_init=False)
    assert isinstance(m.fb_model, models.SequenceModel) and list(m.fb_model.state_dict()) == list(torch_shapes("LSTM", 257, 257, 64, 2, False))
    owner = next(m.parameters())._sefd_owner()
    assert owner is m and all(p._sefd_owner() is m for p in m.parameters())


def lstm_ops(plan):
    return [int((plan.op_kinds(ph)[0] == kind).sum()) if plan.num_ops(ph) else 0 for ph, kind in ((PHASE_FWD, OP_LSTM_FWD), (PHASE_BWD, OP_LSTM_BWD))]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("seq", ["LSTM", "GRU"])
@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_planner_grid(layers, bi, seq, dtype, training):
    shapes = torch_shapes(seq, 21, 5, 64, layers, bi)
    plan = Plan(3, 9, model="SequenceModel", seq=seq_dict(seq, 21, 5, 64, layers, bi, keep=0.2), act_dtype=dtype, training=training)
    assert list(plan.params) == list(shapes) and [s for _, s in plan.params.values()] == list(shapes.values())
    assert plan.num_ops(PHASE_FWD) > 0 and (plan.num_ops(PHASE_BWD) > 0) == training
    assert lstm_ops(plan) == [0, 0]                                   # H = 64: stepped
    for name, n in (("io.x", 9 * 3 * 24), ("io.grad_x", 9 * 3 * 24), ("io.y", 9 * 3 * 5), ("io.grad_y", 9 * 3 * 5)):
        assert plan.buffer(name)[2] == 4 * n, name
    ndrop = int((plan.op_kinds(PHASE_FWD)[0] == OP_DROPOUT_FWD).sum())
    assert ndrop == ((layers - 1) * (2 if bi else 1) if training else 0)     # eval plans: keep = 1, no dropout op


@pytest.mark.parametrize("layers,bi", [(1, False), (1, True), (3, True), (2, False)])
def test_cluster_launches_are_planned_for_bf16_h192(layers, bi):
    sd = seq_dict("LSTM", 21, 5, 192, layers, bi)
    plan = Plan(18, 10, model="SequenceModel", seq=sd, act_dtype="bf16")
    assert lstm_ops(plan) == [layers, layers]                         # ONE launch per layer and phase, both directions inside it
    sz, u, off = ABI["sefd_op_size"] // 4, ABI["op_union_offset"], ABI["lstm_rec_offsets"]
    for ph, kind in ((PHASE_FWD, OP_LSTM_FWD), (PHASE_BWD, OP_LSTM_BWD)):
        n = plan.num_ops(ph)
        import ctypes as C
        raw = np.ctypeslib.as_array((C.c_int32 * (n * sz)).from_address(plan.ops_ptr(ph))).reshape(n, sz)
        for row in raw[raw[:, 0] == kind]:
            f = {k: int(row[(u + o) // 4]) for k, o in off.items()}
            assert f == dict(gx_ld=(8 if bi else 4) * 192, G=2 if bi else 1, nset=2 if bi else 1, t0=0, t1=0, rev_mask=2 if bi else 0), f
    assert lstm_ops(Plan(18, 10, model="SequenceModel", seq=sd, act_dtype="fp32")) == [0, 0]
    assert lstm_ops(Plan(18, 10, model="SequenceModel", seq=dict(sd, sequence_model="GRU"), act_dtype="bf16")) == [0, 0]
    knobs.set("LSTM_STEPPED", "1")
    assert lstm_ops(Plan(18, 10, model="SequenceModel", seq=sd, act_dtype="bf16")) == [0, 0]


@pytest.mark.parametrize("seq,match", [(dict(num_layers=0), r"1 \.\. 8"), (dict(num_layers=9), r"1 \.\. 8"), (dict(hidden_size=60), "multiple of 8"),
                                        (dict(input_size=0), "at least 1"), (dict(output_size=0), "at least 1")])
def test_refusals_name_their_limit(seq, match):
    with pytest.raises(ValueError, match=match):
        Plan(3, 9, model="SequenceModel", seq=dict(seq_dict("LSTM", 21, 5, 64, 2, False), **seq))
    with pytest.raises(ValueError, match="at least 1"):
        Plan(3, 0, model="SequenceModel", seq=seq_dict("LSTM", 21, 5, 64, 2, False))


def test_descriptor_did_not_grow():
    import sefd_amd  # noqa: F401
    from sefd_amd import _lib
    assert _lib.lib().sefd_op_size() == ABI["sefd_op_size"]


def sim_step(plan, P, x, tgt, act, seed=None):
    """Forward, loss = mean((act(y) - tgt)^2), backward on the host simulator.  Returns (y [B, O, T], loss, dx [B, I, T], grads, arenas)."""
    B, I, T = x.shape
    O = tgt.shape[1]
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, P)
    if seed is not None:
        plan.set_seed(ar, seed)
    xt = time_major(x)
    plan.io(ar, "x", tuple(xt.shape)).copy_(xt)
    sim_run(plan, PHASE_FWD, ar)
    pre = plan.io(ar, "y", (T, B, O)).clone().requires_grad_(True)
    y = ACTS[act](pre).permute(1, 2, 0)
    loss = ((y - tgt) ** 2).mean()
    loss.backward()
    plan.io(ar, "grad_y", (T, B, O)).copy_(pre.grad)
    sim_run(plan, PHASE_BWD, ar)
    dx = plan.io(ar, "grad_x", tuple(xt.shape))[:, :, :I].permute(1, 2, 0).clone()
    return y.detach(), float(loss.detach()), dx, read_params(plan, ar, ARENA_GRAD), ar


@pytest.mark.parametrize("name", list(CASES))
def test_host_simulator_fp32_against_reference_golden(name):
    seq, I, O, H, NL, bi, act, B, T = CASES[name]
    g = load_golden("seqmodel_" + name)
    assert (int(g["g/meta/H"]), int(g["g/meta/num_layers"]), int(g["g/meta/bidirectional"]), str(g["g/meta/act"])) == (H, NL, int(bi), str(act))
    assert float(g["g/meta/min_hh_effect"]) >= 0.05                   # the generator's condition 2: no recurrence can be ignored at a 1e-3 bar
    plan = Plan(B, T, model="SequenceModel", seq=seq_dict(seq, I, O, H, NL, bi), act_dtype="fp32")
    P = formula_params(torch_shapes(seq, I, O, H, NL, bi), float(g["g/meta/head_scale"]))
    y, loss, dx, grads, _ = sim_step(plan, P, torch.from_numpy(g["g/x"]), torch.from_numpy(g["g/tgt"]), act)
    e = golden_errors(g, y, loss, dx, grads)
    print(name, e)
    assert_fp32(e, TOL)


@pytest.mark.parametrize("seq", ["LSTM", "GRU"])
def test_reverse_direction_is_the_forward_one_on_flipped_time(seq):
    """Reverse weights = copies of the forward ones: h_rev(x) == flip_t(h_fwd(flip_t(x))), the same arithmetic on the same numbers in another
    frame order (bound 1e-6 relative)."""
    I, O, H, B, T = 21, 5, 64, 3, 9
    plan = Plan(B, T, model="SequenceModel", seq=seq_dict(seq, I, O, H, 1, True), act_dtype="fp32")
    P = formula_params(torch_shapes(seq, I, O, H, 1, True))
    for k in list(P):
        if k.endswith("_reverse"):
            P[k] = P[k[:-len("_reverse")]].clone()
    x = torch.rand(B, I, T, generator=torch.Generator().manual_seed(3)) * 4
    hs = []
    for xin in (x, x.flip(2)):
        ar = plan.alloc_arenas("cpu")
        fill_params(plan, ar, P)
        plan.io(ar, "x", (T, B, 24)).copy_(time_major(xin))
        sim_run(plan, PHASE_FWD, ar)
        hs.append(plan.view(ar, "l0.h").view(2, T, B, H).clone())
    assert float(hs[0][1].abs().max()) > 1e-2
    assert rel_err(hs[0][1], hs[1][0].flip(0)) < 1e-6
    assert rel_err(hs[0][0], hs[1][1].flip(0)) < 1e-6
    assert rel_err(hs[0][1], hs[0][0]) > 1e-2                         # ... and the two directions do differ on one input


def test_dropout_masks_on_the_simulator():
    seq, I, O, H, NL, B, T, keep = "LSTM", 21, 5, 64, 3, 3, 9, 0.2
    plan = Plan(B, T, model="SequenceModel", seq=seq_dict(seq, I, O, H, NL, True, keep=keep), act_dtype="fp32")
    P = formula_params(torch_shapes(seq, I, O, H, NL, True))
    x = torch.rand(B, I, T, generator=torch.Generator().manual_seed(5)) * 4
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, P)
    plan.set_seed(ar, 12345)
    plan.io(ar, "x", (T, B, 24)).copy_(time_major(x))
    sim_run(plan, PHASE_FWD, ar)
    assert "l2.hd" not in plan.buffer_names() and "l1.hd" in plan.buffer_names()      # the last layer is not dropped
    plan.io(ar, "grad_y", (T, B, O)).copy_(torch.rand(T, B, O, generator=torch.Generator().manual_seed(6)) - 0.5)
    n = T * B * H
    # backward up to the DROPOUT_BWD ops of a layer: its dh then holds their output alone (the layer's own recurrence accumulates onto it afterwards)
    drops = [int(i) for i in np.nonzero(plan.op_kinds(PHASE_BWD)[0] == OP_DROPOUT_BWD)[0]]
    assert len(drops) == 4
    masks, cur = [], 0
    for l, stop in ((1, drops[1] + 1), (0, drops[3] + 1)):
        sim_run(plan, PHASE_BWD, ar, cur, stop)
        cur = stop
        h, hd = plan.view(ar, f"l{l}.h").view(2, n), plan.view(ar, f"l{l}.hd").view(2, n)
        dlo, dhi = plan.view(ar, f"dh.{l}").view(2, n), plan.view(ar, f"dhd.{l}").view(2, n)
        for d in (0, 1):
            live = h[d] != 0
            mask = hd[d] != 0
            assert int(live.sum()) > 0.99 * n and not bool((mask & ~live).any())
            frac = float(mask[live].double().mean())
            assert abs(frac - keep) <= 4 * (keep * (1 - keep) / int(live.sum())) ** 0.5, (l, d, frac)
            assert rel_err(hd[d][mask], h[d][mask] / keep) < 1e-6                       # inverted dropout: kept values scaled by 1 / keep
            glive = (dhi[d] != 0) & live
            assert int(glive.sum()) > 0.9 * n
            # the backward uses the forward's mask: the gradient is zero exactly where the mask is
            assert torch.equal((dlo[d] != 0)[glive], mask[glive]) and float(dlo[d][~mask].abs().max()) == 0.0
            assert rel_err(dlo[d][mask], dhi[d][mask] / keep) < 1e-6
            masks.append(mask)
    sim_run(plan, PHASE_BWD, ar, cur, plan.num_ops(PHASE_BWD))
    assert all(bool(torch.isfinite(v).all()) for v in read_params(plan, ar, ARENA_GRAD).values())
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(masks[a], masks[b]), (a, b)     # distinct per (layer, direction)
