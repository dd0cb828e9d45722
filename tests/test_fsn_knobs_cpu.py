"""CPU: FullSubNet with fb_num_neighbors > 0, any sb_num_neighbors and all four output activations in both heads.

* the oracle restatement reproduces the goldens captured from the real reference (tests/golden/make_fsn_knobs_golden.py) at the tolerance of
  tests/test_oracle_fsn.py - this pins the fixtures the GPU tests (tests/test_gpu_fsn_knobs.py) are held to;
* the planner builds every such configuration (fp32 / bf16, training / eval) with the reference's parameter shapes and order;
* the DEFAULT plans are untouched: their op lists, constants and arena sizes hash to tests/golden/fsn_plan_digests.json, produced by
  tests/golden/make_fsn_plan_digests.py on the commit BEFORE these knobs reached the planner."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from oracle.fullsubnet import FSNConfig, fsn_forward, fsn_state_shapes, fsn_targets
from oracle.losses import main_loss
from oracle.step import adam_update
from oracle.weights import formula_state_dict, test_signals as make_signals
from simutil import PHASE_BWD, PHASE_FWD, Plan
from util import GOLDEN, load_golden, rel_err, sub

# name: (sb_num_neighbors, fb_num_neighbors, sequence_model, norm_type, fb act, sb act, hidden)
CASES = {
    "fb4": (15, 4, "LSTM", "offline_laplace_norm", "ReLU", None, (128, 64)),
    "fb1_tanh": (15, 1, "LSTM", "offline_laplace_norm", "Tanh", "Tanh", (128, 64)),
    "fb2_relu6_gru": (15, 2, "GRU", "cumulative_layer_norm", "ReLU6", "ReLU", (128, 64)),
    "fb3_cumlaplace": (15, 3, "LSTM", "cumulative_laplace_norm", None, "ReLU6", (128, 64)),
    "sb10_gauss": (10, 0, "LSTM", "offline_gaussian_norm", "ReLU", None, (128, 64)),
    "default_fb4": (15, 4, "LSTM", "offline_laplace_norm", "ReLU", None, (512, 384)),
}
WIDTH = {"fb4": 40, "fb1_tanh": 34, "fb2_relu6_gru": 36, "fb3_cumlaplace": 38, "sb10_gauss": 22, "default_fb4": 40}


def scale_heads(P, g):
    """The factor the generator applied to a head's fc_output_layer so that its activation clips (g/meta/*_head_scale)."""
    for net in ("fb", "sb"):
        s = float(g[f"g/meta/{net}_head_scale"])
        for leaf in ("weight", "bias"):
            P[f"{net}_model.fc_output_layer.{leaf}"] = P[f"{net}_model.fc_output_layer.{leaf}"] * s
    return P


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_exercises_every_side_of_its_activations(name):
    g = load_golden("fsn_knobs_" + name)
    ns, nf, seq, norm, fb_act, sb_act, hid = CASES[name]
    assert (int(g["g/meta/sb_num_neighbors"]), int(g["g/meta/fb_num_neighbors"])) == (ns, nf)
    assert (str(g["g/meta/fb_act"]), str(g["g/meta/sb_act"])) == (str(fb_act), str(sb_act))
    for net, act in (("fb", fb_act), ("sb", sb_act)):
        st = {k: float(v) for k, v in sub(g, f"g/meta/{net}_pre").items()}
        if act == "ReLU6":
            assert st["gt6"] >= 0.01 and st["lt0"] >= 0.01 and st["mid"] >= 0.01, (net, st)
        elif act == "ReLU":
            assert st["lt0"] >= 0.05 and 1.0 - st["lt0"] >= 0.05, (net, st)
        elif act == "Tanh":
            assert st["abs_gt1"] >= 0.01, (net, st)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_reproduces_reference_golden(name):
    g = load_golden("fsn_knobs_" + name)
    ns, nf, seq, norm, fb_act, sb_act, hid = CASES[name]
    cfg = FSNConfig(sb_num_neighbors=ns, fb_num_neighbors=nf, fb_hidden=hid[0], sb_hidden=hid[1], fb_act=fb_act, sb_act=sb_act,
                    sequence_model=seq, norm_type=norm)
    shapes = fsn_state_shapes(cfg)
    assert shapes["sb_model.sequence_model.weight_ih_l0"][1] == WIDTH[name]
    P = scale_heads(formula_state_dict(shapes), g)
    B, L = int(g["g/meta/B"]), int(g["g/meta/L"])
    x, y = make_signals(B, L)
    noisy_mag, cirm = fsn_targets(x, y, cfg)
    assert rel_err(noisy_mag[:, ::4, ::3], g["g/noisy_mag"]) < 1e-5
    assert rel_err(cirm[:, ::4, ::3], g["g/cirm"]) < 1e-5
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    crm = fsn_forward(Pg, noisy_mag, cfg)
    lossv = main_loss("MSE", cirm, crm)
    names = list(Pg)
    grads = dict(zip(names, torch.autograd.grad(lossv, [Pg[k] for k in names])))
    assert rel_err(crm, g["g/crm"]) < 2e-5
    assert abs(float(lossv) - float(g["g/loss"])) < 2e-5 * max(1.0, abs(float(g["g/loss"])))
    for k, v in sub(g, "g/grad_norm").items():
        assert abs(float(grads[k].double().norm()) - float(v)) <= 3e-4 * float(v) + 1e-9, k
    for k, v in sub(g, "g/grad").items():
        assert rel_err(grads[k], v) < 3e-4, k
    for k, v in sub(g, "g/after_adam").items():
        newp, _, _ = adam_update(P[k], grads[k], torch.zeros_like(P[k]), torch.zeros_like(P[k]), 1)
        mask = np.abs(v - P[k].numpy()) > 0
        assert np.abs((newp.numpy() - P[k].numpy()) - (v - P[k].numpy()))[mask].max() < 5e-5, k


def fsn_dict(name):
    ns, nf, seq, norm, fb_act, sb_act, hid = CASES[name]
    return dict(sb_num_neighbors=ns, fb_num_neighbors=nf, fb_hidden=hid[0], sb_hidden=hid[1], fb_act=fb_act, sb_act=sb_act,
                sequence_model=seq, norm_type=norm)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_planner_builds_every_knob(name, dtype, training):
    ns, nf, seq, norm, fb_act, sb_act, hid = CASES[name]
    plan = Plan(2, 21, model="FullSubNet", fsn=fsn_dict(name), act_dtype=dtype, training=training)
    NG, W = (4 if seq == "LSTM" else 3), (2 * ns + 1) + (2 * nf + 1)
    assert W == WIDTH[name]
    assert plan.params["sb_model.sequence_model.weight_ih_l0"][1] == (NG * hid[1], W)
    shapes = fsn_state_shapes(FSNConfig(sb_num_neighbors=ns, fb_num_neighbors=nf, fb_hidden=hid[0], sb_hidden=hid[1], sequence_model=seq))
    assert list(plan.params) == list(shapes)                          # the module's (= the reference's state_dict) order
    assert [s for _, s in plan.params.values()] == [tuple(s) for s in shapes.values()]
    assert plan.num_ops(PHASE_FWD) > 0 and (plan.num_ops(PHASE_BWD) > 0) == training
    # rows are stored roundup(W, 8) wide: whole 16-byte chunks in bf16
    esz = 2 if dtype == "bf16" else 4
    assert plan.buffer("sb_in")[2] == (21 + 2) * 2 * 257 * ((W + 7) // 8 * 8) * esz


def test_two_gradient_buckets_build_with_the_knobs():
    plan = Plan(2, 21, model="FullSubNet", fsn=fsn_dict("default_fb4"), act_dtype="bf16", training=True, grad_buckets=2)
    op, lo, hi = plan.grad_bucket_range()
    assert lo == 0 and hi == plan.params["sb_model.sequence_model.weight_ih_l0"][0]


@pytest.mark.parametrize("fsn", [dict(fb_num_neighbors=32), dict(sb_num_neighbors=32), dict(fb_num_neighbors=-1)])
def test_plan_error_names_the_limit(fsn):
    with pytest.raises(ValueError, match=r"0 \.\. 31"):
        Plan(2, 21, model="FullSubNet", fsn=fsn)


def test_widest_supported_window_builds():
    plan = Plan(1, 5, model="FullSubNet", fsn=dict(sb_num_neighbors=31, fb_num_neighbors=31, fb_hidden=64, sb_hidden=32, sb_act="ReLU6", fb_act="Tanh"))
    assert plan.params["sb_model.sequence_model.weight_ih_l0"][1] == (128, 126)


def _digest_module():
    spec = importlib.util.spec_from_file_location("make_fsn_plan_digests", os.path.join(GOLDEN, "make_fsn_plan_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_default_plans_are_untouched():
    """Same ops, same constants, same arenas as before the knobs: the digests were recorded on the parent commit."""
    mod = _digest_module()
    want = json.load(open(os.path.join(GOLDEN, "fsn_plan_digests.json")))
    names = [n for n, *_ in mod.cases()]
    assert sorted(names) == sorted(want) and len(names) == 2 * 4 * 2 * 2
    for name, fsn, dt, training in mod.cases():
        got = mod.plan_digest(Plan(mod.B, mod.T, model="FullSubNet", fsn=fsn, act_dtype=dt, training=training))
        assert got == want[name], name
