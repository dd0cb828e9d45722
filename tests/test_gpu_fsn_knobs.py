"""GPU: FullSubNet beyond the default knobs - full-band neighbours, any sub-band width, every output activation in both heads - against
goldens captured from the real reference (tests/golden/make_fsn_knobs_golden.py; pinned on the CPU by tests/test_fsn_knobs_cpu.py).
Budgets are the project's own: TOL (fp32) and the named bf16 budgets of tests/test_gpu_model.py."""
import numpy as np
import pytest
import torch

from oracle.weights import fill_state_dict_, test_signals as make_signals
from test_fsn_knobs_cpu import CASES
from test_gpu_model import BF16_GRAD_L2, BF16_GRAD_WORST, BF16_LOSS, BF16_OUT_L2, BF16_OUT_MAX, TOL
from util import knobs, load_golden, rel_err, rel_l2, sub

pytestmark = pytest.mark.gpu


def make_model(name, g, dtype="fp32"):
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models
    ns, nf, seq, norm, fb_act, sb_act, hid = CASES[name]
    cfg.loss, cfg.act_dtype = "MSE", dtype
    try:
        m = models.FullSubNet(sb_num_neighbors=ns, fb_num_neighbors=nf, sequence_model=seq, fb_output_activate_function=fb_act,
                              sb_output_activate_function=sb_act, fb_model_hidden_size=hid[0], sb_model_hidden_size=hid[1], norm_type=norm)
    finally:
        cfg.act_dtype = "fp32"
    fill_state_dict_(m)
    with torch.no_grad():           # the factor the generator applied so that the head's activation clips (g/meta/*_head_scale)
        for net, key in ((m.fb_model, "fb"), (m.sb_model, "sb")):
            s = float(g[f"g/meta/{key}_head_scale"])
            net.fc_output_layer.weight.mul_(s)
            net.fc_output_layer.bias.mul_(s)
    m = m.to("cuda").train()
    m.dropout_keep = 1.0
    return m


def inputs(g):
    from sefd_amd import tools_for_model as tools
    x, y = make_signals(int(g["g/meta/B"]), int(g["g/meta/L"]))
    x, y = x.cuda(), y.cuda()
    nc, cc = tools.stft(x), tools.stft(y)
    noisy_mag, _ = tools.mag_phase(nc)
    return x, y, noisy_mag, tools.build_complex_ideal_ratio_mask(nc, cc)


@pytest.mark.parametrize("name", list(CASES))
def test_knobs_step_against_reference_golden(name):
    """The body of test_fullsubnet_step_against_reference_golden with the new constructor arguments, fp32, TOL = 1e-3."""
    g = load_golden("fsn_knobs_" + name)
    m = make_model(name, g)
    x, y, noisy_mag, cirm = inputs(g)
    assert rel_err(noisy_mag[:, ::4, ::3], g["g/noisy_mag"]) < TOL
    assert rel_err(cirm[:, ::4, ::3], g["g/cirm"]) < TOL
    crm = m(noisy_mag)
    lossv = m.loss(cirm, crm)
    m.zero_grad()
    lossv.backward()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    print(name, "crm", rel_err(crm, g["g/crm"]), "loss", float(lossv), float(g["g/loss"]))
    for k, v in sub(g, "g/grad_norm").items():
        print("  norm", k, float(grads[k].double().norm()), float(v))
    for k, v in sub(g, "g/grad").items():
        print("  grad", k, rel_l2(grads[k], v))
    for k, v in sub(g, "g/grad_samp").items():
        print("  samp", k, rel_l2(grads[k].reshape(-1)[::211], v))
    assert rel_err(crm, g["g/crm"]) < TOL
    assert abs(float(lossv) - float(g["g/loss"])) < TOL * abs(float(g["g/loss"]))
    for k, v in sub(g, "g/grad_norm").items():
        assert abs(float(grads[k].double().norm()) - float(v)) <= TOL * float(v) + 1e-9, k
    for k, v in sub(g, "g/grad").items():
        assert rel_l2(grads[k], v) < TOL, k
    for k, v in sub(g, "g/grad_samp").items():
        assert rel_l2(grads[k].reshape(-1)[::211], v) < TOL, k


@pytest.mark.parametrize("row_block", [False, True])
def test_bf16_width40_step_against_reference_golden(row_block):
    """fsn_knobs_default_fb4 in bf16 as test_bf16_fullsubnet_step_against_reference_golden: the cluster and (LSTM_ROWS_MIN=64) the row-block
    recurrences behind a width-40 input GEMM, held to that test's budgets."""
    if row_block:
        knobs.set("LSTM_ROWS_MIN", "64")
    g = load_golden("fsn_knobs_default_fb4")
    m = make_model("default_fb4", g, "bf16")
    x, y, noisy_mag, cirm = inputs(g)
    crm = m(noisy_mag)
    lossv = m.loss(cirm, crm)
    lossv.backward()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    vals = [rel_l2(grads[k], v) for k, v in sub(g, "g/grad").items()] + \
           [rel_l2(grads[k].reshape(-1)[::211], v) for k, v in sub(g, "g/grad_samp").items()]
    rec = dict(crm_rel_l2=rel_l2(crm, g["g/crm"]), crm_rel_max=rel_err(crm, g["g/crm"]), loss=float(lossv), loss_ref=float(g["g/loss"]),
               grad_rel_l2_worst=float(max(vals)), grad_rel_l2_median=float(np.median(vals)))
    rec["loss_rel"] = abs(rec["loss"] - rec["loss_ref"]) / abs(rec["loss_ref"])
    print(rec)
    plan = next(v for k, v in m._runtimes.items() if k[0] == "fsn")[0]
    assert (plan.buffer("sb_model.l0.gates")[3] == 1) == row_block         # bf16 gate slabs <=> row-block kernels
    assert plan.buffer("sb_in")[2] == (21 + 2) * 2 * 257 * 40 * 2          # width 40: rows of five 16-byte chunks
    assert rec["crm_rel_l2"] < BF16_OUT_L2 and rec["crm_rel_max"] < BF16_OUT_MAX and rec["loss_rel"] < BF16_LOSS, rec
    assert rec["grad_rel_l2_median"] < BF16_GRAD_L2 and rec["grad_rel_l2_worst"] < BF16_GRAD_WORST, rec


@pytest.mark.parametrize("name", ["fb1_tanh", "fb2_relu6_gru"])
def test_fused_train_step_equals_autograd_route(name):
    from sefd_amd.optim import Adam
    g = load_golden("fsn_knobs_" + name)
    m = make_model(name, g)
    x, y, noisy_mag, cirm = inputs(g)
    m.zero_grad()
    own = m.loss(cirm, m(noisy_mag))
    own.backward()
    g_own, p0 = m._flat_grad.clone(), m._flat_param.clone()
    for (off, n, _), (_, p) in zip(m._param_slices, m._trainable()):
        g_own[off:off + n].copy_(p.grad.reshape(-1))
    fused = float(m.train_step(x, y, Adam(m.parameters(), lr=1e-3), loss_kind="MSE"))
    assert abs(fused - float(own)) < 1e-5 * max(1.0, abs(float(own))), (fused, float(own))
    expect = p0 - 1e-3 * g_own / (g_own.abs() + 1e-8)
    big = g_own.abs() > 1e-4 * g_own.abs().max()                   # (where the gradient is rounding noise its sign is too)
    assert float((m._flat_param - expect)[big].abs().max()) < 2e-5


def test_backward_gather_is_bit_reproducible():
    g = load_golden("fsn_knobs_fb4")
    m = make_model("fb4", g)
    x, y, noisy_mag, cirm = inputs(g)
    flats = []
    for _ in range(2):
        m.zero_grad()
        m.loss(cirm, m(noisy_mag)).backward()
        torch.cuda.synchronize()
        flats.append(m._flat_grad.clone())
    assert float(flats[0].abs().max()) > 0 and torch.equal(flats[0], flats[1])


def test_validate_and_eval_mode_with_the_knobs(tmp_path):
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models, tools_for_model as tools, trainer
    cfg.loss, cfg.act_dtype, cfg.model = "MSE", "fp32", "FullSubNet"
    m = models.FullSubNet(fb_num_neighbors=4, sb_output_activate_function="Tanh", fb_model_hidden_size=128, sb_model_hidden_size=64)
    fill_state_dict_(m)
    m = m.to("cuda").train()
    x, y = make_signals(2, 6000)
    seen = []

    def pesq(est, clean):
        seen.append(est.copy())
        return np.full(len(est), 1.5)

    vloss, p, s = trainer.fullsubnet_validate(m, [(x, y), (x.flip(0), y.flip(0))], None, str(tmp_path), 1, "cuda",
                                              scorers=(pesq, lambda e, c: np.full(len(e), 0.5)))
    assert np.isfinite(float(vloss)) and len(seen) == 2
    assert all(e.shape == (2, 6000) and np.isfinite(e).all() for e in seen)
    noisy_mag = tools.mag_phase(tools.stft(x.cuda()))[0]
    m.train()
    m.dropout_keep = 1.0
    with torch.no_grad():
        crm_train = m(noisy_mag).clone()
        m.eval()
        crm_eval = m(noisy_mag).clone()
    assert float(crm_train.abs().max()) > 0 and float(crm_train.abs().max()) <= 1.0 and torch.equal(crm_train, crm_eval)


def test_stale_backward_is_refused():
    """A forward of the same shape between a forward and its backward overwrites the activations in the runtime's arena: that backward raises; a
    fresh forward and backward reach the parameters (the input is detached)."""
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models
    cfg.loss, cfg.act_dtype = "MSE", "fp32"
    m = models.FullSubNet(sb_num_neighbors=2, fb_num_neighbors=2, fb_model_hidden_size=16, sb_model_hidden_size=16)
    fill_state_dict_(m)
    m = m.to("cuda").train()
    mag = torch.rand(1, 257, 4, generator=torch.Generator().manual_seed(5)).cuda() + 0.1
    crm = m(mag)
    m(mag)
    with pytest.raises(RuntimeError, match="overwrote the activations"):
        (crm ** 2).sum().backward()
    m.zero_grad()
    (m(mag) ** 2).sum().backward()
    g = m.sb_model.fc_output_layer.weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
