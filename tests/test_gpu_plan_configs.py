"""GPU tier over the configuration table (plan_configs.py): every launch of every entry, in every listed dtype and under the entry's knobs, against
the host simulator from the same pre-op state (plan_check.ops_device_vs_sim: an error is localised to one launch, stray writes are detected);
then a few configurations end to end through models.DCCRN / models.CRN against the oracle computed here on the CPU."""
import contextlib

import numpy as np
import pytest
import torch

from oracle.dccrn import dccrn_forward, dccrn_state_shapes, is_trainable
from oracle.losses import main_loss
from oracle.step import adam_update, dccrn_train_step
from oracle.weights import fill_state_dict_, formula_state_dict, test_signals as make_signals
from plan_check import crn_config, dccrn_config, ops_device_vs_sim, report_path
from plan_configs import ACCEPTED, BY_NAME, frames_span, plan_kwargs
from util import knobs, rel_err, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-3                                   # test_gpu_model.py's bar for its fp32 goldens

OP_CASES = [(e, dt) for e in ACCEPTED for dt in e.dtypes]


@pytest.mark.parametrize("e,dtype", OP_CASES, ids=[f"{e.name}-{dt}" for e, dt in OP_CASES])
def test_every_op_of_the_entry_against_host_simulator(e, dtype):
    """Bars of test_gpu_ops.test_every_op_against_host_simulator: fp32 buffers 1e-3, bf16 buffers 1.6e-2, fp32 state of a bf16 recurrence and
    `.bnpart` sums 4e-3.  The entry's knobs steer it: DIRECT_MINM=0 (thin.hip on every eligible N <= 64 GEMM; read per launch), BN_FUSE=2 (BatchNorm
    backward sums in every GEMM kernel's epilogue), CG256_MINM / WG256_MINM = 64 (wide tiles on these few rows), LSTM_STEPPED."""
    from simutil import Plan
    for k, v in e.knobs:
        knobs.set(k, v)
    kw = plan_kwargs(e, dtype)
    if e.model == "CRN":
        from oracle.crn import crn_state_shapes
        P = formula_state_dict(crn_state_shapes(crn_config(e.kw)))
    else:
        okw = {k: v for k, v in kw.items() if k != "masking_mode"}
        P = formula_state_dict(dccrn_state_shapes(dccrn_config(kw.get("masking_mode", "E"), okw)))
    plan = Plan(e.B, e.L, **kw)
    lines, bad = ops_device_vs_sim(plan, P, e.model, e.B, e.L, dtype, report=f"ops_report_cfg_{e.name}_{dtype}.txt")
    assert not bad, "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ through the modules
@contextlib.contextmanager
def _module_cfg(kw, dtype, loss="SI-SNR"):
    """The reference's config.py globals for one module construction (restored afterwards)."""
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg
    names = ("dccrn_kernel_num", "masking_mode", "loss", "perceptual", "lstm", "skip_type", "act_dtype")
    old = {n: getattr(cfg, n) for n in names}
    cfg.dccrn_kernel_num, cfg.masking_mode, cfg.loss, cfg.perceptual = list(kw["kernel_num"]), kw.get("masking_mode", "E"), loss, False
    cfg.lstm, cfg.skip_type, cfg.act_dtype = kw.get("lstm", "complex"), kw.get("skip_type", True), dtype
    try:
        yield
    finally:
        for n, v in old.items():
            setattr(cfg, n, v)


def _make_dccrn(kw, dtype):
    from sefd_amd import models
    m = models.DCCRN(rnn_layers=kw.get("rnn_layers", 2), rnn_units=kw["rnn_units"], win_len=kw.get("win_len", 400), win_inc=kw.get("win_inc", 100),
                     fft_len=kw.get("fft_len", 512), win_type=kw.get("win_type", "hanning"), masking_mode=kw.get("masking_mode", "E"))
    fill_state_dict_(m)
    return m.to("cuda").train()


def noise_bias(k, n):
    return k.endswith("conv.bias") and not k.startswith(f"decoder.{n - 1}.")


def _check_fp32_step(m, x, y, r, n):
    """forward, backward (autograd route) and one fused Adam step of module `m` against the oracle step `r` (dict of oracle.step.dccrn_train_step),
    at test_gpu_model.py's fp32 bars: outputs, loss and gradients 1e-3 (L2; PReLU slopes 5e-3; no element off by 5e-3 of the largest), running
    statistics 1e-3, parameter updates 5e-5 where the oracle gradient is above rounding noise."""
    from sefd_amd.optim import Adam
    out = m(x.cuda(), y.cuda())
    wav = out[-1]
    for got, ref in zip(out, r["outputs"]):
        assert rel_err(got, ref) < TOL
    lossv = m.loss(wav, y.cuda()[:, :wav.shape[1]])
    assert abs(float(lossv) - float(r["loss"])) < TOL * max(1.0, abs(float(r["loss"])))
    lossv.backward()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    for k, v in r["grads"].items():
        if noise_bias(k, n):
            assert float(grads[k].abs().max()) < 1e-4 * float(r["grads"][k.replace(".bias", ".weight")].norm()) + 1e-7, k
            continue
        assert rel_l2(grads[k], v) < (5e-3 if k.endswith(".2.weight") else TOL) and rel_err(grads[k], v) < 5e-3, (k, rel_l2(grads[k], v), rel_err(grads[k], v))
        assert float(v.abs().max()) == 0.0 or float(grads[k].abs().max()) > 0.0, (k, "exactly zero")
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for k, v in r["new_stats"].items():
        assert rel_err(sd[k], v) < TOL, k
    # one fused step from the same parameters (the forward above moved only the running statistics)
    prev = {k: v.clone() for k, v in sd.items()}
    loss = m.train_step(x.cuda(), y.cuda(), Adam(m.parameters(), lr=1e-3))
    assert abs(float(loss) - float(r["loss"])) < TOL * max(1.0, abs(float(r["loss"])))
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    worst, covered, total = 0.0, 0, 0
    for k, v in r["new_params"].items():
        if noise_bias(k, n):
            continue
        gref = r["grads"][k]
        mask = gref.abs() > 1e-3 * gref.abs().max()                  # elsewhere the SIGN of a noise-level gradient decides a +-lr move
        covered += int(mask.sum())
        total += mask.numel()
        if mask.any():
            worst = max(worst, float(((sd[k] - prev[k]) - (v - r["old_params"][k]))[mask].abs().max()))
    assert covered > 0.5 * total and worst < 5e-5, (covered, total, worst)


DCCRN_STEPS = [("odd", dict(kernel_num=(8, 24, 40, 72, 136, 264), rnn_units=96), 2, 3000),
               ("depth3", dict(kernel_num=(24, 40, 72), rnn_units=64, masking_mode="C"), 2, 3000),
               ("fft256_rnn1", dict(kernel_num=(16, 32, 32, 64, 64), rnn_units=64, rnn_layers=1, fft_len=256, win_len=200, win_inc=50), 2, 2000)]


@pytest.mark.parametrize("name,kw,B,L", DCCRN_STEPS, ids=[c[0] for c in DCCRN_STEPS])
def test_dccrn_module_step_against_oracle(name, kw, B, L):
    cfg = dccrn_config(kw.get("masking_mode", "E"), {k: v for k, v in kw.items() if k != "masking_mode"})
    P = formula_state_dict(dccrn_state_shapes(cfg))
    x, y = make_signals(B, L)
    r = dccrn_train_step(P, cfg, x, y, loss_kind="SI-SNR")
    r["old_params"] = P
    with _module_cfg(kw, "fp32"):
        m = _make_dccrn(kw, "fp32")
        _check_fp32_step(m, x, y, r, len(kw["kernel_num"]))


def test_crn_five_layer_module_step_against_oracle():
    from oracle.crn import crn_forward, crn_state_shapes
    from sefd_amd import models
    e = BY_NAME["crn5"]
    kw = dict(e.kw)
    cfg = crn_config(kw)
    P = formula_state_dict(crn_state_shapes(cfg))
    x, y = make_signals(e.B, e.L)
    Pg = {k: (v.clone().requires_grad_(True) if is_trainable(k) else v) for k, v in P.items()}
    outs, new_stats = crn_forward(Pg, x, y, cfg, train=True)
    loss = main_loss("SI-SNR", outs[2], y)
    names = [k for k in P if is_trainable(k)]
    grads = dict(zip(names, torch.autograd.grad(loss, [Pg[k] for k in names])))
    new_params = {k: adam_update(P[k], grads[k], torch.zeros_like(P[k]), torch.zeros_like(P[k]), 1)[0] for k in names}
    r = dict(loss=loss.detach(), grads=grads, new_params=new_params, new_stats=new_stats, outputs=tuple(o.detach() for o in outs), old_params=P)
    with _module_cfg(kw, "fp32"):
        m = models.CRN(rnn_units=kw["rnn_units"], rnn_input_size=cfg.rnn_input_size, masking_mode="E")
        fill_state_dict_(m)
        _check_fp32_step(m.to("cuda").train(), x, y, r, len(kw["kernel_num"]))


def test_module_returns_the_clip_the_frames_cover():
    """L = 3050 at 400 / 100: the reference's ConviSTFT returns 3000 samples (tools_for_model.py:111), and so does models.DCCRN.forward - with the
    oracle's values and gradients; train_step refuses the length by name (its losses compare estimate and target sample by sample)."""
    from sefd_amd.optim import Adam
    e = BY_NAME["len3050"]
    kw = dict(e.kw)
    cfg = dccrn_config("E", kw)
    Lout = frames_span(e.L, cfg.win_len, cfg.win_inc)
    P = formula_state_dict(dccrn_state_shapes(cfg))
    x, y = make_signals(e.B, e.L)
    Pg = {k: (v.clone().requires_grad_(True) if is_trainable(k) else v) for k, v in P.items()}
    (o_r, o_i, wav), _ = dccrn_forward(Pg, x, cfg, targets=y, train=True)
    names = [k for k in P if is_trainable(k)]
    grads = dict(zip(names, torch.autograd.grad(main_loss("SI-SNR", wav, y[:, :Lout]), [Pg[k] for k in names])))
    with _module_cfg(kw, "fp32"):
        m = _make_dccrn(kw, "fp32")
        got = m(x.cuda(), y.cuda())
        assert got[2].shape == (e.B, Lout) == wav.shape
        assert rel_err(got[2], wav) < TOL and rel_err(got[0], o_r) < TOL
        m.loss(got[2], y.cuda()[:, :Lout]).backward()
        for k, p in m.named_parameters():
            if not noise_bias(k, 6):
                assert rel_l2(p.grad.cpu(), grads[k]) < (5e-3 if k.endswith(".2.weight") else TOL), k
        with pytest.raises(ValueError, match="cover 3000 samples"):
            m.train_step(x.cuda(), y.cuda(), Adam(m.parameters(), lr=1e-3))


# bf16 storage against the fp32 oracle on the odd-channel case (kernel_num 8, 24, 40, 72, 136, 264, rnn_units 192, B = 2, L = 3000, SI-SNR).  The bars are
# TWICE what the bf16 HOST SIMULATOR (every sum in double, only the bf16 storage roundings) measures against the fp32 oracle on this case:
#   out_wav max-abs 5.6e-3, loss 1.24e-2 relative, gradients: median relative L2 over the tensors 6.2e-2, worst tensor 9.8e-2 (encoder.5.0.real_conv.weight)
# On the MI355X kernels (fp32 accumulation) the module step measures: out_wav 6.0e-3, loss 1.56e-2, gradient median 6.4e-2, worst tensor 0.157 (encoder.5.2.weight).
BF16_ODD = dict(out_wav=2 * 5.6e-3, loss=2 * 1.24e-2, grad_median=2 * 6.2e-2, grad_worst=2 * 9.8e-2)


def test_bf16_odd_channel_module_step_against_oracle():
    from sefd_amd.optim import Adam
    kw = dict(BY_NAME["odd"].kw)
    B, L = 2, 3000
    cfg = dccrn_config("E", kw)
    P = formula_state_dict(dccrn_state_shapes(cfg))
    x, y = make_signals(B, L)
    r = dccrn_train_step(P, cfg, x, y, loss_kind="SI-SNR")
    with _module_cfg(kw, "bf16"):
        m = _make_dccrn(kw, "bf16")
        o_r, o_i, wav = m(x.cuda(), y.cuda())
        lossv = m.loss(wav, y.cuda())
        lossv.backward()
        errs = {k: rel_l2(p.grad.cpu(), r["grads"][k]) for k, p in m.named_parameters() if not noise_bias(k, 6)}
        fig = dict(out_wav=rel_err(wav, r["outputs"][2]), loss=abs(float(lossv) - float(r["loss"])) / abs(float(r["loss"])),
                   grad_median=float(np.median(list(errs.values()))), grad_worst=max(errs.values()))
        step_loss = float(m.train_step(x.cuda(), y.cuda(), Adam(m.parameters(), lr=1e-3)))
    print("bf16 odd-channel module step:", fig, "worst tensor", max(errs, key=errs.get), "train_step loss", step_loss)
    with open(report_path("bf16_odd_channels.txt"), "w") as f:
        f.write(repr(fig) + f" worst {max(errs, key=errs.get)} train_step loss {step_loss}\n")
    for k, bar in BF16_ODD.items():
        assert fig[k] < bar, (k, fig[k], bar)
    assert abs(step_loss - float(r["loss"])) < BF16_ODD["loss"] * abs(float(r["loss"]))
