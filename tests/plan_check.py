"""Checkers shared by the plan tests (a plain module, not a conftest).

CPU: a DCCRN / CRN plan interpreted by the host simulator against the oracle - forward taps, the three outputs, running statistics and every
parameter gradient - for any depth, channel tuple, front end and recurrent block the planner accepts (test_plan_hostsim.py, test_plan_configs_cpu.py).
GPU: every launch of a plan against the host simulator from the same pre-op state (test_gpu_ops.py, test_gpu_plan_configs.py, test_gpu_recurrence_edges.py,
test_gpu_rungemm_persist.py, test_gpu_clstm.py): transport, change detection and the report here, the comparison rule in opcheck.py."""
import os

import torch

import opcheck
from oracle.dccrn import DCCRNConfig, dccrn_forward, dccrn_state_shapes, is_trainable
from oracle.losses import main_loss
from oracle.weights import formula_state_dict, test_signals as make_signals
from plan_configs import frames_span
from simutil import PHASE_BWD, PHASE_FWD, Plan, act_to_nchw, fill_params, read_params, sim_run, spec_to_ref
from sefd_amd.plan import ARENA_GRAD, ARENA_STATE
from util import rel_err

ORACLE_KEYS = ("kernel_num", "rnn_layers", "rnn_units", "win_len", "win_inc", "fft_len", "lstm", "skip_type", "kernel_size", "win_type", "use_cbn")


def dccrn_config(mode, kw):
    return DCCRNConfig(masking_mode=mode, **{k: v for k, v in kw.items() if k in ORACLE_KEYS})


def _tail_noise(B, n):
    """A gradient laid on the samples behind the last frame (not part of the reference's output): it must reach no parameter."""
    return torch.full((B, n), 0.37)


def check_dccrn_plan_vs_oracle(mode, loss, kw, B, L, bars=None, report=None, oracle_dtype=torch.float32, kink=None, params=None):
    """Plan(B, L, masking_mode=mode, **kw) on the host simulator against oracle/dccrn.py.  Depth, bins per layer and hidden dim follow from
    kw (kernel_num, fft_len).  Bars (max-abs over max-abs): spectrum 1e-5, encoder activations 2e-5, decoder activations and outputs 5e-5,
    running statistics 1e-5, gradients 2e-4 (PReLU slopes 2e-3, encoder.0.1.bias 1e-2, conv biases in front of BatchNorm: noise);
    bars: {parameter name: measured conditioning bar} replaces the gradient bar of single tensors; report: dict that receives every figure.
    A trainable parameter whose oracle gradient is non-zero must not come out exactly zero (max-abs over max-abs cannot see a gradient that is
    zero where it should be small).  oracle_dtype=torch.float64: the same oracle with float64 parameters, inputs and front-end bases, for a case whose
    gradients the float32 oracle itself does not hold to the bars.
    kink = (decoder layer d, channel c): the oracle's BatchNorm output of that channel has ONE element within fp32 rounding of the PReLU kink (asserted:
    closer to zero than two fp32 ulps of 1), so which branch it takes - and with it the term (1 - slope) * dz of that element in decoder.<d>.1.bias[c] - is
    decided by the last bit of the statistics.  That tensor must meet its bar against the oracle's gradient with EITHER branch for that one element.
    params: {state_dict name: tensor} for the plan AND the oracle instead of the formula weights (recurrence_cases.hot_biases of them)."""
    cfg = dccrn_config(mode, kw)
    P = formula_state_dict(dccrn_state_shapes(cfg)) if params is None else params
    plan = Plan(B, L, masking_mode=mode, **kw)
    T, NF = plan.T, plan.NF
    Lout = frames_span(L, cfg.win_len, cfg.win_inc)
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, P)
    x, y = make_signals(B, L)
    plan.io(ar, "wav", (B, L)).copy_(x)
    sim_run(plan, PHASE_FWD, ar)
    report = {} if report is None else report

    # ---- oracle forward with taps
    Pg = {k: (v.to(oracle_dtype).requires_grad_(True) if is_trainable(k) else v.to(oracle_dtype)) for k, v in P.items()}
    taps = {}
    y = y.to(oracle_dtype)
    outs, new_stats = dccrn_forward(Pg, x.to(oracle_dtype), cfg, targets=y, train=True, taps=taps)
    o_r, o_i, wav = (outs[0], outs[2], outs[4]) if mode.startswith("Direct") else outs
    assert wav.shape == (B, Lout), (wav.shape, Lout)
    assert rel_err(spec_to_ref(plan.view(ar, "spec"), B, T, NF), taps["spec"]) < 1e-5
    n = len(cfg.kernel_num)
    ch = (2,) + tuple(cfg.kernel_num)
    F = [(cfg.fft_len // 2) >> i for i in range(n + 1)]
    for i in range(n):
        got = act_to_nchw(plan.view(ar, f"enc{i}.y"), B, T, F[i + 1], ch[i + 1])
        assert rel_err(got, taps[f"enc{i}.conv"]) < 2e-5, f"enc{i}.conv"
        got = act_to_nchw(plan.view(ar, f"enc{i}.z"), B, T, F[i + 1], ch[i + 1])
        assert rel_err(got, taps[f"enc{i}.out"]) < 2e-5, f"enc{i}.out"
    for d in range(n):
        idx = n - d
        cbuf = max(ch[idx - 1], 8) if d == n - 1 else ch[idx - 1]          # the mask layer's buffer is channel-padded to 8 (pad == 0)
        got = act_to_nchw(plan.view(ar, f"dec{d}.y"), B, T + 1, 2 * F[idx], cbuf)
        assert float(got[:, ch[idx - 1]:].abs().max()) == 0.0 if cbuf > ch[idx - 1] else True
        assert rel_err(got[:, :ch[idx - 1]], taps[f"dec{d}.conv"]) < 5e-5, f"dec{d}.conv"
    out_wav = plan.io(ar, "out_wav", (B, L))
    report["out_wav"] = rel_err(out_wav[:, :Lout], wav)
    assert report["out_wav"] < 5e-5
    assert float(out_wav[:, Lout:].abs().max()) == 0.0 if Lout < L else True          # behind the last frame: exactly zero
    assert rel_err(plan.io(ar, "out_real", (B, NF, T)), o_r) < 5e-5
    assert rel_err(plan.io(ar, "out_imag", (B, NF, T)), o_i) < 5e-5
    got_state = read_params(plan, ar, ARENA_STATE, plan.state)
    for k, v in new_stats.items():
        assert rel_err(got_state[k], v) < 1e-5, k

    # ---- backward: loss on the waveform plus a linear functional of the spectra (exercises all three output gradients)
    torch.manual_seed(3)
    cr, ci = torch.randn(B, NF, T) * 1e-3, torch.randn(B, NF, T) * 1e-3
    yo = y[:, :Lout]
    lossv = main_loss(loss, wav, yo) + (o_r * cr.to(oracle_dtype)).sum() + (o_i * ci.to(oracle_dtype)).sum()
    names = [k for k in Pg if is_trainable(k)]
    grads = dict(zip(names, torch.autograd.grad(lossv, [Pg[k] for k in names] + [wav], allow_unused=True, retain_graph=True)[:len(names)]))
    gw = torch.autograd.grad(main_loss(loss, wav, yo), wav, retain_graph=True)[0]
    plan.io(ar, "grad_wav", (B, L))[:, :Lout].copy_(gw)
    if Lout < L:
        plan.io(ar, "grad_wav", (B, L))[:, Lout:].copy_(_tail_noise(B, L - Lout))
    plan.io(ar, "grad_real", (B, NF, T)).copy_(cr)
    plan.io(ar, "grad_imag", (B, NF, T)).copy_(ci)
    sim_run(plan, PHASE_BWD, ar)
    got = read_params(plan, ar, ARENA_GRAD)
    worst = 0.0
    for k in names:
        ref = grads[k]
        if k.endswith("conv.bias") and not k.startswith(f"decoder.{n - 1}."):
            # analytically zero (bias in front of BatchNorm): both sides are rounding noise
            wk = k.replace(".bias", ".weight")
            assert got[k].abs().max() < 1e-4 * grads[wk].abs().max() + 1e-7, k
            continue
        e = rel_err(got[k], ref)
        if kink and k == f"decoder.{kink[0]}.1.bias":
            d, c = kink
            pre = taps[f"dec{d}.conv"][:, c].detach()
            bn = (pre - pre.mean()) / torch.sqrt(pre.var(unbiased=False) + 1e-5) * Pg[f"decoder.{d}.1.weight"][c].detach() + Pg[k][c].detach()
            b_, f_, t_ = (int(v) for v in torch.unravel_index(bn.abs().argmin(), bn.shape))
            assert float(bn[b_, f_, t_].abs()) < 2 * 1.2e-7 and t_ >= 1, (float(bn[b_, f_, t_]), t_)
            dz = torch.autograd.grad(lossv, taps[f"dec{d}.out"], retain_graph=True)[0][b_, c, f_, t_ - 1]      # (frame 0 of the T + 1 buffer is dropped behind the PReLU)
            other = ref.clone()
            other[c] += (1 - float(Pg[f"decoder.{d}.2.weight"])) * float(dz) * (1 if float(bn[b_, f_, t_]) <= 0 else -1)
            report[k + " (oracle's branch)"] = e
            e = min(e, rel_err(got[k], other))
        report[k] = e
        worst = max(worst, e)
        # PReLU slope gradients are one scalar summed over a whole layer with heavy cancellation.  encoder.0.1.bias: on
        # this input ONE pre-activation of channel 1 lies within 1e-6 of zero, so the PReLU branch (and with it one
        # term of the bias gradient) is decided by the last bit of the STFT (A/B: FFT vs framing GEMM moves only this entry)
        tol = 2e-3 if k.endswith(".2.weight") else 1e-2 if k == "encoder.0.1.bias" else 2e-4
        if bars and k in bars:
            tol = bars[k]
        assert e < tol, (k, e)
        assert float(ref.abs().max()) == 0.0 or float(got[k].abs().max()) > 0.0, (k, "exactly zero", float(ref.abs().max()))
    print("worst relative gradient error", worst)
    return report


def crn_config(kw):
    from oracle.crn import CRNConfig
    n = len(kw["kernel_num"])
    D = (kw.get("fft_len", 512) // 2) >> n
    return CRNConfig(rnn_input_size=D * (kw["kernel_num"][-1] // 2), **{k: v for k, v in kw.items() if k in ("kernel_num", "rnn_units", "win_len", "win_inc", "fft_len", "masking_mode", "skip_type")})


def check_crn_plan_vs_oracle(kw, B, L, bars=None, report=None, params=None):
    """The CRN counterpart (mask mode, SI-SNR on the waveform): Plan(B, L, model="CRN", **kw) on the host simulator against oracle/crn.py, same bars;
    params: as in check_dccrn_plan_vs_oracle."""
    from oracle.crn import crn_forward, crn_state_shapes
    cfg = crn_config(kw)
    kn = tuple(cfg.kernel_num)
    n = len(kn)
    P = formula_state_dict(crn_state_shapes(cfg)) if params is None else params
    plan = Plan(B, L, model="CRN", **kw)
    want = [(k, tuple(v)) for k, v in crn_state_shapes(cfg).items() if is_trainable(k)]
    assert [(k, shp) for k, (off, shp) in plan.params.items()] == want
    T, NF = plan.T, plan.NF
    Lout = frames_span(L, cfg.win_len, cfg.win_inc)
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, P)
    x, y = make_signals(B, L)
    plan.io(ar, "wav", (B, L)).copy_(x)
    plan.io(ar, "tgt", (B, L)).copy_(y)
    sim_run(plan, PHASE_FWD, ar)
    report = {} if report is None else report
    Pg = {k: (v.clone().requires_grad_(True) if is_trainable(k) else v.clone()) for k, v in P.items()}
    taps = {}
    (est_mags, tmags, wav), new_stats = crn_forward(Pg, x, y, cfg, train=True, taps=taps)
    assert wav.shape == (B, Lout), (wav.shape, Lout)
    ch = (1,) + tuple(k // 2 for k in kn)
    F = [(cfg.fft_len // 2) >> i for i in range(n + 1)]
    for i in range(n):
        got = act_to_nchw(plan.view(ar, f"enc{i}.y"), B, T, F[i + 1], ch[i + 1])
        assert rel_err(got, taps[f"enc{i}.conv"]) < 2e-5, f"enc{i}.conv"
    for d in range(n):
        idx = n - d
        got = act_to_nchw(plan.view(ar, f"dec{d}.y"), B, T + 1, 2 * F[idx], ch[idx - 1])
        assert rel_err(got, taps[f"dec{d}.conv"]) < 5e-5, f"dec{d}.conv"
    out_wav = plan.io(ar, "out_wav", (B, L))
    report["out_wav"] = rel_err(out_wav[:, :Lout], wav)
    assert report["out_wav"] < 5e-5
    assert float(out_wav[:, Lout:].abs().max()) == 0.0 if Lout < L else True
    assert rel_err(plan.io(ar, "out_real", (B, NF, T)), est_mags) < 5e-5
    assert rel_err(plan.io(ar, "out_imag", (B, NF, T)), tmags) < 5e-5
    got_state = read_params(plan, ar, ARENA_STATE, plan.state)
    for k, v in new_stats.items():
        assert rel_err(got_state[k], v) < 1e-5, k
    lossv = main_loss("SI-SNR", wav, y[:, :Lout])
    names = [k for k in Pg if is_trainable(k)]
    grads = dict(zip(names, torch.autograd.grad(lossv, [Pg[k] for k in names], retain_graph=True)))
    gw = torch.autograd.grad(lossv, wav)[0]
    plan.io(ar, "grad_wav", (B, L))[:, :Lout].copy_(gw)
    if Lout < L:
        plan.io(ar, "grad_wav", (B, L))[:, Lout:].copy_(_tail_noise(B, L - Lout))
    sim_run(plan, PHASE_BWD, ar)
    got = read_params(plan, ar, ARENA_GRAD)
    for k in names:
        if k.endswith("conv.bias") and not k.startswith(f"decoder.{n - 1}."):
            assert got[k].abs().max() < 1e-4 * grads[k.replace(".bias", ".weight")].abs().max() + 1e-7, k
            continue
        report[k] = rel_err(got[k], grads[k])
        tol = 2e-3 if k.endswith(".2.weight") else 2e-4
        if bars and k in bars:
            tol = bars[k]
        assert report[k] < tol, (k, report[k])
        assert float(grads[k].abs().max()) == 0.0 or float(got[k].abs().max()) > 0.0, (k, "exactly zero", float(grads[k].abs().max()))
    return report


def check_fsn_plan_vs_oracle(seq, norm, params=None, report=None):
    """FullSubNet (hidden sizes 128 / 64, B = 2, 6000 samples, keep 1) on the host simulator against oracle/fullsubnet.py: the complex ratio mask to
    2e-5, every gradient to 2e-4 (max-abs over max-abs); params: as in check_dccrn_plan_vs_oracle."""
    from oracle.fullsubnet import FSNConfig, fsn_forward, fsn_state_shapes, fsn_targets
    hid = (128, 64)
    cfg = FSNConfig(fb_hidden=hid[0], sb_hidden=hid[1], sequence_model=seq, norm_type=norm)
    P = formula_state_dict(fsn_state_shapes(cfg)) if params is None else params
    B, L = 2, 6000
    x, y = make_signals(B, L)
    mag, cirm = fsn_targets(x, y, cfg)
    T = mag.shape[-1]
    plan = Plan(B, T, model="FullSubNet", fsn=dict(fb_hidden=hid[0], sb_hidden=hid[1], keep=1.0, sequence_model=seq, norm_type=norm))
    assert [(k, shp) for k, (off, shp) in plan.params.items()] == [(k, tuple(v)) for k, v in fsn_state_shapes(cfg).items()]
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, P)
    plan.io(ar, "mag", (B, 257, T)).copy_(mag)
    sim_run(plan, PHASE_FWD, ar)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    crm = fsn_forward(Pg, mag, cfg)
    report = {} if report is None else report
    report["crm"] = rel_err(plan.io(ar, "crm", (B, 257, T, 2)), crm)
    assert report["crm"] < 2e-5
    loss = torch.mean((cirm - crm) ** 2)
    names = list(Pg)
    grads = dict(zip(names, torch.autograd.grad(loss, [Pg[k] for k in names], retain_graph=True)))
    plan.io(ar, "grad_crm", (B, 257, T, 2)).copy_(torch.autograd.grad(loss, crm)[0])
    sim_run(plan, PHASE_BWD, ar)
    got = read_params(plan, ar, ARENA_GRAD)
    for k in names:
        report[k] = rel_err(got[k], grads[k])
        assert report[k] < 2e-4, (k, report[k])
    return report


# ================================================================================================ GPU: device against simulator, op by op
KIND = {1: "RUNGEMM", 2: "WGRAD", 3: "PACK", 4: "UNPACK", 5: "BN_FINALIZE", 6: "BN_APPLY", 7: "BN_BWD_REDUCE", 8: "BN_BWD_APPLY",
        9: "LSTM_FWD", 10: "LSTM_BWD", 11: "COMBINE_FWD", 12: "COMBINE_BWD", 13: "MASK_FWD", 14: "MASK_BWD", 15: "OLA_FWD",
        16: "OLA_BWD", 17: "SPECOUT_FWD", 18: "SPECOUT_BWD", 19: "MEMSET", 20: "SPLITSUM", 21: "BN_BWD_FINALIZE", 22: "MAGS", 23: "CELL_FWD", 24: "CELL_BWD", 25: "DROPOUT_FWD", 26: "DROPOUT_BWD", 27: "FSN_IN", 28: "FSN_SCALE", 29: "FSN_SBSUM",
        30: "FSN_SBBUILD", 31: "FSN_OUT", 32: "FSN_OUT_BWD", 33: "FSN_SBBWD_SUM", 34: "FSN_SBBWD_APPLY", 35: "REFLECTPAD"}


def report_path(name):
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, name)


def seed_inputs(plan, dev, P, model, B, L):
    """The inputs and upstream gradients of the models this driver knows, from fixed seeds."""
    torch.manual_seed(1)
    if model == "FullSubNet":
        plan.io(dev, "mag", (B, 257, L)).copy_(torch.rand(B, 257, L) * 3)
        plan.io(dev, "grad_crm", (B, 257, L, 2)).copy_(torch.randn(B, 257, L, 2) * 1e-3)
        plan.set_seed(dev, 77)
    elif model == "SequenceModel":
        from seqmodel_common import time_major
        I, O = P["sequence_model.weight_ih_l0"].shape[1], P["fc_output_layer.weight"].shape[0]
        xt = time_major(torch.rand(B, I, L) * 6)
        plan.io(dev, "x", tuple(xt.shape)).copy_(xt)
        plan.io(dev, "grad_y", (L, B, O)).copy_(torch.randn(L, B, O) * 1e-3)
        plan.set_seed(dev, 77)
    else:
        x, y = make_signals(B, L)
        plan.io(dev, "wav", (B, L)).copy_(x)
        if model == "CRN":
            plan.io(dev, "tgt", (B, L)).copy_(y)
        plan.io(dev, "grad_wav", (B, L)).copy_(torch.randn(B, L) * 1e-3)
        plan.io(dev, "grad_real", (B, plan.NF, plan.T)).copy_(torch.randn(B, plan.NF, plan.T) * 1e-4)
        plan.io(dev, "grad_imag", (B, plan.NF, plan.T)).copy_(torch.randn(B, plan.NF, plan.T) * 1e-4)


def ops_device_vs_sim(plan, P, model, B, L, dtype, per_element=False, seed=None, report=None):
    """Run every op of both phases of `plan` on the device and on the host simulator from the SAME pre-op state (so an error is localised to
    one launch) and detect writes outside what the simulator's op changes.  P: {state_dict name: tensor}; model: DCCRN / DCCRN_CBN / CRN /
    FullSubNet / SequenceModel (L = frames), seeded by seed_inputs; seed: a callable (plan, device arenas) that writes the plan's inputs and upstream
    gradients instead (a plan seed_inputs does not know; model, B and L are then unused).
    The comparison rule is opcheck.compare_op.  Bars: fp32 buffers 1e-3 and bf16 buffers 1.6e-2 (two bf16 ulps), relative to the largest element of the
    BUFFER; every tensor of the gradient and the state arena on its own, 1e-3 relative to the largest element of the TENSOR (two named exceptions:
    opcheck), and a byte the device changes in a tensor the simulator leaves alone is a stray write; the weight-gradient partial sums (`gradpart`) launch
    by launch, 1e-3 relative to the largest partial sum the launch writes; fp32 state of a bf16 recurrence op and the fp32
    `.bnpart` sums of a bf16 GEMM 4e-3.  per_element (the cases with saturating gate biases only): a buffer or tensor whose largest element exceeds 1 is
    measured per element, |device - simulator| <= tol * max(1, |simulator|) with the same tol - a bias of 100 in a pre-activation slab or a cell state
    of 10 must not loosen the bar of every other element of its region.
    report: file name in the report directory (report_path) that receives the report lines followed by the per-tensor table (tensor, max|simulator|, worst err over the run).
    Returns (report lines, the lines of the ops that miss)."""
    dev = plan.alloc_arenas("cuda")
    host = plan.alloc_arenas("cpu")
    fill_params(plan, dev, P)
    if seed is not None:
        seed(plan, dev)
    else:
        seed_inputs(plan, dev, P, model, B, L)
    # region table: (arena, byte offset, bytes, dtype, name); GRAD / STATE arenas are single fp32 regions here (change detection and transport) and
    # are split per tensor by the comparator
    table = opcheck.region_table(plan)
    check = [0, 2, 3, 5]
    # The arenas stay on the device.  `host` receives the simulator's op, `got` mirrors the device state and `prev` is the state in front of the op
    # (all three equal at every op boundary); after an op only the regions that the kernel or the simulator changed travel (device -> host), so the
    # per-op cost is one device-side compare + one host-side memcmp instead of ten whole-arena copies.
    for a in range(6):
        host[a].copy_(dev[a])
    prev = {a: host[a].clone() for a in check}
    got = {a: host[a].clone() for a in check}
    by_arena = {a: [(k, r) for k, r in enumerate(table.regions) if r[0] == a and r[2] > 0] for a in check}
    # 8-byte words: every region starts on a 256-byte boundary, so a word never straddles two regions
    w64 = {a: (dev[a].view(torch.uint8).numel() // 8) for a in check}
    lo_idx = {a: torch.tensor([r[1] // 8 for _, r in by_arena[a]], device="cuda") for a in check}
    hi_idx = {a: torch.tensor([min((r[1] + r[2] + 7) // 8, w64[a]) for _, r in by_arena[a]], device="cuda") for a in check}
    # host side: which regions did the SIMULATOR change?  One vectorised pass per arena (words -> 256-byte blocks -> prefix sums; regions start on
    # 256-byte boundaries, so a block never straddles two regions) instead of one memcmp per region and op (28 000 torch.equal calls per case: half of the
    # suite's run time through round 5)
    nblk = {a: (w64[a] + 31) // 32 for a in check}
    lo_blk = {a: torch.tensor([r[1] // 256 for _, r in by_arena[a]]) for a in check}
    hi_blk = {a: torch.tensor([min((r[1] + r[2] + 255) // 256, nblk[a]) for _, r in by_arena[a]]) for a in check}

    def host_changed(a):
        h64 = host[a].view(torch.uint8)[:w64[a] * 8].view(torch.int64)
        p64 = prev[a].view(torch.uint8)[:w64[a] * 8].view(torch.int64)
        ne = h64 != p64
        if ne.numel() % 32:
            ne = torch.cat([ne, torch.zeros(32 - ne.numel() % 32, dtype=torch.bool)])
        cs = torch.cat([torch.zeros(1, dtype=torch.int64), ne.view(-1, 32).any(1).to(torch.int64).cumsum(0)])
        return ((cs[hi_blk[a]] - cs[lo_blk[a]]) > 0).tolist()
    lines, bad, log = [], [], opcheck.TensorLog()
    for phase in (PHASE_FWD, PHASE_BWD):
        kinds, tags = plan.op_kinds(phase)
        for i in range(plan.num_ops(phase)):
            dbefore = {a: dev[a].view(torch.uint8)[:w64[a] * 8].view(torch.int64).clone() for a in check}
            sim_run(plan, phase, host, i, i + 1)
            plan.run(phase, dev, 0, i, i + 1)
            changed = []                                                              # [(region index, the device changed it)]
            for a in check:
                if not by_arena[a]:
                    continue
                d64 = dev[a].view(torch.uint8)[:w64[a] * 8].view(torch.int64)
                cs = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"), (d64 != dbefore[a]).to(torch.int32)]), 0)
                dflags = ((cs[hi_idx[a]] - cs[lo_idx[a]]) > 0).cpu().tolist()        # the one synchronising read per arena
                hflags = host_changed(a)
                g8, d8 = got[a].view(torch.uint8), dev[a].view(torch.uint8)
                for (k, (ra, off, nb, dt, name)), dchg, hchg in zip(by_arena[a], dflags, hflags):
                    if dchg:
                        g8[off:off + nb].copy_(d8[off:off + nb])
                    if hchg or dchg:
                        changed.append((k, dchg))
            v = opcheck.compare_op(prev, host, got, table, int(kinds[i]), dtype, per_element, candidates=[k for k, _ in changed])
            log.add(v)
            for k, dchg in changed:
                a, off, nb, dt, name = table.regions[k]
                g8 = got[a].view(torch.uint8)[off:off + nb]
                host[a].view(torch.uint8)[off:off + nb].copy_(g8)                     # all host copies := device state
                if dchg:
                    prev[a].view(torch.uint8)[off:off + nb].copy_(g8)
            lines.append(f"phase {phase} op {i:3d} {KIND.get(int(kinds[i]), str(int(kinds[i]))):16s} tag {int(tags[i]):4d} elems {v.elems:9d} "
                         f"err/tol {v.worst:.3e} stray {v.stray} {v.where}")
            if not (v.worst < 1.0) or v.stray:
                bad.append(lines[-1])
    if report:
        with open(report_path(report), "w") as f:
            f.write("\n".join(lines + log.lines()) + "\n")
    return lines, bad
