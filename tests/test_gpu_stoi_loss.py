"""GPU tier of the STOI / ESTOI loss: the extended correlate stage and the backward kernels of csrc/stoi.hip (sefd_stoi_gpu_ex,
sefd_stoi_backward) through tools_for_estimate.stoi_batch, torch.ops.sefd.stoi and tools_for_loss.stoi_loss, against the host scorer and the
float64 references of tests/stoi_loss_ref.py (pinned and fenced in tests/test_stoi_loss_cpu.py).  Gradients are held per row to
|g - ref| <= 2^-23 |ref| + 1e-9 max|ref|: the one fp32 rounding of the store, doubled, plus the project's 1e-9 STOI bar scaled by the row's
largest gradient for the fp64 summation order.  Clips are about 1 s long."""
import numpy as np
import pytest
import torch

import stoi_cases as sc
import stoi_loss_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture()
def te():
    import sefd_amd  # noqa: F401
    from sefd_amd import ops, tools_for_estimate  # noqa: F401
    tools_for_estimate.build()
    return tools_for_estimate


@pytest.fixture()
def tfl():
    import sefd_amd  # noqa: F401
    from sefd_amd import ops, tools_for_loss  # noqa: F401
    return tools_for_loss


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(np.atleast_2d(a))).cuda()


def _host(te, clean, est, fs, extended):
    c, e = np.ascontiguousarray(np.atleast_2d(clean), np.float32), np.ascontiguousarray(np.atleast_2d(est), np.float32)
    out = np.zeros(c.shape[0])
    assert te.lib().sefd_stoi_batch_ex(c.ctypes.data, e.ctypes.data, c.shape[0], c.shape[1], fs, int(extended), out.ctypes.data, 0) == 0
    return out


def _op_grad(clean, est, fs, extended, weights):
    """(scores, gradient of sum_b weights[b] d_b) through torch.ops.sefd.stoi's registered autograd."""
    E = _cuda(est).requires_grad_()
    d = torch.ops.sefd.stoi(_cuda(clean), E, fs, extended)
    (d * torch.from_numpy(np.asarray(weights, np.float64)).cuda()).sum().backward()
    return d.detach().cpu().numpy(), E.grad.cpu().numpy()


def _check_rows(got, want, tag):
    """Per row the bound of ref.grad_bound; exact zeros wherever the reference has them.  Prints the worst value of each term."""
    assert got.dtype == np.float32 and got.shape == want.shape and np.all(np.isfinite(got))
    worst_abs = worst_rel = worst_ratio = worst_beyond = 0.0
    for g, w in zip(np.atleast_2d(got), np.atleast_2d(want)):
        err, big = np.abs(g.astype(np.float64) - w), np.abs(w) >= 1e-3 * np.abs(w).max()
        worst_abs = max(worst_abs, float(err.max() / np.abs(w).max()))
        worst_rel = max(worst_rel, float((err[big] / np.abs(w[big])).max()))
        worst_ratio = max(worst_ratio, float((err / ref.grad_bound(w)).max()))
        worst_beyond = max(worst_beyond, float(np.abs(g.astype(np.float64) - w.astype(np.float32)).max() / np.abs(w).max()))
    print(f"\n{tag}: worst |g - ref| / max|ref| {worst_abs:.3e} (bar 1e-9 beside the rounding term), worst |g - ref| / |ref| where "
          f"|ref| >= 1e-3 max {worst_rel:.3e} (2^-23 = {2.0 ** -23:.3e}), worst error / bound {worst_ratio:.3f}, worst |g - fp32(ref)| / max|ref| {worst_beyond:.3e}")
    for g, w in zip(np.atleast_2d(got), np.atleast_2d(want)):
        assert np.all(g[w == 0.0] == 0.0)
        assert np.all(np.abs(g.astype(np.float64) - w) <= ref.grad_bound(w)), tag


# ------------------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("fs", sc.RATES)
def test_estoi_scores_equal_host_and_numpy(te, fs):
    clean, est = sc.speechlike_case(fs + 123)
    got = te.stoi_batch(_cuda(clean), _cuda(est), fs, extended=True).cpu().numpy()
    host = _host(te, clean, est, fs, True)
    want = np.array([ref.estoi_numpy(clean[i], est[i], fs) for i in range(4)])
    print(f"\nestoi fs={fs}: max |gpu - host| {np.abs(got - host).max():.3e}  max |gpu - numpy| {np.abs(got - want).max():.3e}")
    assert np.all(np.abs(got - host) <= TOL) and np.all(np.abs(got - want) <= TOL), (got, host, want)
    assert torch.equal(torch.ops.sefd.stoi(_cuda(clean), _cuda(est), fs, True), te.stoi_batch(_cuda(clean), _cuda(est), fs, True))


def test_estoi_floor_and_plain_scores_through_the_flagged_entry(te):
    clean, est = ref.edge_pair(4096)
    assert te.stoi_batch(_cuda(clean), _cuda(est), 10000, extended=True).item() == 1e-5
    one = te.stoi_batch(_cuda(ref.edge_pair(4097)[0]), _cuda(ref.edge_pair(4097)[1]), 10000, extended=True).item()
    assert abs(one - ref.estoi_numpy(*ref.edge_pair(4097), 10000)) <= TOL
    for fs in (16000, 10000):
        clean, est = sc.speechlike_case(fs + 123)
        C, E = _cuda(clean), _cuda(est)
        plain = te.stoi_batch(C, E, fs)
        for flags in (0, te.STOI_KEEP):                        # flags 0 and the keep bit alone: sefd_stoi_gpu's bits
            assert torch.equal(te.stoi_forward_raw(C, E, fs, flags)[0], plain), (fs, flags)
        ext = te.stoi_batch(C, E, fs, extended=True)
        assert torch.equal(te.stoi_forward_raw(C, E, fs, te.STOI_EXTENDED | te.STOI_KEEP)[0], ext) and not torch.equal(ext, plain)


# ------------------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("fs", sc.RATES)
def test_gradient_equals_reference(te, fs, extended):
    clean, est, d, grad, _ = ref.speech_reference(fs, extended)
    got_d, got = _op_grad(clean, est, fs, extended, ref.WEIGHTS)
    assert np.all(np.abs(got_d - d) <= TOL)
    assert np.all((grad == 0.0).mean(axis=1) > 0.05)            # the interior of the pause: exact zeros, checked in _check_rows
    _check_rows(got, grad, f"stoi grad fs={fs} extended={extended}")


@pytest.mark.parametrize("extended", [False, True])
def test_smallest_shapes(te, tfl, extended):
    """10 kHz, every frame kept.  4096 samples: 30 frames, 29 after the compaction, floored.  4097: exactly one segment.  4225: two overlapping
    segments; the second half of the last kept frame (the last 128 compacted samples) and the sample past it are outside every frame."""
    clean, est = ref.edge_pair(4096)
    E = _cuda(est).requires_grad_()
    loss = tfl.stoi_loss(_cuda(clean), E, 10000, extended)
    loss.backward()
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.item() == np.float32(1 - 1e-5)
    assert E.grad.shape == (1, 4096) and not E.grad.any()
    for L in (4097, 4225):
        clean, est, d, grad, _ = ref.edge_reference(L, extended)
        kept = len(range(0, L - 256, 128))
        assert not grad[(kept - 1) * 128 + 128:].any() and grad[(kept - 1) * 128 + 127] != 0.0
        got_d, got = _op_grad(clean, est, 10000, extended, [1.0])
        assert abs(got_d[0] - d) <= TOL
        _check_rows(got[0], grad, f"stoi grad edge L={L} extended={extended}")


@pytest.mark.parametrize("extended", [False, True])
def test_degenerate_inputs(tfl, extended):
    fs = 16000
    clean, est = sc.speechlike_case(fs + 123)
    zero = np.zeros_like(clean)
    for c, e, zero_grad in ((clean, zero, True), (zero, est, True), (zero, zero, True), (clean, clean, False)):
        E = _cuda(e).requires_grad_()
        loss = tfl.stoi_loss(_cuda(c), E, fs, extended)
        loss.backward()
        assert torch.isfinite(loss) and bool(torch.isfinite(E.grad).all()), (extended, float(loss))
        if zero_grad:                                           # est = 0: every envelope is 0 (zero rule); clean = 0: the cotangent itself is 0
            assert not E.grad.any()
        else:
            assert abs(float(loss.detach())) <= TOL
            d = torch.ops.sefd.stoi(_cuda(c), _cuda(e), fs, extended)
            assert float((1 - d).abs().max()) <= TOL


def _five(fs=16000, n=16000 + 123):
    """Five rows with different kept-frame counts; row 3 is silent but for a burst of 20 frames: floored."""
    clean = np.concatenate([sc.speechlike(1, n, seed=60 + i) for i in range(5)])
    for i in range(5):
        clean[i, 700 + 300 * i:1500 + 900 * i] *= 5e-4
    clean[3, 4300:] = 0.0
    kept = [sc.silence_margin_db(clean[i], fs)[1] for i in range(5)]
    assert len(set(kept)) == 5 and kept[3] < 31 and min(kept[:3] + kept[4:]) > 31, kept
    for i in range(5):
        assert sc.silence_margin_db(clean[i], fs)[0] >= sc.MIN_MARGIN_DB
    est = (clean + 0.02 * np.random.default_rng(61).standard_normal(clean.shape)).astype(np.float32)
    return clean, est


@pytest.mark.parametrize("extended", [False, True])
def test_deterministic_and_batch_independent(te, extended):
    fs = 16000
    clean, est = _five(fs)
    w = [1.0, 0.5, -2.0, 3.0, 0.125]
    d0, g0 = _op_grad(clean, est, fs, extended, w)
    d1, g1 = _op_grad(clean, est, fs, extended, w)
    assert np.array_equal(d0.view(np.uint64), d1.view(np.uint64)) and np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    assert d0[3] == 1e-5 and not g0[3].any() and all(g0[i].any() for i in (0, 1, 2, 4))
    for i in (0, 2, 4):
        da, ga = _op_grad(clean[i], est[i], fs, extended, [w[i]])
        assert np.array_equal(da.view(np.uint64), d0[i:i + 1].view(np.uint64)) and np.array_equal(ga[0].view(np.uint32), g0[i].view(np.uint32)), i
    # a non-contiguous view of the estimate
    C = _cuda(clean)
    wide = torch.ones(5, 2 * est.shape[1], device="cuda")
    wide[:, ::2] = _cuda(est)
    wide.requires_grad_()
    view = wide[:, ::2]
    assert not view.is_contiguous()
    d = torch.ops.sefd.stoi(C, view, fs, extended)
    (d * torch.tensor(w, dtype=torch.float64, device="cuda")).sum().backward()
    assert np.array_equal(wide.grad[:, ::2].cpu().numpy().view(np.uint32), g0.view(np.uint32)) and not wide.grad[:, 1::2].any()


def test_several_forwards_before_their_backwards(tfl):
    fs = 16000
    clean, est = sc.speechlike_case(fs + 123)
    C = _cuda(clean)
    alone = []
    for extended, scale in ((False, 1.0), (True, 1.0), (False, 0.5)):
        E = _cuda(est * np.float32(scale)).requires_grad_()
        tfl.stoi_loss(C, E, fs, extended).backward()
        alone.append(E.grad.clone())
    Es = [_cuda(est * np.float32(s)).requires_grad_() for s in (1.0, 1.0, 0.5)]
    losses = [tfl.stoi_loss(C, E, fs, x) for E, x in zip(Es, (False, True, False))]     # each holds its own workspace
    for loss in reversed(losses):
        loss.backward()
    for E, a in zip(Es, alone):
        assert torch.equal(E.grad, a)
    assert not torch.equal(alone[0], alone[1]) and not torch.equal(alone[0], alone[2])


def test_loss_value_weight_and_upstream_scale(tfl):
    from sefd_amd import config as cfg
    fs = 16000
    clean, est = sc.speechlike_case(fs + 123)
    C = _cuda(clean)
    res = {}
    old = cfg.stoi_loss_weight
    try:
        for weight in (1.0, 2.0):
            cfg.stoi_loss_weight = weight
            for extended in (False, True):
                E = _cuda(est).requires_grad_()
                loss = tfl.stoi_loss(C, E, fs, extended)
                loss.backward()
                res[weight, extended] = (loss.detach(), E.grad.clone())
    finally:
        cfg.stoi_loss_weight = old
    for extended in (False, True):
        d = ref.speech_reference(fs, extended)[2]
        l1, g1 = res[1.0, extended]
        assert l1.dtype == torch.float32 and abs(float(l1) - (1 - d.mean())) <= 1e-7
        l2, g2 = res[2.0, extended]
        assert torch.equal(l2, 2 * l1) and torch.equal(g2, 2 * g1)               # the weight doubles the term and its gradient exactly
        # against the reference: d loss / d est = -weight / B * d (sum_b d_b) / d est
        _, _, _, grad, _ = ref.speech_reference(fs, extended)
        want = -grad / ref.WEIGHTS[:, None] / 4
        _check_rows(g1.cpu().numpy(), want, f"stoi_loss grad extended={extended}")
    E = _cuda(est).requires_grad_()
    (tfl.stoi_loss(C, E, fs) * 0.5).backward()
    assert torch.equal(E.grad, 0.5 * res[1.0, False][1])
    with pytest.raises(ValueError):
        tfl.stoi_loss(C, _cuda(est)[:, :-1], fs)
    with pytest.raises(NotImplementedError, match="`clean` requires a gradient"):
        tfl.stoi_loss(C.clone().requires_grad_(), _cuda(est), fs)


# ------------------------------------------------------------------------------------------------------------ training
def _small_dccrn_cfg(perceptual):
    from sefd_amd import config as cfg
    old = (cfg.perceptual, cfg.loss, cfg.masking_mode, list(cfg.dccrn_kernel_num), cfg.act_dtype)
    cfg.perceptual, cfg.loss, cfg.masking_mode, cfg.dccrn_kernel_num, cfg.act_dtype = perceptual, "SI-SNR", "E", [16, 32, 32, 64, 64, 64], "fp32"
    return old


def _restore(old):
    from sefd_amd import config as cfg
    cfg.perceptual, cfg.loss, cfg.masking_mode, cfg.dccrn_kernel_num, cfg.act_dtype = old


@pytest.mark.parametrize("perceptual", ["STOI", "ESTOI"])
def test_fused_train_step_with_stoi_equals_autograd_route(perceptual):
    """The bars of tests/test_gpu_pmsqe.py::test_fused_train_step_with_perceptual_equals_autograd_route, its small DCCRN, 1 s clips."""
    import sefd_amd  # noqa: F401
    from sefd_amd import models
    from sefd_amd.optim import Adam
    from test_oracle_pmsqe import speechlike
    old = _small_dccrn_cfg(perceptual)
    try:
        c, n = speechlike(3, seconds=1, seed=31)
        c, n = c.cuda(), n.cuda()
        res = []
        for fused in (False, True):
            torch.manual_seed(0)
            m = models.DCCRN(rnn_units=64, masking_mode="E").to("cuda").train()
            opt = Adam(m.parameters(), lr=1e-3)
            for _ in range(2):
                if fused:
                    loss = m.train_step(n, c, opt, perceptual=perceptual)
                else:
                    real, imag, out = m(n)
                    loss = (m.loss(out, c) + m.loss(out, c, real, imag, perceptual=True)) / 2
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
            res.append((float(loss.detach()), torch.cat([p.detach().flatten() for p in m.parameters()]).cpu()))
        assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[0][0])
        assert float((res[0][1] - res[1][1]).norm() / res[0][1].norm()) < 1e-5
        main, perc = m._last_loss_parts
        assert 0.0 < float(perc) < 1.0                          # 1 - STOI of a scored batch, not the floor
    finally:
        _restore(old)


@pytest.mark.parametrize("perceptual", ["STOI", "ESTOI"])
def test_dccrn_perceptual_steps_with_stoi_lower_the_loss(perceptual):
    import sefd_amd  # noqa: F401
    from sefd_amd import models
    from sefd_amd.optim import Adam
    from test_oracle_pmsqe import speechlike
    old = _small_dccrn_cfg(perceptual)
    try:
        torch.manual_seed(0)
        m = models.DCCRN(rnn_units=64, masking_mode="E").to("cuda").train()
        opt = Adam(m.parameters(), lr=1e-3)
        c, n = speechlike(4, seconds=1, seed=21)
        c, n = c.cuda(), n.cuda()
        hist = []
        for _ in range(6):
            opt.zero_grad()
            real, imag, out = m(n)
            loss = (m.loss(out, c) + m.loss(out, c, real, imag, perceptual=True)) / 2
            loss.backward()
            opt.step()
            hist.append(float(loss))
        assert all(map(lambda v: v == v, hist)) and hist[-1] < hist[0], hist
    finally:
        _restore(old)
