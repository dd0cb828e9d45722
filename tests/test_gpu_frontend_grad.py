"""GPU tier of the gradient case table (frontend_grad_cases.py): the backward passes of tools.stft, tools.istft, tools.mag_phase and
tools.build_complex_ideal_ratio_mask through their public signatures with torch.autograd.grad / loss.backward(), against float64 torch autograd, at
bars made of float32 torch autograd on the CPU (test_frontend_grad_cpu.py computes them) - never of the code under test.  Every figure is printed and
written to the report directory before it is asserted.

Measured on the MI355X (the float32-alone figures are torch on that host's CPU):
  stft     kernel 0.72 .. 1.47 x float32 torch autograd alone (1.13e-7 .. 1.75e-7), worst 0.37 of its bar
  istft    K_ref 0.380, K 1.52; kernel 0.22 .. 0.31 on the cases K_ref is taken from (torch 0.24 .. 0.38), 0.32 .. 1.27 on the tail lengths 6190 / 6199 (torch 0.40 .. 1.31),
           1.24 on the one-frame case (torch 2.05; 1.59 when OLA_BWD divided by the rounded envelope instead of multiplying by the float-pair reciprocal);
           through (mag, phase): g_mag <= 0.45, g_phase <= 0.63 of the K-part of their bound
  targets  n = 4194561: every arm of every gradient within its bar, worst 0.46 of it (cirm_noisy on pos_real: kernel 2.13, torch 1.15); mag_phase 2.3 .. 2.9 on the large
           arms (torch 2.4 .. 2.6); the cIRM on the arms that hold v ~ -98 bins: torch 1.8e2 .. 5.4e2 (its quotient rule cancels there), the kernel <= 3.7
  recipe   |cRM| 1.14, loss 2.046449 (float64 2.046450), kappa 1.1, d loss / d cRM 9.9e-7 of the largest element (bar 6.0e-6); with the formula weights' |cRM| ~ 1e-3
           the same comparison measured 7.1e-5: float32 decompress_cIRM's own forward error at small masks, not the kernels'
  the whole file: 51 tests in 9 s
"""
import ctypes as C

import pytest
import torch

import frontend_cases as fc
import frontend_grad_cases as gc

pytestmark = pytest.mark.gpu


def _tools():
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_model as tools
    return tools


def _report(name, lines):
    from plan_check import report_path
    print("\n".join(lines))
    with open(report_path(name), "a") as f:
        f.write("\n".join(lines) + "\n")


def _geom(c):
    return dict(n_fft=fc.NFFT, hop_length=c.hop, win_length=c.win)


# ------------------------------------------------------------------------------------------ stft
def _stft_grad(tools, c, x, g):
    x = x.requires_grad_(True)
    S = tools.stft(x, c.nfft, c.hop, c.win)
    assert S.dtype == torch.complex64 and S.requires_grad
    return torch.autograd.grad(S, x, g)[0]


@pytest.mark.parametrize("case", gc.STFT_GRAD_CASES, ids=fc.stft_id)
def test_stft_gradient_against_float64(case):
    """Max-norm error over the largest float64 element <= max(2e-7, 4 x float32 torch autograd alone); the gradient has the input's dtype and shape."""
    tools = _tools()
    r = gc.stft_grad_reference(case)
    got = _stft_grad(tools, case, fc.stft_input(case).cuda(), gc.stft_cotangent(case).cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (case.B, case.L) and torch.isfinite(got).all()
    err = gc.grad_err(got.cpu(), r.grad)
    _report("frontend_gpu_grad_stft.txt", [f"{fc.stft_id(case)}: float32 torch autograd alone {r.alone:.3e} bar {r.bar:.3e} kernel {err:.3e} = {err / r.alone:.2f} x alone, "
                                           f"{err / r.bar:.2f} of the bar"])
    assert err <= r.bar, (err, r.bar)


@pytest.mark.parametrize("case", gc.STFT_REFUSED_CASES, ids=fc.stft_id)
def test_stft_refuses_a_gradient_at_other_transform_sizes_at_the_forward_call(case):
    """n_fft 256 / 1024: one sentence, NotImplementedError, at the forward call; without a gradient (or under no_grad) the forward runs as before."""
    tools = _tools()
    x = fc.stft_input(case).cuda()
    plain = tools.stft(x, case.nfft, case.hop, case.win)
    xg = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match=rf"n_fft 512 only .* got n_fft {case.nfft}") as ei:
        tools.stft(xg, case.nfft, case.hop, case.win)
    assert "\n" not in str(ei.value)
    with torch.no_grad():
        assert torch.equal(tools.stft(xg, case.nfft, case.hop, case.win), plain)


def test_two_stfts_before_one_backward():
    """stft(noisy), stft(clean), one backward(): nothing is saved from a forward, so the second does not disturb the first."""
    tools = _tools()
    c = fc.StftCase(3, 4801, 512, 300, 400)
    a, b = fc.stft_input(c).cuda().requires_grad_(True), fc.noise(c.B, c.L, 9).cuda().requires_grad_(True)
    g = gc.stft_cotangent(c).cuda()
    Sa, Sb = tools.stft(a, c.nfft, c.hop, c.win), tools.stft(b, c.nfft, c.hop, c.win)
    ((Sa * g.conj()).real.sum() + 2.0 * (Sb * g.conj()).real.sum()).backward()
    one = _stft_grad(tools, c, fc.stft_input(c).cuda(), g)
    assert torch.equal(a.grad, one) and torch.equal(b.grad, 2.0 * one)
    # the gradient comes back in the input's dtype
    xd = fc.stft_input(c).cuda().double().requires_grad_(True)
    gd = torch.autograd.grad(tools.stft(xd, c.nfft, c.hop, c.win), xd, g)[0]
    assert gd.dtype == torch.float64 and torch.equal(gd.float(), one)


# ------------------------------------------------------------------------------------------ istft
def _istft_grads(tools, c, S, gy):
    """Gradients through the complex form and the real-pair form."""
    kw = dict(length=c.L, **_geom(c))
    s = S.clone().requires_grad_(True)
    y = tools.istft(s, **kw)
    assert y.requires_grad and tuple(y.shape) == (c.B, c.L)
    (gc_,) = torch.autograd.grad(y, s, gy)
    sr = torch.view_as_real(S).clone().requires_grad_(True)
    (gr,) = torch.autograd.grad(tools.istft(sr, **kw), sr, gy)
    return gc_, gr


@pytest.mark.parametrize("kind", fc.ISTFT_KINDS)
@pytest.mark.parametrize("case", gc.ISTFT_GRAD_CASES, ids=fc.istft_id)
def test_istft_gradient_against_float64(case, kind):
    """|got - ref64|[k, t] <= K eps32 (c_k / N) A_t, K = 4 x K_ref, tail cases included; complex and real-pair forms bit-identical; Im = 0 at DC and
    Nyquist; through (mag, phase) the same bound taken through the polar adjoint (frontend_grad_cases.polar_reference)."""
    tools = _tools()
    S = gc.istft_spectrum(case, kind).cuda()
    gy = gc.istft_cotangent(case).cuda()
    ref, unit = gc.istft_grad_reference(case, kind)
    g_c, g_r = _istft_grads(tools, case, S, gy)
    assert g_c.dtype == torch.complex64 and tuple(g_c.shape) == tuple(S.shape) and g_r.dtype == torch.float32 and tuple(g_r.shape) == tuple(S.shape) + (2,)
    assert torch.equal(torch.view_as_real(g_c), g_r)
    assert bool((g_c.imag[:, 0] == 0).all()) and bool((g_c.imag[:, -1] == 0).all())
    K = gc.istft_grad_k()
    k = gc.complex_bound_ratio(g_c.cpu(), ref, unit)
    mag, ph, gm_ref, gp_ref, (km, cm), (kp, cp) = gc.polar_reference(case, kind)
    m, p = mag.cuda().requires_grad_(True), ph.cuda().requires_grad_(True)
    gm, gp = torch.autograd.grad(tools.istft((m, p), use_mag_phase=True, length=case.L, **_geom(case)), (m, p), gy)
    dm, dp = (gm.cpu().double() - gm_ref).abs(), (gp.cpu().double() - gp_ref).abs()
    k_m = float(((dm - cm).clamp_min(0) / km.clamp_min(1e-300)).max())
    k_p = float(((dp - cp).clamp_min(0) / kp.clamp_min(1e-300)).max())
    _report("frontend_gpu_grad_istft.txt", [f"{fc.istft_id(case)} {kind}: K_ref {gc.istft_grad_k_reference():.3f} K {K:.3f} kernel {k:.3f} "
                                            f"(float32 torch autograd alone {gc.istft_grad_k_alone(case, kind):.3f}) | through (mag, phase): g_mag {k_m:.3f} g_phase {k_p:.3f}"])
    assert k <= K, (k, K)
    assert gc.polar_bound_ok(gm.cpu(), gm_ref, km, cm, K) and gc.polar_bound_ok(gp.cpu(), gp_ref, kp, cp, K), (k_m, k_p, K)


def test_istft_gradient_of_the_zero_filled_tail_is_zero():
    """(2, 400, 512, 512): one frame covers 256 samples, the clip runs 144 past it.  A cotangent that lives on the tail alone gives exactly 0, and the
    tail's cotangent does not change a bit of the gradient."""
    tools = _tools()
    c = gc.ONE_FRAME_CASE
    S = gc.istft_spectrum(c, "inconsistent").cuda()
    gy = gc.istft_cotangent(c).cuda()
    tail = gy.clone()
    tail[:, :256] = 0.0
    g_tail, _ = _istft_grads(tools, c, S, tail)
    assert bool((torch.view_as_real(g_tail) == 0).all())
    head = gy.clone()
    head[:, 256:] = 0.0
    assert torch.equal(_istft_grads(tools, c, S, head)[0], _istft_grads(tools, c, S, gy)[0])


# ------------------------------------------------------------------------------------------ targets
def _target_grads(tools, noisy, clean, gm, gp, gcirm):
    """(d noisy of mag_phase, d noisy of cIRM, d clean of cIRM) as real pairs [n, 2]."""
    z = noisy.detach().requires_grad_(True)                   # detach, not clone: a view keeps its place in its storage
    (d_mp,) = torch.autograd.grad(tools.mag_phase(z), z, (gm, gp))
    z, c = noisy.detach().requires_grad_(True), clean.detach().requires_grad_(True)
    d_n, d_c = torch.autograd.grad(tools.build_complex_ideal_ratio_mask(z, c), (z, c), gcirm)
    for t in (d_mp, d_n, d_c):
        assert t.dtype == torch.complex64 and tuple(t.shape) == tuple(noisy.shape)
    return tuple(torch.view_as_real(t).cpu() for t in (d_mp, d_n, d_c))


@pytest.mark.parametrize("n", gc.TARGET_GRAD_SIZES)
def test_mag_phase_and_cirm_gradients_against_float64(n):
    """sefd_fsn_targets_backward on the first n bins of the target grid.  Per arm of TARGET_ARMS and per gradient: the largest error in units of
    eps32 x the term magnitudes <= 4 x float32 torch autograd alone on that arm (no arm skipped: an arm without members in a small case has nothing
    to hold, the largest case has members in every arm).  Exact zeros: mag_phase where noisy == 0; the cIRM under a cotangent on the clamp arm alone."""
    tools = _tools()
    noisy, clean = fc.target_inputs(n)
    gm, gp, gcirm = gc.target_cotangents(n)
    r = gc.target_grad_reference(n)
    bars = gc.target_grad_bars()
    got = _target_grads(tools, noisy.cuda(), clean.cuda(), gm.cuda(), gp.cuda(), gcirm.cuda())
    assert all(bool(torch.isfinite(t).all()) for t in got)
    lines, fails = [f"n = {n}"], []
    for which, g, ref, sc in (("mag_phase", got[0], r.d_mp, r.s_mp), ("cirm_noisy", got[1], r.d_noisy, r.s_noisy), ("cirm_clean", got[2], r.d_clean, r.s_clean)):
        for arm in fc.TARGET_ARMS:
            cost = gc.arm_cost(g, ref, sc, r.masks[arm])
            alone, bar = bars[(which, arm)]
            lines.append(f"    {which} {arm}: {int(r.masks[arm].sum())} bins, kernel {cost:.3g} float32 torch autograd alone {alone:.3g} bar {bar:.3g}")
            if cost > bar:
                fails.append((which, arm, cost, bar))
    _report("frontend_gpu_grad_targets.txt", lines)
    assert not fails, fails
    zero = noisy.abs() == 0
    assert bool((got[0][zero] == 0).all())
    g_clamp, any_clamp = gc.clamp_only_cotangent(n)
    z, c = noisy.cuda().requires_grad_(True), clean.cuda().requires_grad_(True)
    d_n, d_c = torch.autograd.grad(tools.build_complex_ideal_ratio_mask(z, c), (z, c), g_clamp.cuda())
    assert bool((torch.view_as_real(d_n) == 0).all()) and bool((torch.view_as_real(d_c) == 0).all())
    assert any_clamp or n < 257


def test_cirm_gradient_to_one_argument_alone():
    """Only the argument that asks gets a gradient, and it is the one both get together."""
    tools = _tools()
    n = 257
    noisy, clean = (t.cuda() for t in fc.target_inputs(n))
    g = gc.target_cotangents(n)[2].cuda()
    z, c = noisy.clone().requires_grad_(True), clean.clone().requires_grad_(True)
    d_n, d_c = torch.autograd.grad(tools.build_complex_ideal_ratio_mask(z, c), (z, c), g)
    z1 = noisy.clone().requires_grad_(True)
    assert torch.equal(torch.autograd.grad(tools.build_complex_ideal_ratio_mask(z1, clean), z1, g)[0], d_n)
    c1 = clean.clone().requires_grad_(True)
    assert torch.equal(torch.autograd.grad(tools.build_complex_ideal_ratio_mask(noisy, c1), c1, g)[0], d_c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tools.mag_phase(noisy.cpu().requires_grad_(True))
    with pytest.raises(RuntimeError, match="sefd stft runs on the MI355X only"):
        tools.stft(torch.zeros(1, 600, requires_grad=True))


# ------------------------------------------------------------------------------------------ bit-equality
def _offset_view(t):
    """The same values in a view that starts 4 bytes into its storage (complex: 4 bytes = half an element, through the float image)."""
    if t.is_complex():
        flat = torch.zeros(t.numel() * 2 + 1, dtype=torch.float32, device=t.device)
        flat[1:].copy_(torch.view_as_real(t).reshape(-1))
        return flat, lambda: flat[1:].view(*t.shape, 2)
    flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:].copy_(t.reshape(-1))
    return flat, lambda: flat[1:].view(t.shape)


def test_stft_backward_is_bit_stable_batch_independent_and_alignment_free():
    tools = _tools()
    c = fc.StftCase(3, 4801, 512, 300, 400)
    x, g = fc.stft_input(c).cuda(), gc.stft_cotangent(c).cuda()
    one = _stft_grad(tools, c, x.clone(), g)
    assert torch.equal(one, _stft_grad(tools, c, x.clone(), g))
    c1 = c._replace(B=1)
    for b in range(c.B):
        assert torch.equal(_stft_grad(tools, c1, x[b:b + 1].clone(), g[b:b + 1].clone()), one[b:b + 1])
    flat, view = _offset_view(x)
    xv = view()
    assert xv.data_ptr() % 16 == 4 or xv.data_ptr() % 8 == 4
    flat.requires_grad_(True)
    S = tools.stft(flat[1:].view(x.shape), c.nfft, c.hop, c.win)
    (gf,) = torch.autograd.grad(S, flat, g)
    assert torch.equal(gf[1:].view(x.shape), one) and float(gf[0]) == 0.0


def test_istft_backward_is_bit_stable_batch_independent_and_alignment_free():
    tools = _tools()
    c = fc.IstftCase(3, 4801, 300, 400)
    S, gy = gc.istft_spectrum(c, "inconsistent").cuda(), gc.istft_cotangent(c).cuda()
    one, _ = _istft_grads(tools, c, S, gy)
    assert torch.equal(one, _istft_grads(tools, c, S, gy)[0])
    c1 = c._replace(B=1)
    for b in range(c.B):
        assert torch.equal(_istft_grads(tools, c1, S[b:b + 1].clone(), gy[b:b + 1].clone())[0], one[b:b + 1])
    flat, view = _offset_view(S)
    flat.requires_grad_(True)
    y = tools.istft(flat[1:].view(*S.shape, 2), length=c.L, **_geom(c))
    (gf,) = torch.autograd.grad(y, flat, gy)
    assert torch.equal(gf[1:].view(*S.shape, 2), torch.view_as_real(one))
    gflat, gview = _offset_view(gy)                            # a cotangent that starts 4 bytes into its storage
    s = S.clone().requires_grad_(True)
    assert torch.equal(torch.autograd.grad(tools.istft(s, length=c.L, **_geom(c)), s, gview())[0], one)


def test_target_backward_is_bit_stable_batch_independent_and_alignment_free():
    tools = _tools()
    n = 257
    noisy, clean = (t.cuda() for t in fc.target_inputs(n))
    gm, gp, gcirm = (t.cuda() for t in gc.target_cotangents(n))
    one = _target_grads(tools, noisy, clean, gm, gp, gcirm)
    two = _target_grads(tools, noisy, clean, gm, gp, gcirm)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    for i in (0, 100, 256):
        part = _target_grads(tools, noisy[i:i + 1].clone(), clean[i:i + 1].clone(), gm[i:i + 1].clone(), gp[i:i + 1].clone(), gcirm[i:i + 1].clone())
        assert all(torch.equal(a, b[i:i + 1]) for a, b in zip(part, one))
    # a complex64 view cannot start half an element into its storage (torch refuses the view): one element, 8 bytes, off the 16-byte grid; the real
    # cotangents start 4 bytes in
    nbuf, cbuf = torch.zeros(n + 1, dtype=torch.complex64, device="cuda"), torch.zeros(n + 1, dtype=torch.complex64, device="cuda")
    nbuf[1:].copy_(noisy)
    cbuf[1:].copy_(clean)
    assert nbuf[1:].data_ptr() % 16 == 8
    off = _target_grads(tools, nbuf[1:], cbuf[1:], _offset_view(gm)[1](), _offset_view(gp)[1](), _offset_view(gcirm)[1]())
    assert all(torch.equal(a, b) for a, b in zip(off, one))


# ------------------------------------------------------------------------------------------ the forward is what it was
def test_forward_without_a_gradient_is_the_plan_and_the_kernel_bit_for_bit():
    """With no input requiring a gradient the four helpers return the bits of the TorchSTFT / TorchISTFT plans and of sefd_fsn_targets run directly;
    with one, the forward values are the same bits again."""
    tools = _tools()
    from sefd_amd import _lib
    from sefd_amd.plan import PHASE_FWD, Plan
    c = fc.StftCase(3, 4801, 512, 300, 400)
    x = fc.stft_input(c).cuda()
    st = torch.cuda.current_stream().cuda_stream
    plan = Plan(c.B, c.L, win_len=c.win, win_inc=c.hop, fft_len=c.nfft, model="TorchSTFT")
    ar = plan.alloc_arenas(x.device)
    plan.io(ar, "wav", (c.B, c.L)).copy_(x)
    plan.run(PHASE_FWD, ar, st)
    direct = torch.view_as_complex(plan.io(ar, "spec", (c.B, plan.NF, plan.T, 2)).clone())
    S = tools.stft(x, c.nfft, c.hop, c.win)
    assert not S.requires_grad and torch.equal(S, direct)
    assert torch.equal(tools.stft(x.clone().requires_grad_(True), c.nfft, c.hop, c.win).detach(), direct)
    ci = fc.IstftCase(3, 4801, 300, 400)
    Si = gc.istft_spectrum(ci, "inconsistent").cuda()
    plan = Plan(ci.B, ci.L, win_len=ci.win, win_inc=ci.hop, fft_len=512, model="TorchISTFT")
    ar = plan.alloc_arenas(x.device)
    plan.io(ar, "spec", (ci.B, 257, plan.T, 2)).copy_(torch.view_as_real(Si))
    plan.run(PHASE_FWD, ar, st)
    direct = plan.io(ar, "wav", (ci.B, ci.L)).clone()
    y = tools.istft(Si, length=ci.L, **_geom(ci))
    assert not y.requires_grad and torch.equal(y, direct)
    assert torch.equal(tools.istft(Si.clone().requires_grad_(True), length=ci.L, **_geom(ci)).detach(), direct)
    n = 257
    noisy, clean = (t.cuda() for t in fc.target_inputs(n))
    mag, ph, cirm = (torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, 2, device="cuda"))
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert _lib.lib().sefd_fsn_targets(vp(torch.view_as_real(noisy)), vp(torch.view_as_real(clean)), n, vp(mag), vp(ph), vp(cirm), C.c_void_p(st)) == 0
    m1, p1 = tools.mag_phase(noisy)
    k1 = tools.build_complex_ideal_ratio_mask(noisy, clean)
    assert not (m1.requires_grad or p1.requires_grad or k1.requires_grad)
    assert torch.equal(m1, mag) and torch.equal(p1, ph) and torch.equal(k1, cirm)
    m2, p2 = tools.mag_phase(noisy.clone().requires_grad_(True))
    k2 = tools.build_complex_ideal_ratio_mask(noisy.clone().requires_grad_(True), clean)
    assert torch.equal(m2.detach(), mag) and torch.equal(p2.detach(), ph) and torch.equal(k2.detach(), cirm)


# ------------------------------------------------------------------------------------------ the recipe end to end
CHAIN_STAGES = 8      # float32 stages between cRM and the loss, each held to its own bar of this size: stft forward, decompress_cIRM, the complex product,
                      # istft forward, the SI-SNR kernel forward and backward, istft backward, the product's and decompress_cIRM's backward


def test_waveform_domain_loss_trains_the_crm_end_to_end():
    """A small FullSubNet, B = 2, L = 3000, noisy = clean + noise: loss = si_snr(istft(decompress_cIRM(cRM) (x) stft(noisy), length=L), clean).
    d loss / d cRM against the float64 torch restatement of everything after the model (on the device's cRM), max-norm over the largest element, within
    the looser of the stft and istft gradient bars times the norm of the chain: its CHAIN_STAGES float32 stages, and the condition number kappa of the one
    ill-conditioned quantity in it, SI-SNR's projection coefficient <est, clean> / <clean, clean> - the gradient is linear in its reciprocal, and float32
    knows the inner product of an untrained model's output with the target to eps32 sum|est clean| / |sum est clean| only.  Every parameter gets a
    finite, non-zero gradient from one backward()."""
    tools = _tools()
    from oracle import losses as olosses
    from oracle.weights import fill_state_dict_
    from sefd_amd import config as cfg, models, tools_for_loss as tfl
    cfg.loss, cfg.act_dtype = "MSE", "fp32"
    m = models.FullSubNet(sb_num_neighbors=2, fb_num_neighbors=2, fb_model_hidden_size=16, sb_model_hidden_size=16)
    fill_state_dict_(m)
    with torch.no_grad():
        # a mask of order 1, as a trained model gives: at the |cRM| ~ 1e-3 of the formula weights float32 decompress_cIRM (torch, K log of a quotient
        # within 2e-4 of 1) knows its own output to 3e-4 only, and the gradient of a loss that is not linear in the waveform inherits that
        m.sb_model.fc_output_layer.bias.add_(torch.tensor([1.5, -0.8]))
    m = m.to("cuda").train()
    m.dropout_keep = 1.0
    B, L = 2, 3000
    clean = fc.noise(B, L, 12)
    noisy = clean + 0.5 * fc.noise(B, L, 11)
    nc = tools.stft(noisy.cuda())
    cRM = m(tools.mag_phase(nc)[0])
    cRM.retain_grad()
    d = tools.decompress_cIRM(cRM)
    enh = torch.complex(d[..., 0] * nc.real - d[..., 1] * nc.imag, d[..., 1] * nc.real + d[..., 0] * nc.imag)
    loss = tfl.si_snr(tools.istft(enh, length=L), clean.cuda())
    m.zero_grad()
    loss.backward()
    assert cRM.grad is not None
    # float64 restatement of everything after the model
    c64 = cRM.detach().cpu().double().requires_grad_(True)
    n64 = torch.stft(noisy.double(), 512, 300, 400, window=fc.hann64(400), return_complex=True)
    lim = 9.9
    mk = lim * (c64 >= lim) - lim * (c64 <= -lim) + c64 * (c64.abs() < lim)
    d64 = -10.0 * torch.log((10.0 - mk) / (10.0 + mk))
    e64 = torch.complex(d64[..., 0] * n64.real - d64[..., 1] * n64.imag, d64[..., 1] * n64.real + d64[..., 0] * n64.imag)
    l64 = olosses.si_snr(torch.istft(e64, 512, 300, 400, window=fc.hann64(400), length=L), clean.double())
    (ref,) = torch.autograd.grad(l64, c64)
    err = gc.grad_err(cRM.grad.cpu(), ref)
    bar_stft = max(gc.stft_grad_reference(c).bar for c in gc.STFT_GRAD_CASES)
    y64 = torch.istft(e64, 512, 300, 400, window=fc.hann64(400), length=L).detach()
    kappa = float(((y64 * clean.double()).abs().sum(-1) / (y64 * clean.double()).sum(-1).abs()).max())
    bar = max(bar_stft, gc.istft_grad_k() * fc.EPS32) * CHAIN_STAGES * kappa
    bad = [k for k, p in m.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all()) or float(p.grad.abs().max()) == 0.0]
    _report("frontend_gpu_grad_recipe.txt", [f"recipe: |cRM| {float(cRM.detach().abs().mean()):.3f} loss {float(loss.detach()):.6f} (float64 {float(l64.detach()):.6f}) | kappa {kappa:.1f} | d loss / d cRM {err:.3e} of the largest element, bar {bar:.3e} "
                                             f"| parameters without a finite non-zero gradient: {bad}"])
    assert abs(float(loss.detach()) - float(l64.detach())) <= 1e-4 * max(1.0, abs(float(l64.detach())))
    assert err <= bar, (err, bar)
    assert not bad, bad
