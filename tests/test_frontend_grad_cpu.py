"""CPU tier of the gradient case table (frontend_grad_cases.py): compress_cIRM against the reference formula, the backward identities of DESIGN.md
section 6 ("The torch-style helpers, differentiable") restated in float64 against torch.autograd.grad of torch.stft / torch.istft, the two adjoint
plans (they build, they refuse what their forward twins refuse, the forward plans keep their bytes), and the float32-torch-alone figures every bar of
the GPU tier (test_gpu_frontend_grad.py) is made of - computed here, so the bars exist before any GPU run.

Measured (torch on the CPU; the istft figure depends on the CPU's FFT: 0.45 on one host, 0.38 on another):
  identities   stft fold + adjoint <= 4.2e-14 of the largest element over the 8 cases (L = 257: every sample but two hit by a mirror; L = 300: T = 2);
               istft adjoint <= 4.3e-16 (the tail lengths 6190 / 6199 included); bar 1e-10
  stft alone   1.16e-7 .. 1.56e-7 (bars 4.7e-7 .. 6.2e-7)
  istft        K_ref = 0.454 over the 18 included case x spectrum pairs, K = 1.82; float32 torch on the cases left out of K_ref: up to 1.60
  round trip   decompress_cIRM(compress_cIRM(m)), |m| < 20, float32: 14.3 eps32 max(1, |m|) (bar 32)
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import frontend_cases as fc
import frontend_grad_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_SPECOUT_BWD, OP_OLA_BWD, OP_STFT_FFT, OP_ISTFT_FFT, OP_OLA_FOLD, OP_SPECOUT_ADJ = 18, 16, 37, 39, 52, 53        # sefd_desc.h OpKind
PARENT_FINGERPRINTS = {"torchstft": "4351b2829d37d1e0", "torchistft": "4f6d0fa1862a051f"}      # tools/plan_fingerprint.py on the commit before the adjoint plans
PARENT_OP_SIZE = 592                                      # sefd_op_size() there


def _tools():
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_model as tools
    return tools


def _report(name, lines):
    from plan_check import report_path
    print("\n".join(lines))
    with open(report_path(name), "a") as f:
        f.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------------------ compress_cIRM
def test_compress_cirm_matches_the_reference_formula_for_tensors_and_numpy():
    """float64 in, float64 out: 1e-12 absolute (the same formula in another order of operations; values within +-10).  mask <= -100 gives the value
    at -100; K and C are taken; the drop-in exports it."""
    tools = _tools()
    m = gc.compress_inputs().double()
    ref = gc.compress_reference(m)
    out_t = tools.compress_cIRM(m)
    out_n = tools.compress_cIRM(m.numpy())
    assert torch.is_tensor(out_t) and out_t.dtype == torch.float64 and isinstance(out_n, np.ndarray)
    assert float((out_t - ref).abs().max()) <= 1e-12 and float(np.abs(out_n - ref.numpy()).max()) <= 1e-12
    at100 = float(gc.compress_reference(torch.tensor([-100.0]))[0])
    for v in (-1e6, -1000.0, -100.5, -100.0):
        assert float(tools.compress_cIRM(torch.tensor([v], dtype=torch.float64))[0]) == pytest.approx(at100, abs=1e-12)
        assert float(tools.compress_cIRM(np.array([v]))[0]) == pytest.approx(at100, abs=1e-12)
    assert float((tools.compress_cIRM(m, K=5, C=0.2) - gc.compress_reference(m, 5.0, 0.2)).abs().max()) <= 1e-12
    assert float(tools.compress_cIRM(np.float64(3.0))) == pytest.approx(float(gc.compress_reference(3.0)), abs=1e-12)
    # differentiable, derivative K C 2 e / (1 + e)^2 and 0 on the clamped arm
    x = torch.tensor([-150.0, -3.0, 0.0, 7.0], dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(tools.compress_cIRM(x).sum(), x)
    e = torch.exp(-0.1 * x.detach())
    want = torch.where(x.detach() <= -100, torch.zeros_like(e), 2.0 * e / (1 + e) ** 2)
    assert float((g - want).abs().max()) <= 1e-14 and float(g[0]) == 0.0


def test_decompress_of_compress_returns_the_mask_within_float32_rounding():
    """|m| < 20 in float32, error in units of eps32 max(1, |m|).  Worst where |m| <= 1: compress forms 1 - e with e within 0.1 of 1 (e's half ulp is 5 eps32
    of the difference), so c = K (1 - e) / (1 + e) ~ m / 2 carries up to ~5 eps32 absolute, which decompress doubles (slope 2 K^2 / (K^2 - c^2)); decompress's own
    K - c, K + c and quotient are 1.5 eps32 relative on a quotient near 1, the log keeps that as an absolute error and K = 10 multiplies it: 15.  Worst case
    ~25, bar 32 (measured 14.3)."""
    tools = _tools()
    m = torch.linspace(-19.9, 19.9, 797)
    back = tools.decompress_cIRM(tools.compress_cIRM(m))
    worst = float(((back.double() - m.double()).abs() / (fc.EPS32 * m.double().abs().clamp_min(1.0))).max())
    _report("frontend_grad_cpu.txt", [f"decompress(compress(m)), |m| < 20: {worst:.2f} eps32 max(1, |m|) (bar 32)"])
    assert back.dtype == torch.float32 and worst <= 32.0, worst


def test_compress_cirm_is_exported_by_the_dropin():
    import subprocess
    import sys
    code = "import sys; sys.path.insert(0, %r); from tools_for_model import compress_cIRM, decompress_cIRM; import sefd_amd; " \
           "assert compress_cIRM is sefd_amd.tools_for_model.compress_cIRM; print('OK')" % os.path.join(ROOT, "dropin")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------ the identities
@pytest.mark.parametrize("case", gc.STFT_GRAD_CASES, ids=fc.stft_id)
def test_stft_fold_and_adjoint_identity_in_float64(case):
    """dxp = overlap-add of w Re sum_{k <= N/2} g e^{+2 pi i k j / N} (no half weights, no 1 / N), folded by the adjoint of the reflect padding,
    equals torch.autograd.grad of float64 torch.stft at 1e-10 of the largest element."""
    ref = gc.stft_grad_reference(case).grad
    got = gc.stft_adjoint64(gc.stft_cotangent(case), case.L, case.nfft, case.hop, case.win)
    err = gc.grad_err(got, ref)
    _report("frontend_grad_cpu.txt", [f"stft identity {fc.stft_id(case)}: {err:.2e}"])
    assert err <= 1e-10, err


def test_the_short_clips_exercise_both_mirrors():
    """L = 257 at n_fft 512: every sample but the first and the last is hit by a mirror, 255 of them by both."""
    L, pad = 257, 256
    i = torch.arange(L)
    left, right = (i >= 1) & (i <= pad), (i >= L - 1 - pad) & (i <= L - 2)
    assert int((left | right).sum()) == L - 0 and int((left & right).sum()) == 255 and int((~left).sum()) == 1 and int((~right).sum()) == 1
    assert any(c.L == 257 for c in gc.STFT_GRAD_CASES) and any(c.L == 300 and 1 + c.L // c.hop == 2 for c in gc.STFT_GRAD_CASES)


@pytest.mark.parametrize("kind", fc.ISTFT_KINDS)
@pytest.mark.parametrize("case", gc.ISTFT_GRAD_CASES, ids=fc.istft_id)
def test_istft_adjoint_identity_in_float64(case, kind):
    """gX = (c_k / N) rfft(w x (gy / env on the covered samples)) equals torch.autograd.grad of float64 torch.istft at 1e-10 of the largest element;
    the imaginary parts of DC and Nyquist are exactly 0 in torch's gradient as well."""
    ref, _ = gc.istft_grad_reference(case, kind)
    got = gc.istft_adjoint64(gc.istft_cotangent(case), ref.shape[-1], case.hop, case.win)
    err = float((got - ref).abs().max() / ref.abs().max())
    _report("frontend_grad_cpu.txt", [f"istft identity {fc.istft_id(case)} {kind}: {err:.2e}"])
    assert err <= 1e-10, err
    assert bool((ref.imag[:, 0] == 0).all()) and bool((ref.imag[:, -1] == 0).all())
    if case == gc.ONE_FRAME_CASE:                              # the zero-filled tail gives nothing: the gradient does not see gy[256:]
        gy = gc.istft_cotangent(case).clone()
        gy[:, 256:] = 0.0
        assert torch.equal(gc.istft_adjoint64(gy, 1, case.hop, case.win), got)


# ------------------------------------------------------------------------------------------ the plans
def _kinds(plan, phase=0):
    return [int(k) for k in plan.op_kinds(phase)[0]]


def test_the_adjoint_plans_build_with_their_op_lists():
    from simutil import Plan
    ps = Plan(3, 4801, win_len=400, win_inc=300, fft_len=512, model="TorchSTFTAdj")
    assert _kinds(ps) == [OP_SPECOUT_BWD, OP_ISTFT_FFT, OP_OLA_FOLD] and ps.num_ops(1) == 0 and ps.T == 17
    assert sorted(ps.buffer_names()) == ["frames", "gspec", "io.grad_spec", "io.grad_wav"]          # no [B][L + N] intermediate
    assert ps.buffer("io.grad_wav")[2] == 3 * 4801 * 4 and ps.buffer("io.grad_spec")[2] == 3 * 257 * 17 * 8 and ps.buffer("frames")[2] == 3 * 17 * 512 * 4
    pi = Plan(3, 4801, win_len=400, win_inc=300, fft_len=512, model="TorchISTFTAdj")
    assert _kinds(pi) == [OP_OLA_BWD, OP_STFT_FFT, OP_SPECOUT_ADJ] and pi.num_ops(1) == 0 and pi.T == 17
    assert pi.buffer("dpad")[2] == 3 * (16 * 300 + 512) * 4
    for c in gc.STFT_GRAD_CASES:
        assert Plan(c.B, c.L, win_len=c.win, win_inc=c.hop, fft_len=c.nfft, model="TorchSTFTAdj").T == 1 + c.L // c.hop
    for c in gc.ISTFT_GRAD_CASES:
        assert Plan(c.B, c.L, win_len=c.win, win_inc=c.hop, fft_len=512, model="TorchISTFTAdj").T == 1 + c.L // c.hop


@pytest.mark.parametrize("kw", [dict(win_inc=301), dict(win_len=600), dict(L=200), dict(win_inc=0), dict(L=6250), dict(fft_len=256, win_len=255, win_inc=100)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_the_adjoint_plans_refuse_what_their_forward_twins_refuse(kw):
    """One sentence, the twin's own; the stft adjoint adds one of its own for fft_len != 512 (its twin runs a GEMM there)."""
    from simutil import Plan
    a = dict(B=2, L=6000, win_len=400, win_inc=300, fft_len=512)
    a.update(kw)
    for twin, adj in (("TorchSTFT", "TorchSTFTAdj"), ("TorchISTFT", "TorchISTFTAdj")):
        try:
            Plan(model=twin, **a)
            want = None
        except ValueError as e:
            want = str(e)
        if want is None and not (adj == "TorchSTFTAdj" and a["fft_len"] != 512):
            Plan(model=adj, **a)
            continue
        with pytest.raises(ValueError) as ei:
            Plan(model=adj, **a)
        msg = str(ei.value)
        assert msg.count("\n") == 0 and msg.startswith("sefd plan: ")
        if want is not None:
            assert msg == want
        else:
            assert "torch.stft backward plan: fft_len 256 is not 512" in msg


def test_the_forward_plans_keep_the_parents_bytes():
    """Model ids 4 and 5 are byte-identical to the commit before (op arrays, constants, buffers), and sizeof(Op) did not move."""
    spec = importlib.util.spec_from_file_location("plan_fingerprint", os.path.join(ROOT, "tools", "plan_fingerprint.py"))
    pf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pf)
    got = {name: pf.digest(pf.plan_bytes(kw, knobs)) for name, kw, knobs in pf.MATRIX if name in PARENT_FINGERPRINTS}
    assert got == PARENT_FINGERPRINTS
    from sefd_amd import _lib
    assert _lib.lib().sefd_op_size() == PARENT_OP_SIZE


# ------------------------------------------------------------------------------------------ the bars
def test_stft_gradient_bars_exist():
    lines = []
    for c in gc.STFT_GRAD_CASES:
        r = gc.stft_grad_reference(c)
        lines.append(f"stft gradient {fc.stft_id(c)}: float32 torch autograd alone {r.alone:.3e} bar {r.bar:.3e}")
        assert 0 < r.alone < 1e-6 and r.bar >= fc.STFT_FLOOR
    _report("frontend_grad_cpu.txt", lines)
    assert {(c.B, c.L) for c in gc.STFT_GRAD_CASES} >= {(1, 257), (1, 300), (3, 4801), (7, 6000), (5, 1000), (2, 1000)}
    assert any(c.win == 399 for c in gc.STFT_GRAD_CASES) and {c.nfft for c in gc.STFT_REFUSED_CASES} == {256, 1024}


def test_istft_gradient_k_reference_and_torch_alone_on_every_included_case():
    kref, K = gc.istft_grad_k_reference(), gc.istft_grad_k()
    lines = [f"istft gradient: K_ref {kref:.3f} K {K:.3f}"]
    for c in gc.ISTFT_GRAD_CASES:
        for kind in fc.ISTFT_KINDS:
            k = gc.istft_grad_k_alone(c, kind)
            inc = gc.in_k_reference(c)
            lines.append(f"    {fc.istft_id(c)} {kind}: float32 torch autograd alone {k:.3f}" + ("" if inc else " (tail: not in K_ref)"))
            if inc:
                assert k <= kref <= K
    _report("frontend_grad_cpu.txt", lines)
    assert 0.25 < kref < 16, kref
    assert [c.L for c in gc.ISTFT_GRAD_CASES if not gc.in_k_reference(c)] == [6190, 6190, 6199, 6199, 1000, 400]     # + hop 256 at win 512 and the one-frame case: their envelopes reach 0 at the clip's ends


def test_target_gradient_bars_cover_every_arm():
    """Every arm of TARGET_ARMS has members in the largest case and a finite float32-alone figure for each of the three gradients."""
    bars = gc.target_grad_bars()
    r = gc.target_grad_reference(max(gc.TARGET_GRAD_SIZES))
    lines = []
    for arm in fc.TARGET_ARMS:
        assert bool(r.masks[arm].any()), arm
        row = []
        for which in ("mag_phase", "cirm_noisy", "cirm_clean"):
            alone, bar = bars[(which, arm)]
            assert np.isfinite(alone) and bar == gc.TARGET_MARGIN * alone, (which, arm, alone)
            row.append(f"{which} {alone:.3g}")
        lines.append(f"target gradient {arm} ({int(r.masks[arm].sum())} bins): float32 torch autograd alone, in eps32 x term magnitudes: " + ", ".join(row))
    _report("frontend_grad_cpu.txt", lines)
    for t in (r.d_mp, r.d_noisy, r.d_clean):
        assert bool(torch.isfinite(t).all())
    zero = (fc.target_inputs(max(gc.TARGET_GRAD_SIZES))[0].abs() == 0)
    assert bool((r.d_mp[zero] == 0).all())                     # torch's complex abs / angle backward: 0 at a zero bin
