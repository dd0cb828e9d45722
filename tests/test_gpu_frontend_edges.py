"""GPU tier of the front-end case table (frontend_cases.py): tools.stft, tools.istft, tools.mag_phase, tools.build_complex_ideal_ratio_mask and
tools.decompress_cIRM through their public signatures against float64 references, at the bars the table derives from float32 torch on the CPU
(never from the code under test).  Every figure is printed before it is asserted and written to the report directory.

Measured on the MI355X (the float32-alone figures are torch on that host's CPU):
  STFT    kernel 1.8 .. 2.8 x float32 torch.stft alone (1.06e-7 .. 1.56e-7), worst 0.70 of its bar.  With ONE accumulator over all fft_len
          products the same GEMM measured 3.9 .. 6.3 x alone (6.8e-7 at B3-L4801, 1.58 of the bar): that is the sequential rounding of an fp32
          sum of 512 terms (a float32 loop on the CPU gives 6.0e-7 there), not operands rounded below fp32 - the planner now sums in chunks of 128
  iSTFT   K_ref = 2.375, K = 9.50; kernel worst 2.24 over the 54 case x spectrum pairs (2.12 through (mag, phase)); 1.2 .. 2.0 at L = 6199 / 6200, where
          the largest sample is 386 .. 2590 for a signal of scale 0.3; fullsubnet_validate at L = 6199: 1.69
  mag     <= 0.97 eps32 relative (bar 4)
  phase   3.0e-7 rad; float32 torch.angle alone 1.44e-7, bar 5.75e-7
  cIRM    kernel / float32 oracle alone / bar:  eps_decides 5.4e-6 / 2.9e-6 / 1.15e-5,  else 1.6e-6 / 2.5e-6 / 1.0e-5,  cancels 5.8e-3 / 9.1e-3 / 3.6e-2,
          noisy_zero 0 / 0 / 0;  clamp: the one float32 value at -100 on all 339 components;  saturate: exactly 10 on all 189
  census  frontend_cases.target_census, n = 4194561: test_frontend_cases_cpu.py's docstring
  decompress_cIRM  inner 1.9e-7 relative (bar 1e-6), small masks 1.3e-6 absolute (bar 4.8e-6), the limit itself 3.6e-9 relative
  the whole file: 74 tests in 5 s
"""

import numpy as np
import pytest
import torch

import frontend_cases as fc

pytestmark = pytest.mark.gpu
PI32 = float(np.float32(np.pi))


def _tools():
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_model as tools
    return tools


def _report(name, lines):
    from plan_check import report_path
    print("\n".join(lines))
    with open(report_path(name), "a") as f:
        f.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------------------ STFT
@pytest.mark.parametrize("case", fc.STFT_CASES, ids=fc.stft_id)
def test_stft_against_float64(case):
    """Max-norm error over the largest float64 bin <= max(2e-7, 4 x float32 torch.stft alone)."""
    tools = _tools()
    r = fc.stft_reference(case)
    got = tools.stft(fc.stft_input(case).cuda(), case.nfft, case.hop, case.win)
    T = 1 + case.L // case.hop
    assert got.dtype == torch.complex64 and tuple(got.shape) == (case.B, case.nfft // 2 + 1, T)
    err = fc.stft_err(got.cpu(), r.spec)
    _report("frontend_gpu_stft.txt", [f"{fc.stft_id(case)}: float32 torch alone {r.alone:.3e} bar {r.bar:.3e} kernel {err:.3e} = {err / r.alone:.2f} x alone, {err / r.bar:.2f} of the bar"])
    assert err <= r.bar, (err, r.bar)


# ------------------------------------------------------------------------------------------ iSTFT
def _istft_forms(tools, spec, case, length="given"):
    """The three entry forms on one spectrum -> (output of the complex form, the spectrum the (mag, phase) form denotes, its output)."""
    kw = dict(n_fft=fc.NFFT, hop_length=case.hop, win_length=case.win)
    if length == "given":
        kw["length"] = case.L
    s = spec.cuda()
    out = tools.istft(s, **kw)
    assert torch.equal(out, tools.istft(torch.view_as_real(s).contiguous(), **kw))
    mag, ph = s.abs(), s.angle()
    out_mp = tools.istft((mag, ph), use_mag_phase=True, **kw)
    s_mp = torch.complex(mag * torch.cos(ph), mag * torch.sin(ph))                # the spectrum (mag, phase) stands for, in the arithmetic of tools.istft
    assert torch.equal(out_mp, tools.istft(s_mp, **kw))
    return out, s_mp.cpu(), out_mp


@pytest.mark.parametrize("kind", fc.ISTFT_KINDS)
@pytest.mark.parametrize("case", fc.ISTFT_CASES, ids=fc.istft_id)
def test_istft_against_float64(case, kind):
    """|out[p] - ref64[p]| <= K eps32 A[p] / env[p] at every sample, K = 4 x K_ref (frontend_cases.istft_k); complex and real-pair input
    bit-identical; (mag, phase) input bit-identical to the complex input of mag x (cos, sin) and inside the bound of THAT spectrum."""
    tools = _tools()
    spec = fc.istft_spectrum(case, kind)
    ref, unit = fc.istft_case_reference(case, kind)
    out, s_mp, out_mp = _istft_forms(tools, spec, case)
    assert out.dtype == torch.float32 and tuple(out.shape) == (case.B, case.L) and torch.isfinite(out).all()
    k = fc.bound_ratio(out.cpu(), ref, unit)
    ref_mp, unit_mp = fc.istft_reference(s_mp, case.hop, case.win, case.L)
    k_mp = fc.bound_ratio(out_mp.cpu(), ref_mp, unit_mp)
    _report("frontend_gpu_istft.txt", [f"{fc.istft_id(case)} {kind}: K_ref {fc.istft_k_reference():.3f} K {fc.istft_k():.3f} kernel {k:.3f} (mag, phase) {k_mp:.3f} "
                                       f"| largest sample {float(ref.abs().max()):.3g}"])
    assert k <= fc.istft_k() and k_mp <= fc.istft_k(), (k, k_mp, fc.istft_k())


def test_istft_without_length_returns_hop_times_frames_minus_one():
    tools = _tools()
    case = fc.LENGTH_NONE_CASE
    spec = fc.istft_spectrum(case, "inconsistent")
    assert case.L == case.hop * (spec.shape[-1] - 1)
    ref, unit = fc.istft_case_reference(case, "inconsistent")
    out, _, _ = _istft_forms(tools, spec, case, length=None)
    assert tuple(out.shape) == (case.B, case.L)
    assert torch.equal(out, tools.istft(spec.cuda(), fc.NFFT, case.hop, case.win, length=case.L))
    assert fc.bound_ratio(out.cpu(), ref, unit) <= fc.istft_k()


def test_istft_refuses_the_lengths_torch_refuses():
    """512 / 300 / 400: at L = 6250 and 6256 the clip reaches samples no window covers (torch: 'window overlap add min'); 6199 and 6200 end on
    the last window's last taps and give results; a frame count that does not belong to `length` is refused."""
    tools = _tools()
    S = fc.istft_spectrum(fc.IstftCase(2, 6250, 300, 400), "inconsistent").cuda()          # 21 frames, as for every L in 6000 .. 6299
    for L in (6250, 6256):
        assert not fc.torch_istft_accepts(L, 300, 400)
        with pytest.raises(ValueError, match=rf"at length {L} the clip reaches sample 6200"):
            tools.istft(S, length=L)
    for L in (6199, 6200):
        assert fc.torch_istft_accepts(L, 300, 400)
        out = tools.istft(S, length=L)
        assert tuple(out.shape) == (2, L) and torch.isfinite(out).all()
    with pytest.raises(ValueError, match=r"21 frames do not match length 5000"):
        tools.istft(S, length=5000)


# ------------------------------------------------------------------------------------------ targets
@pytest.mark.parametrize("n", fc.TARGET_SIZES)
def test_mag_phase_and_cirm_against_float64(n):
    """fsn_targets_kernel on the first n bins of the target grid (n = 4194561 is one pass of the grid-stride loop and 257 bins of the second).
    mag: 4 ulp relative for |noisy| in [1e-6, 1e3], exactly 0 at zero bins.  phase: absolute, 4 x float32 torch.angle alone; exactly +-pi on
    the negative real axis by the sign of the zero imaginary part, 0 at the zero bin.  cIRM: absolute per arm, 4 x float32 build_cirm alone;
    the clamp arm is the one value float32 gives at -100, the saturation arm exactly 10; finite everywhere."""
    tools = _tools()
    noisy, clean = fc.target_inputs(n)
    r = fc.target_reference(n)
    mag, ph = tools.mag_phase(noisy.cuda())
    cirm = tools.build_complex_ideal_ratio_mask(noisy.cuda(), clean.cuda())
    assert mag.dtype == ph.dtype == cirm.dtype == torch.float32 and tuple(mag.shape) == tuple(ph.shape) == (n,) and tuple(cirm.shape) == (n, 2)
    mag, ph, cirm = mag.cpu(), ph.cpu(), cirm.cpu()
    assert torch.isfinite(mag).all() and torch.isfinite(ph).all() and torch.isfinite(cirm).all()
    M = r.masks
    inr = (r.mag >= 1e-6) & (r.mag <= 1e3)
    mag_ulps = float(((mag.double() - r.mag).abs() / (fc.EPS32 * r.mag.clamp_min(1e-30)))[inr].max()) if bool(inr.any()) else 0.0
    ph_err = float((ph.double() - r.phase).abs().max())
    lines = [f"n = {n}: mag {mag_ulps:.3f} eps32 relative | phase {ph_err:.3e} (float32 torch alone {r.phase_alone:.3e}, bar {r.phase_bar:.3e})"]
    cirm_err = {}
    for arm in fc.CIRM_ARMS:
        if bool(M[arm].any()):
            cirm_err[arm] = float((cirm.double() - r.cirm)[M[arm]].abs().max())
            lines.append(f"    cIRM {arm}: {int(M[arm].sum())} components, kernel {cirm_err[arm]:.3e} float32 oracle alone {r.cirm_alone[arm]:.3e} bar {r.cirm_bar[arm]:.3e}")
    _report("frontend_gpu_targets.txt", lines)
    assert mag_ulps <= 4.0, mag_ulps
    assert bool((mag[r.mag == 0] == 0).all())
    assert ph_err <= r.phase_bar, (ph_err, r.phase_bar)
    assert bool((ph[M["neg_real_pos0"]] == PI32).all()) and bool((ph[M["neg_real_neg0"]] == -PI32).all()) and bool((ph[M["zero"]] == 0).all())
    for arm in ("eps_decides", "noisy_zero", "cancels", "else"):
        if arm in cirm_err:
            assert cirm_err[arm] <= r.cirm_bar[arm], (arm, cirm_err[arm], r.cirm_bar[arm])
    assert bool((cirm[M["saturate"]] == 10.0).all())
    assert torch.equal(cirm[M["clamp"]], r.cirm32[M["clamp"]])


def test_decompress_cirm_on_the_three_arms_of_its_limit():
    """Away from the limit: relative 1e-6 against float64 where float32 can give it (|mask| >= 3), 40 eps32 absolute below (frontend_cases); a
    mask at or beyond +-9.9 gives bit for bit what +-9.9 itself gives, and that value is within 1e-6 of float64."""
    tools = _tools()
    d = fc.decompress_inputs()
    out = {arm: tools.decompress_cIRM(m.cuda()).cpu() for arm, m in d.items()}
    ref = {arm: fc.decompress_reference(m) for arm, m in d.items()}
    rel = float(((out["inner"].double() - ref["inner"]).abs() / ref["inner"].abs()).max())
    small = float((out["small"].double() - ref["small"]).abs().max())
    edge = max(abs(float(out[a][0]) - float(ref[a][0])) / abs(float(ref[a][0])) for a in ("upper", "lower"))
    _report("frontend_gpu_decompress.txt", [f"inner relative {rel:.3e} | small absolute {small:.3e} | the limit itself relative {edge:.3e}"])
    assert all(o.dtype == torch.float32 and torch.isfinite(o).all() for o in out.values())
    assert rel <= fc.DECOMPRESS_REL and small <= fc.DECOMPRESS_ABS_SMALL and edge <= fc.DECOMPRESS_REL
    assert float(out["small"][d["small"] == 0][0]) == 0.0
    for arm in ("upper", "lower"):
        assert bool((out[arm] == out[arm][0]).all()), out[arm]
    assert float(out["upper"][0]) == -float(out["lower"][0]) > 0


# ------------------------------------------------------------------------------------------ end to end
def _validate_setup():
    from test_gpu_validate import _cfg
    from oracle.weights import fill_state_dict_
    _cfg(loss="MSE", model="FullSubNet")
    from sefd_amd import models, trainer
    m = models.FullSubNet(fb_model_hidden_size=128, sb_model_hidden_size=64)
    fill_state_dict_(m)
    return m.to("cuda").train(), trainer


def test_fullsubnet_validate_refuses_a_clip_no_window_covers(tmp_path):
    """L = 6250: the enhanced waveform would be divided by an envelope of zero.  ValueError, and no scorer sees anything."""
    m, trainer = _validate_setup()
    x, y = fc.noise(2, 6250, 5), fc.noise(2, 6250, 6)
    calls = []

    def scorer(est, clean):
        calls.append(est.shape)
        return np.full(len(est), 1.0)

    with pytest.raises(ValueError, match=r"at length 6250 the clip reaches sample 6200"):
        trainer.fullsubnet_validate(m, [(x, y)], None, str(tmp_path), 1, "cuda", scorers=(scorer, scorer))
    assert calls == []


def test_fullsubnet_validate_holds_the_istft_bound_at_the_last_tap(tmp_path):
    """L = 6199: what the scorers get is torch.istft of the enhanced spectrum, within the per-sample bound.  The restatement of
    trainer.py:331-345 is that of test_fullsubnet_validate_runs_the_enhancement_path, on the spectrum and the cRM of the device."""
    m, trainer = _validate_setup()
    tools = _tools()
    L = 6199
    x, y = fc.noise(2, L, 7), fc.noise(2, L, 8)
    seen = {}

    def pesq(est, clean):
        seen["est"] = est.copy()
        return np.full(len(est), 1.5)

    trainer.fullsubnet_validate(m, [(x, y)], None, str(tmp_path), 1, "cuda", scorers=(pesq, lambda e, c: np.full(len(e), 0.5)))
    assert seen["est"].shape == (2, L) and np.isfinite(seen["est"]).all()
    m.eval()
    with torch.no_grad():
        nc = tools.stft(x.cuda())
        d = tools.decompress_cIRM(m(tools.mag_phase(nc)[0]))
        enh = torch.complex(d[..., 0] * nc.real - d[..., 1] * nc.imag, d[..., 1] * nc.real + d[..., 0] * nc.imag).cpu()
    ref, unit = fc.istft_reference(enh, 300, 400, L)
    k = fc.bound_ratio(torch.from_numpy(seen["est"]), ref, unit)
    _report("frontend_gpu_validate.txt", [f"L = {L}: enhanced waveform {k:.3f} (K {fc.istft_k():.3f}) | largest sample {float(ref.abs().max()):.3g}"])
    assert k <= fc.istft_k(), (k, fc.istft_k())
