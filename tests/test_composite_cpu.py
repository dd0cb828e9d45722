"""CPU tier of the composite measure (CSIG / CBAK / COVL; reference tools_for_estimate.py:24-45 and composite.m): the fp64 restatement in
tests/composite_ref.py on hand-checkable cases, the drop-in import surface, and the wav-reading rules that refuse a mismatched pair before
anything reaches the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import composite_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _speech(n, seed, fs=16000):
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    x = lfilter([1.0], [1.0, -1.3, 0.6], rng.standard_normal(n))
    t = np.arange(n) / fs
    return 0.05 * x * (0.2 + np.clip(np.sin(2 * np.pi * 3 * t), 0, None))


def test_framing_constants_and_frame_counts():
    assert cr.framing(16000) == (480, 120) and cr.n_fft(16000) == 1024 and cr.lpc_order(16000) == 16
    assert cr.framing(8000) == (240, 60) and cr.n_fft(8000) == 512 and cr.lpc_order(8000) == 10
    assert cr.framing(22050) == (662, 165)                      # round(661.5) = 662: MATLAB rounds half away from zero
    # floor(L / skip - win / skip): L not a multiple of skip
    for L, want in ((48000, 396), (48001, 396), (48119, 396), (48120, 397), (600, 1), (599, 0), (480, 0)):
        assert cr.num_frames(L, 16000) == want, L
    assert cr.num_frames(22050, 22050) == int(np.floor(22050 / 165 - 662 / 165))
    x = np.arange(48119, dtype=np.float64)
    fr = cr.frames(x, 16000)
    assert fr.shape == (396, 480)
    assert fr[395, 0] == (395 * 120 + cr.EPS) * cr.window(480)[0]      # frame k starts at sample k * skip (0-based)


def test_matlab_rounding_of_the_trimmed_mean():
    assert cr.mround(0.95 * 30) == 29 and int(np.round(0.95 * 30)) == 28
    assert cr.mround(2.5) == 3 and cr.mround(-2.5) == -3
    v = np.arange(30, dtype=np.float64)[::-1]
    assert cr.trimmed_mean(v) == np.arange(29).mean()            # 29 smallest of 30, not 28


def test_identical_signals():
    x = _speech(16000, 1)
    llr, wss, seg = cr.frame_measures(x, x, 16000)
    assert llr == 0.0 and wss == 0.0 and seg == 35.0


def test_levinson_matches_solve_toeplitz():
    from scipy.linalg import solve_toeplitz
    fr = cr.frames(_speech(8000, 2), 16000)
    R = cr.autocorr(fr, 16)
    A = cr.levinson(R)
    for f in (0, 10, 40):
        a = solve_toeplitz(R[f, :16], R[f, 1:17])
        np.testing.assert_allclose(-A[f, 1:], a, rtol=1e-7, atol=1e-9)
    assert np.all(A[:, 0] == 1.0)


def test_wss_peak_search_and_filters():
    F = cr.crit_filter(16000)
    assert F.shape == (25, 512) and np.all(F >= 0)
    assert F[0].argmax() == 3 and abs(F[0].max() - 1.0) < 1e-12       # band 1: floor(50 / 8000 * 512) = 3, unit gain (bw = bw_min)
    assert np.all((F > 0).sum(1) > 0)
    E = np.array([[0.0, 1, 2, 1, 0, 0, 3] + [3.0] * 18])
    S = np.diff(E, axis=1)
    P = cr._loc_peak(E, S)
    assert P[0, 0] == 1.0          # right search from band 0: stops at band 2 (first non-positive slope), reports band 1
    assert P[0, 2] == 2.0          # left search from band 2 (slope <= 0): back to band 1 (slope > 0), reports band 2
    assert P[0, 4] == 2.0          # slopes of bands 2..4 are <= 0: back to band 1, reports band 2
    E2 = np.array([[5.0 - i for i in range(25)]])
    assert np.all(cr._loc_peak(E2, np.diff(E2, axis=1))[0] == 5.0)   # a left search that runs off band 0 takes band 0


def test_composite_regression_clamps_before_adding_pesq():
    c = cr.combine(llr=0.0, wss=0.0, seg=35.0, pesq=4.5)
    assert c[0] == pytest.approx(3.093 + 0.603 * 4.5)
    assert c[1] == pytest.approx(1.634 + 0.063 * 35 + 0.478 * 4.5)
    c = cr.combine(llr=0.0, wss=0.0, seg=100.0, pesq=4.5)
    assert c[1] == pytest.approx(5.0 + 0.478 * 4.5) and c[1] > 5.0


def test_dropin_exposes_composite_and_pesq_mos():
    """The reference's scoring import line (estimation/check_object_metrics.py:9) against dropin/ (fresh interpreter)."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tools_for_estimate import cal_pesq, cal_stoi, composite, pesq_mos\n"
            "import sefd_amd\n"
            "assert composite is sefd_amd.tools_for_estimate.composite\n" % os.path.join(ROOT, "dropin"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


def test_mismatched_wav_pairs_are_refused_before_the_gpu(tmp_path, monkeypatch):
    from scipy.io import wavfile
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_estimate as te
    import torch
    monkeypatch.setattr(torch.cuda, "current_device", lambda: (_ for _ in ()).throw(AssertionError("reached the GPU")))
    x = (_speech(16000, 3) * 32767).astype(np.int16)
    a, b, c, d = (str(tmp_path / n) for n in ("a.wav", "b.wav", "c.wav", "d.wav"))
    wavfile.write(a, 16000, x)
    wavfile.write(b, 8000, x)
    wavfile.write(c, 16000, x.astype(np.int32) << 16)
    wavfile.write(d, 8000, x)
    for f in (te.composite, te.pesq_mos):
        with pytest.raises(ValueError, match="do not match"):
            f(a, b)                                   # rate
        with pytest.raises(ValueError, match="do not match"):
            f(a, c)                                   # bit depth
        with pytest.raises(ValueError, match="16 kHz"):
            f(d, d)                                   # the PESQ port is wide-band 16 kHz only
    fs, u, _ = te.read_wav_pair(a, a)
    assert fs == 16000 and u.dtype == np.float64 and np.array_equal(u, x / 32768.0)
    fs, u, _ = te.read_wav_pair(c, c)
    assert np.array_equal(u, x.astype(np.int32) * 65536 / 2.0 ** 31)


def test_composite_batch_refuses_cpu_tensors():
    import torch
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_estimate as te
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        te.composite_batch(torch.zeros(2, 16000), torch.zeros(2, 16000))
    from sefd_amd import ops  # noqa: F401
    e = torch.empty(4, 16000, device="meta")
    assert torch.ops.sefd.composite_measures(e, e, 16000).shape == (4, 3)
