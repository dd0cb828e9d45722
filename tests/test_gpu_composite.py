"""GPU tier of the composite measure: csrc/composite.hip (sefd_composite_frames) through tools_for_estimate.composite_batch against the fp64
restatement of tests/composite_ref.py, on seeded speech-like pairs at 16 and 8 kHz; determinism, batch independence, the wav-file entry
point and the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import composite_ref as cr

pytestmark = pytest.mark.gpu


def speechlike_pair(n, fs, seed, snr_db):
    """AR(2)-filtered noise under an on / off syllable envelope, with runs of exact zeros (digital silence, kept silent in the processed
    signal too, as an enhancer passes it through), plus white noise at `snr_db` over the active part.  float32 (clean, processed)."""
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    x = lfilter([1.0], [1.0, -1.3, 0.6], rng.standard_normal(n))
    env = np.empty(n)
    i, on = 0, True
    while i < n:
        m = int(fs * rng.uniform(0.08, 0.4))
        env[i:i + m] = 1.0 if on else 0.03
        i, on = i + m, not on
    env = lfilter([0.02], [1, -0.98], env)
    clean = 0.1 * x * env
    active = np.ones(n, bool)
    for _ in range(max(1, n // fs)):
        a = int(rng.integers(0, n))
        active[a:a + int(fs * rng.uniform(0.05, 0.2))] = False
    clean[~active] = 0.0
    noise = rng.standard_normal(n) * np.sqrt(np.mean(clean[active] ** 2) / 10 ** (snr_db / 10)) * active
    return clean.astype(np.float32), (clean + noise).astype(np.float32)


def _cases(fs):
    lengths = [fs * s + 37 * k for k, s in enumerate((1, 2, 3, 5, 7, 10), start=1)]
    snrs = [-5, 0, 5, 10, 15, 20]
    return [speechlike_pair(L, fs, 100 * fs // 1000 + k, snr) for k, (L, snr) in enumerate(zip(lengths, snrs))]


def _gpu(*xs):
    return [torch.from_numpy(x)[None].cuda() for x in xs]


@pytest.mark.parametrize("fs", [16000, 8000])
def test_composite_frames_against_the_restatement(fs):
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_estimate as te
    cases = _cases(fs)
    if fs == 16000:
        cases.append(speechlike_pair(60 * fs + 53, fs, 7, 5.0))
    worst = {"llr": 0.0, "seg": 0.0, "wss_rel": 0.0, "c": 0.0}
    for c, e in cases:
        assert len(c) % cr.framing(fs)[1] != 0
        got = te.composite_batch(*_gpu(c, e), fs=fs, pesq=(fs == 16000))
        llr, wss, seg = cr.frame_measures(c.astype(np.float64), e.astype(np.float64), fs)
        worst["llr"] = max(worst["llr"], abs(got["llr"][0] - llr))
        worst["seg"] = max(worst["seg"], abs(got["segsnr"][0] - seg))
        worst["wss_rel"] = max(worst["wss_rel"], abs(got["wss"][0] - wss) / abs(wss))
        assert abs(got["llr"][0] - llr) <= 1e-6, (len(c), got["llr"][0], llr)
        assert abs(got["segsnr"][0] - seg) <= 1e-5, (len(c), got["segsnr"][0], seg)
        assert abs(got["wss"][0] - wss) <= 1e-3 * abs(wss), (len(c), got["wss"][0], wss)
        if fs == 16000:
            want = cr.combine(llr, wss, seg, float(got["pesq"][0]))
            for k, name in enumerate(("csig", "cbak", "covl")):
                worst["c"] = max(worst["c"], abs(got[name][0] - want[k]))
                assert abs(got[name][0] - want[k]) <= 1e-3, (name, got[name][0], want[k])
        else:
            assert np.isnan(got["csig"][0]) and np.isnan(got["pesq"][0])
    print(f"\ncomposite fs={fs}: max |dLLR| {worst['llr']:.3e}  max |dsegSNR| {worst['seg']:.3e} dB  max rel dWSS {worst['wss_rel']:.3e}"
          f"  max |dC| {worst['c']:.3e}")


def test_composite_is_deterministic_and_batch_independent():
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_estimate as te
    fs, L = 16000, 3 * 16000 + 77
    pairs = [speechlike_pair(L, fs, 1000 + i, float(-5 + (i % 6) * 5)) for i in range(64)]
    C = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    E = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    a = te.composite_frames(C, E, fs).cpu().numpy()
    b = te.composite_frames(C, E, fs).cpu().numpy()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    for i in (0, 17, 63):
        alone = te.composite_frames(C[i:i + 1].clone(), E[i:i + 1].clone(), fs).cpu().numpy()
        assert np.array_equal(alone.view(np.uint64), a[i:i + 1].view(np.uint64)), i
    ll, ww, ss = cr.frame_measures(pairs[17][0].astype(np.float64), pairs[17][1].astype(np.float64), fs)
    assert abs(a[17, 0] - ll) <= 1e-6 and abs(a[17, 2] - ss) <= 1e-5 and abs(a[17, 1] - ww) <= 1e-3 * ww


def test_composite_wav_files_equal_the_batch_path(tmp_path):
    from scipy.io import wavfile
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_estimate as te
    c, e = speechlike_pair(2 * 16000 + 91, 16000, 5, 10.0)
    ci, ei = (np.clip(np.round(c * 32768), -32768, 32767).astype(np.int16), np.clip(np.round(e * 32768), -32768, 32767).astype(np.int16))
    pc, pe = str(tmp_path / "clean.wav"), str(tmp_path / "enh.wav")
    wavfile.write(pc, 16000, ci)
    wavfile.write(pe, 16000, ei[:-40])                          # cut to the shorter file
    got = te.composite(pc, pe)
    r = te.composite_batch(*_gpu((ci[:-40] / 32768.0).astype(np.float32), (ei[:-40] / 32768.0).astype(np.float32)), fs=16000)
    assert got == (r["csig"][0], r["cbak"][0], r["covl"][0], r["segsnr"][0])
    assert te.pesq_mos(pc, pe) == r["pesq"][0]
    assert 1.0 < got[0] < 7.0 and np.isfinite(got).all()


def test_composite_refuses_cpu_tensors_and_bad_shapes():
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_estimate as te
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        te.composite_frames(torch.zeros(1, 16000), torch.zeros(1, 16000).cuda(), 16000)
    with pytest.raises(ValueError):
        te.composite_frames(torch.zeros(1, 100).cuda(), torch.zeros(1, 100).cuda(), 16000)      # L < win
    with pytest.raises(ValueError):
        te.composite_frames(torch.zeros(1, 16000).cuda(), torch.zeros(1, 16000).cuda(), 1000)   # n_fft 64: unsupported rate
    with pytest.raises(ValueError, match="16 kHz"):
        te.composite_batch(torch.zeros(1, 16000).cuda(), torch.zeros(1, 16000).cuda(), fs=8000)
    from sefd_amd import ops  # noqa: F401
    out = torch.ops.sefd.composite_measures(torch.zeros(2, 560).cuda(), torch.zeros(2, 560).cuda(), 16000)   # L >= win, no whole frame
    assert out.shape == (2, 3) and torch.isnan(out).all()
