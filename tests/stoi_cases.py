"""Shared inputs of the STOI tests (tests/test_stoi_api_cpu.py, tests/test_gpu_stoi.py): the project's two seeded signal generators, the
case lists both tiers use, and the fence around STOI's only data-dependent branch, the silent-frame cut."""
import numpy as np

from oracle import stoi as so

RATES = (16000, 8000, 10000)
NOISE_SCALES = np.array([[0.1], [0.5], [2.0], [8.0]], np.float32)       # of tests/test_scorers_cpu.py::test_stoi_cpp_equals_oracle
MIN_MARGIN_DB = 1e-6


def speechlike(B, n, seed=0):
    """Noise / tone carriers with syllabic (3-6 Hz) envelopes and a pause: something STOI's 30-frame envelope correlation can see.
    (Copy of tests/test_scorers_cpu.py::speechlike.)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    out = np.zeros((B, n), np.float32)
    for b in range(B):
        s = np.zeros(n)
        for f0 in (300, 700, 1500, 2800, 4200):
            carrier = np.sin(2 * np.pi * f0 * t * (1 + 0.02 * b) + rng.uniform(0, 6)) + 0.3 * rng.standard_normal(n)
            s += carrier * np.clip(np.sin(2 * np.pi * (3 + rng.uniform(0, 3)) * t + rng.uniform(0, 6)), 0, None) ** 2
        s[int(0.4 * n):int(0.5 * n)] *= 5e-4
        out[b] = (0.1 * s).astype(np.float32)
    return out


def speechlike_pair(n, fs, seed, snr_db):
    """AR(2)-filtered noise under an on / off syllable envelope, with runs of exact zeros (digital silence, kept silent in the processed
    signal too, as an enhancer passes it through), plus white noise at `snr_db` over the active part.  float32 (clean, processed).
    (Copy of tests/test_gpu_composite.py::speechlike_pair.)"""
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


def silence_margin_db(clean, fs):
    """(margin, kept, total): the smallest |emax - 40 - e_f| over the 256 / 128 Hann frames of the clean signal at 10 kHz (resampled with
    oracle.stoi.resample), in dB, with the number of frames the silent-frame cut keeps and the number there are."""
    x = np.asarray(clean, dtype=np.float64)
    if fs != so.FS:
        x = so.resample(x, so.FS, fs)
    w = so._window()
    idx = range(0, len(x) - so.N_FRAME, so.N_FRAME // 2)
    e = np.array([20 * np.log10(np.linalg.norm(w * x[i:i + so.N_FRAME]) + so.EPS) for i in idx])
    d = e.max() - so.DYN_RANGE - e
    return float(np.abs(d).min()), int((d < 0).sum()), len(e)


def assert_fenced(clean, fs):
    """No keep / drop decision within MIN_MARGIN_DB of the threshold (a flipped one cannot hide behind a tolerance), and the cut cuts."""
    margin, kept, total = silence_margin_db(clean, fs)
    assert margin >= MIN_MARGIN_DB, (fs, len(clean), margin)
    assert kept < total, (fs, len(clean), kept, total)
    return margin


def speechlike_lengths(fs):
    return (3 * fs, fs + 123, 2 * fs + 77)


def speechlike_case(n):
    """(clean, est) [4, n]: `speechlike` at seed 3 and clean + noise at the four scales."""
    clean = speechlike(4, n, seed=3)
    rng = np.random.default_rng(4)
    est = clean + 0.05 * rng.standard_normal(clean.shape).astype(np.float32) * NOISE_SCALES
    return clean, est.astype(np.float32)


def pair_cases(fs):
    """`speechlike_pair` at fs + 37, 2 fs + 74, 3 fs + 111 with seeds fs / 10 + k, at 0, 8 and 16 dB of SNR."""
    return [speechlike_pair(s * fs + 37 * s, fs, fs // 10 + k, snr) for k, (s, snr) in enumerate(zip((1, 2, 3), (0.0, 8.0, 16.0)))]
