"""GPU tier of the STOI scorer: csrc/stoi.hip (sefd_stoi_gpu) through tools_for_estimate.stoi_batch against the host scorer (cal_stoi,
csrc_host/scorers.cpp) and the oracle (oracle/stoi.py) at 1e-9 - the bar tests/test_scorers_cpu.py holds the host scorer to against the
oracle: with fp64 throughout only summation order and twiddle rounding differ.  Every compared input is fenced first (stoi_cases.assert_fenced):
no keep / drop decision of the silent-frame cut within 1e-6 dB of its threshold.  Then the frame-count edges, degenerate signals, determinism
and batch independence, the op / composite / validation surfaces and the per-rate filter cache."""
import numpy as np
import pytest
import torch

import stoi_cases as sc
from oracle import stoi as so

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture()
def te():
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_estimate
    tools_for_estimate.build()
    return tools_for_estimate


def _gpu(te, clean, est, fs):
    return te.stoi_batch(torch.from_numpy(np.atleast_2d(clean)).cuda(), torch.from_numpy(np.atleast_2d(est)).cuda(), fs).cpu().numpy()


def _host(te, clean, est, fs):
    out = np.zeros(np.atleast_2d(clean).shape[0])
    c, e = np.ascontiguousarray(np.atleast_2d(clean), np.float32), np.ascontiguousarray(np.atleast_2d(est), np.float32)
    assert te.lib().sefd_stoi_batch(c.ctypes.data, e.ctypes.data, c.shape[0], c.shape[1], fs, out.ctypes.data, 0) == 0
    return out


@pytest.mark.parametrize("fs", sc.RATES)
def test_stoi_gpu_equals_host_scorer_and_oracle(te, fs):
    batches = [sc.speechlike_case(n) for n in sc.speechlike_lengths(fs)] + [(c[None], e[None]) for c, e in sc.pair_cases(fs)]
    if fs == 16000:                                            # one minute: the index ranges
        c = sc.speechlike(1, 60 * fs + 53, seed=9)
        batches.append((c, (c + 0.02 * np.random.default_rng(10).standard_normal(c.shape)).astype(np.float32)))
    worst_host = worst_oracle = 0.0
    for clean, est in batches:
        for row in clean:
            sc.assert_fenced(row, fs)
        got, host = _gpu(te, clean, est, fs), _host(te, clean, est, fs)
        worst_host = max(worst_host, float(np.abs(got - host).max()))
        if fs == 16000:
            ref = np.array([so.stoi(c, e, fs) for c, e in zip(clean, est)])
            worst_oracle = max(worst_oracle, float(np.abs(got - ref).max()))
            assert np.all(np.abs(got - ref) <= TOL), (clean.shape, got, ref)
        assert np.all(np.abs(got - host) <= TOL), (clean.shape, got, host)
        assert np.all(got > 1e-3) and np.all(got <= 1.0 + TOL)                  # scored, not floored
    print(f"\nstoi fs={fs}: max |gpu - host| {worst_host:.3e}" + (f"  max |gpu - oracle| {worst_oracle:.3e}" if fs == 16000 else ""))


def test_frame_count_edges(te):
    """10 kHz (no resampler), loud noise so every frame is kept: 30 frames leave 29 after the compaction (the strict `<` of the framing costs
    one), below the 30 a segment needs; 31 leave exactly one segment."""
    rng = np.random.default_rng(21)
    clean = (0.1 * rng.standard_normal(6000)).astype(np.float32)
    est = (clean + 0.05 * rng.standard_normal(6000)).astype(np.float32)
    fs = 10000
    worst = 0.0
    for L, floor in ((4096, True), (4097, False), (4224, False), (4225, False), (256, True), (200, True)):
        c, e = clean[:L], est[:L]
        if L > 256:
            assert sc.silence_margin_db(c, fs)[0] >= sc.MIN_MARGIN_DB
        got, host = _gpu(te, c, e, fs)[0], _host(te, c, e, fs)[0]
        if floor:
            assert got == 1e-5 and host == 1e-5, (L, got, host)
        else:
            worst = max(worst, abs(got - host))
            assert abs(got - host) <= TOL and 0.1 < got < 1.0, (L, got, host)
    assert _gpu(te, clean[:3000], est[:3000], 16000)[0] == 1e-5                  # 1875 samples at 10 kHz: 13 frames
    # 40 frames, only the first 20 of them non-zero: plenty of frames, too few kept
    L = 128 * 39 + 257
    c, e = clean[:L].copy(), est[:L].copy()
    c[2560:] = 0.0
    margin, kept, total = sc.silence_margin_db(c, fs)
    assert (kept, total) == (20, 40) and margin >= sc.MIN_MARGIN_DB
    assert _gpu(te, c, e, fs)[0] == 1e-5 and _host(te, c, e, fs)[0] == 1e-5
    print(f"\nstoi edges: max |gpu - host| {worst:.3e}")


def test_degenerate_signals(te):
    fs = 16000
    clean, est = sc.speechlike_case(fs + 123)
    assert np.all(np.abs(_gpu(te, clean, clean, fs) - 1.0) <= TOL)
    zero = np.zeros_like(clean)
    for c, e in ((zero, est), (clean, zero), (zero, zero)):
        got, host = _gpu(te, c, e, fs), _host(te, c, e, fs)
        assert np.all(np.isfinite(got)) and np.all(np.abs(got - host) <= TOL), (got, host)


def test_deterministic_and_batch_independent(te):
    fs, n, B = 16000, 16000 + 123, 65
    clean = np.concatenate([sc.speechlike(1, n, seed=40 + i) for i in range(B)])
    for i in range(B):                                         # a second pause per row, elsewhere and longer from row to row
        clean[i, 500 + 120 * i:800 + 220 * i] *= 5e-4
    kept = [sc.silence_margin_db(clean[i], fs)[1] for i in range(B)]
    assert len(set(kept)) >= 20 and min(kept) > 31, kept       # rows differ in their frame counts, and all of them are scored
    est = (clean + 0.01 * np.random.default_rng(41).standard_normal(clean.shape)).astype(np.float32)
    C, E = torch.from_numpy(clean).cuda(), torch.from_numpy(est).cuda()
    a = te.stoi_batch(C, E, fs).cpu().numpy()
    b = te.stoi_batch(C, E, fs).cpu().numpy()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.all(a > 0.3) and np.all(a < 1.0) and len(set(a.tolist())) == B
    for i in (0, 17, 64):
        alone = te.stoi_batch(C[i:i + 1].clone(), E[i:i + 1].clone(), fs).cpu().numpy()
        assert alone.shape == (1,) and np.array_equal(alone.view(np.uint64), a[i:i + 1].view(np.uint64)), i
    assert abs(a[17] - _host(te, clean[17], est[17], fs)[0]) <= TOL


def test_surfaces_and_filter_cache(te):
    from sefd_amd import ops  # noqa: F401
    fs = 16000
    clean, est = sc.speechlike_case(fs + 123)
    C, E = torch.from_numpy(clean).cuda(), torch.from_numpy(est).cuda()
    first = te.stoi_batch(C, E, fs)
    assert first.dtype == torch.float64 and first.shape == (4,) and first.is_cuda
    assert torch.equal(torch.ops.sefd.stoi(C, E, fs), first)
    wide_c, wide_e = torch.zeros(4, 2 * C.shape[1], device="cuda"), torch.ones(4, 2 * C.shape[1], device="cuda")
    wide_c[:, ::2], wide_e[:, ::2] = C, E
    assert not wide_c[:, ::2].is_contiguous() and torch.equal(te.stoi_batch(wide_c[:, ::2], wide_e[:, ::2], fs), first)
    r = te.composite_batch(C, E, fs=fs, stoi=True)
    assert np.array_equal(r["stoi"], first.cpu().numpy()) and "stoi" not in te.composite_batch(C, E, fs=fs, pesq=False)
    # another rate, then the first again: each rate's filter comes from its own cache entry
    other = te.stoi_batch(C, E, 8000)
    again = te.stoi_batch(C, E, fs)
    assert torch.equal(again, first) and not torch.equal(other, first)
    assert torch.equal(te.stoi_batch(C, E, 8000), other)
    with pytest.raises(ValueError):
        te.stoi_batch(C, E[:, :-1], fs)
    with pytest.raises(ValueError, match="-4"):
        te.stoi_batch(C, E, 9999)


def test_validation_loop_with_gpu_stoi(te, tmp_path):
    from sefd_amd import trainer
    clean = torch.from_numpy(sc.speechlike(2, 48000, seed=7))
    noisy = clean + 0.02 * torch.randn(clean.shape, generator=torch.Generator().manual_seed(1))

    def batch(inputs, targets):
        return (torch.mean((inputs - targets) ** 2),), inputs
    res, lines = {}, {}
    for mode in ("gpu", "default"):
        d = tmp_path / mode
        d.mkdir()
        res[mode] = trainer._validate(torch.nn.Identity(), [(noisy, clean)], None, str(d), 1, "cuda", batch, 1, mode)
        lines[mode] = open(d / "Epoch_1_SCORES").read().strip().splitlines()
    (lg, pg, sg), (ld, pd, sd) = res["gpu"], res["default"]
    assert float(lg) == float(ld) and pg == pd and abs(sg - sd) <= TOL and 0.5 < sg <= 1.0
    assert len(lines["gpu"]) == len(lines["default"]) == 2
    worst = 0.0
    for a, b in zip(lines["gpu"], lines["default"]):
        assert a.startswith("PESQ ") and " | STOI " in a and a.split(" | ")[0] == b.split(" | ")[0]
        worst = max(worst, abs(float(a.split("STOI ")[1]) - float(b.split("STOI ")[1])))
    assert worst <= 1.5e-6                                     # the file rounds to six decimals
    print(f"\nstoi validation: |avg gpu - avg host| {abs(sg - sd):.3e}")
