"""CPU tier of the GPU STOI scorer (csrc/stoi.hip): the C ABI as declared and exported, the host-only size / validation entry, the refusals
of the Python surface, the routing of the validation loop, and the silent-frame fence of every input tests/test_gpu_stoi.py compares on."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sefd_amd  # noqa: F401
from sefd_amd import _lib, config as cfg, tools_for_estimate as te, trainer

import stoi_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_stoi_entries():
    hdr = open(os.path.join(ROOT, "include", "sefd.h")).read()
    L = _lib.lib()
    for sym in ("sefd_stoi_ws_bytes", "sefd_stoi_gpu"):
        assert sym + "(" in hdr and sym in _lib.EXPORTED and hasattr(L, sym)


def test_ws_bytes_validates_on_the_host():
    f = _lib.lib().sefd_stoi_ws_bytes
    assert f(1, 16000, 16000) > 0 and f(64, 48000, 8000) > 0
    assert f(1, 48000 * 600, 48000) > 0                        # ten minutes at 48 kHz are inside the cap
    assert f(1, 200, 10000) > 0                                # no frame at all is a score (1e-5), not an error
    assert f(0, 16000, 16000) == -1 and f(1, 0, 16000) == -1 and f(65536, 16000, 16000) == -1 and f(1, 16000, 0) == -1
    assert f(1, (1 << 26) + 1, 16000) == -3
    assert f(1, 1 << 26, 8000) == -3                           # fits at 8 kHz, not at 10 kHz
    for fs in (9999, 16001, 1):                                # 10000 / fs does not reduce to factors <= 1024
        assert f(1, 16000, fs) == -4
    for fs in (8000, 10000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000):
        assert f(2, 3 * fs, fs) > 0
    # more samples or more rows never need less
    assert f(2, 48000, 16000) > f(1, 48000, 16000) and f(1, 48001, 16000) >= f(1, 48000, 16000)


def test_gpu_entry_refuses_bad_arguments_before_touching_the_device():
    g = _lib.lib().sefd_stoi_gpu
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert g(None, p, 1, 16000, 16000, p, p, None) == -1 and g(p, p, 1, 16000, 16000, None, p, None) == -1
    assert g(p, p, 0, 16000, 16000, p, p, None) == -1 and g(p, p, 1, 0, 16000, p, p, None) == -1
    assert g(p, p, 1, 16000, 9999, p, p, None) == -4
    assert g(p, p, 1, (1 << 26) + 1, 16000, p, p, None) == -3


def test_python_surface_refuses_cpu_tensors_and_bad_shapes():
    x = torch.zeros(2, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        te.stoi_batch(x, x, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        te.composite_batch(x, x, fs=16000, stoi=True)
    from sefd_amd import ops  # noqa: F401
    assert torch.ops.sefd.stoi(torch.empty(3, 100, device="meta"), torch.empty(3, 100, device="meta"), 16000).shape == (3,)


def test_dropin_reexports_stoi_batch():
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        mod = importlib.import_module("tools_for_estimate")
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        sys.modules.pop("tools_for_estimate", None)
    assert mod.stoi_batch is te.stoi_batch and mod.cal_stoi is te.cal_stoi


def _batch(inputs, targets):
    return (torch.mean((inputs - targets) ** 2),), inputs


def test_validate_with_gpu_scorers_on_a_cpu_device_raises(tmp_path):
    clean = torch.from_numpy(sc.speechlike(2, 16000, seed=7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        trainer._validate(torch.nn.Identity(), [(clean, clean)], None, str(tmp_path), 1, "cpu", _batch, 1, "gpu")
    assert "scorers" in trainer.model_validate.__code__.co_varnames


def test_default_scorers_still_route_stoi_to_the_host(tmp_path, monkeypatch):
    te.build()
    assert cfg.gpu_stoi is False
    calls = []
    real = te.cal_stoi
    monkeypatch.setattr(te, "cal_stoi", lambda est, clean, nthreads=0: calls.append(est.shape) or real(est, clean, nthreads))
    monkeypatch.setattr(te, "stoi_batch", lambda *a, **k: pytest.fail("the default path must not reach the GPU scorer"))
    clean = torch.from_numpy(sc.speechlike(2, 48000, seed=7))
    noisy = clean + 0.02 * torch.randn(clean.shape, generator=torch.Generator().manual_seed(1))
    loss, pesq, stoi = trainer._validate(torch.nn.Identity(), [(noisy, clean)], None, str(tmp_path), 1, "cpu", _batch, 1, "default")
    assert calls == [(2, 48000)] and 0.5 < stoi <= 1.0
    # the knob only reroutes cuda devices: on the CPU "default" stays the host scorer
    monkeypatch.setattr(cfg, "gpu_stoi", True)
    trainer._validate(torch.nn.Identity(), [(noisy, clean)], None, str(tmp_path), 2, "cpu", _batch, 1, "default")
    assert len(calls) == 2


def test_host_scorer_is_unchanged_by_the_shared_filter_header():
    """scorers.cpp now takes the resampling filter, its alignment and the band edges from csrc_host/stoi_tables.h: still the oracle's numbers,
    at a rate that resamples up, one that resamples down and one that does not resample."""
    te.build()
    from oracle import stoi as so
    for fs in sc.RATES:
        clean, est = sc.speechlike_case(fs + 123)
        got = np.zeros(4)
        assert te.lib().sefd_stoi_batch(clean.ctypes.data, est.ctypes.data, 4, clean.shape[1], fs, got.ctypes.data, 0) == 0
        ref = np.array([so.stoi(clean[i], est[i], fs) for i in range(4)])
        assert np.abs(got - ref).max() < 1e-9, (fs, got, ref)


@pytest.mark.parametrize("fs", sc.RATES)
def test_silent_frame_fence_holds_on_every_compared_input(fs):
    """Every input of tests/test_gpu_stoi.py's comparisons: no frame within 1e-6 dB of the 40 dB cut, and the cut drops frames."""
    margins = []
    for n in sc.speechlike_lengths(fs):
        clean, _ = sc.speechlike_case(n)
        margins += [sc.assert_fenced(clean[i], fs) for i in range(4)]
    margins += [sc.assert_fenced(c, fs) for c, _ in sc.pair_cases(fs)]
    print(f"\nstoi fence fs={fs}: smallest margin {min(margins):.3e} dB")
    if fs == 8000:
        assert abs(min(margins) - 5.4e-3) < 1e-4 * 5         # the closest call of the whole set: 8 kHz, 2 fs + 77, row 0
    if fs == 16000:
        from oracle import stoi as so
        scores = [so.stoi(c, e, fs) for c, e in sc.pair_cases(fs)]
        assert 0.3 < min(scores) < max(scores) < 1.0 and max(scores) - min(scores) > 0.1     # the pairs span the scale
