"""CPU tier of the STOI / ESTOI loss (csrc/stoi.hip backward, tools_for_loss.stoi_loss): the reference of tests/stoi_loss_ref.py is pinned first
(its STOI forward to oracle/stoi.py, its gradient to a central finite difference), then the host ESTOI scorer to the numpy restatement, the C
ABI as declared and exported, the host-only size entry, the fences of every input tests/test_gpu_stoi_loss.py compares gradients on, and the
refusals of the Python surfaces."""
import inspect
import os

import numpy as np
import pytest
import torch

import sefd_amd  # noqa: F401
from sefd_amd import _lib, config as cfg, tools_for_estimate as te, tools_for_loss as tfl

import stoi_cases as sc
import stoi_loss_ref as ref
from oracle import stoi as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sefd_stoi_ws_bytes_ex", "sefd_stoi_gpu_ex", "sefd_stoi_backward")


@pytest.mark.parametrize("fs", sc.RATES)
def test_reference_stoi_forward_equals_oracle(fs):
    clean, est, d, _, _ = ref.speech_reference(fs, False)
    want = np.array([so.stoi(clean[i], est[i], fs) for i in range(4)])
    print(f"\nstoi reference fs={fs}: max |torch - oracle| {np.abs(d - want).max():.3e}")
    assert np.abs(d - want).max() <= 1e-12, (d, want)


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("fs", sc.RATES)
def test_reference_gradient_equals_central_finite_difference(fs, extended):
    """Along a random direction v, (f(e + t v) - f(e - t v)) / 2t in float64 against grad . v.  t = 1e-6 on signals of amplitude 0.1 with at
    least 0.005 of noise: the truncation error (t / 0.005)^2 and the rounding error eps f / (t |grad . v|) are both below 1e-7 relative, and a
    step that small moves no envelope across the clip (fenced below at 1e-7 relative, measured margins above 1e-6)."""
    clean, est, _, grad, _ = ref.speech_reference(fs, extended)
    row, t = 2, 1e-6
    v = np.random.default_rng(fs + extended).standard_normal(est.shape[1])
    f = lambda e: float(ref.stoi_torch(clean[row], torch.from_numpy(e), fs, extended).detach())
    e0 = est[row].astype(np.float64)
    fd = (f(e0 + t * v) - f(e0 - t * v)) / (2 * t)
    an = float(grad[row] @ v) / ref.WEIGHTS[row]
    print(f"\nstoi reference fs={fs} extended={extended}: fd {fd:.9e} autograd {an:.9e} rel {abs(fd - an) / abs(an):.2e}")
    assert abs(fd - an) <= 1e-6 * abs(an), (fd, an)


@pytest.mark.parametrize("fs", sc.RATES)
def test_host_estoi_equals_numpy_restatement(fs):
    te.build()
    clean, est = sc.speechlike_case(fs + 123)
    got = np.zeros(4)
    assert te.lib().sefd_stoi_batch_ex(clean.ctypes.data, est.ctypes.data, 4, clean.shape[1], fs, 1, got.ctypes.data, 0) == 0
    want = np.array([ref.estoi_numpy(clean[i], est[i], fs) for i in range(4)])
    print(f"\nhost estoi fs={fs}: {got}  max |host - numpy| {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() < 1e-9, (got, want)
    assert np.all(got > 0.05) and np.all(got < 1.0) and len(set(got.tolist())) == 4
    # the torch restatement says the same, and the flag at 0 is the plain entry, bit for bit
    assert np.abs(ref.speech_reference(fs, True)[2] - want).max() < 1e-12
    a, b = np.zeros(4), np.zeros(4)
    assert te.lib().sefd_stoi_batch_ex(clean.ctypes.data, est.ctypes.data, 4, clean.shape[1], fs, 0, a.ctypes.data, 0) == 0
    assert te.lib().sefd_stoi_batch(clean.ctypes.data, est.ctypes.data, 4, clean.shape[1], fs, b.ctypes.data, 0) == 0
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_cal_stoi_takes_extended_by_keyword_only(monkeypatch):
    te.build()
    sig = inspect.signature(te.cal_stoi)
    assert list(sig.parameters)[:3] == ["estimated_speechs", "clean_speechs", "nthreads"]
    assert sig.parameters["extended"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["extended"].default is False
    sig.bind(1, 2, 3)                                          # (est, clean, nthreads) still binds positionally
    with pytest.raises(TypeError):
        sig.bind(1, 2, 3, True)
    clean, est = sc.speechlike_case(16000 + 123)
    monkeypatch.setattr(cfg, "fs", 16000)
    plain, ext = np.array(te.cal_stoi(est, clean)), np.array(te.cal_stoi(est, clean, 0, extended=True))
    assert np.array_equal(plain, np.array(te.cal_stoi(est, clean, 2, extended=False)))
    assert np.abs(ext - [ref.estoi_numpy(clean[i], est[i], 16000) for i in range(4)]).max() < 1e-9 and not np.allclose(plain, ext)
    assert te.cal_stoi(est[:, :3000], clean[:, :3000], extended=True) == [1e-5] * 4          # 13 frames at 10 kHz: the floor, as in STOI
    assert "sefd_stoi_batch_ex" in te.EXPORTED and "sefd_stoi_batch_ex(" in open(os.path.join(ROOT, "include", "sefd_scorers.h")).read()


def test_header_declares_and_library_exports_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "sefd.h")).read()
    L = _lib.lib()
    for sym in NEW:
        assert sym + "(" in hdr and sym in _lib.EXPORTED and hasattr(L, sym), sym


def test_ws_bytes_ex_validates_like_the_plain_entry_and_grows_with_the_keep_bit():
    f, g = _lib.lib().sefd_stoi_ws_bytes, _lib.lib().sefd_stoi_ws_bytes_ex
    bad = [(0, 16000, 16000), (1, 0, 16000), (65536, 16000, 16000), (1, 16000, 0), (1, (1 << 26) + 1, 16000), (1, 1 << 26, 8000),
           (1, 16000, 9999), (1, 16000, 16001)]
    for args in bad:
        assert f(*args) < 0
        for flags in range(4):
            assert g(*args, flags) == f(*args), (args, flags)
    for args in [(1, 16000, 16000), (64, 48000, 8000), (1, 200, 10000), (2, 30000, 10000), (3, 4097, 10000)]:
        assert g(*args, 0) == f(*args)
        assert g(*args, 1) >= g(*args, 0) and g(*args, 2) >= g(*args, 0) and g(*args, 3) >= g(*args, 1) and g(*args, 3) >= g(*args, 2)
    assert g(2, 48000, 16000, 2) > g(2, 48000, 16000, 0)
    assert g(1, 16000, 16000, 4) == -1 and g(1, 16000, 16000, -1) == -1        # unknown bits
    b = _lib.lib().sefd_stoi_backward
    assert b(1, 16000, 16000, 2, None, None, None, None) == -1                 # refused before the device is touched


@pytest.mark.parametrize("fs", sc.RATES)
def test_fences_hold_on_every_input_the_gradients_are_compared_on(fs):
    """Silence fence (no keep / drop decision within 1e-6 dB, and the cut cuts) and clip fence (no segment entry within 1e-7 relative of the
    clip, computed from the reference's own c, y, x) on speechlike_case(fs + 123); over the set both arms of the clip are taken."""
    clean, _, _, _, details = ref.speech_reference(fs, False)
    for i in range(4):
        sc.assert_fenced(clean[i], fs)
    margins, shares = [d["margin"] for d in details], [d["clipped"] for d in details]
    print(f"\nstoi clip fence fs={fs}: smallest margin {min(margins):.3e}, clipped share per row {min(shares):.4f} .. {max(shares):.4f}")
    assert min(margins) >= 1e-7, margins
    assert 0.0 < min(shares) and max(shares) < 1.0, shares


@pytest.mark.parametrize("L", [4097, 4225])
def test_fences_hold_on_the_frame_count_edges(L):
    clean, _, d, grad, det = ref.edge_reference(L, False)
    assert sc.silence_margin_db(clean, 10000)[0] >= sc.MIN_MARGIN_DB           # loud noise: every frame is kept, none near the cut
    assert det["margin"] >= 1e-7 and 0.1 < d < 1.0
    nz = np.nonzero(grad)[0]
    kept = len(range(0, L - 256, 128))
    # everything from the second half of the last frame on is outside every frame of the compacted signal
    assert nz.max() == (kept - 1) * 128 + 127 and np.all(grad[(kept - 1) * 128 + 128:] == 0.0)


def test_reference_floors_below_thirty_frames():
    clean, est, d, grad, _ = ref.edge_reference(4096, False)
    assert d == 1e-5 and not grad.any() and ref.edge_reference(4096, True)[2] == 1e-5
    assert so.stoi(clean, est, 10000) == 1e-5 and ref.estoi_numpy(clean, est, 10000) == 1e-5


def test_reference_pause_gets_exact_zeros():
    """8-16 % of a speechlike row's gradient is exactly zero: the interior of its pause, which only dropped frames cover."""
    for extended in (False, True):
        _, _, _, grad, _ = ref.speech_reference(10000, extended)
        share = (grad == 0.0).mean(axis=1)
        assert np.all(share > 0.05) and np.all(share < 0.2), share


def test_surfaces_refuse_cpu_tensors_and_a_clean_that_requires_a_gradient():
    from sefd_amd import ops  # noqa: F401
    x = torch.zeros(2, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tfl.stoi_loss(x, x, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tfl.stoi_loss(x, x.clone().requires_grad_(), 16000, extended=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        te.stoi_batch(x, x, 16000, extended=True)
    with pytest.raises(NotImplementedError, match="`clean` requires a gradient"):
        tfl.stoi_loss(x.clone().requires_grad_(), x, 16000)
    m = lambda: torch.empty(3, 100, device="meta")
    assert torch.ops.sefd.stoi(m(), m(), 16000, True).shape == (3,)
    assert torch.ops.sefd.stoi(m(), m(), 16000, extended=True).dtype == torch.float64
    assert torch.ops.sefd.stoi(m(), m(), 16000).shape == (3,)
    assert torch.ops.sefd.stoi(m(), m().requires_grad_(), 16000, True).requires_grad
    with pytest.raises(NotImplementedError, match="`clean` requires a gradient"):
        torch.ops.sefd.stoi(m().requires_grad_(), m(), 16000)


def test_config_and_wiring():
    assert cfg.perceptual_list == [False, 'LMS', 'PMSQE', 'STOI', 'ESTOI'] and cfg.perceptual is False and cfg.stoi_loss_weight == 1.0
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        mod = importlib.import_module("tools_for_loss")
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
        sys.modules.pop("tools_for_loss", None)
    assert mod.stoi_loss is tfl.stoi_loss
    from sefd_amd import models
    src = inspect.getsource(models)
    assert '"STOI", "ESTOI"' in src and "tfl.stoi_loss(target, estimated, cfg.fs" in src
