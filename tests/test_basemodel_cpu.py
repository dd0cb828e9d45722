"""CPU tier of BaseModel on its own (tools_for_model.py:801-1185): the torch restatement of tests/basemodel_common.py - written from the formulas, the
baseline the GPU kernels of csrc/basemodel.hip are benchmarked against - is pinned to the goldens captured from the real reference, forward and
gradient, in float64; the drop-in surface; and FullSubNet's weight init, which now goes through the extended traversal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import basemodel_common as bc
import sefd_amd  # noqa: F401
from sefd_amd.tools_for_model import BaseModel          # the class under test: without it nothing here means anything

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(bc.CASES))
def test_restatement_matches_the_reference_in_float64(name):
    """Both sides float64, the same arithmetic in another summation order: about 1e-12 for sums of up to 1e4 terms.  The bar, 1e-9 of the tensor's
    largest magnitude, is three orders above that and two below the float32 level the GPU test resolves: a wrong adjoint cannot hide in it."""
    ref, e32, seed = bc.load_golden(name)
    assert seed == bc.SEED
    res = bc.run_case(bc.Ref, name, torch.float64, inp=bc.inputs(name, seed))
    assert sorted(res) == sorted(ref)
    for k, v in ref.items():
        assert v.dtype == torch.float64 and bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, (name, k)
        e = bc.rel_err(res[k], v)
        assert e <= bc.CPU_BAR, (name, k, e)
    assert max(e32.values()) < 2e-6                                    # the generator's rule: no fixture with a loose bar


def test_case_table_covers_what_the_kernels_branch_on():
    shapes = {c[1] for c in bc.CASES.values() if c[0] in bc.NORMS3}
    assert {(1, 2, 1), (2, 9, 7), (3, 33, 66), (2, 5, 255), (2, 5, 256), (2, 5, 257), (1, 3, 600)} <= shapes
    for name in bc.NORMS3:
        Ls = {c[2] for c in bc.CASES.values() if c[0] == name and c[1] == (2, 9, 7)}
        assert {1, 2, 4, 6, 7, 8, 192} <= Ls, (name, Ls)
    # sband differs from forgetting_norm only in the frames t >= L: both parities of F must reach them
    assert {c[1][1] % 2 for c in bc.CASES.values() if c[0] == "sband_forgetting_norm" and c[1][2] > c[2]} == {0, 1}
    assert {c[1][1] for c in bc.CASES.values() if c[0] == "sband_forgetting_norm" and c[1][2] > c[2] and c[1][1] % 2 == 0} >= {4, 6, 34}
    for name in bc.NORMS4:                                             # C in {1, 3} at every shape
        for rows, F, T in bc.SHAPES:
            Fs = {F, 3} if (F, T) == (2, 1) else {F}
            assert {c[1][1] for c in bc.CASES.values() if c[0] == name and c[1][0] * c[1][1] in (rows, 3 * rows) and c[1][2] in Fs and c[1][3] == T} == {1, 3}, (name, rows, F, T)
    assert {(c[1][1], c[1][3], c[2]) for c in bc.CASES.values() if c[0] == "unfold"} == {(Cc, T, n) for Cc in (1, 3) for T in (1, 7, 68) for n in (0, 1, 3, 8)}
    assert all(os.path.getsize(os.path.join(bc.GOLDEN, f"basemodel_{n}.npz")) < 200_000 for n in bc.CASES)


def test_reduce_complexity_needs_thirds_as_the_reference_does():
    """B % 3 == 0 and (F - 2) % 3 == 0, or the three parts have different numbers of frequencies and the concatenation raises (F = 9, 10)."""
    inp = bc.inputs("reduce_b6_f11")
    ref, _, _ = bc.load_golden("reduce_b6_f11")
    y = BaseModel._reduce_complexity_separately(inp["x"].double(), inp["x2"].double(), "cpu")       # a pure gather in torch: runs anywhere
    assert torch.equal(y, ref["y"]) and tuple(y.shape) == (6, 3, 1, 10, 5)
    for F in (9, 10):
        with pytest.raises(RuntimeError):
            BaseModel._reduce_complexity_separately(torch.zeros(6, F, 1, 7, 5), torch.zeros(6, F, 1, 3, 5), "cpu")


def test_dropin_surface_in_a_fresh_interpreter():
    code = r'''
import sys
sys.path.insert(0, %r)
import torch
from tools_for_model import BaseModel
from models import FullSubNet
import sefd_amd
assert BaseModel is sefd_amd.models.BaseModel and BaseModel is sefd_amd.tools_for_model.BaseModel
assert issubclass(FullSubNet, BaseModel) and FullSubNet.unfold is BaseModel.unfold
m = FullSubNet(fb_model_hidden_size=16, sb_model_hidden_size=16)
assert isinstance(m, BaseModel) and isinstance(m, torch.nn.Module)
assert list(m.state_dict()) == [p + k for p in ("fb_model.", "sb_model.") for k in list(m.fb_model.state_dict())]
b = BaseModel()
for n in ("offline_laplace_norm", "cumulative_laplace_norm", "offline_gaussian_norm", "cumulative_layer_norm"):
    assert b.norm_wrapper(n) == getattr(BaseModel, n), n
for n in ("forgetting_norm", "sband_forgetting_norm", "hybrid_norm", "batch_norm", ""):
    try:
        b.norm_wrapper(n)
    except NotImplementedError as e:
        assert str(e) == "You must set up a type of Norm. e.g. offline_laplace_norm, cumulative_laplace_norm, forgetting_norm, etc.", str(e)
    else:
        raise AssertionError(n)
x4, x3 = torch.rand(2, 1, 9, 7) + 0.1, torch.rand(2, 9, 7) + 0.1
calls = [lambda: BaseModel.unfold(x4, 2)] + [lambda n=n: getattr(BaseModel, n)(x4) for n in ("offline_laplace_norm", "cumulative_laplace_norm",
         "offline_gaussian_norm", "cumulative_layer_norm")] + [lambda n=n: getattr(BaseModel, n)(x3, 4) for n in ("forgetting_norm",
         "sband_forgetting_norm", "hybrid_norm")] + [lambda: BaseModel.hybrid_norm(x3)]
for c in calls:
    try:
        c()
    except RuntimeError as e:
        assert "no CPU fallback" in str(e), str(e)
    else:
        raise AssertionError("a CPU tensor was accepted")
for bad in (lambda: BaseModel.unfold(x3, 1), lambda: BaseModel.forgetting_norm(x4, 4), lambda: BaseModel.offline_laplace_norm(x3)):
    try:
        bad()
    except AssertionError:
        pass
    else:
        raise SystemExit("a wrong number of dimensions was accepted")
from sefd_amd import ops
for n in ("basemodel_norm", "basemodel_norm_forward", "basemodel_norm_backward", "unfold", "unfold_backward"):
    assert hasattr(torch.ops.sefd, n), n
xm = torch.empty(2, 3, 9, 8, device="meta")
assert torch.ops.sefd.unfold(xm, 2).shape == (2, 9, 3, 5, 8) and torch.ops.sefd.unfold(xm, 0).shape == (2, 9, 3, 1, 8)
assert torch.ops.sefd.basemodel_norm(xm, 1, 1).shape == xm.shape
y, ws = torch.ops.sefd.basemodel_norm_forward(xm, 3, 1)
assert y.shape == xm.shape and ws.numel() == sefd_amd._lib.lib().sefd_norm_ws_floats(3, 6, 9, 8)
assert torch.ops.sefd.basemodel_norm_forward(xm, 0, 1)[1].numel() == sefd_amd._lib.lib().sefd_norm_ws_floats(0, 2, 216, 1)
try:
    torch.ops.sefd.basemodel_norm(x4, 1, 1)
except RuntimeError as e:
    assert "no CPU fallback" in str(e)
else:
    raise AssertionError("op took a CPU tensor")
print("OK")
''' % os.path.join(ROOT, "dropin")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_c_abi_size_function_refuses_what_the_launchers_refuse():
    import sefd_amd  # noqa: F401
    from sefd_amd import _lib
    L = _lib.lib()
    from sefd_amd.models import bm_ws_floats
    # per (row, frame), in doubles: 2 statistics + one partial sum per bin range (two for the layer norm) + 3 coefficients
    assert L.sefd_norm_ws_floats(1, 6, 9, 7) == 2 * 6 * 7 * (2 + 1 + 3) and L.sefd_norm_ws_floats(3, 2, 33, 7) == 2 * 2 * 7 * (2 + 2 * 2 + 3)
    # offline, per row: 2 statistics + 2 partial sums per segment + 3 coefficients
    assert L.sefd_norm_ws_floats(0, 2, 63, 1) == 2 * 2 * (2 + 2 + 3) and L.sefd_norm_ws_floats(2, 2, 3840, 1) == 2 * 2 * (2 + 2 * 2 + 3)
    for kind in range(7):                                              # the Python mirror the fake implementations size their workspace with
        for g in ((1, 2, 1), (2, 9, 7), (3, 33, 66), (2, 5, 257), (32, 257, 193), (2, 513, 5), (2, 6534, 1), (3, 2048, 1), (3, 2049, 1), (1, 600000, 1),
                  (1, 2 ** 31 - 1, 1), (1, 1, 2)):
            n = L.sefd_norm_ws_floats(kind, *g)
            assert n == -1 or n == bm_ws_floats(kind, *g), (kind, g)
    for bad in ((-1, 2, 9, 7), (7, 2, 9, 7), (1, 0, 9, 7), (1, 2, 0, 7), (1, 2, 9, 0), (5, 2, 1, 7), (2, 2, 1, 1)):
        assert L.sefd_norm_ws_floats(*bad) == -1, bad


@pytest.mark.parametrize("seq", ["LSTM", "GRU"])
def test_fullsubnet_weight_init_is_unchanged_and_is_basemodel_weight_init(seq):
    """FullSubNet(weight_init=True) draws what it drew (tests/golden/fsn_weight_init.npz, captured from the reference), and applying
    BaseModel.weight_init by hand - the reference's `model.apply(model.weight_init)` - draws the same."""
    import sefd_amd  # noqa: F401
    from sefd_amd import models
    g = np.load(os.path.join(bc.GOLDEN, "fsn_weight_init.npz"))
    torch.manual_seed(0)
    m = models.FullSubNet(fb_model_hidden_size=64, sb_model_hidden_size=32, sequence_model=seq, weight_init=True)
    torch.manual_seed(0)
    m2 = models.FullSubNet(fb_model_hidden_size=64, sb_model_hidden_size=32, sequence_model=seq, weight_init=False)
    m2.apply(m2.weight_init)                                           # the generator stands where the constructor's own call finds it
    for (k, p), (k2, p2) in zip(m.named_parameters(), m2.named_parameters()):
        v = p.detach().double().reshape(-1)
        got = np.array([float(v.sum()), float(v.abs().sum())] + [float(t) for t in v[:6]])
        assert np.allclose(got, g[f"g/{seq}/{k}"], rtol=1e-6, atol=1e-7), k
        assert k == k2 and torch.equal(p, p2), k


def test_weight_init_covers_the_reference_traversal():
    """Every module type tools_for_model.py:1126-1184 names is touched, with the distribution it names (moments of the draws)."""
    import torch.nn as nn
    b = BaseModel()
    torch.manual_seed(1)
    mods = [nn.Conv1d(8, 8, 3), nn.Conv2d(8, 8, 3), nn.Conv3d(4, 4, 3), nn.ConvTranspose1d(8, 8, 3), nn.ConvTranspose2d(8, 8, 3), nn.ConvTranspose3d(4, 4, 3),
            nn.BatchNorm1d(64), nn.BatchNorm2d(64), nn.BatchNorm3d(64), nn.Linear(32, 32), nn.LSTM(16, 16), nn.LSTMCell(16, 16), nn.GRU(16, 16), nn.GRUCell(16, 16)]
    for m in mods:
        before = [p.detach().clone() for p in m.parameters()]
        b.weight_init(m)
        assert any(not torch.equal(p, q) for p, q in zip(m.parameters(), before)), type(m).__name__
        if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)):
            assert abs(float(m.weight.mean()) - 1) < 0.02 and 0.01 < float(m.weight.std()) < 0.03 and float(m.bias.abs().max()) == 0
        elif isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
            assert 0.8 < float(m.weight.std()) < 1.2
        elif isinstance(m, (nn.LSTM, nn.LSTMCell, nn.GRU, nn.GRUCell)):
            w = m.weight_hh_l0 if hasattr(m, "weight_hh_l0") else m.weight_hh
            assert torch.allclose(w.t() @ w, torch.eye(16), atol=1e-5)
    conv_no_bias = nn.Conv2d(4, 4, 3, bias=False)
    b.weight_init(conv_no_bias)                                        # `if m.bias is not None`
