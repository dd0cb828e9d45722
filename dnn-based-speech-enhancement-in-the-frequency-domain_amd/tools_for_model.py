"""Module-level helpers of the reference's tools_for_model.py that the FullSubNet trainer calls (trainer.py:100-104, 341-345):
`stft`, `istft`, `mag_phase`, `build_complex_ideal_ratio_mask`, `compress_cIRM`, `decompress_cIRM` - same signatures, HIP kernels underneath.
cuda tensors only (no CPU fallback).  All of them carry a gradient ("The torch-style helpers, differentiable"): with no input
requiring one they run exactly the launches of the plain forward."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import config as cfg
from .plan import PHASE_FWD, Plan
from .runtime import Runtime, cached


def __getattr__(name):
    # tools_for_model.SequenceModel (tools_for_model.py:726-795) is models.SequenceModel: resolved on first use, models.py imports this module
    if name == "SequenceModel":
        from .models import SequenceModel
        return SequenceModel
    # tools_for_model.py:36-112, 126-607 and 801-1185, defined in models.py beside the models that hold them
    if name in ("ConvSTFT", "ConviSTFT", "ComplexConv2d", "ComplexConvTranspose2d", "RealConv2d", "RealConvTranspose2d", "ComplexBatchNorm", "cPReLU",
                "complex_cat", "NavieComplexLSTM", "BaseModel"):
        from . import models
        return getattr(models, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

_FE_CACHE = {}


def init_kernels(win_len, win_inc, fft_len, win_type=None, invers=False):
    """tools_for_model.py:16-33: (kernel [2 NF, 1, win_len], window [1, win_len, 1]) of ConvSTFT (invers=False) / ConviSTFT (invers=True)."""
    from .frontend_consts import stft_kernels
    K, Kinv, w = stft_kernels(win_len, fft_len, win_type)
    return (Kinv if invers else K), w


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def _fe_runtime(key, make):
    """Runtime of the parameter-free plan `make()`, cached per shape; the device is the key's last element."""
    return cached(_FE_CACHE, key, lambda: Runtime.owned(make(), key[-1]))


class _StftFunction(torch.autograd.Function):
    """float32 [B, L] -> the real image [B, F, T, 2] of torch.stft.  Forward: the TorchSTFT plan, as `stft` without a gradient.  Backward: the
    TorchSTFTAdj plan (csrc/plan_frontend.cpp) on the cotangent alone - nothing is saved, so any number of forwards may precede their backwards."""

    @staticmethod
    def forward(ctx, y, n_fft, hop_length, win_length):
        ctx.geom = (n_fft, hop_length, win_length)
        ctx.L = y.shape[1]
        return torch.view_as_real(stft(y.detach(), n_fft, hop_length, win_length))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        n_fft, hop, win = ctx.geom
        B, F, T, _ = g.shape
        L = ctx.L
        rt = _fe_runtime(("stft_adj", B, L, n_fft, hop, win, str(g.device)),
                         lambda: Plan(B, L, win_len=win, win_inc=hop, fft_len=n_fft, model="TorchSTFTAdj"))
        rt.io("grad_spec", (B, F, T, 2)).copy_(g)
        rt.run(PHASE_FWD)
        return rt.io("grad_wav", (B, L)).clone(), None, None, None


class _IstftFunction(torch.autograd.Function):
    """The real pair [B, F, T, 2] (float32) -> [B, L].  Forward: the TorchISTFT plan, as `istft` without a gradient.  Backward: the TorchISTFTAdj plan."""

    @staticmethod
    def forward(ctx, features, n_fft, hop_length, win_length, L):
        ctx.geom = (n_fft, hop_length, win_length)
        ctx.fshape = tuple(features.shape)
        return istft(features.detach(), n_fft, hop_length, win_length, length=L)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        n_fft, hop, win = ctx.geom
        B, F, T, _ = ctx.fshape
        L = g.shape[1]
        rt = _fe_runtime(("istft_adj", B, L, T, n_fft, hop, win, str(g.device)),
                         lambda: Plan(B, L, win_len=win, win_inc=hop, fft_len=n_fft, model="TorchISTFTAdj"))
        rt.io("grad_wav", (B, L)).copy_(g)
        rt.run(PHASE_FWD)
        return rt.io("grad_spec", (B, F, T, 2)).clone(), None, None, None, None


def stft(y, n_fft=cfg.fft_len, hop_length=int(cfg.win_len * cfg.ola_ratio), win_length=cfg.win_len):
    """tools_for_model.py:628-648: torch.stft(center=True, reflect, hann_window(win_length)) -> complex64 [B, F, T].  Differentiable in `y` at
    n_fft 512; at any other n_fft a `y` that requires a gradient is refused here, at the forward call."""
    assert y.dim() == 2
    if not y.is_cuda:
        raise RuntimeError("sefd stft runs on the MI355X only (cuda tensors); there is no CPU fallback")
    if _wants_grad(y):
        if n_fft != 512:
            raise NotImplementedError(f"sefd stft: the backward is built for n_fft 512 only (the inverse-FFT frame kernel), got n_fft {n_fft} with an input that requires a gradient")
        return torch.view_as_complex(_StftFunction.apply(y.float().contiguous(), n_fft, hop_length, win_length))
    y = y.detach().float().contiguous()
    B, L = y.shape
    rt = _fe_runtime((B, L, n_fft, hop_length, win_length, str(y.device)),
                     lambda: Plan(B, L, win_len=win_length, win_inc=hop_length, fft_len=n_fft, model="TorchSTFT"))
    rt.io("wav", (B, L)).copy_(y)
    rt.run(PHASE_FWD)
    return torch.view_as_complex(rt.io("spec", (B, rt.plan.NF, rt.plan.T, 2)).clone())


def istft(features, n_fft=cfg.fft_len, hop_length=int(cfg.win_len * cfg.ola_ratio), win_length=cfg.win_len, length=None, use_mag_phase=False):
    """tools_for_model.py:651-680: wrapper of torch.istft(window=hann_window(win_length), center=True, length=length) -> [B, L].
    `features`: complex [B, F, T], the reference's real-pair [B, F, T, 2] (which torch >= 2 rejects in the reference itself,
    SURVEY Q9 - accepted here through view_as_complex semantics), or (mag, phase) with use_mag_phase."""
    if use_mag_phase:
        assert isinstance(features, (tuple, list))
        mag, phase = features
        features = torch.stack([mag * torch.cos(phase), mag * torch.sin(phase)], dim=-1)
    if torch.is_complex(features):
        features = torch.view_as_real(features)
    if not features.is_cuda:
        raise RuntimeError("sefd istft runs on the MI355X only (cuda tensors); there is no CPU fallback")
    B, F, T, two = features.shape
    assert two == 2 and F == n_fft // 2 + 1
    L = int(length) if length is not None else hop_length * (T - 1)
    if _wants_grad(features):
        # every entry form arrives here as the real pair through differentiable torch ops (view_as_real; mag x (cos, sin), whose autograd is the polar adjoint)
        return _IstftFunction.apply(features.float().contiguous(), n_fft, hop_length, win_length, L)
    features = features.detach().float().contiguous()

    def make():
        plan = Plan(B, L, win_len=win_length, win_inc=hop_length, fft_len=n_fft, model="TorchISTFT")
        if plan.T != T:
            raise ValueError(f"istft: {T} frames do not match length {L} at hop {hop_length} (expected {plan.T})")
        return plan
    rt = _fe_runtime(("istft", B, L, T, n_fft, hop_length, win_length, str(features.device)), make)
    rt.io("spec", (B, F, T, 2)).copy_(features)
    rt.run(PHASE_FWD)
    return rt.io("wav", (B, L)).clone()


def _targets(noisy, clean, want_mag, want_phase, want_cirm):
    L_ = _lib.lib()
    nr = torch.view_as_real(noisy.contiguous())
    n = noisy.numel()
    mag = torch.empty(noisy.shape, dtype=torch.float32, device=noisy.device) if want_mag else None
    ph = torch.empty(noisy.shape, dtype=torch.float32, device=noisy.device) if want_phase else None
    cirm = torch.empty(noisy.shape + (2,), dtype=torch.float32, device=noisy.device) if want_cirm else None
    cr = torch.view_as_real(clean.contiguous()) if clean is not None else None
    rc = L_.sefd_fsn_targets(_vp(nr), _vp(cr), n, _vp(mag), _vp(ph), _vp(cirm), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError(f"sefd_fsn_targets failed ({rc})")
    return mag, ph, cirm


def _targets_backward(noisy_ri, clean_ri, g_mag, g_phase, g_cirm, want_noisy, want_clean):
    """sefd_fsn_targets_backward on real-pair images [..., 2]: (d noisy, d clean), each in its argument's shape or None."""
    n = noisy_ri.numel() // 2
    g = [None if t is None else t.float().contiguous() for t in (g_mag, g_phase, g_cirm)]
    dn = torch.empty_like(noisy_ri) if want_noisy else None
    dc = torch.empty_like(clean_ri) if want_clean else None
    rc = _lib.lib().sefd_fsn_targets_backward(_vp(noisy_ri), _vp(clean_ri), n, _vp(g[0]), _vp(g[1]), _vp(g[2]), _vp(dn), _vp(dc),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError(f"sefd_fsn_targets_backward failed ({rc})")
    return dn, dc


class _MagPhaseFunction(torch.autograd.Function):
    """Real pair [..., 2] -> (|z|, angle z).  Where |z| == 0 the gradient is 0 (torch: NaN), the rule of ConvSTFT's (mags, phase)."""

    @staticmethod
    def forward(ctx, z_ri):
        ctx.save_for_backward(z_ri)
        mag, ph, _ = _targets(torch.view_as_complex(z_ri), None, True, True, False)
        return mag, ph

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mag, g_phase):
        (z_ri,) = ctx.saved_tensors
        return _targets_backward(z_ri, None, g_mag, g_phase, None, True, False)[0]


class _CirmFunction(torch.autograd.Function):
    """Real pairs of noisy and clean [..., 2] -> the compressed ratio mask [..., 2]; gradients to both."""

    @staticmethod
    def forward(ctx, noisy_ri, clean_ri):
        ctx.save_for_backward(noisy_ri, clean_ri)
        return _targets(torch.view_as_complex(noisy_ri), torch.view_as_complex(clean_ri), False, False, True)[2]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        noisy_ri, clean_ri = ctx.saved_tensors
        dn, dc = _targets_backward(noisy_ri, clean_ri, None, None, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dn, dc


def _real_pair(z):
    return torch.view_as_real(z.to(torch.complex64)).contiguous()


def mag_phase(complex_tensor):
    """tools_for_model.py:683-684.  Differentiable; where the magnitude is exactly 0 the gradient is 0 (torch.abs / torch.angle: NaN)."""
    if _wants_grad(complex_tensor):
        if not complex_tensor.is_cuda:
            raise RuntimeError("sefd mag_phase runs on the MI355X only (cuda tensors); there is no CPU fallback")
        return _MagPhaseFunction.apply(_real_pair(complex_tensor))
    mag, ph, _ = _targets(complex_tensor, None, True, True, False)
    return mag, ph


def build_complex_ideal_ratio_mask(noisy, clean):
    """tools_for_model.py:687-705 (+ compress_cIRM K=10, C=0.1): complex [B,F,T] x2 -> [B,F,T,2].  Differentiable in both arguments."""
    if _wants_grad(noisy, clean):
        if not (noisy.is_cuda and clean.is_cuda):
            raise RuntimeError("sefd build_complex_ideal_ratio_mask runs on the MI355X only (cuda tensors); there is no CPU fallback")
        return _CirmFunction.apply(_real_pair(noisy), _real_pair(clean))
    return _targets(noisy, clean, False, False, True)[2]


def compress_cIRM(mask, K=10, C=0.1):
    """tools_for_model.py:707-717: (-inf, inf) -> (-K, K), mask <= -100 taken as -100.  Tensors (any device, differentiable through torch) and numpy
    arrays / scalars, as the reference: K (1 - e^{-C m}) / (1 + e^{-C m})."""
    if torch.is_tensor(mask):
        m = torch.where(mask <= -100, torch.full_like(mask, -100.0), mask)
        e = torch.exp(-C * m)
    else:
        m = np.where(np.asarray(mask) <= -100, -100.0, mask)
        e = np.exp(-C * m)
    return K * (1 - e) / (1 + e)


def decompress_cIRM(mask, K=10, limit=9.9):
    """tools_for_model.py:720-723 (validation path; element-wise torch is plumbing here, not the training hot path)."""
    mask = limit * (mask >= limit) - limit * (mask <= -limit) + mask * (torch.abs(mask) < limit)
    return -K * torch.log((K - mask) / (K + mask))


def Bar(iterable, *args, **kwargs):
    """tools_for_model.py:1396-1416 wraps every loader in a console progress bar; the training loops only iterate it."""
    return iterable
