"""`sefd::` PyTorch custom ops (torch.library) over the C ABI of libsefd_hip.so - the dispatcher-level surface of the hot path.

The reference has no native op surface (everything below `models.py` is ATen / cuDNN); north_star asks for the HIP path
"exposed as PyTorch-ROCm custom ops".  Each op below is a thin, allocation-explicit wrapper of ONE C-ABI entry point of include/sefd.h
(same argument meaning, cuda tensors only, current HIP stream), registered with a fake (meta) implementation so that it traces, and - for
the losses and BaseModel's norms and unfold - with a registered backward.  The nn.Module mirrors (`models.py`, `tools_for_loss.py`) call the same C entry points directly
through ctypes (no dispatcher hop inside the fused train step); `tests/test_gpu_ops.py::test_torch_library_ops` pins op == mirror.

    torch.ops.sefd.loss(kind, est, tgt)                       scalar loss of tools_for_loss.py:17-94 (kind 0 MSE, 1 SDR, 2 SI-SNR, 3 SI-SDR),
                                                              differentiable w.r.t. est (rows of any length) and tgt (rows <= 16 elements)
    torch.ops.sefd.adam_step_(param, grad, m, v, step, ...)   torch.optim.Adam.step on flat fp32 buffers, in place
    torch.ops.sefd.mix_snr(speech, bank, start, snr_db, q)   generate_noisy_data.py:46-67 on the GPU
    torch.ops.sefd.composite_measures(clean, enh, fs)         composite.m frame analysis: [B, 3] fp64 (trimmed LLR, trimmed WSS, segSNR)
    torch.ops.sefd.stoi(clean, enh, fs, extended=False)       STOI / ESTOI per utterance: [B] fp64, differentiable in enh (tools_for_estimate.stoi_batch)
    torch.ops.sefd.plan_run(handle, phase, arenas)           one phase (0 forward, 1 backward) of a planned model: sefd_plan_run
    torch.ops.sefd.basemodel_norm(x, kind, sample_len)        BaseModel's seven norms (tools_for_model.py:881-1104) by number, differentiable w.r.t. x
    torch.ops.sefd.unfold(x, n)                               BaseModel.unfold (tools_for_model.py:806-837), differentiable w.r.t. x
"""
import ctypes as C
from typing import List, Tuple

import torch

from . import _lib

ROWS_MAX_L = 16


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("sefd ops run on the MI355X only (cuda tensors); there is no CPU fallback")


# ---------------------------------------------------------------------------------------------- losses
@torch.library.custom_op("sefd::loss_forward", mutates_args=())
def loss_forward(kind: int, est: torch.Tensor, tgt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss [], workspace): est / tgt fp32 [R, L] contiguous."""
    _need_cuda(est, tgt)
    L_ = _lib.lib()
    R, L = est.shape
    out = torch.empty((), dtype=torch.float32, device=est.device)
    if L <= ROWS_MAX_L:
        ws = torch.empty(L_.sefd_loss_rows_ws_floats(R), dtype=torch.float32, device=est.device)
        rc = L_.sefd_loss_rows_forward(kind, _vp(est), _vp(tgt), R, L, _vp(ws), _vp(out), _stream())
    else:
        ws = torch.empty(L_.sefd_loss_ws_floats(R), dtype=torch.float32, device=est.device)
        rc = L_.sefd_loss_forward(kind, _vp(est), _vp(tgt), R, L, _vp(ws), _vp(out), _stream())
    if rc != 0:
        raise RuntimeError(f"sefd::loss_forward failed ({rc})")
    return out, ws


@loss_forward.register_fake
def _(kind, est, tgt):
    # the size functions are host-only arithmetic: a traced graph sees the shape eager execution allocates
    L_ = _lib.lib()
    R, L = est.shape
    n = L_.sefd_loss_rows_ws_floats(R) if L <= ROWS_MAX_L else L_.sefd_loss_ws_floats(R)
    return est.new_empty(()), est.new_empty((n,))


@torch.library.custom_op("sefd::loss_backward", mutates_args=())
def loss_backward(kind: int, est: torch.Tensor, tgt: torch.Tensor, ws: torch.Tensor, grad_scale: torch.Tensor,
                  want_est: bool, want_tgt: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d loss / d est, d loss / d tgt) * grad_scale; a gradient that was not asked for is an empty tensor."""
    _need_cuda(est, tgt, ws, grad_scale)
    L_ = _lib.lib()
    R, L = est.shape
    ge = torch.empty_like(est) if want_est else est.new_empty((0,))
    gt = torch.empty_like(tgt) if want_tgt else tgt.new_empty((0,))
    if L <= ROWS_MAX_L:
        rc = L_.sefd_loss_rows_backward(kind, _vp(est), _vp(tgt), R, L, _vp(ws), _vp(grad_scale), _vp(ge) if want_est else None,
                                        _vp(gt) if want_tgt else None, _stream())
    else:
        if want_tgt:
            raise NotImplementedError("sefd::loss: rows longer than %d elements are differentiable w.r.t. the estimate only" % ROWS_MAX_L)
        rc = L_.sefd_loss_backward(kind, _vp(est), _vp(tgt), R, L, _vp(ws), _vp(grad_scale), _vp(ge), _stream()) if want_est else 0
    if rc != 0:
        raise RuntimeError(f"sefd::loss_backward failed ({rc})")
    return ge, gt


@loss_backward.register_fake
def _(kind, est, tgt, ws, grad_scale, want_est, want_tgt):
    return (torch.empty_like(est) if want_est else est.new_empty((0,))), (torch.empty_like(tgt) if want_tgt else tgt.new_empty((0,)))


@torch.library.custom_op("sefd::loss", mutates_args=())
def loss(kind: int, est: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    """The value the fused kernels compute: MSE itself, the NEGATED metric for SDR / SI-SNR / SI-SDR (what model.loss returns).  Argument
    roles: SDR est = s2, tgt = s1; SI-SNR est = s1, tgt = s2; SI-SDR est = estimation, tgt = reference (tools_for_loss.py:29-94)."""
    e2 = est.float().contiguous().view(-1, est.shape[-1])
    t2 = tgt.float().contiguous().view(-1, tgt.shape[-1])
    return loss_forward(kind, e2, t2)[0].clone()


@loss.register_fake
def _(kind, est, tgt):
    return est.new_empty((), dtype=torch.float32)


def _loss_setup(ctx, inputs, output):
    kind, est, tgt = inputs
    ctx.kind = kind
    ctx.save_for_backward(est, tgt)


def _loss_bwd(ctx, g):
    est, tgt = ctx.saved_tensors
    e2 = est.float().contiguous().view(-1, est.shape[-1])
    t2 = tgt.float().contiguous().view(-1, tgt.shape[-1])
    _, ws = loss_forward(ctx.kind, e2, t2)          # five sums per row: recomputed rather than carried through the dispatcher
    ge, gt = loss_backward(ctx.kind, e2, t2, ws, g.float().contiguous().view(1), ctx.needs_input_grad[1], ctx.needs_input_grad[2])
    return None, (ge.view(est.shape) if ctx.needs_input_grad[1] else None), (gt.view(tgt.shape) if ctx.needs_input_grad[2] else None)


loss.register_autograd(_loss_bwd, setup_context=_loss_setup)


# ---------------------------------------------------------------------------------------------- BaseModel norms and unfold
def _bm_need(x, dims):
    _need_cuda(x)
    if x.dtype != torch.float32:
        raise TypeError(f"sefd BaseModel ops take float32 tensors, got {x.dtype}")
    if x.dim() not in dims:
        raise ValueError(f"sefd BaseModel ops: a {x.dim()}-D input where {' or '.join(map(str, dims))}-D is expected")


@torch.library.custom_op("sefd::basemodel_norm_forward", mutates_args=())
def basemodel_norm_forward(x: torch.Tensor, kind: int, sample_len: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, workspace) of sefd_norm_forward: x fp32 contiguous, [B, C, F, T] for kinds 0..3, [B, F, T] for kinds 4..6."""
    from .models import bm_norm_forward
    _bm_need(x, (4,) if kind < 4 else (3,))
    return bm_norm_forward(x, kind, sample_len)


@basemodel_norm_forward.register_fake
def _(x, kind, sample_len):
    from .models import _bm_geometry, bm_ws_floats
    return torch.empty_like(x), x.new_empty((bm_ws_floats(kind, *_bm_geometry(kind, x.shape)),))      # Python arithmetic: symbolic shapes trace


@torch.library.custom_op("sefd::basemodel_norm_backward", mutates_args=("ws",))
def basemodel_norm_backward(x: torch.Tensor, grad_y: torch.Tensor, ws: torch.Tensor, kind: int, sample_len: int) -> torch.Tensor:
    """grad_x of sefd_norm_backward; ws is the forward's, whose scratch part this call overwrites (the statistics stay).  Because of that write,
    autograd's version check refuses a SECOND backward through a retained graph of sefd::basemodel_norm; the BaseModel methods take one."""
    from .models import bm_norm_backward
    _bm_need(x, (4,) if kind < 4 else (3,))
    _need_cuda(grad_y, ws)
    return bm_norm_backward(x, grad_y, ws, kind, sample_len)


@basemodel_norm_backward.register_fake
def _(x, grad_y, ws, kind, sample_len):
    return torch.empty_like(x)


def _bm_norm_setup(ctx, inputs, output):
    x, ctx.kind, ctx.sample_len = inputs
    ctx.save_for_backward(x, output[1])                 # the input and the forward's statistics: nothing is recomputed


def _bm_norm_bwd(ctx, gy, gws):
    x, ws = ctx.saved_tensors
    return basemodel_norm_backward(x, gy.contiguous(), ws, ctx.kind, ctx.sample_len), None, None


basemodel_norm_forward.register_autograd(_bm_norm_bwd, setup_context=_bm_norm_setup)

# sefd::basemodel_norm(x, kind, sample_len) -> y is the forward op's first output: a composite, so autograd and tracing see the op underneath
torch.library.define("sefd::basemodel_norm", "(Tensor x, int kind, int sample_len) -> Tensor")


@torch.library.impl("sefd::basemodel_norm", "CompositeImplicitAutograd")
def basemodel_norm(x, kind, sample_len):
    """BaseModel's norms (tools_for_model.py:881-1104) by number: 0..3 = offline_laplace, cumulative_laplace, offline_gaussian, cumulative_layer on
    [B, C, F, T]; 4..6 = forgetting, sband_forgetting, hybrid on [B, F, T] with their training sample length."""
    return torch.ops.sefd.basemodel_norm_forward(x.contiguous(), kind, sample_len)[0]


@torch.library.custom_op("sefd::unfold", mutates_args=())
def unfold(x: torch.Tensor, n: int) -> torch.Tensor:
    """BaseModel.unfold (tools_for_model.py:806-837): [B, C, F, T] -> [B, F, C, 2 n + 1, T] (n < 1: the permute)."""
    from .models import bm_unfold_forward
    _bm_need(x, (4,))
    return bm_unfold_forward(x.contiguous(), max(n, 0))


@unfold.register_fake
def _(x, n):
    B, Cc, F, T = x.shape
    return x.new_empty((B, F, Cc, 2 * max(n, 0) + 1, T))


@torch.library.custom_op("sefd::unfold_backward", mutates_args=())
def unfold_backward(grad_out: torch.Tensor, B: int, Cc: int, F: int, T: int, n: int) -> torch.Tensor:
    from .models import bm_unfold_backward
    _bm_need(grad_out, (5,))
    return bm_unfold_backward(grad_out.contiguous(), (B, Cc, F, T), max(n, 0))


@unfold_backward.register_fake
def _(grad_out, B, Cc, F, T, n):
    return grad_out.new_empty((B, Cc, F, T))


def _unfold_setup(ctx, inputs, output):
    x, ctx.n = inputs
    ctx.shape = tuple(x.shape)


def _unfold_bwd(ctx, g):
    return unfold_backward(g, *ctx.shape, ctx.n), None


unfold.register_autograd(_unfold_bwd, setup_context=_unfold_setup)


# ---------------------------------------------------------------------------------------------- Adam
@torch.library.custom_op("sefd::adam_step_", mutates_args=("param", "exp_avg", "exp_avg_sq"))
def adam_step_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int, lr: float,
               beta1: float, beta2: float, eps: float, grad_scale: float) -> None:
    """torch.optim.Adam.step (train_interface.py:59 defaults) on flat fp32 buffers: ONE launch (sefd_adam_step); step counts from 1."""
    _need_cuda(param, grad, exp_avg, exp_avg_sq)
    rc = _lib.lib().sefd_adam_step(_vp(param), _vp(grad), _vp(exp_avg), _vp(exp_avg_sq), param.numel(), step, lr, beta1, beta2, eps, grad_scale, _stream())
    if rc != 0:
        raise RuntimeError(f"sefd::adam_step_ failed ({rc})")


# ---------------------------------------------------------------------------------------------- SNR mixing
@torch.library.custom_op("sefd::mix_snr", mutates_args=())
def mix_snr(speech: torch.Tensor, noise_bank: torch.Tensor, noise_start: torch.Tensor, snr_db: torch.Tensor, quantize: bool) -> torch.Tensor:
    """generate_noisy_data.py:46-67 for a batch (sefd_mix_snr): speech [B, L], flat noise bank, per-utterance noise offsets and SNRs -> noisy
    [B, L]; quantize reproduces the int16 file round trip of the offline script."""
    from .dataloader import mix_snr as _mix
    return _mix(speech, noise_bank, noise_start, snr_db, quantize)


@mix_snr.register_fake
def _(speech, noise_bank, noise_start, snr_db, quantize):
    return torch.empty_like(speech, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- composite measure
@torch.library.custom_op("sefd::composite_measures", mutates_args=())
def composite_measures(clean: torch.Tensor, enhanced: torch.Tensor, fs: int) -> torch.Tensor:
    """composite.m:56-75 frame analysis for a batch (sefd_composite_frames): clean / enhanced [B, L] -> fp64 [B, 3] = (95 % trimmed mean
    LLR, 95 % trimmed mean WSS, mean segSNR) per utterance; tools_for_estimate.composite_batch adds PESQ and the regression."""
    from .tools_for_estimate import composite_frames
    return composite_frames(clean, enhanced, fs)


@composite_measures.register_fake
def _(clean, enhanced, fs):
    return clean.new_empty((clean.shape[0], 3), dtype=torch.float64)


@torch.library.custom_op("sefd::stoi", mutates_args=())
def stoi(clean: torch.Tensor, enhanced: torch.Tensor, fs: int, extended: bool = False) -> torch.Tensor:
    """STOI of a batch on the device (sefd_stoi_gpu, the arithmetic of tools_for_estimate.cal_stoi): clean / enhanced [B, L] at rate fs ->
    fp64 [B]; extended=True: extended STOI.  Differentiable in `enhanced` (sefd_stoi_backward)."""
    from .tools_for_estimate import stoi_batch
    return stoi_batch(clean, enhanced, fs, extended)


@stoi.register_fake
def _(clean, enhanced, fs, extended=False):
    return clean.new_empty((clean.shape[0],), dtype=torch.float64)


def _stoi_setup(ctx, inputs, output):
    clean, enhanced, fs, extended = inputs
    if ctx.needs_input_grad[0]:
        raise NotImplementedError("sefd::stoi differentiates `enhanced` only: `clean` requires a gradient, and the clean signal (with the "
                                  "frames it selects) is a constant of the score")
    ctx.save_for_backward(clean, enhanced)
    ctx.fs, ctx.extended = fs, extended


def _stoi_bwd(ctx, g):
    # the op returns the scores alone, so the backward scores again with the keep flag (tools_for_loss.stoi_loss holds its workspace instead)
    from . import tools_for_estimate as te
    clean, enhanced = ctx.saved_tensors
    flags = te.STOI_KEEP | (te.STOI_EXTENDED if ctx.extended else 0)
    _, ws = te.stoi_forward_raw(clean, enhanced, ctx.fs, flags)
    grad = te.stoi_backward_raw(enhanced.shape[0], enhanced.shape[1], ctx.fs, flags, ws, g)
    return None, grad.to(enhanced.dtype), None, None


stoi.register_autograd(_stoi_bwd, setup_context=_stoi_setup)


# ---------------------------------------------------------------------------------------------- planned models
@torch.library.custom_op("sefd::plan_run", mutates_args=("arenas",))
def plan_run(handle: int, phase: int, arenas: List[torch.Tensor]) -> None:
    """One whole phase of a planned model (sefd_plan_run): `handle` = the sefd_plan* (Plan.h), `arenas` = the six arena tensors in Arena
    order (workspace, parameters, gradients, BatchNorm buffers, constants, I/O block) - the caller owns all device memory."""
    _need_cuda(*arenas)
    ptrs = (C.c_void_p * len(arenas))(*[C.c_void_p(a.data_ptr()) for a in arenas])
    rc = _lib.lib().sefd_plan_run(C.c_void_p(handle), phase, 0, -1, ptrs, _stream())
    if rc != 0:
        raise RuntimeError(f"sefd::plan_run failed ({rc})")
