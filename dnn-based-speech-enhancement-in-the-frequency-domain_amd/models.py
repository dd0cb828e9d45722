"""Drop-in `models` surface: `DCCRN` with the reference's constructor, forward/loss signatures and state_dict keys
(reference models.py:15-323), computed by the gfx950 HIP library through its C ABI.

The nn.Module tree only *holds* parameters (same names, shapes, init and registration order as the reference, so
checkpoints interchange - SURVEY.md Appendix B).  All arithmetic - STFT, complex convs, BatchNorm+PReLU, complex
LSTM, mask, iSTFT, losses, backward, Adam - runs in `libsefd_hip.so`; there is no PyTorch/CPU fallback.
"""
import ctypes as C
import weakref

import torch
import torch.nn as nn

from . import config as cfg
from . import _lib
from .frontend_consts import stft_kernels
from .plan import PHASE_BWD, PHASE_FWD, RUN_WAVE_ONLY, Plan
from .runtime import Runtime, cached
from . import tools_for_loss as tfl


# ------------------------------------------------------------------------------------------ parameter holders
def _default_fft_len(win_len):
    # tools_for_model.py:41-42: np.int(2 ** np.ceil(np.log2(win_len))) - `np.int` no longer exists in numpy; this is the value it meant
    return 1 << max(int(win_len) - 1, 0).bit_length()


def _frontend_runtime(mod, model, B, n, device, complex_io):
    """Runtime of a ConvSTFT / ConviSTFT module at batch B and n = clip length L / frame count T, cached on the module."""
    return cached(mod._runtimes, (model, B, n, str(device), complex_io), lambda: Runtime.owned(
        Plan(B, n, win_len=mod.win_len, win_inc=mod.stride, fft_len=mod.dim, model=model, win_type=mod.win_type,
             feature_type="complex" if complex_io else "real"), device))


def _check_frontend_input(name, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"sefd {name} runs on the MI355X only (inputs must be a cuda tensor); there is no CPU fallback")
        if t.dtype != torch.float32:
            raise RuntimeError(f"sefd {name} is built for float32 only, got {t.dtype}")


_STALE = "sefd: a later forward of the same shape overwrote the activations this backward needs"


def _next_dropout_seed(rt):
    rt.view("io.seed").view(torch.int32)[:1].add_(1)        # fresh dropout masks every forward (device-side counter)


class _PlanFunction(torch.autograd.Function):
    """One plan with a forward and a backward phase at its IO boundary, described by views into the runtime's arenas: `ins` (where the input tensors go),
    `outs` (what is returned, as float32 copies), `gouts` (where the cotangents go; a missing one zero-fills its view), `gins` (the input gradients, one per
    leading input; inputs beyond them get none) and `zero` (views cleared before every backward).  The tensors after the inputs are the owner's parameters:
    each gets its slice of one clone of the flat gradient arena.
    The activations the backward phase reads live in the runtime's arenas.  keep None: a later forward of the same shape invalidates this one's backward
    (stamp; `stale` is the message).  keep = views (the parameter-free frontends: the spectrum under (mags, phase), the polar inputs): they are cloned when
    an input requires grad and put back before the backward phase, so any number of forwards of one shape may precede their backwards.
    The backward phase runs only when autograd asks for it; double backward is not supported."""

    @staticmethod
    def forward(ctx, rt, owner, b, *tensors):
        for dst, t in zip(b["ins"], tensors):
            dst.copy_(t.reshape(dst.shape))
        if b["seed"]:
            _next_dropout_seed(rt)
        rt.run(PHASE_FWD)
        rt.stamp += 1                                # the saved activations live in the runtime's arena, not in ctx
        ctx.rt, ctx.owner, ctx.b, ctx.stamp = rt, owner, b, rt.stamp
        ctx.in_shapes = [t.shape for t in tensors[:len(b["gins"])]]
        if b["keep"] is not None and any(ctx.needs_input_grad):
            ctx.save_for_backward(*[v.clone() for v in b["keep"]])
        res = tuple(v.to(torch.float32, copy=True) for v in b["outs"])      # activation dtype -> fp32 at the boundary
        return res if len(res) > 1 else res[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        rt, owner, b = ctx.rt, ctx.owner, ctx.b
        if b["keep"] is not None:
            for v, t in zip(b["keep"], ctx.saved_tensors):
                v.copy_(t)
        elif ctx.stamp != rt.stamp:
            raise RuntimeError(b["stale"])
        for v in b["zero"]:
            v.zero_()
        for dst, g in zip(b["gouts"], grads):
            if g is None:
                dst.zero_()
            else:
                dst.copy_(g.reshape(dst.shape))
        rt.run(PHASE_BWD)
        pgrads = ()
        if owner is not None:
            flat = owner._flat_grad.clone()
            pgrads = tuple(flat[off:off + n].view(shape) for (off, n, shape) in owner._param_slices)
        gins = tuple(v.clone().reshape(ish) for v, ish in zip(b["gins"], ctx.in_shapes))
        return (None,) * 3 + gins + (None,) * (len(b["ins"]) - len(gins)) + pgrads


def _plan_apply(rt, owner, tensors, ins, outs, gouts, gins=(), zero=(), keep=None, seed=False, stale=_STALE):
    params = [p for _, p in owner._trainable()] if owner is not None else []
    return _PlanFunction.apply(rt, owner, dict(ins=ins, outs=outs, gouts=gouts, gins=gins, zero=zero, keep=keep, seed=seed, stale=stale), *tensors, *params)


class ConvSTFT(nn.Module):
    """tools_for_model.py:36-68, same constructor, buffer (`weight`) and forward: [B, L] or [B, 1, L] -> [B, 2 NF, T] ('complex': real block, then
    imaginary block) or (mags, phase), each [B, NF, T].  Differentiable in the waveform; computed by the ConvSTFT plan (csrc/plan_frontend.cpp).
    Where a bin's magnitude is exactly 0 the gradient of (mags, phase) is 0 (the reference: NaN).  float32 cuda tensors only."""

    def __init__(self, win_len, win_inc, fft_len=None, win_type='hamming', feature_type='real', fix=True):
        super().__init__()
        fft_len = _default_fft_len(win_len) if fft_len is None else fft_len
        K, _, _ = stft_kernels(win_len, fft_len, win_type)
        self.register_buffer('weight', K)
        self.feature_type, self.stride, self.win_len, self.dim = feature_type, win_inc, win_len, fft_len
        self.fft_len, self.win_type = fft_len, win_type
        self._runtimes = {}

    def forward(self, inputs):
        _check_frontend_input("ConvSTFT", inputs)
        if inputs.dim() not in (2, 3) or (inputs.dim() == 3 and inputs.shape[1] != 1):
            raise ValueError(f"ConvSTFT takes [B, L] or [B, 1, L], got {tuple(inputs.shape)}")
        B, L = inputs.shape[0], inputs.shape[-1]
        rt = _frontend_runtime(self, "ConvSTFT", B, L, inputs.device, self.feature_type == 'complex')
        NF, T = rt.plan.NF, rt.plan.T
        if self.feature_type == 'complex':
            outs, gouts, keep = [rt.io("out", (B, 2 * NF, T))], [rt.io("grad_out", (B, 2 * NF, T))], []
        else:
            outs = [rt.io("mags", (B, NF, T)), rt.io("phase", (B, NF, T))]
            gouts, keep = [rt.io("grad_mags", (B, NF, T)), rt.io("grad_phase", (B, NF, T))], [rt.view("spec")]
        return _plan_apply(rt, None, (inputs,), [rt.io("wav", (B, L))], outs, gouts, [rt.io("grad_wav", (B, L))], keep=keep)


class ConviSTFT(nn.Module):
    """tools_for_model.py:71-112, same constructor, buffers (`weight`, `window`, `enframe`) and forward: [B, 2 NF, T], or mags [B, NF, T] with
    `phase`, -> [B, 1, (T - 1) hop + win_len - 2 (win_len - hop)].  No clamp; the overlap-add is divided by coff + 1e-8.  Differentiable in
    `inputs` and `phase`; computed by the ConviSTFT plan (csrc/plan_frontend.cpp).  float32 cuda tensors only."""

    def __init__(self, win_len, win_inc, fft_len=None, win_type='hamming', feature_type='real', fix=True):
        super().__init__()
        fft_len = _default_fft_len(win_len) if fft_len is None else fft_len
        _, Kinv, w = stft_kernels(win_len, fft_len, win_type)
        self.register_buffer('weight', Kinv)
        self.register_buffer('window', w)
        self.register_buffer('enframe', torch.eye(win_len)[:, None, :])
        self.feature_type, self.stride, self.win_len, self.dim = feature_type, win_inc, win_len, fft_len
        self.fft_len, self.win_type = fft_len, win_type
        self._runtimes = {}

    def forward(self, inputs, phase=None):
        _check_frontend_input("ConviSTFT", *([inputs] if phase is None else [inputs, phase]))
        NF = self.dim // 2 + 1
        want = NF if phase is not None else 2 * NF
        if inputs.dim() != 3 or inputs.shape[1] != want or (phase is not None and phase.shape != inputs.shape):
            raise ValueError(f"ConviSTFT takes [B, {2 * NF}, T], or mags and phase [B, {NF}, T] each; got {tuple(inputs.shape)}"
                             + ("" if phase is None else f" and {tuple(phase.shape)}"))
        B, T = inputs.shape[0], inputs.shape[2]
        # the input form decides the plan, not feature_type: the reference's forward looks at `phase` alone (tools_for_model.py:96-99)
        rt = _frontend_runtime(self, "ConviSTFT", B, T, inputs.device, phase is None)
        Lout = (T - 1) * self.stride + self.win_len - 2 * (self.win_len - self.stride)
        if phase is None:
            ins, gins, args, keep = [rt.io("in", (B, 2 * NF, T))], [rt.io("grad_in", (B, 2 * NF, T))], (inputs,), []
        else:
            ins = [rt.io("mags", (B, NF, T)), rt.io("phase", (B, NF, T))]
            gins, args, keep = [rt.io("grad_mags", (B, NF, T)), rt.io("grad_phase", (B, NF, T))], (inputs, phase), ins
        wav = _plan_apply(rt, None, args, ins, [rt.io("wav", (B, Lout))], [rt.io("grad_wav", (B, Lout))], gins, keep=keep)
        return wav.unsqueeze(1)


# (ComplexConv2d, ComplexConvTranspose2d, ComplexBatchNorm, NavieComplexLSTM: below, on _SefdModule)


# ------------------------------------------------------------------------------------------ shared machinery
class _SefdModule(nn.Module):
    """Flat parameter storage + per-(B, L) device runtimes shared by the HIP-backed models."""

    def _init_runtime_state(self):
        self._flat_param = self._flat_grad = self._flat_state = self._flat_nbt = None
        self._param_slices = None
        self._runtimes = {}
        ref = weakref.ref(self)
        for p in self.parameters():              # lets sefd_amd.optim.Adam(model.parameters()) find the model (optim.py)
            p._sefd_owner = ref

    def flatten_parameters(self):
        pass

    def _trainable(self):
        return [(n, p) for n, p in self.named_parameters()]

    def _bn_buffers(self):
        return [(n, b) for n, b in self.named_buffers() if n.rsplit(".", 1)[-1] in ("running_mean", "running_var", "RMr", "RMi", "RVrr", "RVri", "RVii")]

    def _flat_ok(self, device):
        fp = self._flat_param
        if fp is None or fp.device != device:
            return False
        ps = self._trainable()
        first, last = ps[0][1], ps[-1][1]
        off_last, n_last, _ = self._param_slices[-1]
        bn = self._bn_buffers()
        return (first.data_ptr() == fp.data_ptr() and last.data_ptr() == fp.data_ptr() + 4 * off_last
                and (not bn or bn[0][1].data_ptr() == self._flat_state.data_ptr()))

    def _flatten(self, device):
        """Re-home every parameter / BatchNorm buffer as a view of one flat fp32 tensor (the C ABI's arenas)."""
        ps = self._trainable()
        total = sum(p.numel() for _, p in ps)
        flat = torch.empty(total, dtype=torch.float32, device=device)
        slices, off = [], 0
        for _, p in ps:
            n = p.numel()
            flat[off:off + n].copy_(p.data.reshape(-1).to(device=device, dtype=torch.float32))
            p.data = flat[off:off + n].view(p.shape)
            slices.append((off, n, tuple(p.shape)))
            off += n
        bs = self._bn_buffers()
        st = torch.empty(max(sum(b.numel() for _, b in bs), 1), dtype=torch.float32, device=device)
        off = 0
        mods = dict(self.named_modules())
        for name, b in bs:
            n = b.numel()
            st[off:off + n].copy_(b.reshape(-1).to(device=device, dtype=torch.float32))
            mname, leaf = name.rsplit(".", 1) if "." in name else ("", name)         # '': the module itself (a layer on its own)
            mods[mname]._buffers[leaf] = st[off:off + n].view(b.shape)
            off += n
        nbts = [(n, b) for n, b in self.named_buffers() if n.endswith("num_batches_tracked")]
        nbt = torch.zeros(len(nbts), dtype=torch.long, device=device)
        for i, (name, b) in enumerate(nbts):
            nbt[i] = b.to(device)
            mname, leaf = name.rsplit(".", 1) if "." in name else ("", name)
            mods[mname]._buffers[leaf] = nbt[i]
        self._flat_param, self._flat_state, self._flat_nbt = flat, st, nbt
        self._flat_grad = torch.zeros_like(flat)
        self._param_slices = slices
        self._runtimes = {}

    def _runtime(self, B, L, device):
        if not self._flat_ok(device):
            self._flatten(device)
        key = (B, L, bool(self.training), self.masking_mode, self.act_dtype, getattr(self, "_bn_world", 1), getattr(self, "_grad_buckets", 1))

        def make():
            rt = Runtime.bound(self._make_plan(B, L, bool(self.training)), self, device)
            p = rt.plan
            T, NF = p.T, p.NF
            rt.wav = rt.io("wav", (B, L))
            rt.out_wav = rt.io("out_wav", (B, L))
            # ConviSTFT returns the samples the frames cover (tools_for_model.py:111): fewer than L when the hop does not tile the padded clip
            rt.Lout = min(L, (T - 1) * p.cfg.hop + p.cfg.win_len - 2 * (p.cfg.win_len - p.cfg.hop))
            rt.out_real = rt.io("out_real", (B, NF, T))
            rt.out_imag = rt.io("out_imag", (B, NF, T))
            rt.g_wav = rt.io("grad_wav", (B, L))
            rt.g_real = rt.io("grad_real", (B, NF, T))
            rt.g_imag = rt.io("grad_imag", (B, NF, T))
            rt.tgt = rt.io("tgt", (B, L)) if "io.tgt" in p.buffer_names() else None
            return rt
        return cached(self._runtimes, key, make)

    def _forward_plan(self, rt, inputs, targets=None):
        """The model's plan under autograd: (out_real, out_imag, out_wav cropped to the samples the frames cover); gradients to the parameters."""
        tgt = rt.tgt is not None
        return _plan_apply(rt, self, (inputs, targets) if tgt else (inputs,), [rt.wav, rt.tgt] if tgt else [rt.wav],
                           [rt.out_real, rt.out_imag, rt.out_wav[:, :rt.Lout]], [rt.g_real, rt.g_imag, rt.g_wav[:, :rt.Lout]],
                           zero=[rt.g_wav[:, rt.Lout:]],                 # samples behind the last frame are not part of the output
                           stale="sefd: a later forward of the same (batch, length, mode) overwrote the activations this backward needs; "
                                 "call backward before the next forward of that shape")

    def get_params(self, weight_decay=0.0):
        weights, biases = [], []
        for name, param in self.named_parameters():
            (biases if 'bias' in name else weights).append(param)
        return [{'params': weights, 'weight_decay': weight_decay}, {'params': biases, 'weight_decay': 0.0}]

    def _main_loss(self, estimated, target):
        """models.py:315-323 / 558-565."""
        if cfg.loss == 'MSE':
            return tfl.mse(estimated, target)
        elif cfg.loss == 'SDR':
            return -tfl.sdr(target, estimated)
        elif cfg.loss == 'SI-SNR':
            return -(tfl.si_snr(estimated, target))
        elif cfg.loss == 'SI-SDR':
            return -(tfl.si_sdr(target, estimated))
        raise ValueError(cfg.loss)

    # ---- fused training step (what trainer.model_train does per batch, trainer.py:27-39) ---------------------
    def train_step(self, inputs, targets, optimizer, loss_kind=None, exchange=None, perceptual=None):
        """forward -> loss -> backward -> Adam with no autograd bookkeeping over the network; returns the loss as a 0-d device tensor.
        perceptual = 'LMS' | 'PMSQE' | 'STOI' | 'ESTOI': the step of model_perceptual_train (trainer.py:45-82), loss = (main + perceptual) / 2 (DCCRN only:
        CRN + perceptual crashes in the reference)."""
        from .optim import Adam
        if perceptual and not hasattr(self, "_stft_ref"):
            raise NotImplementedError("perceptual losses are defined for DCCRN only (models.py:303-314)")
        if perceptual not in (None, False, "LMS", "PMSQE", "STOI", "ESTOI"):
            raise ValueError(f"unknown perceptual loss {perceptual!r}")
        if not isinstance(optimizer, Adam):
            raise TypeError("train_step needs sefd_amd.optim.Adam (flat fused Adam)")
        kind = tfl.LOSS_KINDS[loss_kind or cfg.loss]
        inputs = inputs.float()
        targets = targets.float().contiguous()
        B, L = inputs.shape
        # SyncBN (exchange.sync_bn): a plan whose BatchNorm counts are global and whose phases are run in the op ranges
        # between its sync points, with the small statistics buffers all-reduced in between (parity with the reference's
        # single-process big batch).  Default: per-rank statistics, whole phases (two-lane backward).
        sync = exchange is not None and exchange.active and getattr(exchange, "sync_bn", False)
        self._bn_world = exchange.world if sync else 1
        # data parallel: plans with two gradient buckets (decoder + LSTM complete before the encoder backward, see ddp.py)
        self._grad_buckets = 2 if (exchange is not None and exchange.active and not sync) else 1
        rt = self._runtime(B, L, inputs.device)
        if rt.Lout != L:
            raise ValueError(f"train_step: the frames of a {L}-sample clip cover {rt.Lout} samples (win_len {rt.plan.cfg.win_len}, win_inc {rt.plan.cfg.hop}); "
                             "the losses compare the estimate with the target sample by sample - crop the clips to a length the hop tiles")
        rt.plan.tolerate_fault = exchange is not None and exchange.active       # a faulty rank keeps its collectives matched; all ranks raise at the guard check
        optimizer.bind(self)
        self._flat_nbt += 1
        stream = torch.cuda.current_stream().cuda_stream
        rt.wav.copy_(inputs)
        if rt.tgt is not None:
            rt.tgt.copy_(targets)
        # the loss of this step reads the waveform only: no [B, NF, T] spectrum copies, no pass over their (zero) gradients (SEFD_RUN_WAVE_ONLY)
        wave_only = RUN_WAVE_ONLY if (not perceptual and not sync and rt.plan.model_name == "DCCRN" and not str(rt.plan.masking_mode).startswith("Direct")) else 0
        if sync:
            rt.plan.run_synced(PHASE_FWD, rt.arenas, stream, exchange.all_reduce_stats)
        elif wave_only:
            rt.plan.run_cb(PHASE_FWD, rt.arenas, stream, -1, None, flags=wave_only)
        else:
            rt.run(PHASE_FWD)
        # sharded batch: SI-SDR's mean of ratios inside the log (tools_for_loss.py:91-94) is taken over all ranks (two floats all-reduced
        # between the loss kernels); the other losses shard exactly
        direct = str(rt.plan.masking_mode).startswith("Direct")
        prev_dp = tfl.set_data_parallel(exchange)
        try:
            if direct:
                # spectral mapping (dccrn_direct_train / crn_direct_train, trainer.py:121-181): the loss compares SPECTRA, over the rows [B * F] of
                # length T (the reductions of tools_for_loss.py run over the last axis); the waveform output carries no loss
                if perceptual:
                    raise NotImplementedError("the reference has no perceptual trainer for the direct-mapping models")
                NFr, Tr = rt.out_real.shape[1], rt.out_real.shape[2]
                rows = lambda t: t.view(B * NFr, Tr)
                if rt.plan.model_name == "DCCRN":             # loss = (loss(real) + loss(imag)) / 2 against the target's spectra
                    tgt_r, tgt_i = self._stft_ref(targets)
                    half = torch.full((1,), 0.5, dtype=torch.float32, device=inputs.device)
                    ws_r, loss_r = tfl.loss_forward_raw(kind, rows(rt.out_real), rows(tgt_r), stream)
                    ws_i, loss_i = tfl.loss_forward_raw(kind, rows(rt.out_imag), rows(tgt_i), stream)
                    tfl.loss_backward_raw(kind, rows(rt.out_real), rows(tgt_r), ws_r, half, rows(rt.g_real), stream)
                    tfl.loss_backward_raw(kind, rows(rt.out_imag), rows(tgt_i), ws_i, half, rows(rt.g_imag), stream)
                    loss = (loss_r + loss_i) / 2
                else:                                         # CRN: mapped magnitudes (first output) against the target magnitudes (second output)
                    est_m, tgt_m = rows(rt.out_real), rows(rt.out_imag)
                    ws, loss = tfl.loss_forward_raw(kind, est_m, tgt_m, stream)
                    tfl.loss_backward_raw(kind, est_m, tgt_m, ws, None, rows(rt.g_real), stream)
                    rt.g_imag.zero_()
                rt.g_wav.zero_()
            else:
                ws, loss = tfl.loss_forward_raw(kind, rt.out_wav, targets, stream)
        finally:
            tfl.set_data_parallel(prev_dp)
        if not wave_only and not direct:
            rt.g_real.zero_()
            rt.g_imag.zero_()
        if direct:
            pass
        elif perceptual:
            half = torch.full((1,), 0.5, dtype=torch.float32, device=inputs.device)
            tfl.loss_backward_raw(kind, rt.out_wav, targets, ws, half, rt.g_wav, stream)
            with torch.enable_grad():                    # the loss kernels' own autograd wrappers on leaf copies of the outputs
                if perceptual in ("PMSQE", "STOI", "ESTOI"):     # waveform-domain terms
                    est = rt.out_wav.detach().requires_grad_()
                    if perceptual == "PMSQE":
                        perc = tfl.get_array_pmsqe_loss(targets, est)
                    else:
                        perc = tfl.stoi_loss(targets, est, cfg.fs, extended=perceptual == "ESTOI")
                    (perc * 0.5).backward()
                    rt.g_wav.add_(est.grad)
                else:
                    clean_real, clean_imag = self._stft_ref(targets)
                    er, ei = rt.out_real.detach().requires_grad_(), rt.out_imag.detach().requires_grad_()
                    perc = tfl.lms_from_spectra(clean_real, clean_imag, er, ei)
                    (perc * 0.5).backward()
                    rt.g_real.copy_(er.grad)
                    rt.g_imag.copy_(ei.grad)
            self._last_loss_parts = (loss, perc.detach())       # (main, perceptual): what model_perceptual_train logs
            loss = (loss + perc.detach()) / 2
        else:
            tfl.loss_backward_raw(kind, rt.out_wav, targets, ws, None, rt.g_wav, stream)
        bucket = rt.plan.grad_bucket() if self._grad_buckets == 2 else None
        if sync:
            rt.plan.run_synced(PHASE_BWD, rt.arenas, stream, exchange.all_reduce_stats)
        elif bucket is not None:
            op, lo = bucket                                  # decoder + LSTM gradients are final at op `op`: their all-reduce starts
            rt.plan.run_cb(PHASE_BWD, rt.arenas, stream, op, lambda: exchange.begin(self._flat_grad[lo:]), flags=wave_only)   # under the encoder backward
        elif wave_only:
            rt.plan.run_cb(PHASE_BWD, rt.arenas, stream, -1, None, flags=wave_only)
        else:
            rt.run(PHASE_BWD)
        _finish_step(self, rt.plan, optimizer, exchange, stream, self._flat_grad[0:1], None if bucket is None else [self._flat_grad[:bucket[1]]])
        return loss


def _finish_step(model, plan, optimizer, exchange, stream, guard, rest):
    """What a train_step does after the backward phase: all-reduce, Adam, guard.  `guard`: the one-element slice of the flat gradient, in the LAST bucket,
    that tells every rank of a faulty one.  `rest`: the slices still to be all-reduced after the bucket that was started under the backward (None: no
    bucket was started; the whole gradient goes in one all-reduce)."""
    active = exchange is not None and exchange.active
    if active:                                               # DDP: sum gradients over ranks (RCCL), average inside Adam
        # a rank whose plan gave up poisons an element of the LAST bucket: every rank's Adam then skips this step (optim.step_flat)
        optimizer.nan_guard = model._dp_guard = guard
        plan.status_poison(guard, stream)
        if rest is not None:
            for g in rest:
                exchange.begin(g)
            exchange.finish(model._flat_grad)
        else:
            exchange.all_reduce(model._flat_grad)
        optimizer.grad_scale = exchange.grad_scale
    optimizer.step_flat()
    if active:
        _dp_guard_tick(model)


DP_GUARD_EVERY = 16          # data parallel: the all-reduced guard element is looked at on the host every this many steps (one 4-byte read behind a sync)


def _check_dp_guard(model):
    """Data parallel: raises on EVERY rank (the guard element went through the sum all-reduce, so all ranks see the same value at the same step) when
    a rank's plan gave up or the gradient itself diverged at that element; replicas skipped those updates (sefd_adam_step_guarded_dp)."""
    guard = getattr(model, "_dp_guard", None)
    if guard is None or bool(torch.isfinite(guard).all()):
        return
    plan = getattr(model, "_status_plan", None)
    mine = plan is not None and plan.status() != 0
    raise RuntimeError(("this rank's plan gave up" + plan._RC5) if mine else
                       "another rank's plan gave up, or the gradient diverged (non-finite guard element of the all-reduced gradient); every replica skipped "
                       "the update of that step - no rank is left waiting in a collective")


def _dp_guard_tick(model):
    model._dp_steps = getattr(model, "_dp_steps", 0) + 1
    if model._dp_steps % DP_GUARD_EVERY == 0:
        _check_dp_guard(model)


# ------------------------------------------------------------------------------------------ the layers of tools_for_model.py:126-607
def _xy_apply(rt, owner, x, out_shape, y=None, seed=False):
    """The boundary of a ConvLayer / ComplexBatchNorm / ComplexLSTM / SequenceModel plan: io.x -> io.y (or the view `y`), io.grad_y -> io.grad_x and the
    flat gradient arena."""
    shape = tuple(x.shape)
    return _plan_apply(rt, owner, (x,), [rt.io("x", shape)], [rt.io("y", out_shape) if y is None else y], [rt.io("grad_y", out_shape)],
                       [rt.io("grad_x", shape)], seed=seed)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class _ConvLayer(_SefdModule):
    """What the four conv layers share: the accepted domain (refusals at construction), the plan of a (B, F, T) and `forward`.  As children of
    DCCRN / CRN they are parameter holders: the parent owns the flat arenas and plans the whole conv stack itself."""

    _KIND = None          # plan.CONV_KINDS name
    _COMPLEX = False

    def _setup(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, complex_axis, output_padding):
        name = self._KIND
        k, s, p, op = _pair(kernel_size), _pair(stride), _pair(padding), _pair(output_padding)
        if _pair(dilation) != (1, 1):
            raise NotImplementedError(f"sefd {name}: dilation {dilation} is not built (1 only)")
        if groups != 1:
            raise NotImplementedError(f"sefd {name}: groups {groups} is not built (1 only)")
        if complex_axis != 1:
            raise NotImplementedError(f"sefd {name}: complex_axis {complex_axis} is not built (the channel axis, 1, only)")
        if s[1] != 1:
            raise NotImplementedError(f"sefd {name}: a time stride of {s[1]} is not built (1 only)")
        if not 1 <= s[0] <= 2:
            raise NotImplementedError(f"sefd {name}: a frequency stride of {s[0]} is not built (1 .. 2)")
        if not 1 <= k[0] <= 7:
            raise NotImplementedError(f"sefd {name}: a kernel of {k[0]} bins is not built (1 .. 7)")
        if not 1 <= k[1] <= 4:
            raise NotImplementedError(f"sefd {name}: a kernel of {k[1]} frames is not built (1 .. 4: a launch descriptor holds 8 runs over two sources)")
        if not (0 <= p[0] < k[0] and 0 <= p[1] < k[1]):
            raise NotImplementedError(f"sefd {name}: padding {tuple(p)} must stay below the kernel extent {tuple(k)}")
        if not (0 <= op[0] < s[0] and 0 <= op[1] < s[1]):
            raise NotImplementedError(f"sefd {name}: output padding {tuple(op)} must stay below the stride {tuple(s)}")
        if self._COMPLEX and (in_channels % 2 or out_channels % 2):
            raise NotImplementedError(f"sefd {name}: odd channel counts ({in_channels} -> {out_channels}) have no real / imaginary halves")
        self._geo = dict(kind=name, in_channels=int(in_channels), out_channels=int(out_channels), kernel_size=k, stride_f=int(s[0]), padding=p,
                         output_padding_f=int(op[0]))
        self.act_dtype = cfg.act_dtype

    def _layer_runtime(self, B, F, T, device):
        if not self._flat_ok(device):
            self._flatten(device)
        return cached(self._runtimes, ("conv", B, F, T, self.act_dtype, str(device)), lambda: Runtime.bound(
            Plan(B, T, act_dtype=self.act_dtype, training=True, model="ConvLayer",
                 conv=dict(self._geo, causal=bool(getattr(self, "causal", True)), F=F)), self, device))

    def forward(self, inputs):
        name, g = self._KIND, self._geo
        if isinstance(inputs, (tuple, list)) and name == "ComplexConvTranspose2d":          # the reference's (real, imag) form, tools_for_model.py:315-317
            inputs = torch.cat([inputs[0], inputs[1]], 1)
        _check_frontend_input(name, inputs)
        if inputs.dim() != 4 or inputs.shape[1] != g["in_channels"]:
            raise ValueError(f"{name} takes [B, {g['in_channels']}, F, T], got {tuple(inputs.shape)}")
        B, _, F, T = inputs.shape
        rt = self._layer_runtime(B, F, T, inputs.device)
        k, p = g["kernel_size"], g["padding"]
        if "Transpose" in name:
            Fo = (F - 1) * g["stride_f"] - 2 * p[0] + k[0] + g["output_padding_f"]
        else:
            Fo = (F + 2 * p[0] - k[0]) // g["stride_f"] + 1
        return _xy_apply(rt, self, inputs.contiguous(), (B, g["out_channels"], Fo, rt.plan.T))


def _init_conv(*convs):
    for c in convs:
        nn.init.normal_(c.weight.data, std=0.05)
        nn.init.constant_(c.bias, 0.)


class ComplexConv2d(_ConvLayer):
    """tools_for_model.py:199-269, same constructor, attributes, parameters (`real_conv`, `imag_conv`) and init; forward [B, C, F, T] ->
    [B, C_out, F_out, T_out] (real half, then imaginary half of the channels), differentiable in the input and the parameters (ConvLayer plan,
    csrc/plan_layers.cpp).  causal: the time padding goes to the left only.  float32 cuda tensors."""
    _KIND, _COMPLEX = "ComplexConv2d", True

    def __init__(self, in_channels, out_channels, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), dilation=1, groups=1, causal=True,
                 complex_axis=1):
        super().__init__()
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, complex_axis, (0, 0))
        self.in_channels, self.out_channels = in_channels // 2, out_channels // 2
        self.kernel_size, self.stride, self.padding, self.causal = kernel_size, stride, padding, causal
        self.groups, self.dilation, self.complex_axis = groups, dilation, complex_axis
        self.real_conv = nn.Conv2d(self.in_channels, self.out_channels, kernel_size, stride, padding=[padding[0], 0], dilation=dilation, groups=groups)
        self.imag_conv = nn.Conv2d(self.in_channels, self.out_channels, kernel_size, stride, padding=[padding[0], 0], dilation=dilation, groups=groups)
        _init_conv(self.real_conv, self.imag_conv)
        self._init_runtime_state()


class ComplexConvTranspose2d(_ConvLayer):
    """tools_for_model.py:272-338; `forward` also takes the reference's (real, imag) tuple or list."""
    _KIND, _COMPLEX = "ComplexConvTranspose2d", True

    def __init__(self, in_channels, out_channels, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), output_padding=(0, 0), causal=False,
                 complex_axis=1, groups=1):
        super().__init__()
        self._setup(in_channels, out_channels, kernel_size, stride, padding, 1, groups, complex_axis, output_padding)
        self.in_channels, self.out_channels = in_channels // 2, out_channels // 2
        self.kernel_size, self.stride, self.padding, self.output_padding, self.groups = kernel_size, stride, padding, output_padding, groups
        self.real_conv = nn.ConvTranspose2d(self.in_channels, self.out_channels, kernel_size, stride, padding=padding, output_padding=output_padding,
                                            groups=groups)
        self.imag_conv = nn.ConvTranspose2d(self.in_channels, self.out_channels, kernel_size, stride, padding=padding, output_padding=output_padding,
                                            groups=groups)
        self.complex_axis = complex_axis
        _init_conv(self.real_conv, self.imag_conv)
        self._init_runtime_state()


class RealConv2d(_ConvLayer):
    """tools_for_model.py:341-388."""
    _KIND = "RealConv2d"

    def __init__(self, in_channels, out_channels, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), dilation=1, groups=1, causal=True,
                 complex_axis=1):
        super().__init__()
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, complex_axis, (0, 0))
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.causal = kernel_size, stride, padding, causal
        self.groups, self.dilation = groups, dilation
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding=[padding[0], 0], dilation=dilation, groups=groups)
        _init_conv(self.conv)
        self._init_runtime_state()


class RealConvTranspose2d(_ConvLayer):
    """tools_for_model.py:391-425."""
    _KIND = "RealConvTranspose2d"

    def __init__(self, in_channels, out_channels, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), output_padding=(0, 0), groups=1):
        super().__init__()
        self._setup(in_channels, out_channels, kernel_size, stride, padding, 1, groups, 1, output_padding)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.output_padding, self.groups = kernel_size, stride, padding, output_padding, groups
        self.conv = nn.ConvTranspose2d(in_channels, out_channels, kernel_size, stride, padding=padding, output_padding=output_padding, groups=groups)
        _init_conv(self.conv)
        self._init_runtime_state()


class ComplexBatchNorm(_SefdModule):
    """tools_for_model.py:430-607, same constructor, parameters (Wrr, Wri, Wii, Br, Bi over num_features // 2 complex channels), buffers (RMr, RMi,
    RVrr, RVri, RVii, num_batches_tracked), `reset_parameters` (Wri ~ U(-0.9, 0.9)) and forward over any [B, C, *rest]: training mode normalises with
    the batch statistics and moves the running ones by `momentum`; eval mode uses the running statistics and leaves the buffers alone.  Differentiable
    in the input and the parameters (ComplexBatchNorm plan, csrc/plan_layers.cpp; kernels csrc/cbn.hip).  Inside DCCRN(use_cbn=True) a holder."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, complex_axis=1):
        super().__init__()
        if num_features % 8:
            raise NotImplementedError(f"sefd ComplexBatchNorm: num_features {num_features} is not a multiple of 8 (the kernels move 4 complex channels per lane)")
        if not affine:
            raise NotImplementedError("sefd ComplexBatchNorm: affine=False is not built")
        if not track_running_stats:
            raise NotImplementedError("sefd ComplexBatchNorm: track_running_stats=False is not built")
        if momentum is None:
            raise NotImplementedError("sefd ComplexBatchNorm: momentum=None (a cumulative average) is not built")
        if complex_axis != 1:
            raise NotImplementedError(f"sefd ComplexBatchNorm: complex_axis {complex_axis} is not built (the channel axis, 1, only)")
        self.num_features, self.eps, self.momentum = num_features // 2, eps, momentum
        self.affine, self.track_running_stats, self.complex_axis = affine, track_running_stats, complex_axis
        h = self.num_features
        for name in ("Wrr", "Wri", "Wii", "Br", "Bi"):
            setattr(self, name, nn.Parameter(torch.empty(h)))
        self.register_buffer("RMr", torch.zeros(h))
        self.register_buffer("RMi", torch.zeros(h))
        self.register_buffer("RVrr", torch.ones(h))
        self.register_buffer("RVri", torch.zeros(h))
        self.register_buffer("RVii", torch.ones(h))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self.reset_parameters()
        self.act_dtype = cfg.act_dtype
        self._init_runtime_state()

    def reset_running_stats(self):
        with torch.no_grad():
            self.RMr.zero_()
            self.RMi.zero_()
            self.RVrr.fill_(1)
            self.RVri.zero_()
            self.RVii.fill_(1)
            self.num_batches_tracked.zero_()

    def reset_parameters(self):
        self.reset_running_stats()
        with torch.no_grad():
            self.Br.zero_()
            self.Bi.zero_()
            self.Wrr.fill_(1)
            self.Wri.uniform_(-.9, +.9)
            self.Wii.fill_(1)

    def extra_repr(self):
        return (f"{self.num_features}, eps={self.eps}, momentum={self.momentum}, affine={self.affine}, "
                f"track_running_stats={self.track_running_stats}")

    def _cbn_runtime(self, B, S, device):
        if not self._flat_ok(device):
            self._flatten(device)
        key = ("cbn", B, S, bool(self.training), float(self.eps), float(self.momentum), self.act_dtype, str(device))
        return cached(self._runtimes, key, lambda: Runtime.bound(
            Plan(B, S, act_dtype=self.act_dtype, training=bool(self.training), model="ComplexBatchNorm",
                 cbn=dict(num_features=2 * self.num_features, eps=self.eps, momentum=self.momentum)), self, device))

    def forward(self, inputs):
        _check_frontend_input("ComplexBatchNorm", inputs)
        C2 = 2 * self.num_features
        if inputs.dim() < 3 or inputs.shape[1] != C2:
            raise ValueError(f"ComplexBatchNorm takes [B, {C2}, *rest] with at least one trailing dimension, got {tuple(inputs.shape)}")
        B, S = inputs.shape[0], int(inputs[0, 0].numel())
        rt = self._cbn_runtime(B, S, inputs.device)
        if self.training:
            self._flat_nbt += 1
        y = _xy_apply(rt, self, inputs.contiguous().view(B, C2, S), (B, C2, S))
        return y.view(inputs.shape)


class NavieComplexLSTM(_SefdModule):
    """tools_for_model.py:141-181, same constructor (`batch_first` is accepted and ignored, as there), parameters (`real_lstm`, `imag_lstm`: one-layer
    nn.LSTM holders, bidirectional when asked; `r_trans`, `i_trans` when `projection_dim` is given) and forward: [real, imag], each [T, B, input_size // 2],
    -> [real_out, imag_out], each [T, B, projection_dim // 2] (without a projection hidden_size // 2, twice that when bidirectional: forward | reverse).
    Each of the four LSTM calls starts from zero state; real_out = real_lstm(real) - imag_lstm(imag), imag_out = real_lstm(imag) + imag_lstm(real).
    Differentiable in both inputs and every parameter (ComplexLSTM plan, csrc/plan_clstm.cpp); train and eval mode compute the same arithmetic.
    As a child of DCCRN it is a parameter holder: the model owns the flat arenas and plans its recurrent block itself.  float32 cuda tensors."""

    def __init__(self, input_size, hidden_size, projection_dim=None, bidirectional=False, batch_first=False):
        super().__init__()
        self.input_dim, self.rnn_units = input_size // 2, hidden_size // 2
        self.bidirectional = bool(bidirectional)
        self.real_lstm = nn.LSTM(self.input_dim, self.rnn_units, num_layers=1, bidirectional=self.bidirectional, batch_first=False)
        self.imag_lstm = nn.LSTM(self.input_dim, self.rnn_units, num_layers=1, bidirectional=self.bidirectional, batch_first=False)
        ndir = 2 if self.bidirectional else 1
        if projection_dim is not None:
            self.projection_dim = projection_dim // 2
            self.r_trans = nn.Linear(self.rnn_units * ndir, self.projection_dim)
            self.i_trans = nn.Linear(self.rnn_units * ndir, self.projection_dim)
        else:
            self.projection_dim = None
        self._sizes = dict(input_size=int(input_size), hidden_size=int(hidden_size), projection_dim=None if projection_dim is None else int(projection_dim),
                           bidirectional=self.bidirectional)
        self.act_dtype = cfg.act_dtype
        self._init_runtime_state()                   # (a DCCRN parent re-tags the parameters as its own afterwards)

    def flatten_parameters(self):
        pass                                         # tools_for_model.py:179-181: cuDNN weight compaction; the parameters here are views of one flat tensor already

    def _clstm_runtime(self, B, T, device):
        if not self._flat_ok(device):
            self._flatten(device)
        # one training-capable plan for both modes: the layer has no mode-dependent arithmetic, and inside a larger network the input gradient is
        # needed in eval mode too
        return cached(self._runtimes, ("clstm", B, T, self.act_dtype, str(device)), lambda: Runtime.bound(
            Plan(B, T, act_dtype=self.act_dtype, training=True, model="ComplexLSTM", clstm=self._sizes), self, device))

    def forward(self, inputs):
        if not isinstance(inputs, (list, tuple)) or len(inputs) != 2:
            raise TypeError("sefd NavieComplexLSTM takes [real, imag], a list or tuple of two [T, B, input_size // 2] tensors; the reference's branch for a "
                            f"bare tensor (torch.chunk(inputs, -1), tools_for_model.py:165-166) raises inside torch - got {type(inputs).__name__}")
        real, imag = inputs
        _check_frontend_input("NavieComplexLSTM", real, imag)
        I, H, P = self.input_dim, self.rnn_units, self.projection_dim
        if real.dim() != 3 or real.shape[2] != I or imag.shape != real.shape:
            raise ValueError(f"NavieComplexLSTM takes two [T, B, {I}] tensors, got {tuple(real.shape)} and {tuple(imag.shape)}")
        T, B = real.shape[0], real.shape[1]
        rt = self._clstm_runtime(B, T, real.device)
        # The [T, B, .] <-> batch-major permutes, the pad to roundup(I, 8) columns per part and the split into halves are element-wise torch at the
        # plan's boundary, O(B T (I + H)) values beside the recurrences' O(B T H H) work; autograd carries the gradient through them.
        pad = -I % 8
        if pad:
            real, imag = nn.functional.pad(real, (0, pad)), nn.functional.pad(imag, (0, pad))
        x = torch.cat([real, imag], 2).permute(1, 0, 2).contiguous()
        if P is not None:                            # batch-major boundary: x [B, T, 2 IP] (real | imaginary) -> y [B, T, 2 P]
            out = _xy_apply(rt, self, x, (B, T, 2 * P))
            halves = (out[..., :P], out[..., P:])
        else:                                        # the directions' combined outputs `hc`, in the activation dtype
            D = 2 if self.bidirectional else 1
            out = _xy_apply(rt, self, x, (D, B, T, 2 * H), y=rt.view("hc").view(D, B, T, 2 * H))
            # [D, B, T, real | imag] -> forward | reverse on the last axis
            halves = tuple(torch.cat([out[d][..., p * H:(p + 1) * H] for d in range(out.shape[0])], -1) for p in (0, 1))
        return [h.permute(1, 0, 2).contiguous() for h in halves]


class cPReLU(nn.Module):
    """tools_for_model.py:126-138: one PReLU for the real half of the channels and one for the imaginary half (element-wise torch)."""

    def __init__(self, complex_axis=1):
        super().__init__()
        self.r_prelu = nn.PReLU()
        self.i_prelu = nn.PReLU()
        self.complex_axis = complex_axis

    def forward(self, inputs):
        real, imag = torch.chunk(inputs, 2, self.complex_axis)
        return torch.cat([self.r_prelu(real), self.i_prelu(imag)], self.complex_axis)


def complex_cat(inputs, axis):
    """tools_for_model.py:184-193: concatenates the real halves, then the imaginary halves, of `inputs` along `axis`."""
    halves = [torch.chunk(t, 2, axis) for t in inputs]
    return torch.cat([h[0] for h in halves] + [h[1] for h in halves], axis)


# ------------------------------------------------------------------------------------------ the models
class DCCRN(_SefdModule):
    """Same constructor as the reference (models.py:17-28)."""

    def __init__(self, rnn_layers=cfg.rnn_layers, rnn_units=cfg.rnn_units, win_len=cfg.win_len, win_inc=cfg.win_inc,
                 fft_len=cfg.fft_len, win_type=cfg.window, masking_mode=cfg.masking_mode, use_cbn=False, kernel_size=5):
        super().__init__()
        self.use_cbn = bool(use_cbn)
        norm = ComplexBatchNorm if use_cbn else nn.BatchNorm2d         # models.py:76, 120
        self.win_len, self.win_inc, self.fft_len, self.win_type = win_len, win_inc, fft_len, win_type
        self.rnn_units = rnn_units
        self.input_dim = self.output_dim = win_len
        self.hidden_layers = rnn_layers
        self.kernel_size = kernel_size
        self.kernel_num = [2] + list(cfg.dccrn_kernel_num)
        self.masking_mode = masking_mode
        self.fix = True
        self.act_dtype = cfg.act_dtype
        self._lstm_kind = cfg.lstm
        self._skip = bool(cfg.skip_type)
        self.stft = ConvSTFT(win_len, win_inc, fft_len, win_type, 'complex')
        self.istft = ConviSTFT(win_len, win_inc, fft_len, win_type, 'complex')
        self.encoder = nn.ModuleList()
        self.decoder = nn.ModuleList()
        kn = self.kernel_num
        for idx in range(len(kn) - 1):
            self.encoder.append(nn.Sequential(
                ComplexConv2d(kn[idx], kn[idx + 1], kernel_size=(kernel_size, 2), stride=(2, 1), padding=(2, 1)),
                norm(kn[idx + 1]), nn.PReLU()))
        hidden_dim = fft_len // (2 ** len(kn))
        if cfg.lstm == 'complex':
            rnns = []
            for idx in range(rnn_layers):
                rnns.append(NavieComplexLSTM(
                    input_size=hidden_dim * kn[-1] if idx == 0 else rnn_units, hidden_size=rnn_units,
                    projection_dim=hidden_dim * kn[-1] if idx == rnn_layers - 1 else None))
            self.enhance = nn.Sequential(*rnns)  # registered here: the reference assigns it before the decoder is filled
        else:                                    # models.py:96-105: two real layers over all features + `tranform` (sic)
            self.enhance = nn.LSTM(input_size=hidden_dim * kn[-1], hidden_size=rnn_units, num_layers=2, dropout=0.0,
                                   bidirectional=False, batch_first=False)
            self.tranform = nn.Linear(rnn_units, hidden_dim * kn[-1])
        mult = 2 if cfg.skip_type else 1
        for idx in range(len(kn) - 1, 0, -1):
            mods = [ComplexConvTranspose2d(kn[idx] * mult, kn[idx - 1], kernel_size=(kernel_size, 2), stride=(2, 1),
                                           padding=(2, 0), output_padding=(1, 0))]
            if idx != 1:
                mods += [norm(kn[idx - 1]), nn.PReLU()]
            self.decoder.append(nn.Sequential(*mods))
        # state_dict order of the reference: stft, istft, encoder, decoder, enhance
        enh = self._modules.pop('enhance')
        self._modules['enhance'] = enh
        if 'tranform' in self._modules:
            self._modules['tranform'] = self._modules.pop('tranform')
        self._init_runtime_state()

    def _make_plan(self, B, L, training):
        return Plan(B, L, kernel_num=tuple(self.kernel_num[1:]), rnn_layers=self.hidden_layers, rnn_units=self.rnn_units,
                    win_len=self.win_len, win_inc=self.win_inc, fft_len=self.fft_len, masking_mode=self.masking_mode,
                    lstm=self._lstm_kind, skip_type=self._skip, act_dtype=self.act_dtype, training=training, model="DCCRN",
                    bn_world=getattr(self, "_bn_world", 1), grad_buckets=getattr(self, "_grad_buckets", 1), use_cbn=self.use_cbn, win_type=self.win_type,
                    cbn_sync=getattr(self, "_bn_world", 1) > 1)

    # ---- reference surface ----------------------------------------------------------------------------------
    def forward(self, inputs, targets=0):
        if not inputs.is_cuda:
            raise RuntimeError("sefd DCCRN runs on the MI355X only (inputs must be a cuda tensor); there is no CPU fallback")
        inputs = inputs.float().contiguous()
        B, L = inputs.shape
        rt = self._runtime(B, L, inputs.device)
        if self.training:
            self._flat_nbt += 1
        out_real, out_imag, out_wav = self._forward_plan(rt, inputs)
        if self.masking_mode == 'Direct(None make)':            # spectral mapping (models.py:232-250): spectra of the target too
            target_real, target_imag = self._stft_ref(targets)
            return out_real, target_real, out_imag, target_imag, out_wav
        return out_real, out_imag, out_wav

    def loss(self, estimated, target, real_spec=0, img_spec=0, perceptual=False):
        """models.py:303-323."""
        if perceptual:
            if cfg.perceptual == 'LMS':
                clean_real, clean_imag = self._stft_ref(target)          # self.stft(target), models.py:306-308
                return tfl.lms_from_spectra(clean_real, clean_imag, real_spec, img_spec)
            if cfg.perceptual == 'PMSQE':
                return tfl.get_array_pmsqe_loss(target, estimated)       # models.py:313-314 (third-party arithmetic: parity unpinned)
            if cfg.perceptual in ('STOI', 'ESTOI'):                      # not in the reference: 1 - STOI of the GPU scorer
                return tfl.stoi_loss(target, estimated, cfg.fs, extended=cfg.perceptual == 'ESTOI')
            raise ValueError(f"unknown cfg.perceptual {cfg.perceptual!r}")
        return self._main_loss(estimated, target)

    def _stft_ref(self, wav):
        """ConvSTFT 'complex' of a waveform batch in the reference layout: ([B,257,T] real, [B,257,T] imag), no grad."""
        wav = wav.detach().float().contiguous()
        B, L = wav.shape
        # the reference forms target / clean spectra with self.stft, i.e. the MODEL's window (models.py:237, 306-308): round 5 built this plan
        # with the default Hann window whatever win_type was - silently wrong losses for 'hamming' / None (goldens dccrn_hamming_direct_mse, _lms)
        fe = cached(self._runtimes, ("stft", B, L, str(wav.device), str(self.win_type)), lambda: Runtime.owned(
            Plan(B, L, win_len=self.win_len, win_inc=self.win_inc, fft_len=self.fft_len, model="STFT", win_type=self.win_type), wav.device))
        fe.io("wav", (B, L)).copy_(wav)
        fe.run(PHASE_FWD)
        NF, T = fe.plan.NF, fe.plan.T
        return fe.io("out_real", (B, NF, T)).clone(), fe.io("out_imag", (B, NF, T)).clone()


class CRN(_SefdModule):
    """Same constructor as the reference (models.py:330-341).  `rnn_layers` is ignored there too (one LSTM layer, Q13)."""

    def __init__(self, rnn_layers=cfg.rnn_layers, rnn_input_size=cfg.rnn_input_size, rnn_units=cfg.rnn_units, win_len=cfg.win_len,
                 win_inc=cfg.win_inc, fft_len=cfg.fft_len, win_type=cfg.window, masking_mode=cfg.masking_mode, kernel_size=5):
        super().__init__()
        self.win_len, self.win_inc, self.fft_len, self.win_type = win_len, win_inc, fft_len, win_type
        self.rnn_input_size = rnn_input_size
        self.rnn_units = rnn_units // 2
        self.input_dim = self.output_dim = win_len
        self.hidden_layers = rnn_layers
        self.kernel_size = kernel_size
        self.kernel_num = [2] + list(cfg.dccrn_kernel_num)
        self.masking_mode = masking_mode
        self.act_dtype = cfg.act_dtype
        self._skip = bool(cfg.skip_type)
        kn = self.kernel_num
        self.stft = ConvSTFT(win_len, win_inc, fft_len, win_type, 'real')
        self.istft = ConviSTFT(win_len, win_inc, fft_len, win_type, 'complex')
        self.encoder = nn.ModuleList()
        self.decoder = nn.ModuleList()
        for idx in range(len(kn) - 1):
            self.encoder.append(nn.Sequential(
                RealConv2d(kn[idx] // 2, kn[idx + 1] // 2, kernel_size=(kernel_size, 2), stride=(2, 1), padding=(2, 1)),
                nn.BatchNorm2d(kn[idx + 1] // 2), nn.PReLU()))
        hidden_dim = fft_len // (2 ** len(kn))
        if hidden_dim * (kn[-1] // 2) != rnn_input_size:
            raise ValueError("rnn_input_size must equal hidden_dim * kernel_num[-1] // 2 (SURVEY Q13)")
        self.enhance = nn.LSTM(input_size=rnn_input_size, hidden_size=self.rnn_units, dropout=0.0, bidirectional=False, batch_first=False)
        self.tranform = nn.Linear(self.rnn_units, rnn_input_size)
        if not cfg.skip_type:
            # the reference's own forward fails there: its full-width decoder (models.py:432-462) expects kernel_num[idx] input channels but is fed
            # kernel_num[idx] // 2 ("expected input[1, 128, 4, 43] to have 256 channels", checked in the build container) - nothing to mirror
            raise NotImplementedError("CRN with cfg.skip_type = False: the reference's own forward raises a channel mismatch (models.py:432-462, 490-493)")
        for idx in range(len(kn) - 1, 0, -1):
            mods = [RealConvTranspose2d(kn[idx], kn[idx - 1] // 2, kernel_size=(kernel_size, 2), stride=(2, 1), padding=(2, 0),
                                        output_padding=(1, 0))]
            if idx != 1:
                mods += [nn.BatchNorm2d(kn[idx - 1] // 2), nn.PReLU()]
            self.decoder.append(nn.Sequential(*mods))
        # reference registration order: stft, istft, encoder, decoder, enhance, tranform
        for name in ("enhance", "tranform"):
            self._modules[name] = self._modules.pop(name)
        self._init_runtime_state()

    def _make_plan(self, B, L, training):
        # models.py:506-532: 'Direct(None make)' = spectral mapping; any other cfg.masking_mode = tanh magnitude mask
        mode = self.masking_mode if self.masking_mode == 'Direct(None make)' else "E"
        return Plan(B, L, kernel_num=tuple(self.kernel_num[1:]), rnn_layers=1, rnn_units=2 * self.rnn_units, win_len=self.win_len,
                    win_inc=self.win_inc, fft_len=self.fft_len, masking_mode=mode, lstm="real", skip_type=self._skip,
                    act_dtype=self.act_dtype, training=training, model="CRN", bn_world=getattr(self, "_bn_world", 1), win_type=self.win_type)

    def forward(self, inputs, targets=0):
        """models.py:467-532: returns (est_mags, target_mags, out_wav).  est_mags (the network's magnitude output: mask x noisy
        magnitude, or the mapped magnitude in 'Direct(None make)' mode) and out_wav carry gradient; target_mags does not."""
        if not torch.is_tensor(targets):
            raise AttributeError("CRN.forward needs targets (the reference calls self.stft(targets) unconditionally, models.py:505)")
        if not inputs.is_cuda:
            raise RuntimeError("sefd CRN runs on the MI355X only (inputs must be a cuda tensor); there is no CPU fallback")
        inputs = inputs.float().contiguous()
        B, L = inputs.shape
        rt = self._runtime(B, L, inputs.device)
        if self.training:
            self._flat_nbt += 1
        est_mags, target_mags, out_wav = self._forward_plan(rt, inputs, targets.float().contiguous())
        return est_mags, target_mags.detach(), out_wav

    def loss(self, estimated, target, out_mags=0, target_mags=0, perceptual=False):
        if perceptual:
            raise NotImplementedError("CRN + perceptual loss is unreachable in the reference (SURVEY Q10)")
        return self._main_loss(estimated, target)


# ------------------------------------------------------------------------------------------ FullSubNet (models.py:568-682)
class SequenceModel(_SefdModule):
    """Same constructor and state_dict as the reference (tools_for_model.py:726-795): nn.LSTM or nn.GRU of any depth, optionally bidirectional
    (dropout=0.8 between the layers), + Linear (+ activation).  As a child of FullSubNet it is a parameter holder: FullSubNet owns the flat arenas
    and plans both of its SequenceModels itself.  On its own, `forward` runs the SequenceModel plan (csrc/plan_seq.cpp)."""

    _ACTS = {None: None, "None": None, "": None, "Tanh": torch.tanh, "ReLU": torch.relu, "ReLU6": nn.functional.relu6}

    def __init__(self, input_size, output_size, hidden_size, num_layers, bidirectional, sequence_model="LSTM", output_activate_function="Tanh"):
        super().__init__()
        if sequence_model not in ("LSTM", "GRU"):
            raise NotImplementedError(f"Not implemented {sequence_model}")
        if output_activate_function not in self._ACTS:
            raise NotImplementedError(f"Not implemented activation function {output_activate_function}")
        rnn = nn.LSTM if sequence_model == "LSTM" else nn.GRU
        self.sequence_model = rnn(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers, batch_first=True,
                                  bidirectional=bool(bidirectional), dropout=0.8)
        self.fc_output_layer = nn.Linear(hidden_size * (2 if bidirectional else 1), output_size)
        self.output_activate_function = output_activate_function
        self._seq = dict(input_size=int(input_size), output_size=int(output_size), hidden_size=int(hidden_size), num_layers=int(num_layers),
                         bidirectional=bool(bidirectional), sequence_model=sequence_model)
        self.dropout_keep = 0.2                      # nn.LSTM(dropout=0.8), as FullSubNet.dropout_keep; eval mode: no dropout
        self.act_dtype = cfg.act_dtype
        self._init_runtime_state()                   # (a FullSubNet parent re-tags the parameters as its own afterwards)

    def _seq_runtime(self, B, T, device):
        if not self._flat_ok(device):
            self._flatten(device)
        keep = self.dropout_keep if self.training else 1.0
        # a training-capable plan in eval mode too (keep = 1): inside a larger network the input gradient is needed in either mode
        return cached(self._runtimes, ("seq", B, T, bool(self.training), keep, self.act_dtype), lambda: Runtime.bound(
            Plan(B, T, act_dtype=self.act_dtype, training=True, model="SequenceModel", seq=dict(self._seq, keep=keep)), self, device))

    def forward(self, x):
        """tools_for_model.py:779-795: x [B, F, T] -> [B, O, T]."""
        assert x.dim() == 3
        if not x.is_cuda:
            raise RuntimeError("sefd SequenceModel runs on the MI355X only (cuda tensors); there is no CPU fallback")
        B, I, T = x.shape
        assert I == self._seq["input_size"], f"{self.__class__.__name__}: expected {self._seq['input_size']} input features, got {I}"
        rt = self._seq_runtime(B, T, x.device)
        # The [B, F, T] <-> time-major permute / pad and the output activation are element-wise torch at the plan's boundary: O(B * (I + O) * T)
        # values beside the recurrences' O(B * T * H * H) work.  Autograd carries the gradient through them.
        xt = x.float().permute(2, 0, 1)
        if I % 8:
            xt = nn.functional.pad(xt, (0, 8 - I % 8))                # IP = roundup(I, 8): zero pad columns
        y = _xy_apply(rt, self, xt.contiguous(), (T, B, self._seq["output_size"]), seed=True)      # time-major: x [T, B, IP] -> pre-activation y [T, B, O]
        act = self._ACTS[self.output_activate_function]
        if act is not None:
            y = act(y)
        return y.permute(1, 2, 0).contiguous()


def _weight_init(m):
    """BaseModel.weight_init (tools_for_model.py:1120-1184), every module type its traversal names: Conv1d / ConvTranspose1d -> normal_ weight;
    Conv2d, Conv3d and their transposes -> xavier_normal_ weight (bias, where there is one: normal_); BatchNorm1d-3d -> weight N(1, 0.02), bias 0;
    Linear -> xavier_normal_ weight, normal_ bias; LSTM / GRU and their cells -> orthogonal_ matrices, normal_ vectors.  `Module.apply` visits
    children first, as the reference's call does: same draws in the same order."""
    if isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
        nn.init.normal_(m.weight.data)
        if m.bias is not None:
            nn.init.normal_(m.bias.data)
    elif isinstance(m, (nn.Conv2d, nn.Conv3d, nn.ConvTranspose2d, nn.ConvTranspose3d)):
        nn.init.xavier_normal_(m.weight.data)
        if m.bias is not None:
            nn.init.normal_(m.bias.data)
    elif isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)):
        nn.init.normal_(m.weight.data, mean=1, std=0.02)
        nn.init.constant_(m.bias.data, 0)
    elif isinstance(m, nn.Linear):
        nn.init.xavier_normal_(m.weight.data)
        nn.init.normal_(m.bias.data)
    elif isinstance(m, (nn.LSTM, nn.LSTMCell, nn.GRU, nn.GRUCell)):
        for param in m.parameters():
            if len(param.shape) >= 2:
                nn.init.orthogonal_(param.data)
            else:
                nn.init.normal_(param.data)


# ------------------------------------------------------------------------------------------ BaseModel (tools_for_model.py:801-1185)
BM_NORMS = ("offline_laplace_norm", "cumulative_laplace_norm", "offline_gaussian_norm", "cumulative_layer_norm",      # 0..3: plan.FSN_NORMS
            "forgetting_norm", "sband_forgetting_norm", "hybrid_norm")                                                # 4..6: [B, F, T], sample length


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _bm_check(name, x, dim):
    assert x.dim() == dim, f"The dim of input is {x.dim()}. It should be {dim} dim."
    if not x.is_cuda:
        raise RuntimeError(f"sefd BaseModel.{name} runs on the MI355X only (cuda tensors); there is no CPU fallback")
    if x.dtype != torch.float32:
        raise TypeError(f"sefd BaseModel.{name} takes float32 tensors, got {x.dtype}")


def _bm_geometry(kind, shape):
    """(rows, F, T) of include/sefd.h for a norm input: the cumulative pair has B * C rows, the offline pair one row of C * F * T values per
    utterance (passed as F = C F T, T = 1), the recurrence norms B rows."""
    if kind in (1, 3):
        B, Cc, F, T = shape
        g = (B * Cc, F, T)
    elif kind in (0, 2):
        B, Cc, F, T = shape
        g = (B, Cc * F * T, 1)
    else:
        g = tuple(shape)
    if max(g) >= 2 ** 31:
        raise ValueError(f"sefd BaseModel norms: a dimension of {tuple(shape)} does not fit 32 bits")
    return g


def bm_ws_floats(kind, rows, F, T):
    """sefd_norm_ws_floats in Python arithmetic (csrc/basemodel.hip norm_args / ws_layout; pinned to the C function by tests/test_basemodel_cpu.py), so that
    the ops' fake implementations trace with symbolic shapes: the statistics, the partial sums and the backward's coefficients, in floats."""
    if kind in (0, 2):
        N = F * T
        ns = min((N + 2047) // 2048, 256)
        seg = ((N + ns - 1) // ns + 3) // 4 * 4
        return 2 * rows * (2 + 2 * ((N + seg - 1) // seg) + 3)
    fs = min((F + 31) // 32, 16)
    fper = (F + fs - 1) // fs
    fs = (F + fper - 1) // fper
    return 2 * rows * T * (2 + fs * (2 if kind == 3 else 1) + 3)


def bm_norm_forward(x, kind, sample_len):
    """(y, ws) of sefd_norm_forward: x float32 cuda contiguous, 4-D (kinds 0..3) or 3-D (kinds 4..6)."""
    L_ = _lib.lib()
    rows, F, T = _bm_geometry(kind, x.shape)
    n = L_.sefd_norm_ws_floats(kind, rows, F, T)
    if n < 0:
        raise RuntimeError(f"sefd {BM_NORMS[kind] if 0 <= kind < 7 else kind}: bad arguments for an input of shape {tuple(x.shape)}")
    ws = torch.empty(n, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    rc = L_.sefd_norm_forward(kind, _vp(x), rows, F, T, int(sample_len), _vp(ws), _vp(y), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError(f"sefd_norm_forward({BM_NORMS[kind]}, shape {tuple(x.shape)}, sample length {sample_len}) failed ({rc})")
    return y, ws


def bm_norm_backward(x, g, ws, kind, sample_len):
    rows, F, T = _bm_geometry(kind, x.shape)
    gx = torch.empty_like(x)
    rc = _lib.lib().sefd_norm_backward(kind, _vp(x), _vp(g), rows, F, T, int(sample_len), _vp(ws), _vp(gx), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError(f"sefd_norm_backward({BM_NORMS[kind]}, shape {tuple(x.shape)}) failed ({rc})")
    return gx


def bm_unfold_forward(x, n):
    B, Cc, F, T = x.shape
    if n >= F:
        raise RuntimeError(f"sefd BaseModel.unfold: num_neighbor {n} must be less than the {F} frequencies (reflect padding)")
    out = torch.empty((B, F, Cc, 2 * n + 1, T), dtype=torch.float32, device=x.device)
    rc = _lib.lib().sefd_unfold_forward(_vp(x), B, Cc, F, T, n, _vp(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError(f"sefd_unfold_forward(shape {tuple(x.shape)}, n {n}) failed ({rc})")
    return out


def bm_unfold_backward(g, shape, n):
    B, Cc, F, T = shape
    gx = torch.empty(tuple(shape), dtype=torch.float32, device=g.device)
    rc = _lib.lib().sefd_unfold_backward(_vp(g), B, Cc, F, T, n, _vp(gx), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError(f"sefd_unfold_backward(shape {tuple(shape)}, n {n}) failed ({rc})")
    return gx


class _BMNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind, sample_len):
        x = x.contiguous()
        y, ws = bm_norm_forward(x, kind, sample_len)
        ctx.kind, ctx.sample_len = kind, sample_len
        ctx.save_for_backward(x, ws)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, ws = ctx.saved_tensors
        return bm_norm_backward(x, g.float().contiguous(), ws, ctx.kind, ctx.sample_len), None, None


class _BMUnfoldFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n):
        ctx.n, ctx.shape = n, tuple(x.shape)
        return bm_unfold_forward(x.contiguous(), n)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return bm_unfold_backward(g.float().contiguous(), ctx.shape, ctx.n), None


def _bm_norm(name, x, dim, sample_len=1):
    _bm_check(name, x, dim)
    return _BMNormFunction.apply(x, BM_NORMS.index(name), int(sample_len))


class BaseModel(nn.Module):
    """The reference's BaseModel (tools_for_model.py:801-1185), the class a FullSubNet variant subclasses: `unfold` and the seven norms are
    static methods on float32 cuda tensors in the reference's layout, each one autograd Function over the streaming kernels of csrc/basemodel.hip
    (sefd_norm_* / sefd_unfold_* of include/sefd.h); it saves the input and the per-frame statistics, there is no double backward.  Inside
    `FullSubNet` the fused plan does this work on its own buffers (csrc/fsn.hip) and does not come through here."""

    def __init__(self):
        super().__init__()

    @staticmethod
    def unfold(input, num_neighbor):
        """[B, C, F, T] -> [B, F, C, 2 num_neighbor + 1, T]: the sub-band units along the reflect-padded frequency axis (:806-837)."""
        _bm_check("unfold", input, 4)
        return _BMUnfoldFunction.apply(input, max(int(num_neighbor), 0))

    @staticmethod
    def _reduce_complexity_separately(sub_band_input, full_band_output, device):
        """tools_for_model.py:840-878: out = cat over i = 0, 1, 2 of cat(sub_band_input, full_band_output; unit axis)[i B/3 : (i+1) B/3, i+1 : F-1 : 3].
        A pure gather: index selects in torch, autograd carries it."""
        both = torch.cat([sub_band_input, full_band_output], dim=-2)          # [B, F, C, K_sb + K_fb, T]
        B, F = both.shape[:2]
        third = B // 3
        thirds = []
        for i in range(3):
            rows = torch.arange(i * third, (i + 1) * third, device=device)
            bins = torch.arange(i + 1, F - 1, 3, device=device)                 # the padded first and last frequencies are never taken
            thirds.append(both.index_select(0, rows).index_select(1, bins))
        return torch.cat(thirds, dim=0)

    @staticmethod
    def sband_forgetting_norm(input, train_sample_length):
        """[B, F, T] (:881-913): forgetting_norm whose frames past the sample length follow the single bin F // 2 - 1."""
        return _bm_norm("sband_forgetting_norm", input, 3, train_sample_length)

    @staticmethod
    def forgetting_norm(input, sample_length_in_training):
        """[B, F, T] (:916-948): x / (mu_t + 1e-10), mu_t the exponentially forgetting mean of the frame means."""
        return _bm_norm("forgetting_norm", input, 3, sample_length_in_training)

    @staticmethod
    def hybrid_norm(input, sample_length_in_training=192):
        """[B, F, T] (:951-994): the forgetting mean for the first sample_length_in_training frames, the cumulative mean afterwards."""
        return _bm_norm("hybrid_norm", input, 3, sample_length_in_training)

    @staticmethod
    def offline_laplace_norm(input):
        """[B, C, F, T] (:997-1011): x / (utterance mean + 1e-5)."""
        return _bm_norm("offline_laplace_norm", input, 4)

    @staticmethod
    def cumulative_laplace_norm(input):
        """[B, C, F, T] (:1014-1044): x / (cumulative mean up to the frame + eps)."""
        return _bm_norm("cumulative_laplace_norm", input, 4)

    @staticmethod
    def offline_gaussian_norm(input):
        """[B, C, F, T] (:1047-1061): (x - utterance mean) / (unbiased utterance std + 1e-5)."""
        return _bm_norm("offline_gaussian_norm", input, 4)

    @staticmethod
    def cumulative_layer_norm(input):
        """[B, C, F, T] (:1064-1104): (x - cumulative mean) / sqrt(cumulative variance + eps)."""
        return _bm_norm("cumulative_layer_norm", input, 4)

    def norm_wrapper(self, norm_type: str):
        if norm_type in BM_NORMS[:4]:
            return getattr(self, norm_type)
        raise NotImplementedError("You must set up a type of Norm. "
                                  "e.g. offline_laplace_norm, cumulative_laplace_norm, forgetting_norm, etc.")

    def weight_init(self, m):
        """Usage: model.apply(model.weight_init) (:1120-1184)."""
        _weight_init(m)


class FullSubNet(_SefdModule, BaseModel):
    """Same constructor as the reference (models.py:569-581); a BaseModel, as there (its unfold and norms run inside the fused plan)."""

    def __init__(self, sb_num_neighbors=cfg.sb_num_neighbors, fb_num_neighbors=cfg.fb_num_neighbors, num_freqs=cfg.num_freqs,
                 look_ahead=cfg.look_ahead, sequence_model=cfg.sequence_model, fb_output_activate_function=cfg.fb_output_activate_function,
                 sb_output_activate_function=cfg.sb_output_activate_function, fb_model_hidden_size=cfg.fb_model_hidden_size,
                 sb_model_hidden_size=cfg.sb_model_hidden_size, weight_init=cfg.weight_init, norm_type=cfg.norm_type):
        super().__init__()
        assert sequence_model in ("GRU", "LSTM"), f"{self.__class__.__name__} only support GRU and LSTM."
        from .plan import FSN_NORMS
        if norm_type not in FSN_NORMS:                # norm_wrapper (tools_for_model.py:1106-1118)
            raise NotImplementedError("You must set up a type of Norm. e.g. offline_laplace_norm, cumulative_laplace_norm, forgetting_norm, etc.")
        self.fb_model = SequenceModel(num_freqs, num_freqs, fb_model_hidden_size, 2, False, sequence_model, fb_output_activate_function)
        self.sb_model = SequenceModel((sb_num_neighbors * 2 + 1) + (fb_num_neighbors * 2 + 1), 2, sb_model_hidden_size, 2, False,
                                      sequence_model, sb_output_activate_function)
        self.sb_num_neighbors, self.fb_num_neighbors, self.look_ahead, self.num_freqs = sb_num_neighbors, fb_num_neighbors, look_ahead, num_freqs
        self._fsn = dict(sb_num_neighbors=sb_num_neighbors, fb_num_neighbors=fb_num_neighbors, look_ahead=look_ahead,
                         fb_hidden=fb_model_hidden_size, sb_hidden=sb_model_hidden_size, fb_act=fb_output_activate_function,
                         sb_act=sb_output_activate_function, sequence_model=sequence_model, norm_type=norm_type)
        if weight_init:                              # models.py:623-624: self.apply(self.weight_init)
            self.apply(_weight_init)
        self.dropout_keep = 0.2                      # nn.LSTM(dropout=0.8); tests set 1.0 to compare with the dropout-free goldens
        self.masking_mode, self.act_dtype = "cIRM", cfg.act_dtype
        self._init_runtime_state()

    def _fsn_runtime(self, B, T, device):
        if not self._flat_ok(device):
            self._flatten(device)
        keep = self.dropout_keep if self.training else 1.0
        nb = getattr(self, "_grad_buckets", 1)
        return cached(self._runtimes, ("fsn", B, T, bool(self.training), keep, self.act_dtype, nb), lambda: Runtime.bound(
            Plan(B, T, fft_len=2 * (self.num_freqs - 1), act_dtype=self.act_dtype, training=True, model="FullSubNet",
                 fsn=dict(self._fsn, keep=keep), grad_buckets=nb), self, device))

    def forward(self, noisy_mag):
        """models.py:626-672: noisy_mag [B, F, T] (or [B, 1, F, T]) -> cRM [B, F, T, 2]."""
        if noisy_mag.dim() == 4:
            assert noisy_mag.shape[1] == 1, f"{self.__class__.__name__} takes the mag feature as inputs."
            noisy_mag = noisy_mag[:, 0]
        if not noisy_mag.is_cuda:
            raise RuntimeError("sefd FullSubNet runs on the MI355X only (cuda tensors); there is no CPU fallback")
        noisy_mag = noisy_mag.detach().float().contiguous()
        B, F, T = noisy_mag.shape
        rt = self._fsn_runtime(B, T, noisy_mag.device)
        return _plan_apply(rt, self, (noisy_mag,), [rt.io("mag", (B, F, T))], [rt.io("crm", (B, F, T, 2))], [rt.io("grad_crm", (B, F, T, 2))], seed=True)

    def loss(self, estimated, target):
        """models.py:674-682: the four losses over the LAST axis (the real / imaginary pair of the [B, F, T, 2] masks)."""
        if cfg.loss == 'MSE':
            return tfl.mse(estimated.reshape(estimated.shape[0], -1), target.reshape(target.shape[0], -1))
        elif cfg.loss == 'SDR':
            return -tfl.sdr(target, estimated)
        elif cfg.loss == 'SI-SNR':
            return -tfl.si_snr(estimated, target)
        elif cfg.loss == 'SI-SDR':
            return -tfl.si_sdr(target, estimated)

    def train_step(self, inputs, targets, optimizer, loss_kind=None, exchange=None):
        """fullsubnet_train body (trainer.py:95-111), fused: stft x2 -> |.|, cIRM -> forward -> MSE -> backward -> Adam."""
        from . import tools_for_model as tools
        from .optim import Adam
        if not isinstance(optimizer, Adam):
            raise TypeError("train_step needs sefd_amd.optim.Adam (flat fused Adam)")
        noisy_complex, clean_complex = tools.stft(inputs), tools.stft(targets)
        noisy_mag, _, cirm = tools._targets(noisy_complex, clean_complex, True, False, True)
        B, F, T = noisy_mag.shape
        # data parallel: two gradient buckets - the full-band model's range is final while the sub-band weight gradients still run (ddp.py)
        self._grad_buckets = 2 if (exchange is not None and exchange.active) else 1
        plan, ar = rt = self._fsn_runtime(B, T, noisy_mag.device)
        plan.tolerate_fault = exchange is not None and exchange.active
        optimizer.bind(self)
        stream = torch.cuda.current_stream().cuda_stream
        plan.io(ar, "mag", (B, F, T)).copy_(noisy_mag)
        _next_dropout_seed(rt)
        plan.run(PHASE_FWD, ar, stream)
        kind = tfl.LOSS_KINDS[loss_kind or cfg.loss]
        prev_dp = tfl.set_data_parallel(exchange)            # SI-SDR: mean of the row ratios over ALL ranks' rows inside the log
        try:
            if kind == 0:
                crm = plan.io(ar, "crm", (B, F * T * 2))
                ws, loss = tfl.loss_forward_raw(0, crm, cirm.view(B, -1), stream)
                tfl.loss_backward_raw(0, crm, cirm.view(B, -1), ws, None, plan.io(ar, "grad_crm", (B, F * T * 2)), stream)
            else:
                # model.loss(cIRM, cRM) (trainer.py:107): in all three the cIRM sits in the kernels' `est` role and the network output in
                # the `tgt` role (sdr(s1 = cRM, s2 = cIRM), si_snr(s1 = cIRM, s2 = cRM), si_sdr(reference = cRM, estimation = cIRM))
                crm = plan.io(ar, "crm", (B * F * T, 2))
                ws, loss = tfl.loss_rows_forward_raw(kind, cirm.view(-1, 2), crm, stream)
                tfl.loss_rows_backward_raw(kind, cirm.view(-1, 2), crm, ws, None, None, plan.io(ar, "grad_crm", (B * F * T, 2)), stream)
        finally:
            tfl.set_data_parallel(prev_dp)                   # an exception in the loss kernels must not leave the exchange set for a later validation loss
        bucket = plan.grad_bucket_range() if self._grad_buckets == 2 else None
        if bucket is not None:
            op, lo, hi = bucket
            plan.run_cb(PHASE_BWD, ar, stream, op, lambda: exchange.begin(self._flat_grad[lo:hi]))
        else:
            plan.run(PHASE_BWD, ar, stream)
        rest = None if bucket is None else [self._flat_grad[a:z] for a, z in ((0, bucket[1]), (bucket[2], self._flat_grad.numel())) if z > a]
        _finish_step(self, plan, optimizer, exchange, stream, self._flat_grad[-1:], rest)      # the guard: in the last bucket, see _finish_step
        return loss
