"""GPU tier: the standalone entry points that close every training step - sefd_loss_*, sefd_loss_rows_*, sefd_adam_step*, sefd_mix_snr - at
the shapes where their launch geometry changes (vector / scalar loads, one workgroup and more, the grid caps and their grid-stride loops) and at
the inputs where fp32 arithmetic is fragile (estimate close to the target).

The reference is always the fp64 restatement of the same operation (oracle.losses.main_loss + autograd, oracle.step.adam_update,
oracle.mixing.generate_noisy_wav), never a kernel.  Bars are those of test_gpu_ops.py / test_gpu_validate.py: value 1e-4 * max(1, |ref|),
gradient rel_err 1e-3, Adam rel_err 1e-6, mixing 1e-6 absolute and, quantized, 1 LSB with < 1e-4 of the samples beyond 0.5 LSB.

Reference-alone condition: every case first evaluates the same oracle formula in torch / numpy fp32 on the CPU and asserts that it lies within a
tenth of the bar against fp64 - the inputs are well conditioned, so a failure can only mean the kernel.

Guards: every buffer a kernel writes lives inside a larger tensor with 64 sentinel elements on each side, checked bit for bit after the call."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import losses as ol
from oracle.mixing import generate_noisy_wav
from oracle.step import adam_update
from oracle.weights import test_signals as make_signals
from util import rel_err

pytestmark = pytest.mark.gpu

KINDS = {"MSE": 0, "SDR": 1, "SI-SNR": 2, "SI-SDR": 3}
VALUE_BAR, GRAD_BAR, ADAM_BAR, MIX_BAR = 1e-4, 1e-3, 1e-6, 1e-6
GUARD = 64
SENTINEL = -725000.0


def _lib():
    from sefd_amd import _lib as m
    return m.lib()


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _tfl(name):
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_loss as tfl
    return {"MSE": lambda e, t: tfl.mse(e, t), "SDR": lambda e, t: -tfl.sdr(t, e), "SI-SNR": lambda e, t: -tfl.si_snr(e, t),
            "SI-SDR": lambda e, t: -tfl.si_sdr(t, e)}[name]


class Guarded:
    """`n` elements for a kernel to write, inside a larger cuda tensor: GUARD sentinels before and after.  The interior (`.t`) starts on 16 bytes
    and holds the sentinel too, so an element the kernel should have written and did not shows up in the comparison."""

    def __init__(self, n, dtype=torch.float32, init=None):
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(init.reshape(-1))
        self.ptr = C.c_void_p(self.t.data_ptr())

    def check(self):
        torch.cuda.synchronize()
        edge = torch.full((GUARD,), SENTINEL, dtype=self.buf.dtype, device="cuda")
        assert torch.equal(self.buf[:GUARD], edge) and torch.equal(self.buf[-GUARD:], edge), "write outside the buffer"

    def untouched(self):
        self.check()
        return bool((self.t == SENTINEL).all())


def _value_err(out, ref, relative=False):
    return abs(out - ref) / (abs(ref) if relative else max(1.0, abs(ref)))


def _loss_ref(name, est, tgt, relative=False, both=False):
    """fp64 oracle value and gradient(s) of main_loss(name, est, tgt) for fp32 inputs, after the reference-alone condition: the same formulas
    in torch fp32 stay within a tenth of the bars.  Returns (value, grad_est, grad_tgt or None, (fp32 value error, fp32 gradient error))."""
    got = {}
    for dt in (torch.float64, torch.float32):
        e, t = est.to(dt).clone().requires_grad_(True), tgt.to(dt).clone().requires_grad_(both)
        v = ol.main_loss(name, e, t)
        v.backward()
        got[dt] = (float(v.detach()), e.grad, t.grad)
    v, ge, gt = got[torch.float64]
    v32, ge32, gt32 = got[torch.float32]
    alone = (_value_err(v32, v, relative), max(rel_err(ge32, ge), rel_err(gt32, gt) if both else 0.0))
    assert alone[0] < 0.1 * VALUE_BAR and alone[1] < 0.1 * GRAD_BAR, ("reference alone", name, tuple(est.shape), alone)
    return v, ge, gt, alone


def _run_long(kind, est_d, tgt_d, scales):
    """sefd_loss_forward, then one sefd_loss_backward per grad scale (None: the NULL pointer, meaning 1); every written buffer guarded."""
    L_ = _lib()
    B, L = est_d.shape
    ws, out = Guarded(L_.sefd_loss_ws_floats(B)), Guarded(1)
    assert L_.sefd_loss_forward(kind, _vp(est_d), _vp(tgt_d), B, L, ws.ptr, out.ptr, None) == 0
    grads = []
    for s in scales:
        g = Guarded(B * L)
        gs = None if s is None else torch.full((1,), s, device="cuda")
        assert L_.sefd_loss_backward(kind, _vp(est_d), _vp(tgt_d), B, L, ws.ptr, _vp(gs), g.ptr, None) == 0
        g.check()
        grads.append(g.t.view(B, L).cpu())
    ws.check()
    out.check()
    return float(out.t[0]), grads


# ------------------------------------------------------------------------------------------ 1. high SNR, long rows
@functools.lru_cache(maxsize=2)
def _snr_case(B, L, snr):
    """Clean test signals as the target, the estimate = target + white noise scaled per row to `snr` dB."""
    tgt = make_signals(B, L)[1]
    n = torch.randn(B, L, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
    t = tgt.double()
    scale = (t.pow(2).sum(1, keepdim=True) / n.pow(2).sum(1, keepdim=True)).sqrt() * 10.0 ** (-snr / 20.0)
    return (t + scale * n).float(), tgt


@pytest.mark.parametrize("B,L,snr,name", [(B, L, snr, name) for B, L in ((3, 4802), (2, 48000)) for snr in (20, 40, 60) for name in KINDS])
def test_long_row_losses_at_high_snr(B, L, snr, name):
    """An estimate 20 / 40 / 60 dB from its target, where training is meant to end up: the error energy has to come from element-wise differences.
    Summed as see - 2 set + stt from three fp32 inner products it cancels: that form measured, on the MI355X, 1.2e-4 on the value and 5.8e-3 on the
    gradient at 40 dB and 2.8e-2 / 1.7 at 60 dB (L = 48000; all of SDR, SI-SNR, SI-SDR, and 1.7e-1 on the MSE value), against 1.6e-7 / 1.7e-4
    with dd = sum (t - e)^2 and det = sum (e - t) t summed beside the inner products.  The kernels keep the expansion only while it loses at most
    6 bits (below about 15 dB), so the 20 dB items take the element-wise sums too (1.6e-7 / 1.4e-6; the expansion gave 1.5e-5 / 3.8e-5).  The MSE
    value goes to zero with the SNR and is held relatively."""
    est, tgt = _snr_case(B, L, snr)
    relative = name == "MSE"
    v, ge, _, alone = _loss_ref(name, est, tgt, relative)
    ed, td = est.cuda(), tgt.cuda()
    val, (g,) = _run_long(KINDS[name], ed, td, (None,))
    em = ed.clone().requires_grad_(True)
    out = _tfl(name)(em, td)
    out.backward()
    ev, eg = _value_err(val, v, relative), rel_err(g, ge)
    evm, egm = _value_err(float(out.detach()), v, relative), rel_err(em.grad.cpu(), ge)
    print(f"high-snr {name} B={B} L={L} {snr} dB: fp32 alone value {alone[0]:.2e} grad {alone[1]:.2e} | kernel value {ev:.2e} grad {eg:.2e} | "
          f"tools_for_loss value {evm:.2e} grad {egm:.2e}")
    assert ev < VALUE_BAR and evm < VALUE_BAR, (val, float(out.detach()), v)
    assert eg < GRAD_BAR and egm < GRAD_BAR, (eg, egm)


# ------------------------------------------------------------------------------------------ 2. shapes, long rows
# L: 17 is the first length the Python dispatch sends to these kernels; L % 4 = 0..3 below and above one workgroup; 16 * 1024 + 4 = one float4 pass
# of all kLossBlk workgroups + 1.  B > 256: the finalize kernel's loop over utterances.  B * L > 4096 * 256: loss_grad_kernel strides.
LONG_SHAPES = ([(2, L) for L in (17, 18, 19, 20, 255, 256, 257, 1023, 4096, 4097, 16 * 1024 + 4, 16 * 1024 + 3)]
               + [(B, L) for B in (1, 257, 300) for L in (64, 67)] + [(5, 262147), (4, 262148)])


@functools.lru_cache(maxsize=2)
def _shape_case(B, L, close=False):
    """The noisy test signal scaled by 0.9 against the clean one (about 0 dB), or - close - the clean one plus a hundredth of the difference
    (about 50 dB): the finalize kernel takes the error energy from the inner products in the first case and from the element-wise sums in the
    second, so every shape meets both."""
    x, y = make_signals(B, L)
    return (y + 0.01 * (x - y), y) if close else (0.9 * x, y)


@pytest.mark.parametrize("B,L,close,name", [(B, L, close, name) for B, L in LONG_SHAPES for close in (False, True) for name in KINDS])
def test_long_row_losses_over_shapes(B, L, close, name):
    est, tgt = _shape_case(B, L, close)
    relative = close and name == "MSE"                 # as in the SNR sweep: a MSE near zero is held relatively
    v, ge, _, _ = _loss_ref(name, est, tgt, relative)
    val, (g1, gh) = _run_long(KINDS[name], est.cuda(), tgt.cuda(), (None, 0.5))
    assert _value_err(val, v, relative) < VALUE_BAR, (val, v)
    assert rel_err(g1, ge) < GRAD_BAR and rel_err(gh, 0.5 * ge) < GRAD_BAR


def test_long_row_losses_refuse_bad_arguments():
    L_ = _lib()
    B, L = 2, 64
    est, tgt = (t.cuda() for t in _shape_case(B, L))
    ws, out, g = Guarded(L_.sefd_loss_ws_floats(B)), Guarded(1), Guarded(B * L)
    for kind, b, l in ((4, B, L), (-1, B, L), (2, 0, L), (2, B, 0)):
        assert L_.sefd_loss_forward(kind, _vp(est), _vp(tgt), b, l, ws.ptr, out.ptr, None) == -1
        assert L_.sefd_loss_backward(kind, _vp(est), _vp(tgt), b, l, ws.ptr, None, g.ptr, None) == -1
    assert ws.untouched() and out.untouched() and g.untouched()


# ------------------------------------------------------------------------------------------ 3. short rows
ROWS_R = (1, 255, 256, 257)                        # around one workgroup
ROWS_R_STRIDE = 4096 * 256 + 257                   # past the 4096-block cap, where every thread strides: with L = 2 and 5 only (a few MB)


@functools.lru_cache(maxsize=2)
def _rows_case(R, L, near=False):
    """Rows with a noise energy bounded away from zero (with `b = a + 0.3 randn` some of a million two-element rows have next to none, and fp32
    alone is then off by 2.7e-2 on the SI-SDR gradient): t = 0.7 randn pushed 0.2 away from zero, n a random vector orthogonal to t and as long,
    est = g t + rho n with g in [0.8, 1.2], rho in [0.1, 0.5] (near: g = 1, rho in [1e-3, 2e-3])."""
    gen = torch.Generator().manual_seed(5 + L)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=gen)
    uni = lambda lo, hi: lo + (hi - lo) * torch.rand(R, 1, dtype=torch.float64, generator=gen)
    t = 0.7 * rnd(R, L)
    t = t + 0.2 * torch.sign(t)
    n = rnd(R, L)
    n = n - (n * t).sum(1, keepdim=True) / (t * t).sum(1, keepdim=True) * t
    nn = n.norm(dim=1, keepdim=True)
    n = n * t.norm(dim=1, keepdim=True) / torch.where(nn > 0, nn, torch.ones_like(nn))        # L = 1: nothing is orthogonal, n = 0
    g, rho = (1.0, uni(1e-3, 2e-3)) if near else (uni(0.8, 1.2), uni(0.1, 0.5))
    return (g * t + rho * n).float(), t.float()


def _run_rows(kind, est_d, tgt_d, scale):
    L_ = _lib()
    R, L = est_d.shape
    ws, out, ge, gt = Guarded(L_.sefd_loss_rows_ws_floats(R)), Guarded(1), Guarded(R * L), Guarded(R * L)
    gs = torch.full((1,), scale, device="cuda")
    assert L_.sefd_loss_rows_forward(kind, _vp(est_d), _vp(tgt_d), R, L, ws.ptr, out.ptr, None) == 0
    assert L_.sefd_loss_rows_backward(kind, _vp(est_d), _vp(tgt_d), R, L, ws.ptr, _vp(gs), ge.ptr, gt.ptr, None) == 0
    for b in (ws, out, ge, gt):
        b.check()
    return float(out.t[0]), ge.t.view(R, L).cpu(), gt.t.view(R, L).cpu()


def _check_rows(name, R, L, near=False):
    est, tgt = _rows_case(R, L, near)
    v, ge, gt, _ = _loss_ref(name, est, tgt, both=True)
    val, de, dt = _run_rows(KINDS[name], est.cuda(), tgt.cuda(), 0.5)
    assert _value_err(val, v) < VALUE_BAR, (val, v)
    assert rel_err(de, 0.5 * ge) < GRAD_BAR and rel_err(dt, 0.5 * gt) < GRAD_BAR


@pytest.mark.parametrize("R,L,name", [(R, L, name) for R in ROWS_R + (ROWS_R_STRIDE,) for L in (1, 2, 3, 5, 16) for name in KINDS
                                      if (L > 1 or name in ("MSE", "SDR"))     # a one-element row has no scale-invariant noise
                                      and (R != ROWS_R_STRIDE or L in (2, 5))])
def test_short_row_losses_over_shapes(R, L, name):
    _check_rows(name, R, L)


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("L", [2, 5])
def test_short_row_losses_near_equal_rows(name, L):
    """The differences are formed element-wise, as the kernels' comment says: an estimate 55 to 60 dB from its target."""
    _check_rows(name, 257, L, near=True)


@pytest.mark.parametrize("name", list(KINDS))
def test_loss_dispatch_boundary(name):
    """tools_for_loss: a last axis of 16 takes the rows kernels (gradient to either slot), 17 the long-row kernels (estimate only)."""
    fn = _tfl(name)
    for L in (16, 17):
        est, tgt = (t.view(3, 5, L) for t in _rows_case(15, L))
        v, ge, gt, _ = _loss_ref(name, est, tgt, both=True)
        for slot in ((0, 1) if L == 16 else (0,)):
            ed, td = est.cuda(), tgt.cuda()
            (ed if slot == 0 else td).requires_grad_(True)
            out = fn(ed, td)
            out.backward()
            assert _value_err(float(out.detach()), v) < VALUE_BAR, (L, slot, float(out.detach()), v)
            assert rel_err((ed if slot == 0 else td).grad.cpu(), ge if slot == 0 else gt) < GRAD_BAR, (L, slot)
    if name != "MSE":                                   # mse() is symmetric and swaps the operand that needs the gradient into the first slot
        with pytest.raises(NotImplementedError):
            fn(est.cuda(), tgt.cuda().requires_grad_(True))


def test_short_row_losses_refuse_long_rows():
    L_ = _lib()
    R, L = 4, 17
    est, tgt = (t.cuda() for t in _rows_case(R, L))
    ws, out, ge, gt = Guarded(L_.sefd_loss_rows_ws_floats(R)), Guarded(1), Guarded(R * L), Guarded(R * L)
    assert L_.sefd_loss_rows_forward(0, _vp(est), _vp(tgt), R, L, ws.ptr, out.ptr, None) == -1
    assert L_.sefd_loss_rows_backward(0, _vp(est), _vp(tgt), R, L, ws.ptr, None, ge.ptr, gt.ptr, None) == -1
    assert ws.untouched() and out.untouched() and ge.untouched() and gt.untouched()


# ------------------------------------------------------------------------------------------ 4. Adam
# the entry point takes its hyper-parameters as C floats: the reference is given the same numbers (0.999f is 1.3e-8 above 0.999, and 1 - beta2
# then differs by 1.3e-5, which is about the argument, not about the kernel)
LR, B1, B2, EPS = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))


@functools.lru_cache(maxsize=2)
def _adam_case(n, first):
    """A 257-element pattern, its largest element first, repeated over n (the period is odd, so it never lines up with the 256-thread workgroups).
    Three fp32 steps round each moment about eight times, which over a million independent elements puts ANY fp32 evaluation at 1.2e-7 to 2e-7 of
    the maximum - above a tenth of the bar.  The pattern (seed 2) keeps fp32 alone at 6.3e-8 for every size, as every size sees the same elements
    and the same maximum; an element that is skipped, written twice or taken from the wrong index still differs."""
    gen = torch.Generator().manual_seed(2)
    r = lambda: torch.randn(257, generator=gen)
    pat = [r(), r() * 1e-2, r() * 5e-3, (r() * 1e-2).pow(2) + 1e-5]
    for t in pat:
        i = int(t.abs().argmax())
        t[[0, i]] = t[[i, 0]]
    p, g, m, v = (t.repeat(n // 257 + 1)[:n].clone() for t in pat)
    return (p, g, torch.zeros(n), torch.zeros(n)) if first == 1 else (p, g, m, v)


ADAM_GRADS = (1.0, 0.5, 2.0)                        # the gradient of the three steps, as multiples of the case's g


def _adam_ref(n, first, scale):
    """Three steps of adam_update in fp64 (the gradient changes size between the steps); reference alone: the same in fp32."""
    got = {}
    for dt in (torch.float64, torch.float32):
        p, g, m, v = (t.to(dt) for t in _adam_case(n, first))
        for k in range(3):
            p, m, v = adam_update(p, ADAM_GRADS[k] * g * scale, m, v, first + k, LR, B1, B2, EPS)
        got[dt] = (p, m, v)
    alone = max(rel_err(a, b) for a, b in zip(got[torch.float32], got[torch.float64]))
    assert alone < 0.1 * ADAM_BAR, ("reference alone", n, first, alone)
    return got[torch.float64]


@pytest.mark.parametrize("n,first,scale", [(n, first, scale) for n in (1, 255, 256, 257, 4096 * 256 + 3) for first in (1, 1000) for scale in (1.0, 0.125)])
def test_adam_over_sizes_and_steps(n, first, scale):
    """One thread, around one workgroup, past the 4096-block cap (grid-stride loop); steps 1-3 and 1000-1002 with non-zero moments for the
    bias-correction powers; grad_scale folded into the kernel."""
    L_ = _lib()
    p, g, m, v = _adam_case(n, first)
    want = _adam_ref(n, first, scale)
    pd, md, vd = Guarded(n, init=p), Guarded(n, init=m), Guarded(n, init=v)
    for k in range(3):
        gd = (ADAM_GRADS[k] * g).cuda()
        assert L_.sefd_adam_step(pd.ptr, _vp(gd), md.ptr, vd.ptr, n, first + k, LR, B1, B2, EPS, scale, None) == 0
    for b in (pd, md, vd):
        b.check()
    for got, ref, what in zip((pd, md, vd), want, ("param", "exp_avg", "exp_avg_sq")):
        assert rel_err(got.t.cpu(), ref) < ADAM_BAR, (what, rel_err(got.t.cpu(), ref))


@pytest.mark.parametrize("n", [257, 4096 * 256 + 3])
def test_guarded_adam_skips_when_the_status_word_is_set(n):
    import sefd_amd  # noqa: F401
    from sefd_amd.plan import Plan
    L_ = _lib()
    plan = Plan(1, 5, model="FullSubNet", fsn=dict(sb_num_neighbors=31, fb_num_neighbors=31, fb_hidden=64, sb_hidden=32))
    word = C.c_void_p(plan.status_word())
    p, g, m, v = _adam_case(n, 1000)
    pd, md, vd, gd = Guarded(n, init=p), Guarded(n, init=m), Guarded(n, init=v), g.cuda()
    plan.status_set()
    assert L_.sefd_adam_step_guarded(pd.ptr, _vp(gd), md.ptr, vd.ptr, n, 1000, LR, B1, B2, EPS, 1.0, word, None) == 0
    for b, before in ((pd, p), (md, m), (vd, v)):
        b.check()
        assert torch.equal(b.t.cpu(), before)
    assert plan.status(clear=True) == 1
    assert L_.sefd_adam_step_guarded(pd.ptr, _vp(gd), md.ptr, vd.ptr, n, 1000, LR, B1, B2, EPS, 1.0, word, None) == 0
    pd.check()
    assert rel_err(pd.t.cpu(), adam_update(p.double(), g.double(), m.double(), v.double(), 1000, LR, B1, B2, EPS)[0]) < ADAM_BAR


# ------------------------------------------------------------------------------------------ 5. mixing
@functools.lru_cache(maxsize=2)
def _mix_case(B, L, amp):
    """Speech and noise with a DC offset, SNRs spread over -5 .. 20 dB, distinct segment starts; amp scales both."""
    rng = np.random.default_rng(7 + B)
    speech = (amp * (rng.standard_normal((B, L)) * 0.05 + 0.003)).astype(np.float32)
    noise = (amp * (rng.standard_normal(L + 977 * B) * 0.2 - 0.01)).astype(np.float32)
    start = (np.arange(B) * 977 + 13).astype(np.int64)
    snr = np.linspace(-5.0, 20.0, B).astype(np.float32) if B > 1 else np.array([7.5], np.float32)
    return speech, noise, start, snr


def _mix_run(speech, noise, start, snr, quantize):
    B, L = speech.shape
    ws, out = Guarded(4 * B, torch.float64), Guarded(B * L)
    sd, nd, st, sn = (torch.from_numpy(a).cuda() for a in (speech, noise, start, snr))
    assert _lib().sefd_mix_snr(_vp(sd), _vp(nd), _vp(st), _vp(sn), B, L, 1 if quantize else 0, ws.ptr, out.ptr, None) == 0
    ws.check()
    out.check()
    return out.t.view(B, L).cpu().numpy().astype(np.float64)


MIX_SHAPES = [(1, 255), (1, 257), (3, 4099), (9, 240001)]      # below / above one workgroup; B * L > 8192 * 256: the apply kernel strides


@pytest.mark.parametrize("B,L", MIX_SHAPES)
def test_mixing_unquantized_over_shapes(B, L):
    speech, noise, start, snr = _mix_case(B, L, 1.0)
    got = _mix_run(speech, noise, start, snr, False)
    for b in range(B):
        want = generate_noisy_wav(speech[b].astype(np.float64), noise.astype(np.float64), float(snr[b]), int(start[b]), quantize=False)
        alone = generate_noisy_wav(speech[b], noise, float(snr[b]), int(start[b]), quantize=False)
        assert np.abs(want).max() < 1.0
        assert alone.dtype == np.float32 and np.abs(alone - want).max() < 0.1 * MIX_BAR, ("reference alone", b, np.abs(alone - want).max())
        assert np.abs(got[b] - want).max() < MIX_BAR, (b, np.abs(got[b] - want).max())


@pytest.mark.parametrize("B,L", MIX_SHAPES)
def test_mixing_quantized_over_shapes(B, L):
    """The int16 truncation.  Reference alone: an fp32 evaluation moves a sample across a truncation boundary with a probability of about
    2^-23 x its size in LSB, so the signals are kept near 50 LSB, where fp32 alone stays below a tenth of the 1e-4 share of samples beyond
    0.5 LSB; the step itself is 1 LSB for any arithmetic and cannot be held to a tenth.  The int16 path therefore runs at these shapes on quiet
    signals only; at full amplitude it is covered by test_on_gpu_snr_mixing_against_the_offline_script (B = 5, L = 48000)."""
    speech, noise, start, snr = _mix_case(B, L, 1.0 / 32)
    got = _mix_run(speech, noise, start, snr, True)
    for b in range(B):
        want = generate_noisy_wav(speech[b].astype(np.float64), noise.astype(np.float64), float(snr[b]), int(start[b])).astype(np.float64)
        alone = generate_noisy_wav(speech[b], noise, float(snr[b]), int(start[b])).astype(np.float64)
        assert np.abs(want).max() < 32768 and np.abs(want).max() > 100
        da = np.abs(alone - want)
        assert da.max() <= 1.0 and (da > 0.5).mean() < 0.1 * 1e-4, ("reference alone", b, da.max(), (da > 0.5).mean())
        d = np.abs(got[b] * 32768 - want)
        assert d.max() <= 1.0 + 1e-6 and (d > 0.5).mean() < 1e-4, (b, d.max(), (d > 0.5).mean())


# ------------------------------------------------------------------------------------------ 6. base pointers off 16 bytes
@pytest.mark.parametrize("close", [False, True])
@pytest.mark.parametrize("name", list(KINDS))
def test_long_row_losses_on_views_one_float_into_their_storage(name, close):
    """A contiguous view with a storage offset is aligned to 4 bytes only: the launcher must not take the float4 path for it, L % 4 == 0 or not."""
    B, L = 3, 4096
    est, tgt = _shape_case(B, L, close)
    relative = close and name == "MSE"
    v, ge, _, _ = _loss_ref(name, est, tgt, relative)
    off = lambda t: torch.cat([torch.zeros(1), t.reshape(-1), torch.zeros(3)]).cuda()[1:1 + B * L].view(B, L)
    ed, td = off(est), off(tgt)
    assert ed.is_contiguous() and ed.data_ptr() % 16 == 4 and td.data_ptr() % 16 == 4
    val, (g,) = _run_long(KINDS[name], ed, td, (None,))
    assert _value_err(val, v, relative) < VALUE_BAR and rel_err(g, ge) < GRAD_BAR
    ed.requires_grad_(True)
    out = _tfl(name)(ed, td)
    out.backward()
    assert _value_err(float(out.detach()), v, relative) < VALUE_BAR and rel_err(ed.grad.cpu(), ge) < GRAD_BAR
