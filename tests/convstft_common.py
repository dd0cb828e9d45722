"""Shared by tests/golden/make_convstft_golden.py, tests/test_convstft_cpu.py and tests/test_gpu_convstft.py: the case table, the closed-form
inputs and cotangents of a case, the error measures of the bar, and a float64 / float32 CPU restatement of ConvSTFT / ConviSTFT
(tools_for_model.py:16-112) for shapes that have no golden."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle.weights import splitmix_uniform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B = 2
# name: (win_len, hop, fft_len, L, window)
CASES = {
    "400_100_512_1000": (400, 100, 512, 1000, "hann"),
    "512_128_512_1100": (512, 128, 512, 1100, "hamming"),
    "400_160_512_1050": (400, 160, 512, 1050, None),
    "400_300_512_1500": (400, 300, 512, 1500, "hann"),
    "200_50_256_600": (200, 50, 256, 600, "hann"),
}
BAR = 4.0                      # per tensor: max|got - ref64| / max|ref64| <= BAR * ref32_err


def geometry(W, hop, NFFT, L):
    trim = W - hop
    T = (L + 2 * trim - W) // hop + 1
    return T, NFFT // 2 + 1, (T - 1) * hop + W - 2 * trim


def _u(idx, shape):
    return splitmix_uniform(idx, int(np.prod(shape))).reshape(shape)


def case_inputs(name, seed, batch=B, length=None):
    """float32 tensors of a case at a seed: waveform 0.1 u; complex input u; magnitudes |u|; phases 4 pi u; one cotangent u per output."""
    W, hop, NFFT, L, _ = CASES[name] if isinstance(name, str) else name
    L = length or L
    T, NF, Lout = geometry(W, hop, NFFT, L)
    s = 7000 + 32 * seed
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return dict(
        wav=f(0.1 * _u(s, (batch, L))),
        cot_out=f(_u(s + 1, (batch, 2 * NF, T))), cot_mags=f(_u(s + 2, (batch, NF, T))), cot_phase=f(_u(s + 3, (batch, NF, T))),
        spec_in=f(_u(s + 4, (batch, 2 * NF, T))), mags_in=f(np.abs(_u(s + 5, (batch, NF, T)))), phase_in=f(4.0 * math.pi * _u(s + 6, (batch, NF, T))),
        cot_wav=f(_u(s + 7, (batch, 1, Lout))))


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / float(ref.abs().max())


def phase_err(got, ref):
    """Circular difference, relative to max|ref|."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = torch.remainder(got - ref + math.pi, 2.0 * math.pi) - math.pi
    return float(d.abs().max()) / float(ref.abs().max())


ERR = {"phase": phase_err}


def err_of(key, got, ref):
    return ERR.get(key, rel_err)(got, ref)


# ---------------------------------------------------------------------------------------------- CPU restatement
def kernels64(W, NFFT, win_type):
    """float64 analysis kernel [2 NF, 1, W], synthesis kernel (pinv of the unwindowed basis, transposed, windowed) and window [W]."""
    from sefd_amd.frontend_consts import window_fn
    w = np.asarray(window_fn(win_type, W), dtype=np.float64)
    n = np.arange(W, dtype=np.float64)[None, :]
    k = np.arange(NFFT // 2 + 1, dtype=np.float64)[:, None]
    ang = 2.0 * np.pi * ((k * n) % NFFT) / NFFT
    K = np.concatenate([np.cos(ang), -np.sin(ang)], 0)
    Kinv = np.linalg.pinv(K).T
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return t(K * w)[:, None, :], t(Kinv * w)[:, None, :], t(w)


def ref_stft(x, K, W, hop, feature_type):
    if x.dim() == 2:
        x = x[:, None, :]
    out = F.conv1d(F.pad(x, [W - hop, W - hop]), K, stride=hop)
    if feature_type == "complex":
        return out
    NF = K.shape[0] // 2
    re, im = out[:, :NF], out[:, NF:]
    return torch.sqrt(re ** 2 + im ** 2), torch.atan2(im, re)


def ref_istft(inputs, phase, Kinv, win, W, hop):
    if phase is not None:
        inputs = torch.cat([inputs * torch.cos(phase), inputs * torch.sin(phase)], 1)
    out = F.conv_transpose1d(inputs, Kinv, stride=hop)
    T = inputs.shape[-1]
    coff = F.conv_transpose1d((win[None, :, None] ** 2).repeat(1, 1, T), torch.eye(W, dtype=win.dtype)[:, None, :], stride=hop)
    out = out / (coff + 1e-8)
    return out[..., W - hop:-(W - hop)]


def run_all(stft_c, stft_r, istft, inp, dtype):
    """Every output and input gradient of a case: `stft_c(x)`, `stft_r(x)`, `istft(a, phase)` are callables on tensors of `dtype`."""
    c = lambda k: inp[k].to(dtype).clone()
    res = {}
    x = c("wav").requires_grad_(True)
    y = stft_c(x)
    (y * c("cot_out")).sum().backward()
    res["out"], res["dwav_out"] = y.detach(), x.grad.detach()
    x = c("wav").requires_grad_(True)
    m, p = stft_r(x)
    ((m * c("cot_mags")).sum() + (p * c("cot_phase")).sum()).backward()
    res["mags"], res["phase"], res["dwav_real"] = m.detach(), p.detach(), x.grad.detach()
    s = c("spec_in").requires_grad_(True)
    w = istft(s, None)
    (w * c("cot_wav")).sum().backward()
    res["wav_spec"], res["dspec_in"] = w.detach(), s.grad.detach()
    a, ph = c("mags_in").requires_grad_(True), c("phase_in").requires_grad_(True)
    w = istft(a, ph)
    (w * c("cot_wav")).sum().backward()
    res["wav_polar"], res["dmags_in"], res["dphase_in"] = w.detach(), a.grad.detach(), ph.grad.detach()
    return res


def restated(shape, inp, dtype):
    """run_all over the CPU restatement at `dtype` (kernels computed in float64, then cast)."""
    W, hop, NFFT, _, win_type = shape
    K, Kinv, win = (t.to(dtype) for t in kernels64(W, NFFT, win_type))
    return run_all(lambda x: ref_stft(x, K, W, hop, "complex"), lambda x: ref_stft(x, K, W, hop, "real"),
                   lambda a, ph: ref_istft(a, ph, Kinv, win, W, hop), inp, dtype)


def measure(res64, res32):
    """ref32_err per tensor: the float32 run against the float64 run."""
    return {k: err_of(k, res32[k], res64[k]) for k in res64}


STFT_KEYS = ("out", "dwav_out", "mags", "phase", "dwav_real")
ISTFT_KEYS = ("wav_spec", "dspec_in", "wav_polar", "dmags_in", "dphase_in")


def load_golden(name):
    """(seed, {key: float64-reference tensor (stored rounded to float32)}, {key: ref32_err}) of a case, from its two fixture files."""
    ref, e32, seed = {}, {}, None
    for part in ("stft", "istft"):
        z = np.load(os.path.join(GOLDEN, f"convstft_{name}_{part}.npz"))
        seed = int(z["seed"])
        for k in z.files:
            if k.startswith("ref/"):
                ref[k[4:]] = torch.from_numpy(z[k])
            elif k.startswith("ref32_err/"):
                e32[k[10:]] = float(z[k])
    return seed, ref, e32
