"""Reference of the STOI / ESTOI loss tests (tests/test_stoi_loss_cpu.py, tests/test_gpu_stoi_loss.py): a float64 numpy restatement of extended
STOI (Jensen & Taal, "An Algorithm for Predicting the Intelligibility of Speech Masked by Modulated Noise Maskers", IEEE/ACM TASLP 2016) on
the framing of oracle/stoi.py, and a float64 torch restatement of STOI and ESTOI whose gradient with respect to the estimate comes from torch
autograd.  In the torch form the silent-frame selection is computed from the clean signal without gradient, and the resampler is a strided
convolution with oracle.stoi.resample_window (scipy.signal.resample_poly's alignment)."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import stoi_cases as sc
from oracle import stoi as so

CLIP = 1 + 10 ** (-so.BETA / 20)
HOP = so.N_FRAME // 2


# ------------------------------------------------------------------------------------------------------------ numpy: ESTOI
def _row_col_normalize(a):
    """[J, 15, 30]: every row (band over time), then every column (frame over bands): mean removed, divided by (norm + eps)."""
    a = a - a.mean(axis=2, keepdims=True)
    a = a / (np.linalg.norm(a, axis=2, keepdims=True) + so.EPS)
    a = a - a.mean(axis=1, keepdims=True)
    return a / (np.linalg.norm(a, axis=1, keepdims=True) + so.EPS)


def estoi_numpy(clean, est, fs):
    x, y = np.asarray(clean, dtype=np.float64), np.asarray(est, dtype=np.float64)
    if fs != so.FS:
        x, y = so.resample(x, so.FS, fs), so.resample(y, so.FS, fs)
    x, y = so.remove_silent_frames(x, y)
    X, Y = so._spec(x), so._spec(y)
    if X.ndim < 2 or X.shape[-1] < so.N_SEG:
        return 1e-5
    obm = so.thirdoct()
    xt, yt = np.sqrt(obm @ np.abs(X) ** 2), np.sqrt(obm @ np.abs(Y) ** 2)
    xs = np.array([xt[:, m - so.N_SEG:m] for m in range(so.N_SEG, xt.shape[1] + 1)])
    ys = np.array([yt[:, m - so.N_SEG:m] for m in range(so.N_SEG, xt.shape[1] + 1)])
    return float((_row_col_normalize(xs) * _row_col_normalize(ys)).sum() / so.N_SEG / xs.shape[0])


# ------------------------------------------------------------------------------------------------------------ torch: STOI / ESTOI
def _resample_t(x, fs):
    """resample_poly(x, 10000, fs, window=h / sum(h)) as a strided convolution of the zero-stuffed signal (float64 tensor [L])."""
    g = math.gcd(so.FS, fs)
    up, down = so.FS // g, fs // g
    h = so.resample_window(so.FS, fs)
    h = h / h.sum()
    T = len(h)
    half = (T - 1) // 2
    pre = down - half % down
    pre_remove = (half + pre) // down
    L = x.shape[0]
    n_out = -(-L * up // down)
    xu = torch.zeros(L * up, dtype=torch.float64)
    xu = xu.index_add(0, torch.arange(L) * up, x)
    # out[o] = up * sum_i h[i] xu[(o + pre_remove) down - pre - i]: a cross-correlation with the flipped filter, the input shifted by `left`
    left = -(pre_remove * down - pre - (T - 1))
    assert left >= 0
    need = (n_out - 1) * down + T
    inp = F.pad(xu, (left, max(0, need - left - L * up)))
    w = torch.from_numpy(np.ascontiguousarray(h[::-1]))
    return F.conv1d(inp[None, None], w[None, None], stride=down)[0, 0, :n_out] * up


def _frames(x):
    """[frames, 256] of x, hop 128, frames start while i < len(x) - 256 (strict)."""
    n = len(range(0, x.shape[0] - so.N_FRAME, HOP))
    if n == 0:
        return x.new_zeros((0, so.N_FRAME))
    return x.unfold(0, so.N_FRAME, HOP)[:n]


def stoi_torch(clean, est, fs, extended=False, detail=None):
    """STOI (or ESTOI) of one pair as a float64 0-d tensor, differentiable in `est` (a float64 tensor [L]); `clean` is a numpy array.
    detail (a dict): receives the clip-fence figures of the STOI correlate stage."""
    x = torch.from_numpy(np.asarray(clean, dtype=np.float64))
    y = est
    if fs != so.FS:
        x, y = _resample_t(x, fs), _resample_t(y, fs)
    w = torch.from_numpy(so._window())
    xf, yf = _frames(x) * w, _frames(y) * w
    floor = y.sum() * 0 + 1e-5
    if xf.shape[0] == 0:
        return floor
    with torch.no_grad():
        e = 20 * np.log10(np.linalg.norm(xf.numpy(), axis=1) + so.EPS)
        keep = torch.from_numpy((e.max() - so.DYN_RANGE - e) < 0)
    xf, yf = xf[keep], yf[keep]
    K = xf.shape[0]
    idx = (torch.arange(K)[:, None] * HOP + torch.arange(so.N_FRAME)[None]).reshape(-1)
    n = (K - 1) * HOP + so.N_FRAME
    xs = torch.zeros(n, dtype=torch.float64).index_add(0, idx, xf.reshape(-1))
    ys = torch.zeros(n, dtype=torch.float64).index_add(0, idx, yf.reshape(-1))
    X, Y = torch.fft.rfft(_frames(xs) * w, n=so.NFFT), torch.fft.rfft(_frames(ys) * w, n=so.NFFT)       # [frames, 257]
    if X.shape[0] < so.N_SEG:
        return floor
    obm = torch.from_numpy(so.thirdoct())
    xt = torch.sqrt((X.real ** 2 + X.imag ** 2) @ obm.T).T                                             # [15, frames]
    yt = torch.sqrt((Y.real ** 2 + Y.imag ** 2) @ obm.T).T
    xs, ys = xt.unfold(1, so.N_SEG, 1).permute(1, 0, 2), yt.unfold(1, so.N_SEG, 1).permute(1, 0, 2)   # [J, 15, 30]
    norm = lambda a, d: torch.sqrt((a * a).sum(dim=d, keepdim=True))
    if extended:
        def rc(a):
            a = a - a.mean(dim=2, keepdim=True)
            a = a / (norm(a, 2) + so.EPS)
            a = a - a.mean(dim=1, keepdim=True)
            return a / (norm(a, 1) + so.EPS)
        return (rc(xs) * rc(ys)).sum() / so.N_SEG / xs.shape[0]
    c = norm(xs, 2) / (norm(ys, 2) + so.EPS)
    if detail is not None:
        with torch.no_grad():
            u, v = ys * c, xs * CLIP
            detail["margin"] = float(((u - v).abs() / v).min())
            detail["clipped"] = float((u > v).double().mean())
    yp = torch.minimum(ys * c, xs * CLIP)
    yp = yp - yp.mean(dim=2, keepdim=True)
    xs = xs - xs.mean(dim=2, keepdim=True)
    yp = yp / (norm(yp, 2) + so.EPS)
    xs = xs / (norm(xs, 2) + so.EPS)
    return (yp * xs).sum() / (xs.shape[0] * xs.shape[1])


def score_and_grad(clean, est, fs, extended=False, weights=None):
    """(d [B] float64, grad [B, L] float64 of sum_b weights[b] d_b with respect to est, details [B]) for numpy batches [B, L]."""
    clean, est = np.atleast_2d(clean), np.atleast_2d(est)
    B = clean.shape[0]
    weights = np.ones(B) if weights is None else np.asarray(weights, dtype=np.float64)
    d, grads, details = np.zeros(B), np.zeros(est.shape), []
    for b in range(B):
        e = torch.from_numpy(est[b].astype(np.float64)).requires_grad_()
        det = {}
        s = stoi_torch(clean[b], e, fs, extended, det)
        (s * float(weights[b])).backward()
        d[b], grads[b] = float(s.detach()), e.grad.numpy()
        details.append(det)
    return d, grads, details


# ------------------------------------------------------------------------------------------------------------ shared cases
WEIGHTS = np.array([1.0, -0.5, 2.0, 0.25])         # unequal upstream weights of the four rows of speechlike_case


@functools.lru_cache(maxsize=None)
def speech_reference(fs, extended):
    """The compared case of a rate, scored once: speechlike_case(fs + 123) with WEIGHTS.  (clean, est, d, grad, details); leave them unchanged."""
    clean, est = sc.speechlike_case(fs + 123)
    d, grad, details = score_and_grad(clean, est, fs, extended, WEIGHTS)
    return clean, est, d, grad, details


def edge_pair(L):
    """The noise pair of tests/test_gpu_stoi.py::test_frame_count_edges, cut to L samples (10 kHz, every frame kept)."""
    rng = np.random.default_rng(21)
    clean = (0.1 * rng.standard_normal(6000)).astype(np.float32)
    est = (clean + 0.05 * rng.standard_normal(6000)).astype(np.float32)
    return clean[:L], est[:L]


@functools.lru_cache(maxsize=None)
def edge_reference(L, extended):
    clean, est = edge_pair(L)
    d, grad, details = score_and_grad(clean, est, 10000, extended)
    return clean, est, d[0], grad[0], details[0]


def grad_bound(ref_row):
    """Per element: one fp32 rounding of the store (2^-24 relative), doubled, plus the project's 1e-9 STOI bar scaled by the row's largest
    gradient for the fp64 summation order."""
    return 2.0 ** -23 * np.abs(ref_row) + 1e-9 * np.abs(ref_row).max()
