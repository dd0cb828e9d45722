"""fp64 numpy restatement of the composite measure's frame analysis (Hu & Loizou 2006; reference composite.m, run there through Octave):
WSS, LLR and segmental SNR of a clean / processed pair, and the trimmed means that composite.m reports.  Written from the published
description of the measure, not from the Octave text; test helper only (the product computes the same numbers in csrc/composite.hip).

Conventions that decide the numbers:
  win = round(30 fs / 1000) (MATLAB round: half away from zero), skip = floor(win / 4), Hann-like window 0.5 (1 - cos(2 pi n / (win + 1))),
  n = 1..win; frame k starts at sample k * skip (0-based) and there are floor(L / skip - win / skip) frames; eps = 2^-52 is added to every
  sample before framing.  WSS and LLR are averaged over the smallest round(0.95 n) frame values, segSNR over all frames."""
import math

import numpy as np

EPS = 2.0 ** -52
# Klatt's 25 critical bands (centre frequency, bandwidth) in Hz, as published for the WSS measure
CENT = [50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72,
        1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63]
BW = [70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154,
      183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136]


def mround(x):
    """MATLAB round: half away from zero (numpy.round is half to even)."""
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def framing(fs):
    win = mround(30 * fs / 1000)
    return win, win // 4


def num_frames(L, fs):
    win, skip = framing(fs)
    return max(0, int(math.floor(L / skip - win / skip)))


def window(win):
    return 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, win + 1) / (win + 1)))


def n_fft(fs):
    win, _ = framing(fs)
    return 1 << (2 * win - 1).bit_length()


def lpc_order(fs):
    return 10 if fs < 10000 else 16


def crit_filter(fs):
    """[25, n_fft / 2] Gaussian band filters around floor(f0) with a log(bw_min / bw) gain, zeroed at or below the -30 dB factor."""
    half = n_fft(fs) // 2
    max_freq = fs / 2
    min_factor = math.exp(-30.0 / (2.0 * 2.303))
    j = np.arange(half, dtype=np.float64)
    out = np.zeros((25, half))
    for i in range(25):
        f0 = CENT[i] / max_freq * half
        bw = BW[i] / max_freq * half
        g = np.exp(-11 * ((j - math.floor(f0)) / bw) ** 2 + (math.log(BW[0]) - math.log(BW[i])))
        out[i] = g * (g > min_factor)
    return out


def frames(x, fs):
    """[n_frames, win] windowed frames of x + eps (x: 1-D, any float dtype; computed in fp64)."""
    win, skip = framing(fs)
    nf = num_frames(len(x), fs)
    x = np.asarray(x, np.float64) + EPS
    idx = np.arange(nf)[:, None] * skip + np.arange(win)[None, :]
    return x[idx] * window(win)[None, :]


def band_db(fr, fs):
    spec = np.abs(np.fft.fft(fr, n_fft(fs), axis=1)[:, :n_fft(fs) // 2]) ** 2
    return 10 * np.log10(np.maximum(spec @ crit_filter(fs).T, 1e-10))


def _loc_peak(E, S):
    """Nearest peak for bands 0..23: to the right while the slope is > 0, else to the left while it is <= 0 (a left search that runs off
    band 0 takes band 0).  The right search reports the band BEFORE the first non-positive slope, as the published code does."""
    nf = E.shape[0]
    peak = np.empty((nf, 24))
    for f in range(nf):
        for i in range(24):
            if S[f, i] > 0:
                n = i
                while n < 24 and S[f, n] > 0:
                    n += 1
                peak[f, i] = E[f, n - 1]
            else:
                n = i
                while n >= 0 and S[f, n] <= 0:
                    n -= 1
                peak[f, i] = E[f, n + 1]
    return peak


def wss_frames(clean, proc, fs):
    Ec, Ep = band_db(frames(clean, fs), fs), band_db(frames(proc, fs), fs)
    Sc, Sp = np.diff(Ec, axis=1), np.diff(Ep, axis=1)
    Pc, Pp = _loc_peak(Ec, Sc), _loc_peak(Ep, Sp)
    Wc = 20.0 / (20.0 + Ec.max(1, keepdims=True) - Ec[:, :24]) * (1.0 / (1.0 + Pc - Ec[:, :24]))
    Wp = 20.0 / (20.0 + Ep.max(1, keepdims=True) - Ep[:, :24]) * (1.0 / (1.0 + Pp - Ep[:, :24]))
    W = (Wc + Wp) / 2.0
    return (W * (Sc - Sp) ** 2).sum(1) / W.sum(1)


def autocorr(fr, P):
    win = fr.shape[1]
    return np.stack([(fr[:, :win - k] * fr[:, k:]).sum(1) for k in range(P + 1)], axis=1)


def levinson(R):
    """Levinson-Durbin on lags R[..., 0..P]: predictor a (R_toeplitz[0:P] a = R[1:P+1]); returns A = [1, -a]."""
    P = R.shape[-1] - 1
    a = np.zeros(R.shape[:-1] + (P,))
    E = R[..., 0].copy()
    for i in range(P):
        k = (R[..., i + 1] - (a[..., :i] * R[..., i:0:-1]).sum(-1)) / E
        prev = a[..., :i].copy()
        a[..., i] = k
        a[..., :i] = prev - k[..., None] * prev[..., ::-1]
        E = (1 - k * k) * E
    return np.concatenate([np.ones(R.shape[:-1] + (1,)), -a], axis=-1)


def llr_frames(clean, proc, fs):
    P = lpc_order(fs)
    Rc, Rp = autocorr(frames(clean, fs), P), autocorr(frames(proc, fs), P)
    Ac, Ap = levinson(Rc), levinson(Rp)
    i = np.arange(P + 1)
    T = Rc[:, np.abs(i[:, None] - i[None, :])]                    # [nf, P+1, P+1] Toeplitz of the clean lags
    num = np.einsum("fi,fij,fj->f", Ap, T, Ap)
    den = np.einsum("fi,fij,fj->f", Ac, T, Ac)
    return np.log(num / den)


def segsnr_frames(clean, proc, fs):
    c, p = frames(clean, fs), frames(proc, fs)
    s = 10 * np.log10((c ** 2).sum(1) / (((c - p) ** 2).sum(1) + EPS) + EPS)
    return np.clip(s, -10.0, 35.0)


def trimmed_mean(v, alpha=0.95):
    v = np.sort(np.asarray(v, np.float64))
    return float(v[:mround(len(v) * alpha)].mean()) if len(v) else float("nan")


def frame_measures(clean, proc, fs):
    """(llr, wss, segsnr) of one pair: the three numbers csrc/composite.hip writes per utterance."""
    n = min(len(clean), len(proc))
    clean, proc = np.asarray(clean)[:n], np.asarray(proc)[:n]
    seg = segsnr_frames(clean, proc, fs)
    return (trimmed_mean(llr_frames(clean, proc, fs)), trimmed_mean(wss_frames(clean, proc, fs)),
            float(seg.mean()) if len(seg) else float("nan"))


def combine(llr, wss, seg, pesq):
    """Regression of Hu & Loizou with the reference's order: composite.m clamps to [1, 5] with PESQ = 0, the Python wrapper adds PESQ after."""
    csig = min(5.0, max(1.0, 3.093 - 1.029 * llr - 0.009 * wss)) + 0.603 * pesq
    cbak = min(5.0, max(1.0, 1.634 - 0.007 * wss + 0.063 * seg)) + 0.478 * pesq
    covl = min(5.0, max(1.0, 1.594 - 0.512 * llr - 0.007 * wss)) + 0.805 * pesq
    return csig, cbak, covl
