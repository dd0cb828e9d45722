"""Objective scorers of the validation loop (reference tools_for_estimate.py:51-125) on the package's C++ library
(`libsefd_scorers.so`, csrc_host/scorers.cpp, C ABI in include/sefd_scorers.h) instead of pystoi / the x86-only PESQ.so.

Same call shapes as the reference: `cal_stoi(estimated_speechs, clean_speechs)` and `cal_pesq(dirty_wavs, clean_wavs)` (wide-band
P.862 MOS-LQO, csrc_host/pesq.cpp) take
`[B, L]` arrays and return per-utterance scores; `cal_snr` is the numpy one-liner of tools_for_estimate.py:104-112.

The composite measure (tools_for_estimate.py:24-45, composite.m): `composite(clean_path, enhanced_path)` and `pesq_mos(clean_path,
enhanced_path)` keep the reference signatures; `composite_batch(clean, enhanced)` scores cuda `[B, L]` batches, the frame analysis (WSS, LLR,
segSNR) in HIP (csrc/composite.hip, sefd_composite_frames) overlapped with the host PESQ.

`stoi_batch(clean, enhanced)` is cal_stoi's arithmetic on the device (csrc/stoi.hip, sefd_stoi_gpu): cuda `[B, L]` in, cuda fp64 `[B]` out on
the current stream; `composite_batch(..., stoi=True)` and the validation loop with `scorers="gpu"` run it under the host PESQ."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import config as cfg

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsefd_scorers.so")
SRC = os.path.join(HERE, "csrc_host", "scorers.cpp")
SRCS = [SRC, os.path.join(HERE, "csrc_host", "pesq.cpp")]
HDRS = [os.path.join(HERE, "csrc_host", "pesq_tables.h"), os.path.join(HERE, "csrc_host", "stoi_tables.h")]
_lib = None


def build(force=False):
    from . import build as _b
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", LIB_PATH] + SRCS
    digest = _b.source_digest(SRCS + HDRS, " ".join(cmd[:-len(SRCS)]))        # contents, not mtimes (build.source_digest)
    if force or not _b.stamp_current(LIB_PATH, digest):
        subprocess.run(cmd, check=True)
        _b.write_stamp(LIB_PATH, digest)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        L.sefd_stoi_batch.restype = C.c_int32
        L.sefd_stoi_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
        L.sefd_stoi_batch_ex.restype = C.c_int32
        L.sefd_stoi_batch_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
        L.sefd_pesq_batch.restype = C.c_int32
        L.sefd_pesq_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
        _lib = L
    return _lib


EXPORTED = ["sefd_stoi_batch", "sefd_stoi_batch_ex", "sefd_pesq_batch"]


def _pair(est, clean):
    est = np.ascontiguousarray(np.atleast_2d(np.asarray(est)), dtype=np.float32)
    clean = np.ascontiguousarray(np.atleast_2d(np.asarray(clean)), dtype=np.float32)
    if est.shape != clean.shape:
        raise ValueError(f"shape mismatch {est.shape} vs {clean.shape}")
    return est, clean


def cal_stoi(estimated_speechs, clean_speechs, nthreads=0, *, extended=False):
    """tools_for_estimate.py:91-99: STOI(clean, estimated, cfg.fs, extended=False) per utterance; extended=True scores extended STOI
    (Jensen & Taal 2016, sefd_stoi_batch_ex), which the reference never asks for."""
    est, clean = _pair(estimated_speechs, clean_speechs)
    out = np.zeros(est.shape[0], dtype=np.float64)
    if extended:
        rc = lib().sefd_stoi_batch_ex(clean.ctypes.data, est.ctypes.data, est.shape[0], est.shape[1], int(cfg.fs), 1, out.ctypes.data, nthreads)
    else:
        rc = lib().sefd_stoi_batch(clean.ctypes.data, est.ctypes.data, est.shape[0], est.shape[1], int(cfg.fs), out.ctypes.data, nthreads)
    if rc != 0:
        raise RuntimeError(f"sefd_stoi_batch failed ({rc})")
    return list(out)


def cal_pesq(dirty_wavs, clean_wavs, nthreads=0):
    """tools_for_estimate.py:68-84: wide-band PESQ MOS-LQO per utterance at cfg.fs = 16 kHz (the reference's PESQ.so is a 16 kHz build):
    `pesq(clean, dirty)` of every pair.  C++ restatement of P.862 / P.862.2 (csrc_host/pesq.cpp), pinned to PESQ.so outputs."""
    return list(_pesq(dirty_wavs, clean_wavs, int(cfg.fs), nthreads))


def _pesq(dirty_wavs, clean_wavs, fs, nthreads=0):
    dirty, clean = _pair(dirty_wavs, clean_wavs)
    out = np.zeros(dirty.shape[0], dtype=np.float64)
    rc = lib().sefd_pesq_batch(clean.ctypes.data, dirty.ctypes.data, dirty.shape[0], dirty.shape[1], fs, out.ctypes.data, nthreads)
    if rc != 0:
        raise RuntimeError(f"sefd_pesq_batch failed ({rc}): needs cfg.fs == 16000 and at least 512 samples")
    return out


def cal_snr(s1, s2, eps=1e-8):
    """tools_for_estimate.py:104-112."""
    signal, noise = s2, s2 - s1
    return 10 * np.log10(np.sum(signal ** 2) / (np.sum(noise ** 2) + eps) + eps)


# ---------------------------------------------------------------------------------------------- composite measure
PESQ_FS = 16000          # the PESQ port is wide-band P.862.2 at 16 kHz only


def composite_frames(clean, enhanced, fs=None):
    """Frame measures of the composite measure on the GPU (sefd_composite_frames): cuda fp32 [B, L] clean / enhanced -> cuda fp64 [B, 3] =
    (95 % trimmed mean LLR, 95 % trimmed mean WSS, mean segSNR) per utterance, launched on the current stream (composite.m:56-75)."""
    import torch
    from . import _lib
    fs = int(cfg.fs if fs is None else fs)
    if not (clean.is_cuda and enhanced.is_cuda):
        raise RuntimeError("sefd composite runs on the MI355X only (cuda tensors); there is no CPU fallback")
    if clean.dim() != 2 or clean.shape != enhanced.shape:
        raise ValueError(f"composite: clean and enhanced must both be [B, L], got {tuple(clean.shape)} and {tuple(enhanced.shape)}")
    clean = clean.float().contiguous()
    enhanced = enhanced.float().contiguous()
    B, L = clean.shape
    L_ = _lib.lib()
    nbytes = L_.sefd_composite_ws_bytes(B, L, fs)
    if nbytes < 0:
        raise ValueError(f"composite: unsupported shape / rate (B={B}, L={L}, fs={fs}): code {nbytes} (include/sefd.h sefd_composite_frames)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=clean.device)
    out = torch.empty((B, 3), dtype=torch.float64, device=clean.device)
    rc = L_.sefd_composite_frames(clean.data_ptr(), enhanced.data_ptr(), B, L, fs, ws.data_ptr(), out.data_ptr(),
                                  torch.cuda.current_stream(clean.device).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"sefd_composite_frames failed ({rc})")
    return out


STOI_EXTENDED, STOI_KEEP = 1, 2        # flags of sefd_stoi_gpu_ex (include/sefd.h)


def stoi_forward_raw(clean, enhanced, fs, flags):
    """sefd_stoi_gpu_ex on the current stream: (scores fp64 [B], workspace).  With STOI_KEEP the workspace is what sefd_stoi_backward reads."""
    import torch
    from . import _lib
    if not (clean.is_cuda and enhanced.is_cuda):
        raise RuntimeError("sefd stoi_batch runs on the MI355X only (cuda tensors); there is no CPU fallback (cal_stoi is the host scorer)")
    if clean.dim() != 2 or clean.shape != enhanced.shape:
        raise ValueError(f"stoi: clean and enhanced must both be [B, L], got {tuple(clean.shape)} and {tuple(enhanced.shape)}")
    clean = clean.detach().float().contiguous()
    enhanced = enhanced.detach().float().contiguous()
    B, L = clean.shape
    L_ = _lib.lib()
    nbytes = L_.sefd_stoi_ws_bytes_ex(B, L, fs, flags)
    if nbytes < 0:
        raise ValueError(f"stoi: unsupported shape / rate (B={B}, L={L}, fs={fs}): code {nbytes} (include/sefd.h sefd_stoi_gpu)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=clean.device)
    out = torch.empty(B, dtype=torch.float64, device=clean.device)
    rc = L_.sefd_stoi_gpu_ex(clean.data_ptr(), enhanced.data_ptr(), B, L, fs, flags, ws.data_ptr(), out.data_ptr(),
                             torch.cuda.current_stream(clean.device).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"sefd_stoi_gpu_ex failed ({rc})")
    return out, ws


def stoi_backward_raw(B, L, fs, flags, ws, grad_out):
    """sefd_stoi_backward on the current stream: grad_out fp64 [B] -> d / d enhanced, fp32 [B, L]; `ws` from stoi_forward_raw with STOI_KEEP."""
    import torch
    from . import _lib
    grad_out = grad_out.detach().to(torch.float64).contiguous()
    grad = torch.empty((B, L), dtype=torch.float32, device=ws.device)
    rc = _lib.lib().sefd_stoi_backward(B, L, fs, flags, ws.data_ptr(), grad_out.data_ptr(), grad.data_ptr(),
                                       torch.cuda.current_stream(ws.device).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"sefd_stoi_backward failed ({rc})")
    return grad


def stoi_batch(clean, enhanced, fs=None, extended=False):
    """STOI on the GPU (sefd_stoi_gpu; the arithmetic of cal_stoi / csrc_host/scorers.cpp stoi_one in fp64): cuda [B, L] clean / enhanced at
    rate fs (default cfg.fs) -> cuda fp64 [B], launched on the current stream; nothing waits for the result.  extended=True: extended STOI
    (the arithmetic of cal_stoi(..., extended=True))."""
    import torch
    from . import _lib
    fs = int(cfg.fs if fs is None else fs)
    if extended:
        return stoi_forward_raw(clean, enhanced, fs, STOI_EXTENDED)[0]
    if not (clean.is_cuda and enhanced.is_cuda):
        raise RuntimeError("sefd stoi_batch runs on the MI355X only (cuda tensors); there is no CPU fallback (cal_stoi is the host scorer)")
    if clean.dim() != 2 or clean.shape != enhanced.shape:
        raise ValueError(f"stoi: clean and enhanced must both be [B, L], got {tuple(clean.shape)} and {tuple(enhanced.shape)}")
    clean = clean.float().contiguous()
    enhanced = enhanced.float().contiguous()
    B, L = clean.shape
    L_ = _lib.lib()
    nbytes = L_.sefd_stoi_ws_bytes(B, L, fs)
    if nbytes < 0:
        raise ValueError(f"stoi: unsupported shape / rate (B={B}, L={L}, fs={fs}): code {nbytes} (include/sefd.h sefd_stoi_gpu)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=clean.device)
    out = torch.empty(B, dtype=torch.float64, device=clean.device)
    rc = L_.sefd_stoi_gpu(clean.data_ptr(), enhanced.data_ptr(), B, L, fs, ws.data_ptr(), out.data_ptr(),
                          torch.cuda.current_stream(clean.device).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"sefd_stoi_gpu failed ({rc})")
    return out


def composite_batch(clean, enhanced, fs=None, pesq=True, nthreads=0, stoi=False):
    """CSIG / CBAK / COVL of a batch (tools_for_estimate.py:24-33 with composite.m): cuda [B, L] clean / enhanced -> dict of float64 numpy [B]
    arrays csig, cbak, covl, segsnr, llr, wss, pesq.  The frame kernels run on the current stream while the host scores PESQ (cal_pesq's
    threaded port) on a copy; then, in the reference's order, composite.m clamps 3.093 - 1.029 LLR - 0.009 WSS (CSIG), 1.634 - 0.007 WSS +
    0.063 segSNR (CBAK) and 1.594 - 0.512 LLR - 0.007 WSS (COVL) to [1, 5] and the wrapper adds 0.603 / 0.478 / 0.805 PESQ afterwards, so a
    result can leave [1, 5].  pesq=False skips PESQ (any supported rate): csig / cbak / covl / pesq are then NaN.  stoi=True adds "stoi"
    (stoi_batch, launched before the host PESQ starts; needs a rate sefd_stoi_gpu takes)."""
    fs = int(cfg.fs if fs is None else fs)
    if not (clean.is_cuda and enhanced.is_cuda):
        raise RuntimeError("sefd composite runs on the MI355X only (cuda tensors); there is no CPU fallback")
    if pesq and fs != PESQ_FS:
        raise ValueError(f"composite: the PESQ port is 16 kHz wide-band only (fs={fs}); use pesq=False for the frame measures alone")
    host = (clean.float().cpu().numpy(), enhanced.float().cpu().numpy()) if pesq else None      # copied BEFORE the launch: no wait on it
    frames = composite_frames(clean, enhanced, fs)
    stoi_dev = stoi_batch(clean, enhanced, fs) if stoi else None
    B = clean.shape[0]
    p = _pesq(host[1], host[0], fs, nthreads) if pesq else np.full(B, np.nan)
    m = frames.cpu().numpy()
    llr, wss, seg = m[:, 0].copy(), m[:, 1].copy(), m[:, 2].copy()
    csig = np.clip(3.093 - 1.029 * llr - 0.009 * wss, 1.0, 5.0) + 0.603 * p
    cbak = np.clip(1.634 - 0.007 * wss + 0.063 * seg, 1.0, 5.0) + 0.478 * p
    covl = np.clip(1.594 - 0.512 * llr - 0.007 * wss, 1.0, 5.0) + 0.805 * p
    res = {"csig": csig, "cbak": cbak, "covl": covl, "segsnr": seg, "llr": llr, "wss": wss, "pesq": p}
    if stoi:
        res["stoi"] = stoi_dev.cpu().numpy()
    return res


def read_wav_pair(clean: str, enhanced: str):
    """(fs, clean, enhanced) as float64, as composite.m:42-55 reads them: same rate and sample format or an error, integer samples scaled
    as audioread does (int16 / 2^15, int32 / 2^31, uint8 (x - 128) / 2^7, float as stored), both cut to the shorter length (mono files)."""
    from scipy.io import wavfile
    fs1, a = wavfile.read(clean)
    fs2, b = wavfile.read(enhanced)
    if fs1 != fs2 or a.dtype != b.dtype:
        raise ValueError(f"composite: the two files do not match ({fs1} Hz {a.dtype} vs {fs2} Hz {b.dtype})")
    if a.ndim != 1 or b.ndim != 1:
        raise ValueError("composite: mono files only")

    def scale(x):
        if x.dtype == np.int16:
            return x.astype(np.float64) / 32768.0
        if x.dtype == np.int32:
            return x.astype(np.float64) / 2147483648.0
        if x.dtype == np.uint8:
            return (x.astype(np.float64) - 128.0) / 128.0
        if x.dtype.kind == "f":
            return x.astype(np.float64)
        raise ValueError(f"composite: unsupported sample format {x.dtype}")
    n = min(len(a), len(b))
    return int(fs1), scale(a[:n]), scale(b[:n])


def pesq_mos(clean: str, enhanced: str):
    """tools_for_estimate.py:40-45: PESQ of two wav files of the same rate.  The port scores wide-band at 16 kHz only (the reference's
    narrow-band mode below 16 kHz is not available: an error); both signals are cut to the shorter length."""
    fs, c, e = read_wav_pair(clean, enhanced)
    if fs != PESQ_FS:
        raise ValueError(f"pesq_mos: the PESQ port is 16 kHz wide-band only, got {fs} Hz")
    return float(_pesq(e[None].astype(np.float32), c[None].astype(np.float32), fs)[0])


def composite(clean: str, enhanced: str):
    """tools_for_estimate.py:24-33: (csig, cbak, covl, segSNR) of two wav files; the frame analysis runs on the GPU (cuda:current)."""
    import torch
    fs, c, e = read_wav_pair(clean, enhanced)
    if fs != PESQ_FS:
        raise ValueError(f"composite: the PESQ port is 16 kHz wide-band only, got {fs} Hz")
    dev = torch.device("cuda", torch.cuda.current_device())
    r = composite_batch(torch.from_numpy(c.astype(np.float32))[None].to(dev), torch.from_numpy(e.astype(np.float32))[None].to(dev), fs=fs)
    return float(r["csig"][0]), float(r["cbak"][0]), float(r["covl"][0]), float(r["segsnr"][0])
