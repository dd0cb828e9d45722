"""Time the GPU STOI scorer against the host scorer on B = 10 (the reference's cfg.batch) and B = 256 clips of 3 s at 16 kHz: device time of
`stoi_batch` (HIP events, 3 warm-ups, median of 20), wall time of host `cal_stoi` on the same batch, and a validation-style step both ways:
host PESQ followed by host STOI, against host PESQ with the GPU STOI enqueued underneath.  Prints one JSON line.

    python tools/stoi_timing.py [--threads 16]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sefd_amd  # noqa: E402,F401
from sefd_amd import tools_for_estimate as te  # noqa: E402
from stoi_cases import speechlike_pair  # noqa: E402


def _median_wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def measure(B, threads, fs=16000, seconds=3):
    L = seconds * fs
    pairs = [speechlike_pair(L, fs, 7000 + i, float(-5 + (i % 6) * 5)) for i in range(B)]
    c, e = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    C, E = torch.from_numpy(c).cuda(), torch.from_numpy(e).cuda()
    for _ in range(3):
        te.stoi_batch(C, E, fs)
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        te.stoi_batch(C, E, fs)
        t.record()
        t.synchronize()
        ts.append(s.elapsed_time(t))
    host = np.array(te.cal_stoi(e, c, nthreads=threads))
    diff = float(np.abs(te.stoi_batch(C, E, fs).cpu().numpy() - host).max())
    reps = 5 if B <= 16 else 3

    def host_step():
        est, clean = E.cpu().numpy(), C.cpu().numpy()
        te.cal_pesq(est, clean, nthreads=threads)
        te.cal_stoi(est, clean, nthreads=threads)

    def gpu_step():
        dev = te.stoi_batch(C, E, fs)
        est, clean = E.cpu().numpy(), C.cpu().numpy()
        te.cal_pesq(est, clean, nthreads=threads)
        dev.cpu().numpy()

    return {"B": B, "stoi_gpu_ms_median": float(np.median(ts)), "stoi_gpu_ms_min": float(np.min(ts)),
            "stoi_host_s": _median_wall(lambda: te.cal_stoi(e, c, nthreads=threads), reps),
            "step_host_pesq_host_stoi_s": _median_wall(host_step, reps), "step_host_pesq_gpu_stoi_s": _median_wall(gpu_step, reps),
            "max_abs_gpu_minus_host": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    assert te.cfg.fs == 16000
    print(json.dumps({"clip_s": 3, "fs": 16000, "host_threads": a.threads, "device": torch.cuda.get_device_name(0),
                      "batches": [measure(B, a.threads) for B in (10, 256)]}))


if __name__ == "__main__":
    main()
