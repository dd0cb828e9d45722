"""Time the composite measure on B = 256 x 3 s clips at 16 kHz: the HIP frame kernels on the device (events, median of 20), the fp64 numpy
restatement (tests/composite_ref.py) and the host PESQ port on the same batch, and the overlapped `composite_batch` wall time.

    python tools/composite_timing.py [--B 256] [--threads 16]"""
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
import composite_ref as cr  # noqa: E402
from test_gpu_composite import speechlike_pair  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    fs, L = 16000, 3 * 16000
    pairs = [speechlike_pair(L, fs, 5000 + i, float(-5 + (i % 6) * 5)) for i in range(a.B)]
    c = np.stack([p[0] for p in pairs])
    e = np.stack([p[1] for p in pairs])
    C, E = torch.from_numpy(c).cuda(), torch.from_numpy(e).cuda()
    for _ in range(3):
        te.composite_frames(C, E, fs)
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        te.composite_frames(C, E, fs)
        t.record()
        t.synchronize()
        ts.append(s.elapsed_time(t))
    t0 = time.perf_counter()
    for b in range(a.B):
        cr.frame_measures(c[b].astype(np.float64), e[b].astype(np.float64), fs)
    host_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    te._pesq(e, c, fs, a.threads)
    pesq_s = time.perf_counter() - t0
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        te.composite_batch(C, E, fs=fs, nthreads=a.threads)
        walls.append(time.perf_counter() - t0)
    print(json.dumps({"B": a.B, "clip_s": 3, "fs": fs, "frames_per_clip": cr.num_frames(L, fs), "pesq_threads": a.threads,
                      "frame_kernels_ms_median": float(np.median(ts)), "host_restatement_s": host_ref, "host_pesq_s": pesq_s,
                      "composite_batch_wall_s_median": float(np.median(walls))}))


if __name__ == "__main__":
    main()
