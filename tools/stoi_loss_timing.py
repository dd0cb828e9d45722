"""Time the STOI / ESTOI loss (tools_for_loss.stoi_loss, csrc/stoi.hip) on B = 32 clips of 3 s at 16 kHz: device time of the forward alone and of
forward + backward (HIP events, 3 warm-ups, median of 20).  Prints one JSON line.

    python tools/stoi_loss_timing.py [--batch 32]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sefd_amd  # noqa: E402,F401
from sefd_amd import tools_for_loss as tfl  # noqa: E402
from stoi_cases import speechlike_pair  # noqa: E402


def _events(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        t.synchronize()
        ts.append(s.elapsed_time(t))
    return float(np.median(ts)), float(np.min(ts))


def measure(B, extended, fs=16000, seconds=3):
    L = seconds * fs
    pairs = [speechlike_pair(L, fs, 7000 + i, float(-5 + (i % 6) * 5)) for i in range(B)]
    C = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    E = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda().requires_grad_()

    def fwd():
        with torch.no_grad():
            return tfl.stoi_loss(C, E, fs, extended)

    def both():
        E.grad = None
        tfl.stoi_loss(C, E, fs, extended).backward()

    f, b = _events(fwd), _events(both)
    return {"extended": extended, "forward_ms_median": f[0], "forward_ms_min": f[1], "forward_backward_ms_median": b[0],
            "forward_backward_ms_min": b[1], "loss": float(fwd())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    print(json.dumps({"B": a.batch, "clip_s": 3, "fs": 16000, "device": torch.cuda.get_device_name(0),
                      "runs": [measure(a.batch, x) for x in (False, True)]}))


if __name__ == "__main__":
    main()
