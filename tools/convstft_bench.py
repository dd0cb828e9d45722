"""Time of the four phases of ConvSTFT / ConviSTFT on their own, the fused inverse-FFT + overlap-add kernel against the composition of existing
ops (OP_ISTFT_FFT + overlap-add, the default; the fused kernel is planned on the knob CONVSTFT_FUSE), same process.

    python tools/convstft_bench.py [--out profiles/convstft_bench.json]

ConvSTFT(400, 100, 512, 'hann') / ConviSTFT at bench.py's DCCRN clip shape (B = 32 clips of 48000 samples), fp32, both feature types.  The plans'
phases are launched directly on resident arenas (no host copies): 20 warm-up launches, then 200 launches per phase and arm, each between two
device events, the arms alternating; the median per phase is reported.  ConvSTFT's backward and ConviSTFT's forward are the phases the two
arms differ in; for those the medians of the per-op times (Plan.run_timed, 50 runs) of the ops that differ are reported too."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OP_NAMES = {1: "RUNGEMM", 15: "OLA_FWD", 16: "OLA_BWD", 37: "STFT_FFT", 39: "ISTFT_FFT", 49: "IFFT_OLA", 50: "SPECCONV"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convstft_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=200)
    a = ap.parse_args()
    import sefd_amd  # noqa: F401
    from sefd_amd import tuning
    from sefd_amd.plan import PHASE_BWD, PHASE_FWD, Plan

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    arms = {}
    for arm in ("fused", "composed"):                        # a plan is a function of the knob table when it is built
        tuning.clear()
        if arm == "fused":
            tuning.set("CONVSTFT_FUSE", "1")
        for ft in ("complex", "real"):
            ps = Plan(a.batch, a.samples, win_len=400, win_inc=100, fft_len=512, model="ConvSTFT", win_type="hann", feature_type=ft)
            pi = Plan(a.batch, ps.T, win_len=400, win_inc=100, fft_len=512, model="ConviSTFT", win_type="hann", feature_type=ft)
            for name, plan in (("ConvSTFT", ps), ("ConviSTFT", pi)):
                ar = plan.alloc_arenas(dev)
                io = ar[5].view(torch.float32)               # every IO buffer holds plausible values: inputs, cotangents
                io.copy_((torch.rand(io.numel(), generator=gen) - 0.5).to(dev))
                arms[(arm, name, ft)] = dict(plan=plan, ar=ar, ms={PHASE_FWD: [], PHASE_BWD: []})
    tuning.clear()
    stream = torch.cuda.current_stream().cuda_stream

    def run(r, phase):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r["plan"].run(phase, r["ar"], stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for i in range(a.warmup + a.runs):
        for r in arms.values():
            for phase in (PHASE_FWD, PHASE_BWD):
                ms = run(r, phase)
                if i >= a.warmup:
                    r["ms"][phase].append(ms)
    rec = dict(shape=dict(B=a.batch, L=a.samples, win_len=400, hop=100, fft_len=512, window="hann"), dtype="fp32", warmup=a.warmup, runs=a.runs,
               device=torch.cuda.get_device_name(0), phases={}, ops={})
    for (arm, name, ft), r in arms.items():
        for phase, tag in ((PHASE_FWD, "fwd"), (PHASE_BWD, "bwd")):
            kinds = [int(k) for k in r["plan"].op_kinds(phase)[0]]
            rec["phases"][f"{name}.{ft}.{tag}.{arm}"] = dict(ms_median=round(statistics.median(r["ms"][phase]), 5), ms_min=round(min(r["ms"][phase]), 5),
                                                            ops=[OP_NAMES.get(k, str(k)) for k in kinds])
    # the ops the arms differ in, one by one
    for (arm, name, ft), r in arms.items():
        if ft != "complex":
            continue
        phase, tag = (PHASE_BWD, "bwd") if name == "ConvSTFT" else (PHASE_FWD, "fwd")
        kinds = [int(k) for k in r["plan"].op_kinds(phase)[0]]
        per = [r["plan"].run_timed(phase, r["ar"], stream) for _ in range(50)]
        med = [statistics.median(p[i] for p in per) for i in range(len(kinds))]
        rec["ops"][f"{name}.{tag}.{arm}"] = {OP_NAMES.get(k, str(k)): round(m, 5) for k, m in zip(kinds, med) if k in (15, 39, 49)}
    for name, tag in (("ConvSTFT", "bwd"), ("ConviSTFT", "fwd")):
        f, c = (sum(rec["ops"][f"{name}.{tag}.{arm}"].values()) for arm in ("fused", "composed"))
        rec[f"{name}_{tag}_composed_over_fused"] = round(c / f, 3)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
