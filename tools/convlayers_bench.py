"""Time of the conv layers on their own (models 9, csrc/plan_layers.cpp) and of their layout kernel (csrc/layout.hip) alone, one process.

    python tools/convlayers_bench.py [--out profiles/convlayers_bench.json]

ComplexConv2d(64, 128, (5, 2), (2, 1), (2, 1)) and ComplexConvTranspose2d(256, 64, (5, 2), (2, 1), (2, 0), (1, 0)) at B = 32, F = 64, T = 483 (a DCCRN
encoder / decoder layer at bench.py's clip shape) in bf16: the plans' phases are launched directly on resident arenas (no host copies), warm-up
launches first, then each phase between two device events, the arms alternating; medians are reported.  The four layout launches of each plan
(input in, output out, cotangent in, input gradient out) are timed alone the same way; their rate is bytes moved (the fp32 tensor on one side, the
padded bf16 tensor on the other) per second, reported beside the streaming-copy rate of the chip (6.3 TB/s for a float4 copy), with the 64 x 64 tile
(default) and the 32 x 32 tile (knob LAYOUT_TILE=32, read per launch) alternating.  No target."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OP_NCHW_CL = 51
COPY_TBS = 6.3                 # measured float4 streaming copy on the MI355X
MODES = {0: "input_in", 1: "output_out", 2: "cotangent_in", 3: "input_gradient_out"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convlayers_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--frames", type=int, default=483)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=50)
    a = ap.parse_args()
    import sefd_amd  # noqa: F401
    from sefd_amd import tuning
    from sefd_amd.plan import PHASE_BWD, PHASE_FWD, Plan

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    layers = {
        "ComplexConv2d(64,128,(5,2),(2,1),(2,1))": dict(kind="ComplexConv2d", in_channels=64, out_channels=128, kernel_size=(5, 2), stride_f=2, padding=(2, 1)),
        "ComplexConvTranspose2d(256,64,(5,2),(2,1),(2,0),(1,0))": dict(kind="ComplexConvTranspose2d", in_channels=256, out_channels=64, kernel_size=(5, 2),
                                                                    stride_f=2, padding=(2, 0), output_padding_f=1),
    }
    arms = {}
    for name, conv in layers.items():
        plan = Plan(a.batch, a.frames, act_dtype="bf16", model="ConvLayer", conv=dict(conv, F=a.bins))
        ar = plan.alloc_arenas(dev)
        ar[1].copy_((0.1 * (torch.rand(ar[1].numel(), generator=gen) - 0.5)).to(dev))
        io = ar[5].view(torch.float32)
        io.copy_((torch.rand(io.numel(), generator=gen) - 0.5).to(dev))
        arms[name] = dict(plan=plan, ar=ar, ms={PHASE_FWD: [], PHASE_BWD: []}, lay={})
    stream = torch.cuda.current_stream().cuda_stream

    def timed(plan, ar, phase, first=0, last=-1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.run(phase, ar, stream, first, last)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for i in range(a.warmup + a.runs):
        for r in arms.values():
            for phase in (PHASE_FWD, PHASE_BWD):
                ms = timed(r["plan"], r["ar"], phase)
                if i >= a.warmup:
                    r["ms"][phase].append(ms)
    for i in range(a.warmup + a.runs):
        for r in arms.values():
            for phase in (PHASE_FWD, PHASE_BWD):
                for k in range(r["plan"].num_ops(phase)):
                    info = r["plan"].op_info(phase, k)
                    if info["kind"] != OP_NCHW_CL:
                        continue
                    for tile in (64, 32):
                        tuning.set("LAYOUT_TILE", str(tile))
                        ms = timed(r["plan"], r["ar"], phase, k, k + 1)
                        if i >= a.warmup:
                            r["lay"].setdefault((info["flags"], info["bytes"], tile), []).append(ms)
                    tuning.clear()
    rec = dict(shape=dict(B=a.batch, F=a.bins, T=a.frames), dtype="bf16", warmup=a.warmup, runs=a.runs, device=torch.cuda.get_device_name(0),
               streaming_copy_TBs=COPY_TBS, layers={})
    for name, r in arms.items():
        out = dict(fwd_ms_median=round(statistics.median(r["ms"][PHASE_FWD]), 5), bwd_ms_median=round(statistics.median(r["ms"][PHASE_BWD]), 5),
                   fwd_ms_min=round(min(r["ms"][PHASE_FWD]), 5), bwd_ms_min=round(min(r["ms"][PHASE_BWD]), 5),
                   out_shape=[a.batch, r["plan"].conv["out_channels"], r["plan"].buffer("io.y")[2] // 4 // a.batch // r["plan"].conv["out_channels"] // r["plan"].T,
                              r["plan"].T], layout={})
        for (mode, nbytes, tile), ms in r["lay"].items():
            med = statistics.median(ms)
            tbs = nbytes / (med * 1e-3) / 1e12
            out["layout"][f"{MODES[mode]}.tile{tile}"] = dict(bytes=nbytes, ms_median=round(med, 5), TBs=round(tbs, 3), of_streaming_copy=round(tbs / COPY_TBS, 3))
        rec["layers"][name] = out
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
