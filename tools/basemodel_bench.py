"""Time of BaseModel's `unfold` and seven norms on their own (csrc/basemodel.hip), forward + backward, one process.

    python tools/basemodel_bench.py [--out profiles/basemodel_bench.json]

Shapes: [32, 1, 257, T] for the 4-D norms and unfold (n = 15), [32, 257, T] for the recurrence norms (sample length 192), at T = 193 (the frames of a
FullSubNet training clip: not a multiple of 4, so the element-by-element path) and at T = 192 (the 16-byte path).  Three arms per op, alternating,
each sample between two device events right after an untimed call of the same arm, 10 warm-ups, median of 50:
  hip    the BaseModel static method under autograd: y = f(x); y.backward(cot)
  abi    the same kernels through sefd_norm_* / sefd_unfold_* on resident buffers (no autograd, no allocation): what the device does
  torch  the torch restatement of tests/basemodel_common.py (the reference's arithmetic: a Python loop over the frames for the recurrence
         norms) in float32 on the same device, under autograd
`of_streaming_copy` is the abi arm's rate over the bytes its kernels move (forward: x twice, y once; backward: grad_y and x twice - x a third time for
the layer norm and offline_gaussian - and grad_x once; unfold: input + output each way) against a float4 streaming copy measured in the same
process (torch's copy of 512 MiB).  No target: the parent commit cannot run any of this."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "basemodel_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--bins", type=int, default=257)
    ap.add_argument("--frames", type=int, nargs="+", default=[193, 192])
    ap.add_argument("--sample-length", type=int, default=192)
    ap.add_argument("--neighbors", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=50)
    a = ap.parse_args()
    import sefd_amd  # noqa: F401
    from sefd_amd import _lib
    from sefd_amd.models import BaseModel, _bm_geometry
    import basemodel_common as bc

    dev = torch.device("cuda:0")
    L_ = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())
    gen = torch.Generator().manual_seed(1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the float4 streaming copy of this device, now
    src = torch.empty(128 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_ms = [timed(lambda: dst.copy_(src)) for _ in range(a.warmup + a.runs)][a.warmup:]
    copy_tbs = 2 * src.numel() * 4 / (statistics.median(copy_ms) * 1e-3) / 1e12
    del src, dst

    ops = []
    for T in a.frames:
        for name in bc.NORMS4:
            ops.append((name, (a.batch, 1, a.bins, T), None))
        for name in bc.NORMS3:
            ops.append((name, (a.batch, a.bins, T), a.sample_length))
        ops.append(("unfold", (a.batch, 1, a.bins, T), a.neighbors))

    arms = []
    for name, shape, arg in ops:
        x = torch.rand(shape, generator=gen)
        x = (2 * x - 1 if name in bc.SIGNED or name == "unfold" else 0.05 + x).to(dev)
        oshape = (shape[0], shape[2], shape[1], 2 * arg + 1, shape[3]) if name == "unfold" else shape
        cot = (2 * torch.rand(oshape, generator=gen) - 1).to(dev)
        y, gx = torch.empty(oshape, device=dev), torch.empty(shape, device=dev)
        n_in, n_out = x.numel(), cot.numel()
        if name == "unfold":
            B, Cc, F, Tn = shape
            moved = 2 * (n_in + n_out) * 4

            def abi(x=x, cot=cot, y=y, gx=gx, g=(B, Cc, F, Tn, arg)):
                assert L_.sefd_unfold_forward(vp(x), *g, vp(y), stream) == 0 and L_.sefd_unfold_backward(vp(cot), *g, vp(gx), stream) == 0
        else:
            kind = bc.KIND[name]
            geo = _bm_geometry(kind, shape)
            ws = torch.empty(L_.sefd_norm_ws_floats(kind, *geo), device=dev)
            moved = (3 + 5 + (1 if name in bc.SIGNED else 0)) * n_in * 4
            sl = arg or 1

            def abi(x=x, cot=cot, y=y, gx=gx, kind=kind, geo=geo, ws=ws, sl=sl):
                assert L_.sefd_norm_forward(kind, vp(x), *geo, sl, vp(ws), vp(y), stream) == 0
                assert L_.sefd_norm_backward(kind, vp(x), vp(cot), *geo, sl, vp(ws), vp(gx), stream) == 0

        def module(ns, name=name, arg=arg, x=x, cot=cot):
            xr = x.detach().requires_grad_(True)
            f = getattr(ns, name)
            out = f(xr) if arg is None else f(xr, arg)
            out.backward(cot)
            return out, xr.grad

        arms.append(dict(name=name, shape=shape, arg=arg, moved=moved, vec16=shape[-1] % 4 == 0,
                         fns=dict(hip=lambda m=module: m(BaseModel), abi=abi, torch=lambda m=module: m(bc.Ref)), ms=dict(hip=[], abi=[], torch=[])))
        # the arms compute the same thing (float32 against float32: the golden tests hold the kernels to float64)
        (y1, g1), (y2, g2) = module(BaseModel), module(bc.Ref)
        arms[-1]["max_rel_diff"] = dict(y=bc.rel_err(y1.detach(), y2.detach()), grad_x=bc.rel_err(g1, g2))

    for i in range(a.warmup + a.runs):
        for r in arms:
            for arm in ("hip", "abi", "torch"):
                r["fns"][arm]()                      # untimed: the sample does not inherit the state the previous arm left (allocator, clocks)
                torch.cuda.synchronize()
                ms = timed(r["fns"][arm])
                if i >= a.warmup:
                    r["ms"][arm].append(ms)

    rec = dict(device=torch.cuda.get_device_name(0), dtype="fp32", warmup=a.warmup, runs=a.runs, timing="device events around forward + backward; median",
               streaming_copy=dict(bytes=2 * (128 << 20) * 4, ms_median=round(statistics.median(copy_ms), 5), TBs=round(copy_tbs, 3)),
               unmeasured=["kernel-by-kernel times (no profiler run)", "the reference's own CPU time for these functions", "shapes other than the ones listed",
                           "float16 / bfloat16 inputs (not supported)"], ops=[])
    for r in arms:
        med = {k: statistics.median(v) for k, v in r["ms"].items()}
        tbs = r["moved"] / (med["abi"] * 1e-3) / 1e12
        rec["ops"].append(dict(op=r["name"], shape=list(r["shape"]), arg=r["arg"], path="16-byte" if r["vec16"] else "element",
                               hip_ms=round(med["hip"], 5), abi_ms=round(med["abi"], 5), torch_ms=round(med["torch"], 5),
                               hip_ms_min=round(min(r["ms"]["hip"]), 5), abi_ms_min=round(min(r["ms"]["abi"]), 5), torch_ms_min=round(min(r["ms"]["torch"]), 5),
                               torch_over_hip=round(med["torch"] / med["hip"], 2), bytes_moved=r["moved"], abi_TBs=round(tbs, 3),
                               of_streaming_copy=round(tbs / copy_tbs, 3), max_rel_diff_vs_torch=r["max_rel_diff"]))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
