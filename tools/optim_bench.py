"""Times the optimizer kernels on device buffers at the flat parameter counts of the stock DCCRN and FullSubNet.

Arms (HIP events around LAUNCHES back-to-back launches, the arms alternating inside every round, (a) twice per round):
  a  sefd_adam_step                      the kernel every default training step ends with: the yardstick          28 B / element
  b  sefd_optim_step, one group, no options, over the chunk table                                                28 B / element
  c  sefd_optim_step, the two get_params groups (weights with L2 decay, biases without), amsgrad                   36 B / element
  d  sefd_grad_norm (partial sums + finalize)                                                                      4 B / element
Every launch works on the next of SETS buffer sets, which together exceed the 256 MiB last-level cache: the rates are HBM rates, as in a training
step, where the optimizer's buffers were last touched a whole step ago.  (b)'s margin is the spread of the two (a) arms.

    python tools/optim_bench.py [--out profiles/optim_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sefd_amd  # noqa: E402,F401
from sefd_amd import _lib, models  # noqa: E402
from sefd_amd.optim import _Group, chunk_table, table_to_device  # noqa: E402

LAUNCHES, ROUNDS, WARMUP = 40, 25, 3
CACHE_BYTES = 256 << 20
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def segments(model):
    """(begin, count, is_bias) of every parameter in flat order: the two groups of get_params."""
    out, off = [], 0
    for name, p in model.named_parameters():
        out.append((off, p.numel(), 1 if "bias" in name else 0))
        off += p.numel()
    return out, off


def bench(name, model):
    L = _lib.lib()
    segs, n = segments(model)
    sets = max(2, -(-2 * CACHE_BYTES // (n * 16)))
    gen = torch.Generator(device="cuda").manual_seed(3)
    bufs = [dict(p=torch.randn(n, device="cuda", generator=gen), g=torch.randn(n, device="cuda", generator=gen) * 1e-2,
                 m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"), x=torch.zeros(n, device="cuda")) for _ in range(sets)]
    one = chunk_table([(b, c, 0) for b, c, _ in segs])
    two = chunk_table(segs)
    one_d, two_d = table_to_device(one), table_to_device(two)
    h_one, h_two = (_Group * 8)(), (_Group * 8)()
    h_one[0] = _Group(LR, B1, B2, EPS, 0.0, 0)
    h_two[0], h_two[1] = _Group(LR, B1, B2, EPS, 1e-5, 2), _Group(LR, B1, B2, EPS, 0.0, 2)
    ws = torch.zeros(L.sefd_grad_norm_ws_floats(n) // 2, dtype=torch.float64, device="cuda")
    out = torch.zeros(2, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    step = [0]

    def arm_a(b):
        return L.sefd_adam_step(vp(b["p"]), vp(b["g"]), vp(b["m"]), vp(b["v"]), n, step[0], LR, B1, B2, EPS, 1.0, stream)

    def arm_b(b):
        return L.sefd_optim_step(vp(b["p"]), vp(b["g"]), vp(b["m"]), vp(b["v"]), None, n, step[0], h_one, 1, C.c_void_p(one.ctypes.data), vp(one_d),
                                 len(one), 1.0, None, None, None, stream)

    def arm_c(b):
        return L.sefd_optim_step(vp(b["p"]), vp(b["g"]), vp(b["m"]), vp(b["v"]), vp(b["x"]), n, step[0], h_two, 2, C.c_void_p(two.ctypes.data), vp(two_d),
                                 len(two), 1.0, None, None, None, stream)

    def arm_d(b):
        return L.sefd_grad_norm(vp(b["g"]), n, 1.0, 1.0, None, None, 0, vp(ws), vp(out), stream)

    order = [("a", arm_a), ("b", arm_b), ("a2", arm_a), ("c", arm_c), ("d", arm_d)]
    times = {k: [] for k, _ in order}
    for rnd in range(WARMUP + ROUNDS):
        for key, fn in order:
            step[0] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(LAUNCHES):
                rc = fn(bufs[i % sets])
                if rc != 0:
                    raise RuntimeError(f"arm {key} failed ({rc})")
            e1.record()
            e1.synchronize()
            if rnd >= WARMUP:
                times[key].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    per_elem = {"a": 28, "b": 28, "a2": 28, "c": 36, "d": 4}
    res = {"model": name, "elements": n, "parameter_tensors": len(segs), "chunks_one_group": len(one), "chunks_two_groups": len(two), "buffer_sets": sets,
           "arms": {}}
    for key, _ in order:
        t = times[key]
        med = statistics.median(t)
        res["arms"][key] = {"us_median": round(med, 3), "us_min": round(min(t), 3), "us_max": round(max(t), 3), "bytes_per_element": per_elem[key],
                            "TB_per_s": round(per_elem[key] * n / med / 1e6, 3)}
    pooled = sorted(times["a"] + times["a2"])                   # (b)'s margin: where the repeated (a) samples of this very run fall
    lo, hi = pooled[len(pooled) // 10], pooled[-1 - len(pooled) // 10]
    b = res["arms"]["b"]["us_median"]
    res["a_p10_p90_us"] = [round(lo, 3), round(hi, 3)]
    res["a_medians_differ_us"] = round(abs(res["arms"]["a"]["us_median"] - res["arms"]["a2"]["us_median"]), 3)
    res["b_minus_a_us"] = round(b - statistics.median(pooled), 3)
    res["b_within_a_spread"] = bool(lo <= b <= hi)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs the GPU: a CPU run says nothing about these kernels")
    results = [bench("DCCRN", models.DCCRN()), bench("FullSubNet", models.FullSubNet())]
    doc = {"device": torch.cuda.get_device_name(0), "launches_per_sample": LAUNCHES, "rounds": ROUNDS,
           "timing": "HIP events around back-to-back launches; us per launch; every launch on the next of buffer_sets buffer sets (together beyond the "
                     "256 MiB last-level cache)", "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
