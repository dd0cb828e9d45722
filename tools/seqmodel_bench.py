"""Forward + backward time of a stand-alone SequenceModel, cluster recurrences against the stepped formulation (knob LSTM_STEPPED), same process.

    python tools/seqmodel_bench.py [--out profiles/seqmodel_bench.json]

SequenceModel(257, 257, 512, 2, bidirectional, "LSTM") at B = 32, T = 200 in bf16: device events around forward + loss + backward, 5 warm-ups, then
20 timed runs per arm with the two arms alternating; the median per arm is reported.  There is no reference time: the commit before this model id
cannot run it."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqmodel_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models, tuning
    from oracle.weights import fill_state_dict_

    cfg.act_dtype = "bf16"
    arms = {}
    for arm in ("cluster", "stepped"):                       # one model per arm: a plan is a function of the knob table when it is built
        tuning.clear()
        if arm == "stepped":
            tuning.set("LSTM_STEPPED", "1")
        m = models.SequenceModel(257, 257, a.hidden, a.layers, True, "LSTM", None)
        fill_state_dict_(m)
        m = m.cuda().train()
        gen = torch.Generator().manual_seed(1)
        x = (3 * torch.rand(a.batch, 257, a.frames, generator=gen)).cuda().requires_grad_(True)
        tgt = torch.rand(a.batch, 257, a.frames, generator=gen).cuda()
        ((m(x) - tgt) ** 2).mean().backward()                # builds the plan under this arm's knobs
        plan = next(v for k, v in m._runtimes.items() if k[0] == "seq")[0]
        kinds = [plan.op_kinds(ph)[0] for ph in (0, 1)]
        arms[arm] = dict(model=m, x=x, tgt=tgt, ms=[], lstm_launches=[int((kinds[0] == 9).sum()), int((kinds[1] == 10).sum())],
                         ops=[int(len(kinds[0])), int(len(kinds[1]))])
    tuning.clear()
    cfg.act_dtype = "fp32"

    def run(arm):
        r = arms[arm]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r["model"].zero_grad()
        r["x"].grad = None
        e0.record()
        ((r["model"](r["x"]) - r["tgt"]) ** 2).mean().backward()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        for arm in arms:
            run(arm)
    for _ in range(a.runs):
        for arm in arms:
            arms[arm]["ms"].append(run(arm))
    rec = dict(model=f"SequenceModel(257, 257, {a.hidden}, {a.layers}, True, 'LSTM')", B=a.batch, T=a.frames, dtype="bf16", warmup=a.warmup, runs=a.runs,
               device=torch.cuda.get_device_name(0),
               arms={k: dict(fwd_bwd_ms_median=statistics.median(v["ms"]), fwd_bwd_ms_min=min(v["ms"]), fwd_bwd_ms_max=max(v["ms"]),
                             lstm_launches_fwd_bwd=v["lstm_launches"], ops_fwd_bwd=v["ops"]) for k, v in arms.items()})
    rec["stepped_over_cluster"] = rec["arms"]["stepped"]["fwd_bwd_ms_median"] / rec["arms"]["cluster"]["fwd_bwd_ms_median"]
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
