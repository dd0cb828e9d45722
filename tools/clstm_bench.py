"""Forward + backward time of a stand-alone NavieComplexLSTM: one direction, two directions with the reverse recurrence on the second stream, the same
plan with every launch in program order on one stream (knob NO_OVERLAP, read per run), and the stepped formulation (knob LSTM_STEPPED), same process.

    python tools/clstm_bench.py [--out profiles/clstm_bench.json]

NavieComplexLSTM(1024, 256, projection_dim=1024) - DCCRN's last recurrent layer - at B = 32, T = 483 in bf16: device events around forward + loss +
backward, 5 warm-ups, then 20 timed runs per arm with the arms alternating; the median per arm is reported.  There is no reference time: the commit
before this model id cannot run the module."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clstm_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=483)
    ap.add_argument("--input", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--projection", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models, tuning
    from oracle.weights import fill_state_dict_

    cfg.act_dtype = "bf16"
    # arm: (bidirectional, knobs while the plan is built, knobs while it runs)
    spec = {"uni": (False, {}, {}), "bi_two_streams": (True, {}, {}), "bi_one_stream": (True, {}, {"NO_OVERLAP": "1"}),
            "bi_stepped": (True, {"LSTM_STEPPED": "1"}, {})}
    arms = {}
    for arm, (bi, build_knobs, run_knobs) in spec.items():   # one module per arm: a plan is a function of the knob table when it is built
        tuning.clear()
        for k, v in build_knobs.items():
            tuning.set(k, v)
        m = models.NavieComplexLSTM(a.input, a.hidden, projection_dim=a.projection, bidirectional=bi)
        fill_state_dict_(m)
        m = m.cuda().train()
        gen = torch.Generator().manual_seed(1)
        xs = [(2 * torch.rand(a.frames, a.batch, a.input // 2, generator=gen) - 1).cuda().requires_grad_(True) for _ in range(2)]
        gs = [(2 * torch.rand(a.frames, a.batch, a.projection // 2, generator=gen) - 1).cuda() for _ in range(2)]
        arms[arm] = dict(model=m, xs=xs, gs=gs, ms=[], run_knobs=run_knobs)
        run(arms[arm], tuning)                               # builds the plan under this arm's knobs
        plan = next(v for k, v in m._runtimes.items() if k[0] == "clstm")[0]
        kinds = [plan.op_kinds(ph)[0] for ph in (0, 1)]
        arms[arm].update(lstm_launches=[int((kinds[0] == 9).sum()), int((kinds[1] == 10).sum())], ops=[int(len(kinds[0])), int(len(kinds[1]))])
    tuning.clear()
    cfg.act_dtype = "fp32"

    for _ in range(a.warmup):
        for r in arms.values():
            run(r, tuning)
    for _ in range(a.runs):
        for r in arms.values():
            r["ms"].append(run(r, tuning))
    rec = dict(model=f"NavieComplexLSTM({a.input}, {a.hidden}, projection_dim={a.projection})", B=a.batch, T=a.frames, dtype="bf16", warmup=a.warmup,
               runs=a.runs, device=torch.cuda.get_device_name(0),
               arms={k: dict(fwd_bwd_ms_median=statistics.median(v["ms"]), fwd_bwd_ms_min=min(v["ms"]), fwd_bwd_ms_max=max(v["ms"]),
                             lstm_launches_fwd_bwd=v["lstm_launches"], ops_fwd_bwd=v["ops"]) for k, v in arms.items()})
    med = lambda k: rec["arms"][k]["fwd_bwd_ms_median"]
    rec["one_stream_over_two_streams"] = med("bi_one_stream") / med("bi_two_streams")
    rec["bi_over_uni"] = med("bi_two_streams") / med("uni")
    rec["stepped_over_two_streams"] = med("bi_stepped") / med("bi_two_streams")
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


def run(r, tuning):
    for k, v in r["run_knobs"].items():
        tuning.set(k, v)
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r["model"].zero_grad()
        for x in r["xs"]:
            x.grad = None
        e0.record()
        out = r["model"](r["xs"])
        ((out[0] * r["gs"][0]).mean() + (out[1] * r["gs"][1]).mean()).backward()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    finally:
        tuning.unset(*r["run_knobs"])


if __name__ == "__main__":
    main()
