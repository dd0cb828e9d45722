"""The kernel family of every conv GEMM launch, recorded: tests/golden/launch_families.json.

No reference and no GPU are needed: the planner and the selection rules of csrc/rungemm.hip alone (Plan.op_info()["family"]).  The file is RECORDED
OUTPUT of the commit it was generated at - the last one before the launch and the reported family became one decision (choose_rungemm / choose_wgrad) -
and tests/test_launch_families_cpu.py holds every later commit to it, entry by entry.  Generate it again only where a change MEANS to move a launch to
another family, and say so.

For each plan, every RUNGEMM and WGRAD op of both phases in op order as [phase, op, tag, family].  The plans (launch_family_plans(), shared with the test):
  exact/<case>/<arm>        every case x every arm of tests/exact_data.py (the arm's knobs stay set while the families are read)
  config/<entry>/<dtype>    the accepted configurations of tests/plan_configs.py under their own knobs
  bench                     tools/plan_fingerprint.py's bench_dccrn_bf16_C_b32_3s: the only size where the row thresholds of the default rules take launches
  bench/<KNOB>=<0 | 2>      ... under each of THIN_MASK, THIN_STAGE, THIN_STAGE64, THIN_WGRAD, RG_PERSIST off and on every launch of the form

    python tests/golden/make_launch_families.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(HERE, "launch_families.json")
KIND_RUNGEMM, KIND_WGRAD = 1, 2                                  # sefd_desc.h OpKind
BENCH = "bench_dccrn_bf16_C_b32_3s"
BENCH_KNOBS = ("THIN_MASK", "THIN_STAGE", "THIN_STAGE64", "THIN_WGRAD", "RG_PERSIST")


def families(plan):
    """[[phase, op, tag, family]] of the RUNGEMM and WGRAD ops of both phases, in op order, under the knobs of the moment."""
    out = []
    for phase in (0, 1):
        for i in range(plan.num_ops(phase)):
            o = plan.op_info(phase, i)
            if o["kind"] in (KIND_RUNGEMM, KIND_WGRAD):
                out.append([phase, i, o["tag"], o["family"]])
    return out


def launch_family_plans():
    """Yields (name, [[phase, op, tag, family]]) for every plan of the module docstring; every knob is unset again behind each."""
    import exact_data as ed
    import plan_configs as pc
    import plan_fingerprint as pf
    from sefd_amd import tuning
    from sefd_amd.plan import Plan

    for case in ed.CASES:
        for arm in ed.ARMS:
            with ed.under(case, arm) as plan:
                yield f"exact/{case.name}/{arm}", families(plan)
    ed._plans.clear()
    for e in pc.ACCEPTED:
        for dtype in e.dtypes:
            with tuning.scope(**dict(e.knobs)):
                yield f"config/{e.name}/{dtype}", families(Plan(e.B, e.L, **pc.plan_kwargs(e, dtype)))
    kw = dict(next(kw for name, kw, _ in pf.MATRIX if name == BENCH))
    bench = Plan(kw.pop("B"), kw.pop("L"), **kw)
    yield "bench", families(bench)
    for knob in BENCH_KNOBS:                                     # (read per launch: the one plan serves every arm)
        for v in ("0", "2"):
            with tuning.scope(**{knob: v}):
                yield f"bench/{knob}={v}", families(bench)


def main():
    import sefd_amd  # noqa: F401
    table = dict(launch_family_plans())
    with open(PATH, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in table.items()) + "\n}\n")
    print(f"{PATH}: {len(table)} plans, {sum(len(v) for v in table.values())} launches, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
