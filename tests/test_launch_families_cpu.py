"""The kernel family of every conv GEMM launch (csrc/rungemm.hip choose_rungemm / choose_wgrad through Plan.op_info()["family"]), without a GPU.

* test_every_launch_keeps_its_family: tests/golden/launch_families.json is the family of every RUNGEMM and WGRAD op of 179 plans, recorded at the last
  commit that wrote the launch chain and the reported family as two hand-kept copies (tests/golden/make_launch_families.py: the plans and the knobs).  The
  table is derived again here and must equal the file entry by entry: a refactor of the selection moves no launch.
* test_every_form_row_reports_its_family: the frame-staged files and the persistent kernel keep one table of instantiated forms each (kMaskRows,
  kStageRows, kThinWgRows, kPersistRows).  ROWS below lists every row by what identifies it; the two small plans of the GPU tests of those kernels
  must hold, for every row, a descriptor that is reported with the row's family under the family's knob at 2 - and with the family it had before under
  the knob at 0.  "Before" follows from the rest of the chain at these sizes, not from a recording: every launch here has fewer rows than DIRECT_MINM
  (65536) and fewer tiles than two resident grids, so a RUNGEMM falls to the tiled kernel; a weight gradient to the LDS-DMA kernel of its wgrad_tn.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_launch_families as mlf  # noqa: E402

import exact_data as ed  # noqa: E402
from test_gpu_rungemm_persist import _make_plan  # noqa: E402
from util import knobs  # noqa: E402


def test_every_launch_keeps_its_family():
    with open(mlf.PATH) as f:
        want = json.load(f)
    seen = []
    for plan, got in mlf.launch_family_plans():
        seen.append(plan)
        assert plan in want, f"{plan}: not in the recorded table"
        assert len(got) == len(want[plan]), f"{plan}: {len(got)} RUNGEMM / WGRAD ops, {len(want[plan])} recorded"
        for (phase, op, tag, fam), (wphase, wop, wtag, wfam) in zip(got, want[plan]):
            assert (phase, op, tag) == (wphase, wop, wtag), f"{plan}: op ({phase}, {op}, tag {tag}) where ({wphase}, {wop}, tag {wtag}) was recorded: the planner moved"
            assert fam == wfam, f"plan {plan} phase {phase} op {op} tag {tag}: family {fam}, recorded {wfam}"
    assert seen == list(want), "the plans of the recorded table, in its order"


RUN, WG = ed.KIND_RUNGEMM, ed.KIND_WGRAD
CASES = [("DCCRN", 3, 4000, "E", (16, 32, 32, 64, 64, 64), 128, "bf16"),
         ("DCCRN", 1, 2400, "C", (32, 64, 128, 256, 256, 256), 256, "bf16")]
# knob -> (op kind, family, the rows of the family's table by row_key())
ROWS = {
    "THIN_MASK": (RUN, 6, [("fwd", 32), ("fwd", 16), ("dgrad", 4), ("dgrad", 2)]),                                       # thin_mask.hip kMaskRows
    "THIN_STAGE": (RUN, 7, [("pm", 64, 2), ("pm", 64, 1), ("pm", 32, 2), ("pm", 32, 1),
                            ("st", 32, 2, 64), ("st", 32, 4, 64), ("st", 16, 1, 64), ("st", 16, 2, 64)]),               # thin_stage.hip kStageRows
    "THIN_STAGE64": (RUN, 8, [("st", 64, 4, 32)]),                                                                       # ... its last row
    "THIN_WGRAD": (WG, 13, [(32, 64), (16, 32), (8, 32)]),                                                               # thin_wgrad.hip kThinWgRows
    "RG_PERSIST": (RUN, 5, [128, 64, 32]),                                                                               # rungemm_persist.hip kPersistRows
}
TILED = 4                                                          # sefd_amd.plan RUN_FAMILY_TILED
WG_DMA = {128: 7, 64: 8, 32: 9}                                    # sefd_amd.plan WG_FAMILY_DMA128 / 64 / 32


def row_key(knob, g):
    """What identifies the form-table row of descriptor `g`, from its fields alone."""
    if knob == "THIN_MASK":
        return ("fwd", g.fstride[0]) if g.x[1].arena >= 0 else ("dgrad", g.N // 16)
    if knob in ("THIN_STAGE", "THIN_STAGE64"):
        if g.seg[0].len == 3 * g.fstride[0]:                       # runs of 3 positions: phase-merged; of 5 positions of two per output position: strided
            return "pm", g.fstride[0], 2 if g.x[1].arena >= 0 else 1
        return "st", g.fstride[0] // 2, g.N // 32, g.Fo
    if knob == "THIN_WGRAD":
        return g.fstride[0] // 2, g.N
    return 128 if g.N > 64 else 64 if g.N > 32 else 32             # sefd_desc.h bn_of


def before(kind, g):
    if kind == RUN:
        return TILED
    return WG_DMA[128 if g.Npad >= 128 else 64 if g.N > 32 else 32]     # sefd_desc.h wgrad_tn of an aligned bf16 descriptor


@pytest.mark.parametrize("knob", list(ROWS))
def test_every_form_row_reports_its_family(knob):
    kind, family, rows = ROWS[knob]
    reached = {}
    for case in CASES:
        plan = _make_plan(case)
        ops = [(phase, i) for phase in (0, 1) for i in range(plan.num_ops(phase)) if plan.op_info(phase, i)["kind"] == kind]
        knobs.set(knob, "2")
        on = {(phase, i): plan.op_info(phase, i)["family"] for phase, i in ops}
        knobs.set(knob, "0")
        off = {(phase, i): plan.op_info(phase, i)["family"] for phase, i in ops}
        knobs.unset(knob)
        for phase, i in ops:
            g = ed.gemm(plan, i, phase)
            where = f"{case[4]} phase {phase} op {i} tag {plan.op_info(phase, i)['tag']}"
            if on[phase, i] != family:
                assert off[phase, i] == on[phase, i], f"{where}: {knob} moves a launch that its family does not take"
                continue
            key = row_key(knob, g)
            assert key in rows, f"{where}: family {family} reported for {key}, which is no row of its table"
            assert off[phase, i] == before(kind, g), f"{where}: row {key} under {knob}=0: family {off[phase, i]}, before it had {before(kind, g)}"
            reached.setdefault(key, where)
    assert sorted(reached, key=str) == sorted(rows, key=str), f"rows without a descriptor: {[r for r in rows if r not in reached]}"
