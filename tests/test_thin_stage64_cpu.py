"""Which launches take the strided frame-staged kernel at 64 channels and 128 columns (csrc/thin_stage.hip, thin_stage_st_kernel<64, 4, 32>; knobs
THIN_STAGE64 / THIN_STAGE64_GRID, read per launch), asserted through Plan.op_info()["family"] without a GPU: the planner and the selection rule alone.

The form: one source of 64 channels per input position, 64 input positions per frame, two runs of 5 positions from position 2 f - 2, N = 128 = Npad,
K = 640, Fo = 32, bf16 in and out, no flag but the two alignment flags; bias + statistics rows (the third encoder layer's forward conv, tag 102) or neither
(the third-to-last decoder layer's input gradients, tag 403: one launch per destination).

* nothing with the knob 0; nothing in these small plans under the default rule (it has a row threshold); with THIN_STAGE64=2 exactly the three launches, by
  (tag, phase, N, K), at every forced grid; nothing in the fp32 twin or with the DCCRN-large channel counts (N = 256 at tag 102); THIN_STAGE and THIN_MASK
  do not switch the kernel, and THIN_STAGE64 does not switch theirs;
* CRN: its real conv stack carries kernel_num[k] / 2 channels where DCCRN's carries kernel_num[k] (real and imaginary halves).  With kernel_num
  (64, 128, 256, ...) its third encoder layer reads 64 channels and writes 128 columns over Fo = 32: field for field the descriptor of DCCRN's at
  (32, 64, 128, ...) - a form check cannot tell the two apart, and must not - and its decoder's input gradients are, like DCCRN's here, one launch per
  destination with the same runs.  So the same three launches are taken, by the same key, and nothing else; at every other channel count tried nothing is.
"""
import pytest

from test_gpu_rungemm_persist import _make_plan
from util import knobs

CASES = [("DCCRN", 1, 2400, "C", (32, 64, 128, 256, 256, 256), 256, "bf16"),
         ("DCCRN", 3, 4000, "E", (32, 64, 128, 128, 128, 128), 128, "bf16")]
GRIDS = [1, 3, 0]
KIND_RUNGEMM = 1
EXPECTED = [(102, 0, 128, 640), (403, 1, 128, 640), (403, 1, 128, 640)]       # (tag, phase, N, K): enc2 forward, dec3's two input gradients


def rungemm_ops(plan):
    return [(phase, i, plan.op_info(phase, i)) for phase in (0, 1) for i in range(plan.num_ops(phase))
            if plan.op_info(phase, i)["kind"] == KIND_RUNGEMM]


def taken(plan, family=None):
    """{(phase, op)} of the RUNGEMM ops that a launch would put on the kernel under the knobs of the moment."""
    from sefd_amd.plan import RUNGEMM_FAMILY_THIN_STAGE64
    family = RUNGEMM_FAMILY_THIN_STAGE64 if family is None else family
    return {(phase, i) for phase, i, o in rungemm_ops(plan) if o["family"] == family}


def assert_exactly_the_three_launches(plan, expected=EXPECTED):
    got = sorted((plan.op_info(p, i)["tag"], p, plan.op_info(p, i)["N"], plan.op_info(p, i)["K"]) for p, i in taken(plan))
    assert got == sorted(expected), got
    # ... and they are every op of the plan with such a key: no launch of the form stays behind
    assert len([1 for p, i, o in rungemm_ops(plan) if (o["tag"], p, o["N"], o["K"]) in expected]) == len(expected)


def test_family_name_stays_out_of_the_shape_reached_list():
    import sefd_amd.plan as sp
    assert sp.RUNGEMM_FAMILY_THIN_STAGE64 == 8 and sp.RUNGEMM_FAMILY_THIN_STAGE64 in sp.RUNGEMM_FAMILY_MORE_NAMES
    assert not [k for k, v in vars(sp).items() if k.startswith("RUN_FAMILY_") and v == 8]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_selection_rule(case):
    from sefd_amd.plan import RUN_FAMILY_THIN_MASK, RUN_FAMILY_THIN_STAGE
    plan = _make_plan(case)
    knobs.set("THIN_STAGE64", "0")
    assert taken(plan) == set()
    knobs.unset("THIN_STAGE64")
    assert taken(plan) == set()                        # default rule: these plans are below its row threshold
    knobs.set("THIN_STAGE64", "1")
    assert taken(plan) == set()
    for other in ("THIN_STAGE", "THIN_MASK"):          # the other frame-staged kernels' knobs do not switch this one
        knobs.unset("THIN_STAGE64")
        knobs.set(other, "2")
        assert taken(plan) == set()
        knobs.set("THIN_STAGE64", "0")
        assert taken(plan) == set()
        knobs.unset(other)
    knobs.set("THIN_STAGE64", "2")
    stage, mask = taken(plan, RUN_FAMILY_THIN_STAGE), taken(plan, RUN_FAMILY_THIN_MASK)
    for grid in GRIDS:
        knobs.set("THIN_STAGE64_GRID", str(grid))
        assert_exactly_the_three_launches(plan)
    knobs.unset("THIN_STAGE64_GRID")
    knobs.set("THIN_STAGE", "2")                       # ... nor does this one's knob switch theirs, and theirs take none of the three
    knobs.set("THIN_MASK", "2")
    assert_exactly_the_three_launches(plan)
    knobs.set("THIN_STAGE64", "0")
    stage2, mask2 = taken(plan, RUN_FAMILY_THIN_STAGE), taken(plan, RUN_FAMILY_THIN_MASK)
    knobs.set("THIN_STAGE64", "2")
    assert taken(plan, RUN_FAMILY_THIN_STAGE) == stage2 and taken(plan, RUN_FAMILY_THIN_MASK) == mask2 and len(stage2) == 4 and len(mask2) == 2
    assert stage == set() and mask == set()
    knobs.unset("THIN_STAGE")
    knobs.unset("THIN_MASK")
    assert taken(_make_plan(case[:6] + ("fp32",))) == set()
    assert taken(_make_plan(("DCCRN", 1, 2400, "C", (64, 128, 256, 512, 512, 512), 512, "bf16"))) == set()


def test_default_rule_takes_the_benchmark_launches():
    """The benchmark's plan (B = 32, L = 48000) is above the row threshold: the three launches are taken with no knob set."""
    knobs.unset("THIN_STAGE64")
    plan = _make_plan(("DCCRN", 32, 48000, "E", (32, 64, 128, 256, 256, 256), 256, "bf16"))
    assert_exactly_the_three_launches(plan)
    assert all(plan.op_info(p, i)["M"] == 494592 for p, i in taken(plan))


def test_crn_plans():
    """See the module docstring: the form check implies CRN's three launches at 64 channels into 128 columns, and nothing at other channel counts."""
    knobs.set("THIN_STAGE64", "2")
    for kn in ((16, 32, 32, 64, 64, 64), (32, 64, 128, 256, 256, 256), (32, 64, 128, 128, 128, 128), (64, 64, 128, 128, 128, 128)):
        assert taken(_make_plan(("CRN", 1, 2400, "C", kn, 128, "bf16"))) == set(), kn
    crn = _make_plan(("CRN", 1, 2400, "C", (64, 128, 256, 512, 512, 512), 128, "bf16"))
    assert_exactly_the_three_launches(crn)
    knobs.unset("THIN_STAGE64")
    assert taken(crn) == set()                         # (below the row threshold)
