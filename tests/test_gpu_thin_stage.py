"""The frame-staged kernels of the thin layers next to the mask layer (csrc/thin_stage.hip; knobs THIN_STAGE / THIN_STAGE_GRID, read per launch).  Phase-merged
form: the second-to-last decoder layer's forward conv (tag 404, phase 0: two sources, BatchNorm statistics rows in the epilogue) and the second encoder
layer's input gradient (tag 101, phase 1: one source, frames u + 1 and u).  Strided form: the second encoder layer's forward conv (tag 101, phase 0:
statistics rows) and the decoder layer's input gradient (tag 404, phase 1: two destinations).

* which launches take the kernel is asserted through Plan.op_info()["family"], without a GPU: none with the knob off, none of these small plans under the
  default rule (it has a row threshold), exactly the four launches above with THIN_STAGE=2 - by tag, phase, N and K -, none in the fp32 twin or with the
  DCCRN-large channel counts, none in a CRN plan but the one forward conv whose descriptor IS DCCRN's, and THIN_MASK does not switch them.  A case whose channel counts the kernel does not instantiate fails
  here: it does not pass with nothing taken;
* every launch of two small DCCRN plans against the host simulator with the four launches on the new kernels, at grid 1 (ONE workgroup walks every frame:
  the LDS ring carries over every batch boundary), grid 3 (uneven runs, still whole statistics rows) and the resident grid.  The simulator's tolerances
  are the bar;
* forward + backward with the kernels off and on, at grids 1, 3 and 0: every byte the phases write is equal - outputs and statistics partial rows keep the
  bits of the kernels replaced (the statistics epilogue sums in their order), so a training run computes what it computed;
* forward + backward at grids 1, 3, 0 and 0 again: every plan buffer - the statistics partial rows among them - and the A_GRAD, A_STATE, A_IO and A_WS
  arenas are bit-equal across the four runs: a second writer, a run that cuts a statistics row in two or a ring slot read too early shows here.

The cases: B = 3, L = 4000, kernel_num (16, 32, 32, 64, 64, 64) - 32 channels per source (two column tiles, two waves share one: the statistics meet
in LDS), 41 / 42 frames per item that no workgroup run divides, 123 encoder frames; B = 1, L = 2400, kernel_num (32, 64, 128, 256, 256, 256) - the
benchmark's 64 channels per source (four column tiles), bins 0 and Fo - 1 of the frequency axis."""
import pytest
import torch

from test_gpu_rungemm_persist import _make_plan, _run_both_phases
from util import knobs

CASES = [("DCCRN", 3, 4000, "E", (16, 32, 32, 64, 64, 64), 128, "bf16"),
         ("DCCRN", 1, 2400, "C", (32, 64, 128, 256, 256, 256), 256, "bf16")]
GRIDS = [1, 3, 0]
KIND_RUNGEMM = 1
MASK_TAG = 405


def _rungemm_ops(plan):
    return [(phase, i, plan.op_info(phase, i)) for phase in (0, 1) for i in range(plan.num_ops(phase))
            if plan.op_info(phase, i)["kind"] == KIND_RUNGEMM]


def _taken(plan, family=None):
    """{(phase, op)} of the RUNGEMM ops that a launch would put on the frame-staged kernel under the knobs of the moment."""
    from sefd_amd.plan import RUN_FAMILY_THIN_STAGE
    family = RUN_FAMILY_THIN_STAGE if family is None else family
    return {(phase, i) for phase, i, o in _rungemm_ops(plan) if o["family"] == family}


def _expected(case):
    """(tag, phase, N, K) of the launches built.  Phase-merged form: dec4 forward (2 sources x 2 frames x 3 positions x kernel_num[1] channels,
    [phase][kernel_num[0]] columns) and enc1 input gradient (2 frames x 3 positions x kernel_num[1] channels).  Strided form: enc1 forward (2 frames x
    5 positions x kernel_num[0] channels) and dec4 input gradient (the same runs of dy, both sources' kernel_num[1] columns)."""
    kn = case[4]
    return [(404, 0, 2 * kn[0], 2 * 2 * 3 * kn[1]), (101, 1, 2 * kn[0], 2 * 3 * kn[1]),
            (101, 0, kn[1], 2 * 5 * kn[0]), (404, 1, 2 * kn[1], 2 * 5 * kn[0])]


def _assert_exactly_the_built_launches(plan, case):
    want = set()
    for tag, phase, N, K in _expected(case):
        hit = [(p, i) for p, i, o in _rungemm_ops(plan) if (o["tag"], p, o["N"], o["K"]) == (tag, phase, N, K)]
        assert len(hit) == 1, (tag, phase, N, K, hit)
        want.add(hit[0])
    assert _taken(plan) == want, (sorted(_taken(plan)), sorted(want))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_selection_rule(case):
    """No GPU: the planner and the selection rule alone."""
    from sefd_amd.plan import RUN_FAMILY_THIN_MASK
    plan = _make_plan(case)
    knobs.set("THIN_STAGE", "0")
    assert _taken(plan) == set()
    knobs.unset("THIN_STAGE")
    assert _taken(plan) == set()                       # default rule: these plans are below its row threshold
    knobs.set("THIN_MASK", "2")
    assert _taken(plan) == set()                       # the mask layer's knob does not switch this kernel
    knobs.unset("THIN_MASK")
    knobs.set("THIN_STAGE", "2")
    for grid in GRIDS:
        knobs.set("THIN_STAGE_GRID", str(grid))
        _assert_exactly_the_built_launches(plan, case)
    knobs.unset("THIN_STAGE_GRID")
    assert _taken(_make_plan(case[:6] + ("fp32",))) == set()
    # CRN: its input gradients are one launch per destination and stay.  Its second encoder layer's forward conv at kernel_num[0] = 32 is, field for
    # field, the descriptor of DCCRN's at kernel_num[0] = 16 (the same planner function: 16 input channels, N = 32, statistics rows): a form check
    # cannot tell the two apart, so that ONE launch is taken and nothing else; at kernel_num[0] = 16 (8 input channels: not built) nothing is
    assert _taken(_make_plan(("CRN",) + CASES[0][1:])) == set()
    crn = _make_plan(("CRN",) + CASES[1][1:])
    assert [(p, crn.op_info(p, i)["tag"], crn.op_info(p, i)["N"], crn.op_info(p, i)["K"]) for p, i in sorted(_taken(crn))] == [(0, 101, 32, 160)]
    assert _taken(_make_plan(("DCCRN", 1, 2400, "C", (64, 128, 256, 512, 512, 512), 512, "bf16"))) == set()
    knobs.set("THIN_MASK", "2")
    knobs.set("THIN_STAGE", "0")
    assert _taken(plan) == set()
    mask = _taken(plan, RUN_FAMILY_THIN_MASK)
    assert len(mask) == 2 and all(plan.op_info(p, i)["tag"] == MASK_TAG for p, i in mask), sorted(mask)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_every_op_against_host_simulator_thin_stage(case, grid):
    from test_gpu_ops import every_op_against_host_simulator
    knobs.set("THIN_STAGE", "2")
    knobs.set("THIN_STAGE_GRID", str(grid))
    _assert_exactly_the_built_launches(_make_plan(case), case)
    every_op_against_host_simulator(*case, report_prefix=f"ops_report_thin_stage_g{grid}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_grids_and_runs_are_bit_equal(case):
    plan = _make_plan(case)
    knobs.set("THIN_STAGE", "2")
    runs = []
    for grid in GRIDS + [0]:
        knobs.set("THIN_STAGE_GRID", str(grid))
        _assert_exactly_the_built_launches(plan, case)
        runs.append(_run_both_phases(case, plan))
    first, diff = runs[0], []
    for k, other in enumerate(runs[1:], 1):
        for name in plan.buffer_names():
            a, off, nb, _ = plan.buffer(name)
            if nb > 0 and not torch.equal(first[a].view(torch.uint8)[off:off + nb], other[a].view(torch.uint8)[off:off + nb]):
                diff.append(f"run{k}:{name}")
        for a, name in ((2, "A_GRAD"), (3, "A_STATE"), (5, "A_IO"), (0, "A_WS")):
            if not torch.equal(first[a].view(torch.uint8), other[a].view(torch.uint8)):
                diff.append(f"run{k}:{name}")
    assert not diff, "buffers that differ from the grid-1 run: " + " ".join(diff)


_reference = {}


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_bit_identical_to_the_kernels_replaced(case, grid):
    """The outputs AND the statistics partial rows keep the bits of the kernels replaced: the statistics epilogue walks a 128-row block in their order
    (four groups of 32 rows, two chains per column and group, groups added in ascending order), so a training run computes what it computed."""
    plan = _make_plan(case)
    if case not in _reference:                         # the replaced kernels' result: computed once per case, never changed
        knobs.set("THIN_STAGE", "0")
        assert _taken(plan) == set()
        _reference[case] = _run_both_phases(case, plan)
    ref = _reference[case]
    knobs.set("THIN_STAGE", "2")
    knobs.set("THIN_STAGE_GRID", str(grid))
    _assert_exactly_the_built_launches(plan, case)
    got = _run_both_phases(case, plan)
    diff = []
    for name in plan.buffer_names():
        a, off, nb, _ = plan.buffer(name)
        if nb > 0 and not torch.equal(ref[a].view(torch.uint8)[off:off + nb], got[a].view(torch.uint8)[off:off + nb]):
            diff.append(name)
    for a, name in ((2, "A_GRAD"), (3, "A_STATE"), (5, "A_IO"), (0, "A_WS")):
        if not torch.equal(ref[a].view(torch.uint8), got[a].view(torch.uint8)):
            diff.append(name)
    assert not diff, "buffers that differ from the kernels replaced: " + " ".join(diff)
