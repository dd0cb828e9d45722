"""The frame-staged kernels of the mask layer (csrc/thin_mask.hip; knobs THIN_MASK / THIN_MASK_GRID, read per launch): the last decoder layer's
phase-merged conv (tag 405, N = 16, no statistics) and its input gradient (K = 80, two destinations).

* which launches take the kernels is asserted through Plan.op_info()["family"], without a GPU: none with the knob off, none of these small plans under
  the default rule (it has a row threshold), exactly the two tag-405 RUNGEMM launches with THIN_MASK=2, none in the fp32 plans.  A case whose channel
  counts the kernels do not instantiate fails here: it does not pass with nothing taken;
* every launch of two small DCCRN plans against the host simulator with the two launches on the new kernels, at grid 1 (ONE workgroup walks every frame:
  the LDS ring carries over every batch boundary), grid 3 (uneven runs) and the resident grid.  The simulator's tolerances are the bar: the 16-column
  MFMA groups the sums over k differently from rungemm_kernel, so identity with the kernels replaced is not asserted;
* forward + backward twice with the kernels on: every plan buffer and the gradient, state and I/O arenas are equal between the two runs.

The cases: B = 3, L = 4000, kernel_num (16, 32, 32, 64, 64, 64) - 16 + 16 input channels (the benchmark has 32 + 32: the other instantiation), 42 frames per
item that no workgroup run divides, the first frame and the dropped lead frame of three items; B = 1, L = 2400, kernel_num (32, 64, 128, 256, 256, 256) - the
benchmark's channel counts, 64 gradient columns to two destinations, positions 0 and Fo - 1 of the frequency axis."""
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


def _taken(plan):
    """{(phase, op)} of the RUNGEMM ops that a launch would put on the frame-staged kernels under the knobs of the moment."""
    from sefd_amd.plan import RUN_FAMILY_THIN_MASK
    return {(phase, i) for phase, i, o in _rungemm_ops(plan) if o["family"] == RUN_FAMILY_THIN_MASK}


def _assert_exactly_the_mask_layer(plan, case):
    """The forward launch of the mask layer and its input gradient, and nothing else."""
    mask = [(phase, i, o) for phase, i, o in _rungemm_ops(plan) if o["tag"] == MASK_TAG]
    fwd = [(p, i) for p, i, o in mask if p == 0]
    bwd = [(p, i) for p, i, o in mask if p == 1]
    assert len(fwd) == 1 and len(bwd) == 1, mask
    o_f, o_b = plan.op_info(*fwd[0]), plan.op_info(*bwd[0])
    assert o_f["N"] == 16 and o_f["K"] == 2 * 3 * 2 * case[4][0], o_f          # 2 frames x 3 positions x (kernel_num[0] + kernel_num[0]) channels
    assert o_b["N"] == 2 * case[4][0] and o_b["K"] == 80, o_b                  # both sources' gradients; 2 frames x 5 positions x 8 buffer channels
    assert _taken(plan) == set(fwd + bwd), (sorted(_taken(plan)), fwd, bwd)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_selection_rule(case):
    """No GPU: the planner and the selection rule alone."""
    plan = _make_plan(case)
    knobs.set("THIN_MASK", "0")
    assert _taken(plan) == set()
    knobs.unset("THIN_MASK")
    assert _taken(plan) == set()                       # default rule: these plans are below its row threshold
    knobs.set("THIN_MASK", "2")
    for grid in GRIDS:
        knobs.set("THIN_MASK_GRID", str(grid))
        _assert_exactly_the_mask_layer(plan, case)
    knobs.unset("THIN_MASK_GRID")
    assert _taken(_make_plan(case[:6] + ("fp32",))) == set()


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_every_op_against_host_simulator_thin_mask(case, grid):
    from test_gpu_ops import every_op_against_host_simulator
    knobs.set("THIN_MASK", "2")
    knobs.set("THIN_MASK_GRID", str(grid))
    _assert_exactly_the_mask_layer(_make_plan(case), case)
    every_op_against_host_simulator(*case, report_prefix=f"ops_report_thin_mask_g{grid}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_two_runs_are_equal(case):
    plan = _make_plan(case)
    knobs.set("THIN_MASK", "2")
    _assert_exactly_the_mask_layer(plan, case)
    first = _run_both_phases(case, plan)
    second = _run_both_phases(case, plan)
    diff = []
    for name in plan.buffer_names():
        a, off, nb, _ = plan.buffer(name)
        if nb > 0 and not torch.equal(first[a].view(torch.uint8)[off:off + nb], second[a].view(torch.uint8)[off:off + nb]):
            diff.append(name)
    for a, name in ((2, "A_GRAD"), (3, "A_STATE"), (5, "A_IO")):
        if not torch.equal(first[a].view(torch.uint8), second[a].view(torch.uint8)):
            diff.append(name)
    assert not diff, "buffers that differ between two runs: " + " ".join(diff)
