"""The strided frame-staged kernel at 64 channels and 128 columns on the GPU (csrc/thin_stage.hip, thin_stage_st_kernel<64, 4, 32>; knobs THIN_STAGE64 /
THIN_STAGE64_GRID): the third encoder layer's forward conv (tag 102: bias, BatchNorm statistics rows of four frames through the fp32 tile in LDS) and the two
input gradients of the third-to-last decoder layer (tag 403: one launch per destination).  Which launches take it: tests/test_thin_stage64_cpu.py.

* every launch of two small DCCRN plans against the host simulator with the three launches on the kernel, at grid 1 (ONE workgroup walks every frame: the
  LDS ring carries over every batch boundary), grid 3 (uneven runs, still whole statistics rows) and the resident grid.  The simulator's tolerances are
  the bar;
* forward + backward with the kernel off and on, at grids 1, 3 and 0: every plan buffer - outputs, the statistics partial rows, mean / invstd - and the
  A_GRAD, A_STATE, A_IO and A_WS arenas are equal in every byte to the kernels replaced;
* forward + backward at grids 1, 3, 0 and 0 again: bit-equal across the four runs.

The cases: B = 1, L = 2400 - one item of 27 frames (a last statistics row of three frames), bins 0 and Fo - 1; B = 3, L = 4000 - 43 output frames per item
(44 in the decoder), so no run of 4-frame rows divides an item and the ring crosses two batch boundaries."""
import pytest
import torch

from test_gpu_rungemm_persist import _make_plan, _run_both_phases
from test_thin_stage64_cpu import CASES, GRIDS, assert_exactly_the_three_launches, taken
from util import knobs

ARENAS = ((2, "A_GRAD"), (3, "A_STATE"), (5, "A_IO"), (0, "A_WS"))


def _differences(plan, ref, got, label=""):
    diff = []
    for name in plan.buffer_names():
        a, off, nb, _ = plan.buffer(name)
        if nb > 0 and not torch.equal(ref[a].view(torch.uint8)[off:off + nb], got[a].view(torch.uint8)[off:off + nb]):
            diff.append(label + name)
    for a, name in ARENAS:
        if not torch.equal(ref[a].view(torch.uint8), got[a].view(torch.uint8)):
            diff.append(label + name)
    return diff


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_every_op_against_host_simulator_thin_stage64(case, grid):
    from test_gpu_ops import every_op_against_host_simulator
    knobs.set("THIN_STAGE64", "2")
    knobs.set("THIN_STAGE64_GRID", str(grid))
    assert_exactly_the_three_launches(_make_plan(case))
    every_op_against_host_simulator(*case, report_prefix=f"ops_report_thin_stage64_g{grid}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_grids_and_runs_are_bit_equal(case):
    plan = _make_plan(case)
    knobs.set("THIN_STAGE64", "2")
    runs = []
    for grid in GRIDS + [0]:
        knobs.set("THIN_STAGE64_GRID", str(grid))
        assert_exactly_the_three_launches(plan)
        runs.append(_run_both_phases(case, plan))
    diff = [d for k, other in enumerate(runs[1:], 1) for d in _differences(plan, runs[0], other, f"run{k}:")]
    assert not diff, "buffers that differ from the grid-1 run: " + " ".join(diff)


_reference = {}


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_bit_identical_to_the_kernels_replaced(case, grid):
    """Outputs AND statistics partial rows keep the bits of the kernels replaced.  At 128 columns those give a column two waves of 64 rows, so per column
    and PAIR of frames there are two chains from 0.f over the rows 4 hh + 8 k + r of the first and then of the second frame; the pair is chain 0 + chain 1,
    a row its two pairs added in ascending order to 0.f."""
    plan = _make_plan(case)
    if case not in _reference:                         # the replaced kernels' result: computed once per case, never changed
        knobs.set("THIN_STAGE64", "0")
        assert taken(plan) == set()
        _reference[case] = _run_both_phases(case, plan)
    knobs.set("THIN_STAGE64", "2")
    knobs.set("THIN_STAGE64_GRID", str(grid))
    assert_exactly_the_three_launches(plan)
    diff = _differences(plan, _reference[case], _run_both_phases(case, plan))
    assert not diff, "buffers that differ from the kernels replaced: " + " ".join(diff)
