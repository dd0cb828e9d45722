"""The frame-staged weight-gradient kernel of the thin layers (csrc/thin_wgrad.hip; knob THIN_WGRAD, read per launch; which launches take it:
test_thin_wgrad_cpu.py).  One workgroup per row split walks the split's 32-row steps frame by frame through an LDS ring, so WG_NSPLIT varies its grid:

* exact sums: the two small DCCRN plans on integer data (exact_data.py) with every launch of a built form on the kernel, at WG_NSPLIT = 1 (one workgroup
  walks every row and every batch boundary), 3 (a batch boundary inside a split), the planner's rule and 100000 (one step per split: the ring is shorter
  than its depth, trailing splits are empty, splits start in the middle of a frame).  Every WGRAD, SPLITSUM and UNPACK launch is byte-equal to the
  host simulator with no stray byte - the zero pad columns and the all-zero partials of empty splits included;
* bit identity on float data: forward + backward with the kernel off and on, at WG_NSPLIT unset, 1 and 3: every plan buffer and the gradient, state,
  I/O and workspace arenas are equal in every byte - the partial sums keep the bits of wgrad_bf16_dma_kernel (one 16 x 16 x 32 MFMA per tile and
  32-row step, steps ascending, the rows of a step in the same k slots), so a training run computes what it computed;
* run to run: the kernel twice more, the same buffers: a ring slot read too early or a second writer shows here."""
import pytest
import torch

import exact_data as ed
from exact_data import Case, DEFAULT_KN, KIND_WGRAD, NSPLITS, SMALL_KN
from test_gpu_rungemm_persist import _make_plan, _run_both_phases
from test_gpu_wgrad_exact import _all_rows_bounds, _state
from util import knobs

ON = (("THIN_WGRAD", "2"),)
EXACT_CASES = [Case("dccrn_small_thin_wgrad", "DCCRN", 3, 4000, "R", SMALL_KN, 128, "bf16", ON),
               Case("dccrn_default_thin_wgrad", "DCCRN", 1, 2400, "C", DEFAULT_KN, 256, "bf16", ON)]
# launches on the kernel: kernel_num[0] = 16: both sources of the second-to-last decoder layer and the second encoder layer (the mask layer's pair would
# need <8, 16>: refused); the default channels: those three and the mask layer's two sources
TAKEN = {"dccrn_small_thin_wgrad": 3, "dccrn_default_thin_wgrad": 5}
# the same plans without the knob (exact_data.CASES): the 2^24 bound is a property of the data and the descriptors, measured once per plan on the host
BASE = {"dccrn_small_thin_wgrad": ed.CASES[0], "dccrn_default_thin_wgrad": ed.CASES[1]}
# exact_data's four and 2: with three batch items, two splits put a batch boundary in the middle of each (three splits cut at the boundaries)
MY_NSPLITS = NSPLITS + (2,)
FLOAT_CASES = [("DCCRN", 3, 4000, "R", SMALL_KN, 128, "bf16"), ("DCCRN", 1, 2400, "C", DEFAULT_KN, 256, "bf16")]
FLOAT_NSPLITS = (None, 1, 3)


def _on_kernel(plan):
    from sefd_amd.plan import WG_FAMILY_THIN
    return [i for i in range(plan.num_ops(1)) if plan.op_info(1, i)["kind"] == KIND_WGRAD and plan.op_info(1, i)["family"] == WG_FAMILY_THIN]


@pytest.mark.gpu
@pytest.mark.parametrize("ns", MY_NSPLITS, ids=lambda n: f"nsplit_{n}")
@pytest.mark.parametrize("case", EXACT_CASES, ids=ed.case_id)
def test_exact_sums_at_every_row_split(case, ns):
    plan, launches, host, dev = _state(case, ns)          # (make_plan unsets the case's knobs behind the planner: the launches read THIN_WGRAD below)
    knobs.set("THIN_WGRAD", "2")
    launches = ed.wgrad_ops(plan)                          # the families of the moment
    exact = [ln for ln in launches if ln.kind == KIND_WGRAD and not ed.fused(ln)]
    assert (case.B, case.L, case.mode, case.kn, case.ru, case.dtype) == BASE[case.name][2:8]
    bounds = _all_rows_bounds(BASE[case.name])
    assert len(bounds) == len(exact) and all(b < ed.LIMIT for b in bounds), (case.name, max(bounds))
    assert len(_on_kernel(plan)) == TAKEN[case.name], _on_kernel(plan)
    mine = [ln for ln in exact if ln.op in _on_kernel(plan)]
    if ns in (1, 2, 3):
        assert all(ln.g.nsplit == ns for ln in mine)
    if ns == 2 and case.B == 3:                            # a batch boundary strictly inside each split
        assert all(ed.rows_of_longest_split(ln.g) * ed.ROWS % (ln.g.Tout * ln.g.Fo) != 0 for ln in mine)
    if ns == 100000:
        assert all(ed.rows_of_longest_split(ln.g) == 1 and ln.g.nsplit > 4 for ln in mine)
    verdicts = ed.run_launches(plan, launches, dev, host)
    assert plan.lib.sefd_plan_status(plan.h, 0) == 0
    bad = [f"op {ln.op} tag {ln.tag} kind {ln.kind} family {ln.family}: {v.miss} stray {v.stray}" for ln, v in verdicts if not v.ok]
    assert not bad, "\n".join(bad[:20])
    assert len(verdicts) == len(launches)


def _plan_at(case, ns):
    knobs.unset("WG_NSPLIT")
    if ns is not None:
        knobs.set("WG_NSPLIT", str(ns))
    try:
        return _make_plan(case)
    finally:
        knobs.unset("WG_NSPLIT")


def _differing(plan, a, b):
    diff = []
    for name in plan.buffer_names():
        ar, off, nb, _ = plan.buffer(name)
        if nb > 0 and not torch.equal(a[ar].view(torch.uint8)[off:off + nb], b[ar].view(torch.uint8)[off:off + nb]):
            diff.append(name)
    for ar, name in ((2, "A_GRAD"), (3, "A_STATE"), (5, "A_IO"), (0, "A_WS")):
        if not torch.equal(a[ar].view(torch.uint8), b[ar].view(torch.uint8)):
            diff.append(name)
    return diff


_runs = {}                                                 # (case, ns) -> (plan, arenas with the kernel on): computed once, never changed


def _on(case, ns):
    if (case, ns) not in _runs:
        for k in [k for k in _runs if k[0] != case]:
            del _runs[k]
        plan = _plan_at(case, ns)
        knobs.set("THIN_WGRAD", "2")
        assert len(_on_kernel(plan)) == (5 if case[4][0] == 32 else 3)
        _runs[(case, ns)] = (plan, _run_both_phases(case, plan))
    knobs.set("THIN_WGRAD", "2")
    return _runs[(case, ns)]


@pytest.mark.gpu
@pytest.mark.parametrize("ns", FLOAT_NSPLITS, ids=lambda n: f"nsplit_{n}")
@pytest.mark.parametrize("case", FLOAT_CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_bit_identical_to_the_kernel_replaced(case, ns):
    plan, got = _on(case, ns)
    knobs.set("THIN_WGRAD", "0")
    assert _on_kernel(plan) == []
    ref = _run_both_phases(case, plan)
    diff = _differing(plan, ref, got)
    assert not diff, "buffers that differ from the kernel replaced: " + " ".join(diff)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", FLOAT_NSPLITS, ids=lambda n: f"nsplit_{n}")
@pytest.mark.parametrize("case", FLOAT_CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_runs_are_bit_equal(case, ns):
    plan, first = _on(case, ns)
    diff = []
    for k in (1, 2):
        diff += [f"run{k}:{n}" for n in _differing(plan, first, _run_both_phases(case, plan))]
    assert not diff, "buffers that differ from the first run: " + " ".join(diff)
