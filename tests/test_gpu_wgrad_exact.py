"""Every weight-gradient kernel against exact sums, at every row split (exact_data.py; the CPU side is test_wgrad_exact_cpu.py).

The other two kinds of launch, the forward and the input-gradient GEMMs (OP_RUNGEMM of both phases), are held to the same bar - byte equality with the
simulator on integer data, on every kernel family at every grid - in test_gpu_rungemm_exact.py; test_gpu_rungemm_persist.py, test_gpu_thin_mask.py and
test_gpu_thin_stage.py vary the grid on float data and compare the kernels with each other.  This is the weight gradients' file.  Knob WG_NSPLIT varies
the row splits at a fixed shape:

  1       one workgroup per tile walks every row of every batch item (hundreds of ring steps, every batch boundary, every stage wrap);
  3       an uneven split with a batch boundary inside a split;
  unset   the planner's rule (4 to 8 steps per split at these sizes);
  100000  one 32-row step per split: the ring is shorter than its depth, and where the rows are walked per batch item trailing splits are empty.

The operands are small integers (exact_data.fill), so every partial sum is an integer below 2^24 (asserted on the host, per launch, over ALL rows of the
launch - which bounds every split of every partition) and the bar is BYTE EQUALITY with the host simulator from the same pre-launch state, for every
WGRAD, SPLITSUM and UNPACK launch of the backward phase; a byte changed anywhere else in any arena is a stray byte.  The one exception is the fused
first-layer launch (kRunDyFromBn: dy formed with float constants), which keeps opcheck's bar; exactly one per bf16 DCCRN plan whose first layer runs on
the spectrum kernels.  Then the chain: the flat gradient arena behind WGRAD, SPLITSUM and UNPACK is the same bytes at all four split counts - exact sums
do not depend on the partition (no simulator involved).

The cases (rows of test_gpu_ops.py / plan_configs.py) reach every family launch_wgrad picks (asserted by name in test_wgrad_exact_cpu.py): the first layer
plain and fused, the rank-N kernel, the LDS-DMA kernel as 256 x 256 tile, with the ones MFMA, as 128 x 512 tile (CRN tags 104, 105, 400, 401) and with
128 / 64 / 32 wide n tiles, the register-staged bf16 kernel 128 / 64 wide (Fo = 514 is no power of two), the fp32 kernel."""
import pytest
import torch

import exact_data as ed
from exact_data import CASES, KIND_WGRAD, NSPLITS, case_id
from plan_check import report_path
from sefd_amd.plan import WG_FAMILY_NAMES

_bounds = {}


def _all_rows_bounds(case):
    """[sum of |x * dy| over ALL rows, largest element] per non-fused WGRAD of the case, in launch order: once per case, on the host."""
    if case not in _bounds:
        plan = ed.make_plan(case, 1)
        ar = plan.alloc_arenas("cpu")
        ed.fill(plan, ar)
        _bounds[case] = [ed.exact_sum_bound(plan, ar, ln) for ln in ed.wgrad_ops(plan) if ln.kind == KIND_WGRAD and not ed.fused(ln)]
    return _bounds[case]


def _state(case, ns):
    plan = ed.make_plan(case, ns)
    host = plan.alloc_arenas("cpu")
    ed.fill(plan, host)
    dev = plan.alloc_arenas("cuda")
    for a in range(6):
        dev[a].copy_(host[a])
    return plan, ed.wgrad_ops(plan), host, dev


@pytest.mark.gpu
@pytest.mark.parametrize("ns", NSPLITS, ids=lambda n: f"nsplit_{n}")
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_launch_byte_equal_to_the_simulator(case, ns):
    plan, launches, host, dev = _state(case, ns)
    exact = [ln for ln in launches if ln.kind == KIND_WGRAD and not ed.fused(ln)]
    bounds = _all_rows_bounds(case)
    assert len(bounds) == len(exact) and all(b < ed.LIMIT for b in bounds), (case.name, max(bounds))
    if ns == 1:
        assert all(ln.g.nsplit == 1 for ln in exact)
    if ns == 100000:
        assert any(ed.rows_of_longest_split(ln.g) == 1 and ln.g.nsplit > 4 for ln in exact)
    verdicts = ed.run_launches(plan, launches, dev, host)
    assert plan.lib.sefd_plan_status(plan.h, 0) == 0
    lines = []
    for ln, v in verdicts:
        what = "WGRAD" if ln.kind == KIND_WGRAD else "SPLITSUM" if ln.kind == ed.KIND_SPLITSUM else "UNPACK"
        geo = f"{WG_FAMILY_NAMES[ln.family]:20s} M {ln.g.M:6d} N {ln.g.N:5d} ldw {ln.g.ldw:5d} nsplit {ln.g.nsplit:4d}" if ln.g is not None else ""
        lines.append(f"op {ln.op:3d} {what:8s} tag {ln.tag:4d} {geo} {'exact' if v.ok and not ed.fused(ln) else 'ok' if v.ok else 'MISS'} stray {v.stray}"
                     + (f" err/tol {v.worst:.3e}" if ed.fused(ln) else "") + (f" {v.miss}" if v.miss else ""))
    with open(report_path(f"wgrad_exact_{case.name}_nsplit_{ns}.txt"), "w") as f:
        f.write("\n".join(lines + [f"largest sum of |x * dy| over all rows of a launch: {max(bounds):.0f}"]) + "\n")
    bad = [line for line, (ln, v) in zip(lines, verdicts) if not v.ok]
    assert not bad, "\n".join(bad[:20])
    assert len(verdicts) == len(launches)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_folded_gradient_does_not_depend_on_the_split_count(case):
    grads, fed = {}, None
    for ns in NSPLITS:
        plan, launches, host, dev = _state(case, ns)
        ed.run_launches(plan, launches, dev)
        torch.cuda.synchronize()
        assert plan.lib.sefd_plan_status(plan.h, 0) == 0
        grads[ns] = dev[ed.GRAD].cpu()
        if fed is None:                                          # what the fused launch feeds: float sums, held to opcheck's bar per tensor below
            fed = ed.fed_by_fused(plan, launches, dev, lambda ar, op: plan.run(ed.PHASE_BWD, ar, 0, op, op + 1)).cpu()
            assert bool(fed.any()) == any(ed.fused(ln) for ln in launches)
    ref = grads[1]
    assert float(ref.abs().max()) > 0
    for ns in NSPLITS:
        same = grads[ns].view(torch.int32) == ref.view(torch.int32)
        assert bool((same | fed).all()), (case.name, ns, int((~(same | fed)).sum()), "gradient elements differ from WG_NSPLIT = 1")
        for name, (off, shape) in plan.params.items():
            n = max(1, int(torch.Size(shape).numel()))
            m = fed[off:off + n]
            if bool(m.any()):
                a, b = grads[ns][off:off + n][m].double(), ref[off:off + n][m].double()
                assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max()), (case.name, ns, name)
