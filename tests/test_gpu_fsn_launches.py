"""Every struct-Fsn launch of the device (csrc/fsn.hip: FSN_IN, FSN_SCALE, FSN_SBSUM, FSN_SBBUILD, FSN_NORMSTAT, FSN_ACT, FSN_OUT, FSN_OUT_BWD,
FSN_SBBWD_SUM, FSN_SBBWD_APPLY plain and gather, FSN_NORMBWD) against a float64 reference of its own, per element (fsn_launch_data.py: the cases, the
planted states, the references, the bars and the comparator; the CPU side - the data conditions, the edges, the coverage by name, the closed forms
against autograd, the comparator on planted faults and the host simulator under the same driver - is test_fsn_launches_cpu.py).

Each launch of a case runs ALONE (plan.run(phase, dev, 0, i, i + 1)) from a state planted straight into the buffers its descriptor names; no GEMM and
no recurrence runs.  Byte equality where the data is dyadic (FSN_IN, every `sums` row, FSN_OUT / FSN_OUT_BWD / FSN_ACT / the gather behind
FSN_NORMBWD with none, ReLU, ReLU6; every pad column), 1 fp32 ulp on the means, 1 / 2 ulps on FSN_NORMSTAT, the rounding-count bars on FSN_SCALE,
FSN_SBBUILD and FSN_SBBWD_APPLY in mode 0, 2^-24 x sum|terms| on FSN_NORMBWD; tanhf is measured against float64, printed, written into the case's
report and held to fsn_launch_data.TANHF_BAR_ULPS.  Every byte outside a launch's outputs is a stray byte.  A FSN_NORMSTAT and a *_SUM launch runs
twice from the same planted input and must give the same bytes."""
import pytest
import torch

import fsn_launch_data as fd
from plan_check import report_path


def device_run(plan, phase, arenas, op):
    plan.run(phase, arenas, 0, op, op + 1)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("case", fd.CASES, ids=fd.case_id)
def test_every_fsn_glue_launch_against_float64(case):
    results = fd.run_case(case, "cuda", device_run)
    plan = fd.plan_of(case)
    assert plan.lib.sefd_plan_status(plan.h, 0) == 0
    lines = fd.report_lines(case, results)
    print("\n".join(lines))
    with open(report_path(f"fsn_launches_{case.name}.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    assert [(ln.phase, ln.op) for ln, _, _, _ in results] == [(ln.phase, ln.op) for ln in fd.launches(plan)]
    bad = [line for line, (_, v, _, _) in zip(lines, results) if not v.ok]
    assert not bad, "\n".join(bad[:20])
