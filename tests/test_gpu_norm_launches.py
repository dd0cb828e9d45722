"""Every BatchNorm2d + PReLU and every ComplexBatchNorm launch of the device against a float64 reference of its own, per element (norm_data.py: the cases, the planted states,
the references, the bars and the comparator; the CPU side - the data conditions, the coverage by name, the comparator on planted faults and the host
simulator under the same driver - is test_norm_launches_cpu.py).

Each launch of a case runs ALONE (plan.run(phase, dev, 0, i, i + 1)) from a state planted straight into the buffers its descriptor names; no GEMM
runs.  BN_APPLY, BN_BWD_REDUCE, BN_BWD_FINALIZE, the mean of BN_FINALIZE and the fp64 totals of its SyncBN mode 1 are held to BYTE EQUALITY with the
float64 value (dyadic data: every fp32 intermediate is exact under any contraction and order); invstd and the running statistics of BN_FINALIZE to
1 fp32 ulp (3 in eval), BN_BWD_APPLY to the rounding-count bar of norm_data.N_ROUNDINGS.  Every byte outside a launch's outputs is a stray byte.
The ComplexBatchNorm launches (csrc/cbn.hip) likewise: CBN_STATS, CBN_APPLY and CBN_BWD_REDUCE byte-equal, CBN_FINALIZE and CBN_BWD_FINALIZE at
2 fp32 ulps / 2 * 2^-24 * sum|terms| against the reference module's closed form and torch autograd in float64, CBN_BWD_APPLY at its rounding count.
A finalize runs three times in a row from the same planted input and must give the same bytes each time (the two-level kernels' tickets reset
themselves only if every chunk arrives), with a finalize of another chunk count in between where the case has one."""
import pytest
import torch

import norm_data as nd
from plan_check import report_path


def device_run(plan, phase, arenas, op):
    plan.run(phase, arenas, 0, op, op + 1)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("case", nd.CASES, ids=nd.case_id)
def test_every_batchnorm_launch_against_float64(case):
    results = nd.run_case(case, "cuda", device_run)
    plan = nd.plan_of(case)
    assert plan.lib.sefd_plan_status(plan.h, 0) == 0
    lines = nd.report_lines(case, results)
    with open(report_path(f"norm_launches_{case.name}.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    assert [(ln.phase, ln.op) for ln, _, _, _ in results] == [(ln.phase, ln.op) for ln in nd.select(case, nd.launches(plan))]
    bad = [line for line, (_, v, _, _) in zip(lines, results) if not v.ok]
    assert not bad, "\n".join(bad[:20])
