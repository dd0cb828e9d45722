"""Every forward and input-gradient GEMM launch against exact sums, on every kernel that can take it (exact_data.py; the CPU side - the conditions,
the coverage by name, the dropped arms and the comparator on planted faults - is test_rungemm_exact_cpu.py; the weight gradients' file is
test_gpu_wgrad_exact.py).

An arm (exact_data.ARMS) is a set of knobs under which a case's plan is built and its launches run: `tiled` switches every other family off, `default`
sets nothing, persist_g1 / g3 / g0 and thin_g1 / g3 / g0 put every launch of the form on the persistent kernel / the frame-staged kernels with ONE
workgroup (every tile, every batch boundary, every ring wrap in one run), three (uneven runs) and the resident grid, `direct` and `wide` lower the
row thresholds of thin.hip and of the 256 x 256 tile, `bnfuse2` gives every layer's input gradient the BatchNorm-backward epilogue (on rungemm_kernel;
wide_bnfuse2 and direct_bnfuse2 take it to the other two kernels that instantiate it, cgemm256.hip and thin.hip).  The arms that
move no launch of a case are dropped at collection (exact_data.DROPPED, asserted against the rule on the host in the CPU file).

Every RUNGEMM of both phases starts from ONE state (exact_data.fill_exact: integers in -3 .. 3 in every buffer, parameters in -1 .. 1, the packed
weights from the plan's own PACK launches) and runs on the simulator and on the device.  The conditions are asserted per launch from the simulator
alone - every value written an integer, the launch over absolute values below 2^24, every statistics sum of squares below 2^24 - so every fp32
accumulator of any MFMA shape and any grouping of k is exact and the bar is BYTE EQUALITY: y, y2 and the statistics rows, in every arena; a byte
changed anywhere else (a pad column, a frame the launch does not store, another buffer) is a stray byte.  Two arms that both pass ran kernels that
are equal to each other on this data - the thin_mask pair included, for which float data admits no identity.  The one exception: the statistics rows
of a kRunBnBwd launch (BatchNorm-backward sums formed with mean_invstd and branch tests) keep opcheck.tolerance()'s bar over every element of the
rows; the report says where they were byte-equal too."""
import pytest

import exact_data as ed
from exact_data import LIMIT, PAIRS, RUN_BN_BWD, RUN_FAMILY_NAMES as NAMES, pair_id
from plan_check import report_path


@pytest.mark.gpu
@pytest.mark.parametrize("case,arm", PAIRS, ids=pair_id)
def test_every_rungemm_byte_equal_to_the_simulator(case, arm):
    with ed.under(case, arm) as plan:
        launches = ed.run_ops(plan)
        state = ed.ExactState(plan, case.name)
        saved = [a.cuda() for a in state.saved]
        dev = [a.clone() for a in saved]
        conds = {}

        def conditions_hold(ln):
            c = conds[(ln.phase, ln.op)] = state.cond
            assert not c.integers, (case.name, arm, ln.tag, "(a) a non-integer value written:", c.integers)
            assert 0 < c.bound < LIMIT, (case.name, arm, ln.tag, "(b)", c.bound)
            assert c.sumsq < LIMIT, (case.name, arm, ln.tag, "(c)", c.sumsq)

        verdicts = ed.run_launches(plan, launches, dev, state=state, saved_device=saved, on_simulated=conditions_hold)
        assert plan.lib.sefd_plan_status(plan.h, 0) == 0
        assert [ln for ln, _ in verdicts] == launches and launches
    lines = []
    for ln, v in verdicts:
        word = "MISS" if not v.ok else "exact" if not v.loose else "ok (rows byte-equal too)" if v.worst == 0 else f"ok (rows err/tol {v.worst:.3e})"
        lines.append(f"op {ln.op:3d} phase {ln.phase} tag {ln.tag:4d} {NAMES.get(ln.family, ln.family):10s} M {ln.g.M:6d} N {ln.g.N:5d} K {ln.K:5d} {word} stray {v.stray}"
                     + (f" {v.miss}" if v.miss else ""))
    bound, sumsq = max(c.bound for c in conds.values()), max(c.sumsq for c in conds.values())
    with open(report_path(f"rungemm_exact_{case.name}_{arm}.txt"), "w") as f:
        f.write("\n".join(lines + [f"largest accumulator bound {bound:.0f}, largest statistics sum of squares {sumsq:.0f} (2^24 = {LIMIT})"]) + "\n")
    bad = [line for line, (ln, v) in zip(lines, verdicts) if not v.ok]
    assert not bad, "\n".join(bad[:20])
    assert {(ln.phase, ln.op) for ln, v in verdicts if v.loose} == {(ln.phase, ln.op) for ln in launches if ln.g.flags & RUN_BN_BWD}
