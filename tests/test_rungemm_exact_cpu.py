"""The exact forward / input-gradient tier without a GPU (exact_data.py; the GPU side is test_gpu_rungemm_exact.py).

* conditions (a) to (c) of exact_data.conditions() for every RUNGEMM of both phases of every case under every arm kept for it, measured with the
  simulator; the largest values go to a report file.  In the same pass the comparator is given the simulator's own result as the device's: it must
  pass, the simulator must have written nothing but the y / y2 / statistics elements the descriptor names (the comparator decodes them itself), and
  the launches with a region outside byte equality must be exactly the kRunBnBwd ones;
* coverage, by name: every RUN_FAMILY_* is taken by a launch of some (case, arm), every one but enc0 in both phases; two destinations, kRunAccum,
  kRunRelu, forward statistics on the tiled, persistent and thin_stage families, kRunBnBwd on each of the three kernels that instantiate the
  epilogue (rungemm_kernel, cgemm256, thin.hip), an M that is no multiple of 128;
* which arms are dropped for which case (exact_data.arms_of) is pinned;
* the comparator on planted faults: the "device" is the simulator's own result from a state altered in one place, or its result altered in one
  place; each must come back as a miss (or as stray bytes) at the right place."""
import pytest
import torch

import exact_data as ed
from exact_data import ARMS, CASES, LIMIT, PHASE_BWD, PHASE_FWD, RUN_ACCUM, RUN_BN_BWD, RUN_RELU, WS
from plan_check import report_path
from sefd_amd import plan as sp

FAMILIES, NAMES = ed.RUN_FAMILIES, ed.RUN_FAMILY_NAMES
_operand, _typed = ed.operand, ed.typed


def test_dropped_arms_are_the_ones_that_move_no_launch():
    """exact_data.DROPPED (the table the (case, arm) pairs of both test files are built from at collection) is what the rule gives on the host."""
    for case in CASES:
        kept, dropped = ed.arms_of(case)
        assert dropped == ed.DROPPED.get(case.name, []), (case.name, dropped)
        assert kept and kept[0] == "tiled" and sorted(kept + dropped) == sorted(ARMS), (case.name, kept)
    assert [(c.name, a) for c, a in ed.PAIRS] == [(c.name, a) for c in CASES for a in ed.arms_of(c)[0]]


def test_cases_and_arms_reach_every_family_and_every_epilogue():
    assert FAMILIES == {k[len("RUN_FAMILY_"):].lower(): v for k, v in vars(sp).items() if k.startswith("RUN_FAMILY_") and k != "RUN_FAMILY_NONE"}
    seen, feats = {}, {}
    for case in CASES:
        for arm in [a for c, a in ed.PAIRS if c is case]:
            with ed.under(case, arm) as plan:
                for ln in ed.run_ops(plan):
                    g, where = ln.g, f"{case.name} / {arm}: phase {ln.phase} op {ln.op} tag {ln.tag} M {ln.g.M} N {ln.g.N} K {ln.K}"
                    assert ln.family in NAMES, where                  # RUN_FAMILY_NONE: a descriptor no kernel takes
                    seen.setdefault((NAMES[ln.family], ln.phase), where)
                    has = [("two destinations", g.n2 > 0), ("kRunAccum", g.flags & RUN_ACCUM), ("kRunRelu", g.flags & RUN_RELU),
                           ("kRunBnBwd", ed.bn_bwd(ln)), (f"kRunBnBwd on {NAMES[ln.family]}", ed.bn_bwd(ln)), ("M % 128 != 0", g.M % ed.KBM),
                           ("two destinations, first not a multiple of 8", g.n2 % 8)]
                    has += [(f"forward statistics on {NAMES[ln.family]}", ln.phase == PHASE_FWD and g.stats.arena >= 0 and not ed.bn_bwd(ln))]
                    for name, on in has:
                        if on:
                            feats.setdefault(name, where)
    for k in sorted(seen):
        print(k, seen[k])
    for k in sorted(feats):
        print(k, "-", feats[k])
    for name in FAMILIES:
        assert (name, PHASE_FWD) in seen, f"no forward launch on {name}"
        assert name == "enc0" or (name, PHASE_BWD) in seen, f"no backward launch on {name}"
    assert ("enc0", PHASE_BWD) not in seen                        # (the first layer has no input gradient)
    for name in ("two destinations", "kRunAccum", "kRunRelu", "kRunBnBwd", "M % 128 != 0", "forward statistics on tiled",
                 "forward statistics on persist", "forward statistics on thin_stage",
                 "kRunBnBwd on tiled", "kRunBnBwd on cgemm256", "kRunBnBwd on direct"):       # the three kernels that instantiate the epilogue
        assert name in feats, f"no launch with {name}"


@pytest.mark.parametrize("case,arm", ed.PAIRS, ids=ed.pair_id)
def test_conditions_hold_and_the_simulator_passes_its_own_comparison(case, arm):
    lines, bound, sumsq, loose, bnb = [], 0.0, 0.0, set(), set()
    with ed.under(case, arm) as plan:
        state = ed.ExactState(plan, case.name)
        launches = ed.run_ops(plan)
        assert launches
        for ln in launches:
            sim = state.simulate(ln)
            c = state.cond
            assert not c.integers, (case.name, arm, ln.tag, "(a) a non-integer value written:", c.integers)
            assert 0 < c.bound < LIMIT, (case.name, arm, ln.tag, "(b)", c.bound)
            assert c.sumsq < LIMIT, (case.name, arm, ln.tag, "(c)", c.sumsq)
            assert (c.sumsq > 0) == (ln.g.stats.arena >= 0 and not ed.bn_bwd(ln)), (case.name, arm, ln.tag)
            if "loose" not in state.notes:                       # (else the same descriptor over the same buffers went through this under an earlier arm)
                v = ed.compare_exact(plan, ln, state.saved, sim, sim)
                assert v.ok and v.stray == 0 and v.worst == 0, (case.name, arm, ln.tag, v)
                state.notes["loose"] = v.loose
            if state.notes["loose"]:
                loose.add((ln.phase, ln.op))
            if ln.g.flags & RUN_BN_BWD:
                bnb.add((ln.phase, ln.op))
            bound, sumsq = max(bound, c.bound), max(sumsq, c.sumsq)
            lines.append(f"op {ln.op:3d} phase {ln.phase} tag {ln.tag:4d} {NAMES[ln.family]:10s} M {ln.g.M:6d} N {ln.g.N:5d} K {ln.K:5d} "
                         f"bound {c.bound:9.0f} statistics {c.sumsq:9.0f}")
    assert loose == bnb, (case.name, arm, sorted(loose ^ bnb))
    assert bool(bnb) == ("bnfuse2" in arm), (case.name, arm, sorted(bnb))      # (BN_FUSE=1 fuses layers of at least 8192 rows: none here)
    tail = f"largest accumulator bound {bound:.0f} = {bound / LIMIT:.5f} * 2^24, largest statistics sum of squares {sumsq:.0f} = {sumsq / LIMIT:.5f} * 2^24"
    print(f"{case.name} / {arm}: {tail}")
    with open(report_path(f"rungemm_exact_cpu_{case.name}_{arm}.txt"), "w") as f:
        f.write("\n".join(lines + [tail]) + "\n")


# ------------------------------------------------------------------------------------------------ planted faults
def _y(ar, g, second=False):
    """(typed view from the destination's Ptr on, element indices [M][columns]) of y (or y2)."""
    ptr, idx, _ = ed.dest_index(g)[1 if second else 0]
    return _typed(ar, ptr.arena, ptr.off, g.ydt), idx


def _readers(g, arena, off, idx):
    """{(row m, packed column k)} of the rows whose run elements are element `idx` of the source at (arena, off) (hostsim.cpp a_elem)."""
    out = set()
    for s in range(g.nseg):
        sg = g.seg[s]
        if sg.src < 0 or (g.x[sg.src].arena, g.x[sg.src].off) != (arena, off):
            continue
        for b in range(g.M // (g.Tout * g.Fo)):
            for u in range(g.Tout):
                for fo in range(g.Fo):
                    j = idx - (b * g.bstride[sg.src] + (u + sg.dt) * g.tstride[sg.src] + g.base[sg.src] + sg.off + fo * g.fstride[sg.src])
                    if 0 <= j < sg.len and _operand(g, s, b, u, fo, j) == (arena, off, idx):
                        out.add(((b * g.Tout + u) * g.Fo + fo, sg.koff + j))
    return out


def _site(g, ar, cands):
    """The first (s, b, u, fo, j) of `cands` that the row really reads, whose operand is not zero and meets a weight that is not zero (the run's
    last channels may be pad channels, whose packed weights are zero: nothing is lost with them)."""
    assert not g.flags & 16                                       # (row-major packed weights: no kRunWTile32 in the arm these tests use)
    w = _typed(ar, g.w.arena, g.w.off, g.xdt)[:g.Npad * g.ldw].view(g.Npad, g.ldw)
    for c in cands:
        at = _operand(g, *c)
        if at is not None and float(_typed(ar, at[0], at[1], g.xdt)[at[2]]) != 0 and bool((w[:g.N, g.seg[c[0]].koff + c[4]] != 0).any()):
            return c
    raise AssertionError("no live operand among the candidates")


def _named_row(miss):
    """(row, column n) that a RUNGEMM miss names."""
    assert ": row " in miss and " column n " in miss, miss
    return int(miss.split(": row ")[1].split(" ")[0]), int(miss.split(" column n ")[1].split(" ")[0])


def _conv_launch(launches, phase):
    """The first conv launch of `phase` with a frame shift, more than one batch item, one destination and statistics where the phase has them."""
    return next(ln for ln in launches if ln.phase == phase and ln.g.n2 == 0 and ln.g.M // (ln.g.Tout * ln.g.Fo) > 1 and ln.g.Fo > 1 and not ln.g.flags & 512
                and any(ln.g.seg[s].dt != 0 and ln.g.seg[s].src >= 0 for s in range(ln.g.nseg)) and (phase == PHASE_BWD or ln.g.stats.arena >= 0))


@pytest.mark.parametrize("name,arm,phase", [("dccrn_small", "tiled", PHASE_FWD), ("dccrn_small", "tiled", PHASE_BWD), ("crn_wide", "tiled", PHASE_FWD),
                                            ("dccrn_small_fp32", "tiled", PHASE_FWD)], ids=str)
def test_a_lost_edge_tap_is_a_miss_at_the_rows_that_read_it(name, arm, phase):
    """One operand element zeroed - at the first frame, and at bin Fo - 1 in the last element of its run: the product of one edge tap is lost in every
    row that reads the element and nowhere else; the miss names the first of them."""
    case = next(c for c in CASES if c.name == name)
    with ed.under(case, arm) as plan:
        state = ed.ExactState(plan)
        ln = _conv_launch(ed.run_ops(plan), phase)
        g = ln.g
        good = [a.clone() for a in state.simulate(ln)]
        nb = g.M // (g.Tout * g.Fo)
        data = sorted((s for s in range(g.nseg) if g.seg[s].src >= 0), key=lambda s: g.seg[s].dt)       # (a run behind a frame shift first)
        sites = {
            "first frame": _site(g, state.saved, ((s, b, -g.seg[s].dt, fo, j) for s in data if g.seg[s].dt <= 0 for b in (nb - 1, 0)
                                                  for fo in range(g.Fo // 2, g.Fo) for j in range(g.seg[s].len))),
            "bin Fo - 1": _site(g, state.saved, ((s, b, u, g.Fo - 1, j) for s in data for b in (nb - 1, 0) for u in range(g.Tout // 2, g.Tout)
                                               for j in reversed(range(g.seg[s].len)))),
        }
        for what, c in sites.items():
            arena, off, idx = _operand(g, *c)
            if what == "first frame":
                assert c[2] + g.seg[c[0]].dt == 0
            altered = [a.clone() for a in state.saved]
            _typed(altered, arena, off, g.xdt)[idx] = 0
            sim_bad = [a.clone() for a in altered]
            ed.sim_run(plan, ln.phase, sim_bad, ln.op, ln.op + 1)
            _typed(sim_bad, arena, off, g.xdt)[idx] = _typed(state.saved, arena, off, g.xdt)[idx]      # the faulty run's OUTPUT on the sound input state
            v = ed.compare_exact(plan, ln, state.saved, good, sim_bad)
            assert not v.ok and v.stray == 0 and v.miss, (what, v)
            readers = _readers(g, arena, off, idx)
            assert (c[1] * g.Tout + c[2]) * g.Fo + c[3] in {m for m, _ in readers}
            (yg, ix), (yb, _) = _y(good, g), _y(sim_bad, g)
            differ = yg[ix] != yb[ix]                                  # [M][N]
            rows = set(differ.any(1).nonzero().flatten().tolist())
            assert rows and rows <= {m for m, _ in readers}, (what, sorted(rows), sorted(readers))
            m, n = _named_row(v.miss)
            first = min(rows, key=lambda r: int(ix[r, 0]))             # the comparator walks the buffer: the row stored first
            assert m == first and bool(differ[m, n]) and not bool(differ[m, :n].any()), (what, v.miss)
            b, u, fo = ed.row_of(g, m)
            assert f"(batch item {b}, frame u {u}, bin fo {fo})" in v.miss and f"{int(differ.sum())} elements differ" in v.miss, v.miss
            for word in (f"tag {ln.tag} ", f"family {ln.family} ", f"M {g.M} ", f"N {g.N} ", f"K {ln.K} ", f"Tout {g.Tout} ", f"Fo {g.Fo} ", "flags 0x", "simulator", "device", "before"):
                assert word in v.miss, (word, v.miss)
            print(f"{name} {what}: {v.miss}")


def test_one_ulp_a_swapped_destination_a_shifted_statistics_row_and_stray_bytes():
    case = next(c for c in CASES if c.name == "dccrn_small")
    with ed.under(case, "tiled") as plan:
        state = ed.ExactState(plan)
        launches = ed.run_ops(plan)
        # one output moved by one bf16 ulp, in the last row of the launch
        ln = _conv_launch(launches, PHASE_FWD)
        g = ln.g
        good = [a.clone() for a in state.simulate(ln)]
        dev = [a.clone() for a in good]
        y, ix = _y(dev, g)
        m, n = g.M - 1, g.N - 1
        assert g.ydt == 1
        y.view(torch.int16)[ix[m, n]] += 1
        v = ed.compare_exact(plan, ln, state.saved, good, dev)
        assert not v.ok and v.stray == 0 and _named_row(v.miss) == (m, n) and "1 elements differ" in v.miss and f"-> y[{n}]" in v.miss, v
        # a statistics row given the sums of the next 128-row block
        assert g.M > 2 * ed.KBM
        a, lo, hi, nst = ed.stats_range(g)
        dev = [x.clone() for x in good]
        rows = ed._u8(dev[a])[lo:hi].view(torch.float32).view(-1, nst, g.Npad)
        rows[1] = rows[2]
        v = ed.compare_exact(plan, ln, state.saved, good, dev)
        col = int((rows[1, 0] != ed._u8(good[a])[lo:hi].view(torch.float32).view(-1, nst, g.Npad)[1, 0]).nonzero()[0])
        assert not v.ok and v.stray == 0 and f"128-row block 1 (rows 128 ..) statistics row 0 column {col}:" in v.miss, v
        # one element of y2 swapped with the same element of y
        two = next(c for c in launches if c.g.n2 > 0)
        g2 = two.g
        good_2 = [x.clone() for x in state.simulate(two)]
        dev = [x.clone() for x in good_2]
        (y1, i1), (y2, i2) = _y(dev, g2), _y(dev, g2, True)
        m, n = next((m, n) for m in range(g2.M // 2, g2.M) for n in range(min(g2.n2, g2.N - g2.n2)) if float(y1[i1[m, n]]) != float(y2[i2[m, n]]))
        t = y1[i1[m, n]].clone()
        y1[i1[m, n]] = y2[i2[m, n]]
        y2[i2[m, n]] = t
        v = ed.compare_exact(plan, two, state.saved, good_2, dev)
        assert not v.ok and v.stray == 0 and _named_row(v.miss)[0] == m, v
        assert (f"column n {n} -> y[{n}]" in v.miss) or (f"column n {n + g2.n2} -> y2[{n}]" in v.miss), v.miss
    with ed.under(next(c for c in CASES if c.name == "crn_wide"), "tiled") as plan:
        state = ed.ExactState(plan)
        launches = ed.run_ops(plan)
        # a byte changed in a column of y's buffer that the launch does not store (the buffer's rows are wider than N: pad columns, or the columns of
        # the other sub-pixel phase's launch), and one in a buffer the launch does not touch: stray, no miss
        pad = next(c for c in launches if c.g.n2 == 0 and c.g.y_fstride > c.g.N and c.g.ydt == 1)
        good_p = [x.clone() for x in state.simulate(pad)]
        yp, ixp = _y(good_p, pad.g)
        e = int(ixp[pad.g.M // 2, pad.g.N - 1]) + 1
        assert not bool((ixp == e).any())
        dev = [x.clone() for x in good_p]
        _y(dev, pad.g)[0].view(torch.int16)[e] ^= 1
        v = ed.compare_exact(plan, pad, state.saved, good_p, dev)
        assert not v.ok and v.stray == 1 and not v.miss, v
        other = next(r for r in ed._buffers(plan) if r[1] == WS and r[3] > 0 and torch.equal(ed._u8(good_p[WS])[r[2]:r[2] + r[3]], ed._u8(state.saved[WS])[r[2]:r[2] + r[3]]))
        dev = [x.clone() for x in good_p]
        ed._u8(dev[WS])[other[2] + other[3] - 1] ^= 1
        v = ed.compare_exact(plan, pad, state.saved, good_p, dev)
        assert not v.ok and v.stray == 1 and not v.miss, v


def test_bn_backward_rows_keep_opchecks_bar_and_the_rest_of_the_launch_does_not():
    """kRunBnBwd: a rounding-sized difference in the statistics rows passes, 1 % of their largest element is a miss at opcheck's bar, one ulp in the
    launch's y is a miss at byte equality; on a launch with forward statistics the same rounding-sized difference is a miss."""
    case = next(c for c in CASES if c.name == "dccrn_small")
    with ed.under(case, "bnfuse2") as plan:
        state = ed.ExactState(plan)
        launches = ed.run_ops(plan)
        ln = next(c for c in launches if ed.bn_bwd(c))
        plain = next(c for c in launches if c.g.stats.arena >= 0 and not ed.bn_bwd(c))
        for launch, loose in ((ln, True), (plain, False)):
            g = launch.g
            good = [a.clone() for a in state.simulate(launch)]
            a, lo, hi, nst = ed.stats_range(g)
            assert nst == (3 if loose else 2)
            big = int(ed._u8(good[a])[lo:hi].view(torch.float32).abs().argmax())
            for scale, passes in ((1 + 2.0 ** -22, loose), (1.01, False)):
                dev = [x.clone() for x in good]
                ed._u8(dev[a])[lo:hi].view(torch.float32)[big] *= scale
                assert not torch.equal(dev[a], good[a])
                v = ed.compare_exact(plan, launch, state.saved, good, dev)
                assert v.ok == passes and v.stray == 0 and v.loose == loose, (launch.tag, scale, v)
                if not passes:
                    blk, col = big // (nst * g.Npad), big % g.Npad
                    assert f"128-row block {blk} (rows {blk * ed.KBM} ..) statistics row {big // g.Npad % nst} column {col}:" in v.miss, v.miss
                    assert ("opcheck's bar" in v.miss) == loose, v.miss
            dev = [x.clone() for x in good]
            y, ix = _y(dev, g)
            y.view(torch.int16 if g.ydt == 1 else torch.int32)[ix[g.M // 2, 0]] += 1
            v = ed.compare_exact(plan, launch, state.saved, good, dev)
            assert not v.ok and _named_row(v.miss) == (g.M // 2, 0), v
