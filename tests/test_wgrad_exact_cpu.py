"""The exact weight-gradient tier without a GPU (exact_data.py; the GPU side is test_gpu_wgrad_exact.py).

* the cases reach every kernel family launch_wgrad can pick (Plan.op_info()["family"], csrc/rungemm.hip wgrad_family), each named in a `want` list; the family
  does not change with WG_NSPLIT; the 128 x 512 tile is taken by exactly the four CRN tags; one fused first-layer launch per bf16 DCCRN plan;
* knob WG_NSPLIT: unset or 0 leaves the plans where they were (the fingerprints recorded in profiles/, the raw descriptors in front of and behind a plan
  built under the knob); n > 0 gives every weight gradient min(n, steps) splits, and the partial sums and the fold are sized from it (the folded
  gradient on the simulator is the same bytes at every split count);
* the integer fill meets the 2^24 condition at every launch of every case (measured with the simulator over the operands' absolute values), and the
  simulator's partial sums are integers;
* the comparator: a second simulator run with ONE operand element raised by 1 - at the first and the last valid bin, at frame 0 behind a frame shift, in
  the last row of a batch item, in the last chunk of a run - is flagged, at the split and the packed column the element feeds; a byte changed elsewhere
  is a stray byte."""
import importlib.util
import os

import pytest
import torch

import exact_data as ed
from exact_data import CASES, KIND_WGRAD, NSPLITS, ROWS, WS, case_id
from sefd_amd import plan as sp
from simutil import PHASE_BWD, sim_run
from util import knobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = ["first layer", "first layer fused", "rank-N", "256 x 256", "256 x 256 ones MFMA", "128 x 512", "aligned 128", "aligned 64", "aligned 32",
        "unaligned bf16 128", "unaligned bf16 64", "fp32"]


def test_cases_reach_every_wgrad_family():
    assert sorted(WANT) == sorted(sp.WG_FAMILY_NAMES[1:])
    seen, wide128 = {}, []
    for case in CASES:
        plans = {ns: ed.make_plan(case, ns) for ns in NSPLITS}
        base = ed.wgrad_ops(plans[None])
        for ln in base:
            if ln.kind == KIND_WGRAD:
                assert ln.family != sp.WG_FAMILY_NONE, (case.name, ln.tag)
                seen.setdefault(sp.WG_FAMILY_NAMES[ln.family], f"{case.name} tag {ln.tag} M {ln.g.M} N {ln.g.N} ldw {ln.g.ldw}")
                if ln.family == sp.WG_FAMILY_WIDE128:
                    wide128.append((case.name, ln.tag))
        for ns, plan in plans.items():                           # the knob changes the split count (and with it the folds planned), not the kernel
            sig = lambda launches: [(ln.tag, ln.family, ln.g.M, ln.g.N, ln.g.ldw) for ln in launches if ln.kind == KIND_WGRAD]
            assert sig(ed.wgrad_ops(plan)) == sig(base), (case.name, ns)
        n_fused = sum(ed.fused(ln) for ln in base)
        # exactly one per bf16 DCCRN plan whose first layer the spectrum kernels take (16, 32 or 64 channels: not ODD_KN's 8), none anywhere else
        on_spectrum = case.model == "DCCRN" and case.dtype == "bf16" and case.kn[0] in (16, 32, 64)
        assert n_fused == (1 if on_spectrum and ("ENC0_BNFUSE", "0") not in case.knobs else 0), (case.name, n_fused)
    for name in WANT:
        print(f"{name}: {seen.get(name)}")
    missing = [name for name in WANT if name not in seen]
    assert not missing, missing
    assert sorted(set(wide128)) == [("crn_wide", t) for t in (104, 105, 400, 401)] and len(wide128) == 6, wide128      # (both sub-pixel phases of 400 / 401)


def _fingerprint_tool():
    spec = importlib.util.spec_from_file_location("plan_fingerprint", os.path.join(ROOT, "tools", "plan_fingerprint.py"))
    fp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fp)
    return fp


def test_knob_unset_leaves_every_plan_where_it_was():
    """The descriptors of default plans in front of this knob (recorded fingerprints: every byte the C ABI exposes) and behind it."""
    fp = _fingerprint_tool()
    want = {}
    for line in open(os.path.join(ROOT, "profiles", "tuning_refactor_fingerprints.txt")):
        if not line.startswith("#"):
            name, parent, head = line.split()
            want[name] = head
    matrix = {name: (kw, kn) for name, kw, kn in fp.MATRIX}
    for name in ("bench_dccrn_bf16_C_b32_3s", "arm_base", "dccrn_bf16_small", "dccrn_fp32_small", "crn_bf16_mask", "fsn_bf16", "fsn_fp32", "arm_ENC0_BNFUSE=0"):
        kw, kn = matrix[name]
        base = fp.plan_bytes(kw, kn)
        assert fp.digest(base) == want[name], name
        knobs.set("WG_NSPLIT", "0")
        assert fp.plan_bytes(kw, kn) == base, name
        knobs.set("WG_NSPLIT", "3")
        moved = fp.plan_bytes(kw, kn)
        assert moved["bwd"] != base["bwd"], name
        knobs.unset("WG_NSPLIT")
        assert fp.plan_bytes(kw, kn) == base, name


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_knob_sets_the_split_count_of_every_weight_gradient(case):
    for ns in NSPLITS:
        plan = ed.make_plan(case, ns)
        need = 0
        for ln in ed.wgrad_ops(plan):
            if ln.kind != KIND_WGRAD:
                continue
            g = ln.g
            steps = (g.M + ROWS - 1) // ROWS
            if ns is not None:
                assert g.nsplit == min(ns, steps), (case.name, ns, ln.tag, g.nsplit, steps)
            assert 1 <= g.nsplit <= max(1, steps)
            assert g.w.off % 4 == 0
            need = max(need, g.w.off + 4 * g.nsplit * g.Npad * g.ldw)
        a, off, nb, dt = plan.buffer("gradpart")
        assert a == WS and need <= off + nb <= plan.arena_bytes[WS], (case.name, ns)          # every split's block lies inside the buffer


def _filled_state(case, ns):
    """(plan, launches, arenas after the fill) - the state every launch of the case starts from."""
    plan = ed.make_plan(case, ns)
    ar = plan.alloc_arenas("cpu")
    ed.fill(plan, ar)
    return plan, ed.wgrad_ops(plan), ar


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fill_meets_the_exact_sum_condition_and_the_fold_is_partition_free(case):
    """Per launch: the sum of |x * dy| over the rows of the longest split below 2^24 (over ALL rows at WG_NSPLIT = 1, which also bounds the fold); the
    simulator's partial sums are integers.  Then the folded gradient arena is the same bytes at every split count."""
    grads, worst = {}, 0.0
    for ns in NSPLITS:
        plan, launches, filled = _filled_state(case, ns)
        ar = [a.clone() for a in filled]
        for ln in launches:
            if ln.kind == KIND_WGRAD and not ed.fused(ln):
                bound = ed.exact_sum_bound(plan, ar, ln)
                worst = max(worst, bound)
                assert bound < ed.LIMIT, (case.name, ns, ln.tag, bound)
                assert bound <= 9 * ROWS * ed.rows_of_longest_split(ln.g), (case.name, ns, ln.tag, bound)      # |x|, |dy| <= 3
            sim_run(plan, PHASE_BWD, ar, ln.op, ln.op + 1)
            if ln.kind == KIND_WGRAD and not ed.fused(ln):
                part = ed.partials(plan, ar, ln.g)
                assert torch.equal(part, part.round()) and float(part.abs().max()) > 0, (case.name, ns, ln.tag)
        grads[ns] = ar[ed.GRAD].clone()
        assert float(grads[ns].abs().max()) > 0
    print(f"{case.name}: largest sum of |x * dy| over a split {worst:.0f} = {worst / ed.LIMIT:.4f} * 2^24")
    fed = _fed_by_fused(case)
    for ns in NSPLITS:
        same = grads[ns].view(torch.int32) == grads[1].view(torch.int32)
        assert bool((same | fed).all()), (case.name, ns, int((~(same | fed)).sum()))


def _fed_by_fused(case):
    plan, launches, filled = _filled_state(case, 1)
    return ed.fed_by_fused(plan, launches, filled, lambda ar, op: sim_run(plan, PHASE_BWD, ar, op, op + 1))


# ------------------------------------------------------------------------------------------------ planted faults
_operand, _typed = ed.operand, ed.typed


def _dy_row(g, ar, b, u, fo):
    o = b * g.y_bstride + u * g.y_tstride + fo * g.y_fstride + g.y_off
    return _typed(ar, g.y.arena, g.y.off, g.ydt)[o:o + g.N].float()


def _split_of(g, b, u, fo):
    tf = g.Tout * g.Fo
    q = u * g.Fo + fo
    per_item = g.xdt == 1 and (g.flags & 1)
    spb = (tf + ROWS - 1) // ROWS
    step = b * spb + q // ROWS if per_item else (b * tf + q) // ROWS
    nsteps = (g.M // tf) * spb if per_item else (g.M + ROWS - 1) // ROWS
    return step // ((nsteps + g.nsplit - 1) // g.nsplit)


def _sites(g, ar):
    """{fault name: (s, b, u, fo, j)} on WGRAD `g`: rows whose dy is not all zero, elements that the row really reads."""
    nb = g.M // (g.Tout * g.Fo)
    data = [s for s in range(g.nseg) if g.seg[s].src >= 0]
    shifted = [s for s in data if g.seg[s].dt < 0]
    longest = max(data, key=lambda s: g.seg[s].len)

    def live(s, b, u, fo, j):
        return _operand(g, s, b, u, fo, j) is not None and bool(_dy_row(g, ar, b, u, fo).abs().max() > 0)

    def first(cands):
        return next(c for c in cands if live(*c))
    frames = list(range(g.Tout // 2, g.Tout)) + list(range(g.Tout // 2))
    s0 = data[0]
    out = {
        "first valid bin": first((s0, b, u, fo, j) for fo in range(g.Fo) for j in range(g.seg[s0].len) for b in range(nb) for u in frames),
        "last valid bin": first((s0, b, u, fo, j) for fo in reversed(range(g.Fo)) for j in reversed(range(g.seg[s0].len)) for b in range(nb) for u in frames),
        "last row of a batch item": first((s, 0, g.Tout - 1, g.Fo - 1, j) for s in data for j in reversed(range(g.seg[s].len))),
        "last chunk of a run": first((longest, b, u, fo, g.seg[longest].len - 1) for b in reversed(range(nb)) for u in frames for fo in range(g.Fo // 2, g.Fo)),
    }
    if shifted:
        s = shifted[0]
        out["frame 0 behind a frame shift"] = first((s, b, -g.seg[s].dt, fo, j) for b in range(nb) for fo in range(g.Fo // 2, g.Fo) for j in range(g.seg[s].len))
    return out


FAULT_CASES = [("dccrn_small", 3), ("dccrn_small", None), ("crn_wide", 3), ("dccrn_small_fp32", 100000), ("fsn_64", 3)]


@pytest.mark.parametrize("name,ns", FAULT_CASES, ids=lambda v: str(v))
def test_planted_single_element_faults_are_flagged(name, ns):
    case = next(c for c in CASES if c.name == name)
    plan, launches, filled = _filled_state(case, ns)
    # the launches under test: the first conv weight gradient with a frame shift and more than one batch item (FullSubNet has no frame shift:
    # its first weight gradient with enough rows for three splits)
    conv = [ln for ln in launches if ln.kind == KIND_WGRAD and not ed.fused(ln) and ln.g.N >= 8 and ln.g.M >= 3 * ROWS]
    ln = next((c for c in conv if any(c.g.seg[s].dt < 0 and c.g.seg[s].src >= 0 for s in range(c.g.nseg)) and c.g.M // (c.g.Tout * c.g.Fo) > 1), conv[0])
    g = ln.g
    before = [a.clone() for a in filled]
    good = [a.clone() for a in filled]
    sim_run(plan, PHASE_BWD, good, ln.op, ln.op + 1)
    again = [a.clone() for a in filled]
    sim_run(plan, PHASE_BWD, again, ln.op, ln.op + 1)
    assert ed.compare_exact(plan, ln, before, good, again).ok
    sites = _sites(g, filled)
    assert case.model == "FullSubNet" or "frame 0 behind a frame shift" in sites
    for what, (s, b, u, fo, j) in sites.items():
        arena, off, idx = _operand(g, s, b, u, fo, j)
        bad_in = [a.clone() for a in filled]
        x = _typed(bad_in, arena, off, g.xdt)
        x[idx] += 1
        assert float(x[idx]) == float(_typed(filled, arena, off, g.xdt)[idx]) + 1
        sim_run(plan, PHASE_BWD, bad_in, ln.op, ln.op + 1)
        bad = [a.clone() for a in good]                          # the faulty run's OUTPUT on the sound input state
        bad[WS].copy_(bad_in[WS])
        x = _typed(bad, arena, off, g.xdt)
        x[idx] -= 1
        v = ed.compare_exact(plan, ln, before, good, bad)
        assert not v.ok and v.miss.startswith("gradpart: split") and v.stray == 0, (what, v)
        split, k = _split_of(g, b, u, fo), g.seg[s].koff + j
        d = ed.partials(plan, bad, g) - ed.partials(plan, good, g)
        assert torch.equal(d[split, :g.N, k], _dy_row(g, filled, b, u, fo)), (what, split, k)       # + 1 on x[m][k] adds dy[m][n] to part[split][n][k]
        first = d.flatten().nonzero()[0].item()
        sz = g.Npad * g.ldw
        assert f"split {first // sz} of {g.nsplit} n {first % sz // g.ldw} k {first % g.ldw}:" in v.miss, (what, v.miss)
    # a byte the "device" changes where the simulator changed nothing
    stray = [a.clone() for a in good]
    name_, a, off, nb, dt = next(r for r in ed._buffers(plan) if r[1] == WS and r[0] != "gradpart" and r[3] > 0)
    stray[WS].view(torch.uint8)[off + nb - 1] ^= 1
    v = ed.compare_exact(plan, ln, before, good, stray)
    assert not v.ok and v.stray == 1 and not v.miss, v


def test_float_sums_of_the_fused_launch_keep_opchecks_bar_and_nothing_else_does():
    """The one exception: inside the fused first-layer launch's partial sums a rounding-sized difference passes and 1 % of the largest element does not - for
    the launch itself and for the SPLITSUM that folds it; the same rounding-sized difference on any other launch's sums is a miss."""
    case = next(c for c in CASES if c.name == "dccrn_small")
    plan, launches, filled = _filled_state(case, 3)
    loose = ed.float_slices(launches)
    assert len(loose) == 1
    ar = [a.clone() for a in filled]
    for ln in launches:
        before = [a.clone() for a in ar]
        sim_run(plan, PHASE_BWD, ar, ln.op, ln.op + 1)
        if ln.kind == ed.KIND_UNPACK:
            continue
        touched = (ar[WS] != before[WS]).nonzero().flatten()
        lo, hi = int(touched[0]) // 4 * 4, int(touched[-1]) // 4 * 4 + 4
        inside = any(a <= lo and hi <= b for a, b, _ in loose)
        if ln.kind == KIND_WGRAD:
            assert inside == ed.fused(ln)
        if not (inside or ln.kind == KIND_WGRAD):
            continue                                             # (a SPLITSUM over many launches: the WGRADs carry the exact half of this test)
        out = ar[WS][lo:hi].view(torch.float32)
        big = int(out.abs().argmax())
        for scale, passes in ((1 + 2e-7, inside), (1.01, False)):
            dev = [a.clone() for a in ar]
            dev[WS][lo:hi].view(torch.float32)[big] *= scale
            v = ed.compare_exact(plan, ln, before, ar, dev, loose)
            assert v.ok == passes and v.stray == 0, (ln.tag, ln.kind, scale, v)
            assert ed.compare_exact(plan, ln, before, ar, dev).ok is False          # without the named slices: byte equality everywhere
