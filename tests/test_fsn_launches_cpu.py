"""CPU side of the per-launch FullSubNet glue tier (fsn_launch_data.py; the device's file is test_gpu_fsn_launches.py): the descriptor mirror, the host
simulator under the SAME driver and bars as the device (a second implementation of the float64 references, not their source), the exactness
conditions of the planted data measured on the float64 references alone, the edges the planted states must reach, the coverage of launch_fsn's
kernels and paths by name, the closed forms of the backward launches against torch autograd in float64, and the comparator on planted faults - each on
a copy of the reference, written over the simulator's result, each refused with the launch and the field named."""
import ctypes as C
import math

import pytest
import torch

import fsn_launch_data as fd
import norm_data as nd
from fsn_launch_data import (ACT_NONE, ACT_RELU, ACT_RELU6, ACT_TANH, BF16, F32, FSN_ACT, FSN_IN, FSN_NORMBWD, FSN_NORMSTAT, FSN_OUT, FSN_OUT_BWD,
                             FSN_SBBUILD, FSN_SBBWD_APPLY, FSN_SBBWD_SUM, FSN_SBSUM, FSN_SCALE, WS)
from simutil import ARENA_COUNT, PHASE_BWD, PHASE_FWD, sim, sim_run


def simulate(plan, phase, arenas, op):
    sim_run(plan, phase, arenas, op, op + 1)


_results = {}


def results_of(case):
    if case.name not in _results:
        _results[case.name] = fd.run_case(case, "cpu", simulate)
    return _results[case.name]


def test_a_moved_struct_layout_fails_loudly():
    """check_mirror() on every launch of every case (launches() runs it), and on a mirror with two fields swapped."""
    kinds = set()
    for case in fd.CASES:
        kinds |= {ln.kind for ln in fd.launches(fd.plan_of(case))}
    assert kinds == set(fd.KIND_NAMES)
    plan = fd.plan_of(fd.BY_NAME["w12_fp32"])
    lns = fd.launches(plan)

    class Moved(C.Structure):                                    # Fsn with act and mode behind stat
        _fields_ = [("in_", fd.Ptr), ("out", fd.Ptr), ("aux", fd.Ptr), ("aux2", fd.Ptr), ("sums", fd.Ptr), ("B", C.c_int32), ("F", C.c_int32),
                    ("T", C.c_int32), ("TP", C.c_int32), ("FP", C.c_int32), ("NB", C.c_int32), ("LA", C.c_int32), ("dt", C.c_int32), ("stat", fd.Ptr),
                    ("act", C.c_int32), ("mode", C.c_int32), ("src", C.c_int32), ("ext", C.c_int32)]

    class Swapped(C.Structure):                                  # Fsn with aux and aux2 exchanged
        _fields_ = [(("aux2" if n == "aux" else "aux" if n == "aux2" else n), t) for n, t in fd.Fsn._fields_]
    assert C.sizeof(Moved) == C.sizeof(Swapped) == C.sizeof(fd.Fsn) == 144
    ln = next(ln for ln in lns if ln.kind == FSN_SBBWD_APPLY)
    for wrong in (Moved, Swapped):
        with pytest.raises(AssertionError):
            fd.check_mirror(plan, ln._replace(d=wrong.from_buffer_copy(bytes(ln.d))))
    with pytest.raises(AssertionError):
        fd.check_mirror(plan, ln._replace(tag=ln.tag + 1))
    # the helpers restated from sefd_desc.h, at the table's widths
    assert [(fd.fsn_nfb(ln.d), fd.fsn_w(ln.d), fd.fsn_wp(ln.d), fd.fsn_sbact(ln.d)) for ln in lns[:1]] == [(7, 12, 16, ACT_RELU6)]


def test_the_simulator_refuses_an_op_it_does_not_know():
    """hostsim_run returns nonzero on an unknown op kind (it used to print and carry on: anything compared with such a run was compared with
    garbage); and a plan with every knob away from its default runs whole, both phases - FSN_ACT among its ops."""
    case = fd.BY_NAME["w12_fp32"]
    plan = fd.plan_of(case)
    arenas = plan.alloc_arenas("cpu")
    ptrs = (C.c_void_p * ARENA_COUNT)(*[C.c_void_p(a.data_ptr()) for a in arenas])
    op = (C.c_int32 * (plan.lib.sefd_op_size() // 4))()
    op[0] = 9999
    assert sim().hostsim_run(C.cast(op, C.c_void_p), 0, 1, ptrs) != 0
    kinds = plan.op_kinds(PHASE_FWD)[0].tolist()
    assert FSN_ACT in kinds
    plan.io(arenas, "mag", (case.B, plan.NF, case.T)).copy_(torch.rand(case.B, plan.NF, case.T))
    sim_run(plan, PHASE_FWD, arenas)
    sim_run(plan, PHASE_BWD, arenas)
    assert bool(torch.isfinite(plan.io(arenas, "crm", (case.B, plan.NF, case.T, 2))).all())


def _kinks_reached(act, k, pre):
    """Each side of each kink and the kink itself; pre: a pre-activation (an OUTPUT of ReLU / ReLU6 has nothing below 0 or above 6)."""
    if act == ACT_RELU:
        return k["at0"] > 0 and k["gt0"] > 0 and (k["lt0"] > 0 or not pre)
    if act == ACT_RELU6:
        return k["at0"] > 0 and k["mid"] > 0 and k["at6"] > 0 and ((k["lt0"] > 0 and k["gt6"] > 0) or not pre)
    if act == ACT_TANH:
        return k["at0"] > 0 and k["neg"] > 0 and k["pos"] > 0 and (k["big"] > 0 or not pre)
    return True


@pytest.mark.parametrize("case", fd.CASES, ids=fd.case_id)
def test_the_simulator_passes_every_bar_and_the_data_is_exact_and_reaches_the_edges(case):
    """The device's driver with the simulator in its place; per launch the conditions of byte equality from the float64 reference alone; and what
    the planted states must contain."""
    res = results_of(case)
    bad = [line for line, (_, v, _, _) in zip(fd.report_lines(case, res), res) if not v.ok]
    assert not bad, "\n".join(bad[:20])
    assert [(ln.phase, ln.op) for ln, _, _, _ in res] == [(ln.phase, ln.op) for ln in fd.launches(fd.plan_of(case))]
    for ln, v, notes, (inexact, sums) in res:
        d, q, where = ln.d, fd.geom(ln.d), (case.name, ln.tag, fd.KIND_NAMES[ln.kind])
        assert not inexact, where + (inexact,)
        for name, (cond, limit) in sums.items():
            assert cond < limit, where + (name, cond, limit)
        if ln.kind in (FSN_IN, FSN_SBSUM, FSN_SBBWD_SUM):
            assert set(sums) == {"sums"}, where
        if ln.kind == FSN_SBBWD_APPLY and q.NFB > 1:
            assert set(sums) == {"gather s"}, where
        assert q.B == 1 or notes["differs"], where               # utterance b differs from utterance b + 1
        if q.LA and "la_fbo" in notes:
            assert notes["la_fbo"] > 0, where                    # the look-ahead frames carry full-band output ...
        if q.LA and "la_grad" in notes:
            assert notes["la_grad"] > 0, where                   # ... and gradients: the recurrences write there
        if ln.kind in (FSN_SCALE, FSN_SBBUILD):
            assert notes["pad"] == (q.FP - q.F if ln.kind == FSN_SCALE else q.WP - q.W), where
            assert notes["inexact"] > 0, where                   # values that need rounding: the bar is in use
        if ln.kind in (FSN_ACT, FSN_OUT, FSN_OUT_BWD):
            act = d.act if ln.kind == FSN_ACT else fd.fsn_sbact(d)
            assert act == ACT_NONE or _kinks_reached(act, notes["kinks"], True), where + (notes["kinks"],)
        if ln.kind == FSN_SBBWD_APPLY:
            assert d.act == ACT_NONE or _kinks_reached(d.act, notes["kinks"], False), where + (notes["kinks"],)
            # the reflect padding maps no position onto bins 0 and F - 1 themselves: they have nf + 1 regular sources and no mirrored one; every
            # other edge bin must receive a nonzero gradient from a mirrored source, in every frame of every utterance
            assert notes["edge"][0] > 0 and notes["edge"][q.F - 1] > 0 and notes["cnt"][0] == notes["cnt"][q.F - 1] == q.nfb + 1, where + (notes,)
            assert notes["mirrored"][0] == notes["mirrored"][q.F - 1] == 0, where
            if q.NFB > 1:
                for f in (1, q.nfb, q.F - 1 - q.nfb, q.F - 2):
                    assert notes["mirrored"][f] > 0, where + (f, notes["mirrored"])
                assert notes["cnt"][1] == notes["cnt"][q.F - 2] == q.NFB + 1, where + (notes["cnt"],)
        if ln.kind == FSN_NORMSTAT and d.mode == 2:
            # N - 1 against N moves the std by far more than its 2 ulps
            assert notes["unbiased"] - 1 > 64 * 2.0 ** -23, where + (notes,)
        if ln.kind == FSN_NORMSTAT and d.mode == 3:
            # frame 0 of the last row is constant: its running variance is 0, the stored std is sqrt(EPSILON)
            assert abs(notes["sd_const"] / math.sqrt(fd.EPSILON) - 1) < 1e-15, where + (notes,)
        exact = all(w == 0 for w in v.per.values())
        if ln.kind in (FSN_SCALE, FSN_SBBUILD, FSN_NORMBWD) or (ln.kind == FSN_SBBWD_APPLY and d.mode == 0):
            assert not exact, where                              # the derived bars measure something
        if ln.kind in (FSN_ACT, FSN_OUT) and (d.act if ln.kind == FSN_ACT else fd.fsn_sbact(d)) == ACT_TANH:
            assert v.tanh is not None and v.tanh <= 0.5 + 1e-9, where + (v.tanh,)    # the simulator: double tanh, one rounding


def test_every_kernel_and_path_of_launch_fsn_is_reached():
    """From the descriptors alone, with launch_fsn's predicates restated (fd.arms): every kernel of its struct-Fsn switch, each arm of the `if`s that
    pick a kernel (mode == 2, src, nfb > 1), the three paths of fsn_sbbuild_kernel and the k + 64 < W branch, each listed with the cases that reach
    it; and the rows of the issue's table."""
    reach = {}
    runs = [(c, ln) for c in fd.CASES for ln in fd.launches(fd.plan_of(c))]
    for c, ln in runs:
        for a in fd.arms(ln):
            reach.setdefault(a, []).append(c.name)
    for a in fd.ALL_ARMS:
        print(f"{a:60s} {' '.join(sorted(set(reach.get(a, []))))}")
    assert set(reach) == set(fd.ALL_ARMS) and all(reach[a] for a in fd.ALL_ARMS)
    by = lambda kind, pred=lambda c, ln: True: {c.name for c, ln in runs if ln.kind == kind and pred(c, ln)}
    assert {fd.fsn_w(ln.d) for c, ln in runs if c.name.startswith("w66")} == {66} and {fd.fsn_w(ln.d) for c, ln in runs if c.name.startswith("w126")} == {126}
    assert set(reach["fsn_normbwd_cum_kernel second lane pass (k + 64 < W)"]) == {"w66_fp32", "w66_bf16", "w126_fp32", "w126_bf16"}
    # the gather in mode 0 and behind FSN_NORMBWD of every other norm, offline_gaussian with NFB > 1 among them; F beyond one 256-thread pass
    assert {ln.d.mode for c, ln in runs if ln.kind == FSN_SBBWD_APPLY and fd.fsn_nfb(ln.d) > 1} == {0, 1, 2, 3}
    assert by(FSN_NORMBWD, lambda c, ln: ln.d.mode == 2 and fd.fsn_nfb(ln.d) > 1) == {"gauss_fb2_fp32", "gauss_fb2_bf16"}
    assert by(FSN_SBBWD_APPLY, lambda c, ln: ln.d.F > 256 and fd.fsn_nfb(ln.d) > 1) == {"f257_bf16"}
    # every cumulative and the gaussian norm in bf16 (ld_elem on a bf16 sb_in in the backward kernels; the element path with WP > W)
    assert {ln.d.mode for c, ln in runs if ln.kind == FSN_NORMBWD and ln.d.dt == BF16} == {1, 2, 3}
    assert by(FSN_SBBUILD, lambda c, ln: ln.d.dt == BF16 and ln.d.mode and fd.fsn_wp(ln.d) > fd.fsn_w(ln.d)) >= {"w66_bf16", "w126_bf16", "w2_bf16", "gauss_fb2_bf16"}
    # look-ahead 0, 1, 2, 3; T = 1; F == FP; W = 2 stored 8 wide; both activations of every kind in both heads
    assert {ln.d.LA for c, ln in runs} == {0, 1, 2, 3} and 1 in {ln.d.T for c, ln in runs}
    assert by(FSN_SCALE, lambda c, ln: ln.d.F == ln.d.FP) == {"w126_fp32", "w126_bf16"}
    assert by(FSN_SBBUILD, lambda c, ln: (fd.fsn_w(ln.d), fd.fsn_wp(ln.d)) == (2, 8)) == {"w2_bf16"}
    assert {ln.d.act for c, ln in runs} == {0, 1, 2, 3} == {fd.fsn_sbact(ln.d) for c, ln in runs}
    assert {ln.d.act for c, ln in runs if ln.kind == FSN_ACT} == {ACT_TANH, ACT_RELU6}
    assert {(ln.d.act, ln.d.mode == 0) for c, ln in runs if ln.kind == FSN_SBBWD_APPLY} >= {(ACT_TANH, True), (ACT_TANH, False), (ACT_RELU6, False), (ACT_RELU, True)}
    assert {ln.phase for c, ln in runs if ln.kind in (FSN_OUT_BWD, FSN_SBBWD_SUM, FSN_SBBWD_APPLY, FSN_NORMBWD)} == {PHASE_BWD}
    assert {ln.phase for c, ln in runs if ln.kind in (FSN_IN, FSN_SCALE, FSN_SBSUM, FSN_SBBUILD, FSN_NORMSTAT, FSN_ACT, FSN_OUT)} == {PHASE_FWD}


# ------------------------------------------------------------------------------------------------ the closed forms against autograd
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_TANH, ACT_RELU6])
@pytest.mark.parametrize("nsb,nfb", [(2, 0), (0, 0), (1, 2), (3, 7)])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_closed_forms_against_autograd_in_float64(mode, nsb, nfb, act):
    """fd.normbwd_closed, fd.apply_closed and fd.ref_gather against torch autograd through the reference-style forward
    act(pre) -> unfold, concatenate -> norm -> sum(g * y), on an unrounded self-consistent state: 1e-12 relative (max-abs over max-abs)."""
    gen = torch.Generator().manual_seed(1000 * mode + 100 * nsb + 10 * nfb + act)
    B, F, TP = 2, 9, 4
    NB, NFB = 2 * nsb + 1, 2 * nfb + 1
    q = fd.Geom(B, F, TP - 1, TP, 16, NB, 1, NFB, NB + NFB, (NB + NFB + 7) // 8 * 8, nsb, nfb)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    # W = 2 (nsb = nfb = 0): the running variance of frame 0 is (mag - fbo)^2 / 4, and where the two values nearly meet 1 / sd^2 amplifies the float64
    # rounding of autograd and closed form alike past any fixed bar; the magnitudes of that state sit 2 above the activations' range instead
    mag = (8.1 if nsb == nfb == 0 else 0.1) + 3 * rnd(B, 1, F, TP)
    pre = (8 * rnd(B, 1, F, TP) - 1).requires_grad_(True)        # on both sides of both kinks, on none of them
    fbo = fd.act_fwd(act, pre)
    fu = fd.ref_unfold(fbo, nfb).reshape(B, F, NFB, TP)
    fu.retain_grad()
    raw = torch.cat([fd.ref_unfold(mag, nsb).reshape(B, F, NB, TP), fu], 2)
    y = fd.ref_norm(raw, mode)
    g = 2 * rnd(B, F, q.W, TP) - 1
    (g * y).sum().backward()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    fbo_t = fd._pad_last(fbo.detach()[:, 0].permute(2, 0, 1), q.FP)
    gt, yt = fd.tm(g), fd.tm(y.detach())
    if mode == 0:
        mu = raw.detach().mean((1, 2, 3))
        Sm = (g * y.detach()).sum((1, 2, 3)) / (F * q.W * TP)
        cols = gt[..., NB:]
        v, _, _ = fd.apply_closed(q, 0, act, cols, fbo_t, mu, Sm)
    else:
        if mode == 2:
            stat = fd.ref_utt_stats(raw.detach())
        else:
            m, s = fd.ref_cum_stats(raw.detach())
            stat = (m.t().reshape(TP, B, F), s.t().reshape(TP, B, F))
        cols, _, _, _ = fd.normbwd_closed(mode, q, gt, yt, fd.tm(fu.detach()), stat)
        assert rel(cols, fd.tm(fu.grad)) < 1e-12
        late, _, _, _ = fd.normbwd_closed(mode, q, gt, yt, fd.tm(fu.detach()), stat, start=1)
        assert mode == 2 or rel(late, fd.tm(fu.grad)) > 1e-3     # the planted fault is one
        v, _, _ = fd.apply_closed(q, mode, act, cols, fbo_t)
    assert rel(v, pre.grad[:, 0].permute(2, 0, 1)) < 1e-12
    # the gather alone is the transpose of the reference's unfold
    x = rnd(B, 1, F, TP)
    c = rnd(TP, B, F, NFB)
    lhs = (fd.tm(fd.ref_unfold(x, nfb).reshape(B, F, NFB, TP)) * c).sum()
    assert abs(float(lhs - (fd.ref_gather(c, nfb) * x[:, 0].permute(2, 0, 1)).sum())) < 1e-12 * float(lhs.abs())


# ------------------------------------------------------------------------------------------------ planted faults
_bench = {}


def _simulated(case, pick):
    """(launch, planted, bench) with the simulator's result of the first launch of `case` that `pick` takes in bench.work."""
    if case.name not in _bench:
        _bench.clear()
        _bench[case.name] = nd.Bench(fd.plan_of(case), "cpu", simulate)
    bench = _bench[case.name]
    ln = next(ln for ln in fd.launches(fd.plan_of(case)) if pick(ln))
    pl = fd.run_one(case, ln, bench)
    assert fd.compare(case, ln, pl.fields, bench.ref, bench.work).ok
    return ln, pl, bench


def _refused(case, ln, pl, bench, field=None, stray=0):
    v = fd.compare(case, ln, pl.fields, bench.ref, bench.work)
    bench.reset(pl, whole=True)
    assert not v.ok and v.stray == stray, v
    if stray == 0:
        assert f"{case.name} phase {ln.phase} op {ln.op} tag {ln.tag} {fd.KIND_NAMES[ln.kind]}" in v.miss and "row" in v.miss and "column" in v.miss, v.miss
        assert field is None or f" {field}: row" in v.miss, (field, v.miss)
    return v


def _overwrite(bench, f, exp):
    nd.write(bench.work, f.arena, f.off, fd._store(f.dt, exp))


def _reference_fault(case, pick, fault, field):
    """The expectation of `fault` (fd.plant(.., fault=..): the same inputs, the wrong closed form) written over the simulator's result."""
    ln, pl, bench = _simulated(case, pick)
    wrong = fd.plant(case, ln, fault=fault)
    changed = 0
    for good, bad in zip(pl.fields, wrong.fields):
        changed += int((good.exp != bad.exp).sum())
        _overwrite(bench, good, bad.exp)
    assert changed > 0
    return _refused(case, ln, pl, bench, field=field)


@pytest.mark.parametrize("name", ["w12_fp32", "w66_bf16", "w126_fp32", "f257_bf16"])
def test_fault_a_dropped_high_mirror_source_in_the_gather(name):
    _reference_fault(fd.BY_NAME[name], lambda ln: ln.kind == FSN_SBBWD_APPLY, "drop_high", "d_fb")


@pytest.mark.parametrize("name", ["w12_fp32", "w12_bf16", "f257_bf16"])
def test_fault_cnt_off_by_one_at_bin_0(name):
    v = _reference_fault(fd.BY_NAME[name], lambda ln: ln.kind == FSN_SBBWD_APPLY, "cnt0", "d_fb")
    assert " column 0 " in v.miss


@pytest.mark.parametrize("name", ["w2_bf16", "gauss_fb2_fp32"])
@pytest.mark.parametrize("src", [0, 1])
def test_fault_n_instead_of_n_minus_1_in_the_gaussian_std(name, src):
    _reference_fault(fd.BY_NAME[name], lambda ln: ln.kind == FSN_NORMSTAT and ln.d.src == src, "std_n", "std")


@pytest.mark.parametrize("name", ["w66_fp32", "w126_bf16", "cumlap_fb1_bf16"])
def test_fault_a_suffix_sum_started_at_t_plus_1(name):
    _reference_fault(fd.BY_NAME[name], lambda ln: ln.kind == FSN_NORMBWD, "suffix_late", "d_fb_pre")


@pytest.mark.parametrize("name", ["w12_fp32", "cumlap_fb1_bf16"])
def test_fault_the_relu6_derivative_open_at_6(name):
    _reference_fault(fd.BY_NAME[name], lambda ln: ln.kind == FSN_OUT_BWD, "relu6_open", "d_sbo")


@pytest.mark.parametrize("name,kind", [("w2_bf16", FSN_SBBUILD), ("w12_bf16", FSN_SBBUILD), ("w12_fp32", FSN_SCALE), ("w66_bf16", FSN_SBBWD_APPLY)])
def test_fault_a_nonzero_pad_column(name, kind):
    """The smallest bf16 / fp32 subnormal in ONE pad column, and a negative zero: the pad columns are held to zero BYTES."""
    case = fd.BY_NAME[name]
    for bits in (1, -32768 if case.dtype == "bf16" else -2 ** 31):
        ln, pl, bench = _simulated(case, lambda ln: ln.kind == kind)
        f = pl.fields[0]
        e = f.C - 1 + 3 * f.C                                    # the last pad column of row 3
        assert float(f.exp[e]) == 0 and float(f.tol[e] if f.tol is not None else 0) == 0
        es = 2 if f.dt == BF16 else 4
        cell = nd._u8(bench.work[f.arena])[f.off + e * es:f.off + (e + 1) * es].view(torch.int16 if es == 2 else torch.int32)
        assert int(cell) == 0
        cell.fill_(bits)
        v = _refused(case, ln, pl, bench, field=f.name)
        assert f" column {f.C - 1} " in v.miss


@pytest.mark.parametrize("name", ["w12_fp32", "w2_bf16", "gauss_fb2_bf16"])
def test_fault_t_minus_la_off_by_one_frame(name):
    """FSN_OUT_BWD with the gradient one frame late (zeros up to t = LA), FSN_OUT reading frame t + LA - 1."""
    case = fd.BY_NAME[name]
    ln, pl, bench = _simulated(case, lambda ln: ln.kind == FSN_OUT_BWD)
    f, q = pl.fields[0], fd.geom(ln.d)
    exp = f.exp.view(q.TP, -1)
    late = torch.zeros_like(exp)
    late[1:] = exp[:-1]
    assert not torch.equal(late, exp)
    _overwrite(bench, f, late.reshape(-1))
    _refused(case, ln, pl, bench, field="d_sbo")
    if q.LA:                                                     # FSN_OUT: the frame in front of the look-ahead offset
        ln, pl, bench = _simulated(case, lambda ln: ln.kind == FSN_OUT)
        f = pl.fields[0]
        sbo = nd.read(bench.ref, ln.d.in_.arena, ln.d.in_.off, q.TP * q.B * q.F * 2, F32).view(q.TP, q.B, q.F, 2)
        early = fd.act_fwd(fd.fsn_sbact(ln.d), sbo[q.LA - 1:q.TP - 1]).permute(1, 2, 0, 3).contiguous()
        _overwrite(bench, f, early.reshape(-1))
        _refused(case, ln, pl, bench)


@pytest.mark.parametrize("name", ["w12_bf16", "w126_fp32"])
def test_fault_a_stray_write_one_element_past_d_fb(name):
    case = fd.BY_NAME[name]
    ln, pl, bench = _simulated(case, lambda ln: ln.kind == FSN_SBBWD_APPLY)
    f = pl.fields[0]
    es = 2 if f.dt == BF16 else 4
    end = f.off + f.exp.numel() * es
    assert end + es <= nd._u8(bench.work[WS]).numel()
    nd._u8(bench.work[WS])[end:end + es] = 0                      # a zero where the background was: one element past the buffer
    _refused(case, ln, pl, bench, stray=es)


def test_fault_a_read_of_the_unused_pad_columns_of_d_sb_in_would_show():
    """The pad columns of d_sb_in stay background (1.5e13): the planted state itself, read back."""
    case = fd.BY_NAME["w12_fp32"]
    ln, pl, bench = _simulated(case, lambda ln: ln.kind == FSN_SBBWD_SUM)
    q = fd.geom(ln.d)
    dsb = nd.read(bench.ref, ln.d.in_.arena, ln.d.in_.off, q.TP * q.B * q.F * q.WP, F32).view(-1, q.WP)
    assert bool((dsb[:, q.W:] == fd.BG32).all()) and float(dsb[:, :q.W].abs().max()) <= 3
    bench.reset(pl, whole=True)
