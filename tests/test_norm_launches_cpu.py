"""CPU side of the per-launch BatchNorm and ComplexBatchNorm tier (norm_data.py; the device's file is test_gpu_norm_launches.py): the descriptor mirrors, the host
simulator under the SAME driver and bars as the device (a second implementation of the float64 references, not their source), the exactness
conditions of the planted data measured on the float64 references alone, the coverage the cases' table names asserted from the descriptors, and the
comparator on planted faults - each on a copy of the simulator's result, each refused with the launch, the channel and the element named."""
import ctypes as C

import pytest
import torch

import norm_data as nd
import opcheck
from norm_data import (BF16, BN_APPLY, BN_BWD_APPLY, BN_BWD_FINALIZE, BN_BWD_REDUCE, BN_FINALIZE, CBN_APPLY, CBN_BWD_APPLY, CBN_BWD_FINALIZE,
                       CBN_BWD_REDUCE, CBN_FINALIZE, CBN_STATS, F32, GRAD, PARAM, WS)
from simutil import PHASE_BWD, PHASE_FWD, sim_run


def sim(plan, phase, arenas, op):
    sim_run(plan, phase, arenas, op, op + 1)


_results = {}


def results_of(case):
    if case.name not in _results:
        _results[case.name] = nd.run_case(case, "cpu", sim)
    return _results[case.name]


def test_a_moved_struct_layout_fails_loudly():
    """check_mirror() on every launch of every case (launches() runs it), and on a mirror with two fields swapped."""
    plan = nd.plan_of(nd.BY_NAME["small_bf16"])
    lns = nd.launches(plan)
    assert {ln.kind for ln in lns} | {ln.kind for ln in nd.launches(nd.plan_of(nd.BY_NAME["cbn_model_fp32"]))} == set(nd.MIRRORS)

    class Moved(C.Structure):                                    # BnApply with R in front of slope
        _fields_ = [("y", nd.Ptr), ("z", nd.Ptr), ("mean_invstd", nd.Ptr), ("gamma", nd.Ptr), ("beta", nd.Ptr), ("R", C.c_int64), ("slope", nd.Ptr),
                    ("C", C.c_int32), ("dt", C.c_int32)]
    ln = next(ln for ln in lns if ln.kind == BN_APPLY)
    with pytest.raises(AssertionError):
        nd.check_mirror(plan, ln._replace(d=Moved.from_buffer_copy(bytes(ln.d))))
    with pytest.raises(AssertionError):
        nd.check_mirror(plan, ln._replace(tag=ln.tag + 1))


@pytest.mark.parametrize("case", nd.CASES, ids=nd.case_id)
def test_the_simulator_passes_every_bar_and_the_data_is_exact(case):
    """The device's driver with the simulator in its place; per launch the conditions of byte equality, from the float64 reference alone: every
    expected value its own fp32 rounding, sum|terms| / (largest power of two dividing all terms) below the accumulator's limit; and what the data
    must contain: bn == 0 elements, bf16 ties and values that need rounding, a channel below 1 beside one above 2^12 times that."""
    res = results_of(case)
    bad = [line for line, (_, v, _, _) in zip(nd.report_lines(case, res), res) if not v.ok]
    assert not bad, "\n".join(bad[:20])
    for ln, v, notes, (inexact, sums) in res:
        where = (case.name, ln.tag, nd.KIND_NAMES[ln.kind])
        assert not inexact, where + (inexact,)
        for name, (cond, limit) in sums.items():
            assert cond < limit, where + (name, cond, limit)
        assert v.exact == (ln.kind in (BN_APPLY, BN_BWD_REDUCE, BN_BWD_FINALIZE, CBN_STATS, CBN_APPLY, CBN_BWD_REDUCE)
                           or (ln.kind == BN_FINALIZE and ln.d.mode == 1)), where
        if ln.kind == CBN_APPLY:
            assert notes["zeros"] > 0 and notes["small"] < 1 and notes["big"] > 64, where + (notes,)      # (34 rows seldom hold xr = xi = 8)
            assert ln.d.dt != BF16 or (notes["ties"] > 0 and notes["inexact_bf16"] >= notes["ties"]), where + (notes,)   # (h = 4: the ties are all that rounds)
            assert (notes["slope"] == 1.0) == case.name.startswith("cbn_alone"), where + (notes,)
        if ln.kind in (CBN_BWD_REDUCE, CBN_BWD_APPLY):
            assert notes["zeros"] > 0, where + (notes,)
        if ln.kind in (CBN_FINALIZE, CBN_BWD_FINALIZE) and "kinds" in notes:
            assert notes["kinds"] >= 4, where + (notes,)              # h = 4: the first four covariances; h >= 8: all five
        if ln.kind == BN_BWD_REDUCE:
            assert set(sums) == {"sum dbn", "sum dbn * xhat", "slope share"} and notes["zeros"] > 0, where + (notes,)
        if ln.kind == BN_APPLY:
            assert notes["zeros"] > 0 and notes["small"] < 1 and notes["big"] > 5e3 and notes["big"] > 4096 * notes["small"], where + (notes,)
            if ln.d.dt == BF16:
                assert notes["ties"] > 0 and notes["inexact_bf16"] > notes["ties"], where + (notes,)
        if ln.kind == BN_BWD_FINALIZE:
            assert notes["other_channels"] > 0, where                # slope shares in every channel, not only channel 0
        if ln.kind == BN_FINALIZE and ln.d.nblk >= 0 and ln.d.mode == 0:
            assert notes["var_const"] == 0 and notes["raw_negative"] < 0 and (notes["mean_big"], notes["var_big"]) == (1000.0, 1.0), where + (notes,)
            assert notes["unbiased"] == ln.d.count / (ln.d.count - 1) > 1, where
    zeros = [notes["zeros"] for ln, _, notes, _ in res if ln.kind == BN_BWD_REDUCE]
    assert not zeros or sum(zeros) >= 100, (case.name, zeros)       # elements with bn == 0 exactly: they take the a * bn branch and add bn * dz = 0


def _all():
    out = []
    for case in nd.CASES:
        plan = nd.plan_of(case)
        every = nd.launches(plan)
        out += [(case, ln, every) for ln in nd.select(case, every)]
    return out


def test_the_cases_contain_what_their_table_names():
    """From the descriptors alone: a later planner change must not empty a row of the table silently."""
    runs = _all()
    by = lambda name: [(ln, every) for c, ln, every in runs if c.name == name]
    kinds = lambda name, kind: [ln for ln, _ in by(name) if ln.kind == kind]
    # small_bf16: C 16 / 32 / 64 in bf16; forward finalizes one-level and two-level; nsub = 2 decoders, one of them two-level; backward 264 .. 9 rows;
    # decoder layers skip > 0 without dz1, encoder layers dz1 with skip 0; the first layer has no BN_BWD_APPLY
    fwd = kinds("small_bf16", BN_FINALIZE)
    assert [ln.d.nblk for ln in fwd if max(ln.d.nsub, 1) == 1] == [129, 65, 33, 17, 9, 5]
    assert {ln.d.C for ln in fwd} == {16, 32, 64} and {nd.chunks(ln) > 0 for ln in fwd} == {True, False}
    sub = [ln for ln in fwd if ln.d.nsub == 2]
    assert {ln.d.substride for ln in sub} == {16, 32, 64} and all(ln.d.Cpad >= 2 * ln.d.C for ln in sub) and any(nd.chunks(ln) > 0 and ln.d.nblk == 66 for ln in sub)
    red = kinds("small_bf16", BN_BWD_REDUCE)
    assert {ln.d.dt for ln in red} == {BF16} and max(ln.d.nblk for ln in red) == 264 and min(ln.d.nblk for ln in red) == 9
    assert sorted(ln.d.skip for ln in red if ln.d.dz1.arena < 0) == [8, 16, 32, 64, 128] and all(ln.d.skip == 0 for ln in red if ln.d.dz1.arena >= 0)
    assert any(ln.d.dz1.arena >= 0 for ln in red)
    first = min(ln.tag for ln, _ in by("small_bf16"))
    assert not [ln for ln in kinds("small_bf16", BN_BWD_APPLY) if ln.tag == first] and [ln for ln in kinds("small_bf16", BN_BWD_FINALIZE) if ln.tag == first]
    bfin = kinds("small_bf16", BN_BWD_FINALIZE)
    assert {nd.chunks(ln) > 0 for ln in bfin} == {True, False}
    # odd: C no power of two, row lanes that do not fill the workgroup (bn.hip: C / V chunk columns, 256 / (C / V) row lanes)
    for name, dt, v in (("odd_fp32", F32, 4), ("odd_bf16", BF16, 8)):
        red = kinds(name, BN_BWD_REDUCE)
        assert {ln.d.C for ln in red} == {8, 24, 40, 72, 136, 264} and {ln.d.dt for ln in red} == {dt}
        lanes = {ln.d.C: (256 // (ln.d.C // v), ln.d.C // v) for ln in red}
        assert lanes[24] == ((85, 3) if dt == BF16 else (42, 6)) and (dt == BF16 or lanes[264] == (3, 66)) and (dt == F32 or lanes[8] == (256, 1))
        assert any(ln.d.substride == 136 and ln.d.Cpad == 256 for ln in kinds(name, BN_FINALIZE))
        assert {ln.d.C for ln in kinds(name, BN_APPLY)} == {8, 24, 40, 72, 136, 264} == {ln.d.r.C for ln in kinds(name, BN_BWD_APPLY)}
    # c1024: the launches of the one layer with the most channels the LDS staging holds, in both dtypes
    for name, dt in (("c1024_fp32", F32), ("c1024_bf16", BF16)):
        assert sorted(ln.kind for ln, _ in by(name)) == sorted([BN_FINALIZE, BN_APPLY, BN_BWD_REDUCE, BN_BWD_FINALIZE, BN_BWD_APPLY])
        assert all(nd.channels(ln) == 1024 for ln, _ in by(name)) and kinds(name, BN_APPLY)[0].d.dt == dt
    # chunks17: 17 chunks forward (a second trip of the 16-wide gather), more than 32 backward; chunks64: the cap, with a short last chunk
    (f17,), (b17,) = kinds("chunks17", BN_FINALIZE), kinds("chunks17", BN_BWD_FINALIZE)
    assert nd.chunks(f17) == 17 and nd.chunks(b17) > 32 and {ln.kind for ln, _ in by("chunks17")} == {BN_FINALIZE, BN_APPLY, BN_BWD_REDUCE, BN_BWD_FINALIZE}
    ((b64, _),) = by("chunks64")
    r = b64.d.r
    assert b64.kind == BN_BWD_FINALIZE and r.rows_per_blk == max(64, (r.R + 2047) // 2048) and r.nblk == (r.R + r.rows_per_blk - 1) // r.rows_per_blk > 2016
    assert nd.chunks(b64) == nd.FIN_MAX_CHUNKS == 64
    per = (r.nblk + 63) // 64
    print(f"chunks64: {r.nblk} partial rows of {r.rows_per_blk}, {per} per chunk, the last chunk holds {r.nblk - 63 * per}")
    assert 0 < r.nblk - 63 * per < per
    # sync2: modes 1 and 2 in pairs, mode 2 with the all-rank count; eval: finalize from the running statistics
    modes = [(ln.d.mode, ln.d.count) for ln in kinds("sync2", BN_FINALIZE)]
    assert [m for m, _ in modes] == [1, 2] * 11 and all(b[1] == 2 * a[1] for a, b in zip(modes[::2], modes[1::2]))
    assert all(ln.d.nblk < 0 for ln in kinds("eval", BN_FINALIZE)) and len(kinds("eval", BN_FINALIZE)) == 11 and not kinds("eval", BN_BWD_REDUCE)
    # crn_fp32: the real-conv planner's descriptors
    assert {ln.d.nsub for ln in kinds("crn_fp32", BN_FINALIZE)} == {0} and {ln.d.C for ln in kinds("crn_fp32", BN_APPLY)} == {8, 16, 32}
    assert {ln.d.dt for ln in kinds("crn_fp32", BN_APPLY)} == {F32}
    # cbn_alone: every cbn.hip kernel at 330 rows (six 64-row blocks, the last of 10 rows) and at 34 rows, h = 4 .. 32, both dtypes, training and eval
    alone = [(c, ln) for c, ln, _ in runs if c.name.startswith("cbn_alone")]
    assert {(ln.d.C, ln.d.R, ln.d.dt) for _, ln in alone} == {(C_, R, dt) for C_ in (8, 24, 40, 64) for R in (330, 34) for dt in (F32, BF16)}
    assert {ln.kind for c, ln in alone if c.kw["training"]} == set(nd.CBN_FWD + nd.CBN_BWD)
    assert {ln.kind for c, ln in alone if not c.kw["training"]} == set(nd.CBN_FWD + nd.CBN_BWD) - {CBN_STATS}
    assert {(ln.d.nblk, ln.d.R - 64 * (ln.d.nblk - 1)) for _, ln in alone if ln.d.R == 330} == {(6, 10)}
    assert all(ln.d.slope.arena == nd.CONST for _, ln in alone)
    # cbn_model: skip > 0, dz1 and a slope parameter, in both dtypes
    for name, dt in (("cbn_model_bf16", BF16), ("cbn_model_fp32", F32)):
        red = kinds(name, CBN_BWD_REDUCE)
        assert {ln.d.dt for ln in red} == {dt} and {ln.d.C for ln in red} == {16, 32, 64} and all(ln.d.slope.arena == PARAM for ln in red)
        assert sorted(ln.d.skip for ln in red if ln.d.dz1.arena < 0) == [8, 16, 32, 64, 128] and any(ln.d.dz1.arena >= 0 and ln.d.skip == 0 for ln in red)
        assert len(kinds(name, CBN_FINALIZE)) == len(kinds(name, CBN_BWD_FINALIZE)) == len(kinds(name, CBN_BWD_APPLY)) == 11
    # every slope arm on every kind that reads the slope
    for kind in (CBN_APPLY, CBN_BWD_REDUCE, CBN_BWD_APPLY):
        assert {nd.slope_of(c, ln) for c, ln, _ in runs if ln.kind == kind and c.name.startswith("cbn_model")} == set(nd.SLOPES), kind
    for kind in (BN_APPLY, BN_BWD_REDUCE, BN_BWD_APPLY):
        assert {nd.slope_of(c, ln) for c, ln, _ in runs if ln.kind == kind} == set(nd.SLOPES), kind
    # a finalize of another chunk count runs between two of the same count
    order = nd.finalize_order([ln for ln, _ in by("small_bf16")])
    assert sum(nd.chunks(a) != nd.chunks(b) for a, b in zip(order, order[1:])) >= 8


# ------------------------------------------------------------------------------------------------ planted faults
SMALL = nd.BY_NAME["small_bf16"]
_bench = {}


def _simulated(case, pick):
    """(launch, planted, bench) with the simulator's result of the first launch of `case` that `pick` takes in bench.work."""
    if case.name not in _bench:
        _bench.clear()
        _bench[case.name] = nd.Bench(nd.plan_of(case), "cpu", sim)
    bench = _bench[case.name]
    ln = next(ln for ln in nd.select(case, nd.launches(nd.plan_of(case))) if pick(ln))
    pl = nd.run_one(case, ln, bench)
    assert nd.compare(case, ln, pl.fields, bench.ref, bench.work).ok
    return ln, pl, bench


def _refused(case, ln, pl, bench, channel=None, stray=0):
    v = nd.compare(case, ln, pl.fields, bench.ref, bench.work)
    bench.reset(pl, whole=True)
    assert not v.ok and v.stray == stray, v
    if stray == 0:
        assert f"{case.name} phase {ln.phase} op {ln.op} tag {ln.tag} {nd.KIND_NAMES[ln.kind]}" in v.miss and ("channel" in v.miss or "block" in v.miss), v.miss
        if channel is not None:
            assert f"channel {channel} " in v.miss, (channel, v.miss)
    return v


def _inputs(bench, r):
    """(y, dz0, dz1, mean, invstd, gamma, beta, slope) of BnBwdReduce / BnApply `r`, read back from the planted state."""
    y = nd.read(bench.ref, r.y.arena, r.y.off, r.R * r.C, r.dt).view(r.R, r.C)
    mi = nd.read(bench.ref, r.mean_invstd.arena, r.mean_invstd.off, 2 * r.C, F32)
    gamma, beta = nd.read(bench.ref, PARAM, r.gamma.off, r.C, F32), nd.read(bench.ref, PARAM, r.beta.off, r.C, F32)
    a = float(nd.read(bench.ref, PARAM, r.slope.off, 1, F32))
    dz0 = dz1 = None
    if hasattr(r, "dz0"):
        n0 = (r.R // r.rpb) * (r.rpb - r.skip)
        dz0 = nd.read(bench.ref, r.dz0.arena, r.dz0.off, n0 * r.C, r.dt).view(n0, r.C)
        dz1 = nd.read(bench.ref, r.dz1.arena, r.dz1.off, r.R * r.C, r.dt).view(r.R, r.C) if r.dz1.arena >= 0 else None
    return y, dz0, dz1, mi[:r.C], mi[r.C:], gamma, beta, a


def test_fault_parameters_of_the_next_channel_on_a_small_channel_only():
    """Refused per channel - and PASSED by opcheck.compare_op's buffer-wide bar: the gap this tier closes."""
    ln, pl, bench = _simulated(SMALL, lambda ln: ln.kind == BN_APPLY)
    d = ln.d
    y, _, _, mean, invstd, gamma, beta, a = _inputs(bench, d)
    c = nd.special_channels(d.C)[0]
    good = nd.read(bench.work, d.z.arena, d.z.off, d.R * d.C, d.dt).view(d.R, d.C)
    z = good.clone()
    z[:, c] = nd.ref_apply(y[:, c], mean[c + 1], invstd[c + 1], gamma[c + 1], beta[c + 1], a)
    nd.write(bench.work, d.z.arena, d.z.off, z.float().to(torch.bfloat16))
    err, own = opcheck.measure(good.reshape(-1), z.float().to(torch.bfloat16).double().reshape(-1), False)
    assert 0 < err < opcheck.tolerance(opcheck.BF16, "enc0.z", BN_APPLY, "bf16"), (err, own)
    _refused(SMALL, ln, pl, bench, channel=c)


def _reduce_fault(pick, faulty_dz=None, ge=False):
    ln, pl, bench = _simulated(SMALL, lambda ln: ln.kind == BN_BWD_REDUCE and pick(ln))
    d = ln.d
    y, dz0, dz1, mean, invstd, gamma, beta, a = _inputs(bench, d)
    dz = nd.upstream(d, dz0, dz1) if faulty_dz is None else faulty_dz(d, dz0, dz1)
    part, _, bn = nd.ref_reduce(d, y, dz, mean, invstd, gamma, beta, a, ge=ge)
    assert int((bn == 0).sum()) > 0
    nd.write(bench.work, d.part.arena, d.part.off, part.float())
    return _refused(SMALL, ln, pl, bench)


def test_fault_branch_test_ge_at_bn_zero():
    _reduce_fault(lambda ln: nd.slope_of(SMALL, ln) != 0.0, ge=True)


def test_fault_skip_offset_dropped():
    def no_skip(d, dz0, dz1):
        nb = d.R // d.rpb
        dz = torch.zeros(nb, d.rpb, d.C, dtype=torch.float64)
        dz[:, :d.rpb - d.skip] = dz0.view(nb, d.rpb - d.skip, d.C)
        return dz.view(d.R, d.C)
    _reduce_fault(lambda ln: ln.d.skip > 0, no_skip)


def test_fault_dz1_ignored():
    _reduce_fault(lambda ln: ln.d.dz1.arena >= 0, lambda d, dz0, dz1: nd.upstream(d, dz0, None))


def _bwd_finalize_fault(change):
    ln, pl, bench = _simulated(SMALL, lambda ln: ln.kind == BN_BWD_FINALIZE)
    r = ln.d.r
    part = nd.read(bench.ref, r.part.arena, r.part.off, r.nblk * 3 * (r.ldp or r.C), F32).view(r.nblk, 3, r.ldp or r.C)[:, :, :r.C]
    for f in pl.fields:
        v = f.exp.clone()
        change(f.name, v, part)
        nd.write(bench.work, f.arena, f.off, v.float())
    return _refused(SMALL, ln, pl, bench)


def test_fault_one_partial_row_left_out_of_a_finalize():
    def change(name, v, part):
        if name == "totals":
            v -= part[7, :2].reshape(-1)
    v = _bwd_finalize_fault(change)
    assert "totals" in v.miss


def test_fault_one_slope_share_dropped_from_a_channel_other_than_0():
    def change(name, v, part):
        if name == "dslope":
            assert float(part[3, 2, 5]) != 0
            v -= part[3, 2, 5]
    v = _bwd_finalize_fault(change)
    assert "dslope" in v.miss


def test_fault_a_sentinel_pad_column_added_in():
    """A forward finalize whose partial rows are wider than its channels: one pad column folded into channel 2's sum."""
    case = nd.BY_NAME["odd_bf16"]
    ln, pl, bench = _simulated(case, lambda ln: ln.kind == BN_FINALIZE and ln.d.Cpad > max(ln.d.nsub, 1) * ln.d.C)
    d = ln.d
    part = nd.read(bench.ref, d.part.arena, d.part.off, d.nblk * 2 * d.Cpad, F32).view(d.nblk, 2, d.Cpad)
    assert float(part[0, 0, d.Cpad - 1]) == float(torch.tensor(nd.SENTINEL).float())
    mean = pl.fields[0].exp.clone()
    mean[2] += float(part[0, 0, d.Cpad - 1]) / d.count
    nd.write(bench.work, pl.fields[0].arena, pl.fields[0].off, mean.float())
    _refused(case, ln, pl, bench, channel=2)


def test_fault_a_bf16_store_truncated_where_it_should_round():
    ln, pl, bench = _simulated(SMALL, lambda ln: ln.kind == BN_APPLY)
    f = pl.fields[0]
    bits = f.exp.float().view(torch.int32)
    cut = (bits & -65536).view(torch.float32).to(torch.bfloat16)                # the low 16 bits dropped: exact in bf16
    assert int((cut.double() != f.exp.float().to(torch.bfloat16).double()).sum()) > 0
    nd.write(bench.work, f.arena, f.off, cut)
    _refused(SMALL, ln, pl, bench)


def test_fault_one_stray_byte_behind_z():
    ln, pl, bench = _simulated(SMALL, lambda ln: ln.kind == BN_APPLY)
    f = pl.fields[0]
    end = f.off + f.exp.numel() * 2
    assert end < nd._u8(bench.work[WS]).numel()
    nd._u8(bench.work[WS])[end] ^= 1
    _refused(SMALL, ln, pl, bench, stray=1)


def test_fault_a_gradient_written_to_another_tensor():
    """The gradient arena outside the tensors a launch writes is stray too: dbeta stored at the first tensor of the arena, its own place untouched."""
    ln, pl, bench = _simulated(SMALL, lambda ln: ln.kind == BN_BWD_FINALIZE)
    f = next(f for f in pl.fields if f.name == "dbeta")
    assert f.off >= 4 * f.exp.numel() and not any(g.arena == GRAD and g.off < 4 * f.exp.numel() for g in pl.fields)
    nd.write(bench.work, GRAD, 0, f.exp.float())
    nd._u8(bench.work[GRAD])[f.off:f.off + 4 * f.exp.numel()].fill_(nd.BACKGROUND)
    v = nd.compare(SMALL, ln, pl.fields, bench.ref, bench.work)
    bench.reset(pl, whole=True)
    assert not v.ok and "dbeta" in v.miss and v.stray >= 4 * f.exp.numel() - 4, v


def test_phases_of_the_launch_kinds():
    lns = nd.launches(nd.plan_of(SMALL))
    assert {ln.phase for ln in lns if ln.kind in (BN_FINALIZE, BN_APPLY)} == {PHASE_FWD}
    assert {ln.phase for ln in lns if ln.kind in (BN_BWD_REDUCE, BN_BWD_FINALIZE, BN_BWD_APPLY)} == {PHASE_BWD}


def test_fault_cbn_coef_entry_off_by_sixteen_ulps_on_a_near_singular_channel():
    """Urr of the xi == xr channel moved by 2^-20 of its value - the size of error a covariance rounded to fp32 in front of the inverse square root
    would leave there - is refused, with the channel named."""
    case = nd.BY_NAME["cbn_model_fp32"]
    ln, pl, bench = _simulated(case, lambda ln: ln.kind == CBN_FINALIZE)
    f = next(f for f in pl.fields if f.name == "Urr")
    v = f.exp.clone()
    v[1] *= 1 + 2.0 ** -20                                        # complex channel 1: xi == xr
    nd.write(bench.work, f.arena, f.off, v.float())
    _refused(case, ln, pl, bench, channel=1)


def test_fault_cbn_slope_gradient_of_a_block_dropped():
    case = nd.BY_NAME["cbn_model_fp32"]
    ln, pl, bench = _simulated(case, lambda ln: ln.kind == CBN_BWD_FINALIZE)
    f = next(f for f in pl.fields if f.name == "dslope")
    h = ln.d.C // 2
    part = nd.read(bench.ref, ln.d.part.arena, ln.d.part.off, ln.d.nblk * 7 * h, F32).view(ln.d.nblk, 7, h)
    assert float(part[2, 6, 0]) != 0
    nd.write(bench.work, f.arena, f.off, (f.exp - part[2, 6, 0]).float())
    assert "dslope" in _refused(case, ln, pl, bench).miss
