"""Per-launch float64 references for the normalisation launches (a plain module, not a conftest): the cases, the descriptor mirrors, the planted
states, the references and the per-channel comparator shared by test_norm_launches_cpu.py (the simulator as the device, the data conditions, the
coverage by name, planted faults) and test_gpu_norm_launches.py (the device).

BatchNorm2d + PReLU runs as BN_FINALIZE, BN_APPLY, BN_BWD_REDUCE, BN_BWD_FINALIZE and BN_BWD_APPLY (csrc/bn.hip, the finalize kernels in
csrc/kernels.hip).  Every launch runs ALONE from a state planted straight into the buffers its descriptor names - no GEMM runs - and the expected
result is computed here, in float64 with torch, from the descriptor's fields and the planted inputs: neither the host simulator nor any product code
has a part in it.  The comparison is per element; every byte outside the launch's outputs - other buffers, the gradient and state arenas outside the
tensors it writes, the bytes between tensors - is a stray byte (the arenas' background is the byte 0x55: 1.5e13 in either dtype, so a read outside
the planted inputs shows too).

The kernels are compiled with FMA contraction, so the data is DYADIC: every fp32 intermediate is exact in any order and under any contraction, and
the bar is byte equality (conditions() measures that on the float64 reference alone: every expected value equals its fp32 rounding, and for a sum
sum|terms| / (largest power of two dividing all terms) < 2^24).  Two profiles:
  wide   (BN_APPLY, BN_BWD_APPLY): y integers in -8 .. 8, mean integers in -4 .. 4, invstd 2^-6 .. 2^6, gamma +-2^-3 .. 2^3;
  narrow (BN_BWD_REDUCE): y in -3 .. 3, mean in -2 .. 2, invstd and |gamma| in {1/2, 1, 2}, dz0 / dz1 integers in -3 .. 3;
both with beta in quarters within -2 .. 2, one channel with gamma 0, one constant channel, and the layer's slope one of 0.25, -0.5, 0, 2 (SLOPES, by
launch).  The wide profile adds a channel whose |z| stays below 1, one that reaches 5e3, and one (invstd 64, gamma 4, beta 1, mean 0) whose values
257, 259, .. are exact ties of the bf16 rounding.

Bars by launch:
  BN_APPLY         z byte-equal to the float64 value as fp32, or rounded to nearest even to bf16;
  BN_BWD_REDUCE    rows 0 and 1 of every partial block byte-equal per channel; row 2 through its sum over the channels (the kernel puts a block's
                   share in channel 0, a GEMM epilogue one per channel: the contract is their sum);
  BN_BWD_FINALIZE  totals, dgamma, dbeta, dslope byte-equal (dyadic partial rows at the layer's pitch, sentinel pad columns, slope shares in EVERY
                   channel);
  BN_FINALIZE      mean byte-equal (integer sums are exact in double, one division, one rounding to fp32); invstd, running_mean and running_var at
                   most 1 fp32 ulp: their double expressions may be contracted, and a difference in the last bit of the double can move the fp32
                   rounding by one.  Mode 1 (SyncBN: partials -> fp64 totals) byte-equal doubles.  Eval (nblk < 0): mean a copy, invstd 3 ulps
                   (a float add, sqrtf and a division round once each);
  BN_BWD_APPLY     not exact (totals * (float)(1 / count) is not dyadic): N_ROUNDINGS * 2^-24 * |gamma * invstd| * (|dbn| + |t0| + |xhat * t1|) per
                   element, + half a bf16 ulp of the expected value in bf16.

ComplexBatchNorm (csrc/cbn.hip: CBN_STATS, CBN_FINALIZE, CBN_APPLY, CBN_BWD_REDUCE, CBN_BWD_FINALIZE, CBN_BWD_APPLY) the same way, on the module alone
(cbn_alone_*: the constant slope 1, where z must equal the affine map) and inside a DCCRN (cbn_model_*: skip > 0, dz1, a slope parameter):
  CBN_STATS        integer y: the five sums of every block byte-equal;
  CBN_APPLY        planted coef with dyadic Z, b': z byte-equal (fp32, or rounded to nearest even to bf16);
  CBN_BWD_REDUCE   dyadic coef, integer dz: six sums per complex channel byte-equal, row 6 through its sum;
  CBN_FINALIZE     planted partial sums whose covariance is, by complex channel, well-conditioned / xi == xr (singular up to eps) / xi identically 0 /
                   both parts constant / mean 1000 with variance 1 (100 where one partial row has to hold the sum): all 14 coef rows against the float64
                   closed form of the reference module (inv_sqrt_2x2), 2 fp32 ulps of the element, sums of terms that may cancel (Z = W U,
                   b' = B - Z M) 2 * 2^-24 * sum|terms|; the running statistics by the reference's rule (lerp, biased, without eps), 4 ulps of the
                   larger of old and new value;
  CBN_BWD_FINALIZE dB and dslope byte-equal (dyadic sums), dW and the coefb rows at the same bars; the expected dV is torch autograd in float64 through
                   phi(V) = sum(dZ * (W U(V))) at the same five covariances (cbn_dv) - not a transcription of the kernel's chain, which serves for the
                   bar's sum|terms| alone (cbn_dv_abs).  The planted slope shares sit in column 0 of row 6, where cbn_bwd_reduce_kernel leaves them
                   (no other kernel writes these rows);
  CBN_BWD_APPLY    N_ROUNDINGS_CBN * 2^-24 * the sum of the absolute terms of each output, + half a bf16 ulp in bf16."""
import ctypes as C
import zlib
from collections import namedtuple

import torch

from simutil import PHASE_BWD, PHASE_FWD, Plan

WS, PARAM, GRAD, STATE, CONST, IO = range(6)                      # sefd_amd.plan ARENA_*
CHECKED = (WS, GRAD, STATE, IO)                                   # the arenas a launch may write
F32, BF16, F64 = 0, 1, 2                                          # dtype codes (0, 1: sefd_desc.h DType)
# sefd_desc.h OpKind
BN_FINALIZE, BN_APPLY, BN_BWD_REDUCE, BN_BWD_APPLY, BN_BWD_FINALIZE = 5, 6, 7, 8, 21
CBN_STATS, CBN_FINALIZE, CBN_APPLY, CBN_BWD_REDUCE, CBN_BWD_FINALIZE, CBN_BWD_APPLY = 42, 43, 44, 45, 46, 47
KIND_NAMES = {BN_FINALIZE: "BN_FINALIZE", BN_APPLY: "BN_APPLY", BN_BWD_REDUCE: "BN_BWD_REDUCE", BN_BWD_APPLY: "BN_BWD_APPLY",
              BN_BWD_FINALIZE: "BN_BWD_FINALIZE", CBN_STATS: "CBN_STATS", CBN_FINALIZE: "CBN_FINALIZE", CBN_APPLY: "CBN_APPLY",
              CBN_BWD_REDUCE: "CBN_BWD_REDUCE", CBN_BWD_FINALIZE: "CBN_BWD_FINALIZE", CBN_BWD_APPLY: "CBN_BWD_APPLY"}
CBN_FWD, CBN_BWD = (CBN_STATS, CBN_FINALIZE, CBN_APPLY), (CBN_BWD_REDUCE, CBN_BWD_FINALIZE, CBN_BWD_APPLY)
# fp32 roundings on the longest path of cbn_bwd_apply_kernel (cbn.hip): a * dz [1], - mean(dbn) [2], Z * . [3] and three additions [4 .. 6]
# (x - M, q * ., the additions: 5), + 1 for the second order as N_ROUNDINGS has it
N_ROUNDINGS_CBN = 7
OP_HEADER = 16                                                    # Op: kind, tag, lane, join, then the descriptor union
LIMIT = 1 << 24
BACKGROUND = 0x55
SENTINEL = 1e30                                                   # pad columns of planted partial rows: must not leak into any channel
SLOPES = (0.25, -0.5, 0.0, 2.0)
# fp32 roundings on the longest path of bn_bwd_apply_kernel_v (bn.hip): inv_n = (float)(1 / count) [1], st = tot * inv_n [2], y - mean [3],
# * invstd [4], xh * t1 [5], dbn - t0 [6], - xh * t1 [7], gamma * invstd [8], the final product [9]; contraction only removes some
N_ROUNDINGS = 9
FIN_TWO_LEVEL, FIN_ROWS_PER_CHUNK, FIN_MAX_CHUNKS = 64, 32, 64      # kernels.hip fin_two_level: nblk >= 64; chunks = min(64, (nblk + 31) / 32)


class Ptr(C.Structure):
    _fields_ = [("arena", C.c_int32), ("pad_", C.c_int32), ("off", C.c_int64)]


class BnFinalize(C.Structure):                                    # sefd_desc.h BnFinalize
    _fields_ = [("part", Ptr), ("mean_invstd", Ptr), ("running_mean", Ptr), ("running_var", Ptr), ("nblk", C.c_int32), ("C", C.c_int32),
                ("Cpad", C.c_int32), ("mode", C.c_int32), ("count", C.c_double), ("eps", C.c_float), ("momentum", C.c_float), ("totals", Ptr),
                ("nsub", C.c_int32), ("substride", C.c_int32)]


class BnApply(C.Structure):                                       # sefd_desc.h BnApply
    _fields_ = [("y", Ptr), ("z", Ptr), ("mean_invstd", Ptr), ("gamma", Ptr), ("beta", Ptr), ("slope", Ptr), ("R", C.c_int64), ("C", C.c_int32),
                ("dt", C.c_int32)]


class BnBwdReduce(C.Structure):                                   # sefd_desc.h BnBwdReduce
    _fields_ = [("y", Ptr), ("dz0", Ptr), ("dz1", Ptr), ("mean_invstd", Ptr), ("gamma", Ptr), ("beta", Ptr), ("slope", Ptr), ("part", Ptr),
                ("R", C.c_int64), ("C", C.c_int32), ("dt", C.c_int32), ("nblk", C.c_int32), ("rows_per_blk", C.c_int32), ("rpb", C.c_int64),
                ("skip", C.c_int32), ("ldp", C.c_int32)]


class BnBwdApply(C.Structure):                                    # sefd_desc.h BnBwdApply
    _fields_ = [("r", BnBwdReduce), ("totals", Ptr), ("dy", Ptr), ("dgamma", Ptr), ("dbeta", Ptr), ("dslope", Ptr), ("count", C.c_double)]


class CbnFwd(C.Structure):                                        # sefd_desc.h CbnFwd
    _fields_ = [("y", Ptr), ("z", Ptr), ("part", Ptr), ("coef", Ptr), ("W", Ptr * 3), ("Bv", Ptr * 2), ("slope", Ptr), ("RM", Ptr * 2),
                ("RV", Ptr * 3), ("R", C.c_int64), ("C", C.c_int32), ("dt", C.c_int32), ("nblk", C.c_int32), ("rows_per_blk", C.c_int32),
                ("training", C.c_int32), ("mode", C.c_int32), ("count", C.c_double), ("eps", C.c_float), ("momentum", C.c_float),
                ("totals", Ptr)]


class CbnBwd(C.Structure):                                        # sefd_desc.h CbnBwd
    _fields_ = [("y", Ptr), ("dz0", Ptr), ("dz1", Ptr), ("dy", Ptr), ("coef", Ptr), ("coefb", Ptr), ("part", Ptr), ("W", Ptr * 3),
                ("slope", Ptr), ("dW", Ptr * 3), ("dB", Ptr * 2), ("dslope", Ptr), ("R", C.c_int64), ("rpb", C.c_int64), ("C", C.c_int32),
                ("dt", C.c_int32), ("nblk", C.c_int32), ("rows_per_blk", C.c_int32), ("skip", C.c_int32), ("mode", C.c_int32),
                ("count", C.c_double), ("totals", Ptr)]


MIRRORS = {BN_FINALIZE: BnFinalize, BN_APPLY: BnApply, BN_BWD_REDUCE: BnBwdReduce, BN_BWD_APPLY: BnBwdApply, BN_BWD_FINALIZE: BnBwdApply,
           CBN_STATS: CbnFwd, CBN_FINALIZE: CbnFwd, CBN_APPLY: CbnFwd, CBN_BWD_REDUCE: CbnBwd, CBN_BWD_FINALIZE: CbnBwd, CBN_BWD_APPLY: CbnBwd}

Launch = namedtuple("Launch", "phase op kind tag d")


# ------------------------------------------------------------------------------------------------ cases
SMALL_KN, ODD_KN, C1024_KN = (16, 32, 32, 64, 64, 64), (8, 24, 40, 72, 136, 264), (16, 32, 32, 64, 64, 1024)
# keep: which launches of the plan the case runs (select())
Case = namedtuple("Case", "name model B L kn ru dtype kw keep", defaults=({}, "all"))
CASES = [
    Case("small_bf16", "DCCRN", 3, 4000, SMALL_KN, 128, "bf16"),
    Case("odd_fp32", "DCCRN", 2, 1000, ODD_KN, 192, "fp32"),
    Case("odd_bf16", "DCCRN", 2, 1000, ODD_KN, 192, "bf16"),
    Case("c1024_fp32", "DCCRN", 1, 800, C1024_KN, 128, "fp32", {}, "c1024"),
    Case("c1024_bf16", "DCCRN", 1, 800, C1024_KN, 128, "bf16", {}, "c1024"),
    Case("chunks17", "DCCRN", 4, 13000, SMALL_KN, 128, "bf16", {}, "first"),
    Case("chunks64", "DCCRN", 8, 13000, SMALL_KN, 128, "bf16", {}, "first_bwd_finalize"),
    Case("sync2", "DCCRN", 3, 4000, SMALL_KN, 128, "bf16", dict(bn_world=2), "finalize"),
    Case("eval", "DCCRN", 3, 4000, SMALL_KN, 128, "bf16", dict(training=False), "forward"),
    Case("crn_fp32", "CRN", 2, 1000, SMALL_KN, 128, "fp32"),                      # (the CRN halves kernel_num: C 8 / 16 / 32)
    # ComplexBatchNorm inside a model: skip > 0, dz1 and a real PReLU slope parameter
    Case("cbn_model_bf16", "DCCRN", 3, 4000, SMALL_KN, 128, "bf16", dict(use_cbn=True)),
    Case("cbn_model_fp32", "DCCRN", 1, 800, SMALL_KN, 128, "fp32", dict(use_cbn=True)),
]
# ComplexBatchNorm on its own (the constant slope 1): B 2, S = 165 (330 rows: six 64-row blocks, the last of 10 rows) and S = 17
CASES += [Case(f"cbn_alone_c{c}_s{S}_{dt}_{'train' if tr else 'eval'}", "ComplexBatchNorm", 2, S, (), 0, dt, dict(training=tr, cbn=dict(num_features=c)))
          for c in (8, 24, 40, 64) for S in (165, 17) for dt in ("fp32", "bf16") for tr in (True, False)]
BY_NAME = {c.name: c for c in CASES}


def case_id(c):
    return c.name


_plans = {}


def plan_of(case):
    """The plan of `case`, built once per process."""
    if case.name not in _plans:
        if case.model == "ComplexBatchNorm":
            _plans[case.name] = Plan(case.B, case.L, act_dtype=case.dtype, model=case.model, **case.kw)
        else:
            _plans[case.name] = Plan(case.B, case.L, masking_mode="E", kernel_num=case.kn, rnn_units=case.ru, act_dtype=case.dtype, model=case.model, **case.kw)
    return _plans[case.name]


def _buffers(plan):
    return [(n,) + plan.buffer(n) for n in plan.buffer_names()]


def buffer_at(plan, ptr):
    """(name, arena, offset, bytes, dtype code) of the named buffer that holds the first byte of `ptr`."""
    for r in _buffers(plan):
        if r[1] == ptr.arena and r[2] <= ptr.off < r[2] + r[3]:
            return r
    raise AssertionError(("a descriptor pointer outside every named buffer: the mirror's layout moved?", ptr.arena, ptr.off))


def _esize(dt):
    return {F32: 4, BF16: 2, F64: 8}[dt]


def _tdtype(dt):
    return {F32: torch.float32, BF16: torch.bfloat16, F64: torch.float64}[dt]


def _table_entry(plan, table, arena, ptr, numel, what):
    """`ptr` must be the first element of a tensor of `table` (plan.params / plan.state) with `numel` elements, in `arena`."""
    assert ptr.arena == arena and ptr.off % 4 == 0, (what, ptr.arena, ptr.off)
    hit = [n for n, (off, shape) in table.items() if off * 4 == ptr.off]
    assert hit, (what, "points at no tensor of the plan: the mirror's layout moved?", ptr.off)
    n = 1
    for s in table[hit[0]][1]:
        n *= s
    assert n == numel, (what, hit[0], n, numel)
    return hit[0]


def check_mirror(plan, ln):
    """A moved struct layout fails here: the op header against op_info's kind and tag, every pointer against the named buffer / parameter / state
    tensor it must fall into, R * C * elementsize against the size of the buffer that holds y."""
    o = plan.op_info(ln.phase, ln.op)
    assert (o["kind"], o["tag"]) == (ln.kind, ln.tag)
    d = ln.d
    if ln.kind in CBN_FWD + CBN_BWD:
        return _check_cbn_mirror(plan, ln)
    if ln.kind == BN_FINALIZE:
        assert 8 <= d.C <= d.Cpad and d.count >= 1 and abs(d.eps - 1e-5) < 1e-9 and abs(d.momentum - 0.1) < 1e-6 and d.mode in (0, 1, 2), "BnFinalize layout moved"
        assert buffer_at(plan, d.mean_invstd)[3] == 2 * d.C * 4, "BnFinalize layout moved: mean_invstd"
        if d.nblk >= 0:
            name, _, off, nb, _ = buffer_at(plan, d.part)
            assert d.part.off - off + 4 * d.nblk * 2 * d.Cpad <= nb, ("BnFinalize layout moved: partial rows", name)
            assert max(d.nsub, 1) * max(d.substride, d.C) <= d.Cpad or d.nsub <= 1
        if d.running_mean.arena >= 0:
            _table_entry(plan, plan.state, STATE, d.running_mean, d.C, "running_mean")
            _table_entry(plan, plan.state, STATE, d.running_var, d.C, "running_var")
        if d.mode:
            assert buffer_at(plan, d.totals)[3] >= 2 * d.C * 8
        return
    r = d if ln.kind in (BN_APPLY, BN_BWD_REDUCE) else d.r
    es = _esize(r.dt)
    assert r.dt in (F32, BF16) and r.C >= 8 and r.R >= 1
    assert buffer_at(plan, r.y)[3] == r.R * r.C * es, f"{KIND_NAMES[ln.kind]} layout moved: R * C * elementsize is not the size of y's buffer"
    assert buffer_at(plan, r.mean_invstd)[3] == 2 * r.C * 4
    _table_entry(plan, plan.params, PARAM, r.gamma, r.C, "gamma")
    _table_entry(plan, plan.params, PARAM, r.beta, r.C, "beta")
    _table_entry(plan, plan.params, PARAM, r.slope, 1, "slope")
    if ln.kind == BN_APPLY:
        assert buffer_at(plan, d.z)[3] == r.R * r.C * es and d.z.off == buffer_at(plan, d.z)[2]
        return
    assert r.R % r.rpb == 0 and 0 <= r.skip < r.rpb and r.rows_per_blk >= 64
    assert buffer_at(plan, r.dz0)[3] == (r.R // r.rpb) * (r.rpb - r.skip) * r.C * es, "BnBwdReduce layout moved: dz0"
    if r.dz1.arena >= 0:
        assert buffer_at(plan, r.dz1)[3] == r.R * r.C * es, "BnBwdReduce layout moved: dz1"
    name, _, off, nb, _ = buffer_at(plan, r.part)
    assert r.part.off - off + 4 * r.nblk * 3 * (r.ldp or r.C) <= nb, ("BnBwdReduce layout moved: partial rows", name)
    if ln.kind == BN_BWD_REDUCE:
        assert r.ldp in (0, r.C) and r.nblk == (r.R + r.rows_per_blk - 1) // r.rows_per_blk
        return
    assert buffer_at(plan, d.totals)[3] == 3 * r.C * 4 and d.count in (r.R, r.R * max(plan.cfg.bn_world, 1)), "BnBwdApply layout moved: totals / count"
    assert buffer_at(plan, d.dy)[3] == r.R * r.C * es, "BnBwdApply layout moved: dy"
    _table_entry(plan, plan.params, GRAD, d.dgamma, r.C, "dgamma")
    _table_entry(plan, plan.params, GRAD, d.dbeta, r.C, "dbeta")
    _table_entry(plan, plan.params, GRAD, d.dslope, 1, "dslope")


def _check_cbn_mirror(plan, ln):
    d, fwd = ln.d, ln.kind in CBN_FWD
    h, es = d.C // 2, _esize(d.dt)
    name = "CbnFwd" if fwd else "CbnBwd"
    assert d.dt in (F32, BF16) and d.C % 8 == 0 and d.R >= 1 and d.rows_per_blk >= 64 and d.nblk == (d.R + d.rows_per_blk - 1) // d.rows_per_blk, f"{name} layout moved"
    assert buffer_at(plan, d.y)[3] == d.R * d.C * es, f"{name} layout moved: R * C * elementsize is not the size of y's buffer"
    assert buffer_at(plan, d.coef)[3] == 14 * h * 4, f"{name} layout moved: coef"
    for k in range(3):
        _table_entry(plan, plan.params, PARAM, d.W[k], h, "W")
    if d.slope.arena == PARAM:
        _table_entry(plan, plan.params, PARAM, d.slope, 1, "slope")
    else:                                                        # the module on its own: a constant 1 in the plan's constants
        assert d.slope.arena == CONST and float(torch.from_numpy(plan.const_image()[d.slope.off:d.slope.off + 4].copy()).view(torch.float32)) == 1.0
    if fwd:
        assert buffer_at(plan, d.z)[3] == d.R * d.C * es and d.training in (0, 1) and abs(d.eps - 1e-5) < 1e-9, "CbnFwd layout moved"
        if d.training:
            assert buffer_at(plan, d.part)[3] >= d.nblk * 5 * h * 4 and d.count >= d.R
        for k in range(2):
            _table_entry(plan, plan.params, PARAM, d.Bv[k], h, "B")
            _table_entry(plan, plan.state, STATE, d.RM[k], h, "RM")
        for k in range(3):
            _table_entry(plan, plan.state, STATE, d.RV[k], h, "RV")
        return
    assert d.R % d.rpb == 0 and 0 <= d.skip < d.rpb and d.count >= d.R, "CbnBwd layout moved"
    assert buffer_at(plan, d.dz0)[3] == (d.R // d.rpb) * (d.rpb - d.skip) * d.C * es, "CbnBwd layout moved: dz0"
    assert d.dz1.arena < 0 or buffer_at(plan, d.dz1)[3] == d.R * d.C * es, "CbnBwd layout moved: dz1"
    assert buffer_at(plan, d.dy)[3] == d.R * d.C * es and buffer_at(plan, d.coefb)[3] == 9 * h * 4 and buffer_at(plan, d.part)[3] >= d.nblk * 7 * h * 4
    for k in range(3):
        _table_entry(plan, plan.params, GRAD, d.dW[k], h, "dW")
    for k in range(2):
        _table_entry(plan, plan.params, GRAD, d.dB[k], h, "dB")
    if d.dslope.arena == GRAD:
        _table_entry(plan, plan.params, GRAD, d.dslope, 1, "dslope")
    else:
        assert buffer_at(plan, d.dslope)[3] == 4


def launches(plan):
    """The BatchNorm and ComplexBatchNorm launches of both phases, in order, each with a copy of its descriptor (checked: check_mirror)."""
    out, sz = [], plan.lib.sefd_op_size()
    for phase in (PHASE_FWD, PHASE_BWD):
        for i in range(plan.num_ops(phase)):
            ptr = plan.ops_ptr(phase) + i * sz
            kind, tag = (C.c_int32 * 2).from_buffer_copy(C.string_at(ptr, 8))
            if kind in MIRRORS:
                cls = MIRRORS[kind]
                ln = Launch(phase, i, kind, tag, cls.from_buffer_copy(C.string_at(ptr + OP_HEADER, C.sizeof(cls))))
                check_mirror(plan, ln)
                out.append(ln)
    return out


def channels(ln):
    return ln.d.r.C if ln.kind in (BN_BWD_FINALIZE, BN_BWD_APPLY) else ln.d.C


def partial_rows(ln):
    """Partial rows a finalize folds (0: none - eval, or SyncBN mode 2)."""
    if ln.kind == BN_FINALIZE:
        return ln.d.nblk if ln.d.nblk > 0 and ln.d.mode != 2 else 0
    return ln.d.r.nblk if ln.kind == BN_BWD_FINALIZE else 0


def chunks(ln):
    """Chunks of the two-level finalize that takes launch `ln` (0: the one-level kernel; kernels.hip launch_misc / fin_two_level)."""
    n = partial_rows(ln)
    if n < FIN_TWO_LEVEL or (ln.kind == BN_FINALIZE and ln.d.mode != 0):
        return 0
    return min(FIN_MAX_CHUNKS, (n + FIN_ROWS_PER_CHUNK - 1) // FIN_ROWS_PER_CHUNK)


def select(case, lns):
    """The launches of its plan that `case` runs."""
    first = min(ln.tag for ln in lns)
    keep = {
        "all": lambda ln: True,
        "c1024": lambda ln: channels(ln) == 1024,
        "first": lambda ln: ln.tag == first,
        "first_bwd_finalize": lambda ln: ln.tag == first and ln.kind == BN_BWD_FINALIZE,
        "finalize": lambda ln: ln.kind == BN_FINALIZE,
        "forward": lambda ln: ln.phase == PHASE_FWD,
    }[case.keep]
    return [ln for ln in lns if keep(ln)]


def finalize_order(lns):
    """The order in which a case's finalize launches run their three repeats: every launch three times in a row, and between two launches of the
    SAME chunk count one of another count where the case has one (the tickets reset themselves only if every chunk arrives: a count left behind by
    one launch shows in the next launch of another count)."""
    fin = [ln for ln in lns if ln.kind in (BN_FINALIZE, BN_BWD_FINALIZE, CBN_FINALIZE, CBN_BWD_FINALIZE)]
    rest = sorted(fin, key=lambda ln: (ln.phase, ln.op))
    out = []
    while rest:
        nxt = next((ln for ln in rest if not out or chunks(ln) != chunks(out[-1])), rest[0])
        rest.remove(nxt)
        out.append(nxt)
    return out


# ------------------------------------------------------------------------------------------------ planted data
def _gen(case, ln):
    return torch.Generator().manual_seed(zlib.crc32(f"{case.name}:{ln.phase}:{ln.op}".encode()))


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def special_channels(C):
    """(small, big, gamma 0, constant, tie): five distinct channels spread over the layer (C >= 8 and no multiple of 7)."""
    idx = [(7 * k + 3) % C for k in range(5)]
    assert len(set(idx)) == 5
    return idx


def slope_of(case, ln):
    return SLOPES[(ln.tag + ln.tag // 100 + (0 if ln.kind == BN_APPLY else 1) + len(case.name)) % 4]


def channel_params(g, C, wide):
    """(mean, invstd, gamma, beta) [C] float64 of a profile."""
    small, big, g0, const, tie = special_channels(C)
    if wide:
        mean, invstd = _ints(g, -4, 4, C), 2.0 ** _ints(g, -6, 6, C)
        gamma = (2 * _ints(g, 0, 1, C) - 1) * 2.0 ** _ints(g, -3, 3, C)
    else:
        mean, invstd = _ints(g, -2, 2, C), 2.0 ** _ints(g, -1, 1, C)
        gamma = (2 * _ints(g, 0, 1, C) - 1) * 2.0 ** _ints(g, -1, 1, C)
    beta = _ints(g, -8, 8, C) / 4
    gamma[g0], beta[g0] = 0.0, 0.0                              # bn == 0 exactly on every row of the channel (others hold scattered zeros)
    if wide:
        invstd[small], gamma[small], beta[small] = 2.0 ** -6, -(2.0 ** -3), 0.25
        mean[big], invstd[big], gamma[big], beta[big] = -4.0, 64.0, 8.0, 2.0     # y = 8 gives 6146 on the branch no slope touches
        mean[tie], invstd[tie], gamma[tie], beta[tie] = 0.0, 64.0, 4.0, 1.0
    return mean, invstd, gamma, beta


def rows_y(g, R, C, wide):
    y = _ints(g, -8, 8, R, C) if wide else _ints(g, -3, 3, R, C)
    y[:, special_channels(C)[3]] = 5.0 if wide else 2.0
    return y


def upstream(r, dz0, dz1):
    """dz [R][C] of BnBwdReduce `r`: y row (b, q) takes dz0 row b * (rpb - skip) + q - skip where q >= skip, nothing below, + dz1 of its own row."""
    nb, rpb, skip = r.R // r.rpb, r.rpb, r.skip
    dz = torch.zeros(nb, rpb, r.C, dtype=torch.float64)
    dz[:, skip:] = dz0.view(nb, rpb - skip, r.C)
    dz = dz.view(r.R, r.C)
    return dz + dz1 if dz1 is not None else dz


# ------------------------------------------------------------------------------------------------ references (float64)
def ref_apply(y, mean, invstd, gamma, beta, a):
    bn = gamma * ((y - mean) * invstd) + beta
    return torch.where(bn > 0, bn, a * bn)


def by_block(r, t):
    """[R][C] -> [nblk][rows_per_blk][C], the short last block padded with zeros."""
    pad = torch.zeros(r.nblk * r.rows_per_blk - r.R, r.C, dtype=t.dtype)
    return torch.cat([t, pad]).view(r.nblk, r.rows_per_blk, r.C)


def ref_reduce(r, y, dz, mean, invstd, gamma, beta, a, ge=False):
    """(part [nblk][3][C] with row 2 = the block's whole slope share in channel 0, terms, bn): BnBwdReduce `r` over blocks of rows_per_blk rows.
    terms = the three [R][C] arrays that are summed (for conditions()).  ge: the WRONG branch test bn >= 0 (a fault the CPU file plants)."""
    xh = (y - mean) * invstd
    bn = gamma * xh + beta
    pos = bn >= 0 if ge else bn > 0
    dbn = torch.where(pos, dz, a * dz)
    sl = torch.where(pos, torch.zeros_like(bn), bn * dz)
    part = torch.zeros(r.nblk, 3, r.C, dtype=torch.float64)
    part[:, 0], part[:, 1], part[:, 2, 0] = by_block(r, dbn).sum(1), by_block(r, dbn * xh).sum(1), by_block(r, sl).sum((1, 2))
    return part + 0.0, (dbn, dbn * xh, sl), bn


def ref_bwd_apply(count, y, dz, mean, invstd, gamma, beta, a, tot):
    """(dy, bar) [R][C]: the value and N_ROUNDINGS * 2^-24 * |gamma * invstd| * (|dbn| + |t0| + |xhat * t1|)."""
    xh = (y - mean) * invstd
    bn = gamma * xh + beta
    dbn = torch.where(bn > 0, dz, a * dz)
    t0, t1 = tot[0] / count, tot[1] / count
    dy = gamma * invstd * (dbn - t0 - xh * t1)
    bar = N_ROUNDINGS * 2.0 ** -24 * (gamma * invstd).abs() * (dbn.abs() + t0.abs() + (xh * t1).abs())
    return dy, bar


def bf16_ulp(v):
    """The bf16 ulp of |v| (float64 tensor; the smallest normal's below it)."""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    return 2.0 ** (e - 7)


def split_exact(total, n):
    """n float64 values, each exact in fp32, that sum to the integer `total` < 2^47: its top 24 bits, the rest, and zeros."""
    total = int(total)
    sign, mag = (-1 if total < 0 else 1), abs(total)
    assert mag < 1 << 47
    if n == 1:                                                   # one partial row: the total itself
        assert float(torch.tensor(float(total)).float()) == total, total
        return [float(total)]
    sh = max(mag.bit_length() - 24, 0)
    hi = mag >> sh << sh
    return [float(sign * hi), float(sign * (mag - hi))] + [0.0] * (n - 2)


# ------------------------------------------------------------------------------------------------ a launch's planted inputs and expected outputs
# One output of a launch: n elements of dtype code dt from byte `off` of `arena` on, C per row.  exp: float64 [n].  tol None and ulps 0: byte equality
# with exp rounded to dt (fp32: exp must be exact; bf16: to nearest even); ulps > 0: at most that many fp32 ulps from exp rounded to fp32; tol: float64
# [n], |device - exp| <= tol.  group: None, or int64 [n] with -1 = compared by element and g >= 0 = compared through the sum of group g against gexp[g].
Field = namedtuple("Field", "name arena off dt C exp tol ulps group gexp", defaults=(None, 0, None, None))
# puts: [(arena, byte offset, tensor)] the inputs; fields: [Field]; terms: {name: (sum of |terms| per sum, terms)} for conditions(); notes: what the
# CPU file asserts about the data (counts of bn == 0 elements, ties, ...)
Planted = namedtuple("Planted", "puts fields terms notes")


def _store(dt, v):
    return v.to(torch.float32).to(_tdtype(dt)) if dt != F64 else v.clone()


def _param_puts(r, mean, invstd, gamma, beta, a):
    return [(r.mean_invstd.arena, r.mean_invstd.off, torch.cat([mean, invstd]).float()), (PARAM, r.gamma.off, gamma.float()),
            (PARAM, r.beta.off, beta.float()), (PARAM, r.slope.off, torch.tensor([a], dtype=torch.float32))]


def _bwd_inputs(g, r, wide):
    lo, hi = (-8, 8) if wide else (-3, 3)
    y = rows_y(g, r.R, r.C, wide)
    dz0 = _ints(g, lo, hi, (r.R // r.rpb) * (r.rpb - r.skip), r.C)
    dz1 = _ints(g, lo, hi, r.R, r.C) if r.dz1.arena >= 0 else None
    puts = [(r.y.arena, r.y.off, _store(r.dt, y)), (r.dz0.arena, r.dz0.off, _store(r.dt, dz0))]
    if dz1 is not None:
        puts.append((r.dz1.arena, r.dz1.off, _store(r.dt, dz1)))
    return y, dz0, dz1, puts


def plant(case, ln):
    """The planted inputs and the float64 expectation of launch `ln` of `case`."""
    g, d, a = _gen(case, ln), ln.d, slope_of(case, ln)
    if ln.kind in CBN_FWD + CBN_BWD:
        return _plant_cbn(g, ln, a, plan_of(case))
    if ln.kind == BN_APPLY:
        mean, invstd, gamma, beta = channel_params(g, d.C, True)
        y = rows_y(g, d.R, d.C, True)
        z = ref_apply(y, mean, invstd, gamma, beta, a)
        bn = gamma * ((y - mean) * invstd) + beta
        bits = z.float().view(torch.int32)
        notes = dict(zeros=int((bn == 0).sum()), ties=int(((bits & 0xffff) == 0x8000).sum()), inexact_bf16=int(((bits & 0xffff) != 0).sum()),
                     small=float(z[:, special_channels(d.C)[0]].abs().max()), big=float(z[:, special_channels(d.C)[1]].abs().max()), slope=a)
        return Planted([(d.y.arena, d.y.off, _store(d.dt, y))] + _param_puts(d, mean, invstd, gamma, beta, a),
                       [Field("z", d.z.arena, d.z.off, d.dt, d.C, z.reshape(-1))], {}, notes)
    if ln.kind == BN_BWD_REDUCE:
        mean, invstd, gamma, beta = channel_params(g, d.C, False)
        y, dz0, dz1, puts = _bwd_inputs(g, d, False)
        part, terms, bn = ref_reduce(d, y, upstream(d, dz0, dz1), mean, invstd, gamma, beta, a)
        group = torch.full((d.nblk, 3, d.C), -1, dtype=torch.int64)
        group[:, 2] = torch.arange(d.nblk)[:, None]
        blocks = lambda t, whole: by_block(d, t.abs()).sum((1, 2)) if whole else by_block(d, t.abs()).sum(1).max(1).values
        sums = {"sum dbn": (blocks(terms[0], False), terms[0]), "sum dbn * xhat": (blocks(terms[1], False), terms[1]),
                "slope share": (blocks(terms[2], True), terms[2])}
        return Planted(puts + _param_puts(d, mean, invstd, gamma, beta, a),
                       [Field("part", d.part.arena, d.part.off, F32, d.C, part.reshape(-1), group=group.reshape(-1), gexp=part[:, 2].sum(1) + 0.0)],
                       sums, dict(zeros=int((bn == 0).sum()), slope=a))
    if ln.kind == BN_BWD_FINALIZE:
        r = d.r
        C_, ld = r.C, (r.ldp or r.C)
        part = torch.full((r.nblk, 3, ld), SENTINEL, dtype=torch.float64)
        part[:, :, :C_] = _ints(g, -32, 32, r.nblk, 3, C_) / 4
        s = part[:, :, :C_].sum(0) + 0.0
        fields = [Field("totals", d.totals.arena, d.totals.off, F32, C_, s[:2].reshape(-1)), Field("dbeta", GRAD, d.dbeta.off, F32, C_, s[0].clone()),
                  Field("dgamma", GRAD, d.dgamma.off, F32, C_, s[1].clone()), Field("dslope", GRAD, d.dslope.off, F32, 1, s[2].sum().reshape(1) + 0.0)]
        t = part[:, :, :C_]
        return Planted([(r.part.arena, r.part.off, part.float())], fields,
                       {"totals": (t[:, :2].abs().sum(0).reshape(-1), t[:, :2]), "dslope": (t[:, 2].abs().sum().reshape(1), t[:, 2])},
                       dict(other_channels=int((part[:, 2, 1:C_] != 0).sum())))
    if ln.kind == BN_BWD_APPLY:
        r = d.r
        mean, invstd, gamma, beta = channel_params(g, r.C, True)
        y, dz0, dz1, puts = _bwd_inputs(g, r, True)
        # t0 and xhat * t1 of the size of dbn: totals = count * (quarters in -8 .. 8 | the same over the channel's largest |xhat|), as fp32
        xmax = ((y - mean) * invstd).abs().max(0).values.clamp(min=1.0)
        tot = torch.stack([d.count * _ints(g, -32, 32, r.C) / 4, d.count * (2 * _ints(g, 0, 1, r.C) - 1) * _ints(g, 8, 32, r.C) / 4 / xmax,
                           torch.zeros(r.C, dtype=torch.float64)]).float()
        dy, bar = ref_bwd_apply(d.count, y, upstream(r, dz0, dz1), mean, invstd, gamma, beta, a, tot.double())
        if r.dt == BF16:
            bar = bar + 0.5 * bf16_ulp(dy)
        return Planted(puts + _param_puts(r, mean, invstd, gamma, beta, a) + [(d.totals.arena, d.totals.off, tot.reshape(-1))],
                       [Field("dy", d.dy.arena, d.dy.off, r.dt, r.C, dy.reshape(-1), tol=bar.reshape(-1))], {}, dict(slope=a))
    assert ln.kind == BN_FINALIZE
    return _plant_finalize(g, d)


def _plant_finalize(g, d):
    C_ = d.C
    mi_mean = Field("mean", d.mean_invstd.arena, d.mean_invstd.off, F32, C_, None)
    eps, mom = float(torch.tensor(d.eps, dtype=torch.float32).double()), float(torch.tensor(d.momentum, dtype=torch.float32).double())
    rm, rv = _ints(g, -16, 16, C_) / 8, _ints(g, 1, 64, C_) / 16
    if d.nblk < 0:                                               # eval: mean_invstd from the running statistics, nothing else written
        puts = [(STATE, d.running_mean.off, rm.float()), (STATE, d.running_var.off, rv.float())]
        inv = 1.0 / torch.sqrt(rv + eps)
        return Planted(puts, [mi_mean._replace(exp=rm), Field("invstd", d.mean_invstd.arena, d.mean_invstd.off + 4 * C_, F32, C_, inv, ulps=3)], {}, dict(eval=True))
    n = int(d.count)
    assert n == d.count
    nsub = max(d.nsub, 1)
    small, big, g0, const, tie = special_channels(C_)            # here: constant, mean 1000 variance 1, slightly negative variance
    puts, terms = [], {}
    if d.mode == 2:                                              # SyncBN: the all-reduced totals are the input
        s = torch.stack([_ints(g, -50 * n, 50 * n, C_), torch.zeros(C_, dtype=torch.float64)])
        s[1] = torch.floor(s[0] ** 2 / n) + _ints(g, n, 40 * n, C_)
    else:
        part = torch.full((d.nblk, 2, d.Cpad), SENTINEL, dtype=torch.float64)
        cols = (torch.arange(nsub)[:, None] * d.substride + torch.arange(C_)[None, :]).reshape(-1)      # [nsub][C]
        part[:, 0, cols] = _ints(g, -100, 100, d.nblk, nsub * C_)
        part[:, 1, cols] = _ints(g, 200, 400, d.nblk, nsub * C_)
        ne = d.nblk * nsub
        for c, (s1, s2) in {const: (3 * n, 9 * n), g0: (3 * n, 9 * n - 1), big: (1000 * n, 1000001 * n)}.items():
            for row, tot in ((0, s1), (1, s2)):
                v = torch.tensor(split_exact(tot, ne), dtype=torch.float64)[torch.randperm(ne, generator=g)].view(d.nblk, nsub)
                for u in range(nsub):
                    part[:, row, u * d.substride + c] = v[:, u]
        per = part[:, :, cols].view(d.nblk, 2, nsub, C_)
        s = per.sum((0, 2)) + 0.0
        terms = {"partial sums": (per.abs().sum((0, 2)).reshape(-1), per)}
        puts.append((d.part.arena, d.part.off, part.float()))
    if d.mode == 1:                                              # SyncBN: this rank's sums as doubles, nothing else
        return Planted(puts, [Field("totals", d.totals.arena, d.totals.off, F64, C_, s.reshape(-1))], terms, dict(mode=1))
    if d.mode == 2:
        puts.append((d.totals.arena, d.totals.off, s.reshape(-1).clone()))
    mean = s[0] / d.count
    var = (s[1] / d.count - mean * mean).clamp(min=0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    fields = [mi_mean._replace(exp=mean.float().double()), Field("invstd", d.mean_invstd.arena, d.mean_invstd.off + 4 * C_, F32, C_, inv, ulps=1)]
    if d.running_mean.arena >= 0:
        unb = var * (d.count / (d.count - 1 if d.count > 1 else 1))
        puts += [(STATE, d.running_mean.off, rm.float()), (STATE, d.running_var.off, rv.float())]
        fields += [Field("running_mean", STATE, d.running_mean.off, F32, C_, (1.0 - mom) * rm + mom * mean, ulps=1),
                   Field("running_var", STATE, d.running_var.off, F32, C_, (1.0 - mom) * rv + mom * unb, ulps=1)]
    notes = dict(mode=d.mode, var_const=float(var[const]), raw_negative=float((s[1] / d.count - mean * mean)[g0]) if d.mode == 0 else -1.0,
                 mean_big=float(mean[big]), var_big=float(var[big]), unbiased=d.count / (d.count - 1))
    return Planted(puts, fields, terms, notes)


# ------------------------------------------------------------------------------------------------ ComplexBatchNorm (csrc/cbn.hip)
# Channel k < h = C / 2 is the real and k + h the imaginary part of complex channel k.  coef fp32 [14][h]: Zrr Zri Zir Zii | br' bi' | Mr Mi |
# Urr Uri Uii | Vrr + eps, Vri, Vii + eps; coefb fp32 [9][h]: Zrr Zri Zir Zii | mean dbn_r, mean dbn_i | 2 dVrr / N, dVri / N, 2 dVii / N.
def cbn_affine(coef, y, h):
    """(yr, yi) [R][h] = Z x + b' from coef rows 0 .. 5."""
    xr, xi = y[:, :h], y[:, h:]
    return coef[0] * xr + coef[1] * xi + coef[4], coef[2] * xr + coef[3] * xi + coef[5]


def _cbn_coef(g, h, wide):
    """Planted coef [14][h] float64 with dyadic Z, b' and means (rows 8 .. 13 - U and V - small integers: the passes do not read them)."""
    lo, hi = (-6, 3) if wide else (-1, 1)
    coef = torch.zeros(14, h, dtype=torch.float64)
    coef[:4] = (2 * _ints(g, 0, 1, 4, h) - 1) * 2.0 ** _ints(g, lo, hi, 4, h)
    coef[4:6] = _ints(g, -8, 8, 2, h) / 4
    coef[6:8] = _ints(g, -2, 2, 2, h)
    coef[8:] = _ints(g, 1, 3, 6, h)
    if wide:
        coef[:4, 0], coef[4:6, 0] = 2.0 ** -6, 0.25               # |z| < 1
        coef[:4, 1], coef[4:6, 1] = 8.0, 2.0                      # |z| to 258
        coef[:4, 2], coef[4:6, 2] = 32.0, 1.0                     # 32 (xr + xi) + 1: 257, 769, .. are ties of the bf16 rounding
        coef[:4, 3], coef[4:6, 3] = 0.0, 0.0                      # bn == 0 on every row
    else:
        coef[:4, 3], coef[4:6, 3] = 0.0, 0.0
    return coef


def _cbn_slope(d, a, plan):
    """(slope, puts): the planted arm where the slope is a parameter, else the plan's constant 1."""
    if d.slope.arena == PARAM:
        return a, [(PARAM, d.slope.off, torch.tensor([a], dtype=torch.float32))]
    return 1.0, []


def _plant_cbn(g, ln, a, plan):
    d, h = ln.d, ln.d.C // 2
    a, sput = _cbn_slope(d, a, plan)
    if ln.kind == CBN_STATS:
        y = _ints(g, -8, 8, d.R, d.C)
        xr, xi = y[:, :h], y[:, h:]
        t = [xr, xi, xr * xr, xi * xi, xr * xi]
        part = torch.stack([by_block(_Rows(d, h), v).sum(1) for v in t], 1) + 0.0               # [nblk][5][h]
        terms = {f"sum {n}": (by_block(_Rows(d, h), v.abs()).sum(1).reshape(-1), v) for n, v in zip(("xr", "xi", "xr^2", "xi^2", "xr xi"), t)}
        return Planted([(d.y.arena, d.y.off, _store(d.dt, y))], [Field("part", d.part.arena, d.part.off, F32, h, part.reshape(-1))], terms, {})
    if ln.kind == CBN_APPLY:
        coef = _cbn_coef(g, h, True)
        y = _ints(g, -8, 8, d.R, d.C)
        yr, yi = cbn_affine(coef, y, h)
        bn = torch.cat([yr, yi], 1)
        z = torch.where(bn > 0, bn, a * bn)
        if d.slope.arena != PARAM:
            assert a == 1.0 and torch.equal(z, bn)                # the module on its own: z is the affine map
        bits = z.float().view(torch.int32)
        notes = dict(zeros=int((bn == 0).sum()), ties=int(((bits & 0xffff) == 0x8000).sum()), inexact_bf16=int(((bits & 0xffff) != 0).sum()),
                     small=float(z[:, 0].abs().max()), big=float(z[:, 1].abs().max()), slope=a)
        return Planted([(d.y.arena, d.y.off, _store(d.dt, y)), (d.coef.arena, d.coef.off, coef.float())] + sput,
                       [Field("z", d.z.arena, d.z.off, d.dt, d.C, z.reshape(-1))], {}, notes)
    if ln.kind in (CBN_BWD_REDUCE, CBN_BWD_APPLY):
        wide = ln.kind == CBN_BWD_APPLY
        coef = _cbn_coef(g, h, wide)
        lo, hi = (-8, 8) if wide else (-3, 3)
        y = _ints(g, lo, hi, d.R, d.C)
        dz0 = _ints(g, lo, hi, (d.R // d.rpb) * (d.rpb - d.skip), d.C)
        dz1 = _ints(g, lo, hi, d.R, d.C) if d.dz1.arena >= 0 else None
        puts = [(d.y.arena, d.y.off, _store(d.dt, y)), (d.dz0.arena, d.dz0.off, _store(d.dt, dz0)), (d.coef.arena, d.coef.off, coef.float())] + sput
        if dz1 is not None:
            puts.append((d.dz1.arena, d.dz1.off, _store(d.dt, dz1)))
        dz = upstream(d, dz0, dz1)
        yr, yi = cbn_affine(coef, y, h)
        gr, gi = dz[:, :h], dz[:, h:]
        dr, di = torch.where(yr > 0, gr, a * gr), torch.where(yi > 0, gi, a * gi)
        cr, ci = y[:, :h] - coef[6], y[:, h:] - coef[7]
        zeros = int((yr == 0).sum() + (yi == 0).sum())
        if ln.kind == CBN_BWD_REDUCE:
            sl = torch.where(yr > 0, torch.zeros_like(yr), yr * gr) + torch.where(yi > 0, torch.zeros_like(yi), yi * gi)
            t = [dr, di, dr * cr, dr * ci, di * cr, di * ci]
            rows = _Rows(d, h)
            part = torch.zeros(d.nblk, 7, h, dtype=torch.float64)
            part[:, :6] = torch.stack([by_block(rows, v).sum(1) for v in t], 1)
            part[:, 6, 0] = by_block(rows, sl).sum((1, 2))
            group = torch.full((d.nblk, 7, h), -1, dtype=torch.int64)
            group[:, 6] = torch.arange(d.nblk)[:, None]
            terms = {f"sum {i}": (by_block(rows, v.abs()).sum(1).reshape(-1), v) for i, v in enumerate(t)}
            terms["slope share"] = (by_block(rows, sl.abs()).sum((1, 2)), sl)
            return Planted(puts, [Field("part", d.part.arena, d.part.off, F32, h, (part + 0.0).reshape(-1), group=group.reshape(-1),
                                        gexp=part[:, 6].sum(1) + 0.0)], terms, dict(zeros=zeros, slope=a))
        # BWD_APPLY: coefb rows 4 .. 8 of the size of the other terms, not dyadic; rows 0 .. 3 (a copy of Z) unread
        cb = torch.cat([coef[:4], _ints(g, -32, 32, 2, h) / 7, _ints(g, -32, 32, 3, h) / 56]).float()
        c64 = cb.double()
        mr_, mi_ = dr - c64[4], di - c64[5]
        o_r = coef[0] * mr_ + coef[2] * mi_ + c64[6] * cr + c64[7] * ci
        o_i = coef[1] * mr_ + coef[3] * mi_ + c64[7] * cr + c64[8] * ci
        ab = lambda zr_, zi_, q0, q1: (zr_.abs() * (dr.abs() + c64[4].abs()) + zi_.abs() * (di.abs() + c64[5].abs()) + (q0 * cr).abs() + (q1 * ci).abs())
        dy = torch.cat([o_r, o_i], 1)
        bar = N_ROUNDINGS_CBN * 2.0 ** -24 * torch.cat([ab(coef[0], coef[2], c64[6], c64[7]), ab(coef[1], coef[3], c64[7], c64[8])], 1)
        if d.dt == BF16:
            bar = bar + 0.5 * bf16_ulp(dy)
        return Planted(puts + [(d.coefb.arena, d.coefb.off, cb.reshape(-1))], [Field("dy", d.dy.arena, d.dy.off, d.dt, d.C, dy.reshape(-1), tol=bar.reshape(-1))],
                       {}, dict(zeros=zeros, slope=a))
    if ln.kind == CBN_FINALIZE:
        return _plant_cbn_finalize(g, d, h)
    return _plant_cbn_bwd_finalize(g, d, h)


def f32_ulp(v):
    """The fp32 ulp of |v| (float64 tensor)."""
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126))) - 23)


def inv_sqrt_2x2(vrr, vri, vii):
    """U = V^-1/2 of [[vrr, vri], [vri, vii]] in the reference module's closed form: (urr, uri, uii, s, t, rst)."""
    tau, delta = vrr + vii, vrr * vii - vri * vri
    s = delta.sqrt()
    t = (tau + 2 * s).sqrt()
    rst = 1.0 / (s * t)
    return (s + vii) * rst, -vri * rst, (s + vrr) * rst, s, t, rst


def cbn_covariances(g, h, big):
    """(mr, mi, vrr, vri, vii) [h] float64, complex channel k of kind k % 5: well-conditioned; xi == xr (singular up to eps); xi identically 0; both
    parts constant; mean +-`big` with variance 1."""
    m = [torch.zeros(h, dtype=torch.float64) for _ in range(5)]
    pick = lambda vals: float(vals[int(torch.randint(0, len(vals), (1,), generator=g))])
    for k in range(h):
        a = pick((-3, -2, -1, 1, 2, 3))
        row = [(a, pick((-3, -1, 0, 2)), pick((2, 3, 5)), pick((-1, 0, 1)), pick((2, 3, 5))), (a, a, 2.0, 2.0, 2.0), (a, 0.0, 3.0, 0.0, 0.0),
               (2.0, -1.0, 0.0, 0.0, 0.0), (float(big), -float(big), 1.0, 0.0, 1.0)][k % 5]
        for j in range(5):
            m[j][k] = row[j]
    return m


def _cbn_wb(g, h):
    """W (positive definite: diagonal 3/4 .. 5/4, off-diagonal within 1/4) and B (quarters), exact in fp32: (wrr, wri, wii, br, bi)."""
    return ((8 + _ints(g, -2, 2, h)) / 8, _ints(g, -2, 2, h) / 8, (8 + _ints(g, -2, 2, h)) / 8, _ints(g, -8, 8, h) / 4, _ints(g, -8, 8, h) / 4)


def _summed(name, ptr, row, h, value, absterms):
    """A coef / coefb row that is a sum of terms that may cancel: 2 * 2^-24 * sum|terms|."""
    return Field(name, ptr.arena, ptr.off + 4 * row * h, F32, h, value, tol=2 * 2.0 ** -24 * absterms + 1e-300)


def _plant_cbn_finalize(g, d, h):
    eps, mom = float(torch.tensor(d.eps, dtype=torch.float32).double()), float(torch.tensor(d.momentum, dtype=torch.float32).double())
    wrr, wri, wii, br, bi = _cbn_wb(g, h)
    puts = [(PARAM, p.off, v.float()) for p, v in zip(list(d.W) + list(d.Bv), (wrr, wri, wii, br, bi))]
    fields, terms, notes = [], {}, dict(training=d.training)
    if d.training:
        assert d.mode == 0
        n = int(d.count)
        big = 1000 if d.nblk >= 2 else 100                        # one partial row: the sum itself has to be exact in fp32
        mr, mi, vrr, vri, vii = cbn_covariances(g, h, big)
        tot = torch.stack([n * mr, n * mi, n * (mr * mr + vrr), n * (mi * mi + vii), n * (mr * mi + vri)])
        part = torch.zeros(d.nblk, 5, h, dtype=torch.float64)
        for j in range(5):
            for k in range(h):
                part[:, j, k] = torch.tensor(split_exact(int(tot[j, k]), d.nblk), dtype=torch.float64)[torch.randperm(d.nblk, generator=g)]
        puts.append((d.part.arena, d.part.off, part.float()))
        terms = {"partial sums": (part.abs().sum(0).reshape(-1), part)}
        t = part.sum(0)
        mr, mi = t[0] / d.count, t[1] / d.count
        vrr, vii, vri = (t[2] / d.count - mr * mr).clamp(min=0.0), (t[3] / d.count - mi * mi).clamp(min=0.0), t[4] / d.count - mr * mi
        old = [_ints(g, -16, 16, h) / 8 for _ in range(2)] + [_ints(g, 1, 64, h) / 16, _ints(g, -8, 8, h) / 16, _ints(g, 1, 64, h) / 16]
        for ptr, o, new, nm in zip(list(d.RM) + list(d.RV), old, (mr, mi, vrr, vri, vii), ("RMr", "RMi", "RVrr", "RVri", "RVii")):
            puts.append((STATE, ptr.off, o.float()))
            new32 = new.float().double()                          # the reference's rule: lerp towards the fp32 statistic, biased, without eps
            exp = o + mom * (new32 - o)
            fields.append(Field(nm, STATE, ptr.off, F32, h, exp, tol=4 * f32_ulp(torch.maximum(o.abs(), exp.abs()))))
        notes.update(big=big, kinds=min(h, 5))
    else:                                                        # eval: the running statistics are the input, nothing in the state arena changes
        mr, mi, vrr, vri, vii = cbn_covariances(g, h, 100)
        puts += [(STATE, ptr.off, v.float()) for ptr, v in zip(list(d.RM) + list(d.RV), (mr, mi, vrr, vri, vii))]
    vrr, vii = vrr + eps, vii + eps
    urr, uri, uii, _, _, _ = inv_sqrt_2x2(vrr, vri, vii)
    zrr, zri, zir, zii = wrr * urr + wri * uri, wrr * uri + wri * uii, wri * urr + wii * uri, wri * uri + wii * uii
    fields += [_summed("Zrr", d.coef, 0, h, zrr, (wrr * urr).abs() + (wri * uri).abs()), _summed("Zri", d.coef, 1, h, zri, (wrr * uri).abs() + (wri * uii).abs()),
               _summed("Zir", d.coef, 2, h, zir, (wri * urr).abs() + (wii * uri).abs()), _summed("Zii", d.coef, 3, h, zii, (wri * uri).abs() + (wii * uii).abs()),
               _summed("br'", d.coef, 4, h, br - zrr * mr - zri * mi, br.abs() + (zrr * mr).abs() + (zri * mi).abs()),
               _summed("bi'", d.coef, 5, h, bi - zir * mr - zii * mi, bi.abs() + (zir * mr).abs() + (zii * mi).abs())]
    for row, (nm, v) in enumerate((("Mr", mr), ("Mi", mi), ("Urr", urr), ("Uri", uri), ("Uii", uii), ("Vrr", vrr), ("Vri", vri), ("Vii", vii)), 6):
        fields.append(Field(nm, d.coef.arena, d.coef.off + 4 * row * h, F32, h, v, ulps=2))
    return Planted(puts, fields, terms, notes)


def cbn_dv(wrr, wri, wii, dz, vrr, vri, vii):
    """(dvrr, dvri, dvii): the gradient of phi(V) = sum(dZ * (W U(V))), U = V^-1/2 in the reference's closed form, by torch autograd in float64 -
    no transcription of the kernel's hand-derived chain.  dvri is the derivative with respect to the ONE scalar vri."""
    v = [t.clone().requires_grad_(True) for t in (vrr, vri, vii)]
    urr, uri, uii, _, _, _ = inv_sqrt_2x2(*v)
    phi = (dz[0] * (wrr * urr + wri * uri) + dz[1] * (wrr * uri + wri * uii) + dz[2] * (wri * urr + wii * uri) + dz[3] * (wri * uri + wii * uii)).sum()
    return torch.autograd.grad(phi, v)


def cbn_dv_abs(wrr, wri, wii, dz, vrr, vri, vii):
    """sum|terms| of (dvrr, dvri, dvii) - the running bound of the chain rule through s, t, rst with every term taken absolute.  For the BAR only."""
    a = lambda t: t.abs()
    _, _, _, s, t, rst = inv_sqrt_2x2(vrr, vri, vii)
    durr, duii = a(wrr * dz[0]) + a(wri * dz[2]), a(wri * dz[1]) + a(wii * dz[3])
    duri = a(wrr * dz[1]) + a(wri * dz[3]) + a(wri * dz[0]) + a(wii * dz[2])
    d_rst = durr * (s + vii) + duii * (s + vrr) + duri * a(vri)
    d_st = d_rst * rst * rst
    d_u = d_st * s / (2 * t)
    d_s = (durr + duii) * rst + d_st * t + 2 * d_u
    d_delta = d_s / (2 * s)
    return duii * rst + d_delta * vii + d_u, duri * rst + 2 * a(vri) * d_delta, durr * rst + d_delta * vrr + d_u


def _plant_cbn_bwd_finalize(g, d, h):
    assert d.mode == 0
    eps = float(torch.tensor(1e-5, dtype=torch.float32).double())
    wrr, wri, wii, _, _ = _cbn_wb(g, h)
    _, _, vrr, vri, vii = cbn_covariances(g, h, 1000)
    v32 = [t.float().double() for t in (vrr + eps, vri, vii + eps)]   # what the forward saved: the covariance, eps added, as fp32
    u32 = [t.float().double() for t in inv_sqrt_2x2(*v32)[:3]]
    coef = torch.cat([_cbn_coef(g, h, False)[:8], torch.stack(u32), torch.stack(v32)])
    part = torch.zeros(d.nblk, 7, h, dtype=torch.float64)
    part[:, :6] = _ints(g, -32, 32, d.nblk, 6, h) / 4
    part[:, 6, 0] = _ints(g, -32, 32, d.nblk) / 4                 # cbn_bwd_reduce_kernel leaves a block's whole share in column 0 and zeros behind it
    puts = [(PARAM, p.off, v.float()) for p, v in zip(list(d.W), (wrr, wri, wii))]
    puts += [(d.part.arena, d.part.off, part.float()), (d.coef.arena, d.coef.off, coef.float())]
    t = part.sum(0) + 0.0
    dbr, dbi, dz = t[0], t[1], t[2:6]
    urr, uri, uii = u32
    N = d.count
    fields = [Field("dBr", GRAD, d.dB[0].off, F32, h, dbr.clone()), Field("dBi", GRAD, d.dB[1].off, F32, h, dbi.clone()),
              Field("dslope", d.dslope.arena, d.dslope.off, F32, 1, t[6].sum().reshape(1) + 0.0)]
    dw = [(dz[0] * urr + dz[1] * uri, (dz[0] * urr).abs() + (dz[1] * uri).abs()),
          (dz[0] * uri + dz[1] * uii + dz[2] * urr + dz[3] * uri, (dz[0] * uri).abs() + (dz[1] * uii).abs() + (dz[2] * urr).abs() + (dz[3] * uri).abs()),
          (dz[2] * uri + dz[3] * uii, (dz[2] * uri).abs() + (dz[3] * uii).abs())]
    for k, (v, ab) in enumerate(dw):
        fields.append(Field(("dWrr", "dWri", "dWii")[k], GRAD, d.dW[k].off, F32, h, v, tol=2 * 2.0 ** -24 * ab + 1e-300))
    for row in range(4):                                         # Z: a copy of coef's rows
        fields.append(Field(f"coefb Z{row}", d.coefb.arena, d.coefb.off + 4 * row * h, F32, h, coef[row].clone()))
    fields += [Field("mean dbn_r", d.coefb.arena, d.coefb.off + 4 * 4 * h, F32, h, dbr / N, ulps=2),
               Field("mean dbn_i", d.coefb.arena, d.coefb.off + 4 * 5 * h, F32, h, dbi / N, ulps=2)]
    dv, dva = cbn_dv(wrr, wri, wii, dz, *v32), cbn_dv_abs(wrr, wri, wii, dz, *v32)
    for row, nm, f, j in ((6, "2 dVrr / N", 2.0, 0), (7, "dVri / N", 1.0, 1), (8, "2 dVii / N", 2.0, 2)):
        fields.append(_summed(nm, d.coefb, row, h, f * dv[j] / N, f * dva[j] / N))
    return Planted(puts, fields, {"totals": (part[:, :6].abs().sum(0).reshape(-1), part[:, :6]), "dslope": (part[:, 6].abs().sum().reshape(1), part[:, 6])},
                   dict(kinds=min(h, 5)))


class _Rows:
    """by_block()'s view of a CbnFwd / CbnBwd over h columns."""

    def __init__(self, d, h):
        self.nblk, self.rows_per_blk, self.R, self.C = d.nblk, d.rows_per_blk, d.R, h


# the sums a finalize folds are accumulated in double on every kernel (2^53); the passes over the rows accumulate in fp32 (2^24)
SUM_LIMITS = {"partial sums": 2.0 ** 53, "totals": 2.0 ** 53, "dslope": 2.0 ** 53}


def conditions(pl):
    """The exactness of a planted launch, from the float64 reference alone: ("" or the first byte-equal field with a value that is not its own fp32
    rounding, {sum: (sum|terms| / (largest power of two dividing all terms), the accumulator's limit)})."""
    bad = ""
    for f in pl.fields:
        if f.tol is None and f.ulps == 0 and f.dt != F64:
            e = f.exp if f.group is None else torch.cat([f.exp[f.group < 0], f.gexp])
            ne = e.float().double() != e
            if bool(ne.any()) and not bad:
                bad = f"{f.name}: element {int(ne.nonzero()[0])} = {float(e[ne][0])!r}"
    sums = {}
    for name, (sabs, t) in pl.terms.items():
        nz = t[t != 0]
        if nz.numel() == 0:
            continue
        q = (nz.abs() * 2.0 ** 20)
        assert bool((q == q.round()).all()) and float(q.max()) < 2.0 ** 62, (name, "terms are not multiples of 2^-20")
        qi = q.to(torch.int64)
        sums[name] = (float(sabs.max()) / (float((qi & -qi).min()) / 2.0 ** 20), SUM_LIMITS.get(name, float(LIMIT)))
    return bad, sums


# ------------------------------------------------------------------------------------------------ the bench: state, run, compare
Verdict = namedtuple("Verdict", "ok miss stray worst exact")     # worst: largest error / bar of the derived bars (0: all byte equality)


def _u8(t):
    return t.view(torch.uint8).reshape(-1)


def _ordered(bits):
    """fp32 bit patterns (int32) as integers that are ordered like the floats."""
    b = bits.to(torch.int64)
    return torch.where(b < 0, -(b & 0x7fffffff), b)


def compare(case, ln, fields, before, after):
    """The verdict on one launch: every field of `fields` in `after` (the arenas behind the launch, on any device) against its float64 expectation,
    per element; every byte of the checked arenas outside the fields against `before`.  A miss names case, launch, field, row, channel and values."""
    dev = _u8(after[WS]).device
    head = f"{case.name} phase {ln.phase} op {ln.op} tag {ln.tag} {KIND_NAMES[ln.kind]}"
    miss, worst, exact = "", 0.0, True
    owned = {a: torch.zeros(_u8(after[a]).numel(), dtype=torch.bool, device=dev) for a in CHECKED}
    for f in fields:
        n, es = f.exp.numel(), _esize(f.dt)
        owned[f.arena][f.off:f.off + n * es] = True
        got = _u8(after[f.arena])[f.off:f.off + n * es].view(_tdtype(f.dt))
        exp = f.exp.to(dev)
        each = torch.ones(n, dtype=torch.bool, device=dev) if f.group is None else (f.group.to(dev) < 0)
        if f.tol is not None:
            exact = False
            err = (got.double() - exp).abs()
            ratio = torch.where(err == 0, torch.zeros_like(err), err / f.tol.to(dev))
            ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
            bad = (ratio > 1) & each
            worst = max(worst, float(ratio[each].max()))
        elif f.ulps:
            exact = False
            want = exp.to(torch.float32)
            dist = (_ordered(got.view(torch.int32)) - _ordered(want.view(torch.int32))).abs().double()
            dist = torch.where(torch.isfinite(got), dist, torch.full_like(dist, float("inf")))
            bad = (dist > f.ulps) & each
            worst = max(worst, float(dist[each].max()) / f.ulps)
        else:
            want = exp if f.dt == F64 else exp.to(torch.float32).to(_tdtype(f.dt))
            ity = {2: torch.int16, 4: torch.int32, 8: torch.int64}[es]
            bad = (got.view(ity) != want.view(ity)) & each
        if bool(bad.any()) and not miss:
            e = int(bad.nonzero()[0])
            miss = (f"{head} {f.name}: row {e // f.C} channel {e % f.C} (element {e}): expected {float(exp[e])!r} device {float(got[e])!r}; "
                    f"{int(bad.sum())} elements outside the bar")
        if f.group is not None:
            grp = f.group.to(dev)
            sums = torch.zeros(f.gexp.numel(), dtype=torch.float64, device=dev).index_add_(0, grp[grp >= 0], got.double()[grp >= 0])
            gbad = ~(sums == f.gexp.to(dev))
            if bool(gbad.any()) and not miss:
                e = int(gbad.nonzero()[0])
                miss = f"{head} {f.name}: the sum over the channels of row 2 of block {e}: expected {float(f.gexp[e])!r} device {float(sums[e])!r}"
    stray = 0
    for a in CHECKED:
        ne = (_u8(after[a]) != _u8(before[a])) & ~owned[a]
        stray += int(ne.sum())
    return Verdict(not miss and stray == 0, miss, stray, worst, exact)


class Bench:
    """The arenas of one plan on `device`: `ref` (the state in front of a launch) and `work` (where it runs).  The checked arenas start as the
    background byte; plant() writes a launch's inputs into both, run() executes it in `work`, reset() puts both back."""

    def __init__(self, plan, device, run):
        self.plan, self.run_op = plan, run
        self.ref = plan.alloc_arenas(device)
        for a in CHECKED:
            _u8(self.ref[a]).fill_(BACKGROUND)
        self.ref[PARAM].zero_()
        self.work = [a.clone() for a in self.ref]
        self.dirty = []

    def put(self, arena, off, t):
        raw = _u8(t.contiguous())
        for ar in (self.ref, self.work):
            _u8(ar[arena])[off:off + raw.numel()].copy_(raw)
        self.dirty.append((arena, off, raw.numel()))

    def plant(self, pl):
        for arena, off, t in pl.puts:
            self.put(arena, off, t)

    def run(self, ln):
        self.run_op(self.plan, ln.phase, self.work, ln.op)

    def reset(self, pl, whole=False):
        """Back to the background: the planted inputs and the fields of `pl` (whole: everything - after a stray byte)."""
        for arena, off, nb in self.dirty + [(f.arena, f.off, f.exp.numel() * _esize(f.dt)) for f in pl.fields]:
            for ar in (self.ref, self.work):
                _u8(ar[arena])[off:off + nb].fill_(0 if arena == PARAM else BACKGROUND)
        self.dirty = []
        if whole:
            for a in CHECKED:
                _u8(self.work[a]).copy_(_u8(self.ref[a]))

    def restore_outputs(self, pl):
        """The fields of `pl` in `work` back to what they held in front of the launch (a finalize's repeats start from the same planted input)."""
        for f in pl.fields:
            nb = f.exp.numel() * _esize(f.dt)
            _u8(self.work[f.arena])[f.off:f.off + nb].copy_(_u8(self.ref[f.arena])[f.off:f.off + nb])


def read(arenas, arena, off, n, dt):
    """n elements of dtype code dt from byte `off` of `arena`, as float64 on the host."""
    return _u8(arenas[arena])[off:off + n * _esize(dt)].view(_tdtype(dt)).double().cpu()


def write(arenas, arena, off, t):
    raw = _u8(t.contiguous())
    _u8(arenas[arena])[off:off + raw.numel()].copy_(raw)


def run_one(case, ln, bench):
    """Launch `ln` alone from its planted state in `bench` (reset it afterwards: bench.reset(planted, whole=True))."""
    pl = plant(case, ln)
    bench.plant(pl)
    bench.run(ln)
    return pl


def geometry(ln):
    """The report's words on a launch: C, rows, blocks or chunks."""
    d = ln.d
    if ln.kind in CBN_FWD:
        return f"C {d.C:4d} rows {d.R:7d} blocks {d.nblk:5d} of {d.rows_per_blk} training {d.training} mode {d.mode}"
    if ln.kind in CBN_BWD:
        return f"C {d.C:4d} rows {d.R:7d} blocks {d.nblk:5d} of {d.rows_per_blk} skip {d.skip} dz1 {int(d.dz1.arena >= 0)} mode {d.mode}"
    if ln.kind == BN_FINALIZE:
        return f"C {d.C:4d} count {int(d.count):7d} partial rows {d.nblk:5d} nsub {max(d.nsub, 1)} mode {d.mode} chunks {chunks(ln):2d}"
    r = d if ln.kind in (BN_APPLY, BN_BWD_REDUCE) else d.r
    if ln.kind == BN_APPLY:
        return f"C {r.C:4d} rows {r.R:7d}"
    tail = f" chunks {chunks(ln):2d} pitch {r.ldp or r.C}" if ln.kind == BN_BWD_FINALIZE else ""
    return f"C {r.C:4d} rows {r.R:7d} blocks {r.nblk:5d} of {r.rows_per_blk} skip {r.skip} dz1 {int(r.dz1.arena >= 0)}" + tail


def run_case(case, device, run, only=None):
    """Every launch of `case` alone from its planted state under compare(); a finalize three times in a row from the same planted input (the same
    bytes each time), in finalize_order().  Returns [(launch, Verdict, Planted notes, conditions)] in launch order."""
    plan = plan_of(case)
    lns = select(case, launches(plan))
    assert lns, case.name
    bench = Bench(plan, device, run)
    fin = finalize_order(lns)
    out = {}
    for ln in [ln for ln in lns if ln not in fin] + fin:
        if only is not None and not only(ln):
            continue
        pl = plant(case, ln)
        bench.plant(pl)
        bench.run(ln)
        v = compare(case, ln, pl.fields, bench.ref, bench.work)
        if ln in fin and v.ok:
            first = [_u8(bench.work[f.arena])[f.off:f.off + f.exp.numel() * _esize(f.dt)].clone() for f in pl.fields]
            for rep in (2, 3):
                bench.restore_outputs(pl)
                bench.run(ln)
                again = [_u8(bench.work[f.arena])[f.off:f.off + f.exp.numel() * _esize(f.dt)] for f in pl.fields]
                v2 = compare(case, ln, pl.fields, bench.ref, bench.work)
                if not v2.ok or not all(torch.equal(x, y) for x, y in zip(first, again)):
                    v = Verdict(False, v2.miss or f"{case.name} tag {ln.tag} {KIND_NAMES[ln.kind]}: run {rep} from the same planted input gave other bytes than run 1",
                                v2.stray, max(v.worst, v2.worst), v.exact)
                    break
        out[(ln.phase, ln.op)] = (ln, v, pl.notes, conditions(pl))
        bench.reset(pl, whole=v.stray > 0)
    return [out[(ln.phase, ln.op)] for ln in lns if (ln.phase, ln.op) in out]


def report_lines(case, results):
    lines = []
    for ln, v, notes, _ in results:
        word = "MISS" if not v.ok else "exact" if v.exact else f"err/bar {v.worst:.3f}"
        lines.append(f"{case.name:12s} tag {ln.tag:4d} {KIND_NAMES[ln.kind]:16s} {geometry(ln)} {word} stray {v.stray}" + (f" {v.miss}" if v.miss else ""))
    return lines
