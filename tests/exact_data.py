"""Exact data for the weight-gradient path (a plain module, not a conftest): the cases, the integer fill, the 2^24 condition and the byte-equality
comparator shared by test_wgrad_exact_cpu.py (no GPU) and test_gpu_wgrad_exact.py.

A weight gradient is part[split][n][k] = sum over the rows m of the split of dy[m][n] * x[m][k].  The operands are bf16 (fp32 in the first layer and in
fp32 plans), every kernel accumulates in fp32 and the host simulator in double.  With operands that are small INTEGERS every product and every partial
sum is an integer, and as long as the sum of |x * dy| over the rows of a split stays below 2^24 every fp32 accumulator holds its sum exactly - in any
order of additions and for any partition of the rows.  So the device must equal the simulator byte for byte, at every split count (knob WG_NSPLIT),
and the folded gradient (SPLITSUM, UNPACK) must not depend on the split count at all.  "Close" is not a bar here: an edge tap, a pad row or the last
chunk of a run that is wrong by one product fails.

One launch per bf16 DCCRN plan is no exact sum: the first layer's fused weight gradient (kRunDyFromBn) forms dy from dz with float constants.  It keeps
the bar of opcheck.py (1e-3 of the launch's largest partial sum) and is the only exception."""
import ctypes as C
import math
import zlib
from collections import namedtuple

import torch

import opcheck
from simutil import PHASE_BWD, Plan, sim, sim_run
from util import knobs

KIND_WGRAD, KIND_UNPACK, KIND_SPLITSUM = 2, 4, 20                 # sefd_desc.h OpKind
RUN_DY_FROM_BN = 1024                                            # sefd_desc.h kRunDyFromBn
WS, PARAM, GRAD, STATE, CONST, IO = range(6)                      # sefd_amd.plan ARENA_*
CHECKED = (WS, GRAD, STATE, IO)                                   # the arenas an op may write
LIMIT = 1 << 24                                                  # integers below it are exact in fp32
ROWS = 32                                                        # sefd_desc.h kWgRows: rows per step of every weight-gradient kernel
NSPLITS = (1, 3, None, 100000)                                    # WG_NSPLIT: one workgroup per tile walks every row; uneven, a batch boundary inside a
#                                                                   split; the planner's rule; one step per split (ring shorter than its depth, empty splits)

Case = namedtuple("Case", "name model B L mode kn ru dtype knobs")
SMALL_KN, DEFAULT_KN, ODD_KN = (16, 32, 32, 64, 64, 64), (32, 64, 128, 256, 256, 256), (8, 24, 40, 72, 136, 264)
CASES = [
    Case("dccrn_small", "DCCRN", 3, 4000, "R", SMALL_KN, 128, "bf16", ()),
    Case("dccrn_default", "DCCRN", 1, 2400, "C", DEFAULT_KN, 256, "bf16", ()),
    Case("dccrn_default_wide", "DCCRN", 1, 2400, "C", DEFAULT_KN, 256, "bf16", (("WG256_MINM", "64"),)),
    Case("crn_wide", "CRN", 2, 2400, "E", DEFAULT_KN, 256, "bf16", (("WG256_MINM", "64"),)),             # the 128 x 512 tile: tags 104, 105, 400, 401
    Case("dccrn_odd", "DCCRN", 2, 3000, "E", ODD_KN, 192, "bf16", ()),                                   # the unaligned 128-wide kernel
    # the knobs of this row in test_gpu_ops.py: 256 x 256 tile, the ones MFMA, the rank-N kernel
    Case("fsn_512", "FullSubNet", 1, 11, "E", (512, 384), 0, "bf16", (("WG256_MINM", "64"), ("WGRANK_MINM", "64"), ("LSTM_ROWS_MIN", "64"))),
    Case("fsn_64", "FullSubNet", 2, 9, "E", (64, 32), 0, "bf16", ()),                                    # the unaligned kernels at Fo = 514
    Case("dccrn_small_fp32", "DCCRN", 3, 4000, "R", SMALL_KN, 128, "fp32", ()),
    Case("dccrn_small_unfused", "DCCRN", 3, 4000, "R", SMALL_KN, 128, "bf16", (("ENC0_BNFUSE", "0"),)),  # the unfused first-layer weight gradient
]


def case_id(c):
    return c.name


def make_plan(case, nsplit=None):
    """The plan of `case` under its knobs and WG_NSPLIT = nsplit (None: unset); the knobs are unset again (the planner reads them while it builds)."""
    names = [k for k, _ in case.knobs] + ["WG_NSPLIT"]
    knobs.unset(*names)
    for k, v in case.knobs:
        knobs.set(k, v)
    if nsplit is not None:
        knobs.set("WG_NSPLIT", str(nsplit))
    try:
        if case.model == "FullSubNet":
            return Plan(case.B, case.L, act_dtype=case.dtype, model="FullSubNet",
                        fsn=dict(fb_hidden=case.kn[0], sb_hidden=case.kn[1], keep=0.2, sequence_model="LSTM", norm_type="offline_laplace_norm"))
        return Plan(case.B, case.L, masking_mode=case.mode, kernel_num=case.kn, rnn_units=case.ru, act_dtype=case.dtype, model=case.model)
    finally:
        knobs.unset(*names)


# ------------------------------------------------------------------------------------------------ descriptors
class _Ptr(C.Structure):
    _fields_ = [("arena", C.c_int32), ("pad_", C.c_int32), ("off", C.c_int64)]


class _Seg(C.Structure):
    _fields_ = [("src", C.c_int32), ("dt", C.c_int32), ("off", C.c_int32), ("len", C.c_int32), ("koff", C.c_int32)]


class _RunGemm(C.Structure):
    """csrc/sefd_desc.h RunGemm up to `flags` (checked against the simulator's own reading of every descriptor: gemm())."""
    _fields_ = [("x", _Ptr * 2), ("xdt", C.c_int32), ("ydt", C.c_int32), ("bstride", C.c_int64 * 2), ("tstride", C.c_int32 * 2), ("base", C.c_int32 * 2),
                ("rowlen", C.c_int32 * 2), ("fstride", C.c_int32 * 2), ("Tin", C.c_int32 * 2), ("M", C.c_int32), ("Tout", C.c_int32), ("Fo", C.c_int32),
                ("nseg", C.c_int32), ("seg", _Seg * 8), ("w", _Ptr), ("ldw", C.c_int32), ("N", C.c_int32), ("Npad", C.c_int32), ("bias", _Ptr), ("y", _Ptr),
                ("y_bstride", C.c_int64), ("y_tstride", C.c_int32), ("y_fstride", C.c_int32), ("y_off", C.c_int32), ("stats", _Ptr), ("nsplit", C.c_int32),
                ("flags", C.c_int32)]


_OP_HEADER = 16                                                  # csrc/sefd_desc.h Op: the bytes in front of the descriptor union


def gemm(plan, i, phase=PHASE_BWD):
    """The RunGemm descriptor of op i (a copy)."""
    sz = plan.lib.sefd_op_size()
    ptr = plan.ops_ptr(phase) + i * sz
    g = _RunGemm.from_buffer_copy(C.string_at(ptr + _OP_HEADER, C.sizeof(_RunGemm)))
    f = sim().hostsim_gemm_fields
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
    v = (C.c_int64 * 8)()
    assert f(ptr, v) == 0
    o = plan.op_info(phase, i)
    assert (g.Npad, g.ldw, g.nseg, g.nsplit, g.ydt, g.M, g.N, g.xdt, g.flags & 0xffffffff) == (v[0], v[1], v[2], v[3], v[4], o["M"], o["N"], o["dtype"], o["flags"]), \
        "RunGemm layout moved: fix _RunGemm"
    return g


Launch = namedtuple("Launch", "op kind tag family g")            # g: the RunGemm of a WGRAD, else None


def wgrad_ops(plan):
    """The WGRAD, SPLITSUM and UNPACK launches of the backward phase, in order."""
    out = []
    for i in range(plan.num_ops(PHASE_BWD)):
        o = plan.op_info(PHASE_BWD, i)
        if o["kind"] in (KIND_WGRAD, KIND_SPLITSUM, KIND_UNPACK):
            out.append(Launch(i, o["kind"], o["tag"], o["family"] if o["kind"] == KIND_WGRAD else None, gemm(plan, i) if o["kind"] == KIND_WGRAD else None))
    return out


def fused(launch):
    return launch.kind == KIND_WGRAD and bool(launch.g.flags & RUN_DY_FROM_BN)


def rows_of_longest_split(g):
    """32-row steps the longest split of WGRAD `g` walks (hostsim.cpp wgrad(): the aligned bf16 kernels walk the rows per batch item)."""
    tf = g.Tout * g.Fo
    per_item = g.xdt == 1 and (g.flags & 1)
    steps = (g.M // tf) * ((tf + ROWS - 1) // ROWS) if per_item else (g.M + ROWS - 1) // ROWS
    return (steps + g.nsplit - 1) // g.nsplit


# ------------------------------------------------------------------------------------------------ fill
def _buffers(plan):
    return [(n,) + plan.buffer(n) for n in plan.buffer_names()]


def fill(plan, arenas, seed=20):
    """Every named buffer of the workspace and the I/O arena: integers uniform in -3 .. 3 from a seeded generator (no pattern, so nothing is symmetric
    in any index: a swapped tap or channel shows), in the buffer's own dtype.  The parameters (read by the one fused launch only): uniform in (-1, 1).
    The constant arena (zero and ones pages, tables) is the plan's own."""
    g = torch.Generator()
    for name, a, off, nb, dt in _buffers(plan):
        if a not in (WS, IO) or nb <= 0:
            continue
        g.manual_seed(seed + zlib.crc32(name.encode()))          # per buffer: the same data at every split count, whatever the partial sums' size
        n = nb // (2 if dt == opcheck.BF16 else 4)
        v = torch.randint(-3, 4, (n,), generator=g).to(torch.bfloat16 if dt == opcheck.BF16 else torch.float32)
        arenas[a].view(torch.uint8)[off:off + v.numel() * v.element_size()].copy_(v.view(torch.uint8))
    g.manual_seed(seed)
    arenas[PARAM].copy_(torch.rand(arenas[PARAM].numel(), generator=g) * 2 - 1)


def absolute(plan, arenas):
    """A copy of `arenas` with every named workspace / I/O buffer replaced by its absolute values."""
    out = [a.clone() for a in arenas]
    for name, a, off, nb, dt in _buffers(plan):
        if a in (WS, IO) and nb > 0:
            n = nb // (2 if dt == opcheck.BF16 else 4) * (2 if dt == opcheck.BF16 else 4)
            v = out[a].view(torch.uint8)[off:off + n].view(torch.bfloat16 if dt == opcheck.BF16 else torch.float32)
            v.copy_(v.abs())
    return out


def partials(plan, arenas, g):
    """The fp32 partial sums [nsplit][Npad][ldw] of WGRAD `g` inside the workspace arena (a view)."""
    n = g.nsplit * g.Npad * g.ldw
    assert g.w.arena == WS
    return arenas[WS].view(torch.uint8)[g.w.off:g.w.off + 4 * n].view(torch.float32).view(g.nsplit, g.Npad, g.ldw)


def exact_sum_bound(plan, arenas, launch):
    """The 2^24 condition of one WGRAD launch, measured and not assumed: the simulator's launch over the ABSOLUTE values of the operands gives, per split
    and element, the sum of |x * dy| over the split's rows; the largest of them bounds every intermediate sum of any order of additions.  Returns it."""
    assert launch.kind == KIND_WGRAD and not fused(launch)
    ab = absolute(plan, arenas)
    sim_run(plan, PHASE_BWD, ab, launch.op, launch.op + 1)
    return float(partials(plan, ab, launch.g).max())


def fed_by_fused(plan, launches, arenas, run):
    """Mask over the flat gradient arena: the elements the fused first-layer launch feeds - float sums, which may move with the partition of the rows.
    Marked partial sums of that launch alone, gathered by the plan's own UNPACK launches; run(arenas, op) executes one (simulator or device)."""
    ar = [a.clone() for a in arenas]
    a, off, nb, dt = plan.buffer(opcheck.PARTIALS)
    ar[WS].view(torch.uint8)[off:off + nb].zero_()
    ar[GRAD].zero_()
    for ln in launches:
        if fused(ln):
            part = partials(plan, ar, ln.g)
            part.copy_(torch.rand(part.shape, generator=torch.Generator().manual_seed(5)) + 1)      # (no two entries of a signed sum cancel)
    for ln in launches:
        if ln.kind == KIND_UNPACK:
            run(ar, ln.op)
    return ar[GRAD] != 0


# ------------------------------------------------------------------------------------------------ comparator
# ok: no miss and no stray byte; miss: text of the first differing element ("" = none); stray: bytes the device changed outside every region either side
# was expected to change; worst: err / tol of the one launch held to opcheck's bar (0 elsewhere)
Verdict = namedtuple("Verdict", "ok miss stray worst")


def _u8(t):
    return t.view(torch.uint8).reshape(-1)


def float_slices(launches):
    """[(first byte, end byte, end byte of split 0) in the workspace arena] of the partial sums that hold float sums: those of the fused first-layer launch."""
    return [(ln.g.w.off, ln.g.w.off + 4 * ln.g.nsplit * ln.g.Npad * ln.g.ldw, ln.g.w.off + 4 * ln.g.Npad * ln.g.ldw) for ln in launches if fused(ln)]


def compare_exact(plan, launch, before, simulated, device, loose=()):
    """The verdict on one launch.  before / simulated / device: the arenas (lists indexed by arena, on any torch device) in front of the launch, after it
    on the simulator and after it on the device.  Over every named buffer and every arena that either side changed the device must equal the simulator
    byte for byte; a byte the device changed where the simulator changed nothing is a stray byte.  A miss names the first differing element: for a WGRAD
    the split and (n, k) of the packed matrix, both values; else the buffer (or gradient tensor) and the element.
    loose: float_slices() of the plan.  The block of them that the launch writes - the fused first-layer launch every split (its kernel stores the whole
    block), the SPLITSUM that folds them, in another order of additions than the simulator's, split 0 - is held to opcheck's bar, max|device - simulator|
    below 1e-3 of the block's largest element, over EVERY element of the block (which of them the simulator's value happens to leave as it was plays no
    part); everything outside that block is held to byte equality in those launches too."""
    miss, stray, worst = "", 0, 0.0
    regions = [(n, a, off, nb) for n, a, off, nb, dt in _buffers(plan) if nb > 0] + [("A_GRAD", GRAD, 0, plan.arena_bytes[GRAD]), ("A_STATE", STATE, 0, plan.arena_bytes[STATE])]
    covered = {a: torch.zeros(_u8(before[a]).numel(), dtype=torch.bool, device=_u8(before[a]).device) for a in CHECKED}
    for name, a, off, nb in regions:
        p, s, d = (_u8(x[a])[off:off + nb] for x in (before, simulated, device))
        covered[a][off:off + nb] = True
        if torch.equal(s, d):
            continue
        if torch.equal(s, p):                                    # a region the simulator left alone
            stray += int((d != p).sum())
            continue
        if name == opcheck.PARTIALS and loose and launch.kind in (KIND_WGRAD, KIND_SPLITSUM):
            s, d = s.clone(), d.clone()                          # (the slices are taken out of the exact comparison below)
            for lo, hi_all, hi_first in loose:
                lo, hi = max(lo - off, 0), min((hi_all if launch.kind == KIND_WGRAD else hi_first) - off, nb)
                if hi <= lo or (launch.kind == KIND_WGRAD and not fused(launch)):
                    continue
                sf, df = (x[lo:hi].view(torch.float32).double().cpu() for x in (s, d))
                err, own = opcheck.measure(sf, df, False)
                worst = max(worst, err / 1e-3)
                if not err < 1e-3 and not miss:
                    miss = f"{name}+{lo // 4}: err {err:.3e} of the largest element {own:.3e}: opcheck's bar 1e-3 (float sums of the fused first-layer launch)"
                d[lo:hi] = s[lo:hi]
            if torch.equal(s, d):
                continue
        n4 = nb // 4 * 4
        ne = (s[:n4].view(torch.int32) != d[:n4].view(torch.int32)) if n4 else torch.zeros(0, dtype=torch.bool)
        if miss:
            continue
        if n4 and bool(ne.any()):
            e = int(torch.nonzero(ne)[0])                        # first differing 4-byte element of the region
            sv, dv, pv = (float(x[:n4].view(torch.float32)[e]) for x in (s, d, p))
            if name == opcheck.PARTIALS and launch.kind == KIND_WGRAD:
                g = launch.g
                rel = e - (g.w.off - off) // 4
                sz = g.Npad * g.ldw
                if 0 <= rel < g.nsplit * sz:
                    miss = (f"{name}: split {rel // sz} of {g.nsplit} n {rel % sz // g.ldw} k {rel % g.ldw}: simulator {sv!r} device {dv!r} (before {pv!r}); "
                            f"tag {launch.tag} family {launch.family} M {g.M} N {g.N} Npad {g.Npad} ldw {g.ldw} Tout {g.Tout} Fo {g.Fo}")
                else:
                    miss = f"{name}: element {e} outside the launch's partial sums: simulator {sv!r} device {dv!r} (before {pv!r})"
            elif a == GRAD:
                t = next((k for k, (o, shp) in plan.params.items() if o <= e < o + math.prod(shp)), "?")
                miss = f"A_GRAD element {e} ({t}): simulator {sv!r} device {dv!r} (before {pv!r})"
            else:
                miss = f"{name}: 4-byte element {e}: simulator {sv!r} device {dv!r} (before {pv!r})"
        else:
            miss = f"{name}: the last {nb - n4} bytes differ"
    for a in CHECKED:                                            # bytes of an arena outside every named buffer
        rest = ~covered[a]
        if bool(rest.any()):
            p, s, d = (_u8(x[a])[rest] for x in (before, simulated, device))
            if not torch.equal(s, d):
                stray += int((d != s).sum())
    return Verdict(not miss and stray == 0, miss, stray, worst)


def run_launches(plan, launches, device, host=None, stop_at_first=False):
    """Run `launches` in order on the device arenas - and, with `host` (the same state on the host), on the simulator from the same pre-launch state,
    under compare_exact.  Whole arenas are compared on the device (one upload of the simulator's state per launch); only a launch that differs is taken
    apart.  After a launch that differs - the fused one always may - the host state becomes the device's.  Returns [(launch, Verdict)]."""
    out, loose = [], float_slices(wgrad_ops(plan))
    for ln in launches:
        if host is None:
            plan.run(PHASE_BWD, device, 0, ln.op, ln.op + 1)
            continue
        before = {a: device[a].clone() for a in CHECKED}
        sim_run(plan, PHASE_BWD, host, ln.op, ln.op + 1)
        plan.run(PHASE_BWD, device, 0, ln.op, ln.op + 1)
        torch.cuda.synchronize()
        up = {a: host[a].to(device[a].device) for a in CHECKED}
        if all(torch.equal(_u8(up[a]), _u8(device[a])) for a in CHECKED):
            out.append((ln, Verdict(True, "", 0, 0.0)))
            continue
        v = compare_exact(plan, ln, before, up, device, loose)
        out.append((ln, v))
        for a in CHECKED:
            host[a].copy_(device[a])
        if stop_at_first and not v.ok:
            break
    return out
