"""Exact data for the conv GEMM kernels (a plain module, not a conftest): the cases, the integer fills, the 2^24 conditions and the byte-equality
comparator shared by test_wgrad_exact_cpu.py / test_gpu_wgrad_exact.py (weight gradients) and test_rungemm_exact_cpu.py / test_gpu_rungemm_exact.py (the
forward and input-gradient launches, OP_RUNGEMM of both phases).

Weight gradients.  part[split][n][k] = sum over the rows m of the split of dy[m][n] * x[m][k].  The operands are bf16 (fp32 in the first layer and in
fp32 plans), every kernel accumulates in fp32 and the host simulator in double.  With operands that are small INTEGERS every product and every partial
sum is an integer, and as long as the sum of |x * dy| over the rows of a split stays below 2^24 every fp32 accumulator holds its sum exactly - in any
order of additions and for any partition of the rows.  So the device must equal the simulator byte for byte, at every split count (knob WG_NSPLIT),
and the folded gradient (SPLITSUM, UNPACK) must not depend on the split count at all.  "Close" is not a bar here: an edge tap, a pad row or the last
chunk of a run that is wrong by one product fails.

One launch per bf16 DCCRN plan is no exact sum: the first layer's fused weight gradient (kRunDyFromBn) forms dy from dz with float constants.  It keeps
the bar of opcheck.py (1e-3 of the launch's largest partial sum) and is the only exception of that half.

Forward and input gradients.  hostsim.cpp rungemm(): v = (float)(sum_k a[m][k] * w[n][k]) + bias[n], + y under kRunAccum, max(v, 0) under kRunRelu,
stored in ydt (bf16: round to nearest even); with `stats`, per 128-row block and column the sums of v and of v * v as fp32.  The state (fill_exact):
every named workspace / I/O buffer integers in -3 .. 3 (activations, cotangents, prior y), the parameter arena integers in -1 .. 1, and the packed
weights and biases written from those parameters by the plan's OWN PACK launches on the simulator (a kernel is entitled to the zero pad columns and
the zero pad K that PACK writes).  Every launch starts from that one state (launches are not chained: chained outputs would leave the exact range).
Measured per launch on the simulator alone (conditions()): (a) every value written is an integer, (b) the launch over the ABSOLUTE values of operands,
bias and prior y stays below 2^24 - which bounds every partial sum of every grouping of k, for every MFMA shape -, (c) every statistics sum of squares
stays below 2^24 (non-negative integer terms, and |sum v| <= sum v * v).  Then every kernel family must equal the simulator byte for byte at every
grid, and two families that both do are equal to each other.  The one exception of this half: the statistics rows of a kRunBnBwd launch are
BatchNorm-backward sums formed with the layer's mean_invstd and branch tests; they keep opcheck.tolerance()'s bar over every element of those rows
(the y / y2 the launch stores is held to byte equality)."""
import contextlib
import ctypes as C
import math
import zlib
from collections import namedtuple

import torch

import opcheck
from simutil import PHASE_BWD, PHASE_FWD, Plan, sim, sim_run
from util import knobs

KIND_RUNGEMM, KIND_WGRAD, KIND_PACK, KIND_UNPACK, KIND_SPLITSUM, KIND_PACKMULTI = 1, 2, 3, 4, 20, 38      # sefd_desc.h OpKind
RUN_ACCUM, RUN_RELU, RUN_BN_BWD = 2, 4, 64                       # sefd_desc.h kRunAccum, kRunRelu, kRunBnBwd
RUN_DY_FROM_BN = 1024                                            # sefd_desc.h kRunDyFromBn
KBM = 128                                                        # sefd_desc.h kBM: rows per statistics block
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


def _construct(case):
    if case.model == "FullSubNet":
        return Plan(case.B, case.L, act_dtype=case.dtype, model="FullSubNet",
                    fsn=dict(fb_hidden=case.kn[0], sb_hidden=case.kn[1], keep=0.2, sequence_model="LSTM", norm_type="offline_laplace_norm"))
    return Plan(case.B, case.L, masking_mode=case.mode, kernel_num=case.kn, rnn_units=case.ru, act_dtype=case.dtype, model=case.model)


def make_plan(case, nsplit=None):
    """The plan of `case` under its knobs and WG_NSPLIT = nsplit (None: unset); the knobs are unset again (the planner reads them while it builds)."""
    names = [k for k, _ in case.knobs] + ["WG_NSPLIT"]
    knobs.unset(*names)
    for k, v in case.knobs:
        knobs.set(k, v)
    if nsplit is not None:
        knobs.set("WG_NSPLIT", str(nsplit))
    try:
        return _construct(case)
    finally:
        knobs.unset(*names)


# The arms of the RUNGEMM tier: the knobs under which a case's plan is built AND its launches run (launch_rungemm reads most of them per launch, so
# they stay set for as long as the plan is used: under()).
_GRIDS = (1, 3, 0)                                               # one workgroup walks everything; uneven runs; the resident grid
ARMS = dict(
    # every other family switched off: per launch RG_PERSIST, THIN_MASK, THIN_STAGE and a DIRECT_MINM above every M; at planning CG256 and ENC0_DIRECT
    tiled=dict(RG_PERSIST="0", THIN_MASK="0", THIN_STAGE="0", DIRECT_MINM=str(2 ** 31 - 1), CG256="0", ENC0_DIRECT="0"),
    default={},
    **{f"persist_g{g}": dict(RG_PERSIST="2", RG_PERSIST_GRID=str(g)) for g in _GRIDS},
    **{f"thin_g{g}": dict(THIN_MASK="2", THIN_STAGE="2", THIN_MASK_GRID=str(g), THIN_STAGE_GRID=str(g)) for g in _GRIDS},
    direct=dict(DIRECT_MINM="64"),
    wide=dict(CG256_MINM="64"),                                  # (BN_FUSE=1 fuses no layer at the cases' sizes: no kRunBnBwd here, see wide_bnfuse2)
    bnfuse2=dict(BN_FUSE="2"),                                   # kRunBnBwd on rungemm_kernel (the persistent form refuses the epilogue)
    # ... and on the other two kernels that instantiate the epilogue: cgemm256 - the only one the product runs by default, where BN_FUSE=1 fuses the
    # wide-tile layers of at least 8192 rows, more than any case has - and thin.hip
    wide_bnfuse2=dict(CG256_MINM="64", BN_FUSE="2"),
    direct_bnfuse2=dict(DIRECT_MINM="64", BN_FUSE="2"),
)


# knobs that no planner reads (csrc/rungemm_persist.hip, thin_mask.hip, thin_stage.hip, thin.hip read them per launch): arms that differ in these
# alone share one plan of the case (building the default-size plan with its constant arena takes longer than simulating it); one case's plans at a time
_PER_LAUNCH = {"RG_PERSIST", "RG_PERSIST_GRID", "THIN_MASK", "THIN_MASK_GRID", "THIN_STAGE", "THIN_STAGE_GRID", "DIRECT_MINM"}
_plans = {}


@contextlib.contextmanager
def under(case, arm):
    """The plan of `case` built under its knobs and those of ARMS[arm], which stay set inside the block (op_info()["family"] and the launches read them)."""
    kn = dict(case.knobs)
    kn.update(ARMS[arm])
    knobs.unset(*kn)
    for k, v in kn.items():
        knobs.set(k, v)
    try:
        key = (case.name,) + tuple(sorted((k, v) for k, v in kn.items() if k not in _PER_LAUNCH))
        if key not in _plans:
            for k in [k for k in _plans if k[0] != case.name]:
                del _plans[k]
            _plans[key] = _construct(case)
        yield _plans[key]
    finally:
        knobs.unset(*kn)


_GRID_KNOB = {5: "RG_PERSIST_GRID", 6: "THIN_MASK_GRID", 7: "THIN_STAGE_GRID"}      # sefd_amd.plan RUN_FAMILY_PERSIST, _THIN_MASK, _THIN_STAGE


def launch_key(launch, arm):
    """What an arm runs of one launch: the launch itself (phase, tag, geometry, flags, destinations, statistics), the family it takes and, on a
    family whose grid a knob forces, that grid (0: the resident grid)."""
    g = launch.g
    grid = int(ARMS[arm].get(_GRID_KNOB.get(launch.family, ""), 0))
    return launch.phase, launch.tag, g.M, g.N, launch.K, g.flags, g.n2, g.stats.arena >= 0, launch.family, grid


# The arms that arms_of() below drops, per case - the table the (case, arm) pairs of both test files are built from at collection; that it is what
# the rule gives on the host from op_info is asserted in test_rungemm_exact_cpu.py:
#   the CRN has no first layer on the spectrum, no layer for the wide tile at these sizes and no BatchNorm-backward fusion (default = tiled; wide; bnfuse2);
#   the odd channel counts fit neither the first-layer kernel nor the frame-staged ones (default = tiled; thin_*);
#   FullSubNet's GEMMs are dense layers: fsn_512's input gradients fit the persistent form, nothing else of either plan moves;
#   an fp32 plan runs rungemm_kernel<float> alone (bnfuse2 adds the kRunBnBwd epilogue to it).
#   in the small DCCRN the wide tile takes no layer that BN_FUSE=2 fuses: wide_bnfuse2 = the launches of wide and of bnfuse2.
DROPPED = {
    "dccrn_small": ["wide_bnfuse2"],
    "dccrn_small_unfused": ["wide_bnfuse2"],
    "crn_wide": ["default", "wide", "bnfuse2", "wide_bnfuse2", "direct_bnfuse2"],
    "dccrn_odd": ["default", "thin_g1", "thin_g3", "thin_g0"],
    "fsn_512": ["default", "thin_g1", "thin_g3", "thin_g0", "direct", "wide", "bnfuse2", "wide_bnfuse2", "direct_bnfuse2"],
    "fsn_64": [a for a in ARMS if a != "tiled"],
    "dccrn_small_fp32": [a for a in ARMS if a not in ("tiled", "bnfuse2")],
}
PAIRS = [(case, arm) for case in CASES for arm in ARMS if arm not in DROPPED.get(case.name, ())]      # case-major: ExactState shares results inside a case


def pair_id(v):
    return v.name if isinstance(v, Case) else str(v)


_arms = {}


def arms_of(case):
    """(the arms kept for `case`, [dropped arms]), decided on the host from op_info: in the order of ARMS, an arm is dropped where it gives no launch
    a family (or a forced grid on that family) that the arms already kept for the case do not give it - it would run the same kernels on the same
    descriptors again."""
    if case.name not in _arms:
        kept, dropped, seen = [], [], set()
        for arm in ARMS:
            with under(case, arm) as plan:
                keys = {launch_key(ln, arm) for ln in run_ops(plan)}
            if keys <= seen:
                dropped.append(arm)
            else:
                kept.append(arm)
                seen |= keys
        _arms[case.name] = (kept, dropped)
    return _arms[case.name]


_simulated = {}                                                  # one case at a time: {(case, buffer table, phase, descriptor bytes): (regions written, Conditions)}


class ExactState:
    """fill_exact's state of `plan` on the host, its absolute values, and a working copy of each: every launch is simulated from the one state.
    key (a case's name): the arms of a case mostly run the SAME descriptors over the same buffers on other kernels (the family knobs are read per
    launch), so the simulator's result of a launch - the regions it wrote - and its conditions are kept per (buffer table, descriptor) and reused by
    the next arm of the case; the results of another case are dropped."""

    def __init__(self, plan, key=None):
        self.plan = plan
        self.saved = plan.alloc_arenas("cpu")
        fill_exact(plan, self.saved)
        self.work = [a.clone() for a in self.saved]
        self.abs_saved = self.abs_work = None
        self.key = None if key is None else (key, tuple(_buffers(plan)))
        if key is not None and any(k[0] != key for k in _simulated):
            _simulated.clear()
        self.cond, self.notes = None, {}
        self._unnamed = None

    def _rest(self):
        """{arena: mask of the bytes outside every named buffer} of the workspace and the I/O arena."""
        if self._unnamed is None:
            self._unnamed = {}
            for a in (WS, IO):
                m = torch.ones(_u8(self.saved[a]).numel(), dtype=torch.bool)
                for _, ba, off, nb, _ in _buffers(self.plan):
                    if ba == a and nb > 0:
                        m[off:off + nb] = False
                self._unnamed[a] = m
        return self._unnamed

    def simulate(self, launch):
        """The arenas behind the simulator's launch from the saved state (the working copy: valid until the next call); its conditions in self.cond."""
        for a in CHECKED:
            self.work[a].copy_(self.saved[a])
        k = None if self.key is None else self.key + (launch.phase, bytes(launch.g))
        self.fresh = k not in _simulated                          # False: this very launch was simulated before, under another arm of the case
        if not self.fresh:
            wrote, self.cond, self.notes = _simulated[k]
            for a, off, v in wrote:
                _u8(self.work[a])[off:off + v.numel()].copy_(v)
            return self.work
        sim_run(self.plan, launch.phase, self.work, launch.op, launch.op + 1)
        if self.abs_saved is None:
            self.abs_saved = absolute_exact(self.plan, self.saved)
            self.abs_work = [a.clone() for a in self.abs_saved]
        self.cond = conditions(self.plan, launch, self.saved, self.work, self.abs_saved, self.abs_work)
        self.notes = {}                                           # what a caller keeps with the launch's result (the comparator's verdict on it)
        if k is not None:
            for a, m in self._rest().items():                     # the replay below restores named buffers only: nothing else may have been written
                assert not bool(((_u8(self.work[a]) != _u8(self.saved[a])) & m).any()), (launch.tag, "the simulator wrote outside every named buffer of arena", a)
            regions = [(a, off, nb) for _, a, off, nb, _ in _buffers(self.plan) if nb > 0 and a in CHECKED] + [(a, 0, self.plan.arena_bytes[a]) for a in (GRAD, STATE)]
            _simulated[k] = ([(a, off, _u8(self.work[a])[off:off + nb].clone()) for a, off, nb in regions
                              if not torch.equal(_u8(self.work[a])[off:off + nb], _u8(self.saved[a])[off:off + nb])], self.cond, self.notes)
        return self.work


# ------------------------------------------------------------------------------------------------ descriptors
class _Ptr(C.Structure):
    _fields_ = [("arena", C.c_int32), ("pad_", C.c_int32), ("off", C.c_int64)]


class _Seg(C.Structure):
    _fields_ = [("src", C.c_int32), ("dt", C.c_int32), ("off", C.c_int32), ("len", C.c_int32), ("koff", C.c_int32)]


class _RunGemm(C.Structure):
    """csrc/sefd_desc.h RunGemm up to `y2` (checked against the simulator's own reading of every descriptor: gemm())."""
    _fields_ = [("x", _Ptr * 2), ("xdt", C.c_int32), ("ydt", C.c_int32), ("bstride", C.c_int64 * 2), ("tstride", C.c_int32 * 2), ("base", C.c_int32 * 2),
                ("rowlen", C.c_int32 * 2), ("fstride", C.c_int32 * 2), ("Tin", C.c_int32 * 2), ("M", C.c_int32), ("Tout", C.c_int32), ("Fo", C.c_int32),
                ("nseg", C.c_int32), ("seg", _Seg * 8), ("w", _Ptr), ("ldw", C.c_int32), ("N", C.c_int32), ("Npad", C.c_int32), ("bias", _Ptr), ("y", _Ptr),
                ("y_bstride", C.c_int64), ("y_tstride", C.c_int32), ("y_fstride", C.c_int32), ("y_off", C.c_int32), ("stats", _Ptr), ("nsplit", C.c_int32),
                ("flags", C.c_int32), ("zero", _Ptr), ("div", C.c_uint32 * 4), ("bnb_y", _Ptr), ("bnb_mi", _Ptr), ("bnb_gamma", _Ptr), ("bnb_beta", _Ptr),
                ("bnb_slope", _Ptr), ("bnb_bstride", C.c_int64), ("bnb_tstride", C.c_int32), ("bnb_fstride", C.c_int32), ("bnb_off", C.c_int32),
                ("n2", C.c_int32), ("y2", _Ptr)]


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
    t = sim().hostsim_gemm_tail
    t.restype, t.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
    w = (C.c_int64 * 16)()
    assert t(ptr, w) == 0
    mine = (g.n2, g.y2.arena, g.y2.off, g.stats.arena, g.stats.off, g.bnb_y.arena, g.bnb_y.off, g.bnb_bstride, g.bnb_tstride, g.bnb_fstride, g.bnb_off,
            g.bnb_mi.arena, g.bnb_mi.off, g.bias.arena, g.bias.off, g.y.off)
    assert mine == tuple(w) and g.n2 == v[5], f"RunGemm layout moved behind `flags`: fix _RunGemm ({mine} against the simulator's {tuple(w)})"
    return g


# g: the RunGemm of a WGRAD / RUNGEMM, else None; phase, K: filled by run_ops() (the weight-gradient launches all belong to the backward phase)
Launch = namedtuple("Launch", "op kind tag family g phase K", defaults=(PHASE_BWD, 0))


def wgrad_ops(plan):
    """The WGRAD, SPLITSUM and UNPACK launches of the backward phase, in order."""
    out = []
    for i in range(plan.num_ops(PHASE_BWD)):
        o = plan.op_info(PHASE_BWD, i)
        if o["kind"] in (KIND_WGRAD, KIND_SPLITSUM, KIND_UNPACK):
            out.append(Launch(i, o["kind"], o["tag"], o["family"] if o["kind"] == KIND_WGRAD else None, gemm(plan, i) if o["kind"] == KIND_WGRAD else None))
    return out


def run_ops(plan):
    """The RUNGEMM launches of both phases, in order, with the family a launch would pick under the knobs of the moment."""
    out = []
    for phase in (PHASE_FWD, PHASE_BWD):
        for i in range(plan.num_ops(phase)):
            o = plan.op_info(phase, i)
            if o["kind"] == KIND_RUNGEMM:
                out.append(Launch(i, KIND_RUNGEMM, o["tag"], o["family"], gemm(plan, i, phase), phase, o["K"]))
    return out


def fused(launch):
    return launch.kind == KIND_WGRAD and bool(launch.g.flags & RUN_DY_FROM_BN)


def bn_bwd(launch):
    """A RUNGEMM whose statistics rows are BatchNorm-backward sums (kRunBnBwd): the one region of that tier outside byte equality."""
    return launch.kind == KIND_RUNGEMM and bool(launch.g.flags & RUN_BN_BWD) and launch.g.stats.arena >= 0


def stats_range(g):
    """(arena, first byte, end byte, rows per block) of the statistics rows [blocks][2 or 3][Npad] fp32 that RUNGEMM `g` writes, or None."""
    if g.stats.arena < 0:
        return None
    nst = 3 if g.flags & RUN_BN_BWD else 2
    return g.stats.arena, g.stats.off, g.stats.off + 4 * ((g.M + KBM - 1) // KBM) * nst * g.Npad, nst


def row_of(g, m):
    """(batch item, frame u, bin fo) of row m."""
    tf = g.Tout * g.Fo
    return m // tf, m % tf // g.Fo, m % g.Fo


def dest_index(g, device="cpu"):
    """[(Ptr of the destination, element indices [M][columns] from that Ptr on, first GEMM column)] of RUNGEMM `g`: y, and y2 where n2 > 0
    (hostsim.cpp rungemm(): columns n >= n2 go to y2 at column n - n2 with the same row offsets)."""
    m = torch.arange(g.M, dtype=torch.int64, device=device)
    tf = g.Tout * g.Fo
    row = (m // tf) * g.y_bstride + (m % tf // g.Fo) * g.y_tstride + (m % g.Fo) * g.y_fstride + g.y_off
    n1 = g.n2 if g.n2 > 0 else g.N
    out = [(g.y, row[:, None] + torch.arange(n1, dtype=torch.int64, device=device), 0)]
    if g.n2 > 0:
        out.append((g.y2, row[:, None] + torch.arange(g.N - g.n2, dtype=torch.int64, device=device), g.n2))
    return out


def operand(g, s, b, u, fo, j):
    """(arena, byte offset of the source, element index) of run element (s, j) of row (b, u, fo), or None where the row reads a zero (hostsim.cpp a_elem)."""
    sg = g.seg[s]
    if sg.src < 0 or not 0 <= j < sg.len:
        return None
    tt, r = u + sg.dt, sg.off + fo * g.fstride[sg.src] + j
    if not 0 <= tt < g.Tin[sg.src] or not 0 <= r < g.rowlen[sg.src]:
        return None
    return g.x[sg.src].arena, g.x[sg.src].off, b * g.bstride[sg.src] + tt * g.tstride[sg.src] + g.base[sg.src] + r


def typed(ar, arena, off, dt):
    """The arena from byte `off` on as elements of dtype code `dt`."""
    raw = ar[arena].view(torch.uint8)[off:]
    return raw[:raw.numel() // 4 * 4].view(torch.bfloat16 if dt == 1 else torch.float32)


RUN_FAMILIES = {"enc0": 1, "cgemm256": 2, "direct": 3, "tiled": 4, "persist": 5, "thin_mask": 6, "thin_stage": 7}     # sefd_amd.plan RUN_FAMILY_*
RUN_FAMILY_NAMES = {v: k for k, v in RUN_FAMILIES.items()}


def buffer_at(plan, arena, off):
    """(name, arena, offset, bytes, dtype code) of the named buffer that holds byte `off` of `arena`."""
    for r in _buffers(plan):
        if r[1] == arena and r[2] <= off < r[2] + r[3]:
            return r
    raise KeyError((arena, off))


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


def fill_exact(plan, arenas, seed=20):
    """The state every RUNGEMM launch starts from, on host arenas: fill()'s integers in -3 .. 3 in every named workspace / I/O buffer (activations,
    cotangents, the prior y of an accumulating launch, mean_invstd), integers in -1 .. 1 in the parameter arena, then the plan's own PACK launches of
    both phases on the simulator: the packed weights are integers in -1 .. 1 and the combined biases (b_r - b_i, b_ih + b_hh) in -2 .. 2, with the zero
    pad columns and zero pad K that PACK writes.  The constant arena is the plan's own."""
    fill(plan, arenas, seed)
    g = torch.Generator().manual_seed(seed)
    arenas[PARAM].copy_(torch.randint(-1, 2, (arenas[PARAM].numel(),), generator=g).float())
    packs = 0
    for phase in (PHASE_FWD, PHASE_BWD):
        for i in range(plan.num_ops(phase)):
            if plan.op_info(phase, i)["kind"] in (KIND_PACK, KIND_PACKMULTI):
                sim_run(plan, phase, arenas, i, i + 1)
                packs += 1
    assert packs > 0 or not plan.params


def absolute_exact(plan, arenas):
    """absolute() and the parameter arena's absolute values: the operands, biases and prior y of every RUNGEMM (packed weights are copies, differences
    and sums of parameters: PACK is not run again, the packed values themselves are taken absolute)."""
    out = absolute(plan, arenas)
    out[PARAM].abs_()
    return out


# integers: "" or the first region of the launch's writes that holds a non-integer; bound: the largest value the launch over the absolute values
# stores to y / y2 (widened by one bf16 rounding where y is bf16); sumsq: the largest statistics sum of squares written (0: no statistics or kRunBnBwd)
Conditions = namedtuple("Conditions", "integers bound sumsq")


def conditions(plan, launch, state, simulated, abs_state, abs_work):
    """Conditions (a) to (c) of one RUNGEMM launch, from the simulator alone.  state / simulated: the arenas in front of and behind the simulator's
    launch; abs_state: absolute_exact(state); abs_work: arenas equal to abs_state on entry and on return (the launch runs in them)."""
    g, st = launch.g, stats_range(launch.g)
    # (b) bounds the launch only if every operand was made absolute: absolute_exact() covers the named workspace / I/O buffers and the parameter arena
    reads = [g.w] + [g.x[g.seg[s].src] for s in range(g.nseg) if g.seg[s].src >= 0] + ([g.bias] if g.bias.arena >= 0 else [])
    reads += [ptr for ptr, _, _ in dest_index(g)] if g.flags & RUN_ACCUM else []
    for ptr in reads:
        assert ptr.arena == PARAM or (ptr.arena in (WS, IO) and buffer_at(plan, ptr.arena, ptr.off)), (launch.tag, "an operand outside the absolute state", ptr.arena, ptr.off)
    bad = ""
    for name, a, off, nb, dt in _buffers(plan) + [("A_GRAD", GRAD, 0, plan.arena_bytes[GRAD], 0), ("A_STATE", STATE, 0, plan.arena_bytes[STATE], 0)]:
        if nb <= 0 or a not in CHECKED:
            continue
        p, s = (_u8(x[a])[off:off + nb] for x in (state, simulated))
        if torch.equal(p, s):
            continue
        es = 2 if dt == opcheck.BF16 else 4
        v = s[:nb // es * es].view(torch.bfloat16 if dt == opcheck.BF16 else torch.float32).double()
        ok = torch.isfinite(v) & (v == v.round())
        if bn_bwd(launch) and a == st[0] and dt != opcheck.BF16:    # the rows outside byte equality are outside this condition too
            lo, hi = max(st[1] - off, 0) // 4, max(min(st[2] - off, nb), 0) // 4
            ok[lo:hi] = True
        if not bool(ok.all()) and not bad:
            bad = f"{name}: element {int((~ok).nonzero()[0])} = {float(v[(~ok).nonzero()[0]])!r}"
    sim_run(plan, launch.phase, abs_work, launch.op, launch.op + 1)
    bound = 0.0
    for ptr, idx, _ in dest_index(g):
        es = 2 if g.ydt == opcheck.BF16 else 4
        y = _u8(abs_work[ptr.arena])[ptr.off:]
        y = y[:y.numel() // es * es].view(torch.bfloat16 if g.ydt == opcheck.BF16 else torch.float32)
        bound = max(bound, float(y[idx.reshape(-1)].double().max()) * (1 + 2.0 ** -8 if g.ydt == opcheck.BF16 else 1))
    for a in CHECKED:
        abs_work[a].copy_(abs_state[a])
    sumsq = 0.0
    if st is not None and not bn_bwd(launch):
        rows = _u8(simulated[st[0]])[st[1]:st[2]].view(torch.float32).view(-1, 2, g.Npad)
        sumsq = float(rows[:, 1].max())
        assert float(rows[:, 1].min()) >= 0 and bool((rows[:, 0].abs() <= rows[:, 1]).all()), (launch.tag, "statistics rows are not (sum, sum of squares)")
    return Conditions(bad, bound, sumsq)


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
# loose: the launch has a region held to opcheck's bar instead of byte equality (the statistics rows of a kRunBnBwd RUNGEMM)
Verdict = namedtuple("Verdict", "ok miss stray worst loose", defaults=(False,))


def _u8(t):
    return t.view(torch.uint8).reshape(-1)


def float_slices(launches):
    """[(first byte, end byte, end byte of split 0) in the workspace arena] of the partial sums that hold float sums: those of the fused first-layer launch."""
    return [(ln.g.w.off, ln.g.w.off + 4 * ln.g.nsplit * ln.g.Npad * ln.g.ldw, ln.g.w.off + 4 * ln.g.Npad * ln.g.ldw) for ln in launches if fused(ln)]


def _compare_rungemm(plan, launch, region, p, s, d):
    """One named region (name, arena, offset, bytes, dtype code) that the simulator's RUNGEMM changed; p / s / d: its bytes before, on the simulator and
    on the device.  The descriptor says which elements the launch writes: y and y2 at (row, column) and the statistics rows.  Inside them the device
    must equal the simulator (the statistics rows of a kRunBnBwd launch: opcheck.tolerance()'s bar over every element of the rows); a byte that differs
    anywhere else in the region - a pad column, a frame the launch does not store - is a stray byte.  Returns (miss in y / y2, miss in the
    statistics rows, stray bytes, err / tol of the rows held to opcheck's bar): a lost product shows in both, and the row is the better address."""
    name, a, off, nb, dt = region
    g, dev = launch.g, s.device
    es, yes = (2 if dt == opcheck.BF16 else 4), (2 if g.ydt == opcheck.BF16 else 4)
    ne = nb // es
    geo = f"tag {launch.tag} family {launch.family} M {g.M} N {g.N} K {launch.K} Tout {g.Tout} Fo {g.Fo} flags {g.flags & 0xffffffff:#x}"
    owner = torch.full((ne,), -1, dtype=torch.int64, device=dev)         # GEMM position m * N + n of the element's writer
    for ptr, idx, n0 in dest_index(g, dev):
        if ptr.arena != a:
            continue
        at = idx * yes + (ptr.off - off)                                 # byte inside the region
        inside = (at >= 0) & (at < nb)
        if bool(inside.any()):
            assert es == yes and (ptr.off - off) % es == 0, (name, "the destination's dtype is not the buffer's")
            pos = torch.arange(g.M, dtype=torch.int64, device=dev)[:, None] * g.N + n0 + torch.arange(idx.shape[1], dtype=torch.int64, device=dev)
            owner[at[inside] // es] = pos[inside]
    written = torch.zeros(nb, dtype=torch.bool, device=dev)
    written[:ne * es] = (owner >= 0).repeat_interleave(es)
    st = stats_range(g)
    lo = hi = 0
    if st is not None and st[0] == a and st[1] < off + nb and st[2] > off:
        lo, hi = st[1] - off, st[2] - off
        assert dt != opcheck.BF16 and lo >= 0 and hi <= nb and lo % 4 == 0, (name, "the statistics rows do not lie inside one fp32 buffer")
        written[lo:hi] = True
    assert not bool(((s != p) & ~written).any()), f"{name}: the simulator wrote outside the y / y2 / statistics elements of the descriptor ({geo})"
    stray = int(((d != s) & ~written).sum())
    miss, late, worst = "", "", 0.0
    ity = torch.int16 if es == 2 else torch.int32
    fty = torch.bfloat16 if es == 2 else torch.float32
    ne_y = (s[:ne * es].view(ity) != d[:ne * es].view(ity)) & (owner >= 0)
    if bool(ne_y.any()):
        e = int(ne_y.nonzero()[0])
        m, nn = int(owner[e]) // g.N, int(owner[e]) % g.N
        b, u, fo = row_of(g, m)
        sv, dv, pv = (float(x[:ne * es].view(fty)[e]) for x in (s, d, p))
        second = g.n2 > 0 and nn >= g.n2
        miss = (f"{name}: row {m} = (batch item {b}, frame u {u}, bin fo {fo}) column n {nn} -> {'y2' if second else 'y'}[{nn - g.n2 if second else nn}]: "
                f"simulator {sv!r} device {dv!r} (before {pv!r}); {int(ne_y.sum())} elements differ; {geo}")
    if hi > lo:
        sf, df = (x[lo:hi].view(torch.float32) for x in (s, d))
        nst = st[3]
        where = lambda e: (f"128-row block {e // (nst * g.Npad)} (rows {e // (nst * g.Npad) * KBM} ..) statistics row {e // g.Npad % nst} column {e % g.Npad}: "
                           f"simulator {float(sf[e])!r} device {float(df[e])!r} (before {float(p[lo:hi].view(torch.float32)[e])!r})")
        if bn_bwd(launch):
            tol = opcheck.tolerance(dt, name, KIND_RUNGEMM, "bf16" if plan.cfg.act_dtype == 1 else "fp32")
            err, own = opcheck.measure(sf.double().cpu(), df.double().cpu(), False)
            worst = err / tol
            if not err < tol:
                e = int((sf.double() - df.double()).abs().nan_to_num(nan=float("inf")).argmax())
                late = f"{name}: {where(e)}: err {err:.3e} of the rows' largest element {own:.3e}: opcheck's bar {tol:.1e} (BatchNorm-backward sums); {geo}"
        else:
            ne_s = sf.view(torch.int32) != df.view(torch.int32)
            if bool(ne_s.any()):
                late = f"{name}: {where(int(ne_s.nonzero()[0]))}; {int(ne_s.sum())} elements differ; {geo}"
    return miss, late, stray, worst


def compare_exact(plan, launch, before, simulated, device, loose=()):
    """The verdict on one launch.  before / simulated / device: the arenas (lists indexed by arena, on any torch device) in front of the launch, after it
    on the simulator and after it on the device.  Over every named buffer and every arena that either side changed the device must equal the simulator
    byte for byte; a byte the device changed where the simulator changed nothing is a stray byte.  A miss names the first differing element: for a WGRAD
    the split and (n, k) of the packed matrix, both values; for a RUNGEMM (_compare_rungemm) the buffer, the row as (batch item, frame u, bin fo), the
    column n and whether it went to y or y2, both values and the value before, and tag, family, M, N, K, Tout, Fo, flags - in statistics rows the
    128-row block and the column; else the buffer (or gradient tensor) and the element.
    loose: float_slices() of the plan.  The block of them that the launch writes - the fused first-layer launch every split (its kernel stores the whole
    block), the SPLITSUM that folds them, in another order of additions than the simulator's, split 0 - is held to opcheck's bar, max|device - simulator|
    below 1e-3 of the block's largest element, over EVERY element of the block (which of them the simulator's value happens to leave as it was plays no
    part); everything outside that block is held to byte equality in those launches too."""
    miss, late, stray, worst = "", "", 0, 0.0                     # late: a miss in statistics rows, named only where no y / y2 element differs
    regions = [(n, a, off, nb, dt) for n, a, off, nb, dt in _buffers(plan) if nb > 0] + [("A_GRAD", GRAD, 0, plan.arena_bytes[GRAD], 0), ("A_STATE", STATE, 0, plan.arena_bytes[STATE], 0)]
    covered = {a: torch.zeros(_u8(before[a]).numel(), dtype=torch.bool, device=_u8(before[a]).device) for a in CHECKED}
    for name, a, off, nb, dt in regions:
        p, s, d = (_u8(x[a])[off:off + nb] for x in (before, simulated, device))
        covered[a][off:off + nb] = True
        if launch.kind == KIND_RUNGEMM and not torch.equal(s, p):
            m, ms, n, w = _compare_rungemm(plan, launch, (name, a, off, nb, dt), p, s, d)  # (also with s == d: the simulator's writes are checked against the descriptor)
            miss, late, stray, worst = miss or m, late or ms, stray + n, max(worst, w)
            continue
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
        s, d = _u8(simulated[a]), _u8(device[a])
        if not torch.equal(s, d):
            stray += int(((d != s) & ~covered[a]).sum())
    miss = miss or late
    return Verdict(not miss and stray == 0, miss, stray, worst, bn_bwd(launch))


def run_launches(plan, launches, device, host=None, stop_at_first=False, state=None, saved_device=None, on_simulated=None):
    """Run `launches` in order on the device arenas - and, with `host` (the same state on the host), on the simulator from the same pre-launch state,
    under compare_exact.  Whole arenas are compared on the device (one upload of the simulator's state per launch); only a launch that differs is taken
    apart.  state None (the weight-gradient tier): the launches are chained, and after a launch that differs - the fused one always may - the host
    state becomes the device's.  state = an ExactState, saved_device = its saved arenas on the device (the RUNGEMM tier): every launch starts from
    that one state - the simulator's result comes from state.simulate(), the device arenas are restored before each launch, `before` is the saved
    state - and on_simulated(launch) is called in front of the device's launch (the conditions are asserted there).  Returns [(launch, Verdict)]."""
    out, loose = [], float_slices(wgrad_ops(plan))
    for ln in launches:
        if host is None and state is None:
            plan.run(ln.phase, device, 0, ln.op, ln.op + 1)
            continue
        if state is None:
            before = {a: device[a].clone() for a in CHECKED}
            sim_run(plan, ln.phase, host, ln.op, ln.op + 1)
        else:
            before, host = saved_device, state.simulate(ln)
            if on_simulated is not None:
                on_simulated(ln)
            for a in CHECKED:
                device[a].copy_(saved_device[a])
        plan.run(ln.phase, device, 0, ln.op, ln.op + 1)
        torch.cuda.synchronize()
        up = {a: host[a].to(device[a].device) for a in CHECKED}
        if all(torch.equal(_u8(up[a]), _u8(device[a])) for a in CHECKED):
            out.append((ln, Verdict(True, "", 0, 0.0, bn_bwd(ln))))
            continue
        v = compare_exact(plan, ln, before, up, device, loose)
        out.append((ln, v))
        if state is None:
            for a in CHECKED:
                host[a].copy_(device[a])
        if stop_at_first and not v.ok:
            break
    return out
