"""CPU: SyncBN plans for DCCRN(use_cbn=True) - structure only.  Each ComplexBatchNorm finalize (forward and backward) becomes a
"publish this rank's fp64 sums" op (mode 1), a sync point on those sums and a "finish from the all-reduced sums" op (mode 2) with the
global row count.  The host simulator does not execute the modes; the numbers are checked on the GPU (tests/test_gpu_cbn_syncbn.py)."""
import ctypes as C

import pytest
import torch

from norm_data import OP_HEADER, CbnBwd, CbnFwd, Ptr                 # the ctypes mirrors of sefd_desc.h, shared with the per-launch tier
from simutil import PHASE_BWD, PHASE_FWD, Plan

SMALL = dict(kernel_num=(16, 32, 32, 64, 64, 64), rnn_units=128)
OP_CBN_FINALIZE, OP_CBN_BWD_FINALIZE = 43, 46          # sefd_desc.h OpKind (checked against the descriptors' own fields below)


def ops_bytes(plan, ph):
    n, sz = plan.num_ops(ph), plan.lib.sefd_op_size()
    return [bytes((C.c_uint8 * sz).from_address(plan.ops_ptr(ph) + i * sz)) for i in range(n)]


def desc(raw):
    kind = int.from_bytes(raw[:4], "little", signed=True)
    cls = CbnFwd if kind == OP_CBN_FINALIZE else CbnBwd
    return kind, cls.from_buffer_copy(raw[OP_HEADER:OP_HEADER + C.sizeof(cls)])


def plan(B=4, world=2, dtype="fp32", training=True):
    return Plan(B, 3000, masking_mode="E", act_dtype=dtype, use_cbn=True, bn_world=world, training=training, cbn_sync=True, **SMALL)


# complex channel pairs h of the normed layers: encoder 0..5, decoder 0..4 (decoder 5, the mask layer, has no norm)
ENC_H = [k // 2 for k in SMALL["kernel_num"]]
DEC_H = [k // 2 for k in SMALL["kernel_num"][-2::-1]]


def test_descriptor_mirror_matches_the_library():
    """The ctypes mirrors above read back what the planner wrote: channel counts, row counts, training flag, momentum."""
    p = plan(world=1)
    fin = [desc(r) for r in ops_bytes(p, PHASE_FWD) if int.from_bytes(r[:4], "little") == OP_CBN_FINALIZE]
    assert [d.C // 2 for _, d in fin] == ENC_H + DEC_H
    assert all(d.training == 1 and abs(d.momentum - 0.1) < 1e-7 and abs(d.eps - 1e-5) < 1e-10 and d.count == d.R and d.mode == 0 for _, d in fin)
    bfin = [desc(r) for r in ops_bytes(p, PHASE_BWD) if int.from_bytes(r[:4], "little") == OP_CBN_BWD_FINALIZE]
    assert sorted(d.C // 2 for _, d in bfin) == sorted(ENC_H + DEC_H)
    assert all(d.count == d.R and d.R % d.rpb == 0 and d.R // d.rpb == 4 and d.mode == 0 for _, d in bfin)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("world", [2, 4])
def test_cbn_syncbn_plan_sync_points_and_modes(world, dtype):
    """One forward and one backward sync point per normed layer on fp64 totals of 5 h / 6 h values, each between a mode-1 and a mode-2 copy
    of the finalize; mode 2 carries the global row count (the big-batch plan's count)."""
    p = plan(world=world, dtype=dtype)
    syncs = p.sync_points()
    assert [s[0] for s in syncs] == [PHASE_FWD] * 11 + [PHASE_BWD] * 11
    assert all(s[5] == torch.float64 for s in syncs)
    big = plan(B=4 * world, world=1, dtype=dtype)
    assert not big.sync_points()
    big_count = {}
    for ph, kind in ((PHASE_FWD, OP_CBN_FINALIZE), (PHASE_BWD, OP_CBN_BWD_FINALIZE)):
        big_count[kind] = sorted((d.C // 2, d.count) for k, d in map(desc, ops_bytes(big, ph)) if k == kind)
    seen = {OP_CBN_FINALIZE: [], OP_CBN_BWD_FINALIZE: []}
    for ph, op, arena, off, cnt, _ in syncs:
        ops = ops_bytes(p, ph)
        k1, d1 = desc(ops[op])
        k2, d2 = desc(ops[op + 1])
        assert k1 == k2 == (OP_CBN_FINALIZE if ph == PHASE_FWD else OP_CBN_BWD_FINALIZE)
        h, ns = d1.C // 2, (5 if ph == PHASE_FWD else 6)
        assert (d1.mode, d2.mode) == (1, 2)
        assert cnt == ns * h
        assert (d1.totals.arena, d1.totals.off) == (d2.totals.arena, d2.totals.off) == (arena, off)
        assert d1.count == d1.R and d2.count == world * d1.R and d2.R == d1.R
        if ph == PHASE_BWD:
            assert d1.R // d1.rpb == 4
        seen[k1].append((h, d2.count))
    assert sorted(h for h, _ in seen[OP_CBN_FINALIZE]) == sorted(ENC_H + DEC_H)
    for kind in seen:
        assert sorted(seen[kind]) == big_count[kind]
    # the totals buffers are distinct and each holds its cnt doubles
    spans = sorted((off, off + 8 * cnt) for _, _, _, off, cnt, _ in syncs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][1] <= p.arena_bytes[0]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_cbn_syncbn_plan_differs_from_world1_only_at_the_finalizes(dtype):
    """Dropping the mode-1 copies and undoing mode 2 (mode 0, local count, no totals) gives the bn_world = 1 plan's op arrays byte for byte."""
    world = 2
    p, p1 = plan(world=world, dtype=dtype), plan(world=1, dtype=dtype)
    for ph in (PHASE_FWD, PHASE_BWD):
        got = []
        for raw in ops_bytes(p, ph):
            kind = int.from_bytes(raw[:4], "little", signed=True)
            if kind not in (OP_CBN_FINALIZE, OP_CBN_BWD_FINALIZE) or (kind == OP_CBN_FINALIZE and not desc(raw)[1].training):
                got.append(raw)
                continue
            _, d = desc(raw)
            if d.mode == 1:
                continue
            assert d.mode == 2
            d.mode, d.count, d.totals = 0, d.count / world, Ptr()
            got.append(raw[:OP_HEADER] + bytes(d) + raw[OP_HEADER + C.sizeof(d):])
        assert got == ops_bytes(p1, ph)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_cbn_eval_and_world1_plans_have_no_sync_points(dtype):
    """Eval plans carry no SyncBN ops whatever bn_world says, and bn_world = 1 training plans only mode-0 finalizes."""
    ev2, ev1 = plan(world=2, dtype=dtype, training=False), plan(world=1, dtype=dtype, training=False)
    assert not ev2.sync_points()
    for ph in (PHASE_FWD, PHASE_BWD):
        assert ops_bytes(ev2, ph) == ops_bytes(ev1, ph)
    p1 = plan(world=1, dtype=dtype)
    assert not p1.sync_points()
    for ph in (PHASE_FWD, PHASE_BWD):
        for raw in ops_bytes(p1, ph):
            if int.from_bytes(raw[:4], "little") in (OP_CBN_FINALIZE, OP_CBN_BWD_FINALIZE):
                d = desc(raw)[1]
                assert d.mode == 0 and (d.totals.arena, d.totals.off) == (0, 0)


def test_cbn_syncbn_plan_is_built_on_request_only():
    """bn_world > 1 alone keeps refusing a ComplexBatchNorm plan (test_plan_hostsim.test_hostsim_complex_batch_norm); cbn_sync = True, which
    models.py sets for GradientExchange(sync_bn=True), builds the SyncBN plan.  With bn_world = 1 the flag changes no op."""
    for training in (True, False):
        with pytest.raises(ValueError, match="cbn_sync"):
            Plan(2, 3000, masking_mode="E", use_cbn=True, bn_world=2, training=training, **SMALL)
    assert len(plan(B=2, world=2).sync_points()) == 22
    p0 = Plan(4, 3000, masking_mode="E", use_cbn=True, **SMALL)
    p1 = plan(world=1)
    for ph in (PHASE_FWD, PHASE_BWD):
        assert ops_bytes(p0, ph) == ops_bytes(p1, ph)
