"""Test-only helpers: build/load the host simulator and the product library, drive a Plan on host or device arenas."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

from util import rel_err

import sefd_amd  # noqa: F401  (alias of the hyphenated package)
from sefd_amd import build as sefd_build
from sefd_amd.plan import ARENA_COUNT, ARENA_GRAD, ARENA_PARAM, ARENA_STATE, PHASE_BWD, PHASE_FWD, Plan  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "hostsim", "hostsim.cpp")
SIM_LIB = os.path.join(HERE, "hostsim", "_build", "libhostsim.so")


SIM_CMD = ["g++", "-O3", "-fopenmp", "-std=c++17", "-fPIC", "-shared", "-o", SIM_LIB, SIM_SRC]


def build_sim(force=False):
    desc = os.path.join(sefd_build.CSRC, "sefd_desc.h")
    digest = sefd_build.source_digest([SIM_SRC, desc], " ".join(SIM_CMD[:-2]))      # contents, not mtimes (build.source_digest)
    if force or not sefd_build.stamp_current(SIM_LIB, digest):
        import fcntl
        os.makedirs(os.path.dirname(SIM_LIB), exist_ok=True)
        with open(SIM_LIB + ".lock", "w") as lock:          # one builder at a time across processes (the two ranks of a gloo test), like build.build()
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                if force or not sefd_build.stamp_current(SIM_LIB, digest):
                    subprocess.run(SIM_CMD, check=True)
                    sefd_build.write_stamp(SIM_LIB, digest)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)


_built = False


def ensure_built():
    global _built
    if _built:                               # once per process: the digests read every source file
        return
    sefd_build.build()
    build_sim()
    _built = True


_sim = None


def sim():
    global _sim
    if _sim is None:
        ensure_built()
        _sim = C.CDLL(SIM_LIB)
        _sim.hostsim_run.restype = C.c_int
        _sim.hostsim_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        _sim.hostsim_enc0_accepts.restype = C.c_int
        _sim.hostsim_enc0_accepts.argtypes = [C.c_void_p, C.c_int]
    return _sim


def sim_run(plan: Plan, phase, arenas, first=0, last=-1):
    n = plan.num_ops(phase)
    last = n if last < 0 else last
    assert sim().hostsim_op_size() == plan.lib.sefd_op_size()
    ptrs = (C.c_void_p * ARENA_COUNT)(*[C.c_void_p(a.data_ptr()) for a in arenas])
    rc = sim().hostsim_run(C.c_void_p(plan.ops_ptr(phase)), first, last, ptrs)
    assert rc == 0, f"host simulator refused the plan's ops [{first}, {last}) of phase {phase} ({rc})"


def fill_params(plan: Plan, arenas, values: dict):
    """Copy {state_dict name: tensor} into the flat PARAM / STATE arenas."""
    for table, arena in ((plan.params, ARENA_PARAM), (plan.state, ARENA_STATE)):
        flat = arenas[arena]
        for name, (off, shape) in table.items():
            v = values[name].reshape(-1).to(torch.float32)
            flat[off:off + v.numel()].copy_(v)


def read_params(plan: Plan, arenas, arena_id, table=None):
    table = plan.params if table is None else table
    flat = arenas[arena_id].detach().cpu()
    return {name: flat[off:off + int(np.prod(shape))].reshape(shape).clone() for name, (off, shape) in table.items()}


# ---- layout converters: channels-last workspace buffers -> reference NCHW
def act_to_nchw(buf, B, Tn, F, Cc, drop_first=0):
    """[B][Tn][F][C] -> [B, C, F, Tn-drop_first] float32 (CPU)."""
    x = buf.detach().float().cpu().view(B, Tn, F, Cc)[:, drop_first:]
    return x.permute(0, 3, 2, 1).contiguous()


def spec_to_ref(buf, B, T, NF):
    """[B][T][NF+1][2] slot layout -> [B, 2*NF, T] (real rows then imag rows)."""
    x = buf.detach().float().cpu().view(B, T, NF + 1, 2)[:, :, 1:]
    return torch.cat([x[..., 0].permute(0, 2, 1), x[..., 1].permute(0, 2, 1)], 1).contiguous()


# ---- SyncBN: `world` ranks of a bn_world plan in lock step against one plan over the whole batch
def syncbn_vs_big_batch(make_plan, params, inputs, grads, world, device="cpu", stream=0):
    """Emulate `world` SyncBN ranks in one process and run the big-batch plan they must reproduce.

    make_plan(B, bn_world) -> Plan (knobs are read when it is called); params: {state_dict name: tensor};
    inputs / grads: {io name: [B, ...] tensor} copied in before the forward / the backward (io buffers not named stay zero).
    Each rank gets an equal shard of the batch.  The ranks run the op ranges between their plans' sync points in lock
    step, and each synced statistics buffer is replaced by its sum over the ranks, as the all-reduce of the data-parallel
    step does.  device "cpu": host arenas under the host simulator; "cuda": device arenas under Plan.run on `stream`.
    Returns dict(full=..., ranks=...): out (io outputs, ranks concatenated), grad (ranks summed, fp64), state (one per rank
    for `ranks`), plans."""
    B = next(iter(inputs.values())).shape[0]
    assert B % world == 0, (B, world)
    Bl = B // world

    def run(plan, ar, ph, first, last):
        if device == "cpu":
            sim_run(plan, ph, ar, first, last)
        else:
            plan.run(ph, ar, stream, first, last)

    def prep(plan, lo, hi):
        ar = plan.alloc_arenas(device)
        fill_params(plan, ar, params)
        for name, t in inputs.items():
            plan.io(ar, name, (hi - lo,) + tuple(t.shape[1:])).copy_(t[lo:hi])
        return ar

    def seed_grads(plan, ar, lo, hi):
        for name, t in grads.items():
            plan.io(ar, name, (hi - lo,) + tuple(t.shape[1:])).copy_(t[lo:hi])

    def outputs(plan, ar, b):
        out = {"out_wav": plan.io(ar, "out_wav", (b, plan.L))}
        for name in ("out_real", "out_imag"):
            out[name] = plan.io(ar, name, (b, plan.NF, plan.T))
        return {k: v.detach().float().cpu().clone() for k, v in out.items()}

    full = make_plan(B, 1)
    assert not full.sync_points()
    far = prep(full, 0, B)
    run(full, far, PHASE_FWD, 0, full.num_ops(PHASE_FWD))
    seed_grads(full, far, 0, B)
    run(full, far, PHASE_BWD, 0, full.num_ops(PHASE_BWD))

    ranks = [make_plan(Bl, world) for _ in range(world)]
    syncs = ranks[0].sync_points()
    assert syncs and all(p.sync_points() == syncs for p in ranks)
    ars = [prep(p, r * Bl, (r + 1) * Bl) for r, p in enumerate(ranks)]
    for ph in (PHASE_FWD, PHASE_BWD):
        if ph == PHASE_BWD:
            for r, p in enumerate(ranks):
                seed_grads(p, ars[r], r * Bl, (r + 1) * Bl)
        cur = 0
        for sph, op, a, off, cnt, dtype in syncs:
            if sph != ph:
                continue
            nb = cnt * (8 if dtype == torch.float64 else 4)
            views = []
            for r, p in enumerate(ranks):
                run(p, ars[r], ph, cur, op + 1)
                views.append(ars[r][a].view(torch.uint8)[off:off + nb].view(dtype))
            tot = views[0].clone()
            for v in views[1:]:
                tot += v
            for v in views:
                v.copy_(tot)
            cur = op + 1
        for r, p in enumerate(ranks):
            run(p, ars[r], ph, cur, p.num_ops(ph))
    if device != "cpu":
        torch.cuda.synchronize()

    rout = [outputs(p, ars[r], Bl) for r, p in enumerate(ranks)]
    rgrad = [read_params(p, ars[r], ARENA_GRAD) for r, p in enumerate(ranks)]
    return dict(
        full=dict(out=outputs(full, far, B), grad={k: v.double() for k, v in read_params(full, far, ARENA_GRAD).items()},
                  state=read_params(full, far, ARENA_STATE, full.state), plan=full),
        ranks=dict(out={k: torch.cat([o[k] for o in rout]) for k in rout[0]},
                   grad={k: sum(g[k].double() for g in rgrad) for k in rgrad[0]},
                   state=[read_params(p, ars[r], ARENA_STATE, p.state) for r, p in enumerate(ranks)], plans=ranks))


KIND_WGRAD, RUN_DY_FROM_BN = 2, 1024       # sefd_desc.h: OP_WGRAD, kRunDyFromBn
DEFAULT_KN = (32, 64, 128, 256, 256, 256)
# The default-size DCCRN in bf16: its deeper BatchNorm stacks over few rows amplify the rounding flips of this comparison to 3e-2 .. 6e-2 on
# weights and to O(1) on near-cancelling one-element bias gradients (decoder.5), in the fused and the unfused (ENC0_BNFUSE=0) plan alike, at
# every B x L tried (2 x 1200 .. 4 x 3200): above the bf16 bars.  Its case pins the N = 32 first layer (the path it exists for), outputs and
# running statistics; every other tensor is held to the bars by the small-model cases and to 1e-3 by fp32.
DEFAULT_KN_ONLY = "encoder.0."


def syncbn_bars(dtype):
    """(gradient, PReLU-slope gradient, outputs and running statistics) bars, max-abs relative error per tensor.  bf16: the ranks sum their
    statistics in a different order than the big batch and bf16 activations then round to neighbouring values (worst seen on the host
    simulator: weights 9.8e-3, a slope - one scalar summed over a whole layer - 4.1e-2, outputs 3.4e-3); a count that misses the world factor
    moves the layer's gradient by ~0.3."""
    return (1e-3, 1e-3, 1e-4) if dtype == "fp32" else (2e-2, 6e-2, 1e-2)


def unit_slopes(P):
    """PReLU slopes = 1 (identity): the runs sum their statistics in different orders, so a pre-activation within rounding of zero can take
    different PReLU branches in the two backwards and move that layer's sums by (1 - slope) * dz of the element - a discontinuity that is not
    what these tests are about (the SyncBN plumbing is); the PReLU branches are pinned by the oracle and per-op tests."""
    return {k: (torch.ones_like(v) if k.endswith(".2.weight") else v) for k, v in P.items()}


def check_syncbn_result(res, dtype, only=None, grad_bar=None):
    """Per-tensor errors of a syncbn_vs_big_batch result against the bars of `dtype`; only: check just the gradients whose names start with it;
    grad_bar: replaces the weight / bias gradient bar."""
    gbar, sbar, obar = syncbn_bars(dtype)
    gbar = grad_bar or gbar
    errs = {}
    for k, v in res["full"]["out"].items():
        errs[k] = rel_err(res["ranks"]["out"][k], v)
        assert errs[k] < obar, (k, errs[k])
    for k, v in res["full"]["grad"].items():
        if k.endswith("conv.bias") and not k.startswith("decoder.5."):
            continue                      # conv biases in front of a BatchNorm: analytically zero gradient, rounding noise on both sides
        if only and not k.startswith(only):
            continue
        if k.endswith(".2.weight") and dtype != "fp32":
            # a PReLU slope is ONE scalar summed over a whole layer and can cancel to near zero (CRN decoder.1: -1.7e-4 in fp32, while bf16 rounding
            # moves it by ~1e-3 in the big-batch plan itself): measured against the larger of its value and its layer's BatchNorm weight
            # gradient, the same kind of sum per channel
            den = max(float(v.abs().max()), float(res["full"]["grad"][k[:-len("2.weight")] + "1.weight"].abs().max()))
            errs[k] = float((res["ranks"]["grad"][k] - v).abs().max()) / den
        else:
            errs[k] = rel_err(res["ranks"]["grad"][k], v)
        assert errs[k] < (sbar if k.endswith(".2.weight") else gbar), (k, errs[k])
    for r, st in enumerate(res["ranks"]["state"]):
        for k, v in res["full"]["state"].items():
            e = rel_err(st[k], v)
            errs[k] = max(errs.get(k, 0.0), e)
            assert e < obar, (r, k, e)
    return errs
