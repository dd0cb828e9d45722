"""GPU: SyncBN for DCCRN(use_cbn=True).  The ComplexBatchNorm finalize kernels run as "publish this rank's fp64 sums" (mode 1) and "finish
from the all-reduced sums" (mode 2) around a sync point (csrc/cbn.hip, plan.cpp finalize_rungemms).  A world-W run must reproduce one plan
over the union batch: outputs, gradients summed over the ranks, and every rank's CBN running statistics.

1. the ranks emulated in lock step on one GPU against the big-batch plan (simutil.syncbn_vs_big_batch);
2. two processes over gloo, one utterance of the dccrn_cbn_E_sisnr golden each, through models.train_step -> Plan.run_synced ->
   GradientExchange.all_reduce_stats -> fused Adam: pinned to the reference's ComplexBatchNorm over the whole batch;
3. the same two ranks without sync_bn: their running statistics miss the golden by far more than the bar of 2."""
import os
import socket

import numpy as np
import pytest
import torch

from oracle.dccrn import DCCRNConfig, dccrn_state_shapes
from oracle.weights import formula_state_dict, test_signals as make_signals
from util import rel_err

pytestmark = pytest.mark.gpu
SMALL_KN = (16, 32, 32, 64, 64, 64)
DEFAULT_KN = (32, 64, 128, 256, 256, 256)
GOLDEN = "dccrn_cbn_E_sisnr"


# ------------------------------------------------------------------------------------------------ 1. lock step on one GPU
# Bars: (weight / bias gradient, PReLU slope gradient, outputs and running statistics), max-abs relative error per tensor, with the worst
# error measured on an MI355X over the cases of that dtype.  fp32 keeps simutil.syncbn_bars("fp32").  bf16: the ranks' statistics differ from
# the big batch's in the last bits and the bf16 activations then round to neighbouring values in many places; the CBN stack shows more of that
# noise than BatchNorm's (gradients of 4 - 7e-2 on many tensors; BatchNorm bf16 reached 3.3e-2 in test_gpu_ops).  A count without the world
# factor, or a rank's own statistics in place of the all-reduced ones, moves gradients by O(1) and the running statistics by ~0.4.
BARS = {
    "fp32": (1e-3, 1e-3, 1e-4),       # measured: 5.6e-6 (decoder.5.0.real_conv.bias, default kernel_num), -, 9.9e-7 (decoder.1.1.RMr)
    "bf16": (1.5e-1, 1.5e-1, 1e-2),   # measured: 7.3e-2 (decoder.5.0.real_conv.bias), 6.9e-2 (encoder.5.2.weight), 4.0e-3 (out_wav)
}


def check_cbn_syncbn_result(res, dtype):
    """simutil.check_syncbn_result for ComplexBatchNorm layers: a PReLU slope gradient (one scalar summed over a layer, it can cancel to near
    zero) is measured against the larger of its value and its layer's CBN weight gradient `.1.Wrr`, the same kind of per-channel sum."""
    gbar, sbar, obar = BARS[dtype]
    errs = {}
    for k, v in res["full"]["out"].items():
        errs[k] = (rel_err(res["ranks"]["out"][k], v), obar)
    for k, v in res["full"]["grad"].items():
        if k.endswith("conv.bias") and not k.startswith("decoder.5."):
            continue                      # conv biases in front of a normalisation: analytically zero gradient, rounding noise on both sides
        if k.endswith(".2.weight"):
            den = max(float(v.abs().max()), float(res["full"]["grad"][k[:-len("2.weight")] + "1.Wrr"].abs().max()))
            errs[k] = (float((res["ranks"]["grad"][k] - v).abs().max()) / den, sbar)
        else:
            errs[k] = (rel_err(res["ranks"]["grad"][k], v), gbar)
    for st in res["ranks"]["state"]:
        for k, v in res["full"]["state"].items():
            errs[k] = (max(errs.get(k, (0.0, obar))[0], rel_err(st[k], v)), obar)
    return errs


@pytest.mark.parametrize("dtype,kn,world", [("fp32", SMALL_KN, 2), ("fp32", SMALL_KN, 4), ("fp32", DEFAULT_KN, 2), ("bf16", SMALL_KN, 2)])
def test_cbn_syncbn_ranks_emulated_on_one_gpu(dtype, kn, world):
    from simutil import Plan, syncbn_vs_big_batch, unit_slopes
    ru = 128 if kn == SMALL_KN else 256
    B, L = 4, (3000 if kn == SMALL_KN else 2400)
    cfg = DCCRNConfig(masking_mode="C", kernel_num=kn, rnn_units=ru, use_cbn=True)
    # PReLU slopes = 1: the ranks sum their statistics in another order than the big batch, and a pre-activation within rounding of zero would
    # take different PReLU branches in the two backwards (test_gpu_ops._syncbn_ranks_on_one_gpu, simutil.unit_slopes)
    P = unit_slopes(formula_state_dict(dccrn_state_shapes(cfg)))
    assert any(k.endswith(".1.Wrr") for k in P)
    x, _ = make_signals(B, L)
    torch.manual_seed(7)
    gw = torch.randn(B, L)

    def make_plan(b, bn_world):
        return Plan(b, L, masking_mode="C", kernel_num=kn, rnn_units=ru, act_dtype=dtype, use_cbn=True, bn_world=bn_world, cbn_sync=True)
    res = syncbn_vs_big_batch(make_plan, P, {"wav": x}, {"grad_wav": gw}, world, device="cuda", stream=torch.cuda.current_stream().cuda_stream)
    assert len(res["ranks"]["plans"][0].sync_points()) == 22
    errs = check_cbn_syncbn_result(res, dtype)
    worst = sorted(errs.items(), key=lambda kv: -kv[1][0] / kv[1][1])
    print(f"cbn syncbn {dtype} kn{kn[0]} world {world}: " + ", ".join(f"{k} {e:.3e} (bar {b:.1e})" for k, (e, b) in worst[:6]))
    for k, (e, b) in errs.items():
        assert e < b, (k, e, b)


# ------------------------------------------------------------------------------------------------ 2. / 3. two gloo ranks, golden
def _golden_worker(rank, world, port, q):
    """One utterance of the golden's batch per rank: one train_step with SyncBN, then (a fresh model) one without it."""
    import torch.distributed as dist
    import sefd_amd  # noqa: F401
    from sefd_amd.ddp import GradientExchange
    from sefd_amd.optim import Adam
    from test_gpu_model import case_meta, make_model
    from util import load_golden
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = load_golden(GOLDEN)
        B, L = int(g["g/meta/B"]), int(g["g/meta/L"])
        kn, ru = tuple(int(k) for k in g["g/meta/kernel_num"]), int(g["g/meta/rnn_units"])
        skip, scale, _ = case_meta(g)
        assert B == world and int(g["g/meta/use_cbn"]) == 1
        x, y = make_signals(B, L)
        x, y = (x * scale)[rank:rank + 1].cuda(), (y * scale)[rank:rank + 1].cuda()
        out = {}
        for sync in (True, False):
            m = make_model(kn, ru, str(g["g/meta/mask"]), str(g["g/meta/loss"]), skip=skip, use_cbn=True)
            m.train()
            P0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
            opt = Adam(m.parameters(), lr=1e-3)
            ex = GradientExchange(sync_bn=sync)
            loss = float(m.train_step(x, y, opt, exchange=ex))
            torch.cuda.synchronize()
            sd = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
            # the flat gradient arena holds the sum over the ranks; Adam applied it with grad_scale 1 / world
            grads = {n: (m._flat_grad[off:off + cnt].view(shp).cpu() / world).numpy()
                     for (n, _), (off, cnt, shp) in zip(m._trainable(), m._param_slices)}
            # numpy, not tensors: torch would hand CPU tensors over as shared-memory handles that die with this process
            out[sync] = dict(loss=loss, state=sd, p0={k: v.numpy() for k, v in P0.items()}, grads=grads,
                             sync_points=len(next(iter(m._runtimes.values())).plan.sync_points()))
        q.put((rank, out))
    except BaseException as e:           # the parent reports it; the other rank's collectives end with the process group
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def golden_ranks():
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_golden_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = {}
        for _ in procs:
            rank, r = q.get(timeout=300)
            assert not isinstance(r, str), (rank, r)
            res[rank] = r
    finally:
        for p in procs:
            p.join(60)
            if p.exitcode is None:
                p.kill()
                p.join(10)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return res


def test_cbn_syncbn_two_gloo_ranks_match_the_reference_golden(golden_ranks):
    from test_gpu_model import TOL, noise_bias
    from util import load_golden, rel_l2, sub
    g = load_golden(GOLDEN)
    lines = []
    for rank, res in golden_ranks.items():
        r = res[True]
        assert r["sync_points"] == 22
        sd, P0, grads = r["state"], r["p0"], r["grads"]
        for k, v in sub(g, "g/running").items():
            e = rel_err(sd[k], v)
            lines.append(f"rank {rank} running {k} {e:.3e}")
            assert e < TOL, (rank, k, e)
        for k, v in sub(g, "g/after_adam").items():
            if noise_bias(k):
                continue
            e = float(np.abs((sd[k] - P0[k]) - (v - P0[k])).max())
            lines.append(f"rank {rank} after_adam {k} {e:.3e}")
            assert e < 5e-5, (rank, k, e)                      # updates are ~lr = 1e-3
        # test_gpu_model.test_module_step_against_reference_golden's gradient criteria
        gn = sub(g, "g/grad_norm")
        for k, v in gn.items():
            if noise_bias(k):
                continue
            assert abs(float(np.linalg.norm(grads[k].astype(np.float64))) - float(v)) <= TOL * float(v) + 1e-7, (rank, k)
        for k, v in sub(g, "g/grad").items():
            if noise_bias(k):
                assert float(np.abs(grads[k]).max()) < 1e-4 * float(gn[k.replace(".bias", ".weight")]) + 1e-7, (rank, k)
                continue
            tol = 5e-3 if k.endswith(".2.weight") else TOL
            lines.append(f"rank {rank} grad {k} {rel_l2(grads[k], v):.3e} {rel_err(grads[k], v):.3e}")
            assert rel_l2(grads[k], v) < tol and rel_err(grads[k], v) < 5e-3, (rank, k)
        for k, v in sub(g, "g/grad_samp").items():
            if not noise_bias(k):
                assert rel_err(grads[k].reshape(-1)[::int(g["g/meta/gstride"])], v) < TOL, (rank, k)
    print("\n".join(sorted(lines, key=lambda s: -float(s.split()[-1]))[:8]))


def test_cbn_without_syncbn_misses_the_golden_running_statistics(golden_ranks):
    """Control: per-rank CBN statistics (no sync_bn) are those of one utterance, not of the batch - far outside test 2's bar of 1e-3 (the CPU
    oracle's one-utterance statistics miss the golden by 0.43 and 0.36)."""
    from test_gpu_model import TOL
    from util import load_golden, sub
    g = load_golden(GOLDEN)
    worst = {}
    for rank, res in golden_ranks.items():
        assert res[False]["sync_points"] == 0
        worst[rank] = max(rel_err(res[False]["state"][k], v) for k, v in sub(g, "g/running").items())
    print(" ".join(f"rank {r} worst running {e:.3e}" for r, e in worst.items()))
    assert all(e > 100 * TOL for e in worst.values()), worst
