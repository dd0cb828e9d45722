"""GPU, two ranks: AdamW with parameter groups and global-norm clipping under the gradient exchange.  Both ranks (gloo, sharing the box's GPU) see the
same two clips, so the mean gradient is each rank's own (the sum of two equal floats, halved, is exact): the ranks must stay bitwise equal to each other
- the norm is taken after the all-reduce, on grad * grad_scale - and to a single process that runs the same three steps."""
import os
import queue
import time

import pytest

pytestmark = pytest.mark.gpu
STEPS = 3


def _setup():
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models
    from oracle.weights import fill_state_dict_, test_signals
    cfg.dccrn_kernel_num, cfg.masking_mode, cfg.loss, cfg.act_dtype = [16, 32, 32, 64, 64, 64], "E", "SI-SNR", "fp32"
    m = models.DCCRN(rnn_units=128, masking_mode="E")
    fill_state_dict_(m)
    x, y = test_signals(4, 4000)
    return m.to("cuda").train(), x[:2].cuda(), y[:2].cuda()


def _run(max_grad_norm, steps, exchange=None):
    import torch
    from sefd_amd.optim import AdamW
    m, x, y = _setup()
    opt = AdamW(m.get_params(0.1), lr=1e-3, max_grad_norm=max_grad_norm)
    for _ in range(steps):
        m.train_step(x, y, opt, exchange=exchange)
    torch.cuda.synchronize()
    return m._flat_param.cpu(), opt.last_grad_norm.cpu()


def _worker(rank, world, port, clip, q):
    import torch.distributed as dist
    import sefd_amd  # noqa: F401
    from sefd_amd.ddp import GradientExchange
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p, norm = _run(clip, STEPS, GradientExchange())
        q.put((rank, p.numpy(), norm.numpy()))
    finally:
        dist.destroy_process_group()


def test_clipped_adamw_keeps_two_ranks_bitwise_equal_to_one_process():
    import socket
    import numpy as np
    import torch.multiprocessing as mp
    _, first = _run(float("inf"), 1)
    clip = 0.5 * float(first)
    want_p, want_norm = _run(clip, STEPS)
    moved_p, _ = _run(float("inf"), STEPS)
    assert not np.array_equal(moved_p.numpy(), want_p.numpy())          # the clip is active: without it the three steps end elsewhere
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, clip, q)) for r in range(2)]
    for p in procs:
        p.start()
    res, deadline = {}, time.monotonic() + 300
    while len(res) < 2:                                  # results first: a rank cannot exit while its parameters sit in the queue's pipe
        try:
            rank, prm, norm = q.get(timeout=2)
            res[rank] = (prm, norm)
        except queue.Empty:
            assert all(p.is_alive() or p.exitcode == 0 for p in procs) and time.monotonic() < deadline, "a rank hung or died"
    for p in procs:
        p.join(300)
        assert p.exitcode == 0, "a rank hung or died"
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][0], want_p.numpy()) and np.array_equal(res[0][1], want_norm.numpy())
