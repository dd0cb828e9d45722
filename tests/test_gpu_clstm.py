"""GPU: NavieComplexLSTM on its own - the module against goldens captured from the real reference (tests/golden/make_clstm_golden.py; pinned on the CPU by
tests/test_clstm_cpu.py), every launch of its plans against the host simulator, the reverse walk of the persistent recurrence kernels bit for bit against
their forward walk, bit reproducibility across the two streams, stacked layers, and the module's modes.  Budgets are the project's own: TOL (fp32) and the
named bf16 budgets of tests/test_gpu_model.py (restated in tests/recurrence_cases.py)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import clstm_common as cc
from clstm_common import CASES, TOL
from plan_check import KIND, _typed, report_path
from recurrence_cases import hot_biases
from simutil import PHASE_BWD, PHASE_FWD, Plan, fill_params, sim_run
from util import GOLDEN, knobs, load_golden

pytestmark = pytest.mark.gpu
ABI = json.load(open(os.path.join(GOLDEN, "seqmodel_abi.json")))


def make_module(case, dtype="fp32", P=None):
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models
    isz, hsz, pdim, bi, _, _ = case
    cfg.act_dtype = dtype
    try:
        m = models.NavieComplexLSTM(isz, hsz, projection_dim=pdim, bidirectional=bi)
    finally:
        cfg.act_dtype = "fp32"
    m.load_state_dict(cc.formula_params(case) if P is None else P)
    return m.to("cuda").train()


def step(m, xr, xi, gr, gi):
    """[out_r, out_i] = m([xr, xi]); loss = mean(out_r g_r) + mean(out_i g_i); backward.  Returns (out_r, out_i, loss, dxr, dxi, {name: grad}) on the CPU."""
    xr, xi = xr.cuda().requires_grad_(True), xi.cuda().requires_grad_(True)
    m.zero_grad()
    out_r, out_i = m([xr, xi])
    loss = cc.loss_of(out_r, out_i, gr.cuda(), gi.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return (out_r.detach().cpu(), out_i.detach().cpu(), float(loss.detach()), xr.grad.detach().cpu(), xi.grad.detach().cpu(),
            {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()})


def the_plan(m):
    (plan, _), = [v for k, v in m._runtimes.items() if k[0] == "clstm"]
    return plan


_report = {}


# ------------------------------------------------------------------------------------------------ 1. the module against the reference's golden
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_module_against_reference_golden(name, dtype):
    case = CASES[name]
    g = load_golden("clstm_" + name)
    m = make_module(case, dtype)
    res = step(m, *(torch.from_numpy(g["g/" + k]) for k in ("xr", "xi", "gr", "gi")))
    e = cc.golden_errors(g, *res)
    _report[f"{name}/{dtype}"] = e
    with open(report_path("clstm_gpu.json"), "w") as f:
        json.dump(_report, f, indent=1)
    print(name, dtype, {k: v for k, v in e.items() if not isinstance(v, dict)}, "worst grad l2", max(e["grad"].values()), max(e["grad"], key=e["grad"].get))
    assert the_plan(m).status() == 0
    assert all(bool(torch.isfinite(v).all()) for v in res[5].values())
    if dtype == "fp32":
        cc.assert_fp32(e)
    else:
        cc.assert_bf16(e)


# ------------------------------------------------------------------------------------------------ 2. every launch against the host simulator
def ops_device_vs_sim(plan, P, x, gy, dtype, per_element=False):
    """plan_check.ops_device_vs_sim for a ComplexLSTM plan.  That driver seeds the inputs of the models it knows and cannot take this one as it is, so
    this is its body with the plan's own inputs (x, gy) in place of the seeding: every op of both phases on the device and on the host simulator from
    the SAME pre-op state, with the same bars - relative to the largest element of a region fp32 buffers 1e-3, bf16 buffers 1.6e-2, the fp32 state of
    a bf16 recurrence op 4e-3; per_element: regions whose largest element exceeds 1 per element - and the same stray-write detection.
    Returns (report lines, the lines of the ops that miss)."""
    dev = plan.alloc_arenas("cuda")
    host = plan.alloc_arenas("cpu")
    fill_params(plan, dev, P)
    plan.io(dev, "x", tuple(x.shape)).copy_(x)
    plan.io(dev, "grad_y", tuple(gy.shape)).copy_(gy)
    # region table: (arena, byte offset, bytes, dtype, name); GRAD / STATE arenas are single fp32 regions
    regions = []
    for name in plan.buffer_names():
        a, off, nb, dt = plan.buffer(name)
        regions.append((a, off, nb, dt, name))
    regions.append((2, 0, plan.arena_bytes[2], 0, "A_GRAD"))
    regions.append((3, 0, plan.arena_bytes[3], 0, "A_STATE"))
    check = [0, 2, 3, 5]
    # The arenas stay on the device.  `host` mirrors the device state at every op boundary and `prev` is a second host copy
    # of that state; after an op only the regions that the kernel or the simulator changed travel (device -> host), so the
    # per-op cost is one device-side compare + one host-side memcmp instead of ten whole-arena copies.
    for a in range(6):
        host[a].copy_(dev[a])
    prev = {a: host[a].clone() for a in check}
    by_arena = {a: [r for r in regions if r[0] == a and r[2] > 0] for a in check}
    # 8-byte words: every region starts on a 256-byte boundary, so a word never straddles two regions
    w64 = {a: (dev[a].view(torch.uint8).numel() // 8) for a in check}
    lo_idx = {a: torch.tensor([r[1] // 8 for r in by_arena[a]], device="cuda") for a in check}
    hi_idx = {a: torch.tensor([min((r[1] + r[2] + 7) // 8, w64[a]) for r in by_arena[a]], device="cuda") for a in check}
    # host side: which regions did the SIMULATOR change?  One vectorised pass per arena (words -> 256-byte blocks -> prefix sums; regions start on
    # 256-byte boundaries, so a block never straddles two regions) instead of one memcmp per region and op (28 000 torch.equal calls per case: half of the
    # suite's run time through round 5)
    nblk = {a: (w64[a] + 31) // 32 for a in check}
    lo_blk = {a: torch.tensor([r[1] // 256 for r in by_arena[a]]) for a in check}
    hi_blk = {a: torch.tensor([min((r[1] + r[2] + 255) // 256, nblk[a]) for r in by_arena[a]]) for a in check}

    def host_changed(a):
        h64 = host[a].view(torch.uint8)[:w64[a] * 8].view(torch.int64)
        p64 = prev[a].view(torch.uint8)[:w64[a] * 8].view(torch.int64)
        ne = h64 != p64
        if ne.numel() % 32:
            ne = torch.cat([ne, torch.zeros(32 - ne.numel() % 32, dtype=torch.bool)])
        cs = torch.cat([torch.zeros(1, dtype=torch.int64), ne.view(-1, 32).any(1).to(torch.int64).cumsum(0)])
        return ((cs[hi_blk[a]] - cs[lo_blk[a]]) > 0).tolist()
    lines, bad = [], []
    for phase in (PHASE_FWD, PHASE_BWD):
        kinds, tags = plan.op_kinds(phase)
        for i in range(plan.num_ops(phase)):
            dbefore = {a: dev[a].view(torch.uint8)[:w64[a] * 8].view(torch.int64).clone() for a in check}
            sim_run(plan, phase, host, i, i + 1)
            plan.run(phase, dev, 0, i, i + 1)
            worst, nchg, stray, where = 0.0, 0, 0, ""
            for a in check:
                if not by_arena[a]:
                    continue
                d64 = dev[a].view(torch.uint8)[:w64[a] * 8].view(torch.int64)
                cs = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"), (d64 != dbefore[a]).to(torch.int32)]), 0)
                dflags = ((cs[hi_idx[a]] - cs[lo_idx[a]]) > 0).cpu().tolist()        # the one synchronising read per arena
                hflags = host_changed(a)
                h8, p8, d8 = host[a].view(torch.uint8), prev[a].view(torch.uint8), dev[a].view(torch.uint8)
                for (ra, off, nb, dt, name), dchg, hchg in zip(by_arena[a], dflags, hflags):
                    if not (hchg or dchg):
                        continue
                    g8 = d8[off:off + nb].cpu() if dchg else p8[off:off + nb]
                    if hchg:
                        hv, gv = _typed(h8[off:off + nb], dt).double(), _typed(g8, dt).double()
                        den = float(hv.abs().max())
                        if per_element and den > 1.0:
                            err = float(((hv - gv).abs() / hv.abs().clamp(min=1.0)).max())
                        else:
                            err = float((hv - gv).abs().max()) / (den if den > 0 else 1.0)
                        if not np.isfinite(err):
                            err = float("inf")
                        tol = 1.6e-2 if dt == 1 else 1e-3
                        if dt != 1 and dtype == "bf16" and int(kinds[i]) == 1 and name.endswith(".bnpart"):
                            tol = 4e-3     # fp32 partial sums of the bf16 gradient tile this launch ALSO stores: where kernel and simulator round an
                                           # element of that tile to different bf16 neighbours (allowed above: 2 ulps), a 128-row sum with cancellation
                                           # moves by up to that ulp (seen 1.06e-3 of the region's largest sum)
                        if dt != 1 and dtype == "bf16" and int(kinds[i]) in (9, 10):
                            tol = 4e-3     # fp32 state of a bf16 recurrence (cell state, dh): h_t is rounded to bf16 every frame, and a
                                           # rounding flip (one bf16 ulp = 4e-3 of h) between kernel and simulator feeds back into c
                        nchg += hv.numel()
                        if err / tol > worst:
                            worst, where = err / tol, f"{name} err {err:.2e} tol {tol:.0e}"
                    else:
                        # stray write: the kernel changed bytes of a region the simulator did not touch
                        stray += int((g8 != p8[off:off + nb]).sum())
                    h8[off:off + nb].copy_(g8)                                        # both host copies := device state
                    if dchg:
                        p8[off:off + nb].copy_(g8)
            lines.append(f"phase {phase} op {i:3d} {KIND.get(int(kinds[i]), str(int(kinds[i]))):16s} tag {int(tags[i]):4d} elems {nchg:9d} "
                         f"err/tol {worst:.3e} stray {stray} {where}")
            if not (worst < 1.0) or stray:
                bad.append(lines[-1])
    return lines, bad


@pytest.mark.parametrize("hot", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["bi_h32", "bi_h128_proj", "bi_h192_proj"])
def test_every_launch_against_host_simulator(name, dtype, hot):
    case = CASES[name]
    s = cc.sizes(case)
    P = cc.formula_params(case)
    if hot:
        P = hot_biases(P)
        assert float((P["real_lstm.bias_ih_l0_reverse"] - cc.formula_params(case)["real_lstm.bias_ih_l0_reverse"]).abs().max()) == 100.0
    xr, xi, gr, gi = cc.inputs(case)
    n = s["T"] * s["B"] * s["O"]
    plan = Plan(s["B"], s["T"], model="ComplexLSTM", clstm=cc.clstm_dict(case), act_dtype=dtype)
    lines, bad = ops_device_vs_sim(plan, P, cc.to_plan_x(case, xr, xi), cc.to_plan_gy(case, gr / n, gi / n), dtype, per_element=hot)
    with open(report_path(f"clstm_ops_{name}_{dtype}{'_hot' if hot else ''}.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    assert not bad, "\n".join(bad)
    assert plan.status() == 0
    compared = lambda kind: [int(re.search(r"elems\s+(\d+)", l).group(1)) for l in lines if f" {kind} " in l]
    if dtype == "bf16" or s["H"] <= 128:       # persistent or cluster kernels: one launch per direction and phase, each compared
        assert len(compared("LSTM_FWD")) == 2 and len(compared("LSTM_BWD")) == 2 and min(compared("LSTM_FWD") + compared("LSTM_BWD")) > 0
        masks = [mk for _, mk, _, _, _ in cc.lstm_launches(plan, ABI)]
        assert masks == [0xF, 0, 0xF, 0]
    else:                                      # stepped: a cell launch per direction and frame
        assert len(compared("CELL_FWD")) == 2 * s["T"] and len(compared("CELL_BWD")) == 2 * s["T"] and min(compared("CELL_FWD") + compared("CELL_BWD")) > 0


# ------------------------------------------------------------------------------------------------ 3. the reverse walk itself
def mirrored_params(case):
    P = cc.formula_params(case)
    for k in list(P):
        if k.endswith("_reverse"):
            P[k] = P[k[:-len("_reverse")]].clone()
    return P


@pytest.mark.parametrize("dtype,H,rpw", [("bf16", 32, 4), ("bf16", 32, 16), ("bf16", 64, 4), ("bf16", 64, 16), ("bf16", 96, 4), ("bf16", 96, 16),
                                         ("bf16", 128, 4), ("bf16", 128, 16), ("fp32", 48, 0), ("fp32", 128, 0)])
def test_reverse_walk_is_the_forward_walk_on_flipped_time(dtype, H, rpw):
    """A bidirectional layer without projection whose `_reverse` tensors are copies of the forward ones.  Run A: inputs x, upstream gradient g.  Run B:
    inputs flip_t(x), upstream gradient with the halves of g swapped and flipped in time.  Then the reverse direction of A is the forward direction of B
    on the same numbers in the same order, so, BIT FOR BIT: the reverse half of each output of A is the time-flip of the forward half of B's, the saved
    hidden sequences and the gate gradients of the two recurrences are each other's time-flips, and - with the upstream gradient on one direction only
    (the other direction then adds exact zeros) - so are the input gradients.  rpw: LSTM_RPW and LSTM_RPW_BWD (bf16: both variants; fp32 has one)."""
    if rpw:
        knobs.set("LSTM_RPW", str(rpw))
        knobs.set("LSTM_RPW_BWD", str(rpw))
    I = 24
    base = (2 * I, 2 * H, None, True)
    m = make_module(base + (1, 1), dtype, mirrored_params(base + (1, 1)))
    for T in (1, 2, 3, 4, 5, 7, 10):
        for B in (1, 5, 18):
            case = base + (B, T)
            xr, xi, gr, gi = cc.inputs(case)
            gr[..., :H], gi[..., :H] = 0.0, 0.0                      # run A: upstream gradient on the reverse direction only
            swap = lambda g: torch.cat([g[..., H:], g[..., :H]], 2).flip(0)
            runs = []
            for ins in ((xr, xi, gr, gi), (xr.flip(0), xi.flip(0), swap(gr), swap(gi))):
                res = step(m, *ins)
                (plan, ar), = [v for k, v in m._runtimes.items() if k[:3] == ("clstm", B, T)]
                assert plan.status() == 0
                assert [mk for _, mk, _, _, _ in cc.lstm_launches(plan, ABI)] == [0xF, 0, 0xF, 0]
                bufs = {k: plan.view(ar, k).clone().cpu() for k in ("h.f", "h.r", "dgates.f", "dgates.r")}
                runs.append((res, bufs))
            (ra, ba), (rb, bb) = runs
            tag = (dtype, H, rpw, T, B)
            flip_h = lambda v: v.view(4, B, T, H).flip(2)
            flip_g = lambda v: v.view(2, B, T, 8 * H).flip(2)
            assert float(ba["h.r"].float().abs().max()) > 1e-3 and float(ba["dgates.r"].float().abs().max()) > 0, tag
            assert torch.equal(ba["h.r"].view(4, B, T, H), flip_h(bb["h.f"])), ("h", tag)
            assert torch.equal(ba["h.f"].view(4, B, T, H), flip_h(bb["h.r"])), ("h (forward of A = reverse of B)", tag)
            assert torch.equal(ba["dgates.r"].view(2, B, T, 8 * H), flip_g(bb["dgates.f"])), ("dgates", tag)
            for k in (0, 1):                                       # out_r, out_i
                assert torch.equal(ra[k][..., H:], rb[k][..., :H].flip(0)), ("output", k, tag)
                assert torch.equal(ra[k][..., :H], rb[k][..., H:].flip(0)), ("output (forward of A = reverse of B)", k, tag)
            for k in (3, 4):                                       # dxr, dxi
                assert float(ra[k].abs().max()) > 0 and torch.equal(ra[k], rb[k].flip(0)), ("input gradient", k, tag)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_launchers_refuse_a_chunked_reversed_launch(dtype):
    """A reversed group resumes from no saved state.  The planner never chunks one; a descriptor that is (t1 written into the plan's op list here) is not
    launched: the buffers stay untouched, the plan's status word is raised and the next run refuses, as the cluster launcher does."""
    import ctypes as C
    case = CASES["bi_h32"]
    s = cc.sizes(case)
    plan = Plan(s["B"], s["T"], model="ComplexLSTM", clstm=cc.clstm_dict(case), act_dtype=dtype)
    ar = plan.alloc_arenas("cuda")
    fill_params(plan, ar, cc.formula_params(case))
    x = cc.to_plan_x(case, *cc.inputs(case)[:2])
    plan.io(ar, "x", tuple(x.shape)).copy_(x)
    sz, u, off = ABI["sefd_op_size"] // 4, ABI["op_union_offset"], ABI["lstm_rec_offsets"]
    n = plan.num_ops(PHASE_FWD)
    raw = np.ctypeslib.as_array((C.c_int32 * (n * sz)).from_address(plan.ops_ptr(PHASE_FWD))).reshape(n, sz)
    rev, = [i for i in range(n) if raw[i, 0] == cc.OP_LSTM_FWD and raw[i, (u + off["rev_mask"]) // 4] == 0xF]
    plan.run(PHASE_FWD, ar, 0, 0, rev)                              # everything in front of the reverse recurrence
    raw[rev, (u + off["t1"]) // 4] = 5
    try:
        plan.run(PHASE_FWD, ar, 0, rev, rev + 1)
        torch.cuda.synchronize()
        assert plan.status() == 1
        assert float(plan.view(ar, "h.r").float().abs().max()) == 0.0 and float(plan.view(ar, "c.r").abs().max()) == 0.0
        with pytest.raises(RuntimeError, match="sefd_plan_run failed"):
            plan.run(PHASE_FWD, ar, 0, rev, rev + 1)
    finally:
        raw[rev, (u + off["t1"]) // 4] = 0
    assert plan.status(clear=True) == 1
    plan.run(PHASE_FWD, ar, 0, rev, rev + 1)                        # the planner's own descriptor runs
    torch.cuda.synchronize()
    assert plan.status() == 0 and float(plan.view(ar, "h.r").float().abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 4. bit reproducibility
def test_two_streams_are_bit_reproducible():
    """Forward + backward of bi_h128_proj in bf16, four times (the later ones replay the captured graph where that is on): identical bytes.  The two
    directions run on different streams; a missing join would show as a race."""
    case = CASES["bi_h128_proj"]
    m = make_module(case, "bf16")
    ins = cc.inputs(case)
    first = step(m, *ins)
    assert float(first[0].abs().max()) > 1e-3
    for _ in range(3):
        again = step(m, *ins)
        for a, b in zip(first[:2] + first[3:5], again[:2] + again[3:5]):
            assert torch.equal(a, b)
        assert first[2] == again[2]
        for k, v in first[5].items():
            assert torch.equal(v, again[5][k]), k
    assert the_plan(m).status() == 0


# ------------------------------------------------------------------------------------------------ 5. stacked layers
def test_stacked_layers_against_fp64():
    """nn.Sequential of two layers, as DCCRN stacks them (lists pass through), against the plain float64 reference; gradients reach the first layer's
    parameters and the inputs."""
    c0, c1 = (48, 64, None, False, 3, 9), (64, 64, 48, False, 3, 9)
    P0, P1 = cc.formula_params(c0), cc.formula_params(c1)
    net = torch.nn.Sequential(make_module(c0, "fp32", P0), make_module(c1, "fp32", P1))
    xr, xi, _, _ = cc.inputs(c0)
    _, _, gr, gi = cc.inputs(c1)
    out_r, out_i, loss, dxr, dxi, grads = step(net, xr, xi, gr, gi)
    W0 = {k: v.double().requires_grad_(True) for k, v in P0.items()}
    W1 = {k: v.double().requires_grad_(True) for k, v in P1.items()}
    xs = [xr.double().requires_grad_(True), xi.double().requires_grad_(True)]
    ref_r, ref_i = cc.plain_forward(c1, W1, *cc.plain_forward(c0, W0, *xs))
    ref_loss = cc.loss_of(ref_r, ref_i, gr.double(), gi.double())
    names = [("0." + k, W0[k]) for k in W0] + [("1." + k, W1[k]) for k in W1]
    g = torch.autograd.grad(ref_loss, [w for _, w in names] + xs)
    ref = dict(out_r=ref_r.detach(), out_i=ref_i.detach(), loss=float(ref_loss.detach()), loss_scale=cc.loss_scale(ref_r.detach(), ref_i.detach(), gr, gi),
               dxr=g[-2], dxi=g[-1], grads={k: v for (k, _), v in zip(names, g[:-2])})
    assert list(grads) == [k for k, _ in names]
    e = cc.errors(ref, out_r, out_i, loss, dxr, dxi, grads)
    print({k: v for k, v in e.items() if not isinstance(v, dict)}, max(e["grad_max"].values()))
    assert float(grads["0.real_lstm.weight_hh_l0"].abs().max()) > 0 and float(dxr.abs().max()) > 0
    cc.assert_fp32(e, TOL)


# ------------------------------------------------------------------------------------------------ 6. modes
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_no_grad_eval_and_the_stale_activation_guard(dtype):
    case = CASES["bi_h128_proj"]
    m = make_module(case, dtype)
    xr, xi, gr, gi = (t.cuda() for t in cc.inputs(case))
    train = [t.detach().clone() for t in m([xr, xi])]
    with torch.no_grad():
        ng = m([xr, xi])
    assert not ng[0].requires_grad and all(torch.equal(a, b) for a, b in zip(train, ng))
    m.eval()
    ev = m((xr, xi))                                              # a tuple is taken like a list
    assert all(torch.equal(a, b) for a, b in zip(train, ev))
    m.train()
    with pytest.raises(TypeError, match="list or tuple of two"):
        m(torch.cat([xr, xi], 2))
    xg = xr.clone().requires_grad_(True)
    out = m([xg, xi])
    m([xr, xi])                                                   # a second forward of the same shape before the backward
    with pytest.raises(RuntimeError, match="overwrote the activations"):
        cc.loss_of(out[0], out[1], gr, gi).backward()
    out = m([xg, xi])
    cc.loss_of(out[0], out[1], gr, gi).backward()
    assert float(xg.grad.abs().max()) > 0
