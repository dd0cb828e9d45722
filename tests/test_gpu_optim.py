"""GPU: the grouped optimizer step (csrc/optim.hip) - sefd_grad_norm and sefd_optim_step against the fp64 restatement in optim_ref.py at their
edges (segments off the 16-byte lines, frozen segments, more chunks than workgroups, the three skips), then sefd_amd.optim.Adam / AdamW on a model:
against torch.optim.AdamW + clip_grad_norm_, checkpoint round trips, frozen parameters and a scheduler.

Reference-alone condition of the kernel cases: the same reference evaluated in fp32 on the CPU stays below 2.5e-7 (measured 0.7e-7 to 1.8e-7), a
quarter of ADAM_BAR."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from optim_ref import clip_coef, grad_norm, optim_update
from oracle.weights import fill_state_dict_, test_signals as make_signals
from test_gpu_loss_edges import ADAM_BAR, ADAM_GRADS, B1, B2, EPS, LR, Guarded, _adam_case
from util import rel_err

pytestmark = pytest.mark.gpu
SMALL = (16, 32, 32, 64, 64, 64)
ALONE_BAR = 2.5e-7
FROZEN = -1
LR1 = float(np.float32(3e-4))
WD0, WD1 = float(np.float32(1e-2)), float(np.float32(0.1))
# group 0: L2 decay 1e-2;  group 1: decoupled decay 0.1 + amsgrad, its own lr;  group 2: no decay, amsgrad (vmax starts at 1.5 v)
GROUPS = (dict(lr=LR, weight_decay=WD0, decoupled=False, amsgrad=False), dict(lr=LR1, weight_decay=WD1, decoupled=True, amsgrad=True),
          dict(lr=LR, weight_decay=0.0, decoupled=False, amsgrad=True))
LAYOUTS = {"A": ((1, 3, 256, 257, 1021, 4099, 8, 65541), (0, 1, 2, FROZEN, 0, 1, FROZEN, 2)),        # almost every boundary off a 16-byte line
           "B": ((4096 * 256 + 3,), (1,)),                                                          # 1025 chunks in one tensor
           # 12 000 tensors of 7 elements: 9000 owned chunks, more than a launch has workgroups (the grid-stride loop), none on a 16-byte line
           "C": ((7,) * 12000, (0, 1, 2, FROZEN) * 3000)}


def _lib():
    from sefd_amd import _lib as m
    return m.lib()


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _segments(layout):
    lens, gids = LAYOUTS[layout]
    begins = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return [(int(b), int(n), int(g)) for b, n, g in zip(begins, lens, gids)]


@functools.lru_cache(maxsize=None)
def _mask(layout, gid):
    n = sum(LAYOUTS[layout][0])
    mk = torch.zeros(n, dtype=torch.bool)
    for b, c, g in _segments(layout):
        if g == gid:
            mk[b:b + c] = True
    return mk


@functools.lru_cache(maxsize=None)
def _table(layout):
    """(host table, device table, number of chunks) of the layout's owned segments."""
    import sefd_amd  # noqa: F401
    from sefd_amd.optim import chunk_table, table_to_device
    tab = chunk_table([s for s in _segments(layout) if s[2] != FROZEN])
    return tab, table_to_device(tab), len(tab)


def _hyper(groups=GROUPS):
    from sefd_amd.optim import _Group
    arr = (_Group * 8)()
    for i, g in enumerate(groups):
        arr[i] = _Group(g["lr"], B1, B2, EPS, g["weight_decay"], (1 if g["decoupled"] else 0) | (2 if g["amsgrad"] else 0))
    return arr


def _start(layout, first, dt=torch.float32):
    n = sum(LAYOUTS[layout][0])
    p, g, m, v = (t.to(dt) for t in _adam_case(n, first))
    vmax = v.clone()
    vmax[_mask(layout, 2)] *= 1.5
    return p, g, m, v, vmax


@functools.lru_cache(maxsize=None)
def _reference(layout, first, scale, clip=True):
    """Three steps per group in fp64 (gradient multiples ADAM_GRADS, grad * scale, the clip coefficient of max_norm = half the first gradient's norm
    over the owned elements), after the reference-alone condition in fp32.  Returns (max_norm, {gid: (p, m, v, vmax)}, [norm of each step])."""
    owned = ~_mask(layout, FROZEN)
    got = {}
    for dt in (torch.float64, torch.float32):
        p, g, m, v, vmax = _start(layout, first, dt)
        # the norm is an fp64 accumulation in the kernel too: both evaluations take the fp64 norm, and the coefficient in their own dtype
        norms = [float(grad_norm(ADAM_GRADS[k] * g.double()[owned] * scale)) for k in range(3)]
        max_norm = float(np.float32(0.5 * norms[0])) if clip else None
        coefs = [torch.tensor(clip_coef(nk, max_norm), dtype=dt) if clip else 1.0 for nk in norms]
        out = {}
        for gid, h in enumerate(GROUPS):
            mk = _mask(layout, gid)
            if not mk.any():
                continue
            st = (p[mk], m[mk], v[mk], vmax[mk])
            for k in range(3):
                st = optim_update(st[0], ADAM_GRADS[k] * g[mk] * scale, st[1], st[2], st[3], first + k, h["lr"], B1, B2, EPS, h["weight_decay"],
                                  h["decoupled"], h["amsgrad"], coefs[k])
            out[gid] = st
        got[dt] = out
    alone = max(rel_err(a, b) for gid in got[torch.float64] for a, b, use in
                zip(got[torch.float32][gid], got[torch.float64][gid], (1, 1, 1, GROUPS[gid]["amsgrad"])) if use)
    print("alone", layout, first, scale, alone)
    assert alone < ALONE_BAR, ("reference alone", layout, first, scale, alone)
    return max_norm, got[torch.float64], norms


class _Buffers:
    """param, moments and gradient of a layout in guarded device buffers, with their starting values kept on the host."""

    def __init__(self, layout, first):
        self.layout, self.n = layout, sum(LAYOUTS[layout][0])
        self.start = _start(layout, first)
        p, g, m, v, vmax = self.start
        self.p, self.m, self.v, self.vmax = (Guarded(self.n, init=t) for t in (p, m, v, vmax))
        self.g = g
        self.ws = Guarded(_lib().sefd_grad_norm_ws_floats(self.n) // 2, torch.float64)
        self.out = Guarded(2)

    def step(self, step, grad, scale, max_norm=None, coef=None, word=None, nan=None, groups=None, table=None, n=None, ngroups=3):
        L_ = _lib()
        th, td, nc = table if table is not None else _table(self.layout)
        thp = C.c_void_p(th.ctypes.data) if th is not None else None
        if max_norm is not None:
            assert L_.sefd_grad_norm(_vp(grad), self.n, scale, max_norm, thp, _vp(td), nc, self.ws.ptr, self.out.ptr, None) == 0
            coef = C.c_void_p(self.out.t.data_ptr() + 4)
        return L_.sefd_optim_step(self.p.ptr, _vp(grad), self.m.ptr, self.v.ptr, self.vmax.ptr, self.n if n is None else n, step,
                                  groups if groups is not None else _hyper(), ngroups, thp, _vp(td), nc, scale, coef, word, nan, None)

    def state(self):
        for b in (self.p, self.m, self.v, self.vmax):
            b.check()
        return tuple(b.t.cpu() for b in (self.p, self.m, self.v, self.vmax))

    def unchanged(self):
        return all(torch.equal(a, b) for a, b in zip(self.state(), (self.start[0],) + self.start[2:]))


# ------------------------------------------------------------------------------------------ 1. sefd_optim_step
@pytest.mark.parametrize("layout,first,scale", [(lay, first, scale) for lay in ("A", "B") for first in (1, 1000) for scale in (1.0, 0.125)] + [("C", 1000, 1.0)])
def test_optim_step_over_layouts_groups_and_steps(layout, first, scale):
    """Three steps (1-3 and 1000-1002 with non-zero moments) over three groups with different decay / amsgrad / lr, clipped by the coefficient that
    sefd_grad_norm leaves on the device; per group at ADAM_BAR; frozen segments, the gradient and the guard zones bitwise untouched."""
    max_norm, want, norms = _reference(layout, first, scale)
    bufs = _Buffers(layout, first)
    for k in range(3):
        gd = Guarded(bufs.n, init=ADAM_GRADS[k] * bufs.g)
        assert bufs.step(first + k, gd.t, scale, max_norm=max_norm) == 0
        bufs.out.check()
        norm, coef = (float(x) for x in bufs.out.t.cpu())
        assert abs(norm - norms[k]) <= 2.0 ** -23 * norms[k] and coef < 1.0
        gd.check()
        assert torch.equal(gd.t.cpu(), ADAM_GRADS[k] * bufs.g)
    got = bufs.state()
    for gid, ref in want.items():
        mk = _mask(layout, gid)
        for a, b, what in zip(got, ref, ("param", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")):
            if what != "max_exp_avg_sq" or GROUPS[gid]["amsgrad"]:
                err = rel_err(a[mk], b)
                print(layout, first, scale, gid, what, err)
                assert err < ADAM_BAR, (gid, what, err)
    fz = _mask(layout, FROZEN)
    for a, b in zip(got, (bufs.start[0],) + bufs.start[2:]):
        assert torch.equal(a[fz], b[fz])
    mk0 = _mask(layout, 0)                                       # a group without amsgrad leaves max_exp_avg_sq alone
    assert torch.equal(got[3][mk0], bufs.start[4][mk0])


def test_optim_step_without_a_coefficient_and_one_group_equals_adam():
    """coef NULL means 1: one group with no options over the whole buffer is sefd_adam_step's update.  Two fp32 evaluations of one formula: each is
    within ADAM_BAR of the exact result (test_adam_over_sizes_and_steps), so of each other."""
    import sefd_amd  # noqa: F401
    from sefd_amd.optim import chunk_table, table_to_device
    n = 65541 + 257
    p, g, m, v = _adam_case(n, 1000)
    tab = chunk_table([(0, 257, 0), (257, 65541, 0)])
    td = table_to_device(tab)
    a = [Guarded(n, init=t) for t in (p, m, v)]
    b = [Guarded(n, init=t) for t in (p, m, v)]
    gd = g.cuda()
    hyper = _hyper([dict(lr=LR, weight_decay=0.0, decoupled=False, amsgrad=False)])
    for k in range(2):
        assert _lib().sefd_adam_step(a[0].ptr, _vp(gd), a[1].ptr, a[2].ptr, n, 1000 + k, LR, B1, B2, EPS, 0.125, None) == 0
        assert _lib().sefd_optim_step(b[0].ptr, _vp(gd), b[1].ptr, b[2].ptr, None, n, 1000 + k, hyper, 1, C.c_void_p(tab.ctypes.data), _vp(td), len(tab),
                                      0.125, None, None, None, None) == 0
    for x, y in zip(a, b):
        y.check()
        print("bitwise", bool(torch.equal(x.t, y.t)), rel_err(y.t, x.t))
        assert rel_err(y.t, x.t) < ADAM_BAR


def test_optim_step_skips_leave_everything_as_it_was():
    """The status word, the poisoned gradient element and a NaN clip coefficient: p, m, v and vmax stay bitwise as they were; with the word cleared
    the step matches the reference."""
    import sefd_amd  # noqa: F401
    from sefd_amd.plan import Plan
    plan = Plan(1, 5, model="FullSubNet", fsn=dict(sb_num_neighbors=31, fb_num_neighbors=31, fb_hidden=64, sb_hidden=32))
    word = C.c_void_p(plan.status_word())
    bufs = _Buffers("A", 1000)
    gd = bufs.g.cuda()
    nan = torch.full((1,), float("nan"), device="cuda")
    one = torch.ones(1, device="cuda")
    plan.status_set()
    assert bufs.step(1000, gd, 1.0, word=word) == 0 and bufs.unchanged()
    assert plan.status(clear=True) == 1
    assert bufs.step(1000, gd, 1.0, word=word, nan=_vp(nan)) == 0 and bufs.unchanged()
    assert bufs.step(1000, gd, 1.0, word=word, nan=_vp(one), coef=_vp(nan)) == 0 and bufs.unchanged()
    bad = gd.clone()
    bad[5] = float("inf")                                         # in a segment of group 2: the norm is Inf, the coefficient NaN, the step skipped
    assert bufs.step(1000, bad, 1.0, max_norm=1.0, word=word) == 0 and bufs.unchanged()
    assert bufs.step(1000, gd, 1.0, word=word, nan=_vp(one), coef=_vp(one)) == 0
    got = bufs.state()
    p, g, m, v, vmax = (t.double() for t in bufs.start)
    for gid, h in enumerate(GROUPS):
        mk = _mask("A", gid)
        ref = optim_update(p[mk], g[mk], m[mk], v[mk], vmax[mk], 1000, h["lr"], B1, B2, EPS, h["weight_decay"], h["decoupled"], h["amsgrad"])
        for a, b, use in zip(got, ref, (1, 1, 1, h["amsgrad"])):
            assert not use or rel_err(a[mk], b) < ADAM_BAR


def test_optim_step_goes_float_by_float_when_the_buffers_sit_differently_on_16_bytes():
    """exp_avg one float off the 16-byte lines the other buffers sit on: no float4 access is possible for all of them at once, every element takes
    the single-float path - the same update."""
    bufs = _Buffers("A", 1000)
    gd = bufs.g.cuda()
    p, g, m, v, vmax = bufs.start
    off = Guarded(bufs.n + 1, init=torch.cat([torch.full((1,), 7.0), m]))
    th, td, nc = _table("A")
    assert _lib().sefd_optim_step(bufs.p.ptr, _vp(gd), _vp(off.t[1:]), bufs.v.ptr, bufs.vmax.ptr, bufs.n, 1000, _hyper(), 3, C.c_void_p(th.ctypes.data),
                                  _vp(td), nc, 1.0, None, None, None, None) == 0
    off.check()
    assert float(off.t[0]) == 7.0
    got = bufs.state()
    got = (got[0], off.t[1:].cpu(), got[2], got[3])
    for gid, h in enumerate(GROUPS):
        mk = _mask("A", gid)
        ref = optim_update(p.double()[mk], g.double()[mk], m.double()[mk], v.double()[mk], vmax.double()[mk], 1000, h["lr"], B1, B2, EPS,
                           h["weight_decay"], h["decoupled"], h["amsgrad"])
        for a, b, use in zip(got, ref, (1, 1, 1, h["amsgrad"])):
            assert not use or rel_err(a[mk], b) < ADAM_BAR
    fz = _mask("A", FROZEN)
    for a, b in zip(got, (p, m, v, vmax)):
        assert torch.equal(a[fz], b[fz])


def test_optim_step_refuses_bad_arguments_without_a_launch():
    import sefd_amd  # noqa: F401
    from sefd_amd.optim import chunk_table, table_to_device
    bufs = _Buffers("A", 1)
    gd = bufs.g.cuda()
    assert bufs.step(1, gd, 1.0, n=0) == -1
    assert bufs.step(0, gd, 1.0) == -1
    assert bufs.step(1, gd, 1.0, ngroups=9) == -1
    assert bufs.step(1, gd, 1.0, ngroups=2) == -1                       # the table names group 2
    assert bufs.step(1, gd, 1.0, table=(None, None, 0)) == -1
    past = chunk_table([(bufs.n - 3, 4, 0)])
    assert bufs.step(1, gd, 1.0, table=(past, table_to_device(past), 1)) == -1
    assert bufs.step(1, gd, 1.0, n=bufs.n - 1) == -1                    # the last chunk of the layout's table reaches past n - 1
    assert bufs.unchanged()


# ------------------------------------------------------------------------------------------ 2. sefd_grad_norm
def _norm(gd, n, scale, max_norm, table=(None, None, 0)):
    ws, out = Guarded(_lib().sefd_grad_norm_ws_floats(n) // 2, torch.float64), Guarded(2)
    th, td, nc = table
    assert _lib().sefd_grad_norm(_vp(gd), n, scale, max_norm, C.c_void_p(th.ctypes.data) if th is not None else None, _vp(td), nc, ws.ptr, out.ptr,
                                 None) == 0
    ws.check()
    out.check()
    return out.t.cpu()


@pytest.mark.parametrize("n", [1, 255, 257, 65537, 3700001])
def test_grad_norm_over_sizes(n):
    """One fp32 rounding of the fp64 norm (the accumulation is fp64) for norm and coefficient; the same bits twice; zero, no clip, NaN and Inf."""
    g = _adam_case(n, 1)[1]
    gd = g.cuda()
    for scale in (1.0, 0.125):
        ref = float(grad_norm(g.double() * scale))
        max_norm = float(np.float32(0.5 * ref))
        out = _norm(gd, n, scale, max_norm)
        cref = clip_coef(ref, max_norm)
        print(n, scale, abs(float(out[0]) - ref) / ref, abs(float(out[1]) - cref) / cref)
        assert abs(float(out[0]) - ref) <= 2.0 ** -23 * ref
        assert abs(float(out[1]) - cref) <= 2.0 ** -23 * cref
        assert torch.equal(out, _norm(gd, n, scale, max_norm))
        above = _norm(gd, n, scale, float(np.float32(1.01 * ref)))
        assert float(above[1]) == 1.0 and torch.equal(above[:1], out[:1])
    if n > 1:                                                    # off the 16-byte lines: the same elements from a view that starts one float in
        assert abs(float(_norm(gd[1:], n - 1, 1.0, 1.0)[0]) - float(grad_norm(g.double()[1:]))) <= 2.0 ** -23 * float(grad_norm(g.double()[1:]))
    zero = _norm(torch.zeros(n, device="cuda"), n, 1.0, 1.0)
    assert float(zero[0]) == 0.0 and float(zero[1]) == 1.0
    for bad in (float("nan"), float("inf")):
        gb = gd.clone()
        gb[n // 2] = bad
        out = _norm(gb, n, 1.0, 1.0)
        assert not np.isfinite(float(out[0])) and np.isnan(float(out[1]))


def test_grad_norm_over_a_chunk_table_leaves_frozen_segments_out():
    n = sum(LAYOUTS["A"][0])
    g = _adam_case(n, 1)[1].clone()
    fz = _mask("A", FROZEN)
    ref = float(grad_norm(g.double()[~fz]))
    g[fz] = 1e6
    out = _norm(g.cuda(), n, 1.0, 1.0, _table("A"))
    assert abs(float(out[0]) - ref) <= 2.0 ** -23 * ref
    assert _lib().sefd_grad_norm(_vp(g.cuda()), n - 1, 1.0, 1.0, C.c_void_p(_table("A")[0].ctypes.data), _vp(_table("A")[1]), _table("A")[2],
                                 Guarded(2048).ptr, Guarded(2).ptr, None) == -1


# ------------------------------------------------------------------------------------------ 3. the optimizer on a model
def _cfg():
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg
    for k, v in dict(dccrn_kernel_num=list(SMALL), masking_mode="C", loss="SI-SNR", perceptual=False, lstm="complex", skip_type=True, act_dtype="fp32",
                     model="DCCRN", chkpt_model=None).items():
        setattr(cfg, k, v)
    return cfg


def _fresh():
    from sefd_amd import models
    m = models.DCCRN(rnn_units=128, masking_mode="C")
    fill_state_dict_(m)
    return m.to("cuda").train()


def _restore_cfg():
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg
    cfg.masking_mode = "E"


@functools.lru_cache(maxsize=1)
def _first_norm():
    """The gradient norm of the first step, from an optimizer that computes it and never clips."""
    from sefd_amd.optim import AdamW
    _cfg()
    x, y = (t.cuda() for t in make_signals(3, 4000))
    m = _fresh()
    o = AdamW(m.get_params(0.5), lr=1e-3, amsgrad=True, max_grad_norm=float("inf"))
    m.train_step(x, y, o)
    return float(o.last_grad_norm)


def test_adamw_groups_amsgrad_clipping_against_torch_and_round_trips(tmp_path):
    """AdamW over get_params(0.5) with amsgrad and clipping at half the first norm: two fused steps, a checkpoint, then one more step - against
    torch.optim.AdamW + clip_grad_norm_ on a fresh model that loaded both state dicts (1e-5, the bar of the plain checkpoint round trip), against
    the optimizer's own generic step() route, and bitwise against a fresh fused optimizer that loaded the checkpoint."""
    from sefd_amd import train_interface as ti
    from sefd_amd.optim import AdamW
    clip = 0.5 * _first_norm()
    _cfg()
    x, y = (t.cuda() for t in make_signals(3, 4000))
    a = _fresh()
    oa = AdamW(a.get_params(0.5), lr=1e-3, amsgrad=True, max_grad_norm=clip)
    a.train_step(x, y, oa)
    assert abs(float(oa.last_grad_norm) - 2 * clip) <= 1e-5 * clip            # the same first gradient as the unclipped optimizer saw
    a.train_step(x, y, oa)
    path = str(tmp_path / "chkpt_2.pt")
    ti.save_checkpoint(path, a, oa, 2)
    la = float(a.train_step(x, y, oa))
    pa, na = a._flat_param.clone(), float(oa.last_grad_norm)
    ck = torch.load(path)
    assert len(ck["optimizer"]["param_groups"]) == 2 and "max_exp_avg_sq" in ck["optimizer"]["state"][0]

    # bitwise: a fresh fused optimizer continues where the first one stopped
    b = _fresh()
    ob = AdamW(b.get_params(0.5), lr=1e-3, amsgrad=True, max_grad_norm=clip)
    assert ti.load_checkpoint(path, b, ob, map_location="cuda") == 3
    lb = float(b.train_step(x, y, ob))
    assert la == lb and torch.equal(pa, b._flat_param) and float(ob.last_grad_norm) == na

    def torch_step(weight_decay, max_norm):
        c = _fresh()
        oc = torch.optim.AdamW(c.get_params(weight_decay), lr=1e-3, amsgrad=True)
        c.load_state_dict(ck["model"])
        sd = torch.load(path)["optimizer"]
        for grp in sd["param_groups"]:
            grp["weight_decay"] = weight_decay if grp["weight_decay"] else 0.0
        oc.load_state_dict(sd)
        _, _, wav = c(x, y)
        lc = c.loss(wav, y)
        oc.zero_grad()
        lc.backward()
        total = float(torch.nn.utils.clip_grad_norm_(list(c.parameters()), max_norm)) if max_norm is not None else None
        oc.step()
        return float(lc), c._flat_param.clone(), total

    lc, pc, total = torch_step(0.5, clip)
    print("torch", abs(lc - la) / abs(la), rel_err(pc, pa), abs(na - total) / total)
    assert abs(lc - la) < 1e-5 * abs(la) and rel_err(pc, pa) < 1e-5
    assert abs(na - total) < 1e-5 * total
    _, plain, _ = torch_step(0.0, None)                                      # the options matter: without decay and clipping the step differs
    assert rel_err(plain, pa) > 1e-4

    # the optimizer's own generic route: loss.backward(), then step()
    d = _fresh()
    od = AdamW(d.get_params(0.5), lr=1e-3, amsgrad=True, max_grad_norm=clip)
    ti.load_checkpoint(path, d, od, map_location="cuda")
    _, _, wav = d(x, y)
    ld = d.loss(wav, y)
    od.zero_grad()
    ld.backward()
    od.step()
    print("generic", abs(float(ld) - la) / abs(la), rel_err(d._flat_param, pa))
    assert abs(float(ld) - la) < 1e-5 * abs(la) and rel_err(d._flat_param, pa) < 1e-5
    assert abs(float(od.last_grad_norm) - total) < 1e-5 * total
    _restore_cfg()


def test_parameters_outside_the_optimizer_are_frozen():
    from sefd_amd.optim import Adam
    _cfg()
    x, y = (t.cuda() for t in make_signals(3, 4000))
    m = _fresh()
    opt = Adam([p for n, p in m.named_parameters() if not n.startswith("encoder.")], lr=1e-3)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    for _ in range(2):
        m.train_step(x, y, opt)
    torch.cuda.synchronize()
    moved = 0
    for n, p in m.named_parameters():
        if n.startswith("encoder."):
            assert torch.equal(p.detach(), before[n]), n
        else:
            moved += int(not torch.equal(p.detach(), before[n]))
    print("moved", moved, "of", sum(1 for n in before if not n.startswith("encoder.")))
    assert moved > 0.5 * sum(1 for n in before if not n.startswith("encoder."))
    off, cnt, _ = m._param_slices[[n for n, _ in m.named_parameters()].index("encoder.0.0.real_conv.weight")]
    assert not opt._m[off:off + cnt].any() and not opt._v[off:off + cnt].any()
    _restore_cfg()


def test_scheduler_halves_each_groups_learning_rate():
    """StepLR over two groups with different lr: the second step's update of a group-1 parameter is the reference's at the halved group-1 lr."""
    from sefd_amd.optim import Adam
    _cfg()
    x, y = (t.cuda() for t in make_signals(3, 4000))
    m = _fresh()
    groups = m.get_params(0.0)
    groups[0]["lr"], groups[1]["lr"] = 1e-3, 4e-4
    opt = Adam(groups, lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1, gamma=0.5)
    m.train_step(x, y, opt)
    sched.step()
    assert opt.param_groups[0]["lr"] == 5e-4 and opt.param_groups[1]["lr"] == 2e-4
    # the group-1 parameter (a bias) with the largest first gradient
    index = {id(p): i for i, (_, p) in enumerate(m.named_parameters())}
    slices = [m._param_slices[index[id(p)]] for p in opt.param_groups[1]["params"]]
    off, cnt, _ = max(slices, key=lambda s: float(m._flat_grad[s[0]:s[0] + s[1]].abs().max()))
    sl = slice(off, off + cnt)
    p1, m1, v1 = (t[sl].double().cpu() for t in (m._flat_param, opt._m, opt._v))
    m.train_step(x, y, opt)
    g2 = m._flat_grad[sl].double().cpu()
    want = optim_update(p1, g2, m1, v1, None, 2, lr=2e-4)[0]
    full = optim_update(p1, g2, m1, v1, None, 2, lr=4e-4)[0]
    got = m._flat_param[sl].double().cpu()
    print("scheduler", rel_err(got, want), rel_err(got, full))
    assert rel_err(got, want) < ADAM_BAR and rel_err(got, full) > 10 * ADAM_BAR
    _restore_cfg()
