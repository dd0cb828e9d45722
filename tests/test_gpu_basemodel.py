"""GPU: BaseModel on its own (tools_for_model.py:801-1185) - `unfold` and the seven norms as differentiable ops over the streaming kernels of
csrc/basemodel.hip - against goldens captured from the real reference in float64 (tests/golden/make_basemodel_golden.py; the torch restatement
is pinned to the same goldens on the CPU by tests/test_basemodel_cpu.py).  Per tensor max|got - ref| / max|ref| <= 4 x E32, E32 the reference's own
float32 error on the case (not below 1e-7): the rule of tests/test_gpu_convlayers.py.  Then what no golden shows: the C ABI's refusals launch nothing,
and the result does not depend, in any bit, on strides, the run, the rest of the batch, the alignment, or the door it was called through.

tests/opcheck.py compares the ops of a PLAN with the host simulator; these entry points belong to no plan, so it does not apply here: the dispatcher
registration is checked with torch.library.opcheck instead."""
import ctypes as C

import pytest
import torch

import basemodel_common as bc
import sefd_amd  # noqa: F401
from sefd_amd.tools_for_model import BaseModel

pytestmark = pytest.mark.gpu


def BM():
    return BaseModel


@pytest.mark.parametrize("name", list(bc.CASES))
def test_case_against_the_reference_golden(name):
    ref, e32, seed = bc.load_golden(name)
    res = bc.run_case(BM(), name, torch.float32, device="cuda", inp=bc.inputs(name, seed))
    torch.cuda.synchronize()
    bc.check(res, ref, e32, name)


# one shape per family with T % 4 == 0 (the 16-byte path), two bin ranges (F = 33) and, for the offline pair, four segments
X4, X3 = (3, 2, 33, 68), (3, 33, 68)
PROPS = ([(n, X4, None) for n in bc.NORMS4] + [(n, X3, 5) for n in bc.NORMS3] + [(n, X3, 100) for n in bc.NORMS3] + [("unfold", X4, 3)]
         + [("sband_forgetting_norm", (3, 34, 68), 5)])                 # even F with frames past the sample length
IDS = [f"{n}{'' if a is None else '_' + str(a)}{'_f34' if sh[-2] == 34 else ''}" for n, sh, a in PROPS]


def _inputs(fn, shape, arg):
    x = bc._u(31000, shape)
    if fn in bc.NORMS4 + bc.NORMS3 and fn not in bc.SIGNED:
        x = 0.05 + (x + 1) / 2
    oshape = (shape[0], shape[2], shape[1], 2 * arg + 1, shape[3]) if fn == "unfold" else shape
    return x.cuda(), bc._u(31001, oshape).cuda()


def _f(fn, arg, ns=None):
    f = getattr(ns or BM(), fn)
    return (lambda x: f(x)) if arg is None else (lambda x: f(x, arg))


def _run(f, x, cot):
    x = x.detach().requires_grad_(True)
    y = f(x)
    (y * cot).sum().backward()
    return y.detach(), x.grad.detach()


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("fn,shape,arg", PROPS, ids=IDS)
def test_bit_identical_across_runs_strides_batch_alignment_and_door(fn, shape, arg):
    x, cot = _inputs(fn, shape, arg)
    f = _f(fn, arg)
    base = _run(f, x, cot)
    assert all(bool(torch.isfinite(t).all()) for t in base)
    assert _same(base, _run(f, x, cot)), "two runs differ"
    # a permuted view of the same values: made contiguous inside
    xp = x.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not xp.is_contiguous() and torch.equal(xp, x)
    y, gx = _run(f, xp, cot)
    assert _same(base, (y, gx)), "a non-contiguous input differs from its contiguous copy"
    cp = cot.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert _same(base, _run(f, x, cp)), "a non-contiguous cotangent differs"
    # every utterance alone
    for b in range(shape[0]):
        yb, gb = _run(f, x[b:b + 1].clone(), cot[b:b + 1].clone())
        assert torch.equal(yb[0], base[0][b]) and torch.equal(gb[0], base[1][b]), f"utterance {b} alone differs from the batch"
    # one float past a 16-byte boundary: the element-by-element path
    buf = torch.empty(x.numel() + 4, dtype=torch.float32, device="cuda")
    xu = buf[1:1 + x.numel()].view(shape)
    xu.copy_(x)
    cbuf = torch.empty(cot.numel() + 4, dtype=torch.float32, device="cuda")
    cu = cbuf[1:1 + cot.numel()].view(cot.shape)
    cu.copy_(cot)
    assert x.data_ptr() % 16 == 0 and xu.data_ptr() % 16 == 4 and xu.is_contiguous()
    assert _same(base, _run(f, xu, cu)), "the unaligned path differs from the aligned one"
    # the dispatcher's door
    from sefd_amd import ops  # noqa: F401
    if fn == "unfold":
        g = lambda t: torch.ops.sefd.unfold(t, arg)
    else:
        g = lambda t: torch.ops.sefd.basemodel_norm(t, bc.KIND[fn], 1 if arg is None else arg)
    assert _same(base, _run(g, x, cot)), "torch.ops.sefd differs from the method"
    assert _same(base, _run(g, xp, cot)), "torch.ops.sefd on a non-contiguous input differs"
    with torch.no_grad():
        assert torch.equal(f(x), base[0]) and not f(x).requires_grad


def test_input_rules():
    B = BM()
    x4 = torch.rand(2, 1, 9, 8, device="cuda") + 0.1
    for bad in (x4.double(), x4.half(), x4.to(torch.int32)):
        with pytest.raises(TypeError):
            B.cumulative_laplace_norm(bad)
        with pytest.raises(TypeError):
            B.unfold(bad, 1)
    with pytest.raises(RuntimeError):
        B.unfold(x4, 9)                                   # n >= F: torch's reflect pad refuses it too
    with pytest.raises(RuntimeError):
        B.forgetting_norm(x4[:, 0], 0)                    # sample length below 1
    with pytest.raises(RuntimeError):
        B.sband_forgetting_norm(x4[:, 0, :1], 4)          # F = 1: there is no bin F // 2 - 1
    assert torch.equal(B.unfold(x4, 0), x4.permute(0, 2, 1, 3).reshape(2, 9, 1, 1, 8)) and torch.equal(B.unfold(x4, -2), B.unfold(x4, 0))
    x = x4.clone().requires_grad_(True)
    y = B.cumulative_laplace_norm(x)
    g, = torch.autograd.grad(y.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):                     # no double backward
        torch.autograd.grad(g.sum(), x)


def test_c_abi_refusals_launch_nothing():
    import sefd_amd  # noqa: F401
    from sefd_amd import _lib
    L = _lib.lib()
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, F, T = 2, 4, 8
    x = torch.rand(rows * F * T, device="cuda") + 0.1
    g = torch.rand(rows * F * T, device="cuda")
    fill = 123.25
    y = torch.full((rows * F * T * 8,), fill, device="cuda")          # a norm output, then the unfold output at n = 3 (7 times the input)
    nws = L.sefd_norm_ws_floats(4, rows, F, T)
    ws = torch.full((nws + 16,), fill, device="cuda")
    refused = [
        lambda: L.sefd_norm_forward(-1, vp(x), rows, F, T, 4, vp(ws), vp(y), st),
        lambda: L.sefd_norm_forward(7, vp(x), rows, F, T, 4, vp(ws), vp(y), st),
        lambda: L.sefd_norm_forward(1, vp(x), 0, F, T, 4, vp(ws), vp(y), st),
        lambda: L.sefd_norm_forward(1, vp(x), rows, 0, T, 4, vp(ws), vp(y), st),
        lambda: L.sefd_norm_forward(3, vp(x), rows, F, 0, 4, vp(ws), vp(y), st),
        lambda: L.sefd_norm_forward(4, vp(x), rows, F, T, 0, vp(ws), vp(y), st),
        lambda: L.sefd_norm_forward(5, vp(x), rows, F, T, -3, vp(ws), vp(y), st),
        lambda: L.sefd_norm_forward(6, vp(x), rows, F, T, 0, vp(ws), vp(y), st),
        lambda: L.sefd_norm_forward(5, vp(x), rows, 1, T, 4, vp(ws), vp(y), st),
        lambda: L.sefd_norm_forward(2, vp(x), rows, 1, 1, 4, vp(ws), vp(y), st),
        lambda: L.sefd_norm_backward(7, vp(x), vp(g), rows, F, T, 4, vp(ws), vp(y), st),
        lambda: L.sefd_norm_backward(4, vp(x), vp(g), rows, F, T, 0, vp(ws), vp(y), st),
        lambda: L.sefd_norm_backward(5, vp(x), vp(g), rows, 1, T, 4, vp(ws), vp(y), st),
        lambda: L.sefd_norm_backward(2, vp(x), vp(g), rows, 1, 1, 4, vp(ws), vp(y), st),
        lambda: L.sefd_norm_backward(1, vp(x), vp(g), rows, F, -1, 4, vp(ws), vp(y), st),
        lambda: L.sefd_unfold_forward(vp(x), 1, rows, F, T, F, vp(y), st),
        lambda: L.sefd_unfold_forward(vp(x), 1, rows, F, T, -1, vp(y), st),
        lambda: L.sefd_unfold_forward(vp(x), 0, rows, F, T, 1, vp(y), st),
        lambda: L.sefd_unfold_backward(vp(g), 1, rows, F, T, F, vp(y), st),
        lambda: L.sefd_unfold_backward(vp(g), 1, rows, F, T, -1, vp(y), st),
        lambda: L.sefd_unfold_backward(vp(g), 1, rows, F, 0, 1, vp(y), st),
    ]
    for i, call in enumerate(refused):
        assert call() == -1, i
    torch.cuda.synchronize()
    assert bool((y == fill).all()) and bool((ws == fill).all())
    # the same buffers are written when the arguments are fine
    assert L.sefd_norm_forward(4, vp(x), rows, F, T, 4, vp(ws), vp(y), st) == 0
    assert L.sefd_unfold_forward(vp(x), 1, rows, F, T, 3, vp(y[rows * F * T:]), st) == 0
    torch.cuda.synchronize()
    assert bool((y != fill).all()) and bool((ws[:rows * T * 4] != fill).all()) and bool((ws[nws:] == fill).all())


@pytest.mark.parametrize("fn", bc.SIGNED)
def test_two_values_per_row(fn):
    """F = 2, T = 1 for the two signed norms: the smallest size the entry points take.  Two values normalised by their own mean and std are
    +- 1 / sqrt(2) (unbiased std) or +- 1 (the layer norm) up to the eps term, whatever they are, so the gradient is zero but for that term and the
    generator refuses a golden (the reference's own float32 gradient is off by 2.7e-2 of it).  Against the float64 restatement instead: the forward at
    the golden tests' bar at its floor; the gradient, whose terms of size |g| / sd <= 1e4 cancel in double (2^-52 of them, 2e-12) before one float32
    rounding, within the same bar of its largest element plus 1e-10."""
    x, cot = bc._u(33000, (3, 1, 2, 1)), bc._u(33001, (3, 1, 2, 1))
    assert float((x[:, 0, 0, 0] - x[:, 0, 1, 0]).abs().min()) > 1e-3               # |g| / sd stays below 1e4
    x64 = x.double().requires_grad_(True)
    ref = getattr(bc.Ref, fn)(x64)
    ref.backward(cot.double())
    xg = x.cuda().requires_grad_(True)
    y = getattr(BM(), fn)(xg)
    y.backward(cot.cuda())
    e = bc.rel_err(y.detach(), ref.detach())
    gmax = float(x64.grad.abs().max())
    ge = float((xg.grad.double().cpu() - x64.grad).abs().max())
    print(f"{fn} [3, 1, 2, 1]: forward {e:.2e} bar {bc.BAR * bc.E32_FLOOR:.1e}; gradient max {gmax:.2e} abs err {ge:.2e} bar {bc.BAR * bc.E32_FLOOR * gmax + 1e-10:.2e}")
    assert e <= bc.BAR * bc.E32_FLOOR
    assert ge <= bc.BAR * bc.E32_FLOOR * gmax + 1e-10


def test_dispatcher_registration():
    from sefd_amd import ops  # noqa: F401
    x4 = (torch.rand(2, 2, 9, 8, device="cuda") + 0.1).requires_grad_(True)
    x3 = (torch.rand(2, 9, 7, device="cuda") + 0.1).requires_grad_(True)
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.sefd.basemodel_norm.default, (x4, 3, 1), test_utils=tests)
    torch.library.opcheck(torch.ops.sefd.basemodel_norm.default, (x3, 6, 4), test_utils=tests)
    torch.library.opcheck(torch.ops.sefd.unfold.default, (x4, 2), test_utils=tests)
    torch.library.opcheck(torch.ops.sefd.basemodel_norm_forward.default, (x4.detach(), 1, 1), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.sefd.unfold_backward.default, (torch.rand(2, 9, 2, 5, 8, device="cuda"), 2, 2, 9, 8, 2),
                          test_utils=("test_schema", "test_faketensor"))


def test_unfold_of_a_norm_feeds_a_sequence_model():
    """x -> cumulative_laplace_norm -> unfold -> [B F, 2 n + 1, T] -> SequenceModel -> sum(out * cot), one backward.  The SequenceModel hands back
    g = d loss / d (its input); the float64 restatement on the CPU pulls the same g back through ref_unfold(ref_norm(x)).  Two float32 roundings (the
    unfold gradient, the norm gradient) separate the two: within 4 x 1e-7 of the largest gradient, the golden tests' bar at its floor."""
    import sefd_amd  # noqa: F401
    from sefd_amd import models
    from oracle.weights import fill_state_dict_
    B, F, T, n = 2, 9, 7, 3
    m = models.SequenceModel(2 * n + 1, 2, 64, 1, False, "LSTM", None)
    fill_state_dict_(m)
    m = m.to("cuda").train()
    m.dropout_keep = 1.0
    x0 = 0.05 + (bc._u(32000, (B, 1, F, T)) + 1) / 2
    cot = bc._u(32001, (B * F, 2, T)).cuda()
    x = x0.cuda().requires_grad_(True)
    u = models.BaseModel.unfold(models.BaseModel.cumulative_laplace_norm(x), n)
    u.retain_grad()
    out = m(u.reshape(B * F, 2 * n + 1, T))
    (out * cot).sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all()) and float(u.grad.abs().max()) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    x64 = x0.double().requires_grad_(True)
    u64 = bc.ref_unfold(bc.ref_cumulative_laplace_norm(x64), n)
    (u64 * u.grad.double().cpu()).sum().backward()
    ef, eg = bc.rel_err(u, u64.detach()), bc.rel_err(x.grad, x64.grad)
    print(f"composed: forward {ef:.2e} gradient {eg:.2e} bar {bc.BAR * bc.E32_FLOOR:.1e}")
    assert ef <= bc.BAR * bc.E32_FLOOR and eg <= bc.BAR * bc.E32_FLOOR
