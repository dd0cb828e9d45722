"""GPU: the conv layers and ComplexBatchNorm on their own (models.py, csrc/plan_layers.cpp models 9 / 10, csrc/layout.hip) against goldens captured
from the real reference in float64 (tests/golden/make_convlayer_golden.py).

The bar of the fp32 modules, per tensor: max|got - ref64| / max|ref64| <= 4 x E32, E32 = the largest ref32_err among the case's tensors (the same
measure of the reference's own float32 CPU run; 1.1e-7 .. 7.2e-7 over the cases).  The factor 4 is convstft_common.BAR: same-precision arithmetic
summed in another order errs by the same order of magnitude; a wrong tap, sign, phase or pad is four to six orders above that.  The per-case maximum
is used because some tensors (running statistics after a lerp_, a near-constant dWri) have a float32 reference error below one float32 ulp."""
import pytest
import torch

import convlayer_common as lc
import opcheck
from plan_check import report_path
from simutil import ARENA_COUNT, ARENA_GRAD, PHASE_BWD, PHASE_FWD, Plan, fill_params, read_params, sim_run

pytestmark = pytest.mark.gpu
OP_NCHW_CL = 51                # sefd_desc.h OpKind


def _ns():
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, tools_for_model
    cfg.act_dtype = "fp32"
    return tools_for_model


def _gpu(module, inp, training=True, forward_of=None):
    lc.fill_(module, lc.SEED)
    module = module.cuda().train(training)
    res = lc.run_module(module, inp, torch.float32, "cuda", forward=forward_of(module) if forward_of else None)
    for k, v in res.items():
        assert torch.isfinite(v).all(), k
    return res, module


@pytest.mark.parametrize("name", list(lc.CASES))
def test_conv_modules_against_reference_golden(name):
    ref, e32, seed = lc.load_golden(name)
    res, m = _gpu(lc.make_conv(_ns(), name), lc.conv_inputs(name, seed))
    assert set(ref) <= set(res)
    lc.check(res, ref, e32, name)
    if name == "t_dec":                       # the reference's (real, imag) input form
        x = lc.conv_inputs(name, seed)["x"].cuda()
        assert torch.equal(m(list(torch.chunk(x, 2, 1))), m(x)) and torch.equal(m(tuple(torch.chunk(x, 2, 1))), m(x))


@pytest.mark.parametrize("name", list(lc.CBN_CASES))
def test_cbn_module_against_reference_golden(name):
    """... and the buffers: training advances num_batches_tracked by one per forward and moves the running statistics; eval leaves every buffer bit-equal."""
    C, rest, training, momentum = lc.CBN_CASES[name]
    ref, e32, seed = lc.load_golden(name)
    m = _ns().ComplexBatchNorm(C, momentum=momentum)
    lc.fill_(m, lc.SEED)
    before = {k: v.clone() for k, v in m.state_dict().items() if k[0] == "R" or k == "num_batches_tracked"}
    res, m = _gpu(m, lc.cbn_inputs(name, seed), training)
    lc.check(res, ref, e32, name)
    after = m.state_dict()
    if training:
        assert int(after["num_batches_tracked"]) == 1
        m(lc.cbn_inputs(name, seed)["x"].cuda())
        assert int(m.num_batches_tracked) == 2
        assert not torch.equal(after["RMr"].cpu(), before["RMr"])
    else:
        for k, v in before.items():
            assert torch.equal(after[k].cpu(), v), k
        assert int(after["num_batches_tracked"]) == 0


@pytest.mark.parametrize("name", list(lc.CORR_CASES))
def test_cbn_module_on_correlated_parts_per_channel(name):
    """Imaginary part = rho * real + sqrt(1 - rho^2) * noise (rho 0.9, 0.999, 1): every family of tensors of every complex channel within BAR times
    the error of the reference's own float32 run in that channel; both sides' figures go to the report file."""
    ref, e32, seed = lc.load_corr_golden(name)
    m = _ns().ComplexBatchNorm(lc.CORR_C, momentum=lc.CORR_MOMENTUM)
    res, m = _gpu(m, lc.corr_inputs(name, seed), True)
    path = report_path(f"convlayers_{name}.txt")
    open(path, "w").close()
    lc.check_per_channel(res, ref, e32, name, report=path)


def _layout(B, C, F, T, dt, mode, t_off, Tcl, nchw, cl):
    """One OP_NCHW_CL launch through the C ABI's test entry (sefd_nchw_cl): nchw / cl are device tensors."""
    import ctypes as ct
    from sefd_amd import _lib
    cpad = -(-C // 8) * 8
    rc = _lib.lib().sefd_nchw_cl(ct.c_void_p(nchw.data_ptr()), ct.c_void_p(cl.data_ptr()), B, C, cpad, F, T, Tcl, t_off, dt, mode,
                                 ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("tile", [64, 32])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 2, 17, 7), (1, 12, 33, 5), (2, 40, 3, 70), (3, 64, 5, 33), (2, 24, 170, 1), (1, 72, 2, 130)])
def test_layout_kernel_alone(shape, dtype, tile):
    """All four modes, bit-equal to permute + zero pad + .to(bfloat16) in torch, pad channels exactly 0; a frame offset of 1 on every shape but the T = 1 form.
    tile: the 64 x 64 tile (default) and the 32 x 32 one (knob LAYOUT_TILE); the shapes have C and T below, at and across either edge."""
    from util import knobs
    knobs.set("LAYOUT_TILE", tile)
    B, C, F, T = shape
    td, dt = (torch.float32, 0) if dtype == "fp32" else (torch.bfloat16, 1)
    cpad = -(-C // 8) * 8
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g).cuda()
    want = torch.nn.functional.pad(x.permute(0, 3, 2, 1), (0, cpad - C)).contiguous().to(td)            # [B][T][F][Cpad]
    for mode in (0, 2):                                                                                 # input in, cotangent in
        for t_off in ((0,) if T == 1 else (0, 1)):
            Tcl = T + t_off
            cl = torch.full((B, Tcl, F, cpad), 7.0, dtype=td, device="cuda")
            _layout(B, C, F, T, dt, mode, t_off, Tcl, x, cl)
            assert torch.equal(cl[:, t_off:], want), (mode, t_off)
            assert float(cl[:, t_off:, :, C:].float().abs().sum()) == 0.0
            assert bool((cl[:, :t_off] == 7.0).all())                                                   # frames in front of the offset: untouched
    for mode in (1, 3):                                                                                 # output out, input gradient out
        for t_off in ((0,) if T == 1 else (0, 1)):
            Tcl = T + t_off
            cl = torch.randn((B, Tcl, F, cpad), generator=g).cuda().to(td)
            out = torch.full(shape, 7.0, device="cuda")
            _layout(B, C, F, T, dt, mode, t_off, Tcl, out, cl)
            assert torch.equal(out, cl[:, t_off:, :, :C].float().permute(0, 3, 2, 1).contiguous()), (mode, t_off)


def _ops_against_simulator(plan, values, inputs, report):
    """Every op but the layout ops on the device and on the host simulator from the same pre-op state, under the rule of tests/opcheck.py: fp32
    buffers 1e-3, bf16 buffers 1.6e-2 (test_gpu_ops.test_every_op_against_host_simulator), relative to the largest element of the buffer; every
    parameter gradient and module buffer relative to the largest element of that tensor; no byte written where the simulator writes none.  The
    layout ops run on the device only.  report: file in the report directory (plan_check.report_path) for the per-op lines and the per-tensor table."""
    dev = plan.alloc_arenas("cuda")
    fill_params(plan, dev, values)
    table = opcheck.region_table(plan)
    assert not any(r[4].endswith(".bnpart") for r in table.regions)      # no statistics sums in these plans: every fp32 bar here is 1e-3
    n_checked, lines, log = 0, [], opcheck.TensorLog()
    for phase, (io, t) in ((PHASE_FWD, inputs[0]), (PHASE_BWD, inputs[1])):
        plan.io(dev, io, tuple(t.shape)).copy_(t)
        kinds = [int(k) for k in plan.op_kinds(phase)[0]]
        for i, kind in enumerate(kinds):
            host = [a.cpu().clone() for a in dev]
            prev = [a.clone() for a in host]
            plan.run(phase, dev, 0, i, i + 1)
            torch.cuda.synchronize()
            assert plan.status() == 0
            if kind == OP_NCHW_CL:
                continue
            sim_run(plan, phase, host, i, i + 1)
            v = opcheck.compare_op(prev, host, [a.cpu() for a in dev], table, kind, "bf16")
            log.add(v)
            lines.append(f"phase {phase} op {i:3d} kind {kind:3d} elems {v.elems:9d} err/tol {v.worst:.3e} stray {v.stray} {v.where}")
            print(lines[-1])
            with open(report_path(report), "w") as f:
                f.write("\n".join(lines + log.lines()) + "\n")
            assert v.stray == 0, f"phase {phase} op {i} (kind {kind}) wrote {v.stray} bytes that the simulator leaves alone"
            assert v.worst < 1.0, (phase, i, kind, v.where)
            n_checked += len(v.rows)
    assert n_checked > 0


@pytest.mark.parametrize("name", ["enc_mid", "odd_ch", "k3s1", "t_dec", "t_mask", "r_dec"])
def test_bf16_conv_plans_op_by_op(name):
    from sefd_amd import models
    cls, ci, co, k, s, p, extra, F, T = lc.CASES[name]
    plan = Plan(lc.B, T, act_dtype="bf16", model="ConvLayer",
                conv=dict(kind=cls, in_channels=ci, out_channels=co, kernel_size=k, stride_f=s[0], padding=p, causal=extra.get("causal", True),
                          output_padding_f=extra.get("output_padding", (0, 0))[0], F=F))
    m = lc.make_conv(models, name)
    lc.fill_(m, lc.SEED)
    inp = lc.conv_inputs(name)
    _ops_against_simulator(plan, m.state_dict(), (("x", inp["x"]), ("grad_y", inp["cot"])), f"convlayer_ops_{name}.txt")


@pytest.mark.parametrize("name", lc.INT_CASES)
def test_bf16_conv_plans_on_integer_data_equal_the_reference_exactly(name):
    """The anchor outside the descriptor (the simulator reads the same RunGemm as the kernel): on integer data the real reference's result
    (tests/golden/make_convlayer_golden.py, convlayer_<name>_int.npz) is exact in any arithmetic.  Both phases of the bf16 plan run whole; y and dx must
    equal the golden rounded to bf16, byte for byte, and every parameter gradient the golden itself, as fp32 (the CPU twin, on the simulator:
    test_convlayers_cpu.py)."""
    from sefd_amd import models
    cls, ci, co, k, s, p, extra, F, T = lc.CASES[name]
    Fo, To = lc.out_geometry(name)
    ref, seed = lc.load_int_golden(name)
    plan = Plan(lc.B, T, act_dtype="bf16", model="ConvLayer",
                conv=dict(kind=cls, in_channels=ci, out_channels=co, kernel_size=k, stride_f=s[0], padding=p, causal=extra.get("causal", True),
                          output_padding_f=extra.get("output_padding", (0, 0))[0], F=F))
    m = lc.make_conv(models, name)
    lc.fill_int_(m, seed)
    inp = lc.int_inputs(name, seed)
    dev = plan.alloc_arenas("cuda")
    fill_params(plan, dev, m.state_dict())
    plan.io(dev, "x", tuple(inp["x"].shape)).copy_(inp["x"])
    plan.run(PHASE_FWD, dev)
    plan.io(dev, "grad_y", tuple(inp["cot"].shape)).copy_(inp["cot"])
    plan.run(PHASE_BWD, dev)
    torch.cuda.synchronize()
    assert plan.status() == 0
    res = {"y": plan.io(dev, "y", (lc.B, co, Fo, To)).cpu(), "dx": plan.io(dev, "grad_x", (lc.B, ci, F, T)).cpu()}
    for key in ("y", "dx"):
        got, want = res[key].to(torch.bfloat16), ref[key].to(torch.bfloat16)
        assert torch.equal(got.float(), res[key])                    # (the fp32 I/O tensor holds the plan's bf16 values)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (name, key, int((got != want).sum()), "elements differ from the reference")
    grads = read_params(plan, dev, ARENA_GRAD)
    assert set(ref) == {"y", "dx"} | {"d/" + n for n in grads}
    for n, v in grads.items():
        assert torch.equal(v, ref["d/" + n]), (name, n, int((v != ref["d/" + n]).sum()), "elements differ from the reference")


def test_bf16_cbn_plan_op_by_op():
    from sefd_amd import models
    name = "cbn24_5x6_train01"
    C, rest, training, momentum = lc.CBN_CASES[name]
    plan = Plan(lc.B, 30, act_dtype="bf16", training=True, model="ComplexBatchNorm", cbn=dict(num_features=C, momentum=momentum))
    m = models.ComplexBatchNorm(C, momentum=momentum)
    lc.fill_(m, lc.SEED)
    inp = lc.cbn_inputs(name)
    _ops_against_simulator(plan, m.state_dict(), (("x", inp["x"].reshape(lc.B, C, 30)), ("grad_y", inp["cot"].reshape(lc.B, C, 30))), f"convlayer_ops_{name}.txt")


def test_composition_and_stamp():
    """nn.Sequential(ComplexConv2d, ComplexBatchNorm, PReLU) followed by ComplexConvTranspose2d: every parameter gradient and the input gradient against
    the float64 golden of the same stack; then two forwards of one shape followed by the first one's backward raise the stamp error."""
    ref, e32, seed = lc.load_golden(lc.STACK)
    res, stack = _gpu(lc.make_stack(_ns()), lc.stack_inputs(seed), True, lc.stack_forward)
    assert set(ref) <= set(res)
    lc.check(res, ref, e32, lc.STACK)
    conv = stack[0][0]
    x = lc.stack_inputs(seed)["x"].cuda().requires_grad_(True)
    y1 = conv(x)
    conv(x)
    with pytest.raises(RuntimeError, match="a later forward of the same shape overwrote the activations"):
        y1.sum().backward()
