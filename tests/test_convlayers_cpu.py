"""CPU: the conv layers, ComplexBatchNorm, cPReLU and complex_cat of tools_for_model.py:126-607 on their own - exports, constructor signatures,
state_dict keys, every refusal sentence, the two planner models (csrc/plan_layers.cpp, ids 9 and 10) over the golden case table, and the op range
between the layout ops on the host simulator against the float64 goldens (the simulator does not interpret OP_NCHW_CL: the test fills and reads the
channels-last buffers itself)."""
import inspect
import os
import subprocess
import sys

import pytest
import torch

import convlayer_common as lc
from simutil import ARENA_GRAD, ARENA_STATE, PHASE_BWD, PHASE_FWD, Plan, act_to_nchw, fill_params, read_params, sim, sim_run

OP_NCHW_CL = 51                # sefd_desc.h OpKind
TOL = 1e-3                     # the project's fp32 simulator bar (plan_check.TOL): an index error is O(0.1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ("ComplexConv2d", "ComplexConvTranspose2d", "RealConv2d", "RealConvTranspose2d", "ComplexBatchNorm", "cPReLU", "complex_cat")


def _ns():
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_model
    return tools_for_model


def test_exports_and_dropin():
    from sefd_amd import models
    tfm = _ns()
    for n in LAYERS:
        assert getattr(tfm, n) is getattr(models, n)
    code = ("import sys; sys.path.insert(0, %r); import tools_for_model as t, models as m; "
            "assert all(getattr(t, n) is getattr(m, n) for n in %r); print('same')") % (os.path.join(ROOT, "dropin"), LAYERS)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "same" in out.stdout, out.stderr


def test_constructor_signatures_and_state_dicts():
    tfm = _ns()
    conv = ["self", "in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation", "groups", "causal", "complex_axis"]
    want = {
        "ComplexConv2d": (conv, [(1, 1), (1, 1), (0, 0), 1, 1, True, 1]),
        "RealConv2d": (conv, [(1, 1), (1, 1), (0, 0), 1, 1, True, 1]),
        "ComplexConvTranspose2d": (["self", "in_channels", "out_channels", "kernel_size", "stride", "padding", "output_padding", "causal", "complex_axis",
                                    "groups"], [(1, 1), (1, 1), (0, 0), (0, 0), False, 1, 1]),
        "RealConvTranspose2d": (["self", "in_channels", "out_channels", "kernel_size", "stride", "padding", "output_padding", "groups"],
                                [(1, 1), (1, 1), (0, 0), (0, 0), 1]),
        "ComplexBatchNorm": (["self", "num_features", "eps", "momentum", "affine", "track_running_stats", "complex_axis"], [1e-5, 0.1, True, True, 1]),
        "cPReLU": (["self", "complex_axis"], [1]),
    }
    for name, (params, defaults) in want.items():
        sig = inspect.signature(getattr(tfm, name).__init__)
        assert list(sig.parameters) == params, name
        assert [p.default for p in sig.parameters.values() if p.default is not inspect.Parameter.empty] == defaults, name
    c = tfm.ComplexConv2d(16, 32, (5, 2), (2, 1), (2, 1))
    assert list(c.state_dict()) == ["real_conv.weight", "real_conv.bias", "imag_conv.weight", "imag_conv.bias"]
    assert (c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.causal, c.groups, c.dilation, c.complex_axis) == \
        (8, 16, (5, 2), (2, 1), (2, 1), True, 1, 1, 1)
    assert tuple(c.real_conv.weight.shape) == (16, 8, 5, 2) and tuple(c.real_conv.padding) == (2, 0) and float(c.imag_conv.bias.detach().abs().max()) == 0.0
    t = tfm.ComplexConvTranspose2d(32, 16, (5, 2), (2, 1), (2, 0), (1, 0))
    assert list(t.state_dict()) == ["real_conv.weight", "real_conv.bias", "imag_conv.weight", "imag_conv.bias"]
    assert (t.in_channels, t.out_channels, t.output_padding, t.complex_axis) == (16, 8, (1, 0), 1) and tuple(t.real_conv.weight.shape) == (16, 8, 5, 2)
    r, rt = tfm.RealConv2d(8, 16, (5, 2), (2, 1), (2, 1)), tfm.RealConvTranspose2d(16, 8, (5, 2), (2, 1), (2, 0), (1, 0))
    assert list(r.state_dict()) == ["conv.weight", "conv.bias"] == list(rt.state_dict())
    assert (r.in_channels, r.out_channels) == (8, 16) and tuple(rt.conv.weight.shape) == (16, 8, 5, 2)
    d = tfm.ComplexConv2d(4, 4)
    assert (d.kernel_size, d.stride, d.padding) == ((1, 1), (1, 1), (0, 0))
    n = tfm.ComplexBatchNorm(16, momentum=0.3)
    assert list(n.state_dict()) == ["Wrr", "Wri", "Wii", "Br", "Bi", "RMr", "RMi", "RVrr", "RVri", "RVii", "num_batches_tracked"]
    assert (n.num_features, n.eps, n.momentum, n.affine, n.track_running_stats, n.complex_axis) == (8, 1e-5, 0.3, True, True, 1)
    assert float(n.Wrr.detach().min()) == 1.0 and float(n.Wri.detach().abs().max()) <= 0.9 and float(n.Br.detach().abs().max()) == 0.0 and float(n.RVii.min()) == 1.0
    n.RMr.fill_(3.0)
    n.num_batches_tracked.fill_(5)
    n.reset_running_stats()
    assert float(n.RMr.abs().max()) == 0.0 and int(n.num_batches_tracked) == 0
    p = tfm.cPReLU()
    assert list(p.state_dict()) == ["r_prelu.weight", "i_prelu.weight"] and p.complex_axis == 1
    x = torch.arange(-8.0, 8.0).view(1, 4, 2, 2)
    assert torch.equal(p(x), torch.where(x > 0, x, 0.25 * x))
    a, b = torch.arange(8.0).view(1, 4, 2), 10 + torch.arange(4.0).view(1, 2, 2)
    assert torch.equal(tfm.complex_cat([a, b], 1), torch.cat([a[:, :2], b[:, :1], a[:, 2:], b[:, 1:]], 1))
    for m, shape in ((c, (2, 16, 9, 5)), (n, (2, 16, 4))):
        with pytest.raises(RuntimeError, match="runs on the MI355X only"):
            m(torch.zeros(shape))


@pytest.mark.parametrize("cls,args,kw,text", [
    ("ComplexConv2d", (8, 8), dict(dilation=2), "dilation 2 is not built"),
    ("RealConv2d", (8, 8), dict(groups=2), "groups 2 is not built"),
    ("ComplexConvTranspose2d", (8, 8), dict(groups=2), "groups 2 is not built"),
    ("ComplexConv2d", (8, 8), dict(complex_axis=0), "complex_axis 0 is not built"),
    ("ComplexConv2d", (8, 8, (3, 2), (1, 2)), {}, "a time stride of 2 is not built"),
    ("RealConv2d", (8, 8, (5, 2), (3, 1)), {}, r"a frequency stride of 3 is not built \(1 \.\. 2\)"),
    ("ComplexConv2d", (8, 8, (8, 2)), {}, r"a kernel of 8 bins is not built \(1 \.\. 7\)"),
    ("RealConvTranspose2d", (8, 8, (3, 5)), {}, r"a kernel of 5 frames is not built \(1 \.\. 4"),
    ("ComplexConv2d", (8, 8, (3, 2), (1, 1), (3, 0)), {}, "padding .* must stay below the kernel extent"),
    ("ComplexConv2d", (8, 8, (3, 2), (1, 1), (1, 2)), {}, "padding .* must stay below the kernel extent"),
    ("ComplexConvTranspose2d", (8, 8, (3, 2), (2, 1), (1, 0), (2, 0)), {}, "output padding .* must stay below the stride"),
    ("RealConvTranspose2d", (8, 8, (3, 2), (1, 1), (1, 0), (0, 1)), {}, "output padding .* must stay below the stride"),
    ("ComplexConv2d", (7, 8), {}, "odd channel counts"),
    ("ComplexConvTranspose2d", (8, 3), {}, "odd channel counts"),
    ("ComplexBatchNorm", (12,), {}, "num_features 12 is not a multiple of 8"),
    ("ComplexBatchNorm", (16,), dict(affine=False), "affine=False is not built"),
    ("ComplexBatchNorm", (16,), dict(track_running_stats=False), "track_running_stats=False is not built"),
    ("ComplexBatchNorm", (16,), dict(momentum=None), "momentum=None .* is not built"),
])
def test_every_refusal_names_its_limit(cls, args, kw, text):
    with pytest.raises(NotImplementedError, match=f"sefd {cls}: {text}"):
        getattr(_ns(), cls)(*args, **kw)


def test_geometries_without_output_are_refused_with_their_numbers():
    conv = dict(kind="ComplexConv2d", in_channels=8, out_channels=8, kernel_size=(5, 2), stride_f=2, padding=(0, 0), F=3)
    with pytest.raises(ValueError, match=r"ComplexConv2d plan: 3 bins x 6 frames under kernel \(5, 2\).* leave 0 output bins x 5 output frames"):
        Plan(2, 6, model="ConvLayer", conv=conv)
    with pytest.raises(ValueError, match=r"ComplexConv2d plan: 9 bins x 1 frames .* leave 3 output bins x 0 output frames"):
        Plan(2, 1, model="ConvLayer", conv=dict(conv, F=9))
    with pytest.raises(ValueError, match="num_features must be a multiple of 8"):
        Plan(2, 6, model="ComplexBatchNorm", cbn=dict(num_features=12))


def test_dccrn_and_crn_still_hold_their_layers():
    from sefd_amd import config as cfg, models
    cfg.dccrn_kernel_num, cfg.skip_type, cfg.lstm = [16, 32, 32, 64, 64, 64], True, "complex"
    for m, kw in ((models.DCCRN(rnn_units=128), {}), (models.DCCRN(rnn_units=128, use_cbn=True), {}), (models.CRN(rnn_units=128, rnn_input_size=128), {})):
        plan = m._make_plan(2, 1600, True)
        assert [n for n, _ in m.named_parameters()] == list(plan.params), type(m).__name__
        assert [n for n, _ in m._bn_buffers()] == list(plan.state), type(m).__name__
        assert all(p._sefd_owner() is m for p in m.parameters())
    keys = list(models.DCCRN(rnn_units=128, use_cbn=True).state_dict())
    assert keys[4:9] == ["encoder.0.0.real_conv.weight", "encoder.0.0.real_conv.bias", "encoder.0.0.imag_conv.weight", "encoder.0.0.imag_conv.bias", "encoder.0.1.Wrr"]
    assert keys[13:19] == ["encoder.0.1.RMr", "encoder.0.1.RMi", "encoder.0.1.RVrr", "encoder.0.1.RVri", "encoder.0.1.RVii", "encoder.0.1.num_batches_tracked"]


def test_op_size_is_pinned():
    assert Plan(2, 6, model="ConvLayer", conv=dict(F=4)).lib.sefd_op_size() == 592 == sim().hostsim_op_size()


def _conv_plan(name, dtype):
    cls, ci, co, k, s, p, extra, F, T = lc.CASES[name]
    return Plan(lc.B, T, act_dtype=dtype, model="ConvLayer",
                conv=dict(kind=cls, in_channels=ci, out_channels=co, kernel_size=k, stride_f=s[0], padding=p, causal=extra.get("causal", True),
                          output_padding_f=extra.get("output_padding", (0, 0))[0], F=F))


def _kinds(plan, phase):
    return [int(k) for k in plan.op_kinds(phase)[0]]


def _run_between_layout_ops(plan, phase, ar):
    """Every op of the phase but the layout ops, in order."""
    kinds = _kinds(plan, phase)
    assert kinds.count(OP_NCHW_CL) == 2
    first = 0
    for i, k in enumerate(kinds + [OP_NCHW_CL]):
        if k == OP_NCHW_CL:
            if i > first:
                sim_run(plan, phase, ar, first, i)
            first = i + 1


def _to_cl(plan, ar, name, t, cpad):
    """[B, C, F, T] -> the channels-last buffer [B][T][F][Cpad] (pad channels zero)."""
    x = t.permute(0, 3, 2, 1)
    x = torch.nn.functional.pad(x, (0, cpad - x.shape[-1])).contiguous()
    plan.view(ar, name).copy_(x.reshape(-1))


@pytest.mark.parametrize("name", list(lc.CASES))
def test_conv_plans_and_host_simulator(name):
    from sefd_amd import models
    cls, ci, co, k, s, p, extra, F, T = lc.CASES[name]
    Fo, To = lc.out_geometry(name)
    cip, cop = -(-ci // 8) * 8, -(-co // 8) * 8
    for dtype in ("fp32", "bf16"):
        plan = _conv_plan(name, dtype)
        assert plan.T == To
        es = 4 if dtype == "fp32" else 2
        assert plan.buffer("x")[2] == lc.B * T * F * cip * es and plan.buffer("y")[2] == lc.B * To * Fo * cop * es
        assert plan.buffer("io.y")[2] == lc.B * co * Fo * To * 4 and plan.buffer("io.grad_x")[2] == lc.B * ci * F * T * 4
    plan = _conv_plan(name, "fp32")
    m = lc.make_conv(models, name)
    lc.fill_(m, lc.SEED)
    assert list(plan.params) == list(m.state_dict())
    ref, e32, seed = lc.load_golden(name)
    inp = lc.conv_inputs(name, seed)
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, m.state_dict())
    _to_cl(plan, ar, "x", inp["x"], cip)
    _run_between_layout_ops(plan, PHASE_FWD, ar)
    _to_cl(plan, ar, "dy", inp["cot"], cop)
    _run_between_layout_ops(plan, PHASE_BWD, ar)
    res = {"y": act_to_nchw(plan.view(ar, "y"), lc.B, To, Fo, cop)[:, :co], "dx": act_to_nchw(plan.view(ar, "dx"), lc.B, T, F, cip)[:, :ci]}
    res.update({"d/" + n: v for n, v in read_params(plan, ar, ARENA_GRAD).items()})
    assert float(act_to_nchw(plan.view(ar, "y"), lc.B, To, Fo, cop)[:, co:].abs().sum()) == 0.0          # pad channels: exact zeros
    for key, v in ref.items():
        err = lc.rel_err(res[key], v)
        print(f"{name} {key}: {err:.2e}")
        assert err < TOL, (name, key, err)


@pytest.mark.parametrize("name", lc.INT_CASES)
def test_bf16_conv_plans_on_integer_data_equal_the_reference_exactly(name):
    """The anchor outside the descriptor: simulator and kernel read the same RunGemm, so a tap the planner describes wrongly is wrong on both sides.  On
    integer data (convlayer_common.int_inputs / fill_int_) the real reference's result is exact in any arithmetic; the bf16 plan on the simulator must give
    y and dx equal to it rounded to bf16, byte for byte, and every parameter gradient equal to it as fp32 (the GPU twin: test_gpu_convlayers.py)."""
    from sefd_amd import models
    cls, ci, co, k, s, p, extra, F, T = lc.CASES[name]
    Fo, To = lc.out_geometry(name)
    cip, cop = -(-ci // 8) * 8, -(-co // 8) * 8
    ref, seed = lc.load_int_golden(name)
    assert all(torch.equal(v, v.round()) and float(v.abs().max()) < 2 ** 16 for v in ref.values())
    plan = _conv_plan(name, "bf16")
    m = lc.make_conv(models, name)
    lc.fill_int_(m, seed)
    inp = lc.int_inputs(name, seed)
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, m.state_dict())
    _to_cl(plan, ar, "x", inp["x"], cip)
    _run_between_layout_ops(plan, PHASE_FWD, ar)
    _to_cl(plan, ar, "dy", inp["cot"], cop)
    _run_between_layout_ops(plan, PHASE_BWD, ar)
    assert plan.view(ar, "y").dtype == torch.bfloat16 and plan.view(ar, "dx").dtype == torch.bfloat16
    res = {"y": act_to_nchw(plan.view(ar, "y"), lc.B, To, Fo, cop)[:, :co], "dx": act_to_nchw(plan.view(ar, "dx"), lc.B, T, F, cip)[:, :ci]}
    for key in ("y", "dx"):
        got, want = res[key].to(torch.bfloat16), ref[key].to(torch.bfloat16)
        assert torch.equal(got.float(), res[key])                    # (the buffer holds bf16 values)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (name, key, int((got != want).sum()), "elements differ from the reference")
    grads = read_params(plan, ar, ARENA_GRAD)
    assert set(ref) == {"y", "dx"} | {"d/" + n for n in grads}
    for n, v in grads.items():
        assert torch.equal(v, ref["d/" + n]), (name, n, int((v != ref["d/" + n]).sum()), "elements differ from the reference")


@pytest.mark.parametrize("name", list(lc.CBN_CASES))
def test_cbn_plans_and_host_simulator(name):
    from sefd_amd import models
    C, rest, training, momentum = lc.CBN_CASES[name]
    S = 1
    for r in rest:
        S *= r
    for dtype in ("fp32", "bf16"):
        plan = Plan(lc.B, S, act_dtype=dtype, training=training, model="ComplexBatchNorm", cbn=dict(num_features=C, momentum=momentum))
        assert plan.buffer("io.x")[2] == lc.B * C * S * 4 and plan.n_param == 5 * (C // 2) and plan.n_state == 5 * (C // 2)
    plan = Plan(lc.B, S, act_dtype="fp32", training=training, model="ComplexBatchNorm", cbn=dict(num_features=C, momentum=momentum))
    m = models.ComplexBatchNorm(C, momentum=momentum)
    lc.fill_(m, lc.SEED)
    ref, e32, seed = lc.load_golden(name)
    inp = lc.cbn_inputs(name, seed)
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, m.state_dict())
    before = read_params(plan, ar, ARENA_STATE, plan.state)
    flat = lambda t: t.reshape(lc.B, C, 1, S)
    _to_cl(plan, ar, "y", flat(inp["x"]), C)
    _run_between_layout_ops(plan, PHASE_FWD, ar)
    _to_cl(plan, ar, "dz", flat(inp["cot"]), C)
    _run_between_layout_ops(plan, PHASE_BWD, ar)
    shape = (lc.B, C) + tuple(rest)
    res = {"y": act_to_nchw(plan.view(ar, "z"), lc.B, S, 1, C).reshape(shape), "dx": act_to_nchw(plan.view(ar, "dy"), lc.B, S, 1, C).reshape(shape)}
    res.update({"d/" + n: v for n, v in read_params(plan, ar, ARENA_GRAD).items()})
    after = read_params(plan, ar, ARENA_STATE, plan.state)
    res.update({"buf/" + n: v for n, v in after.items()})
    if not training:
        assert all(torch.equal(after[n], before[n]) for n in before)
    for key, v in ref.items():
        if key == "buf/num_batches_tracked":
            continue                                        # the module's counter, not the plan's
        err = lc.rel_err(res[key], v)
        print(f"{name} {key}: {err:.2e}")
        assert err < TOL, (name, key, err)


@pytest.mark.parametrize("name", list(lc.CORR_CASES))
def test_cbn_plan_on_correlated_parts_per_channel(name):
    """ComplexBatchNorm where the imaginary part is rho * real + sqrt(1 - rho^2) * noise (rho 0.9, 0.999, 1: the covariance singular up to eps): the
    fp32 plan on the host simulator against the reference's float64 run, per complex channel, at convlayer_common.BAR times the error of the
    reference's own float32 run in that channel (convlayer_common.check_per_channel; the device's twin is in test_gpu_convlayers.py)."""
    from sefd_amd import models
    C, rest, S = lc.CORR_C, lc.CORR_REST, lc.CORR_REST[0] * lc.CORR_REST[1]
    plan = Plan(lc.B, S, act_dtype="fp32", training=True, model="ComplexBatchNorm", cbn=dict(num_features=C, momentum=lc.CORR_MOMENTUM))
    m = models.ComplexBatchNorm(C, momentum=lc.CORR_MOMENTUM)
    lc.fill_(m, lc.SEED)
    ref, e32, seed = lc.load_corr_golden(name)
    inp = lc.corr_inputs(name, seed)
    ar = plan.alloc_arenas("cpu")
    fill_params(plan, ar, m.state_dict())
    flat = lambda t: t.reshape(lc.B, C, 1, S)
    _to_cl(plan, ar, "y", flat(inp["x"]), C)
    _run_between_layout_ops(plan, PHASE_FWD, ar)
    _to_cl(plan, ar, "dz", flat(inp["cot"]), C)
    _run_between_layout_ops(plan, PHASE_BWD, ar)
    shape = (lc.B, C) + tuple(rest)
    res = {"y": act_to_nchw(plan.view(ar, "z"), lc.B, S, 1, C).reshape(shape), "dx": act_to_nchw(plan.view(ar, "dy"), lc.B, S, 1, C).reshape(shape)}
    res.update({"d/" + n: v for n, v in read_params(plan, ar, ARENA_GRAD).items()})
    res.update({"buf/" + n: v for n, v in read_params(plan, ar, ARENA_STATE, plan.state).items()})
    lc.check_per_channel(res, ref, e32, name + " (host simulator)")
