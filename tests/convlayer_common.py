"""Shared by tests/golden/make_convlayer_golden.py, tests/test_convlayers_cpu.py and tests/test_gpu_convlayers.py: the case tables of the conv
layers and ComplexBatchNorm on their own (tools_for_model.py:199-607), the closed-form inputs, cotangents and parameter values of a case
(splitmix streams of oracle/weights.py at the stored seed), the generic run over a module (the reference's or this package's), and the fixtures."""
import os

import numpy as np
import torch

from oracle.weights import splitmix_uniform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B = 2
BAR = 4.0                      # per tensor: max|got - ref64| / max|ref64| <= BAR * E32, E32 = the largest ref32_err among the case's tensors
SEED = 3

# name: (class, C_in, C_out, kernel, stride, padding, extra keywords, F, T)
_DEC = dict(output_padding=(1, 0))
CASES = {
    "enc_first": ("ComplexConv2d", 2, 16, (5, 2), (2, 1), (2, 1), {}, 17, 7),
    "enc_mid": ("ComplexConv2d", 16, 32, (5, 2), (2, 1), (2, 1), {}, 16, 9),
    "odd_ch": ("ComplexConv2d", 12, 20, (5, 2), (2, 1), (2, 1), {}, 33, 5),
    "k3s1": ("ComplexConv2d", 8, 24, (3, 3), (1, 1), (1, 2), {}, 10, 6),
    "point": ("ComplexConv2d", 16, 16, (1, 1), (1, 1), (0, 0), {}, 5, 6),
    "noncausal": ("ComplexConv2d", 8, 8, (3, 3), (1, 1), (1, 1), dict(causal=False), 9, 7),
    "k7s2": ("ComplexConv2d", 8, 8, (7, 2), (2, 1), (3, 1), {}, 13, 6),
    "pad0": ("ComplexConv2d", 8, 16, (3, 2), (2, 1), (0, 0), {}, 11, 6),
    "rows129": ("ComplexConv2d", 8, 8, (5, 2), (2, 1), (2, 1), {}, 6, 43),          # 258 output rows: a partial 128-row block
    "t_dec": ("ComplexConvTranspose2d", 32, 16, (5, 2), (2, 1), (2, 0), _DEC, 8, 7),
    "t_mask": ("ComplexConvTranspose2d", 32, 2, (5, 2), (2, 1), (2, 0), _DEC, 16, 5),
    "t_odd_ch": ("ComplexConvTranspose2d", 24, 12, (5, 2), (2, 1), (2, 0), _DEC, 9, 6),
    "t_k3s1": ("ComplexConvTranspose2d", 16, 8, (3, 1), (1, 1), (1, 0), {}, 10, 6),
    "t_k4s2": ("ComplexConvTranspose2d", 8, 8, (4, 2), (2, 1), (1, 0), {}, 7, 6),
    "t_tpad": ("ComplexConvTranspose2d", 8, 8, (3, 2), (2, 1), (1, 1), _DEC, 6, 7),
    "r_enc": ("RealConv2d", 8, 16, (5, 2), (2, 1), (2, 1), {}, 17, 7),
    "r_k3s1": ("RealConv2d", 12, 8, (3, 3), (1, 1), (1, 2), {}, 10, 6),
    "r_dec": ("RealConvTranspose2d", 16, 8, (5, 2), (2, 1), (2, 0), _DEC, 8, 7),
    "r_mask": ("RealConvTranspose2d", 16, 1, (5, 2), (2, 1), (2, 0), _DEC, 16, 5),
}

# ComplexBatchNorm: num_features x trailing shape x (training, momentum); momentum plays no part in eval mode
CBN_SHAPES = {"5x6": (5, 6), "33x5": (33, 5), "17": (17,)}
CBN_MODES = {"train01": (True, 0.1), "train03": (True, 0.3), "eval": (False, 0.1)}
CBN_CASES = {f"cbn{C}_{s}_{m}": (C, CBN_SHAPES[s], *CBN_MODES[m]) for C in (8, 24, 32, 40) for s in CBN_SHAPES for m in CBN_MODES}
# ComplexBatchNorm on CORRELATED parts (C = 8, trailing shape (33, 5), training, momentum 0.1): imaginary = rho * real + sqrt(1 - rho^2) * noise.  The
# covariance of a complex channel is then near singular (rho = 1: singular up to eps), where V^-1/2 and its derivative are ill-conditioned
CORR_CASES = {"cbn8_corr09": 0.9, "cbn8_corr0999": 0.999, "cbn8_corr1": 1.0}
CORR_C, CORR_REST, CORR_MOMENTUM = 8, (33, 5), 0.1
STACK = "stack"                # the composition case: conv + ComplexBatchNorm + PReLU + transposed conv on [2, 2, 16, 9]
STACK_SHAPE, STACK_OUT = (2, 2, 16, 9), (2, 2, 16, 10)      # 8 bins x 9 frames in between; the transposed conv adds a frame


def _u(idx, shape):
    return torch.from_numpy(np.ascontiguousarray(splitmix_uniform(idx, int(np.prod(shape))).reshape(shape), dtype=np.float32))


def make_conv(ns, name):
    """The module of a conv case from namespace `ns` (the reference's tools_for_model or this package's)."""
    cls, ci, co, k, s, p, extra, _, _ = CASES[name]
    return getattr(ns, cls)(ci, co, k, s, p, **extra)


def out_geometry(name):
    cls, ci, co, (kh, kw), (sf, _), (pf, pt), extra, F, T = CASES[name]
    if "Transpose" in cls:
        return (F - 1) * sf - 2 * pf + kh + extra.get("output_padding", (0, 0))[0], T + kw - 1 - 2 * pt
    return (F + 2 * pf - kh) // sf + 1, T + (pt if extra.get("causal", True) and pt else 2 * pt) - kw + 1


def fill_(module, seed, base=0):
    """Every parameter 0.3 u (biases and Wri included: a zero bias hides a bias bug), ComplexBatchNorm's diagonal weights 1 + 0.3 u, running means
    0.2 u, running variances 1 + 0.3 u (RVri 0.2 u): W and V stay positive definite."""
    with torch.no_grad():
        for i, (n, t) in enumerate(list(module.named_parameters()) + list(module.named_buffers())):
            if n.endswith("num_batches_tracked"):
                continue
            leaf = n.rsplit(".", 1)[-1]
            v = _u(9000 + 64 * seed + base + i, tuple(t.shape)).to(t.dtype)
            if leaf in ("Wrr", "Wii", "RVrr", "RVii"):
                v = 1 + 0.3 * v
            elif leaf in ("RMr", "RMi", "RVri"):
                v = 0.2 * v
            elif t.dim() == 1 and t.numel() == 1:          # a PReLU slope
                v = 0.25 + 0.1 * v
            else:
                v = 0.3 * v
            t.copy_(v.to(t.device))


def conv_inputs(name, seed=SEED):
    cls, ci, co, k, s, p, extra, F, T = CASES[name]
    Fo, To = out_geometry(name)
    return dict(x=_u(8000 + 16 * seed, (B, ci, F, T)), cot=_u(8001 + 16 * seed, (B, co, Fo, To)))


# The integer variant of the bf16 plans' cases (convlayer_<name>_int.npz): x and the cotangent integers in -3 .. 3, every weight and bias an integer in
# -1 .. 1.  Every y, dx and parameter gradient is then an integer far below 2^24: float32 and float64 give the same numbers, in any order of additions,
# and a bf16 plan must give y and dx rounded to bf16 and the parameter gradients themselves, exactly.
INT_CASES = ("enc_mid", "odd_ch", "k3s1", "t_dec", "t_mask", "r_dec")


def _ints(idx, shape, hi):
    """Integers uniform in -hi .. hi from splitmix stream `idx`, as float32."""
    u = splitmix_uniform(idx, int(np.prod(shape)))
    v = np.minimum(np.floor((u + 1.0) * (hi + 0.5)), 2 * hi) - hi
    return torch.from_numpy(np.ascontiguousarray(v.reshape(shape), dtype=np.float32))


def int_inputs(name, seed=SEED):
    cls, ci, co, k, s, p, extra, F, T = CASES[name]
    Fo, To = out_geometry(name)
    return dict(x=_ints(8007 + 16 * seed, (B, ci, F, T), 3), cot=_ints(8008 + 16 * seed, (B, co, Fo, To), 3))


def fill_int_(module, seed):
    with torch.no_grad():
        for i, (n, t) in enumerate(module.named_parameters()):
            t.copy_(_ints(9500 + 64 * seed + i, tuple(t.shape), 1).to(device=t.device, dtype=t.dtype))


def load_int_golden(name):
    """({"y", "dx", "d/<parameter>": tensor of integers, float32}, seed) of an integer case."""
    z = np.load(os.path.join(GOLDEN, f"convlayer_{name}_int.npz"))
    return {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("ref/")}, int(z["seed"])


def cbn_inputs(name, seed=SEED):
    C, rest, _, _ = CBN_CASES[name]
    shape = (B, C) + tuple(rest)
    x = _u(8002 + 16 * seed, shape) + 0.5 * _u(8003 + 16 * seed, (1, C) + (1,) * len(rest))      # per-channel offsets: means that matter
    return dict(x=x, cot=_u(8004 + 16 * seed, shape))


def corr_inputs(name, seed=SEED):
    rho, h = CORR_CASES[name], CORR_C // 2
    shape = (B, h) + CORR_REST
    real = _u(8009 + 16 * seed, shape).double() + 0.5 * _u(8010 + 16 * seed, (1, h, 1, 1)).double()
    imag = rho * real + (1.0 - rho * rho) ** 0.5 * _u(8011 + 16 * seed, shape).double()
    return dict(x=torch.cat([real, imag], 1).float(), cot=_u(8012 + 16 * seed, (B, CORR_C) + CORR_REST))


# Per complex channel k (channels k and k + h of y / dx, element k of every parameter and buffer): the tensors of a ComplexBatchNorm result in
# families that share one denominator - the channel's own largest reference value of the family
CHANNEL_FAMILIES = {"y": ("y",), "dx": ("dx",), "dW": ("d/Wrr", "d/Wri", "d/Wii"), "dB": ("d/Br", "d/Bi"), "buf/RM": ("buf/RMr", "buf/RMi"),
                    "buf/RV": ("buf/RVrr", "buf/RVri", "buf/RVii")}


def channel_errors(got, ref):
    """{family: float64 [h]}: max|got - ref| / max|ref| over the family's entries of complex channel k."""
    out = {}
    for fam, keys in CHANNEL_FAMILIES.items():
        num, den = [], []
        for key in keys:
            g, r = torch.as_tensor(got[key]).double().cpu(), torch.as_tensor(ref[key]).double().cpu()
            assert g.shape == r.shape, (key, g.shape, r.shape)
            if r.dim() > 1:                                    # [B, 2h, ...] -> [h][everything of the channel]
                h = r.shape[1] // 2
                per = lambda t: torch.stack([t[:, :h], t[:, h:]], 0).transpose(0, 2).reshape(h, -1)
            else:
                per = lambda t: t.reshape(-1, 1)
            num.append((per(g) - per(r)).abs().max(1).values)
            den.append(per(r).abs().max(1).values)
        den = torch.stack(den).max(0).values
        out[fam] = torch.stack(num).max(0).values / torch.where(den > 0, den, torch.ones_like(den))
    return out


def load_corr_golden(name):
    """(float64-reference tensors rounded to float32, {family: ref32 error [h]}, seed) of a correlated case."""
    z = np.load(os.path.join(GOLDEN, f"convlayer_{name}.npz"))
    ref = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("ref/")}
    e32 = {k[len("ref32_err_ch/"):]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith("ref32_err_ch/")}
    return ref, e32, int(z["seed"])


def check_per_channel(res, ref, e32, label="", report=None):
    """check()'s rule per complex channel: every family's error of channel k within BAR * E32_k, E32_k = the largest error of the reference's own
    float32 run among the families of channel k.  report: a file that receives both sides' figures."""
    errs = channel_errors(res, ref)
    E32 = torch.stack(list(e32.values())).max(0).values
    lines = [f"{label}: per complex channel, this package's error | the reference's float32 error; bar {BAR} x the channel's largest float32 error"]
    for fam in CHANNEL_FAMILIES:
        lines.append(f"  {fam:7s} " + " ".join(f"{float(a):.2e}|{float(b):.2e}" for a, b in zip(errs[fam], e32[fam])))
    lines.append("  E32     " + " ".join(f"{float(v):.2e}" for v in E32))
    print("\n".join(lines))
    if report is not None:
        with open(report, "a") as f:
            f.write("\n".join(lines) + "\n")
    for fam, e in errs.items():
        for k in range(e.numel()):
            assert float(e[k]) <= BAR * float(E32[k]), (label, fam, "complex channel", k, float(e[k]), BAR * float(E32[k]))
    return errs


def stack_inputs(seed=SEED):
    return dict(x=_u(8005 + 16 * seed, STACK_SHAPE), cot=_u(8006 + 16 * seed, STACK_OUT))


def make_stack(ns):
    import torch.nn as nn
    enc = nn.Sequential(ns.ComplexConv2d(2, 16, (5, 2), (2, 1), (2, 1)), ns.ComplexBatchNorm(16), nn.PReLU())
    dec = ns.ComplexConvTranspose2d(16, 2, (5, 2), (2, 1), (2, 0), (1, 0))
    return nn.ModuleList([enc, dec])


def run_module(module, inp, dtype, device="cpu", forward=None):
    """y = module(x), loss = sum(y * cot), backward: {"y", "dx", "d/<parameter>", "buf/<buffer>" (after the forward)} as float64 CPU tensors.
    `module` is already filled, in its mode, of `dtype`, on `device`."""
    x = inp["x"].to(device=device, dtype=dtype).clone().requires_grad_(True)
    for p in module.parameters():
        p.grad = None
    y = forward(x) if forward is not None else module(x)
    (y * inp["cot"].to(device=device, dtype=dtype)).sum().backward()
    res = {"y": y.detach(), "dx": x.grad.detach()}
    for n, p in module.named_parameters():
        res["d/" + n] = p.grad.detach()
    for n, b in module.named_buffers():
        res["buf/" + n] = b.detach()
    return {k: v.double().cpu().clone() for k, v in res.items()}


def stack_forward(stack):
    return lambda x: stack[1](stack[0](x))


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = float(ref.abs().max())
    return float((got - ref).abs().max()) / (den if den > 0 else 1.0)


# A conv bias in front of a batch norm has an analytically zero gradient (float64: 1e-17): its error is measured against the scale of the same conv's
# weight gradient, a sum of the same kind
SCALE_KEY = {"d/0.0.real_conv.bias": "d/0.0.real_conv.weight", "d/0.0.imag_conv.bias": "d/0.0.imag_conv.weight"}


def err_of(key, got, ref, name=""):
    """max|got[key] - ref[key]| / max|ref[key]| (the stack's analytically zero tensors: over max|ref[SCALE_KEY[key]]|)."""
    if name == STACK and key in SCALE_KEY:
        return float((got[key].double().cpu() - ref[key].double()).abs().max()) / float(ref[SCALE_KEY[key]].abs().max())
    return rel_err(got[key], ref[key])


def load_golden(name):
    """({key: float64-reference tensor (stored rounded to float32; integer buffers as they are)}, {key: ref32_err}, seed) of a case."""
    z = np.load(os.path.join(GOLDEN, f"convlayer_{name}.npz"))
    ref = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("ref/")}
    e32 = {k[10:]: float(z[k]) for k in z.files if k.startswith("ref32_err/")}
    return ref, e32, int(z["seed"])


def check(res, ref, e32, label=""):
    """Every tensor of `ref` within BAR * E32 of it; returns {key: error}."""
    E32 = max(e32.values())
    errs = {}
    for k, v in ref.items():
        assert k in res, (label, k, sorted(res))
        errs[k] = err_of(k, res, ref, label)
    print(f"{label}: E32 {E32:.3e} bar {BAR * E32:.3e} worst " + ", ".join(f"{k} {e:.2e}" for k, e in sorted(errs.items(), key=lambda kv: -kv[1])[:4]))
    for k, e in errs.items():
        assert e <= BAR * E32, (label, k, e, BAR * E32)
    return errs
