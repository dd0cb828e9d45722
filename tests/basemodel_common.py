"""Shared by tests/golden/make_basemodel_golden.py, tests/test_basemodel_cpu.py, tests/test_gpu_basemodel.py and tools/basemodel_bench.py: the case
table of BaseModel on its own (tools_for_model.py:801-1185), the closed-form inputs and cotangents of a case (splitmix streams of oracle/weights.py at
the stored seed), a torch restatement `ref_*` of every function written from the formulas (the float64 CPU check and the bench's baseline), and the
fixtures' loader.

Shapes are the smallest at which the kernels of csrc/basemodel.hip can go wrong: one frame; T not a multiple of 4; more than one wave of frames;
255 / 256 / 257 frames around the scan's 256-frame chunk and 600 frames (three chunks); 33 bins = two bin ranges of the reduce grid; 6534 values per
utterance = four segments of the offline reduce; even and odd F for the sband bin F // 2 - 1; sample lengths around the number of frames."""
import os

import numpy as np
import torch

from oracle.weights import splitmix_uniform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 7                       # of seeds 1..9 the reference alone resolves every case to 2e-6 in float32 at 6..9 (the generator's rule); 7 is its best
BAR = 4.0                      # per tensor: max|got - ref64| / max|ref64| <= BAR * E32, E32 = the largest ref32_err among the case's tensors ...
E32_FLOOR = 1e-7               # ... and not less than float32's unit round-off (2^-24 = 6e-8) rounded up
CPU_BAR = 1e-9                 # float64 restatement against the float64 reference: summation order only (1e-12 for sums of 1e4 terms)
EPS = float(np.finfo(np.float32).eps)

NORMS4 = ("offline_laplace_norm", "cumulative_laplace_norm", "offline_gaussian_norm", "cumulative_layer_norm")      # kinds 0..3, [B, C, F, T]
NORMS3 = ("forgetting_norm", "sband_forgetting_norm", "hybrid_norm")                                               # kinds 4..6, [B, F, T], L
KIND = {n: i for i, n in enumerate(NORMS4 + NORMS3)}
SIGNED = ("offline_gaussian_norm", "cumulative_layer_norm")          # the others divide by a mean: strictly positive inputs

SHAPES = [(1, 2, 1), (2, 9, 7), (3, 33, 66), (2, 5, 255), (2, 5, 256), (2, 5, 257), (1, 3, 600)]      # (rows, F, T)


def _cases():
    c = {}
    for name in NORMS4:
        for rows, F, T in SHAPES:
            if name in SIGNED and (F, T) == (2, 1):
                # two values normalised by their own mean and std are +-1 / sqrt(2) whatever they are: the gradient is zero but for the eps term, the
                # reference's own float32 gradient is off by 2.7e-2 of it and the generator refuses the fixture.  Three values in one frame instead.
                F = 3
            c[f"{name}_b{rows}c1_{F}x{T}"] = (name, (rows, 1, F, T), None)
        c[f"{name}_b2c3_9x7"] = (name, (2, 3, 9, 7), None)                 # C = 3: six rows for the cumulative pair, three channels per utterance
        c[f"{name}_b1c3_33x66"] = (name, (1, 3, 33, 66), None)
    for name in NORMS3:
        for rows, F, T in SHAPES:
            c[f"{name}_{rows}x{F}x{T}_L4"] = (name, (rows, F, T), 4)
        for L in (1, 2, 6, 7, 8, 192):                                     # T - 1, T, T + 1 at T = 7; 4 is above
            c[f"{name}_2x9x7_L{L}"] = (name, (2, 9, 7), L)
        for L in (255, 256, 257):                                          # T - 1, T, T + 1 at the chunk length
            c[f"{name}_2x5x256_L{L}"] = (name, (2, 5, 256), L)
        c[f"{name}_2x5x257_L192"] = (name, (2, 5, 257), 192)               # the default sample length inside a longer utterance
        c[f"{name}_1x3x600_L192"] = (name, (1, 3, 600), 192)
    for Cc in (1, 3):
        for T in (1, 7, 68):
            for n in (0, 1, 3, 8):                                         # F = 9: n = F - 1 is the widest reflect pad torch takes
                c[f"unfold_c{Cc}_t{T}_n{n}"] = ("unfold", (2, Cc, 9, T), n)
    c["reduce_b6_f11"] = ("_reduce_complexity_separately", (6, 11, 1, 7, 5), None)
    # (appended, so that the streams of the cases above stay where they are)
    # sband at EVEN F with frames past the sample length: the only frames where it differs from forgetting_norm - the single bin F // 2 - 1 in the
    # forward, the adjoint scattered to that bin alone in the backward
    c["sband_forgetting_norm_2x4x7_L2"] = ("sband_forgetting_norm", (2, 4, 7), 2)
    c["sband_forgetting_norm_2x6x257_L4"] = ("sband_forgetting_norm", (2, 6, 257), 4)
    c["sband_forgetting_norm_3x34x66_L4"] = ("sband_forgetting_norm", (3, 34, 66), 4)      # two bin ranges, the bin in the first
    # C = 3 at the remaining shapes: for the offline pair 3 x 5 x 256 values are two segments where C = 1 gives one
    for name in NORMS4:
        for rows, F, T in ((1, 2, 1), (2, 5, 255), (2, 5, 256), (2, 5, 257), (1, 3, 600)):
            if name == "cumulative_layer_norm" and (F, T) == (2, 1):
                F = 3                                                      # rows of two values again (see above); offline_gaussian has six per utterance here
            c[f"{name}_b{rows}c3_{F}x{T}"] = (name, (rows, 3, F, T), None)
    return c


CASES = _cases()
REDUCE_FB_UNITS = 3            # the full-band input of the reduce case: [6, 11, 1, 3, 5]


def _u(idx, shape):
    return torch.from_numpy(np.ascontiguousarray(splitmix_uniform(idx, int(np.prod(shape))).reshape(shape), dtype=np.float32))


def case_index(name):
    return list(CASES).index(name)


def out_shape(name):
    fn, shape, arg = CASES[name]
    if fn == "unfold":
        B, Cc, F, T = shape
        return (B, F, Cc, 2 * max(arg, 0) + 1, T)
    if fn == "_reduce_complexity_separately":
        B, F, Cc, K, T = shape
        return (B // 3 * 3, len(range(1, F - 1, 3)), Cc, K + REDUCE_FB_UNITS, T)
    return tuple(shape)


def inputs(name, seed=SEED):
    """dict(x, cot[, x2]) float32 CPU tensors of a case: x = u in (-1, 1) for the signed norms and unfold, 0.05 + (u + 1) / 2 for the norms that divide
    by a mean (no denominator near 0); cot = u; x2 = the full-band input of the reduce case."""
    fn, shape, arg = CASES[name]
    base = 20000 + 4096 * seed + 4 * case_index(name)
    x = _u(base, shape)
    if fn in NORMS4 + NORMS3 and fn not in SIGNED:
        x = 0.05 + (x + 1) / 2
    d = dict(x=x, cot=_u(base + 1, out_shape(name)))
    if fn == "_reduce_complexity_separately":
        B, F, Cc, K, T = shape
        d["x2"] = _u(base + 2, (B, F, Cc, REDUCE_FB_UNITS, T))
    return d


def call(ns, name, x, x2=None, device=None):
    """The case's function of the BaseModel class `ns` (the reference's or this package's) on x."""
    fn, shape, arg = CASES[name]
    f = getattr(ns, fn)
    if fn == "_reduce_complexity_separately":
        return f(x, x2, device if device is not None else x.device)
    return f(x) if arg is None else f(x, arg)


def run_case(ns, name, dtype, device="cpu", inp=None):
    """y = f(x), loss = sum(y * cot), backward: {"y", "grad_x"[, "grad_x2"]} as float64 CPU tensors."""
    inp = inp if inp is not None else inputs(name)
    x = inp["x"].to(device=device, dtype=dtype).clone().requires_grad_(True)
    x2 = inp["x2"].to(device=device, dtype=dtype).clone().requires_grad_(True) if "x2" in inp else None
    y = call(ns, name, x, x2)
    (y * inp["cot"].to(device=device, dtype=dtype)).sum().backward()
    res = {"y": y.detach(), "grad_x": x.grad.detach()}
    if x2 is not None:
        res["grad_x2"] = x2.grad.detach()
    return {k: v.double().cpu().clone() for k, v in res.items()}


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = float(ref.abs().max())
    return float((got - ref).abs().max()) / (den if den > 0 else 1.0)


def load_golden(name):
    """({key: float64 reference tensor}, {key: ref32_err}, seed) of a case."""
    z = np.load(os.path.join(GOLDEN, f"basemodel_{name}.npz"))
    ref = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("ref/")}
    e32 = {k[10:]: float(z[k]) for k in z.files if k.startswith("ref32_err/")}
    return ref, e32, int(z["seed"])


def check(res, ref, e32, label=""):
    """Every tensor of `ref` within BAR * max(E32, E32_FLOOR) of it (the rule of tests/test_gpu_convlayers.py); returns {key: error}."""
    E32 = max(max(e32.values()), E32_FLOOR)
    errs = {k: rel_err(res[k], v) for k, v in ref.items()}
    print(f"{label}: E32 {E32:.3e} bar {BAR * E32:.3e} " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= BAR * E32, (label, k, e, BAR * E32)
    return errs


# ---------------------------------------------------------------------------------------------- the restatement, from the formulas
def _frame_stats(x3):
    """x3 [R, F, T] -> (S_t cumulative sum over bins and frames, Q_t the same of the squares, n_t = F (t + 1))."""
    R, F, T = x3.shape
    n = F * torch.arange(1, T + 1, dtype=x3.dtype, device=x3.device)
    return x3.sum(1).cumsum(-1), (x3 * x3).sum(1).cumsum(-1), n


def ref_offline_laplace_norm(x):
    assert x.dim() == 4
    return x / (x.mean(dim=(1, 2, 3), keepdim=True) + 1e-5)


def ref_offline_gaussian_norm(x):
    assert x.dim() == 4
    mu = x.mean(dim=(1, 2, 3), keepdim=True)
    n = x[0].numel()
    sd = (((x - mu) ** 2).sum(dim=(1, 2, 3), keepdim=True) / (n - 1)).sqrt()
    return (x - mu) / (sd + 1e-5)


def ref_cumulative_laplace_norm(x):
    assert x.dim() == 4
    B, Cc, F, T = x.shape
    x3 = x.reshape(B * Cc, F, T)
    S, _, n = _frame_stats(x3)
    return (x3 / ((S / n)[:, None, :] + EPS)).reshape(B, Cc, F, T)


def ref_cumulative_layer_norm(x):
    assert x.dim() == 4
    B, Cc, F, T = x.shape
    x3 = x.reshape(B * Cc, F, T)
    S, Q, n = _frame_stats(x3)
    mu = S / n
    sd = torch.sqrt((Q - 2 * mu * S) / n + mu * mu + EPS)
    return ((x3 - mu[:, None, :]) / sd[:, None, :]).reshape(B, Cc, F, T)


def _forgetting_mean(x, L, new_term, last):
    """mu_t = a_t mu_{t-1} + (1 - a_t) new_term(t) for t < last, mu_{-1} = 0: a_t = float32(min((t - 1) / (t + 1), alpha)) and 1 - a_t in float32 for
    the warm-up frames t < L, alpha = (L - 1) / (L + 1) in double afterwards.  Returns [B, last]."""
    alpha = (L - 1) / (L + 1)
    mu = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    out = []
    for t in range(last):
        if t < L:
            a32 = np.float32(min((t - 1) / (t + 1), alpha))
            a, om = float(a32), float(np.float32(1) - a32)
        else:
            a, om = alpha, 1 - alpha
        mu = a * mu + om * new_term(t)
        out.append(mu)
    return torch.stack(out, dim=-1) if out else x.new_zeros((x.shape[0], 0))


def ref_forgetting_norm(x, L):
    assert x.dim() == 3
    mu = _forgetting_mean(x, L, lambda t: x[:, :, t].mean(1), x.shape[-1])
    return x / (mu[:, None, :] + 1e-10)


def ref_sband_forgetting_norm(x, L):
    assert x.dim() == 3
    F = x.shape[1]
    mu = _forgetting_mean(x, L, lambda t: x[:, :, t].mean(1) if t < L else x[:, F // 2 - 1, t], x.shape[-1])
    return x / (mu[:, None, :] + 1e-10)


def ref_hybrid_norm(x, L=192):
    assert x.dim() == 3
    T = x.shape[-1]
    S, _, n = _frame_stats(x)
    warm = _forgetting_mean(x, L, lambda t: x[:, :, t].mean(1), min(L, T))
    mu = torch.cat([warm, (S / n)[:, L:]], dim=-1)
    return x / (mu[:, None, :] + 1e-10)


def ref_unfold(x, n):
    assert x.dim() == 4
    B, Cc, F, T = x.shape
    n = max(int(n), 0)
    if n >= F:
        raise RuntimeError("reflect padding needs n < F")
    p = torch.arange(F, device=x.device)[:, None] - n + torch.arange(2 * n + 1, device=x.device)[None, :]      # [F, K] un-reflected positions
    p = torch.where(p < 0, -p, torch.where(p >= F, 2 * (F - 1) - p, p))
    return x[:, :, p, :].permute(0, 2, 1, 3, 4)                        # [B, C, F, K, T] -> [B, F, C, K, T]


def ref__reduce_complexity_separately(sub_band_input, full_band_output, device=None):
    B, F = full_band_output.shape[:2]
    sub = B // 3
    parts = []
    for i in range(3):
        rows = slice(i * sub, (i + 1) * sub)
        bins = slice(i + 1, F - 1, 3)
        parts.append(torch.cat([sub_band_input[rows, bins], full_band_output[rows, bins]], dim=-2))
    return torch.cat(parts, dim=0)


class Ref:
    """The restatement under the names of BaseModel's members (so that `call` / `run_case` take it like a class)."""
    offline_laplace_norm = staticmethod(ref_offline_laplace_norm)
    offline_gaussian_norm = staticmethod(ref_offline_gaussian_norm)
    cumulative_laplace_norm = staticmethod(ref_cumulative_laplace_norm)
    cumulative_layer_norm = staticmethod(ref_cumulative_layer_norm)
    forgetting_norm = staticmethod(ref_forgetting_norm)
    sband_forgetting_norm = staticmethod(ref_sband_forgetting_norm)
    hybrid_norm = staticmethod(ref_hybrid_norm)
    unfold = staticmethod(ref_unfold)
    _reduce_complexity_separately = staticmethod(ref__reduce_complexity_separately)
