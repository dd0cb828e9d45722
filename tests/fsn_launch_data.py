"""Per-launch float64 references for FullSubNet's glue launches (a plain module, not a conftest): the cases, the descriptor mirror, the planted
states, the references and the comparator shared by test_fsn_launches_cpu.py (the host simulator as the device, the data conditions, the edges, the
coverage by name, the closed forms against autograd, planted faults) and test_gpu_fsn_launches.py (the device).

The struct-Fsn launches of csrc/fsn.hip - FSN_IN, FSN_SCALE, FSN_SBSUM, FSN_SBBUILD, FSN_NORMSTAT, FSN_ACT, FSN_OUT, FSN_OUT_BWD, FSN_SBBWD_SUM,
FSN_SBBWD_APPLY (plain and LDS gather), FSN_NORMBWD - each run ALONE (plan.run(phase, arenas, 0, i, i + 1)) from a state planted straight into the
buffers the descriptor names: no GEMM, no recurrence.  The arenas' background is the byte 0x55 (1.5e13 as fp32 or bf16, so a read outside the planted
inputs shows too) and every byte outside a launch's documented outputs is a stray byte.  Outputs include the partial `sums` rows, the finalised
means in `aux2`, and the pad columns W .. WP - 1 of sb_in and F .. FP - 1 of fb_in / d_fb, which must be zero BYTES.  fbo's pad columns are inputs,
planted as zeros, and must still be zero behind FSN_ACT.  The pad columns of d_sb_in are documented as unused: they are left as background.

The expectation is float64 torch written from the reference model's definition of the operation - BaseModel.unfold as F.pad(mode="reflect") +
F.unfold (ref_unfold), the four norms as BaseModel states them with the look-ahead frames counted as data (ref_norm, ref_utt_stats,
ref_cum_stats), the activations as SequenceModel applies them - neither the kernels nor the host simulator have a part in it.

Backward launches: closed forms in float64 over the inputs AS STORED (the planted fp32 statistics, the planted sb_in in the plan's dtype).  With
L = sum g y over a normalised row set, g = d_sb_in, y = sb_in, x the un-normalised value, N / n_t the number of values behind a statistic:
  offline_laplace     y = x / (mu + e), mu = sum x / N:  dL/dx_i = g_i / (mu + e) - sum_k g_k x_k / ((mu + e)^2 N) = (g_i - S / N) / (mu + e),
                      S = sum g y.  FSN_SBBWD_SUM stores S / N, FSN_SBBWD_APPLY applies it.
  offline_gaussian    y = (x - mu) / (sd + e), sd^2 = sum (x - mu)^2 / (N - 1), d sd / dx_i = (x_i - mu) / ((N - 1) sd):
                      dL/dx_i = (g_i - G / N) / (sd + e) - sum_k g_k (x_k - mu) / (sd + e)^2 * d sd / dx_i
                              = (g_i - G / N) / (sd + e) - y_i S / ((N - 1) sd),   G = sum g   (the mean's own term through sd vanishes: sum (x - mu) = 0)
  cumulative_laplace  y_t = x_t / (m_t + E), m_t = sum_{u <= t} x_u / n_t: frame t feeds every m_u, u >= t:
                      dL/dx_t = g_t / (m_t + E) - sum_{u >= t} S_u / ((m_u + E) n_u),   S_u = sum_k g y at frame u
  cumulative_layer    y_t = (x_t - m_t) / sd_t, sd_t^2 = Q_t / n_t - m_t^2 + E, d sd_u / dx_t = (x_t - m_u) / (n_u sd_u) (u >= t):
                      dL/dx_t = g_t / sd_t - sum_{u >= t} [ G_u / (n_u sd_u) + (x_t - m_u) S_u / (n_u sd_u^2) ]
(normbwd_closed; test_fsn_launches_cpu.py pins each against torch autograd in float64 through ref_norm(ref_sb_raw(..)) on an unrounded,
self-consistent state at 1e-12).  The column -> bin gather of fb_num_neighbors > 0 is the vector-Jacobian product of ref_unfold itself
(ref_gather): autograd through F.pad(mode="reflect") + F.unfold, not a restatement of the kernel's mirrored sources.

The kernels are compiled with FMA contraction, so the data is DYADIC where the launch allows: magnitudes and gradients are small integers, fbo small
integers with planted zeros and sixes (eighths inside (-1, 1) behind a Tanh head), sb_in quarters.  conditions() measures on the float64 reference
alone that every byte-equal value is its own fp32 rounding and that sum|terms| / (largest power of two dividing all terms) < 2^24 for every
float-accumulated sum (the `sums` of FSN_IN, FSN_SBSUM and FSN_SBBWD_SUM, the gather's s).

Bars by launch:
  byte equality   FSN_IN mag_t (the zeros at t >= T too) and the `sums` rows of FSN_IN / FSN_SBSUM / FSN_SBBWD_SUM; FSN_OUT and FSN_OUT_BWD with
                  none / ReLU / ReLU6 (zeros at t < LA; the derivative at exactly 0 and exactly 6 is 0); FSN_ACT with ReLU6; FSN_SBBWD_APPLY and the
                  gather behind FSN_NORMBWD (mode != 0) with none / ReLU / ReLU6; the partial (S, G) rows of the gaussian FSN_NORMBWD; every pad column;
  means           aux2 (a double sum, one division, one cast): 1 fp32 ulp;
  FSN_NORMSTAT    mean 1 ulp, std 2 ulps, the unused std slot of cumulative_laplace an exact 0;
  rounding count  FSN_SCALE, FSN_SBBUILD, FSN_SBBWD_APPLY and the gather in mode 0: N_ROUNDINGS_* x 2^-24 x sum|terms| per element, + half a bf16 ulp of
                  the expected value in bf16;
  FSN_NORMBWD     double arithmetic on stored inputs and one cast: 2^-24 x sum|terms| of the closed form per element;
  Tanh            the device's tanhf is measured against float64 on the planted pre-activations, in fp32 ulps of the exact value, and held to
                  TANHF_BAR_ULPS; the 1 - y^2 factor of FSN_OUT_BWD gets that (2 |y| per ulp of y) and its rounding count on top.  The ROCm
                  installation documents no bound for tanhf (no statement in its device-library, HIP or compiler documents), so the bar is twice the
                  worst value MEASURED on an MI355X: 0.929 ulps (the same figure in FSN_ACT and FSN_OUT, fp32 and bf16 plans), on 2026-10-21, over
                  the planted pre-activations of every Tanh case here - the 513 multiples of 1 / 64 in -4 .. 4."""
import ctypes as C
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as Fn

from norm_data import BF16, CHECKED, F32, IO, WS, OP_HEADER, Bench, Planted, Ptr, _esize, _ordered, _store, _tdtype, _u8, bf16_ulp, buffer_at, f32_ulp
from simutil import PHASE_BWD, PHASE_FWD, Plan

# sefd_desc.h OpKind
FSN_IN, FSN_SCALE, FSN_SBSUM, FSN_SBBUILD, FSN_OUT, FSN_OUT_BWD, FSN_SBBWD_SUM, FSN_SBBWD_APPLY = 27, 28, 29, 30, 31, 32, 33, 34
FSN_NORMSTAT, FSN_NORMBWD, FSN_ACT = 40, 41, 48
KIND_NAMES = {FSN_IN: "FSN_IN", FSN_SCALE: "FSN_SCALE", FSN_SBSUM: "FSN_SBSUM", FSN_SBBUILD: "FSN_SBBUILD", FSN_OUT: "FSN_OUT", FSN_OUT_BWD: "FSN_OUT_BWD",
              FSN_SBBWD_SUM: "FSN_SBBWD_SUM", FSN_SBBWD_APPLY: "FSN_SBBWD_APPLY", FSN_NORMSTAT: "FSN_NORMSTAT", FSN_NORMBWD: "FSN_NORMBWD",
              FSN_ACT: "FSN_ACT"}
RERUN = (FSN_NORMSTAT, FSN_SBSUM, FSN_SBBWD_SUM)                  # run twice from the same planted input: the same bytes
ACT_NONE, ACT_RELU, ACT_TANH, ACT_RELU6 = 0, 1, 2, 3
ACTS = {None: 0, "ReLU": 1, "Tanh": 2, "ReLU6": 3}
NORMS = {"offline_laplace_norm": 0, "cumulative_laplace_norm": 1, "offline_gaussian_norm": 2, "cumulative_layer_norm": 3}
EPSILON = float(np.finfo(np.float32).eps)                        # tools_for_model.py EPSILON: the cumulative norms
LIMIT = 1 << 24
# fp32 roundings on the longest path of fsn_scale_kernel / the element path of fsn_sbbuild_kernel (offline_gaussian): x - mean [1], std + 1e-5f [2],
# the quotient [3]; + 1 for the second order as norm_data.N_ROUNDINGS has it.  (The 16-byte paths of fsn_sbbuild_kernel: den [1], x / den [2].)
N_ROUNDINGS_NORM = 4
# ... of fsn_sbbwd_gather_kernel in mode 0 with a Tanh head: den = mu + 1e-5f [1], s / den [2], (float)cnt * Sm [3], / den [4], the difference [5],
# y * y [6], 1 - . [7], v * . [8] (the sum s itself is exact on integer data); fsn_sbbwd_apply_kernel has the same chain without [3]
N_ROUNDINGS_APPLY = 8
# ... of head_act_grad with Tanh (FSN_OUT_BWD): y * y [1], 1 - . [2], g * . [3], + 1 for the second order
N_ROUNDINGS_ACTGRAD = 4
TANHF_MEASURED_ULPS = 0.93                                        # worst |tanhf(x) - tanh(x)| / ulp32(tanh(x)) on the device (see the docstring)
TANHF_BAR_ULPS = 2 * TANHF_MEASURED_ULPS
BG32 = float(torch.tensor([0x55555555], dtype=torch.int32).view(torch.float32))   # the background as an fp32 value


class Fsn(C.Structure):                                           # sefd_desc.h Fsn
    _fields_ = [("in_", Ptr), ("out", Ptr), ("aux", Ptr), ("aux2", Ptr), ("sums", Ptr), ("B", C.c_int32), ("F", C.c_int32), ("T", C.c_int32),
                ("TP", C.c_int32), ("FP", C.c_int32), ("NB", C.c_int32), ("LA", C.c_int32), ("dt", C.c_int32), ("act", C.c_int32), ("mode", C.c_int32),
                ("stat", Ptr), ("src", C.c_int32), ("ext", C.c_int32)]


PTRS = ("in_", "out", "aux", "aux2", "sums", "stat")


# sefd_desc.h fsn_nfb / fsn_w / fsn_wp / fsn_sbact
def fsn_nfb(d):
    return (d.ext & 0xff) + 1


def fsn_w(d):
    return d.NB + fsn_nfb(d)


def fsn_wp(d):
    return (fsn_w(d) + 7) & ~7


def fsn_sbact(d):
    return (d.ext >> 8) & 3


Launch = namedtuple("Launch", "phase op kind tag d")
Geom = namedtuple("Geom", "B F T TP FP NB LA NFB W WP nsb nfb")


def geom(d):
    return Geom(d.B, d.F, d.T, d.TP, d.FP, d.NB, d.LA, fsn_nfb(d), fsn_w(d), fsn_wp(d), (d.NB - 1) // 2, fsn_nfb(d) >> 1)


# ------------------------------------------------------------------------------------------------ cases
Case = namedtuple("Case", "name B T LA fft sb fb norm fb_act sb_act dtype")
_TABLE = [
    ("w12", 2, 5, 2, 64, 2, 3, "offline_laplace_norm", "Tanh", "ReLU6", ("fp32", "bf16")),
    ("w66", 3, 6, 2, 70, 31, 1, "cumulative_layer_norm", "ReLU6", "Tanh", ("fp32", "bf16")),
    ("w126", 1, 3, 0, 78, 31, 31, "cumulative_laplace_norm", None, "ReLU", ("fp32", "bf16")),
    ("w2", 2, 1, 1, 64, 0, 0, "offline_gaussian_norm", "ReLU", None, ("bf16",)),
    ("gauss_fb2", 2, 4, 3, 64, 3, 2, "offline_gaussian_norm", "Tanh", None, ("fp32", "bf16")),
    ("w32", 2, 5, 2, 64, 15, 0, "offline_laplace_norm", "ReLU", None, ("bf16",)),          # W == WP, NFB == 1: the fast path of fsn_sbbuild_kernel
    ("f257", 1, 2, 2, 512, 1, 2, "offline_laplace_norm", "ReLU", None, ("bf16",)),         # F beyond one 256-thread pass of the gather
    ("cumlap_fb1", 2, 5, 2, 64, 2, 1, "cumulative_laplace_norm", "ReLU", "ReLU6", ("bf16",)),
]
CASES = [Case(f"{r[0]}_{dt}", *r[1:10], dt) for r in _TABLE for dt in r[10]]
BY_NAME = {c.name: c for c in CASES}


def case_id(c):
    return c.name


_plans = {}


def plan_of(case):
    """The plan of `case`, built once per process: hidden sizes 16 / 8, dropout keep 1 (the GEMMs and cells never run here)."""
    if case.name not in _plans:
        fsn = dict(sb_num_neighbors=case.sb, fb_num_neighbors=case.fb, look_ahead=case.LA, fb_hidden=16, sb_hidden=8, fb_act=case.fb_act,
                   sb_act=case.sb_act, keep=1.0, norm_type=case.norm)
        _plans[case.name] = Plan(case.B, case.T, model="FullSubNet", fft_len=case.fft, fsn=fsn, act_dtype=case.dtype, training=True)
    return _plans[case.name]


def expected_buffers(d, kind):
    """{pointer field: (buffer name, bytes)} of a struct-Fsn launch, from its kind and dimensions; every other pointer must be A_NONE."""
    q, es, m = geom(d), _esize(d.dt), d.mode
    f4 = lambda *n: (int(np.prod(n)) * 4)
    mag_t, fbo = ("mag_t", f4(q.TP, q.B, q.F)), ("fbo", f4(q.TP, q.B, q.FP))
    sb_in, d_sbin = ("sb_in", q.TP * q.B * q.F * q.WP * es), ("d_sbin", f4(q.TP, q.B, q.F, q.WP))
    st_fb = ("stat_fb", f4(2, q.B) if m == 2 else f4(q.TP, q.B, 2))
    st_sb = ("stat_sb", f4(2, q.B) if m == 2 else f4(q.TP, q.B, q.F, 2))
    mu_sb, sbo = ("mu_sb", f4(q.B)), ("sbo", f4(q.TP, q.B, q.F, 2))
    d_fb = ("d_fb", q.TP * q.B * q.FP * es)
    if kind == FSN_IN:
        return dict(in_=("io.mag", f4(q.B, q.F, q.T)), out=mag_t, sums=("sum_fb", f4(q.B, q.F)), aux2=("mu_fb", f4(q.B)))
    if kind == FSN_SCALE:
        return dict(in_=mag_t, out=("fb_in", q.TP * q.B * q.FP * es), sums=("mu_fb", f4(q.B)), **(dict(stat=st_fb) if m else {}))
    if kind == FSN_NORMSTAT:
        return dict(in_=mag_t, aux=fbo, stat=st_sb) if d.src else dict(in_=mag_t, stat=st_fb)
    if kind == FSN_ACT:
        return dict(out=fbo)
    if kind == FSN_SBSUM:
        return dict(in_=mag_t, aux=fbo, sums=("sum_sb", f4(q.B, q.F)), aux2=mu_sb)
    if kind == FSN_SBBUILD:
        return dict(in_=mag_t, aux=fbo, sums=mu_sb, out=sb_in, **(dict(stat=st_sb) if m else {}))
    if kind == FSN_OUT:
        return dict(in_=sbo, out=("io.crm", f4(q.B, q.F, q.T, 2)))
    if kind == FSN_OUT_BWD:
        return dict(in_=("io.grad_crm", f4(q.B, q.F, q.T, 2)), out=("d_sbo", q.TP * q.B * q.F * 2 * es), **(dict(aux=sbo) if fsn_sbact(d) else {}))
    if kind == FSN_SBBWD_SUM:
        return dict(in_=d_sbin, aux=sb_in, sums=("sum_S", f4(q.B, q.F)), aux2=("Sm", f4(q.B)))
    if kind == FSN_NORMBWD:
        return dict(in_=d_sbin, aux=fbo, aux2=sb_in, stat=st_sb, sums=("normbwd_part", f4(2, q.B, q.F)), out=("d_fb_pre", f4(q.TP, q.B, q.F, q.NFB)))
    assert kind == FSN_SBBWD_APPLY
    return dict(in_=d_sbin if m == 0 else ("d_fb_pre", f4(q.TP, q.B, q.F, q.NFB)), aux=fbo, aux2=mu_sb, sums=("Sm", f4(q.B)), out=d_fb)


def check_mirror(plan, ln):
    """A moved struct layout fails here: the op header against op_info's kind and tag, the dimensions against the plan's, every pointer against the
    named buffer it must be the start of, and that buffer's size against TP * B * F * WP * elementsize and the like."""
    o = plan.op_info(ln.phase, ln.op)
    assert (o["kind"], o["tag"]) == (ln.kind, ln.tag)
    d = ln.d
    nsb, nfb, la, _, _, actf, acts, _, _, norm = [int(v) for v in plan.cfg.kernel_num[:10]]    # csrc/plan_fsn.cpp: the knobs as the planner reads them
    assert (d.B, d.F, d.T, d.LA) == (plan.B, plan.NF, plan.L, la), "Fsn layout moved: B / F / T / LA"
    assert (d.TP, d.FP, d.NB) == (d.T + d.LA, (d.F + 7) // 8 * 8, 2 * nsb + 1), "Fsn layout moved: TP / FP / NB"
    assert d.dt == plan.cfg.act_dtype and d.act == actf and d.mode in (0, norm), "Fsn layout moved: dt / act / mode"
    assert d.src in (0, 1) and d.ext == (2 * nfb) | (acts << 8), "Fsn layout moved: src / ext"
    want = expected_buffers(d, ln.kind)
    for name in PTRS:
        p = getattr(d, name)
        if name not in want:
            assert p.arena == -1, (KIND_NAMES[ln.kind], name, "should be A_NONE")
            continue
        bname, _, off, nb, _ = buffer_at(plan, p)
        assert (bname, nb) == want[name] and p.off == off, (KIND_NAMES[ln.kind], name, bname, nb, want[name])


def launches(plan):
    """The struct-Fsn launches of both phases, in order, each with a copy of its descriptor (checked: check_mirror)."""
    out, sz = [], plan.lib.sefd_op_size()
    for phase in (PHASE_FWD, PHASE_BWD):
        for i in range(plan.num_ops(phase)):
            ptr = plan.ops_ptr(phase) + i * sz
            kind, tag = (C.c_int32 * 2).from_buffer_copy(C.string_at(ptr, 8))
            if kind in KIND_NAMES:
                ln = Launch(phase, i, kind, tag, Fsn.from_buffer_copy(C.string_at(ptr + OP_HEADER, C.sizeof(Fsn))))
                check_mirror(plan, ln)
                out.append(ln)
    return out


def sbbuild_path(d):
    """The path of fsn_sbbuild_kernel that descriptor `d` takes (its two `if`s restated)."""
    W, WP = fsn_w(d), fsn_wp(d)
    if d.mode == 0 and d.dt == BF16 and d.TP * d.B * d.F * (WP // 8) < 1 << 31 and not (W == WP and fsn_nfb(d) == 1):
        return "fsn_sbbuild_kernel 16-byte chunks, any width"
    if d.mode == 0 and d.dt == BF16 and W == WP and d.TP * d.B * d.F * (W // 8) < 1 << 31:
        return "fsn_sbbuild_kernel 16-byte chunks, W == WP and NFB == 1"
    return "fsn_sbbuild_kernel by element"


ALL_ARMS = ("fsn_in_kernel", "fsn_mean_kernel", "fsn_scale_kernel", "fsn_sbsum_kernel", "fsn_sbbuild_kernel 16-byte chunks, any width",
            "fsn_sbbuild_kernel 16-byte chunks, W == WP and NFB == 1", "fsn_sbbuild_kernel by element", "fsn_out_kernel", "fsn_out_bwd_kernel",
            "fsn_act_kernel", "fsn_sbbwd_sum_kernel", "fsn_normstat_utt_kernel", "fsn_normstat_cum_kernel 64 threads (src 1)",
            "fsn_normstat_cum_kernel 256 threads (src 0)", "fsn_normbwd_utt_part_kernel + fsn_normbwd_utt_kernel", "fsn_normbwd_cum_kernel",
            "fsn_normbwd_cum_kernel second lane pass (k + 64 < W)", "fsn_sbbwd_apply_kernel", "fsn_sbbwd_gather_kernel")


def arms(ln):
    """The kernels and paths launch_fsn picks for launch `ln`: its `if`s (mode == 2, src, nfb > 1) and the in-kernel paths, restated."""
    d, k = ln.d, ln.kind
    if k == FSN_IN:
        return ["fsn_in_kernel", "fsn_mean_kernel"]
    if k == FSN_SBSUM:
        return ["fsn_sbsum_kernel", "fsn_mean_kernel"]
    if k == FSN_SBBWD_SUM:
        return ["fsn_sbbwd_sum_kernel", "fsn_mean_kernel"]
    if k == FSN_SBBUILD:
        return [sbbuild_path(d)]
    if k == FSN_NORMSTAT:
        return ["fsn_normstat_utt_kernel" if d.mode == 2 else "fsn_normstat_cum_kernel 64 threads (src 1)" if d.src else "fsn_normstat_cum_kernel 256 threads (src 0)"]
    if k == FSN_NORMBWD:
        if d.mode == 2:
            return ["fsn_normbwd_utt_part_kernel + fsn_normbwd_utt_kernel"]
        return ["fsn_normbwd_cum_kernel"] + (["fsn_normbwd_cum_kernel second lane pass (k + 64 < W)"] if fsn_w(d) > 64 else [])
    if k == FSN_SBBWD_APPLY:
        return ["fsn_sbbwd_gather_kernel" if fsn_nfb(d) > 1 else "fsn_sbbwd_apply_kernel"]
    return [{FSN_SCALE: "fsn_scale_kernel", FSN_OUT: "fsn_out_kernel", FSN_OUT_BWD: "fsn_out_bwd_kernel", FSN_ACT: "fsn_act_kernel"}[k]]


# ------------------------------------------------------------------------------------------------ references (float64, the reference model's definitions)
def ref_unfold(x, n, mode="reflect"):
    """BaseModel.unfold (tools_for_model.py:806-837): x [B, C, F, T] -> [B, F, C, 2 n + 1, T].  mode "constant": the same windows over a ZERO padded
    spectrum - what reaches a bin without any mirrored source (the edge assertions' yardstick only); "low": see below."""
    B, Cc, F, T = x.shape
    if n < 1:
        return x.permute(0, 2, 1, 3).reshape(B, F, Cc, 1, T)
    out = x.reshape(B * Cc, 1, F, T)
    if mode == "low":                                            # mirrored at the lower edge only (a planted fault's yardstick)
        out = Fn.pad(Fn.pad(out, [0, 0, n, 0], mode="reflect"), [0, 0, 0, n])
    else:
        out = Fn.pad(out, [0, 0, n, n], mode=mode)
    out = Fn.unfold(out, (2 * n + 1, T))
    assert out.shape[-1] == F
    return out.reshape(B, Cc, 2 * n + 1, T, F).permute(0, 4, 1, 2, 3).contiguous()


def to_ref(x):
    """Time-major [TP][B][F] -> the reference's [B, 1, F, TP]."""
    return x.permute(1, 2, 0).unsqueeze(1)


def ref_sb_raw(mag, fbo, nsb, nfb, mode="reflect"):
    """The un-normalised sub-band input (models.py:647-660): mag, fbo [B, 1, F, TP] -> [B, F, W, TP]."""
    B, _, F, TP = mag.shape
    fu = ref_unfold(fbo, nfb, mode).reshape(B, F, 2 * nfb + 1, TP)
    mu = ref_unfold(mag, nsb, mode).reshape(B, F, 2 * nsb + 1, TP)
    return torch.cat([mu, fu], 2)


def tm(x):
    """The reference's [B, F, W, TP] -> the kernels' time-major [TP][B][F][W]."""
    return x.permute(3, 0, 1, 2).contiguous()


def ref_utt_stats(x):
    """(mean, unbiased std) [B] of offline_gaussian_norm (tools_for_model.py:1047-1061); x [B, C, F, T]."""
    return torch.mean(x, dim=(1, 2, 3)), torch.std(x, dim=(1, 2, 3))


def ref_cum_stats(x):
    """(cumulative mean, cumulative std) [B * C, T] as cumulative_layer_norm forms them (tools_for_model.py:1064-1104); x [B, C, F, T]."""
    b, c, f, t = x.shape
    xi = x.reshape(b * c, f, t)
    cs, cq = torch.cumsum(torch.sum(xi, dim=1), dim=-1), torch.cumsum(torch.sum(torch.square(xi), dim=1), dim=-1)
    n = torch.arange(f, f * t + 1, f, dtype=x.dtype).reshape(1, t)
    mean = cs / n
    var = (cq - 2 * mean * cs) / n + mean.pow(2)
    return mean, torch.sqrt(var + EPSILON)


def ref_norm(x, mode):
    """BaseModel's four norms on x [B, C, F, T] (tools_for_model.py:997-1104), by Fsn::mode."""
    if mode == 0:
        return x / (torch.mean(x, dim=(1, 2, 3), keepdim=True) + 1e-5)
    if mode == 2:
        return (x - torch.mean(x, dim=(1, 2, 3), keepdim=True)) / (torch.std(x, dim=(1, 2, 3), keepdim=True) + 1e-5)
    b, c, f, t = x.shape
    mean, sd = ref_cum_stats(x)
    xi = x.reshape(b * c, f, t)
    out = xi / (mean.reshape(b * c, 1, t) + EPSILON) if mode == 1 else (xi - mean.reshape(b * c, 1, t)) / sd.reshape(b * c, 1, t)
    return out.reshape(b, c, f, t)


def norm_stored(x, mode, mu=None, stat=None):
    """(value, sum|terms|): x [TP][B][..] through norm `mode` with the statistics AS STORED - mode 0: mu [B]; 2: stat = (mean, std) [B]; 1 / 3:
    stat = (mean, std) shaped like x without its last dimension."""
    ex = lambda v: v.reshape(v.shape + (1,) * (x.dim() - v.dim()))
    if mode == 0:
        den = ex(mu.reshape(1, -1)) + 1e-5
        return x / den, x.abs() / den
    if mode == 2:
        m, den = ex(stat[0].reshape(1, -1)), ex(stat[1].reshape(1, -1)) + 1e-5
        return (x - m) / den, (x.abs() + m.abs()) / den
    m, sd = ex(stat[0]), ex(stat[1])
    if mode == 1:
        return x / (m + EPSILON), x.abs() / (m + EPSILON)
    return (x - m) / sd, (x.abs() + m.abs()) / sd


def act_fwd(act, x):
    """SequenceModel's output activation (tools_for_model.py:766-775)."""
    return {0: lambda v: v, 1: torch.relu, 2: torch.tanh, 3: Fn.relu6}[act](x)


def act_grad_pre(act, x, open6=False):
    """The activation's derivative at the pre-activation x: 0 at the kinks themselves (open6: the WRONG ReLU6 derivative that is 1 at exactly 6)."""
    if act == 1:
        return (x > 0).double()
    if act == 2:
        return 1 - torch.tanh(x) ** 2
    if act == 3:
        return ((x > 0) & ((x <= 6) if open6 else (x < 6))).double()
    return torch.ones_like(x)


def act_grad_out(act, y):
    """The same from the activation's output y."""
    if act == 2:
        return 1 - y * y
    return act_grad_pre(act, y)


def ref_gather(cols, nfb, mode="reflect"):
    """Columns [TP][B][F][NFB] of the unfolded full-band output -> bins [TP][B][F]: the vector-Jacobian product of ref_unfold."""
    TP, B, F, NFB = cols.shape
    x = torch.zeros(B, 1, F, TP, dtype=torch.float64, requires_grad=True)
    u = ref_unfold(x, nfb, mode).reshape(B, F, NFB, TP)
    (gx,) = torch.autograd.grad(u, x, cols.permute(1, 2, 3, 0).contiguous())
    return gx[:, 0].permute(2, 0, 1).contiguous()


def normbwd_closed(mode, q, g, y, xfb, stat, start=0):
    """(dx, sum|terms|, S, G): the closed forms of the module docstring.  g, y [TP][B][F][W] (d_sb_in, sb_in as stored), xfb [TP][B][F][NFB] the raw
    full-band columns (mode 3), stat as norm_stored takes it -> dx [TP][B][F][NFB].  start = 1: the WRONG suffix sum that begins at frame t + 1."""
    gk, yk = g[..., q.NB:], y[..., q.NB:]
    if mode == 2:
        N = q.TP * q.F * q.W
        sd = stat[1].reshape(1, -1, 1, 1)
        Gf, Sf = g.sum((0, 3)), (g * y).sum((0, 3))                # [B][F]: the partial rows of the launch
        G, S = Gf.sum(1).reshape(1, -1, 1, 1), Sf.sum(1).reshape(1, -1, 1, 1)
        Ga, Sa = g.abs().sum((0, 2, 3)).reshape(1, -1, 1, 1), (g * y).abs().sum((0, 2, 3)).reshape(1, -1, 1, 1)
        dx = (gk - G / N) / (sd + 1e-5) - yk * S / ((N - 1) * sd)
        return dx, (gk.abs() + Ga / N) / (sd + 1e-5) + yk.abs() * Sa / ((N - 1) * sd), Sf, Gf
    suffix = lambda a: (a.flip(0).cumsum(0).flip(0) - (a if start else 0))
    m, sd = stat
    n = (q.W * torch.arange(1, q.TP + 1, dtype=torch.float64)).reshape(-1, 1, 1)
    G, S, Ga, Sa = g.sum(-1), (g * y).sum(-1), g.abs().sum(-1), (g * y).abs().sum(-1)
    if mode == 1:
        den = m + EPSILON
        dx = gk / den[..., None] - suffix(S / (den * n))[..., None]
        return dx, gk.abs() / den[..., None] + suffix(Sa / (den * n))[..., None], None, None
    bb, ba = S / (n * sd * sd), Sa / (n * sd * sd)
    dx = gk / sd[..., None] - suffix(G / (n * sd))[..., None] - xfb * suffix(bb)[..., None] + suffix(bb * m)[..., None]
    ab = gk.abs() / sd[..., None] + suffix(Ga / (n * sd))[..., None] + xfb.abs() * suffix(ba)[..., None] + suffix(ba * m.abs())[..., None]
    return dx, ab, None, None


def apply_closed(q, mode, act, cols, fbo, mu=None, Sm=None, cnt_off=0, drop_high=False):
    """(d_fb [TP][B][F], sum|terms|, mirrored share): FSN_SBBWD_APPLY over the columns [TP][B][F][NFB] (mode 0: of d_sb_in; else FSN_NORMBWD's output).
    mode 0:  sum over the sources of (g - S / N) / (mu + 1e-5)  (the docstring's offline_laplace form, once per source).
    cnt_off / drop_high: the planted faults (the source count of bin 0 off by one; the sources mirrored at the upper edge dropped)."""
    s, sa = ref_gather(cols, q.nfb), ref_gather(cols.abs(), q.nfb)
    mirrored = s - ref_gather(cols, q.nfb, "constant")
    if drop_high:
        s = ref_gather(cols, q.nfb, "low")
    if mode == 0:
        cnt = ref_gather(torch.ones_like(cols), q.nfb)
        cnt[:, :, 0] += cnt_off
        den = mu.reshape(1, -1, 1) + 1e-5
        v, ab = (s - cnt * Sm.reshape(1, -1, 1)) / den, (sa + cnt * Sm.abs().reshape(1, -1, 1)) / den
    else:
        v, ab = s, sa
    dy = act_grad_out(act, fbo[..., :q.F])
    return v * dy + 0.0, ab * (1 + fbo[..., :q.F] ** 2 if act == 2 else dy.abs()), mirrored           # (+ 0.0: no negative zero)


# ------------------------------------------------------------------------------------------------ planted data
# One output of a launch: n elements of dtype code dt from byte `off` of `arena` on, C per row.  exp float64 [n].  tol None: ulps (an int, or an int
# tensor [n]) fp32 ulps from exp rounded to fp32, 0 = byte equality with exp rounded to dt (fp32: exp must be exact).  tol float64 [n]:
# |device - exp| <= tol, and where tol == 0 byte equality (the pad columns: zero BYTES).  meas: a tanhf measurement - tol is TANHF_BAR_ULPS fp32
# ulps of the exact value, the worst error in ulps is reported.
Field = namedtuple("Field", "name arena off dt C exp tol ulps meas", defaults=(None, 0, False))


def _gen(case, ln):
    return torch.Generator().manual_seed(zlib.crc32(f"fsn:{case.name}:{ln.phase}:{ln.op}".encode()))


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def gen_mag_t(g, q, mode):
    """mag_t [TP][B][F]: integers 0 .. 7, the look-ahead frames zero as F.pad makes them; cumulative_layer_norm: frame 0 of the last utterance constant
    (its running variance is 0 there: the + EPSILON under the root shows)."""
    m = _ints(g, 0, 7, q.TP, q.B, q.F)
    m[q.T:] = 0
    if mode == 3:
        m[0, q.B - 1] = 3
    return m


def gen_fbo(g, q, act, mode, pre=False):
    """fbo [TP][B][FP], pad columns zero.  The full-band head's OUTPUT (pre = False): integers of the activation's range (none -2 .. 8, ReLU 0 .. 8,
    ReLU6 0 .. 6) with planted zeros and sixes, eighths inside (-1, 1) behind Tanh; its PRE-activation (FSN_ACT): integers -2 .. 8 with zeros and
    sixes for ReLU6, multiples of 1 / 64 in -4 .. 4 for Tanh (513 values: the tanhf measurement).  The look-ahead frames carry data like every other frame: the recurrences write there."""
    shape = (q.TP, q.B, q.F)
    if act == ACT_TANH:
        v = _ints(g, -256, 256, *shape) / 64 if pre else _ints(g, -7, 7, *shape) / 8
        v[0, 0, 0], v[-1, -1, q.F - 1] = 0.0, 0.0
    else:
        lo, hi = (-2, 8) if (pre or act == ACT_NONE) else (0, 8) if act == ACT_RELU else (0, 6)
        v = _ints(g, lo, hi, *shape)
        v[0, 0, 0], v[0, 0, 1], v[-1, -1, q.F - 1], v[-1, -1, q.F - 2] = 0.0, 6.0, 0.0, 6.0
        v[0, 0, 2], v[0, 0, 3] = 1.0, 5.0
        if pre or act == ACT_NONE:
            v[0, 0, 4], v[0, 0, 5] = -1.0, 7.0
    if mode == 3 and not pre:
        v[0, q.B - 1] = 0.5 if act == ACT_TANH else 3.0
    out = torch.zeros(q.TP, q.B, q.FP, dtype=torch.float64)
    out[..., :q.F] = v
    return out


def gen_head_pre(g, q, act):
    """sbo [TP][B][F][2], the sub-band head's pre-activation: integers -2 .. 8 with zeros and sixes, multiples of 1 / 64 in -4 .. 4 for Tanh."""
    if act == ACT_TANH:
        v = _ints(g, -256, 256, q.TP, q.B, q.F, 2) / 64
        v[q.LA, 0, 0, 0] = 0.0
        return v
    v = _ints(g, -2, 8, q.TP, q.B, q.F, 2)
    v[q.LA, 0, 0], v[q.LA, 0, 1], v[q.LA, 0, 2] = torch.tensor([0.0, 6.0]), torch.tensor([-1.0, 1.0]), torch.tensor([5.0, 7.0])
    v[q.TP - 1, q.B - 1, q.F - 1] = torch.tensor([6.0, 0.0])
    return v


def kink_notes(act, x, weight=None):
    """How many planted elements sit below / at / above each kink of `act` (weight: only where the upstream gradient is not zero)."""
    x = x if weight is None else x[weight != 0]
    n = lambda m: int(m.sum())
    if act == ACT_RELU:
        return dict(lt0=n(x < 0), at0=n(x == 0), gt0=n(x > 0))
    if act == ACT_RELU6:
        return dict(lt0=n(x < 0), at0=n(x == 0), mid=n((x > 0) & (x < 6)), at6=n(x == 6), gt6=n(x > 6))
    if act == ACT_TANH:
        return dict(at0=n(x == 0), neg=n(x < 0), pos=n(x > 0), big=n(x.abs() > 2))
    return {}


def _pad_last(v, n):
    out = torch.zeros(v.shape[:-1] + (n,), dtype=torch.float64)
    out[..., :v.shape[-1]] = v
    return out


def _with_bg(v, n):
    """v [..][W] in rows stored n wide, the pad columns left as the background (documented as unused: a read of them shows)."""
    out = torch.full(v.shape[:-1] + (n,), BG32, dtype=torch.float64)
    out[..., :v.shape[-1]] = v
    return out


def _tol(count, absterms, exp, dt):
    t = count * 2.0 ** -24 * absterms + 1e-300
    return t + 0.5 * bf16_ulp(exp) if dt == BF16 else t


def _differs(x):
    """Utterance b differs from utterance b + 1 (x [TP][B][..]): an index slip in b shows."""
    return all(not torch.equal(x[:, b], x[:, b + 1]) for b in range(x.shape[1] - 1))


def _stats_of(x_ref, mode, lead):
    """The statistics FSN_NORMSTAT leaves for x_ref [B, C, F, TP], as stored (fp32): mode 2 (mean, std) [B]; 1 / 3 (mean, std) [TP] + lead."""
    if mode == 2:
        m, s = ref_utt_stats(x_ref)
    else:
        m, s = ref_cum_stats(x_ref)
        m, s = m.t().reshape((-1,) + lead), s.t().reshape((-1,) + lead)
        if mode == 1:
            s = torch.zeros_like(s)
    return m.float().double(), s.float().double()


def _stat_image(mode, m, s):
    """(mean, std) in the layout of `stat`: [2][B], or [TP][rows][2]."""
    return (torch.stack([m, s]) if mode == 2 else torch.stack([m, s], -1)).reshape(-1).float()


FAULTS = ("std_n", "relu6_open", "suffix_late", "drop_high", "cnt0")


def plant(case, ln, fault=None):
    """The planted inputs and the float64 expectation of launch `ln` of `case`.  fault: the same inputs with a WRONG expectation, for the comparator's
    own test - std_n (N instead of N - 1 under the gaussian std), relu6_open (ReLU6' = 1 at exactly 6), suffix_late (the cumulative norms' suffix
    sums begin at frame t + 1), drop_high (the gather without the sources mirrored at the upper edge), cnt0 (bin 0's source count off by one)."""
    assert fault is None or fault in FAULTS
    g, d, k, q = _gen(case, ln), ln.d, ln.kind, geom(ln.d)
    mode, dt = d.mode, d.dt
    P = lambda p, t: (p.arena, p.off, t)
    f32 = lambda t: t.reshape(-1).float()

    if k == FSN_IN:
        mag = _ints(g, 0, 7, q.B, q.F, q.T)
        mag_t = torch.zeros(q.TP, q.B, q.F, dtype=torch.float64)
        mag_t[:q.T] = mag.permute(2, 0, 1)
        sums = mag.sum(-1)
        fields = [Field("mag_t", d.out.arena, d.out.off, F32, q.F, mag_t.reshape(-1)), Field("sums", d.sums.arena, d.sums.off, F32, q.F, sums.reshape(-1)),
                  Field("mean", d.aux2.arena, d.aux2.off, F32, 1, sums.sum(1) / (q.F * q.TP), ulps=1)]
        return Planted([P(d.in_, f32(mag))], fields, {"sums": (mag.abs().sum(-1).reshape(-1), mag)},
                       dict(differs=_differs(mag_t), zero_frames=q.LA))

    if k in (FSN_SCALE, FSN_SBSUM, FSN_SBBUILD, FSN_NORMSTAT):
        mag_t = gen_mag_t(g, q, mode)
        puts = [P(d.in_, f32(mag_t))]
        notes = dict(differs=_differs(mag_t))
        sub = k != FSN_SCALE and not (k == FSN_NORMSTAT and d.src == 0)
        if sub:
            fbo = gen_fbo(g, q, d.act, mode)
            puts.append(P(d.aux, f32(fbo)))
            raw_ref = ref_sb_raw(to_ref(mag_t), to_ref(fbo[..., :q.F]), q.nsb, q.nfb)            # [B, F, W, TP]
            raw = tm(raw_ref)                                                                    # [TP][B][F][W]
            notes.update(differs=notes["differs"] and _differs(fbo), la_fbo=int((fbo[q.T:, :, :q.F] != 0).sum()))
            x_ref, x, lead, width = raw_ref, raw, (q.B, q.F), q.W
        else:
            x_ref, x, lead, width = to_ref(mag_t), mag_t, (q.B,), q.F
        if k == FSN_SBSUM:
            sums = raw.sum((0, 3))
            fields = [Field("sums", d.sums.arena, d.sums.off, F32, q.F, sums.reshape(-1)),
                      Field("mean", d.aux2.arena, d.aux2.off, F32, 1, sums.sum(1) / (q.F * q.TP * q.W), ulps=1)]
            return Planted(puts, fields, {"sums": (raw.abs().sum((0, 3)).reshape(-1), raw)}, notes)
        if k == FSN_NORMSTAT:
            if mode == 2:
                m, s = ref_utt_stats(x_ref)
                n = x_ref[0].numel()
                if fault == "std_n":
                    s = s * ((n - 1) / n) ** 0.5
                notes.update(unbiased=float((n / (n - 1)) ** 0.5), n=n)
                fields = [Field("mean", d.stat.arena, d.stat.off, F32, 1, m, ulps=1), Field("std", d.stat.arena, d.stat.off + 4 * q.B, F32, 1, s, ulps=2)]
            else:
                m, s = ref_cum_stats(x_ref)
                m, s = m.t().contiguous(), s.t().contiguous()                                    # [TP][rows]
                notes.update(sd_const=float(s[0, -1]))
                if mode == 1:
                    s = torch.zeros_like(s)                                                      # the unused slot: an exact 0
                ulps = torch.stack([torch.ones_like(m), torch.full_like(s, 2.0 if mode == 3 else 0.0)], -1).reshape(-1).to(torch.int64)
                fields = [Field("mean | std", d.stat.arena, d.stat.off, F32, 2, torch.stack([m, s], -1).reshape(-1), ulps=ulps)]
            return Planted(puts, fields, {}, notes)
        # FSN_SCALE / FSN_SBBUILD: the statistics as an earlier launch stored them (fp32)
        mu = stat = None
        if mode == 0:
            mu = (1 + 2 * torch.rand(q.B, generator=g)).float().double()
            puts.append(P(d.sums, mu.float()))
        else:
            stat = _stats_of(x_ref, mode, lead)
            puts.append(P(d.stat, _stat_image(mode, *stat)))
            if mode == 3:
                notes.update(sd_const=float(stat[1].reshape(q.TP, -1)[0, -1]))
        v, ab = norm_stored(x, mode, mu, stat)
        wide = q.FP if k == FSN_SCALE else q.WP
        exp, tol = _pad_last(v, wide), _pad_last(_tol(N_ROUNDINGS_NORM, ab, v, dt), wide)
        notes.update(pad=wide - width, inexact=int((exp.float().double() != exp).sum()))
        return Planted(puts, [Field("fb_in" if k == FSN_SCALE else "sb_in", d.out.arena, d.out.off, dt, wide, exp.reshape(-1), tol=tol.reshape(-1))], {}, notes)

    if k == FSN_ACT:
        pre = gen_fbo(g, q, d.act, mode, pre=True)
        exp = act_fwd(d.act, pre)
        notes = dict(kinks=kink_notes(d.act, pre[..., :q.F]), pad=q.FP - q.F, la_fbo=int((pre[q.T:, :, :q.F] != 0).sum()), differs=_differs(pre))
        if d.act == ACT_TANH:
            tol = _pad_last(TANHF_BAR_ULPS * f32_ulp(exp[..., :q.F]), q.FP)
            return Planted([P(d.out, f32(pre))], [Field("tanh fbo", d.out.arena, d.out.off, F32, q.FP, exp.reshape(-1), tol=tol.reshape(-1), meas=True)], {}, notes)
        return Planted([P(d.out, f32(pre))], [Field("fbo", d.out.arena, d.out.off, F32, q.FP, exp.reshape(-1))], {}, notes)

    if k == FSN_OUT:
        act = fsn_sbact(d)
        pre = gen_head_pre(g, q, act)
        exp = act_fwd(act, pre[q.LA:]).permute(1, 2, 0, 3).contiguous()                          # [B][F][T][2]: sb_mask[:, :, :, look_ahead:]
        notes = dict(kinks=kink_notes(act, pre[q.LA:]), differs=_differs(pre))
        if act == ACT_TANH:
            return Planted([P(d.in_, f32(pre))], [Field("tanh crm", d.out.arena, d.out.off, F32, 2 * q.T, exp.reshape(-1),
                                                        tol=(TANHF_BAR_ULPS * f32_ulp(exp)).reshape(-1), meas=True)], {}, notes)
        return Planted([P(d.in_, f32(pre))], [Field("crm", d.out.arena, d.out.off, F32, 2 * q.T, exp.reshape(-1))], {}, notes)

    if k == FSN_OUT_BWD:
        act = fsn_sbact(d)
        gc = _ints(g, -3, 3, q.B, q.F, q.T, 2)
        gt = torch.zeros(q.TP, q.B, q.F, 2, dtype=torch.float64)
        gt[q.LA:] = gc.permute(2, 0, 1, 3)
        puts, notes = [P(d.in_, f32(gc))], dict(differs=_differs(gt), zero_frames=q.LA)
        if not act:
            return Planted(puts, [Field("d_sbo", d.out.arena, d.out.off, dt, 2, gt.reshape(-1))], {}, notes)
        pre = gen_head_pre(g, q, act)
        gt[q.LA, 0, :3] = torch.where(gt[q.LA, 0, :3] == 0, torch.ones(3, 2, dtype=torch.float64), gt[q.LA, 0, :3])   # a gradient on every planted kink
        gt[q.TP - 1, q.B - 1, q.F - 1] = torch.tensor([2.0, -1.0])
        puts = [P(d.in_, f32(gt[q.LA:].permute(1, 2, 0, 3).contiguous())), P(d.aux, f32(pre))]
        notes.update(kinks=kink_notes(act, pre, gt))
        exp = gt * act_grad_pre(act, pre, open6=fault == "relu6_open") + 0.0                   # (no negative zero where the derivative is 0)
        if act != ACT_TANH:
            return Planted(puts, [Field("d_sbo", d.out.arena, d.out.off, dt, 2, exp.reshape(-1))], {}, notes)
        y = torch.tanh(pre)
        tol = gt.abs() * (2 * y.abs() * TANHF_BAR_ULPS * f32_ulp(y) + N_ROUNDINGS_ACTGRAD * 2.0 ** -24 * (1 + y * y))
        tol = torch.where(gt == 0, torch.zeros_like(tol), tol + (0.5 * bf16_ulp(exp) if dt == BF16 else 0) + 1e-300)   # t < LA, g == 0: zero bytes
        return Planted(puts, [Field("d_sbo", d.out.arena, d.out.off, dt, 2, exp.reshape(-1), tol=tol.reshape(-1))], {}, notes)

    # the launches behind the sub-band model: d_sb_in integers -3 .. 3 (pad columns: background), sb_in quarters in -4 .. 4 (pad columns zero)
    if k in (FSN_SBBWD_SUM, FSN_NORMBWD) or (k == FSN_SBBWD_APPLY and mode == 0):
        gsb = _ints(g, -3, 3, q.TP, q.B, q.F, q.W)
    if k == FSN_SBBWD_SUM:
        y = _ints(g, -16, 16, q.TP, q.B, q.F, q.W) / 4
        prod = gsb * y
        sums = prod.sum((0, 3))
        fields = [Field("sums", d.sums.arena, d.sums.off, F32, q.F, sums.reshape(-1)),
                  Field("mean", d.aux2.arena, d.aux2.off, F32, 1, sums.sum(1) / (q.F * q.TP * q.W), ulps=1)]
        return Planted([P(d.in_, f32(_with_bg(gsb, q.WP))), P(d.aux, _store(dt, _pad_last(y, q.WP)).reshape(-1))], fields,
                       {"sums": (prod.abs().sum((0, 3)).reshape(-1), prod)}, dict(differs=_differs(gsb) and _differs(y), la_grad=int((gsb[q.T:] != 0).sum())))

    if k == FSN_NORMBWD:
        y = _ints(g, -16, 16, q.TP, q.B, q.F, q.W) / 4
        fbo = gen_fbo(g, q, d.act, mode)
        xfb = tm(ref_unfold(to_ref(fbo[..., :q.F]), q.nfb).reshape(q.B, q.F, q.NFB, q.TP))
        if mode == 2:
            stat = ((1 + 2 * torch.rand(q.B, generator=g)).float().double(), (0.5 + torch.rand(q.B, generator=g)).float().double())
        else:
            stat = ((1 + 2 * torch.rand(q.TP, q.B, q.F, generator=g)).float().double(),
                    (0.5 + torch.rand(q.TP, q.B, q.F, generator=g)).float().double() if mode == 3 else torch.zeros(q.TP, q.B, q.F, dtype=torch.float64))
        puts = [P(d.in_, f32(_with_bg(gsb, q.WP))), P(d.aux2, _store(dt, _pad_last(y, q.WP)).reshape(-1)), P(d.stat, _stat_image(mode, *stat))]
        if mode == 3:
            puts.append(P(d.aux, f32(fbo)))                      # the raw full-band output: read by cumulative_layer_norm's backward alone
        dx, ab, Sf, Gf = normbwd_closed(mode, q, gsb, y, xfb, stat, start=int(fault == "suffix_late"))
        fields = [Field("d_fb_pre", d.out.arena, d.out.off, F32, q.NFB, dx.reshape(-1), tol=(2.0 ** -24 * ab + 1e-300).reshape(-1))]
        if mode == 2:
            fields.append(Field("partial S | G", d.sums.arena, d.sums.off, F32, q.F, torch.stack([Sf, Gf]).reshape(-1)))
        return Planted(puts, fields, {}, dict(differs=_differs(gsb) and _differs(y), la_grad=int((gsb[q.T:] != 0).sum()), la_fbo=int((fbo[q.T:, :, :q.F] != 0).sum())))

    assert k == FSN_SBBWD_APPLY
    fbo = gen_fbo(g, q, d.act, mode)
    mu = Sm = None
    if mode == 0:
        cols = gsb[..., q.NB:]
        mu = (1 + 2 * torch.rand(q.B, generator=g)).float().double()
        # S / N of FSN_SBBWD_SUM, 1 <= |Sm| < 2.1: one source too many or too few moves a bin by |Sm| / (mu + e) >= 1 / 3, more than two half bf16
        # ulps of the largest |d_fb| these integers can give at an edge bin (< 32: 2^-4)
        Sm = ((2 * _ints(g, 0, 1, q.B) - 1) * (1 + _ints(g, 0, 8, q.B) / 8) + torch.arange(q.B) / 32).float().double()
        puts = [P(d.in_, f32(_with_bg(gsb, q.WP))), P(d.aux, f32(fbo)), P(d.aux2, mu.float()), P(d.sums, Sm.float())]
    else:
        cols = _ints(g, -3, 3, q.TP, q.B, q.F, q.NFB)
        puts = [P(d.in_, f32(cols)), P(d.aux, f32(fbo))]
    for f in {0, 1, q.nfb, q.F - 1 - q.nfb, q.F - 2, q.F - 1}:   # a gradient on every column that feeds an edge bin, in every frame
        cols[:, :, max(f - q.nfb, 0):f + q.nfb + 1] = torch.where(cols[:, :, max(f - q.nfb, 0):f + q.nfb + 1] == 0, 1.0, cols[:, :, max(f - q.nfb, 0):f + q.nfb + 1])
    if mode == 0:
        gsb[..., q.NB:] = cols
        puts[0] = P(d.in_, f32(_with_bg(gsb, q.WP)))
    else:
        puts[0] = P(d.in_, f32(cols))
    v, ab, _ = apply_closed(q, mode, d.act, cols, fbo, mu, Sm, cnt_off=int(fault == "cnt0"), drop_high=fault == "drop_high")
    cnt = ref_gather(torch.ones_like(cols), q.nfb)
    mirrored = ref_gather(cols.abs(), q.nfb) - ref_gather(cols.abs(), q.nfb, "constant")         # sum |gradient| over a bin's mirrored sources
    notes = dict(differs=_differs(cols) and _differs(fbo), la_grad=int((cols[q.T:] != 0).sum()), la_fbo=int((fbo[q.T:, :, :q.F] != 0).sum()),
                 kinks=kink_notes(d.act, fbo[..., :q.F]), mirrored={f: float(mirrored[:, :, f].min()) for f in (0, 1, q.nfb, q.F - 1 - q.nfb, q.F - 2, q.F - 1)},
                 edge={f: float(ref_gather(cols.abs(), q.nfb)[:, :, f].min()) for f in (0, q.F - 1)},
                 cnt={f: float(cnt[0, 0, f]) for f in (0, 1, q.F - 2, q.F - 1)}, pad=q.FP - q.F)
    terms = {"gather s": (ref_gather(cols.abs(), q.nfb).reshape(-1), cols)} if q.NFB > 1 else {}
    exp = _pad_last(v, q.FP)
    if mode != 0 and d.act != ACT_TANH:
        return Planted(puts, [Field("d_fb", d.out.arena, d.out.off, dt, q.FP, exp.reshape(-1))], terms, notes)
    tol = _pad_last(_tol(N_ROUNDINGS_APPLY, ab, v, dt), q.FP)
    return Planted(puts, [Field("d_fb", d.out.arena, d.out.off, dt, q.FP, exp.reshape(-1), tol=tol.reshape(-1))], terms, notes)


def conditions(pl):
    """The exactness of a planted launch, from the float64 reference alone: ("" or the first byte-equal fp32 value that is not its own fp32 rounding,
    {sum: (sum|terms| / (largest power of two dividing all terms), 2^24)})."""
    bad = ""
    for f in pl.fields:
        if f.tol is None and f.dt == F32:
            exact = torch.as_tensor(f.ulps).expand(f.exp.shape) == 0
            ne = (f.exp.float().double() != f.exp) & exact
            if bool(ne.any()) and not bad:
                bad = f"{f.name}: element {int(ne.nonzero()[0])} = {float(f.exp[ne][0])!r}"
    sums = {}
    for name, (sabs, t) in pl.terms.items():
        nz = t[t != 0]
        if nz.numel() == 0:
            continue
        q = nz.abs() * 2.0 ** 20
        assert bool((q == q.round()).all()) and float(q.max()) < 2.0 ** 62, (name, "terms are not multiples of 2^-20")
        qi = q.to(torch.int64)
        sums[name] = (float(sabs.max()) / (float((qi & -qi).min()) / 2.0 ** 20), float(LIMIT))
    return bad, sums


# ------------------------------------------------------------------------------------------------ the comparator and the driver
Verdict = namedtuple("Verdict", "ok miss stray per tanh")       # per: {field: worst error / bar (0: byte equality held)}; tanh: worst tanhf error in ulps


def compare(case, ln, fields, before, after):
    """The verdict on one launch: every field in `after` (the arenas behind the launch) against its float64 expectation, per element; every byte of
    the checked arenas outside the fields against `before`.  A miss names case, launch, field, row, column and both values."""
    dev = _u8(after[WS]).device
    head = f"{case.name} phase {ln.phase} op {ln.op} tag {ln.tag} {KIND_NAMES[ln.kind]}"
    miss, per, tanh = "", {}, None
    owned = {a: torch.zeros(_u8(after[a]).numel(), dtype=torch.bool, device=dev) for a in CHECKED}
    for f in fields:
        n, es = f.exp.numel(), _esize(f.dt)
        owned[f.arena][f.off:f.off + n * es] = True
        got = _u8(after[f.arena])[f.off:f.off + n * es].view(_tdtype(f.dt))
        exp = f.exp.to(dev)
        ity = {2: torch.int16, 4: torch.int32}[es]
        same = got.view(ity) == exp.to(torch.float32).to(_tdtype(f.dt)).view(ity)
        if f.tol is not None:
            tol = f.tol.to(dev)
            err = (got.double() - exp).abs()
            ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp(min=1e-300))
            ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
            ratio = torch.where(tol == 0, (~same).double() * float("inf"), ratio).nan_to_num(nan=0.0, posinf=float("inf"))
            bad = ratio > 1
            worst = float(ratio.max())
            if f.meas:
                tanh = max(tanh or 0.0, worst * TANHF_BAR_ULPS)
        elif torch.is_tensor(f.ulps) or f.ulps:
            ulps = torch.as_tensor(f.ulps, device=dev).expand(n).double()
            dist = (_ordered(got.view(torch.int32)) - _ordered(exp.to(torch.float32).view(torch.int32))).abs().double()
            dist = torch.where(torch.isfinite(got), dist, torch.full_like(dist, float("inf")))
            bad = torch.where(ulps == 0, ~same, dist > ulps)
            worst = float(torch.where(ulps == 0, (~same).double() * float("inf"), dist / ulps.clamp(min=1)).nan_to_num(nan=0.0, posinf=float("inf")).max())
        else:
            bad, worst = ~same, 0.0
        per[f.name] = worst if not bool(bad.any()) else float("inf") if worst <= 1 else worst
        if bool(bad.any()) and not miss:
            e = int(bad.nonzero()[0])
            miss = (f"{head} {f.name}: row {e // f.C} column {e % f.C} (element {e}): expected {float(exp[e])!r} device {float(got[e])!r}; "
                    f"{int(bad.sum())} elements outside the bar")
    stray = 0
    for a in CHECKED:
        stray += int(((_u8(after[a]) != _u8(before[a])) & ~owned[a]).sum())
    return Verdict(not miss and stray == 0, miss, stray, per, tanh)


def run_one(case, ln, bench):
    """Launch `ln` alone from its planted state in `bench` (reset it afterwards: bench.reset(planted, whole=True))."""
    pl = plant(case, ln)
    bench.plant(pl)
    bench.run(ln)
    return pl


def _bytes(bench, pl):
    return [_u8(bench.work[f.arena])[f.off:f.off + f.exp.numel() * _esize(f.dt)].clone() for f in pl.fields]


def run_case(case, device, run, only=None):
    """Every struct-Fsn launch of `case` alone from its planted state under compare(); a FSN_NORMSTAT and a *_SUM launch twice from the same planted
    input (the same bytes).  Returns [(launch, Verdict, Planted notes, conditions)] in launch order."""
    plan = plan_of(case)
    bench = Bench(plan, device, run)
    out = []
    for ln in launches(plan):
        if only is not None and not only(ln):
            continue
        pl = run_one(case, ln, bench)
        v = compare(case, ln, pl.fields, bench.ref, bench.work)
        if ln.kind in RERUN and v.ok:
            first = _bytes(bench, pl)
            bench.restore_outputs(pl)
            bench.run(ln)
            v2 = compare(case, ln, pl.fields, bench.ref, bench.work)
            if not v2.ok or not all(torch.equal(a, b) for a, b in zip(first, _bytes(bench, pl))):
                v = Verdict(False, v2.miss or f"{case.name} tag {ln.tag} {KIND_NAMES[ln.kind]}: run 2 from the same planted input gave other bytes than run 1",
                            v2.stray, v2.per, v2.tanh)
        out.append((ln, v, pl.notes, conditions(pl)))
        bench.reset(pl, whole=v.stray > 0)
    return out


def geometry(ln):
    q = geom(ln.d)
    return f"B {q.B} F {q.F}/{q.FP} T {q.T}+{q.LA} W {q.W}/{q.WP} NFB {q.NFB} mode {ln.d.mode} src {ln.d.src} act {ln.d.act}/{fsn_sbact(ln.d)} dt {ln.d.dt}"


def report_lines(case, results):
    """One line per launch: the worst error of every field in units of its bar (0: byte equality held), the measured tanhf error, the verdict."""
    lines = []
    for ln, v, _, _ in results:
        per = " ".join(f"[{name}] {w:.3f}" for name, w in v.per.items())
        tanh = f" tanhf {v.tanh:.3f} ulps (bar {TANHF_BAR_ULPS})" if v.tanh is not None else ""
        lines.append(f"{case.name:16s} tag {ln.tag:4d} {KIND_NAMES[ln.kind]:16s} {geometry(ln)}: err/bar {per}{tanh} {'ok' if v.ok else 'MISS'} stray {v.stray}"
                     + (f" {v.miss}" if v.miss else ""))
    return lines
