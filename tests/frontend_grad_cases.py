"""The gradient half of the front-end case table (frontend_cases.py holds the forward half and is imported, never edited): inputs, seeded Gaussian
cotangents and float64 references of the backward passes of tools_for_model's `stft`, `istft`, `mag_phase` and `build_complex_ideal_ratio_mask`,
shared by the CPU tier (test_frontend_grad_cpu.py) and the GPU tier (test_gpu_frontend_grad.py).  Everything here runs on the CPU from torch and
the oracle alone and imports nothing of the package under test.  Complex cotangents and gradients are in PyTorch's convention, g = dL/dRe + i dL/dIm.

stft.  Every STFT_CASES entry with n_fft 512 (the others are refused at the forward call when the input requires a gradient).  Reference:
torch.autograd.grad of float64 torch.stft.  Metric: max-norm error over the largest float64 element.  Bar: max(STFT_FLOOR, STFT_MARGIN x alone),
`alone` = float32 torch autograd with the hann32 window against float64 - the project's margin and floor for this transform.

istft.  Lengths 300, 4801, 6000, 6150 and the tail lengths 6190, 6199 at B = 1 and 3, the hop 128 / 256 cases and the one-frame case, on both
spectrum kinds.  Reference: torch.autograd.grad of float64 torch.istft.  Bound per element
    |got - ref64|[k, t] <= K eps32 (c_k / N) A_t,   A_t = sum_j w[j] |gy[t hop + j - pad]| / env[t hop + j]   (float64, covered samples only),
K = ISTFT_MARGIN x K_ref, K_ref the smallest K at which float32 torch autograd meets the bound on the cases whose float64 envelope stays above
1e-2 over the covered samples (istft_grad_k_reference()).  The tail cases are held to the same K but left out of K_ref: float32 torch's own envelope is
wrong there, the planner's is not.  K_ref = 0.45 (measured, torch on the CPU; the CPU tier prints and pins it), K = 1.82.
Through (mag, phase) the polar adjoint g_m = g_re cos + g_im sin, g_ph = m (g_im cos - g_re sin) adds two products and a sum of float32 values and
float32 cos / sin (<= 2 ulp each): 4 eps32 of the two terms' magnitudes (5 for g_ph: one more product) on top of the spectrum bound taken through the
same map (polar_reference()).

Targets.  The first n bins of frontend_cases' target grid, n in TARGET_GRAD_SIZES.  Reference: float64 torch autograd of torch.abs / torch.angle and of
the oracle's build_cirm.  Metric per arm of TARGET_ARMS: the largest |got - ref64| / (eps32 S) over the arm's gradient elements, S the sum of the
magnitudes of the terms of that element's gradient formula in float64, with what float32 can know of the ratio mask v carried through e^{-C v}
(target_scales(): a condition-aware unit, so that one badly conditioned bin does not set the figure for a whole arm).  Bar per arm: TARGET_MARGIN x the figure of float32 torch autograd alone, taken over the
largest case, which holds every other as a prefix.  A bin-level arm covers both components of its bins; a cIRM arm covers the bins with at least one
mask component in it.  Where noisy == 0 the mag_phase gradient is exactly 0 (torch's complex abs / angle backward gives 0 there too; the
sqrt / atan2 formulation gives NaN); a cotangent that lives on the clamp arm alone gives a cIRM gradient of exactly 0.
"""
import functools
import warnings
from collections import namedtuple

import numpy as np
import torch

import frontend_cases as fc
from oracle import fullsubnet as ofsn

EPS32 = fc.EPS32
FLT_MIN = float(np.finfo(np.float32).tiny)
NFFT = fc.NFFT


def gauss(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    if dtype.is_complex:
        return torch.view_as_complex(torch.randn(tuple(shape) + (2,), generator=g))
    return torch.randn(tuple(shape), generator=g)


def c_weights(nfft=NFFT):
    """c_k / N, [N/2 + 1]: 1 at DC and Nyquist, else 2."""
    c = torch.full((nfft // 2 + 1,), 2.0, dtype=torch.float64)
    c[0] = c[-1] = 1.0
    return c / nfft


# ------------------------------------------------------------------------------------------ the identities, restated in float64
def stft_adjoint64(g, L, nfft, hop, win):
    """The stft backward as the issue and DESIGN.md section 6 state it: g complex [B, N/2 + 1, T] -> dx [B, L] (float64)."""
    g = g.to(torch.complex128)
    B, NF, T = g.shape
    pad = nfft // 2
    w = fc.padded_window(win, nfft)
    k = torch.arange(NF, dtype=torch.float64)
    j = torch.arange(nfft, dtype=torch.float64)
    E = torch.exp(2j * np.pi * torch.outer(j, k) / nfft)                       # e^{+2 pi i k j / N}: no half weights, no 1 / N
    frames = torch.einsum("jk,bkt->btj", E, g).real * w                        # [B, T, N]
    dxp = torch.zeros(B, L + nfft, dtype=torch.float64)
    for t in range(T):
        dxp[:, t * hop:t * hop + nfft] += frames[:, t]
    i = torch.arange(L)
    dx = dxp[:, i + pad]
    left = (i >= 1) & (i <= pad)
    dx[:, left] += dxp[:, pad - i[left]]
    right = (i >= L - 1 - pad) & (i <= L - 2)
    dx[:, right] += dxp[:, pad + 2 * (L - 1) - i[right]]
    return dx


def _covered(T, hop, L, nfft=NFFT):
    """(Lp, Lcov): the padded span of T frames and how many samples of the clip it covers (Ola::Lout of the plan)."""
    Lp = (T - 1) * hop + nfft
    return Lp, min(L, Lp - nfft // 2)


def istft_adjoint64(gy, T, hop, win, nfft=NFFT):
    """The istft backward as stated: gy [B, L] -> gX complex128 [B, N/2 + 1, T]."""
    gy = gy.double()
    B, L = gy.shape
    pad = nfft // 2
    Lp, Lcov = _covered(T, hop, L, nfft)
    env = fc.envelope(T, hop, win, nfft)
    gyp = torch.zeros(B, Lp, dtype=torch.float64)
    gyp[:, pad:pad + Lcov] = gy[:, :Lcov] / env[pad:pad + Lcov]
    w = fc.padded_window(win, nfft)
    gframes = torch.stack([gyp[:, t * hop:t * hop + nfft] * w for t in range(T)], -1)          # [B, N, T]
    gX = torch.fft.rfft(gframes, dim=1) * c_weights(nfft)[:, None]
    gX.imag[:, 0] = 0.0
    gX.imag[:, -1] = 0.0
    return gX


# ------------------------------------------------------------------------------------------ stft gradient
STFT_GRAD_CASES = tuple(c for c in fc.STFT_CASES if c.nfft == 512)
STFT_REFUSED_CASES = tuple(c for c in fc.STFT_CASES if c.nfft != 512)
StftGradRef = namedtuple("StftGradRef", "grad alone bar")


@functools.lru_cache(maxsize=None)
def stft_cotangent(c):
    return gauss((c.B, c.nfft // 2 + 1, 1 + c.L // c.hop), 300 + c.L + c.hop + c.win + c.B, torch.complex64)


def _stft_autograd(c, dtype):
    x = fc.stft_input(c).to(dtype).clone().requires_grad_(True)       # clone: frontend_cases caches its inputs
    w = fc.hann64(c.win) if dtype == torch.float64 else fc.hann32(c.win)
    S = torch.stft(x, c.nfft, c.hop, c.win, window=w, return_complex=True)
    return torch.autograd.grad(S, x, stft_cotangent(c).to(S.dtype))[0]


def grad_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def stft_grad_reference(c):
    ref = _stft_autograd(c, torch.float64)
    alone = grad_err(_stft_autograd(c, torch.float32), ref)
    return StftGradRef(ref, alone, max(fc.STFT_FLOOR, fc.STFT_MARGIN * alone))


# ------------------------------------------------------------------------------------------ istft gradient
ISTFT_GRAD_LENGTHS = (300, 4801, 6000, 6150)
ISTFT_GRAD_TAILS = (6190, 6199)
ISTFT_GRAD_CASES = tuple(fc.IstftCase(B, L, 300, 400) for L in ISTFT_GRAD_LENGTHS + ISTFT_GRAD_TAILS for B in (1, 3)) + (
    fc.IstftCase(2, 1000, 128, 512), fc.IstftCase(2, 1000, 256, 512), fc.IstftCase(2, 400, 512, 512))
ONE_FRAME_CASE = fc.IstftCase(2, 400, 512, 512)
ENV_FLOOR = 1e-2


def istft_spectrum(c, kind):
    """complex64 [B, 257, T]: frontend_cases' spectrum where it has the case (B = 1, 3 at hop 300), the same recipe elsewhere."""
    return fc.istft_spectrum(c, kind)


@functools.lru_cache(maxsize=None)
def istft_cotangent(c):
    return gauss((c.B, c.L), 400 + c.L + 3 * c.B + c.hop)


def in_k_reference(c):
    """Is the float64 envelope above ENV_FLOOR over the covered samples?"""
    T = 1 + c.L // c.hop
    _, Lcov = _covered(T, c.hop, c.L)
    env = fc.envelope(T, c.hop, c.win)
    return float(env[NFFT // 2:NFFT // 2 + Lcov].min()) > ENV_FLOOR


def _istft_autograd(c, kind, dtype):
    S = istft_spectrum(c, kind).to(torch.complex128 if dtype == torch.float64 else torch.complex64).clone().requires_grad_(True)
    w = fc.hann64(c.win) if dtype == torch.float64 else fc.hann32(c.win)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = torch.istft(S, NFFT, c.hop, c.win, window=w, length=c.L)
    return torch.autograd.grad(y, S, istft_cotangent(c).to(dtype))[0]


def istft_grad_unit(c):
    """eps32 (c_k / N) A_t, [257, T] per batch item -> [B, 257, T]."""
    gy = istft_cotangent(c).double()
    T = 1 + c.L // c.hop
    pad = NFFT // 2
    Lp, Lcov = _covered(T, c.hop, c.L)
    env = fc.envelope(T, c.hop, c.win)
    a = torch.zeros(c.B, Lp, dtype=torch.float64)
    a[:, pad:pad + Lcov] = gy[:, :Lcov].abs() / env[pad:pad + Lcov]
    w = fc.padded_window(c.win, NFFT)
    A = torch.stack([(a[:, t * c.hop:t * c.hop + NFFT] * w).sum(-1) for t in range(T)], -1)    # [B, T]
    return EPS32 * c_weights()[None, :, None] * A[:, None, :]


@functools.lru_cache(maxsize=None)
def istft_grad_reference(c, kind):
    """(float64 gradient complex128 [B, 257, T], unit [B, 257, T])."""
    return _istft_autograd(c, kind, torch.float64), istft_grad_unit(c)


def complex_bound_ratio(got, ref, unit):
    """The smallest K at which both parts of `got` meet the bound; where the unit is 0 the gradient has to be exact."""
    g = torch.view_as_real(got.to(torch.complex128))
    r = torch.view_as_real(ref.to(torch.complex128))
    return fc.bound_ratio(g, r, unit[..., None].expand_as(r))


@functools.lru_cache(maxsize=None)
def istft_grad_k_alone(c, kind):
    ref, unit = istft_grad_reference(c, kind)
    return complex_bound_ratio(_istft_autograd(c, kind, torch.float32), ref, unit)


@functools.lru_cache(maxsize=None)
def istft_grad_k_reference():
    return max(istft_grad_k_alone(c, kind) for c in ISTFT_GRAD_CASES if in_k_reference(c) for kind in fc.ISTFT_KINDS)


def istft_grad_k():
    return fc.ISTFT_MARGIN * istft_grad_k_reference()


def polar_reference(c, kind):
    """(mag, phase) float32 of the case's spectrum, the float64 gradients (g_m, g_ph) of istft(mag (cos, sin)(phase)), and their bounds' units:
    (K-part, constant part) for each - the bound is K x K-part + constant part (module docstring)."""
    S = istft_spectrum(c, kind)
    mag, ph = S.abs(), S.angle()
    m64, p64 = mag.double().requires_grad_(True), ph.double().requires_grad_(True)
    Sp = torch.complex(m64 * torch.cos(p64), m64 * torch.sin(p64))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = torch.istft(Sp, NFFT, c.hop, c.win, window=fc.hann64(c.win), length=c.L)
    gX = torch.autograd.grad(y, Sp, istft_cotangent(c).double(), retain_graph=True)[0]
    gm, gp = torch.autograd.grad(y, (m64, p64), istft_cotangent(c).double())
    unit = istft_grad_unit(c)
    cs, sn = torch.cos(p64).detach().abs(), torch.sin(p64).detach().abs()
    terms = gX.real.abs() * cs + gX.imag.abs() * sn
    terms_p = gX.imag.abs() * cs + gX.real.abs() * sn
    m = m64.detach()
    return mag, ph, gm, gp, (unit * (cs + sn), 4 * EPS32 * terms), (m * unit * (cs + sn), 5 * EPS32 * m * terms_p)


def polar_bound_ok(got, ref, kpart, const, K):
    return bool(((got.double() - ref).abs() <= K * kpart + const).all())


# ------------------------------------------------------------------------------------------ targets
TARGET_GRAD_SIZES = (1, 257, fc.TARGET_PASS + 257)
TARGET_MARGIN = fc.TARGET_MARGIN
TargetGradRef = namedtuple("TargetGradRef", "d_mp d_noisy d_clean s_mp s_noisy s_clean masks")


def target_cotangents(n):
    """(g_mag [n], g_phase [n], g_cirm [n, 2]): prefixes of one seeded draw."""
    big = max(TARGET_GRAD_SIZES)
    g = _cot_pool(big)
    return g[0][:n].clone(), g[1][:n].clone(), g[2][:n].clone()


@functools.lru_cache(maxsize=None)
def _cot_pool(n):
    return gauss((n,), 501), gauss((n,), 502), gauss((n, 2), 503)


def _target_autograd(n, dtype):
    """Gradients as real pairs [n, 2]: (d noisy of mag_phase, d noisy of cIRM, d clean of cIRM)."""
    noisy, clean = fc.target_inputs(n)
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    gm, gp, gc = (t.to(dtype) for t in target_cotangents(n))
    z = noisy.to(cd).clone().requires_grad_(True)
    d_mp = torch.autograd.grad((torch.abs(z), torch.angle(z)), z, (gm, gp))[0]
    z, c = noisy.to(cd).clone().requires_grad_(True), clean.to(cd).clone().requires_grad_(True)
    d_n, d_c = torch.autograd.grad(ofsn.build_cirm(z, c), (z, c), gc)
    return tuple(torch.view_as_real(t.resolve_conj()).clone() for t in (d_mp, d_n, d_c))


def target_scales(n):
    """float64 sums of the magnitudes of the terms of every gradient element, [n, 2] each: (mag_phase, d noisy of cIRM, d clean of cIRM)."""
    noisy, clean = fc.target_inputs(n)
    gm, gp, gc = (t.double() for t in target_cotangents(n))
    nr, ni, cr, ci = noisy.real.double(), noisy.imag.double(), clean.real.double(), clean.imag.double()
    m = torch.sqrt(nr * nr + ni * ni)
    ms = m.clamp_min(1e-300)
    s_mp = torch.stack((gm.abs() * nr.abs() / ms + gp.abs() * ni.abs() / ms ** 2, gm.abs() * ni.abs() / ms + gp.abs() * nr.abs() / ms ** 2), -1)
    den = nr * nr + ni * ni + ofsn.EPSILON
    v = fc.cirm_ratio64(noisy, clean)
    # T_e >= |v_e|: the ratio's terms over den - eps32 T_e is what float32 can know of v_e (products that cancel included), and e^{-C v} turns an
    # absolute error d of v into a relative one of C d; a float32 e^{-C v} is no better than FLT_MIN absolute (it goes subnormal past v ~ 870)
    T = torch.stack((((nr * cr).abs() + (ni * ci).abs()) / den, ((nr * ci).abs() + (ni * cr).abs()) / den), -1)
    ex = torch.exp(-0.1 * v)
    h = torch.where(v <= -100.0, torch.zeros_like(v), gc.abs() * 2.0 * (ex + FLT_MIN / EPS32) / (1.0 + ex) ** 2 * (1.0 + 0.1 * T))
    hv = 2.0 * (h[:, 0] * T[:, 0] + h[:, 1] * T[:, 1])
    s_n = torch.stack(((h[:, 0] * cr.abs() + h[:, 1] * ci.abs() + nr.abs() * hv) / den, (h[:, 0] * ci.abs() + h[:, 1] * cr.abs() + ni.abs() * hv) / den), -1)
    s_c = torch.stack(((h[:, 0] * nr.abs() + h[:, 1] * ni.abs()) / den, (h[:, 0] * ni.abs() + h[:, 1] * nr.abs()) / den), -1)
    return s_mp, s_n, s_c


def bin_masks(n):
    """{arm: bool [n]}: frontend_cases' masks, a cIRM arm reduced to the bins with at least one component in it."""
    noisy, clean = fc.target_inputs(n)
    return {a: (v if v.dim() == 1 else v.any(-1)) for a, v in fc.target_masks(noisy, clean).items()}


@functools.lru_cache(maxsize=None)
def target_grad_reference(n):
    d = _target_autograd(n, torch.float64)
    return TargetGradRef(*d, *target_scales(n), bin_masks(n))


def arm_cost(got, ref, scale, mask):
    """Largest |got - ref| / (eps32 S) over the bins of `mask` ([n, 2] gradients); an element whose scale is 0 has to be exact.  0.0 for an empty arm."""
    if not bool(mask.any()):
        return 0.0
    return fc.bound_ratio(got[mask], ref[mask], EPS32 * scale[mask])


@functools.lru_cache(maxsize=None)
def target_grad_bars():
    """{(which, arm): (alone, bar)} over the largest case; which in ('mag_phase', 'cirm_noisy', 'cirm_clean')."""
    n = max(TARGET_GRAD_SIZES)
    r = target_grad_reference(n)
    a32 = _target_autograd(n, torch.float32)
    out = {}
    for which, got, ref, sc in (("mag_phase", a32[0], r.d_mp, r.s_mp), ("cirm_noisy", a32[1], r.d_noisy, r.s_noisy), ("cirm_clean", a32[2], r.d_clean, r.s_clean)):
        for arm in fc.TARGET_ARMS:
            alone = arm_cost(got, ref, sc, r.masks[arm])
            out[(which, arm)] = (alone, TARGET_MARGIN * alone)
    return out


def clamp_only_cotangent(n):
    """g_cirm restricted to the components on the clamp arm (zero elsewhere), and whether there is any."""
    noisy, clean = fc.target_inputs(n)
    clamp = fc.target_masks(noisy, clean)["clamp"]
    return target_cotangents(n)[2] * clamp, bool(clamp.any())


# ------------------------------------------------------------------------------------------ compress_cIRM
def compress_reference(mask, K=10.0, C=0.1):
    """tools_for_model.py:707-717 in float64."""
    m = torch.as_tensor(mask, dtype=torch.float64)
    m = torch.where(m <= -100, torch.full_like(m, -100.0), m)
    return K * (1 - torch.exp(-C * m)) / (1 + torch.exp(-C * m))


def compress_inputs():
    return torch.cat([torch.linspace(-19.9, 19.9, 399), torch.tensor([-1e6, -1000.0, -100.5, -100.0, -99.99, -50.0, 0.0, 50.0, 500.0])]).float()
