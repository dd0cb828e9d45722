"""The case table of the FullSubNet helpers of tools_for_model.py - `stft` (TorchSTFT plan), `istft` (TorchISTFT plan), `mag_phase` and
`build_complex_ideal_ratio_mask` (fsn_targets_kernel), `decompress_cIRM` - shared by the CPU tier (test_frontend_cases_cpu.py: the plans on the
host simulator, the planners' refusals, are the cases any good?) and the GPU tier (test_gpu_frontend_edges.py: do the kernels hold on them?).
Inputs and float64 references only: everything here is deterministic, runs on the CPU from torch and the oracle alone, and imports nothing of
the package under test.

STFT.  (B, L, n_fft, hop, win) on seeded Gaussian noise of scale 0.3 - energy at both clip ends, where reflect padding is what differs from
the DCCRN front end.  Reference torch.stft in float64.  Bar: max-norm error over the largest reference bin, 4 x the distance of float32
torch.stft to float64 (another accumulation order in the GEMM), floor 2e-7.

iSTFT.  (B, L, hop, win) at n_fft 512, a consistent spectrum (float32 torch.stft of noise) and an inconsistent one (the same x (1 + randn / 2)).
Reference torch.istft in float64.  The lengths walk the clip's end down the falling edge of the last window (L mod 300 = 150 .. 200 at win 400:
the envelope goes from 0.25 to 3.8e-9), where the inverse is ill-conditioned, so the bar is per sample:
    |out[p] - ref64[p]| <= K * eps32 * A[p] / env[p],   A[p] = sum_t Fmax_t * w[p + pad - t * hop],
Fmax_t the largest |sample| of frame t's float64 inverse FFT, env the float64 window envelope.  K = 4 x K_ref, K_ref the smallest K at which
float32 torch.istft itself meets the bound on every case (istft_k_reference()).

The float32 runs of torch take the window as the float64 Hann table rounded to float32 - what the planners build.  torch.hann_window in float32
evaluates 0.5 - 0.5 cos in float32, which costs 3e-8 ABSOLUTE on every tap: 5e-4 of the tap the last sample of L = 6200 is divided by.  A K_ref
taken from that window is ~100 x larger and no longer sees an envelope that is off by 1e-8 at L = 6190.

Targets.  A crafted complex grid (every arm of TARGET_ARMS, see target_census) followed by seeded noise; a case of n elements is the first n.
"""
import functools
import warnings
from collections import namedtuple

import numpy as np
import torch

from oracle import fullsubnet as ofsn

EPS32 = float(np.finfo(np.float32).eps)


def hann64(win):
    return torch.hann_window(win, dtype=torch.float64)


def hann32(win):
    """The float64 table rounded once (module docstring)."""
    return hann64(win).float()


def padded_window(win, nfft):
    w = torch.zeros(nfft, dtype=torch.float64)
    left = (nfft - win) // 2
    w[left:left + win] = hann64(win)
    return w


def noise(B, L, seed):
    return torch.randn(B, L, generator=torch.Generator().manual_seed(seed)) * 0.3


# ------------------------------------------------------------------------------------------ STFT
StftCase = namedtuple("StftCase", "B L nfft hop win")
STFT_CASES = tuple(StftCase(*c) for c in (
    (2, 6000, 512, 300, 400),            # the configuration every other test uses
    (3, 4801, 512, 300, 400),            # odd length
    (1, 257, 512, 300, 400),             # the shortest clip reflect padding takes: T = 1
    (5, 1000, 512, 128, 512),            # window as long as the transform
    (2, 3001, 256, 100, 255),            # odd window, no room left of it
    (2, 3001, 1024, 300, 400),
    (2, 3000, 512, 300, 399),            # odd room around the window
    (7, 6000, 512, 300, 400),            # 147 frames: several GEMM row tiles, the last one partial
    (1, 300, 512, 300, 400),             # T = 2, both frames reflect-padded on both sides
    (2, 1000, 512, 256, 512),
))
STFT_MARGIN, STFT_FLOOR = 4.0, 2e-7


def stft_id(c):
    return f"B{c.B}-L{c.L}-fft{c.nfft}-hop{c.hop}-win{c.win}"


@functools.lru_cache(maxsize=None)
def stft_input(c):
    return noise(c.B, c.L, 100 + c.L + c.nfft + c.hop + c.win + c.B)


StftRef = namedtuple("StftRef", "spec alone bar")


@functools.lru_cache(maxsize=None)
def stft_reference(c):
    """float64 torch.stft [B, n_fft/2 + 1, T], what float32 torch.stft alone costs against it, and the bar - all relative to the largest bin."""
    x = stft_input(c)
    ref = torch.stft(x.double(), c.nfft, c.hop, c.win, window=hann64(c.win), return_complex=True)
    s32 = torch.stft(x, c.nfft, c.hop, c.win, window=hann32(c.win), return_complex=True)
    alone = stft_err(s32, ref)
    return StftRef(ref, alone, max(STFT_FLOOR, STFT_MARGIN * alone))


def stft_err(got, ref):
    return float((got.to(torch.complex128) - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------ iSTFT
IstftCase = namedtuple("IstftCase", "B L hop win")
NFFT = 512
TAIL_LENGTHS = (300, 4801, 6000, 6150, 6180, 6190, 6199, 6200)
ISTFT_CASES = tuple(IstftCase(B, L, 300, 400) for L in TAIL_LENGTHS for B in (1, 3, 5)) + (
    IstftCase(2, 1000, 128, 512), IstftCase(2, 1000, 256, 512),
    IstftCase(2, 400, 512, 512))             # one frame, and the clip runs 144 samples past it: zeros there, as torch pads
ISTFT_KINDS = ("consistent", "inconsistent")
ISTFT_MARGIN = 4.0
LENGTH_NONE_CASE = IstftCase(3, 6000, 300, 400)              # L = hop * (T - 1): what length=None means
SWEEP_CONFIGS = ((300, 400), (128, 512), (256, 512), (512, 512), (100, 400))
SWEEP_LENGTHS = range(250, 1400)


def istft_id(c):
    return f"B{c.B}-L{c.L}-hop{c.hop}-win{c.win}"


@functools.lru_cache(maxsize=None)
def istft_spectrum(c, kind):
    """complex64 [B, 257, 1 + L // hop]."""
    seed = 200 + c.L + 7 * c.B + c.hop
    S = torch.stft(noise(c.B, c.L, seed), NFFT, c.hop, c.win, window=hann32(c.win), return_complex=True)
    if kind == "inconsistent":
        S = S * (1.0 + 0.5 * torch.randn(S.shape, generator=torch.Generator().manual_seed(seed + 1)))
    return S


def _overlap_add(per_frame, w, hop):
    """[..., T] weights x window [nfft] -> [..., (T - 1) * hop + nfft]."""
    T, n = per_frame.shape[-1], w.numel()
    out = torch.zeros(per_frame.shape[:-1] + ((T - 1) * hop + n,), dtype=torch.float64)
    for t in range(T):
        out[..., t * hop:t * hop + n] += per_frame[..., t:t + 1] * w
    return out


def _clip(x, L, fill):
    """Samples [n_fft/2, n_fft/2 + L) of a padded signal; what lies past its end is `fill` (torch.istft pads the clip with zeros there)."""
    x = x[..., NFFT // 2:NFFT // 2 + L]
    return torch.nn.functional.pad(x, (0, L - x.shape[-1]), value=fill)


def envelope(T, hop, win, nfft=NFFT):
    """float64 window envelope over the padded signal, [(T - 1) * hop + nfft]."""
    w = padded_window(win, nfft)
    return _overlap_add(torch.ones(T, dtype=torch.float64), w * w, hop)


def istft64(spec, hop, win, L, env_eps=0.0):
    """torch.istft in float64, restated so that the envelope can be damaged (env_eps: the mutant of the CPU tier); env_eps = 0 is asserted
    against torch.istft itself in the CPU tier."""
    S = spec.to(torch.complex128)
    w = padded_window(win, NFFT)
    frames = torch.fft.irfft(S, n=NFFT, dim=1)                                  # [B, nfft, T]
    y = torch.zeros(S.shape[0], (S.shape[-1] - 1) * hop + NFFT, dtype=torch.float64)
    for t in range(S.shape[-1]):
        y[:, t * hop:t * hop + NFFT] += frames[:, :, t] * w
    return _clip(y, L, 0.0) / (_clip(envelope(S.shape[-1], hop, win), L, 1.0) + env_eps)


def istft_reference(spec, hop, win, L):
    """(float64 torch.istft [B, L], the bound's unit eps32 * A / env [B, L]) of any complex64 spectrum [B, 257, T]."""
    S = spec.to(torch.complex128)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                # "the output will be padded with zeros": IstftCase(2, 400, 512, 512)
        ref = torch.istft(S, NFFT, hop, win, window=hann64(win), length=L)
    fmax = torch.fft.irfft(S, n=NFFT, dim=1).abs().amax(dim=1)                  # [B, T]
    A = _clip(_overlap_add(fmax, padded_window(win, NFFT), hop), L, 0.0)
    return ref, EPS32 * A / _clip(envelope(S.shape[-1], hop, win), L, 1.0)


@functools.lru_cache(maxsize=None)
def istft_case_reference(c, kind):
    return istft_reference(istft_spectrum(c, kind), c.hop, c.win, c.L)


def bound_ratio(got, ref, unit):
    """The smallest K at which `got` meets the bound; a sample whose bound is 0 (past the last frame) has to be exact."""
    d = (got.double() - ref).abs()
    return float(torch.where(unit > 0, d / unit.clamp_min(1e-300), torch.where(d > 0, float("inf"), 0.0).double()).max())


@functools.lru_cache(maxsize=None)
def istft_k_reference():
    """K_ref: float32 torch.istft against float64 over every case and both spectra, in units of the bound."""
    worst = 0.0
    for c in ISTFT_CASES:
        for kind in ISTFT_KINDS:
            ref, unit = istft_case_reference(c, kind)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = torch.istft(istft_spectrum(c, kind), NFFT, c.hop, c.win, window=hann32(c.win), length=c.L)
            worst = max(worst, bound_ratio(got, ref, unit))
    return worst


def istft_k():
    return ISTFT_MARGIN * istft_k_reference()


def torch_istft_accepts(L, hop, win):
    """Does torch.istft return a clip of L samples from 1 + L // hop frames (its window overlap-add test)?"""
    S = torch.zeros(1, NFFT // 2 + 1, 1 + L // hop, dtype=torch.complex64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            torch.istft(S, NFFT, hop, win, window=hann32(win), length=L)
        except RuntimeError as e:
            assert "window overlap add min" in str(e), e
            return False
    return True


# ------------------------------------------------------------------------------------------ targets
TARGET_PASS = 16384 * 256                      # elements one pass of the grid-stride launch takes (csrc/fsn.hip gridn: at most 16384 blocks of 256)
TARGET_SIZES = (1, 255, 256, 257, TARGET_PASS + 257)       # 4.2M complex bins: 67 MB of input, well under a second of kernel and reference
DECADES = tuple(range(-6, 3))                  # |noisy| in [10^k, 10^(k+1)), k = -6 .. 2, and 1e3 itself in the last
TARGET_ARMS = (("zero", "neg_real_pos0", "neg_real_neg0", "pos_real", "pos_imag", "neg_imag", "q1", "q2", "q3", "q4")
               + tuple(f"mag_1e{k}" for k in DECADES) + ("clamp", "saturate", "eps_decides", "noisy_zero", "cancels", "else"))
CIRM_ARMS = ("clamp", "saturate", "eps_decides", "noisy_zero", "cancels", "else")
CANCELS = 100.0                                # a ratio component whose two products cancel to less than 1 / 100 of their size
CLAMP_CLEAR, SATURATE_FROM = -100.01, 200.0    # crafted members stay this clear of the clamp's edge / this far into the saturation


def _crafted():
    """(noisy, clean) complex64: every arm several times over, in an order that puts one of each kind into the first 255."""
    n, c = [], []

    def add(nr, ni, cr, ci):
        n.append(complex(nr, ni))
        c.append(complex(cr, ci))

    rows = []
    # zero bins, the signed zeros on the negative real axis, the axes
    for cl in ((0.0, 0.0), (0.5, -0.25), (-3.0, 2.0)):
        rows += [(0.0, 0.0) + cl, (0.0, -0.0) + cl]
        for m in (1e-6, 0.3, 1.0, 1e3):
            rows += [(-m, 0.0) + cl, (-m, -0.0) + cl, (m, 0.0) + cl, (m, -0.0) + cl, (0.0, m) + cl, (0.0, -m) + cl, (-0.0, m) + cl, (-0.0, -m) + cl]
    rows += [(-0.0, 0.0, 1.0, 1.0), (-0.0, -0.0, 1.0, 1.0)]
    # magnitudes 1e-6 .. 1e3 in every quadrant, clean of the same and of unit scale
    for k in range(-6, 4):
        for j, th in enumerate(np.linspace(0.1, 2 * np.pi + 0.1, 12, endpoint=False)):
            m = 10.0 ** k * (1.0 if k == 3 or j % 3 == 0 else 1.0 + 0.7 * j)
            m = min(m, 1e3)
            rows.append((m * np.cos(th), m * np.sin(th), m * np.cos(th + 0.5 * j), m * np.sin(th + 0.5 * j)))
            rows.append((m * np.cos(th), m * np.sin(th), np.cos(1.0 + j), np.sin(1.0 + j)))
    # the clamp (ratio component <= -100) and the saturation (>= 200), on either component: clean = ratio x noisy
    for r in (-100.5, -101.0, -150.0, -1e3, -1e5, 200.0, 250.0, 1e3, 1e6):
        for nz in (complex(1.0, 0.0), complex(0.6, -0.8), complex(-2.0, 3.0), complex(0.05, 0.02)):
            for ratio in (complex(r, 0.3), complex(-0.7, r), complex(r, r)):
                cl = ratio * nz
                rows.append((nz.real, nz.imag, cl.real, cl.imag))
    # |noisy|^2 within a factor 4 of float32 eps: the denominator's epsilon decides
    for s in (0.26, 0.5, 0.9, 1.0, 1.1, 2.0, 3.9):
        for th in (0.0, 0.7, 2.0, 3.5, 5.5):
            m = float(np.sqrt(s * EPS32))
            for cs in (m, 1.0, 1e-3):
                rows.append((m * np.cos(th), m * np.sin(th), cs * np.cos(th + 1.0), cs * np.sin(th + 1.0)))
    # spread the kinds: a stride walk over the list (its length and the stride are coprime)
    stride = 37
    assert np.gcd(stride, len(rows)) == 1, len(rows)
    for i in range(len(rows)):
        add(*rows[(i * stride) % len(rows)])
    return torch.tensor(n, dtype=torch.complex64), torch.tensor(c, dtype=torch.complex64)


@functools.lru_cache(maxsize=None)
def _target_pool():
    n0, c0 = _crafted()
    m = max(TARGET_SIZES) - n0.numel()
    gen = torch.Generator().manual_seed(77)
    nz = torch.view_as_complex(torch.randn(m, 2, generator=gen))
    cl = torch.view_as_complex(torch.randn(m, 2, generator=gen))
    return torch.cat([n0, nz]), torch.cat([c0, cl])


def target_inputs(n):
    """(noisy, clean) complex64 [n]."""
    nz, cl = _target_pool()
    return nz[:n].clone(), cl[:n].clone()


def cirm_ratio64(noisy, clean):
    """The uncompressed ratio mask [n, 2] in float64 (oracle.fullsubnet.build_cirm before its clamp)."""
    n, c = noisy.to(torch.complex128), clean.to(torch.complex128)
    den = n.real ** 2 + n.imag ** 2 + ofsn.EPSILON
    return torch.stack(((n.real * c.real + n.imag * c.imag) / den, (n.real * c.imag - n.imag * c.real) / den), -1)


def target_masks(noisy, clean):
    """{arm: bool mask}.  The geometry and magnitude arms are over bins [n]; the cIRM arms over components [n, 2] and disjoint, in the order of
    CIRM_ARMS: a component of a bin with noisy == 0 is `noisy_zero`, else `clamp` / `saturate` by its float64 ratio, else `eps_decides`, else
    `cancels`: nr * cr + ni * ci (or nr * ci - ni * cr) below 1 / CANCELS of its terms.  float32 loses that factor there whatever the order of
    the operations (the clean side of a clamp or saturation member is 1e5 x the noisy one, and its OTHER component is such a difference), so
    these components have a bar of their own and do not set the bar of the rest."""
    nr, ni = noisy.real.double(), noisy.imag.double()
    neg0 = torch.signbit(noisy.imag)
    mag = torch.sqrt(nr * nr + ni * ni)
    m = {"zero": (nr == 0) & (ni == 0) & ~torch.signbit(noisy.real),
         "neg_real_pos0": (ni == 0) & ~neg0 & ((nr < 0) | ((nr == 0) & torch.signbit(noisy.real))),
         "neg_real_neg0": (ni == 0) & neg0 & ((nr < 0) | ((nr == 0) & torch.signbit(noisy.real))),
         "pos_real": (ni == 0) & (nr > 0), "pos_imag": (nr == 0) & (ni > 0), "neg_imag": (nr == 0) & (ni < 0),
         "q1": (nr > 0) & (ni > 0), "q2": (nr < 0) & (ni > 0), "q3": (nr < 0) & (ni < 0), "q4": (nr > 0) & (ni < 0)}
    for k in DECADES:
        m[f"mag_1e{k}"] = (mag >= 10.0 ** k) & ((mag < 10.0 ** (k + 1)) | ((k == DECADES[-1]) & (mag <= 1e3 * (1 + 1e-6))))
    ratio = cirm_ratio64(noisy, clean)
    nzero = ((mag == 0) & (clean.abs() > 0))[:, None].expand(-1, 2)
    clamp = ~nzero & (ratio <= -100.0)
    sat = ~nzero & (ratio >= SATURATE_FROM)
    epsd = ~nzero & ~clamp & ~sat & ((mag * mag >= EPS32 / 4) & (mag * mag <= EPS32 * 4))[:, None].expand(-1, 2)
    cr, ci = clean.real.double(), clean.imag.double()
    terms = torch.stack(((nr * cr).abs() + (ni * ci).abs(), (nr * ci).abs() + (ni * cr).abs()), -1)
    sums = torch.stack(((nr * cr + ni * ci).abs(), (nr * ci - ni * cr).abs()), -1)
    canc = ~(nzero | clamp | sat | epsd) & (terms > CANCELS * sums)
    m.update(clamp=clamp, saturate=sat, eps_decides=epsd, noisy_zero=nzero, cancels=canc, **{"else": ~(nzero | clamp | sat | epsd | canc)})
    return m


def target_census(noisy, clean):
    return {k: int(v.sum()) for k, v in target_masks(noisy, clean).items()}


TargetRef = namedtuple("TargetRef", "mag phase cirm cirm32 phase_alone phase_bar cirm_alone cirm_bar masks")
TARGET_MARGIN = 4.0


@functools.lru_cache(maxsize=None)
def target_reference(n):
    """float64 references of the first n bins; the phase and cIRM bars are taken over the LARGEST case, which holds every other as a prefix:
    4 x the worst distance of float32 torch.angle / float32 build_cirm to float64 (cIRM: per arm of CIRM_ARMS)."""
    noisy, clean = target_inputs(n)
    n128, c128 = noisy.to(torch.complex128), clean.to(torch.complex128)
    mag, phase, cirm = n128.abs(), torch.angle(n128), ofsn.build_cirm(n128, c128)
    cirm32 = ofsn.build_cirm(noisy, clean)
    masks = target_masks(noisy, clean)
    if n != max(TARGET_SIZES):
        big = target_reference(max(TARGET_SIZES))
        return TargetRef(mag, phase, cirm, cirm32, big.phase_alone, big.phase_bar, big.cirm_alone, big.cirm_bar, masks)
    phase_alone = float((torch.angle(noisy).double() - phase).abs().max())
    cirm_alone = {a: float((cirm32.double() - cirm)[masks[a]].abs().max()) for a in CIRM_ARMS}
    return TargetRef(mag, phase, cirm, cirm32, phase_alone, TARGET_MARGIN * phase_alone, cirm_alone,
                     {a: TARGET_MARGIN * v for a, v in cirm_alone.items()}, masks)


# ------------------------------------------------------------------------------------------ decompress_cIRM
LIMIT = 9.9
DECOMPRESS_REL = 1e-6                          # against float64 where float32 can give it: |out| >= 6 (|mask| >= 3)
# below that the quotient's rounding alone is 10 x 1.5 eps32 absolute, whatever the output (K x log of a ratio within 1.5 eps): an absolute bar
DECOMPRESS_ABS_SMALL = 10 * 4 * EPS32


def decompress_inputs():
    """{arm: float32 masks}: `upper` (>= limit, 9.9 itself first), `lower`, `inner` (3 <= |mask| < limit) and `small` (|mask| < 3, with 0)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    inner = torch.cat([torch.linspace(3.0, 9.89, 97), f([9.899, 9.8999, 3.0, 5.0, 7.5])])
    small = torch.cat([torch.linspace(-2.99, 2.99, 61), f([0.0, 1e-3, -1e-3, 1e-6])])
    up = f([9.9, 9.9000006, 9.95, 10.0, 10.5, 100.0, 1e6])
    return {"upper": up, "lower": -up, "inner": torch.cat([inner, -inner]), "small": small}


def decompress_reference(mask):
    return ofsn.decompress_cirm(mask.double())
