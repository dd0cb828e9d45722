"""The case table of the two perceptual losses (csrc/pmsqe.hip, csrc/lms.hip), shared by the CPU tier (test_perceptual_cases_cpu.py: are the
cases any good?) and the GPU tier (test_gpu_perceptual_edges.py: do the kernels hold on them?).  Everything here is deterministic and runs on
the CPU from the oracle alone.

PMSQE.  A case is `speechlike(B, seconds=S, seed)` with the estimate damaged so that the loss leaves the branches plain noisy speech stays on:
  - two runs of 768 exact zeros in every second of every utterance (48 ms dropouts: whole frames without audible power -> gain clamp at 5),
  - utterance 0 low-passed to 1e-4 above 3.4 kHz (Bark equaliser clamp at 100),
  - utterance 1 with noise above 4.5 kHz added at half full scale (equaliser clamp at 0.01, asymmetry factor saturated at 12, frame caps of 45),
    as a burst over the first quarter of every second: laid over the whole second it pins nearly every frame of every pair to the caps in
    `power` mode, the pair losses of that utterance then differ by 1e-3 at most and no seed keeps the permutation apart (S = 6: the best of
    25 seeds gave a gap of 3.4e-3, most 1e-4) - the choice between near-ties is not something float32 can be held to,
  - the seconds of the last utterance permuted, so that the PIT choice is not the identity.
One plain `speechlike` case of 257 one-second utterances drives the strided utterance loop of the PIT kernel.
No case contains a digitally silent second: the SLL equalisation divides by the second's mean speech-band power, so the published algorithm
itself is 0 / 0 there in `power` mode (the 1e-8 under the magnitude's root only hides it in the default mode) - there is nothing to compare.

LMS.  fft_len x (B, T) x input kind.  The loss re-views the contiguous [B, NF, T] array as [B, T, NF] without transposing, so a
"frame" and a "bin" below are a row and a column of THAT view: they are what one workgroup of the kernel sees.
  - "randn":  randn * 3
  - "zeros":  the same with rows 0..2 of the estimate and rows 2..4 of the clean side exactly zero (as many of them as T has)
  - "range":  the same scaled by 10^(-4 .. 2) across the bins, reversed on the clean side
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import losses as ol
from oracle import pmsqe
from test_gpu_pmsqe import TOL_GRAD          # the bar of the existing PMSQE tier (a plain module: nothing of the GPU is imported)
from test_oracle_pmsqe import speechlike

FS = 16000
PmsqeCase = namedtuple("PmsqeCase", "B S power seed damaged")
# seeds: chosen so that every case keeps a permutation gap >= 1e-2 in both modes (test_perceptual_cases_cpu.py asserts it; a seed that misses
# is replaced, the bound stays): these measure 4.2e-2 (B3-S6-mag) to 5.9e-1
_DAMAGED = ((2, 1, 41), (3, 2, 59), (3, 3, 51), (2, 4, 53), (1, 5, 53), (3, 6, 61))
PMSQE_CASES = tuple(PmsqeCase(B, S, power, seed, True) for power in (False, True) for B, S, seed in _DAMAGED) + tuple(
    PmsqeCase(257, 1, power, 47, False) for power in (False, True))
NOISE_BURST = 4000               # samples of every second that carry the high-band noise of utterance 1
PMSQE_ALONE_CAP = 1e-3          # float32 evaluation of the oracle against float64, gradient, per case (batch and worst second)
PMSQE_MARGIN = 3.0              # the kernel sums in another order than torch float32


def pmsqe_id(c):
    return f"B{c.B}-S{c.S}-{'power' if c.power else 'mag'}{'' if c.damaged else '-plain'}"


def _second_perm(S, rng):
    """A permutation of the seconds with no fixed point left where S allows one (S >= 2): a rotation by a drawn amount."""
    return np.roll(np.arange(S), int(rng.integers(1, S)))


@functools.lru_cache(maxsize=None)
def pmsqe_waves(B, S, seed, damaged):
    """(clean, estimate) float32 [B, S * 16000]; the mode of the loss does not enter."""
    c, n = speechlike(B, seconds=S, seed=seed)
    if not damaged:
        return c, n
    rng = np.random.default_rng(1000 + seed)
    L = S * FS
    e = n.double().numpy().copy()
    f = np.fft.rfftfreq(L, 1.0 / FS)
    X = np.fft.rfft(e[0])
    X[f > 3400.0] *= 1e-4
    e[0] = np.fft.irfft(X, L)
    if B > 1:
        N = np.fft.rfft(rng.standard_normal(L))
        N[f < 4500.0] = 0.0
        hp = np.fft.irfft(N, L) * (np.arange(L) % FS < NOISE_BURST)
        e[1] += 0.5 * hp / np.abs(hp).max()
    if S > 1:
        e[-1] = e[-1].reshape(S, FS)[_second_perm(S, rng)].reshape(-1)
    for b in range(B):
        for s in range(S):
            for start in (int(rng.integers(256, 7000)), int(rng.integers(8000, FS - 768 - 256))):
                e[b, s * FS + start:s * FS + start + 768] = 0.0
    e = np.clip(e, -1.0, 1.0)
    assert all(np.abs(e[b, s * FS:(s + 1) * FS]).max() > 1e-2 for b in range(B) for s in range(S)), "a silent second"
    return c, torch.tensor(e, dtype=torch.float32)


def per_second_err(g, ref, S):
    """Relative L2 of the gradient second by second ([B, S * 16000] -> the worst of the B * S figures): an error confined to one second
    cannot hide behind the others as it can in the figure of the whole batch."""
    d = (g.double() - ref.double()).reshape(-1, FS).norm(dim=1)
    n = ref.double().reshape(-1, FS).norm(dim=1)
    assert float(n.min()) > 0.0, "a second without gradient: the case cannot hold the kernel there"
    return float((d / n).max())


def batch_err(g, ref):
    return float((g.double() - ref.double()).norm() / ref.double().norm())


PmsqeRef = namedtuple("PmsqeRef", "value grad perm gap census alone_value alone_batch alone_second grad_bar")


def _eval(case, dtype, mutant=None, details=False):
    c, e = pmsqe_waves(case.B, case.S, case.seed, case.damaged)
    ev = e.to(dtype).clone().requires_grad_()
    out = pmsqe.pmsqe_loss(c, ev, case.power, dtype=dtype, mutant=mutant, details=details)
    loss, info = out if details else (out, None)
    loss.backward()
    return float(loss.detach()), ev.grad, info


@functools.lru_cache(maxsize=None)
def pmsqe_reference(case):
    """float64 oracle of the case and what float32 alone costs on it (the same formulas in torch float32 on the CPU, measured against float64
    - never a kernel).  grad_bar = max(TOL_GRAD, 3 * the float32-alone figure) is the bar of the GPU tier for both gradient metrics."""
    v, g, info = _eval(case, torch.float64, details=True)
    v32, g32, _ = _eval(case, torch.float32)
    ab, asec = batch_err(g32, g), per_second_err(g32, g, case.S)
    return PmsqeRef(v, g, info["perm"], info["gap"], info["census"], abs(v32 - v) / abs(v), ab, asec,
                    max(TOL_GRAD, PMSQE_MARGIN * max(ab, asec)))


def pmsqe_mutant_grad(case, mutant):
    v, g, _ = _eval(case, torch.float64, mutant=mutant)
    return v, g


# ------------------------------------------------------------------------------------------ LMS
LmsCase = namedtuple("LmsCase", "nfft B T kind")
LMS_SHAPES = ((512, 1, 1), (512, 2, 7), (512, 1, 300), (256, 2, 7), (1024, 2, 5))      # T = 1; B * T > 256: the reduction loops; 6 empty bands at 256
LMS_KINDS = ("randn", "zeros", "range")
LMS_CASES = tuple(LmsCase(nfft, B, T, kind) for nfft, B, T in LMS_SHAPES for kind in LMS_KINDS)
LMS_VALUE_BAR = 1e-4            # test_gpu_model.test_lms_loss_kernel_vs_oracle, relative
LMS_GRAD_BAR = 1e-3             # TOL of test_gpu_model.py


def lms_id(c):
    return f"fft{c.nfft}-B{c.B}-T{c.T}-{c.kind}"


@functools.lru_cache(maxsize=None)
def lms_inputs(case):
    """(clean_r, clean_i, est_r, est_i) float32 [B, NF, T]."""
    NF = case.nfft // 2 + 1
    gen = torch.Generator().manual_seed(case.nfft + 7 * case.T + case.B)
    cr, ci, er, ei = (torch.randn(case.B, NF, case.T, generator=gen) * 3 for _ in range(4))
    rows = lambda t: t.view(case.B, case.T, NF)                                   # the loss's own view of the array (Q8)
    if case.kind == "zeros":
        for t in (er, ei):
            rows(t)[:, 0:3] = 0.0
        for t in (cr, ci):
            rows(t)[:, 2:5] = 0.0
    if case.kind == "range":
        ramp = 10.0 ** torch.linspace(-4.0, 2.0, NF)
        for t in (er, ei):
            rows(t).mul_(ramp)
        for t in (cr, ci):
            rows(t).mul_(ramp.flip(0))
    return cr, ci, er, ei


def lms_magnitudes(case):
    """The inputs of the magnitude signature: plain sqrt(re^2 + im^2), float32, so the zero rows are exact zeros."""
    cr, ci, er, ei = lms_inputs(case)
    cm, em = torch.sqrt(cr.double() ** 2 + ci.double() ** 2).float(), torch.sqrt(er.double() ** 2 + ei.double() ** 2).float()
    if case.kind == "zeros":
        assert int((em == 0).sum()) >= case.nfft // 2 + 1 and (case.T < 3 or int((cm == 0).sum()) >= case.nfft // 2 + 1)
    return cm, em


def lms_eval(case, dtype, spectra):
    """Oracle value and gradient(s) w.r.t. the estimate in `dtype`: (value, (grad_r, grad_i)) from spectra, (value, (grad_mag,)) from magnitudes."""
    if spectra:
        cr, ci, er, ei = (t.to(dtype) for t in lms_inputs(case))
        er, ei = er.clone().requires_grad_(), ei.clone().requires_grad_()
        v = ol.lms_loss(torch.sqrt(cr ** 2 + ci ** 2 + 1e-7), torch.sqrt(er ** 2 + ei ** 2 + 1e-7), n_fft=case.nfft)
        v.backward()
        return float(v.detach()), (er.grad, ei.grad)
    cm, em = (t.to(dtype) for t in lms_magnitudes(case))
    em = em.clone().requires_grad_()
    v = ol.lms_loss(cm, em, n_fft=case.nfft)
    v.backward()
    return float(v.detach()), (em.grad,)


def grad_errs(g, ref):
    """(relative L2, max-abs over max) of a gradient against its reference; a reference that is zero everywhere holds the gradient absolutely."""
    g, ref = g.double(), ref.double()
    n, m = float(ref.norm()), float(ref.abs().max())
    return float((g - ref).norm()) / (n if n > 0 else 1.0), float((g - ref).abs().max()) / (m if m > 0 else 1.0)


LmsRef = namedtuple("LmsRef", "value grads alone_value alone_grad")


@functools.lru_cache(maxsize=None)
def lms_reference(case, spectra):
    """float64 oracle and the float32-alone figures (value relative, gradient the worse of the two measures over the outputs)."""
    v, gs = lms_eval(case, torch.float64, spectra)
    v32, gs32 = lms_eval(case, torch.float32, spectra)
    return LmsRef(v, gs, abs(v32 - v) / abs(v), max(max(grad_errs(a, b)) for a, b in zip(gs32, gs)))
