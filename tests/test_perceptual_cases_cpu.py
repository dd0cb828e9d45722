"""CPU tier of the perceptual-loss case table (perceptual_cases.py): are the cases good enough to hold csrc/pmsqe.hip and csrc/lms.hip to?

Everything asserted here is a CONDITION on the inputs, evaluated with the oracle alone: that the PMSQE cases visit every branch the kernel's
hand-derived gradient has an arm for, that the PIT choice is not a near-tie, that float32 alone stays far enough from the bars for a miss to mean
the kernel, and that a gradient with ONE wrong arm (oracle.pmsqe.MUTANTS) could not pass the GPU tier.  A case that misses a condition gets
another seed; the bound stays.  The measured figures are printed and written to the report directory."""
import numpy as np
import pytest
import torch

import perceptual_cases as pc
from oracle import losses as ol
from oracle import pmsqe
from test_gpu_pmsqe import TOL_GRAD, TOL_LOSS

MIN_MEMBERS = 3
MIN_GAP = 1e-2


def _report(name, lines):
    from plan_check import report_path
    print("\n".join(lines))
    with open(report_path(name), "w") as f:
        f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("power", [False, True], ids=["mag", "power"])
def test_pmsqe_cases_visit_every_branch(power):
    """Every arm of the census has at least 3 members in the union of the mode's cases.  The one exception is the gain ratio below 3e-4 in
    magnitude mode: it needs a reference frame without audible power against a degraded frame above 1.6e7, and on magnitudes the SLL-scaled
    Bark spectrum of these inputs never gets there (0 members; power mode reaches it in hundreds of frames, asserted below all the same)."""
    total = dict.fromkeys(pmsqe.CENSUS_ARMS, 0)
    for c in pc.PMSQE_CASES:
        if c.power == power:
            for k, v in pc.pmsqe_reference(c).census.items():
                total[k] += v
    print(total)
    for arm, n in total.items():
        if arm == "gain_below" and not power:
            continue
        assert n >= MIN_MEMBERS, (arm, n)
    if power:
        assert total["gain_below"] >= 100


@pytest.mark.parametrize("power", [False, True], ids=["mag", "power"])
def test_pmsqe_cases_take_a_permutation_that_is_not_the_identity(power):
    seen = set()
    for c in pc.PMSQE_CASES:
        if c.power == power and c.S > 1:
            perm = pc.pmsqe_reference(c).perm
            assert perm.shape == (c.B, c.S) and all(sorted(p) == list(range(c.S)) for p in perm.tolist())
            if any(p != list(range(c.S)) for p in perm.tolist()):
                seen.add(c.S)
    assert seen == {2, 3, 4, 5, 6}, seen                 # in fact every S of the table, so every walk of the factorial decoding ends off the identity


@pytest.mark.parametrize("case", pc.PMSQE_CASES, ids=pc.pmsqe_id)
def test_pmsqe_case_is_well_conditioned(case):
    """Permutation gap >= 1e-2 relative; float32 alone within a tenth of TOL_LOSS on the value and within 1e-3 on the gradient (batch and worst
    second - the damaged inputs measure up to 6.3e-4 / 6.5e-4 (B3-S6-power 9.4e-4 on another host: a float32 rounding that flips one of the
    loss's hard thresholds moves the figure), the plain ones 1.4e-5 / 7.9e-5, so a tenth of TOL_GRAD cannot hold here and the
    GPU bar is max(TOL_GRAD, 3 x the case's figure) instead); no second without gradient."""
    r = pc.pmsqe_reference(case)
    _report(f"perceptual_cpu_{pc.pmsqe_id(case)}.txt",
            [f"{pc.pmsqe_id(case)}: value {r.value:.6f} gap {float(r.gap.min()):.2e} | float32 alone value {r.alone_value:.2e} grad batch "
             f"{r.alone_batch:.2e} worst second {r.alone_second:.2e} | GPU gradient bar {r.grad_bar:.2e}", f"census {r.census}"])
    assert float(r.gap.min()) >= MIN_GAP, r.gap
    assert r.alone_value <= 0.1 * TOL_LOSS, r.alone_value
    assert r.alone_batch <= pc.PMSQE_ALONE_CAP and r.alone_second <= pc.PMSQE_ALONE_CAP, (r.alone_batch, r.alone_second)
    assert r.grad_bar == max(TOL_GRAD, 3 * max(r.alone_batch, r.alone_second))
    assert float(r.grad.reshape(case.B, case.S, pc.FS)[:, :, 15872:].abs().max()) == 0.0


@pytest.mark.parametrize("mutant", pmsqe.MUTANTS)
def test_pmsqe_cases_see_a_gradient_with_one_wrong_arm(mutant):
    """The mutant has the value of the loss and ONE arm of its gradient changed.  Some case must put its float64 gradient more than 3 GPU bars
    from the true float64 gradient in the per-second metric of the GPU tier, or a kernel with that bug would pass."""
    seen = []
    for c in pc.PMSQE_CASES:
        if c.B > 16:
            continue
        r = pc.pmsqe_reference(c)
        v, g = pc.pmsqe_mutant_grad(c, mutant)
        assert abs(v - r.value) <= 1e-12 * abs(r.value), "a mutant changes the gradient only"
        seen.append((pc.pmsqe_id(c), pc.per_second_err(g, r.grad, c.S) / r.grad_bar))
        if seen[-1][1] > 3.0:
            break
    print(mutant, seen)
    assert seen[-1][1] > 3.0, (mutant, seen)


def test_pmsqe_oracle_follows_its_input_dtype():
    c, e = pc.pmsqe_waves(2, 1, 41, True)
    for dt in (torch.float32, torch.float64):
        assert pmsqe.spectra(e.to(dt)).dtype == dt and pmsqe.pairwise(e.to(dt), c.to(dt)).dtype == dt
        assert pmsqe.pmsqe_loss(c, e, dtype=dt).dtype == dt
    assert pmsqe.pmsqe_loss(c, e).dtype == torch.float64                       # the default, whatever comes in
    with pytest.raises(ValueError):
        pmsqe.single_src_pmsqe(pmsqe.spectra(e.double()), pmsqe.spectra(c.double()), mutant="no_such_arm")


# ------------------------------------------------------------------------------------------ LMS
@pytest.mark.parametrize("spectra", [True, False], ids=["spectra", "magnitudes"])
@pytest.mark.parametrize("case", pc.LMS_CASES, ids=pc.lms_id)
def test_lms_reference_alone(case, spectra):
    """oracle.losses.lms_loss in float32 against float64 at a tenth of the bars of the GPU tier (measured: value <= 1.3e-7, gradient <= 5.9e-7)."""
    r = pc.lms_reference(case, spectra)
    print(f"{pc.lms_id(case)} {'spectra' if spectra else 'magnitudes'}: value {r.value:.6f} float32 alone value {r.alone_value:.2e} grad {r.alone_grad:.2e}")
    assert all(g.dtype == torch.float64 and torch.isfinite(g).all() for g in r.grads)
    assert r.alone_value <= 0.1 * pc.LMS_VALUE_BAR and r.alone_grad <= 0.1 * pc.LMS_GRAD_BAR, (r.alone_value, r.alone_grad)
    if not spectra and case.kind == "zeros":
        assert int((pc.lms_magnitudes(case)[1] == 0).sum()) > 0


@pytest.mark.parametrize("nfft", [256, 512, 1024])
def test_lms_band_table_is_the_oracle_bank(nfft):
    """The sparse (first bin, taps, offset, scale) rows the kernel reads, densified, are melFilterBank exactly; no row reaches past the bins."""
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_loss as tfl
    rows, taps = tfl._band_table(nfft)
    taps = np.asarray(taps, np.float32)
    nbins = nfft // 2 + 1
    assert len(rows) == sum(tfl.MEL_SCALES) and [r[3] for r in rows] == [si for si, nb in enumerate(tfl.MEL_SCALES) for _ in range(nb)]
    at, empty = 0, 0
    for si, nb in enumerate(tfl.MEL_SCALES):
        dense = np.zeros((nbins, nb), np.float32)
        for k, (lo, n, off, _) in enumerate(rows[at:at + nb]):
            assert 0 <= lo and lo + n <= nbins and 0 <= off and off + n <= len(taps)
            dense[lo:lo + n, k] = taps[off:off + n]
        want = ol.mel_filter_bank(nb, nfft)
        assert np.array_equal(dense, want), (nfft, nb)
        for k, (lo, n, off, _) in enumerate(rows[at:at + nb]):
            if not want[:, k].any():
                assert n == 0
                empty += 1
        at += nb
    assert empty == (6 if nfft == 256 else 0), empty       # at 256 the 64-band bank has bands between two equal floor-binned edges


def test_pmsqe_device_tables_are_the_oracle_constants():
    """The float / int tables handed to csrc/pmsqe.hip against oracle.pmsqe.constants() and stft_filters(), to float32 rounding.  Needs the
    built library for the table size only; nothing runs on a GPU."""
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_loss as tfl
    tab, itab = (t.numpy() for t in tfl._pmsqe_tables("cpu"))
    thr, zp, width, M, mask = (t.numpy() for t in pmsqe.constants())
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    corr = np.array(pmsqe.T_.POW_DENS_CORRECTION)
    aterm = pmsqe.T_.SL_16K * (thr / 0.5) ** zp
    for off, want in ((0, thr), (49, zp), (98, width), (147, corr), (196, aterm), (245, mask)):
        assert np.array_equal(tab[off:off + len(want)], f32(want)), off
    C, S = (t.numpy() for t in pmsqe.stft_filters())          # [257][512]
    n = C.size
    for k, want in enumerate((C.T, S.T, C, S)):               # cos / -sin [512][257], then their transposes
        got = tab[512 + k * n:512 + (k + 1) * n].reshape(want.shape)
        assert np.abs(got - f32(want)).max() <= 2.0 ** -24 * np.abs(want).max(), k
    lo = np.concatenate([[0], np.cumsum(pmsqe.T_.HZ_BINS_PER_BAND)])
    assert np.array_equal(itab[:50], lo)
    band_of = np.full(257, -1)
    for k in range(49):
        band_of[lo[k]:lo[k + 1]] = k
        assert np.all(M[lo[k]:lo[k + 1], k] == corr[k]) and np.count_nonzero(M[:, k]) == lo[k + 1] - lo[k]
    assert np.array_equal(itab[64:64 + 257], band_of)
    assert float(np.float32(pmsqe.T_.SP_16K)) == float(np.float32(6.910853e-006))       # the SP constant compiled into the kernel
