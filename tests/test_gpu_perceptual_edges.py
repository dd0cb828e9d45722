"""GPU tier: the two perceptual losses - csrc/pmsqe.hip and csrc/lms.hip - at their branches and edges, against the float64 oracle
(oracle/pmsqe.py, oracle.losses.lms_loss + autograd) on the case table of perceptual_cases.py.  test_perceptual_cases_cpu.py shows, without a
GPU, that the table visits every branch the PMSQE gradient has an arm for, that its PIT choices are no near-ties, what float32 alone costs on every
case, and that a gradient with one wrong arm misses the bars used here by more than a factor of 3.

Every case runs twice: through the C ABI with every written buffer between sentinels (`Guarded` of test_gpu_loss_edges.py) and through
tools_for_loss with an upstream gradient of 0.5.

Bars.  PMSQE: value TOL_LOSS of test_gpu_pmsqe.py; gradient, as relative L2 of the batch AND of the worst single second, max(TOL_GRAD, 3 x the
case's float32-alone figure) - the figure is measured on the oracle in torch float32, never on the kernel, and the 3 covers a summation order
other than torch's.  LMS: value 1e-4 relative and gradient 1e-3 (test_gpu_model.py), the gradient as relative L2 and as max-abs over max.
The figures of every case are printed and written to the report directory."""
import ctypes as C

import pytest
import torch

import perceptual_cases as pc
from test_gpu_loss_edges import Guarded
from test_gpu_pmsqe import TOL_LOSS

pytestmark = pytest.mark.gpu

T_FRAMES, NBINS, NB = 61, 257, 49           # csrc/pmsqe.hip


def _tfl():
    import sefd_amd  # noqa: F401
    from sefd_amd import _lib, config as cfg, tools_for_loss as tfl
    return _lib.lib(), cfg, tfl


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _report(name, lines):
    from plan_check import report_path
    print("\n".join(lines))
    with open(report_path(name), "w") as f:
        f.write("\n".join(lines) + "\n")


def _sel_offset(B, S):
    """Float offset of the chosen-permutation region in the PMSQE workspace (`carve` of csrc/pmsqe.hip)."""
    BS = B * S
    return BS * T_FRAMES * NBINS * 2 + 2 * BS * T_FRAMES * NB + 2 * BS * T_FRAMES + BS * S + BS * T_FRAMES * NB + BS + B


# ------------------------------------------------------------------------------------------ PMSQE
@pytest.mark.parametrize("case", pc.PMSQE_CASES, ids=pc.pmsqe_id)
def test_pmsqe_kernels_on_the_case_table(case):
    """Measured on the MI355X, kernel against float64 (value / gradient of the batch / worst second; C ABI and tools_for_loss agree to the digits
    shown), with the float32-alone figures of the oracle beside them:
      B2-S1-mag            kernel 8.0e-08 / 2.5e-04 / 2.5e-04   float32 alone 3.6e-08 / 2.8e-04 / 2.8e-04   bar 2.0e-03
      B3-S2-mag            kernel 2.6e-08 / 2.0e-04 / 2.4e-04   float32 alone 4.3e-08 / 2.2e-04 / 2.6e-04   bar 2.0e-03
      B3-S3-mag            kernel 1.1e-08 / 2.5e-04 / 2.8e-04   float32 alone 1.3e-07 / 2.8e-04 / 3.2e-04   bar 2.0e-03
      B2-S4-mag            kernel 4.1e-08 / 6.4e-05 / 8.6e-05   float32 alone 2.2e-08 / 7.1e-05 / 9.7e-05   bar 2.0e-03
      B1-S5-mag            kernel 6.8e-08 / 7.5e-05 / 1.6e-04   float32 alone 6.8e-08 / 8.5e-05 / 1.8e-04   bar 2.0e-03
      B3-S6-mag            kernel 3.5e-08 / 1.4e-04 / 1.8e-04   float32 alone 3.1e-08 / 1.6e-04 / 2.2e-04   bar 2.0e-03
      B2-S1-power          kernel 3.0e-08 / 5.5e-04 / 5.5e-04   float32 alone 3.0e-08 / 6.0e-04 / 6.0e-04   bar 2.0e-03
      B3-S2-power          kernel 3.8e-08 / 4.9e-04 / 5.6e-04   float32 alone 4.8e-08 / 5.6e-04 / 6.1e-04   bar 2.0e-03
      B3-S3-power          kernel 8.6e-08 / 4.4e-04 / 4.6e-04   float32 alone 8.6e-08 / 5.0e-04 / 5.2e-04   bar 2.0e-03
      B2-S4-power          kernel 1.9e-08 / 4.0e-05 / 7.5e-05   float32 alone 1.9e-08 / 4.5e-05 / 8.6e-05   bar 2.0e-03
      B1-S5-power          kernel 1.8e-08 / 6.3e-05 / 9.4e-05   float32 alone 8.9e-08 / 7.2e-05 / 1.1e-04   bar 2.0e-03
      B3-S6-power          kernel 3.1e-08 / 2.9e-04 / 4.1e-04   float32 alone 5.1e-08 / 5.4e-04 / 9.4e-04   bar 2.8e-03
      B257-S1-mag-plain    kernel 5.1e-08 / 1.3e-05 / 1.0e-04   float32 alone 2.1e-08 / 1.3e-05 / 6.5e-05   bar 2.0e-03
      B257-S1-power-plain  kernel 1.3e-08 / 6.2e-06 / 7.1e-05   float32 alone 1.3e-08 / 4.4e-06 / 3.4e-05   bar 2.0e-03
    The permutation read from the workspace equals the oracle's in every case."""
    L_, cfg, tfl = _tfl()
    B, S, L = case.B, case.S, case.S * pc.FS
    r = pc.pmsqe_reference(case)
    c, e = pc.pmsqe_waves(case.B, case.S, case.seed, case.damaged)
    cd, ed = c.cuda(), e.cuda()
    tab, itab = tfl._pmsqe_tables(ed.device)
    n = L_.sefd_pmsqe_ws_floats(B, L)
    assert n >= _sel_offset(B, S) + B * S
    ws, out, g = Guarded(n), Guarded(1), Guarded(B * L)
    assert L_.sefd_pmsqe_forward(_vp(ed), _vp(cd), B, L, int(case.power), _vp(tab), _vp(itab), ws.ptr, out.ptr, None) == 0
    assert L_.sefd_pmsqe_backward(B, L, int(case.power), _vp(tab), _vp(itab), ws.ptr, None, g.ptr, None) == 0
    for b in (ws, out, g):
        b.check()
    val, grad = float(out.t[0]), g.t.view(B, L).cpu()
    sel = ws.t[_sel_offset(B, S):_sel_offset(B, S) + B * S].view(torch.int32).view(B, S).cpu()
    # the same through the autograd wrapper, upstream gradient 0.5
    old = getattr(cfg, "pmsqe_power", False)
    cfg.pmsqe_power = case.power
    try:
        em = ed.clone().requires_grad_()
        lm = tfl.get_array_pmsqe_loss(cd, em)
        (lm * 0.5).backward()
    finally:
        cfg.pmsqe_power = old
    valm, gradm = float(lm.detach()), em.grad.cpu()
    ev, evm = abs(val - r.value) / abs(r.value), abs(valm - r.value) / abs(r.value)
    eb, es = pc.batch_err(grad, r.grad), pc.per_second_err(grad, r.grad, S)
    ebm, esm = pc.batch_err(gradm, 0.5 * r.grad), pc.per_second_err(gradm, 0.5 * r.grad, S)
    _report(f"perceptual_gpu_pmsqe_{pc.pmsqe_id(case)}.txt",
            [f"{pc.pmsqe_id(case)}: float32 alone value {r.alone_value:.1e} batch {r.alone_batch:.1e} second {r.alone_second:.1e} | bar {r.grad_bar:.1e} | "
             f"kernel value {ev:.1e} batch {eb:.1e} second {es:.1e} | tools_for_loss value {evm:.1e} batch {ebm:.1e} second {esm:.1e}"])
    assert ev <= TOL_LOSS and evm <= TOL_LOSS, (val, valm, r.value)
    assert torch.equal(sel.long(), r.perm), (sel, r.perm)
    assert eb < r.grad_bar and es < r.grad_bar, (eb, es, r.grad_bar)
    assert ebm < r.grad_bar and esm < r.grad_bar, (ebm, esm, r.grad_bar)
    # the last 128 samples of every second are in no frame
    assert float(grad.reshape(B, S, pc.FS)[:, :, 15872:].abs().max()) == 0.0 and float(gradm.reshape(B, S, pc.FS)[:, :, 15872:].abs().max()) == 0.0


def test_pmsqe_still_refuses_seven_seconds_and_broken_seconds():
    L_, cfg, tfl = _tfl()
    tab, itab = tfl._pmsqe_tables(torch.device("cuda"))
    x = torch.zeros(1, 7 * pc.FS, device="cuda")
    ws, out, g = Guarded(4096), Guarded(1), Guarded(7 * pc.FS)
    for L in (7 * pc.FS, pc.FS + 4000, pc.FS - 1, 0):
        assert L_.sefd_pmsqe_ws_floats(1, L) == -1
        assert L_.sefd_pmsqe_forward(_vp(x), _vp(x), 1, L, 0, _vp(tab), _vp(itab), ws.ptr, out.ptr, None) == -1
        assert L_.sefd_pmsqe_backward(1, L, 0, _vp(tab), _vp(itab), ws.ptr, None, g.ptr, None) == -1
        if L:
            with pytest.raises(ValueError):
                tfl.get_array_pmsqe_loss(x[:, :L], x[:, :L])
    assert L_.sefd_pmsqe_ws_floats(0, pc.FS) == -1
    assert ws.untouched() and out.untouched() and g.untouched()


# ------------------------------------------------------------------------------------------ LMS
def _lms_abi(L_, tfl, case, ins):
    """forward + backward through the C ABI; ins = (clean_r, clean_i, est_r, est_i) on the device, the *_i None for the magnitude signature."""
    cr, ci, er, ei = ins
    B, NF, T = er.shape
    bands, weights, nbands, sizes, extent = tfl._banks(er.device, case.nfft)
    ws, out, gr, gi = Guarded(B * T), Guarded(1), Guarded(B * NF * T), (Guarded(B * NF * T) if ei is not None else None)
    assert L_.sefd_lms_forward(_vp(cr), _vp(ci), _vp(er), _vp(ei), B, NF, T, _vp(bands), _vp(weights), nbands, extent, sizes, len(tfl.MEL_SCALES),
                               case.nfft, ws.ptr, out.ptr, None) == 0
    assert L_.sefd_lms_backward(_vp(cr), _vp(ci), _vp(er), _vp(ei), B, NF, T, _vp(bands), _vp(weights), nbands, extent, sizes, len(tfl.MEL_SCALES),
                                case.nfft, None, gr.ptr, gi.ptr if gi else None, None) == 0
    for b in (ws, out, gr) + ((gi,) if gi else ()):
        b.check()
    return float(out.t[0]), tuple(b.t.view(B, NF, T).cpu() for b in ((gr, gi) if gi else (gr,)))


@pytest.mark.parametrize("spectra", [True, False], ids=["spectra", "magnitudes"])
@pytest.mark.parametrize("case", pc.LMS_CASES, ids=pc.lms_id)
def test_lms_kernels_on_the_case_table(case, spectra):
    """Measured on the MI355X, kernel against float64 (value relative; gradient relative L2 / max-abs over max, the worst output;
    the worst of the three input kinds and both signatures per shape, the per-case lines are in the report files):
      fft512-B1-T1     kernel 2.0e-07 / 6.9e-07 / 6.4e-07   float32 alone 1.2e-07 / 4.5e-07
      fft512-B2-T7     kernel 1.5e-07 / 3.0e-07 / 3.3e-07   float32 alone 4.3e-08 / 2.6e-07
      fft512-B1-T300   kernel 6.7e-08 / 3.1e-07 / 2.1e-07   float32 alone 6.3e-08 / 2.6e-07
      fft256-B2-T7     kernel 1.3e-07 / 1.9e-07 / 2.3e-07   float32 alone 8.0e-08 / 1.6e-07
      fft1024-B2-T5    kernel 1.1e-07 / 8.4e-07 / 8.7e-07   float32 alone 9.2e-08 / 5.2e-07"""
    L_, cfg, tfl = _tfl()
    r = pc.lms_reference(case, spectra)
    if spectra:
        ins = tuple(t.cuda() for t in pc.lms_inputs(case))
    else:
        cm, em = pc.lms_magnitudes(case)
        assert case.kind != "zeros" or int((em == 0).sum()) > 0
        ins = (cm.cuda(), None, em.cuda(), None)
    val, grads = _lms_abi(L_, tfl, case, ins)
    old = cfg.fft_len
    cfg.fft_len = case.nfft
    try:
        leaves = [t.clone().requires_grad_() for t in ins[2:] if t is not None]
        lm = tfl.lms_from_spectra(ins[0], ins[1], *leaves) if spectra else tfl.get_array_lms_loss(ins[0], leaves[0])
        (lm * 0.5).backward()
    finally:
        cfg.fft_len = old
    valm, gradsm = float(lm.detach()), tuple(t.grad.cpu() for t in leaves)
    ev, evm = abs(val - r.value) / abs(r.value), abs(valm - r.value) / abs(r.value)
    eg = tuple(max(pc.grad_errs(g, ref)[k] for g, ref in zip(grads, r.grads)) for k in (0, 1))
    egm = tuple(max(pc.grad_errs(g, 0.5 * ref)[k] for g, ref in zip(gradsm, r.grads)) for k in (0, 1))
    _report(f"perceptual_gpu_lms_{pc.lms_id(case)}_{'spectra' if spectra else 'magnitudes'}.txt",
            [f"{pc.lms_id(case)} {'spectra' if spectra else 'magnitudes'}: float32 alone value {r.alone_value:.1e} grad {r.alone_grad:.1e} | kernel value {ev:.1e} "
             f"grad L2 {eg[0]:.1e} max {eg[1]:.1e} | tools_for_loss value {evm:.1e} grad L2 {egm[0]:.1e} max {egm[1]:.1e}"])
    assert ev < pc.LMS_VALUE_BAR and evm < pc.LMS_VALUE_BAR, (val, valm, r.value)
    assert max(eg) < pc.LMS_GRAD_BAR and max(egm) < pc.LMS_GRAD_BAR, (eg, egm)


def test_lms_refuses_arrays_that_do_not_match_the_band_table():
    """NF must be cfg.fft_len // 2 + 1: with fewer bins the band rows index past what the kernel staged (uninitialised LDS) and the call used to
    return a number.  The wrapper raises; the C entry points return -1 for a table that reaches past NF and for NF, T, B <= 0, and write nothing."""
    L_, cfg, tfl = _tfl()
    assert cfg.fft_len == 512
    x = torch.rand(2, 129, 4, device="cuda")
    with pytest.raises(ValueError):
        tfl.get_array_lms_loss(x, x.clone().requires_grad_())
    with pytest.raises(ValueError):
        tfl.lms_from_spectra(x, x, x.clone().requires_grad_(), x.clone().requires_grad_())
    bands, weights, nbands, sizes, extent = tfl._banks(x.device, 512)
    assert extent == 257
    ws, out, gr, gi = Guarded(8), Guarded(1), Guarded(x.numel()), Guarded(x.numel())
    for B, NF, T, ext in ((2, 129, 4, extent), (2, 256, 2, extent), (2, 0, 4, 0), (2, 129, 0, 129), (0, 129, 4, 129), (2, 129, 4, -1), (2, 1025, 1, 257)):
        assert L_.sefd_lms_forward(_vp(x), _vp(x), _vp(x), _vp(x), B, NF, T, _vp(bands), _vp(weights), nbands, ext, sizes, 3, 512, ws.ptr, out.ptr, None) == -1
        assert L_.sefd_lms_backward(_vp(x), _vp(x), _vp(x), _vp(x), B, NF, T, _vp(bands), _vp(weights), nbands, ext, sizes, 3, 512, None, gr.ptr, gi.ptr, None) == -1
    assert ws.untouched() and out.untouched() and gr.untouched() and gi.untouched()
