"""CPU tier of the front-end case table (frontend_cases.py): the TorchSTFT / TorchISTFT plans on the host simulator at the bars of the GPU tier
(which holds tests/hostsim/hostsim.cpp to what csrc/kernels.hip computes), the planners' refusals over a sweep of lengths against torch.istft
itself, and conditions on the cases: every arm of the target census has members, float32 alone stays inside the bars, and an overlap-add that
divides by `envelope + 1e-8` - what the torch-style plan did before it was told apart from ConviSTFT - could not pass the iSTFT bar.

Measured here (host simulator; the float32-alone figures are torch on the CPU and move with the host's FFT library):
  STFT   float32 torch alone 9.8e-8 .. 1.9e-7 of the largest bin (bars 3.9e-7 .. 7.7e-7); the simulator, which sums in double, <= 0.10 of its bar
  iSTFT  K_ref = 1.94 (float32 torch.istft in units of eps32 * A / env; 2.38 on another host), K = 7.75; simulator worst 1.21; the mutant
         misses K by 32 x .. 60 x (L = 6190), 1.5e4 x (6199), 1.0e5 x (6200); before the fix the simulator missed at every case from L = 6180 up
  sweep  torch refuses 347 of 1150 lengths at 300 / 400 (168 of them, L mod 300 in 201 .. 256, used to build), 888 at 512 / 512, none elsewhere
  census (n = 4194561) zero 6, negative real axis +0 / -0 14 / 13, axes 73 / 24 / 24, quadrants 1.05e6 each, decades 24 .. 2.5e6,
         clamp 339, saturate 189, eps_decides 153, noisy_zero 12, cancels 34209, else 8.35e6 components
"""
import pytest
import torch

import frontend_cases as fc
from simutil import PHASE_FWD, Plan, sim_run

MIN_MEMBERS = 3


def _report(name, lines):
    from plan_check import report_path
    print("\n".join(lines))
    with open(report_path(name), "w") as f:
        f.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------------------ STFT
@pytest.mark.parametrize("case", fc.STFT_CASES, ids=fc.stft_id)
def test_stft_plan_on_host_simulator(case):
    r = fc.stft_reference(case)
    plan = Plan(case.B, case.L, win_len=case.win, win_inc=case.hop, fft_len=case.nfft, model="TorchSTFT")
    T, NF = 1 + case.L // case.hop, case.nfft // 2 + 1
    assert plan.T == T and r.spec.shape == (case.B, NF, T)
    ar = plan.alloc_arenas("cpu")
    plan.io(ar, "wav", (case.B, case.L)).copy_(fc.stft_input(case))
    sim_run(plan, PHASE_FWD, ar)
    got = torch.view_as_complex(plan.io(ar, "spec", (case.B, NF, T, 2)).clone())
    err = fc.stft_err(got, r.spec)
    print(f"{fc.stft_id(case)}: float32 torch alone {r.alone:.2e} bar {r.bar:.2e} simulator {err:.2e} ({err / r.bar:.2f} of the bar)")
    assert r.alone <= 2.5e-7                                   # float32 alone: the 4 x margin is over a figure of float32's own size
    assert err <= r.bar, (err, r.bar)


def test_stft_plan_refuses_what_it_cannot_run():
    """One message per limit.  win_len > fft_len used to write in front of the window table; hop % 4 is this project's own limit and says so."""
    kw = dict(fft_len=512, model="TorchSTFT")
    with pytest.raises(ValueError, match=r"win_len 513 .*fft_len = 512"):
        Plan(2, 6000, win_len=513, win_inc=300, **kw)
    with pytest.raises(ValueError, match=r"win_len 600 .*fft_len = 512"):
        Plan(2, 6000, win_len=600, win_inc=300, **kw)
    for hop in (150, 301, 0):
        with pytest.raises(ValueError, match=rf"hop {hop} is not a positive multiple of 4.*torch\.stft has no such limit") as e:
            Plan(2, 6000, win_len=400, win_inc=hop, **kw)
        assert "win_len" not in str(e.value) and "fft_len/2" not in str(e.value)
    for L in (256, 100):
        with pytest.raises(ValueError, match=rf"clip of {L} samples is not longer than fft_len/2 = 256") as e:
            Plan(2, L, win_len=400, win_inc=300, **kw)
        assert "hop" not in str(e.value)
    assert Plan(2, 257, win_len=512, win_inc=4, **kw).T == 65


# ------------------------------------------------------------------------------------------ iSTFT
def _sim_istft(case, spec):
    plan = Plan(case.B, case.L, win_len=case.win, win_inc=case.hop, fft_len=fc.NFFT, model="TorchISTFT")
    assert plan.T == spec.shape[-1]
    ar = plan.alloc_arenas("cpu")
    plan.io(ar, "spec", (case.B, fc.NFFT // 2 + 1, plan.T, 2)).copy_(torch.view_as_real(spec))
    sim_run(plan, PHASE_FWD, ar)
    return plan.io(ar, "wav", (case.B, case.L)).clone()


@pytest.mark.parametrize("kind", fc.ISTFT_KINDS)
@pytest.mark.parametrize("case", fc.ISTFT_CASES, ids=fc.istft_id)
def test_istft_plan_on_host_simulator(case, kind):
    ref, unit = fc.istft_case_reference(case, kind)
    mine = fc.istft64(fc.istft_spectrum(case, kind), case.hop, case.win, case.L)
    assert fc.bound_ratio(mine, ref, unit) < 1e-3                   # the restatement the mutant is made from is torch.istft
    got = _sim_istft(case, fc.istft_spectrum(case, kind))
    k = fc.bound_ratio(got, ref, unit)
    print(f"{fc.istft_id(case)} {kind}: K_ref {fc.istft_k_reference():.2f} K {fc.istft_k():.2f} simulator {k:.2f} | largest sample {float(ref.abs().max()):.3g}")
    assert torch.isfinite(got).all() and k <= fc.istft_k(), (k, fc.istft_k())


def test_istft_bar_is_of_float32_size():
    """K_ref is a handful of float32 roundings per sample, not a property of one ill-conditioned tail: the bar scales with the conditioning and
    does not have to absorb it."""
    k = fc.istft_k_reference()
    _report("frontend_cpu_istft_k.txt", [f"K_ref {k:.3f} K {fc.istft_k():.3f}"])
    assert 0.5 <= k <= 8.0, k


@pytest.mark.parametrize("L", [6190, 6199, 6200])
def test_istft_cases_see_an_envelope_with_an_epsilon(L):
    """The mutant: the float64 iSTFT with the envelope replaced by envelope + 1e-8.  It must miss the bar by more than 3 x on every case of
    these lengths, inconsistent spectrum - or a kernel that still adds ConviSTFT's epsilon would pass."""
    seen = []
    for case in fc.ISTFT_CASES:
        if case.L != L:
            continue
        spec = fc.istft_spectrum(case, "inconsistent")
        ref, unit = fc.istft_case_reference(case, "inconsistent")
        seen.append(fc.bound_ratio(fc.istft64(spec, case.hop, case.win, case.L, env_eps=1e-8), ref, unit) / fc.istft_k())
    print(L, seen)
    assert len(seen) == 3 and min(seen) > 3.0, seen


@pytest.mark.parametrize("hop,win", fc.SWEEP_CONFIGS)
def test_istft_plan_refuses_exactly_the_lengths_torch_refuses(hop, win):
    """Plan construction only.  torch.istft refuses a clip that reaches a sample whose window envelope is below 1e-11; the plan must refuse the
    same lengths (it would divide by that envelope), say which length and window, and build for every other length above fft_len/2."""
    refused, wrongly_built, wrongly_refused = 0, [], []
    for L in fc.SWEEP_LENGTHS:
        accepts = fc.torch_istft_accepts(L, hop, win)
        try:
            Plan(1, L, win_len=win, win_inc=hop, fft_len=fc.NFFT, model="TorchISTFT")
            built = True
        except ValueError as e:
            built, msg = False, str(e)
        if not accepts:
            refused += 1
            if built:
                wrongly_built.append(L)
            elif L <= fc.NFFT // 2:                                # too short comes first
                assert f"length {L} is not above fft_len/2" in msg, msg
            else:
                assert f"at length {L} " in msg and f"{win}-sample Hann window at hop {hop}" in msg and "envelope" in msg, msg
        elif L > fc.NFFT // 2:
            if not built:
                wrongly_refused.append((L, msg))
        else:
            assert not built and f"length {L} is not above fft_len/2" in msg, (L, built)
    print(f"hop {hop} win {win}: torch refuses {refused} of {len(fc.SWEEP_LENGTHS)} lengths")
    assert not wrongly_built, (len(wrongly_built), wrongly_built[:8])
    assert not wrongly_refused, wrongly_refused[:4]
    if (hop, win) == (300, 400):
        assert refused == sum(1 for L in fc.SWEEP_LENGTHS if L % 300 > 200)          # the clip's end past the last window's last tap
    if (hop, win) == (512, 512):
        # sample 256 of the clip is the start of frame 1, where the Hann window is 0; with ONE frame (L < 512) the clip ends in zeros instead
        assert refused == sum(1 for L in fc.SWEEP_LENGTHS if L >= 512)
    if (hop, win) in ((128, 512), (256, 512), (100, 400)):
        assert refused == 0


def test_istft_plan_messages_name_the_limit():
    kw = dict(win_inc=300, model="TorchISTFT")
    with pytest.raises(ValueError, match=r"fft_len 256 is not 512"):
        Plan(2, 6000, win_len=200, fft_len=256, **kw)
    with pytest.raises(ValueError, match=r"win_len 600 .*fft_len = 512"):
        Plan(2, 6000, win_len=600, fft_len=512, **kw)
    with pytest.raises(ValueError, match=r"length 256 is not above fft_len/2 = 256"):
        Plan(2, 256, win_len=400, fft_len=512, **kw)
    for L in (6250, 6256, 6299):
        with pytest.raises(ValueError, match=rf"at length {L} the clip reaches sample 6200, where the overlap-add envelope of the 400-sample Hann window"):
            Plan(2, L, win_len=400, fft_len=512, **kw)
    assert Plan(2, 6200, win_len=400, fft_len=512, **kw).T == 21


# ------------------------------------------------------------------------------------------ targets
def test_target_cases_put_members_on_every_arm():
    """Census of the largest case (every other is a prefix of it); the first 255 bins already hold every geometry arm.  Conditions the GPU tier's
    exact checks rest on: crafted clamp members clear the clamp's edge by 1e-4 relative, so the float32 ratio is on the same side; the float32
    oracle gives exactly 10.0 on the whole saturation arm and one value on the whole clamp arm."""
    noisy, clean = fc.target_inputs(max(fc.TARGET_SIZES))
    census = fc.target_census(noisy, clean)
    small = fc.target_census(*fc.target_inputs(255))
    r = fc.target_reference(max(fc.TARGET_SIZES))
    _report("frontend_cpu_target_census.txt", [f"n = {noisy.numel()}: {census}", f"n = 255: {small}", f"phase: float32 alone {r.phase_alone:.3e} bar {r.phase_bar:.3e}",
                                               f"cIRM float32 alone {r.cirm_alone}", f"cIRM bars {r.cirm_bar}"])
    assert tuple(census) == fc.TARGET_ARMS
    for arm, n in census.items():
        assert n >= MIN_MEMBERS, (arm, n)
    for arm in fc.TARGET_ARMS[:10]:
        assert small[arm] >= 1, (arm, small)
    ratio = fc.cirm_ratio64(noisy, clean)
    on_edge = (ratio <= -100.0) & (ratio > fc.CLAMP_CLEAR) & ~r.masks["noisy_zero"]
    assert int(on_edge.sum()) == 0
    assert bool((r.cirm32[r.masks["saturate"]] == 10.0).all())
    assert r.cirm32[r.masks["clamp"]].unique().numel() == 1
    assert float(r.cirm[r.masks["noisy_zero"]].abs().max()) == 0.0
    assert torch.isfinite(r.cirm).all() and torch.isfinite(r.cirm32).all()
    # float32 alone is of float32's size: the bars are 4 x a rounding figure, not 4 x something a bug could hide in
    assert 1e-7 <= r.phase_alone <= 5e-7, r.phase_alone
    assert all(v <= 2e-5 for a, v in r.cirm_alone.items() if a != "cancels"), r.cirm_alone


def test_decompress_cases_cover_the_three_arms():
    d = fc.decompress_inputs()
    lim = torch.tensor(fc.LIMIT, dtype=torch.float32)
    assert float(d["upper"][0]) == float(lim) and float(d["lower"][0]) == -float(lim)
    assert bool((d["upper"] >= lim).all()) and bool((d["lower"] <= -lim).all())
    assert bool((d["inner"].abs() < lim).all()) and bool((d["inner"].abs() >= 3).all()) and bool((d["small"].abs() < 3).all())
    ref = fc.decompress_reference(d["inner"])
    assert float(ref.abs().min()) >= 6.0                         # where relative 1e-6 is within float32's reach (frontend_cases.DECOMPRESS_REL)
    for arm, m in d.items():                                     # the oracle in float32 against float64 meets the bars the GPU tier asserts
        got, ref = fc.ofsn.decompress_cirm(m).double(), fc.decompress_reference(m)
        if arm == "small":
            assert float((got - ref).abs().max()) <= fc.DECOMPRESS_ABS_SMALL
        elif arm == "inner":
            assert float(((got - ref).abs() / ref.abs()).max()) <= fc.DECOMPRESS_REL
        else:
            assert got.unique().numel() == 1 and abs(float(got[0] - ref[0])) <= fc.DECOMPRESS_REL * abs(float(ref[0]))
