"""CPU: ConvSTFT and ConviSTFT on their own (tools_for_model.py:36-112) - exports, constructor defaults, buffers, init_kernels, the two planner
models (csrc/plan_frontend.cpp, ids 7 and 8) over the golden case table, and every refusal sentence.  No phase of these plans consists only of
ops the host simulator interprets (each has a spectrum conversion); the analysis transform that opens ConvSTFT's forward does, and it is run there
against the float64 goldens."""
import os
import subprocess
import sys

import pytest
import torch

import convstft_common as cc
from simutil import PHASE_BWD, PHASE_FWD, Plan, sim_run, spec_to_ref
from util import knobs

OP_RUNGEMM, OP_OLA_FWD, OP_OLA_BWD, OP_STFT_FFT, OP_ISTFT_FFT, OP_IFFT_OLA, OP_SPECCONV = 1, 15, 16, 37, 39, 49, 50        # sefd_desc.h OpKind
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kinds(plan, phase):
    return [int(k) for k in plan.op_kinds(phase)[0]]


def modes(plan, phase):
    return [plan.op_info(phase, i)["flags"] for i in range(plan.num_ops(phase)) if plan.op_info(phase, i)["kind"] == OP_SPECCONV]


def test_exports_and_dropin():
    import sefd_amd  # noqa: F401
    from sefd_amd import models, tools_for_model
    assert tools_for_model.ConvSTFT is models.ConvSTFT and tools_for_model.ConviSTFT is models.ConviSTFT
    code = ("import sys; sys.path.insert(0, %r); import tools_for_model, models; from tools_for_model import ConvSTFT, ConviSTFT, init_kernels; "
            "assert ConvSTFT is models.ConvSTFT and ConviSTFT is models.ConviSTFT; print('same')") % os.path.join(ROOT, "dropin")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "same" in out.stdout, out.stderr


def test_constructor_defaults_and_buffers():
    import inspect
    import sefd_amd  # noqa: F401
    from sefd_amd.frontend_consts import stft_kernels
    from sefd_amd.tools_for_model import ConvSTFT, ConviSTFT, init_kernels
    for cls in (ConvSTFT, ConviSTFT):
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters) == ["self", "win_len", "win_inc", "fft_len", "win_type", "feature_type", "fix"]
        assert [sig.parameters[k].default for k in ("fft_len", "win_type", "feature_type", "fix")] == [None, "hamming", "real", True]
        assert cls(400, 100).dim == 512 and cls(200, 50).dim == 256 and cls(512, 128).dim == 512 and cls(513, 128).dim == 1024
        m = cls(400, 100)
        assert (m.feature_type, m.stride, m.win_len, m.win_type) == ("real", 100, 400, "hamming")
    K, Kinv, w = stft_kernels(400, 512, "hann")
    s, i = ConvSTFT(400, 100, 512, "hann", "complex"), ConviSTFT(400, 100, 512, "hann", "complex")
    assert list(s.state_dict()) == ["weight"] and list(i.state_dict()) == ["weight", "window", "enframe"]
    assert torch.equal(s.weight, K) and torch.equal(i.weight, Kinv) and torch.equal(i.window, w) and torch.equal(i.enframe, torch.eye(400)[:, None, :])
    for win in (None, "hann", "hamming"):
        K, Kinv, w = stft_kernels(200, 256, win)
        k, ww = init_kernels(200, 50, 256, win)
        ki, wi = init_kernels(200, 50, 256, win, invers=True)
        assert tuple(k.shape) == (258, 1, 200) and tuple(ww.shape) == (1, 200, 1)
        assert torch.equal(k, K) and torch.equal(ki, Kinv) and torch.equal(ww, w) and torch.equal(wi, w)
    with pytest.raises(RuntimeError, match="cuda"):
        s(torch.zeros(2, 1000))
    with pytest.raises(RuntimeError, match="cuda"):
        i(torch.zeros(2, 257, 13), torch.zeros(2, 257, 13))


def test_dccrn_and_crn_keep_their_front_end_buffers():
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models
    cfg.dccrn_kernel_num, cfg.skip_type = [16, 32, 32, 64, 64, 64], True
    for m, ft in ((models.DCCRN(rnn_units=128), "complex"), (models.CRN(rnn_units=128, rnn_input_size=128), "real")):
        assert list(m.state_dict())[:4] == ["stft.weight", "istft.weight", "istft.window", "istft.enframe"]
        assert m.stft.feature_type == ft and m.istft.feature_type == "complex" and tuple(m.stft.weight.shape) == (514, 1, 400)
        assert not any(k.startswith(("stft.", "istft.")) for k, _ in m.named_parameters())


@pytest.mark.parametrize("ft", ["complex", "real"])
@pytest.mark.parametrize("name", list(cc.CASES))
def test_plans_over_the_case_table(name, ft):
    W, hop, NFFT, L, win = cc.CASES[name]
    T, NF, Lout = cc.geometry(W, hop, NFFT, L)
    B = cc.B
    polar = ft != "complex"
    fft = NFFT == 512
    ps = Plan(B, L, win_len=W, win_inc=hop, fft_len=NFFT, model="ConvSTFT", win_type=win, feature_type=ft)
    assert ps.T == T and ps.NF == NF and ps.n_param == 0
    want = ({"io.wav": B * L, "io.grad_wav": B * L, "io.mags": B * NF * T, "io.phase": B * NF * T, "io.grad_mags": B * NF * T, "io.grad_phase": B * NF * T}
            if polar else {"io.wav": B * L, "io.grad_wav": B * L, "io.out": B * 2 * NF * T, "io.grad_out": B * 2 * NF * T})
    assert {n: ps.buffer(n)[2] // 4 for n in ps.buffer_names() if n.startswith("io.")} == want
    assert kinds(ps, PHASE_FWD) == [OP_STFT_FFT if fft else OP_RUNGEMM, OP_SPECCONV]
    assert kinds(ps, PHASE_BWD) == [OP_SPECCONV, OP_ISTFT_FFT if fft else OP_RUNGEMM, OP_OLA_FWD]
    assert modes(ps, PHASE_FWD) == [2 if polar else 0] and modes(ps, PHASE_BWD) == [3 if polar else 1]
    pi = Plan(B, T, win_len=W, win_inc=hop, fft_len=NFFT, model="ConviSTFT", win_type=win, feature_type=ft)
    assert pi.T == T and pi.NF == NF
    want = ({"io.wav": B * Lout, "io.grad_wav": B * Lout, "io.mags": B * NF * T, "io.phase": B * NF * T, "io.grad_mags": B * NF * T, "io.grad_phase": B * NF * T}
            if polar else {"io.wav": B * Lout, "io.grad_wav": B * Lout, "io.in": B * 2 * NF * T, "io.grad_in": B * 2 * NF * T})
    assert {n: pi.buffer(n)[2] // 4 for n in pi.buffer_names() if n.startswith("io.")} == want
    assert kinds(pi, PHASE_FWD) == [OP_SPECCONV, OP_ISTFT_FFT if fft else OP_RUNGEMM, OP_OLA_FWD]
    assert kinds(pi, PHASE_BWD) == [OP_OLA_BWD, OP_STFT_FFT if fft else OP_RUNGEMM, OP_SPECCONV]
    assert modes(pi, PHASE_FWD) == [4 if polar else 1] and modes(pi, PHASE_BWD) == [5 if polar else 0]
    if fft:
        # the fused kernel, on request: frames per workgroup, the halo it recomputes = ceil(win_len / hop) - 1, and its stage within 40 KiB of LDS
        knobs.set("CONVSTFT_FUSE", 1)
        ps = Plan(B, L, win_len=W, win_inc=hop, fft_len=NFFT, model="ConvSTFT", win_type=win, feature_type=ft)
        pi = Plan(B, T, win_len=W, win_inc=hop, fft_len=NFFT, model="ConviSTFT", win_type=win, feature_type=ft)
        assert kinds(ps, PHASE_BWD) == [OP_SPECCONV, OP_IFFT_OLA] and kinds(pi, PHASE_FWD) == [OP_SPECCONV, OP_IFFT_OLA]
        for plan, phase in ((ps, PHASE_BWD), (pi, PHASE_FWD)):
            info = plan.op_info(phase, 1)
            assert info["N"] == -(-W // hop) - 1 and info["M"] in (4, 8, 16) and (info["M"] + info["N"]) * W * 4 <= 40 * 1024


def test_small_hops_that_do_not_fit_the_stage_take_the_composition():
    knobs.set("CONVSTFT_FUSE", 1)
    pi = Plan(2, 40, win_len=512, win_inc=16, fft_len=512, model="ConviSTFT", win_type="hann")      # halo 31: 35 frames of 2 KiB > 40 KiB
    assert kinds(pi, PHASE_FWD) == [OP_SPECCONV, OP_ISTFT_FFT, OP_OLA_FWD]


@pytest.mark.parametrize("model,kw,text", [
    ("ConvSTFT", dict(L=100, win_len=400, win_inc=300, fft_len=512), "gives no frame"),
    ("ConvSTFT", dict(L=0, win_len=400, win_inc=100, fft_len=512), "gives no frame"),
    ("ConviSTFT", dict(L=0, win_len=400, win_inc=100, fft_len=512), r"0 frames \(T < 1\)"),
    ("ConviSTFT", dict(L=2, win_len=400, win_inc=100, fft_len=512), r"Lout = -100 <= 0"),
    ("ConviSTFT", dict(L=3, win_len=400, win_inc=100, fft_len=512), r"Lout = 0 <= 0"),
    ("ConvSTFT", dict(L=1000, win_len=600, win_inc=100, fft_len=512), "win_len 600 is above fft_len 512"),
    ("ConviSTFT", dict(L=13, win_len=600, win_inc=100, fft_len=512), "win_len 600 is above fft_len 512"),
    ("ConvSTFT", dict(L=1000, win_len=400, win_inc=0, fft_len=512), r"hop 0 must lie in 1 \.\. win_len = 400"),
    ("ConviSTFT", dict(L=13, win_len=400, win_inc=-4, fft_len=512), r"hop -4 must lie in 1 \.\. win_len = 400"),
    ("ConvSTFT", dict(L=1000, win_len=400, win_inc=401, fft_len=512), r"hop 401 must lie in 1 \.\. win_len = 400"),
    ("ConviSTFT", dict(L=13, win_len=400, win_inc=401, fft_len=512), r"hop 401 must lie in 1 \.\. win_len = 400"),
])
def test_every_refusal_names_its_limit(model, kw, text):
    with pytest.raises(ValueError, match=model + " plan: .*" + text):
        Plan(2, model=model, **kw)


def test_limits_are_not_refused_early():
    """One frame, hop == win_len (no trim at all), and the shortest clip that still gives a frame."""
    assert Plan(2, 400, win_len=400, win_inc=400, fft_len=512, model="ConvSTFT").T == 1
    assert Plan(2, 1, win_len=400, win_inc=400, fft_len=512, model="ConviSTFT").buffer("io.wav")[2] == 2 * 400 * 4
    assert Plan(2, 1, win_len=400, win_inc=100, fft_len=512, model="ConvSTFT").T == 3
    assert Plan(2, 4, win_len=400, win_inc=100, fft_len=512, model="ConviSTFT").buffer("io.wav")[2] == 2 * 100 * 4


@pytest.mark.parametrize("name", list(cc.CASES))
def test_analysis_transform_on_the_host_simulator(name):
    """Op 0 of ConvSTFT's forward (the FFT kernel, or the framing GEMM at fft_len 256) on the host simulator against the float64 golden spectrum, at
    the GPU tests' bar."""
    W, hop, NFFT, L, win = cc.CASES[name]
    seed, ref, e32 = cc.load_golden(name)
    plan = Plan(cc.B, L, win_len=W, win_inc=hop, fft_len=NFFT, model="ConvSTFT", win_type=win, feature_type="complex")
    ar = plan.alloc_arenas("cpu")
    plan.io(ar, "wav", (cc.B, L)).copy_(cc.case_inputs(name, seed)["wav"])
    sim_run(plan, PHASE_FWD, ar, 0, 1)
    got = spec_to_ref(plan.view(ar, "spec"), cc.B, plan.T, plan.NF)
    err = cc.rel_err(got, ref["out"])
    print(f"{name}: err {err:.3e} ref32_err {e32['out']:.3e}")
    assert err <= cc.BAR * e32["out"]
