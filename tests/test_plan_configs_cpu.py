"""CPU tier over the configuration table (plan_configs.py): every entry the planner accepts, interpreted by the host simulator, must reproduce
the oracle's forward and backward; every entry must build or be refused by name in every listed dtype, training and eval; and the table as a
whole must reach every class of GEMM descriptor whose kernel path the two stock configurations never take."""
import ctypes as C

import pytest
import torch

from plan_check import check_crn_plan_vs_oracle, check_dccrn_plan_vs_oracle
from plan_configs import ACCEPTED, TABLE, entry_id, plan_kwargs
from simutil import PHASE_BWD, PHASE_FWD, Plan, sim
from sefd_amd.plan import WG_FAMILY_WIDE128, WG_FAMILY_WIDE256, WG_FAMILY_WIDE256_ONES
from util import knobs

KIND_RUNGEMM, KIND_WGRAD, KIND_STFT_FFT = 1, 2, 37          # sefd_desc.h OpKind
RUN_ALIGNED, RUN_ACCUM, RUN_RELU, RUN_Y_ALIGNED, RUN_WTILE32, RUN_WG_WIDE, RUN_ENC0 = 1, 2, 4, 8, 16, 32, 512      # sefd_desc.h kRun*

# Cases whose gradients the float32 ORACLE does not hold to the bars (conditioning, measured on the reference alone: the oracle in float32 against the
# oracle in float64, same parameters and inputs, max-abs over max-abs).  They are compared with the float64 oracle instead, at the unchanged bars: the
# simulator accumulates in double, and a wrong gradient still misses 2e-4.
FLOAT64_ORACLE = {
    # D = 2: every BatchNorm of the deep layers sees 2 bins x T frames per channel.  float32 against float64 oracle: 49 tensors between 2.7e-4 and 6.4e-3
    # (decoder.1.0.real_conv.weight 6.40e-3, decoder.1.0.imag_conv.weight 4.19e-3, encoder.4.2.weight 3.26e-3, encoder.0.2.weight 2.56e-3);
    # the plan against the float64 oracle: worst gradient 4.6e-7
    "fft256_6",
    # float32 against float64 oracle: decoder.3.1.bias 2.03e-4, enhance.1.{real,imag}_lstm.weight_hh_l0 2.21e-4 / 2.22e-4, just above the 2e-4 bar;
    # the plan against the float64 oracle: worst gradient 5.9e-6
    "len3050",
}
# One BatchNorm output on the PReLU kink (plan_check.check_dccrn_plan_vs_oracle `kink`): entry -> (decoder layer, channel).  noskip: element (b 1, bin 13,
# frame 33) of channel 26 is -1.05e-7 in the float64 oracle (-1.6e-7 in float32); the plan takes the other branch, which moves decoder.1.1.bias[26] by
# (1 - 0.25) * 7.22e-4 = 5.42e-4, 3.09e-4 of the tensor's largest element - the whole of the plan's 3.09e-4 distance to the oracle.  Against the oracle's
# gradient with that one element on the other branch the tensor is held to the unchanged 2e-4 (measured: 2.7e-7).
KINKS = {"noskip": (1, 26)}


def _set_knobs(e):
    for k, v in e.knobs:
        knobs.set(k, v)


@pytest.mark.parametrize("e", ACCEPTED, ids=entry_id)
def test_entry_on_host_simulator_vs_oracle(e):
    """Forward taps, the three outputs, running statistics and all parameter gradients, fp32.  Clip lengths the frames do not tile: out_wav[:, :Lout]
    is the oracle's clip, out_wav[:, Lout:] exactly zero, and a gradient laid on that tail reaches no parameter (plan_check._tail_noise)."""
    _set_knobs(e)
    kw = {k: v for k, v in plan_kwargs(e).items() if k not in ("model", "act_dtype", "training")}
    report = {}
    try:
        if e.model == "CRN":
            check_crn_plan_vs_oracle(kw, e.B, e.L, report=report)
        else:
            mode = kw.pop("masking_mode", "E")
            check_dccrn_plan_vs_oracle(mode, "SI-SNR", kw, e.B, e.L, report=report, kink=KINKS.get(e.name),
                                       oracle_dtype=torch.float64 if e.name in FLOAT64_ORACLE else torch.float32)
    finally:
        worst = sorted(report.items(), key=lambda kv: -kv[1])[:4]
        print(e.name, " ".join(f"{k} {v:.1e}" for k, v in worst))


def _gemm_ops(plan):
    """[(phase, op_info dict + Npad, ldw, nseg, nsplit, ydt, n2, longest run, odd runs)] of every RUNGEMM / WGRAD; asserts the first-layer predicate."""
    out = []
    f = sim().hostsim_gemm_fields
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
    sz = plan.lib.sefd_op_size()
    for ph in (PHASE_FWD, PHASE_BWD):
        for i in range(plan.num_ops(ph)):
            o = plan.op_info(ph, i)
            if o["kind"] not in (KIND_RUNGEMM, KIND_WGRAD):
                continue
            ptr = plan.ops_ptr(ph) + i * sz
            assert sim().hostsim_enc0_accepts(ptr, 0) == 1, (ph, i, o)
            v = (C.c_int64 * 8)()
            assert f(ptr, v) == 0
            o.update(phase=ph, Npad=int(v[0]), ldw=int(v[1]), nseg=int(v[2]), nsplit=int(v[3]), ydt=int(v[4]), n2=int(v[5]), longest=int(v[6]), odd=int(v[7]))
            out.append(o)
    return out


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("e", TABLE, ids=entry_id)
def test_every_entry_builds_or_is_refused_by_name(e, training):
    """Every listed dtype, training and eval: a plan whose first-layer descriptors pass sefd_desc.h enc0_accepts (what the host simulator checks
    before it runs one), or a ValueError that carries the planner's named error - never a signal (which would end this process)."""
    _set_knobs(e)
    for dtype in e.dtypes:
        if e.refused is not None:
            with pytest.raises(ValueError, match=e.refused):
                Plan(e.B, e.L, **plan_kwargs(e, dtype, training))
            continue
        plan = Plan(e.B, e.L, **plan_kwargs(e, dtype, training))
        assert plan.num_ops(PHASE_FWD) > 0 and (plan.num_ops(PHASE_BWD) > 0) == training
        gemms = _gemm_ops(plan)
        assert gemms and all(g["nseg"] <= 8 for g in gemms)


def bn_of(N):
    return 128 if N > 64 else 64 if N > 32 else 32


def wgrad_tn(g):
    """sefd_desc.h wgrad_tn for the aligned bf16 kernel, plan_builder.h wgrad() for the others."""
    bf16 = g["dtype"] == 1
    if g["flags"] & RUN_ALIGNED:
        return 64 if not bf16 else 128 if g["Npad"] >= 128 else 64 if g["N"] > 32 else 32
    return 128 if bf16 and g["Npad"] >= 128 else 64


def test_table_reaches_every_descriptor_class():
    """The shapes are the ones that can go wrong: over all entries, dtypes and knobs of the table there is at least one RUNGEMM / WGRAD descriptor of
    every class below (each names the kernel path it selects).  A class that disappears from the table fails here by name."""
    seen = {}

    def hit(name, e, dtype, g):
        seen.setdefault(name, f"{e.name}/{dtype} tag {g['tag']} M {g['M']} N {g['N']} K {g['K']}" if g else f"{e.name}/{dtype}")

    for e in ACCEPTED:
        knobs.unset(*[k for other in ACCEPTED for k, _ in other.knobs])          # every entry is planned under its own knobs only, as the GPU sweep runs it
        _set_knobs(e)
        for dtype in e.dtypes:
            plan = Plan(e.B, e.L, **plan_kwargs(e, dtype))
            kinds, _ = plan.op_kinds(PHASE_FWD)
            gemms = _gemm_ops(plan)
            bf16 = dtype == "bf16"
            framing = [g for g in gemms if g["phase"] == PHASE_FWD and g["kind"] == KIND_RUNGEMM and g["tag"] == 1]
            if framing and KIND_STFT_FFT not in [int(k) for k in kinds]:
                hit("framing-GEMM STFT (no OP_STFT_FFT)", e, dtype, framing[0])
            for g in gemms:
                run, wg = g["kind"] == KIND_RUNGEMM, g["kind"] == KIND_WGRAD
                conv = 100 <= g["tag"] < 500 and g["tag"] != 300
                if g["Npad"] > g["N"]:
                    hit("Npad > N (tile tail in N)", e, dtype, g)
                if conv:
                    hit(f"bn_of(N) = {bn_of(g['N'])}", e, dtype, g)
                if bf16 and g["dtype"] == 1 and not g["flags"] & RUN_ALIGNED:
                    hit("bf16 RUNGEMM without kRunAligned (non-DMA rungemm_kernel)" if run else "bf16 WGRAD without kRunAligned (wgrad_bf16_kernel<64 / 128>)", e, dtype, g)
                if bf16 and run and g["ydt"] == 1 and not g["flags"] & RUN_Y_ALIGNED:
                    hit("bf16 RUNGEMM without kRunYAligned (non-staged epilogue)", e, dtype, g)
                if (bf16 and run and g["dtype"] == 1 and g["ydt"] == 1 and dict(e.knobs).get("DIRECT_MINM") == "0" and g["flags"] & RUN_ALIGNED and g["flags"] & RUN_Y_ALIGNED
                        and not g["flags"] & (RUN_ACCUM | RUN_RELU | RUN_WTILE32) and g["Npad"] <= 64 and g["ldw"] <= 128 and g["ldw"] % 8 == 0 and g["odd"] == 0):
                    hit("thin-eligible RUNGEMM under DIRECT_MINM=0 (thin.hip)", e, dtype, g)
                if run and g["flags"] & RUN_WTILE32:
                    hit("wide-tile RUNGEMM, Npad % 256 == 0 (cgemm256.hip)", e, dtype, g)
                if wg and g["flags"] & RUN_WG_WIDE:                   # launch_wgrad: Npad % 256 == 0 -> launch_wgrad_wide, else launch_wgrad_wide128
                    wide256 = g["Npad"] % 256 == 0
                    assert g["family"] in ((WG_FAMILY_WIDE256, WG_FAMILY_WIDE256_ONES) if wide256 else (WG_FAMILY_WIDE128,)), (e.name, g)
                    assert wide256 or (g["Npad"] == 128 and g["ldw"] >= 1024), (e.name, g)
                    hit("wide-tile WGRAD (256 x 256 tile)" if wide256 else "wide-tile WGRAD (128 x 512 tile)", e, dtype, g)
                if bf16 and conv and g["Npad"] == 384 and dict(e.knobs).get("CG256_MINM"):
                    hit("Npad = 384 beside the wide tiles (128-wide kernels)", e, dtype, g)
                if wg and bf16 and g["dtype"] == 1:
                    hit(f"wgrad_tn = {wgrad_tn(g)}", e, dtype, g)
                if bf16 and run and g["tag"] == 100 and g["phase"] == PHASE_FWD and not g["flags"] & RUN_ENC0:
                    hit("bf16 first layer without kRunEnc0", e, dtype, g)
                if g["nseg"] == 8 and g["tag"] in (200, 201) and g["flags"] & RUN_ACCUM and run:
                    hit("recurrent input GEMM in chunks of 8 channel slices (kRunAccum)", e, dtype, g)
                if wg and g["nseg"] == 1 and g["K"] == 1 and g["tag"] == 200:
                    hit("bias-only WGRAD behind a full run list (D >= 8)", e, dtype, g)
    want = ["Npad > N (tile tail in N)", "bn_of(N) = 32", "bn_of(N) = 64", "bn_of(N) = 128",
            "bf16 RUNGEMM without kRunAligned (non-DMA rungemm_kernel)", "bf16 WGRAD without kRunAligned (wgrad_bf16_kernel<64 / 128>)",
            "bf16 RUNGEMM without kRunYAligned (non-staged epilogue)", "thin-eligible RUNGEMM under DIRECT_MINM=0 (thin.hip)",
            "wide-tile RUNGEMM, Npad % 256 == 0 (cgemm256.hip)", "wide-tile WGRAD (256 x 256 tile)", "wide-tile WGRAD (128 x 512 tile)", "Npad = 384 beside the wide tiles (128-wide kernels)",
            "wgrad_tn = 32", "wgrad_tn = 64", "wgrad_tn = 128", "framing-GEMM STFT (no OP_STFT_FFT)", "bf16 first layer without kRunEnc0",
            "recurrent input GEMM in chunks of 8 channel slices (kRunAccum)", "bias-only WGRAD behind a full run list (D >= 8)"]
    for name in want:
        print(f"{name}: {seen.get(name)}")
    missing = [name for name in want if name not in seen]
    assert not missing, missing


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("model,kn5,channels", [("DCCRN", 1040, 1040), ("DCCRN", 2064, 2064), ("CRN", 2064, 1032), ("CRN", 4128, 2064)])
def test_batchnorm_layer_wider_than_the_lds_staging_is_refused(model, kn5, channels, dtype):
    """bn.hip stages 4 * C floats of a layer's parameters in LDS arrays sized for sefd_desc.h kBnMaxC = 1024 channels, and reduces a block of rows
    through an array sized for it: a wider BatchNorm2d layer is refused by the conv stack both planners share, with the layer named - as the
    ComplexBatchNorm branch refuses its own.  (The CRN's layers have kernel_num / 2 channels: its kernel_num[5] = 1040 is a 520-channel layer.)
    Such a plan is never run: every BatchNorm launch of the layer would write past the arrays."""
    kn = (16, 32, 32, 64, 64, kn5)
    with pytest.raises(ValueError, match=rf"BatchNorm2d: at most 1024 channels per layer .*encoder\.5 has {channels}"):
        Plan(1, 800, masking_mode="E", kernel_num=kn, rnn_units=128, act_dtype=dtype, model=model)
    with pytest.raises(ValueError, match="BatchNorm2d: at most 1024 channels"):
        Plan(1, 800, masking_mode="E", kernel_num=kn, rnn_units=128, act_dtype=dtype, model=model, training=False)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("model,kn5", [("DCCRN", 1024), ("CRN", 2048), ("CRN", 1040)])
def test_batchnorm_layer_of_1024_channels_still_builds(model, kn5, dtype):
    p = Plan(1, 800, masking_mode="E", kernel_num=(16, 32, 32, 64, 64, kn5), rnn_units=128, act_dtype=dtype, model=model)
    assert p.params["encoder.5.1.weight"][1] == ((kn5 if model == "DCCRN" else kn5 // 2),)
