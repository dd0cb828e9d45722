"""The table of DCCRN / CRN plan configurations beyond the two stock channel tuples (16, 32, 32, 64, 64, 64) and
(32, 64, 128, 256, 256, 256) at fft_len 512, 400 / 100: odd channel counts (tile tails in N, unaligned bf16 runs), every depth, other
front ends, every recurrent-block variant, a first layer the spectrum kernels decline, clip lengths the frames do not tile.

The CPU tier (test_plan_configs_cpu.py) runs every accepted entry in fp32 on the host simulator against the oracle, builds every entry in
every listed dtype in training and in eval mode, and asserts that the table as a whole reaches every descriptor class of COVERAGE below;
the GPU tier (test_gpu_plan_configs.py) runs the listed dtypes op by op against the host simulator.

B stays at 1 to 3 and L at 2000 to 4000 (20 to 45 frames): a few seconds per GPU case, and still partial M tiles everywhere."""
from collections import namedtuple

# name; model: DCCRN / DCCRN_CBN / CRN; B, L; kw: Plan keywords (kernel_num, rnn_units, front end, ...); dtypes to run;
# knobs: the tuning knobs the GPU op sweep (and the coverage check) plans the entry under; refused: the planner's error text when it declines the entry
Entry = namedtuple("Entry", "name model B L kw dtypes knobs refused", defaults=((), None))

SMALL_KN = (16, 32, 32, 64, 64, 64)
ODD_KN = (8, 24, 40, 72, 136, 264)
DEEP7_KN = (8, 16, 24, 32, 40, 48, 56)
BOTH = ("fp32", "bf16")
F32 = ("fp32",)
# the knobs of test_every_op_against_host_simulator's steered cases: the direct-operand kernel (thin.hip) on every N <= 64 GEMM with aligned runs,
# BatchNorm backward sums in the epilogues of all three GEMM kernels, the wide tiles (cgemm256.hip, the 256 x 256 WGRAD tile) on small cases
THIN = (("DIRECT_MINM", "0"), ("BN_FUSE", "2"))
WIDE = (("CG256_MINM", "64"), ("WG256_MINM", "64"), ("BN_FUSE", "2"))
STEPPED = (("LSTM_STEPPED", "1"),)

TABLE = [
    # ---- odd channels: N = 8, 24, 40, 72, 136, 264 -> Npad 32, 32, 64, 128, 256, 384; bf16 runs of 5 * 12, 5 * 20, 5 * 36 ... elements
    Entry("odd", "DCCRN", 2, 3000, dict(kernel_num=ODD_KN, rnn_units=192), BOTH),
    Entry("odd_thin", "DCCRN", 2, 3000, dict(kernel_num=ODD_KN, rnn_units=192, masking_mode="C"), ("bf16",), THIN),
    Entry("odd_wide", "DCCRN", 1, 2400, dict(kernel_num=(8, 24, 40, 72, 256, 384), rnn_units=192, masking_mode="C"), ("bf16",), WIDE),
    Entry("odd_cbn", "DCCRN_CBN", 2, 3000, dict(kernel_num=ODD_KN, rnn_units=64), BOTH),           # channel pairs 4, 12, 20, 36, 68, 132
    # ---- depths at fft_len 512: hidden dim D = 128, 64, 32, 16 (the recurrent input GEMM reads its D channel slices 8 at a time), 8, 2
    Entry("depth1", "DCCRN", 1, 2000, dict(kernel_num=(32,), rnn_units=64), BOTH),
    Entry("depth2", "DCCRN", 1, 2000, dict(kernel_num=(16, 32), rnn_units=64), BOTH),
    Entry("depth3", "DCCRN", 2, 3000, dict(kernel_num=(24, 40, 72), rnn_units=64), BOTH),
    Entry("depth4", "DCCRN", 2, 3000, dict(kernel_num=(16, 32, 32, 64), rnn_units=64), BOTH),
    Entry("depth5", "DCCRN", 2, 3000, dict(kernel_num=(16, 32, 32, 64, 64), rnn_units=64), BOTH),
    Entry("depth7", "DCCRN", 2, 3000, dict(kernel_num=DEEP7_KN, rnn_units=64), BOTH),
    # ---- front ends: the framing GEMMs (fft_len != 512), win_len == fft_len, a hop that is no multiple of 4, the rectangular window
    Entry("fft256_5", "DCCRN", 2, 2000, dict(kernel_num=SMALL_KN[:5], rnn_units=64, fft_len=256, win_len=200, win_inc=50), F32),
    Entry("fft256_6", "DCCRN", 2, 2000, dict(kernel_num=SMALL_KN, rnn_units=64, fft_len=256, win_len=200, win_inc=50), BOTH),
    Entry("fft1024_6", "DCCRN", 1, 4000, dict(kernel_num=SMALL_KN, rnn_units=64, fft_len=1024, win_len=800, win_inc=200), BOTH),
    Entry("fft1024_7", "DCCRN", 1, 4000, dict(kernel_num=SMALL_KN + (64,), rnn_units=64, fft_len=1024, win_len=800, win_inc=200), F32),
    Entry("win512", "DCCRN", 2, 3072, dict(kernel_num=SMALL_KN, rnn_units=64, win_len=512, win_inc=128), BOTH),
    Entry("hop99", "DCCRN", 2, 2966, dict(kernel_num=SMALL_KN, rnn_units=64, win_len=400, win_inc=99), BOTH),      # 2966 + 602 - 400 = 32 * 99
    Entry("win_none", "DCCRN", 2, 3000, dict(kernel_num=SMALL_KN, rnn_units=64, win_type=None, masking_mode="C"), F32),
    # ---- recurrence
    Entry("rnn1", "DCCRN", 2, 3000, dict(kernel_num=SMALL_KN, rnn_units=64, rnn_layers=1), BOTH),
    Entry("rnn3", "DCCRN", 2, 3000, dict(kernel_num=SMALL_KN, rnn_units=64, rnn_layers=3), F32),
    Entry("lstm_real", "DCCRN", 2, 3000, dict(kernel_num=ODD_KN, rnn_units=64, lstm="real"), BOTH),
    Entry("noskip", "DCCRN", 2, 3000, dict(kernel_num=ODD_KN, rnn_units=64, skip_type=False), BOTH),
    Entry("ru96", "DCCRN", 2, 3000, dict(kernel_num=ODD_KN, rnn_units=96), F32),
    Entry("depth3_stepped", "DCCRN", 1, 2000, dict(kernel_num=(24, 40, 72), rnn_units=64), BOTH, STEPPED),
    # ---- a bf16 first layer that the spectrum kernels (enc0.hip: 16, 32 or 64 output channels) decline
    Entry("enc0_24", "DCCRN", 2, 3000, dict(kernel_num=(24, 32, 32, 64, 64, 64), rnn_units=64, masking_mode="C"), BOTH),
    # ---- clip lengths the frames do not tile: ConviSTFT returns 3000 of 3050 / 3001 samples
    Entry("len3050", "DCCRN", 2, 3050, dict(kernel_num=SMALL_KN, rnn_units=64), BOTH),
    Entry("len3001", "DCCRN", 3, 3001, dict(kernel_num=SMALL_KN, rnn_units=64, masking_mode="C"), F32),
    Entry("crn_len3050", "CRN", 2, 3050, dict(kernel_num=SMALL_KN, rnn_units=64), F32),
    # ---- CRN (real convs over kernel_num / 2 channels): 8, 24, 40, 72, 136 channels in five layers (D = 8), and fft_len 256
    Entry("crn5", "CRN", 2, 3000, dict(kernel_num=(16, 48, 80, 144, 272), rnn_units=64), BOTH),
    Entry("crn_fft256", "CRN", 2, 2000, dict(kernel_num=SMALL_KN, rnn_units=64, fft_len=256, win_len=200, win_inc=50), BOTH),
    # CRN at the default channels under the wide-tile knobs: 128 real channels with K >= 1024 packed columns (tags 104, 105, 400, 401) - the 128 x 512
    # weight-gradient tile, which no DCCRN layer takes (its N = 128 layers have 640 columns)
    Entry("crn_wide", "CRN", 2, 2400, dict(kernel_num=(32, 64, 128, 256, 256, 256), rnn_units=256), ("bf16",), WIDE),
    Entry("crn3", "CRN", 1, 2000, dict(kernel_num=(16, 48, 80), rnn_units=64), F32),                # D = 32: four chunks of channel slices
    # CRN halves cfg.dccrn_kernel_num: (8, 24, 40, 72, 136) would be 4, 12, 20, 36, 68 real channels, not multiples of 8
    Entry("crn_odd_refused", "CRN", 2, 3000, dict(kernel_num=(8, 24, 40, 72, 136), rnn_units=64), BOTH, (), "channel counts must be multiples of 8"),
]

ACCEPTED = [e for e in TABLE if e.refused is None]
BY_NAME = {e.name: e for e in TABLE}


def entry_id(e):
    return e.name


def plan_kwargs(e, dtype="fp32", training=True):
    """Plan keyword arguments of entry `e`."""
    kw = dict(e.kw)
    kw.update(act_dtype=dtype, training=training, model=e.model.split("_")[0])
    if e.model == "DCCRN_CBN":
        kw["use_cbn"] = True
    return kw


def frames_span(L, win_len, win_inc):
    """Samples ConviSTFT returns for an L-sample clip (tools_for_model.py:111): the frames' span without the two (win_len - win_inc) pads - fewer
    than L when the hop does not tile the padded clip."""
    T = (L + 2 * (win_len - win_inc) - win_len) // win_inc + 1
    return min(L, (T - 1) * win_inc + win_len - 2 * (win_len - win_inc))


def lout(e):
    return frames_span(e.L, e.kw.get("win_len", 400), e.kw.get("win_inc", 100))
