/* sefd.h - C ABI of the MI355X (gfx950) speech-enhancement training hot path.
 *
 * Drop-in boundary: the reference exposes this path only as Python objects -
 *   models.DCCRN.__init__/forward/loss          /root/reference/models.py:15-323
 *   ConvSTFT / ConviSTFT                        /root/reference/tools_for_model.py:36-112
 *   ComplexConv2d / ComplexConvTranspose2d      /root/reference/tools_for_model.py:199-338
 *   NavieComplexLSTM                            /root/reference/tools_for_model.py:141-181
 *   sdr / si_snr / si_sdr / F.mse_loss          /root/reference/tools_for_loss.py:17-94, models.py:315-323
 *   torch.optim.Adam step                       /root/reference/train_interface.py:59, trainer.py:35-37
 * so this header is what a ctypes binding of those objects calls.
 * Plain pointers and sizes only; every function enqueues on the given HIP stream and returns 0 or a negative code.
 * No hidden device allocation: all device memory ("arenas") is owned by the caller.
 */
#ifndef SEFD_H_
#define SEFD_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sefd_plan sefd_plan;

/* Mirror of the config.py knobs that shape DCCRN (config.py:35-68) plus batch geometry. */
typedef struct sefd_model_config {
  int32_t model;          /* 0 DCCRN, 1 CRN, 2 ConvSTFT front end, 3 FullSubNet, 4 torch.stft front end, 5 torch.istft,
                             6 SequenceModel on its own, 7 ConvSTFT on its own, 8 ConviSTFT on its own, 9 one conv layer on its own (ConvLayer),
                             10 ComplexBatchNorm on its own, 11 NavieComplexLSTM on its own (ComplexLSTM), 12 the backward of model 4 (TorchSTFTAdj:
                             grad_spec [B][NF][T][2] -> grad_wav [B][L]), 13 the backward of model 5 (TorchISTFTAdj: grad_wav [B][L] -> grad_spec [B][NF][T][2]);
                             both fft_len 512 only, forward phase only, nothing saved from models 4 / 5 (see build_plan, csrc/plan.cpp) */
  int32_t B, L;           /* batch, samples per clip (models 3, 6, 8, 9 and 11: L = frames T; model 10: L = rows per batch item) */
  int32_t win_len, hop, fft_len;
  int32_t n_layers;
  int32_t kernel_num[12]; /* cfg.dccrn_kernel_num; FullSubNet (model 3): sb/fb neighbours (each 0 .. 31), look_ahead, fb/sb hidden,
                             fb/sb output activation (0 None, 1 ReLU, 2 Tanh, 3 ReLU6), dropout keep in 1/1000, [8] sequence model (0 LSTM, 1 GRU), [9] norm type (0 offline_laplace_norm,
                             1 cumulative_laplace_norm, 2 offline_gaussian_norm, 3 cumulative_layer_norm);
                             SequenceModel (model 6; B = sequences, L = frames T): input size, output size, hidden size (multiple of 8), num_layers (1 .. 8), bidirectional,
                             sequence model (0 LSTM, 1 GRU), dropout keep in 1/1000.  I/O, time-major fp32: x [T][B][roundup(I, 8)] -> y [T][B][O]; grad_y -> grad_x;
                             ConvSTFT / ConviSTFT (models 7 / 8, tools_for_model.py:36-112; fp32, NF = fft_len / 2 + 1, window / window_values as for DCCRN): [0] = feature type,
                             0 'complex' (one [B][2 NF][T] tensor, real block then imaginary block), 1 anything else ((mags, phase), [B][NF][T] each).
                             Model 7, T = (L + 2 (win_len - hop) - win_len) / hop + 1: forward wav [B][L] -> out | mags, phase; backward grad_out | grad_mags, grad_phase -> grad_wav
                             (where a bin's magnitude is exactly 0 its (mags, phase) gradient is 0; the reference has NaN there).
                             Model 8, L = T, Lout = (T - 1) hop + win_len - 2 (win_len - hop): forward in | mags, phase -> wav [B][Lout] (no clamp, overlap-add / (coff + 1e-8));
                             backward grad_wav -> grad_in | grad_mags, grad_phase.  Refused, one sentence each: T < 1, Lout <= 0, win_len > fft_len, hop outside 1 .. win_len.
                             fft_len 512 runs the FFT kernels, any other even fft_len the framing / synthesis GEMMs and their transposes;
                             ConvLayer (model 9, tools_for_model.py:199-425, csrc/plan_layers.cpp; B = batch, L = input frames T): [0] kind (0 ComplexConv2d, 1 ComplexConvTranspose2d,
                             2 RealConv2d, 3 RealConvTranspose2d), [1] C_in, [2] C_out (complex kinds: real + imaginary, even), [3] KH (1 .. 7), [4] KW (1 .. 4), [5] frequency stride
                             (1 .. 2; the time stride is 1), [6] padding F (< KH), [7] padding T (< KW), [8] causal (kinds 0, 2: time padding on the left only), [9] output padding F
                             (kinds 1, 3; < stride), [10] input bins F.  I/O fp32 in the reference layout: x [B][C_in][F][T] -> y [B][C_out][Fo][To]; grad_y -> grad_x and the flat
                             gradients (parameters real_conv / imag_conv or conv, .weight then .bias).  Storage inside the plan: act_dtype, channels padded to multiples of 8.
                             A geometry without an output bin or frame is refused with its numbers;
                             ComplexBatchNorm (model 10, tools_for_model.py:430-607; B = batch, L = S, the product of the trailing dimensions): [0] num_features (real + imaginary,
                             a multiple of 8), [1] eps, [2] momentum, both as float32 bit patterns.  x [B][C][S] -> y; grad_y -> grad_x; parameters Wrr Wri Wii Br Bi, buffers
                             RMr RMi RVrr RVri RVii.  training = 1: batch statistics, running update; 0: running statistics, buffers untouched;
                             ComplexLSTM (model 11, tools_for_model.py:141-181, csrc/plan_clstm.cpp; B = sequences, L = frames T): [0] input size per part I, [1] hidden size per
                             part H (a multiple of 8), [2] projection size per part P (0: no r_trans / i_trans), [3] bidirectional.  I/O, batch-major fp32, IP = roundup(I, 8):
                             x [B][T][2 IP] (real | imaginary, pad columns zero) -> y [B][T][2 P] (real | imaginary); P = 0: the workspace buffer `hc` [D][B][T][2 H] in the
                             activation dtype (direction, real | imaginary).  grad_y ([B][T][2 P], or [D][B][T][2 H]) -> grad_x [B][T][2 IP] and the flat gradients (parameters
                             real_lstm.*, imag_lstm.*, r_trans.*, i_trans.* in torch's order, `_reverse` tensors behind a direction's forward ones) */
  int32_t rnn_layers, rnn_units;
  int32_t mask_mode;      /* 0 'E', 1 'C', 2 'R' (cfg.masking_mode) */
  int32_t lstm_complex;   /* cfg.lstm == 'complex' */
  int32_t skip;           /* cfg.skip_type */
  int32_t act_dtype;      /* 0 fp32, 1 bf16 storage / MFMA dtype */
  int32_t kernel_size;    /* 5 */
  int32_t training;       /* 1 train (batch statistics + backward plan), 0 eval */
  int32_t bn_world;       /* 0/1: BatchNorm statistics of this process only (standard DDP).  N > 1: SyncBN over N ranks - the plan
                             exposes sync points (sefd_plan_num_syncs / sefd_plan_sync) where the caller sum-all-reduces a small
                             statistics buffer between two op ranges; counts are scaled by N.  Makes N ranks x B/N utterances
                             equal to the reference's single process with batch B */
  int32_t grad_buckets;   /* 0/1: one UNPACK at the end of the backward phase.  2 (DCCRN): the gradients of decoder + LSTM (the flat
                             range [sefd_plan_grad_bucket elem, end)) are final at op `bucket op` of the backward phase, BEFORE the encoder
                             backward: a data-parallel caller starts their all-reduce there (sefd_plan_run_cb) and it rides under the
                             encoder's dgrad / wgrad kernels; the encoder range follows at the end of the phase (reverse layer order) */
  int32_t use_cbn;        /* DCCRN(use_cbn=True) (models.py:25, 76, 120): ComplexBatchNorm (tools_for_model.py:430-607) instead of nn.BatchNorm2d */
  int32_t window;         /* ConvSTFT / ConviSTFT window (tools_for_model.py:17-20): 0 periodic Hann (cfg.window = 'hanning'), 1 rectangular (win_type None),
                             2 the table `window_values` (any other scipy.signal.get_window(name, win_len, fftbins=True): the host evaluates it) */
  int32_t cbn_sync;       /* use_cbn with bn_world > 1: 1 builds the ComplexBatchNorm SyncBN plan (fp64 sync points); 0 refuses it */
  const double* window_values;   /* window == 2: win_len doubles, read during sefd_plan_create only */
} sefd_model_config;

enum { SEFD_ARENA_WS = 0, SEFD_ARENA_PARAM = 1, SEFD_ARENA_GRAD = 2, SEFD_ARENA_STATE = 3, SEFD_ARENA_CONST = 4, SEFD_ARENA_IO = 5,
       SEFD_ARENA_COUNT = 6 };
enum { SEFD_PHASE_FWD = 0, SEFD_PHASE_BWD = 1 };
enum { SEFD_LOSS_MSE = 0, SEFD_LOSS_SDR = 1, SEFD_LOSS_SISNR = 2, SEFD_LOSS_SISDR = 3 };

/* ---- plan life cycle (host only) ---------------------------------------------------------------- */
sefd_plan* sefd_plan_create(const sefd_model_config* cfg);        /* replaces models.DCCRN.__init__ (models.py:17-172) */
void sefd_plan_destroy(sefd_plan* p);
const char* sefd_plan_error(const sefd_plan* p);                  /* "" when the plan is valid */
int64_t sefd_plan_arena_bytes(const sefd_plan* p, int arena);
int32_t sefd_plan_frames(const sefd_plan* p);                     /* T */
/* parameters in reference state_dict order; kind 0 = trainable (A_PARAM / A_GRAD), 1 = buffer (A_STATE) */
int32_t sefd_plan_num_params(const sefd_plan* p, int kind);
const char* sefd_plan_param_name(const sefd_plan* p, int kind, int i);
int64_t sefd_plan_param_offset(const sefd_plan* p, int kind, int i);   /* in elements */
int64_t sefd_plan_param_numel(const sefd_plan* p, int kind, int i);
int32_t sefd_plan_param_shape(const sefd_plan* p, int kind, int i, int64_t* shape4);  /* returns ndim */
/* named workspace / io buffers (tests, debugging). returns 0 if found */
int32_t sefd_plan_buffer(const sefd_plan* p, const char* name, int32_t* arena, int64_t* off, int64_t* bytes, int32_t* dtype);
/* SyncBN (bn_world > 1): sync point i says "after op `op` of `phase` has been enqueued, sum-all-reduce `count` elements
   (dtype 0 fp32 / 1 fp64) at byte offset `off` of arena `arena` over the ranks, then continue with op + 1". */
int32_t sefd_plan_num_syncs(const sefd_plan* p);
int32_t sefd_plan_sync(const sefd_plan* p, int i, int32_t* phase, int32_t* op, int32_t* arena, int64_t* off, int64_t* count, int32_t* dtype);
int32_t sefd_plan_num_buffers(const sefd_plan* p);
const char* sefd_plan_buffer_name(const sefd_plan* p, int i);
/* host image of the constant arena (STFT bases, OLA normaliser, index tables): copy it to device memory once */
const void* sefd_plan_const_data(const sefd_plan* p);
/* op lists (POD array of sefd::Op, see csrc/sefd_desc.h) */
int32_t sefd_plan_num_ops(const sefd_plan* p, int phase);
const void* sefd_plan_ops(const sefd_plan* p, int phase);
int32_t sefd_op_size(void);
/* per-op summary for measurement: out = {kind, tag, M, N, K (true run length), operand dtype, algorithmic flops, algorithmic bytes};
   out[5] of a GEMM op: bits 0-7 operand dtype, bits 8-39 descriptor flags, bits 48-55 (RUNGEMM) the kernel family a launch would pick under the
   tuning table of the moment: 1 first-layer, 2 wide-tile, 3 direct-operand, 4 tiled (one tile per workgroup), 5 persistent tiled, 0 none */
int32_t sefd_plan_op_info(const sefd_plan* p, int phase, int i, int64_t* out8);

/* ---- execution (device) --------------------------------------------------------------------------
 * arenas: SEFD_ARENA_COUNT device pointers.  Runs ops [first, last) of the phase on `stream`.
 * Forward  = DCCRN.forward  (models.py:176-284): IO.wav -> IO.out_wav, IO.out_real, IO.out_imag.
 * Backward = autograd of it: IO.grad_wav / grad_real / grad_imag -> A_GRAD (all parameters).
 * Returns 0, or < 0: -1 invalid plan, -2 a launch failed, -3 stream / event creation failed, -5 a cluster-LSTM launch of an EARLIER
 * call gave up waiting for a peer workgroup (bounded spin ran out: co-residency lost on a shared / preempted GPU) - that step's
 * results are invalid; the flag is cleared by the call that reports it. */
int32_t sefd_plan_run(const sefd_plan* p, int phase, int first, int last, void* const* arenas, void* stream);
/* grad_buckets == 2: index (backward phase) of the UNPACK op that completes the first gradient bucket and the first flat element
   of that bucket; returns -1 when the plan has a single bucket. */
int32_t sefd_plan_grad_bucket(const sefd_plan* p, int32_t* op, int64_t* elem);
/* The same as an explicit element range [lo, hi) of the flat gradient arena: DCCRN / CRN complete the TAIL of the arena first (decoder + LSTM,
 * hi = end), FullSubNet the FRONT (the full-band model: its weight gradients run on the main stream while the sub-band model's still
 * occupy the second lane, lo = 0). */
int32_t sefd_plan_grad_bucket_range(const sefd_plan* p, int32_t* op, int64_t* lo, int64_t* hi);
/* Whole phase as sefd_plan_run(first = 0, last = -1), and `cb(ctx)` is called on the host right after op `at` has been enqueued on
   `stream` (everything up to and including that op is ordered before whatever the callback enqueues behind an event on `stream`). */
int32_t sefd_plan_run_cb(const sefd_plan* p, int phase, void* const* arenas, void* stream, int at, void (*cb)(void*), void* ctx);
/* The same with run flags (cb may be NULL, at = -1).  SEFD_RUN_WAVE_ONLY: the caller's loss is a function of the enhanced WAVEFORM only
 * (trainer.py:27-39 without a perceptual term): the reference-layout copies out_real / out_imag [B][NF][T] are not produced and the
 * (all-zero) gradient with respect to them is not accumulated - DCCRN.forward's first two return values are not valid after such a run. */
#define SEFD_RUN_WAVE_ONLY 1
int32_t sefd_plan_run_flags(const sefd_plan* p, int phase, void* const* arenas, void* stream, int flags, int at, void (*cb)(void*), void* ctx);
/* Measurement only (bench.py's in-situ roofline leg): the whole phase in its real two-stream schedule with a HIP event pair around every
   op on the stream it is launched on; synchronises; ms[i] = duration of op i while the other lane runs beside it.  n >= number of ops. */
int32_t sefd_plan_run_timed(const sefd_plan* p, int phase, void* const* arenas, void* stream, float* ms, int32_t n);

/* ---- losses (tools_for_loss.py:17-94, models.py:315-323) ---------------------------------------
 * est, tgt: fp32 [B][L] device.  ws: fp32 device scratch of sefd_loss_ws_floats(B) floats.
 * forward writes the scalar loss to loss_out[0]; backward writes grad_est[B][L] = d(loss)/d(est) * grad_scale[0] (grad_scale NULL: 1).
 * Both return -1, and launch nothing, for a kind outside SEFD_LOSS_MSE .. SEFD_LOSS_SISDR or B < 1 or L < 1.
 * est and tgt need 4-byte alignment only: rows are read as float4 when L % 4 == 0 and both base pointers are 16-byte aligned, element by
 * element otherwise (same result, lower bandwidth). */
int64_t sefd_loss_ws_floats(int32_t B);
int32_t sefd_loss_forward(int kind, const float* est, const float* tgt, int32_t B, int32_t L, float* ws, float* loss_out, void* stream);
int32_t sefd_loss_backward(int kind, const float* est, const float* tgt, int32_t B, int32_t L, const float* ws,
                           const float* grad_scale, float* grad_est, void* stream);

/* Short rows: FullSubNet.loss (models.py:674-682) applies the same four losses to cRM / cIRM tensors [B, F, T, 2], whose last axis - the
 * reduction axis of tools_for_loss.py:17-94 - has two elements, and trainer.py:107 passes the network output in the `target` slot.
 * est, tgt: fp32 [R][L] device, L <= 16, same argument roles as above (SDR: est = s2, tgt = s1; SI-SNR: est = s1, tgt = s2; SI-SDR:
 * est = estimation, tgt = reference).  backward writes d(loss)/d(est) and / or d(loss)/d(tgt) (either pointer may be NULL), times grad_scale[0]. */
int64_t sefd_loss_rows_ws_floats(int64_t R);
int32_t sefd_loss_rows_forward(int kind, const float* est, const float* tgt, int64_t R, int32_t L, float* ws, float* loss_out, void* stream);
int32_t sefd_loss_rows_backward(int kind, const float* est, const float* tgt, int64_t R, int32_t L, const float* ws, const float* grad_scale,
                                float* grad_est, float* grad_tgt, void* stream);

/* SI-SDR under data parallelism (no counterpart in the reference, which is single-process; the arithmetic it must reproduce is
 * tools_for_loss.py:91-94: `ratio = torch.mean(ratio)` over the WHOLE batch, then the log).  After sefd_loss_forward / sefd_loss_rows_forward
 * with kind SI-SDR, ws + sefd_loss_dp_offset(n, rows) holds this rank's { sum of ratios, row count } (n = B, or R with rows = 1): the host
 * sum-all-reduces those TWO floats in place over the ranks and calls sefd_loss_dp_finish, which rewrites loss_out[0] to the global-batch
 * loss and re-scales the saved row coefficients so that the following sefd_loss_*_backward yields world x d(global loss)/d(est) for this
 * rank's rows (the gradient exchange sums over ranks, Adam applies 1 / world). */
int64_t sefd_loss_dp_offset(int64_t n, int32_t rows);
int32_t sefd_loss_dp_finish(int32_t rows, int64_t n, float* ws, int32_t world, float* loss_out, void* stream);

/* ---- LMS log-mel perceptual loss (tools_for_loss.py:120-249 + the magnitude step of models.py:306-312) ------------
 * clean_* / est_*: fp32 [B][NF][T] device (reference layout).  If the *_i pointers are NULL the *_r arrays are magnitudes
 * already (get_array_lms_loss(clean_mags, est_mags) signature); otherwise mag = sqrt(r^2 + i^2 + 1e-7) is fused in.
 * bands: int32 [nbands][4] = {first bin, taps, weight offset, scale index}; weights: the triangle taps (melFilterBank);
 * band_bins: the largest first bin + taps over the band rows, from the host that built them - a table that reaches past NF is refused (-1);
 * scale_sizes_host: HOST int32[nscales] = filters per scale (16, 32, 64).  rowloss_ws: fp32 [B*T] device scratch. */
int32_t sefd_lms_forward(const float* clean_r, const float* clean_i, const float* est_r, const float* est_i, int32_t B, int32_t NF, int32_t T,
                         const int32_t* bands, const float* weights, int32_t nbands, int32_t band_bins, const int32_t* scale_sizes_host,
                         int32_t nscales, int32_t nfft, float* rowloss_ws, float* loss_out, void* stream);
int32_t sefd_lms_backward(const float* clean_r, const float* clean_i, const float* est_r, const float* est_i, int32_t B, int32_t NF, int32_t T,
                          const int32_t* bands, const float* weights, int32_t nbands, int32_t band_bins, const int32_t* scale_sizes_host,
                          int32_t nscales, int32_t nfft, const float* grad_scale, float* grad_est_r, float* grad_est_i, void* stream);

/* ---- PMSQE perceptual loss (call chain tools_for_loss.py:253-269 `get_array_pmsqe_loss`, models.py:313-314) ----------------------
 * The arithmetic is third-party (asteroid SingleSrcPMSQE + PITLossWrapper('pw_pt') + asteroid_filterbanks STFTFB / Encoder / mag), absent
 * from the reference tree and unversioned there: PARITY UNPINNED; this is the published algorithm as oracle/pmsqe.py restates it.
 * est / clean: fp32 [B][L] device waves, L a whole number of seconds (the reference's view(N, -1, fs)), at most 6 seconds (PIT over
 * the seconds enumerates the permutations).  power: 1 = the loss works on the power spectrum re^2 + im^2 (the paper's definition; the host default),
 * 0 = on the magnitude sqrt(re^2 + im^2 + 1e-8) that transforms.mag hands over in the reference call chain, taken literally.
 * tab: fp32 [sefd_pmsqe_table_floats()] device = thr[49] zp[49] width[49] corr[49] aterm[49] mask[257] (at 245), then at 512 the
 * windowed DFT tables cos [512][257], -sin [512][257] and their transposes [257][512] x 2;  itab: int32 [64 + 257] device = prefix sums
 * of the FFT bins per Bark band [50] and, at 64, the band of every bin (-1: none).  ws: fp32 [sefd_pmsqe_ws_floats(B, L)] device, must
 * stay untouched between forward and backward.  backward writes d loss / d est * *grad_scale into grad_est [B][L]. */
int64_t sefd_pmsqe_table_floats(void);
int64_t sefd_pmsqe_ws_floats(int32_t B, int32_t L);
int32_t sefd_pmsqe_forward(const float* est, const float* clean, int32_t B, int32_t L, int32_t power, const float* tab, const int32_t* itab,
                           float* ws, float* loss_out, void* stream);
int32_t sefd_pmsqe_backward(int32_t B, int32_t L, int32_t power, const float* tab, const int32_t* itab, float* ws, const float* grad_scale,
                            float* grad_est, void* stream);

/* ---- FullSubNet training targets (trainer.py:100-104; tools_for_model.py:683-717) -------------------------------------
 * noisy_c64 / clean_c64: interleaved complex64 [n] (the torch.stft outputs).  Any of mag / phase / cirm may be NULL.
 * mag = |noisy| (mag_phase), phase = angle(noisy), cirm [n][2] = compress_cIRM(build_complex_ideal_ratio_mask(noisy, clean)). */
/* On-GPU SNR mixing of a batch (replaces the offline generate_noisy_data.py:46-67 `generate_noisy_wav`, the random segment start chosen by
   the caller): noisy[b] = speech[b] + alpha_b * noise[noise_start[b] : +L], alpha_b = sqrt(10^(-snr_db[b]/10) * P_speech / (P_noise + 1e-6)) with
   the powers taken after removing the DC bias; quantize != 0 adds the reference's int16 file round trip.  speech / noisy [B][L] fp32, noise a
   flat fp32 bank, ws: 4 * B doubles.  All device pointers. */
int32_t sefd_mix_snr(const float* speech, const float* noise, const int64_t* noise_start, const float* snr_db, int32_t B, int32_t L,
                     int32_t quantize, double* ws, float* noisy, void* stream);
/* ---- Composite measure frame analysis (reference composite.m:151-562, called by tools_for_estimate.py:24-33) ------------------------------
 * For a batch of clean / processed pairs (fp32 [B][L] device, same length): per 30 ms frame (win = round(30 fs / 1000), hop floor(win / 4),
 * window 0.5 (1 - cos(2 pi n / (win + 1))), floor(L / hop - win / hop) frames, eps = 2^-52 added to every sample) the WSS distance
 * (composite.m:151-384), the LLR (:385-491, LPC order 10 below 10 kHz, else 16) and the segmental SNR (:492-562); then per utterance
 * out[b][0] = mean of the round(0.95 n) smallest LLRs, out[b][1] = the same of the WSS values, out[b][2] = mean segSNR (fp64 device [B][3]).
 * No PESQ term and no [1, 5] clamp: the regression lives with the caller.  Bit-identical from run to run and independent of the rest of the
 * batch.  ws: sefd_composite_ws_bytes(B, L, fs) bytes of device memory.  Returns 0, -1 bad arguments (B outside 1..65535, L < win, NULL),
 * -2 launch failure, -3 more than SEFD_COMPOSITE_MAX_FRAMES frames per utterance, -4 fs whose n_fft = 2^nextpow2(2 win) is outside 256..4096
 * (supported: about 4.3 to 68 kHz).  An utterance with L >= win but no whole frame (L < win + hop) gets NaN, the mean of nothing. */
#define SEFD_COMPOSITE_MAX_FRAMES (1 << 24)
int64_t sefd_composite_ws_bytes(int32_t B, int32_t L, int32_t fs);
int32_t sefd_composite_frames(const float* clean, const float* enhanced, int32_t B, int32_t L, int32_t fs, void* ws, double* out, void* stream);
/* ---- STOI on the device (Taal et al. 2011 with the conventions of pystoi 0.3.3; reference tools_for_estimate.py:90-96) ---------------------
 * The host scorer sefd_stoi_batch (include/sefd_scorers.h) restated in HIP, extended = False: for a batch of clean / estimated pairs (fp32
 * [B][L] device, rate fs) resample to 10 kHz (resample_poly, Kaiser-windowed sinc; skipped at fs == 10000), drop the 256-sample Hann frames
 * (hop 128, frames start while i < n - 256) of the clean signal more than 40 dB below its loudest, overlap-add the K kept ones, take the
 * 512-point STFT of the result, 15 one-third octave band envelopes from 150 Hz, and the clipped, normalised correlation over every 30-frame
 * segment: out[b] (fp64 device [B]) is its mean, or 1e-5 where fewer than 30 frames are left.  fp64 after the load.  Bit-identical from run
 * to run and independent of the rest of the batch; the whole call (one table copy, five launches) is enqueued on `stream`, the host never
 * waits, allocates or frees; safe from several host threads.  ws: sefd_stoi_ws_bytes(B, L, fs) bytes of device memory.
 * Returns 0, -1 bad arguments (NULL, B outside 1..65535, L < 1, fs < 1), -2 launch failure, -3 an utterance of more than
 * SEFD_STOI_MAX_SAMPLES samples at fs or at 10 kHz (2^26: 23 minutes at 48 kHz), -4 a rate whose reduced ratio 10000 / fs has a factor above
 * 1024 (8, 10, 11.025, 16, 22.05, 24, 32, 44.1, 48 and 96 kHz all pass).  sefd_stoi_ws_bytes is host arithmetic only and returns the same
 * negative codes for the same arguments. */
#define SEFD_STOI_MAX_SAMPLES (1 << 26)
int64_t sefd_stoi_ws_bytes(int32_t B, int32_t L, int32_t fs);
int32_t sefd_stoi_gpu(const float* clean, const float* est, int32_t B, int32_t L, int32_t fs, void* ws, double* out, void* stream);
/* The same scorer with flags.  Bit 0 (SEFD_STOI_EXTENDED): extended STOI (Jensen & Taal 2016) - same resampling, silent-frame cut, band
 * envelopes and 30-frame segments, then per segment the 15 x 30 clean and estimate matrices are normalised alike, every row (band over time)
 * to zero mean and divided by (norm + eps), then every column (frame over bands) likewise; the segment's score is sum(x_n y_n) / 30 and out[b]
 * the mean over the segments (1e-5 below 30 frames); no norm-ratio scaling, no clip; one wave per segment, fixed summation order, no atomics.
 * Bit 1 (SEFD_STOI_KEEP): the workspace is left as sefd_stoi_backward reads it and is larger (the frame -> kept-position map, the estimate at
 * 10 kHz in fp64, and the backward's own buffers, 450 doubles per segment the largest).  flags == 0 is sefd_stoi_gpu, bit for bit; any other
 * bit set is -1.  sefd_stoi_ws_bytes_ex sizes the workspace for the same flags (host arithmetic, the same negative codes).
 *
 * sefd_stoi_backward: the gradient of sum_b grad_out[b] out[b] with respect to the estimate, after sefd_stoi_gpu_ex ran with the keep bit on
 * the same (B, L, fs, flags, ws).  grad_out fp64 device [B]; grad_est fp32 device [B][L], every element written, fp64 arithmetic rounded
 * once at the store.  The clean signal, the selection of frames it decides and the resampling filter are constants.  Stages in reverse, all
 * gathers (no atomics; bit-identical from run to run, independent of the rest of the batch): per-segment cotangents of the estimate's band
 * envelopes (STOI through the clip - a clipped entry passes nothing directly - the scale c and the normalisation; ESTOI through both
 * normalisations), their sum per envelope element in ascending segment order, per compacted frame the spectrum again and the
 * inverse-direction 512-point transform of G[k] = g_yt Y[k] / yt times the window, per 10 kHz sample its at most two kept frames, and the
 * transpose of the resampler (at 10 kHz the cast alone).  Samples that only dropped frames cover, the last 128 compacted samples and an
 * utterance scored 1e-5 get exactly 0.  Where torch would give NaN - a band envelope that is exactly 0 under the square root, a norm that
 * is exactly 0 under a division - the gradient through that term is 0.  Enqueued on `stream`; the host never waits, allocates or frees.
 * Returns 0, -1 bad arguments (NULL, the keep bit missing, unknown bits), -2 launch failure, -3 / -4 as sefd_stoi_gpu. */
#define SEFD_STOI_EXTENDED 1
#define SEFD_STOI_KEEP 2
int64_t sefd_stoi_ws_bytes_ex(int32_t B, int32_t L, int32_t fs, int32_t flags);
int32_t sefd_stoi_gpu_ex(const float* clean, const float* est, int32_t B, int32_t L, int32_t fs, int32_t flags, void* ws, double* out, void* stream);
int32_t sefd_stoi_backward(int32_t B, int32_t L, int32_t fs, int32_t flags, void* ws, const double* grad_out, float* grad_est, void* stream);
int32_t sefd_fsn_targets(const float* noisy_c64, const float* clean_c64, int64_t n, float* mag, float* phase, float* cirm, void* stream);
/* Its backward, one pass over the interleaved complex inputs (fp32 device, n bins).  Cotangents g_mag, g_phase [n] and g_cirm [n][2], each NULL for
 * "no gradient"; d_noisy / d_clean [n][2] (NULL: not wanted) receive (dL/dre, dL/dim) of that argument and are written once, no accumulation.
 *   mag, phase: d re = g_m re / m - g_p im / m^2, d im = g_m im / m + g_p re / m^2; both 0 where m == 0 (torch: NaN)
 *   cIRM: through K (1 - e^{-C v}) / (1 + e^{-C v}), K = 10, C = 0.1 (derivative 0 on the clamped arm v <= -100) and the ratio with den = |noisy|^2 + float32 eps.
 * clean_c64 may be NULL when g_cirm is.  Returns 0, -1 bad arguments, -2 launch failure. */
int32_t sefd_fsn_targets_backward(const float* noisy_c64, const float* clean_c64, int64_t n, const float* g_mag, const float* g_phase, const float* g_cirm,
                                  float* d_noisy, float* d_clean, void* stream);

/* ---- BaseModel on its own (tools_for_model.py:801-1185): the seven norms and `unfold` on tensors in the reference's layout ----------
 * x, y, grad_y, grad_x: fp32 device, [rows][F][T] with the frames contiguous.  A row is what the statistics are taken over per frame:
 * B * C rows for cumulative_laplace_norm / cumulative_layer_norm on [B, C, F, T], B rows for the three recurrence norms on [B, F, T].  The two
 * offline norms take one mean (and std) over ALL F * T values of a row: pass rows = B, F = C * F * T, T = 1 (any split of the row's
 * values into F x T gives the same result).
 * kind: SEFD_NORM_* below; 0..3 in the order of FSN_NORMS.  sample_len: the recurrence norms' training sample length (ignored by kinds 0..3).
 * ws: sefd_norm_ws_floats(kind, rows, F, T) floats of device memory, 8-byte aligned, owned by ONE forward / backward pair.  It begins with the
 * per-(row, frame) statistics as doubles { mean, std }, which forward writes and backward reads (with the same x); the rest is the pair's scratch (the
 * per-frame partial sums of each pass, then the backward's per-frame coefficients), and the backward OVERWRITES it - its ws is const for the statistics only.
 * The tensors need 4-byte alignment only: frames are moved 16 bytes at a time when T % 4 == 0 (offline: F * T % 4 == 0) and every tensor pointer is
 * 16-byte aligned, element by element otherwise (same values).
 * Both return -1, and launch nothing, for a kind out of range, a size below 1, sample_len < 1 (kinds 4..6), sband_forgetting with F < 2,
 * offline_gaussian with fewer than 2 values per row, a NULL or misaligned pointer; -2: launch failure.  They only enqueue: no allocation,
 * no synchronisation, no state inside the library.  No atomics: results are bit-identical from run to run, and a row's result depends on that row alone. */
#define SEFD_NORM_OFFLINE_LAPLACE 0
#define SEFD_NORM_CUMULATIVE_LAPLACE 1
#define SEFD_NORM_OFFLINE_GAUSSIAN 2
#define SEFD_NORM_CUMULATIVE_LAYER 3
#define SEFD_NORM_FORGETTING 4
#define SEFD_NORM_SBAND_FORGETTING 5
#define SEFD_NORM_HYBRID 6
int64_t sefd_norm_ws_floats(int32_t kind, int32_t rows, int32_t F, int32_t T);
int32_t sefd_norm_forward(int32_t kind, const float* x, int32_t rows, int32_t F, int32_t T, int32_t sample_len, float* ws, float* y, void* stream);
int32_t sefd_norm_backward(int32_t kind, const float* x, const float* grad_y, int32_t rows, int32_t F, int32_t T, int32_t sample_len,
                           const float* ws, float* grad_x, void* stream);
/* BaseModel.unfold: x [B][C][F][T] -> out [B][F][C][2 n + 1][T], out[b, f, c, k, :] = x[b, c, reflect(f - n + k), :] (F.pad(mode="reflect"));
 * n = 0 is the permute to [B][F][C][1][T].  backward: grad_x[b, c, j, :] = the sum, in a fixed order, of the grad_out rows that read bin j.
 * -1, and nothing launched, for n < 0 or n >= F (torch's reflect pad refuses it), a size below 1 or a NULL pointer. */
int32_t sefd_unfold_forward(const float* x, int32_t B, int32_t C, int32_t F, int32_t T, int32_t n, float* out, void* stream);
int32_t sefd_unfold_backward(const float* grad_out, int32_t B, int32_t C, int32_t F, int32_t T, int32_t n, float* grad_x, void* stream);

/* ---- Adam (torch.optim.Adam defaults, train_interface.py:59) on flat fp32 buffers ------------------
 * step is 1-based. */
int32_t sefd_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t step,
                       float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);
/* The same update, skipped entirely (parameters and moments untouched) while *skip_if_set != 0.  skip_if_set = sefd_plan_status_word(plan)
 * of the plan that produced `grad`: a kernel of that plan that had to give up (bounded hand-over waits of the cluster LSTM kernels on a
 * shared / preempted GPU) sets the word, so a garbage gradient never reaches the parameters; NULL = unconditional. */
int32_t sefd_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t step,
                               float lr, float beta1, float beta2, float eps, float grad_scale, const int32_t* skip_if_set, void* stream);
/* Per-plan status word (0 = fine), kept twice: host-mapped (what sefd_plan_run / sefd_plan_status read) and in device memory (what
 * sefd_plan_status_word returns, for sefd_adam_step_guarded).  sefd_plan_run returns -5 while it is set (sticky); sefd_plan_status reads
 * it (after a stream synchronisation for a definite answer) and optionally clears both copies; sefd_plan_status_set sets both from the
 * host (test hook: what a kernel that gives up does). */
const int32_t* sefd_plan_status_word(const sefd_plan* p);
/* Data parallel: a rank whose status word is set must not hand its gradient to the others as if it were good, and the replicas must take the
 * same decision.  sefd_plan_status_poison (enqueued behind the backward, in front of the last gradient all-reduce) overwrites *grad_elem - an
 * element of that last bucket - with NaN when the word is set; the sum carries the NaN to every rank; sefd_adam_step_guarded_dp skips the
 * update on every rank while *skip_if_nan is NaN (and, as before, while *skip_if_set != 0).  No extra collective. */
int32_t sefd_plan_status_poison(const sefd_plan* p, float* grad_elem, void* stream);
int32_t sefd_adam_step_guarded_dp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t step, float lr, float beta1,
                                  float beta2, float eps, float grad_scale, const int32_t* skip_if_set, const float* skip_if_nan, void* stream);
int32_t sefd_plan_status(const sefd_plan* p, int32_t clear);
int32_t sefd_plan_status_set(const sefd_plan* p);

/* ---- Grouped optimizer step (optim.hip): Adam / AdamW with weight decay, amsgrad, parameter groups, frozen parameters and global-norm clipping
 * on the same flat fp32 buffers.  sefd_adam_step* above stay what they are; this is the path for every configuration they cannot express.
 *
 * Chunk table.  The part of the flat buffer that is updated is listed as chunks of at most SEFD_OPTIM_CHUNK elements: [begin, begin + count) in group
 * `group`.  No chunk crosses a parameter tensor's boundary (a tensor is cut into full chunks and one remainder), chunks do not overlap, and an
 * element that no chunk covers is frozen: its value and moments are neither read nor written.  The caller builds the table once, keeps one copy in
 * host memory (the entry points check it against n on every call: a wrong table is refused, not launched) and one in device memory (what the kernels
 * read).  One workgroup of 256 threads takes one chunk - up to 8192 chunks every chunk has its own workgroup, beyond that a workgroup goes on to
 * chunk blockIdx.x + gridDim.x, ... with the grid sized so that all make the same number of trips; within a chunk the elements in front of
 * the first 16-byte line of the buffers and behind the last whole one are handled one float at a time, the body as one float4 per thread.  That
 * needs all buffers of a call to sit alike relative to 16 bytes (torch allocations do); otherwise the whole chunk goes one float at a time.  For the
 * streaming order, sort the table by begin. */
#define SEFD_OPTIM_CHUNK 1024
#define SEFD_OPTIM_MAX_GROUPS 8
#define SEFD_OPTIM_DECOUPLED 1u /* flags bit 0: AdamW's decay, p *= 1 - lr * weight_decay; otherwise L2: g += weight_decay * p */
#define SEFD_OPTIM_AMSGRAD 2u   /* flags bit 1: max_exp_avg_sq = max(max_exp_avg_sq, exp_avg_sq) is kept and used in the denominator */
typedef struct sefd_optim_chunk {
  int64_t begin;
  int32_t count; /* 1 .. SEFD_OPTIM_CHUNK */
  int32_t group; /* 0 .. ngroups - 1 */
} sefd_optim_chunk;
typedef struct sefd_optim_group {
  float lr, beta1, beta2, eps, weight_decay;
  uint32_t flags;
} sefd_optim_group;
/* Global L2 norm of grad * grad_scale over the chunks of the table (table_host == table_dev == NULL: over all n elements) and the clip
 * coefficient of torch.nn.utils.clip_grad_norm_: out[0] = norm, out[1] = min(1, max_norm / (norm + 1e-6)); both stay in device memory.  Squares
 * and sums are fp64; two launches (per-workgroup partial sums, then one workgroup that adds them in index order), no atomics: the same data give
 * the same bits.  A non-finite norm (a NaN or Inf element, sefd_plan_status_poison's among them) is written as it is and out[1] becomes NaN;
 * norm 0 gives 1.  ws: sefd_grad_norm_ws_floats(n) floats on an 8-byte boundary.  -1, nothing launched: n < 1, max_norm < 0 or NaN, a NULL or
 * misaligned pointer, one table pointer without the other, nchunks < 1 with a table, a chunk outside [0, n) or with count outside 1 .. SEFD_OPTIM_CHUNK. */
int64_t sefd_grad_norm_ws_floats(int64_t n);
int32_t sefd_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, const sefd_optim_chunk* table_host,
                       const sefd_optim_chunk* table_dev, int32_t nchunks, float* ws, float* out, void* stream);
/* ONE launch for all groups.  Per element of a chunk, in torch's order:  g = grad * grad_scale * coef[0] (coef NULL: 1);  weight_decay != 0:
 * decoupled p *= 1 - lr * weight_decay (as p - (lr * weight_decay) * p, one fma), else g += weight_decay * p;  m, v as in sefd_adam_step;  amsgrad: vmax = max(vmax, v) and the denominator
 * takes vmax;  p -= lr / bc1 * m / (sqrt(v or vmax) / sqrt(bc2) + eps), the bias corrections formed on the host in double from `step` (1-based, one
 * count for all groups).  grad is only read: clipping is the factor coef, typically out + 1 of sefd_grad_norm on the same stream.  The whole update
 * is skipped, before anything is written, while *skip_if_set != 0, *skip_if_nan is NaN (both as in sefd_adam_step_guarded_dp) or coef[0] is NaN.
 * max_exp_avg_sq may be NULL when no group has SEFD_OPTIM_AMSGRAD.  Traffic: 28 bytes per element, 36 with amsgrad.
 * -1, nothing launched: n < 1, step < 1, ngroups outside 1 .. SEFD_OPTIM_MAX_GROUPS, a NULL buffer, groups or table pointer, nchunks < 1, an amsgrad
 * group without max_exp_avg_sq, a chunk outside [0, n), with count outside 1 .. SEFD_OPTIM_CHUNK or with a group outside 0 .. ngroups - 1. */
int32_t sefd_optim_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n, int32_t step,
                        const sefd_optim_group* groups, int32_t ngroups, const sefd_optim_chunk* table_host, const sefd_optim_chunk* table_dev,
                        int32_t nchunks, float grad_scale, const float* coef, const int32_t* skip_if_set, const float* skip_if_nan, void* stream);

/* ---- tuning table ------------------------------------------------------------------------------------
 * The planner's and the launchers' tuning knobs (tile thresholds, fusions, lane placement, ...: INTEGRATION.md section 6) live in ONE process-wide
 * table, not in the environment: a plan is a function of its sefd_model_config and of this table at the moment sefd_plan_create runs; launch- and
 * run-time knobs are read on every launch / run.  The table starts from the single environment variable SEFD_TUNING="KNOB=value,KNOB=value" (parsed
 * once, the first time the table is consulted) and is changed by these calls.  value NULL unsets a knob; sefd_tuning_get returns NULL for a knob that
 * is not set (then the built-in default applies); sefd_tuning_clear returns the table to the pairs of SEFD_TUNING (empty when it is not set).  The reference has
 * no counterpart (its behaviour is fixed by config.py); nothing here changes results beyond floating-point summation order. */
/* One launch of the layout kernel behind OP_NCHW_CL on raw device pointers (tests, tools/convlayers_bench.py): nchw fp32 [B][C][F][T], cl (dt 0 fp32, 1 bf16)
 * [B][Tcl][F][Cpad] (Cpad a multiple of 8, >= C), nchw frame t = cl frame t + t_off (T + t_off <= Tcl); mode 0 / 2: nchw -> cl (pad channels zero), 1 / 3: cl -> nchw.
 * Returns 0, -1 for arguments outside that domain. */
int32_t sefd_nchw_cl(void* nchw, void* cl, int32_t B, int32_t C, int32_t Cpad, int32_t F, int32_t T, int32_t Tcl, int32_t t_off, int32_t dt, int32_t mode,
                     void* stream);
void sefd_tuning_set(const char* knob, const char* value);
const char* sefd_tuning_get(const char* knob);
void sefd_tuning_clear(void);

#ifdef __cplusplus
}
#endif
#endif
