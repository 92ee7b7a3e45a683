/*
 * libabd -- MI355X (gfx950) poisoned-audio training hot path, C ABI.
 *
 * The reference (quantum-bitss/Audio-Backdoor-Attack) is pure Python; its drop-in
 * boundary is a set of Python call signatures.  Each entry point below replaces the
 * reference interface cited next to it; the Python host package
 * (audio-backdoor-attack_amd/) binds these with ctypes and re-exports the reference
 * names.
 *
 * Conventions
 *   - Plain pointers and sizes only; no torch types.  Device pointers are HBM
 *     buffers owned by the caller; the library allocates device memory only inside
 *     *_create() (constant tables), never inside a launch.
 *   - Every launch is asynchronous on the given stream (a hipStream_t passed as
 *     void*; NULL = the legacy default stream) and is hipGraph-capture safe.
 *   - Return value: 0 on success, a hipError_t value or ABD_E_* on failure;
 *     abd_last_error() returns a thread-local description.
 */
#ifndef ABD_H_
#define ABD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* abd_stream_t;

#define ABD_OK 0
#define ABD_E_INVALID 1001
#define ABD_E_UNSUPPORTED 1002
#define ABD_E_WORKSPACE 1003

const char* abd_last_error(void);
int abd_version(void);

/* ------------------------------------------------------------------ features
 * Replaces prepare_dataset.py:35-47  MFCC(waveform, sample_rate, n_mfcc, n_fft, hop_length)
 *      (torchaudio T.MFCC: HTK mel, reflect pad) and
 *      utils/daba_selection_tools.py:16-22  librosa_MFCC(waveform, sample_rate, n_mfcc)
 *      (librosa: Slaney mel+norm, constant pad, n_fft 2048 / hop 512).
 * Output layout is what the callers feed the model: (B, 1, T, n_mfcc) fp32,
 * i.e. MFCC(...).numpy().T[np.newaxis] stacked (prepare_dataset.py:65). */
enum { ABD_MEL_HTK = 0, ABD_MEL_SLANEY = 1 };
enum { ABD_PAD_REFLECT = 0, ABD_PAD_CONSTANT = 1 };

typedef struct abd_mfcc_plan abd_mfcc_plan;

int abd_mfcc_plan_create(int sample_rate, int n_fft, int hop_length, int n_mels, int n_mfcc,
                         int mel_kind, int pad_mode, float top_db, int64_t length,
                         abd_mfcc_plan** plan);
void abd_mfcc_plan_destroy(abd_mfcc_plan* plan);
int abd_mfcc_plan_frames(const abd_mfcc_plan* plan);
/* fft_size = M (== n_fft, or the Bluestein length for non-{2,3,5}-smooth n_fft). */
int abd_mfcc_plan_describe(const abd_mfcc_plan* plan, int* fft_size, int* bluestein,
                           int* n_passes, int* radices /* >= 16 ints */);
size_t abd_mfcc_workspace_bytes(const abd_mfcc_plan* plan, int64_t batch);
/* Which kernels a plan runs (tests): what = ABD_MFCC_INFO_*; -1 for an unknown what or a NULL plan.
 *   FAST        1 = a specialised STFT kernel (n_fft 400, 2048, 1103), 0 = the runtime-radix one
 *   PPB, CHUNKS frame pairs per work item, work items per utterance
 *   MEL_PATH    ABD_MFCC_MEL_*: the runtime-radix kernel's loop, or the specialised kernels' half-filter
 *               slots, filter segments, or Bluestein slot table
 *   DCT_KERNEL  ABD_MFCC_DCT_*, for a 16-byte aligned output (an unaligned one takes PLAIN instead of LDS)
 *   BWD_OK      1 = every bin lies in at most two mel filters (abd_mfcc_deploy_backward needs it) */
enum { ABD_MFCC_INFO_FAST = 0, ABD_MFCC_INFO_PPB = 1, ABD_MFCC_INFO_CHUNKS = 2, ABD_MFCC_INFO_MEL_PATH = 3,
       ABD_MFCC_INFO_DCT_KERNEL = 4, ABD_MFCC_INFO_BWD_OK = 5 };
enum { ABD_MFCC_MEL_GENERIC = 0, ABD_MFCC_MEL_HALF_SLOT = 1, ABD_MFCC_MEL_SEGMENTED = 2, ABD_MFCC_MEL_BLUE_SLOTS = 3 };
enum { ABD_MFCC_DCT_PLAIN = 0, ABD_MFCC_DCT_LDS = 1, ABD_MFCC_DCT_MFMA1 = 2, ABD_MFCC_DCT_MFMA2 = 3,
       ABD_MFCC_DCT_MFMA3 = 4 };
int abd_mfcc_plan_info(const abd_mfcc_plan* plan, int what);

/* Trigger injection fused into the feature load / epilogue.
 *   ADD        x + trigger                      ultrasonic.py:75,96 (trigger from
 *                                               utils/ultra_trigger.py:92-111, length L)
 *   SNR_WINDOW x[p:p+Lt] += sqrt(|x|^2/|t|^2 * 10^(-snr/10)) * t      flowmur.py:77-85
 *   HALF_MIX   x/2 outside, (x+t)/2 inside [p, p+Lt)                  flowmur.py:101-106
 *   DEPLOY     s=10^(30/20)|t|/|x|: (s x + t)/(s+1) inside, s x/(s+1) outside
 *                                  utils/flowmur_generate_trigger.py:49-62
 *   DEPLOY_CLAMP  DEPLOY then clamp(-1, 1): the trigger-optimisation input
 *                                  utils/flowmur_generate_trigger.py:91-92
 *   patch      MFCC[t0:t1, c0:c1] = value on poisoned rows        utils/badnet_trigger.py:18-27
 * poison (uint8 per batch row) selects the rows that are injected (NULL = all);
 * position (int32 per batch row) is the window start for the windowed modes. */
enum { ABD_INJECT_NONE = 0, ABD_INJECT_ADD = 1, ABD_INJECT_SNR_WINDOW = 2,
       ABD_INJECT_HALF_MIX = 3, ABD_INJECT_DEPLOY = 4, ABD_INJECT_DEPLOY_CLAMP = 5 };

typedef struct abd_inject {
  int mode;
  const float* trigger;
  int64_t trigger_len;
  const uint8_t* poison;
  const int32_t* position;
  float snr_db;
  int patch;
  int patch_t0, patch_t1, patch_c0, patch_c1;
  float patch_value;
  /* ragged rows (utils/daba_selection_tools.py:70-76): frames[row] = 1 + len/hop of the
   * clip, zero-extended in its row; the top_db max sees only those frames and later
   * frames are set to frame_pad (-200 there).  NULL = every row has all T frames. */
  const int32_t* frames;
  float frame_pad;
  /* optional (round 5): the SNR / DEPLOY scale of every row of the wave TABLE, indexed by the
   * table row (rows[u]), as abd_inject_row_scales() writes it for a resident table whose rows and
   * trigger do not change (flowmur.py mixes the trigger into each clip once, offline).  NULL = the
   * call computes the scales of its batch itself (one extra launch per call). */
  const float* row_scale;
} abd_inject;

/* wave: row-major utterances (row_stride floats apart, plan length samples each) in
 * HBM.  rows (int32[batch], NULL = 0..batch-1) gathers the batch from the table.
 * out: (batch, 1, T, n_mfcc).  workspace: abd_mfcc_workspace_bytes(plan, batch). */
int abd_mfcc_f32(const abd_mfcc_plan* plan, const float* wave, int64_t row_stride,
                 const int32_t* rows, int64_t batch, const abd_inject* inj, float* out,
                 void* workspace, size_t workspace_bytes, abd_stream_t stream);

/* abd_mfcc_f32 with an output-row indirection: batch row u's (T, n_mfcc) block is written at
 * out + out_rows[u] * T * n_mfcc (int32[batch], distinct rows; NULL = u, i.e. abd_mfcc_f32), so a
 * batch lands directly in the rows of a larger table -- the resident trainer's feature cache, keyed
 * by the wave-table row.  rows, inj->poison / position / frames stay indexed by the batch row. */
int abd_mfcc_rows_f32(const abd_mfcc_plan* plan, const float* wave, int64_t row_stride,
                      const int32_t* rows, int64_t batch, const abd_inject* inj, float* out,
                      const int32_t* out_rows, void* workspace, size_t workspace_bytes,
                      abd_stream_t stream);

/* out[u] = table[rows[u]] for u < n: rows of row_elems floats (row_elems * 4 B a multiple of 16, both
 * buffers 16-byte aligned, else ABD_E_UNSUPPORTED), moved as 16-byte vectors with 64-bit offsets;
 * rows may repeat; n = 0 launches nothing.  The feature cache's per-step read: the batch's cached
 * (T, n_mfcc) blocks into the model input. */
int abd_gather_rows_f32(const float* table, int64_t row_elems, const int32_t* rows, int64_t n,
                        float* out, abd_stream_t stream);

/* The injected waveform itself (batch, length): the reference's bd_*_wav arrays
 * (ultrasonic.py:75, flowmur.py:85/106). */
int abd_inject_waveform_f32(const float* wave, int64_t row_stride, int64_t length,
                            const int32_t* rows, int64_t batch, const abd_inject* inj,
                            float* out, void* workspace, size_t workspace_bytes,
                            abd_stream_t stream);
size_t abd_inject_workspace_bytes(int64_t batch);

/* The SNR_WINDOW / DEPLOY scale of each of n_rows table rows (flowmur.py:77-80,
 * flowmur_generate_trigger.py:50-52) into scales[n_rows]: every row as if poisoned (inj->poison is
 * ignored), rows 0..n_rows-1 of the table.  For abd_inject.row_scale. */
int abd_inject_row_scales(const float* wave, int64_t row_stride, int64_t length, int64_t n_rows,
                          const abd_inject* inj, float* scales, abd_stream_t stream);

/* FlowMur trigger optimisation, backward half (utils/flowmur_generate_trigger.py:89-104):
 * given dmfcc = d loss / d MFCC (batch, 1, T, n_mfcc) of
 *     MFCC(clamp(deploy(wave, trigger, position), -1, 1))          (inj->mode DEPLOY_CLAMP;
 *     DEPLOY skips the clamp), write d loss / d trigger (trigger_len floats) into dtrigger.
 * flags: ABD_BWD_ACCUMULATE adds to dtrigger; ABD_BWD_FORWARD_IN_WORKSPACE says the same
 * workspace just ran abd_mfcc_f32 on these inputs (its leading abd_mfcc_workspace_bytes()
 * hold the dB values, maxima and SNR scales), so the forward is not recomputed.
 * The gradient flows through the top_db clamp (ties split
 * like torch.maximum / amax), the dB log, the mel projection, |STFT|^2, the framing and
 * reflect padding, the clamp, the mix and the SNR scale s = 10^(30/20)|t|/|w|.
 * Needs a non-Bluestein specialised FFT plan (n_fft 2048 or 400; flowmur uses 2048) and
 * inj->poison == NULL.  workspace: abd_mfcc_deploy_backward_workspace_bytes(). */
size_t abd_mfcc_deploy_backward_workspace_bytes(const abd_mfcc_plan* plan, int64_t batch,
                                                int64_t trigger_len);
enum { ABD_BWD_ACCUMULATE = 1, ABD_BWD_FORWARD_IN_WORKSPACE = 2 };
int abd_mfcc_deploy_backward(const abd_mfcc_plan* plan, const float* wave, int64_t row_stride,
                             const int32_t* rows, int64_t batch, const abd_inject* inj,
                             const float* dmfcc, float* dtrigger, int flags,
                             void* workspace, size_t workspace_bytes, abd_stream_t stream);

/* DABA int16 path: pydub gain + overlay (utils/daba_selection_tools.py:24-39).
 * host/trig int16 (batch rows of host_len / trig_len); gain per row is the LINEAR factor
 * pydub applies, db_to_float(po_db - trig.dBFS) = 10 ** (dB / 20) evaluated in double by the
 * caller (so audioop.mul's floor sees the same product); out int16 (batch, host_len). */
int abd_pydub_overlay_i16(const int16_t* host, int64_t host_len, const int16_t* trig,
                          int64_t trig_len, const double* gain, int64_t batch,
                          int16_t* out, abd_stream_t stream);

/* DABA selection front end (utils/daba_selection_tools.py:24-39 + the soundfile.read that
 * follows the wav export, :70): hosts of their own lengths host_len[row] (NULL = length),
 * row-major with host_stride; trig rows trig_stride apart (0 = one trigger for every row).
 * Writes `length` samples per row: the overlay inside the host, 0 past its end, as int16
 * (out_i16) and/or as float v/32768 (out_f32); either may be NULL. */
int abd_pydub_overlay_ragged_i16(const int16_t* host, int64_t host_stride, const int32_t* host_len,
                                 const int16_t* trig, int64_t trig_stride, int64_t trig_len,
                                 const double* gain, int64_t batch, int64_t length,
                                 int16_t* out_i16, float* out_f32, abd_stream_t stream);

/* utils/daba_selection_tools.py:55-65,78-81  F.softmax(output) + calc_ent (log2 entropy,
 * double accumulation) per row of log-probs; probs (n, K) optional. */
int abd_softmax_entropy(const float* logprobs, int64_t n, int num_classes, float* probs,
                        double* entropy, abd_stream_t stream);
/* utils/daba_selection_tools.py:67-68  cross_entropy(a, y) per row pair (float32, nan_to_num). */
int abd_pair_cross_entropy(const float* probs_a, const float* probs_y, int64_t n, int num_classes,
                           float* out, abd_stream_t stream);

/* ------------------------------------------------------------------ resampling
 * Replaces prepare_dataset.py:60  torchaudio.functional.resample(waveform, orig_freq, new_freq)
 * (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99 by default): 16 kHz Speech
 * Commands -> 44.1 kHz for the ultrasonic attack.  Output length ceil(new * L / orig) on the
 * gcd-reduced rates.  Supported: <= 448 output phases and <= 176 taps after the gcd
 * reduction (16000 -> 44100 is 441 phases x 174 taps). */
typedef struct abd_resample_plan abd_resample_plan;
int abd_resample_plan_create(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff,
                             abd_resample_plan** plan);
void abd_resample_plan_destroy(abd_resample_plan* plan);
int64_t abd_resample_output_length(const abd_resample_plan* plan, int64_t length);
/* in: batch rows of `length` samples, in_stride apart; out: rows of output_length, out_stride apart */
int abd_resample_f32(const abd_resample_plan* plan, const float* in, int64_t in_stride, int64_t batch,
                     int64_t length, float* out, int64_t out_stride, abd_stream_t stream);

/* ------------------------------------------------------------------ JingleBack style boards
 * Replaces utils/styles_trigger.py:8-53  get_boards() / poison_style(wav, board, sr), the
 * pedalboard (JUCE dsp, float32) chains jingleback.py applies to the poisoned clips.  A board
 * is a chain of up to 8 effects, each run like pedalboard does (reset=True: zero state, snapped
 * smoothers per clip).  Parameters p[] per kind (pedalboard argument order):
 *   GAIN        p0 gain_db
 *   DISTORTION  p0 drive_db                                   (tanh waveshaper after the gain)
 *   LADDER      p0 mode (0 LPF12, 1 HPF12, 2 BPF12, 3 LPF24, 4 HPF24, 5 BPF24), p1 cutoff_hz,
 *               p2 resonance, p3 drive                        (at most one per board)
 *   PHASER      p0 rate_hz, p1 depth, p2 centre_frequency_hz, p3 feedback, p4 mix (one per board)
 *   CHORUS      p0 rate_hz, p1 depth, p2 centre_delay_ms, p3 feedback (must be 0), p4 mix
 *               (its delay line reads the chain's input history: only memoryless effects
 *               may precede it, see below)
 *   REVERB      p0 room_size, p1 damping, p2 wet_level, p3 dry_level, p4 width, p5 freeze_mode
 *               (juce::Reverb mono, JUCE_UNDENORMALISE as on x86 builds; one per board;
 *               its comb / allpass buffers live in the caller's workspace)
 *   PITCHSHIFT  p0 semitones                                  (first effect of the board, at most one)
 *               pedalboard.PitchShift is Rubber Band (R2: phase-vocoder stretch by r = 2^(st/12),
 *               then a resample by 1/r); no bit-level spec is public, so this is a phase vocoder of
 *               the same structure defined in oracle/effects.py (pitch_shift): parity unpinned.
 *   Effects between the board's start (after a PitchShift) and a Chorus must be memoryless (Gain,
 *   Distortion): the chorus delay line re-applies them to the history it reads.
 *
 * Accepted range (tests/style_envelope_cases.py walks it, profiles/styles/envelope.md reports it):
 *   abd_style_board_create   0 <= n <= 8 effects (n = 0, or a lone PitchShift: the chain is a copy);
 *     sample_rate > 0 (the reverb sizes sample_rate * tuning / 44100 are formed in 64 bits);
 *     max_length >= 0; semitones in [-24, 24]; every parameter finite, and every derived
 *     coefficient and table entry finite -- a LadderFilter drive <= 0 is refused (its gain is
 *     drive^-2.642), ABD_E_INVALID naming the effect.  Finite values outside JUCE's debug
 *     assertions run as JUCE's release build runs them: Chorus depth 5 (the reference's own),
 *     centre_delay_ms outside [1, 100] (clamped), a Phaser centre_frequency_hz <= 0 (the LFO's
 *     lower clamp), mix / resonance / room_size outside [0, 1], any finite rate_hz (the LFO's phase
 *     is reduced with fmod: the same value as JUCE's repeated subtraction up to the LFO's own rate).  A second LadderFilter, Phaser or
 *     Reverb, a Chorus feedback != 0, a stateful effect before a Chorus, a PitchShift that is
 *     not first: ABD_E_UNSUPPORTED.
 *   abd_style_board_apply    any batch >= 0 (a PitchShift board: <= 65535), 0 <= length <=
 *     max_length (a plan made for a longer clip gives bit for bit what a plan of that length
 *     gives), in_stride and out_stride >= length, any alignment of in / out (the 16-byte path is
 *     taken only where both row pointers allow it), rows with repeats.  Samples of a row are
 *     adjacent: there is no element stride. */
enum { ABD_FX_GAIN = 0, ABD_FX_DISTORTION = 1, ABD_FX_LADDER = 2, ABD_FX_PHASER = 3, ABD_FX_CHORUS = 4,
       ABD_FX_REVERB = 5, ABD_FX_PITCHSHIFT = 6 };
typedef struct abd_effect {
  int kind;
  float p[8];
} abd_effect;
typedef struct abd_style_board abd_style_board;
int abd_style_board_create(const abd_effect* fx, int n, int sample_rate, int64_t max_length,
                           abd_style_board** board);
void abd_style_board_destroy(abd_style_board* board);
/* bytes of workspace abd_style_board_apply needs for `batch` clips of up to max_length samples
 * (0 without a Reverb or a PitchShift) */
size_t abd_style_board_workspace_bytes(const abd_style_board* board, int64_t batch);
/* out[u] = board(in[rows ? rows[u] : u]) for `length` samples (<= max_length) */
int abd_style_board_apply(const abd_style_board* board, const float* in, int64_t in_stride,
                          const int32_t* rows, int64_t batch, int64_t length, float* out,
                          int64_t out_stride, void* workspace, size_t workspace_bytes,
                          abd_stream_t stream);

/* ------------------------------------------------------------------ smallcnn
 * Replaces utils/models.py:17-65 smallcnn(num_classes, linear_features) forward /
 * backward, utils/training_tools.py:52-85 train() inner step (CrossEntropyLoss on
 * the log-probs, Adam step, loss/accuracy/ASR bookkeeping) and :87-134 test().
 *
 * Parameters live in ONE flat fp32 buffer in torch parameter order
 * (conv1.w, conv1.b, bn1.w, bn1.b, conv2.w, conv2.b, bn2.w, bn2.b, conv3.w, conv3.b,
 *  bn3.w, bn3.b, fc1.w, fc1.b, fc2.w, fc2.b) -- torch-layout views are handed to the
 * nn.Module, so state_dict()/checkpoints are the reference's.  Gradients and the
 * two Adam moments use the same flat layout. */
typedef struct abd_cnn abd_cnn;

int abd_smallcnn_create(int H0, int W0, int num_classes, int max_batch, abd_cnn** net);
/* GEMM precision of the conv2/conv3 forward, data- and weight-gradient products.
 * ABD_PREC_F32_SPLIT (the default of a new handle, the bench and the drop-in smallcnn): fp32
 * operands split exactly into three bf16 planes (x = x0 + x1 + x2) and multiplied as the six
 * terms with i + j <= 2 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- every term exact,
 * dropped terms <= ~2^-26 |a*b| (below one fp32 rounding), i.e. fp32-accurate GEMMs, parity-tested
 * at the same 1e-4 fp32 tolerance as ABD_PREC_F32.  ABD_PREC_F32 (opt-in): fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), slower.  ABD_PREC_BF16 (BASELINE configs[2]/[4]: "bf16, conv-as-GEMM
 * on MFMA"): operands rounded to bf16, fp32 accumulation; BatchNorm, fc layers and the loss stay
 * fp32. */
enum { ABD_PREC_F32 = 0, ABD_PREC_BF16 = 1, ABD_PREC_F32_SPLIT = 2 };
int abd_smallcnn_set_precision(abd_cnn* net, int precision);
void abd_smallcnn_destroy(abd_cnn* net);
int64_t abd_smallcnn_param_count(const abd_cnn* net);
/* offsets (floats) of the 16 parameter tensors inside the flat buffer */
int abd_smallcnn_param_offsets(const abd_cnn* net, int64_t* offsets /* 17 */);
int abd_smallcnn_flat_features(const abd_cnn* net);
size_t abd_smallcnn_workspace_bytes(const abd_cnn* net, int64_t batch);
/* Byte offset of a named activation buffer inside the workspace (tests / debugging):
 * p1 r2 p2 r3 p3d d2 logp dz dp3 da dz3 dp2 dz2 dp1 coef bcoef mask1 mask2 rowinfo p1s dz2s xh3. */
int64_t abd_smallcnn_workspace_offset(const abd_cnn* net, int64_t batch, const char* name);
/* 1 when abd_smallcnn_train_step at this batch folds BN1 into conv2 (ABD_PREC_F32_SPLIT; a step
 * with SyncBN (abd_train_args.bn_sync set) never folds): the workspace's p1 then holds m, the
 * pool1-selected relu(conv1) value per window, and p1 = alpha * m + beta' with BN1's coefficients
 * (coef[0][c] = (mean, invstd, alpha, beta')); 0 otherwise. */
int abd_smallcnn_bn1_folded(const abd_cnn* net, int64_t batch);
/* Plane count of the conv2 plane mode of abd_smallcnn_train_step at this batch (no SyncBN): 3
 * (ABD_PREC_F32_SPLIT) or 1 (ABD_PREC_BF16) when the step keeps conv2's two activation operands as
 * exact bf16 planes -- the workspace's "p1s" (pool1 output m, [planes][B*H1*W1p*64] uint16, replacing
 * p1) and "dz2s" (BN2 backward output, [planes][B*H2*W2*64], replacing dz2), x = sum of the planes
 * exactly for 3 planes, rne(x) for 1 -- else 0 (p1 / dz2 hold fp32). */
int abd_smallcnn_conv2_planes(const abd_cnn* net, int64_t batch);

/* Device-side counters written by the train/eval launches (int64 / double):
 *   [0] sum of per-batch mean losses (double bits; train steps weight each by
 *       grad_scale)  [1] samples  [2] correct
 *   [3] poisoned samples  [4] poisoned & predicted==label  [5] batches     */
#define ABD_METRICS_WORDS 8

typedef struct abd_train_args {
  const float* x;            /* (B,1,H0,W0) MFCC input                        */
  const int64_t* labels;     /* (B)                                           */
  const int64_t* indicators; /* (B) poison indicator, NULL = none             */
  int64_t batch;
  float* params;             /* flat                                          */
  float* grads;              /* flat (written)                                */
  float* exp_avg;            /* flat Adam m                                   */
  float* exp_avg_sq;         /* flat Adam v                                   */
  float* running;            /* 6 BN buffers packed: rm1,rv1,rm2,rv2,rm3,rv3  */
  int64_t adam_step;         /* step index after increment (1-based)          */
  float lr, beta1, beta2, eps;
  int do_update;             /* 0: forward/backward only (grads), 1: + Adam   */
  const uint8_t* mask1_in;   /* optional dropout keep masks (B,flat),(B,128)  */
  const uint8_t* mask2_in;   /*   NULL -> generated from (seed, counter)      */
  uint64_t seed, counter;
  uint8_t* mask1_out;        /* optional: masks used (for tests)              */
  uint8_t* mask2_out;
  float* logprobs_out;       /* optional (B,K)                                */
  int64_t* metrics;          /* ABD_METRICS_WORDS accumulators (device)       */
  float grad_scale;          /* multiply loss gradient (DP: B_local/B_global);
                              * also weights metrics[0]'s batch-mean loss, so
                              * the ranks' words sum to the global batch mean
                              * (uneven last batch included).  batch >= 1:
                              * a 1-row batch is valid (BatchNorm2d counts
                              * N*H*W elements per channel)                  */
  int64_t* num_batches_tracked; /* optional int64[3] (bn1..bn3), += 1          */
  void* fc_grads_event;      /* optional hipEvent_t, recorded on the stream once
                              * the fc1/fc2 gradients (flat tail from offset
                              * abd_smallcnn_param_offsets()[12]) are final, so
                              * a DP caller can start their all-reduce while the
                              * conv backward is still running               */
  int64_t row_offset;        /* DP: global batch row of this rank's row 0.  The
                              * generated dropout masks hash the GLOBAL element
                              * index, so N ranks on slices of one global batch
                              * draw exactly the masks one process would.     */
  /* Synchronised BatchNorm (optional; NULL = per-rank statistics like DDP).  At each of the
   * 6 BatchNorm reductions of a step (forward bn1..bn3, then backward bn3..bn1) libabd writes
   * this rank's per-channel double sums into bn_sync_buf + point * ABD_BN_SYNC_STRIDE
   * (2*C+1 doubles: [sum_c | sum2_c | element count] forward, [sum dy_c | sum dy*xhat_c | count]
   * backward) and calls bn_sync(ctx, point, offset, n) from the launching thread; the callback
   * must enqueue an in-place SUM all-reduce of those n doubles on `stream` (torch.distributed
   * on the current stream does).  The statistics then use the global sums and counts: the
   * normalisation, running statistics and input gradients equal one process's on the global
   * batch; BN weight/bias gradients stay this rank's share (summed by the gradient all-reduce). */
  double* bn_sync_buf;       /* device, >= 6 * ABD_BN_SYNC_STRIDE doubles               */
  int (*bn_sync)(void* ctx, int point, int64_t offset, int64_t n);
  void* bn_sync_ctx;
} abd_train_args;
#define ABD_BN_SYNC_STRIDE 136

int abd_smallcnn_train_step(abd_cnn* net, const abd_train_args* a, void* workspace,
                            size_t workspace_bytes, abd_stream_t stream);

/* Split step for data parallelism: forward+backward (grads), then the caller
 * all-reduces grads/BN stats, then abd_smallcnn_apply(). */
int abd_smallcnn_apply(abd_cnn* net, const abd_train_args* a, void* workspace,
                       size_t workspace_bytes, abd_stream_t stream);

/* Autograd path (nn.Module forward/backward outside the fused train()):
 * forward keeps every activation in the workspace; backward consumes d(log-probs)
 * and must follow the forward on the same workspace.  train_mode selects batch
 * statistics + dropout (a->mask*, seed, counter, running updated) vs running stats. */
int abd_smallcnn_forward(abd_cnn* net, const abd_train_args* a, int train_mode, void* workspace,
                         size_t workspace_bytes, abd_stream_t stream);
int abd_smallcnn_backward(abd_cnn* net, const abd_train_args* a, const float* dlogprobs,
                          void* workspace, size_t workspace_bytes, abd_stream_t stream);

/* A batch of independent batch-1 train-mode forwards (utils/daba_selection_tools.py:68-87
 * runs the freshly built, untrained model -- nn.Module defaults to train() -- on one clip at
 * a time): BatchNorm normalises each utterance by its OWN statistics, dropout is active
 * (masks from mask*_in or from (seed, counter)), running statistics are left untouched (the
 * reference's selection model is discarded).  logprobs (batch, K).
 * workspace: abd_smallcnn_forward_per_utterance_workspace_bytes(). */
size_t abd_smallcnn_forward_per_utterance_workspace_bytes(const abd_cnn* net, int64_t batch);
int abd_smallcnn_forward_per_utterance(abd_cnn* net, const float* x, int64_t batch, const float* params,
                                       uint64_t seed, uint64_t counter, const uint8_t* mask1_in,
                                       const uint8_t* mask2_in, float* logprobs, void* workspace,
                                       size_t workspace_bytes, abd_stream_t stream);

/* eval forward (model.eval()): running BN statistics, no dropout.  Writes log-probs
 * and, if labels != NULL, accumulates loss/correct/ASR counters like test(). */
int abd_smallcnn_eval(abd_cnn* net, const float* x, int64_t batch, const float* params,
                      const float* running, const int64_t* labels,
                      const int64_t* indicators, float* logprobs, int64_t* metrics,
                      void* workspace, size_t workspace_bytes, abd_stream_t stream);

/* Batched neuron-ablation sweep: the defenses' loss-change scan (ft_reg.py:173-190 prune_one_neuron +
 * get_loss_change; :163-171 pruning and tsbd.py:43-47 zero_reinit_toget with a set of filters per
 * variant).  Variant v is the model with the parameters its mask row selects set to zero --
 * conv<i>.weight[c] = 0 (ABD_ABLATE_CONV_FILTER) or bn<i>.weight[c] = 0 (ABD_ABLATE_BN_WEIGHT,
 * --layer_type bn) -- run as model.eval() on the batch with nn.CrossEntropyLoss on the log-probs.
 * The parameters are never patched: an ablated channel's pooled activation is one constant, the next
 * conv's pre-activation differs from the baseline's by a rank-1 term, and (variant, row) pairs run
 * through the eval kernels as one virtual batch.  Per call each layer is computed at most once for
 * all variants whose earliest ablated layer lies after it; a variant costs only the layers behind
 * its earliest ablated one.
 *   masks   HOST memory, (n_variants, 160) bytes, nonzero = ablated: conv1 channels 0..63, conv2
 *           64..127, conv3 128..159.  Any mask: empty (the baseline), several channels in several
 *           layers, a whole layer.  Read before the call returns; it reaches the device as kernel
 *           arguments, so the launch sequence stays capture-safe.
 *   loss_sum[v] += sum over the batch rows of the CE loss (double), correct[v] += rows whose arg-max
 *           is the label (int64): device buffers of n_variants entries that accumulate over calls.
 *   variants_per_pass  variants evaluated together inside the workspace (any n_variants, the tail
 *           pass included); variants_per_pass * batch rows must keep the layer-3 kernels' 32-bit
 *           offsets (else ABD_E_INVALID).
 * batch == 0 or n_variants == 0 launches nothing.  ABD_PREC_F32 / ABD_PREC_F32_SPLIT only.
 * workspace: abd_smallcnn_ablate_workspace_bytes(net, batch, variants_per_pass). */
enum { ABD_ABLATE_CONV_FILTER = 0, ABD_ABLATE_BN_WEIGHT = 1 };
size_t abd_smallcnn_ablate_workspace_bytes(const abd_cnn* net, int64_t batch, int variants_per_pass);
int abd_smallcnn_ablate_eval(abd_cnn* net, const float* x, int64_t batch, const float* params,
                             const float* running, const int64_t* labels, const uint8_t* masks,
                             int n_variants, int kind, int variants_per_pass, double* loss_sum,
                             int64_t* correct, void* workspace, size_t workspace_bytes,
                             abd_stream_t stream);

/* Frozen-model input gradient (utils/flowmur_generate_trigger.py:98-103: the benign model,
 * saved by EarlyStoppingModel right after clean_test() and therefore in eval mode, with
 * requires_grad off): eval forward (running BN statistics, no dropout), CrossEntropyLoss on
 * the log-probs scaled by loss_scale (mean over the batch), backward to the input x.
 * Writes log-probs (B,K), dx (B,1,H0,W0) and, if metrics != NULL, accumulates the loss /
 * accuracy counters.  workspace: abd_smallcnn_input_grad_workspace_bytes(). */
size_t abd_smallcnn_input_grad_workspace_bytes(const abd_cnn* net, int64_t batch);
int abd_smallcnn_input_grad(abd_cnn* net, const float* x, int64_t batch, const float* params,
                            const float* running, const int64_t* labels, float loss_scale,
                            float* logprobs, float* dx, int64_t* metrics, void* workspace,
                            size_t workspace_bytes, abd_stream_t stream);

/* torch.optim.Adam single-tensor step over a flat buffer (weight_decay 0). */
int abd_adam_f32(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                 int64_t n, int64_t step, float lr, float beta1, float beta2, float eps,
                 abd_stream_t stream);

/* ------------------------------------------------------------------ regularised fine-tuning
 * Replaces ft_reg.py:83-123 train_finetuning_reg (one batch: gradient g1 at the parameters, every
 * parameter tensor moved by r * g1 / ||g1||, gradient g2 at the moved point, torch.optim.SGD with
 * momentum on (1 - alpha) g1 + alpha g2, a train-mode forward for loss / accuracy) and the plain
 * train_finetuning of ft_reg.py:57-81 / tsbd.py:140-161 (SGD with momentum).  The reference
 * deep-copies the model per batch; here the displaced parameters live in the workspace.
 *
 * Segments: `offsets` is HOST memory, n_seg + 1 ascending int64 element offsets into the flat fp32
 * buffers (abd_smallcnn_param_offsets() gives the model's 16 tensors); segment s is
 * [offsets[s], offsets[s + 1]).  1 <= n_seg <= ABD_MAX_SEGMENTS and no segment may be empty, else
 * ABD_E_INVALID.  The offsets are read before the call returns and reach the device as kernel
 * arguments.  Every reduction runs in a fixed order (no floating-point atomics): equal inputs give
 * bit-equal results. */
#define ABD_MAX_SEGMENTS 32

/* norms[s] = ||buf[offsets[s] : offsets[s + 1]]||_2 (device float[n_seg]): squares accumulated in
 * double (per-block partial sums in the workspace, then one fixed-order sum per segment), sqrt in
 * double, rounded to fp32 once.  buf needs only its natural 4-byte alignment. */
size_t abd_segment_norms_workspace_bytes(const int64_t* offsets, int n_seg);
int abd_segment_norms_f32(const float* buf, const int64_t* offsets, int n_seg, float* norms,
                          void* workspace, size_t workspace_bytes, abd_stream_t stream);

/* out[i] = p[i] + r * (g[i] / norms[seg(i)]) for offsets[0] <= i < offsets[n_seg], each operation
 * rounded to fp32 in that order: ft_reg.py:101 ``param.data += r * (grad / grad.norm())``.  out may
 * not alias p or g (ABD_E_INVALID when out == p or out == g).  A zero norm gives NaN (0 / 0) in
 * every element of that segment, as the reference does; it is not guarded. */
int abd_perturb_f32(const float* p, const float* g, const float* norms, const int64_t* offsets,
                    int n_seg, float r, float* out, abd_stream_t stream);

/* torch.optim.SGD single-tensor step over flat buffers (dampening 0, no Nesterov, weight_decay 0):
 *     d = g                                  (g2 == NULL)
 *     d = (1 - alpha) * g + alpha * g2       (g2 != NULL: ft_reg.py:109 final_gradients)
 *     buf = momentum * buf + d ; p -= lr * buf          (buf != NULL)
 *     p -= lr * d                                        (buf == NULL, requires momentum == 0)
 * A zero-initialised buf reproduces torch's first step (buf = d) exactly, so there is no step index.
 * grad_out (optional) receives d; it may alias g or g2. */
int abd_sgd_f32(float* p, const float* g, const float* g2, float alpha, float* buf, float momentum,
                float lr, float* grad_out, int64_t n, abd_stream_t stream);

/* One batch of train_finetuning_reg on the device.  Forward k (0, 1, 2) takes its dropout keep masks
 * from mask1_in[k] / mask2_in[k] ((B, flat) / (B, 128) bytes; NULL = generated from (seed,
 * counter + k)) and reports the masks it used in mask1_out[k] / mask2_out[k] (optional).
 *   1. train step without update at params -> g1; its BN running statistics go to a scratch copy
 *   2. per-tensor norms of g1, perturbed parameters into the workspace
 *   3. train step without update at the perturbed parameters, same batch, scratch statistics -> g2
 *   4. abd_sgd_f32 on params with (g1, g2, alpha); the blended gradient is left in grads
 *   5. train-mode forward at the updated params with the real running / num_batches_tracked, which
 *      therefore advance exactly once per batch (the reference's forwards 1 and 2 run on the
 *      discarded copy)
 *   6. *loss_sum += the batch-mean CrossEntropyLoss of forward 5's log-probs (double),
 *      *correct += its arg-max hits
 * The net's GEMM precision applies to all three passes.  batch >= 1.
 * workspace: abd_smallcnn_finetune_reg_workspace_bytes(net, batch). */
typedef struct abd_finetune_reg_args {
  const float* x;               /* (B,1,H0,W0)                                        */
  const int64_t* labels;        /* (B)                                                */
  int64_t batch;
  float* params;                /* flat, updated in place                             */
  float* grads;                 /* flat (written): (1 - alpha) g1 + alpha g2          */
  float* running;               /* 6 BN buffers packed like abd_train_args.running    */
  int64_t* num_batches_tracked; /* optional int64[3], += 1                            */
  uint64_t seed, counter;
  int64_t row_offset;
  float r, alpha, lr, momentum;
  float* momentum_buf;          /* flat; NULL requires momentum == 0                  */
  const uint8_t* mask1_in[3];
  const uint8_t* mask2_in[3];
  uint8_t* mask1_out[3];
  uint8_t* mask2_out[3];
  float* logprobs_out;          /* optional (3, B, K): the log-probs of the 3 forwards */
  double* loss_sum;             /* device accumulators                                */
  int64_t* correct;
} abd_finetune_reg_args;
size_t abd_smallcnn_finetune_reg_workspace_bytes(const abd_cnn* net, int64_t batch);
int abd_smallcnn_finetune_reg_step(abd_cnn* net, const abd_finetune_reg_args* a, void* workspace,
                                   size_t workspace_bytes, abd_stream_t stream);

/* ------------------------------------------------------------------ TSBD: unlearning, weight change, re-init
 * Replaces tsbd.py:108-138 train_unlearning (one batch: gradient ASCENT on the loss with Adam, the record
 * layer's per-neuron gradient norm; the same loop at correlation_analysis.py:41-71), tsbd.py:342-363 /
 * correlation_analysis.py:76-99 (neuron weight change: |p_unlearned - p_original| per weight and summed
 * per neuron) and tsbd.py:49-63 zero_reinit_weight for all ratios of the sweep at :371-380.
 *
 * Row table: HOST memory, n_seg (1 .. ABD_MAX_SEGMENTS) segments of `rows` rows of `row_len` floats
 * starting at element `offset` of a flat fp32 buffer, ascending and not overlapping; rows >= 1 and
 * row_len >= 1, else ABD_E_INVALID.  For smallcnn the conv table is 64 x 4, 64 x 256, 32 x 256 at the
 * offsets of conv<i>.weight, the bn table 64, 64, 32 rows of length 1 at bn<i>.weight.  The table's rows
 * are numbered in segment order and its values are "packed" in that order (no gaps between segments).
 * The table is read before the call returns and reaches the device as kernel arguments.  Buffers need
 * only their natural 4-byte alignment.  No floating-point atomics; every reduction has a fixed order. */
typedef struct abd_row_segment {
  int64_t offset, rows, row_len;
} abd_row_segment;

/* absdiff = |a - b| (|a| when b == NULL) over the table's rows: one fp32 subtraction and a sign clear,
 * bit-equal to torch's (a - b).abs().  absdiff_out (optional, device) receives the packed rows;
 * row_sums (device float[total rows]) the sum of each row, accumulated in double in a fixed order and
 * rounded to fp32 once. */
int abd_row_abs_sums_f32(const float* a, const float* b, const abd_row_segment* table, int n_seg,
                         float* absdiff_out, float* row_sums, abd_stream_t stream);

/* One batch of train_unlearning on the device:
 *   1. abd_smallcnn_train_step with do_update = 0 at params: the running statistics and
 *      num_batches_tracked advance once, metrics (optional) accumulate the POSITIVE loss and the hits
 *   2. grads <- -grads (the .grad that (-loss).backward() leaves) and torch.optim.Adam on it, with
 *      exactly abd_adam_f32's arithmetic
 *   3. record_abs_sums[r] = sum |grads[record_offset + r * record_row_len ...]| for the record layer's
 *      record_rows rows (tsbd.py:126-128); record_rows == 0 records nothing
 * The net's GEMM precision applies.  batch >= 1, adam_step >= 1 (1-based, after increment).
 * workspace: abd_smallcnn_unlearn_workspace_bytes(net, batch). */
typedef struct abd_unlearn_args {
  const float* x;               /* (B,1,H0,W0)                                        */
  const int64_t* labels;        /* (B)                                                */
  int64_t batch;
  float* params;                /* flat, updated in place                             */
  float* grads;                 /* flat (written): the gradient of -loss              */
  float* exp_avg;               /* flat Adam m                                        */
  float* exp_avg_sq;            /* flat Adam v                                        */
  float* running;               /* 6 BN buffers packed like abd_train_args.running    */
  int64_t* num_batches_tracked; /* optional int64[3], += 1                            */
  int64_t adam_step;
  float lr, beta1, beta2, eps;
  uint64_t seed, counter;
  int64_t row_offset;
  const uint8_t* mask1_in;      /* optional dropout keep masks (B,flat),(B,128)       */
  const uint8_t* mask2_in;      /*   NULL -> generated from (seed, counter)           */
  uint8_t* mask1_out;           /* optional: masks used                               */
  uint8_t* mask2_out;
  float* logprobs_out;          /* optional (B,K)                                     */
  int64_t* metrics;             /* optional ABD_METRICS_WORDS accumulators (device)   */
  int64_t record_offset, record_rows, record_row_len;
  float* record_abs_sums;       /* device float[record_rows]                          */
} abd_unlearn_args;
size_t abd_smallcnn_unlearn_workspace_bytes(const abd_cnn* net, int64_t batch);
int abd_smallcnn_unlearn_step(abd_cnn* net, const abd_unlearn_args* a, void* workspace,
                              size_t workspace_bytes, abd_stream_t stream);

/* The re-initialised parameter sets of n_variants (1 .. ABD_MAX_REINIT_VARIANTS) ratios in one call.
 *   absdiff     the packed rows abd_row_abs_sums_f32 wrote (device); NaN is the caller's error
 *   row_select  HOST bytes (n_variants, total rows), nonzero = the neuron is among the variant's top_num
 *   k           HOST int64[n_variants]: int(m * wratio), m = the number of weights in the selected rows
 * thr[v] (device float) = the k[v]-th largest absdiff of variant v's selected rows (radix select on the
 * bit patterns), out[v][i] (device, (n_variants, n_params)) = 0 where i lies in a selected row and its
 * absdiff >= thr[v] -- ties at the threshold zero more than k weights, as the reference's ``>=`` does
 * -- else params[i]; parameters outside the table's rows are copied.  zeroed[v] (device int64) = the
 * number of weights set to zero.  Each out + v * n_params is a params pointer for abd_smallcnn_eval.
 * ABD_E_INVALID when k[v] < 1 or k[v] > m (the reference's min([]) ValueError), when a variant selects
 * no row, or when the table has more than ABD_MAX_REINIT_ROWS rows or reaches past n_params. */
#define ABD_MAX_REINIT_VARIANTS 16
#define ABD_MAX_REINIT_ROWS 1024
int abd_reinit_weights_f32(const float* params, int64_t n_params, const float* absdiff,
                           const abd_row_segment* table, int n_seg, const uint8_t* row_select,
                           const int64_t* k, int n_variants, float* out, float* thr, int64_t* zeroed,
                           abd_stream_t stream);

/* ------------------------------------------------------------------ correlation analysis of two unlearnings
 * Replaces correlation_analysis.py:141-157: the unlearning loop (every call of train_unlearning there
 * trains on the FIRST batch of an unshuffled loader, so all --unlearn_epochs steps of a model see one fixed
 * batch) and the per-neuron weight-change sums of the clean- and the poison-unlearned model with their
 * Pearson correlation.
 *
 * abd_smallcnn_unlearn_run enqueues n_steps (>= 1) unlearning steps on the batch of `a`: step i is exactly
 * abd_smallcnn_unlearn_step with adam_step + i and counter + i, so the result is bit-equal to n_steps
 * separate calls in every GEMM precision.  One host call, no synchronisation, nothing allocated.
 *   mask1_in / mask2_in    optional, n_steps consecutive mask sets: (n_steps, B, flat), (n_steps, B, 128)
 *   mask1_out / mask2_out  optional, likewise
 *   metrics                optional int64 (n_steps, ABD_METRICS_WORDS), zeroed by the caller: row i
 *                          accumulates step i only
 *   logprobs_out           optional (B, K): the last step's values
 * The record fields must be unset (record_rows == 0, record_abs_sums == NULL): correlation_analysis.py's
 * train_unlearning records nothing.  ABD_E_INVALID for n_steps < 1, set record fields and whatever the
 * step refuses.  workspace: abd_smallcnn_unlearn_workspace_bytes(net, batch). */
int abd_smallcnn_unlearn_run(abd_cnn* net, const abd_unlearn_args* a, int64_t n_steps, void* workspace,
                             size_t workspace_bytes, abd_stream_t stream);

/* get_neuron_weight_change (correlation_analysis.py:76-99) of two unlearned parameter sets against one
 * original, and :149-157 on the result.  Row table as for abd_row_abs_sums_f32, at most
 * ABD_MAX_REINIT_ROWS rows in all (one block computes the statistics), else ABD_E_INVALID.  Two launches,
 * no atomics.
 *   absdiff_a / absdiff_b  optional: the packed |params_a - orig| and |params_b - orig|
 *   sums32_a / sums32_b    float[rows]: their row sums, bit-equal to abd_row_abs_sums_f32 (the ucn text)
 *   sums64                 double[2][rows], a first: the same sums before their rounding to fp32 (the
 *                          reference's CSV holds Python's sequential double sum() of the fp32 values; the
 *                          order here is the lane groups', within row_len * 2^-53 relative of it)
 *   stats                  double[ABD_NWC_STATS_WORDS] = {n, mean_x, mean_y, sxx, syy, sxy, r, slope,
 *                          intercept} with x = sums64[0] (a: the clean-unlearned model), y = sums64[1]:
 *                          means first, then the centred sums, all in double in a fixed order;
 *                          r = sxy / sqrt(sxx * syy), NaN when n < 2 or sxx * syy == 0 (pandas' value for
 *                          a constant column); slope = sxy / sxx and intercept = mean_y - slope * mean_x,
 *                          the least-squares line of the reference's lmplot, NaN when sxx == 0 */
#define ABD_NWC_STATS_WORDS 9
int abd_nwc_pair_f32(const float* orig, const float* params_a, const float* params_b,
                     const abd_row_segment* table, int n_seg, float* absdiff_a, float* absdiff_b,
                     float* sums32_a, float* sums32_b, double* sums64, double* stats, abd_stream_t stream);

/* ------------------------------------------------------------------ Fine-Pruning: ranking, prune sweep, masked tuning
 * Replaces fp.py:131-147 (the mean input activation of the model's last child over clean batches),
 * fp.py:164-195 (the prune sweep: temp_test of the model with the lowest units masked out of the first
 * Linear of that child, for every step) and fp.py:52-76 train_finetuning under prune.custom_from_mask.
 * The reference's last child of smallcnn is the unused nn.Softmax(); with it deleted the last child is
 * fc2, the pruned layer is fc2 and its input is relu(fc1(...)) in eval mode, ABD_FCPRUNE_UNITS units.
 * The network passes are abd_smallcnn_eval / abd_smallcnn_train_step (do_update = 0) themselves: every
 * GEMM precision they support applies unchanged (ABD_PREC_BF16 included; fc2 and the loss are fp32 in
 * all of them).  No floating-point atomics; every reduction has a fixed order. */
#define ABD_FCPRUNE_UNITS 128
#define ABD_FCPRUNE_PASS_VARIANTS 128

/* One eval forward of the batch, then sums[u] += sum over the rows of fc2's input unit u, accumulated
 * in double in a fixed order.  sums: device double[ABD_FCPRUNE_UNITS], accumulates over calls (zero it
 * before the first).  batch == 0 launches nothing.  workspace: abd_smallcnn_workspace_bytes(net, batch). */
int abd_smallcnn_hidden_sums(abd_cnn* net, const float* x, int64_t batch, const float* params,
                             const float* running, double* sums, void* workspace,
                             size_t workspace_bytes, abd_stream_t stream);

/* The prune sweep on one batch: ONE eval forward, then per variant v and row fc2 with the pruned units'
 * columns removed, log_softmax, nn.CrossEntropyLoss on the log-probs (temp_test, fp.py:36-50) and the
 * arg-max (first index on ties).
 *   masks   HOST memory, (n_variants, ABD_FCPRUNE_UNITS) bytes, nonzero = pruned.  Any mask: empty (the
 *           baseline), all units (the logits equal the bias), nested or not.  Read before the call
 *           returns; it reaches the device as kernel arguments, ABD_FCPRUNE_PASS_VARIANTS variants per
 *           pass (any n_variants, the tail pass included), so the launch sequence stays capture-safe.
 *   loss_sum[v] += sum over the batch rows of the CE loss (double), correct[v] += rows whose arg-max is
 *           the label (int64): device buffers of n_variants entries that accumulate over calls, the
 *           accumulators of abd_smallcnn_ablate_eval.
 * batch == 0 or n_variants == 0 launches nothing.  labels must lie in [0, num_classes).
 * workspace: abd_smallcnn_fcprune_workspace_bytes(net, batch, n_variants). */
size_t abd_smallcnn_fcprune_workspace_bytes(const abd_cnn* net, int64_t batch, int n_variants);
int abd_smallcnn_fcprune_eval(abd_cnn* net, const float* x, int64_t batch, const float* params,
                              const float* running, const int64_t* labels, const uint8_t* masks,
                              int n_variants, double* loss_sum, int64_t* correct, void* workspace,
                              size_t workspace_bytes, abd_stream_t stream);

/* One batch of train_finetuning (fp.py:52-76) with prune.custom_from_mask active on fc2.weight:
 *   1. abd_smallcnn_train_step with do_update = 0 at params (whose pruned fc2.weight columns the caller
 *      zeroed once: params holds the EFFECTIVE weight); running statistics and num_batches_tracked
 *      advance once, metrics (optional) accumulate the loss and the hits
 *   2. grads at fc2.weight[:, j] <- 0 for every pruned unit j, written back: the .grad torch leaves on
 *      weight_orig
 *   3. torch.optim.Adam on it, with exactly abd_adam_f32's arithmetic
 * With zero gradient and zero moments the pruned columns stay exactly zero.  pruned: device
 * uint8[ABD_FCPRUNE_UNITS], nonzero = pruned.  batch >= 1, adam_step >= 1 (1-based, after increment).
 * workspace: abd_smallcnn_pruned_finetune_workspace_bytes(net, batch). */
typedef struct abd_pruned_finetune_args {
  const float* x;               /* (B,1,H0,W0)                                        */
  const int64_t* labels;        /* (B)                                                */
  int64_t batch;
  float* params;                /* flat, updated in place                             */
  float* grads;                 /* flat (written): the masked gradient                */
  float* exp_avg;               /* flat Adam m                                        */
  float* exp_avg_sq;            /* flat Adam v                                        */
  float* running;               /* 6 BN buffers packed like abd_train_args.running    */
  int64_t* num_batches_tracked; /* optional int64[3], += 1                            */
  const uint8_t* pruned;        /* device uint8[ABD_FCPRUNE_UNITS]                    */
  int64_t adam_step;
  float lr, beta1, beta2, eps;
  uint64_t seed, counter;
  int64_t row_offset;
  const uint8_t* mask1_in;      /* optional dropout keep masks (B,flat),(B,128)       */
  const uint8_t* mask2_in;      /*   NULL -> generated from (seed, counter)           */
  uint8_t* mask1_out;           /* optional: masks used                               */
  uint8_t* mask2_out;
  float* logprobs_out;          /* optional (B,K)                                     */
  int64_t* metrics;             /* optional ABD_METRICS_WORDS accumulators (device)   */
} abd_pruned_finetune_args;
size_t abd_smallcnn_pruned_finetune_workspace_bytes(const abd_cnn* net, int64_t batch);
int abd_smallcnn_pruned_finetune_step(abd_cnn* net, const abd_pruned_finetune_args* a, void* workspace,
                                      size_t workspace_bytes, abd_stream_t stream);

/* ------------------------------------------------------------------ profiling
 * Per-phase HIP-event brackets around libabd launches (bench.py roofline).  Bit i of
 * phase_mask enables phase i (see csrc/prof.h: 0 stft_mel, 1 db_dct, 6 conv2 fwd,
 * 20 conv2 wgrad, 21 conv2 dgrad, ...).  stop() synchronises the recorded events and
 * returns the summed milliseconds and launch counts per phase. */
int abd_profile_start(unsigned long long phase_mask, int max_records);
/* The same, bracketing only every `every`-th launch of each enabled phase (1, 1 + every, ...):
 * each bracket costs the stream a serialising timestamp (~4-5 us of idle GPU on MI355X), so
 * bench.py samples the launches of its timed steps instead of bracketing all of them. */
int abd_profile_start_every(unsigned long long phase_mask, int max_records, int every);
/* Mark the start of a step (call once per step, before its launches).  Once called, sampling
 * is per STEP: every launch of an enabled phase inside steps 0, every, 2 every, ... is bracketed
 * (launch-count sampling aliases with a phase launched several times per step). */
int abd_profile_step(void);
int abd_profile_stop(double* total_ms, int* counts, int n_phases);

/* ------------------------------------------------------------------ lstmwithattention
 * Replaces utils/models.py:180-228 lstmwithattention(classes, time_len, seq_len) forward / backward
 * and the train() / test() inner steps for it.  Input (B, 1, T, F) fp32 with T = seq_len,
 * F = time_len; the module returns raw logits (nn.CrossEntropyLoss does the log-softmax).
 *
 * Parameters live in ONE flat fp32 buffer in named_parameters() order, 34 tensors: conv1.w/b,
 * batchnorm1.w/b, conv2.w/b, batchnorm2.w/b, rnn1 {weight_ih, weight_hh, bias_ih, bias_hh}_l0 and the
 * four _reverse ones, the same eight of rnn2, then dense1, attention, dense2, dense3, output (.w, .b).
 * running: rm1[10] rv1[10] rm2[1] rv2[1]; num_batches_tracked: int64[2].
 *
 * Every product is fp32 (v_mfma_f32_32x32x2_f32 GEMMs, fp32 FMAs in the recurrence); there is no
 * bf16 mode.  Each LSTM layer's recurrence is one launch whose workgroups keep W_hh of their
 * direction in LDS for all T steps (abd_lstmattn_tile_rows() batch rows per workgroup).  All
 * reductions have a fixed order: two calls on equal inputs give bit-equal results.  The entry points
 * allocate nothing, never synchronise and take nothing from host memory but their arguments. */
typedef struct abd_lstmattn abd_lstmattn;

typedef struct abd_lstmattn_args {
  const float* x;            /* (B,1,T,F)                                      */
  const int64_t* labels;     /* (B)                                            */
  const int64_t* indicators; /* (B) poison indicator, NULL = none              */
  int64_t batch;
  float* params;             /* flat                                           */
  float* grads;              /* flat (written)                                 */
  float* exp_avg;            /* flat Adam m                                    */
  float* exp_avg_sq;         /* flat Adam v                                    */
  float* running;            /* 22 floats                                      */
  int64_t adam_step;         /* step index after increment (1-based)           */
  float lr, beta1, beta2, eps;
  int do_update;             /* 0: forward/backward only (grads), 1: + Adam    */
  const uint8_t* mask_in;    /* optional dropout keep mask (B,64); NULL ->
                              * generated from (seed, counter, global row)     */
  uint64_t seed, counter;
  uint8_t* mask_out;         /* optional: the mask used                        */
  float* logits_out;         /* optional (B,K)                                 */
  int64_t* metrics;          /* optional ABD_METRICS_WORDS accumulators        */
  float grad_scale;          /* multiplies the loss gradient and weights
                              * metrics[0]'s batch-mean loss                   */
  int64_t* num_batches_tracked; /* optional int64[2], += 1 per train forward   */
  int64_t row_offset;        /* global batch row of row 0 (dropout hash)       */
} abd_lstmattn_args;

/* ABD_E_UNSUPPORTED outside 1 <= F <= 128, 1 <= T <= 1024 */
int abd_lstmattn_create(int T, int F, int num_classes, abd_lstmattn** net);
void abd_lstmattn_destroy(abd_lstmattn* net);
int64_t abd_lstmattn_param_count(const abd_lstmattn* net);
int abd_lstmattn_param_offsets(const abd_lstmattn* net, int64_t* offsets /* 35 */);
/* batch rows one workgroup of the recurrent kernels carries through the sequence */
int abd_lstmattn_tile_rows(void);
size_t abd_lstmattn_workspace_bytes(const abd_lstmattn* net, int64_t batch);
/* Byte offset of a saved activation inside the workspace (tests), -1 for an unknown name:
 * a1 a2 x0 (conv / BatchNorm outputs), y1 y2 ((B,T,128) h_t of rnn1 / rnn2, forward | reverse half),
 * c1 c2 ([2][B][T][64] cell states), gates1 gates2 ([2][B][T][256] activated i f g o), q att av d2 d3
 * logits dlogits mask rowinfo dy2 dy1 dx0. */
int64_t abd_lstmattn_workspace_offset(const abd_lstmattn* net, int64_t batch, const char* name);
/* forward keeps every activation in the workspace and writes the logits to a->logits_out (if set);
 * train_mode selects batch statistics + dropout (running statistics updated) vs running statistics.
 * backward consumes d(logits) and must follow a train-mode forward on the same workspace.
 * Train mode needs B*T*F > 1 (BatchNorm over one value has no variance; torch raises too), else
 * ABD_E_INVALID. */
int abd_lstmattn_forward(abd_lstmattn* net, const abd_lstmattn_args* a, int train_mode, void* workspace,
                         size_t workspace_bytes, abd_stream_t stream);
int abd_lstmattn_backward(abd_lstmattn* net, const abd_lstmattn_args* a, const float* dlogits,
                          void* workspace, size_t workspace_bytes, abd_stream_t stream);
/* forward, cross entropy on the logits (mean over the batch) with the ABD_METRICS_WORDS counters as
 * abd_smallcnn_train_step defines them, backward, and abd_adam_f32 on the flat buffer when do_update.
 * labels are required (ABD_E_INVALID).  The step's d(logits) follows the arithmetic of torch's
 * log_softmax / nll_loss backward (its exp and log routines, its reduction order for K <= 64), so the
 * autograd path -- forward, torch's CrossEntropyLoss, backward -- gives bit-equal gradients. */
int abd_lstmattn_train_step(abd_lstmattn* net, const abd_lstmattn_args* a, void* workspace,
                            size_t workspace_bytes, abd_stream_t stream);
/* eval forward: running statistics, no dropout.  Writes the logits and, if labels != NULL,
 * accumulates the counters like test(). */
int abd_lstmattn_eval(abd_lstmattn* net, const float* x, int64_t batch, const float* params,
                      const float* running, const int64_t* labels, const int64_t* indicators,
                      float* logits, int64_t* metrics, void* workspace, size_t workspace_bytes,
                      abd_stream_t stream);

/* A batch of independent batch-1 train-mode forwards of lstmwithattention, the selection forward of
 * utils/daba_selection_tools.py:68-87 (the freshly built model -- train mode -- on one clip at a time) for
 * every row at once; the counterpart of abd_smallcnn_forward_per_utterance.
 *   - BatchNorm1 (10 channels) and BatchNorm2 (1 channel) normalise each utterance by the statistics of its
 *     OWN T*F values per channel: biased variance, eps 1e-5, sums accumulated in double, variance clamped
 *     at 0 (as the batched train-mode forward takes them over B*T*F values).
 *   - Dropout is active: the keep mask comes from mask_in (batch, 64), or, when NULL, from the hash of
 *     (seed, counter, row * 64 + unit) that the batched forward uses with row_offset 0.
 *   - Running statistics and num_batches_tracked are neither read nor written (the reference discards its
 *     selection model).  logits (batch, K) are the raw logits, like the module's forward.
 * One workgroup per utterance runs conv1 -> BatchNorm1 -> conv2 -> BatchNorm2 with the utterance and
 * relu(conv2) in LDS (8*T*F bytes); the ten conv1 planes are recomputed, never stored.  Behind it the two
 * LSTM layers and the head are the batched forward's own launches.  Two calls on equal inputs are bit-equal,
 * and a row's logits do not depend on the other rows of the batch.
 * T*F = 1: ABD_E_INVALID (no variance; torch raises too).  T*F > ABD_LSTMATTN_PER_UTTERANCE_MAX_TF:
 * ABD_E_UNSUPPORTED (every F in [1, 128] at DABA's T = 32 is far inside).  Both, NULL x / params / logits,
 * the batch range and a short or misaligned workspace are refused before any launch.
 * workspace: abd_per_utterance_lstmattn_workspace_bytes(), smaller than abd_lstmattn_workspace_bytes() (no
 * conv1 planes, no gradient or statistics buffers, one set of gate / cell buffers for both layers). */
#define ABD_LSTMATTN_PER_UTTERANCE_MAX_TF 16384
size_t abd_per_utterance_lstmattn_workspace_bytes(const abd_lstmattn* net, int64_t batch);
int abd_per_utterance_lstmattn_forward(abd_lstmattn* net, const float* x, int64_t batch, const float* params,
                                       uint64_t seed, uint64_t counter,
                                       const uint8_t* mask_in /* (batch,64) or NULL */,
                                       float* logits /* (batch,K) */, void* workspace, size_t workspace_bytes,
                                       abd_stream_t stream);

/* ------------------------------------------------------------------ RNN
 * Replaces utils/models.py:231-257 RNN(num_classes, time_len): nn.LSTM(time_len, 768, 3, batch_first)
 * from zero initial states, nn.Linear(768, num_classes) on the last time step; forward / backward and
 * the train() / test() inner steps.  Input (B, 1, T, F) fp32 with F = time_len; raw logits out.  The
 * model has no BatchNorm and no dropout, so train and eval forwards are the same computation.
 *
 * Parameters live in ONE flat fp32 buffer in named_parameters() order, 14 tensors:
 * lstm.{weight_ih, weight_hh, bias_ih, bias_hh}_l0, _l1, _l2, then fc.weight, fc.bias.
 *
 * Every product is fp32: an LDS-tiled v_mfma_f32_32x32x2_f32 GEMM (input projections of all B*T rows,
 * data and weight gradients, fc) and one launch per time step for the recurrence, whose workgroups own
 * the four gates of their hidden units (W_hh, 9.4 MB per layer, is streamed; it does not fit LDS).  The
 * weight gradients' B*T reduction is cut into slices summed in slice order; there are no float atomics
 * and two calls on equal inputs give bit-equal results.  The entry points allocate nothing, never
 * synchronise and take nothing from host memory but their arguments.
 *
 * The workspace keeps h, c and the four activated gates of every layer and step for BPTT:
 * 3 * B*T * (768 + 768 + 3072) floats and a (B*T, 768) gradient buffer, about 1.5 GB at B = 256,
 * T = 100; abd_rnn_workspace_bytes reports the exact size.  backward overwrites the saved gates with
 * the gate gradients, so it runs once per forward. */
typedef struct abd_rnn abd_rnn;

/* abd_lstmattn_args without the dropout and running-statistics fields */
typedef struct abd_rnn_args {
  const float* x;            /* (B,1,T,F)                                      */
  const int64_t* labels;     /* (B)                                            */
  const int64_t* indicators; /* (B) poison indicator, NULL = none              */
  int64_t batch;
  float* params;             /* flat                                           */
  float* grads;              /* flat (written)                                 */
  float* exp_avg;            /* flat Adam m                                    */
  float* exp_avg_sq;         /* flat Adam v                                    */
  int64_t adam_step;         /* step index after increment (1-based)           */
  float lr, beta1, beta2, eps;
  int do_update;             /* 0: forward/backward only (grads), 1: + Adam    */
  float* logits_out;         /* optional (B,K)                                 */
  int64_t* metrics;          /* optional ABD_METRICS_WORDS accumulators        */
  float grad_scale;          /* multiplies the loss gradient and weights
                              * metrics[0]'s batch-mean loss                   */
} abd_rnn_args;

/* ABD_E_UNSUPPORTED outside 1 <= F <= 128, 1 <= T <= 1024 */
int abd_rnn_create(int T, int F, int num_classes, abd_rnn** net);
void abd_rnn_destroy(abd_rnn* net);
int64_t abd_rnn_param_count(const abd_rnn* net);
int abd_rnn_param_offsets(const abd_rnn* net, int64_t* offsets /* 15 */);
/* kernel geometry (tests): 0 batch rows of a recurrent workgroup, 1 / 2 edge of the small / large GEMM
 * block tile, 3 least rows of a weight-gradient slice, 4 rows above which column sums take two stages,
 * 5 least count of large tiles for which the large tile is used; -1 otherwise */
int abd_rnn_tile_info(int what);
size_t abd_rnn_workspace_bytes(const abd_rnn* net, int64_t batch);
/* Byte offset of a saved activation inside the workspace (tests), -1 for an unknown name:
 * h1 h2 h3 c1 c2 c3 ((B,T,768) per layer), gates1 gates2 gates3 ((B*T,3072) activated i f g o after
 * forward), logits dlogits rowinfo. */
int64_t abd_rnn_workspace_offset(const abd_rnn* net, int64_t batch, const char* name);
/* forward keeps every activation in the workspace and writes the logits to a->logits_out (if set).
 * backward consumes d(logits) and must follow a forward on the same workspace. */
int abd_rnn_forward(abd_rnn* net, const abd_rnn_args* a, void* workspace, size_t workspace_bytes,
                    abd_stream_t stream);
int abd_rnn_backward(abd_rnn* net, const abd_rnn_args* a, const float* dlogits, void* workspace,
                     size_t workspace_bytes, abd_stream_t stream);
/* forward, cross entropy (mean over the batch) with the ABD_METRICS_WORDS counters, backward, and
 * abd_adam_f32 on the flat buffer when do_update; d(logits) in torch's log_softmax / nll_loss
 * arithmetic as in abd_lstmattn_train_step.  labels are required (ABD_E_INVALID). */
int abd_rnn_train_step(abd_rnn* net, const abd_rnn_args* a, void* workspace, size_t workspace_bytes,
                       abd_stream_t stream);
/* Writes the logits and, if labels != NULL, accumulates the counters like test(). */
int abd_rnn_eval(abd_rnn* net, const float* x, int64_t batch, const float* params, const int64_t* labels,
                 const int64_t* indicators, float* logits, int64_t* metrics, void* workspace,
                 size_t workspace_bytes, abd_stream_t stream);

/* ------------------------------------------------------------------ largecnn
 * Replaces utils/models.py:68-119 largecnn(num_classes, linear_features): conv1(1->96), pool 2x2,
 * conv2(96->256), pool 2x2, relu conv3(256->384), relu conv4(384->384), relu conv5(384->256), pool 3x3
 * stride 2, flatten, relu fc1(->256), dropout 0.5, relu fc2(->128), dropout 0.5, fc3, log_softmax; every
 * conv 3x3, stride 1, padding 1; forward / backward and the train() / test() inner steps.  Input
 * (B, 1, H, W) fp32; the module returns log-probabilities, and the loss is cross entropy ON them
 * (log_softmax twice), as the reference trains it.
 *
 * Parameters live in ONE flat fp32 buffer in named_parameters() order, 16 tensors: conv1..conv5
 * (.weight (Cout, Cin, 3, 3), .bias), fc1, fc2, fc3 (.weight, .bias).
 *
 * Every product is fp32.  Activations are channels-last (B, H, W, C) in the workspace.  conv2..conv5 and
 * their data and weight gradients are implicit GEMMs on v_mfma_f32_32x32x2_f32 (no im2col buffer); the
 * weight gradients' pixel reduction is cut into slices summed in slice order; conv1 is a direct kernel.
 * The pools' backward passes recompute the argmax (first maximum in row-major window order, torch's rule).
 * There are no float atomics and two calls on equal inputs give bit-equal results.  The entry points
 * allocate nothing, never synchronise and take nothing from host memory but their arguments. */
typedef struct abd_largecnn abd_largecnn;

typedef struct abd_largecnn_args {
  const float* x;            /* (B,1,H,W)                                      */
  const int64_t* labels;     /* (B)                                            */
  const int64_t* indicators; /* (B) poison indicator, NULL = none              */
  int64_t batch;
  float* params;             /* flat                                           */
  float* grads;              /* flat (written)                                 */
  float* exp_avg;            /* flat Adam m                                    */
  float* exp_avg_sq;         /* flat Adam v                                    */
  int64_t adam_step;         /* step index after increment (1-based)           */
  float lr, beta1, beta2, eps;
  int do_update;             /* 0: forward/backward only (grads), 1: + Adam    */
  const uint8_t* mask1_in;   /* optional dropout keep masks (B,256), (B,128);  */
  const uint8_t* mask2_in;   /* NULL -> hashed from (seed, counter, global row) */
  uint64_t seed, counter;
  uint8_t* mask1_out;        /* optional: the masks used                       */
  uint8_t* mask2_out;
  float* logits_out;         /* optional (B,K): the log-probabilities          */
  int64_t* metrics;          /* optional ABD_METRICS_WORDS accumulators        */
  float grad_scale;          /* multiplies the loss gradient and weights
                              * metrics[0]'s batch-mean loss                   */
  int64_t row_offset;        /* global batch row of row 0 (dropout hash)       */
} abd_largecnn_args;

/* fc1's inputs for an (H, W) input: 256 * ((H/4 - 3)/2 + 1) * ((W/4 - 3)/2 + 1) in integer division;
 * -1 when H/4 < 3 or W/4 < 3 (pool3 has no window) */
int64_t abd_largecnn_linear_features(int H, int W);
/* ABD_E_UNSUPPORTED for H/4 < 3 or W/4 < 3 (12 x 12 is the smallest input), a side above 4096, a
 * geometry whose element indices leave 32 bits, num_classes outside [1, 4096] */
int abd_largecnn_create(int H, int W, int num_classes, abd_largecnn** net);
void abd_largecnn_destroy(abd_largecnn* net);
/* The least count of 128 x 128 GEMM blocks from which a product runs the large tile instead of the
 * 64 x 64 one (default: abd_largecnn_tile_info(4)).  The two tiles compute the same sums in another
 * order; 1 runs every product on the large tile, INT_MAX on the small one (tests, tuning).
 * ABD_E_INVALID below 1. */
int abd_largecnn_set_large_min_blocks(abd_largecnn* net, int min_blocks);
int64_t abd_largecnn_param_count(const abd_largecnn* net);
int abd_largecnn_param_offsets(const abd_largecnn* net, int64_t* offsets /* 17 */);
/* kernel geometry (tests): 0 / 1 edge of the small / large GEMM block tile, 2 least pixels of a
 * weight-gradient slice, 3 rows above which column sums take two stages, 4 least count of large tiles for
 * which the large tile is used, 5 most slices; -1 otherwise */
int abd_largecnn_tile_info(int what);
size_t abd_largecnn_workspace_bytes(const abd_largecnn* net, int64_t batch);
/* Byte offset of a saved activation inside the workspace (tests), -1 for an unknown name: a1 p1 a2 p2 a3
 * a4 a5 (channels-last (B, H, W, C) conv / pool outputs, a3..a5 after relu), p3 ((B, 256, PH, PW): fc1's
 * input row in the reference's flatten order), h1 h2 (after relu and dropout), z3 (fc3's output), logits
 * (the log-probabilities), dlogits rowinfo keep1 keep2, da2 (conv2's output gradient after backward). */
int64_t abd_largecnn_workspace_offset(const abd_largecnn* net, int64_t batch, const char* name);
/* forward keeps every activation in the workspace and writes the log-probabilities to a->logits_out (if
 * set); train_mode selects dropout.  backward consumes d(log-probabilities) and must follow a train-mode
 * forward on the same workspace. */
int abd_largecnn_forward(abd_largecnn* net, const abd_largecnn_args* a, int train_mode, void* workspace,
                         size_t workspace_bytes, abd_stream_t stream);
int abd_largecnn_backward(abd_largecnn* net, const abd_largecnn_args* a, const float* dlogits, void* workspace,
                          size_t workspace_bytes, abd_stream_t stream);
/* forward, cross entropy on the log-probabilities (mean over the batch) with the ABD_METRICS_WORDS
 * counters, backward, and abd_adam_f32 on the flat buffer when do_update; d(logits) in torch's
 * log_softmax / nll_loss arithmetic as in abd_lstmattn_train_step.  labels are required (ABD_E_INVALID). */
int abd_largecnn_train_step(abd_largecnn* net, const abd_largecnn_args* a, void* workspace,
                            size_t workspace_bytes, abd_stream_t stream);
/* eval forward (no dropout).  Writes the log-probabilities and, if labels != NULL, accumulates the
 * counters like test(). */
int abd_largecnn_eval(abd_largecnn* net, const float* x, int64_t batch, const float* params,
                      const int64_t* labels, const int64_t* indicators, float* logits, int64_t* metrics,
                      void* workspace, size_t workspace_bytes, abd_stream_t stream);

/* ------------------------------------------------------------------ ResNet
 * Replaces utils/models.py:261-332 ResNet(ResidualBlock, [2, 2, 2], num_classes, linear_features): stem
 * conv3x3(1->16) BN relu; layer1 two blocks 16->16; layer2 a stride-2 block 16->32 whose residual is a
 * conv3x3 stride 2 + BN downsample, then a block 32->32; layer3 the same for 32->64 and 64->64; conv2d
 * 1x1 64->64 stride (2, 1) with bias; AvgPool2d(4) (floor); fc on the (C, PH, PW) flatten.  A block is
 * relu(bn2(conv2(relu(bn1(conv1(x))))) + residual).  Every 3x3 conv has padding 1 and no bias.  Input
 * (B, 1, H, W) fp32; raw logits out; the loss is cross entropy on them.
 *
 * Parameters live in ONE flat fp32 buffer in named_parameters() order, 49 tensors: for each of the
 * fifteen conv + BatchNorm units (conv/bn, layer1.0.conv1/bn1, layer1.0.conv2/bn2, layer1.1.., layer2.0
 * conv1/bn1, conv2/bn2, downsample.0/.1, layer2.1.., layer3 alike) the conv weight (Cout, Cin, 3, 3), the
 * BN weight and the BN bias; then conv2d.weight, conv2d.bias, fc.weight, fc.bias.  running: for each unit
 * in that order running_mean[Cout] then running_var[Cout], 1120 floats; num_batches_tracked: int64[15].
 *
 * Every product is fp32.  Activations are channels-last (B, H, W, C) in the workspace.  The fourteen convs
 * behind the stem and their data and weight gradients are implicit GEMMs on v_mfma_f32_16x16x4_f32 (no
 * im2col buffer), stride 1 and 2; the weight gradients' pixel reduction is cut into slices summed in slice
 * order; the stem is a direct kernel.  BatchNorm takes per-block sums in double, combined in block order
 * and in double (biased variance, eps 1e-5; running statistics with momentum 0.1 and the unbiased
 * variance).  There are no float atomics and two calls on equal inputs give bit-equal results.  The entry
 * points allocate nothing, never synchronise and take nothing from host memory but their arguments. */
typedef struct abd_resnet abd_resnet;

/* abd_rnn_args plus the running statistics */
typedef struct abd_resnet_args {
  const float* x;            /* (B,1,H,W)                                      */
  const int64_t* labels;     /* (B)                                            */
  const int64_t* indicators; /* (B) poison indicator, NULL = none              */
  int64_t batch;
  float* params;             /* flat                                           */
  float* grads;              /* flat (written)                                 */
  float* exp_avg;            /* flat Adam m                                    */
  float* exp_avg_sq;         /* flat Adam v                                    */
  float* running;            /* 1120 floats; NULL in a train-mode call leaves
                              * the running statistics alone                   */
  int64_t adam_step;         /* step index after increment (1-based)           */
  float lr, beta1, beta2, eps;
  int do_update;             /* 0: forward/backward only (grads), 1: + Adam    */
  float* logits_out;         /* optional (B,K)                                 */
  int64_t* metrics;          /* optional ABD_METRICS_WORDS accumulators        */
  float grad_scale;          /* multiplies the loss gradient and weights
                              * metrics[0]'s batch-mean loss                   */
  int64_t* num_batches_tracked; /* optional int64[15], += 1 per train forward  */
} abd_resnet_args;

/* fc's inputs for an (H, W) input: 64 * (H4 / 4) * (W3 / 4) with H2 = (H - 1) / 2 + 1, H3 = (H2 - 1) / 2 + 1,
 * H4 = (H3 - 1) / 2 + 1 and W3 alike, in integer division; -1 below 25 x 13 (the pool has no window) */
int64_t abd_resnet_linear_features(int H, int W);
/* ABD_E_UNSUPPORTED for H < 25 or W < 13, a side above 4096, a geometry whose element indices leave 32
 * bits, num_classes outside [1, 4096] */
int abd_resnet_create(int H, int W, int num_classes, abd_resnet** net);
void abd_resnet_destroy(abd_resnet* net);
int64_t abd_resnet_param_count(const abd_resnet* net);
int abd_resnet_param_offsets(const abd_resnet* net, int64_t* offsets /* 50 */);
int64_t abd_resnet_running_count(const abd_resnet* net);
/* offsets[u]: unit u's running_mean inside running (its running_var follows); offsets[15] = the count */
int abd_resnet_running_offsets(const abd_resnet* net, int64_t* offsets /* 16 */);
/* kernel geometry (tests): 0 rows of a GEMM block tile, 1 the K-step, 2 least pixels of a weight-gradient
 * slice, 3 most slices, 4 least pixels of a BatchNorm partial block, 5 most such blocks; -1 otherwise */
int abd_resnet_tile_info(int what);
size_t abd_resnet_workspace_bytes(const abd_resnet* net, int64_t batch);
/* Byte offset of a saved map inside the workspace (tests), -1 for an unknown name.  For unit u = 0..14:
 * z<u> the conv output, a<u> what the unit's BatchNorm pass wrote (after the residual add and the relu where
 * the unit has them), s<u> the batch mean[Cout] then 1 / sqrt(var + eps)[Cout]; all maps channels-last.
 * sub ((B, H4, W3, 64): the rows conv2d reads), c2 (conv2d's output), pool ((B, 64, PH, PW): fc's input row
 * in the reference's flatten order), logits dlogits rowinfo. */
int64_t abd_resnet_workspace_offset(const abd_resnet* net, int64_t batch, const char* name);
/* forward keeps every map in the workspace and writes the logits to a->logits_out (if set); train_mode
 * selects batch statistics (running statistics and num_batches_tracked updated when given) vs the running
 * statistics (required then).  backward consumes d(logits) and must follow a train-mode forward on the same
 * workspace. */
int abd_resnet_forward(abd_resnet* net, const abd_resnet_args* a, int train_mode, void* workspace,
                       size_t workspace_bytes, abd_stream_t stream);
int abd_resnet_backward(abd_resnet* net, const abd_resnet_args* a, const float* dlogits, void* workspace,
                        size_t workspace_bytes, abd_stream_t stream);
/* forward, cross entropy on the logits (mean over the batch) with the ABD_METRICS_WORDS counters, backward,
 * and abd_adam_f32 on the flat buffer when do_update; d(logits) in torch's log_softmax / nll_loss
 * arithmetic as in abd_lstmattn_train_step.  labels are required (ABD_E_INVALID). */
int abd_resnet_train_step(abd_resnet* net, const abd_resnet_args* a, void* workspace, size_t workspace_bytes,
                          abd_stream_t stream);
/* eval forward: running statistics, nothing updated.  Writes the logits and, if labels != NULL,
 * accumulates the counters like test(). */
int abd_resnet_eval(abd_resnet* net, const float* x, int64_t batch, const float* params, const float* running,
                    const int64_t* labels, const int64_t* indicators, float* logits, int64_t* metrics,
                    void* workspace, size_t workspace_bytes, abd_stream_t stream);

/* ------------------------------------------------------------------ smalllstm
 * Replaces utils/models.py:121-178 smalllstm(num_classes, rnn_features): conv1 2x2 (1->64, bias) relu bn1
 * MaxPool2d((1,3)); conv2 2x2 (64->64) relu bn2 MaxPool2d((2,2), padding (1,1)); conv3 2x2 (64->32) relu bn3
 * MaxPool2d((2,2), padding (0,1)); Dropout(0.4); the pooled (B, 32, T, Wf) map permuted to (B, T, Wf * 32) feeds
 * nn.LSTM(32 Wf, 128, 2, batch_first) from a zero state; fc2 (128 -> K) on the top layer's last step;
 * log_softmax.  ReLU comes before BatchNorm.  Input (B, 1, H, W) fp32; log-probabilities out; the loss is cross
 * entropy on them.  Geometry (integer division): H1 = H - 1, W1 = W - 1, Wp1 = W1 / 3, H2 = H1 - 1,
 * W2 = Wp1 - 1, Hp2 = H2 / 2 + 1, Wp2 = W2 / 2 + 1, H3 = Hp2 - 1, W3 = Wp2 - 1, T = (H3 - 2) / 2 + 1,
 * Wf = W3 / 2 + 1.
 *
 * Parameters live in ONE flat fp32 buffer in named_parameters() order, 24 tensors: conv1.weight, conv1.bias,
 * bn1.weight, bn1.bias, the same for conv2 / bn2 and conv3 / bn3, rnn.weight_ih_l0, weight_hh_l0, bias_ih_l0,
 * bias_hh_l0, the same for l1, fc1.weight (128, 224), fc1.bias, fc2.weight, fc2.bias.  fc1 is a parameter the
 * forward never reads: its gradient is written as exactly zero.  running: bn1, bn2, bn3 running_mean then
 * running_var, 320 floats; num_batches_tracked: int64[3].
 *
 * Every product is fp32.  Activations are channels-last in the workspace, so the pooled map IS the LSTM's input
 * sequence.  conv2 and conv3 and their gradients are implicit GEMMs on v_mfma_f32_16x16x4_f32; BatchNorm sums are
 * per-block double partials combined in block order; the max pools take torch's first maximum and backward
 * recomputes it.  Each LSTM layer's recurrence is ONE launch for all T steps (one more for its BPTT): a workgroup
 * owns 16 batch rows and keeps W_hh in registers as MFMA operands.  There are no float atomics and two calls on
 * equal inputs give bit-equal results.  The entry points allocate nothing, never synchronise and take nothing
 * from host memory but their arguments. */
typedef struct abd_smalllstm abd_smalllstm;

/* the fields of abd_lstmattn_args */
typedef struct abd_smalllstm_args {
  const float* x;            /* (B,1,H,W)                                      */
  const int64_t* labels;     /* (B)                                            */
  const int64_t* indicators; /* (B) poison indicator, NULL = none              */
  int64_t batch;
  float* params;             /* flat                                           */
  float* grads;              /* flat (written)                                 */
  float* exp_avg;            /* flat Adam m                                    */
  float* exp_avg_sq;         /* flat Adam v                                    */
  float* running;            /* 320 floats; NULL in a train-mode call leaves
                              * the running statistics and
                              * num_batches_tracked alone                      */
  int64_t adam_step;         /* step index after increment (1-based)           */
  float lr, beta1, beta2, eps;
  int do_update;             /* 0: forward/backward only (grads), 1: + Adam    */
  const uint8_t* mask_in;    /* optional drop1 keep mask in the reference's
                              * (B,32,T,Wf) element order, scale 1/0.6; NULL ->
                              * hashed from (seed, counter, global element)    */
  uint64_t seed, counter;
  uint8_t* mask_out;         /* optional: the mask used                        */
  float* logits_out;         /* optional (B,K): the log-probabilities          */
  int64_t* metrics;          /* optional ABD_METRICS_WORDS accumulators        */
  float grad_scale;          /* multiplies the loss gradient and weights
                              * metrics[0]'s batch-mean loss                   */
  int64_t* num_batches_tracked; /* optional int64[3], += 1 per train forward   */
  int64_t row_offset;        /* global batch row of row 0 (dropout hash)       */
} abd_smalllstm_args;

/* the LSTM's input width 32 * Wf for an (H, W) input; -1 below 6 x 10 (conv3 or pool3 has no window) */
int64_t abd_smalllstm_rnn_features(int H, int W);
/* ABD_E_UNSUPPORTED for H < 6 or W < 10, a side above 4096, a geometry whose element indices leave 32 bits,
 * num_classes outside [1, 4096] */
int abd_smalllstm_create(int H, int W, int num_classes, abd_smalllstm** net);
void abd_smalllstm_destroy(abd_smalllstm* net);
int64_t abd_smalllstm_param_count(const abd_smalllstm* net);
int abd_smalllstm_param_offsets(const abd_smalllstm* net, int64_t* offsets /* 25 */);
int64_t abd_smalllstm_running_count(const abd_smalllstm* net);
/* offsets[i]: bn<i+1>'s running_mean inside running (its running_var follows); offsets[3] = the count */
int abd_smalllstm_running_offsets(const abd_smalllstm* net, int64_t* offsets /* 4 */);
/* kernel geometry (tests): 0 rows of a conv block tile, 1 the convs' K-step, 2 least rows of a weight-gradient
 * slice, 3 most slices of a conv weight gradient, 4 least pixels of a BatchNorm partial block, 5 most such
 * blocks, 6 batch rows of a recurrent workgroup, 7 / 8 edge of the small / large GEMM block tile, 9 the GEMM's
 * K-step, 10 most slices of an LSTM weight gradient, 11 rows above which column sums take two stages, 12 least
 * count of large GEMM tiles for which the large tile is used; -1 otherwise */
int abd_smalllstm_tile_info(int what);
size_t abd_smalllstm_workspace_bytes(const abd_smalllstm* net, int64_t batch);
/* Byte offset of a saved map inside the workspace (tests), -1 for an unknown name.  For i = 1..3: z<i> conv i's
 * output after bias and ReLU (what BatchNorm reads), a<i> the BatchNorm output, p<i> the pooled map, all
 * channels-last; s<i> the batch mean[C] then 1 / sqrt(var + eps)[C].  seq ((B, T, Wf, 32): the LSTM input, p3
 * after dropout), keep (uint8, the reference's (B, 32, T, Wf) order).  For layer l = 0, 1: h<l> c<l> ((B, T, 128)),
 * g<l> ((B, T, 512): the activated gates i f g o after a forward, the gate gradients after a backward).  logits
 * (the log-probabilities), dlogits, rowinfo. */
int64_t abd_smalllstm_workspace_offset(const abd_smalllstm* net, int64_t batch, const char* name);
/* forward keeps every map in the workspace and writes the log-probabilities to a->logits_out (if set);
 * train_mode selects batch statistics (running statistics and num_batches_tracked updated when given) and
 * dropout vs the running statistics (required then).  backward consumes d(log-probabilities), overwrites the
 * saved gates, and must follow a train-mode forward on the same workspace. */
int abd_smalllstm_forward(abd_smalllstm* net, const abd_smalllstm_args* a, int train_mode, void* workspace,
                          size_t workspace_bytes, abd_stream_t stream);
int abd_smalllstm_backward(abd_smalllstm* net, const abd_smalllstm_args* a, const float* dlogits, void* workspace,
                           size_t workspace_bytes, abd_stream_t stream);
/* forward, cross entropy on the log-probabilities (mean over the batch) with the ABD_METRICS_WORDS counters,
 * backward, and abd_adam_f32 on the flat buffer when do_update.  labels are required (ABD_E_INVALID). */
int abd_smalllstm_train_step(abd_smalllstm* net, const abd_smalllstm_args* a, void* workspace, size_t workspace_bytes,
                             abd_stream_t stream);
/* eval forward: running statistics, no dropout, nothing updated.  Writes the log-probabilities and, if
 * labels != NULL, accumulates the counters like test(). */
int abd_smalllstm_eval(abd_smalllstm* net, const float* x, int64_t batch, const float* params, const float* running,
                       const int64_t* labels, const int64_t* indicators, float* logits, int64_t* metrics,
                       void* workspace, size_t workspace_bytes, abd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ABD_H_ */
