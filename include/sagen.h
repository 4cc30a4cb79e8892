/*
 * sagen.h — C ABI of the MI355X-native (gfx950) spatialaudiogen inference path.
 *
 * The reference (pedro-morgado/spatialaudiogen, TF1/Python) has no FFI; its de-facto operator
 * boundary for this path is Python.  Each entry point below names the reference
 * interface it replaces (file:line relative to the reference repo).  The shared library
 * libsagen_hip.so implements this header with hand-written HIP kernels; there is NO CPU
 * implementation of it — every compute entry point fails with SAGEN_ERR_HIP when no gfx950
 * device is present.
 *
 * Conventions
 *  - plain C: pointers + sizes only.  All data pointers are DEVICE pointers to fp32 unless the
 *    name ends in _h.  Tensors are NHWC exactly as the TF1 graph lays them out.
 *  - `stream` is a hipStream_t passed as void*.  Every launch is asynchronous on that stream; no
 *    entry point synchronises, allocates or frees device memory.  The caller owns all memory
 *    (weights, inputs, outputs, workspace) — e.g. torch tensors' data_ptr().
 *  - return value: 0 (SAGEN_OK) or a negative sagen_status; sagen_last_error() returns a
 *    thread-local message for the last failure.  No exceptions / aborts cross the ABI.
 *  - one sagen_ctx per (device, stream) pair in flight; contexts are independent.
 */
#ifndef SAGEN_H
#define SAGEN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAGEN_VERSION 100   /* 0.1.0 */

typedef enum {
    SAGEN_OK = 0,
    SAGEN_ERR_NULL = -1,         /* null pointer argument */
    SAGEN_ERR_SHAPE = -2,        /* bad / inconsistent shape */
    SAGEN_ERR_UNSUPPORTED = -3,  /* configuration the HIP path does not implement */
    SAGEN_ERR_WEIGHTS = -4,      /* missing / misnamed / mis-shaped variable at bind */
    SAGEN_ERR_WORKSPACE = -5,    /* workspace too small or not bound */
    SAGEN_ERR_HIP = -6           /* HIP runtime error (no device, launch failure, ...) */
} sagen_status;

/* encoder bit mask (reference definitions.py:1-4; model.py:47-51) */
#define SAGEN_ENC_AUDIO 1
#define SAGEN_ENC_VIDEO 2
#define SAGEN_ENC_FLOW  4

/* separation mode (reference definitions.py:6-8) */
#define SAGEN_SEP_NONE      0   /* 'none'      : model.py:274-280 */
#define SAGEN_SEP_FREQ_MASK 1   /* 'unet_mask' : model.py:282-348 */

/* Mirrors SptAudioGen.__init__ + SptAudioGenParams (model.py:10-60) and the batch size the
 * caller fixes at graph-build time (deploy.py:50, eval.py:44, train.py:38). */
typedef struct {
    int32_t batch;            /* windows per forward call (BN statistics are per call) */
    int32_t encoders;         /* SAGEN_ENC_* mask; AUDIO is mandatory (model.py:207) */
    int32_t separation;       /* SAGEN_SEP_* */
    int32_t num_sep_tracks;   /* params.sep_num_tracks (32) */
    int32_t n_loc_units;      /* len(params.loc_fc_units) (2) */
    int32_t loc_units[4];     /* params.loc_fc_units ([512,512]) */
    int32_t ambi_order;       /* 1 or 2 (model.py:242-243: num_in = order^2 input channels, num_out = 2*order+1 predicted) */
    int32_t audio_rate;       /* 48000 */
    int32_t video_rate;       /* 10 */
    float   context;          /* 1.0 s */
    float   sample_duration;  /* 0.1 s */
    float   fft_window;       /* 0.025 s -> wind_size 1024 */
} sagen_config;

/* One TF variable: name is the checkpoint key, data is a device pointer in the TF
 * layout (conv HWIO, conv2d_transpose [kh,kw,Cout,Cin], FC [in,out], vectors [C]). */
typedef struct {
    const char*  name;
    const float* data;
    int32_t      ndim;
    int64_t      shape[4];
} sagen_tensor;

typedef struct sagen_ctx sagen_ctx;

int  sagen_version(void);
/* the compiler flags this library was built with (the Python host refuses a build without -fno-slp-vectorize -fno-vectorize:
 * packed-fp32 VALU next to bf16 MFMA waves of another stream returned wrong results on MI355X) */
const char* sagen_build_info(void);
/* sha256 (first 16 hex digits) over every source of this library (every .hip and .h under csrc/, and this header) at the moment it was
 * linked: the prebuilt .so travels to the GPU box with the tree, and the tests compare this with the digest of the sources that
 * travelled with it (spatialaudiogen_amd.build.source_digest) */
const char* sagen_source_digest(void);
const char* sagen_last_error(void);

/* ---- model-level: replaces SptAudioGen.inference_ops (model.py:356-434), as called at
 *      deploy.py:77,141 / eval.py:90,145 -------------------------------------------------
 * ambi_order 1 (num_in = 1, num_out = 3) or 2 (num_in = 4, num_out = 5; train.py:28,109-111, eval.py:69-70,96): at order 2 the
 * first-order W,Y,Z,X recording goes in and the five second-order channels (ACN 4..8) come out.  Order 2 changes, per window:
 * audio_encoder/conv1/weights [7,16,4,32] (one STFT magnitude channel per input channel, channels last: model.py:174);
 * separation/deconv1 [7,16,4*nsep,64] (channel i*nsep + j = track j of input channel i: model.py:326-327); the last localisation FC
 * num_out*num_in*(nsep+1) = 20*(nsep+1) outputs read as [B,3,5,4,nsep+1] (model.py:253-258).  Order 3 and above:
 * SAGEN_ERR_UNSUPPORTED.  Order 2 runs inference only (sagen_train_bind refuses it). */
int    sagen_create(sagen_ctx** out, const sagen_config* cfg);
void   sagen_destroy(sagen_ctx* ctx);
/* bytes of scratch the caller must provide (activations + packed weights); fixed per ctx */
size_t sagen_workspace_bytes(const sagen_ctx* ctx);
/* number of variables the configuration expects, and the i-th expected name/shape */
int    sagen_num_variables(const sagen_ctx* ctx);
int    sagen_variable_spec(const sagen_ctx* ctx, int i, const char** name, int32_t* ndim, int64_t shape[4]);
/* Borrow the variables (replaces tf.train.Saver.restore, deploy.py:79-87) and repack them into
 * the kernels' layouts inside `workspace`.  Tensors must stay alive only until the stream
 * reaches the end of this call's work; workspace must stay alive and untouched by the caller
 * for the life of the ctx. */
int    sagen_bind_weights(sagen_ctx* ctx, const sagen_tensor* tensors, int n,
                          void* workspace, size_t workspace_bytes, void* stream);
/* audio [B, snd_size] (=[B,52799,1]); video/flow [B,224,448,3] (=[B,1,224,448,3]) or NULL;
 * ambi_yzx [B, snd_dur, 3] (channels Y,Z,X = ACN 1,2,3).
 * ambi_order 2: audio [B, snd_size, 4] = W,Y,Z,X interleaved (the feeder's ambix[:, :, :4], eval.py:69); output [B, snd_dur, 5]
 * (ACN 4..8): out[b,n,o] = sum_i sum_j w[b,s(n),o,i,j] sep[b,i,j,n] + bias[b,s(n),o, input channel 0] (model.py:428-430 reads the
 * biases of channel 0 only).  Separation 'none' (model.py:274-280): the reference's decoder product broadcasts the four audio
 * channels against the one track, so out[b,n,o] = (sum_i w[b,s,o,i,0]) * (sum_c audio[b, snd_contx/2 + n, c]) + w[b,s,o,0,1].
 * The same holds for the _u8 and grouped entries below. */
int    sagen_forward(sagen_ctx* ctx, const float* audio, const float* video, const float* flow,
                     float* ambi_yzx, void* stream);
/* The same with the video frames as they come out of the JPEG decoder: uint8 [B,224,448,3]; the reference's pixel normalisation
 * x/255 - 0.5 (myutils.py:88-89, img_prep of feeder.py:121-132) is applied on the device, bit-identical to the float32 the feeder
 * would have produced.  Host -> device traffic per window: 301 KB instead of 1.2 MB. */
int    sagen_forward_u8(sagen_ctx* ctx, const float* audio, const uint8_t* video_u8, const float* flow,
                        float* ambi_yzx, void* stream);
/* Grouped launch (round 6).  The reference runs ONE sess.run per batch (deploy.py:141, eval.py:145) and its batch-norm couples the
 * windows OF a batch (model.py:197, resnet.py:123: is_training=True), so a batch is the unit of work.  A grouped context runs
 * `groups` INDEPENDENT batches of cfg->batch windows as ONE launch per layer (the group is a grid dimension of every kernel): each
 * batch keeps its own batch-norm statistics, plane scales and maxima, and its output is bit-identical to what sagen_forward[_u8] of
 * an ungrouped context (running the same launch plan: sagen_plan_set / none) gives for that batch alone - the semantics per batch are untouched, the fixed cost of a launch is paid once
 * per `groups` batches.  sagen_create_grouped: as sagen_create; sagen_workspace_bytes then covers `groups` copies of the per-batch
 * region (the packed filters are shared).  sagen_forward_grouped[_u8]: audio [groups*B, snd_size], video / flow [groups*B,224,448,3],
 * ambi_yzx [groups*B, snd_dur, 3] - the batches back to back; `groups` must be the context's.  FREQ_MASK separation and the default
 * arithmetic only (sagen_set_option values that leave it are refused at the next forward); sagen_forward[_u8] on a grouped context
 * (groups > 1) is an error, as is the training step.  sagen_get_intermediate returns the tensors of group
 * sagen_set_option(ctx, "intermediate_group", g) (default 0). */
int    sagen_create_grouped(sagen_ctx** out, const sagen_config* cfg, int groups);
int    sagen_forward_grouped(sagen_ctx* ctx, int groups, const float* audio, const float* video, const float* flow,
                             float* ambi_yzx, void* stream);
int    sagen_forward_grouped_u8(sagen_ctx* ctx, int groups, const float* audio, const uint8_t* video_u8, const float* flow,
                                float* ambi_yzx, void* stream);
/* deploy.py:143-152: out[b, n, :] = [mono[b, snd_contx/2 + n], ambi_yzx[b, n, 0..2]] -> [B,snd_dur,4] WYZX */
int    sagen_assemble_wyzx(const float* audio, const float* ambi_yzx, float* out_wyzx,
                           int batch, int snd_size, int snd_contx, int snd_dur, void* stream);
/* named intermediate of the last forward (device pointer inside the workspace) for parity tests:
 * "mag", "stft", "audio_encoder/conv1".."conv5", "<enc>_encoder/conv5_2", "bottleneck",
 * "localization/coeffs", "separation/deconv1" (needed rows only). Returns dims in shape[4].
 * With num_in input channels: "mag" [B,127,1024,num_in]; "stft" [B, num_in*28, 513, 2] (= [B,num_in,28,513,2]);
 * "localization/coeffs" [B, 3, num_out*num_in, nsep+1] (= [B,3,num_out,num_in,nsep+1]); "separation/deconv1" [B,23,1024,num_in*nsep]. */
int    sagen_get_intermediate(const sagen_ctx* ctx, const char* name, const float** data,
                              int32_t* ndim, int64_t shape[4], int64_t* pixel_stride);

/* Per-layer launch planning (no reference analogue; cuDNN-style autotune): runs one forward on the given
 * inputs in which every contraction times its (tile shape, split-K) candidates with hipEvents and keeps the
 * fastest; later sagen_forward calls use the stored plan.  Synchronises the stream.  Without it (or with
 * SAGEN_NO_AUTOTUNE set) shape heuristics are used.  sagen_plan_describe writes
 * "layer\ttile\tsplitk\tmicroseconds\n" per contraction and returns the number of lines. */
int    sagen_autotune(sagen_ctx* ctx, const float* audio, const float* video, const float* flow,
                      float* ambi_yzx, void* stream);
int    sagen_plan_describe(sagen_ctx* ctx, char* buf, size_t buflen);
/* pin one layer's launch: tile = index into the contraction kernels' instantiation table (sagen_num_tiles /
 * sagen_tile_name below), splitk >= 1.  An instantiation that cannot run the layer falls back to the heuristic. */
int    sagen_plan_set(sagen_ctx* ctx, const char* layer, int tile, int splitk);
/* the instantiation table: names as sagen_plan_describe / sagen_profile_report print them (host-only calls, no device
 * needed): "igemm_kernel<...>" = exact fp32 MFMA, "igemm3*_kernel<...>" = fp32-equivalent bf16x3 */
int         sagen_num_tiles(void);
const char* sagen_tile_name(int tile);

/* Measurement aid (the reference's only analogue is the samples/sec printout, myutils.py:15-26):
 * when enabled, every launch of the following sagen_forward calls is bracketed by a pair of
 * hipEvents on the launch stream.  sagen_profile_report waits for the last forward's events and
 * writes one line per launch, "kernel\tlayer\tmicroseconds\tflops\n"; returns the number of lines
 * (>= 0) or a negative sagen_status. */
int    sagen_profile_enable(sagen_ctx* ctx, int on);
/* Per-context switches.  "materialize_mask" (default 0): 1 keeps the mask decoder's last layer (model.py:320-337) and the mask
 * application as two kernels so that the logits exist in the workspace ("separation/deconv1" of sagen_get_intermediate); 0 lets the
 * forward fold sigmoid + track mix into the deconvolution's epilogue (same result, 94 MB less HBM traffic per batch of 32). */
int    sagen_set_option(sagen_ctx* ctx, const char* name, int value);
/* Further switches: "fp16x2" (default 1: the ResNet trunk's convs - resnet.py:141-236 - run on two fp16 planes per operand, three matrix
 * products per multiply; 0: three bf16 planes, six products), "plane_gather", "u8_fast_stem", "planes_from_stage" (INTEGRATION.md 5).
 * sagen_counter reads a diagnostic counter of the context after synchronising `stream`: "fp16x2_saturations" = activation elements the
 * fp16x2 plane passes had to clamp to +-65000 since sagen_bind_weights (scales come from batch statistics with 64 x headroom beyond
 * eight standard deviations: 0 unless an activation is not finite or that far out; > 0 means results of the affected forwards are
 * not fp32-equivalent - rerun with "fp16x2" = 0). */
int    sagen_counter(sagen_ctx* ctx, const char* name, uint64_t* value, void* stream);
int    sagen_profile_report(sagen_ctx* ctx, char* buf, size_t buflen);

/* ---- op-level (unit-testable; same conventions) ----------------------------------------- */

/* myutils.stft (myutils.py:119-147) fused with the crop + tf.abs of audio_encoder_ops
 * (model.py:166-178): hop = wind/4, periodic Hann, 1024-pt FFT.
 * mag [B, f1-f0, 1024] magnitudes of frames [f0,f1); spec [B, c1-c0, 513, 2] (re,im) of frames
 * [c0,c1) (bins 0..512; the rest is the Hermitian mirror).  Either output may be NULL, not both.
 * Legal frames are the reference's: frame t covers samples [256 t, 256 t + 1024), and n_samples has
 * 4 * (n_samples / 1024 - 1) of them (integer division; 200 at 52799 samples, none below 2048) - frames that merely fit behind
 * those are not produced by myutils.stft and are refused.  SAGEN_ERR_SHAPE, before anything is launched, for batch <= 0,
 * f0 < 0, f1 <= f0, f1 > 4 * (n_samples / 1024 - 1) and, where spec is given, c0 < f0, c1 > f1 or c1 <= c0 (c0, c1 are ignored
 * where spec is NULL).  Both libraries share the rule (csrc/stft_frames.h). */
int sagen_stft_mag(const float* audio, int batch, int n_samples, int f0, int f1, float* mag,
                   int c0, int c1, float* spec, void* stream);

/* tfw.conv_2d (core.py:156-220) = tf.nn.convolution NHWC/HWIO + (bias | nothing) + optional ReLU.
 * padding: 0 = VALID, 1 = SAME (TF asymmetric).  Batch-norm is NOT applied here: pass bn_stats
 * (>= sagen_bn_stats_floats(...) floats, 8-byte aligned; holds 2*cout fp64 accumulators that the call
 * zeroes and fills with the per-channel sum and sum of squares of the raw output) and
 * call sagen_bn_finalize; the consumer applies scale/shift (+ReLU) via in_scale/in_shift.
 * in_scale/in_shift [Cin] (nullable): input is relu(x*scale+shift) before padding.
 * scratch: >= sagen_conv2d_scratch_bytes(...) bytes for the repacked filter (and, for cin == 3, the
 * zero-bordered 4-channel copy of the input).  Supported cin: a power of two >= 4; 3; or 1 with
 * padding VALID, kw % 4 == 0 and sw % 4 == 0 (the spectrogram conv). */
size_t sagen_conv2d_scratch_bytes(int batch, int h, int w, int kh, int kw, int cin, int cout);
/* The least scratch sagen_conv2d accepts: the repacked filter (and the 4-channel copy for cin == 3) without the room
 * sagen_conv2d_scratch_bytes adds for the activation planes of a dense 3x3 stride-1 SAME conv with cin % 16 == 0 (the size callers
 * allocated before those planes existed).  With less than sagen_conv2d_scratch_bytes such a conv runs on the fp32-activation kernels. */
size_t sagen_conv2d_min_scratch_bytes(int batch, int h, int w, int kh, int kw, int cin, int cout);
size_t sagen_bn_stats_floats(int batch, int hout, int wout, int cout);
int sagen_conv2d(const float* x, int batch, int h, int w, int cin,
                 const float* w_hwio, int kh, int kw, int cout, int sh, int sw, int padding,
                 const float* bias, int relu, const float* in_scale, const float* in_shift,
                 float* y, float* bn_stats, void* scratch, size_t scratch_bytes, void* stream);

/* contrib batch_norm in training mode (core.py:6,209-210; eps 1e-3, biased variance):
 * turns the partial sums into scale = gamma/sqrt(var+eps), shift = beta - mean*scale. */
int sagen_bn_finalize(const float* bn_stats, int batch, int hout, int wout, int cout,
                      const float* gamma, const float* beta, float eps,
                      float* scale, float* shift, void* stream);
/* y = relu(x*scale + shift (+ residual)) elementwise over [n_pixels, C] (resnet.py:221,235) */
int sagen_bn_apply_relu(const float* x, const float* scale, const float* shift,
                        const float* residual, float* y, int64_t n_pixels, int c, void* stream);
/* tf.nn.max_pool 3x3 s2 'SAME' (resnet.py:135) of relu(x*scale+shift) (scale NULL = identity) */
int sagen_maxpool3x3s2(const float* x, const float* scale, const float* shift, float* y,
                       int batch, int h, int w, int c, void* stream);

/* tfw.fully_connected (core.py:43-93): y[M,N] = act(x[M,K] @ w[K,N] + b). */
size_t sagen_fc_scratch_bytes(int m, int k, int n);
int sagen_fc(const float* x, int m, int k, const float* w_kn, int n, const float* bias, int relu,
             float* y, void* scratch, size_t scratch_bytes, void* stream);

/* tfw.deconv_2d (core.py:96-153) = tf.nn.conv2d_transpose VALID, w [kh,kw,Cout,Cin], + bias
 * (+ReLU).  y [B, h*sh+kh-sh, w*sw+kw-sw, cout]. */
size_t sagen_deconv2d_scratch_bytes(int kh, int kw, int cin, int cout, int sh, int sw);
int sagen_deconv2d(const float* x, int batch, int h, int w, int cin,
                   const float* w_hwoi, int kh, int kw, int cout, int sh, int sw,
                   const float* bias, int relu, float* y,
                   void* scratch, size_t scratch_bytes, void* stream);

/* Test accessors (host only, launch nothing): what sagen_conv2d / sagen_fc / sagen_deconv2d would run for these shapes, a scratch of
 * scratch_bytes and these optional operands (has_* != 0: the pointer would be non-NULL), as "<tile name> splitk=S planes=0|1" -
 * the instantiation name as sagen_tile_name spells it, the split-K factor (sagen_fc only; 1 elsewhere) and whether the plane
 * pre-pass of the dense 3x3 stride-1 SAME convs runs first.  They share the descriptor construction and the tile choice with the
 * ops themselves and return the op's own refusal for bad dimensions, unsupported channel counts and a short scratch, and
 * SAGEN_ERR_UNSUPPORTED for a tile that cannot run the problem.  They do NOT repeat the checks the contraction's launcher makes
 * after the filter has been packed - the prologue on a one-tap conv, a padded conv with more than 64 taps, the limit on the number of
 * taps, operands beyond 2 GiB buffer addressing: for such arguments an accessor names a kernel although the op refuses the call.
 * buf: >= 96 bytes. */
int sagen_conv2d_kernel_name(int batch, int h, int w, int cin, int kh, int kw, int cout, int sh, int sw, int padding, int has_prologue,
                             int has_stats, int has_bias, size_t scratch_bytes, char* buf, size_t buf_bytes);
int sagen_fc_kernel_name(int m, int k, int n, int has_bias, size_t scratch_bytes, char* buf, size_t buf_bytes);
int sagen_deconv2d_kernel_name(int batch, int h, int w, int cin, int kh, int kw, int cout, int sh, int sw, int has_bias,
                               size_t scratch_bytes, char* buf, size_t buf_bytes);

/* separation tail + decoder (model.py:326-347, myutils.istft myutils.py:181-211, model.py:421-434):
 * dmask  [B, 28, 1024, ntracks] : deconv1 output rows 43:71 (pre-sigmoid), NHWC
 * spec   [B, 28, 513, 2]        : STFT frames 89:117 (bins 0..512)
 * coeffs [B, 3, 3, ntracks+1]   : localization output (step, out-channel, track | bias)
 * ambi_yzx [B, 4800, 3].  scratch >= sagen_mask_istft_mix_scratch_bytes(batch). */
size_t sagen_mask_istft_mix_scratch_bytes(int batch);
int sagen_mask_istft_mix(const float* dmask, const float* spec, const float* coeffs, int batch,
                         int ntracks, float* ambi_yzx, void* scratch, size_t scratch_bytes, void* stream);
/* The same tail for nin input and nout output channels (ambi_order 2: nin = 4, nout = 5, the only pair implemented;
 * model.py:326-347, 428-430):
 * dmask  [B, 28, 1024, nin*ntracks] : deconv1 output rows 43:71 (pre-sigmoid); channel i*ntracks + j = track j of input channel i
 * spec   [B, nin, 28, 513, 2]       : STFT frames 89:117 of each input channel
 * coeffs [B, 3, nout, nin, ntracks+1]
 * out    [B, 4800, nout] = sum_i sum_j w[s,o,i,j] istft(sigmoid(m_ij) X_i) + coeffs[b,s,o,0,ntracks] (the bias of input channel 0).
 * scratch >= sagen_mask_istft_mix_hoa_scratch_bytes(batch, nout). */
size_t sagen_mask_istft_mix_hoa_scratch_bytes(int batch, int nout);
int sagen_mask_istft_mix_hoa(const float* dmask, const float* spec, const float* coeffs, int batch, int ntracks, int nin, int nout,
                             float* out, void* scratch, size_t scratch_bytes, void* stream);

/* SptAudioGen.evaluation_ops (model.py:110-154) for 0.1 s windows at 48 kHz, first-order (3 predicted channels):
 * per_sample [4][B][3] = stft distance (model.py:62-76; before the x100 and channel masking of :122-127), log-spectral
 * distance on the 1200-point STFT (:78-94), temporal MSE (:96-99; before x5e3) and SNR (:101-108);
 * power_sums[2] (fp64) = sum pred^2, sum target^2 over everything (-> pow/pred, pow/gt after /(3B)).
 * scratch: >= sagen_eval_scratch_bytes(batch) bytes, initialised ONCE with sagen_eval_init (DFT matrix). */
size_t sagen_eval_scratch_bytes(int batch);
int sagen_eval_init(void* scratch, size_t scratch_bytes, int batch, void* stream);
int sagen_eval_metrics(const float* pred_yzx, const float* target_yzx, int batch, float* per_sample,
                       double* power_sums, void* scratch, size_t scratch_bytes, void* stream);
/* The same metrics for `channels` predicted channels (ambi_order 2: 5, ACN 4..8): pred / target [B][4800][channels],
 * per_sample [4][B][channels]; power_sums as above (-> /(channels*B)).  scratch: >= sagen_eval_scratch_bytes_c(batch, channels)
 * bytes, initialised once with sagen_eval_init.  channels = 3 computes exactly what sagen_eval_metrics computes. */
size_t sagen_eval_scratch_bytes_c(int batch, int channels);
int sagen_eval_metrics_c(const float* pred, const float* target, int batch, int channels, float* per_sample,
                         double* power_sums, void* scratch, size_t scratch_bytes, void* stream);

/* AmbiDecoder.decode('projection') + RMS map (pyutils/ambisonics/decoder.py:24-28,
 * distance.py:41-52; SH matrix common.py:151-178, order 1 ACN/SN3D):
 * ambi_wyzx [T,4]; sh [P,4] device matrix; rms [P] = sqrt(mean_t (ambi . sh[p])^2).
 * The rms buffer must hold P + 24 floats (the tail is used for the 4x4 second-moment matrix). */
int sagen_power_map(const float* ambi_wyzx, int64_t t, const float* sh, int p, float* rms, void* stream);

/* One map per chunk: SphericalAmbisonicsVisualizer.loop_frames (pyutils/ambisonics/distance.py:41-59) yields one RMS map
 * per `window` seconds of audio; ambix_emd (distance.py:133-143, called at eval.py:190) compares them frame by frame.
 * ambi_wyzx [nchunks, T, 4] (chunks back to back); rms [nchunks, P]; moments = caller scratch of nchunks*10 doubles. */
int sagen_power_map_batched(const float* ambi_wyzx, int nchunks, int64_t t, const float* sh, int p, float* rms, double* moments,
                            void* stream);

/* The per-sample metrics eval.py computes on the host (eval.py:172-182), for 0.1 s windows at 48 kHz:
 *  - mel_lsd [B][C] = myutils.compute_lsd_dist (myutils.py:96-106): librosa 0.6.0 melspectrogram(sr=48000, n_mels=128, fmax=12000;
 *    reflect pad 1024, 10 frames of 2048 at hop 512, periodic Hann, power 2, Slaney mel basis with norm=1), L = 10 log10(M + 0.01),
 *    sqrt(mean over 128 x 10 of (L_gt - L_pred)^2);
 *  - env_mse [B][C] = myutils.compute_envelope_dist (myutils.py:109-116): |scipy.signal.hilbert| with N = 4800 (circular),
 *    sqrt(mean_n (env_gt - env_pred)^2).
 * pred / target [B][4800][C] (first order: C = 3, Y,Z,X; 1 <= C <= 8, SAGEN_ERR_UNSUPPORTED otherwise), no channel masking.
 * scratch: >= sagen_eval_mel_env_scratch_bytes(batch, channels) bytes (no init). */
size_t sagen_eval_mel_env_scratch_bytes(int batch, int channels);
int sagen_eval_mel_env(const float* pred, const float* target, int batch, int channels, float* mel_lsd, float* env_mse, void* scratch,
                       size_t scratch_bytes, void* stream);

/* emd/dir and emd/dir2 of eval.py:188-193 (ambix_emd -> emd, distance.py:100-143; pyemd 0.5.1 emd with its default extra-mass
 * penalty max(cost)) between directional RMS maps, exactly in fp64:
 *   emd[m][0] = EMD-hat(p_m / nodes, q_m / nodes), emd[m][1] = EMD-hat(p_m / (sum p_m + 0.01), q_m / (sum q_m + 0.01)),
 *   EMD-hat(P, Q) = min sum f_ij cost_ij over f >= 0 with row sums <= P_i, column sums <= Q_j, total min(sum P, sum Q)
 *                   + |sum P - sum Q| * max cost.
 * p / q [n_maps][nodes] (sagen_power_map_batched rows; nodes <= 96, SAGEN_ERR_UNSUPPORTED otherwise), cost [nodes][nodes] fp64 metric
 * (ambisonics.angular_distance), emd [n_maps][2] fp64.  A non-finite map gives NaN.  *not_converged (device uint32, not cleared)
 * is incremented once per problem that hit the solver's augmentation cap - the caller checks it. */
int sagen_eval_emd(const float* p, const float* q, int n_maps, int nodes, const double* cost, double* emd, uint32_t* not_converged,
                   void* stream);

/* ---- ambisonic rendering: one rotated FIR matrix ------------------------------------------------------------------------
 * Every rendering of the reference's output stage is linear and time-invariant after an optional rotation of the sound field,
 * so one operation replaces them all: the W+-Y stereo fold-down of myutils.gen_360video (myutils.py:285-294), AmbiDecoder.decode
 * (pyutils/ambisonics/decoder.py:24-28), DirectAmbisonicBinauralizer (binauralizer.py:156-166) and AmbisonicBinauralizer
 * (:124-153) over VirtualStereoMic.binauralize (:18-36) or Convolvotron.binauralize (:63-76) - the taps per rendering are built
 * on the host (spatialaudiogen_amd/render.py).  For a stream x[s, c] of `channels` ambisonic channels (ACN / SN3D; 4 or 9):
 *   x'[s]   = M(s) . x[s],   M(s) = (1 - a) R[m] + a R[min(m + 1, n_rot - 1)],
 *             m = min(floor(s / rot_hop), n_rot - 1), a = (s - m rot_hop) / rot_hop, a = 0 once m = n_rot - 1 (the last
 *             matrix is held exactly)                                                         (rot == NULL: M = I)
 *   y[t, o] = sum_c sum_{k < ntaps} taps[o][c][k] x'[t - k, c],                               x'[s] = 0 for s < 0
 * s, t are ABSOLUTE positions in the stream, so a stream may be rendered in pieces: x holds n_hist rows of history (the rows at
 * positions pos0 - n_hist .. pos0 - 1, unrotated) followed by the n new rows at pos0 .. pos0 + n - 1; rows the taps reach
 * before x[0] count as zero (n_hist < ntaps - 1 is legal at the start of a stream; n_hist <= pos0).  y [n, outputs]; outputs at
 * absolute t < zero_before are written as 0 (Convolvotron places a 'valid' convolution at ntaps - 1).  taps [outputs][channels]
 * [ntaps] and rot [n_rot][channels][channels] are device arrays.  fp32 throughout; the sum of one output sample runs in a fixed
 * order (channels outermost, taps ascending, one accumulator), so its value does not depend on how the stream is cut.
 * Supported: channels 4 or 9, outputs <= 32, ntaps <= 512 (SAGEN_ERR_UNSUPPORTED otherwise); a 4-channel x is 16-byte aligned. */
int sagen_render_fir(const float* x, int64_t n_hist, int64_t n, int channels, const float* taps, int outputs, int ntaps, const float* rot,
                     int n_rot, int rot_hop, int64_t pos0, int64_t zero_before, float* y, void* stream);

/* ---- power-map overlay: the sound-direction heat map over the video frames ---------------------------------------------
 * The visual half of myutils.gen_360video(overlay_map=True) (myutils.py:246-279): RMS maps of the decimated stream
 * (SphericalAmbisonicsVisualizer(ambix[::5], rate / 5, 5 / fps, 5.), pyutils/ambisonics/distance.py:16-59), normalised,
 * interpolated between consecutive maps, coloured and alpha-blended over the frames.
 *
 * sagen_power_map_windows: the maps of a strided stream (distance.py:41-52 over myutils.py:252's ambix[::5]).
 *   ambi [n_rows][channels] (ACN / SN3D; channels 4 or 9 = orders 1 and 2, SAGEN_ERR_UNSUPPORTED otherwise; a 4-channel ambi is
 *   16-byte aligned); map m reads the rows (m window + k) stride, k < window; n_maps = ((n_rows + stride - 1) / stride) / window
 *   (= len(ambix[::stride]) // window, distance.py:30); sh [p][channels] fp32 ('projection' decoding, decoder.py:24-28);
 *   rms [n_maps][p] = sqrt(max(sh[p]^T S_m sh[p], 0) / window) in fp64, S_m the second moments of window m.  n_maps == 0 returns
 *   SAGEN_OK and touches nothing.  A map depends on its own window only, so a stream may be cut at any window boundary.
 *   scratch: >= sagen_power_map_windows_scratch_bytes(n_maps, channels) bytes, 8-byte aligned. */
size_t sagen_power_map_windows_scratch_bytes(int n_maps, int channels);
int sagen_power_map_windows(const float* ambi, int64_t n_rows, int channels, int stride, int64_t window, const float* sh, int p, float* rms,
                            void* scratch, size_t scratch_bytes, void* stream);

/* sagen_overlay_blend: myutils.py:255-279 for a run of frames.  maps [n_maps][mh][mw] raw rms maps in IMAGE orientation (top row
 * +90 degrees elevation: the flipud of distance.py:52 is folded into the order of the sh rows), maps[0] being map `map0` of the
 * stream; lut [256][3] fp64 device colour table (plt.cm.YlOrRd(linspace(0, 1, 256))[:, :3], myutils.py:253); frames / out
 * [n_frames][h][w][3] uint8, frames[0] being frame `frame0` of the stream.  For the frame with absolute index F:
 *   prev = F / frames_per_map, cur = prev + 1 (absolute map indices), beta = (F % frames_per_map) / (double)frames_per_map
 *   n(map) = (map - min map) / (max map - min map + 0.005)                                   (myutils.py:256, 262; per map)
 *   v = (1 - beta) n(prev) + beta n(cur);  v = v 2 - 0.7;  v = 0 where v < 0                 (:270-272)
 *   idx = min(int(v 255), 255);  dir = resize(lut[idx], (h, w)) 255                          (:273-275)
 *   alpha = resize(v, (h, w)) 0.6;  out = uint8(alpha dir + (1 - alpha) frame)               (:277-279)
 * in fp64, in this operation order, without contraction.  resize is scikit-image 0.13.1's (order 1, mode 'constant', cval 0,
 * clip) restated: source coordinates r = (y + 0.5)(mh / h) - 0.5, c = (x + 0.5)(mw / w) - 0.5; corners floor / ceil, a corner
 * outside the map reads 0; top = (1 - dc) g(r0, c0) + dc g(r0, c1), bot likewise on r1, val = (1 - dr) top + dr bot; then with
 * lo / hi the minimum / maximum of the array handed to resize (the three colour channels together; v): lo <= 0 <= hi clips val
 * into [lo, hi], otherwise an exact 0 stays 0 and everything else is clipped into [lo, hi].
 * A frame whose two maps are not both inside [map0, map0 + n_maps) is SAGEN_ERR_SHAPE; n_frames == 0 returns SAGEN_OK.
 * Supported: mh <= 4096, mw <= 1000, h <= 65535, w <= 1048576, n_frames <= 65535.  scratch: >= sagen_overlay_blend_scratch_bytes(...) bytes,
 * 16-byte aligned. */
size_t sagen_overlay_blend_scratch_bytes(int n_maps, int mh, int mw, int n_frames);
int sagen_overlay_blend(const float* maps, int n_maps, int64_t map0, int mh, int mw, const double* lut, const uint8_t* frames, int n_frames,
                        int64_t frame0, int h, int w, int frames_per_map, uint8_t* out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- reprojection of 360-degree frames: equirectangular, cube maps, equi-angular cube maps, head viewport ----------------
 * What the reference does offline before the network sees a frame - the first-eye crop of scraping/preprocess.py:51-52, the
 * equi-angular unwarp and x / y remap tables of scraping/utils.py:91-144, the cube <-> equirect step of 3rd-party/vrProjector
 * (CubemapProjection.py:68-121, EquirectangularProjection.py:23-42) - and, behind the network, the pinhole view of a listener whose
 * head is turned by the Rot that ambisonics.head_rotation_matrix takes.  One operation: every destination sub-sample has a
 * direction, the direction is rotated, lands on a source pixel and is fetched bilinearly.
 *
 * World frame: x front, y left, z up; az = atan2(y, x), el = atan2(z, hypot(x, y)).  Positions are pixel centres: sub-sample (a, b)
 * of pixel (i, j) of a cell of W x H pixels sits at xf = (i + (a + 0.5) / S) / W, yf = (j + (b + 0.5) / S) / H, S = supersample.
 *   SAGEN_PROJ_ER    az = pi - 2 pi xf, el = pi / 2 - pi yf (front at the centre, the listener's left on the left).  As a source:
 *                    x = (pi - az) / (2 pi) W - 0.5, y = (pi / 2 - el) / pi H - 0.5, bilinear, wrapping in x, clamped in y.  The
 *                    image is the rectangle (x0, y0, w, h) of the frame (w = h = 0: the whole frame); top-bottom stereo is the
 *                    rectangle of the top half.
 *   SAGEN_PROJ_CUBE  face coordinates (p, q) = (2 xf - 1, 2 yf - 1) in the face's cell; direction = axis + p right + q down.  As a
 *                    source the face is the one whose axis has the largest |component|; x = (p + 1) / 2 n - 0.5 clamped into
 *                    [0, n - 1] (likewise y): bilinear inside the face, no filtering across faces.
 *   SAGEN_PROJ_EAC   the same with p -> tan(pi p / 4), q -> tan(pi q / 4) (the inverse of utils.py:97-98).
 *   SAGEN_PROJ_VIEW  destination only: direction = (1, t (1 - 2 xf), t (H / W) (1 - 2 yf)), t = tan(hfov / 2), hfov in radians.
 * face[f], f = 0..5, is the face of axis +x -x +y -y +z -z: a square rectangle of the frame and an orientation 0..7 against
 * vrProjector's face image of that axis (bit 2: mirrored left-right; bits 0-1: quarter turns, 1 = the cell is np.rot90(image)).
 * Destination pixels that lie in no rectangle are not written.
 *
 * src [n][src_h][src_w][3], dst [n][dst_h][dst_w][3] uint8 (RGB only).  rot [n_rot][3][3] fp64 DEVICE array, row-major, world
 * direction = rot . head direction; n_rot = 0 (identity; rot is ignored), 1 (all frames) or n (one per frame).  Per channel the
 * mean of the S x S bilinear samples, in fp64, stored as floor(mean + 0.5).
 * Returns: n == 0 SAGEN_OK, nothing touched; a null argument SAGEN_ERR_NULL; SAGEN_ERR_SHAPE for n < 0, a frame dimension < 1, a
 * rectangle outside its frame, a non-square face, an orientation outside 0..7, n_rot not in {0, 1, n}, hfov outside (0, pi);
 * SAGEN_ERR_UNSUPPORTED for supersample outside 1..8, a dimension above 16384, n > 65535, an unknown kind, VIEW as a source.
 * scratch: >= sagen_reproject_scratch_bytes(...) bytes (0 today: the kernel is fused; a null scratch is accepted then). */
enum { SAGEN_PROJ_ER = 0, SAGEN_PROJ_CUBE = 1, SAGEN_PROJ_EAC = 2, SAGEN_PROJ_VIEW = 3 };
typedef struct sagen_proj_face {
    int32_t x0, y0, w, h;       /* rectangle of the frame, w == h */
    int32_t orient;             /* 0..7 */
} sagen_proj_face;
typedef struct sagen_projection {
    int32_t kind;               /* SAGEN_PROJ_* */
    int32_t x0, y0, w, h;       /* ER / VIEW: rectangle of the frame (w = h = 0: all of it) */
    double hfov;                /* VIEW: horizontal field of view, radians */
    sagen_proj_face face[6];    /* CUBE / EAC */
} sagen_projection;
size_t sagen_reproject_scratch_bytes(int n, int dst_h, int dst_w, int supersample);
int sagen_reproject(const uint8_t* src, int n, int src_h, int src_w, const sagen_projection* src_proj, uint8_t* dst, int dst_h, int dst_w,
                    const sagen_projection* dst_proj, const double* rot, int n_rot, int supersample, void* scratch, size_t scratch_bytes,
                    void* stream);

/* ---- dense optical flow between consecutive frames, and the flow folder's byte coding --------------------------------------
 * The reference's third encoder reads a folder flow/%06d.jpg + flow/flow_limits.npy (feeder.py:135-161) that it makes offline with
 * FlowNet2 under caffe (scraping/preprocess.py:156-204, scraping/flow.py).  sagen_optical_flow is NOT that network: it is a
 * classical pyramidal Horn-Schunck estimator with warping, so a checkpoint trained on FlowNet2 flows sees another estimator here.
 * sagen_flow_encode restates the storage format of preprocess.py:183-196 exactly.
 *
 * frames [n_frames][h][w][3] uint8 RGB -> flow [n_frames - 1][h][w][2] fp32: flow k goes from frame k to frame k + 1, u (channel 0)
 * in pixels to the right, v (channel 1) in pixels down.  Everything before the one rounding to fp32 is fp64.
 * Neighbour and fetch rule, used everywhere: a row index (or coordinate) is clamped into [0, h - 1]; a column index wraps modulo w
 * when wrap = 1 (the equirectangular seam) and is clamped into [0, w - 1] when wrap = 0.  Bilinear fetches apply the rule to the
 * taps of floor(coordinate); coordinates are held within +-2^20.
 *   luma      0.299 R + 0.587 G + 0.114 B, levels 0..255
 *   pyramid   level l + 1 is the 2 x 2 mean of level l; a fine centre (x, y) sits at coarse ((x + .5) / 2 - .5, (y + .5) / 2 - .5).
 *             h and w must be divisible by 2^(levels - 1)
 *   level     coarsest first.  Both images are smoothed by the separable binomial [1 4 6 4 1] / 16, rows first.  The flow starts at
 *             zero on the coarsest level, elsewhere at 2 x the bilinear fetch of the coarser flow at the coordinates above
 *   warp      (u0, v0) = the flow so far; I2w(x, y) = bilinear fetch of the smoothed second image at (x + u0, y + v0);
 *             Ix = ((I2w[x+1] - I2w[x-1]) + (I1[x+1] - I1[x-1])) / 4, Iy likewise, It = I2w - I1
 *   iteration (Jacobi, `iters` per warp, from (u0, v0))  ubar = the 4 edge neighbours / 6 + the 4 diagonal neighbours / 12;
 *             t = (Ix (ubar - u0) + Iy (vbar - v0) + It) / (alpha^2 + Ix^2 + Iy^2); u = ubar - Ix t, v = vbar - Iy t
 * fuse: Jacobi iterations per launch on a tile held in LDS (temporal blocking), 1..8, 0 = the library's choice.  The result does
 * not depend on it, bit for bit; sagen_flow_auto_fuse() is the depth that 0 takes (host-only).  Identical frames give a flow of
 * exactly zero.
 * Returns: n_frames <= 1 (but >= 0) SAGEN_OK, nothing touched; a null argument SAGEN_ERR_NULL; SAGEN_ERR_SHAPE for n_frames < 0,
 * h or w < 1, h or w not divisible by 2^(levels - 1), scratch smaller than sagen_optical_flow_scratch_bytes(...) or not 8-byte
 * aligned; SAGEN_ERR_UNSUPPORTED for levels outside 1..8, warps outside 1..16, iters outside 1..1000, fuse outside 0..8, alpha <= 0
 * or not finite, h or w above 4096, a coarsest level of fewer than 4 rows or columns, n_frames > 65535.  A refused call writes
 * nothing; sagen_last_error names the parameter.  sagen_optical_flow_scratch_bytes is 0 for sizes the call would refuse.
 *
 * sagen_flow_encode: flow [n][h][w][2] fp32 -> rgb [n][h][w][3] uint8 and limits [n][2] fp32 (the rows of flow_limits.npy).
 *   per pixel  mag = (float)sqrt((double)u^2 + (double)v^2); ang = atan2(v, u) + pi in fp64, 0 where mag < 0.005
 *   per frame  lo, hi = min, max of mag; if hi - lo < 1 then hi = lo + 1, in fp32: the stored limits are the ones used
 *   bytes      R = trunc(ang * 255 / (2 pi)), G = 0, B = trunc((mag - lo) / (hi - lo) * 255) in fp64 on the fp32 mag, lo, hi
 * The + pi is the reference's: feeder.py:147-160 decodes m cos(a), m sin(a) WITHOUT subtracting it, so the network sees the
 * NEGATED flow vector, there as here.
 * Returns: n == 0 SAGEN_OK, nothing touched; a null argument SAGEN_ERR_NULL; SAGEN_ERR_SHAPE for n < 0, h or w < 1, scratch
 * smaller than sagen_flow_encode_scratch_bytes(...); SAGEN_ERR_UNSUPPORTED for h or w above 4096, n > 65535. */
typedef struct sagen_flow_params {
    int32_t levels;             /* pyramid levels, 1..8 */
    int32_t warps;              /* warps per level, 1..16 */
    int32_t iters;              /* Jacobi iterations per warp, 1..1000 */
    int32_t wrap;               /* 1: columns wrap (equirectangular), 0: clamped */
    int32_t fuse;               /* Jacobi iterations per launch, 1..8; 0: the library chooses */
    double alpha;               /* smoothness weight, in levels of 0..255 */
} sagen_flow_params;
size_t sagen_optical_flow_scratch_bytes(int n_frames, int h, int w, int levels);
int sagen_optical_flow(const uint8_t* frames, int n_frames, int h, int w, const sagen_flow_params* p, float* flow, void* scratch,
                       size_t scratch_bytes, void* stream);
int sagen_flow_auto_fuse(void);
size_t sagen_flow_encode_scratch_bytes(int n, int h, int w);
int sagen_flow_encode(const float* flow, int n, int h, int w, uint8_t* rgb, float* limits, void* scratch, size_t scratch_bytes,
                      void* stream);

/* ---- rational polyphase FIR resampling, and the RMS of strided windows ---------------------------------------------------------
 * The reference resamples in three places: resampy.resample(..., 'kaiser_fast') in load_wav(fname, rate) (pyutils/iolib/audio.py:23),
 * `ffmpeg -ar 48000` with the `pan=4c|c0=c...` channel remap of prepare_ambisonics (scraping/preprocess.py:14-34), and
 * AmbisonicArray.convert(sample_rate, ordering, normalization) (pyutils/ambisonics/common.py:34-59); compute_audio_pow
 * (scraping/preprocess.py:146-153) then writes the RMS of 0.1-s windows.  sagen_resample_fir is NOT resampy's tabulated filter nor
 * swresample: it is a Kaiser-windowed sinc of our own in rational polyphase form, bit-compatible with neither.
 *
 * Rates rate_in : rate_out = M : L in lowest terms; h[k], k = -H .. H, is the prototype filter at L x the input rate (zero phase:
 * output 0 sits on input 0).  With z[m][o] = sum_c mix[o][c] x[m][c] (c ascending; mix null: z = x, c_out = c_in),
 *   y[n][o] = sum_m h[n M - m L] z[m][o]   over |n M - m L| <= H, m ascending,
 * both sums in fp64, each product rounded before it is added, one rounding to fp32 at the end.
 *   taps [L][T] fp64, T = ceil((2 H + 1) / L): row p serves the outputs of phase (n M) mod L = p, in the order of m:
 *        taps[p][t] = h[kmax(p) - t L], kmax(p) = p + L floor((H - p) / L), zero where that index falls below -H;
 *        output n reads the rows m = ceil((n M - H) / L) + t
 *   x    [n_in][c_in] fp32: the stream's rows x0 .. x0 + n_in - 1.  Rows outside the buffer (and before the stream, m < 0) count as
 *        zero: the caller supplies every row the stream really has among those the outputs reach
 *   y    [n][c_out] fp32: the outputs n0 .. n0 + n - 1
 * An output's value depends on n and the rows alone, not on the window (x0, n_in, n0, n) it is computed in: a stream resampled in
 * pieces gives the bits of the one-call result.
 * Returns: n == 0 SAGEN_OK, nothing touched; a null taps, y or (with n_in > 0) x SAGEN_ERR_NULL; SAGEN_ERR_SHAPE for L, M or T < 1,
 * H < 0, T != ceil((2 H + 1) / L), a negative x0, n_in, n0 or n, c_in or c_out < 1, c_out != c_in without a mix;
 * SAGEN_ERR_UNSUPPORTED for more than 64 channels on either side, T > 4096, L or M > 2^20, a table above 64 MiB, a position or count
 * above 2^40.  A refused call writes nothing; sagen_last_error names the parameter.
 *
 * sagen_window_rms: x [n][channels] fp32 -> rms[i] = sqrt(sum_{j < length} x[first + i hop + j][channel]^2 / length), i < count, fp64:
 * the device form of compute_audio_pow.  The sum runs in one fixed order: 64 partial sums (partial l takes j = l, l + 64, ...
 * ascending), then a butterfly over the partials (l with l ^ 1, then ^ 2, ... ^ 32).
 * Returns: count == 0 SAGEN_OK, nothing touched; a null argument SAGEN_ERR_NULL; SAGEN_ERR_SHAPE for a negative n or count, a channel
 * outside the row, length < 1, hop or first < 0, a window that does not lie inside the n rows; SAGEN_ERR_UNSUPPORTED for n > 2^40,
 * channels > 2^20, count >= 2^31. */
int sagen_resample_fir(const float* x, int64_t x0, int64_t n_in, int c_in, const double* taps, int L, int M, int H, int T, const double* mix,
                       int c_out, int64_t n0, int64_t n, float* y, void* stream);
int sagen_window_rms(const float* x, int64_t n, int channels, int channel, int64_t first, int64_t hop, int64_t length, int64_t count,
                     double* rms, void* stream);

/* ---- baseline JPEG decode ---------------------------------------------------------------------------------------------------
 * The reference reads every frame with skimage / PIL on the host (feeder.py:18-23 behind the video and flow readers; the scraping
 * tools likewise) - libjpeg.  sagen_jpeg_decode takes the FILE BYTES of n frames on the device and writes out [n][h][w][3] uint8
 * RGB, the layout sagen_reproject, sagen_optical_flow, sagen_overlay_blend and sagen_forward_u8 read, byte for byte what libjpeg's
 * default decode path gives (PIL's Image.open(...).convert('RGB')): integer arithmetic end to end.
 *
 * Scope: baseline sequential DCT (SOF0), 8-bit samples, Huffman coding, ONE interleaved scan; components = 1 (grey, replicated to
 * R = G = B; hs = vs = 1) or 3 (YCbCr, luma sampling (hs, vs) in {(1, 1), (2, 1), (2, 2)}, chroma (1, 1)); an optional restart
 * interval.  All frames of a call share width, height, components, hs, vs; tables, restart interval and scan length are per frame.
 * The marker walk is the caller's (spatialaudiogen_amd/jpeg.py); the library sees:
 *   bytes     [total_bytes] uint8 DEVICE: the files (or just their scans), concatenated; 4-byte aligned, total_bytes a multiple of 4
 *             (the caller pads): the entropy stage refills its bit window by aligned 32-bit loads and reads nothing outside
 *   frames    [n] sagen_jpeg_frame DEVICE (64 bytes each)
 *   segments  [n_segments][2] int32 DEVICE: (frame, offset of the segment's first byte inside that frame's scan).  A frame without
 *             restart interval has one segment at offset 0; with an interval of R MCUs it has ceil(MCUs / R), segment k > 0 starting
 *             right behind the marker FF D0+((k-1) & 7); a segment ends 2 bytes before the next one, the last at the scan's end.
 *             Frame f owns the rows first_segment .. first_segment + n_segments - 1
 *   qtabs     [n_qtabs][64] uint16 DEVICE: quantisation tables in the file's (zigzag) order
 *   hufftabs  [n_hufftabs][272] uint8 DEVICE: 16 counts (codes of length 1..16) + 256 symbols, as in DHT (unused symbols: any value)
 *   status    [n] int32 DEVICE: 0, or a set of SAGEN_JPEG_ST_* bits; a frame with a non-zero status has unspecified pixels, every
 *             other frame of the call is exact
 * Entropy decode: one lane per segment: Huffman decode (8-bit lookahead table + code-length search), EXTEND, DC prediction per
 * component reset at every segment, EOB / ZRL, FF 00 unstuffing, coefficients to natural order.  Dequantisation coef * q[k], the
 * "islow" inverse DCT (CONST_BITS 13, PASS1_BITS 2: columns (x + 1024) >> 11, rows (x + 2^17) >> 18, + 128, clamped), "fancy"
 * triangle chroma upsampling on the ceil(w / hs) x ceil(h / vs) plane (edges replicated at THOSE bounds), and
 * R = y + ((91881 cr + 32768) >> 16), G = y + ((-22554 cb - 46802 cr + 32768) >> 16), B = y + ((116130 cb + 32768) >> 16), clamped.
 * Every >> is an arithmetic shift of a signed 32-bit integer.  For coefficients an encoder can make from 8-bit samples every
 * product stays inside 32 bits; where a hostile stream overflows them the arithmetic wraps modulo 2^32 (defined, pixels unspecified).
 * Hostile bytes: every loop is bounded by the geometry (MCUs x blocks x 64 coefficients x 16 code bits); a lane that needs bits
 * past its segment's end reads zeros and sets SAGEN_JPEG_ST_OVERRUN; descriptors are checked on the device before they are used
 * (SAGEN_JPEG_ST_DESC: offsets outside bytes, table indices outside the tables, a segment list that is not the frame's).
 * Returns: n == 0 SAGEN_OK, nothing touched; a null argument SAGEN_ERR_NULL; SAGEN_ERR_SHAPE for n < 0, w or h < 1, total_bytes < 0
 * or not a multiple of 4, n_segments < n, a table count < 1, bytes / frames / segments / qtabs / scratch misaligned (4, 8, 4, 2, 16
 * bytes; status 4); SAGEN_ERR_UNSUPPORTED for components / sampling outside the scope, w or h above 16384, n > 65535, more than
 * 2^31 - 1 blocks, output bytes or file bytes per call, more than 65536 tables of a kind; SAGEN_ERR_WORKSPACE for scratch smaller than sagen_jpeg_decode_scratch_bytes(...).  A refused
 * call writes nothing.  sagen_jpeg_decode_scratch_bytes is 0 for a geometry the call would refuse. */
enum {
    SAGEN_JPEG_ST_OVERRUN = 1,   /* bits needed past the end of a segment (truncated stream) */
    SAGEN_JPEG_ST_CODE = 2,      /* a bit pattern that is no code of the table */
    SAGEN_JPEG_ST_INDEX = 4,     /* a run past coefficient 63 */
    SAGEN_JPEG_ST_MARKER = 8,    /* a marker inside a segment, or not the expected restart marker in front of it */
    SAGEN_JPEG_ST_DESC = 16,     /* the frame's descriptor or segment rows are inconsistent */
    SAGEN_JPEG_ST_TABLE = 32,    /* a Huffman table that is no prefix code (or lists more than 256 symbols) */
    SAGEN_JPEG_ST_RANGE = 64,    /* a magnitude category above baseline's (DC 11, AC 10), or a DC value outside 16 bits */
    SAGEN_JPEG_ST_TRAILING = 128 /* bytes left in a segment after its last MCU */
};
typedef struct sagen_jpeg_frame {
    int64_t scan_offset;        /* offset in `bytes` of the first entropy-coded byte (behind the SOS header) */
    int32_t scan_bytes;         /* length of the entropy-coded data, restart markers included, the EOI marker not */
    int32_t restart_interval;   /* MCUs per segment; 0: none */
    int32_t first_segment;      /* row of `segments` */
    int32_t n_segments;
    int32_t qtab[3];            /* per component: row of qtabs */
    int32_t dctab[3];           /* per component: row of hufftabs */
    int32_t actab[3];
    int32_t reserved;           /* 0 */
} sagen_jpeg_frame;             /* 64 bytes */
size_t sagen_jpeg_decode_scratch_bytes(int n, int w, int h, int components, int hs, int vs, int n_hufftabs);
int sagen_jpeg_decode(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, int n, const int32_t* segments,
                      int n_segments, const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, int w, int h,
                      int components, int hs, int vs, uint8_t* out, int32_t* status, void* scratch, size_t scratch_bytes, void* stream);

/* ---- baseline JPEG decode, scans without restart markers on many lanes ---------------------------------------------------------
 * sagen_jpeg_decode_split takes every argument of sagen_jpeg_decode, in the same order, and writes EXACTLY the out and status that
 * call writes for them, hostile input included.  Its entropy stage cuts every restart segment - the whole scan of a file without
 * an interval - into chunks of chunk_bytes bytes with one lane per chunk; the lanes find their entry states by self-synchronisation
 * of the Huffman stream in `rounds` passes (csrc/jpeg_split_core.h has the algorithm and the argument for the guarantee).
 *   chunk_bytes  bytes of scan per lane: a multiple of 4 in [16, 65536]
 *   rounds       synchronisation passes, [1, 64]; rounds >= the chunks of the longest segment always settles
 *   max_chunks   capacity of the chunk tables in the scratch, n_segments <= max_chunks <= 2^31 - 1; a segment of L bytes has
 *                max(1, ceil(L / chunk_bytes)) chunks, and segments are placed in the order of their rows
 *   path         [n] int32 DEVICE, may be null: who produced the frame's coefficients.  0: the split path (also a frame the
 *                descriptor check refused: nothing decodes it).  Otherwise the frame was zeroed again and decoded by one lane per
 *                segment, as sagen_jpeg_decode does it, because (the first that applies) its chunks did not fit max_chunks
 *                (CAPACITY), a chunk was not synchronised after `rounds` passes (UNSETTLED), or the split path met anything the
 *                one-lane path would report, or an inconsistency of its own (ANOMALY).  A deterministic function of the arguments.
 * Returns: as sagen_jpeg_decode; SAGEN_ERR_SHAPE also for chunk_bytes, rounds or max_chunks outside their ranges and a path that is
 * not 4-byte aligned; SAGEN_ERR_WORKSPACE for scratch smaller than sagen_jpeg_decode_split_scratch_bytes(...), which is 0 for a call
 * that would be refused.  n == 0 SAGEN_OK, nothing touched.  A refused call writes nothing.  No host synchronisation, no allocation;
 * the number of launches depends on the arguments only. */
enum {
    SAGEN_JPEG_PATH_UNSETTLED = 1,
    SAGEN_JPEG_PATH_ANOMALY = 2,
    SAGEN_JPEG_PATH_CAPACITY = 4
};
size_t sagen_jpeg_decode_split_scratch_bytes(int n, int w, int h, int components, int hs, int vs, int n_hufftabs, int n_segments, int64_t max_chunks);
int sagen_jpeg_decode_split(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, int n, const int32_t* segments,
                            int n_segments, const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, int w, int h,
                            int components, int hs, int vs, uint8_t* out, int32_t* status, void* scratch, size_t scratch_bytes, void* stream,
                            int chunk_bytes, int rounds, int64_t max_chunks, int32_t* path);

/* ---- baseline JPEG encode ---------------------------------------------------------------------------------------------------
 * The reference gets its frame folders from ffmpeg's "%06d.jpg" extraction (scraping/preprocess.py:183-196) and leaves every later
 * frame write to the host's libjpeg.  sagen_jpeg_encode takes n frames on the device and writes the ENTROPY-CODED DATA of each,
 * what stands between the SOS header and FF D9, bit for bit what libjpeg's default path writes (PIL's save with optimize=False)
 * for the same pixels, quantisation tables and sampling: integer arithmetic end to end.  Headers, FF D9 and the file are the
 * caller's (spatialaudiogen_amd/jpeg.py).
 *   frames   [n][h][w][3] uint8 RGB DEVICE for components == 3 (what sagen_reproject and sagen_flow_encode write); [n][h][w] grey
 *            for components == 1
 *   hs, vs   luma sampling factors, (1,1), (2,1) or (2,2); chroma is (1,1); grey is (1,1)
 *   qtabs    [2][64] uint16 DEVICE, luma then chroma, in file (zigzag) order, entries 1..255; grey reads row 0 only.  An entry
 *            outside 1..255 is found on the device and gives every frame SAGEN_JPEG_ENC_ST_RANGE; nothing divides by zero
 *   out      [n][stride] uint8 DEVICE
 *   sizes    [n] int32 DEVICE: the bytes frame f's stream needs (saturating at 2^31 - 1), filled even when that exceeds stride: then
 *            nothing beyond out[f][stride - 1] is written, the status is CAPACITY and the frame's bytes are unspecified
 *   status   [n] int32 DEVICE: 0 or a set of SAGEN_JPEG_ENC_ST_* bits; a frame with a non-zero status leaves every other exact
 * The Huffman tables are the four of Annex K.3 - K.6, compiled in.  No restart intervals.
 * Arithmetic: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16,
 * Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16; the image's columns are replicated to whole blocks and its rows to a
 * multiple of vs, chroma is the 2 x 2 or 2 x 1 box mean with the bias alternating by output column (1, 2 / 0, 1), then the
 * COMPONENT's last row is replicated to whole blocks; the "islow" forward DCT (CONST_BITS 13, PASS1_BITS 2) on samples - 128;
 * (|c| + 4 q) / (8 q) with the sign put back; DC differences per component over the whole frame; luma blocks of an MCU that lie
 * wholly outside the image repeat the DC in front of them and hold no AC.  Bits MSB first, the last byte filled with ones, 00
 * behind every FF.
 * sagen_jpeg_encode_max_bytes: the stride that can never be too small, 2 ceil(blocks 1658 / 8) + 2 (a block is at most 9 + 11
 * bits of DC and 63 x (16 + 10) bits of AC; stuffing can double the bytes); 0 for a geometry outside the scope.
 * Returns: n == 0 SAGEN_OK, nothing touched; a null argument SAGEN_ERR_NULL; SAGEN_ERR_SHAPE for n < 0, w or h < 1, stride < 1 or
 * not a multiple of 4, out / sizes / status / qtabs / scratch misaligned (4, 4, 4, 2, 16 bytes); SAGEN_ERR_UNSUPPORTED for
 * components / sampling outside the scope, w or h above 16384, n > 65535, stride > 2^28, more than 2^31 - 1 blocks or frame bytes
 * per call; SAGEN_ERR_WORKSPACE for scratch smaller than sagen_jpeg_encode_scratch_bytes(...), which is 0 for a geometry the call
 * would refuse.  A refused call writes nothing. */
enum {
    SAGEN_JPEG_ENC_ST_CAPACITY = 1, /* the stream needs more than `stride` bytes; sizes[f] holds what it needs */
    SAGEN_JPEG_ENC_ST_RANGE = 2     /* a DC difference above category 11 or an AC value above category 10 (or a bad quantiser) */
};
size_t sagen_jpeg_encode_scratch_bytes(int n, int w, int h, int components, int hs, int vs, int64_t stride);
int64_t sagen_jpeg_encode_max_bytes(int w, int h, int components, int hs, int vs);
int sagen_jpeg_encode(const uint8_t* frames, int n, int w, int h, int components, int hs, int vs, const uint16_t* qtabs, uint8_t* out,
                      int64_t stride, int32_t* sizes, int32_t* status, void* scratch, size_t scratch_bytes, void* stream);

/* ---- baseline JPEG encode with restart intervals ----------------------------------------------------------------------------
 * sagen_jpeg_decode runs one lane per restart segment, so a file without restart interval is decoded by one lane.
 * sagen_jpeg_encode_rst is sagen_jpeg_encode with a restart interval: every argument, status bit and return code as there, plus
 *   restart_interval  MCUs per segment, as the DRI segment of the header names it (the caller's, FF DD 00 04 RRRR directly in
 *                     front of SOS); 0: none, and then the call writes exactly what sagen_jpeg_encode writes; 1..65535 are
 *                     accepted, anything else is SAGEN_ERR_UNSUPPORTED.  An interval of at least the frame's MCU count writes
 *                     no marker
 * The stream is the one libjpeg writes for the same interval (PIL's save with restart_marker_blocks=R, optimize=False).  In front
 * of MCU number k R for k >= 1, never behind the last MCU: the bit buffer is filled with ones to a byte boundary (nothing where it
 * stands on one); that byte is followed by 00 if it comes out as FF, like any other; FF D0+((k-1) & 7) follows and is NOT stuffed;
 * every component's DC prediction goes back to 0, so the DC difference of a segment's first blocks is against 0 (a luma block
 * wholly outside the image still repeats the DC in front of it: an MCU's first block is never one).  The end of the scan is
 * unchanged.  No stage walks a frame: the bit positions come from a segmented prefix sum, each segment starting on a byte, and
 * the markers are placed by the pass that stuffs the bytes.
 * sagen_jpeg_encode_rst_max_bytes: the stride that can never be too small.  With S = ceil(MCUs / R) segments (1 for R = 0 or
 * R >= MCUs) it is sagen_jpeg_encode_max_bytes + 4 (S - 1): each fill moves the unstuffed bytes up by less than one per segment
 * (ceil(a / 8) + ceil(b / 8) <= ceil((a + b) / 8) + 1), so by at most S - 1 in all, a fill byte that is FF included; stuffing can
 * double those; the S - 1 markers of two bytes are not stuffed.  sizes[f] never exceeds it.  0 for a geometry or an interval
 * outside the scope.  sagen_jpeg_encode_rst_scratch_bytes likewise; for restart_interval 0 it is
 * sagen_jpeg_encode_scratch_bytes. */
size_t sagen_jpeg_encode_rst_scratch_bytes(int n, int w, int h, int components, int hs, int vs, int restart_interval, int64_t stride);
int64_t sagen_jpeg_encode_rst_max_bytes(int w, int h, int components, int hs, int vs, int restart_interval);
int sagen_jpeg_encode_rst(const uint8_t* frames, int n, int w, int h, int components, int hs, int vs, int restart_interval,
                          const uint16_t* qtabs, uint8_t* out, int64_t stride, int32_t* sizes, int32_t* status, void* scratch,
                          size_t scratch_bytes, void* stream);

/* ---- re-segmenting existing JPEG files: a lossless transcode ------------------------------------------------------------------
 * sagen_jpeg_transcode gives files that exist (ffmpeg's extraction, PIL's saves) a restart interval without computing a pixel.
 * Inputs as sagen_jpeg_decode takes them - bytes, frames, segments, hufftabs and the geometry; no qtabs (the descriptors' qtab
 * indices only have to be non-negative), no pixels - plus restart_interval as sagen_jpeg_encode_rst takes it.  The decoder's table,
 * check and entropy stages fill int16 coefficients, a kernel puts them from natural into zigzag order, and the entropy half of
 * sagen_jpeg_encode_rst codes THOSE coefficients with the standard tables (Annex K.3 - K.6) and the new interval.  Every block the
 * source scan holds is coded as it stands, the luma blocks of an MCU that lie wholly outside the image included: the pixel
 * encoder's rule for such blocks does not apply, the DC prediction is the component's previous block in the segment.  The
 * coefficients of the written scan equal those of the source; header and FF D9 are the caller's (spatialaudiogen_amd/jpeg.py).
 *   out, sizes  as sagen_jpeg_encode: [n][stride] and the bytes each stream needs, filled even where that exceeds stride
 *   status      [n] int32 DEVICE: the decoder's SAGEN_JPEG_ST_* bits in bits 0..7, the encoder's SAGEN_JPEG_ENC_ST_* bits shifted
 *               left by 8 (a DC difference that the new segmentation pushes above category 11 is RANGE << 8).  A frame with a
 *               non-zero status has unspecified bytes and leaves every other frame exact
 * sagen_jpeg_transcode_max_bytes: 2 ceil(blocks 1660 / 8) + 2 + 4 (S - 1) for S segments - a file's block can hold what the
 * tables allow (11 + 11 bits of DC, 63 x (16 + 10) of AC), not only what 8-bit samples reach; the terms for the segments as above.
 * Returns: as sagen_jpeg_decode and sagen_jpeg_encode_rst for the arguments each shares (n == 0 SAGEN_OK, nothing touched; a null
 * argument SAGEN_ERR_NULL; shapes, alignments and the scope as there); SAGEN_ERR_WORKSPACE for scratch smaller than
 * sagen_jpeg_transcode_scratch_bytes(...), which is 0 for a call that would be refused.  A refused call writes nothing. */
size_t sagen_jpeg_transcode_scratch_bytes(int n, int w, int h, int components, int hs, int vs, int n_hufftabs, int restart_interval,
                                          int64_t stride);
int64_t sagen_jpeg_transcode_max_bytes(int w, int h, int components, int hs, int vs, int restart_interval);
int sagen_jpeg_transcode(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, int n, const int32_t* segments,
                         int n_segments, const uint8_t* hufftabs, int n_hufftabs, int w, int h, int components, int hs, int vs,
                         int restart_interval, uint8_t* out, int64_t stride, int32_t* sizes, int32_t* status, void* scratch,
                         size_t scratch_bytes, void* stream);

/* ---- PNG frames: the row filters and a zlib stream -------------------------------------------------------------------------
 * The reference muxes lossless frames (myutils.py:246-279) and leaves their compression to the host; the overlay writers here
 * called PIL's save per frame.  These two ops are that step over frames that lie on the device: sagen_png_filter turns frames into
 * PNG's filtered rows, sagen_deflate turns each frame's rows (any byte strings of one length) into one complete zlib stream.  The
 * file around it (signature, IHDR, IDAT, IEND and the chunk CRCs) is the caller's (spatialaudiogen_amd/png.py).  8 bit, colour type
 * 2 or 0, no interlace.  Integer arithmetic end to end: the CPU twin writes the same bytes.
 *
 * sagen_png_filter
 *   frames   [n][h][w][3] uint8 RGB DEVICE for components == 3, [n][h][w] grey for components == 1
 *   rows     [n][h][1 + w components] uint8 DEVICE: the filter's number, then the filtered row
 * Each row takes, of None / Sub / Up / Average / Paeth (0..4), the filter whose sum of min(v, 256 - v) over the filtered bytes is
 * smallest, the lowest number among equals; the row above row 0 is zeros.
 * Returns: n == 0 SAGEN_OK, nothing touched; SAGEN_ERR_SHAPE for n < 0, w or h < 1; SAGEN_ERR_UNSUPPORTED for components other
 * than 1 or 3, w or h above 16384, n > 65535; SAGEN_ERR_NULL for a null argument.  A refused call writes nothing.
 *
 * sagen_deflate
 *   data     [n][length] uint8 DEVICE, any alignment; may be null when length == 0
 *   out      [n][stride] uint8 DEVICE: frame f's stream - 78 01, the deflate blocks, Adler-32 of the input big-endian
 *   sizes    [n] int32 DEVICE: the bytes frame f's stream needs, filled even when that exceeds stride: then nothing beyond
 *            out[f][stride - 1] is written, the status is CAPACITY and the frame's bytes are unspecified.  Otherwise nothing
 *            beyond out[f][sizes[f] - 1] is written
 *   status   [n] int32 DEVICE: 0 or SAGEN_DEFLATE_ST_CAPACITY; a frame with a non-zero status leaves every other exact
 * The input is cut into blocks of 16384 bytes (length 0: one empty block).  Inside a block a maximal run of m equal bytes is a
 * literal followed by matches of distance 1 that cover the other m - 1 bytes in chunks of 258; a last chunk shorter than 3 is
 * literals; a block's first byte is always a literal.  Each block is the cheapest of stored / fixed / dynamic by bit count, a stored
 * block counted at its worst padding (42 bits + its bytes), ties to stored, then fixed.  A dynamic block carries a Huffman code
 * over the 286 literal / length symbols of at most 15 bits, built from the block's histogram (minimum redundancy over symbols
 * ordered by (count, symbol); lengths above 15 cut and the Kraft sum restored one code at a time), the single distance code 0 of
 * 1 bit, and sends all 287 lengths plainly through a code-length code of sixteen 4-bit codes: a header of 1222 bits.  No matches at
 * other distances: general LZ77 is out of scope.
 * sagen_deflate_max_bytes: the stride that can never be too small, length + 6 + ceil(5.25 blocks) with blocks =
 * max(1, ceil(length / 16384)) - at most length + 6 blocks + 7; 0 for a length the call would refuse.  sizes[f] never exceeds it.
 * Returns: n == 0 SAGEN_OK, nothing touched; SAGEN_ERR_SHAPE for n < 0, length < 0, stride < 4 or not a multiple of 4, out / sizes
 * / status / scratch misaligned (4, 4, 4, 16 bytes); SAGEN_ERR_UNSUPPORTED for n > 65535, length or stride above 2^28;
 * SAGEN_ERR_NULL for a null argument (data with length > 0); SAGEN_ERR_WORKSPACE for scratch smaller than
 * sagen_deflate_scratch_bytes(...), which is 0 for arguments the call would refuse.  A refused call writes nothing. */
enum {
    SAGEN_DEFLATE_ST_CAPACITY = 1 /* the stream needs more than `stride` bytes; sizes[f] holds what it needs */
};
int sagen_png_filter(const uint8_t* frames, int n, int w, int h, int components, uint8_t* rows, void* stream);
int64_t sagen_deflate_max_bytes(int64_t length);
size_t sagen_deflate_scratch_bytes(int n, int64_t length, int64_t stride);
int sagen_deflate(const uint8_t* data, int n, int64_t length, uint8_t* out, int64_t stride, int32_t* sizes, int32_t* status, void* scratch,
                  size_t scratch_bytes, void* stream);

/* ---- frame batches from a resident clip -------------------------------------------------------------------------------------
 * The reference's reader threads pick the frame of every window, roll it by the yaw rotation, un-code the flow bytes and stack the
 * batch on the host (feeder.py:106-161), and the batch crosses the bus.  sagen_assemble_frames is that step over frames that already
 * lie on the device (what sagen_jpeg_decode wrote): one launch builds the frames of n_out batch items.
 *   frames   [n_frames][h][w][3] uint8 DEVICE; may be null when n_frames == 0
 *   index    [n_out] int32 DEVICE: the frame of item i.  A value outside [0, n_frames) makes item i PADDING: every element of it is
 *            written as zero (bytes in mode 0, 0.0f otherwise) and no frame is read
 *   shift    [n_out] int32 DEVICE: output column x of item i is source column (x - shift[i]) mod w, the mathematical modulo, any
 *            int32: numpy's roll(frame, shift[i], axis=1)
 *   out      [n_out][h][w][3] DEVICE, by mode:
 *     0  uint8: the bytes
 *     1  fp32: table[byte], table [256] fp32 DEVICE (e.g. byte / 255 - 0.5 as the host computes it)
 *     2  fp32, the flow folder's un-coding (feeder.py:147-160): table [512] fp32 = cos[256] then sin[256] of the angle a byte
 *        stands for, scale_lo [n_frames][2] fp64 DEVICE = ((hi - lo) / 255, lo) of each frame's row of flow_limits.npy.  For the
 *        source bytes (b0, b1, b2) of frame f:  m = (float)((double)b2 * scale_lo[f][0]);  m = (float)((double)m + scale_lo[f][1]);
 *        out = (m * cos[b0], m * sin[b0], m), the products in fp32.  b1 is not used.
 * The kernel is a total function of its arrays - no content of index or shift moves an address out of bounds -, so there is no
 * status word, and the entry point reads no device memory.
 * Returns: n_out == 0 SAGEN_OK, nothing touched; SAGEN_ERR_SHAPE for n_out or n_frames < 0, h or w < 1, a mode outside 0..2, a float
 * out or table not 4-byte aligned, scale_lo not 8-byte aligned, index or shift not 4-byte aligned; SAGEN_ERR_UNSUPPORTED for h or w
 * above 16384; SAGEN_ERR_NULL for a null index, shift or out, null frames with n_frames > 0, a null table in modes 1 and 2, a null
 * scale_lo in mode 2 with n_frames > 0.  A refused call writes nothing. */
int sagen_assemble_frames(const uint8_t* frames, int n_frames, int h, int w, const int32_t* index, const int32_t* shift, int n_out, int mode,
                          const float* table, const double* scale_lo, void* out, void* stream);

/* ---- audio windows from a resident clip -------------------------------------------------------------------------------------
 * The reference's reader threads cut every 52799-sample window out of the 1-second wav pieces, pad it with zeros where the clip
 * ends, rotate it about the vertical axis (feeder.py:50-103), and the batch crosses the bus; train.py:107-111 then slices the
 * network's mono input and its target out of it.  sagen_assemble_audio is those steps over samples that already lie on the device,
 * as the files store them: one launch builds the windows of n_out batch items and writes up to three views of them.
 *   samples    [n_samples][channels] DEVICE, row-major, by sample_type: 0 int16, value (double)s / 32768.0; 1 fp32, widened;
 *              2 fp64 - the values feeder.load_wav returns for PCM16 and float wavs.  May be null when n_samples == 0
 *   lead, read_from, count   [n_out] int32 / int64 / int32 DEVICE, columns of feeder.window_table.  Window i has `size` rows; row j
 *              is a SOURCE ROW iff 0 <= k < count[i] with k = (int64)j - lead[i], and 0 <= read_from[i] + k < n_samples - evaluated
 *              without int64 overflow, as read_from >= -k and read_from < n_samples - k.  A source row holds source row
 *              read_from[i] + k; every channel of any other row is 0.0f
 *   rot        [n_out][2] fp64 (cos, sin) DEVICE, or null for no rotation; needs channels == 4 (W, Y, Z, X).  Per source row, in fp64,
 *              not contracted, in exactly this order:  Y' = c*Y + s*X;  X' = c*X - s*Y;  W and Z unchanged - the product with
 *              feeder.rotation_matrix_z (feeder.py:92-101).  Padding rows stay 0.  The host computes cos and sin: the device calls no
 *              trig.  (c, s) = (1, 0) is NOT null: it turns a sample of -0.0 in Y or X into +0.0
 *   outputs    every value is narrowed once, fp64 -> fp32, round to nearest.  Any of the three may be null, not all:
 *     full     [n_out][size][channels]
 *     mono     [n_out][size]: channel 0, the network's input
 *     target   [n_out][t_len][channels - 1]: the channels 1.. of the rows [t_off, t_off + t_len) of every window; needs
 *              channels >= 2, t_off >= 0, t_len >= 1 and t_off + t_len <= size (t_off and t_len are not looked at without it)
 * The kernel is a total function of its arrays - any int32 / int64 content of lead, read_from and count is legal and moves no
 * address out of bounds -, so there is no status word, and the entry point reads no device memory.
 * Returns: n_out == 0 SAGEN_OK, nothing touched, before any pointer is examined; SAGEN_ERR_SHAPE for n_out or n_samples < 0,
 * size < 1, channels < 1, a sample_type outside 0..2, a target with channels == 1 or with t_off / t_len outside the rule above, a
 * pointer not aligned to its element (samples 2 / 4 / 8 bytes by type, lead and count 4, read_from and rot 8, full, mono and target
 * 4); SAGEN_ERR_UNSUPPORTED for channels > 16, size > 1 << 24, rot with channels != 4; SAGEN_ERR_NULL for a null lead, read_from or
 * count, all three outputs null, null samples with n_samples > 0.  A refused call writes nothing. */
int sagen_assemble_audio(const void* samples, int sample_type, int64_t n_samples, int channels, const int32_t* lead, const int64_t* read_from,
                         const int32_t* count, const double* rot, int n_out, int size, int t_off, int t_len, float* full, float* mono,
                         float* target, void* stream);

/* ---- moving point sources: encode to ambisonics, binauralise, track ------------------------------------------------------
 * The front end of the reference's ambisonics toolbox: AmbiEncoder.encode / encode_frame / encode_v2 (pyutils/ambisonics/
 * encoder.py:10-55), SourceBinauralizer over VirtualStereoMic and Convolvotron, static and per frame (binauralizer.py:12-121), and
 * the positions SphericalSourceVisualizer draws (distance.py:62-97), all over MovingSource.tic (position.py:73-102).  The reference
 * walks these per audio sample in Python; here every sample is independent.  Coordinates: x front, y left, z up; polar
 * (phi, nu, r); ACN / SN3D.
 *
 * Source s: a mono signal sig_s[0 .. N) fp32 at signals + s ld (device; ld >= every nframes), P_s >= 1 control points
 * (phi_j, nu_j, r_j) fp64 in the rows pt_off[s] .. pt_off[s + 1] - 1 of ctrl [sum P][3] (device), duration[s] = N / float(rate),
 * nframes[s] = int(duration rate) (position.py:78-82; it can be N - 1).  pt_off [n_sources + 1], nframes and duration [n_sources]
 * are HOST arrays, read during the call.  n_sources <= 64 (SAGEN_ERR_UNSUPPORTED otherwise).
 *
 * Trajectory (MovingSource.tic, fp64, evaluated per sample i < nframes):
 *   P == 1: the control point.  Otherwise idx = (i == nframes - 1) ? P - 1 : floor(i ((P - 1) / (double)(nframes - 1)))
 *   (numpy's linspace followed by floor, :85); idx == P - 1: the last control point; otherwise
 *   t_j = (j == P - 1) ? duration : j (duration / (P - 1)),  alpha = (i (1 / (double)rate) - t_idx) / (t_{idx+1} - t_idx),
 *   (phi, nu, r) = alpha p_{idx+1} + (1 - alpha) p_idx                                                      (:98-100)
 *   - linear in polar coordinates with no wrap handling; alpha may be slightly negative at a segment start.
 *   Unit direction u = sgn(r) (cos phi cos nu, sin phi cos nu, sin nu), u = (1, 0, 0) when r == 0: what set_polar ->
 *   calc_cartesian -> calc_polar leaves behind (:24-37).  Cartesian position: |r| u.
 * Harmonics of u = (x, y, z), fp64 (common.py:136-157 in closed form):
 *   W 1 | Y y | Z z | X x | V sqrt(3) x y | T sqrt(3) y z | R (3 z^2 - 1) / 2 | S sqrt(3) x z | U (sqrt(3) / 2)(x^2 - y^2)
 *
 * Every operation takes the WHOLE signals plus an absolute output range [t0, t0 + n): a stream rendered in pieces is bit-identical
 * to one call.  The largest sample requested must be < min_s nframes[s] (the scripts' `while all(tic())` loop stops at the shortest
 * source), SAGEN_ERR_SHAPE otherwise.  Trajectory, direction, distance and nearest index are fp64; the sample sums are fp32 with
 * one accumulator in a fixed order: sources outermost, taps ascending.
 *
 * sagen_source_track: the direction, and optionally the nearest index in a direction set, of sample t0 + i stride, i < n.
 *   unit [n][n_sources][3] fp64 or NULL; nearest [n][n_sources] int32 or NULL (needs dirs [n_dirs][3] fp64 unit vectors, device,
 *   n_dirs <= 4096): the index with the maximum fp64 dot product with u; every candidate within 1e-12 of the maximum ties and the
 *   lowest index wins (render.py: HrirSet.closest).  Signals are not read.
 *
 * sagen_encode_sources: ambi[t][c] = sum_s g_s(t) sig_s[t - d_s(t)] Y_c(u_s(t)), ambi [n][channels], channels 4 or 9.
 *   distance_model == 0: g = 1, d = 0 (encode / encode_frame).  distance_model == 1 with radius > 0 (encode_v2, encoder.py:36-55):
 *   dist = |r| - radius, d = int(dist / 343. rate), g = 1 / (1 + dist); a sample with t - d < 0 contributes 0.  For a static source
 *   this is the reference, where scipy.ndimage.shift by an integer is an integer delay.  DEVIATION: the reference applies encode_v2
 *   to static sources only; evaluating it per sample for a moving source is this project's extension.  |r| <= radius is the
 *   caller's error (the Python layer raises ValueError); here such a sample reads sig at t - d > t, or nothing past nframes.
 *
 * sagen_binauralize_sources, y [n][2] (left, right):
 *   SAGEN_SOURCES_MIC (VirtualStereoMic.binauralize_frame, binauralizer.py:38-55): ears at (0, +-0.1, 0); per ear e
 *     dist = |pos - ear|, d = int(dist / 343. rate), y[t][e] = (1 / S) sum_s sig_s[t - d] / (1 + dist), terms with t - d < 0 dropped.
 *   SAGEN_SOURCES_HRIR (Convolvotron, :58-90): near_s(t) = the nearest index of u_s(t) in dirs [n_dirs][3] (as in
 *     sagen_source_track); y[t][e] = sum_s sum_{k < ntaps, t - k >= 0} hrir[near_s(t)][e][k] sig_s[t - k], hrir [n_dirs][2][ntaps] fp32
 *     impulse responses in time order; outputs at t < zero_before are written as 0: zero_before = ntaps - 1 gives the static
 *     binauralize (:63-76), 0 gives binauralize_frame (:78-90).  DEVIATION: the reference's frame form assigns instead of
 *     accumulating, so only its last source survives; here the sources are summed, as in its static form (one source: the same).
 *     n_dirs <= 4096, ntaps <= 512 (SAGEN_ERR_UNSUPPORTED otherwise).  dirs / hrir / n_dirs / ntaps / zero_before are ignored by the
 *     mic mode.
 * y must be 8-byte aligned, a 4-channel ambi 16-byte aligned. */
enum { SAGEN_SOURCES_MIC = 0, SAGEN_SOURCES_HRIR = 1 };
int sagen_source_track(const double* ctrl, const int32_t* pt_off, const int64_t* nframes, const double* duration, int n_sources, double rate,
                       int64_t t0, int64_t n, int64_t stride, const double* dirs, int n_dirs, double* unit, int32_t* nearest, void* stream);
int sagen_encode_sources(const float* signals, int64_t ld, const double* ctrl, const int32_t* pt_off, const int64_t* nframes,
                         const double* duration, int n_sources, double rate, int channels, int distance_model, double radius, int64_t t0,
                         int64_t n, float* ambi, void* stream);
int sagen_binauralize_sources(const float* signals, int64_t ld, const double* ctrl, const int32_t* pt_off, const int64_t* nframes,
                              const double* duration, int n_sources, double rate, int mode, const double* dirs, const float* hrir, int n_dirs,
                              int ntaps, int64_t zero_before, int64_t t0, int64_t n, float* y, void* stream);

/* ---- training step (reference train.py:137-236) -------------------------------------------------------
 * Loss of the reference: losses['stft/mse'] = metrics['stft/avg'] (model.py:156-159, 122-127; stft_for_loss myutils.py:151-178).
 * pred / target [B,4800,3]; mask [B,3] channel mask (the Y,Z,X columns of the feeder's [B,4] W,Y,Z,X mask, train.py:127) or NULL;
 * grad [B,4800,3] = dL/dpred (or NULL); loss = one fp64 (or NULL). */
int sagen_stft_loss_grad(const float* pred_yzx, const float* target_yzx, const float* mask, int batch, float* grad, double* loss,
                         void* stream);
/* tf.train.AdamOptimizer (myutils.py:214-222) on one flat fp32 bucket of n floats (n % 4 == 0, 16-byte aligned):
 * m,v slots updated in place, params -= lr_t * m / (sqrt(v) + epsilon); lr_t = lr * sqrt(1-beta2^t) / (1-beta1^t) from the host;
 * grads are multiplied by grad_scale first (1 / world_size after a sum all-reduce). */
int sagen_adam_update(float* params, const float* grads, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                      float epsilon, float grad_scale, void* stream);

/* One sess.run(train_op) without the optimiser (train.py:208; opt.minimize = compute_gradients + apply_gradients,
 * myutils.py:220-221): forward with retained activations, loss, backward.  Replaces tf.gradients over the graph of
 * model.py:356-434 for separation 'unet_mask'.
 *  - the ctx must be bound (sagen_bind_weights) to the LIVE parameter tensors: every sagen_train_step re-packs the filters from
 *    them first, so the optimiser may update them in place between steps;
 *  - sagen_train_bind: `grads` names, for every trainable variable, where its gradient is written (same name / shape / layout
 *    as the variable; e.g. views into flat gradient buckets); `moving` (optional) names writable bn/moving_mean and
 *    bn/moving_variance tensors, updated like the contrib batch_norm update ops (decay 0.99) when update_moving_averages != 0;
 *    train_workspace: >= sagen_train_workspace_bytes(ctx) bytes, 256-byte aligned, owned by the caller, used only by this ctx;
 *  - sagen_train_step: target_yzx [B,4800,3], mask [B,3] or NULL, pred_yzx [B,4800,3] or NULL (the prediction of this step),
 *    loss: device pointer to one fp64 or NULL.  Asynchronous on `stream`; gradients are complete when the stream reaches the end
 *    of the call's work.  Weight gradients are reduced in a fixed order (bit-reproducible). */
/* The training step implements ambi_order 1: sagen_train_bind refuses a context of another order (SAGEN_ERR_UNSUPPORTED). */
size_t sagen_train_workspace_bytes(sagen_ctx* ctx);
int sagen_train_bind(sagen_ctx* ctx, const sagen_tensor* grads, int n_grads, const sagen_tensor* moving, int n_moving,
                     void* train_workspace, size_t train_workspace_bytes, void* stream);
int sagen_train_step(sagen_ctx* ctx, const float* audio, const float* video, const float* flow, const float* target_yzx,
                     const float* mask, float* pred_yzx, double* loss, int update_moving_averages, void* stream);
/* The same with the video frames as the training feeder decodes them (feeder.py:222-260: uint8 [B,224,448,3], normalised
 * x / 255 - 0.5 by myutils.py:88-89 - here on the device, as in sagen_forward_u8): the stem's forward runs on the exact one-plane
 * operand u - 128 (three matrix products per multiply instead of six). */
int sagen_train_step_u8(sagen_ctx* ctx, const float* audio, const uint8_t* video_u8, const float* flow, const float* target_yzx,
                        const float* mask, float* pred_yzx, double* loss, int update_moving_averages, void* stream);
/* sagen_autotune for the training step: one step on these inputs in which every contraction (forward and data gradients) times
 * its launch candidates; the plan is stored in the ctx.  The gradients it leaves behind are not meaningful.  Synchronises. */
int sagen_train_autotune(sagen_ctx* ctx, const float* audio, const float* video, const float* flow, const float* target_yzx,
                         const float* mask, void* stream);
/* Data-parallel training (train.py runs one device; here one process per GPU, gradients summed over the ranks): overlap the
 * exchange with the backward pass.  The caller partitions the trainable variables into n_buckets flat buckets (names[i] belongs to
 * bucket[i]) and hands in one event per bucket (hipEvent_t, e.g. torch.cuda.Event.cuda_event); every following sagen_train_step
 * records events[b] as soon as the last kernel writing a gradient of bucket b has been enqueued - behind both of the step's streams -
 * so a communication stream that waits for events[b] can all-reduce bucket b under the rest of the backward.  Every event is
 * recorded by every step (buckets that never complete early are recorded at the end).  n = 0 switches it off. */
int sagen_train_set_grad_events(sagen_ctx* ctx, const char* const* names, const int32_t* bucket, int n, void* const* events, int n_buckets);
/* named buffer of the train workspace (parity tests): e.g. "t:dcoeffs" [B*3][100], "t:ddmask" [B,31,1024,ntracks] (deconv1 output
 * rows 40..70), "t:dpred", "t:g:feat" (dL/d conv5_2) */
int sagen_train_get_buffer(const sagen_ctx* ctx, const char* name, const float** data, size_t* n_floats);

/* ---- backward, op level (unit-testable) ------------------------------------------------------------------------------
 * Filter gradient of tf.nn.convolution / tf.nn.conv2d_transpose / tf.matmul (core.py:206,140,79) in one form:
 *   dw[th,tw,g,d] = sum_{b,i,j} G[b, i*sh + th + h0, j*sw + tw + w0, g] * D[b,i,j,d]      (G zero outside [hg) x [wg))
 * conv (HWIO): G = x [B,hg,wg,cg=cin], D = dy [B,hd,wd,cd=cout], h0/w0 = -pad_before; conv2d_transpose ([kh,kw,Cout,Cin]):
 * G = dy, D = x, h0 = w0 = 0; FC: hg = wg = hd = wd = kh = kw = 1, batch = rows.  cg, cd multiples of 4.  scratch (optional,
 * sagen_wgrad_scratch_bytes) enables pixel-range splitting. */
size_t sagen_wgrad_scratch_bytes(int kh, int kw, int cg, int cd);
int sagen_wgrad(const float* g, int batch, int hg, int wg, int cg, const float* d, int hd, int wd, int cd, int kh, int kw, int sh, int sw,
                int h0, int w0, float* dw, void* scratch, size_t scratch_bytes, void* stream);
/* Test accessor (host only, launches nothing): what sagen_wgrad would run for these arguments and a scratch of scratch_bytes
 * (0 = none), as "<kernel><BM,BN> fold=F splitk=S" (just "wgrad_ref_kernel fold=1 splitk=1" under SAGEN_WGRAD_REF=1).
 * buf: >= 64 bytes. */
int sagen_wgrad_kernel_name(int batch, int hg, int wg, int cg, int hd, int wd, int cd, int kh, int kw, int sh, int sw, int h0, int w0,
                            size_t scratch_bytes, char* buf, size_t buf_bytes);
/* Input gradient of tfw.conv_2d (core.py:206): dy [B,hout,wout,cout], w HWIO -> dx [B,h,w,cin].  Stride 1: any padding; strided:
 * VALID, or SAME with no padding before (every strided conv of the path).  cout a power of two >= 4. */
size_t sagen_conv2d_bwd_data_scratch_bytes(int kh, int kw, int cin, int cout, int sh, int sw);
int sagen_conv2d_bwd_data(const float* dy, int batch, int hout, int wout, int cout, const float* w_hwio, int kh, int kw, int cin,
                          int sh, int sw, int padding, int h, int w, float* dx, void* scratch, size_t scratch_bytes, void* stream);
/* contrib batch_norm (training mode) backward: dz = (ga + gb) * (act > 0) (gb, act nullable) is the gradient at the BN output;
 * bn_stats = the accumulators sagen_conv2d filled for the raw conv output y.  dy = gradient at y; dz (nullable) = the masked
 * gradient itself; dgamma / dbeta [C].  scratch: sagen_bn_bwd_scratch_bytes(c) bytes, 16-byte aligned. */
size_t sagen_bn_bwd_scratch_bytes(int c);
int sagen_bn_bwd(const float* ga, const float* gb, const float* act, const float* y, const float* bn_stats, const float* gamma,
                 const float* beta, float eps, int64_t n_pixels, int c, float* dy, float* dz, float* dgamma, float* dbeta,
                 void* scratch, size_t scratch_bytes, void* stream);
/* backward of sagen_maxpool3x3s2(relu(bn(y0))): pooled = its output, ga (+ gb) = gradient at the pooled tensor -> dz at bn(y0) */
int sagen_maxpool3x3s2_bwd(const float* y0, const float* bn_stats, const float* gamma, const float* beta, float eps, const float* pooled,
                           const float* ga, const float* gb, float* dz, int batch, int h, int w, int c, void* stream);
/* adjoint of sagen_mask_istft_mix: dpred [B,4800,3] -> d_dmask [B,28,1024,ntracks], d_coeffs [B,3,3,ntracks+1] */
size_t sagen_mask_istft_mix_bwd_scratch_bytes(int batch, int ntracks);
int sagen_mask_istft_mix_bwd(const float* dmask, const float* spec, const float* coeffs, const float* dpred, int batch, int ntracks,
                             float* d_dmask, float* d_coeffs, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAGEN_H */
