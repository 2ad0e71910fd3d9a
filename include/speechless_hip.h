/*
 * speechless_hip.h -- C-ABI of the MI355X (gfx950) implementation of the speechless Wav2Letter hot path.
 *
 * The reference (juliuskunze/speechless) exposes NO native / FFI interface for this path: every operator below
 * replaces an *implicit* third-party op that speechless/net.py reaches through Keras/TensorFlow.  Each entry
 * point cites the reference call site it stands in for (paths relative to the reference root).
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes; device pointers are raw HBM addresses (e.g. tensor.data_ptr()).
 *   - return 0 on success, a negative sl_status on error; never throw, never abort, never allocate.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no hidden synchronisation.
 *   - no global mutable state; sl_last_error() is thread-local.
 *
 * Data layout in HBM ("halo'd channels-last"): an activation tensor is [batch][rows][channels] with
 *   rows     = halo_top + padded_time + halo_bottom   (halo rows and rows >= valid time are ZERO, always)
 *   channels = channel count padded to a multiple of 128 (padded lanes are ZERO, always)
 * so a SAME-padded conv tap is a plain row-shifted view and no kernel needs bounds checks on reads.
 * padded_time must be a multiple of SL_TIME_TILE (256): the conv kernels read whole time tiles of up to 256 rows, i.e.
 * rows x_row0 .. x_row0 + ceil(t_out / 256) * 256 + taps - 2 of every utterance must lie inside its `rows`.
 */
#ifndef SPEECHLESS_HIP_H
#define SPEECHLESS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SL_VERSION 1
#define SL_TIME_TILE 256

typedef enum sl_status {
    SL_OK = 0,
    SL_ERR_INVALID_ARGUMENT = -1,
    SL_ERR_UNSUPPORTED = -2,
    SL_ERR_WORKSPACE_TOO_SMALL = -3,
    SL_ERR_LAUNCH_FAILED = -4
} sl_status;

/* SL_F16 (round 6): fp16 operands on v_mfma_f32_16x16x32_f16 with fp32 or hi + lo PLANE outputs -- sl_conv1d_nt (out_f32 = 1
 * or 2), sl_conv1d_wgrad and sl_conv1d_wgrad_multi only: the "f16x3" parity path (every fp32 value as two fp16 planes, three
 * MFMA terms per product; speechless_amd/engine_x3.py).  No reference counterpart: the reference computes in fp32. */
typedef enum sl_dtype { SL_BF16 = 0, SL_F32 = 1, SL_F16 = 2 } sl_dtype;

/* epilogue of sl_conv1d_nt */
typedef enum sl_epilogue {
    SL_EPI_NONE = 0,      /* y = acc                                  (dgrad into a linear layer)              */
    SL_EPI_BIAS = 1,      /* y = acc + bias[co]                       (output_conv logits, net.py:328-330)     */
    SL_EPI_BIAS_RELU = 2, /* y = max(acc + bias[co], 0)               (Conv1D(activation="relu"), net.py:304)  */
    SL_EPI_RELU_MASK = 3, /* y = acc * (mask[b,t,co] > 0)             (autodiff through relu, net.py:389,550)  */
    SL_EPI_BIAS_ELU = 4,  /* y = elu(acc + bias[co])                  (activation="elu", main.py:71-78)         */
    SL_EPI_ELU_MASK = 5   /* y = acc * (m > 0 ? 1 : m + 1), m = mask  (autodiff through elu via its output)      */
} sl_epilogue;

/*
 * Geometry of one stride-1 "row-shifted GEMM" convolution.  A stride-2 layer (striding_conv, net.py:317-319) is
 * presented in its PAIR VIEW: two consecutive input frames form one row of 2*Cin channels, which turns the
 * k=48/stride-2 conv into a k=24/stride-1 conv over the same memory (no padding waste, no strided loads).
 *
 *   out[b][y_row0 + t][co] = epi( sum_{tap < taps} sum_{c < cin} x[b][x_row0 + t + tap][c] * w[co][tap][c] )
 *   for t in [0, t_out), co in [0, cout)
 */
typedef struct sl_conv_geom {
    int32_t batch;          /* B                                                                        */
    int32_t t_out;          /* valid output rows per utterance (T'); rows >= t_out are never written     */
    int32_t taps;           /* taps of the (pair-)view                                                   */
    int32_t cin;            /* contraction channels per tap, multiple of 64                              */
    int32_t cout;           /* output channels, multiple of 128                                          */
    int32_t x_row0;         /* first input row read by (t = 0, tap = 0)                                  */
    int32_t x_row_stride;   /* elements between input rows (>= cin)                                      */
    int64_t x_batch_stride; /* elements between utterances in x                                          */
    int32_t y_row0;         /* output row of t = 0                                                       */
    int32_t y_row_stride;   /* elements between output rows (>= cout)                                    */
    int64_t y_batch_stride; /* elements between utterances in y (and in mask)                            */
    float acc_scale;        /* SL_F16 only: sl_conv1d_nt multiplies the accumulator by this before bias / mask (the f16x3 path
                             * stores weights and gradients scaled by powers of two); 0 = 1.  Ignored by the other dtypes. */
} sl_conv_geom;

int sl_version(void);
const char* sl_last_error(void);

/* Measurement hook (bench.py's roofline leg): the two HIP events (hipEvent_t, created with timing enabled) are attached to
 * the dispatch of the MAIN kernel of the next sl_conv1d_nt / sl_conv1d_wgrad / sl_conv1d_wgrad_grouped call
 * (hipExtLaunchKernelGGL: they carry the kernel's own begin and end timestamps) -- not to its split-K epilogue or reduction
 * tail -- and the hook disarms itself.  The duration between them is what `rocprofv3 --kernel-trace --stats` reports for
 * that kernel.  Either pointer may be NULL. */
int sl_profile_next_kernel(void* start_event, void* stop_event);

/* ---- conv forward and input-gradient (both are the same row-shifted NT GEMM) ---------------------------------
 * Replaces: Keras Conv1D forward (net.py:304-305 -> TF conv2d/bias_add/relu) and, with flipped/transposed packed
 * weights, TF Conv2DBackpropInput reached by autodiff from net.py:389,550.
 *   x      : [B][rows][x_row_stride]  dtype
 *   w      : packed weights [cout][taps][cin] dtype (see sl_pack_weights)
 *   bias   : float[cout] or NULL (SL_EPI_BIAS*)
 *   mask   : same geometry as y, dtype (SL_EPI_RELU_MASK) or NULL
 *   y      : [B][rows][y_row_stride]; dtype, or float when out_f32 = 1.  out_f32 = 2 (bf16 only; epilogues NONE, BIAS,
 *            BIAS_RELU, RELU_MASK): the result leaves the kernel as bf16x3 planes -- rows [hi | lo | hi] of 3 x cout
 *            channels (y_row_stride >= 3 cout), hi = bf16(v), lo = bf16(v - hi) of the fp32 value v after the epilogue;
 *            RELU_MASK then reads the mask's hi plane in y's geometry (what sl_split3 does in a second pass over HBM).
 *   cfg    : 0 = library picks the tile shape / pipeline depth / split-K for this geometry (measured table);
 *            otherwise (tuner / tests) wm | wn<<4 | stages<<8 | ksplit<<12 | it<<20 | m32<<24 | (1+log2 gm)<<25 |
 *            slab<<29 | interleaved<<30: wm x wn waves, each a (16*it) x 64 patch (it = 0 means 4; it = 5: the it = 4
 *            tile with eight waves, the two waves of a SIMD splitting the k-halves; m32: 32x32x16 MFMA, 64x64 patch);
 *            stages = ring slots, +8 = register-pipelined loop; gm = m-tiles per raster block; slab = chunk-major
 *            kernel with the activation slab in LDS; interleaved = hand-interleaved MFMA / LDS-read / request
 *            streams.  SL_ERR_INVALID_ARGUMENT for a shape that is not instantiated
 *            or that the geometry rules out.  SL_F32: 0 = exact-fp32 MFMA kernel (v_mfma_f32_32x32x2_f32, 128 x 128
 *            tiles), 1 = the plain VALU FMA kernel (independent cross-check of the former).
 *   workspace: sl_conv1d_nt_workspace_bytes(geom, dtype, cfg) bytes (split-K partial tiles; 0 when not split).
 */
size_t sl_conv1d_nt_workspace_bytes(const sl_conv_geom* geom, int dtype, int cfg);
int sl_conv1d_nt(const void* x, const void* w, const float* bias, const void* mask, void* y,
                 const sl_conv_geom* geom, int epilogue, int dtype, int out_f32, int cfg, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- a RUN of identical stride-1 convolutions in one launch (bf16) --------------------------------------------------
 * Replaces: the seven Conv1D(250, 7) `inner_conv_i` of net.py:321-323 -- n_layers consecutive sl_conv1d_nt calls of the
 * same geometry (256 padded channels in and out, odd taps <= 9, every tensor in the same halo'd layout) whose
 * intermediate activations stay in LDS; each layer's output is still written to HBM (ys[i]: the backward pass needs it).
 *   epilogue SL_EPI_BIAS_RELU: forward; layer i: ys[i] = relu(conv(i == 0 ? x : ys[i-1], ws[i]) + biases[i])
 *   epilogue SL_EPI_RELU_MASK: input gradients; layer i: ys[i] = conv(i == 0 ? x : ys[i-1], ws[i]) * (masks[i] > 0),
 *            ws[i] the dgrad operand (taps flipped) of the i-th convolution from the TOP of the run
 *   geom: the geometry ONE layer of the run would pass to sl_conv1d_nt.  sl_conv1d_chain_supported() = 1 when the run
 *   fits; otherwise (or for fp32 / ELU / dropout between the layers) use n_layers calls of sl_conv1d_nt.
 */
int sl_conv1d_chain_supported(const sl_conv_geom* geom, int n_layers, int dtype);
/* Measurement / test hook: output frames per work-group of sl_conv1d_chain.  0 (default) = chosen per launch (64, or 48 where
 * that fills the chip's rounds of 256 work-groups better: long utterances in small batches), 48 / 64 = forced.  Process-wide. */
int sl_conv1d_chain_select(int tile_rows);
/* Measurement / test hook: the output frames per work-group (48 or 64) that sl_conv1d_chain would choose for this geometry
 * on the calling thread right now (sl_conv1d_chain_select, sl_set_available_cus); 0 when the run does not fit the kernel.
 * Launches nothing. */
int sl_conv1d_chain_plan(const sl_conv_geom* geom, int n_layers, int dtype);
int sl_conv1d_chain(const void* x, void* const* ys, const void* const* ws, const float* const* biases,
                    const void* const* masks, const sl_conv_geom* geom, int n_layers, int epilogue, int dtype,
                    void* stream);

/* ---- conv weight gradient -------------------------------------------------------------------------------------
 * Replaces: TF Conv2DBackpropFilter reached by autodiff from net.py:389,550.
 *   dw[tap][c][co] = sum_b sum_{t < t_pad} x[b][x_row0 + t + tap][c] * g[b][g_row0 + t][co]     (fp32 out)
 * geom: batch,taps,cin,cout,x_* as above; y_* describe g (y_row0 = g_row0, ...); t_out = valid rows of g
 * (rows >= t_out of g are zero by the layout invariant, so the kernel sums whole 64-row chunks).
 * Deterministic: split-K partials go to `workspace` and are reduced in a fixed order.
 * cfg: 0 = library picks tile shape / ring depth / batch split (measured table); otherwise
 *      wm | wn<<4 | stages<<8 | splits<<12 (tile = 64*wm input channels x 64*wn output channels; splits 0 = auto).
 *      SL_F32: 0 = exact-fp32 MFMA kernel (channel counts that are multiples of 128), 1 = VALU FMA kernel.
 */
size_t sl_conv1d_wgrad_workspace_bytes(const sl_conv_geom* geom, int dtype, int cfg);
int sl_conv1d_wgrad(const void* x, const void* g, float* dw, const sl_conv_geom* geom, int dtype, int cfg,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The same weight gradient for `groups` layers of IDENTICAL geometry in one launch (bf16 only): layer q reads
 * x + q*x_group_stride and g + q*g_group_stride (elements) and writes dw + q*dw_group_stride (floats).  The seven
 * inner_conv_i (net.py:321-323) are such a group: one grid of 7 x 28 tiles needs 3 batch splits instead of 16 per
 * layer, runs 80-step contractions instead of 16-step ones and one reduction instead of seven. */
size_t sl_conv1d_wgrad_grouped_workspace_bytes(const sl_conv_geom* geom, int groups, int cfg);
int sl_conv1d_wgrad_grouped(const void* x, const void* g, float* dw, const sl_conv_geom* geom, int groups,
                            int64_t x_group_stride, int64_t g_group_stride, int64_t dw_group_stride, int cfg,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- backward of a 1x1 convolution onto <= 32 real output channels in ONE launch (bf16) -----------------------------------
 * Replaces, for output_conv (net.py:326-330: Conv1D(grapheme_set_size, 1)), the pair sl_conv1d_nt(dgrad) +
 * sl_conv1d_wgrad reached by autodiff from net.py:389,550: both gradients of that layer are HBM-bound passes over its 2000-
 * channel input, which this call reads ONCE.
 *   x       : the layer's input [B][rows][x_row_stride] bf16 -- also the stored activation whose sign (ReLU) / value (ELU)
 *             is the mask of dx
 *   g       : gradient w.r.t. the layer's output, [B][rows][y_row_stride] bf16, columns >= k_real zero
 *   w_dgrad : the layer's dgrad operand [cin][1][cout] bf16 (sl_pack_weights)
 *   dx      : gradient w.r.t. x, same geometry as x:  dx = (g . w^T) * act'(x);  frames in [t_out, ceil(t_out / 64) * 64)
 *             are written with the zeros they hold by the layout invariant
 *   dw      : float[cin][cout], complete on return (columns >= 32 zero); its row cin - 1 is the bias gradient when x carries
 *             the ones channel (sl_bias_grad_from_wgrad)
 *   geom    : the layer's WEIGHT-GRADIENT geometry (taps = 1; x_* describe x and dx, y_* describe g), cin % 128 == 0
 *   epilogue: SL_EPI_RELU_MASK or SL_EPI_ELU_MASK
 *   cfg     : 0 = library picks the number of work-groups (one per CU); otherwise (tuner / tests) that number
 *   workspace: sl_conv1d_backward_1x1_workspace_bytes() bytes (per-work-group partial sums of dw, combined in a fixed order
 *             by a small second kernel of the same call: deterministic, no float atomics). */
int sl_conv1d_backward_1x1_supported(const sl_conv_geom* geom, int k_real, int dtype);
size_t sl_conv1d_backward_1x1_workspace_bytes(const sl_conv_geom* geom, int k_real, int dtype, int cfg);
int sl_conv1d_backward_1x1(const void* x, const void* g, const void* w_dgrad, void* dx, float* dw, const sl_conv_geom* geom,
                           int epilogue, int k_real, int dtype, int cfg, void* workspace, size_t workspace_bytes,
                           void* stream);
/* The same for ONE PART of the batch (x, g, dx point at the part's first utterance, geom->batch = its utterances):
 * accumulate = 0 writes dw (the first part), accumulate = 1 adds this part's sum to what dw holds (later parts; same stream,
 * fixed order: deterministic).  The engine runs the top of the step by half-batches so that the CTC lattice of one half
 * (net.py:402-406, a handful of latency-bound waves) runs under the top layers of the other half (Engine.split_top). */
int sl_conv1d_backward_1x1_part(const void* x, const void* g, const void* w_dgrad, void* dx, float* dw,
                                const sl_conv_geom* geom, int epilogue, int k_real, int dtype, int cfg, int accumulate,
                                void* workspace, size_t workspace_bytes, void* stream);

/* How many CUs the library's grid choosers may count on: 0 = all (default 256), else 64 .. 256.  Per calling THREAD
 * (thread-local; round 6 -- it was process-wide), read when a launch is enqueued on that thread.  The MFMA kernels take a whole CU per work-group and size their grids to whole rounds of the chip; when
 * communication kernels own some CUs during backward (data-parallel runs: GradBucketReducer sets 256 - its channel count) the
 * split / segment / tile-height choosers of sl_conv1d_nt, sl_conv1d_wgrad[_grouped|_multi], sl_conv1d_chain and
 * sl_conv1d_backward_1x1 plan their rounds for that many CUs instead.  (No reference counterpart: the reference is
 * single-device, main.py:14-24.) */
int sl_set_available_cus(int cus);

/* ---- the weight gradients of SEVERAL layers in one balanced launch (bf16) ------------------------------------------------
 * Replaces a sequence of sl_conv1d_wgrad / sl_conv1d_wgrad_grouped calls (TF Conv2DBackpropFilter of several Conv1D layers,
 * net.py:389,550) for layers with few 256 x 256 tiles -- inner_conv_1..7 and striding_conv of net.py:317-323: the
 * (tile, 64-frame step) space of all jobs is cut into one equal range per CU, so no CU idles behind a batch split whose
 * granularity is an utterance; per-range partial tiles are added in a fixed order by a second kernel of the same call
 * (deterministic).  job.geom: the layer's weight-gradient geometry as for sl_conv1d_wgrad; every job needs the same
 * batch and t_out, cin % 256 == 0, cout % 256 == 0.  SL_ERR_UNSUPPORTED otherwise (use the per-layer calls). */
#define SL_WGRAD_MULTI_MAX_JOBS 16
typedef struct sl_wgrad_job {
    const void* x;     /* the layer's input  (geom.x_*) */
    const void* g;     /* the gradient w.r.t. its output (geom.y_*) */
    float* dw;         /* float[taps][cin][cout] */
    sl_conv_geom geom;
} sl_wgrad_job;
size_t sl_conv1d_wgrad_multi_workspace_bytes(const sl_wgrad_job* jobs, int n_jobs, int dtype);
int sl_conv1d_wgrad_multi(const sl_wgrad_job* jobs, int n_jobs, int dtype, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Measurement / test hook: the plan sl_conv1d_wgrad_multi would launch for these jobs on the calling thread right now
 * (sl_set_available_cus): *segs = segments per tile (2 * CUs / tiles, at most batch * ceil(t_out / 64), at least 1), *workers
 * = work-groups of the main kernel (tiles * (segs / 2), plus ceil(tiles / 2) when segs is odd).  Either pointer may be NULL;
 * the jobs' pointers are not read.  Launches nothing. */
int sl_conv1d_wgrad_multi_plan(const sl_wgrad_job* jobs, int n_jobs, int dtype, int* segs, int* workers);

/* bias gradient db[co] = sum_{b,t} g[b][g_row0+t][co] (fp32 out, deterministic two-stage).  Same autodiff site. */
size_t sl_bias_grad_workspace_bytes(const sl_conv_geom* geom);
int sl_bias_grad(const void* g, float* db, const sl_conv_geom* geom, int dtype, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- weight packing -------------------------------------------------------------------------------------------
 * master weights are fp32 in the Keras kernel layout [k][cin_pad][cout_pad] (net.py:251-255 evidence for
 * (kernel_size, in_channels, filters)).  Produces
 *   w_fwd [cout_pad][k][cin_pad]            (forward operand)      and, if w_dgrad != NULL,
 *   w_dgrad[cin_pad][k][cout_pad]  with taps flipped: w_dgrad[ci][j][co] = w[k-1-j][ci][co]
 */
int sl_pack_weights(const float* w_master, void* w_fwd, void* w_dgrad, int k, int cin_pad, int cout_pad,
                    int dtype, void* stream);

/* ---- input packing  (net.py:578-587 zero-pad + cast; rows offset by the SAME left pad) -------------------------
 * src: float[B][t_in][f] (dense, host-packed batch already resident in HBM)
 * dst: [B][dst_rows][dst_row_stride] dtype, PRE-ZEROED; frame t lands in row dst_row0 + t.
 */
int sl_pack_input(const float* src, void* dst, int batch, int t_in, int f, int dst_row0, int dst_row_stride,
                  int64_t dst_batch_stride, int dtype, void* stream);
/* Raw-wave input (net.py:310-312: `wave_conv`, Conv1D(250, kernel 250, stride 160, padding="same") over the samples in front
 * of striding_conv when use_raw_wave_input=True): the sample windows of the t_out = ceil(t_in / stride) output frames as rows of
 * k * cin columns (zero padded to dst_row_stride), pad_left = TF's SAME rule for this t_in -- over which the layer is a 1 x 1
 * GEMM for sl_conv1d_nt (forward, output straight into the pair-view input buffer of the stack) and sl_conv1d_wgrad.
 *   audio: float[B][t_in][cin];   dst: [B][rows >= t_out][dst_row_stride] dtype at dst_batch_stride elements per utterance */
int sl_wave_frames(const float* audio, void* dst, int batch, int t_in, int cin, int k, int stride, int pad_left, int t_out,
                   int dst_row_stride, int64_t dst_batch_stride, int dtype, void* stream);
/* The same with a ONES CHANNEL: padding channel `ones_channel` (f <= ones_channel < dst_row_stride) of every packed frame is set
 * to 1 (-1: none).  Its weight rows are and stay zero, so the forward pass does not see it; the first layer's weight-gradient
 * GEMM then leaves that layer's BIAS gradient in row ones_channel of dW (sl_bias_grad_from_wgrad) -- the bias gradient of
 * striding_conv (net.py:317-319) without a pass of its own over the layer's gradient tensor. */
int sl_pack_input_ones(const float* src, void* dst, int batch, int t_in, int f, int dst_row0, int dst_row_stride,
                       int64_t dst_batch_stride, int ones_channel, int dtype, void* stream);

/* ---- output softmax (net.py:131,328-330) + the Keras ctc_batch_cost prologue log(p+eps) re-normalised -----------
 * logits: float, row t of utterance b at logits + b*logit_batch_stride + t*logit_stride (first k valid).
 * probs,logq: float[B][t_out][k] dense.
 * logq = log_softmax(log(probs + eps)) = what tf.nn.ctc_loss sees after its own softmax (net.py:405-406).
 */
int sl_softmax_logq(const float* logits, float* probs, float* logq, int batch, int t_out, int k, int logit_stride,
                    int64_t logit_batch_stride, float eps, void* stream);

/* ---- output layer fused with the softmax (bf16): the 1x1 convolution onto k <= 32 classes (net.py:326-330,
 * Conv1D(grapheme_set_size, 1, activation="softmax")) and everything sl_softmax_logq computes, in one launch that
 * streams the layer's input once and never writes the logits unless asked to.
 *   x, geom (batch, t_out, taps = 1, cin, cout >= 32 rows of w, x_*): as for sl_conv1d_nt;  w: packed [cout][1][cin]
 *   probs, logq: float[B][t_out][k];  logits: optional float, row t of utterance b at b*logit_batch_stride +
 *   t*logit_stride (first k written), or NULL.   sl_output_softmax_supported() = 1 when the geometry fits the kernel
 *   (otherwise use sl_conv1d_nt + sl_softmax_logq).
 */
int sl_output_softmax_supported(const sl_conv_geom* geom, int k, int dtype);
/* Measurement / test hook: which kernel sl_output_softmax runs.  0 (default) = automatic: the weights in REGISTERS (each of
 * the four waves of a work-group owns a quarter of the input channels and its own LDS-DMA ring; cin = 256 ... 2048) where
 * that applies, else in LDS; 1 = always the LDS kernel; 2 = as 0.  Process-wide. */
int sl_output_softmax_select(int variant);
int sl_output_softmax(const void* x, const void* w, const float* bias, float* probs, float* logq, float* logits,
                      const sl_conv_geom* geom, int k, int logit_stride, int64_t logit_batch_stride, float eps, int dtype,
                      void* stream);

/* ---- CTC loss and gradient (net.py:402-406: keras.backend.ctc_batch_cost -> tf.nn.ctc_loss) --------------------
 * labels: int32[B][l_max] (padding ignored, grapheme_enconding.py:28 uses -1); blank = k-1 (grapheme_enconding.py:125).
 * loss:   float[B]  (-log p(label | x); +inf when no valid alignment exists)
 * dlogits: gradient of  grad_scale * sum_b loss[b]  w.r.t. the PRE-softmax logits of output_conv, written into the
 *          halo'd tensor described by (g_row0, g_row_stride, g_batch_stride), dtype `dtype`; frames >=
 *          input_len[b] get zeros.  grad_scale = 1/B realises Keras' mean over the batch (net.py:389).
 * workspace: sl_ctc_workspace_bytes(...) bytes (alpha/beta lattices).
 * Two lattice kernels: with labels of up to 255 graphemes and k <= 63 a probability-domain one (one wave per utterance
 * and direction, eight lattice states per lane, block floating point with one exponent per lane and 8 / 16 frames, no
 * transcendental, no LDS exchange and no barrier on the T'-long sequential path) in doubles; the gradient kernel then
 * checks every frame's posteriors against 1, and an utterance that lost mass to underflow is redone in the log domain --
 * in doubles since round 6: as accurate as the lattice it replaces -- by the last work-group of the same launch (no further
 * launches; none of the regimes of a training run -- near-uniform start, blank collapse, a net that has learnt its labels
 * -- needs it; alignments with next to no slack, labels filling > 90 % of the frames, can).  Labels beyond 255 graphemes, and
 * k = 64 at any label length, go through the log-domain lattice in doubles of csrc/ctc_long.hip (two or four lattice states per
 * thread, LDS edge exchange + barrier per frame).  Both meet the same bounds against a float64 lattice: loss 1e-5 relative,
 * every gradient entry within 1e-4 * grad_scale.
 *
 * Limits: batch, t_out > 0, 2 <= k <= 64, 1 <= l_max <= 2047 (4095 lattice states).  l_max > 2047 is SL_ERR_UNSUPPORTED with a
 * message that names l_max and 2047, before anything is launched; a null pointer is SL_ERR_INVALID_ARGUMENT, a workspace below
 * sl_ctc_workspace_bytes() SL_ERR_WORKSPACE_TOO_SMALL.  The cap is 2047 and not the aligners' 8191 because (a) the loss keeps TWO
 * full lattices per utterance, alpha and beta, in doubles beyond 255 letters: 64 KiB per frame at 4095 states (8 utterances of
 * 4000 frames: 2.1 GB), and (b) the gradient kernel's LDS -- labels, class lists and one occupancy row per wave, 6 * l_max + 321
 * words -- is 50.4 KB at 2047, inside the default 64 KB limit.
 * A batch goes wholly to the kernels its l_max (the width of the label batch) and k select:
 *     l_max        lattice kernel                                   rows                  gradient kernel
 *     1 .. 255     ctc_lattice_helped_kernel (sl_ctc_select: 0)     linear, hi words      ctc_grad_kernel<8, 1> (+ repair)
 *     256 .. 1023  ctc_long_lattice_kernel<2>, 2 states per thread  log2, doubles         ctc_long_grad_kernel
 *     1024 .. 2047 ctc_long_lattice_kernel<4>, 4 states per thread  log2, doubles         ctc_long_grad_kernel
 * (k = 64, which the wave lattice does not take, sends l_max <= 255 to the second row as well.)  With l_max <= 255 and k <= 63
 * nothing differs from what it was: same launches, same bytes.  The kernels of csrc/ctc_long.hip keep the lattice values in
 * doubles and take only each step's log2 of a sum in [1, 3] in fp32; loss and gradient meet the bounds of the wave lattice
 * against the float64 oracle (CTC section).  Until this rule, 256 .. 511 letters and k = 64 ran ctc_lattice_kernel
 * (one state per thread, rows in fp32 log2 units) with ctc_grad_kernel<4|8|16, 0>: up to 3e-3 absolute from the float64 gradient
 * on labels with little slack.  sl_ctc_select(1) still runs it, for every l_max <= 511 (measurement and tests); no other variant
 * changes what runs beyond the wave lattice, and none applies beyond 511 letters.
 * sl_ctc_workspace_bytes: with sp = (2 * l_max + 1 rounded up to 64) it is 2 * batch * t_out * sp * 8 bytes of log-domain rows
 * + batch * (l_max + 65) * 4 of class lists + (l_max <= 255: the wave lattice's rows, exponents and dump rows) + per-utterance
 * words and done slots + (l_max >= 256: 4 KiB per utterance where the lanes of ctc_long.hip beyond a row's end store; up to 255
 * the wave lattice's dump rows serve, so these sizes are what they always were), every part rounded up to
 * 256 bytes; monotonic in batch, t_out and l_max over 0 .. 2047 (a workspace sized for l_max serves every narrower batch), 0 for
 * non-positive sizes and beyond 2047; 64-bit throughout.
 */
size_t sl_ctc_workspace_bytes(int batch, int t_out, int l_max);
int sl_ctc_loss_grad(const float* probs, const float* logq, const int32_t* labels, const int32_t* label_len,
                     const int32_t* input_len, float* loss, void* dlogits, int batch, int t_out, int k, int l_max,
                     int g_row0, int g_row_stride, int64_t g_batch_stride, int dtype, float eps, float grad_scale,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Measurement / test hook: which lattice sl_ctc_loss_grad runs.  0 (default) = as described above, 1 = log-domain lattice
 * only; probability-domain lattice in doubles: 2 = without the repair pass, 3 = and then EVERY utterance redone by the
 * repair pass, 4 = + repair; in floats (faster, but the repair pass is needed in some regimes: ctc.hip:WaveReal): 6 / 7 / 5
 * likewise; 10 / 11 (round 6) = the lone double lattice wave with a HELPER wave beside it that fetches the probabilities and gathers
 * every lattice lane's emissions into 48 contiguous bytes of LDS per frame (three wide LDS reads per frame instead of five, no
 * staging work in the lattice wave) with / without the repair pass.  8 / 9 (the lattice on a pair of waves) are retired: they,
 * and every value not named here, are refused with SL_ERR_INVALID_ARGUMENT and leave the setting as it was.  Process-wide; not for concurrent use with sl_ctc_loss_grad.
 * Label batches wider than 511 are not affected by it; of what the wave lattice does not take below that (256 .. 511 letters,
 * k = 64) only variant 1 changes the kernels: the fp32 log-domain lattice instead of the doubles of csrc/ctc_long.hip. */
int sl_ctc_select(int variant);

/* ---- greedy decode (net.py:452-454 tf.nn.ctc_greedy_decoder, merge_repeated=True; numpy twin
 *      grapheme_enconding.py:34-57): per-frame argmax (first max wins) for t < input_len, merge repeats, drop blank.
 * out: int32[B][t_out] filled with -1 past out_len[b] (sparse_to_dense default, net.py:436). frame_argmax: optional
 * int32[B][t_out] raw per-frame argmax (for parity attribution), or NULL.
 */
int sl_greedy_decode(const float* probs, const int32_t* input_len, int32_t* out, int32_t* out_len,
                     int32_t* frame_argmax, int batch, int t_out, int k, int blank, void* stream);

/* ---- CTC forced alignment (Viterbi over the CTC lattice).  No reference counterpart: the reference's data model consumes
 *      word timings (speechless/labeled_example.py:32-60 PositionalLabel, :219-234 sections()); this produces them. -------
 * logq: float[B][t_out][k] (sl_softmax_logq / sl_output_softmax); labels, label_len: as for sl_ctc_loss_grad (label_len
 * clamped to [0, l_max]); input_len: T_b, clamped to [0, t_out].  blank = k-1.  Limits: 1 < k <= 64, 0 <= l_max <= 511,
 * SL_ERR_UNSUPPORTED otherwise.  Every operation is an exact max or ONE fp32 add (no multiply, nothing to contract), so a
 * float32 restatement of the following reproduces score and path bit for bit:
 *   states s in [0, S), S = 2L+1: even s blank, odd s label position (s-1)/2.
 *   delta_0(0) = logq_0(blank), delta_0(1) = logq_0(l_0), every other state -inf;
 *   delta_t(s) = max(delta_{t-1}(s), delta_{t-1}(s-1), delta_{t-1}(s-2)) + logq_t(label(s)) for 0 < t < T_b, where the s-2
 *   term counts only for an odd s >= 3 whose label differs from l_{(s-1)/2 - 1}.  Ties: strict > in the order stay, s-1,
 *   s-2 (the earlier candidate wins).  End state: S-2 if delta(S-2) > delta(S-1), else S-1.
 * Outputs: score[b] = the best path's log-probability (delta of the end state at T_b - 1); path int32[B][t_out]: path[b][t]
 * = the state the best path occupies at frame t for t < T_b, -1 for t >= T_b.  No feasible path (T_b < L + number of
 * adjacent equal labels): score -inf, the whole row -1.  L = 0 aligns every frame to blank; T_b = 0 with L = 0: score 0.
 * workspace: sl_ctc_align_workspace_bytes(batch, t_out, l_max) bytes, 0 when the backpointers (2 bits per state and frame)
 * fit the work-group's LDS -- otherwise they go to HBM (monotonic in t_out and l_max).  One wave per utterance. */
size_t sl_ctc_align_workspace_bytes(int batch, int t_out, int l_max);
int sl_ctc_align(const float* logq, const int32_t* labels, const int32_t* label_len, const int32_t* input_len,
                 int32_t* path, float* score, int batch, int t_out, int k, int l_max, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- CTC forced alignment of long recordings: sl_ctc_align beyond 511 letters.  Arguments, their order and every rule
 *      (states, recursion, strict-> tie order stay / s-1 / s-2, end state, infeasible rows, L = 0, T_b = 0, the clamping of
 *      label_len, input_len and label values) are those of sl_ctc_align above; score and path are bit for bit what it
 *      returns where both accept the shape.  Limits: 1 < k <= 64, 0 <= l_max <= 8191 (16 383 lattice states: one work-group
 *      of 1 / 2 / 4 / 8 / 16 waves per recording for l_max <= 511 / 1023 / 2047 / 4095 / 8191, 16 states per lane),
 *      SL_ERR_UNSUPPORTED otherwise; t_out is limited by the workspace only.  A null pointer is SL_ERR_INVALID_ARGUMENT, a
 *      workspace below the size asked for SL_ERR_WORKSPACE_TOO_SMALL; all of these are refused on the host before any launch.
 * workspace: sl_ctc_align_long_workspace_bytes(batch, t_out, l_max) bytes = batch * t_out * 256 * waves: the backpointers (2 bits
 * per state and frame) always go to HBM.  Monotonic in t_out and l_max, 0 for arguments out of range. */
size_t sl_ctc_align_long_workspace_bytes(int batch, int t_out, int l_max);
int sl_ctc_align_long(const float* logq, const int32_t* labels, const int32_t* label_len, const int32_t* input_len,
                      int32_t* path, float* score, int batch, int t_out, int k, int l_max, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- CTC segment posteriors: the probability that a stretch of frames, read on its own, says exactly a stretch of a label
 *      (the forward SUM over the CTC lattice where the aligners above take the max).  With the word ranges of a forced
 *      alignment: a confidence per word; over all frames and the whole label: minus the CTC loss.  No reference counterpart. ---
 * logq: float[B][t_out][k], as the aligners take it; labels: int32[B][l_max]; input_len: T_b; blank = k-1.
 * segments: int32[n_segments][5] = {b, frame_begin, frame_end, label_begin, label_end}, half-open ranges into utterance b.
 * Limits: 1 < k <= 64, 0 <= seg_l_max <= 511, n_segments >= 1: SL_ERR_UNSUPPORTED otherwise.  A null pointer (labels may be
 * null when l_max = 0) or batch, t_out <= 0 or l_max < 0 is SL_ERR_INVALID_ARGUMENT, a workspace below the size asked for
 * SL_ERR_WORKSPACE_TOO_SMALL; all of these are refused on the host before any launch.
 * Per segment: frame_begin and frame_end are each clamped into [0, min(max(T_b, 0), t_out)], T = frame_end - frame_begin (0 if
 * that is negative); label_begin and label_end are each clamped into [0, l_max], L = min(label_end - label_begin, seg_l_max)
 * (0 if negative); the segment's letters are l_i = labels[b][label_begin + i], i < L, its frames logq_t = logq[b][frame_begin
 * + t], t < T.  A letter's column is clamped into [0, k) as the aligners clamp it.
 *   states s in [0, S), S = 2L+1: even s blank, odd s letter (s-1)/2.
 *   a_0(0) = logq_0(blank), a_0(1) = logq_0(l_0), every other state -inf;
 *   a_t(s) = logsumexp(a_{t-1}(s), a_{t-1}(s-1), a_{t-1}(s-2)) + logq_t(label(s)) for 0 < t < T, where the s-2 term counts only
 *   for an odd s >= 3 whose letter differs from l_{(s-1)/2 - 1} (sl_ctc_align's rule).
 *   log_posterior[i] = logsumexp(a_{T-1}(2L), a_{T-1}(2L-1)), float32, natural logarithm.
 * L = 0: the sum of logq_t(blank) over the frames; L = 0 and T = 0: 0.  T < L + (number of adjacent equal letters of the
 * segment): -inf.  b outside [0, batch): -inf, and nothing else of the segment is read.  Only log_posterior[0 .. n_segments) is
 * written.  Not bit-exact: the lattice is held in doubles in log2 units and each step's log2 of a sum in [1, 3] is taken in
 * fp32; against a float64 evaluation of the above the result is within 1e-6 * (T + |log_posterior|).
 * workspace: sl_ctc_segment_scores_workspace_bytes(n_segments, seg_l_max) bytes -- 0 today: a segment's lattice lives in the
 * registers of its wave (workspace may then be null).  One wave per segment; 2 / 4 / 8 / 16 states per lane for seg_l_max <=
 * 63 / 127 / 255 / 511. */
size_t sl_ctc_segment_scores_workspace_bytes(int n_segments, int seg_l_max);
int sl_ctc_segment_scores(const float* logq, const int32_t* labels, const int32_t* input_len, const int32_t* segments,
                          float* log_posterior, int batch, int t_out, int k, int l_max, int n_segments, int seg_l_max,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC phrase search (keyword / phrase spotting): where in an utterance a phrase is said, and how well.  One launch searches
 *      any number of queries, each a phrase of up to 511 letters in one utterance of the batch: a Viterbi search over the
 *      phrase's CTC states in which every frame may open a new occurrence at no cost.  A begin-frame tag travels with every
 *      score, so there are no backpointers and no backtrace.  No reference counterpart. ---
 * logq: float[B][t_out][k] and input_len: as the aligners take them; blank = k-1; T_b = input_len[b] clamped into [0, t_out].
 * queries: int32[n_queries][q_max], query_len[n_queries], query_utt[n_queries] (the utterance b a query is searched in); L =
 * query_len clamped into [0, q_max].  A letter's emission column is clamped into [0, k) as the aligners clamp it; the skip rule
 * compares the letters as given.  min_score: float[n_queries].
 * Limits: 1 < k <= 64, 1 <= q_max <= 511, 1 <= max_hits <= 64, n_queries >= 1: SL_ERR_UNSUPPORTED otherwise.  A null pointer
 * (frame_score and frame_begin may be null) or batch, t_out <= 0 is SL_ERR_INVALID_ARGUMENT, a workspace below the size asked
 * for SL_ERR_WORKSPACE_TOO_SMALL; all of these are refused on the host before any launch, in this order.
 * Every operation is an exact compare or ONE fp32 add (no multiply, nothing to contract), so a float32 restatement of the
 * following reproduces every output bit for bit:
 *   states s in [0, 2L-1): even s letter s/2, odd s the blank between two letters.  No leading and no trailing blank: a span
 *   starts and ends on a letter frame.
 *   Before frame 0 every state is -inf.  A filler below state 0 has score 0 at every frame.
 *   delta_t(s) = max(candidates) + logq_t(col(s)) for 0 <= t < T_b; the candidates, in order: stay delta_{t-1}(s);
 *   delta_{t-1}(s-1), which for s = 0 is the filler's 0; delta_{t-1}(s-2), only for an even s >= 2 whose letter differs from
 *   the letter before it.  A later candidate replaces an earlier one only by strict >, so ties go to the earlier.
 *   beg_t(s) = the tag of the winning candidate; entering from the filler sets it to t; a state at -inf has tag -1.
 * Per-frame outputs (optional): frame_score[q][t] = delta_t(2L-2), frame_begin[q][t] = beg_t(2L-2): the best occurrence that
 * ends at frame t covers the frames [frame_begin, t].  For t >= T_b, for L = 0 and for query_utt outside [0, B): -inf / -1.
 * Hit picking, on the device in the same launch; repeat up to max_hits times: among the frames not yet suppressed with
 * frame_score > -inf and frame_score >= min_score[q] take the largest score, on equal scores the smallest t; emit hit =
 * {frame_begin[t], t+1} (half-open) with that score; suppress every frame u whose span [frame_begin[u], u] intersects
 * [frame_begin[t], t].  Outputs: hits int32[n_queries][max_hits][2], hit_score float[n_queries][max_hits], n_hits
 * int32[n_queries]; unused slots hold -1 / -inf.  Hits never overlap and their scores never increase.  NaN in logq is outside
 * the contract.
 * workspace: sl_ctc_spot_workspace_bytes(n_queries, t_out, q_max) bytes = n_queries * t_out * 8 (every query's per-frame score and
 * begin, which the picking reads whether frame_score / frame_begin are given or not): monotonic, 0 for arguments out of range;
 * t_out is limited by memory only.  One wave per query; 2 / 4 / 8 / 16 states per lane for q_max <= 63 / 127 / 255 / 511. */
size_t sl_ctc_spot_workspace_bytes(int n_queries, int t_out, int q_max);
int sl_ctc_spot(const float* logq, const int32_t* input_len, const int32_t* queries, const int32_t* query_len,
                const int32_t* query_utt, const float* min_score, int32_t* hits, float* hit_score, int32_t* n_hits,
                float* frame_score, int32_t* frame_begin, int batch, int t_out, int k, int n_queries, int q_max, int max_hits,
                void* workspace, size_t workspace_bytes, void* stream);

/* ---- ASG criterion (auto segmentation criterion of the wav2letter paper, arXiv:1609.03193).  No reference counterpart:
 *      the reference raises NotImplementedError where its ASG loss would be (speechless/net.py:397-399). ----------------------
 * K = k letters and NO blank.  trans: float[k][k], trans[i*k + j] = g(i, j) = the score of moving from letter i to letter
 * j; init: float[k], g0.  labels, label_len, input_len: as for the CTC loss (L = label_len clamped to [0, l_max], T_b =
 * input_len clamped to [0, t_out], label values clamped to [0, k)).  Emissions e_t(j) = log(probs_t(j) + eps).
 *   numerator    a_0(0) = g0(l_0) + e_0(l_0), a_0(s > 0) = -inf;
 *                a_t(s) = e_t(l_s) + LSE(a_{t-1}(s) + g(l_s, l_s), a_{t-1}(s-1) + g(l_{s-1}, l_s));   N = a_{T_b-1}(L-1)
 *   denominator  d_0(j) = g0(j) + e_0(j);   d_t(j) = e_t(j) + LSE_i(d_{t-1}(i) + g(i, j));   Z = LSE_j d_{T_b-1}(j)
 *   loss[b] = Z - N, >= 0 for a label without equal neighbours (what AsgGraphemeEncoding produces).  Adjacent equal labels
 *   need no special rule, but there N counts one letter sequence once per way of cutting the joint run, and may exceed Z.
 * Gradients of grad_scale * sum_b loss[b], with G_t(j) = (denominator posterior - numerator posterior) of letter j at frame
 * t, xi the posteriors of a pair of letters at frames t-1, t, p = probs and r = p / (p + eps):
 *   dlogits_t(j) = grad_scale * (G_t(j) r_t(j) - p_t(j) sum_i G_t(i) r_t(i)), w.r.t. the PRE-softmax logits, written like
 *                  the CTC gradient (g_row0, g_row_stride, g_batch_stride, dtype; zeros for t >= T_b; may be NULL)
 *   dtrans[i][j] = grad_scale * sum_b sum_{1 <= t < T_b} (xi_den_t(i, j) - xi_num_t(i, j));  dinit[j] = grad_scale * sum_b G_0(j)
 * dtrans / dinit (both or neither NULL) are OVERWRITTEN and bitwise reproducible: per-utterance partial sums, reduced over
 * b = 0 .. B-1 in that order, no float atomics.  An utterance with L = 0, T_b = 0 or L > T_b is infeasible: loss +inf, its
 * rows of dlogits zero, nothing added to dtrans / dinit.  logq is not read (log(p + eps) is taken from probs in doubles; logq
 * differs from it by a per-frame constant, which cancels in Z - N) and may be NULL.
 * Limits: 2 <= k <= 64, 0 <= l_max <= 511, SL_ERR_UNSUPPORTED otherwise (nothing is written).
 * workspace: sl_asg_workspace_bytes(batch, t_out, k, l_max) bytes (the four lattices in doubles; 0 = unsupported shape). */
size_t sl_asg_workspace_bytes(int batch, int t_out, int k, int l_max);
int sl_asg_loss_grad(const float* probs, const float* logq, const float* trans, const float* init, const int32_t* labels,
                     const int32_t* label_len, const int32_t* input_len, float* loss, void* dlogits, float* dtrans,
                     float* dinit, int batch, int t_out, int k, int l_max, int g_row0, int g_row_stride,
                     int64_t g_batch_stride, int dtype, float eps, float grad_scale, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---- ASG Viterbi decode over the full graph: the best letter per frame under emissions + transition scores.
 * logq: float[B][t_out][k], the emissions e_t(j) used AS THEY ARE (sl_softmax_logq's logq: log(p + eps) re-normalised per
 * frame -- the path is that of log(p + eps), the score differs by the per-frame constants).  fp32:
 *   v_0(j) = g0(j) + e_0(j);   v_t(j) = (max_i (v_{t-1}(i) + g(i, j))) + e_t(j), strict > in ascending i (the lowest index
 *   wins a tie); end state = the first maximal j.  Every operation is a max or ONE fp32 add in the order written, so a
 *   float32 restatement reproduces path and score bit for bit.
 * path: int32[B][t_out], the letter of the best path per frame, -1 for t >= T_b; score: float[B].  T_b = 0: row -1, score
 * -inf.  Limits: 2 <= k <= 64.  workspace: sl_asg_viterbi_workspace_bytes(batch, t_out, k), 0 when the backpointers (t_out *
 * k bytes) fit the work-group's LDS.  One wave per utterance. */
size_t sl_asg_viterbi_workspace_bytes(int batch, int t_out, int k);
int sl_asg_viterbi(const float* logq, const float* trans, const float* init, const int32_t* input_len, int32_t* path,
                   float* score, int batch, int t_out, int k, void* workspace, size_t workspace_bytes, void* stream);

/* ---- ASG forced alignment: the best segmentation of a label over the frames (Viterbi over the label's own states; the ASG
 *      counterpart of sl_ctc_align -- no blank, transition and start scores, the run-length-encoded label).
 * logq: float[B][t_out][k], the emissions e_t(j) used AS THEY ARE (as sl_asg_viterbi).  trans[i*k + j] = g(i, j), init[j] =
 * g0(j).  labels, label_len, input_len: as for sl_asg_loss_grad (L = label_len clamped to [0, l_max], T_b = input_len clamped
 * to [0, t_out], label values clamped to [0, k)); adjacent equal labels need no special rule.  fp32, states s in [0, L),
 * state s = letter l_s:
 *   delta_0(0) = g0(l_0) + e_0(l_0);   delta_0(s > 0) = -inf
 *   stay = delta_{t-1}(s) + g(l_s, l_s);   move = delta_{t-1}(s-1) + g(l_{s-1}, l_s)  (s >= 1)
 *   delta_t(s) = (move > stay ? move : stay) + e_t(l_s)   for 0 < t < T_b   (a tie keeps stay)
 * Every operation is an exact max or ONE fp32 add in the order written (no multiply, nothing to contract or reassociate), so
 * a float32 restatement reproduces path and score bit for bit.  -inf entries of trans / init are legal and propagate as -inf;
 * finite-or--inf inputs never give a NaN.
 * End state: L-1 at frame T_b-1.  score[b] = delta_{T_b-1}(L-1); path int32[B][t_out]: path[b][t] = the state occupied at
 * frame t for t < T_b (found by backtracking the recorded decisions), -1 for t >= T_b.  An utterance with L = 0, T_b = 0,
 * L > T_b or a score of -inf is infeasible: score -inf and the whole row -1 (where sl_asg_loss_grad gives +inf).
 * Limits: 2 <= k <= 64, 1 <= l_max <= 511, SL_ERR_UNSUPPORTED otherwise (nothing is written).
 * workspace: sl_asg_align_workspace_bytes(batch, t_out, l_max) bytes, 0 when the backpointers (ONE bit per state and frame)
 * fit the work-group's LDS -- otherwise they go to HBM (monotonic in t_out and l_max).  One wave per utterance; all work on
 * the caller's stream, no allocation, no synchronisation. */
size_t sl_asg_align_workspace_bytes(int batch, int t_out, int l_max);
int sl_asg_align(const float* logq, const float* trans, const float* init, const int32_t* labels, const int32_t* label_len,
                 const int32_t* input_len, int32_t* path, float* score, int batch, int t_out, int k, int l_max, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- ASG segment posteriors: the probability that a stretch of frames says exactly a stretch of an encoded label under the
 *      ASG criterion (the ASG counterpart of sl_ctc_segment_scores).  ASG is globally normalised: over a stretch of frames the
 *      constrained forward score minus the full-graph forward score is the log of a proper probability, with no approximation;
 *      over the whole label and all frames it is exactly minus the loss of sl_asg_loss_grad.  No reference counterpart. ---
 * logq, trans, init, labels, input_len: exactly as sl_asg_align takes them -- emissions e_t(j) = logq[b][t][j] used AS THEY
 * ARE, trans[i*k + j] = g(i, j), init[j] = g0(j), label values clamped to [0, k); labels are encoded graphemes, there is no blank.
 * segments: int32[n_segments][5] = {b, frame_begin, frame_end, label_begin, label_end}, half-open ranges into utterance b, clamped
 * exactly as sl_ctc_segment_scores clamps them: frame_begin and frame_end each into [0, min(max(T_b, 0), t_out)], T = frame_end -
 * frame_begin (0 if negative); label_begin and label_end each into [0, l_max], L = min(label_end - label_begin, seg_l_max) (0 if
 * negative); l_i = clamp(labels[b][label_begin + i]), i < L; e_t = logq[b][frame_begin + t], t < T.
 * Start scores: s(j) = g0(j) if the clamped label_begin is 0, else s(j) = g(p, j) with p = clamp(labels[b][label_begin - 1]), the
 * grapheme just before the segment: a word in mid-utterance is scored given that the frame before it lay on the grapheme the
 * label puts before it, and the whole label is scored as the loss scores it.
 *   numerator    a_0(0) = s(l_0) + e_0(l_0),  a_0(i > 0) = -inf
 *                a_t(i) = e_t(l_i) + LSE(a_{t-1}(i) + g(l_i, l_i),  a_{t-1}(i-1) + g(l_{i-1}, l_i));      N = a_{T-1}(L-1)
 *   denominator  d_0(j) = s(j) + e_0(j);   d_t(j) = e_t(j) + LSE_i(d_{t-1}(i) + g(i, j));                Z = LSE_j d_{T-1}(j)
 *   log_posterior[i] = N - Z, float32, natural logarithm.
 * Adjacent equal graphemes need no special rule (as in sl_asg_loss_grad).  A per-frame constant added to a logq row cancels in
 * N - Z, so logq may be sl_softmax_logq's output or log(p + eps), at any magnitude.
 * L = 0 and T = 0: 0.  L = 0 and T > 0: -inf (without a blank no path says nothing).  T < L: -inf.  N = -inf through -inf entries
 * of trans / init: -inf; Z = -inf (then N = -inf too): -inf.  Inputs that are finite or -inf never give a NaN.  b outside
 * [0, batch): -inf, and nothing else of the segment is read.  Only log_posterior[0 .. n_segments) is written.
 * Limits: 2 <= k <= 64, 0 <= seg_l_max <= 511, n_segments >= 1: SL_ERR_UNSUPPORTED otherwise.  A null pointer (labels may be
 * null when l_max = 0) or batch, t_out <= 0 or l_max < 0 is SL_ERR_INVALID_ARGUMENT, a workspace below the size asked for
 * SL_ERR_WORKSPACE_TOO_SMALL; all of these are refused on the host before any launch, in sl_ctc_segment_scores' order.  The score
 * tables may be as large as sl_asg_loss_grad's denominator supports (exp(g) is held in doubles); the project tests +-30.
 * Not bit-exact: the numerator is held in doubles in log2 units with each step's log2 of a sum in [1, 2] taken in fp32, the
 * denominator in doubles in the probability domain, rescaled every frame; against a float64 evaluation of the above over the
 * same float32 inputs the result is within 1e-6 * (T + |log_posterior|), and -inf matches exactly.
 * workspace: sl_asg_segment_scores_workspace_bytes(n_segments, seg_l_max, k) bytes -- 0 today: a segment's lattices live in the
 * registers and LDS of its work-group (workspace may then be null).  One work-group of two waves per segment (numerator beside
 * denominator); 1 / 2 / 4 / 8 label states per lane for seg_l_max <= 64 / 128 / 256 / 511. */
size_t sl_asg_segment_scores_workspace_bytes(int n_segments, int seg_l_max, int k);
int sl_asg_segment_scores(const float* logq, const float* trans, const float* init, const int32_t* labels,
                          const int32_t* input_len, const int32_t* segments, float* log_posterior, int batch, int t_out, int k,
                          int l_max, int n_segments, int seg_l_max, void* workspace, size_t workspace_bytes, void* stream);

/* ---- ASG forced alignment of long recordings: sl_asg_align beyond 511 graphemes.  Arguments, their order and every rule
 *      (states, stay / move, the strict-> compare with a tie that stays, three separately rounded fp32 adds and no multiply,
 *      end state L-1 at T_b-1, infeasible rows -- L = 0, T_b = 0, L > T_b or a score of -inf: score -inf and the whole row -1 --,
 *      -1 past T_b, the clamping of label_len, input_len and label values, -inf entries of trans / init that never give a
 *      NaN) are those of sl_asg_align above; score and path are bit for bit what it returns where both accept the shape, and
 *      bit for bit the float32 restatement everywhere.
 * Limits: 2 <= k <= 64, 1 <= l_max <= 8191, SL_ERR_UNSUPPORTED otherwise; t_out is limited by the workspace only.  A null
 * pointer (the workspace included) is SL_ERR_INVALID_ARGUMENT, a workspace below the size asked for
 * SL_ERR_WORKSPACE_TOO_SMALL; all of these are refused on the host before any launch, and nothing is written.
 * One work-group per recording, 8 states per lane = 512 per wave, the waves chosen from l_max:
 *      l_max   1..512   513..1024   1025..2048   2049..4096   4097..8191
 *      waves      1         2            4            8           16
 * workspace: sl_asg_align_long_workspace_bytes(batch, t_out, l_max) bytes = batch * t_out * 64 * waves: the backpointers (ONE
 * bit per state and frame; state s at bit (s >> 3) & 63 of 64-bit word (s >> 9) * 8 + (s & 7) of its frame's row) always go to
 * HBM.  Monotonic in t_out and l_max, 0 for arguments out of range.  All work on the caller's stream, no allocation, no
 * synchronisation. */
size_t sl_asg_align_long_workspace_bytes(int batch, int t_out, int l_max);
int sl_asg_align_long(const float* logq, const float* trans, const float* init, const int32_t* labels,
                      const int32_t* label_len, const int32_t* input_len, int32_t* path, float* score, int batch, int t_out,
                      int k, int l_max, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC beam search, optionally scored by an n-gram language model: the device twin of sl_host_ctc_beam_search
 *      (include/speechless_host.h; speechless/net.py:444-451).  The host decoder is the specification: for the same
 *      inputs the result is the same search, step for step --
 *   frame: logf(p + eps), minus max + logf(sum over j = 0..k-1 in that order of expf(x_j - max));
 *   branches = the beam stable-sorted by total, descending; first loop from the parents' old probabilities with the
 *   `previous` rule of merge_repeated; child loop over branches in that order with is_candidate / push, a full beam
 *   evicting the FIRST minimum in slot order, the new entry taking its slot; an equal total never displaces the bottom;
 *   prefixes are trie nodes with a canonical id per (parent, label), so a prefix that leaves the beam and comes back is
 *   the same node; at the end expand_state_end + end_expansion_score, then LabelSeq(merge_repeated) of the first best
 *   leaf in slot order.
 * probs: float[batch][t_max][k] probabilities (device); lengths: int32[batch] (device), clamped to [0, t_max] (0 = the
 * empty result).  out: int32[batch][t_max], -1 behind out_len[batch] labels; log_prob: float[batch] or NULL.
 * lm: NULL = plain search; otherwise device pointers to the tables that sl_host_scorer_export of speechless_host.h
 * fills, and the scalars it returns.  With lm, blank must be k - 1.
 * Numerics: logf / expf / log1pf are evaluated in double and rounded to float (glibc's float functions are within an
 * ulp or so of that), everything else is the host's float arithmetic without contraction: transcripts agree with the
 * host decoder, log_prob to about 1e-6 relative (tests require 1e-4 * max(1, |log_prob|)); not bit-identical.
 * Limits: 2 <= k <= 64 (one lane per class), 1 <= beam_width <= 128, 1 <= lm->order <= 6, t_max * beam_width < 2^25;
 * SL_ERR_UNSUPPORTED otherwise.  workspace: sl_ctc_beam_search_workspace_bytes(batch, t_max, k, beam_width) bytes
 * (node arena + hash map per utterance, cleared by the call).  One wave per utterance; out_len[b] = -1 flags an arena
 * overflow, which the workspace bound rules out. */
typedef struct {
    const int32_t* trie_child;  /* [n_trie_nodes][k - 1] */
    const float* trie_min;      /* [n_trie_nodes][k - 1] */
    const int32_t* trie_word;   /* [n_trie_nodes] */
    const uint32_t* ngrams;     /* [ngram_slots][8] */
    int64_t n_trie_nodes;
    int64_t ngram_slots;        /* power of two */
    int order;
    int bos, eos, space_label;  /* space_label -1: no word boundary in the alphabet */
    float oov_score, lm_weight, word_count_weight, valid_word_count_weight;
} sl_beam_lm;
size_t sl_ctc_beam_search_workspace_bytes(int batch, int t_max, int k, int beam_width);
int sl_ctc_beam_search(const float* probs, const int32_t* lengths, int batch, int t_max, int k, int blank, int beam_width,
                       int merge_repeated, float eps, const sl_beam_lm* lm, int32_t* out, int32_t* out_len,
                       float* log_prob, void* workspace, size_t workspace_bytes, void* stream);

/* ---- ASG beam search, optionally scored by an n-gram language model: the max (Viterbi) search over prefixes under emissions
 *      + transition scores + scorer terms.  No reference or host counterpart; this text is the definition, and a float32
 *      restatement (tests/asg_beam_ref.py) reproduces transcripts and scores bit for bit.
 * Inputs.  logq: float[B][t_out][k], used AS IT IS (as sl_asg_viterbi); trans[i*k + j] = g(i, j), init[j] = g0(j); input_len
 * clamped to [0, t_out] = T_b.  k = characters + 2: asg_twice = k-2, asg_thrice = k-1.  1 <= beam_width W <= 128, 2 <= k <= 64.
 * lm: NULL (plain search) or the sl_beam_lm tables of sl_host_scorer_export built for the k-2 CHARACTERS (trie tables of k-2
 * columns, space_label in [-1, k-2), order <= 6).
 * Hypotheses.  A hypothesis is a prefix: a grapheme sequence with no two adjacent graphemes equal, with a float32 score a and
 * a scorer state.  The beam is an ordered list of at most W hypotheses.  A candidate is a pair (i, j): the position of its
 * source in the current beam and a grapheme.  Candidate order: score descending, then i ascending, then j ascending (a total
 * order: no two candidates share a key).
 * Arithmetic.  float32; each line below is ONE rounded operation in the order written, no contraction; -inf entries of
 * trans / init are legal.
 * Scorer terms.  The characters grapheme j writes behind last grapheme l: j itself if j < k-2; nothing if j is a mark and l
 * is absent or a mark; l once (asg_twice) or l twice (asg_thrice) otherwise (AsgGraphemeEncoding.decode_grapheme; a mark
 * behind the space writes spaces, each scoring an empty word as <unk> like any other).  For each written character in turn:
 *   state = expand(state, c);   a = lw * state.delta + a     (one multiply, then one add)
 * expand / expand_end are the CTC decoder's scorer in the arithmetic and operation order of csrc/beam_shared.h.  lm == NULL: no
 * scorer terms.  A grapheme that writes nothing leaves state and score alone.
 * Frame 0, every j:   a = g0(j) + e_0(j);   the scorer terms of j from the initial state;   source position 0.
 * Frame t > 0, every hypothesis i (last grapheme l, score s) and every j:
 *   a = s + g(l, j);   a = a + e_t(j);   j == l: i's own prefix, state unchanged (a stay);   otherwise the child prefix with
 *   the scorer terms of j behind l.
 * Merge.  Two candidates can name the same prefix -- at most two: the stay of (p, l) and the extension of p by l.  The one
 * that comes first in candidate order survives with its own key; the other is dropped.
 * Prune.  Candidates of score -inf are dropped; the first W in candidate order, in that order, are the next beam.  Prefix
 * identity is the sequence itself: a prefix that leaves the beam and is created again later is the same prefix (a canonical
 * node id per (parent, label), as in sl_ctc_beam_search).
 * End.  After frame T_b - 1: total_i = lw * expand_end(state_i).delta + a_i with lm, a_i without.  The result is the first
 * maximal total in beam order (strict >).  out: int32[B][t_out], the prefix's graphemes then -1; out_len: int32[B]; score:
 * float[B] or NULL.  T_b = 0 or an empty beam: out_len 0, score -inf.
 * Status codes and argument checks as sl_ctc_beam_search; t_out * beam_width < 2^25.  workspace:
 * sl_asg_beam_search_workspace_bytes(batch, t_out, k, beam_width) bytes (0 = unsupported shape; node arena + hash map per
 * utterance, cleared by the call); out_len[b] = -1 flags an arena overflow, which the workspace bound rules out.  One
 * work-group per utterance; all work on the caller's stream, no allocation, no synchronisation. */
size_t sl_asg_beam_search_workspace_bytes(int batch, int t_out, int k, int beam_width);
int sl_asg_beam_search(const float* logq, const float* trans, const float* init, const int32_t* input_len, int batch, int t_out,
                       int k, int beam_width, const sl_beam_lm* lm, int32_t* out, int32_t* out_len, float* score,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- letter and word error counts: the two editdistance.eval calls of the reference's result object (speechless/net.py:
 *      31-37, over the characters and over the .split() of expected / predicted), on index rows that are in HBM already. ----
 * a: int32[batch] rows a_stride apart, the expected indices (the labels of sl_ctc_loss_grad); b: likewise b_stride apart,
 * the predicted indices (`out` of sl_greedy_decode); a_len, b_len: int32[batch].  Entries at or past a row's length are
 * never read, whatever they hold.
 *   letter_errors[i] = Levenshtein distance (unit costs) between a[i][:a_len[i]] and b[i][:b_len[i]];
 *   word_errors[i]   = the same between their word sequences.  A word is a maximal run of indices != space -- str.split() for
 *     an alphabet whose only whitespace character sits at index `space`: leading, trailing and repeated separators yield no
 *     empty words.  Two words are equal iff they have the same length and the same indices (compared index by index: exact).
 *     space < 0: no separator, every non-empty row is one word;
 *   a_word_count[i]  = number of words of a[i] (the denominator of the word error rate); may be NULL.
 * Integers only; any index values (the symbols are only compared, so the grapheme set size does not enter).
 * Errors.  What the host can see is refused before anything is launched: SL_ERR_INVALID_ARGUMENT for batch <= 0, a negative
 * maximum, a null pointer, or a maximum above its row stride (a length up to it would leave the row).  The lengths themselves
 * are in HBM and the call does not synchronise: a row whose a_len / b_len lies outside [0, a_max] / [0, b_max] reads nothing
 * and reports -1 in all three outputs of that row -- a code per utterance, no fault; the other rows are unaffected.
 * Limits: a_max <= 1024 (64 lanes x 16 columns of the DP row in registers), and both rows with their word spans in 64 KiB of
 * LDS, 8 (a_max + b_max) + 16 bytes at most. The engine's shapes (labels <= 200, predictions <= T' = 500..4000) are far
 * inside; anything larger is REJECTED with SL_ERR_UNSUPPORTED, and sl_edit_distance_supported(a_max, b_max) tells in advance
 * (1 / 0) -- the Python layer counts such a batch on the host.  No workspace.  One work-group of two waves per utterance: the
 * letter pass and the word pass run side by side. */
int sl_edit_distance_supported(int a_max, int b_max);
int sl_edit_distance(const int32_t* a, const int32_t* a_len, int a_stride, const int32_t* b, const int32_t* b_len,
                     int b_stride, int batch, int a_max, int b_max, int space, int32_t* letter_errors,
                     int32_t* word_errors, int32_t* a_word_count, void* stream);

/* The same fused update for SEVERAL layers in one launch (the small layers' launches are pure latency): layer i's
 * block starts `offset` floats into param / grad / m / v (weights [k][cin_pad][cout_pad] followed by cout_pad biases). */
#define SL_ADAM_MAX_LAYERS 16
typedef struct {
    int64_t offset;  /* first weight of the layer, in floats from the four base pointers (multiple of 4) */
    void* w_fwd;     /* [cout_pad][k][cin_pad] dtype */
    void* w_dgrad;   /* [cin_pad][k][cout_pad] dtype, taps flipped; NULL for a layer without input gradient */
    int32_t k, cin_pad, cout_pad;
} sl_adam_layer;
int sl_adam_pack_layers(float* param, const float* grad, float* m, float* v, const sl_adam_layer* layers, int n_layers,
                        int dtype, int step, float lr, float beta1, float beta2, float eps, void* stream);
/* The operand rewrite alone (sl_pack_weights for several layers in one launch, same table): used when the masters were
 * updated elsewhere -- the data-parallel step with a sharded optimizer runs sl_adam_step on this rank's slice of the flat
 * buffers and all-gathers the masters (speechless_amd/parallel.py; the reference has no counterpart, main.py:14-24). */
int sl_pack_layers(const float* param, const sl_adam_layer* layers, int n_layers, int dtype, void* stream);

/* ---- Bias gradients out of the weight-gradient GEMM ("ones channel") ------------------------------------------------
 * The channel padding of an activation tensor (250 -> 256, 2000 -> 2048) is multiplied through every GEMM anyway.  When the
 * LAST padded output channel of layer i-1 carries the constant 1 on every valid frame (bias 1, zero weights; the host side
 * sets that up), row cin_pad - 1 of layer i's weight gradient is  dW[k][cin_pad-1][co] = sum over the frames whose tap-k
 * input frame is valid of g[frame][co]  -- for the tap that reads the frame itself (k = pad_left) exactly the bias gradient
 * of layer i (BiasAddGrad, net.py:389 autodiff), computed by sl_conv1d_wgrad at no extra cost instead of by sl_bias_grad's
 * extra pass over g.  This call moves it to the bias-gradient slot and zeroes the row for all taps, so that the padded
 * weights stay zero under the optimizer.  grads: the flat fp32 gradient buffer; per layer the element offsets of dW
 * ([k][cin_pad][cout_pad]) and db ([cout_pad]); copy = 0: zero the row only (e.g. dropout was applied to the ones).
 */
#define SL_BGW_MAX_LAYERS 16
typedef struct sl_bgw_layer {
    int64_t w_off, b_off;
    int32_t k, cin_pad, cout_pad, tap;
} sl_bgw_layer;
int sl_bias_grad_from_wgrad(float* grads, const sl_bgw_layer* layers, int n_layers, int copy, void* stream);

/* ---- Dropout (net.py:301-303: a Keras Dropout(rate) layer in front of every conv except the last three; training
 * phase only, `dropout=None` in every reference configuration) ------------------------------------------------------
 * sl_dropout: dst[i] = keep_i ? src[i] / (1 - rate) : 0 over n elements (dst may be src), keep_i a pure function of
 * (seed, i) -> a step is reproducible from its seed.  Zero halo / padding elements stay zero, so it can run over a
 * whole halo'd tensor.  Because the activation is stored AFTER dropout, the ReLU-mask epilogue of the next dgrad
 * (mask = stored value > 0) applies the keep mask for free; sl_scale supplies the remaining 1 / (1 - rate) factor of
 * the backward pass (x[i] *= scale).
 */
int sl_dropout(const void* src, void* dst, size_t n, int dtype, float rate, uint64_t seed, void* stream);
int sl_scale(void* x, size_t n, int dtype, float scale, void* stream);
/* Dropout behind an ELU layer (activation="elu", main.py:71-78, with dropout=...): a stored zero cannot tell a dropped
 * element from elu(z) == 0, so the input gradient is produced with SL_EPI_NONE and this pass applies both factors:
 *   g[i] = keep_i ? g[i] / (1 - rate) * (y[i] > 0 ? 1 : y[i] * (1 - rate) + 1) : 0
 * with y the stored post-dropout activation and keep_i recomputed from (seed, i) exactly as sl_dropout drew it. */
int sl_elu_dropout_backward(void* g, const void* y, size_t n, int dtype, float rate, uint64_t seed, void* stream);

/* ---- Keras-2.0 Adam (net.py:132): lr_t = lr*sqrt(1-b2^t)/(1-b1^t); p -= lr_t*m/(sqrt(v)+eps) ------------------- */
int sl_adam_step(float* param, const float* grad, float* m, float* v, size_t n, int step, float lr, float beta1,
                 float beta2, float eps, void* stream);

/* Same Adam update for ONE layer block laid out [k][cin_pad][cout_pad] weights followed by cout_pad biases (param,
 * grad, m, v point at the block's first weight), fused with sl_pack_weights: the pass that updates the fp32 masters
 * also rewrites w_fwd [cout_pad][k][cin_pad] and (if non-NULL) w_dgrad [cin_pad][k][cout_pad] (taps flipped). */
int sl_adam_pack_layer(float* param, const float* grad, float* m, float* v, void* w_fwd, void* w_dgrad, int k,
                       int cin_pad, int cout_pad, int dtype, int step, float lr, float beta1, float beta2, float eps,
                       void* stream);

/* ---- Gradient clipping on the device (Keras 2.0.x optimizers.py, Optimizer.get_gradients: every Keras optimizer takes
 * clipnorm / clipvalue; restated from knowledge of Keras 2.0 like the Adam row above -- not checkable offline) ------------
 *   n = sqrt(sum over the TRAINABLE tensors of sum(g * g));   g = g * clipnorm / n if n >= clipnorm else g
 *   then g = clip(g, -clipvalue, +clipvalue)
 * The optimisation step never waits for the host, so n is reduced on the device and the Adam kernels read the factor from
 * device memory.  A NaN / Inf norm gets no special handling: the comparison is false and g passes through, as in Keras.
 *
 * Squared norm: *sqnorm = sum over the ranges [offset, offset + count) of grad (floats; any alignment of the ranges, grad
 * itself 16-byte aligned) of g * g, accumulated in double.  The order of the additions is fixed by the ranges alone (a
 * partial per 16384-float chunk, then the partials in index order; no floating-point atomics), so the same data gives the same
 * bits on every call, whatever sl_set_available_cus says.  norm / scale (each may be NULL): sl_clip_scale's outputs for this
 * one term, written by the same final launch. */
#define SL_NORM_MAX_RANGES 16
typedef struct {
    int64_t offset; /* first float of the range in grad */
    int64_t count;  /* floats (0 allowed) */
} sl_norm_range;
size_t sl_grad_sqnorm_workspace_bytes(const sl_norm_range* ranges, int n_ranges);
int sl_grad_sqnorm(const float* grad, const sl_norm_range* ranges, int n_ranges, float clipnorm, double* sqnorm, float* norm,
                   float* scale, void* workspace, size_t workspace_bytes, void* stream);
/* n = sqrt(sqnorm[0] + ... + sqnorm[n_terms - 1]) (one term per range table, or the all-reduced sum of the ranks' terms);
 * *norm = (float)n;  *scale = n >= clipnorm ? (float)(clipnorm / n) : exactly 1.0f  (clipnorm <= 0: 1.0f). */
int sl_clip_scale(const double* sqnorm, int n_terms, float clipnorm, float* scale, float* norm, void* stream);

/* Clipped twins of the four Adam entry points: the update sees clip(g * *grad_scale, -clipvalue, +clipvalue) in place of g
 * (grad_scale: device pointer, NULL = 1; clipvalue 0 = off).  grad itself is not rewritten; the operand-repack half is the
 * original's.  With NULL and 0 a twin IS its original (same kernel, same bits). */
int sl_adam_step_clipped(float* param, const float* grad, float* m, float* v, size_t n, int step, float lr, float beta1,
                         float beta2, float eps, const float* grad_scale, float clipvalue, void* stream);
int sl_adam_pack_layers_clipped(float* param, const float* grad, float* m, float* v, const sl_adam_layer* layers, int n_layers,
                                int dtype, int step, float lr, float beta1, float beta2, float eps, const float* grad_scale,
                                float clipvalue, void* stream);
int sl_split3_adam_pack_layers_clipped(float* param, const float* grad, float* m, float* v, const sl_adam_layer* layers,
                                       int n_layers, int step, float lr, float beta1, float beta2, float eps,
                                       const float* grad_scale, float clipvalue, void* stream);
int sl_splitf16_adam_pack_layers_clipped(float* param, const float* grad, float* m, float* v, const sl_adam_layer* layers,
                                         int n_layers, int step, float lr, float beta1, float beta2, float eps, float w_scale,
                                         const float* grad_scale, float clipvalue, void* stream);

/* ---- Keras-2.0 optimizers beside Adam (optimizers.py of Keras 2.0.x; restated, like the Adam row -- not checkable offline) --
 * g: the gradient after clipping (as in the clipped Adam twins); lr: the DECAYED rate lr0 / (1 + decay * it), computed by the
 * caller; state slots start at zero.
 *   SGD       v = momentum * m - lr * g;  m' = v;  p' = p + v            (nesterov: p' = p + momentum * v - lr * g)   1 slot
 *   RMSprop   a' = rho * a + (1 - rho) * g^2;  p' = p - lr * g / (sqrt(a') + eps)                                     1 slot
 *   Adagrad   a' = a + g^2;                    p' = p - lr * g / (sqrt(a') + eps)                                     1 slot
 *   Adadelta  a' = rho * a + (1 - rho) * g^2;  u = g * sqrt(d + eps) / sqrt(a' + eps);  p' = p - lr * u;
 *             d' = rho * d + (1 - rho) * u^2                                                                          2 slots (a, d)
 *   Adamax    m' = b1 * m + (1 - b1) * g;  u' = max(b2 * u, |g|);  p' = p - lr * m' / (u' + eps), where lr is ALREADY
 *             lr_decayed / (1 - b1^t), divided by the caller in double                                                2 slots (m, u)
 * s0 / s1 are the slots in the order named above.  A one-slot rule takes s1 == NULL and the kernels neither read nor write a
 * second buffer (3 fp32 reads + 2 writes per parameter instead of Adam's 4 + 3); a two-slot rule requires s1.
 * grad_scale (device float*, NULL = 1) and clipvalue (0 = off) as in the clipped Adam twins: with NULL and 0 the instantiation
 * without clipping is launched.  The flat and the fused kernels apply ONE definition of each rule: the same bits.
 * SL_OPT_ADAM names Adam's place in the kernels' rule table; Adam keeps its own entry points above (they take the step
 * count) and these reject it. */
#define SL_OPT_ADAM 0
#define SL_OPT_SGD 1
#define SL_OPT_RMSPROP 2
#define SL_OPT_ADAGRAD 3
#define SL_OPT_ADADELTA 4
#define SL_OPT_ADAMAX 5
typedef struct {
    int32_t rule;     /* SL_OPT_* */
    float lr;         /* decayed; Adamax: and divided by 1 - beta1^t */
    float momentum;   /* SGD */
    int32_t nesterov; /* SGD: 0 / 1 */
    float rho;        /* RMSprop, Adadelta */
    float beta1, beta2; /* Adamax */
    float eps;        /* all but SGD */
} sl_opt_rule;
/* sl_adam_step_clipped / sl_adam_pack_layers_clipped / sl_split3_... / sl_splitf16_... for these rules (n a multiple of 4;
 * 1 .. SL_ADAM_MAX_LAYERS layers, the table and the operand formats of the Adam versions) */
int sl_optimizer_step(float* param, const float* grad, float* s0, float* s1, size_t n, const sl_opt_rule* rule,
                      const float* grad_scale, float clipvalue, void* stream);
int sl_optimizer_pack_layers(float* param, const float* grad, float* s0, float* s1, const sl_adam_layer* layers, int n_layers,
                             int dtype, const sl_opt_rule* rule, const float* grad_scale, float clipvalue, void* stream);
int sl_split3_optimizer_pack_layers(float* param, const float* grad, float* s0, float* s1, const sl_adam_layer* layers,
                                    int n_layers, const sl_opt_rule* rule, const float* grad_scale, float clipvalue,
                                    void* stream);
int sl_splitf16_optimizer_pack_layers(float* param, const float* grad, float* s0, float* s1, const sl_adam_layer* layers,
                                      int n_layers, const sl_opt_rule* rule, float w_scale, const float* grad_scale,
                                      float clipvalue, void* stream);

/* ---- "bf16x3": the fast parity path ---------------------------------------------------------------------------------------
 * north_star: greedy-decoded indices bit-exact against the reference's fp32 CPU path (net.py:417-436 on Keras / TF float32),
 * gradients within 1e-3.  Every fp32 value is carried as two bf16 numbers (hi = bf16(v), lo = bf16(v - hi)) in THREE planes
 * per tensor row, [hi | lo | hi] (3 x channels), against packed weight rows [w_hi | w_hi | w_lo]: the unchanged
 * sl_conv1d_nt over 3 x channels then computes x_hi w_hi + x_lo w_hi + x_hi w_lo in fp32 (out_f32 = 1 into a staging buffer, or out_f32 = 2 straight into planes),
 * and these HBM-bound helpers move between the fp32 staging form and the planes.  See csrc/split3.hip.
 *   sl_split3            fp32 [B][src rows][channels] (valid rows t < t_out) -> planes [B][rows][3 * channels] at row
 *                        dst_row0 + t.  mode 0: copy; 1: relu; 2: elu (Conv1D activations, net.py:304); 3 / 4: multiply by the
 *                        ReLU / ELU derivative taken from `mask`, the stored activation in plane form (autodiff, net.py:389)
 *   sl_split3_pack_input float[B][t_in][f] -> planes, channels >= f zero (net.py:578-587)
 *   sl_split3_weights    v -> (float(hi), v - float(hi)): sl_pack_weights of the two arrays yields the hi and lo operands
 *   sl_split3_assemble   rows of `width` bf16: dst[r] = [a[r] | a[r] | b[r]]
 *   sl_split3_wgrad_combine  RA = sl_conv1d_wgrad of (x planes [hi | lo ...], g_hi), RB = of (x planes [hi ...], g_lo), float
 *                        [taps / frames][r*_cin][c_out] -> dw[tap][ci][co] = hh + hl + lh;  frames = 2, fstride = 3 * c_in for
 *                        the pair view of a stride-2 layer (two frames' planes per row); rb_fstride = the frame stride inside
 *                        RB's rows (= fstride, or c_in when RB's x operand was the [hi of frame 0 | hi of frame 1] window
 *                        in the middle of the pair row)
 *   sl_split3_bias_grad  db[co] = sum over valid frames of g_hi + g_lo (two stages, fixed order; workspace from
 *                        sl_split3_bias_grad_workspace_bytes) */
int sl_split3(const float* src, void* dst, const void* mask, int batch, int t_out, int channels, int64_t src_batch_stride,
              int dst_row0, int64_t dst_batch_stride, int mode, void* stream);
int sl_split3_pack_input(const float* src, void* dst, int batch, int t_in, int f, int channels, int dst_row0,
                         int64_t dst_batch_stride, void* stream);
int sl_split3_weights(const float* v, float* hi, float* lo, size_t n, void* stream);
int sl_split3_assemble(const void* a, const void* b, void* dst, int64_t rows, int width, void* stream);
/* The bf16x3 operand copies of one layer from its fp32 master [k][cin_pad][cout_pad] in one pass: w_fwd3 [cout][k][3 cin]
 * = rows [w_hi | w_hi | w_lo], w_dgrad3 [cin][k-1-tap][3 cout] likewise (or NULL); what sl_split3_weights + 2 x
 * sl_pack_weights + 2 x sl_split3_assemble produce, bit for bit. */
int sl_split3_pack_weights(const float* w_master, void* w_fwd3, void* w_dgrad3, int k, int cin_pad, int cout_pad,
                           void* stream);
/* sl_adam_pack_layers for the bf16x3 path: Keras-2.0 Adam on the fp32 masters of up to SL_ADAM_MAX_LAYERS layers and their
 * [w_hi | w_hi | w_lo] operand copies (layers[i].w_fwd / .w_dgrad = the 3-plane tensors) rewritten in the same pass. */
int sl_split3_adam_pack_layers(float* param, const float* grad, float* m, float* v, const sl_adam_layer* layers, int n_layers,
                               int step, float lr, float beta1, float beta2, float eps, void* stream);
int sl_split3_wgrad_combine(const float* ra, const float* rb, float* dw, int taps, int c_in, int c_out, int frames,
                            int fstride, int ra_cin, int rb_cin, int rb_fstride, void* stream);
size_t sl_split3_bias_grad_workspace_bytes(int channels);
int sl_split3_bias_grad(const void* g, float* db, int batch, int t_out, int channels, int g_row0, int64_t g_batch_stride,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Dropout on a plane tensor of `rows` rows of [hi | lo | hi] over `channels` channels (Keras Dropout, net.py:301-303, on the
 * bf16x3 path).  The keep decision of (row r, channel c) is the one sl_dropout draws for element r * channels + c of the
 * single-plane tensor of the same logical shape, so a seed means the same masks on every path; values are re-split after the
 * arithmetic.  mode 0: dst = keep ? v / (1 - rate) : 0 (forward);  mode 1: dst = v / (1 - rate) (what is left of
 * d dropout / dx behind a ReLU, cf. sl_scale);  mode 2: dst = keep ? v / (1 - rate) * elu'(z) : 0 with y the stored
 * post-dropout activation (cf. sl_elu_dropout_backward).  dst may be src. */
int sl_split3_dropout(const void* src, void* dst, const void* y, int64_t rows, int channels, int mode, float rate,
                      uint64_t seed, void* stream);

/* ---- "f16x3" (round 6): the same three-plane scheme on fp16 pairs -- hi = fp16(v), lo = fp16(v - hi): 22 significand bits
 * where |v| >= 2^-3 and an absolute 2^-25 below (the lo plane runs into fp16 denormals, which v_mfma_f32_16x16x32_f16 keeps:
 * tools/f16_denorm_probe.hip) against bf16x3's 16-17, at the same three MFMA terms and the same rate; range 65504, so the engine
 * stores weights and back-propagated gradients multiplied by powers of two (exact) and the kernels divide them out again:
 * sl_conv1d_nt(dtype = SL_F16) through sl_conv_geom.acc_scale, the helpers below through `scale`.  Same reference rows as
 * bf16x3 (net.py:304, 389, 402-406: one fp32 arithmetic).  Twins of the sl_split3* entry points above, fp16 planes:
 *   sl_splitf16, sl_splitf16_pack_input, sl_splitf16_dropout    as sl_split3, sl_split3_pack_input, sl_split3_dropout
 *   sl_splitf16_pack_weights   operand copies of scale * w
 *   sl_splitf16_adam_pack_layers  Adam on the masters, operand copies of w_scale * w
 *   sl_splitf16_bias_grad      db = scale * sum over valid frames of (g_hi + g_lo)
 *   sl_split3_wgrad_combine_scaled  dw = scale * (hh + hl + lh)   (fp32 in and out: either plane format) */
int sl_splitf16(const float* src, void* dst, const void* mask, int batch, int t_out, int channels, int64_t src_batch_stride,
                int dst_row0, int64_t dst_batch_stride, int mode, void* stream);
int sl_splitf16_pack_input(const float* src, void* dst, int batch, int t_in, int f, int channels, int dst_row0,
                           int64_t dst_batch_stride, void* stream);
int sl_splitf16_pack_weights(const float* w_master, void* w_fwd3, void* w_dgrad3, int k, int cin_pad, int cout_pad, float scale,
                             void* stream);
int sl_splitf16_adam_pack_layers(float* param, const float* grad, float* m, float* v, const sl_adam_layer* layers, int n_layers,
                                 int step, float lr, float beta1, float beta2, float eps, float w_scale, void* stream);
int sl_split3_wgrad_combine_scaled(const float* ra, const float* rb, float* dw, int taps, int c_in, int c_out, int frames,
                                   int fstride, int ra_cin, int rb_cin, int rb_fstride, float scale, void* stream);
int sl_splitf16_bias_grad(const void* g, float* db, int batch, int t_out, int channels, int g_row0, int64_t g_batch_stride,
                          float scale, void* workspace, size_t workspace_bytes, void* stream);
int sl_splitf16_dropout(const void* src, void* dst, const void* y, int64_t rows, int channels, int mode, float rate,
                        uint64_t seed, void* stream);
/* Raw-wave input on the plane paths (net.py:310-312: `wave_conv`): sl_wave_frames(SL_F32) on scale * audio followed by
 * sl_splitf16 / sl_split3 mode 0, in ONE launch that never writes the fp32 windows (1.5 KiB per row of 256 columns instead of
 * 1 KiB written, 1 KiB read and 1.5 KiB written) -- bit for bit the planes of those two.  Row t < t_out of utterance b receives
 * [hi | lo | hi] over `channels` columns each of v = scale * audio[b][t * stride + j - pad_left][c] at column j * cin + c
 * (0 outside [0, t_in) and in the columns >= k * cin), hi = cvt(v), lo = cvt(v - float(hi)), round to nearest even; rows
 * >= t_out are not written.  fp16 planes carry 22 bits only where |v| >= 2^-3 and audio sits in [-1, 1] with quiet passages
 * far below: `scale` (a finite positive power of two: exact) lifts the samples, and whatever contracts the windows divides it
 * out again (sl_conv_geom.acc_scale, sl_split3_wgrad_combine_scaled).
 *   audio: float[B][t_in][cin];   dst: [B][rows >= t_out][3 * channels] at dst_batch_stride elements per utterance (a multiple
 *   of 8);   channels: a multiple of 8, >= k * cin;   dtype: SL_F16 or SL_BF16 (the plane format) */
int sl_wave_frames_planes(const float* audio, void* dst, int batch, int t_in, int cin, int k, int stride, int pad_left,
                          int t_out, int channels, int64_t dst_batch_stride, float scale, int dtype, void* stream);

/* ---- audio front end (speechless/labeled_example.py:99-160, 28-29) ---------------------------
 * sl_stft_power_db: librosa.stft(y, n_fft, hop_length) with its defaults (periodic Hann window of n_fft samples,
 * center=True with reflect padding of n_fft/2, 1 + len/hop frames, 1 + n_fft/2 bins; labeled_example.py:99-100), then
 * |D|^2 (:93-97) and the power level 10 log10(.) with `min_db` for zero power and as the floor (:150-158), in one pass.
 *   audio   : float, all utterances back to back; utterance b starts at audio + offsets[b] and has lengths[b] samples
 *             (lengths[b] > n_fft / 2: reflect padding)
 *   out     : float[B][max_frames][row_stride] at batch_stride; row t of utterance b holds its 1 + n_fft/2 levels followed
 *             by zeros up to row_stride; rows t >= 1 + lengths[b] / hop are zero.  Time-major, so that the mel projection
 *             (labeled_example.py:106-109: a matrix applied to the LEVEL spectrogram) is a 1 x 1 sl_conv1d_nt over it.
 * n_fft: power of two in [64, 1024].
 */
int sl_stft_power_db(const float* audio, const int64_t* offsets, const int32_t* lengths, float* out, int batch,
                     int max_frames, int n_fft, int hop, int row_stride, int64_t batch_stride, float min_db,
                     void* stream);

/* sl_stft: the same transform (input layout, frame rule, window, n_fft range, rows and zero padding of sl_stft_power_db) with a
 * choice of what a row holds -- the spectrogram types of labeled_example.py:17-25, 120-134 and the complex STFT itself (:99-100):
 *      SL_STFT_POWER        |D|^2
 *      SL_STFT_AMPLITUDE    |D|
 *      SL_STFT_COMPLEX      D, interleaved: bin k of a row is the two floats at 2k (re) and 2k + 1 (im); row_stride >= 2 * bins
 *      SL_STFT_POWER_LEVEL  what sl_stft_power_db writes, bit for bit (the same kernel)
 * min_db is read in the power-level mode only.  Columns behind the bins (behind 2 * bins for complex rows) and rows
 * t >= 1 + lengths[b] / hop are zero in every mode.  Digital silence gives exact zeros in the first three.  With a the float64
 * amplitude and delta_t = 16 log2(n_fft) 2^-24 sum_n |x_t[n]| (w[n] + 2^-23) over the frame (DESIGN.md sections 3.8, 3.9):
 * each of re and im within delta_t, |amplitude - a| <= delta_t + 1e-5 a, |power - a^2| <= 2 a delta_t + delta_t^2 + 1e-5 a^2.
 * Errors: SL_ERR_INVALID_ARGUMENT for a null pointer, a mode not listed, n_fft outside the range or rows too short. */
#define SL_STFT_POWER 0
#define SL_STFT_AMPLITUDE 1
#define SL_STFT_COMPLEX 2
#define SL_STFT_POWER_LEVEL 3
int sl_stft(const float* audio, const int64_t* offsets, const int32_t* lengths, float* out, int batch, int max_frames,
            int n_fft, int hop, int row_stride, int64_t batch_stride, int mode, float min_db, void* stream);

/* sl_istft: complex rows in the layout SL_STFT_COMPLEX writes -> audio, as librosa.istft(D, hop_length, win_length=n_fft) with
 * its defaults (labeled_example.py:162-164), in the form that normalises by the summed squared window:
 *      frame t = real inverse transform of its 1 + n_fft/2 bins (the imaginary parts of the DC and Nyquist bins are ignored,
 *                as numpy.fft.irfft does), times the periodic Hann window, added at sample t * hop of a buffer of
 *                n_fft + hop (frames[b] - 1) samples;
 *      the buffer is divided by the sum of the squared windows wherever that sum exceeds the smallest normal float and left as
 *      it is elsewhere; n_fft / 2 samples are cut off both ends.
 * This normalisation is taken from knowledge of librosa; the 2017 librosa the reference ran on cannot be imported where this
 * library is built and tested, so the choice is NOT verified against it.
 *   spec        : float[B][max_frames][row_stride] at batch_stride, row_stride >= 2 * bins; utterance b has frames[b] >= 1 rows
 *                 (frames: int32 in HBM; capped at max_frames); rows >= frames[b] and columns >= 2 * bins are never read
 *   audio       : utterance b's hop * (frames[b] - 1) samples go to audio + out_offsets[b]; nothing else is written.  A single
 *                 frame yields no samples, and that is legal.
 * One work-group per (utterance, tile of sl_istft_tile_frames(n_fft, hop) * hop consecutive samples): it inverse-transforms the
 * frames that cover the tile into LDS (the forward kernel's half-length transform run backwards) and every thread sums the up to
 * 8 windowed contributions of its samples in ascending frame order -- no floating-point atomics, and a sample's value depends on
 * its utterance's rows alone, not on the tile, the tile size or the batch.  Error bound per sample: DESIGN.md section 3.9.
 * Limits: n_fft a power of two in [64, 1024]; n_fft / 8 <= hop <= n_fft (at most 8 overlapping frames per sample), outside that
 * SL_ERR_UNSUPPORTED.  SL_ERR_INVALID_ARGUMENT for a null pointer, batch outside [1, 65535], max_frames or hop < 1, n_fft
 * outside the range, rows too short, max_frames * hop + n_fft >= 2^31.  All of these on the host, before any launch.
 * All work on `stream`, no workspace, no allocation, no synchronisation.
 * sl_istft_tile_frames: frames of output per work-group at (n_fft, hop); 0 outside the limits. */
int sl_istft_tile_frames(int n_fft, int hop);
int sl_istft(const float* spec, const int32_t* frames, float* audio, const int64_t* out_offsets, int batch, int max_frames,
             int n_fft, int hop, int row_stride, int64_t batch_stride, void* stream);

/* z_normalize (labeled_example.py:28-29, 136-140): per utterance (a - mean(a)) / std(a) over its frames[b] x f values
 * (population standard deviation, float64 statistics like numpy), written densely as float[B][max_frames][f]; rows
 * t >= frames[b] are zero -- exactly the zero-padded input batch of net.py:578-587, ready for sl_pack_input.
 * workspace: sl_z_normalize_workspace_bytes(batch) bytes. */
size_t sl_z_normalize_workspace_bytes(int batch);
int sl_z_normalize(const float* src, const int32_t* frames, float* dst, int batch, int max_frames, int f,
                   int src_row_stride, int64_t src_batch_stride, void* workspace, size_t workspace_bytes, void* stream);

/* ---- sample-rate conversion (speechless/labeled_example.py:200-205: librosa.load(file, sr=16000); DESIGN.md "Resampling") ----
 * sl_resample_polyphase: a ragged batch of utterances (the layout of sl_stft_power_db) through the polyphase FIR bank that
 * speechless_amd/resample.py: polyphase_bank(sr_orig, sr_new) builds, q / p = sr_new / sr_orig in lowest terms:
 *      y[t] = sum_{j < width} bank[r][j] * x[n - (left - 1) + j],   n = (t p) div q,  r = (t p) mod q   (exact integers),
 *      x = 0 outside [0, in_lengths[b]);   t < floor(len q / p);   y[t] = 0 for floor(len q / p) <= t < ceil(len q / p).
 *   audio, in_offsets, in_lengths: utterance b is read at audio + in_offsets[b] and has in_lengths[b] >= 1 samples
 *   out, out_offsets             : its ceil(in_lengths[b] q / p) outputs go to out + out_offsets[b]; nothing else is written
 *   bank                         : float[q][width] in HBM, left = taps at and before sample n (1 <= left <= width)
 * fp32 FMAs accumulated in fp32, in an order that depends on nothing but (p, q, width): an utterance's output does not depend
 * on the batch it sits in.  |y[t] - exact| <= (width + 2) 2^-24 sum_j |bank[r][j]| |x[..]|.
 * Errors (on the host, before any launch): SL_ERR_INVALID_ARGUMENT for a null pointer, batch outside [1, 65535], p or q < 1,
 * p == q, a common factor of p and q, left outside [1, width].  SL_ERR_UNSUPPORTED beyond the limits: q <= SL_RESAMPLE_MAX_PHASES,
 * width <= SL_RESAMPLE_MAX_TAPS, and the LDS of a tile -- its input span, (SL_RESAMPLE_TILE - 1) p / q + 1 + width floats, plus a
 * bank chunk of q * (min(width, 4096 / q) | 1) floats -- within 64 KiB: p / q up to about 7 (96 -> 16 kHz fits, 192 -> 16 kHz
 * does not).  One work-group per (utterance, tile of SL_RESAMPLE_TILE consecutive outputs), a fixed grid striding over the
 * tiles (the lengths are in HBM); all work on `stream`, no workspace, no allocation, no synchronisation. */
#define SL_RESAMPLE_TILE 2048
#define SL_RESAMPLE_MAX_PHASES 1024
#define SL_RESAMPLE_MAX_TAPS 4096
int sl_resample_polyphase(const float* audio, const int64_t* in_offsets, const int32_t* in_lengths, float* out,
                          const int64_t* out_offsets, const float* bank, int batch, int p, int q, int left, int width,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPEECHLESS_HIP_H */
