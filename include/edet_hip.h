/*
 * edet_hip.h -- C ABI of the MI355X (gfx950) EfficientDet hot path.
 *
 * The reference (google/automl, efficientdet/) has no FFI boundary of its own:
 * its hot path is Python calling un-vendored TensorFlow ops.  Each entry point
 * below therefore replaces one *TensorFlow op call site* of the reference and
 * cites it (paths relative to the reference root).  The caller is the Python
 * host mirror in automl_amd/ (ctypes); see INTEGRATION.md for the binding a
 * reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative code on failure;
 *     edet_last_error() returns a thread-local message.
 *   - all tensors are NHWC in device memory (HBM), element type `dtype`
 *     (EDET_F32 or EDET_BF16), channel stride `ld` >= c (ld % 8 == 0);
 *     statistics, gates, scales, parameters' master copies and parameter
 *     gradients are always fp32.
 *   - the caller owns every buffer; the library allocates nothing and only
 *     enqueues work on the HIP stream passed in (`stream` is a hipStream_t
 *     passed as void*; NULL = default stream).  Nothing synchronises, so all
 *     entry points are legal inside hipGraph stream capture.
 *   - not thread-safe per stream; re-entrant across streams.
 */
#ifndef EDET_HIP_H_
#define EDET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDET_F32 0
#define EDET_BF16 1

#define EDET_ACT_NONE 0
#define EDET_ACT_SWISH 1
/* utils.activation_fn (utils.py:36-53) beyond swish: value and derivative at every activated view */
#define EDET_ACT_RELU 2
#define EDET_ACT_RELU6 3
#define EDET_ACT_HSWISH 4   /* x * relu6(x + 3) / 6 */
#define EDET_ACT_MISH 5     /* x * tanh(softplus(x)) */
#define EDET_ACT_SRELU 6    /* utils.srelu_fn (utils.py:25-31): x - log(beta x + 1) / beta for x > 0, else 0; beta = 20^4 */
#define EDET_ACT_LAST EDET_ACT_SRELU

/* resample modes of one BiFPN fusion input */
#define EDET_RS_IDENTITY 0
#define EDET_RS_UP2 1   /* nearest-neighbour upsample, src = min(floor(dst*in/out), in-1) */
#define EDET_RS_POOL 2  /* max-pool 3x3 stride 2, TF 'SAME', padding excluded from the max */

/* number of per-workgroup statistic partial rows a kernel may write */
#define EDET_MAX_PARTS 1024

/*
 * "Activated view" of a stored tensor: value(n,h,w,c) =
 *     act(data * scale[c] + shift[c]) * gate[n,c]
 * scale/shift NULL -> identity affine; gate NULL -> 1.  This is how BatchNorm
 * (utils.py:166-266), swish (utils.py:36-39) and the SE gate
 * (efficientnet_model.py:183-195) are applied on load by the consuming kernel
 * instead of as separate HBM passes.
 */
typedef struct edet_tview {
  const void* data;
  const float* scale;
  const float* shift;
  const float* gate;
  int act;
  int n, h, w, c, ld;
} edet_tview_t;

/*
 * Gradient view: dy(n,h,w,c) = a[c]*dz + b[c]*y + cc[c]  (a == NULL -> dy = dz).
 * This is the BatchNorm backward applied on load: dz is the gradient w.r.t. the
 * BN output, y the saved output of THE convolution whose gradients are being taken
 * (see EDET_EPI_Y_IS_CONV_OF_INPUT), and (a,b,cc) come from edet_bn_bwd_finalize.
 */
typedef struct edet_gview {
  const void* dz;
  const void* y;
  const float* a;
  const float* b;
  const float* cc;
  int n, h, w, c, ld;
} edet_gview_t;

/*
 * What a data-gradient kernel does with d(view) for its input view `in`:
 *   plain        : g = d
 *   act          : g = d * act'(z),  z = data*scale+shift
 *   gate         : store D = d (the gated gradient) and accumulate
 *                  dgate[n,c] += sum_hw D * act(z); edet_se_gate_bwd finishes.
 *                  (beta must be 0 with a gate: the gate sums are taken from
 *                  the gradient just stored, in a fixed order, after the
 *                  data-gradient kernel or in ordered slots of the one-pass
 *                  kernel -- no atomics; an SE output has one consumer.)
 *   beta != 0    : g += previous contents of gout.
 *   stat_partials: per-workgroup partial sums of (g, g*xhat), xhat =
 *                  (data-mean)*rstd, row p at stat_partials[p*2*c .. ]; the
 *                  kernel writes exactly `*nparts_out` rows.
 */
typedef struct edet_bwd_epi {
  void* gout;
  int beta;
  const float* mean;
  const float* rstd;
  float* stat_partials;
  float* dgate;
  int flags;      /* EDET_EPI_* bits */
} edet_bwd_epi_t;
/* The convolution whose output gradient `dy` is has NO bias, so dy->y (its saved output) equals view(in) * W as
 * edet_pw_fwd stored it.  With this bit set the pointwise backward entry points may apply the b*y term of the
 * BatchNorm backward through the convolution INPUT (dx = dz (W diag a)^T + x~ (W diag(b) W^T) + c W^T, dW = (x~^T dz)
 * diag a + (x~^T x~) W diag b + (sum x~) c^T) and never read y: for an MBConv expansion that is 43 % less HBM traffic.
 * Without it they read y.  Valid only while the stored y is exactly what edet_pw_fwd wrote from THIS input view and THIS
 * kernel (no in-place modification of x, W or y in between); the recomputed product is not rounded to the storage type,
 * so the gradients differ from the read-y form by the rounding of y (2^-9 relative per element, zero mean) --
 * tests/test_gpu_kernels.py::test_pw_bwd runs both forms (EDET_PW_NOY=0 / 1) against the oracle under this contract.  */
#define EDET_EPI_Y_IS_CONV_OF_INPUT 1

const char* edet_last_error(void);
int edet_version(void);

/* ---- debug launch log ----------------------------------------------------------
 * Test infrastructure on the product side of the boundary: while the log is on, the library counts every
 * kernel launch by kernel symbol.  edet_debug_launch_log(1) clears the log and starts it, (0) stops it;
 * edet_debug_launch_names writes "count<TAB>demangled kernel name<NEWLINE>" lines (NUL terminated, truncated
 * to `capacity`; *needed = bytes for the whole text).  tests/test_gpu_bench_shapes.py uses it to assert that
 * every kernel symbol of the full-size benchmark step is also launched by a test that checks results
 * against the oracle.  The reference has no counterpart (TensorFlow picks its kernels internally).  */
int edet_debug_launch_log(int enable);
int edet_debug_launch_names(char* buf, size_t capacity, size_t* needed);

/* ---- parameter preparation ------------------------------------------------
 * fp32 master -> compute copy (dtype), optionally transposed [rows][cols] ->
 * [cols][ld_out].  Replaces the Keras mixed-precision variable cast
 * (utils.py:552-566).  */
int edet_cast(const float* src, void* dst, int64_t count, int dtype, void* stream);
int edet_cast_matrix(const float* src, void* dst, int rows, int cols, int ld_out,
                     int transpose, int dtype, void* stream);

/* all compute copies of a step in ONE launch: items_dev is a device array of `count` descriptors (the
 * arguments of edet_cast_matrix), max_blocks_per_item bounds the 256-thread blocks that stride over one item.  */
typedef struct edet_cast_item {
  const float* src;
  void* dst;
  int rows, cols, ld_out, transpose;
} edet_cast_item_t;
int edet_cast_batch(const edet_cast_item_t* items_dev, int count, int max_blocks_per_item, int dtype,
                    void* stream);

/* ---- stem: Conv2D 3x3 stride 2 'SAME', Cin = 3, no bias --------------------
 * efficientnet_model.py:511-519.  images [n,h,w,3] (ld 3), weight fp32 HWIO
 * [3,3,3,cout].  Writes raw conv output and BN statistic partials.  */
int edet_stem_fwd(const void* images, int n, int h, int w, const float* weight,
                  void* out, int cout, int ldo, float* stat_partials, int* nparts_out,
                  int dtype, void* stream);
/* dweight [3,3,3,cout] fp32 is accumulated into.  workspace: caller-owned device scratch for the per-workgroup
 * partial sums (27 * cout floats each, at most EDET_MAX_PARTS of them), added in a fixed order -- the same
 * gradient on every run; may be NULL (or smaller than EDET_MAX_PARTS rows), then ONE workgroup computes the whole sum
 * and adds it into dweight itself (slow, still the same bits on every run: the library has no floating-point atomics
 * on this path in either storage type).  */
int edet_stem_bwd_weight(const void* images, int n, int h, int w,
                         const edet_gview_t* dy, float* dweight, void* workspace, size_t workspace_bytes,
                         int dtype, void* stream);

/* ---- pointwise (1x1) convolution = GEMM on the matrix cores ----------------
 * Conv2D 1x1 call sites: efficientnet_model.py:304-312,345-353;
 * efficientdet_keras.py:286-290 and the pointwise half of SeparableConv2D
 * (:195-207,459-464,546-556).  wt is the compute copy [cout][ldw] (K contiguous),
 * bias fp32 [cout] or NULL.  */
int edet_pw_fwd(const edet_tview_t* in, const void* wt, int ldw, const float* bias,
                void* out, int cout, int ldo, float* stat_partials, int* nparts_out,
                int dtype, void* stream);
/* the same 1x1 convolution of a bf16 view with the output stored as fp32 [rows][ldo] (ldo in floats, a multiple of 4,
 * >= cout rounded up to 8: the padding columns up to there are written as 0, those behind are left alone), no statistics: the class / box predict layers of the inference forward (efficientdet_keras.py:459-464,
 * 546-556) -- rounding the logits to bf16 alone costs 3e-3 of their range, the convolution itself 1e-4 */
int edet_pw_fwd_f32out(const edet_tview_t* in, const void* wt, int ldw, const float* bias, float* out,
                       int cout, int ldo, void* stream);
/* d(in) from dy: w is the compute copy [cin][ldw] (Cout contiguous).  */
int edet_pw_bwd_data(const edet_gview_t* dy, const void* w, int ldw,
                     const edet_tview_t* in, const edet_bwd_epi_t* epi, int* nparts_out,
                     int dtype, void* stream);
/* dweight[cin][cout] (fp32, HWIO of a 1x1 kernel) += in^T dy.
 * workspace: caller-owned device scratch (fp32 partial sums [splits][cin][cout], deterministic
 * two-pass reduction); may be NULL -- the fp32 / generic kernel then runs a single row split that adds into dweight
 * itself (slow, no atomics, the same bits on every run).  64 MiB covers every EfficientDet-D0..D7x layer at full speed.  */
int edet_pw_bwd_weight(const edet_tview_t* in, const edet_gview_t* dy, float* dweight,
                       void* workspace, size_t workspace_bytes, int dtype, void* stream);
/* both gradients of one layer in one call (TF's Conv2DBackpropInput + Conv2DBackpropFilter under the reference's
 * GradientTape, train_lib.py:623-669): the same result as edet_pw_bwd_weight followed by edet_pw_bwd_data with the
 * same arguments (workspace required).  In bf16, "expand"-shaped layers whose weight matrix fits a wave's registers
 * (cout >= 2 cin, cin <= 32, cout <= 144: the first MBConv expansions, where the 6x expanded gradient pair
 * dominates the traffic) run ONE fused kernel that reads dy, the saved convolution output behind it and the saved
 * input once; other shapes run the two kernels.  */
int edet_pw_bwd(const edet_gview_t* dy, const void* w, int ldw, const edet_tview_t* in,
                const edet_bwd_epi_t* epi, int* nparts_out, float* dweight, void* workspace,
                size_t workspace_bytes, int dtype, void* stream);

/* ---- dense k x k convolution, k in {1,3,5}, stride in {1,2}, TF 'SAME', no bias ----
 * Fused-MBConv call sites: efficientnetv2/effnetv2_model.py:338-346 (k x k expand conv) and
 * :362-371 (the single k x k conv of an expand_ratio == 1 block).  wt is the compute copy
 * [cout][ldw] with the reduction index (ky*k + kx)*cin + c contiguous (edet_cast_matrix of the
 * HWIO kernel viewed as [k*k*cin][cout], transposed; ldw >= k*k*cin).  Writes the raw conv output
 * and BatchNorm statistic partials like edet_pw_fwd.  */
int edet_conv_fwd(const edet_tview_t* in, const void* wt, int ldw, int k, int stride,
                  void* out, int cout, int ldo, float* stat_partials, int* nparts_out,
                  int dtype, void* stream);

/* gradients of the dense convolution (TF Conv2DBackpropInput / Conv2DBackpropFilter under the reference's
 * GradientTape).  w_t: compute copy [cin][ldw] with the reduction index (ky*k + kx)*cout + co contiguous (the HWIO
 * kernel permuted to [cin][k][k][cout]); epi as for edet_pw_bwd_data (no gate).  dweight: fp32 HWIO
 * [k][k][cin][cout], accumulated into; workspace as for edet_pw_bwd_weight.  */
int edet_conv_bwd_data(const edet_gview_t* dy, const void* w_t, int ldw, int k, int stride,
                       const edet_tview_t* in, const edet_bwd_epi_t* epi, int* nparts_out,
                       int dtype, void* stream);
int edet_conv_bwd_weight(const edet_tview_t* in, const edet_gview_t* dy, int k, int stride,
                         float* dweight, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ---- head of an MBConv block in one kernel (bf16 storage) ----------------------------------
 * efficientnet_model.py:378-392: x = act(bn0(expand_conv(x))); x = act(bn1(depthwise_conv(x))) -- the layers of
 * :304-327.  The expanded tensor (6 x the block input) is produced by the matrix cores INSIDE the depthwise march
 * instead of being written by edet_pw_fwd and read back by edet_dw_fwd (automl_amd/csrc/mbconv_fused.hip).
 *   in           : the block input as an affine view (the producer's BatchNorm on load, or a stored tensor): no
 *                  activation, no gate, c <= 32 channels (c % 8 == 0).
 *   w_t          : the expansion kernel as edet_pw_fwd takes it -- compute copy [cexp][ldw], input channel contiguous;
 *                  cexp % 48 == 0 (every EfficientNet expansion width is).
 *   exp_scale/exp_shift : the expansion's BatchNorm as edet_bn_finalize / edet_bn_eval wrote it; act: its activation.
 *   expanded_out : NULL (inference: the expanded tensor is never stored) or the raw expanded tensor [n,h,w,lde], which
 *                  the training backward pass reads (edet_dw_bwd, edet_pw_bwd) exactly as if edet_pw_fwd had stored it.
 *   out / stat_partials / nparts_out : as edet_dw_fwd.
 * Training needs the batch statistics of the expansion before the depthwise convolution can run:
 * edet_mbconv_expand_stats makes the partial rows (same matrix-core products, same bf16 rounding, nothing stored) that
 * edet_bn_finalize turns into exp_scale / exp_shift.  edet_mbconv_fused_supported: 1 = these two entry points apply to
 * the layer, 0 = the caller runs edet_pw_fwd + edet_dw_fwd.  */
int edet_mbconv_fused_supported(const edet_tview_t* in, int cexp, int k, int stride, int dtype);
int edet_mbconv_expand_stats(const edet_tview_t* in, const void* w_t, int ldw, int cexp,
                             float* stat_partials, int* nparts_out, int dtype, void* stream);
int edet_mbconv_expand_dw_fwd(const edet_tview_t* in, const void* w_t, int ldw, int cexp,
                              const float* exp_scale, const float* exp_shift, int act,
                              void* expanded_out, int lde, const float* dw_weight, int k, int stride,
                              void* out, int ldo, float* stat_partials, int* nparts_out, int dtype,
                              void* stream);

/* ---- depthwise convolution k in {3,5}, stride in {1,2}, TF 'SAME' ----------
 * DepthwiseConv2D call sites: efficientnet_model.py:320-327 and the depthwise
 * half of SeparableConv2D.  weight fp32 [k,k,c] (HWIO with multiplier 1).  */
int edet_dw_fwd(const edet_tview_t* in, const float* weight, int k, int stride,
                void* out, int ldo, float* stat_partials, int* nparts_out,
                int dtype, void* stream);
int edet_dw_bwd_data(const edet_gview_t* dy, const float* weight, int k, int stride,
                     const edet_tview_t* in, const edet_bwd_epi_t* epi, int* nparts_out,
                     int dtype, void* stream);
/* dweight [k,k,c] fp32 is accumulated into; workspace as for edet_pw_bwd_weight (may be NULL). */
int edet_dw_bwd_weight(const edet_tview_t* in, const edet_gview_t* dy, int k, int stride,
                       float* dweight, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* both gradients of one layer in one call: the same result as edet_dw_bwd_weight followed by
 * edet_dw_bwd_data (same arguments); in bf16, for either stride, a single kernel (k_bwd_one) that reads dy,
 * the saved conv output behind it and the saved input once.  */
int edet_dw_bwd(const edet_gview_t* dy, const float* weight, int k, int stride,
                const edet_tview_t* in, const edet_bwd_epi_t* epi, int* nparts_out,
                float* dweight, void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ---- deferred weight-gradient reductions -------------------------------------------------
 * Every weight-gradient entry point above that takes a workspace ends in "dweight += sum of the partial sums it left
 * there" (a small kernel per call: ~190 of them per EfficientDet-D0 step).  edet_reduce_defer(stream, 1): from now on those
 * sums on `stream` are recorded instead of launched; edet_reduce_flush(stream) adds everything recorded in ONE launch
 * (same destinations in recording order -- a fixed summation order, the same result on every run; legal inside a
 * stream capture).  Between a call and the flush the caller must not reuse the part of the workspace that holds its partial
 * sums: edet_reduce_deferred_end gives the highest address of the recorded partial regions (NULL: nothing recorded), so a
 * caller can hand the next call the workspace from there on.  edet_reduce_defer(stream, 0) flushes and returns to the
 * immediate mode.  Host-side state per stream; not thread safe.  */
int edet_reduce_defer(void* stream, int enable);
int edet_reduce_flush(void* stream);
int edet_reduce_deferred_end(void* stream, const void** hi_out);

/* ---- BatchNorm statistics --------------------------------------------------
 * utils.py:244-266 / util_keras.py:29-66 (eps 1e-3, momentum 0.99).
 * finalize: partial sums -> batch mean / biased variance -> scale, shift, mean,
 * rstd; moving statistics updated in place when momentum >= 0: moving_var with the Bessel-corrected batch
 * variance when bessel != 0 (Keras' fused BatchNormalization, the single-replica classes of utils.py:244-266),
 * with the biased one when bessel == 0 (SyncBatchNormalization / TpuBatchNormalization force fused=False,
 * utils.py:166-213).  */
int edet_bn_finalize(const float* partials, int nparts, int c, double count,
                     const float* gamma, const float* beta, float eps, float momentum, int bessel,
                     float* moving_mean, float* moving_var,
                     float* scale, float* shift, float* mean, float* rstd, void* stream);
/* inference: scale/shift from the moving statistics */
int edet_bn_eval(int c, const float* gamma, const float* beta, float eps,
                 const float* moving_mean, const float* moving_var,
                 float* scale, float* shift, void* stream);
/* partial sums of (dz, dz*xhat) over a stored gradient (multi-consumer case) */
int edet_bn_bwd_reduce(const void* dz, const void* y, int64_t rows, int c, int ld,
                       const float* mean, const float* rstd,
                       float* stat_partials, int* nparts_out, int dtype, void* stream);
/* partials -> dgamma, dbeta (accumulated) and the on-load coefficients a,b,cc.
 * dbias is ignored (may be NULL): the gradient of a bias that feeds a BatchNorm is
 * analytically zero because BN removes the per-channel mean.  */
int edet_bn_bwd_finalize(const float* partials, int nparts, int c, double count,
                         const float* gamma, const float* mean, const float* rstd,
                         float* dgamma, float* dbeta, float* dbias,
                         float* a, float* b, float* cc, void* stream);

/* ---- block output: out = view(y) (+ residual) ---------------------------------
 * efficientnet_model.py:393-410 (project BN, identity skip).  y->gate [n][c], when set, is the
 * stochastic-depth scale floor(p + u_n) / p of utils.drop_connect (utils.py:329-344), constant along c.  */
int edet_bn_res(const edet_tview_t* y, const void* residual, void* out, int ldo,
                int dtype, void* stream);
/* dst = (beta ? dst : 0) + src, elementwise on [rows][c] with ld */
int edet_add(void* dst, const void* src, int64_t rows, int c, int ld, int beta,
             int dtype, void* stream);

/* ---- squeeze-and-excitation --------------------------------------------------
 * efficientnet_model.py:153-195: mean over H,W -> 1x1 (+bias) -> act (the model's relu_fn, an EDET_ACT_* code)
 * -> 1x1 (+bias) -> sigmoid.
 * edet_se_pool: pooled_sum [n,c] = sum over H,W of view(in) (the gate of `in` is ignored).  No atomics: an image's rows
 * are summed in chunks whose size depends on (H*W, c) only, the chunk sums (written to `scratch`, caller-owned, at
 * least n * ceil(H*W / chunk) * c floats: 8 MB covers every EfficientDet / EfficientNetV2 layer; the chunks grow if it
 * is smaller) are added in chunk order -- the same image gives the same bits in every batch and on every run.
 * edet_se_squeeze_excite: the pooling and both 1x1 layers in two launches (the FC kernel adds the chunk sums itself);
 * also writes pooled_sum (edet_se_fc_bwd reads it).  inv_hw = 1 / (H*W).  */
int edet_se_pool(const edet_tview_t* in, float* pooled_sum, void* scratch, size_t scratch_bytes,
                 int dtype, void* stream);
int edet_se_fc(const float* pooled_sum, int n, int c, int se, float inv_hw,
               const float* w1, const float* b1, const float* w2, const float* b2,
               float* hidden_pre, float* gate, int act, void* stream);
int edet_se_squeeze_excite(const edet_tview_t* in, void* scratch, size_t scratch_bytes, int se, float inv_hw,
                           const float* w1, const float* b1, const float* w2, const float* b2,
                           float* pooled_sum, float* hidden_pre, float* gate, int act, int dtype, void* stream);
/* dgate [n,c] -> dpool [n,c] (already divided by H*W), parameter gradients.
 * scratch: caller-owned fp32 workspace of n * (c + (2 + ceil(c / 128)) * se) + 8 * (2 * c * se + c + se) elements
 * (the second term: the parameter gradients of 8 image slices, added in slice order -- no atomics).  */
int edet_se_fc_bwd(const float* pooled_sum, const float* hidden_pre, const float* gate,
                   const float* dgate, int n, int c, int se, float inv_hw,
                   const float* w1, const float* w2,
                   float* dw1, float* db1, float* dw2, float* db2,
                   float* dpool, float* scratch, int act, void* stream);
/* in place on g (holding the gated gradient D): dz = (D*gate + dpool)*act'(z);
 * writes BN backward partials for `in`'s BatchNorm.  */
int edet_se_gate_bwd(const edet_tview_t* in, void* g, const float* dpool,
                     const float* mean, const float* rstd,
                     float* stat_partials, int* nparts_out, int dtype, void* stream);

/* ---- BiFPN weighted fusion ---------------------------------------------------
 * efficientdet_keras.py:75-121 (fuse_features), :254-281 (max-pool / nearest
 * resample), :214-217 (swish before the separable conv).
 * out = act( sum_i wn_i * resample_i(view_i) ), wn = normalised weights, fp32 [3][wc]: wc = 1 for one weight per
 * input (fastattn / attn / sum), wc = c for the per-channel methods channel_fastattn / channel_attn
 * (efficientdet_keras.py:100-113: the same two formulas applied per channel; WSM variables of shape [c]).  */
int edet_fuse_weights(const float* w0, const float* w1, const float* w2, int nin,
                      int method /*0 fastattn, 1 sum, 2 attn (softmax)*/, float* wn, int wc, void* stream);
/* wraw (may be NULL): the raw fusion variables {w0, w1, w2} (device scalars) when wc == 1 -- the kernel normalises them
 * itself with edet_fuse_weights' arithmetic (method as there) and stores the result in wn for the backward calls, so
 * the edet_fuse_weights launch is not needed; NULL or wc > 1: wn is read as computed by edet_fuse_weights.  */
int edet_fuse_fwd(const edet_tview_t* in0, const edet_tview_t* in1, const edet_tview_t* in2,
                  const int* modes, int nin, float* wn, int wc, int act,
                  void* out, int oh, int ow, int ldo, const float* const* wraw, int method, int dtype, void* stream);
/* ds = dout * act'(s) (s recomputed) written to `ds`; dwn[i] += sum ds * x_i.
 * gin / gbeta (may be NULL): per input, the gradient buffer of an EDET_RS_IDENTITY input that this call writes itself
 * (gin[i] (+)= wn[i] * ds when gbeta[i]; exactly what edet_fuse_bwd_input gives) -- saves that launch and its read of
 * ds; write_ds = 0 when no other input needs the stored ds (`ds` may then be NULL).  Also accepted: gin[1] of a node {EDET_RS_IDENTITY,
 * EDET_RS_UP2} with wc == 1, oh == 2 h and ow == 2 w (the top-down nodes of a BiFPN): gin[1] (+)= wn[1] * (the sum of
 * the 2x2 ds above each pixel, each rounded to the storage type, in row-major order) -- again edet_fuse_bwd_input's bits.
 * gin of any other resampled input (a pool, another up-sampling ratio, per-channel weights) is an error.
 * workspace (may be NULL): caller-owned scratch for the per-workgroup partial sums of the scalar fusion weights
 * (16 bytes per workgroup: 64 KiB is enough; per-channel weights: nin * c floats per workgroup), added in a fixed order
 * -- the same dwn on every run; NULL or too small: the kernel runs as ONE workgroup that adds its sums into dwn itself
 * (slow, no atomics).
 * pool_argmax (may be NULL): caller-owned bytes [npool][n][oh][ow][c], one plane per EDET_RS_POOL
 * input in input order; receives the winning tap (ky*3+kx, first maximum of the row-major scan) of
 * every pooled element so that edet_fuse_bwd_input does not have to recompute the 3x3 windows.
 * wraw / dwraw (may be NULL): the raw scalar fusion variables and their gradients {dw0, dw1, dw2}; with both (and
 * wc == 1, a workspace, method 0 or 2) the ordered finish of dwn also adds the normalisation's backward into dwraw --
 * edet_fuse_weights_bwd's arithmetic without its launch (an error when the partial-row path is not available).  */
int edet_fuse_bwd_pre(const edet_tview_t* in0, const edet_tview_t* in1, const edet_tview_t* in2,
                      const int* modes, int nin, const float* wn, int wc, int act,
                      const void* dout, int oh, int ow, int ldo,
                      void* ds, float* dwn, void* pool_argmax, void* const* gin, const int* gbeta, int write_ds,
                      void* workspace, size_t workspace_bytes, const float* const* wraw, int method,
                      float* const* dwraw, int dtype, void* stream);
/* gradient of one fusion input: gout (+)= wn[i] * resample_i^T(ds).  pool_argmax: this input's
 * plane written by edet_fuse_bwd_pre (EDET_RS_POOL only; NULL -> the windows are recomputed).  */
int edet_fuse_bwd_input(const edet_tview_t* in, int mode, const float* wn, int wc, int idx,
                        const void* ds, int oh, int ow, int lds_, const void* pool_argmax,
                        void* gout, int beta, int dtype, void* stream);
/* raw weight gradients from dwn (fast-attention normalisation backward) */
int edet_fuse_weights_bwd(const float* w0, const float* w1, const float* w2, int nin,
                          int method, const float* dwn, float* dw0, float* dw1, float* dw2,
                          int wc, void* stream);

/* ---- detection loss forward + backward --------------------------------------
 * train_lib.py:357-437,493-604: focal loss (alpha, gamma) on class logits,
 * Huber(delta) on box codes; writes d(loss)/d(logits) and accumulates
 * sums[0] += cls_loss, sums[1] += box_loss (already normalised).
 * cls_targets int32 [n,h,w,a] (-1 background, -2 ignore).
 * norm_scale_dev (may be NULL): device scalar multiplied into inv_normalizer at run time, so that a
 * captured hipGraph of the step can be replayed with the next batch's normalizer
 * (sum(mean_num_positives) + 1, train_lib.py:517).
 * workspace: caller-owned device scratch for the per-workgroup partial rows (loss sum + bias gradient), added in a
 * fixed order -- the same loss and bias gradient on every run; (a few thousand rows of 1 + channels floats: 8 MiB
 * covers every EfficientDet head); NULL or too small: the kernel runs as ONE workgroup (slow, no atomics).
 * Refused (-1, nothing launched): alpha outside [0, 1], gamma negative or not finite (gamma == 1.5 has kernels of its own,
 * every other value goes through pow; 0 is accepted: sigmoid^0 = 1 also where the sigmoid underflows to 0), label_smoothing
 * outside [0, 1], delta <= 0 or not finite, ld no multiple of 8, below the channels or above 2048, no classes / anchors /
 * channels, positions < 0.  positions == 0 is accepted and writes nothing.  Padding columns and the logits of ignored anchors
 * (-2) / the box outputs of masked targets (+-0.0) are not read into the result: they may hold anything, NaN included; the
 * padding columns of the gradient are written as zeros.  */
int edet_focal_loss(const void* logits, int ld, const int32_t* cls_targets,
                    int64_t positions, int num_anchors, int num_classes,
                    float alpha, float gamma, float inv_normalizer, const float* norm_scale_dev,
                    void* dlogits, float* dbias, float* sums, void* workspace, size_t workspace_bytes,
                    int dtype, void* stream);
/* the same with FocalLoss(label_smoothing) (train_lib.py:400-402, config.label_smoothing): the cross entropy is taken
 * against y*(1 - label_smoothing) + label_smoothing/2, alpha and the modulating factor keep the hard label */
int edet_focal_loss_smooth(const void* logits, int ld, const int32_t* cls_targets,
                           int64_t positions, int num_anchors, int num_classes,
                           float alpha, float gamma, float label_smoothing, float inv_normalizer,
                           const float* norm_scale_dev,
                           void* dlogits, float* dbias, float* sums, void* workspace, size_t workspace_bytes,
                           int dtype, void* stream);
int edet_box_loss(const void* box_out, int ld, const float* box_targets,
                  int64_t positions, int nch, float delta, float inv_normalizer,
                  float grad_scale, const float* norm_scale_dev, void* dbox, float* dbias, float* sums,
                  void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ---- the evaluation step's losses (train_lib.py:686-732, test_step): loss only, nothing else written -----------------------
 * edet_focal_loss_eval / edet_box_loss_eval add into sums[0] / sums[1] EXACTLY what edet_focal_loss (label_smoothing == 0) or
 * edet_focal_loss_smooth, and edet_box_loss, add for the same logits, targets, normalizer arguments and workspace size, bit for
 * bit: the same per-element arithmetic (instantiations of the same kernel bodies without the gradient), the same grid, the
 * same order of the sums (wave shuffles, waves in order, the workgroups' partial values in order).  No dlogits, no dbias: the
 * logits are read once and nothing of their size is written.  workspace: as above ([workgroups][1 + channels] floats decide
 * between the grid and ONE workgroup exactly as in training, although only one float per workgroup is used).
 * edet_l2_loss: l2_out[0] = weight_decay * sum over the segments with EDET_SEG_L2 and without EDET_SEG_FROZEN of sum(w^2) / 2
 * (train_lib.py:486-491), the value edet_opt_l2_norms + edet_opt_clip_factors add into l2_sum for the same variables, bit for
 * bit (the same slices, the same sums, the same final order) -- written, not added, and the gradient arena is not touched.
 * seg_l2: scratch [nseg][EDET_OPT_SPLIT] floats.  */
int edet_focal_loss_eval(const void* logits, int ld, const int32_t* cls_targets,
                         int64_t positions, int num_anchors, int num_classes,
                         float alpha, float gamma, float label_smoothing, float inv_normalizer,
                         const float* norm_scale_dev, float* sums, void* workspace, size_t workspace_bytes,
                         int dtype, void* stream);
int edet_box_loss_eval(const void* box_out, int ld, const float* box_targets,
                       int64_t positions, int nch, float delta, float inv_normalizer,
                       const float* norm_scale_dev, float* sums, void* workspace, size_t workspace_bytes,
                       int dtype, void* stream);
int edet_l2_loss(const float* params, const int64_t* seg_offsets, const int32_t* seg_flags, int nseg,
                 float weight_decay, float* seg_l2, float* l2_out, void* stream);

/* ---- the IoU / GIoU / DIoU / CIoU box loss (efficientdet/iou_utils.py; train_lib.py:440-464, :580-600) --------------------
 * iou_type: 0 iou, 1 giou, 2 diou, 3 ciou.  The gradient is the reference's as TensorFlow executes it: the aspect-ratio term v
 * of ciou is a constant of the backward pass (its tf.custom_gradient reaches the target's size only), alpha is differentiated
 * through iou; ties of maximum / minimum go to the first argument as the reference writes them; divide_no_nan has zero
 * gradient where its denominator is 0; squared lengths are sums of squares (zero gradient at the zero vector).
 *
 * edet_iou_loss: iou_utils.iou_loss on decoded fp32 boxes [rows][k][ymin, xmin, ymax, xmax] (16-byte aligned):
 * loss_out[r] = sum over the k anchors of m * (1 - metric), m = the target has positive height and width;
 * dpred_out (may be NULL) [rows][4k] = d loss_out[r] / d pred_boxes[r].  One launch.
 *
 * edet_box_iou_loss / edet_box_iou_loss_eval: edet_box_loss / edet_box_loss_eval with the IoU loss fused into the same pass.
 * anchors: the level's first anchor row [ymin, xmin, ymax, xmax] fp32 (16-byte aligned), row (p mod hw) * (nch / 4) + a for
 * position p and anchor a; hw divides positions.  The outputs and the targets of an anchor are decoded with that anchor
 * (anchors.py:30-58), each decoded coordinate of both boxes times (its raw target component != 0); an anchor whose four targets
 * are 0 does no arithmetic.  sums[3] += sum of the anchors' losses * inv_normalizer [* norm_scale_dev[0]]; sums[1] as
 * edet_box_loss, bit for bit.  dbox = Huber gradient * inv_norm * grad_scale + IoU gradient * inv_norm * iou_grad_scale, added
 * in fp32 and rounded to the storage type once; dbias += its column sums.  With iou_grad_scale = 0 and finite inputs dbox and
 * dbias are edet_box_loss's bit for bit.  The grid of edet_box_loss; workspace: [workgroups][1 + nch] + [workgroups] floats,
 * else ONE workgroup.  No atomics: the same bits on every run.  edet_box_iou_loss_eval adds to sums[1] and sums[3] what
 * edet_box_iou_loss adds, bit for bit, and writes nothing else.  */
int edet_iou_loss(const float* pred_boxes, const float* target_boxes, int64_t rows, int k, int iou_type,
                  float* loss_out, float* dpred_out, void* stream);
int edet_box_iou_loss(const void* box_out, int ld, const float* box_targets,
                      int64_t positions, int nch, float delta, float inv_normalizer,
                      float grad_scale, const float* norm_scale_dev, void* dbox, float* dbias, float* sums,
                      void* workspace, size_t workspace_bytes, int dtype, void* stream,
                      const float* anchors, int64_t hw, int iou_type, float iou_grad_scale);
int edet_box_iou_loss_eval(const void* box_out, int ld, const float* box_targets,
                           int64_t positions, int nch, float delta, float inv_normalizer,
                           const float* norm_scale_dev, float* sums, void* workspace, size_t workspace_bytes,
                           int dtype, void* stream, const float* anchors, int64_t hw, int iou_type);

/* ---- EfficientNetV2 classifier loss and head dropout (efficientnetv2/main_tf2.py:89-117,199-207) ----
 * edet_softmax_xent: tf.keras.losses.CategoricalCrossentropy(label_smoothing, from_logits=True) with the default mean over
 * the batch (main_tf2.py:201-202), its gradient, and the counts behind TopKCategoricalAccuracy(k=1) / (k=5) (:203-206), in
 * one pass.  logits [batch][ld] in `dtype` (num_classes valid columns), labels int32 [batch] in [0, num_classes) -- sparse
 * labels only; the CALLER checks the range (a label outside it is an argument error, the kernel merely reads nothing out of
 * bounds for one).  Per row in fp32: m = max x, lse = m + log sum exp(x - m), y_c = (1 - s)[c == label] + s / num_classes,
 * loss = lse - sum_c y_c x_c.  dlogits [batch][ld] = (softmax - y) * grad_scale / batch, padding columns written as zeros;
 * sums[0] += mean loss, sums[1] / sums[2] += rows whose label is in the top 1 / top 5 (ties: the number of logits strictly
 * greater than the label's is < k).  Rows are added in a fixed order through `workspace` ([ceil(batch / 4)][3] floats;
 * without one a single workgroup walks the rows): no atomics, the same bits on every run.
 * Stated from the Keras definition; TensorFlow is not installed where this library is tested, so the fp32 restatement in
 * tests/test_effnetv2_train.py (itself pinned against torch.nn.functional.cross_entropy) is what the tests compare with. */
int edet_softmax_xent(const void* logits, int ld, const int32_t* labels, int batch, int num_classes,
                      float label_smoothing, float grad_scale, void* dlogits, float* sums, void* workspace,
                      size_t workspace_bytes, int dtype, void* stream);
/* dst[i] = (dtype) (src[i] * mask[i]): the head dropout (effnetv2_model.py:464-467,483-484: after global pooling, before the
 * dense layer) folded into the cast of the pooled sums; mask = fp32 {0, 1 / (1 - rate)} drawn by the caller, NULL = edet_cast.
 * dst may be src (fp32): the same mask on d(pooled) in the backward pass. */
int edet_dropout_cast(const float* src, const float* mask, void* dst, int64_t count, int dtype, void* stream);

/* ---- soft labels, mixup and cutmix (efficientnetv2/datasets.py:191-301, :321-323) ----
 * edet_softmax_xent_soft: edet_softmax_xent against dense fp32 labels soft_labels [batch][label_ld] (num_classes valid
 * columns, label_ld >= num_classes; 16-byte loads when label_ld is a multiple of 8 and the pointer is 16-byte aligned) --
 * what the reference's input pipeline hands its loss: one-hot rows or mixtures of them.  Keras smooths whatever y it is
 * given, y'_c = (1 - s) y_c + s / num_classes, and a row need not sum to 1: loss = lse * sum_c y'_c - sum_c y'_c x_c,
 * dlogits = (softmax_c * sum_c y'_c - y'_c) * grad_scale / batch, padding columns written as zeros.  The metrics are
 * TopKCategoricalAccuracy's: the row's class is argmax_c y_c (the first index on ties), counted as edet_softmax_xent counts
 * it.  Same sums, workspace, order and run-to-run identity as edet_softmax_xent; no atomics. */
int edet_softmax_xent_soft(const void* logits, int ld, const float* soft_labels, int label_ld, int batch, int num_classes,
                           float label_smoothing, float grad_scale, void* dlogits, float* sums, void* workspace,
                           size_t workspace_bytes, int dtype, void* stream);
/* edet_mix_images: mixup and cutmix of images [batch][height][width][channels] (dense, `dtype`) IN PLACE.  Rows
 * [0, n_mixup) are mixed by mixup, rows [n_mixup, batch) by cutmix, each part with itself in reverse (datasets.py:238,267
 * within the halves of :287-294): the partner of mixup row i is n_mixup - 1 - i, of cutmix row i n_mixup + batch - 1 - i.
 * mixup: out_i = x_i w_i + x_partner (1 - w_i) in fp32, rounded once to `dtype`; cutmix: out_i = x_partner inside row i's
 * OWN box, x_i outside it.  weights: device fp32 [batch] (read for the mixup rows); boxes: device int32 [batch][4] =
 * y1, x1, y2, x2, half-open, clamped to the image by the kernel (read for the cutmix rows) -- device memory, so that a
 * replayed graph sees new draws.  One thread owns the same chunk of a row and of its partner and reads both before it writes
 * either; a row that is its own partner is written once (mixup) or left alone (cutmix).  16-byte chunks when
 * height * width * channels elements are a whole number of them, element by element otherwise.  The cutmix part reads and
 * writes only the image rows that one of the pair's two boxes touches.  Nothing is summed: the same bits on every run. */
int edet_mix_images(void* images, int batch, int height, int width, int channels, int n_mixup, const float* weights,
                    const int32_t* boxes, int dtype, void* stream);
/* edet_mix_labels: the labels of the same mixing.  labels int32 [batch] -> soft_labels fp32 [batch][label_ld], columns
 * [num_classes, label_ld) written as zeros.  mixup rows: w_i onehot(l_i) + (1 - w_i) onehot(l_partner); cutmix rows:
 * (1 - A) onehot(l_i) + A onehot(l_partner), A = (sum of the clamped box areas of the cutmix rows) / ((batch - n_mixup) *
 * height * width): ONE scalar for the whole part, the mean mask area of datasets.py:236 (an integer sum, exact in any
 * order).  A label outside [0, num_classes) adds nothing to its rows (the caller checks the range). */
int edet_mix_labels(const int32_t* labels, int batch, int num_classes, int height, int width, int n_mixup,
                    const float* weights, const int32_t* boxes, float* soft_labels, int label_ld, void* stream);

/* ---- RandAugment (efficientnetv2/autoaugment.py:79-441, :663-702) on uint8 images [batch][height][width][3] ----
 * One layer applies one operation per image; the choice and its arguments are device memory, so that the launch sequence
 * does not depend on the draws and a replayed graph sees new ones.  Operation ids (available_ops, :683-686):
 * 0 AutoContrast, 1 Equalize, 2 Invert, 3 Rotate, 4 Posterize, 5 Solarize, 6 Color, 7 Contrast, 8 Brightness, 9 Sharpness,
 * 10 ShearX, 11 ShearY, 12 TranslateX, 13 TranslateY, 14 Cutout, 15 SolarizeAdd; 16 (and anything outside [0, 16]) = copy.
 * ops int32 [batch]; iargs int32 [batch][4]: Posterize {shift = 8 - bits}, Solarize {threshold}, SolarizeAdd {addition,
 * threshold}, Cutout {y1, x1, y2, x2 half-open}; fargs fp32 [batch][8]: {a0, a1, a2, b0, b1, b2, factor, unused} -- the
 * geometric operations read source pixel (round(a0 x + a1 y + a2), round(b0 x + b1 y + b2)), halves away from zero, 128
 * outside the image; Color / Contrast / Brightness / Sharpness blend with `factor`.  Every index is clamped in the kernel.
 * The arithmetic (single fp32 operations in a stated order, truncating conversions) is restated in tests/randaug_ref.py and
 * compared bit for bit.
 * edet_randaug_stats: for the images whose operation is AutoContrast or Equalize, per-channel histograms (integer LDS
 * atomics) -> luts uint8 [batch][3][256]; the other images' tables are left alone.  Run it in front of edet_randaug_apply
 * of the same layer on the same src.
 * edet_randaug_apply: dst = layer(src), src != dst.  out_dtype EDET_U8: dst uint8, same layout; EDET_F32 / EDET_BF16: the
 * normalised network input (v - 128) / 128 (preprocessing.py:153; exact in both).  ops == NULL: every image is copied
 * (with out_dtype F32 / BF16: the normalising copy of a batch without augmentation); iargs / fargs / luts may then be NULL. */
#define EDET_U8 2
int edet_randaug_stats(const uint8_t* src, int batch, int height, int width, const int32_t* ops, uint8_t* luts, void* stream);
int edet_randaug_apply(const uint8_t* src, void* dst, int batch, int height, int width, const int32_t* ops,
                       const int32_t* iargs, const float* fargs, const uint8_t* luts, int out_dtype, void* stream);
/* edet_randaug_apply_norm: edet_randaug_apply (the same kernel body) whose fp32 / bf16 conversion is the legacy pipeline's
 * (efficientnetv2/preprocess_legacy.py:239-243): fp32 = (float(v) - mean[c]) / std[c], two individually rounded fp32
 * operations with a true IEEE division; bf16 = that value rounded to nearest even.  mean_std: a HOST pointer to six floats
 * {mean r, g, b, std r, g, b}, read at the call and passed to the kernel by value; never NULL, no std zero or NaN.
 * EDET_U8 is edet_randaug_apply's output byte for byte. */
int edet_randaug_apply_norm(const uint8_t* src, void* dst, int batch, int height, int width, const int32_t* ops,
                            const int32_t* iargs, const float* fargs, const uint8_t* luts, int out_dtype, const float* mean_std,
                            void* stream);
/* The same two on a CANVAS batch: src (and dst, in its own element type) [batch][canvas_h][canvas_w][3]; image b is the
 * top-left sizes_dev[b] = {height, width} of its slot (int32 [batch][2], DEVICE memory), its row pitch canvas_w.  Every
 * height, width and pixel count above is then the image's own: the in-image test and the 128 fill of the geometric
 * operations, Sharpness' border, Cutout's clamps, Contrast's H W / 256, Equalize's step; the histograms count the image's
 * pixels only.  Image b inside its rectangle is what the dense call gives for that image alone, bit for bit.  The sizes
 * are clamped in the kernel, height into [1, canvas_h] and width into [1, canvas_w], so no row can send an access outside
 * its slot.  Nothing outside the rectangle is read; dst is written INSIDE the rectangle only, the rest of its slot is left as
 * it was (nothing downstream reads it).  The grid is sized from the canvas.  The four-pixel path is chosen per image: where
 * width % 4 == 0, canvas_w % 4 == 0 and src / dst are 16-byte aligned; the byte path otherwise.
 * batch <= 65535, canvas_h * canvas_w * 3 < 2^31. */
int edet_randaug_stats_canvas(const uint8_t* src, int batch, int canvas_h, int canvas_w, const int32_t* sizes_dev,
                              const int32_t* ops, uint8_t* luts, void* stream);
int edet_randaug_apply_canvas(const uint8_t* src, void* dst, int batch, int canvas_h, int canvas_w, const int32_t* sizes_dev,
                              const int32_t* ops, const int32_t* iargs, const float* fargs, const uint8_t* luts, int out_dtype,
                              void* stream);

/* ---- crop, resize and flip of decoded images (efficientnetv2/preprocessing.py:22-70) ----
 * raw uint8 [batch][canvas_h][canvas_w][3]; image b occupies the top-left height x width of its canvas.  Per image:
 * tf.image.resize(tf.slice(image, crop), [out_h, out_w]) -- bilinear, half-pixel centres, no antialiasing, the taps clamped
 * at the CROP edges -- then, with flip != 0, the left-right mirror of the OUTPUT (column x = column out_w - 1 - x of the
 * resized crop).  out [batch][out_h][out_w][3]: out_dtype EDET_U8 = clip(v, 0, 255) truncated (preprocessing.py:49-50, the
 * input of edet_randaug_*); EDET_F32 / EDET_BF16 = (v - 128) / 128 (:153), bf16 rounded to nearest even.  The fp32 arithmetic
 * is that of edet_preprocess_infer, restated in tests/crop_ref.py and compared bit for bit.  Every field of per_image_dev is
 * clamped in the kernel: height into [1, canvas_h], width into [1, canvas_w], crop_y into [0, height - 1], crop_h into
 * [1, height - crop_y], likewise for x.  batch <= 65535, canvas_h * canvas_w * 3 < 2^31. */
typedef struct edet_crop_image { /* 32 bytes, one per image, read from DEVICE memory */
  int32_t height, width;         /* valid extent of the raw image inside its canvas  */
  int32_t crop_y, crop_x, crop_h, crop_w;
  int32_t flip, reserved;
} edet_crop_image_t;
int edet_crop_resize(const uint8_t* raw, int batch, int canvas_h, int canvas_w, const edet_crop_image_t* per_image_dev,
                     void* out, int out_h, int out_w, int out_dtype, void* stream);
/* edet_crop_resize_bicubic: the same contract (raw, per_image_dev and its clamps, the flip on the OUTPUT column, one launch
 * that does not depend on the draws, the same limits) with tf.image.resize_bicubic of the crop in place of the bilinear
 * resize (efficientnetv2/preprocess_legacy.py:80-127) -- TensorFlow's LEGACY bicubic: align_corners=False,
 * half_pixel_centers=False, a 1024-entry coefficient table with a = -0.75.  Per axis, scale = float(crop_n) / float(out_n):
 *   in_f = float(o) * scale; in = floor(in_f); delta = in_f - float(in); off = lrintf(delta * 1024.0f) (halves to even);
 *   weights (T[2 off + 1], T[2 off], T[2 (1024 - off)], T[2 (1024 - off) + 1]) on the taps in - 1, in, in + 1, in + 2, each
 *   clamped into [0, crop_n - 1] (the CROP's edges);
 *   T[2i] = float(((a + 2) x - (a + 3)) x x + 1), T[2i + 1] = float(((a x' - 5a) x' + 8a) x' - 4a) for x = float(i / 1024.0),
 *   x' = float(x + 1.0f), i = 0 .. 1024, the polynomials in double.  The 2050 floats are evaluated once by the HOST compiler
 *   (constexpr) and lie in the library's code object: no call builds, allocates or copies a table.
 * A value is formed vertically first: for each of the four tap columns c_k = p0 wy0 + p1 wy1 + p2 wy2 + p3 wy3, left to right
 * in fp32, the pixels converted to float; then v = c0 wx0 + c1 wx1 + c2 wx2 + c3 wx3 the same way.  Results overshoot
 * [0, 255].  EDET_U8 = clip(v, 0, 255) truncated (:168-169).  mean_std: a HOST pointer to six floats {mean r, g, b, std r, g,
 * b}, read at the call and passed to the kernel by value: EDET_F32 = (v - mean[c]) / std[c], two individually rounded fp32
 * operations with a true IEEE division, EDET_BF16 = that value rounded to nearest even; NULL = no normalisation (fp32 gets
 * the resized values as they are, bf16 their rounding); uint8 never reads it.  This definition is written from TensorFlow's
 * published resize_bicubic_op and is NOT pinned against TensorFlow (not installed where this project is tested); its numpy
 * restatement tests/bicubic_ref.py is the definition, compared bit for bit. */
int edet_crop_resize_bicubic(const uint8_t* raw, int batch, int canvas_h, int canvas_w, const edet_crop_image_t* per_image_dev,
                             void* out, int out_h, int out_w, int out_dtype, const float* mean_std, void* stream);

/* ---- mosaic augmentation (efficientdet/aug/mosaic.py) ----
 * raw uint8 [batch][canvas_h][canvas_w][3] as for edet_crop_resize; `groups` mosaics [groups][out_h][out_w][3] in one
 * launch.  Mosaic g is made of four source images: with the divide points (x, y) of its row, image index[0] resized to
 * x rows by y columns fills rows [0, x), columns [0, y); index[1], (out_h - x) by y, lies BELOW it (rows [x, out_h));
 * index[2], x by (out_w - y), to its right (columns [y, out_w)); index[3] takes the rest (mosaic.py:115-128, :246-250).
 * Every pixel is tf.image.resize of the WHOLE source image to its quadrant's size at the quadrant-local position, in
 * edet_crop_resize's arithmetic (csrc/resize_tap.h), restated in tests/mosaic_ref.py and compared bit for bit.
 * out_dtype EDET_F32 = the resized values as they are (what the reference returns), EDET_U8 = clip(v, 0, 255) truncated.
 * Every field of per_mosaic_dev is clamped in the kernel: index into [0, batch - 1], height into [1, canvas_h], width
 * into [1, canvas_w], x into [1, out_h - 1], y into [1, out_w - 1]: nothing outside a source image's rectangle is read.
 * out_h, out_w >= 2, groups <= 65535, batch * canvas_h * canvas_w * 3 addressed as size_t, canvas_h * canvas_w * 3 < 2^31. */
typedef struct edet_mosaic { /* 64 bytes, one per mosaic, read from DEVICE memory */
  int32_t index[4];              /* source images: top-left, below it, right of it, the rest */
  int32_t x, y;                  /* divide points: x splits the ROWS, y the COLUMNS (the reference's names) */
  int32_t height[4], width[4];   /* valid extent of each source image inside its canvas */
  int32_t reserved[2];
} edet_mosaic_t;
int edet_mosaic(const uint8_t* raw, int batch, int canvas_h, int canvas_w, const edet_mosaic_t* per_mosaic_dev, int groups,
                void* out, int out_h, int out_w, int out_dtype, void* stream);
/* The boxes of the same mosaics (this library's batch form; the reference's class scales pixel boxes on the host).
 * boxes [batch][max_boxes][4] float normalised (ymin, xmin, ymax, xmax), classes [batch][max_boxes] float, counts [batch]
 * valid rows per image (clamped into [0, max_boxes]).  boxes_out [groups][4 * max_boxes][4], classes_out
 * [groups][4 * max_boxes], counts_out [groups]: the valid rows of source 0, then 1, 2, 3, in their order, the rest -1.
 * For a quadrant at offset (oy, ox) of size (qh, qw), one rounded fp32 operation each:
 *   ymin' = ((float)oy + ymin * (float)qh) / (float)out_h,  xmin' = ((float)ox + xmin * (float)qw) / (float)out_w,
 * the maxima likewise; nothing is clipped.  index, x and y are clamped as in edet_mosaic; heights and widths are not
 * read.  One thread per output row, no atomics.  max_boxes >= 1, groups * 4 * max_boxes < 2^31. */
int edet_mosaic_boxes(const float* boxes, const float* classes, const int32_t* counts, int batch, int max_boxes,
                      const edet_mosaic_t* per_mosaic_dev, int groups, int out_h, int out_w, float* boxes_out,
                      float* classes_out, int32_t* counts_out, void* stream);

/* ---- optimizer -----------------------------------------------------------------
 * train_lib.py:486-491 (L2), :675-682 (per-tensor clip_by_norm then
 * clip_by_global_norm), Keras SGD momentum, TFA MovingAverage (:176-199).
 * All parameters live in one flat fp32 arena; seg_offsets[nseg+1] delimits the
 * tensors, seg_flags bit0 (EDET_SEG_L2) = L2-regularised (kernel/weight variables), bit1 (EDET_SEG_FROZEN) =
 * frozen by config.var_freeze_expr (tf2/train_lib.py:478-491: out of the L2 term, of the gradient list and of the
 * update -- its gradient is zeroed, it adds nothing to the norms, value / momentum / EMA shadow are never touched).  */
#define EDET_SEG_L2 1
#define EDET_SEG_FROZEN 2
/* seg_sqnorm: [2][nseg][EDET_OPT_SPLIT] floats -- EDET_OPT_SPLIT partial squared gradient norms per tensor and, behind
 * them, the tensors' partial L2 losses; written by edet_opt_l2_norms, summed in a fixed order by
 * edet_opt_clip_factors (large tensors are processed by up to EDET_OPT_SPLIT workgroups).  */
#define EDET_OPT_SPLIT 16
int edet_opt_l2_norms(float* grads, const float* params, const int64_t* seg_offsets,
                      const int32_t* seg_flags, int nseg, float weight_decay,
                      float* seg_sqnorm, void* stream);
/* seg_factor[s] = clip_by_norm factor * clip_by_global_norm factor; global_norm_out = norm after clipping;
 * l2_sum[0] += the L2 loss (either may be NULL) */
int edet_opt_clip_factors(const float* seg_sqnorm, int nseg, float clip_norm,
                          float* seg_factor, float* global_norm_out, float* l2_sum, void* stream);
/* grads[s] *= seg_factor[s]  (data-parallel path: clip locally, then all-reduce, train_lib.py:675-683) */
int edet_opt_scale(float* grads, const int64_t* seg_offsets, const float* seg_factor,
                   int nseg, void* stream);
/* hyper_dev = device float[2] {learning_rate, ema_decay}; seg_factor may be NULL (already scaled);
 * ema may be NULL; seg_flags may be NULL (no frozen variables).  v = momentum*v - lr*g; w += v;
 * ema -= (1-decay)*(ema - w); segments flagged EDET_SEG_FROZEN are skipped.  */
int edet_opt_sgd_ema(float* params, float* grads, float* velocity, float* ema,
                     const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                     const float* hyper_dev, float momentum, void* stream);
/* optimizer = 'adam' (train_lib.py:183-186: tf.keras.optimizers.Adam(learning_rate, beta_1=momentum), beta_2 0.999,
 * epsilon 1e-7): m, v = the two slot arenas; hyper_dev[0] = alpha_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) of THIS step
 * (formed by the host: Engine.set_hyper), hyper_dev[1] = EMA decay; clip factors, frozen segments and the EMA as above */
int edet_opt_adam_ema(float* params, const float* grads, float* m, float* v, float* ema,
                      const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                      const float* hyper_dev, float beta1, float beta2, float epsilon, void* stream);
/* tf.keras.optimizers.RMSprop(lr, rho, momentum, epsilon) as efficientnetv2/main_tf2.py:49-52 builds it (0.9, 0.9, 0.001;
 * the V2 default, hparams.py:249), TensorFlow's ApplyRMSProp form with momentum: ms += (1 - rho)(g^2 - ms);
 * mom = momentum * mom + lr * g / sqrt(ms + epsilon); w -= mom.  ms, mom = the two slot arenas (both start at zero, Keras
 * add_slot); hyper_dev[0] = learning rate, hyper_dev[1] = EMA decay; clip factors, frozen segments and the optional EMA shadow
 * as for edet_opt_adam_ema (ema == NULL: the reference's TF2 trainer has none).  Stated from TensorFlow's documented
 * kernel, not run against it: the numpy restatement in tests/test_effnetv2_train.py is what pins it. */
int edet_opt_rmsprop_ema(float* params, const float* grads, float* ms, float* mom, float* ema,
                         const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                         const float* hyper_dev, float rho, float momentum, float epsilon, void* stream);
/* Lion (lion/lion_tf2.py:60-74, _resource_apply_dense; defaults beta_1 0.9, beta_2 0.99, wd 0): c = m*beta1 + g*(1 - beta1);
 * w -= lr*(sign(c) + w*wd), from the OLD m; m = m*beta2 + g*(1 - beta2).  m = the one slot arena (the SGD velocity's);
 * hyper_dev[0] = the step's learning rate as the schedule gives it (no bias correction), hyper_dev[1] = EMA decay; clip factors,
 * frozen segments and the optional EMA shadow as above.  Every product and sum is one rounded float32 operation (no FMA, the
 * EMA tail included), sign(0) = 0, sign(NaN) = NaN: tests/lion_ref.py restates it in numpy bit for bit. */
int edet_opt_lion_ema(float* params, const float* grads, float* m, float* ema,
                      const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                      const float* hyper_dev, float beta1, float beta2, float wd, void* stream);

/* ---- step plumbing (round 6): the few operations of a step that are not layers, so that EVERY launch of a step goes
 * through this ABI and a step can be recorded and replayed without the Python interpreter (include/edet_net.h).
 * edet_zero: the start-of-step clears of the accumulation targets and the gradient arena (Engine._begin).
 * edet_axpy_clear: dst += src, then src = 0 when clear_src -- the side chain's gradient arena joined into the main one
 *   (Engine._join_side).
 * edet_loss_normalizer: inv_out[0] = 1 / (sum(mean_num_positives[0..n)) + 1), the per-step loss normalizer of
 *   tf2/train_lib.py:517-534 (positives_momentum = 0) kept on the device.  */
int edet_zero(void* dst, size_t bytes, void* stream);
/* dst [rows][c] = the first c elements of every row of src [rows][ld]: the level outputs without their padding columns, as
 * tf2/postprocess.py's reshape to [B, -1, num_classes] / [B, -1, 4] (:67-79) needs them (what `.contiguous()` did on the
 * Python host); rows of whole 4-byte words */
int edet_compact_rows(const void* src, int64_t rows, int c, int ld, void* dst, int elem_bytes, void* stream);
/* dst[i] = (float)src[i]: the fp32 copy of a stored tensor in front of a layer that runs in fp32 inside a bf16 network (the
 * box-predict island of the inference pass, Engine._to_f32); exact (bf16 -> fp32 widens) */
int edet_cast_to_f32(const void* src, float* dst, int64_t count, int src_dtype, void* stream);
int edet_axpy_clear(float* dst, float* src, int64_t n, int clear_src, void* stream);
int edet_loss_normalizer(const float* mean_num_positives, int n, float* inv_out, void* stream);

/* ---- detection post-processing -------------------------------
 * tf2/postprocess.py: merge_class_box_level_outputs :67-79, topk_class_boxes :82-117, pre_nms :120-157, nms :160-206,
 * clip_boxes :61-64, postprocess_global :375-406, per_class_nms :409-467; nms_np.py: hard_nms :84-120, soft_nms
 * :123-184, per_class_nms :214-265; tf2/anchors.py decode_box_outputs :30-58.
 *
 * edet_pre_nms: cls_levels[l] / box_levels[l] are the network outputs of level l, [batch][level_pixels[l]]
 * [anchors_per_pixel * num_classes] and [...][anchors_per_pixel * 4] (HOST arrays of DEVICE pointers); anchor_boxes
 * = the [N][4] fp32 anchors (ymin, xmin, ymax, xmax) in the order of anchors.Anchors.boxes.  Per anchor: the first
 * maximum class, sigmoid of its logit, the decoded box.  Outputs boxes [batch][N][4], scores [batch][N] fp32,
 * classes [batch][N] int32.  The first call for a given pyramid geometry uploads a (level, first anchor) table of a
 * few KB that stays cached on the device for the life of the process (one hipMalloc + one stream synchronisation);
 * every later call only launches.
 * edet_pre_nms_topk: the nms_configs.max_nms_inputs = k > 0 branch: the k largest (anchor, class) logits of every
 * image in descending order (ties: lower flat index), outputs [batch][k]...; k <= 8192.  */
int edet_pre_nms(const void* const* cls_levels, const void* const* box_levels, const int* level_pixels,
                 int nlevels, int batch, int anchors_per_pixel, int num_classes, const float* anchor_boxes,
                 int dtype, float* boxes, float* scores, int* classes, void* stream);
int edet_pre_nms_topk_workspace_bytes(int batch, int k, size_t* bytes);
int edet_pre_nms_topk(const void* const* cls_levels, const void* const* box_levels, const int* level_pixels,
                      int nlevels, int batch, int anchors_per_pixel, int num_classes, const float* anchor_boxes,
                      int dtype, int k, void* workspace, size_t workspace_bytes, float* boxes, float* scores,
                      int* classes, void* stream);

#define EDET_NMS_HARD 0
#define EDET_NMS_GAUSSIAN 1
#define EDET_NMS_LINEAR 2      /* nms_np.py only */
#define EDET_NMS_TF_V5 0       /* tf.raw_ops.NonMaxSuppressionV5: IoU on the corner extents, `score > score_thresh`
                                  filter up front, a decayed score <= score_thresh drops the candidate, sigma =
                                  soft_nms_sigma (= nms_configs.sigma / 2, postprocess.py:193-201) */
#define EDET_NMS_NUMPY 1       /* nms_np.py: pixel-inclusive extents (+1), no filter up front, a decayed score
                                  < score_thresh drops the candidate, weight exp(-iou^2 / sigma); hard = hard_nms */
typedef struct edet_nms_cfg {
  int method, convention;
  float iou_thresh, score_thresh, sigma;
  int max_output_size;
} edet_nms_cfg_t;
/* boxes [batch][n][4], scores [batch][n], classes [batch][n] (may be NULL when segments == 1).  segments == 1:
 * one suppression per image over all candidates (postprocess_global); segments == num_classes: one per (image,
 * class), merged per image to the max_output_size best by score (postprocess.per_class_nms, nms_np.per_class_nms).
 * out_index [batch][max_output_size]: index of the selected candidate or -1 (padding row), out_score: its decayed
 * score (0 for padding), out_valid [batch]: number of selected rows.  */
int edet_nms_workspace_bytes(int batch, int n, int segments, int max_output_size, size_t* bytes);
int edet_nms(const float* boxes, const float* scores, const int* classes, int batch, int n, int segments,
             const edet_nms_cfg_t* cfg, void* workspace, size_t workspace_bytes, int* out_index,
             float* out_score, int* out_valid, void* stream);
#define EDET_NMS_PAD_INDEX0 0  /* padding rows gather candidate 0 (tf.gather on the zero-padded indices), score 0 */
#define EDET_NMS_PAD_ZERO 1    /* padding rows are zeros (tf.pad in per_class_nms) */
#define EDET_NMS_PAD_DUMMY 2   /* padding rows are zeros with score -1e5 (nms_np._generate_dummy_detections) */
/* nms_boxes [batch][M][4] = boxes of the selected candidates, clipped to [0, clip_h] x [0, clip_w] when clip_h > 0
 * and multiplied by image_scales[b] when given; nms_classes = class + 1 (CLASS_OFFSET) as float.  */
int edet_nms_gather(const float* boxes, const int* classes, const int* out_index, const float* out_score,
                    int batch, int n, int max_output_size, int pad_mode, float clip_h, float clip_w,
                    const float* image_scales, float* nms_boxes, float* nms_scores, float* nms_classes,
                    void* stream);

/* ---- anchor labelling -------------------------------------------
 * tf2/anchors.py AnchorLabeler.label_anchors :215-250 for a batch of images.  anchor_boxes [N][4] as for
 * edet_pre_nms; level_anchors[l] = anchors of level l (H_l * W_l * A); gt_boxes [batch][max_gt][4] (ymin, xmin, ymax,
 * xmax), gt_labels [batch][max_gt] (1-based class ids), gt_count [batch] valid rows per image (device arrays).
 * Outputs per level (HOST arrays of DEVICE pointers): cls_targets[l] int32 [batch][H_l][W_l][A] (class - 1, -1 =
 * background), box_targets[l] fp32 [batch][H_l][W_l][4A]; num_positives fp32 [batch].  */
int edet_label_anchors_workspace_bytes(int batch, int num_anchors, size_t* bytes);
int edet_label_anchors(const float* anchor_boxes, const int* level_anchors, int nlevels, const float* gt_boxes,
                       const int* gt_labels, const int* gt_count, int batch, int max_gt, float match_threshold,
                       void* workspace, size_t workspace_bytes, int* const* cls_targets, float* const* box_targets,
                       float* num_positives, void* stream);

/* ---- inference image preprocessing ----------------------------------
 * efficientdet_keras.py:920-951 (mode 'infer'): raw_images [batch][height][width][3] uint8 (raw_is_float = 0) or
 * float32 (1) on the device, all of one size; out [batch][out_height][out_width][3] in `dtype`: normalised with
 * mean_rgb / stddev_rgb (HOST arrays of 3), aspect-preserving bilinear resize into the top-left corner, zero padding.
 * *image_scale_to_original (HOST) = 1 / scale, the factor that maps detections back to the raw image.  */
int edet_preprocess_infer(const void* raw_images, int raw_is_float, int batch, int height, int width,
                          int out_height, int out_width, const float* mean_rgb, const float* stddev_rgb, void* out,
                          float* image_scale_to_original, int dtype, void* stream);
/* The same on a CANVAS batch, every image at its own size (infer_lib.py:219-235 runs the input processor per image):
 * raw_images [batch][canvas_h][canvas_w][3]; image b is the top-left sizes_dev[b] = {height, width} of its slot (int32
 * [batch][2], DEVICE memory, clamped in the kernel into [1, canvas_h] x [1, canvas_w]), its row pitch canvas_w.  scaled_dev
 * [batch][2] = {scaled_h, scaled_w} (int32, DEVICE memory, clamped into [1, out_height] x [1, out_width]): the size image b
 * is resized to, the caller's set_scale_factors_to_output_size of that image's own size; the scales back to the raw images
 * stay with the caller, who made them from the same values.  The resize ratio and the tap clamps use the image's own size, so
 * nothing outside the image is read.  out is written whole, zeros included: image b is what edet_preprocess_infer gives for
 * that image alone, bit for bit.  out_mirrored, when not NULL (and not out), receives the same batch mirrored along the
 * PADDED width, out_mirrored[b][y][out_width - 1 - x] = out[b][y][x], every pixel computed once and stored twice: the
 * second network input of flip test-time augmentation.  batch <= 65535.  */
int edet_preprocess_infer_canvas(const void* raw_images, int raw_is_float, int batch, int canvas_h, int canvas_w,
                                 const int32_t* sizes_dev, const int32_t* scaled_dev, int out_height, int out_width,
                                 const float* mean_rgb, const float* stddev_rgb, void* out, void* out_mirrored, int dtype,
                                 void* stream);


/* ---- training image + box preprocessing --------------------------------
 * dataloader.py DetectionInputProcessor as InputReader.process_example drives it in training (:321-336): normalize_image
 * :58-64, random_horizontal_flip :150-153 (object_detection/preprocessor.py:113-199), set_training_random_scale_factors
 * :66-111, resize_and_crop_image :126-139, resize_and_crop_boxes :165-189 (clip_boxes :155-163, zero-area filter).
 * The random draws and the float32 scale arithmetic of set_training_random_scale_factors stay with the caller, who
 * hands over five integers per image (DEVICE array): flip decision, size of the resized image, crop offset.
 * raw_images as for edet_preprocess_infer.  boxes_in [batch][max_boxes][4] normalised (ymin, xmin, ymax, xmax),
 * classes_in [batch][max_boxes] float, counts_in [batch] valid rows; outputs: the kept boxes in pixels of the output
 * image and their classes IN ORDER, rows past counts_out[b] filled with -1 (dataloader.pad_to_fixed_size).  max_boxes
 * = 0 skips the box part (all box pointers may be NULL).  */
typedef struct edet_prep_image {
  int flip, scaled_h, scaled_w, offset_y, offset_x;
} edet_prep_image_t;
int edet_preprocess_train(const void* raw_images, int raw_is_float, int batch, int height, int width,
                          int out_height, int out_width, const float* mean_rgb, const float* stddev_rgb,
                          const edet_prep_image_t* per_image_dev, void* out, const float* boxes_in,
                          const float* classes_in, const int* counts_in, int max_boxes, float* boxes_out,
                          float* classes_out, int* counts_out, int dtype, void* stream);
/* The same on a CANVAS batch: raw_images [batch][canvas_h][canvas_w][3]; image b is the top-left sizes_dev[b] = {height,
 * width} of its slot (int32 [batch][2], DEVICE memory, clamped in the kernel into [1, canvas_h] x [1, canvas_w]), its row
 * pitch canvas_w.  The resize ratio, the tap clamps and the mirrored tap width - 1 - x use the image's own size, so nothing
 * outside the image is read; the per-image rows are the caller's, made from that size.  out is written whole, as above:
 * image b is what the dense call gives for that image alone, bit for bit. */
int edet_preprocess_train_canvas(const void* raw_images, int raw_is_float, int batch, int canvas_h, int canvas_w,
                                 const int32_t* sizes_dev, int out_height, int out_width, const float* mean_rgb,
                                 const float* stddev_rgb, const edet_prep_image_t* per_image_dev, void* out,
                                 const float* boxes_in, const float* classes_in, const int* counts_in, int max_boxes,
                                 float* boxes_out, float* classes_out, int* counts_out, int dtype, void* stream);

/* ---- ground truth of an evaluation batch (dataloader.py:344-353, :389) ----------------------------------------------------
 * boxes [batch][max_boxes][4], classes [batch][max_boxes], kept_counts [batch]: what edet_preprocess_train leaves (the kept
 * boxes in pixels of the output image, compacted, classes padded with -1).  is_crowds, areas fp32 [batch][max_boxes] and
 * counts [batch]: the caller's annotations as given.  image_scales [batch] = image_scale_to_original.  All DEVICE memory.
 * groundtruth_data fp32 [batch][max_instances][7], rows {y1, x1, y2, x2, is_crowd, area, class}: a coordinate is one rounded
 * fp32 product with the scale; box and class columns of the rows at or past kept_counts[b] are -1; is_crowd is 0 and area -1
 * at or past counts[b].  As the reference is written: the zero-area filter drops boxes with their classes but not their
 * is_crowd / area, so behind a dropped box columns 4-5 of a row belong to another annotation than columns 0-3 and 6.  Both
 * counts are clamped to [0, max_boxes]; max_instances >= max_boxes.  One thread per row.  Restated in tests/det_eval_ref.py,
 * compared bit for bit.  */
int edet_pack_groundtruth(const float* boxes, const float* classes, const int32_t* kept_counts, const float* is_crowds,
                          const float* areas, const int32_t* counts, const float* image_scales, int batch, int max_boxes,
                          int max_instances, float* groundtruth_data, void* stream);

/* ---- GridMask of a training batch (efficientdet/aug/gridmask.py:22-136) ------------------------
 * src, dst uint8 [batch][height][width][3], src != dst.  Per image (DEVICE array): apply != 0 -> dst = src * mask, else the
 * copy.  The S x S mask of the reference (S = size) is never stored; every output pixel (y, x) evaluates it at mask
 * position (Y, X) = (y + (S - height) / 2, x + (S - width) / 2), floor divisions (crop, :58-63):
 *   stripes (:92-102)   m[r][c] = stripe(r; s1) | stripe(c; s2), stripe(t; s) = 1 iff 0 <= t < S, q = t - s >= 0,
 *                       q / d < S / d (integer divisions) and q % d < l.  1 = kept: the image survives on the stripes.
 *   rotation (:50-55)   ImageProjectiveTransformV2, BILINEAR, constant fill 0, on int32: source position
 *                       (coef[0] X + coef[1] Y + coef[2], coef[3] X + coef[4] Y + coef[5]) in fp32, left to right; the
 *                       low taps are floor(), the high taps floor() + 1, each 0 outside [0, S); row blend
 *                       (x_ceil - x) v00 + (x - x_floor) v01, the column blend likewise; the result truncated to int32.
 * The caller makes the draws and the coefficients (automl_amd/gridmask.py: sine and cosine are numpy float32 on the host).
 * Every field is clamped in the kernel: size into [0, 2^30], d >= 1, l into [0, d], s1 and s2 into [0, d]; a source
 * position that is not finite, or whose four taps all lie outside the mask, gives 0.  The arithmetic (single fp32
 * operations in the stated order) is restated in tests/gridmask_ref.py and compared bit for bit.
 * batch <= 65535, height * width * 3 < 2^31. */
typedef struct edet_gridmask_image { /* 48 bytes, one per image, read from DEVICE memory */
  int32_t apply;                 /* the occurrence draw (:116)                                          */
  int32_t size;                  /* S, the side of the square mask (:70-73)                             */
  int32_t d, l;                  /* gridblock and length (:76-90)                                       */
  int32_t s1, s2;                /* the two stripe starts: s1 lands on rows, s2 on columns (:92-102)    */
  float coef[6];                 /* angles_to_projective_transforms of the drawn angle on an S x S image */
} edet_gridmask_image_t;
int edet_gridmask(const uint8_t* src, uint8_t* dst, int batch, int height, int width,
                  const edet_gridmask_image_t* per_image_dev, void* stream);
/* The same on a CANVAS batch: src, dst [batch][canvas_h][canvas_w][3]; image b is the top-left sizes_dev[b] = {height,
 * width} of its slot (int32 [batch][2], DEVICE memory, clamped in the kernel into [1, canvas_h] x [1, canvas_w]), its row
 * pitch canvas_w.  The crop corner (S - height) / 2, (S - width) / 2 is the image's own (S is per row already).  Nothing
 * outside the rectangle is read and dst is written INSIDE it only: the rest of a dst slot is left as it was (nothing
 * downstream reads it).  The grid is sized from the canvas; the dword path is chosen per image, where width % 4 == 0,
 * canvas_w % 4 == 0 and src / dst are 16-byte aligned.  batch <= 65535, canvas_h * canvas_w * 3 < 2^31. */
int edet_gridmask_canvas(const uint8_t* src, uint8_t* dst, int batch, int canvas_h, int canvas_w, const int32_t* sizes_dev,
                         const edet_gridmask_image_t* per_image_dev, void* stream);

/* ---- box-aware AutoAugment / RandAugment of the detector's input (efficientdet/aug/autoaugment.py) ----------------------
 * The image operations are edet_randaug_stats / edet_randaug_apply above; the two calls here make the boxes follow and write
 * what those read.  Per layer and image the caller gives, in DEVICE memory: policy int32 [batch], the reference's operation
 * (NAME_TO_FUNC, :1350-1372): 0 AutoContrast, 1 Equalize, 2 Posterize, 3 Solarize, 4 SolarizeAdd, 5 Color, 6 Contrast,
 * 7 Brightness, 8 Sharpness, 9 Cutout, 10 BBox_Cutout, 11 Rotate_BBox, 12 TranslateX_BBox, 13 TranslateY_BBox, 14 ShearX_BBox,
 * 15 ShearY_BBox, anything else = none; and ops / iargs / fargs in edet_randaug_apply's layout, with the apply id of the
 * image kernel: *_BBox -> Rotate / Translate / Shear with the host-made coefficients, Cutout and BBox_Cutout -> Cutout,
 * Contrast -> 16 (copy) until edet_autoaug_contrast_lut has made its table.  Launch order of one layer:
 * edet_autoaug_boxes, edet_randaug_stats, edet_autoaug_contrast_lut, edet_randaug_apply.
 * edet_autoaug_boxes: boxes, boxes_out fp32 [batch][max_boxes][4] normalised (ymin, xmin, ymax, xmax), the same buffer or
 * two, 16-byte aligned; rows at or past counts[b] are copied.  Rotate_BBox reads cos = fargs[0], sin = fargs[3] (no
 * trigonometry on the device), TranslateX/Y_BBox the pixels fargs[2] / fargs[5], ShearX/Y_BBox the level fargs[1] / fargs[3]:
 * _rotate_bbox (:785-835), _shift_bbox (:881-919), _shear_bbox (:978-1025), _clip_bbox and _check_bbox_area with delta 0.05
 * (:435-483) in fp32 -- to_int32 truncates, every entry of the 2 x 4 matrix product is two rounded products and one rounded
 * add, one rounded division.  BBox_Cutout leaves the boxes alone and writes the rectangle of _cutout_inside_bbox
 * (:1245-1281) into the image's iargs row {lower, left, height - upper, width - right}: dargs fp64 [batch][4] = {pad_fraction,
 * box draw, centre draw y, centre draw x}, draws in [0, 1); the box is int(u count), a centre lo + int(u (hi + 1 - lo)), the
 * pad sizes int(pad_fraction * (extent / 2)) in fp64; counts[b] == 0: the empty rectangle (:1344).
 * edet_autoaug_contrast_lut: for the images whose policy is Contrast (:267-280) the grey levels (the rgb_to_grayscale of
 * Color) are summed as integers, mean = fp32(sum) / fp32(height width) clipped and truncated to uint8, luts[b][c][v] =
 * blend(mean, v, fargs[b][6]) and ops[b] = 1, the table look-up of edet_randaug_apply.  Beyond a grey sum of 2^24 this exact
 * sum is the definition (reduce_mean's summation order is not).  Restated in tests/det_autoaug_ref.py, compared bit for bit. */
int edet_autoaug_boxes(const float* boxes, float* boxes_out, const int32_t* counts, int batch, int max_boxes, int height,
                       int width, const int32_t* policy, int32_t* iargs, const float* fargs, const double* dargs, void* stream);
int edet_autoaug_contrast_lut(const uint8_t* src, int batch, int height, int width, const int32_t* policy, int32_t* ops,
                              const float* fargs, uint8_t* luts, void* stream);
/* The same two on a CANVAS batch (edet_randaug_stats_canvas above): H and W of the box arithmetic, BBox_Cutout's rectangle
 * and the divisor of Contrast's mean are sizes_dev[b] = {height, width} (int32 [batch][2], DEVICE memory).  The boxes are
 * normalised, so edet_autoaug_boxes_canvas needs no canvas: it clamps a size into [1, 2^24 - 1], what the dense call accepts.
 * edet_autoaug_contrast_lut_canvas clamps into [1, canvas_h] x [1, canvas_w] and sums the image's own pixels only. */
int edet_autoaug_boxes_canvas(const float* boxes, float* boxes_out, const int32_t* counts, int batch, int max_boxes,
                              const int32_t* sizes_dev, const int32_t* policy, int32_t* iargs, const float* fargs,
                              const double* dargs, void* stream);
int edet_autoaug_contrast_lut_canvas(const uint8_t* src, int batch, int canvas_h, int canvas_w, const int32_t* sizes_dev,
                                     const int32_t* policy, int32_t* ops, const float* fargs, uint8_t* luts, void* stream);

/* ---- COCO box AP / AR of an evaluator state (efficientdet/coco_metric.py; COCOeval for iouType 'bbox') ----------------------
 * The images of the state in ascending image id, padded: dets fp32 [n_images][max_dets][6] rows {x, y, width, height, score,
 * class}, gts fp32 [n_images][max_gts][7] rows {x, y, width, height, is_crowd (0 or 1), area, class}; a row whose class is not
 * > -1 is padding.  Classes are compared as the fp32 values they are.  1 <= max_dets <= 100, 1 <= max_gts <= 128.
 * edet_coco_match (one wave per image, lanes = the 40 (area range, IoU threshold) pairs): rank int32 [n_images][max_dets], the
 * row's position among the kept rows of its image and class by descending score, equal scores in row order, -1 for padding;
 * matched, ignored uint16 [n_images][4][max_dets], bit t = IoU threshold t.  iou_thrs fp64 [10], area_rng fp64 [4][2] {lo, hi}
 * in DEVICE memory.  IoU in fp64 from the fp32 values: w = min(d.x + d.w, g.x + g.w) - max(d.x, g.x), 0 if w <= 0, h likewise,
 * i = w h, u = d.w d.h for a crowd, else (d.w d.h + g.w g.h) - i, iou = i / u.  A ground truth is ignored in an area range when
 * it is a crowd or its area is < lo or > hi; per threshold the rows are visited by descending score, best = min(t, 1 - 1e-10),
 * the ground truths of the row's class not ignored first, then ignored, each in row order: skip one already matched unless a
 * crowd, stop at an ignored one once a not ignored one is held, skip iou < best, else take it (an equal IoU replaces).  A
 * matched row inherits the ground truth's ignore flag; an unmatched row is ignored when fp32(width height) is < lo or > hi.
 * edet_coco_accumulate (one workgroup per (category, area range, cap, threshold)): perm int32 [n_images max_dets] = the rows
 * ordered by (category, descending score, image, rank), seg int32 [n_cats + 1] = where each category starts in perm, npig int32
 * [n_cats][4] = the not ignored ground truths, caps int32 [3] = maxDets, rec_thrs fp64 [101], all DEVICE memory.  precision
 * fp64 [10][101][n_cats][4][3] and recall fp64 [10][n_cats][4][3] are the caller's, pre-set to -1: a cell with npig = 0 is
 * left alone.  tp = matched & ~ignored and fp = ~matched & ~ignored of the rows with rank < cap, summed as integers along the
 * segment; rc = tp / npig, pr = tp / ((fp + tp) + 2^-52), pr made non-increasing from the right; recall = the last rc,
 * precision[r] = pr at the first row with rc >= rec_thrs[r], 0 past the end.  No atomics; the same bits on every run.
 * Restated in tests/coco_ref.py and compared bit for bit.  n_images * max_dets < 2^29. */
#define EDET_COCO_THRS 10
#define EDET_COCO_RECS 101
#define EDET_COCO_AREAS 4
#define EDET_COCO_CAPS 3
#define EDET_COCO_MAX_DETS 100
#define EDET_COCO_MAX_GTS 128
int edet_coco_match(const float* dets, const float* gts, int n_images, int max_dets, int max_gts, const double* iou_thrs,
                    const double* area_rng, int32_t* rank, uint16_t* matched, uint16_t* ignored, void* stream);
int edet_coco_accumulate(const int32_t* perm, const int32_t* seg, const int32_t* rank, const uint16_t* matched,
                         const uint16_t* ignored, const int32_t* npig, int n_images, int max_dets, int n_cats,
                         const double* rec_thrs, const int32_t* caps, double* precision, double* recall, void* stream);

/* ---- weighted box fusion of the detections of several passes (efficientdet/tf2/wbf.py:70-95) ------------------------------
 * dets fp32 [batch][rows][7], rows {image id, x1, y1, x2, y2, score, class} (the corner form of generate_detections), counts
 * int32 [batch] = the rows of each image that count (NULL: all; clamped to 0..rows), 1 <= rows <= 1024, num_models >= 1.
 * Finite coordinates and scores only.
 * edet_wbf_cluster (one wave per (image, class)): for cid in 0 .. num_classes - 1 the rows with class == (float)cid, in input
 * order; any other class value is dropped.  A row founds a cluster when its class has none yet or when the largest IoU with the
 * clusters' current averages is < 0.55f; else it joins the cluster of that IoU, the lowest index among equals.  A NaN IoU (0 / 0:
 * two boxes without area) is not below 0.55 and beats every number, the lowest such index first (numpy's max / argmax).  IoU in
 * fp32: xa = max(x11, x21), ya, xb = min(x12, x22), yb likewise, inter = max(xb - xa, 0) max(yb - ya, 0), iou = inter /
 * ((area_a + area_b) - inter).  Per cluster five running fp32 sums that start at +0 and take the members in order: x1 s, y1 s,
 * x2 s, y2 s (each product rounded, then added) and s; the average of a coordinate is its sum / the sum of s.  When the class
 * is done the cluster's row {image id of the first member, the four averages, (sum of s / (float)n) * (float)min(1, (double)n
 * / num_models), class of the first member} is written to scratch fp32 [batch][rows][7] at the row of its first member and
 * flags int32 [batch][rows] is set to 1 there.  flags must be ZERO on entry; scratch need not be initialised.  No atomics.
 * edet_wbf_order (one workgroup per image): the flagged rows of scratch by descending score, equal scores by (class, row)
 * ascending -- rank = the number of flagged rows ahead, by counting -- written densely to fused fp32 [batch][rows][7]; the rows
 * at or past fused_counts[b] (int32 [batch], the number of clusters) are zero.
 * Restated in tests/wbf_ref.py and compared bit for bit. */
#define EDET_WBF_MAX_ROWS 1024
int edet_wbf_cluster(const float* dets, const int32_t* counts, int batch, int rows, int num_classes, int num_models,
                     float* scratch, int32_t* flags, void* stream);
int edet_wbf_order(const float* scratch, const int32_t* flags, int batch, int rows, float* fused, int32_t* fused_counts,
                   void* stream);

/* ---- baseline JPEG decode (tf.io.decode_jpeg / decode_image(channels=3): object_detection/tf_example_decoder.py:57,
 * inference.py:63, tf2/train_lib.py:258, efficientnetv2/preprocessing.py:142, efficientnetv2/datasets.py:328,502) ----------
 * libjpeg's default decoder -- the integer-accurate inverse DCT (jidctint.c), fancy chroma upsampling (jdsample.c), YCbCr ->
 * RGB (jdcolor.c) -- split in two: the serial entropy stage on the HOST (csrc/jpeg_host.cpp: plain C++, no device call, the
 * only entry points of this header that take host pointers and block), everything behind it on the device (csrc/jpeg.hip).
 * Decoded are 8-bit Huffman streams of SOF0 / SOF1 with one interleaved scan: one component, or three (YCbCr) whose chroma
 * is sampled 1x1 and whose luma is 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0).  Everything else is a status, never a guess.
 * Restated in tests/jpeg_ref.py; both stages are compared with it, and it with Pillow's libjpeg-turbo, byte for byte. */
#define EDET_JPEG_OK 0
#define EDET_JPEG_PROGRESSIVE 1   /* SOF2                                                                                   */
#define EDET_JPEG_ARITHMETIC 2    /* SOF9 .. SOF11, SOF13 .. SOF15                                                          */
#define EDET_JPEG_PRECISION 3     /* a sample precision other than 8 bits (12-bit files)                                    */
#define EDET_JPEG_COMPONENTS 4    /* neither one component nor three (CMYK / YCCK)                                          */
#define EDET_JPEG_SAMPLING 5      /* sampling factors outside the supported set (4:4:0, 4:1:1, subsampled luma, ...)        */
#define EDET_JPEG_TOO_LARGE 6     /* higher or wider than the canvas                                                        */
#define EDET_JPEG_MALFORMED 7     /* truncated; a bad marker, segment, table, code, restart marker or coefficient index     */
#define EDET_JPEG_UNSUPPORTED 8   /* lossless / hierarchical frames, several or non-interleaved scans, RGB-coded components */
#define EDET_JPEG_KIND_BASELINE 0      /* SOF0 */
#define EDET_JPEG_KIND_EXTENDED 1      /* SOF1: extended sequential, Huffman */
#define EDET_JPEG_KIND_PROGRESSIVE 2   /* SOF2 */
#define EDET_JPEG_KIND_OTHER 3         /* every other frame marker; `sof` tells which */
typedef struct edet_jpeg_info { /* 56 bytes: the frame header and what precedes the first SOS marker */
  int32_t height, width;         /* of the frame; 0 is possible in the file (DNL) and is refused by the decoder            */
  int32_t components;            /* as the frame header says (the arrays below hold the first four)                        */
  int32_t precision;             /* bits per sample                                                                        */
  int32_t kind;                  /* EDET_JPEG_KIND_*                                                                       */
  int32_t restart_interval;      /* of the last DRI segment in front of SOS, 0 = none                                      */
  int32_t sof;                   /* the frame marker's second byte, 0xC0 .. 0xCF                                           */
  int32_t jfif;                  /* 1 if an APP0 JFIF segment was seen                                                     */
  int32_t adobe_transform;       /* the transform byte of an APP14 Adobe segment, -1 if there is none                      */
  int32_t reserved;
  uint8_t h_samp[4], v_samp[4];  /* per component: sampling factors                                                        */
  uint8_t quant_id[4];           /* per component: the quantisation table it names                                         */
  uint8_t comp_id[4];            /* per component: its identifier                                                          */
} edet_jpeg_info_t;
typedef struct edet_jpeg_image { /* 80 bytes, one per image: written by the host stage, read by the kernels from DEVICE memory */
  int32_t status;                /* EDET_JPEG_*; not 0: the other fields are 0 and the image's canvas comes out all zero    */
  int32_t height, width;
  int32_t components;            /* 1 or 3                                                                                 */
  int32_t h_max, v_max;          /* the luma sampling factors, 1 or 2 (chroma is 1x1; one component: 1, 1)                 */
  int32_t blocks_w[3], blocks_h[3]; /* per component: its 8x8-block grid, padded to whole MCUs                             */
  int32_t quant_id[3];           /* per component: row 0 .. 3 of the image's [4][64] quantisation tables                   */
  int32_t first_block[3];        /* per component: where its blocks start in BOTH arenas, in blocks: coefficient element
                                    64 first_block, plane byte 64 first_block.  The components of an image are adjacent.  */
  int32_t total_blocks;          /* of the image: the sum of blocks_w blocks_h                                             */
  int32_t reserved;              /* 0; edet_jpeg_entropy_decode_scaled: the denominator 1, 2, 4 or 8 (height, width: the output) */
} edet_jpeg_image_t;
/* edet_jpeg_info (host): walks the markers of `data` up to the first SOS.  Fails (-1) on a stream without SOI, with a bad
 * segment length, with two frame headers, or that ends before SOS; every read is bounds-checked.
 * edet_jpeg_entropy_decode (host, blocks until done): the Huffman stage of `batch` streams on `threads` worker threads
 * (clamped to 1 .. 16; <= 0: min(16, batch); never derived from the machine's core count).  Per image a descriptor, its
 * status (the descriptor's, repeated in status[batch]) and its quantisation tables uint16 [4][64] in natural order (zero where
 * the file defines none) in qtables_host [batch][4][64]; the coefficients int16, NOT dequantised, 64 per block in natural
 * order, per image and component in raster order over the block grid, densely packed in image order (first_block).  The DC
 * predictor wraps: its low 16 bits are stored.  coef_capacity counts int16 elements; an image that no longer fits gets
 * EDET_JPEG_TOO_LARGE.  A refused image occupies no blocks.  The call itself fails only on a null pointer or batch < 1.
 * edet_jpeg_idct (device, one launch): coef, images, qtables as the host stage wrote them, copied to DEVICE memory; planes
 * uint8, per image and component [blocks_h 8][blocks_w 8] at byte 64 first_block, padding blocks included.  Per block:
 * coefficient x table entry, jidctint.c's column pass, then its row pass (CONST_BITS 13, PASS1_BITS 2; descale by
 * (x + (1 << (s - 1))) >> s with s = 11, then 18), + 128, clamped to 0 .. 255.  All sums, products and left shifts wrap at
 * 32 bits and the right shifts are arithmetic, so a corrupt stream gives the restatement's bytes.  max_blocks >= every
 * image's total_blocks sizes the grid.  plane_capacity is the size of planes in bytes, and coef holds at least as many
 * ELEMENTS: a descriptor that does not lie inside them, or that the host stage could not have written, is treated as refused
 * before anything is read or written.  coef and qtables 16-byte aligned, planes 8-byte aligned.
 * edet_jpeg_color (device, one launch): planes -> raw uint8 [batch][canvas_h][canvas_w][3].  Chroma: h2v1 -- first output
 * of a row in[0], last in[last], even (3 cur + prev + 1) >> 2, odd (3 cur + next + 2) >> 2; h2v2 -- per output row colsum =
 * 3 near + far, far = the chroma row above for the upper output row of a pair and below for the lower, clamped to the
 * ceil(height / 2) real rows; even (3 this + last + 8) >> 4, (4 this + 8) >> 4 at the first column, odd (3 this + next + 7)
 * >> 4, (4 this + 7) >> 4 at the last of the ceil(width / 2) real columns.  R = Y + ((91881 cr + 32768) >> 16), G = Y +
 * ((-22554 cb - 46802 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16), cb and cr minus 128, clamped; one component:
 * R = G = B = Y.  Every canvas pixel outside height x width, and the whole canvas of an image whose status is not 0, is
 * written 0: raw needs no memset and equals v2_preprocessing.pad_batch of the decoded images.  batch <= 65535. */
int edet_jpeg_info(const uint8_t* data, size_t n, edet_jpeg_info_t* out);
int edet_jpeg_entropy_decode(const uint8_t* const* datas, const size_t* sizes, int batch, int canvas_h, int canvas_w,
                             int16_t* coef_host, size_t coef_capacity, edet_jpeg_image_t* images_host,
                             uint16_t* qtables_host, int32_t* status, int threads);
int edet_jpeg_idct(const int16_t* coef, const edet_jpeg_image_t* images_dev, const uint16_t* qtables_dev, int batch,
                   int max_blocks, uint8_t* planes, size_t plane_capacity, void* stream);
int edet_jpeg_color(const uint8_t* planes, const edet_jpeg_image_t* images_dev, int batch, int canvas_h, int canvas_w,
                    size_t plane_capacity, uint8_t* raw, void* stream);

/* ---- JPEG decode at reduced size (tf.io.decode_jpeg's `ratio`; libjpeg's scale_denom 2, 4, 8: jdmaster.c, jidctred.c,
 * jdsample.c) ----------------------------------------------------------------------------------------------------------------
 * The same split and the same arenas as above, through three entry points of their own (csrc/jpeg_host.cpp, csrc/
 * jpeg_scaled.hip); the full-size ones above are untouched.  With denom in {1, 2, 4, 8} and m = 8 / denom the output is
 * ceil(height / denom) x ceil(width / denom), and a block of component c is inverse-transformed to s_c x s_c samples:
 * s_c = m, except the chroma of a 4:2:0 file at m < 8, which is 2 m and then needs no upsampling.  Restated in
 * tests/jpeg_scaled_ref.py, which is compared with Pillow's draft mode (libjpeg-turbo) byte for byte.
 * edet_jpeg_entropy_decode_scaled (host, blocks until done): edet_jpeg_entropy_decode with a denominator per image.  denoms
 * NULL: each image gets the smallest of 1, 2, 4, 8 not above max_denom (itself 1, 2, 4 or 8) whose output fits the canvas;
 * none fits: EDET_JPEG_TOO_LARGE.  denoms int32 [batch]: each image gets denoms[b] (max_denom does not bound it), and an
 * output that does not fit is EDET_JPEG_TOO_LARGE.  The descriptor's height and width are the OUTPUT size and its `reserved`
 * field is the denominator (edet_jpeg_entropy_decode writes 0, which the kernels below read as 1); block grids, first_block,
 * total_blocks, the quantisation tables and every coefficient are the full-size stage's: 64 int16 per block whatever the
 * denominator, so coef_capacity bounds the blocks of the FILES, not of the outputs.  The call fails (-1) on a null pointer,
 * batch < 1, a max_denom or a denoms[b] outside {1, 2, 4, 8}; nothing is written then.
 * edet_jpeg_idct_scaled (device, one launch): edet_jpeg_idct's arguments.  The plane of component c is uint8 [blocks_h s_c]
 * [blocks_w s_c] at byte 64 first_block[c] -- it starts where the full-size plane would and is never longer.  Per block,
 * coefficient x table entry first, then by s_c -- 8: edet_jpeg_idct's transform.  4 (jpeg_idct_4x4): a pass reads entries 0-3
 * and 5-7; t0 = v0 << 14, t2 = 15137 v2 - 6270 v6, t10 = t0 + t2, t12 = t0 - t2, a = -1730 v7 + 11893 v5 - 17799 v3 + 8697 v1,
 * b = -4176 v7 - 4926 v5 + 7373 v3 + 20995 v1, outputs (t10 + b, t12 + a, t12 - a, t10 - b), each (x + (1 << (n - 1))) >> n
 * with n = 12 behind the columns (all but column 4) and 19 behind rows 0-3.  2 (jpeg_idct_2x2): entries 0, 1, 3, 5, 7;
 * t10 = v0 << 15, t0 = -5906 v7 + 6967 v5 - 10426 v3 + 29692 v1, outputs (t10 + t0, t10 - t0), n = 13, then 20.  1: (c0 q0 + 4)
 * >> 3.  Then + 128, clamped to 0 .. 255.  Sums, products and left shifts wrap at 32 bits, right shifts are arithmetic.  A
 * descriptor that fails edet_jpeg_idct's check, whose `reserved` is none of 0, 1, 2, 4, 8, or whose output does not lie inside
 * its reduced planes is treated as refused before anything is read or written.  Alignment as for edet_jpeg_idct.
 * edet_jpeg_color_scaled (device, one launch): edet_jpeg_color's arguments and contract -- the whole canvas is written, zero
 * outside height x width, zero for a refused descriptor.  Chroma is upsampled by (h_max s_0 / s_1, v_max s_0 / s_1) = (1, 1),
 * (2, 1) or (2, 2).  Where that is not (1, 1), edet_jpeg_color's h2v1 / h2v2 formulas apply only if m > 1 AND the component
 * has more than two real columns, ceil(width / 2) of the output; otherwise (jdsample.c) every sample is repeated twice in its
 * row, and every row twice for (2, 2).  Colour conversion as in edet_jpeg_color. */
int edet_jpeg_entropy_decode_scaled(const uint8_t* const* datas, const size_t* sizes, int batch, int canvas_h, int canvas_w,
                                    int max_denom, const int32_t* denoms, int16_t* coef_host, size_t coef_capacity,
                                    edet_jpeg_image_t* images_host, uint16_t* qtables_host, int32_t* status, int threads);
int edet_jpeg_idct_scaled(const int16_t* coef, const edet_jpeg_image_t* images_dev, const uint16_t* qtables_dev, int batch,
                          int max_blocks, uint8_t* planes, size_t plane_capacity, void* stream);
int edet_jpeg_color_scaled(const uint8_t* planes, const edet_jpeg_image_t* images_dev, int batch, int canvas_h, int canvas_w,
                           size_t plane_capacity, uint8_t* raw, void* stream);

/* ---- JPEG decode of a crop window (tf.image.decode_and_crop_jpeg's crop_window = [crop_y, crop_x, crop_height, crop_width];
 * efficientnetv2/preprocess_legacy.py:53-68, 112-125) ------------------------------------------------------------------------
 * The window of an image is, byte for byte, rows y .. y + h - 1 and columns x .. x + w - 1 of what the entry points above
 * decode at the same denominator (1: edet_jpeg_idct / edet_jpeg_color; 2, 4, 8: the *_scaled pair), written at the top-left of
 * the image's canvas slot; nothing is redefined.  The window is in the coordinates of the OUTPUT image, ceil(height / denom) x
 * ceil(width / denom), as in TensorFlow's jpeg_mem, and must lie inside it with h >= 1 and w >= 1.  Only the blocks the window
 * needs are stored, copied and inverse-transformed (csrc/jpeg_host.cpp, csrc/jpeg_window.hip; restated in
 * tests/jpeg_window_ref.py).
 * The kept grid.  Component c is inverse-transformed to s_c x s_c samples per block (above) and then up-sampled by u_x, u_y in
 * {1, 2} (edet_jpeg_color_scaled: luma 1; chroma h_max s_0 / s_c, v_max s_0 / s_c); C_c = ceil(image_w / u_x) and R_c =
 * ceil(image_h / u_y) are its real sample columns and rows.  The samples the window needs along x are [x, x + w - 1] for
 * u_x = 1 and [max(0, (x >> 1) - 1), min(C_c - 1, ((x + w - 1) >> 1) + 1)] for u_x = 2 -- what the fancy formulas read, and
 * used where libjpeg replicates as well; along y alike with R_c.  Blocks are samples / s_c, and the kept grid is the smallest
 * rectangle of whole MCUs (mcu_x0, mcu_y0, mcus_w, mcus_h) that holds these blocks of every component.  A window that is the
 * whole image keeps the whole grid. */
#define EDET_JPEG_WINDOW 9        /* a window outside the output image, or with a side below 1                              */
typedef struct edet_jpeg_window { /* 48 bytes, one per image: written by edet_jpeg_entropy_decode_window, read from DEVICE memory */
  int32_t y, x, h, w;            /* the window, in output pixels; all fields 0 for an image whose status is not 0           */
  int32_t image_h, image_w;      /* the output size of the WHOLE image: the edge rules of the up-sampling use these         */
  int32_t mcu_x0, mcu_y0;        /* the first kept MCU column and row of the file's MCU grid                                */
  int32_t mcus_w, mcus_h;        /* kept MCU columns and rows                                                               */
  int32_t reserved[2];           /* 0                                                                                       */
} edet_jpeg_window_t;
/* edet_jpeg_entropy_decode_window (host, blocks until done): edet_jpeg_entropy_decode_scaled's arguments, windows int32
 * [batch][4] = (y, x, h, w) and windows_host [batch], which it writes.  denoms NULL: every image is decoded at denominator 1
 * (a window is in the coordinates of one denominator, so none is chosen); otherwise denoms[b].  The image descriptor
 * describes the KEPT grid as an image of its own, so that edet_jpeg_idct_scaled runs on it unchanged: blocks_w / blocks_h
 * are the kept blocks per component, first_block / total_blocks count kept blocks only, `reserved` is the denominator, and
 * height / width are the output pixels the kept MCUs cover inside the image.  Coefficients are stored densely per component,
 * in raster order over the kept grid.  Blocks outside it are parsed -- the DC predictors must advance -- and not stored, and
 * parsing STOPS behind the last kept MCU row: damage behind that point is not reported (libjpeg, which reads a file row by
 * row, would never read it either), so a stream that the whole-image entry points call EDET_JPEG_MALFORMED can decode here.
 * Statuses, in this order behind the frame and scan checks: a window outside the output image or with a side below 1 is
 * EDET_JPEG_WINDOW; a window higher or wider than the canvas is EDET_JPEG_TOO_LARGE (the IMAGE may exceed the canvas); an
 * arena that runs out is EDET_JPEG_TOO_LARGE.  The call fails (-1) for what edet_jpeg_entropy_decode_scaled fails for and for
 * null windows or windows_host.  Threads as above.
 * The inverse DCT of a windowed batch is edet_jpeg_idct_scaled on these descriptors.
 * edet_jpeg_color_window (device, one launch whatever the mix of samplings, denominators and windows):
 * edet_jpeg_color_scaled's contract with an origin.  Canvas pixel (r, q) of the slot, r < h and q < w, is image pixel
 * (y + r, x + q); sample (i, j) of component c lies at row i - mcu_y0 v_c s_c, column j - mcu_x0 h_c s_c of its kept plane
 * (h_c, v_c: the component's blocks per MCU).  The first-column, last-column and row-clamp rules of the up-sampling, and the
 * "more than two real columns" rule, use image_h and image_w, not the kept region.  The whole canvas is written: zero outside
 * h x w, zero for a refused descriptor and for a pair of descriptors that the host stage could not have written -- the image
 * descriptor must pass edet_jpeg_color_scaled's check against plane_capacity, and the window descriptor must name a window
 * inside image_h x image_w and the canvas whose needed samples all lie inside the kept planes -- checked before anything is
 * indexed.  windows_dev 4-byte aligned in DEVICE memory; the rest as edet_jpeg_color_scaled. */
int edet_jpeg_entropy_decode_window(const uint8_t* const* datas, const size_t* sizes, int batch, int canvas_h, int canvas_w,
                                    int max_denom, const int32_t* denoms, const int32_t* windows, int16_t* coef_host,
                                    size_t coef_capacity, edet_jpeg_image_t* images_host, edet_jpeg_window_t* windows_host,
                                    uint16_t* qtables_host, int32_t* status, int threads);
int edet_jpeg_color_window(const uint8_t* planes, const edet_jpeg_image_t* images_dev, const edet_jpeg_window_t* windows_dev,
                           int batch, int canvas_h, int canvas_w, size_t plane_capacity, uint8_t* raw, void* stream);

/* ---- JPEG Huffman decode on the device (JpegDecoder(entropy='device')) ---------------------------------------------------
 * The entropy stage moved behind the bus: the host keeps the marker walk and ONE byte-copy pass over each scan
 * (edet_jpeg_scan_prepare, csrc/jpeg_host.cpp), the device decodes the Huffman stream with a self-synchronising parallel
 * decoder (edet_jpeg_entropy_device, csrc/jpeg_entropy.hip) and writes the coefficient arena edet_jpeg_idct[_scaled] read,
 * bit for bit what edet_jpeg_entropy_decode[_scaled] write.  What crosses the bus is the compressed scan, not its
 * coefficients.  The per-unit code is one text for host and device (csrc/jpeg_entropy_impl.h); restated in
 * tests/jpeg_entropy_ref.py.
 * Segments and units.  A SEGMENT is the entropy-coded data of one restart interval (the whole scan without DRI) with the
 * FF 00 stuffing removed, at a 4-byte aligned offset of the scan arena, zero-padded to a whole word.  A UNIT is one
 * subsequence of subseq_bits bits (a multiple of 32 in 64 .. 8192) of one segment; the last may be shorter.
 * The decoder's state at a bit position is (p, b, k): the bit, the block inside the MCU, the zigzag position (0: a DC symbol
 * is next); (0, 0, 0) at a segment's start.  decode_unit(state, unit end) decodes whole symbols until p >= unit end and
 * returns the end state and the blocks completed; an absent code, or one that runs past the segment, stops it at (segment
 * end, 0, 0).  Round 0 decodes every unit from (unit start, 0, 0); in round r a unit whose predecessor's end state differs
 * from the start state it last used decodes again from it; unit 0 of a segment starts from the truth, so after at most
 * `units` rounds every unit starts where the serial decode passes, whatever the speculative units did.  A prefix sum of the
 * completed blocks gives every unit its first block, segment j starts at block j restart_interval blocks_per_mcu, a last pass
 * writes the AC values and the DC differences, and a segmented prefix sum per component (32-bit, wrapping; low 16 bits
 * stored) turns the differences into the host stage's predictors. */
#define EDET_JPEG_TABLES 6          /* derived Huffman tables per image: a DC and an AC table for each of three components */
#define EDET_JPEG_TABLE_BYTES 2512  /* one of them: look uint16 [1024], mincode, count, valptr int32 [17], vals uint8 [256], pad */
#define EDET_JPEG_UNIT_WORDS 8      /* uint32 words of device scratch per unit                                                */
typedef struct edet_jpeg_segment { /* 16 bytes, one per restart interval */
  uint32_t offset;               /* of its first byte in the scan arena, a multiple of 4                                    */
  uint32_t length;               /* in bytes, stuffing removed; below 2^28                                                  */
  uint32_t first_unit;           /* its first unit among the image's units                                                  */
  uint32_t reserved;
} edet_jpeg_segment_t;
typedef struct edet_jpeg_scan { /* 64 bytes, one per image: written by edet_jpeg_scan_prepare, read from DEVICE memory */
  int32_t status;                /* 0; edet_jpeg_entropy_device: EDET_JPEG_MALFORMED for a scan it refused                  */
  int32_t first_segment, segments; /* the image's rows of the segment table: ceil(MCUs / restart_interval), or 1            */
  int32_t first_unit, units;     /* the image's units of the unit scratch; the sum of its segments' units                   */
  int32_t restart_interval;      /* MCUs per segment, 0: one segment                                                        */
  int32_t mcus_w, mcus_h;        /* the file's MCU grid                                                                     */
  int32_t blocks_per_mcu;        /* h_max v_max + 2, or 1                                                                   */
  int32_t dc_table[3], ac_table[3]; /* per component: its slot 0 .. 5 among the image's tables                              */
  int32_t rounds;                /* 0; edet_jpeg_entropy_device: the rounds it ran for this image (round 0 included)        */
} edet_jpeg_scan_t;
/* edet_jpeg_scan_prepare (host, blocks until done; no device call): edet_jpeg_entropy_decode_scaled's streams, canvas,
 * max_denom, denoms, images_host, qtables_host, status and threads, and the same walk, frame check, scan check and Huffman
 * table build, so every header-level refusal comes back here with the status it always had; the descriptors and
 * quantisation tables are those of edet_jpeg_entropy_decode_scaled for the same batch (with max_denom 1 and denoms NULL:
 * edet_jpeg_entropy_decode's, `reserved` 0), first_block placed against coef_capacity (int16 elements of the DEVICE arena)
 * by the same rule.  Then one pass over the entropy-coded bytes per image, in parallel over images: copied into scan_host
 * with the stuffing removed and cut into segments -- a segment ends at an FF that 00 does not follow, fill FFs are skipped,
 * the marker behind segment j must be RST(j mod 8), else EDET_JPEG_MALFORMED; nothing behind the last segment is looked at.
 * An image's room in scan_host is what is left of its file behind SOS plus 4 bytes per segment, rounded up to 16, so
 * placement does not depend on the walk.  scans_host [batch], segments_host [segment_capacity] and tables_host [batch]
 * [EDET_JPEG_TABLES][EDET_JPEG_TABLE_BYTES] (components that name one table share a slot; unused slots zero) are written;
 * an image whose scan, segments or units do not fit scan_capacity (bytes, below 2^31), segment_capacity or unit_capacity is
 * EDET_JPEG_TOO_LARGE.  A refused image has a zero descriptor, zero tables and a zero scan row.  A stream damaged INSIDE a
 * segment is not found here: the device finds it.  used[3] receives the bytes of scan_host, the segments and the units in
 * use.  Fails (-1) for what edet_jpeg_entropy_decode_scaled fails for, a bad subseq_bits or a scan_host not 4-byte aligned.
 * edet_jpeg_entropy_device (device, one launch, one workgroup per image; every wait is a workgroup barrier): the arrays above
 * in DEVICE memory -- scan_dev [scan_bytes], segments_dev [segment_count], tables_dev, scans_dev, images_dev -- -> coef, in
 * the layout and with the values of the host stage: natural order, not dequantised, padding blocks included, the image's
 * block range zeroed first.  units_dev: uint32 [unit_capacity][EDET_JPEG_UNIT_WORDS] scratch; dc_dev: uint16 [coef_capacity
 * / 64] scratch.  An image whose descriptor carries a status is left alone.  A segment that completes fewer blocks than its
 * share -- min(restart_interval, MCUs left) blocks_per_mcu -- makes its image EDET_JPEG_MALFORMED: images_dev[b].status and
 * scans_dev[b].status are set (so the inverse DCT and colour kernels, launched behind this one, zero its canvas slot), its
 * coefficients stay zero.  Blocks a segment decodes behind its share are dropped.  status_dev int32 [batch] receives every
 * image's status.  Nothing is trusted: descriptors, segment rows and table entries are checked against the capacities passed
 * here before they index anything, and an image that fails is EDET_JPEG_MALFORMED.  Loops: a unit decodes at most subseq_bits
 * + 31 symbols; at most `units` rounds; every other loop runs over the image's units, segments, MCUs or blocks.  coef
 * 16-byte aligned, scan_dev and the others 4-byte aligned; batch <= 65535. */
int edet_jpeg_scan_prepare(const uint8_t* const* datas, const size_t* sizes, int batch, int canvas_h, int canvas_w,
                           int max_denom, const int32_t* denoms, size_t coef_capacity, int subseq_bits, uint8_t* scan_host,
                           size_t scan_capacity, edet_jpeg_segment_t* segments_host, size_t segment_capacity,
                           size_t unit_capacity, uint8_t* tables_host, edet_jpeg_scan_t* scans_host,
                           edet_jpeg_image_t* images_host, uint16_t* qtables_host, int32_t* status, size_t* used, int threads);
int edet_jpeg_entropy_device(const uint8_t* scan_dev, size_t scan_bytes, const edet_jpeg_segment_t* segments_dev,
                             size_t segment_count, const uint8_t* tables_dev, edet_jpeg_scan_t* scans_dev,
                             edet_jpeg_image_t* images_dev, int batch, int subseq_bits, uint32_t* units_dev,
                             size_t unit_capacity, uint16_t* dc_dev, int16_t* coef, size_t coef_capacity, int32_t* status_dev,
                             void* stream);

/* ---- TFRecord input (dataloader.py:404-460 reads TFRecord shards of tf.train.Example; object_detection/
 * tf_example_decoder.py:30-169 names the keys) -- HOST only, csrc/tfrecord_host.cpp: plain C++, no device call.  Every input
 * is a (pointer, length) pair into the caller's memory, every output a caller-allocated array with a stated capacity; nothing
 * is allocated for the caller, and a malformed input gives a status without a read outside its buffer.  The formats are
 * read by their specifications (tensorflow/core/lib/io/record_writer.h, core/example/{example,feature}.proto); restated in
 * tests/tfrecord_ref.py.
 * edet_crc32c: CRC-32C (Castagnoli, reflected 0x82f63b78) of data[n] continuing from *crc (0 to begin); slicing by eight.
 * edet_tfrecord_index: walks the framing of buf[nbytes] -- uint64 length (little-endian), uint32 masked CRC of those eight
 * bytes, payload, uint32 masked CRC of the payload; mask(c) = ((c >> 15 | c << 17) + 0xa282ead8) -- and writes each payload's
 * offset and length; verify = 0 skips both CRCs.  Returns an EDET_TFRECORD_* status (-1: a null pointer); *count = records
 * written, *consumed = the offset of the record the status is about, which after EDET_TFRECORD_CAPACITY is where a second
 * call (buf + consumed, nbytes - consumed) goes on, and nbytes after EDET_TFRECORD_OK.  The length is checked before anything
 * is added to it. */
#define EDET_TFRECORD_OK 0
#define EDET_TFRECORD_TRUNCATED_HEADER 1   /* fewer than 12 bytes are left                                                   */
#define EDET_TFRECORD_TRUNCATED_PAYLOAD 2  /* verify: the length's CRC matched, and the payload or its CRC ends behind the buffer */
#define EDET_TFRECORD_LENGTH_CRC 3
#define EDET_TFRECORD_DATA_CRC 4
#define EDET_TFRECORD_LENGTH_RANGE 5       /* verify = 0: a length, checked by nobody, that runs past the buffer            */
#define EDET_TFRECORD_CAPACITY 6           /* `capacity` records are written and another follows, its payload not yet checked */
/* edet_example_parse: n serialized tf.train.Example messages on min(threads, 16, n) worker threads (threads <= 0: 16; never
 * the machine's core count).  Example.features = 1; Features.feature = 1, map entries with key = 1 and value = 2; Feature =
 * oneof bytes_list = 1, float_list = 2, int64_list = 3, each with a repeated value = 1.  spec[nspec] names the wanted keys;
 * values[k] is where key k's values go: EDET_EXAMPLE_BYTES int64 [n][capacity][2] = (offset into the record, length) -- the
 * bytes are not copied --, EDET_EXAMPLE_FLOAT float [n][capacity] (the stored bits), EDET_EXAMPLE_INT64 int64 [n][capacity];
 * counts int32 [n][nspec] is the number of values, -1 for a key the record does not have.  Accepted: packed (wire type 2) and
 * unpacked (5 / 0) repeated scalars, mixed too; unknown fields of any wire type, skipped (a group field by field up to its
 * end tag, at most 32 deep); a repeated map key (the last entry wins); a Feature with no member set (count 0); a member set twice (merged), another member after it (the last
 * wins).  Unwanted features are skipped unread.  status int32 [n] is an EDET_EXAMPLE_* per record; the values and counts of a
 * record whose status is not 0 are unspecified.  The call itself fails (-1) only on its arguments. */
#define EDET_EXAMPLE_BYTES 1
#define EDET_EXAMPLE_FLOAT 2
#define EDET_EXAMPLE_INT64 3
#define EDET_EXAMPLE_OK 0
#define EDET_EXAMPLE_VARINT 1      /* a varint of more than ten bytes, or cut off by the end of its message                  */
#define EDET_EXAMPLE_LENGTH 2      /* a length, a fixed-width value or a packed float list that does not fit its message    */
#define EDET_EXAMPLE_WIRE_TYPE 3   /* a known field with another wire type; an end-group tag that closes nothing; 6 and 7    */
#define EDET_EXAMPLE_CAPACITY 4    /* a list longer than its spec's capacity                                                 */
#define EDET_EXAMPLE_KIND 5        /* a wanted key whose Feature holds another kind of list                                  */
typedef struct edet_example_spec { /* 24 bytes */
  const char* key;                 /* not NUL-terminated: key_len bytes                                                      */
  int32_t key_len;
  int32_t kind;                    /* EDET_EXAMPLE_BYTES / FLOAT / INT64                                                     */
  int32_t capacity;                /* values per record                                                                      */
  int32_t reserved;
} edet_example_spec_t;
int edet_crc32c(const uint8_t* data, size_t n, uint32_t* crc);
int edet_tfrecord_index(const uint8_t* buf, size_t nbytes, int verify, uint64_t* offsets, uint64_t* lengths,
                        size_t capacity, size_t* count, size_t* consumed);
int edet_example_parse(const uint8_t* const* records, const size_t* lengths, int n, const edet_example_spec_t* spec,
                       int nspec, int threads, void* const* values, int32_t* counts, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif  /* EDET_HIP_H_ */
