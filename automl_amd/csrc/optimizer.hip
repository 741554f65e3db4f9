// The parameter-update path of both trainers over a flat fp32 parameter arena: L2 regularisation, per-tensor + global
// gradient clipping, and the SGD-momentum / Adam / RMSprop update with the EMA shadow riding on each.
//
// Reference: efficientdet/tf2/train_lib.py:486-491 (_reg_l2_loss), :675-683 (clip + apply), :176-199 (optimizer).
#include "common.h"

namespace {

constexpr int THREADS = 256;

__device__ __forceinline__ float block_sum(float v, float* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < THREADS / 64; ++i) t += sh[i];
  return t;
}

// Every tensor segment is cut into up to OPT_SPLIT slices of >= 1024 elements, one workgroup per
// (segment, slice): the few large kernels (>100 k elements) no longer serialise on one workgroup, the
// many small tensors still cost one workgroup each, and every reduction keeps a fixed order.
constexpr int OPT_SPLIT = EDET_OPT_SPLIT;

__device__ __forceinline__ bool slice_range(const int64_t* seg_off, int s, int j, int64_t& b, int64_t& e) {
  const int64_t sb = seg_off[s], se = seg_off[s + 1];
  int64_t chunk = ((se - sb + OPT_SPLIT - 1) / OPT_SPLIT + 3) / 4 * 4;
  if (chunk < 1024) chunk = 1024;
  b = sb + (int64_t)j * chunk;
  e = b + chunk < se ? b + chunk : se;
  return b < e;
}

// GRAD = false (k_l2_loss_slices, the evaluation step): the wsq sums alone, in the same order -- the gradient arena is neither
// read nor written, seg_sqnorm is [nseg][OPT_SPLIT] L2 shares
template <bool GRAD>
__device__ __forceinline__ void l2_norms_body(float* grads, const float* params,
                                                     const int64_t* seg_off, const int32_t* seg_flags,
                                                     float wd, float* seg_sqnorm, int nseg) {
  __shared__ float sh[THREADS / 64];
  const int s = blockIdx.x, j = blockIdx.y;
  int64_t b, e;
  const bool any = slice_range(seg_off, s, j, b, e);
  const bool frozen = (seg_flags[s] & EDET_SEG_FROZEN) != 0;
  const bool reg = (seg_flags[s] & EDET_SEG_L2) != 0 && !frozen;
  float gsq = 0.f, wsq = 0.f;
  if (any && frozen) {
    // a frozen variable (config.var_freeze_expr) has no gradient: zeroed here, no share in the norms, skipped by the update
    if (GRAD) {
      for (int64_t i = b + threadIdx.x; i < e; i += THREADS) grads[i] = 0.f;
    }
  } else if (any) {
    if ((b & 3) == 0) {
      const int64_t nv = (e - b) >> 2;
      float4* g4 = GRAD ? reinterpret_cast<float4*>(grads + b) : nullptr;
      const float4* w4 = reinterpret_cast<const float4*>(params + b);
      for (int64_t i = threadIdx.x; i < nv; i += THREADS) {
        float4 g = GRAD ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (reg) {
          const float4 w = w4[i];
          if (GRAD) {
            g.x = fmaf(wd, w.x, g.x); g.y = fmaf(wd, w.y, g.y); g.z = fmaf(wd, w.z, g.z); g.w = fmaf(wd, w.w, g.w);
            g4[i] = g;
          }
          wsq += w.x * w.x + w.y * w.y + w.z * w.z + w.w * w.w;
        }
        if (GRAD) gsq += g.x * g.x + g.y * g.y + g.z * g.z + g.w * g.w;
      }
      b += nv << 2;
    }
    for (int64_t i = b + threadIdx.x; i < e; i += THREADS) {
      float g = GRAD ? grads[i] : 0.f;
      if (reg) {
        const float w = params[i];
        if (GRAD) {
          g = fmaf(wd, w, g);
          grads[i] = g;
        }
        wsq = fmaf(w, w, wsq);
      }
      if (GRAD) gsq = fmaf(g, g, gsq);
    }
  }
  const float tg = GRAD ? block_sum(gsq, sh) : 0.f;
  const float tw = block_sum(wsq, sh);
  if (threadIdx.x == 0) {
    if (GRAD) seg_sqnorm[(size_t)s * OPT_SPLIT + j] = tg;
    // this slice's share of the L2 loss, summed in a fixed order by k_clip_factors (r04: no atomics)
    seg_sqnorm[((size_t)(GRAD ? nseg : 0) + s) * OPT_SPLIT + j] = (any && reg) ? 0.5f * wd * tw : 0.f;
  }
}

__global__ __launch_bounds__(THREADS) void k_l2_norms(float* grads, const float* params,
                                                     const int64_t* seg_off, const int32_t* seg_flags,
                                                     float wd, float* seg_sqnorm, int nseg) {
  l2_norms_body<true>(grads, params, seg_off, seg_flags, wd, seg_sqnorm, nseg);
}
__global__ __launch_bounds__(THREADS) void k_l2_loss_slices(const float* params, const int64_t* seg_off,
                                                           const int32_t* seg_flags, float wd, float* seg_l2, int nseg) {
  l2_norms_body<false>(nullptr, params, seg_off, seg_flags, wd, seg_l2, nseg);
}
// the L2 half of k_clip_factors: the slices' shares added in its order (segments strided over the lanes, a segment's slices
// in order, block_sum), WRITTEN to l2_out[0]
__global__ __launch_bounds__(THREADS) void k_l2_loss_sum(const float* seg_l2, int nseg, float* l2_out) {
  __shared__ float sh[THREADS / 64];
  float l2 = 0.f;
  for (int s = threadIdx.x; s < nseg; s += THREADS) {
#pragma unroll
    for (int j = 0; j < OPT_SPLIT; ++j) l2 += seg_l2[(size_t)s * OPT_SPLIT + j];
  }
  const float l2tot = block_sum(l2, sh);
  if (threadIdx.x == 0) l2_out[0] = l2tot;
}

// tf.clip_by_norm per tensor, then tf.clip_by_global_norm over the clipped tensors
__global__ __launch_bounds__(THREADS) void k_clip_factors(const float* seg_sqnorm, int nseg, float clip,
                                                         float* seg_factor, float* gnorm_out, float* l2_sum) {
  __shared__ float sh[THREADS / 64];
  float acc = 0.f, l2 = 0.f;
  for (int s = threadIdx.x; s < nseg; s += THREADS) {
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < OPT_SPLIT; ++j) {
      sq += seg_sqnorm[(size_t)s * OPT_SPLIT + j];
      l2 += seg_sqnorm[((size_t)nseg + s) * OPT_SPLIT + j];
    }
    const float nrm = sqrtf(sq);
    float f = 1.f;
    if (clip > 0.f) f = clip / fmaxf(nrm, clip);
    seg_factor[s] = f;
    const float cn = nrm * f;
    acc = fmaf(cn, cn, acc);
  }
  const float tot = block_sum(acc, sh);
  const float l2tot = block_sum(l2, sh);
  if (threadIdx.x == 0 && l2_sum) l2_sum[0] += l2tot;
  const float gn = sqrtf(tot);
  float f2 = 1.f;
  if (clip > 0.f) f2 = clip / fmaxf(gn, clip);
  __syncthreads();
  for (int s = threadIdx.x; s < nseg; s += THREADS) seg_factor[s] *= f2;
  if (threadIdx.x == 0 && gnorm_out) gnorm_out[0] = gn * f2;
}

__global__ __launch_bounds__(THREADS) void k_scale(float* grads, const int64_t* seg_off,
                                                  const float* seg_factor) {
  const int s = blockIdx.x;
  int64_t b, e;
  if (!slice_range(seg_off, s, blockIdx.y, b, e)) return;
  const float f = seg_factor[s];
  if ((b & 3) == 0) {
    const int64_t nv = (e - b) >> 2;
    float4* g4 = reinterpret_cast<float4*>(grads + b);
    for (int64_t i = threadIdx.x; i < nv; i += THREADS) {
      float4 g = g4[i];
      g.x *= f; g.y *= f; g.z *= f; g.w *= f;
      g4[i] = g;
    }
    b += nv << 2;
  }
  for (int64_t i = b + threadIdx.x; i < e; i += THREADS) grads[i] *= f;
}

// ---- the parameter update: one walk over a segment's slice (update_walk), whatever the optimizer.  A rule holds its scalars, says how
// many slot arrays it keeps (SLOTS) and updates one element; the TFA MovingAverage shadow (ema -= (1-decay)*(ema - w)) rides
// on every rule.  hyper[0] = the step's learning rate (Adam: bias-corrected by the host), hyper[1] = the EMA decay.
// Keras SGD: v = m*v - lr*g ; w += v
struct SgdRule {
  static constexpr int SLOTS = 1;
  float momentum;
  __device__ __forceinline__ void operator()(float g, float& v, float&, float& w, float& em, float lr, float decay,
                                             bool has_ema) const {
    v = momentum * v - lr * g;
    w += v;
    if (has_ema) em -= (1.f - decay) * (em - w);
  }
};

// tf.keras.optimizers.Adam (ResourceApplyAdam): m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); w -= alpha m / (sqrt(v) + eps)
// with alpha = lr sqrt(1 - b2^t) / (1 - b1^t) formed by the host for this step (hyper[0])
struct AdamRule {
  static constexpr int SLOTS = 2;
  float b1, b2, eps;
  __device__ __forceinline__ void operator()(float g, float& m, float& u, float& w, float& em, float alpha, float decay,
                                             bool has_ema) const {
    m += (g - m) * (1.f - b1);
    u += (g * g - u) * (1.f - b2);
    w -= (m * alpha) / (sqrtf(u) + eps);
    if (has_ema) em -= (1.f - decay) * (em - w);
  }
};

// TensorFlow's ApplyRMSProp with momentum (what tf.keras.optimizers.RMSprop runs): ms += (1 - rho)(g^2 - ms);
// mom = momentum mom + lr g / sqrt(ms + eps); w -= mom
struct RmspropRule {
  static constexpr int SLOTS = 2;
  float rho, momentum, eps;
  __device__ __forceinline__ void operator()(float g, float& ms, float& mom, float& w, float& em, float lr, float decay,
                                             bool has_ema) const {
    ms += (g * g - ms) * (1.f - rho);
    mom = momentum * mom + (lr * g) / sqrtf(ms + eps);
    w -= mom;
    if (has_ema) em -= (1.f - decay) * (em - w);
  }
};

// Lion (lion/lion_tf2.py:60-74, _resource_apply_dense): c = m b1 + g (1 - b1); w -= lr (sign(c) + w wd), with the OLD m;
// m = m b2 + g (1 - b2).  One slot.  Every product and sum is one rounded float32 operation in the order the reference
// writes them -- nothing contracts into an FMA here, the EMA tail included -- so the result equals a numpy float32
// restatement bit for bit (tests/lion_ref.py).  sign(+-0) = 0 and sign(NaN) = NaN: a diverged run stays visible.
// This file is compiled with the default contraction, and HIP's __fmul_rn / __fadd_rn / __fsub_rn are plain operators that
// contract like any other (the compiler fused them here when they were tried): the three helpers below are those operators
// under `fp contract(off)`, which the default mode (fast-honor-pragmas) keeps out of every FMA after inlining.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

struct LionRule {
  static constexpr int SLOTS = 1;
  float b1, b2, wd;
  __device__ __forceinline__ void operator()(float g, float& m, float&, float& w, float& em, float lr, float decay,
                                             bool has_ema) const {
    const float c = add_rn(mul_rn(m, b1), mul_rn(g, sub_rn(1.f, b1)));
    const float s = c > 0.f ? 1.f : (c < 0.f ? -1.f : (c == 0.f ? 0.f : c));
    w = sub_rn(w, mul_rn(lr, add_rn(s, mul_rn(w, wd))));
    m = add_rn(mul_rn(m, b2), mul_rn(g, sub_rn(1.f, b2)));
    if (has_ema) em = sub_rn(em, mul_rn(sub_rn(1.f, decay), sub_rn(em, w)));
  }
};

template <typename Rule>
__device__ __forceinline__ void update_walk(Rule rule, float* params, const float* grads, float* slot_a, float* slot_b,
                                            float* ema, const int64_t* seg_off, const float* seg_factor,
                                            const int32_t* seg_flags, const float* hyper) {
  constexpr bool two = Rule::SLOTS == 2;      // slot_b is read and written by the two-slot rules only
  const int s = blockIdx.x;
  int64_t b, e;
  if (!slice_range(seg_off, s, blockIdx.y, b, e)) return;
  // frozen variables are not in the optimizer's variable list (tf2/train_lib.py:478-491,683): value, slots and EMA shadow
  // stay exactly as they are
  if (seg_flags && (seg_flags[s] & EDET_SEG_FROZEN)) return;
  const float f = seg_factor ? seg_factor[s] : 1.f;
  const float lr = hyper[0], decay = hyper[1];
  const bool has_ema = ema != nullptr;
  if ((b & 3) == 0) {
    const int64_t nv = (e - b) >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(grads + b);
    float4* p4 = reinterpret_cast<float4*>(slot_a + b);
    float4* q4 = reinterpret_cast<float4*>(two ? slot_b + b : nullptr);
    float4* w4 = reinterpret_cast<float4*>(params + b);
    float4* e4 = has_ema ? reinterpret_cast<float4*>(ema + b) : nullptr;
    for (int64_t i = threadIdx.x; i < nv; i += THREADS) {
      const float4 g = g4[i];
      float4 p = p4[i], q = make_float4(0.f, 0.f, 0.f, 0.f), w = w4[i], em = has_ema ? e4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (two) q = q4[i];
      rule(g.x * f, p.x, q.x, w.x, em.x, lr, decay, has_ema);
      rule(g.y * f, p.y, q.y, w.y, em.y, lr, decay, has_ema);
      rule(g.z * f, p.z, q.z, w.z, em.z, lr, decay, has_ema);
      rule(g.w * f, p.w, q.w, w.w, em.w, lr, decay, has_ema);
      p4[i] = p;
      if constexpr (two) q4[i] = q;
      w4[i] = w;
      if (has_ema) e4[i] = em;
    }
    b += nv << 2;
  }
  for (int64_t i = b + threadIdx.x; i < e; i += THREADS) {
    float p = slot_a[i], q = 0.f, w = params[i], em = has_ema ? ema[i] : 0.f;
    if constexpr (two) q = slot_b[i];
    rule(grads[i] * f, p, q, w, em, lr, decay, has_ema);
    slot_a[i] = p;
    if constexpr (two) slot_b[i] = q;
    params[i] = w;
    if (has_ema) ema[i] = em;
  }
}

// The kernels keep their names and parameter lists: the committed rocprofv3 statistics (profiles/) and the coverage test
// that reads them know the update by kernel symbol.  The second launch bound (8 waves per SIMD, so at most 64 VGPRs) is
// for the two-slot rules: without it the 4-wide Adam body takes 73 VGPRs and drops to 6 waves.
__global__ __launch_bounds__(THREADS, 8) void k_sgd_ema(float* params, float* grads, float* vel, float* ema,
                                                    const int64_t* seg_off, const float* seg_factor,
                                                    const int32_t* seg_flags, const float* hyper, float momentum) {
  update_walk(SgdRule{momentum}, params, grads, vel, nullptr, ema, seg_off, seg_factor, seg_flags, hyper);
}

__global__ __launch_bounds__(THREADS, 8) void k_adam_ema(float* params, const float* grads, float* m1, float* m2, float* ema,
                                                     const int64_t* seg_off, const float* seg_factor,
                                                     const int32_t* seg_flags, const float* hyper, float b1, float b2, float eps) {
  update_walk(AdamRule{b1, b2, eps}, params, grads, m1, m2, ema, seg_off, seg_factor, seg_flags, hyper);
}

__global__ __launch_bounds__(THREADS, 8) void k_rmsprop_ema(float* params, const float* grads, float* ms, float* mom, float* ema,
                                                        const int64_t* seg_off, const float* seg_factor,
                                                        const int32_t* seg_flags, const float* hyper, float rho, float momentum,
                                                        float eps) {
  update_walk(RmspropRule{rho, momentum, eps}, params, grads, ms, mom, ema, seg_off, seg_factor, seg_flags, hyper);
}

__global__ __launch_bounds__(THREADS, 8) void k_lion_ema(float* params, const float* grads, float* m, float* ema,
                                                     const int64_t* seg_off, const float* seg_factor,
                                                     const int32_t* seg_flags, const float* hyper, float b1, float b2, float wd) {
  update_walk(LionRule{b1, b2, wd}, params, grads, m, nullptr, ema, seg_off, seg_factor, seg_flags, hyper);
}

}  // namespace

extern "C" int edet_l2_loss(const float* params, const int64_t* seg_offsets, const int32_t* seg_flags, int nseg,
                            float weight_decay, float* seg_l2, float* l2_out, void* stream) {
  EDET_CHECK(params && seg_offsets && seg_flags && seg_l2 && l2_out && nseg > 0, "edet_l2_loss: bad arguments");
  edet_launch(k_l2_loss_slices, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), params, seg_offsets, seg_flags, weight_decay, seg_l2, nseg);
  edet_launch(k_l2_loss_sum, dim3(1), dim3(THREADS), 0, to_stream(stream), (const float*)seg_l2, nseg, l2_out);
  EDET_LAUNCH_CHECK("edet_l2_loss");
  return 0;
}

extern "C" int edet_opt_l2_norms(float* grads, const float* params, const int64_t* seg_offsets,
                                 const int32_t* seg_flags, int nseg, float weight_decay,
                                 float* seg_sqnorm, void* stream) {
  EDET_CHECK(grads && params && seg_offsets && seg_flags && seg_sqnorm && nseg > 0, "edet_opt_l2_norms: bad arguments");
  edet_launch(k_l2_norms, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), grads, params, seg_offsets, seg_flags, weight_decay, seg_sqnorm, nseg);
  EDET_LAUNCH_CHECK("edet_opt_l2_norms");
  return 0;
}

extern "C" int edet_opt_clip_factors(const float* seg_sqnorm, int nseg, float clip_norm,
                                     float* seg_factor, float* global_norm_out, float* l2_sum, void* stream) {
  EDET_CHECK(seg_sqnorm && seg_factor && nseg > 0, "edet_opt_clip_factors: bad arguments");
  edet_launch(k_clip_factors, dim3(1), dim3(THREADS), 0, to_stream(stream), seg_sqnorm, nseg, clip_norm, seg_factor, global_norm_out, l2_sum);
  EDET_LAUNCH_CHECK("edet_opt_clip_factors");
  return 0;
}

extern "C" int edet_opt_scale(float* grads, const int64_t* seg_offsets, const float* seg_factor,
                              int nseg, void* stream) {
  EDET_CHECK(grads && seg_offsets && seg_factor && nseg > 0, "edet_opt_scale: bad arguments");
  edet_launch(k_scale, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), grads, seg_offsets, seg_factor);
  EDET_LAUNCH_CHECK("edet_opt_scale");
  return 0;
}

extern "C" int edet_opt_sgd_ema(float* params, float* grads, float* velocity, float* ema,
                                const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                                const float* hyper_dev, float momentum, void* stream) {
  EDET_CHECK(params && grads && velocity && seg_offsets && hyper_dev && nseg > 0, "edet_opt_sgd_ema: bad arguments");
  edet_launch(k_sgd_ema, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), params, grads, velocity, ema, seg_offsets,
              seg_factor, seg_flags, hyper_dev, momentum);
  EDET_LAUNCH_CHECK("edet_opt_sgd_ema");
  return 0;
}

extern "C" int edet_opt_adam_ema(float* params, const float* grads, float* m, float* v, float* ema,
                                 const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                                 const float* hyper_dev, float beta1, float beta2, float epsilon, void* stream) {
  EDET_CHECK(params && grads && m && v && seg_offsets && hyper_dev && nseg > 0, "edet_opt_adam_ema: bad arguments");
  edet_launch(k_adam_ema, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), params, grads, m, v, ema, seg_offsets,
              seg_factor, seg_flags, hyper_dev, beta1, beta2, epsilon);
  EDET_LAUNCH_CHECK("edet_opt_adam_ema");
  return 0;
}

extern "C" int edet_opt_rmsprop_ema(float* params, const float* grads, float* ms, float* mom, float* ema,
                                    const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                                    const float* hyper_dev, float rho, float momentum, float epsilon, void* stream) {
  EDET_CHECK(params && grads && ms && mom && seg_offsets && hyper_dev && nseg > 0, "edet_opt_rmsprop_ema: bad arguments");
  edet_launch(k_rmsprop_ema, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), params, grads, ms, mom, ema, seg_offsets,
              seg_factor, seg_flags, hyper_dev, rho, momentum, epsilon);
  EDET_LAUNCH_CHECK("edet_opt_rmsprop_ema");
  return 0;
}

extern "C" int edet_opt_lion_ema(float* params, const float* grads, float* m, float* ema,
                                 const int64_t* seg_offsets, const float* seg_factor, const int32_t* seg_flags, int nseg,
                                 const float* hyper_dev, float beta1, float beta2, float wd, void* stream) {
  EDET_CHECK(params && grads && m && seg_offsets && hyper_dev && nseg > 0, "edet_opt_lion_ema: bad arguments");
  edet_launch(k_lion_ema, dim3(nseg, OPT_SPLIT), dim3(THREADS), 0, to_stream(stream), params, grads, m, ema, seg_offsets,
              seg_factor, seg_flags, hyper_dev, beta1, beta2, wd);
  EDET_LAUNCH_CHECK("edet_opt_lion_ema");
  return 0;
}
