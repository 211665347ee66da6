// mlp_math.h -- the scalar arithmetic every kernel family shares, each formula defined once: activations,
// the objective transform, binary cross-entropy from logits, the accuracy hit, the Adam update and its
// step size.  Device-only.  Two flavours of rounding live here: the FIT's forms (fit_*,
// adam_update: hardware rcp / sqrt / 2^t, at most 1 ulp per operation) and the IEEE forms of everything
// else.  The library is built with -ffp-contract=off: the order of the operations below IS the rounding.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bore_hip.h"

namespace bore {

__device__ __forceinline__ float sigmoid_stable(float x) {
  float e = expf(-fabsf(x));  // expf: ocml, <=1 ulp
  float d = 1.f + e;
  return x >= 0.f ? 1.f / d : e / d;
}

// The fit's arithmetic is "at most 1 ulp per operation", not IEEE-correctly-rounded: square root,
// reciprocal and exp2 are the hardware's v_sqrt_f32 / v_rcp_f32 / v_exp_f32 (1 ulp each).  TensorFlow's
// own Eigen kernels are not correctly rounded either; the parity gate is the oracle
// tolerance of tests/test_gpu_parity.py, not the bits of a previous build.  The correctly rounded forms
// (ocml expf, IEEE division and sqrt: ~30 dependent instructions per updated register) were 0.8 - 1.2 k
// cycles of a 3.3 - 3.7 k-cycle Adam step (profiles/r3/fit_marks_final.txt).  The L-BFGS-B (fp64,
// lbfgsb.h) and the objective evaluation keep their IEEE forms.

// ---- the FIT's arithmetic: "<= 1 ulp per operation" (DESIGN.md 2), hardware rcp / sqrt / 2^t ----
__device__ __forceinline__ float fit_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fit_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
// exp(x) for x <= 0: 2^(x log2 e) with the product's rounding error fed back (the argument's error
// would otherwise be |x| 2^-24 in the exponent); flushes to zero below 2^-126 like the result's use
// (1 + e) does not notice
__device__ __forceinline__ float fit_exp_neg(float x) {
  const float L2E = 1.442695040888963f, L2E_LO = 1.925963033500e-8f;  // log2(e) = hi + lo
  const float t = x * L2E;
  const float r = fmaf(x, L2E_LO, fmaf(x, L2E, -t));                 // exact remainder of the product
  const float e = __builtin_amdgcn_exp2f(t);
  return fmaf(e, r * 0.6931471805599453f, e);                          // 2^(t + r) = 2^t (1 + r ln 2)
}
// elu(x) in the fit (round 6).  The reference's layers are Keras `activation="elu"` (plugins/hpbandster/base.py:
// 152-155), whose TF kernel forms exp(x) - 1 for x < 0 (Eigen: features.exp() - 1).  ocml's expm1f is ~60
// instructions with branches, 24 calls per lane in a forward pass of 16->32-32-32-1: 6.7 k of an 18 k-cycle Adam
// step (profiles/r6/fit_marks_plugin.txt).  Here, for x < 0: the hardware's 2^(x log2 e) minus one -- the error of
// the rounded exponent is e^x |x| 2^-24 <= 0.37 x 2^-24 in absolute terms, under the half-ulp the exponential itself
// may be off near 1, so no feedback term; the subtraction is exact from x >= -0.69 on -- and the series
// x + x^2/2 + x^3/6 + x^4/24 where that difference would cancel (|x| < 1/32: truncation x^5 / 120 < 2^-26 |x|).
// Absolute error <= 2^-24 everywhere against the float64 oracle's expm1, relative <= 2e-6 (at the seam).
__device__ __forceinline__ float fit_elu(float x) {
  const float xn = fminf(x, 0.f);
  const float big = __builtin_amdgcn_exp2f(xn * 1.442695040888963f) - 1.f;
  const float ser = xn * fmaf(xn, fmaf(xn, fmaf(xn, 1.f / 24.f, 1.f / 6.f), 0.5f), 1.f);
  const float neg = xn > -0.03125f ? ser : big;
  return x > 0.f ? x : neg;
}

// FIT: the caller is a fit kernel (fit_elu instead of ocml's expm1f; everything else alike)
template <bool FIT = false>
__device__ __forceinline__ float act_fwd(int a, float x) {
  switch (a) {
    case BORE_ACT_RELU: return fmaxf(x, 0.f);
    case BORE_ACT_ELU:
      if constexpr (FIT) return fit_elu(x);
      else return x > 0.f ? x : expm1f(x);
    case BORE_ACT_SIGMOID: return sigmoid_stable(x);
    case BORE_ACT_TANH: return tanhf(x);
    default: return x;
  }
}

// d act / d pre-activation, from the activation OUTPUT h.
__device__ __forceinline__ float act_grad(int a, float h) {
  switch (a) {
    case BORE_ACT_RELU: return h > 0.f ? 1.f : 0.f;
    case BORE_ACT_ELU: return h > 0.f ? 1.f : h + 1.f;
    case BORE_ACT_SIGMOID: return h * (1.f - h);
    case BORE_ACT_TANH: return 1.f - h * h;
    default: return 1.f;
  }
}

// The objective transform of the acquisition (BORE_T_*): T(u) and dT / du, u = sign * f.  The callers
// form sign * dT * act_grad(...) themselves (their rounding of that product differs by flavour).
__device__ __forceinline__ void objective_transform(int transform, float u, float &T, float &dT) {
  if (transform == BORE_T_SIGMOID) {
    T = sigmoid_stable(u);
    dT = T * (1.f - T);
  } else if (transform == BORE_T_EXP) {
    T = expf(u);
    dT = T;
  } else {
    T = u;
    dT = 1.f;
  }
}

// Binary cross-entropy from the logit x, label z, IEEE form: the loss term of one row.
__device__ __forceinline__ float bce_loss(float x, float z) {
  return fmaxf(x, 0.f) - x * z + log1pf(expf(-fabsf(x)));
}
// The same under a sample weight w (Keras sample_weight / class_weight): the row's term of sum_i w_i loss_i.
__device__ __forceinline__ float bce_loss_weighted(float x, float z, float w) { return w * bce_loss(x, z); }
// 1 where the output o (a probability, or whatever a head without a sigmoid gives) and the label z lie
// on the same side of 0.5 (Keras binary_accuracy), else 0.
__device__ __forceinline__ float accuracy_hit(float o, float z) { return ((o > 0.5f) == (z > 0.5f)) ? 1.f : 0.f; }

// The same in the FIT's arithmetic: returns sigmoid(x) - z = d loss / d logit (the caller scales it by
// 1 / rows) and, when `want_loss`, adds the row's loss term to `loss`.  exp(-|x|) is shared by the two.
__device__ __forceinline__ float fit_bce(float x, float z, bool want_loss, float &loss) {
  const float ex = fit_exp_neg(-fabsf(x));
  const float rden = fit_rcp(1.f + ex);
  const float sig = x >= 0.f ? rden : ex * rden;
  if (want_loss) loss += fmaxf(x, 0.f) - x * z + log1pf(ex);
  return sig - z;
}
// The weighted fit (sample weight w of the row): the same sigmoid(x) - z, and w times the row's loss term added to
// `loss`.  The caller forms (fit_bce_weighted(...) * inv_nb) * w, in that order: the divisor stays the ROW COUNT
// (Keras' SUM_OVER_BATCH_SIZE), and with w == 1 every intermediate is the unweighted kernel's, bit for bit.
__device__ __forceinline__ float fit_bce_weighted(float x, float z, float w, bool want_loss, float &loss) {
  float l = 0.f;
  const float d = fit_bce(x, z, want_loss, l);
  if (want_loss) loss += w * l;
  return d;
}

// Adam update of one parameter (ResourceApplyAdam, non-nesterov); returns the new weight.
__device__ __forceinline__ float adam_update(float w, float g, float &m, float &v, float alpha,
                                             float omb1, float omb2, float eps) {
  m += (g - m) * omb1;
  v += (g * g - v) * omb2;
  return fmaf(-(m * alpha), fit_rcp(fit_sqrt(v) + eps), w);
}
// The same in the IEEE form (the LSTM fits): division and sqrtf, and the gradient 2 f w of the weight's l2 penalty
// (factor f) added to `grad` first.
__device__ __forceinline__ float adam_update_ieee(float w, float grad, float f, float &m, float &v, float alpha,
                                                  float omb1, float omb2, float eps) {
  const float g = grad + 2.f * f * w;
  m += (g - m) * omb1;
  v += (g * g - v) * omb2;
  return w - (m * alpha) / (sqrtf(v) + eps);
}

// Step size of Adam step t: lr * sqrt(1 - beta2^t) / (1 - beta1^t), from running beta powers in fp64
// that are rounded to fp32 at use (DESIGN.md "Adam").  Starts at the t0 steps a model has behind it.
struct AdamClock {
  double b1p, b2p;  // beta1^t, beta2^t
  __device__ __forceinline__ AdamClock(float beta1, float beta2, long long t0)
      : b1p(pow((double)beta1, (double)t0)), b2p(pow((double)beta2, (double)t0)) {}
  __device__ __forceinline__ float advance(float lr, float beta1, float beta2) {
    b1p *= (double)beta1;
    b2p *= (double)beta2;
    return lr * sqrtf(1.f - (float)b2p) / (1.f - (float)b1p);
  }
};

}  // namespace bore
