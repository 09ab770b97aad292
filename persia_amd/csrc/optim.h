// Row-wise sparse optimizer math and the ordered gradient reduction — the one
// copy every update kernel in kernels.hip calls.
//
// The optimizer functions are pure register math, one element at a time:
// they take the loaded values and return the new ones, so each kernel keeps
// its own load / compute / store interleaving (the multi-key kernels issue
// the loads of all their keys before the dependent math).  The expressions
// are exact-math variants of the reference (persia-simd lib.rs:21-251); every
// kernel inlines the same expression tree.  Where a sum has two products the
// fused one is written out (pa_adagrad_acc, pa_adam_m, pa_adam_v): which one
// the compiler contracts is otherwise its choice, per kernel and per column.
// FTRL (pa_ftrl, not in the reference) spells out every fma it has.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <cstdint>

#include "common.h"

__device__ __forceinline__ float pa_to_float(float x) { return x; }
__device__ __forceinline__ float pa_to_float(__half x) { return __half2float(x); }
__device__ __forceinline__ float pa_to_float(__hip_bfloat16 x) {
  return __bfloat162float(x);
}

// opt: 0 = SGD      p0=lr p1=weight_decay
//      1 = Adagrad  p0=lr p1=g_square_momentum p2=eps p3=vectorwise_shared
//      2 = Adam     p0=lr p1=beta1 p2=beta2 p3=eps      (store.py _opt_params)
//      3 = FTRL     p0=lr p1=beta p2=l1 p3=l2
// The launchers reject any other code; no kernel has a default arm.
struct PaOptArgs {
  int opt;
  float p0, p1, p2, p3;
  float weight_bound;
  float om1, om2, c1, c2;  // Adam: 1-beta, 1/(1-beta^t)
  float ilr;               // FTRL: 1/lr
};

__device__ __forceinline__ PaOptArgs pa_opt_args(int opt, float p0, float p1,
                                                 float p2, float p3,
                                                 float b1_power, float b2_power,
                                                 float weight_bound) {
  PaOptArgs a;
  a.opt = opt;
  a.p0 = p0; a.p1 = p1; a.p2 = p2; a.p3 = p3;
  a.weight_bound = weight_bound;
  a.om1 = 1.0f - p1;
  a.om2 = 1.0f - p2;
  a.c1 = 1.0f / (1.0f - b1_power);
  a.c2 = 1.0f / (1.0f - b2_power);
  a.ilr = 1.0f / p0;
  return a;
}

__device__ __forceinline__ bool pa_adagrad_shared(const PaOptArgs& a) {
  return a.p3 > 0.5f;
}

__device__ __forceinline__ float pa_clamp_weight(const PaOptArgs& a, float w) {
  if (a.weight_bound > 0.0f) w = fminf(fmaxf(w, -a.weight_bound), a.weight_bound);
  return w;
}

// SGD: w -= lr*(g + wd*w)
__device__ __forceinline__ float pa_sgd(const PaOptArgs& a, float w, float g) {
  return pa_clamp_weight(a, w - a.p0 * (g + a.p1 * w));
}

// Adagrad weight step; acc is the column's accumulator, or the row's one
// scalar accumulator when vectorwise-shared
__device__ __forceinline__ float pa_adagrad_w(const PaOptArgs& a, float w,
                                              float acc, float g) {
  return pa_clamp_weight(a, w - a.p0 * g * rsqrtf(acc + a.p2));
}

// Adagrad state step, per column: acc*p1 + g*g as one explicit fma.  Left to
// the compiler, which of the two products is fused into the add depends on
// the surrounding kernel, and the choice is part of the result (a last-ulp
// difference that golden training results and the bit-equality tests between
// kernels pin).  Default: g*g rounded, acc*p1 fused — what update_kernel and
// the multi-key kernels compute.  FUSE_GG: acc*p1 rounded, g*g fused — what
// scatter_update_kernel computes.
template <bool FUSE_GG = false>
__device__ __forceinline__ float pa_adagrad_acc(const PaOptArgs& a, float acc,
                                                float g) {
  if constexpr (FUSE_GG) return __builtin_fmaf(g, g, acc * a.p1);
  return __builtin_fmaf(acc, a.p1, g * g);
}

// Adagrad state step, vectorwise-shared: gsq = sum of g*g over the row
__device__ __forceinline__ float pa_adagrad_shared_acc(const PaOptArgs& a,
                                                       float acc, float gsq,
                                                       int dim) {
  return acc * a.p1 + gsq / (float)dim;
}

// Adam moment steps, then the weight step from the NEW moments.  Both are
// sums of two products, so as in pa_adagrad_acc the fused product is spelled
// out: left to the compiler the choice differed between kernels and, inside
// the hinted multi-key kernels, between unrolled columns, so a hinted update
// from non-zero moments was not the bits of the unhinted one.  Default: the
// gradient product fused, the decayed moment rounded — what every fused
// scatter kernel computed.  FUSE_STATE: the other way round — what
// update_kernel computed.
template <bool FUSE_STATE = false>
__device__ __forceinline__ float pa_adam_m(const PaOptArgs& a, float m, float g) {
  if constexpr (FUSE_STATE) return __builtin_fmaf(a.p1, m, a.om1 * g);
  return __builtin_fmaf(a.om1, g, a.p1 * m);
}
template <bool FUSE_STATE = false>
__device__ __forceinline__ float pa_adam_v(const PaOptArgs& a, float v, float g) {
  if constexpr (FUSE_STATE) return __builtin_fmaf(a.p2, v, a.om2 * g * g);
  return __builtin_fmaf(a.om2 * g, g, a.p2 * v);
}
__device__ __forceinline__ float pa_adam_w(const PaOptArgs& a, float w, float m,
                                           float v) {
  return pa_clamp_weight(a, w - a.p0 * (m * a.c1) / (a.p3 + sqrtf(v * a.c2)));
}

// FTRL-Proximal, per coordinate (McMahan et al. 2013, "Ad Click Prediction",
// Algorithm 1); row = [w | z | n], z where Adam keeps m and n where it keeps v:
//   n1    = n + g*g
//   sigma = (sqrt(n1) - sqrt(n)) / lr
//   z1    = z + (g - sigma*w)
//   w1    = (clip(z1, -l1, +l1) - z1) / ((beta + sqrt(n1))/lr + l2)
// The new weight is a function of (z1, n1) alone, exactly 0 where |z1| <= l1;
// the old weight enters only through sigma*w.  The divisions by lr are
// products with the rounded reciprocal a.ilr.  Every sum that takes a product
// is a spelled-out fma, and there is one expression tree for every kernel:
// s0 = sqrtf(n) and s1 = sqrtf(n1) are computed once in pa_ftrl and shared.
__device__ __forceinline__ float pa_ftrl_n(float n, float g) {
  return __builtin_fmaf(g, g, n);
}
__device__ __forceinline__ float pa_ftrl_z(const PaOptArgs& a, float w, float z,
                                           float s0, float s1, float g) {
  const float sigma = (s1 - s0) * a.ilr;
  return z + __builtin_fmaf(-sigma, w, g);
}
__device__ __forceinline__ float pa_ftrl_w(const PaOptArgs& a, float z1,
                                           float s1) {
  const float q = __builtin_fmaf(a.p1 + s1, a.ilr, a.p3);
  const float clip = fminf(fmaxf(z1, -a.p2), a.p2);
  return pa_clamp_weight(a, (clip - z1) / q);
}
struct PaFtrlRow {
  float w, z, n;
};
__device__ __forceinline__ PaFtrlRow pa_ftrl(const PaOptArgs& a, float w,
                                             float z, float n, float g) {
  PaFtrlRow r;
  r.n = pa_ftrl_n(n, g);
  const float s1 = sqrtf(r.n);
  r.z = pa_ftrl_z(a, w, z, sqrtf(n), s1, g);
  r.w = pa_ftrl_w(a, r.z, s1);
  return r;
}

// Ordered gradient reduction of one unique key: accumulate its positions
// [lo, hi) (contiguous in sort order) into acc[t] for the lane's columns
// c0, c0+st, ... < dim.  A position with seg_id < 0 (raw-slot positions,
// handled by a separate indexed add) or seg_scale == 0 (NaN-slot mask)
// contributes nothing: its gradient is neither read nor multiplied — never
// multiply a NaN gradient, even by zero.  Null seg_scale = 1.  acc is any
// T-element accumulator indexable by [t]; T == 1 is the one-column form (st
// unused).
template <int T, typename AccT, typename GradT>
__device__ __forceinline__ void pa_reduce_positions(
    AccT& acc, const GradT* __restrict__ grads,
    const int64_t* __restrict__ perm, const int64_t* __restrict__ seg_id,
    const float* __restrict__ seg_scale, int64_t lo, int64_t hi, int dim,
    int c0, int st) {
  for (int64_t p = lo; p < hi; ++p) {
    const int64_t s = seg_id[perm[p]];
    if (s < 0) continue;
    const float sc = seg_scale ? seg_scale[s] : 1.0f;
    if (sc == 0.0f) continue;
    const GradT* g = grads + s * dim;
    if constexpr (T == 1) {
      acc[0] += pa_to_float(g[c0]) * sc;
    } else {
      for (int t = 0, c = c0; c < dim; c += st, ++t)
        acc[t] += pa_to_float(g[c]) * sc;
    }
  }
}
