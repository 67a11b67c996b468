// fedmi — the BatchNorm arithmetic of the CNN engines, each formula written ONCE as a fixed sequence of
// correctly rounded operations.  bn_apply / bn_bwd_* (cnn_ops.hip, both grids) and the DGRAD epilogues'
// BN-backward sums (common.h) call these and hold no formula of their own, so the same element gets the same
// bits whichever kernel or grid computes it, under any compiler:
//   * every fused step is an explicit fma / fmaf (one rounding of a * b + c);
//   * every other step sits under "fp contract(off)": the compiler may not fuse it with a neighbour;
//   * 1 / sqrt and the divisions are the IEEE operations (correctly rounded), not the approximate rsq / rcp.
// Host and device: tests/bn_math_host.cpp evaluates every function on the CPU against tests/bn_check.py.
// profiles/r17_bn_math/README.md records why each sequence is the one it is.
#pragma once
#include <math.h>

#if defined(__HIP__) || defined(__CUDACC__)
#define BN_FN __host__ __device__ __forceinline__
#else
#define BN_FN inline
#endif

namespace bn {

// ---- per element --------------------------------------------------------------------------------------------
// z * sc + sh in one rounding: the forward's value; bn_affine(..) > 0.f is the ReLU mask of every backward that
// re-derives it from z
BN_FN float bn_affine(float z, float sc, float sh) { return fmaf(z, sc, sh); }
// the forward's residual: a = bn_affine(..) of branch A, r = the identity input or bn_affine(..) of branch B
BN_FN float bn_add(float a, float r) {
#pragma clang fp contract(off)
  return a + r;
}
BN_FN float bn_relu(float x) { return fmaxf(x, 0.f); }

// s + g * xhat, xhat = (z - mean) * inv, as the accumulations of "sum g * xhat" take it: d = z - mean, p = g * d,
// then ONE fma folds p * inv into the running sum (three roundings per term)
BN_FN float bn_sum_term(float s, float g, float z, float mean, float inv) {
#pragma clang fp contract(off)
  const float d = z - mean;
  const float p = g * d;
  return fmaf(p, inv, s);
}

// dz = k * g + b * z + c, two fmas; the optional bypassing grad is one more addition
BN_FN float bn_dz(float k, float g, float b, float z, float c) { return fmaf(k, g, fmaf(b, z, c)); }
BN_FN float bn_dz_add(float dz, float dadd) {
#pragma clang fp contract(off)
  return dz + dadd;
}

// ---- per channel: forward -----------------------------------------------------------------------------------
// batch mean of (z - shift) and biased variance from the fp64 sums s1 = sum, s2 = sum of squares over M rows
BN_FN void bn_batch_stats(double s1, double s2, int M, float* mean_shifted, float* var) {
#pragma clang fp contract(off)
  const double msd = s1 / (double)M;
  *mean_shifted = (float)msd;
  *var = (float)fmax(fma(-msd, msd, s2 / (double)M), 0.0);
}
BN_FN float bn_unshift(float mean_shifted, float shift) {
#pragma clang fp contract(off)
  return mean_shifted + shift;
}
BN_FN float bn_inv_std(float var, float eps) {
#pragma clang fp contract(off)
  return 1.f / sqrtf(var + eps);
}
// running stats (torch BatchNorm2d: unbiased variance, the producing conv's bias enters the mean only)
BN_FN float bn_running_mean(float mom, float old, float mean, float cbias) {
#pragma clang fp contract(off)
  const float m = mean + cbias;
  const float t = mom * m;
  return fmaf(1.f - mom, old, t);
}
BN_FN float bn_running_var(float mom, float old, float var, int M) {
#pragma clang fp contract(off)
  const float unbias = (float)M / (float)(M > 1 ? M - 1 : 1);
  const float t = mom * var * unbias;
  return fmaf(1.f - mom, old, t);
}
BN_FN float bn_eval_mean(float rmean, float cbias) {
#pragma clang fp contract(off)
  return rmean - cbias;
}
BN_FN float bn_scale(float gamma, float inv) {
#pragma clang fp contract(off)
  return gamma * inv;
}
BN_FN float bn_shift(float beta, float mean, float sc) { return fmaf(-mean, sc, beta); }

// ---- per channel: backward ----------------------------------------------------------------------------------
// dz = k * (g - sg/M - xhat * sgx/M) regrouped over g and z:  k = gamma * inv (bn_scale),
// b = -k * sgx / M * inv,  c = -k * sg / M - b * mean
BN_FN float bn_inv_count(int M) {
#pragma clang fp contract(off)
  return 1.f / (float)M;
}
BN_FN float bn_bwd_b(float k, float sgx, float invM, float inv) {
#pragma clang fp contract(off)
  return -k * sgx * invM * inv;
}
BN_FN float bn_bwd_c(float k, float sg, float invM, float b, float mean) {
#pragma clang fp contract(off)
  const float t = -k * sg * invM;
  return fmaf(-b, mean, t);
}

}  // namespace bn
