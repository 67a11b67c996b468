// fedmi — client-side drift correction inside the local SGD step (fedmi/parallel/client_opt.py).
//
// Under non-IID shards every client's iterates walk toward its own optimum during the local epoch.  Two
// remedies change the gradient the SGD tail consumes; all buffers are fp32 and n = n_params() entries long:
//   drift_grad<FEDPROX>  (once per step):  g = fma(mu, p - anchor, g)          (Li et al. 2020; anchor = the
//                                                                               round's starting model)
//   drift_grad<SCAFFOLD> (once per step):  acc = acc + g;  g = g + corr        (Karimireddy et al. 2020;
//                                                                               corr = c - c_i, acc sums the RAW g)
//   scaffold_finish (once per round, before the collective):
//                                          new = acc / K;  delta = new - ci;  ci = new
//   scaffold_begin  (once per round, after the collective):
//                                          c = c + dmean;  corr = c - ci;  acc = 0
// c_i is the mean of the round's raw gradients, not (w_global - y_K)/(K*lr): the clients run momentum that
// persists across rounds, for which the latter is not the gradient mean.
//
// Streams 16 B per lane and grid-strides like flat_ops.hip (memory-bound: 16 B per entry for FedProx, 20 B
// for SCAFFOLD's step).  drift_grad is specialised on the kind, so a kind never touches a buffer it does not
// need (those may be null).  Every output is one correctly rounded fp32 operation (the fma and the division
// are written as such, so the compiler's contraction / reciprocal choices are not part of the result) computed
// by one lane from its own inputs: no atomics, no LDS, the same bits on every rank.
#include "common.h"

namespace {

enum { FEDPROX = 0, SCAFFOLD = 1 };

typedef float4 V4;

template <int KIND>
__global__ __launch_bounds__(256) void drift_grad_kernel(float* __restrict__ g, const float* __restrict__ p,
                                                         const float* __restrict__ anchor,
                                                         const float* __restrict__ corr, float* __restrict__ acc,
                                                         float mu, long n) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    V4 gv = reinterpret_cast<V4*>(g)[i];
    float* gg = reinterpret_cast<float*>(&gv);
    if (KIND == FEDPROX) {
      const V4 pv = reinterpret_cast<const V4*>(p)[i];
      const V4 av = reinterpret_cast<const V4*>(anchor)[i];
      const float* pp = reinterpret_cast<const float*>(&pv);
      const float* aa = reinterpret_cast<const float*>(&av);
#pragma unroll
      for (int j = 0; j < 4; ++j) gg[j] = __fmaf_rn(mu, pp[j] - aa[j], gg[j]);
    } else {
      const V4 cv = reinterpret_cast<const V4*>(corr)[i];
      V4 sv = reinterpret_cast<V4*>(acc)[i];
      const float* cc = reinterpret_cast<const float*>(&cv);
      float* ss = reinterpret_cast<float*>(&sv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ss[j] = ss[j] + gg[j];
        gg[j] = gg[j] + cc[j];
      }
      reinterpret_cast<V4*>(acc)[i] = sv;
    }
    reinterpret_cast<V4*>(g)[i] = gv;
  }
  // tail (n % 4 entries)
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gv = g[i];
    if (KIND == FEDPROX) {
      g[i] = __fmaf_rn(mu, p[i] - anchor[i], gv);
    } else {
      acc[i] = acc[i] + gv;
      g[i] = gv + corr[i];
    }
  }
}

FEDMI_DEV void finish_elem(float& a, float& ci, float& d, float k) {
  const float nw = __fdiv_rn(a, k);
  d = nw - ci;
  ci = nw;
}

__global__ __launch_bounds__(256) void scaffold_finish_kernel(const float* __restrict__ acc, float* __restrict__ ci,
                                                              float* __restrict__ delta, float k, long n) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    V4 av = reinterpret_cast<const V4*>(acc)[i];
    V4 cv = reinterpret_cast<V4*>(ci)[i];
    V4 dv;
    float* aa = reinterpret_cast<float*>(&av);
    float* cc = reinterpret_cast<float*>(&cv);
    float* dd = reinterpret_cast<float*>(&dv);
#pragma unroll
    for (int j = 0; j < 4; ++j) finish_elem(aa[j], cc[j], dd[j], k);
    reinterpret_cast<V4*>(ci)[i] = cv;
    reinterpret_cast<V4*>(delta)[i] = dv;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float av = acc[i], cv = ci[i], dv;
    finish_elem(av, cv, dv, k);
    ci[i] = cv;
    delta[i] = dv;
  }
}

__global__ __launch_bounds__(256) void scaffold_begin_kernel(float* __restrict__ c, const float* __restrict__ dmean,
                                                             const float* __restrict__ ci, float* __restrict__ corr,
                                                             float* __restrict__ acc, long n) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  const V4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    V4 cv = reinterpret_cast<V4*>(c)[i];
    const V4 dv = reinterpret_cast<const V4*>(dmean)[i];
    const V4 iv = reinterpret_cast<const V4*>(ci)[i];
    V4 rv;
    float* cc = reinterpret_cast<float*>(&cv);
    const float* dd = reinterpret_cast<const float*>(&dv);
    const float* ii = reinterpret_cast<const float*>(&iv);
    float* rr = reinterpret_cast<float*>(&rv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cc[j] = cc[j] + dd[j];
      rr[j] = cc[j] - ii[j];
    }
    reinterpret_cast<V4*>(c)[i] = cv;
    reinterpret_cast<V4*>(corr)[i] = rv;
    reinterpret_cast<V4*>(acc)[i] = zero;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float cv = c[i] + dmean[i];
    c[i] = cv;
    corr[i] = cv - ci[i];
    acc[i] = 0.f;
  }
}

int grid_for(long n) {
  long blocks = (n / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;   // 256 CUs x 8: grid-stride the rest, as flat_ops.hip
  return (int)blocks;
}

}  // namespace

namespace fedmi {

// kind: 0 fedprox (g, p, anchor, mu), 1 scaffold (g, corr, acc); the other kind's buffers may be null.  Every
// buffer holds n floats and is 16-byte aligned (the binding checks all of it).
void launch_drift_grad(hipStream_t st, int kind, float* g, const float* p, const float* anchor, const float* corr,
                       float* acc, float mu, long n) {
  if (n <= 0) return;
  const dim3 grid(grid_for(n)), block(256);
  if (kind == FEDPROX)
    hipLaunchKernelGGL(drift_grad_kernel<FEDPROX>, grid, block, 0, st, g, p, anchor, corr, acc, mu, n);
  else if (kind == SCAFFOLD)
    hipLaunchKernelGGL(drift_grad_kernel<SCAFFOLD>, grid, block, 0, st, g, p, anchor, corr, acc, mu, n);
}

void launch_scaffold_finish(hipStream_t st, const float* acc, float* ci, float* delta, long K, long n) {
  if (n <= 0 || K < 1) return;
  hipLaunchKernelGGL(scaffold_finish_kernel, dim3(grid_for(n)), dim3(256), 0, st, acc, ci, delta, (float)K, n);
}

void launch_scaffold_begin(hipStream_t st, float* c, const float* dmean, const float* ci, float* corr, float* acc,
                           long n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(scaffold_begin_kernel, dim3(grid_for(n)), dim3(256), 0, st, c, dmean, ci, corr, acc, n);
}

}  // namespace fedmi
