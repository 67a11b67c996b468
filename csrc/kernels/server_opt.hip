// fedmi — server-side optimizers on the aggregated flat state (fedmi/parallel/server_opt.py).
//
// After the FedAvg collective every client holds x = mean(clients) and a copy of the previous global
// model (anchor); d = x - anchor is the round's pseudo-gradient.  One launch applies, per entry i < n_opt,
//   fedavgm :   m = beta1*m + d                                x = anchor + lr*m
//   adaptive:   m = beta1*m + (1-beta1)*d
//     fedadagrad: v = v + d*d
//     fedyogi   : v = v - (1-beta2)*d*d*sgn(v - d*d)           (sgn(0) = 0)
//     fedadam   : v = beta2*v + (1-beta2)*d*d
//                                                              x = anchor + lr*m / (sqrt(v) + tau)
// and anchor = x (the new global model).  Entries n_opt <= i < n (float buffers: BN running statistics) stay
// the plain mean: x is left alone and anchor = x.  No bias correction, no step counter (Hsu et al. 2019;
// Reddi et al. 2021 have none).
//
// Streams 16 B per lane and grid-strides like flat_ops.hip (memory-bound: 24 B per entry for FedAvgM,
// 32 B for the adaptive kinds).  Specialised on the kind, so FedAvgM never touches v (it may be null).  Every
// entry is computed by one lane from its own inputs only (no atomics, no LDS), so the same binary on the
// same inputs gives the same bits on every rank: the replicated optimizer state stays in lockstep.
//
// The kernel keeps its own loop and shares only the grid rule of flat_map.h.  On that skeleton the adaptive kinds
// measured 2.3 % slower at 11.2 M entries, and the two sums of two products (m, FedAdam's v) were contracted into
// another fma than here, which moved a quarter of all m by one ulp (profiles/r9_flatmap/).
#include "flat_map.h"

namespace {

enum { FEDAVGM = 0, FEDADAGRAD = 1, FEDYOGI = 2, FEDADAM = 3 };

struct ServerHyper {
  float lr, beta1, beta2, tau;
};

// one entry; x, a, m, v are the lane's register copies (v unused for FEDAVGM)
template <int KIND>
FEDMI_DEV void server_elem(float& x, float& a, float& m, float& v, const ServerHyper h) {
  const float d = x - a;
  if (KIND == FEDAVGM) {
    m = h.beta1 * m + d;
    x = a + h.lr * m;
  } else {
    m = h.beta1 * m + (1.f - h.beta1) * d;
    const float dd = d * d;
    if (KIND == FEDADAGRAD) {
      v = v + dd;
    } else if (KIND == FEDYOGI) {
      const float s = v - dd;
      const float sgn = (s > 0.f) ? 1.f : ((s < 0.f) ? -1.f : 0.f);
      v = v - (1.f - h.beta2) * dd * sgn;
    } else {
      v = h.beta2 * v + (1.f - h.beta2) * dd;
    }
    x = a + h.lr * m / (sqrtf(v) + h.tau);
  }
  a = x;
}

template <int KIND>
FEDMI_DEV void server_scalar(float* __restrict__ x, float* __restrict__ anchor, float* __restrict__ m,
                             float* __restrict__ v, long i, long n_opt, const ServerHyper h) {
  if (i >= n_opt) {
    anchor[i] = x[i];
    return;
  }
  float xv = x[i], av = anchor[i], mv = m[i], vv = 0.f;
  if (KIND != FEDAVGM) vv = v[i];
  server_elem<KIND>(xv, av, mv, vv, h);
  x[i] = xv;
  anchor[i] = av;
  m[i] = mv;
  if (KIND != FEDAVGM) v[i] = vv;
}

template <int KIND>
__global__ __launch_bounds__(256) void server_opt_kernel(float* __restrict__ x, float* __restrict__ anchor,
                                                         float* __restrict__ m, float* __restrict__ v, long n,
                                                         long n_opt, ServerHyper h) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const long e = i << 2;
    if (e >= n_opt) {                       // float buffers: the mean stays, the anchor follows
      reinterpret_cast<float4*>(anchor)[i] = reinterpret_cast<const float4*>(x)[i];
    } else if (e + 4 <= n_opt) {
      float4 xv = reinterpret_cast<float4*>(x)[i];
      float4 av = reinterpret_cast<float4*>(anchor)[i];
      float4 mv = reinterpret_cast<float4*>(m)[i];
      float4 vv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (KIND != FEDAVGM) vv = reinterpret_cast<float4*>(v)[i];
      float* xx = reinterpret_cast<float*>(&xv);
      float* aa = reinterpret_cast<float*>(&av);
      float* mm = reinterpret_cast<float*>(&mv);
      float* vp = reinterpret_cast<float*>(&vv);
#pragma unroll
      for (int j = 0; j < 4; ++j) server_elem<KIND>(xx[j], aa[j], mm[j], vp[j], h);
      reinterpret_cast<float4*>(x)[i] = xv;
      reinterpret_cast<float4*>(anchor)[i] = av;
      reinterpret_cast<float4*>(m)[i] = mv;
      if (KIND != FEDAVGM) reinterpret_cast<float4*>(v)[i] = vv;
    } else {                                // the one vector that straddles n_opt
      for (int j = 0; j < 4; ++j) server_scalar<KIND>(x, anchor, m, v, e + j, n_opt, h);
    }
  }
  // tail (n % 4 entries)
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    server_scalar<KIND>(x, anchor, m, v, i, n_opt, h);
}

}  // namespace

namespace fedmi {

// kind: 0 fedavgm, 1 fedadagrad, 2 fedyogi, 3 fedadam (fedmi/parallel/server_opt.py KINDS).  x, anchor, m
// (and v unless kind == 0) hold n floats and are 16-byte aligned; 0 <= n_opt <= n (the binding checks all of it).
void launch_server_opt(hipStream_t st, float* x, float* anchor, float* m, float* v, long n, long n_opt, int kind,
                       float lr, float beta1, float beta2, float tau) {
  if (n <= 0 || kind < FEDAVGM || kind > FEDADAM) return;
  const ServerHyper h = {lr, beta1, beta2, tau};
  const dim3 grid(flat_grid(n)), block(256);
  switch (kind) {
    case FEDAVGM:    hipLaunchKernelGGL(server_opt_kernel<FEDAVGM>, grid, block, 0, st, x, anchor, m, v, n, n_opt, h); break;
    case FEDADAGRAD: hipLaunchKernelGGL(server_opt_kernel<FEDADAGRAD>, grid, block, 0, st, x, anchor, m, v, n, n_opt, h); break;
    case FEDYOGI:    hipLaunchKernelGGL(server_opt_kernel<FEDYOGI>, grid, block, 0, st, x, anchor, m, v, n, n_opt, h); break;
    default:         hipLaunchKernelGGL(server_opt_kernel<FEDADAM>, grid, block, 0, st, x, anchor, m, v, n, n_opt, h); break;
  }
}

}  // namespace fedmi
