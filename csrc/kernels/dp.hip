// fedmi — differentially private FedAvg on the client's flat state (fedmi/parallel/dp.py): clip the round's update
// to L2 norm S and add Gaussian noise calibrated to S (McMahan et al. 2018), before the collective.
//
// x = float_state(), a = the round's starting global model, k = n_params() entries of each:
//   dp_sumsq  :  d_i = x_i - a_i (fp32);  partial[wg] = sum of d_i^2 over the workgroup's entries (fp64)
//   dp_finish :  sumsq = sum of the partials;  norm = sqrt(sumsq);  scale = norm > S ? (float)(S / norm) : 1
//                stats = {sumsq, norm, scale} (three fp64; scale holds the fp32 value)
//   DpApply   :  y_i = scale == 1 ? x_i : fma(scale, d_i, a_i);  x_i = NOISE ? fma(sigma, g_i, y_i) : y_i
// Entries at and past k (BN running statistics) are never read or written.
//
// Determinism.  The square of an fp32 number is exact in fp64, so the sum's only roundings are the additions, and
// their order is fixed: a lane adds its grid-strided entries in index order, a workgroup folds its 256 lanes in an LDS
// tree, dp_finish folds the partials the same way.  The grid is a function of k alone (flat_grid).  There are no atomics,
// so the same inputs, key and draw give the same bits on every run.
//
// Noise.  Philox4x32-10 (Salmon et al. 2011), key = the client's 64-bit secret, counter = (block lo, block hi, draw lo,
// draw hi) with block = i >> 2; entry i takes lane i & 3 of its block, on the vector path and on the tail alike.  The
// four outputs r0..r3 give two Box-Muller pairs: u(r) = ((r >> 9) + 0.5) * 2^-23 is exact in fp32 and never 0 or 1;
// lanes 0, 1 = sqrt(-2 ln u(r0)) * {cos, sin}(2 pi u(r1)), lanes 2, 3 the same from r2, r3.  The angle goes through
// sincospif(2 u): 2 u is exact, so no rounded multiple of pi enters the result.  logf / sqrtf / sincospif are the
// accurate library functions, not the fast intrinsics.
//
// Cost per entry: 8 B read by dp_sumsq, 8 B read + 4 B written by the apply (4 B + 4 B when nothing is clipped,
// nothing at all for clip-only with scale == 1), and a quarter of a Philox block and half a Box-Muller pair.
#include "flat_map.h"

namespace {

using fedmi::flat_load;
using fedmi::flat_store;

constexpr int DP_THREADS = 256;

// fixed-order sum of one fp64 per lane over the workgroup; the result is valid in thread 0
FEDMI_DEV double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = DP_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(DP_THREADS) void dp_sumsq_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ anchor, long k,
                                                              double* __restrict__ partial) {
  __shared__ double sh[DP_THREADS];
  const long k4 = k >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  double acc = 0.0;
  for (long i = t; i < k4; i += stride) {
    const auto xv = flat_load<4>(x, i << 2), av = flat_load<4>(anchor, i << 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)(xv[j] - av[j]);
      acc += d * d;
    }
  }
  for (long i = (k4 << 2) + t; i < k; i += stride) {   // the k % 4 entries of the vector that straddles k
    const double d = (double)(x[i] - anchor[i]);
    acc += d * d;
  }
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(DP_THREADS) void dp_finish_kernel(const double* __restrict__ partial, int n_partial,
                                                               double clip, double* __restrict__ stats) {
  __shared__ double sh[DP_THREADS];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partial; i += DP_THREADS) acc += partial[i];
  const double sumsq = block_sum(acc, sh);
  if (threadIdx.x == 0) {
    const double norm = __dsqrt_rn(sumsq);
    const float scale = norm > clip ? (float)__ddiv_rn(clip, norm) : 1.f;
    stats[0] = sumsq;
    stats[1] = norm;
    stats[2] = (double)scale;
  }
}

struct Philox {
  uint32_t k0, k1, d0, d1;   // key and draw, low word first

  static FEDMI_DEV void round(uint32_t (&c)[4], uint32_t ka, uint32_t kb) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ ka;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ kb;
    c[3] = lo0;
  }

  // the four 32-bit outputs of one block
  FEDMI_DEV void block(long blk, uint32_t (&c)[4]) const {
    c[0] = (uint32_t)blk;
    c[1] = (uint32_t)((unsigned long)blk >> 32);
    c[2] = d0;
    c[3] = d1;
    uint32_t ka = k0, kb = k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      round(c, ka, kb);
      ka += 0x9E3779B9u;
      kb += 0xBB67AE85u;
    }
  }
};

FEDMI_DEV float unit_open(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 0x1p-23f; }

// one Box-Muller pair from two 32-bit words: (radius * cos, radius * sin)
FEDMI_DEV void box_muller(uint32_t ra, uint32_t rb, float& gc, float& gs) {
  const float radius = sqrtf(-2.f * logf(unit_open(ra)));
  float s, c;
  sincospif(2.f * unit_open(rb), &s, &c);
  gc = radius * c;
  gs = radius * s;
}

template <bool NOISE>
struct DpApply {
  float* x;
  const float* anchor;
  const double* stats;
  float sigma;
  Philox rng;

  template <int W>
  FEDMI_DEV void run(long e) const {
    const float scale = (float)stats[2];
    if (!NOISE && scale == 1.f) return;          // nothing clipped, nothing added: no store
    auto xv = flat_load<W>(x, e);
    if (scale != 1.f) {
      const auto av = flat_load<W>(anchor, e);
#pragma unroll
      for (int j = 0; j < W; ++j) xv[j] = __fmaf_rn(scale, xv[j] - av[j], av[j]);
    }
    if (NOISE) {
      uint32_t r[4];
      rng.block(e >> 2, r);
      if (W == 4) {
        float g[4];
        box_muller(r[0], r[1], g[0], g[1]);
        box_muller(r[2], r[3], g[2], g[3]);
#pragma unroll
        for (int j = 0; j < W; ++j) xv[j] = __fmaf_rn(sigma, g[j], xv[j]);
      } else {                                   // the tail takes its lane of the same block
        const int lane = (int)(e & 3);
        float gc, gs;
        box_muller((lane & 2) ? r[2] : r[0], (lane & 2) ? r[3] : r[1], gc, gs);
        xv[0] = __fmaf_rn(sigma, (lane & 1) ? gs : gc, xv[0]);
      }
    }
    flat_store<W>(x, e, xv);
  }
};

}  // namespace

namespace fedmi {

// workgroups of dp_sumsq == partials it writes: a function of k only, at most 2048
int dp_partials(long k) { return k > 0 ? flat_grid(k) : 0; }

// stages: bit 0 dp_sumsq, bit 1 dp_finish, bit 2 the apply (7: the round's three launches; single stages are for
// timing).  x and anchor hold at least k floats and are 16-byte aligned, partial holds dp_partials(k) doubles and stats
// 3; clip > 0, sigma >= 0 (the binding checks all of it).  sigma == 0 launches the clip-only apply.
void launch_dp(hipStream_t st, float* x, const float* anchor, long k, double* partial, double* stats, double clip,
               float sigma, uint64_t key, uint64_t draw, int stages) {
  if (k <= 0) return;
  const int grid = dp_partials(k);
  if (stages & 1)
    hipLaunchKernelGGL(dp_sumsq_kernel, dim3(grid), dim3(DP_THREADS), 0, st, x, anchor, k, partial);
  if (stages & 2)
    hipLaunchKernelGGL(dp_finish_kernel, dim3(1), dim3(DP_THREADS), 0, st, partial, grid, clip, stats);
  if (stages & 4) {
    const Philox rng = {(uint32_t)key, (uint32_t)(key >> 32), (uint32_t)draw, (uint32_t)(draw >> 32)};
    if (sigma > 0.f)
      flat_map(st, k, DpApply<true>{x, anchor, stats, sigma, rng});
    else
      flat_map(st, k, DpApply<false>{x, anchor, stats, sigma, rng});
  }
}

}  // namespace fedmi
