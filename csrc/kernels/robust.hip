// fedmi — Byzantine-robust aggregation of the clients' gathered float states (fedmi/parallel/robust.py): the
// coordinate-wise median or trimmed mean of robust_fold.h over a [W, ld] fp32 buffer, row r = client r's state.
//
//   robust_reduce :  out[i] = fold(rows[0][i] .. rows[W-1][i], b) for i < n;  partial[wg][r] = the number of the
//                    workgroup's coordinates at which rank r's entry fell outside the kept window (int64)
//   robust_finish :  stats[r] = sum over the workgroups of partial[wg][r], r < W (int64; entries past W are left alone)
//
// Rows start every ld floats (ld % 4 == 0, ld >= n), so every row is 16-byte aligned and a lane reads one float4 per
// row: 4 coordinates, W independent 16-B loads in flight.  The n % 4 entries after the whole vectors go one by one
// through the same fold, so body and tail cannot differ.  Grid: flat_grid(n), grid-strided.
//
// Determinism.  The fold orders by (key, rank), never by arrival, so out is a function of the rows alone; the cut counts
// are integers, summed per wave by shuffles, per workgroup by integer LDS atomics and over the workgroups by
// robust_finish.  No float atomics: the same rows give the same bits on every run and on every client.
//
// Cost per coordinate: (W + 1) * 4 B of traffic and 66 / 127 / 286 / 699 VALU instructions at W = 2 / 4 / 8 / 16
// (counted; 6 per compare-exchange, robust_fold.h).
#include "flat_map.h"
#include "robust_fold.h"

namespace {

using namespace fedmi;

constexpr int RB_THREADS = 256;

// (no __restrict__ and no unrolled trips: either lets the compiler hoist the next trips' W loads over the fold, which
// at W >= 3 took all 256 VGPRs and spilled)
template <int W>
__global__ __launch_bounds__(RB_THREADS) void robust_reduce_kernel(const float* rows, long ld, long n, int b,
                                                                   float* out, long long* partial) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  RobustCuts<W> cuts;
#pragma unroll 1
  for (long i = t; i < n4; i += stride) {
    FlatVec<4> v[W], o;
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = flat_load<4>(rows + r * ld, i << 2);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float x[W];
#pragma unroll
      for (int r = 0; r < W; ++r) x[r] = v[r][c];
      uint32_t cut;
      o[c] = robust_fold<W>(x, b, cut);
      cuts.add(cut);
    }
    flat_store<4>(out, i << 2, o);
  }
#pragma unroll 1
  for (long i = (n4 << 2) + t; i < n; i += stride) {   // tail (n % 4 entries)
    float x[W];
#pragma unroll
    for (int r = 0; r < W; ++r) x[r] = rows[r * ld + i];
    uint32_t cut;
    out[i] = robust_fold<W>(x, b, cut);
    cuts.add(cut);
  }
  cuts.store(partial + (long)blockIdx.x * kRobustMaxRanks);
}

// one workgroup of 1024: the 2048 x 16 partials of a large state are 32 dependent-latency trips per lane, not 128
constexpr int RF_THREADS = 1024;

__global__ __launch_bounds__(RF_THREADS) void robust_finish_kernel(const long long* __restrict__ partial,
                                                                   int n_partial, int W,
                                                                   long long* __restrict__ stats) {
  __shared__ long long sh[RF_THREADS];
  const int r = threadIdx.x & (kRobustMaxRanks - 1), g = threadIdx.x / kRobustMaxRanks;
  long long acc = 0;
#pragma unroll 4
  for (int i = g; i < n_partial; i += RF_THREADS / kRobustMaxRanks) acc += partial[(long)i * kRobustMaxRanks + r];
  sh[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int s = RF_THREADS / 2; s >= kRobustMaxRanks; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if ((int)threadIdx.x < W) stats[threadIdx.x] = sh[threadIdx.x];
}

}  // namespace

namespace fedmi {

// workgroups of robust_reduce == rows of int64[16] partials it writes: a function of n only, at most 2048
int robust_partials(long n) { return n > 0 ? flat_grid(n) : 0; }

// stats[r] (r < W) = the column sums of n_partial rows of partials; also finishes the fused peer kernel's partials
void launch_robust_finish(hipStream_t st, const long long* partial, int n_partial, int W, long long* stats) {
  hipLaunchKernelGGL(robust_finish_kernel, dim3(1), dim3(RF_THREADS), 0, st, partial, n_partial, W, stats);
}

// rows: W rows of ld floats, 16-byte aligned, ld % 4 == 0, ld >= n; out: n floats, 16-byte aligned (it may be one
// of the rows' owners' state but must not alias rows); partial: robust_partials(n) x 16 int64; stats: 16 int64;
// 2 <= W <= 16, 0 <= b <= (W - 1) / 2 (the binding checks all of it)
void launch_robust_reduce(hipStream_t st, const float* rows, long ld, int W, long n, int b, float* out,
                          long long* partial, long long* stats) {
  if (n <= 0) return;
  const int grid = robust_partials(n);
  robust_dispatch(W, [&](auto w) {
    hipLaunchKernelGGL(robust_reduce_kernel<decltype(w)::value>, dim3(grid), dim3(RB_THREADS), 0, st, rows, ld, n, b,
                       out, partial);
  });
  launch_robust_finish(st, partial, grid, W, stats);
}

}  // namespace fedmi
