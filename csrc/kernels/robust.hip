// fedmi — Byzantine-robust aggregation of the clients' gathered float states (fedmi/parallel/robust.py): the
// coordinate-wise median or trimmed mean of robust_fold.h over a [W, ld] fp32 buffer, row r = client r's state.
//
//   robust_reduce :  out[i] = fold(rows[0][i] .. rows[W-1][i], b) for i < n;  partial[wg][r] = the number of the
//                    workgroup's coordinates at which rank r's entry fell outside the kept window (int64)
//   robust_finish :  stats[r] = sum over the workgroups of partial[wg][r], r < W (int64; entries past W are left alone)
//
// Rows start every ld floats (ld % 4 == 0, ld >= n), so every row is 16-byte aligned.  robust_reduce is the row sweep
// of row_sweep.h (one float4 per row and lane, the n % 4 tail through the same rule) with RobustRule, then the
// workgroup's cut counts; robust_finish is fold_partial_rows on int64.  Grid: flat_grid(n), grid-strided.
//
// Determinism.  The fold orders by (key, rank), never by arrival, so out is a function of the rows alone; the cut counts
// are integers, summed per wave by shuffles, per workgroup by integer LDS atomics and over the workgroups by
// robust_finish.  No float atomics: the same rows give the same bits on every run and on every client.
//
// Cost per coordinate: (W + 1) * 4 B of traffic and 66 / 127 / 286 / 699 VALU instructions at W = 2 / 4 / 8 / 16
// (counted; 6 per compare-exchange, robust_fold.h).
#include "flat_map.h"
#include "robust_fold.h"
#include "row_sweep.h"

namespace {

using namespace fedmi;

constexpr int RB_THREADS = 256;

template <int W>
__global__ __launch_bounds__(RB_THREADS) void robust_reduce_kernel(const float* rows, long ld, long n, int b,
                                                                   float* out, long long* partial) {
  RobustRule<W> rule{b};
  row_sweep<W>(StridedRows{rows, ld}, n, out, rule);
  rule.cuts.store(partial + (long)blockIdx.x * kRobustMaxRanks);
}

__global__ __launch_bounds__(kFoldThreads) void robust_finish_kernel(const long long* partial, int n_partial, int W,
                                                                     long long* stats) {
  const long long sum = fold_partial_rows(partial, n_partial, W);
  if ((int)threadIdx.x < W) stats[threadIdx.x] = sum;
}

}  // namespace

namespace fedmi {

// workgroups of robust_reduce == rows of int64[16] partials it writes: a function of n only, at most 2048
int robust_partials(long n) { return n > 0 ? flat_grid(n) : 0; }

// stats[r] (r < W) = the column sums of n_partial rows of partials; also finishes the fused peer kernel's partials
void launch_robust_finish(hipStream_t st, const long long* partial, int n_partial, int W, long long* stats) {
  hipLaunchKernelGGL(robust_finish_kernel, dim3(1), dim3(kFoldThreads), 0, st, partial, n_partial, W, stats);
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
