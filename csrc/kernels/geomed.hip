// fedmi — geometric-median aggregation of the clients' gathered float states (fedmi/parallel/geomed.py): smoothed
// Weiszfeld (RFA, Pillutla et al. 2022) over a [W, ld] fp32 buffer, row r = client r's state.
//
//   geomed_pass<W, FIRST> :  z[i] = FIRST ? the mean of the finite x_r[i] : sum_r w_r x_r[i]   (fp32, rank order);
//                            partial[wg][r] = sum over the workgroup's coordinates of (x_r[i] - z[i])^2   (fp64)
//   geomed_finish         :  sumsq_r = sum of the partials;  dist_r = sqrt(sumsq_r);
//                            beta_r = isfinite(dist_r) ? 1 / max(nu, dist_r) : 0;  B = sum_r beta_r (rank order);
//                            w_r = B > 0 ? (float)(beta_r / B) : 1 / W;  history row t = {sumsq, dist, w}[16] (fp64)
// A round is pass 0 (FIRST) and T weighted passes, each followed by its finish: 2 (T + 1) launches on one stream, no
// host sync in between; pass t reads the weights that finish t - 1 wrote.  The result is the z of pass T.
//
// One pass reads every row exactly once and never reads z back: it is the row sweep of row_sweep.h with GeomedRule --
// a lane takes one float4 per row, forms the four z (coord), stores them with one 16-B store and then accumulates the
// W x 4 squared distances from the values still in registers (stored): (W + 1) * 4 B of traffic per coordinate.  The
// n % 4 entries after the whole vectors go through the same two calls.  Registers at W = 16: 64 of rows, 32 of fp64
// accumulators, 4 of z; the weights are wave-uniform and live in SGPRs.
//
// Determinism.  (x - z) is an fp32 number, so its square is exact in fp64 and the sums' only roundings are their
// additions, in a fixed order: a lane adds its grid-strided coordinates in index order; the workgroup folds its 256
// lanes per rank in a two-level 16-ary LDS tree (lane (r, j) adds the 16 entries j, j + 16, .. of rank r in that order,
// lane (r, 0) the 16 results); the finish folds the partials in 64 strided groups and an LDS tree (fold_partial_rows,
// robust_fold.h; tests/geomed_check.py emulates the whole order and the GPU test compares bits).  The grid is a
// function of n alone (flat_grid) and there are no atomics: the same rows give the same bits on every run and client.
#include <math.h>

#include "flat_map.h"
#include "robust_fold.h"
#include "row_sweep.h"

namespace {

using namespace fedmi;

constexpr int GM_THREADS = 256;
constexpr int GM_FAN = 16;                          // GM_THREADS == GM_FAN * GM_FAN: both levels of the tree
constexpr int GM_ROW = 3 * kRobustMaxRanks;         // one history row: sumsq[16], dist[16], w[16]

FEDMI_DEV bool gm_finite(float v) { return (__float_as_uint(v) & 0x7FFFFFFFu) < 0x7F800000u; }

// The rule for one coordinate, in two steps shared by the vector body and the tail.  x = its value on ranks 0 .. W-1,
// w = the ranks' weights (unused when FIRST).  A rank of weight 0 is skipped by a select, not multiplied: its NaN stays
// out of z.
template <int W, bool FIRST>
FEDMI_DEV float geomed_z(const float (&x)[W], const float (&w)[W]) {
  float s = 0.f;
  if (FIRST) {
    int count = 0;
#pragma unroll
    for (int r = 0; r < W; ++r) {
      const bool ok = gm_finite(x[r]);
      s = ok ? __fadd_rn(s, x[r]) : s;
      count += ok ? 1 : 0;
    }
    return __fdiv_rn(s, (float)count);              // no finite entry: 0 / 0 = NaN
  }
#pragma unroll
  for (int r = 0; r < W; ++r) s = w[r] != 0.f ? __fmaf_rn(w[r], x[r], s) : s;
  return s;
}

// acc[r] += (x_r - z)^2
template <int W>
FEDMI_DEV void geomed_acc(const float (&x)[W], float z, double (&acc)[W]) {
#pragma unroll
  for (int r = 0; r < W; ++r) {
    const double d = (double)__fsub_rn(x[r], z);
    acc[r] = __fma_rn(d, d, acc[r]);                // d * d is exact: one rounding, the addition's
  }
}

// The rule of one pass for row_sweep.h: z before the store, the fp64 sums after it, per rank in index order.
template <int W, bool FIRST>
struct GeomedRule {
  float w[W];
  double acc[W];
  FEDMI_DEV float coord(const float (&x)[W]) const { return geomed_z<W, FIRST>(x, w); }
  FEDMI_DEV void stored(const float (&x)[W], float z) { geomed_acc<W>(x, z, acc); }
};

template <int W, bool FIRST>
__global__ __launch_bounds__(GM_THREADS) void geomed_pass_kernel(const float* rows, long ld, long n, const float* w32,
                                                                 const double* w64, float* out, double* partial) {
  __shared__ double sh[W][GM_THREADS];
  GeomedRule<W, FIRST> rule;
#pragma unroll
  for (int r = 0; r < W; ++r) {                     // once per kernel, the same in every lane: scalar registers
    float v = 0.f;
    if (!FIRST) v = w32 ? w32[r] : (float)w64[r];
    rule.w[r] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
    rule.acc[r] = 0.0;
  }
  row_sweep<W>(StridedRows{rows, ld}, n, out, rule);   // z leaves before the fp64 work and is never read back
  // the workgroup's sum per rank: 256 lanes -> 16 -> 1, each level 16 additions in a fixed order
#pragma unroll
  for (int r = 0; r < W; ++r) sh[r][threadIdx.x] = rule.acc[r];
  __syncthreads();
  const int r = threadIdx.x / GM_FAN, j = threadIdx.x % GM_FAN;
  if (r < W) {
    double s = sh[r][j];
#pragma unroll
    for (int k = 1; k < GM_FAN; ++k) s += sh[r][j + GM_FAN * k];
    sh[r][j] = s;                                   // (no other lane reads or writes slot j of rank r at this level)
  }
  __syncthreads();
  if (r < W && j == 0) {
    double s = sh[r][0];
#pragma unroll
    for (int k = 1; k < GM_FAN; ++k) s += sh[r][k];
    partial[(long)blockIdx.x * kRobustMaxRanks + r] = s;
  }
}

// fold_partial_rows on fp64 (its order is part of the rule's bits), then lanes r < W form the weights
__global__ __launch_bounds__(kFoldThreads) void geomed_finish_kernel(const double* partial, int n_partial, int W,
                                                                     double nu, int t, double* history) {
  __shared__ double beta[kRobustMaxRanks];
  const double sum = fold_partial_rows(partial, n_partial, W);
  const bool mine = (int)threadIdx.x < W;
  double sumsq = 0.0, dist = 0.0;
  if (mine) {
    sumsq = sum;
    dist = __dsqrt_rn(sumsq);
    beta[threadIdx.x] = isfinite(dist) ? __ddiv_rn(1.0, fmax(nu, dist)) : 0.0;
  }
  __syncthreads();
  if (mine) {
    double B = 0.0;
    for (int q = 0; q < W; ++q) B += beta[q];       // rank order, the same bits in every lane
    const float w = B > 0.0 ? (float)__ddiv_rn(beta[threadIdx.x], B) : __fdiv_rn(1.f, (float)W);
    double* row = history + (long)t * GM_ROW;
    row[threadIdx.x] = sumsq;
    row[kRobustMaxRanks + threadIdx.x] = dist;
    row[2 * kRobustMaxRanks + threadIdx.x] = (double)w;
  }
}

}  // namespace

namespace fedmi {

// workgroups of a pass == rows of double[16] partials it writes: a function of n only, at most 2048
int geomed_partials(long n) { return n > 0 ? flat_grid(n) : 0; }

// One pass and its finish.  first: pass 0 (the weights are not read); otherwise the W weights come from w32 (fp32)
// if it is non-null, else from w64 (fp64 holding fp32 values: the w column of a history row).  Writes row t of
// history.  Buffers as launch_geomed.
void launch_geomed_pass(hipStream_t st, const float* rows, long ld, int W, long n, bool first, const float* w32,
                        const double* w64, double nu, float* out, double* partial, double* history, int t) {
  if (n <= 0) return;
  const int grid = geomed_partials(n);
  robust_dispatch(W, [&](auto w) {
    constexpr int kW = decltype(w)::value;
    if (first)
      hipLaunchKernelGGL((geomed_pass_kernel<kW, true>), dim3(grid), dim3(GM_THREADS), 0, st, rows, ld, n, w32, w64,
                         out, partial);
    else
      hipLaunchKernelGGL((geomed_pass_kernel<kW, false>), dim3(grid), dim3(GM_THREADS), 0, st, rows, ld, n, w32, w64,
                         out, partial);
  });
  hipLaunchKernelGGL(geomed_finish_kernel, dim3(1), dim3(kFoldThreads), 0, st, partial, grid, W, nu, t, history);
}

// rows: W rows of ld floats, 16-byte aligned, ld % 4 == 0, ld >= n; out: n floats, 16-byte aligned, not aliasing rows;
// partial: geomed_partials(n) x 16 doubles; history: (T + 1) x 3 x 16 doubles; 2 <= W <= 16, 1 <= T <= 64, nu > 0
// (the binding checks all of it).  out = the z of pass T; history row T - 1's w formed it, row T's dist measures it.
void launch_geomed(hipStream_t st, const float* rows, long ld, int W, long n, int T, double nu, float* out,
                   double* partial, double* history) {
  for (int t = 0; t <= T; ++t)
    launch_geomed_pass(st, rows, ld, W, n, t == 0, nullptr,
                       t ? history + (long)(t - 1) * GM_ROW + 2 * kRobustMaxRanks : nullptr, nu, out, partial, history,
                       t);
}

}  // namespace fedmi
