// fedmi — Krum / multi-Krum aggregation of the clients' gathered float states (fedmi/parallel/krum.py; Blanchard et
// al. 2017) over a [W, ld] fp32 buffer, row r = client r's state.  Three launches on one stream, no host sync:
//
//   krum_gram<P>  :  partial[wg] = the workgroup's share of G = X X^T (fp64), P = 4 / 8 / 16 = the smallest >= W
//   krum_finish   :  G = the sum of the partials;  d[i][j] = (G[i][i] + G[j][j]) - 2 G[i][j], clamped below at 0, +inf
//                    if not finite;  score[i] = the k smallest d[i][j], j != i, added in ascending (d, j) order;
//                    selected = the m clients of lowest (score, rank);  stats = [18][16] fp64: row 0 score, row 1
//                    selected (1.0 / 0.0), rows 2 .. 17 d;  record = {m, the selected ranks ascending} (int32)
//   krum_select   :  z[i] = (x_s0[i] + x_s1[i] + ..) / (float)m over the record's rows, __fadd_rn in rank order and one
//                    __fdiv_rn: (m + 1) * 4 B per entry; m = 1 is a bit-exact copy of the winner
//
// The Gram pass.  The W (W - 1) / 2 distances cannot live in a lane's registers the way geomed_pass keeps its W sums;
// they are exactly one fp64 MFMA tile.  v_mfma_f64_16x16x4_f64 computes D[i][j] += sum_{k<4} A[i][k] B[k][j] with lane
// l = (r = l % 16, q = l / 16) holding A[r][q] and B[q][r] -- with B = A^T both operands are the SAME register, and any
// assignment of columns to (step, q) is a valid sum.  Lane (r, q) loads the float4 at columns c .. c + 3, c = base +
// 16 g + 4 q, of client r % P, converts the four floats (every product of two fp32 values is exact in fp64: the only
// roundings are the additions) and issues four MFMAs, alternating two accumulator tiles so that consecutive MFMAs do
// not depend on each other.  For P < 16 the tile is folded: lane row r serves client r % P in column group g = r / P,
// so one step covers 16 / P groups of 16 columns and the 16 / P diagonal P x P blocks of the tile each hold a partial
// Gram of disjoint columns; the off-diagonal blocks mix column groups and are never read.  Rows of clients >= W load
// nothing and feed 0.0; entries at or past n go in as 0.0 by a select (the buffer's padding is never trusted).  The
// accumulator of lane l holds D[4 v + l / 16][l % 16] in its double v (the f64 tile's layout: one row per register,
// unlike the fp32 tiles' four consecutive rows per lane).  A client's NaN reaches D[i][j] only through row i or j.
//
// Determinism.  A wave takes chunks of 4 steps, grid-strided; the grid is a function of n alone and the order of every
// sum a function of W and n: step and MFMA order in the wave, tile 0 + tile 1, the four waves through LDS in wave order;
// the diagonal blocks in block order, the partials in strided groups and an LDS tree (fold_partial_tiles).  No atomics.
#include <math.h>

#include "flat_map.h"
#include "krum_gram.h"
#include "robust_fold.h"

namespace {

using namespace fedmi;

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int KR_THREADS = 256;
constexpr int KR_WAVES = KR_THREADS / 64;
constexpr int KR_STEPS = 4;                         // steps per chunk: four 16-B loads in flight per lane
constexpr int KR_STATS_ROWS = 2 + kRobustMaxRanks;

template <int P>
__global__ __launch_bounds__(KR_THREADS) void krum_gram_kernel(const float* rows, long ld, int W, long n,
                                                               double* partial) {
  static_assert(P == 4 || P == 8 || P == 16, "the tile holds 16 / P diagonal blocks");
  constexpr int GROUPS = 16 / P;
  constexpr long STEP = 16 * GROUPS, CHUNK = KR_STEPS * STEP;   // columns per step and per chunk of a wave
  __shared__ double sh[KR_WAVES][KR_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int client = r % P, group = r / P;
  const bool live = client < W;
  const float* row = rows + (long)(live ? client : 0) * ld + 16 * group + 4 * q;
  const long first = 16 * group + 4 * q;

  double4_t acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
  for (long base = ((long)blockIdx.x * KR_WAVES + wave) * CHUNK; base < n; base += (long)gridDim.x * KR_WAVES * CHUNK) {
    float4 x[KR_STEPS];
#pragma unroll
    for (int u = 0; u < KR_STEPS; ++u) {            // c < n and ld % 4 == 0, ld >= n: the vector lies inside the row
      const long c = base + u * STEP;
      x[u] = (live && c + first < n) ? *reinterpret_cast<const float4*>(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < KR_STEPS; ++u) {
      const long left = n - (base + u * STEP + first);   // entries of this vector before n
      const float v[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double a = (double)(k < left ? v[k] : 0.f);
        acc[k & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc[k & 1], 0, 0, 0);
      }
    }
  }
  // tile 0 + tile 1, then into LDS as D[i][j]: register v of lane (r, q) is row 4 v + q, column r
#pragma unroll
  for (int v = 0; v < 4; ++v) sh[wave][(4 * v + q) * 16 + r] = acc[0][v] + acc[1][v];
  __syncthreads();
  // the workgroup's partial: entry (i, j), i, j < P = the diagonal blocks in block order, each the waves in wave order
  if ((int)threadIdx.x < P * P) {
    const int i = threadIdx.x / P, j = threadIdx.x % P;
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < GROUPS; ++b) {
      const int e = (b * P + i) * 16 + b * P + j;
      const double t = ((sh[0][e] + sh[1][e]) + sh[2][e]) + sh[3][e];
      s = b == 0 ? t : s + t;
    }
    partial[(long)blockIdx.x * (P * P) + threadIdx.x] = s;
  }
}

// One workgroup.  gram != null: only G is written ([16][16], 0 outside W x W) -- the test's entry.  Otherwise stats and
// the record.  G is read from its upper triangle, so it is symmetric whatever the tile holds.
__global__ __launch_bounds__(kFoldThreads) void krum_finish_kernel(const double* partial, int n_partial, int P, int W,
                                                                   int k, int m, double* gram, double* stats,
                                                                   int* record) {
  __shared__ double G[kRobustMaxRanks][kRobustMaxRanks], d[kRobustMaxRanks][kRobustMaxRanks];
  __shared__ double near[kRobustMaxRanks][kRobustMaxRanks], score[kRobustMaxRanks];
  const double sum = fold_partial_tiles(partial, n_partial, P * P);
  const int t = threadIdx.x;
  if (t < P * P) G[t / P][t % P] = sum;
  __syncthreads();
  const int i = t / kRobustMaxRanks, j = t % kRobustMaxRanks;
  const bool pair = t < KR_TILE && i < W && j < W;
  if (gram) {
    if (t < KR_TILE) gram[t] = pair ? G[i < j ? i : j][i < j ? j : i] : 0.0;
    return;
  }
  if (t < KR_TILE) {
    double v = 0.0;
    if (pair && i != j) {
      v = __dsub_rn(__dadd_rn(G[i][i], G[j][j]), __dmul_rn(2.0, G[i < j ? i : j][i < j ? j : i]));
      v = isfinite(v) ? (v < 0.0 ? 0.0 : v) : INFINITY;
    }
    d[i][j] = v;
    stats[2 * kRobustMaxRanks + t] = v;
  }
  __syncthreads();
  if (pair && i != j) {                             // row i in ascending (d, j) order: every pair finds its own place
    int place = 0;
    for (int o = 0; o < W; ++o)
      place += (o != i && (d[i][o] < d[i][j] || (d[i][o] == d[i][j] && o < j))) ? 1 : 0;
    near[i][place] = d[i][j];
  }
  __syncthreads();
  if (t < kRobustMaxRanks) {                        // the k smallest, added in that order
    double s = 0.0;
    if (t < W) {
      s = near[t][0];
      for (int c = 1; c < k; ++c) s += near[t][c];
    }
    score[t] = s;
  }
  __syncthreads();
  select_lowest(score, W, m, stats, record);
}

// The mean of the record's rows, as an operation of flat_map.h.  m and the ranks are the same in every lane: the row
// pointers are wave-uniform.
struct KrumSelect {
  const float* rows;
  long ld;
  const int* record;
  float* out;
  template <int V>
  FEDMI_DEV void run(long e) const {
    const int m = record[0];
    FlatVec<V> z = flat_load<V>(rows + (long)record[1] * ld, e);   // the first selected row starts the sum
    for (int s = 1; s < m; ++s) {
      const FlatVec<V> x = flat_load<V>(rows + (long)record[1 + s] * ld, e);
#pragma unroll
      for (int j = 0; j < V; ++j) z[j] = __fadd_rn(z[j], x[j]);
    }
    const float div = (float)m;
#pragma unroll
    for (int j = 0; j < V; ++j) z[j] = __fdiv_rn(z[j], div);
    flat_store<V>(out, e, z);
  }
};

}  // namespace

namespace fedmi {

void launch_gram_pass(hipStream_t st, const float* rows, long ld, int W, long n, double* partial) {
  const int grid = krum_grid(n);
  switch (krum_tile(W)) {
    case 4: hipLaunchKernelGGL(krum_gram_kernel<4>, dim3(grid), dim3(KR_THREADS), 0, st, rows, ld, W, n, partial); break;
    case 8: hipLaunchKernelGGL(krum_gram_kernel<8>, dim3(grid), dim3(KR_THREADS), 0, st, rows, ld, W, n, partial); break;
    default: hipLaunchKernelGGL(krum_gram_kernel<16>, dim3(grid), dim3(KR_THREADS), 0, st, rows, ld, W, n, partial);
  }
}

void launch_krum_select(hipStream_t st, const float* rows, long ld, long n, const int* record, float* out) {
  flat_map(st, n, KrumSelect{rows, ld, record, out});
}

// rows of 256 doubles in `partial`: one per workgroup of the Gram pass (a function of n only, at most 1024) and one
// for the record
int krum_partials(long n) { return n > 0 ? krum_grid(n) + 1 : 0; }

// the rule's counts at W clients (fedmi/parallel/krum.py): F_eff, then k and m
void krum_counts(int W, int byz, bool multi, int* k, int* m) {
  int f = (W - 3) / 2;
  f = byz < f ? byz : f;
  f = f < 0 ? 0 : f;
  *k = W - f - 2 < 1 ? 1 : W - f - 2;
  *m = multi ? W - f : 1;
}

// G as [16][16] doubles (0 outside W x W) into gram; buffers as launch_krum
void launch_krum_gram(hipStream_t st, const float* rows, long ld, int W, long n, double* partial, double* gram) {
  if (n <= 0) return;
  launch_gram_pass(st, rows, ld, W, n, partial);
  hipLaunchKernelGGL(krum_finish_kernel, dim3(1), dim3(kFoldThreads), 0, st, partial, krum_grid(n), krum_tile(W), W, 0,
                     0, gram, nullptr, nullptr);
}

// rows: W rows of ld floats, 16-byte aligned, ld % 4 == 0, ld >= n; out: n floats, 16-byte aligned, not aliasing rows;
// partial: krum_partials(n) x 256 doubles; stats: 18 x 16 doubles; 2 <= W <= 16, byz >= 0 (the binding checks all of it)
void launch_krum(hipStream_t st, const float* rows, long ld, int W, long n, int byz, bool multi, float* out,
                 double* partial, double* stats) {
  if (n <= 0) return;
  int k, m;
  krum_counts(W, byz, multi, &k, &m);
  const int grid = krum_grid(n);
  int* record = gram_record(partial, n);
  launch_gram_pass(st, rows, ld, W, n, partial);
  hipLaunchKernelGGL(krum_finish_kernel, dim3(1), dim3(kFoldThreads), 0, st, partial, grid, krum_tile(W), W, k, m,
                     nullptr, stats, record);
  launch_krum_select(st, rows, ld, n, record, out);
}

}  // namespace fedmi
