// fedmi — what the rules built on an fp64 Gram pass share (krum.hip, bulyan.hip, dnc.hip): the grid and tile rules, the
// fold of the pass's partial tiles, the record's place, and the launchers of Krum's pass and of the mean of the record's
// rows (the kernels live in krum.hip).
#pragma once
#include "robust_fold.h"

namespace fedmi {

constexpr int KR_TILE = kRobustMaxRanks * kRobustMaxRanks;
constexpr int KR_MAX_GRID = 1024;                   // 256 CUs x 4 workgroups: the whole grid is resident
constexpr int KR_COLS_PER_WG = 1024;                // below the cap a workgroup takes this many columns

inline int krum_grid(long n) {
  long blocks = (n + KR_COLS_PER_WG - 1) / KR_COLS_PER_WG;
  return (int)(blocks < 1 ? 1 : blocks > KR_MAX_GRID ? KR_MAX_GRID : blocks);
}

inline int krum_tile(int W) { return W <= 4 ? 4 : W <= 8 ? 8 : 16; }

// partial[wg] = the workgroup's share of G = X X^T as krum_tile(W)^2 doubles, wg < krum_grid(n)  (krum.hip)
void launch_gram_pass(hipStream_t st, const float* rows, long ld, int W, long n, double* partial);

// the finish's record {count, the picked ranks ascending} (int32): the row of 256 doubles behind the pass's tiles
inline int* gram_record(double* partial, long n) { return reinterpret_cast<int*>(partial + (long)krum_grid(n) * KR_TILE); }

// out[i] = (x_s0[i] + x_s1[i] + ..) / (float)m over the record's rows, in fp32 in rank order  (krum.hip: krum_select)
void launch_krum_select(hipStream_t st, const float* rows, long ld, long n, const int* record, float* out);

// fold_partial_rows' sibling for tiles: n_partial rows of E = P * P doubles (E = 16, 64 or 256); returns in lane t the
// sum of entry t % E.  Lane (g, e), g = t / E, adds rows g, g + 1024 / E, .. in that order from 0, then a binary LDS
// tree folds the 1024 / E groups (slot += slot + s for s = 512 .. E).
FEDMI_DEV double fold_partial_tiles(const double* partial, int n_partial, int E) {
  __shared__ double sh[kFoldThreads];
  const int e = threadIdx.x % E, g = threadIdx.x / E;
  double acc = 0.0;
#pragma unroll 4
  for (int i = g; i < n_partial; i += kFoldThreads / E) acc += partial[(long)i * E + e];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kFoldThreads / 2; s >= E; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[e];
}

// The end of a one-round finish (krum_finish, dnc_finish), called by the whole workgroup once score[0 .. 16) stands in
// LDS behind a barrier (no NaN; 0.0 at and past W): the m clients of lowest (score, rank) into stats rows 0 (score) and
// 1 (1.0 / 0.0) and into the record {m, their ranks ascending}.
FEDMI_DEV void select_lowest(const double* score, int W, int m, double* stats, int* record) {
  __shared__ int chosen[kRobustMaxRanks];
  const int t = threadIdx.x;
  if (t < kRobustMaxRanks) {
    int before = 0;                                 // clients ahead of t in (score, rank)
    if (t < W)
      for (int o = 0; o < W; ++o) before += (score[o] < score[t] || (score[o] == score[t] && o < t)) ? 1 : 0;
    chosen[t] = (t < W && before < m) ? 1 : 0;
    stats[t] = score[t];
    stats[kRobustMaxRanks + t] = chosen[t] ? 1.0 : 0.0;
  }
  __syncthreads();
  if (t < kRobustMaxRanks) {
    int slot = 0;
    for (int o = 0; o < t; ++o) slot += chosen[o];
    if (chosen[t]) record[1 + slot] = t;
    if (t == 0) record[0] = m;
  }
}

}  // namespace fedmi
