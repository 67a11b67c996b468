// fedmi — Bulyan aggregation of the clients' gathered float states (fedmi/parallel/bulyan.py; El Mhamdi, Guerraoui and
// Rouault 2018) over a [W, ld] fp32 buffer, row r = client r's state: Krum, run again and again, picks theta = W - 2 F
// clients, and per coordinate the beta = theta - 2 F of their values closest to the median are averaged.  Four
// launches on one stream, no host sync:
//
//   krum_gram<P>     :  krum.hip's Gram pass, unchanged: partial[wg] = the workgroup's share of G = X X^T (fp64)
//   bulyan_finish    :  G, d[i][j] as krum_finish forms them, then theta rounds over the alive set A (all W at first):
//                       k = max(1, |A| - F - 2), score[i] = the k smallest d[i][j], j in A \ {i}, added in ascending
//                       (d, j) order (0.0 for a lone client), the client of lowest (score, rank) is picked and leaves A;
//                       stats rows 0 .. 17 = score when picked (never picked: in the last round), round picked (1-based,
//                       0 = never), d;  record = {theta, the picked ranks ascending} (int32)
//   bulyan_fold<TH>  :  the row sweep over the record's TH rows with BulyanRule: out[i] and, per workgroup, the number
//                       of coordinates at which each selected client's value was dropped;  (TH + 1) * 4 B per entry
//   bulyan_cut       :  stats row 18 = the column sums of those partials (fold_partial_rows on int64, exact), as
//                       doubles at the clients' ORIGINAL ranks; 0.0 for a client that was not selected
//
// The finish.  d (2 KiB) and the alive mask stay in LDS for all rounds.  Per round, pair (i, j) of alive clients finds
// the place of d[i][j] in row i's alive entries by counting, as krum_finish does (256 lanes, 16 compares each); after
// one barrier the first 16 lanes add their k nearest in order and rank the scores among themselves by wave shuffles
// (they are one wave: no barrier between the two), and the winner clears its bit: two barriers per round, at most 16
// rounds.  Rounds with k = 1 hold exact ties (the mutually nearest pair share one number); the rank settles them.
//
// The fold.  A lane sorts the TH values of a coordinate with robust_fold.h's network (keys (robust_key, position in the
// record); the record is ascending, so that IS rank order), takes the median, and drops c = 2 F values one at a time
// from whichever end of the window lies further from it (ties: the high end).  Every lane ends with its own number `a`
// of values dropped at the low end, 0 <= a <= c, and `a` must never index a register.  So:
//   * only the c positions at either end can be dropped: their distance keys are formed once (at most 12);
//   * step s of the greedy (s < c, c the same in every lane: a scalar branch) needs dist[a] and dist[TH-1-(s-a)] with
//     a <= s: two select chains over the s + 1 values `a` can have -- for c = 6, 15 compares and 30 selects in all;
//   * the window sum runs over ALL positions in order from -0.0f, a dropped one adding -0.0f: x + (-0.0f) == x for
//     every x, -0.0f included, so the bits are those of a sum that starts at the first kept value and adds the rest in
//     position order -- c more adds and 2 c selects, not a (c + 1)-way select per kept position;
//   * a position's cut bit is the same window test; positions c .. TH-1-c are always kept and cost nothing.
// The merge-of-two-descending-lists shortcut (position i < c is dropped iff i + #{j < c : dist[TH-1-j] >= dist[i]} < c)
// is NOT used: with a median of -inf the low side's distances are NaN next to the median and inf further out, the
// lists are not descending, and the shortcut and the greedy part (tests/test_bulyan_gpu.py holds such columns).
//
// Determinism: as krum.hip for G; every later step is a function of G and the rows alone (integer cut counts, summed by
// shuffles, integer LDS atomics and the fold).  No float atomics.
#include <math.h>

#include "flat_map.h"
#include "krum_gram.h"
#include "robust_fold.h"
#include "row_sweep.h"

namespace {

using namespace fedmi;

constexpr int BY_THREADS = 256;
constexpr int BY_MAX_CUT = 6;                       // c = 2 F_eff <= 2 ((16 - 3) / 4)
constexpr int BY_CUT_ROW = 2 + kRobustMaxRanks;     // stats row 18

struct BulyanRanks {                                // a record passed by value (the test's entry)
  int n;
  int rank[kRobustMaxRanks];
};

__global__ void bulyan_record_kernel(BulyanRanks ranks, int* record) {
  const int t = threadIdx.x;
  if (t == 0) record[0] = ranks.n;
  if (t < ranks.n) record[1 + t] = ranks.rank[t];
}

// One workgroup.  f = F_eff, theta = W - 2 f.  G is read from its upper triangle, so d is symmetric bit for bit.
__global__ __launch_bounds__(kFoldThreads) void bulyan_finish_kernel(const double* partial, int n_partial, int P, int W,
                                                                     int f, int theta, double* stats, int* record) {
  __shared__ double G[kRobustMaxRanks][kRobustMaxRanks], d[kRobustMaxRanks][kRobustMaxRanks];
  __shared__ double near[kRobustMaxRanks][kRobustMaxRanks];
  __shared__ unsigned alive_sh;
  const double sum = fold_partial_tiles(partial, n_partial, P * P);
  const int t = threadIdx.x;
  if (t < P * P) G[t / P][t % P] = sum;
  if (t == 0) alive_sh = (1u << W) - 1u;
  __syncthreads();
  const int i = t / kRobustMaxRanks, j = t % kRobustMaxRanks;
  const bool pair = t < KR_TILE && i < W && j < W && i != j;
  if (t < KR_TILE) {
    double v = 0.0;
    if (pair) {
      v = __dsub_rn(__dadd_rn(G[i][i], G[j][j]), __dmul_rn(2.0, G[i < j ? i : j][i < j ? j : i]));
      v = isfinite(v) ? (v < 0.0 ? 0.0 : v) : INFINITY;
    }
    d[i][j] = v;
    stats[2 * kRobustMaxRanks + t] = v;
  }
  __syncthreads();
  double score = 0.0;                               // lanes 0 .. 15: the client's score in its last round alive
  int picked = 0;                                   // and the round in which it was picked
  for (int r = 0; r < theta; ++r) {
    const unsigned alive = alive_sh;
    const int count = W - r;
    const int k = count - f - 2 < 1 ? 1 : count - f - 2;
    if (pair && ((alive >> i) & (alive >> j) & 1u)) {   // row i's alive entries in ascending (d, j) order
      const double mine = d[i][j];
      int place = 0;
      for (int o = 0; o < W; ++o) {
        const double other = d[i][o];
        place += (o != i && ((alive >> o) & 1u) && (other < mine || (other == mine && o < j))) ? 1 : 0;
      }
      near[i][place] = mine;
    }
    __syncthreads();
    if (t < 64) {                                   // one wave: the 16 clients' lanes rank each other by shuffles
      const bool live = t < W && ((alive >> t) & 1u);
      double s = INFINITY;
      if (live) {
        s = 0.0;                                    // a lone alive client
        if (count > 1) {
          s = near[t][0];
          for (int c = 1; c < k; ++c) s += near[t][c];
        }
      }
      int before = 0;                               // alive clients ahead of t in (score, rank): no score is NaN
      for (int o = 0; o < W; ++o) {
        const double so = __shfl(s, o, 64);
        before += (((alive >> o) & 1u) && (so < s || (so == s && o < t))) ? 1 : 0;
      }
      if (live) {
        score = s;
        if (before == 0) {
          picked = r + 1;
          alive_sh = alive & ~(1u << t);
        }
      }
    }
    __syncthreads();
  }
  if (t < kRobustMaxRanks) {
    const unsigned chosen = ((1u << W) - 1u) & ~alive_sh;
    stats[t] = t < W ? score : 0.0;
    stats[kRobustMaxRanks + t] = (double)picked;
    if ((chosen >> t) & 1u) record[1 + __popc(chosen & ((1u << t) - 1u))] = t;
    if (t == 0) record[0] = theta;
  }
}

// The record's rows.  The ranks are the same in every lane, so the pointers are wave-uniform; a rank outside 0 .. W-1
// (no finish writes one) is clamped, so that no record can send a load outside the buffer.
template <int TH>
struct RecordRows {
  const float* row[TH];
  FEDMI_DEV RecordRows(const float* rows, long ld, int W, const int* record) {
#pragma unroll
    for (int s = 0; s < TH; ++s) {
      const int r = record[1 + s];
      row[s] = rows + (long)(r < 0 ? 0 : r > W - 1 ? W - 1 : r) * ld;
    }
  }
  FEDMI_DEV const float* operator()(int s) const { return row[s]; }
};

// "The beta values closest to the median" as a rule of row_sweep.h; c = TH - beta is even, 0 <= c <= 6, c < TH, the
// same in every lane.  x is in record order; bit s of a cut mask is the record's s-th client.
template <int TH>
struct BulyanRule {
  static_assert(TH >= 2 && TH <= kRobustMaxRanks, "2 .. 16 selected clients");
  static constexpr int E = TH - 1 < BY_MAX_CUT ? TH - 1 : BY_MAX_CUT;   // positions that can be dropped at either end
  int c;
  RobustCuts<TH> cuts;

  FEDMI_DEV static uint32_t dist_key(float v, float med) { return robust_key(fabsf(__fsub_rn(v, med))); }

  FEDMI_DEV float coord(const float (&x)[TH]) {
    uint64_t k[TH];
#pragma unroll
    for (int s = 0; s < TH; ++s) k[s] = ((uint64_t)robust_key(x[s]) << 32) | (uint32_t)s;
    robust_sort<TH>(k, std::make_index_sequence<robust_net(TH).count>{});
    float v[TH];
#pragma unroll
    for (int p = 0; p < TH; ++p) v[p] = robust_unkey((uint32_t)(k[p] >> 32));
    const float med = (TH & 1) ? v[TH / 2] : __fdiv_rn(__fadd_rn(v[TH / 2 - 1], v[TH / 2]), 2.f);
    uint32_t lo_key[E], hi_key[E];                  // of positions q and TH - 1 - q
#pragma unroll
    for (int q = 0; q < E; ++q) {
      lo_key[q] = dist_key(v[q], med);
      hi_key[q] = dist_key(v[TH - 1 - q], med);
    }
    int a = 0;                                      // values dropped at the low end so far: the window is
#pragma unroll                                      // [a, TH - 1 - (s - a)] before step s
    for (int s = 0; s < E; ++s) {
      if (s < c) {
        uint32_t lo = lo_key[0], hi = hi_key[s];
#pragma unroll
        for (int q = 1; q <= s; ++q) {
          const bool at = a == q;
          lo = at ? lo_key[q] : lo;
          hi = at ? hi_key[s - q] : hi;
        }
        a += hi >= lo ? 0 : 1;
      }
    }
    const int top = TH - 1 - c + a;                 // the last kept position
    float sum = -0.f;
    uint32_t cut = 0u;
#pragma unroll
    for (int p = 0; p < TH; ++p) {
      if (p < E || p >= TH - E) {
        const bool out = (p < E && p < a) || (p >= TH - E && p > top);
        sum = __fadd_rn(sum, out ? -0.f : v[p]);
        cut |= out ? 1u << ((uint32_t)k[p] & 31u) : 0u;
      } else {
        sum = __fadd_rn(sum, v[p]);
      }
    }
    cuts.add(cut);
    return __fdiv_rn(sum, (float)(TH - c));
  }
  FEDMI_DEV void stored(const float (&)[TH], float) {}
};

template <int TH>
__global__ __launch_bounds__(BY_THREADS) void bulyan_fold_kernel(const float* rows, long ld, int W, long n,
                                                                 const int* record, int c, float* out,
                                                                 long long* partial) {
  const RecordRows<TH> chosen(rows, ld, W, record);
  BulyanRule<TH> rule{c};
  row_sweep<TH>(chosen, n, out, rule);
  rule.cuts.store(partial + (long)blockIdx.x * kRobustMaxRanks);
}

// row[r] = the number of coordinates at which client r's value was dropped, r < 16: column s of the partials belongs
// to the record's s-th client
__global__ __launch_bounds__(kFoldThreads) void bulyan_cut_kernel(const long long* partial, int n_partial, int theta,
                                                                  const int* record, double* row) {
  __shared__ double by_slot[kRobustMaxRanks];
  const long long sum = fold_partial_rows(partial, n_partial, theta);
  const int t = threadIdx.x;
  if (t < kRobustMaxRanks) by_slot[t] = (double)sum;   // (0 at and past theta; a count is far below 2^53)
  __syncthreads();
  if (t < kRobustMaxRanks) {
    double v = 0.0;
    for (int s = 0; s < theta; ++s) v = record[1 + s] == t ? by_slot[s] : v;
    row[t] = v;
  }
}

// launches 3 and 4 over the record that `partial` holds
void launch_fold(hipStream_t st, const float* rows, long ld, int W, long n, int theta, int c, float* out,
                 double* partial, double* stats) {
  const int* record = gram_record(partial, n);
  long long* cuts = reinterpret_cast<long long*>(partial + (long)(krum_grid(n) + 1) * KR_TILE);
  const int grid = flat_grid(n);
  robust_dispatch(theta, [&](auto th) {
    hipLaunchKernelGGL(bulyan_fold_kernel<decltype(th)::value>, dim3(grid), dim3(BY_THREADS), 0, st, rows, ld, W, n,
                       record, c, out, cuts);
  });
  hipLaunchKernelGGL(bulyan_cut_kernel, dim3(1), dim3(kFoldThreads), 0, st, cuts, grid, theta, record,
                     stats + BY_CUT_ROW * kRobustMaxRanks);
}

}  // namespace

namespace fedmi {

// rows of 256 doubles in `partial`: one per workgroup of the Gram pass, one for the record, and the fold's
// flat_grid(n) rows of 16 int64 cut counts (16 of them per row of 256 doubles)
int bulyan_partials(long n) {
  return n > 0 ? krum_grid(n) + 1 + (flat_grid(n) * kRobustMaxRanks + KR_TILE - 1) / KR_TILE : 0;
}

// the rule's counts at W clients (fedmi/parallel/bulyan.py): F_eff, then theta and c
void bulyan_counts(int W, int byz, int* f, int* theta, int* c) {
  int e = (W - 3) / 4;
  e = byz < e ? byz : e;
  e = e < 0 ? 0 : e;
  *f = e;
  *theta = W - 2 * e;
  *c = 2 * e;
}

// The fold alone over a caller's record (theta ranks, ascending, each below W; c even, 0 <= c <= 6, c < theta): out and
// stats row 18.  Buffers as launch_bulyan.
void launch_bulyan_fold(hipStream_t st, const float* rows, long ld, int W, long n, const int* ranks, int theta, int c,
                        float* out, double* partial, double* stats) {
  if (n <= 0) return;
  BulyanRanks by_value{theta, {}};
  for (int s = 0; s < theta; ++s) by_value.rank[s] = ranks[s];
  hipLaunchKernelGGL(bulyan_record_kernel, dim3(1), dim3(64), 0, st, by_value, gram_record(partial, n));
  launch_fold(st, rows, ld, W, n, theta, c, out, partial, stats);
}

// rows: W rows of ld floats, 16-byte aligned, ld % 4 == 0, ld >= n; out: n floats, 16-byte aligned, not aliasing rows;
// partial: bulyan_partials(n) x 256 doubles; stats: 19 x 16 doubles; 2 <= W <= 16, byz >= 0 (the binding checks all of it)
void launch_bulyan(hipStream_t st, const float* rows, long ld, int W, long n, int byz, float* out, double* partial,
                   double* stats) {
  if (n <= 0) return;
  int f, theta, c;
  bulyan_counts(W, byz, &f, &theta, &c);
  launch_gram_pass(st, rows, ld, W, n, partial);
  hipLaunchKernelGGL(bulyan_finish_kernel, dim3(1), dim3(kFoldThreads), 0, st, partial, krum_grid(n), krum_tile(W), W,
                     f, theta, stats, gram_record(partial, n));
  launch_fold(st, rows, ld, W, n, theta, c, out, partial, stats);
}

}  // namespace fedmi
