// fedmi — Divide-and-Conquer aggregation of the clients' gathered float states (fedmi/parallel/dnc.py; Shejwalkar and
// Houmansadr 2021) over a [W, ld] fp32 buffer, row r = client r's state: every client is scored by its squared
// projection on the top principal direction of the centred updates, the m = W - F_eff lowest scores are averaged.  With
// W <= 16 that direction is fully determined by the W x W centred Gram matrix.  Three launches on one stream, no host
// sync:
//
//   dnc_gram<P>  :  partial[wg] = the workgroup's share of G = Y Y^T (fp64), y_r[k] = (double)x_r[k] - (double)p[k], p[k]
//                   the fp32 column pivot; P = 4 / 8 / 16 = the smallest >= W
//   dnc_finish   :  G = the sum of the partials;  A = the clients with a finite G[i][i];  C = G double-centred over A;
//                   B = C / tr C, 12 times B <- B B / tr(B B);  u = the column of B with the largest diagonal entry;
//                   score[i] = ((C u)_i)^2 / (u^T C u), +inf outside A;  selected = the m clients of lowest (score, rank);
//                   stats = [18][16] fp64: row 0 score, row 1 selected (1.0 / 0.0), rows 2 .. 17 C;  record = {m, the
//                   selected ranks ascending} (int32)
//   krum_select  :  krum.hip's mean of the record's rows, unchanged
//
// The Gram pass has the shape of krum_gram<P> (krum.hip: lane (r, q) = (lane % 16, lane / 16) loads the float4 of
// client r % P at column group r / P, both operands of v_mfma_f64_16x16x4_f64 are the same register, two alternating
// accumulator tiles, the diagonal P x P blocks of a folded tile are partial Grams of disjoint columns) and the same grid
// and partials (krum_gram.h).  New is what stands between the load and the MFMA.  The P lanes that hold the P clients'
// values of ONE column are the aligned group of P adjacent lanes r = g P .. g P + P - 1 of the DPP row q, so the column
// sum is a butterfly in registers (xlane.h: xor 1, xor 2 for P = 4; + row_half_mirror for 8; + row_ror:8 for 16): two to
// four v_add_f32_dpp per entry, no LDS, no ds_bpermute, and a butterfly over an aligned group of P never leaves it, so
// the 16 / P column groups of a folded tile cannot mix.  An entry enters the sum only if its client is < W, its column
// is < n and it is finite; everything else enters as 0.f.  p = sum * (1 / W) in fp32 (0.f if the sum overflowed), the
// same bits in all P lanes: after every butterfly step both partners hold the sum of the same two values.  Then
// y = (double)x - (double)p in fp64 (one rounding at most), and only AFTER that the select to 0.0 for an entry at or past
// n or of a client >= W: such an entry is never fed as 0 - p, and the buffer's padding is never trusted.  A non-finite x
// stays non-finite in y and reaches only its own row and column of G.  The pivot only has to be NEAR the mean: the
// finish's double-centring removes whatever common part is left, exactly, so the pivot's rounding is no part of the
// result's meaning -- it only keeps the entries of G at the size of the clients' differences, where the fp64 sums lose
// nothing that matters.
//
// The finish.  G, C, B and the product live in LDS (2 KiB each); thread t < 256 owns entry (t / 16, t % 16).  C is
// formed for i <= j and mirrored, so C and every B are symmetric bit for bit (entry (i, j) and (j, i) of a product add
// the same products in the same order).  A squaring is one 16 x 16 x 16 product, one entry per thread, then the trace
// and the divide: two barriers.  (lambda_2 / lambda_1)^4096 is what is left of the second eigenvector.  Every fp64
// operation is spelled with its rounding (a product that feeds a sum goes through mul_add, so that no FMA is formed)
// and every sum runs from 0.0 in ascending index order, over all 16 indices where the entries outside A are 0.0 (adding
// +-0.0 to a sum that started at +0.0 changes no bit): fedmi/parallel/dnc.py's dnc_finish_torch reproduces the bits.
//
// Determinism: as krum.hip.  The grid is a function of n alone and the order of every sum a function of W and n; no
// atomics.
#include <math.h>

#include "krum_gram.h"
#include "robust_fold.h"
#include "xlane.h"

namespace {

using namespace fedmi;

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int DN_THREADS = 256;
constexpr int DN_WAVES = DN_THREADS / 64;
constexpr int DN_STEPS = 4;                         // steps per chunk: four 16-B loads in flight per lane
constexpr int DN_SQUARINGS = 12;
constexpr int R = kRobustMaxRanks;

FEDMI_DEV bool finite32(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// s + a * b in two roundings.  (__dmul_rn and __dadd_rn are a plain * and + in the HIP headers, which the compiler fuses
// into one v_fma_f64 wherever they meet: the product is kept apart here.)
FEDMI_DEV double mul_add(double s, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return s + p;
}

// the sum of v over the aligned group of P lanes of a DPP row, the same bits in each of them
template <int P>
FEDMI_DEV float column_sum(float v) {
  if constexpr (P == 4) return xlane::sum4(v);
  if constexpr (P == 8) return xlane::sum8(v);
  if constexpr (P == 16) return xlane::sum16(v);
}

template <int P>
__global__ __launch_bounds__(DN_THREADS) void dnc_gram_kernel(const float* rows, long ld, int W, long n,
                                                              double* partial) {
  static_assert(P == 4 || P == 8 || P == 16, "the tile holds 16 / P diagonal blocks");
  constexpr int GROUPS = 16 / P;
  constexpr long STEP = 16 * GROUPS, CHUNK = DN_STEPS * STEP;   // columns per step and per chunk of a wave
  __shared__ double sh[DN_WAVES][KR_TILE];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: the column loop is a scalar branch
  const int r = lane & 15, q = lane >> 4;
  const int client = r % P, group = r / P;
  const bool live = client < W;
  const float* row = rows + (long)(live ? client : 0) * ld + 16 * group + 4 * q;
  const long first = 16 * group + 4 * q;
  const float inv_w = __fdiv_rn(1.f, (float)W);

  double4_t acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
  // base is the same in all 64 lanes: every lane runs every step, as the DPP reads need
  for (long base = ((long)blockIdx.x * DN_WAVES + wave) * CHUNK; base < n; base += (long)gridDim.x * DN_WAVES * CHUNK) {
    float4 x[DN_STEPS];
#pragma unroll
    for (int u = 0; u < DN_STEPS; ++u) {            // c < n and ld % 4 == 0, ld >= n: the vector lies inside the row
      const long c = base + u * STEP;
      x[u] = (live && c + first < n) ? *reinterpret_cast<const float4*>(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < DN_STEPS; ++u) {
      const long left = n - (base + u * STEP + first);   // entries of this vector before n: the same in the P lanes
      const float v[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool mine = live && k < left;
        const float s = column_sum<P>((mine && finite32(v[k])) ? v[k] : 0.f);
        const float p = finite32(s) ? __fmul_rn(s, inv_w) : 0.f;
        const double y = __dsub_rn((double)v[k], (double)p);
        const double a = mine ? y : 0.0;            // after centring: never 0 - p
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
__global__ __launch_bounds__(kFoldThreads) void dnc_finish_kernel(const double* partial, int n_partial, int P, int W,
                                                                  int m, double* gram, double* stats, int* record) {
  __shared__ double G[R][R], C[R][R], B[R][R], T[R][R];
  __shared__ double rbar[R], cu[R], score[R];
  const double sum = fold_partial_tiles(partial, n_partial, P * P);
  const int t = threadIdx.x;
  if (t < P * P) G[t / P][t % P] = sum;
  __syncthreads();
  const int i = t / R, j = t % R;
  const bool cell = t < KR_TILE;
  const bool pair = cell && i < W && j < W;
  if (gram) {
    if (cell) gram[t] = pair ? G[i < j ? i : j][i < j ? j : i] : 0.0;
    return;
  }
  unsigned alive = 0u;                              // A: the same in every thread
  for (int o = 0; o < W; ++o) alive |= isfinite(G[o][o]) ? 1u << o : 0u;
  const int count = __popc(alive);
  const double na = (double)count;
  const bool in = pair && ((alive >> i) & (alive >> j) & 1u);
  if (t < R) {                                      // the mean of row t over A
    double s = 0.0;
    if ((alive >> t) & 1u) {
      for (int o = 0; o < W; ++o)
        if ((alive >> o) & 1u) s = __dadd_rn(s, G[t < o ? t : o][t < o ? o : t]);
      s = __ddiv_rn(s, na);
    }
    rbar[t] = s;
  }
  __syncthreads();
  double gbar = 0.0;
  for (int o = 0; o < W; ++o)
    if ((alive >> o) & 1u) gbar = __dadd_rn(gbar, rbar[o]);
  if (count > 0) gbar = __ddiv_rn(gbar, na);
  if (cell) {
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const double c = in ? __dadd_rn(__dsub_rn(__dsub_rn(G[lo][hi], rbar[lo]), rbar[hi]), gbar) : 0.0;
    C[i][j] = c;
    stats[2 * R + t] = c;
  }
  __syncthreads();
  double tr = 0.0;
  for (int o = 0; o < R; ++o) tr = __dadd_rn(tr, C[o][o]);
  const bool spectral = count >= 2 && tr > 0.0 && tr < INFINITY;   // else every score in A is 0
  if (spectral) {                                   // (the same in every thread: the barriers inside are safe)
    if (cell) B[i][j] = __ddiv_rn(C[i][j], tr);
    __syncthreads();
    for (int round = 0; round < DN_SQUARINGS; ++round) {
      if (cell) {
        double s = 0.0;
#pragma unroll
        for (int o = 0; o < R; ++o) s = mul_add(s, B[i][o], B[o][j]);
        T[i][j] = s;
      }
      __syncthreads();
      if (cell) {
        double tt = 0.0;
#pragma unroll
        for (int o = 0; o < R; ++o) tt = __dadd_rn(tt, T[o][o]);
        B[i][j] = __ddiv_rn(T[i][j], tt);
      }
      __syncthreads();
    }
    int top = 0;                                    // the largest diagonal entry, ties to the lower rank
    for (int o = 1; o < W; ++o) top = B[o][o] > B[top][top] ? o : top;
    if (t < R) {
      double s = 0.0;
      for (int o = 0; o < R; ++o) s = mul_add(s, C[t][o], B[o][top]);
      cu[t] = s;
    }
    __syncthreads();
    if (t < R) {
      double den = 0.0;
      for (int o = 0; o < R; ++o) den = mul_add(den, B[o][top], cu[o]);
      const double s = den > 0.0 ? __ddiv_rn(__dmul_rn(cu[t], cu[t]), den) : 0.0;
      score[t] = s == s ? s : INFINITY;             // (a NaN from an overflow in C u counts as +inf)
    }
  } else if (t < R) {
    score[t] = 0.0;
  }
  if (t < R && t < W && !((alive >> t) & 1u)) score[t] = INFINITY;
  __syncthreads();
  select_lowest(score, W, m, stats, record);
}

void launch_dnc_pass(hipStream_t st, const float* rows, long ld, int W, long n, double* partial) {
  const int grid = krum_grid(n);
  switch (krum_tile(W)) {
    case 4: hipLaunchKernelGGL(dnc_gram_kernel<4>, dim3(grid), dim3(DN_THREADS), 0, st, rows, ld, W, n, partial); break;
    case 8: hipLaunchKernelGGL(dnc_gram_kernel<8>, dim3(grid), dim3(DN_THREADS), 0, st, rows, ld, W, n, partial); break;
    default: hipLaunchKernelGGL(dnc_gram_kernel<16>, dim3(grid), dim3(DN_THREADS), 0, st, rows, ld, W, n, partial);
  }
}

}  // namespace

namespace fedmi {

// rows of 256 doubles in `partial`: one per workgroup of the Gram pass and one for the record, as krum_partials
int dnc_partials(long n) { return n > 0 ? krum_grid(n) + 1 : 0; }

// the rule's count at W clients (fedmi/parallel/dnc.py): m = W - F_eff
int dnc_kept(int W, int byz) {
  int f = (W - 1) / 2;
  f = byz < f ? byz : f;
  return W - (f < 0 ? 0 : f);
}

// the centred G as [16][16] doubles (0 outside W x W) into gram; buffers as launch_dnc
void launch_dnc_gram(hipStream_t st, const float* rows, long ld, int W, long n, double* partial, double* gram) {
  if (n <= 0) return;
  launch_dnc_pass(st, rows, ld, W, n, partial);
  hipLaunchKernelGGL(dnc_finish_kernel, dim3(1), dim3(kFoldThreads), 0, st, partial, krum_grid(n), krum_tile(W), W, 0,
                     gram, nullptr, nullptr);
}

// rows: W rows of ld floats, 16-byte aligned, ld % 4 == 0, ld >= n; out: n floats, 16-byte aligned, not aliasing rows;
// partial: dnc_partials(n) x 256 doubles; stats: 18 x 16 doubles; 2 <= W <= 16, byz >= 0 (the binding checks all of it)
void launch_dnc(hipStream_t st, const float* rows, long ld, int W, long n, int byz, float* out, double* partial,
                double* stats) {
  if (n <= 0) return;
  int* record = gram_record(partial, n);
  launch_dnc_pass(st, rows, ld, W, n, partial);
  hipLaunchKernelGGL(dnc_finish_kernel, dim3(1), dim3(kFoldThreads), 0, st, partial, krum_grid(n), krum_tile(W), W,
                     dnc_kept(W, byz), nullptr, stats, record);
  launch_krum_select(st, rows, ld, n, record, out);
}

}  // namespace fedmi
