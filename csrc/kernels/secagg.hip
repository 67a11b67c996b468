// fedmi — secure aggregation by pairwise masking (fedmi/parallel/secagg.py; Bonawitz et al. 2017 without dropout
// recovery): a client's update leaves it as fixed-point words under ChaCha20 masks that cancel in the sum.
//
//   secagg_mask<W>   :  q[i] = fixed-point (x[i] - a[i]) at f fraction bits, clamped to +-(2^27 - 1), NaN -> 0;
//                       u[i] = q[i] + sum_{j > rank} m_j[i] - sum_{j < rank} m_j[i]  (mod 2^32);
//                       partial[wg][0] = the workgroup's number of clamped or NaN entries (int64)
//   secagg_finish    :  stats[0] = sum of the partials (fold_partial_rows, one column)
//   secagg_unmask<W> :  S[i] = sum_r rows[r][i] (uint32 bit patterns, mod 2^32), read as int32;
//                       x[i] = a[i] + (float)((double)S * 2^-f / W)      (fp64 product and division, one rounding each)
//
// m_j[i] is a ChaCha20 keystream word (RFC 8439 block function, 20 rounds) under the pair's 256-bit key (row j of
// the [W, 8] table; row `rank` is not read), block counter i >> 4, nonce (draw lo, draw hi, 0).
//
// The mask kernel.  The four lanes of a quad share one block: lane c holds column c of the 4x4 state, words c, 4 + c,
// 8 + c, 12 + c, as (a, b, c, d).  A column round is four lane-local quarter rounds; the diagonal round rotates b, c, d
// by 1, 2, 3 lanes inside the quad (quad_perm DPP: no LDS, no ds_bpermute), runs the same quarter round and rotates
// back.  After the 10 double rounds and the feed-forward add, lane c holds words c, 4 + c, 8 + c, 12 + c of the
// output, and they mask the four coordinates of the lane's own 16-B vector: coordinate 16 B + 4 c + k takes output
// word 4 k + c.  So every lane issues one 16-B load of x, one of a and one 16-B store of u, all coalesced, and no word
// ever changes lanes after the last round.  The W - 1 streams of a vector are independent chains: they are held side
// by side (4 state registers each) and every step of a quarter round is issued for all of them before the next, so
// W - 1 dependent chains are in flight.  The round loop is not unrolled (one double round of W - 1 streams is 30 (W - 1)
// instructions: W = 16 stays far inside the instruction cache).  The sign of a stream (j > rank) is wave-uniform: a
// scalar all-ones / zero word, applied as (m ^ s) - s, no branch.  Rotates are v_alignbit_b32.
//
// The grid strides over whole 16-coordinate blocks, four lanes each, with sgd_flat's block cap; the stride is a
// multiple of 256 lanes, so a quad always sits on one block and the loop condition is the same in its four lanes (the
// DPP moves read active lanes only).  The n % 16 entries after the whole blocks run through the same code: entries at
// and past n are loaded as 0 (x == a: q = 0, not clamped) and not stored.
//
// The unmask kernel is the row sweep of row_sweep.h over W + 1 rows: the W gathered payload rows and, as row W, the
// anchor (AnchoredRows).  row_sweep.h is untouched, so robust_reduce and geomed_pass compile to the code they had.
// The payload words travel through fp32 registers as bit patterns; the sweep does no arithmetic on them.
//
// Determinism: integers mod 2^32 and named roundings only; the clamp count is an integer (wave shuffles, LDS integer
// atomics, fold_partial_rows).  No float atomics.  Built without packed fp32 instructions (fedmi/_build.py).
#include "flat_map.h"
#include "robust_fold.h"
#include "row_sweep.h"

namespace {

using namespace fedmi;

constexpr int SA_THREADS = 256;
constexpr int SA_QMAX = (1 << 27) - 1;
constexpr int DPP_ROT1 = 0x39;   // quad_perm:[1,2,3,0]: lane c takes lane c + 1
constexpr int DPP_ROT2 = 0x4E;   // quad_perm:[2,3,0,1]
constexpr int DPP_ROT3 = 0x93;   // quad_perm:[3,0,1,2]

template <int CTRL>
FEDMI_DEV uint32_t quad_rot(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}

template <int N>
FEDMI_DEV uint32_t rotl(uint32_t v) { return __builtin_amdgcn_alignbit(v, v, 32 - N); }

// one quarter round on S independent states, step by step across all of them
template <int S>
FEDMI_DEV void quarter(uint32_t (&a)[S], uint32_t (&b)[S], uint32_t (&c)[S], uint32_t (&d)[S]) {
#pragma unroll
  for (int s = 0; s < S; ++s) a[s] += b[s];
#pragma unroll
  for (int s = 0; s < S; ++s) d[s] = rotl<16>(d[s] ^ a[s]);
#pragma unroll
  for (int s = 0; s < S; ++s) c[s] += d[s];
#pragma unroll
  for (int s = 0; s < S; ++s) b[s] = rotl<12>(b[s] ^ c[s]);
#pragma unroll
  for (int s = 0; s < S; ++s) a[s] += b[s];
#pragma unroll
  for (int s = 0; s < S; ++s) d[s] = rotl<8>(d[s] ^ a[s]);
#pragma unroll
  for (int s = 0; s < S; ++s) c[s] += d[s];
#pragma unroll
  for (int s = 0; s < S; ++s) b[s] = rotl<7>(b[s] ^ c[s]);
}

template <int S, int RB, int RC, int RD>
FEDMI_DEV void quad_shift(uint32_t (&b)[S], uint32_t (&c)[S], uint32_t (&d)[S]) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    b[s] = quad_rot<RB>(b[s]);
    c[s] = quad_rot<RC>(c[s]);
    d[s] = quad_rot<RD>(d[s]);
  }
}

// q of one entry; `up` = 2^f.  |s| < 2^27 is |s| <= 2^27 - 1 for an fp32 s (no fp32 number lies between), and false
// for a NaN.
FEDMI_DEV uint32_t secagg_encode(float x, float a, float up, uint32_t& clamped) {
  const float s = __fmul_rn(__fsub_rn(x, a), up);
  const bool inside = fabsf(s) < 134217728.f;
  const int edge = s != s ? 0 : (s < 0.f ? -SA_QMAX : SA_QMAX);
  clamped += inside ? 0u : 1u;
  return (uint32_t)(inside ? (int)rintf(s) : edge);
}

template <int W>
__global__ __launch_bounds__(SA_THREADS) void secagg_mask_kernel(const float* x, const float* a, const uint32_t* keys,
                                                                 int rank, uint32_t draw_lo, uint32_t draw_hi, long n,
                                                                 float up, uint32_t* u, long long* partial) {
  constexpr int S = W - 1;
  __shared__ unsigned long long total;
  if (threadIdx.x == 0) total = 0ull;
  const int c = threadIdx.x & 3;
  const uint32_t k0 = c == 0 ? 0x61707865u : c == 1 ? 0x3320646eu : c == 2 ? 0x79622d32u : 0x6b206574u;
  const uint32_t d_rest = c == 1 ? draw_lo : c == 2 ? draw_hi : 0u;      // words 13, 14, 15; word 12 is the counter
  uint32_t kb[S], kc[S], neg[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int j = s + (s >= rank ? 1 : 0);            // the peers in rank order, the client's own row left out
    kb[s] = keys[j * 8 + c];
    kc[s] = keys[j * 8 + 4 + c];
    neg[s] = s >= rank ? 0u : 0xFFFFFFFFu;            // j < rank: the mask is subtracted
  }
  const long nv = ((n + 15) >> 4) << 2;               // 16-B vectors of the whole blocks, the last one padded
  const long stride = (long)gridDim.x * SA_THREADS;
  uint32_t clamped = 0u;
#pragma unroll 1
  for (long v = (long)blockIdx.x * SA_THREADS + threadIdx.x; v < nv; v += stride) {
    const long e = v << 2;
    const bool whole = e + 4 <= n;
    FlatVec<4> xv, av;
    if (whole) {
      xv = flat_load<4>(x, e);
      av = flat_load<4>(a, e);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xv[k] = e + k < n ? x[e + k] : 0.f;
        av[k] = e + k < n ? a[e + k] : 0.f;
      }
    }
    const uint32_t d0 = c == 0 ? (uint32_t)(v >> 2) : d_rest;
    uint32_t sa[S], sb[S], sc[S], sd[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      sa[s] = k0;
      sb[s] = kb[s];
      sc[s] = kc[s];
      sd[s] = d0;
    }
#pragma unroll 1
    for (int round = 0; round < 10; ++round) {
      quarter<S>(sa, sb, sc, sd);
      quad_shift<S, DPP_ROT1, DPP_ROT2, DPP_ROT3>(sb, sc, sd);
      quarter<S>(sa, sb, sc, sd);
      quad_shift<S, DPP_ROT3, DPP_ROT2, DPP_ROT1>(sb, sc, sd);
    }
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = secagg_encode(xv[k], av[k], up, clamped);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      o[0] += ((sa[s] + k0) ^ neg[s]) - neg[s];
      o[1] += ((sb[s] + kb[s]) ^ neg[s]) - neg[s];
      o[2] += ((sc[s] + kc[s]) ^ neg[s]) - neg[s];
      o[3] += ((sd[s] + d0) ^ neg[s]) - neg[s];
    }
    if (whole) {
      *reinterpret_cast<uint4*>(u + e) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < n) u[e + k] = o[k];
    }
  }
  // the workgroup's count: a wave by shuffles, the waves by an integer LDS atomic (any order, the same bits)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) clamped += __shfl_xor(clamped, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && clamped) atomicAdd(&total, (unsigned long long)clamped);
  __syncthreads();
  if (threadIdx.x == 0) partial[(long)blockIdx.x * kRobustMaxRanks] = (long long)total;
}

__global__ __launch_bounds__(kFoldThreads) void secagg_finish_kernel(const long long* partial, int n_partial,
                                                                     long long* stats) {
  const long long sum = fold_partial_rows(partial, n_partial, 1);
  if (threadIdx.x == 0) stats[0] = sum;
}

// rows 0 .. W-1: the gathered payloads, ld floats apart; row W: the anchor
template <int W>
struct AnchoredRows {
  const float* base;
  long ld;
  const float* anchor;
  FEDMI_DEV const float* operator()(int r) const { return r < W ? base + r * ld : anchor; }
};

// the decode of one coordinate for row_sweep.h: x[0 .. W-1] are payload words, x[W] is the anchor's entry
template <int W>
struct UnmaskRule {
  double down;                                        // 2^-f
  FEDMI_DEV float coord(const float (&x)[W + 1]) const {
    uint32_t sum = 0u;
#pragma unroll
    for (int r = 0; r < W; ++r) sum += __float_as_uint(x[r]);
    const double m = __ddiv_rn(__dmul_rn((double)(int)sum, down), (double)W);
    return __fadd_rn(x[W], __double2float_rn(m));
  }
  FEDMI_DEV void stored(const float (&)[W + 1], float) {}
};

template <int W>
__global__ __launch_bounds__(SA_THREADS) void secagg_unmask_kernel(const float* rows, long ld, const float* a, long n,
                                                                   double down, float* out) {
  UnmaskRule<W> rule{down};
  row_sweep<W + 1>(AnchoredRows<W>{rows, ld, a}, n, out, rule);
}

}  // namespace

namespace fedmi {

// workgroups of secagg_mask == rows of int64[16] partials it writes (column 0): a function of n only, at most 2048
int secagg_partials(long n) {
  if (n <= 0) return 0;
  const long blocks = (((n + 15) >> 4) * 4 + SA_THREADS - 1) / SA_THREADS;
  return (int)(blocks > 2048 ? 2048 : blocks);
}

// x, a, u: n entries, 16-byte aligned, u aliasing neither; keys: W x 8 uint32; 2 <= W <= 16, 0 <= rank < W,
// 19 <= f <= 35; partial: secagg_partials(n) x 16 int64; stats: 1 int64 (the binding checks all of it)
void launch_secagg_mask(hipStream_t st, const float* x, const float* a, const uint32_t* keys, int W, int rank,
                        uint64_t draw, long n, int f, uint32_t* u, long long* partial, long long* stats) {
  if (n <= 0) return;
  const int grid = secagg_partials(n);
  const float up = ldexpf(1.f, f);
  robust_dispatch(W, [&](auto w) {
    hipLaunchKernelGGL(secagg_mask_kernel<decltype(w)::value>, dim3(grid), dim3(SA_THREADS), 0, st, x, a, keys, rank,
                       (uint32_t)draw, (uint32_t)(draw >> 32), n, up, u, partial);
  });
  hipLaunchKernelGGL(secagg_finish_kernel, dim3(1), dim3(kFoldThreads), 0, st, partial, grid, stats);
}

// rows: W rows of ld floats holding uint32 payload words, 16-byte aligned, ld % 4 == 0, ld >= n; a, out: n floats,
// 16-byte aligned, out aliasing neither rows nor a
void launch_secagg_unmask(hipStream_t st, const float* rows, long ld, int W, const float* a, long n, int f,
                          float* out) {
  if (n <= 0) return;
  robust_dispatch(W, [&](auto w) {
    hipLaunchKernelGGL(secagg_unmask_kernel<decltype(w)::value>, dim3(flat_grid(n)), dim3(SA_THREADS), 0, st, rows, ld,
                       a, n, ldexp(1.0, -f), out);
  });
}

}  // namespace fedmi
