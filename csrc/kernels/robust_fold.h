// fedmi — the coordinate-wise robust fold (median / trimmed mean over the clients' values of one coordinate), shared by
// robust_reduce (robust.hip) and peer_robust_f32_kernel (comm/peer_comm.hip).  Rule: fedmi/parallel/robust.py.
//
// One call takes the W values x_0 .. x_{W-1} of one coordinate (rank order, in registers) and the trim count b:
//   key_r   = 0xFFFFFFFF if x_r is NaN;  bits ^ 0xFFFFFFFF if the sign bit is set;  bits ^ 0x80000000 otherwise
//             (-inf < ... < -0 < +0 < ... < +inf < NaN as unsigned integers)
//   order   = ascending (key, rank): the pair is one 64-bit integer (key << 32 | rank), so the order is total
//   window  = positions [b, W - b), m = W - 2b entries
//   result  = (((v[b] + v[b+1]) + ...) + v[W-b-1]) / (float)m      (__fadd_rn in position order, one __fdiv_rn)
//   cut     = the set of ranks outside the window, as a bit mask; RobustCuts counts it per rank
// The value of a position is rebuilt from its key (the transform is its own inverse up to the NaN payload; a NaN in
// the window makes the result NaN whatever its payload).
//
// W is a template parameter (2 .. 16): every width gets its own sorting network, Knuth's merge exchange (TAOCP 5.2.2
// Algorithm M), which sorts any W (not only powers of two) -- a 2-client run pays one compare-exchange, a 9-client
// run 26 and not the 63 of a network padded to 16, and there are no padding lanes to fill or to keep out of the
// window.  The network is built at compile time and applied through an index sequence, so every register index is a
// constant: no local array is indexed at run time and the kernels use no scratch (checked with
// -Rpass-analysis=kernel-resource-usage: ScratchSize 0 for all 15 widths of both kernels).
//
// Cost per coordinate, in VALU instructions per lane.  Planned:
//   key transform        4 W      (and, compare, xor-select, or the NaN key)
//   compare-exchange     5 CE(W)  (one 64-bit compare, four selects);  CE = 1, 3, 5, 9, 12, 16, 19, 26, 31, 37, 41,
//                                  48, 53, 59, 63 for W = 2 .. 16
//   window fold + mask   4 W      (inverse key, add or select, shift / or of the rank bit; the window test is scalar)
//   cut counters         2 W      (bit extract, add)
//   the divide           ~12
// Counted in the gfx950 code of robust_reduce (all VALU instructions of the kernel over its five inlined folds, so
// loop and address arithmetic are included): 66 (W = 2), 127 (4), 286 (8), 347 (9), 699 (16).  The compiler turns the
// two selects of a compare-exchange into a 64-bit min and a 64-bit max with a compare each, 6 instructions per
// exchange and not 5 (W = 16: 630 compares for 315 exchanges).
// A CU issues 4 SIMDs x 32 lanes = 128 lane-instructions per cycle and streams about 10 B per cycle from HBM, so
// the (W + 1) * 4 bytes of a coordinate take 0.4 (W + 1) cycles = 51 (W + 1) lane-instructions of issue time:
//   153 (W = 2), 256 (4), 460 (8), 512 (9), 870 (16)
// Every width stays below it: 0.43, 0.50, 0.62, 0.68, 0.80 of the budget.  Measured: profiles/r14_robust/README.md.
#pragma once
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "common.h"

namespace fedmi {

constexpr int kRobustMaxRanks = 16;   // == kPeerMaxRanks; the stats row and every row of partials hold 16 int64

// The compare-exchange pairs of merge exchange for n inputs, in order.
struct RobustNet {
  int count;
  unsigned char lo[64], hi[64];
};

constexpr RobustNet robust_net(int n) {
  RobustNet net{};
  int t = 0;
  while ((1 << t) < n) ++t;
  for (int p = 1 << (t - 1); p >= 1; p >>= 1) {
    int q = 1 << (t - 1), r = 0, d = p;
    while (true) {
      for (int i = 0; i + d < n; ++i)
        if ((i & p) == r) {
          net.lo[net.count] = (unsigned char)i;
          net.hi[net.count] = (unsigned char)(i + d);
          ++net.count;
        }
      if (q == p) break;
      d = q - p;
      q >>= 1;
      r = p;
    }
  }
  return net;
}

FEDMI_DEV uint32_t robust_key(float v) {
  const uint32_t u = __float_as_uint(v);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
  return (u & 0x80000000u) ? ~u : u ^ 0x80000000u;
}

FEDMI_DEV float robust_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }

FEDMI_DEV void robust_cmpx(uint64_t& a, uint64_t& b) {
  const bool swap = b < a;
  const uint64_t lo = swap ? b : a, hi = swap ? a : b;
  a = lo;
  b = hi;
}

template <int W, size_t... C>
FEDMI_DEV void robust_sort(uint64_t (&k)[W], std::index_sequence<C...>) {
  constexpr RobustNet net = robust_net(W);
  (robust_cmpx(k[net.lo[C]], k[net.hi[C]]), ...);
}

// x: the coordinate's value on ranks 0 .. W-1; 0 <= b <= (W - 1) / 2 (the same in every lane).  Returns the robust
// aggregate and sets bit r of `cut` for every rank r whose entry fell outside the window.
template <int W>
FEDMI_DEV float robust_fold(const float (&x)[W], int b, uint32_t& cut) {
  static_assert(W >= 2 && W <= kRobustMaxRanks, "2 .. 16 clients");
  uint64_t k[W];
#pragma unroll
  for (int r = 0; r < W; ++r) k[r] = ((uint64_t)robust_key(x[r]) << 32) | (uint32_t)r;
  robust_sort<W>(k, std::make_index_sequence<robust_net(W).count>{});
  float s = 0.f;
  cut = 0u;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const float v = robust_unkey((uint32_t)(k[j] >> 32));
    if (j < b || j >= W - b)
      cut |= 1u << ((uint32_t)k[j] & 31u);
    else
      s = j == b ? v : __fadd_rn(s, v);        // the first kept entry starts the sum: no 0 + v (it would lose -0)
  }
  return __fdiv_rn(s, (float)(W - 2 * b));
}

// per-thread cut counters, one per rank
template <int W>
struct RobustCuts {
  uint32_t n[W];
  FEDMI_DEV RobustCuts() {
#pragma unroll
    for (int r = 0; r < W; ++r) n[r] = 0u;
  }
  FEDMI_DEV void add(uint32_t cut) {
#pragma unroll
    for (int r = 0; r < W; ++r) n[r] += (cut >> r) & 1u;
  }
  // Integer sum over the workgroup (a wave's lanes by shuffles, the waves by integer LDS atomics: any order gives
  // the same bits), then one row of kRobustMaxRanks int64 for the workgroup; entries at and past W are written as 0.
  FEDMI_DEV void store(long long* row) const {
    __shared__ unsigned long long sh[kRobustMaxRanks];
    if (threadIdx.x < kRobustMaxRanks) sh[threadIdx.x] = 0ull;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < W; ++r) {
      uint32_t v = n[r];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sh[r], (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x < kRobustMaxRanks) row[threadIdx.x] = (long long)sh[threadIdx.x];
  }
};

// Calls f(std::integral_constant<int, W>{}) for the run-time W in 2 .. 16; false for any other W.
template <class F, int W = 2>
bool robust_dispatch(int world, F&& f) {
  if constexpr (W > kRobustMaxRanks) {
    return false;
  } else {
    if (world == W) {
      f(std::integral_constant<int, W>{});
      return true;
    }
    return robust_dispatch<F, W + 1>(world, static_cast<F&&>(f));
  }
}

}  // namespace fedmi
