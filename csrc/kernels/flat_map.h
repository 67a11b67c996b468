// fedmi — the one skeleton of the flat fp32 elementwise kernels (flat_ops.hip, client_opt.hip; server_opt.hip
// keeps its own loop and shares the grid rule).
//
// An operation is a small struct that holds its pointers and scalars and has one member,
//   template <int W> void run(long e) const
// which loads W consecutive entries of each operand at e, applies its per-entry function in a `for (j < W)` loop
// and stores the results.  The kernel calls run<4> (one 16-B access per operand and lane, grid-strided) on the
// n / 4 whole vectors and run<1> on the n % 4 entries after them, so every formula is written once and the tail
// cannot drift from the body.  Every buffer holds n floats and is 16-byte aligned.
#pragma once
#include <type_traits>

#include "common.h"

namespace fedmi {

// W floats in registers: W = 4 is one 16-B access, W = 1 one float
template <int W>
struct FlatVec {
  static_assert(W == 1 || W == 4, "one float or one 16-B vector");
  typename std::conditional<W == 4, float4, float>::type v;
  FEDMI_DEV float& operator[](int j) { return reinterpret_cast<float*>(&v)[j]; }
  FEDMI_DEV const float& operator[](int j) const { return reinterpret_cast<const float*>(&v)[j]; }
};

template <int W>
FEDMI_DEV FlatVec<W> flat_load(const float* p, long e) { return *reinterpret_cast<const FlatVec<W>*>(p + e); }

template <int W>
FEDMI_DEV void flat_store(float* p, long e, const FlatVec<W>& x) { *reinterpret_cast<FlatVec<W>*>(p + e) = x; }

template <class Op>
__global__ __launch_bounds__(256) void flat_map_kernel(const Op op, long n) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long i = t; i < n4; i += stride) op.template run<4>(i << 2);
  for (long i = (n4 << 2) + t; i < n; i += stride) op.template run<1>(i);   // tail (n % 4 entries)
}

// blocks of 256 threads for n entries; memory-bound: one vector per lane up to 2048 blocks (256 CUs x 8),
// grid-stride the rest
inline int flat_grid(long n) {
  long blocks = (n / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  return (int)blocks;
}

template <class Op>
void flat_map(hipStream_t st, long n, const Op& op) {
  if (n <= 0) return;
  hipLaunchKernelGGL(flat_map_kernel<Op>, dim3(flat_grid(n)), dim3(256), 0, st, op, n);
}

}  // namespace fedmi
