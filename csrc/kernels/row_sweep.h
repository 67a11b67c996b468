// fedmi — the one sweep over W gathered fp32 rows (row r = client r's state), shared by robust_reduce (robust.hip),
// geomed_pass (geomed.hip) and the fused peer_robust_f32_kernel (comm/peer_comm.hip).
//
// A lane takes one float4 per row (4 coordinates, W independent 16-B loads in flight), transposes them to x[c][r],
// asks the rule for the four results, stores them with one 16-B store and then lets the rule accumulate from the
// values still in registers; the n % 4 entries after the whole vectors go one by one through the same two calls, so
// body and tail cannot differ.  Grid-strided by (long)gridDim.x * blockDim.x: vector i = t, t + stride, .. and then
// tail entry 4 (n / 4) + t, .. of lane t, in that order (geomed's fp64 sums rely on it).
//
//   rows :  rows(r) = pointer to row r, 16-byte aligned, n floats readable (StridedRows: base + r * ld)
//   rule :  float coord(const float (&x)[W])             the result of one coordinate from its value on ranks 0 .. W-1;
//                                                        called for c = 0..3 of a vector in that order, before the store
//           void stored(const float (&x)[W], float z)    the same x and its result z, after the store, c = 0..3 again
//           (a tail entry: coord, the store, stored).  The rule keeps its own side state (cut counters, fp64 sums).
//
// No __restrict__ on any pointer that reaches this loop, and `unroll 1` on both trips: either lets the compiler hoist
// the next trip's W loads over the rule, and every width from 3 up then takes all 256 VGPRs and spills
// (profiles/r14_robust/README.md §1).  The workgroup size is read with the scalar builtin: blockDim.x, read in a device
// function and not in the kernel itself, became a vector load and put the stride into VGPRs -- 4 more registers and
// one wave per SIMD less at W = 6, 8 and 11 (profiles/r23_row_sweep/README.md).  No fp32 arithmetic happens here, so the header compiles to the same code with
// and without packed fp32 instructions (geomed.hip is built without).
#pragma once
#include "flat_map.h"

namespace fedmi {

struct StridedRows {
  const float* base;
  long ld;
  FEDMI_DEV const float* operator()(int r) const { return base + r * ld; }
};

template <int W, class Rows, class Rule>
FEDMI_DEV void row_sweep(const Rows& rows, long n, float* out, Rule& rule) {
  const long n4 = n >> 2;
  const int lanes = __builtin_amdgcn_workgroup_size_x();   // == blockDim.x, see above
  const long stride = (long)gridDim.x * lanes;
  const long t = (long)blockIdx.x * lanes + threadIdx.x;
#pragma unroll 1
  for (long i = t; i < n4; i += stride) {
    FlatVec<4> v[W], o;
#pragma unroll
    for (int r = 0; r < W; ++r) v[r] = flat_load<4>(rows(r), i << 2);
    float x[4][W];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int r = 0; r < W; ++r) x[c][r] = v[r][c];
      o[c] = rule.coord(x[c]);
    }
    flat_store<4>(out, i << 2, o);
#pragma unroll
    for (int c = 0; c < 4; ++c) rule.stored(x[c], o[c]);
  }
#pragma unroll 1
  for (long i = (n4 << 2) + t; i < n; i += stride) {   // tail (n % 4 entries)
    float x[W];
#pragma unroll
    for (int r = 0; r < W; ++r) x[r] = rows(r)[i];
    const float z = rule.coord(x);
    out[i] = z;
    rule.stored(x, z);
  }
}

}  // namespace fedmi
