// fedmi — cross-lane exchange in registers (gfx950, wave64): the butterflies of the LeNet sample step (KS1)
// on DPP and lane-permute instructions instead of ds_bpermute_b32 (what __shfl_xor / __shfl compile to: a
// trip through the LDS pipeline, waited for with s_waitcnt lgkmcnt(0), per step).
//
// Contract of every helper: for every lane, the result has the SAME BITS as the __shfl_xor butterfly it
// replaces.  At each step the same two values are added (or max'd / min'd), in the same step order; only
// which lane supplies the partner's copy may differ.  Two facts carry that:
//
//  (a) v_add_f32 / v_max_f32 / v_min_f32 of two non-NaN operands give the same bits in either operand order
//      (max / min order -0 below +0).  So after the xor-w step of an all-reduce both partners hold identical
//      bits: each combined the same two values.  (NaN operands are outside the contract: KS1 feeds none.)
//
//  (b) xor 4.  gfx9 DPP has no xor-4 pattern.  row_half_mirror gives lane i (of an aligned group of 8) the
//      value of lane 7 - i.  AFTER the xor-1 and xor-2 steps the four lanes of a quad hold identical bits by
//      (a), and lanes i ^ 4 and 7 - i lie in the same quad (the other one of the group), so lane 7 - i holds
//      exactly what lane i ^ 4 holds.  This is why the step order 1, 2, 4, 8 is kept and why row_half_mirror
//      may stand only behind the two quad_perm steps.
//
//  xor 1, xor 2   quad_perm:[1,0,3,2], quad_perm:[2,3,0,1]   -- the partner lane itself
//  xor 4          row_half_mirror, see (b)
//  xor 8          row_ror:8                                   -- the partner lane itself
//  xor 16, 32     v_permlane16_swap_b32 / v_permlane32_swap_b32 of two copies (a, b) of v: the swap leaves a
//                 with the even rows' (lower half's) values in both rows of a pair (both halves) and b with the
//                 odd rows' (upper half's), so a + b is own + partner in the even rows (lower half) and
//                 partner + own in the others: the same bits by (a).
//
// Every helper needs all 64 lanes active (a DPP read of an inactive lane gives 0, a swap skips it); the call
// sites sit under wave-uniform conditions only.
//
// The DPP operand is folded into the consuming VALU instruction, one instruction per step:
//  * sums: the move is written as update_dpp with bound_ctrl and full row / bank masks, the form the
//    compiler's DPP combiner accepts (mov_dpp's pattern passes the source as the `old` operand as well, which
//    it does not), and the result passes through an empty asm: without it the last add of a butterfly sinks
//    into the `if (lane == ...)` block that stores it, and a move cannot be combined across a change of EXEC.
//    The wait states between a VALU write and a DPP or permlane read of the same register are the compiler's
//    to insert for the builtins.
//  * max / min: fmaxf / fminf of a value the compiler cannot prove canonical get a v_max_f32 x, x, x in front
//    (sNaN quieting, a no-op for every other value, denormals included: they are not flushed here), which
//    stands between the move and its user.  These steps are one v_max_f32_dpp / v_min_f32_dpp in inline
//    assembly, each with the two wait states a DPP read needs after a VALU write of its source (s_nop 1) in
//    its own string.  For non-NaN operands the instruction gives fmaxf's / fminf's bits.
//    These asm statements need no pin() against the sinking described above: clang marks every inline asm of
//    HIP device code convergent, so it is never moved under a condition it did not stand under (a step sunk
//    into an `if (lane < 16)` block would read inactive lanes as 0 through bound_ctrl).
//    NOT covered: the compiler's hazard recognizer does not look inside inline assembly, and a VALU write of
//    EXEC (v_cmpx) directly in front of a DPP instruction needs 5 wait states on gfx9.  hipcc emits no v_cmpx
//    for gfx950 in KS1 today (it masks with s_and_saveexec); a call site behind one would need its own pad.
//    Where the compiler pads a builtin's result in front of one of these steps as well, a wait state or two
//    is spent twice (the cross-entropy block: 8 steps).
#pragma once
#include "common.h"

namespace xlane {

constexpr int DPP_XOR1 = 0xB1;          // quad_perm:[1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;          // quad_perm:[2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141;  // row_half_mirror
constexpr int DPP_ROR = 0x120;          // row_ror:n = DPP_ROR + n

template <int CTRL>
FEDMI_DEV float dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

FEDMI_DEV float pin(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// all-reduce sum over aligned groups of 8 lanes: the xor 1, 2, 4 butterfly
FEDMI_DEV float sum8_steps(float v) {
  v += dpp<DPP_XOR1>(v);
  v += dpp<DPP_XOR2>(v);
  v += dpp<DPP_HALF_MIRROR>(v);
  return v;
}
FEDMI_DEV float sum8(float v) { return pin(sum8_steps(v)); }
// all-reduce sum over a DPP row of 16 lanes: the xor 1, 2, 4, 8 butterfly
FEDMI_DEV float sum16(float v) {
  v = sum8_steps(v);
  v += dpp<DPP_ROR + 8>(v);
  return pin(v);
}

// one max / min step: v op (v of the lane the DPP control names), see the header
#define FEDMI_XLANE_STEP(name, insn, ctrl)                                                              \
  FEDMI_DEV float name(float v) {                                                                       \
    float r;                                                                                            \
    asm("s_nop 1\n\t" insn " %0, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(r) : "v"(v)); \
    return r;                                                                                           \
  }
FEDMI_XLANE_STEP(max_xor1, "v_max_f32_dpp", "quad_perm:[1,0,3,2]")
FEDMI_XLANE_STEP(max_xor2, "v_max_f32_dpp", "quad_perm:[2,3,0,1]")
FEDMI_XLANE_STEP(max_half_mirror, "v_max_f32_dpp", "row_half_mirror")
FEDMI_XLANE_STEP(max_ror8, "v_max_f32_dpp", "row_ror:8")
FEDMI_XLANE_STEP(min_xor1, "v_min_f32_dpp", "quad_perm:[1,0,3,2]")
FEDMI_XLANE_STEP(min_xor2, "v_min_f32_dpp", "quad_perm:[2,3,0,1]")
FEDMI_XLANE_STEP(min_half_mirror, "v_min_f32_dpp", "row_half_mirror")
FEDMI_XLANE_STEP(min_ror8, "v_min_f32_dpp", "row_ror:8")
#undef FEDMI_XLANE_STEP
// all-reduce max / min over a DPP row of 16 lanes: the xor 1, 2, 4, 8 butterfly
FEDMI_DEV float max16(float v) { return max_ror8(max_half_mirror(max_xor2(max_xor1(v)))); }
FEDMI_DEV float min16(float v) { return min_ror8(min_half_mirror(min_xor2(min_xor1(v)))); }

// v + (v of lane ^ 16), v + (v of lane ^ 32)
FEDMI_DEV float add_xor16(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}
FEDMI_DEV float add_xor32(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}
// all-reduce over aligned groups of 32 lanes: the xor 1, 2, 4, 8, 16 butterfly
FEDMI_DEV float sum32(float v) { return add_xor16(sum16(v)); }

// sum over the 16 lanes of a DPP row by rotations 8, 4, 2, 1: every lane ends with the row total, each in
// its own fixed order (fc1's row sums: lane 0 of the row is the one read).  N values at once, step by step
// across all of them, so that N independent chains are in flight (fc1 forward: its 8 rows); N = 1 is the
// plain row sum.
template <int R, int N>
FEDMI_DEV void ror_add(float (&v)[N]) {
#pragma unroll
  for (int m = 0; m < N; ++m) v[m] += dpp<DPP_ROR + R>(v[m]);
}
template <int N>
FEDMI_DEV void row_sum16(float (&v)[N]) {
  ror_add<8>(v);
  ror_add<4>(v);
  ror_add<2>(v);
  ror_add<1>(v);
#pragma unroll
  for (int m = 0; m < N; ++m) v[m] = pin(v[m]);
}
FEDMI_DEV float row_sum16(float v) {
  float a[1] = {v};
  row_sum16(a);
  return a[0];
}

// v of lane `src`, which must be the same in every lane of the wave (it is made scalar here)
FEDMI_DEV float bcast(float v, int src) {
  const int sl = __builtin_amdgcn_readfirstlane(src) & 63;
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), sl));
}

}  // namespace xlane
