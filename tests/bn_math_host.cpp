// Stand-alone host program for tests/test_bn_math.py: evaluates every function of csrc/kernels/bn_math.h on the
// rows of tests/golden/bn_math_inputs.txt (six fp32 and two fp64 as hex words, M) read from stdin, and prints the
// results' bits, one row per line in the order of bn_check.OUTPUTS.  The operand each function takes from a row is
// fixed here and mirrored by bn_check.evaluate.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "kernels/bn_math.h"

static float f32(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static double f64(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main() {
  uint32_t w[6];
  uint64_t dw[2];
  int M, rows = 0;
  while (std::scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx64 " %" SCNx64 " %d",
                    &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &dw[0], &dw[1], &M) == 9) {
    const float a = f32(w[0]), b = f32(w[1]), c = f32(w[2]), d = f32(w[3]), e = f32(w[4]);
    float bm, bv;
    bn::bn_batch_stats(f64(dw[0]), f64(dw[1]), M, &bm, &bv);
    const float out[] = {
        bn::bn_affine(a, b, c), bn::bn_add(a, b), bn::bn_relu(a), bn::bn_sum_term(a, b, c, d, e),
        bn::bn_dz(a, b, c, d, e), bn::bn_dz_add(a, b), bm, bv, bn::bn_unshift(a, b),
        bn::bn_inv_std(fabsf(a), fabsf(b)), bn::bn_running_mean(a, b, c, d), bn::bn_running_var(a, b, c, M),
        bn::bn_eval_mean(a, b), bn::bn_scale(a, b), bn::bn_shift(a, b, c), bn::bn_inv_count(M),
        bn::bn_bwd_b(a, b, c, d), bn::bn_bwd_c(a, b, c, d, e)};
    for (float v : out) std::printf("%08" PRIx32 " ", bits(v));
    std::printf("\n");
    ++rows;
  }
  std::fprintf(stderr, "bn_math_host: %d rows\n", rows);
  return rows > 0 ? 0 : 1;
}
