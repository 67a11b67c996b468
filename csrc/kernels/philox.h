// fedmi — the counter-based generator of standard normals that dp.hip (the DP noise) and powersgd.hip (the start of
// the Q factors) share.
//
// Philox4x32-10 (Salmon et al. 2011), key = 64 bits, counter = (block lo, block hi, draw lo, draw hi) with
// block = i >> 2; entry i takes lane i & 3 of its block.  The four outputs r0..r3 give two Box-Muller pairs:
// u(r) = ((r >> 9) + 0.5) * 2^-23 is exact in fp32 and never 0 or 1; lanes 0, 1 = sqrt(-2 ln u(r0)) * {cos, sin}(2 pi u(r1)),
// lanes 2, 3 the same from r2, r3.  The angle goes through sincospif(2 u): 2 u is exact, so no rounded multiple of pi
// enters the result.  logf / sqrtf / sincospif are the accurate library functions, not the fast intrinsics.
#pragma once
#include "common.h"

namespace fedmi {

struct Philox {
  uint32_t k0, k1, d0, d1;   // key and draw, low word first

  static FEDMI_DEV void round(uint32_t (&c)[4], uint32_t ka, uint32_t kb) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ ka;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ kb;
    c[3] = lo0;
  }

  // the four 32-bit outputs of one block
  FEDMI_DEV void block(long blk, uint32_t (&c)[4]) const {
    c[0] = (uint32_t)blk;
    c[1] = (uint32_t)((unsigned long)blk >> 32);
    c[2] = d0;
    c[3] = d1;
    uint32_t ka = k0, kb = k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      round(c, ka, kb);
      ka += 0x9E3779B9u;
      kb += 0xBB67AE85u;
    }
  }
};

FEDMI_DEV float unit_open(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 0x1p-23f; }

// one Box-Muller pair from two 32-bit words: (radius * cos, radius * sin)
FEDMI_DEV void box_muller(uint32_t ra, uint32_t rb, float& gc, float& gs) {
  const float radius = sqrtf(-2.f * logf(unit_open(ra)));
  float s, c;
  sincospif(2.f * unit_open(rb), &s, &c);
  gc = radius * c;
  gs = radius * s;
}

// the standard normal of entry e (lane e & 3 of block e >> 2)
FEDMI_DEV float philox_normal(const Philox& rng, long e) {
  uint32_t r[4];
  rng.block(e >> 2, r);
  const int lane = (int)(e & 3);
  float gc, gs;
  box_muller((lane & 2) ? r[2] : r[0], (lane & 2) ? r[3] : r[1], gc, gs);
  return (lane & 1) ? gs : gc;
}

}  // namespace fedmi
