// fedmi — the convolution problem and the POD geometry the conv kernels take by value (conv_igemm.hip) and the
// host planner fills (conv_plan.h).  Plain C++: no device code, no HIP runtime.
#pragma once
#include <stdint.h>

namespace fedmi {

// One dense convolution: input [N][H][W][C] (C padded to % 8, Cw real channels), O filters R x S, output P x Q.
struct ConvShape {
  int N, H, W, C, Cw, O, P, Q, R, S, st, pad;
};

}  // namespace fedmi

// Internal linkage on purpose: the kernels are local to conv_igemm.hip, and so are their argument types.
namespace {

constexpr int BK = 64;   // K step of every conv GEMM

struct FastDiv {   // q = x / d for 0 <= x < 2^31 (Granlund-Montgomery)
  uint32_t d, m, s;
};

inline FastDiv make_div(uint32_t d) {
  FastDiv f;
  f.d = d;
  uint32_t s = 0;
  while ((1ull << s) < d) ++s;
  f.s = s;
  f.m = (uint32_t)((((1ull << 32) * ((1ull << s) - d)) / d) + 1);
  return f;
}

struct ConvGeom {
  int N, H, W, C;          // input (C = padded channel count, % 8 == 0)
  int O, P, Q;             // output channels / spatial
  int R, S, st, pad;
  int M, NC, K;            // GEMM rows / cols / reduction for the launched mode
  int Cw;                  // channel count of the fp32 master weight (unpadded; WGRAD epilogue)
  // DGRAD sub-pixel phase (stride 2: one launch per output parity (ph, pw), each
  // summing only the taps r = r0 + 2i, s = s0 + 2j that land on that parity;
  // stride 1: ph = pw = 0, r0 = s0 = 0, nr = R, ns = S, Hp = H, Wp = W)
  int ph, pw, r0, s0, nr, ns, Hp, Wp;
  FastDiv dC, dO, dS, dQ, dPQ, dW, dHW, dNS, dWp, dHWp;
};

// GEMM row m = (n, p, q) over an output grid P x Q -> row of the stored output:
// identity, or the stride-`st` sub-pixel scatter of a DGRAD phase:
// ((n * OH + p * st + ph) * OW + q * st + pw).
struct RowMap {
  int on;
  int P, Q, OH, OW, st, ph, pw;
  FastDiv dPQ, dQ;
};

// conv_tap problem
struct TapGeom {
  int N, H, W, C;          // input [N][H][W][C], C % 64 == 0
  int O;                   // GEMM columns = weight rows [O][R][S][C]
  int P, Q;                // output grid, GEMM rows M = N * P * Q
  int R, S, st, pad_h, pad_w;
  int M, K;                // K = R * S * C
  FastDiv dPQ, dQ;
};

// The sub-pixel phases of a stride-2 DGRAD in one conv_tap_phases launch.
constexpr int MAX_TAP_PHASES = 4;
struct TapMulti {
  TapGeom g[MAX_TAP_PHASES];
  RowMap rm[MAX_TAP_PHASES];
  long woff[MAX_TAP_PHASES];       // weight-image offset (elements)
  long wsoff[MAX_TAP_PHASES];      // workspace offset (floats), -1: no split (the epilogue writes dX)
  int kps[MAX_TAP_PHASES];         // K steps per split
  int splits[MAX_TAP_PHASES];
  int tile0[MAX_TAP_PHASES + 1];   // first tile of each phase; tile0[n] = total
  int n;
};

// Halo-patch geometry for 3x3 / stride 1 / pad 1: a 128-pixel tile is IMGS images x TH rows x W
// columns whose input window (TH + 2 rows x W + 2 columns per image, zero halo) is DMA'd into LDS
// once per 64-channel chunk; the nine taps read shifted rows of the same patch (conv_wgrad_halo).
struct HaloGeom {
  int N, H, W, C, O;
  int M, K;                // M = N * H * W output pixels, K = 9 * C (weight row length)
  int TH, IMGS;            // tile = IMGS images x TH rows x W columns = 128 pixels
  int PW, NPR;             // patch row width W + 2, patch rows IMGS * (TH + 2) * (W + 2)
  int nchunks;             // C / 64
  FastDiv dPI, dPW, dTHW, dW, dHW;   // by (TH + 2) * PW, PW, TH * W, W, H * W
};

struct StemGeom {
  int N, H, W, O, M;   // input [N][H][W][8], output [N][H][W][O], M = N * H * W
};

}  // namespace
