// fedmi — public interface of the dense convolution launchers (conv_igemm.hip): the one declaration the defining
// file and the Python bindings (bindings_cnn.cpp) both include.
#pragma once
#include <vector>

#include "common.h"
#include "conv_geom.h"      // ConvShape
#include "wgrad_reduce.h"   // WredItem

namespace fedmi {

// Y[N,P,Q,O] = conv(X[N,H,W,C], W_rsc); stats (optional) += [sum | sumsq] of (Y - shift) per output channel.
// ws / ws_floats: optional split-K workspace (null / 0 floats: never split).  res: a residual added in the epilogue
// (tap path only).
void launch_conv_fwd(hipStream_t st, const ConvShape& s, const bf16* x, const bf16* wrsc, bf16* y, double* stats,
                     const float* shift, float* ws, long ws_floats, const bf16* res);

// dX[N,H,W,C] = conv_transpose(dY[N,P,Q,O], W_rsc)   (every element written).
// wd: the DGRAD weight image (launch_dgrad_pack_multi) opens the tap path.  acc: dx += result (the data gradient of
// one branch of a multi-branch block).  add: dx = result + add (a second incoming grad, e.g. the shortcut branch's;
// != dx) and bs: the producer BN's backward sums taken in the epilogue -- both only where conv_dgrad_fusable.
void launch_conv_dgrad(hipStream_t st, const ConvShape& s, const bf16* dy, const bf16* wrsc, bf16* dx, float* ws,
                       long ws_floats, const bf16* wd, int acc, const bf16* add, const BnSums* bs);
int conv_dgrad_fusable(const ConvShape& s, int has_wd);

// Workspace (floats) split-K FWD + DGRAD want for this shape (0: they never split).
long conv_fd_ws_floats(const ConvShape& s);

// dW[O][Cw][R][S] (fp32, PyTorch layout) = (or +=) X^T dY.  ``ws`` holds
// ws_floats floats; splits <= 0 picks automatically within that capacity.
// dw: [Ow][Cw][R][S] (Ow <= 0: O) -- the first Ow filters of an O-padded conv land in the unpadded gradient.
// G > 1: a grouped conv run densely with a block-diagonal weight image; filter o keeps only its group's Cw
// channels of the dense gradient.
// defer: the partial reduction is not launched; its descriptor is stored for launch_wgrad_reduce_multi.
// allow_1x1 = 0: no conv_wgrad_halo<1> route (the aten backend: mixed results across the zoo families)
void launch_conv_wgrad(hipStream_t st, const ConvShape& s, const bf16* x, const bf16* dy, float* dw, float* ws,
                       long ws_floats, int splits, int accumulate, int Ow, int G, WredItem* defer, int allow_1x1);
long conv_wgrad_ws_floats(const ConvShape& s);

// Forward weight images [O8][R][S][C] bf16 from the fp32 masters [O][Cw][R][S].
struct PackItem {
  const float* w;
  bf16* wr;
  int O, Cw, C, RS;
  int O8;            // <= 0: O (no zero filters)
  int G;             // <= 1: dense; > 1: block-diagonal image of a grouped conv (C = G * Cw channels)
};
void launch_conv_pack_multi(hipStream_t st, const PackItem* items, int n);
void launch_conv_pack(hipStream_t st, const float* w, bf16* wrsc, int O, int Cw, int C, int RS, int O8, int G);

// DGRAD weight images (conv_tap layout, phases concatenated) for several convs.
struct DPackItem {
  const float* w;
  bf16* wd;
  int O, Cw, C, R, S, st, pad;
};
void launch_dgrad_pack_multi(hipStream_t st, const DPackItem* items, int n);

// Fused SGD + weight images (sgd_pack_kernel): the host builds the table once per engine (convs first, then the
// flat segments, in workgroup order); the caller copies `table` to device memory and launches with it.
struct SgdPackConv {
  long off;          // element offset of the fp32 weight [O][Cw][R][S] in the flat master
  bf16* wr;          // forward image [O][R][S][C] (nullptr: none)
  bf16* wd;          // DGRAD image, phases concatenated (nullptr: none; needs O % 64 == 0, or O % 8 at stride 1)
  int O, Cw, C, R, S, st, pad;
};
struct SgdPackPlan {
  std::vector<char> table;
  int n_entries, n_blocks, lds_bytes;
};
SgdPackPlan build_sgd_pack_plan(const SgdPackConv* convs, int nc, const long* segs, int nseg);
void launch_sgd_pack(hipStream_t st, const void* table, int n_entries, int n_blocks, int lds_bytes, float* P,
                     const float* G, float* B, float lr, float m, float wd, float dampening, int nesterov, int first);

}  // namespace fedmi
