// fedmi — public interface of the non-GEMM CNN launchers: BatchNorm, pooling, input prep, classifier head
// (cnn_ops.hip) and depthwise convolution (dwconv.hip).  Included by the defining files and by bindings_cnn.cpp.
#pragma once
#include "common.h"
#include "wgrad_reduce.h"   // WredItem

namespace fedmi {

struct BNDesc {
  const double* stats; const float* gamma; const float* beta; float* rmean; float* rvar; long long* nbt;
  float* smean; float* sinv; const float* shift; const float* cbias;
};
struct BNBwdDesc {
  const bf16* dya; const bf16* dyb; const bf16* y;
  const bf16* za; const float* meanA; const float* invA; const float* gammaA; float* dgammaA; float* dbetaA; bf16* dza;
  const bf16* zb; const float* meanB; const float* invB; const float* gammaB; float* dgammaB; float* dbetaB; bf16* dzb;
  bf16* gout;
  float* shiftA; float* shiftB;
  const bf16* dadd;
  const float* msc;
};

void launch_maxpool2(hipStream_t st, const bf16* x, bf16* y, int N, int H, int W, int C);
void launch_maxpool2_bwd(hipStream_t st, const bf16* x, const bf16* dy, bf16* dx, int N, int H, int W, int C);
void launch_maxpool3(hipStream_t st, const bf16* x, bf16* y, uint8_t* idx, int N, int H, int W, int C, int stride);
void launch_maxpool3_bwd(hipStream_t st, const bf16* dy, const uint8_t* idx, bf16* dx, int N, int H, int W, int C,
                         int stride, int acc);
void launch_prep_input(hipStream_t st, const uint8_t* images, int base, const int* dbase, int nb, int augment,
                       uint32_t seed, const int* round_ctr, bf16* out);
void launch_sched_next(hipStream_t st, const int* sched, int* counter, int* cur, double* zero, long n);
void launch_bn_apply(hipStream_t st, const bf16* z, const BNDesc& a, const bf16* z2, const BNDesc* b, const bf16* res,
                     bf16* y, int M, int C, float eps, float mom, int train, int relu, int ldy, float* co_out);
void launch_bn_bwd(hipStream_t st, const BNBwdDesc& d, double* red, int M, int C, double* ws, long ws_floats, int ldd,
                   int ldy, int chained, int presummed);
long bn_bwd_ws_floats(int M, int C);
int bn_bwd_chain_reps(int C);
void launch_head(hipStream_t st, const bf16* y, const int* labels, int base, const int* dbase, int N, int HW, int C, int J,
                 const float* W, const float* b, float* pooled, float* dlog, bf16* dy, float* stats, float* lossv,
                 float* dW, float* db, int train, float* zero_buf, long zero_n);

// depthwise convolution (dwconv.hip)
struct DwShape {
  int N, H, W, C, R, S, st, pad;
};
void launch_dw_fwd(hipStream_t st, const DwShape& s, const bf16* x, const float* w, bf16* y, double* stats,
                   const float* shift);
void launch_dw_dgrad(hipStream_t st, const DwShape& s, const bf16* dy, const float* w, bf16* dx, const BnSums* bs);
long dw_wgrad_ws_floats(const DwShape& s);
void launch_dw_wgrad(hipStream_t st, const DwShape& s, const bf16* x, const bf16* dy, float* dw, float* ws,
                     long ws_floats, int accumulate, WredItem* defer);

}  // namespace fedmi
