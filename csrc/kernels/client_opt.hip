// fedmi — client-side drift correction inside the local SGD step (fedmi/parallel/client_opt.py).
//
// Under non-IID shards every client's iterates walk toward its own optimum during the local epoch.  Two
// remedies change the gradient the SGD tail consumes; all buffers are fp32 and n = n_params() entries long:
//   DriftGrad<FEDPROX>  (once per step):  g = fma(mu, p - anchor, g)          (Li et al. 2020; anchor = the
//                                                                              round's starting model)
//   DriftGrad<SCAFFOLD> (once per step):  acc = acc + g;  g = g + corr        (Karimireddy et al. 2020;
//                                                                              corr = c - c_i, acc sums the RAW g)
//   ScaffoldFinish (once per round, before the collective):
//                                         new = acc / K;  delta = new - ci;  ci = new
//   ScaffoldBegin  (once per round, after the collective):
//                                         c = c + dmean;  corr = c - ci;  acc = 0
// c_i is the mean of the round's raw gradients, not (w_global - y_K)/(K*lr): the clients run momentum that
// persists across rounds, for which the latter is not the gradient mean.
//
// Streams 16 B per lane and grid-strides on the shared skeleton (flat_map.h; memory-bound: 16 B per entry for
// FedProx, 20 B for SCAFFOLD's step).  DriftGrad is specialised on the kind, so a kind never touches a buffer it
// does not need (those may be null).  Every output is one correctly rounded fp32 operation (the fma and the division
// are written as such, so the compiler's contraction / reciprocal choices are not part of the result) computed
// by one lane from its own inputs: no atomics, no LDS, the same bits on every rank.
#include "flat_map.h"

namespace {

using fedmi::flat_load;
using fedmi::flat_store;

enum { FEDPROX = 0, SCAFFOLD = 1 };

template <int KIND>
struct DriftGrad {
  float* g;
  const float *p, *anchor, *corr;
  float* acc;
  float mu;
  template <int W>
  FEDMI_DEV void run(long e) const {
    auto gv = flat_load<W>(g, e);
    if (KIND == FEDPROX) {
      const auto pv = flat_load<W>(p, e), av = flat_load<W>(anchor, e);
#pragma unroll
      for (int j = 0; j < W; ++j) gv[j] = __fmaf_rn(mu, pv[j] - av[j], gv[j]);
    } else {
      const auto cv = flat_load<W>(corr, e);
      auto sv = flat_load<W>(acc, e);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        sv[j] = sv[j] + gv[j];
        gv[j] = gv[j] + cv[j];
      }
      flat_store<W>(acc, e, sv);
    }
    flat_store<W>(g, e, gv);
  }
};

struct ScaffoldFinish {
  const float* acc;
  float *ci, *delta;
  float k;
  template <int W>
  FEDMI_DEV void run(long e) const {
    const auto av = flat_load<W>(acc, e);
    auto cv = flat_load<W>(ci, e);
    fedmi::FlatVec<W> dv;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float nw = __fdiv_rn(av[j], k);
      dv[j] = nw - cv[j];
      cv[j] = nw;
    }
    flat_store<W>(ci, e, cv);
    flat_store<W>(delta, e, dv);
  }
};

struct ScaffoldBegin {
  float* c;
  const float *dmean, *ci;
  float *corr, *acc;
  template <int W>
  FEDMI_DEV void run(long e) const {
    auto cv = flat_load<W>(c, e);
    const auto dv = flat_load<W>(dmean, e), iv = flat_load<W>(ci, e);
    fedmi::FlatVec<W> rv;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      cv[j] = cv[j] + dv[j];
      rv[j] = cv[j] - iv[j];
    }
    flat_store<W>(c, e, cv);
    flat_store<W>(corr, e, rv);
    flat_store<W>(acc, e, fedmi::FlatVec<W>{});
  }
};

}  // namespace

namespace fedmi {

// kind: 0 fedprox (g, p, anchor, mu), 1 scaffold (g, corr, acc); the other kind's buffers may be null.  Every
// buffer holds n floats and is 16-byte aligned (the binding checks all of it).
void launch_drift_grad(hipStream_t st, int kind, float* g, const float* p, const float* anchor, const float* corr,
                       float* acc, float mu, long n) {
  if (kind == FEDPROX)
    flat_map(st, n, DriftGrad<FEDPROX>{g, p, anchor, corr, acc, mu});
  else if (kind == SCAFFOLD)
    flat_map(st, n, DriftGrad<SCAFFOLD>{g, p, anchor, corr, acc, mu});
}

void launch_scaffold_finish(hipStream_t st, const float* acc, float* ci, float* delta, long K, long n) {
  if (K < 1) return;
  flat_map(st, n, ScaffoldFinish{acc, ci, delta, (float)K});
}

void launch_scaffold_begin(hipStream_t st, float* c, const float* dmean, const float* ci, float* corr, float* acc,
                           long n) {
  flat_map(st, n, ScaffoldBegin{c, dmean, ci, corr, acc});
}

}  // namespace fedmi
