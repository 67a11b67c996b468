// fedmi — flat-buffer elementwise kernels for the generic (model-zoo) engine
// (FedAvg itself is one collective over the flat buffer: fedmi/parallel/fedavg.py).
//
//  * sgd_flat:       torch.optim.SGD(momentum, weight_decay) over ONE flat fp32
//                    parameter buffer (multi-tensor apply in a single launch;
//                    the reference issues 4 ops x #tensors, src/main.py:151).
// All kernels stream 16 B per lane and grid-stride (memory-bound; HBM roof).
#include "flat_map.h"

namespace {

struct SgdFlat {
  float* p;
  const float* g;
  float* buf;
  float lr, m, wd, dampening;
  int nesterov, first;
  template <int W>
  FEDMI_DEV void run(long e) const {
    auto pv = fedmi::flat_load<W>(p, e);
    const auto gv = fedmi::flat_load<W>(g, e);
    auto bv = fedmi::flat_load<W>(buf, e);
#pragma unroll
    for (int j = 0; j < W; ++j) fedmi::sgd_elem(pv[j], gv[j], bv[j], lr, m, wd, dampening, nesterov, first);
    fedmi::flat_store<W>(p, e, pv);
    fedmi::flat_store<W>(buf, e, bv);
  }
};

}  // namespace

namespace fedmi {

void launch_sgd_flat(hipStream_t st, float* p, const float* g, float* buf, long n, float lr, float m, float wd,
                     float dampening, int nesterov, int first) {
  flat_map(st, n, SgdFlat{p, g, buf, lr, m, wd, dampening, nesterov, first});
}

}  // namespace fedmi
