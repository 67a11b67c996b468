// fedmi — Python bindings for the native runtime and HIP kernels.
//
// Device memory is owned by PyTorch tensors (caching allocator); the native
// side receives raw device pointers and the torch stream handle, so every
// launch is ordered on torch's current stream and can be graph-captured.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <string>
#include <vector>

#include "kernels/common.h"
#include "kernels/lenet_layout.h"
#include "runtime/lenet_engine.h"

namespace py = pybind11;

namespace fedmi {
void launch_lenet_conv_fwd(hipStream_t, const uint8_t*, int, int, const bf16*, const float*, uint32_t, const int*, int,
                           bf16*, bf16*, int, bf16*, uint8_t*, uint8_t*, lenet::Stats*);
void launch_lenet_fc_eval(hipStream_t, const bf16*, const int*, int, const bf16*, const float*, float*, long,
                          lenet::Stats*);
bool stamps_enabled();
void read_stamps(unsigned long long*, bool);
void set_ks1_diag(int);
void launch_lenet_pack(hipStream_t, const float*, bf16*);
void launch_lenet_prep_batch(hipStream_t, const uint8_t*, int, int, uint32_t, const int*, int, bf16*);
int xlane_probe_helpers();
void launch_lenet_xlane_probe(hipStream_t, const float*, const int*, int, float*);
void launch_sgd_flat(hipStream_t, float*, const float*, float*, long, float, float, float, float, int, int);
void launch_server_opt(hipStream_t, float*, float*, float*, float*, long, long, int, float, float, float, float);
void launch_drift_grad(hipStream_t, int, float*, const float*, const float*, const float*, float*, float, long);
void launch_scaffold_finish(hipStream_t, const float*, float*, float*, long, long);
void launch_scaffold_begin(hipStream_t, float*, const float*, const float*, float*, float*, long);
int dp_partials(long);
void launch_dp(hipStream_t, float*, const float*, long, double*, double*, double, float, uint64_t, uint64_t, int);
int robust_partials(long);
void launch_robust_reduce(hipStream_t, const float*, long, int, long, int, float*, long long*, long long*);
int geomed_partials(long);
void launch_geomed_pass(hipStream_t, const float*, long, int, long, bool, const float*, const double*, double, float*,
                        double*, double*, int);
void launch_geomed(hipStream_t, const float*, long, int, long, int, double, float*, double*, double*);
int krum_partials(long);
void launch_krum_gram(hipStream_t, const float*, long, int, long, double*, double*);
void launch_krum(hipStream_t, const float*, long, int, long, int, bool, float*, double*, double*);
int bulyan_partials(long);
void launch_bulyan(hipStream_t, const float*, long, int, long, int, float*, double*, double*);
void launch_bulyan_fold(hipStream_t, const float*, long, int, long, const int*, int, int, float*, double*, double*);
int dnc_partials(long);
void launch_dnc_gram(hipStream_t, const float*, long, int, long, double*, double*);
void launch_dnc(hipStream_t, const float*, long, int, long, int, float*, double*, double*);
int secagg_partials(long);
void launch_secagg_mask(hipStream_t, const float*, const float*, const uint32_t*, int, int, uint64_t, long, int,
                        uint32_t*, long long*, long long*);
void launch_secagg_unmask(hipStream_t, const float*, long, int, const float*, long, int, float*);
void launch_ef_delta(hipStream_t, const float*, const float*, const float*, float*, long);
size_t topk_state_bytes();
size_t topk_overflow_offset();
void launch_topk_ef(hipStream_t, const float*, const float*, float*, long, int, void*, int*, unsigned*, int*, float*);
void launch_scatter_add_ranked(hipStream_t, float*, const int*, const float*, int, long, float, long);
void launch_quant_int8(hipStream_t, const float*, long, signed char*, float*, float*);
void launch_dequant_accum(hipStream_t, const signed char*, const float*, int, long, float*, float);
void psgd_geometry(int (&)[11]);
void launch_psgd_qinit(hipStream_t, float*, long, uint64_t);
void launch_psgd_project(hipStream_t, const float*, const float*, float*, const void*, const void*, int, const float*, int,
                         float*, float*, const void*, int);
void launch_psgd_orth(hipStream_t, const void*, int, float*, int);
void launch_psgd_backproject(hipStream_t, const float*, const void*, const void*, int, const float*, int, float*, float*,
                             const void*, int);
void launch_psgd_apply(hipStream_t, float*, float*, float*, const void*, const void*, int, const float*, const float*,
                       const float*, int);
}  // namespace fedmi

using namespace fedmi;

void fedmi_bind_cnn(py::module_& m);   // bindings_cnn.cpp
void fedmi_bind_comm(py::module_& m);  // bindings_comm.cpp
void fedmi_bind_zoo(py::module_& m);   // bindings_zoo.cpp
void fedmi_bind_io(py::module_& m);    // bindings_io.cpp

template <typename T>
static T* P(uintptr_t p) { return reinterpret_cast<T*>(p); }
static hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

static void check_last(const char* what) { check_hip(hipGetLastError(), what); }

static LeNetBuffers buffers_from(const py::dict& d) {
  auto get = [&](const char* k) -> uintptr_t { return d.contains(k) ? d[k].cast<uintptr_t>() : 0; };
  LeNetBuffers b;
  b.train_images = P<const uint8_t>(get("train_images"));
  b.train_labels = P<const int>(get("train_labels"));
  b.n_train = d.contains("n_train") ? d["n_train"].cast<int>() : 0;
  b.params = P<float>(get("params"));
  b.mom = P<float>(get("mom"));
  b.pk = P<bf16>(get("pk"));
  b.act2 = P<bf16>(get("act2"));
  b.act2_rows = d.contains("act2_rows") ? d["act2_rows"].cast<int>() : 0;
  b.act2T = P<bf16>(get("act2T"));
  b.h1 = P<bf16>(get("h1"));
  b.dact2 = P<float>(get("dact2"));
  b.dZ1T = P<bf16>(get("dZ1T"));
  b.conv_slab = P<float>(get("conv_slab"));
  b.eval_part = P<float>(get("eval_part"));
  b.eval_part_floats = d.contains("eval_part_floats") ? d["eval_part_floats"].cast<long>() : 0;
  b.train_stats = P<lenet::Stats>(get("train_stats"));
  b.eval_stats = P<lenet::Stats>(get("eval_stats"));
  b.round_ctr = P<int>(get("round_ctr"));
  b.xprep = P<bf16>(get("xprep"));
  return b;
}

static void fedmi_bind(py::module_& m) {
  fedmi_bind_cnn(m);
  fedmi_bind_comm(m);
  fedmi_bind_zoo(m);
  fedmi_bind_io(m);
  m.def("stamps_enabled", &stamps_enabled);
  m.def("set_ks1_diag", &set_ks1_diag);
  m.def("read_stamps", [](bool clear) {
    const size_t n = (size_t)FEDMI_STAMP_KERNELS * FEDMI_STAMP_WGS * FEDMI_STAMP_SLOTS;
    std::vector<unsigned long long> buf(n, 0ull);
    read_stamps(buf.data(), clear);
    return py::bytes(reinterpret_cast<const char*>(buf.data()), n * sizeof(unsigned long long));
  }, py::arg("clear") = true);
  m.attr("STAMP_SHAPE") = py::make_tuple(FEDMI_STAMP_KERNELS, FEDMI_STAMP_WGS, FEDMI_STAMP_SLOTS);
  m.doc() = "fedmi native runtime: fused LeNet HIP kernels, graph executor, flat-buffer and compression kernels (gfx950)";

  m.def("lenet_layout", []() {
    using namespace lenet;
    py::dict d;
    d["P_C1W"] = P_C1W; d["P_C1B"] = P_C1B; d["P_C2W"] = P_C2W; d["P_C2B"] = P_C2B;
    d["P_F1W"] = P_F1W; d["P_F1B"] = P_F1B; d["P_F2W"] = P_F2W; d["P_F2B"] = P_F2B;
    d["P_F3W"] = P_F3W; d["P_F3B"] = P_F3B; d["P_TOTAL"] = P_TOTAL;
    d["CS"] = CS; d["FS"] = FS; d["F1W_N"] = F1W_N; d["DZ1_LD"] = DZ1_LD; d["PK_TOTAL"] = PK_TOTAL; d["F0"] = F0; d["F0P"] = F0P; d["NP1"] = NP1;
    d["MAX_TRAIN_BATCH"] = MAX_TRAIN_BATCH; d["FC_SPW"] = FC_SPW;
    d["IMG_BYTES"] = IMG_BYTES; d["STATS_BYTES"] = (int)sizeof(Stats);
    d["PK_W1C"] = PK_W1C; d["PK_W2C"] = PK_W2C; d["PK_W2DG"] = PK_W2DG; d["PK_FC1"] = PK_FC1;
    d["PK_FC2"] = PK_FC2; d["PK_FC2T"] = PK_FC2T; d["PK_FC3"] = PK_FC3;
    d["XP_H"] = XP_H; d["XP_W"] = XP_W; d["XP_C"] = XP_C; d["XP_ELEMS"] = XP_ELEMS;
    return d;
  });

  py::class_<SgdConfig>(m, "SgdConfig")
      .def(py::init<>())
      .def_readwrite("lr", &SgdConfig::lr)
      .def_readwrite("momentum", &SgdConfig::momentum)
      .def_readwrite("weight_decay", &SgdConfig::weight_decay);

  py::class_<LeNetEngine>(m, "LeNetEngine")
      .def(py::init([](const py::dict& bufs, float lr, float momentum, float wd, uint32_t seed, bool augment) {
             SgdConfig c;
             c.lr = lr; c.momentum = momentum; c.weight_decay = wd;
             return new LeNetEngine(buffers_from(bufs), c, seed, augment);
           }),
           py::arg("buffers"), py::arg("lr"), py::arg("momentum"), py::arg("weight_decay"), py::arg("seed"),
           py::arg("augment"))
      .def("set_schedule", &LeNetEngine::set_schedule)
      .def("schedule_len", &LeNetEngine::schedule_len)
      .def("step", [](LeNetEngine& e, uintptr_t st, int start, int nb, bool bump, bool reset) {
             e.step(S(st), start, nb, bump, reset);
           }, py::arg("stream"), py::arg("start"), py::arg("nb"), py::arg("bump_round") = false,
           py::arg("reset_stats") = false,
           py::call_guard<py::gil_scoped_release>())
      .def("run_epoch", [](LeNetEngine& e, uintptr_t st, bool use_graph) { e.run_epoch(S(st), use_graph); },
           py::call_guard<py::gil_scoped_release>())
      .def("eval", [](LeNetEngine& e, uintptr_t st, uintptr_t images, uintptr_t labels, int n) {
             e.eval(S(st), P<const uint8_t>(images), P<const int>(labels), n);
           }, py::arg("st"), py::arg("images"), py::arg("labels"), py::arg("n"), py::call_guard<py::gil_scoped_release>())
      .def("pack", [](LeNetEngine& e, uintptr_t st) { e.pack(S(st)); }, py::call_guard<py::gil_scoped_release>())
      .def("set_sgd", [](LeNetEngine& e, float lr, float m, float wd) {
             SgdConfig c; c.lr = lr; c.momentum = m; c.weight_decay = wd; e.set_sgd(c);
           })
      .def("graph_ready", &LeNetEngine::graph_ready);

  // ---- raw LeNet kernels (numerics tests drive them one by one) -------------
  m.def("lenet_conv_fwd", [](uintptr_t st, uintptr_t images, int base, int nb, uintptr_t pk, uintptr_t params,
                             uint32_t seed, uintptr_t round_ctr, int augment, uintptr_t act2, uintptr_t act2T,
                             int tstride, uintptr_t pool1, uintptr_t am1, uintptr_t am2, uintptr_t zero_stats) {
    launch_lenet_conv_fwd(S(st), P<const uint8_t>(images), base, nb, P<const bf16>(pk), P<const float>(params), seed,
                          P<const int>(round_ctr), augment, P<bf16>(act2), P<bf16>(act2T), tstride, P<bf16>(pool1),
                          P<uint8_t>(am1), P<uint8_t>(am2), P<lenet::Stats>(zero_stats));
    check_last("lenet_conv_fwd");
  });
  m.def("lenet_prep_batch", [](uintptr_t st, uintptr_t images, int base, int nb, uint32_t seed, uintptr_t round_ctr,
                               int augment, uintptr_t xprep) {
    launch_lenet_prep_batch(S(st), P<const uint8_t>(images), base, nb, seed, P<const int>(round_ctr), augment,
                            P<bf16>(xprep));
    check_last("lenet_prep_batch");
  });
  m.def("lenet_pack", [](uintptr_t st, uintptr_t params, uintptr_t pk) {
    launch_lenet_pack(S(st), P<const float>(params), P<bf16>(pk));
    check_last("lenet_pack");
  });
  // KS1's cross-lane helpers (kernels/xlane.h) next to the shuffle formulations they replaced, one wave per row
  // of 64 floats: out is [rows][XLANE_PROBE_HELPERS][2 = helper, reference][64] floats, labels [rows] int32
  m.attr("XLANE_PROBE_HELPERS") = xlane_probe_helpers();
  m.def("lenet_xlane_probe", [](uintptr_t st, uintptr_t in, uintptr_t labels, int rows, uintptr_t out) {
    launch_lenet_xlane_probe(S(st), P<const float>(in), P<const int>(labels), rows, P<float>(out));
    check_last("lenet_xlane_probe");
  }, py::arg("stream"), py::arg("inp"), py::arg("labels"), py::arg("rows"), py::arg("out"));

  // ---- flat-buffer ops --------------------------------------------------------
  m.def("sgd_flat", [](uintptr_t st, uintptr_t p, uintptr_t g, uintptr_t buf, long n, float lr, float mo, float wd,
                       float damp, bool nesterov, bool first) {
    launch_sgd_flat(S(st), P<float>(p), P<const float>(g), P<float>(buf), n, lr, mo, wd, damp, nesterov ? 1 : 0,
                    first ? 1 : 0);
    check_last("sgd_flat");
  });
  // server-side optimizer step on the aggregated state (kind: 0 fedavgm, 1 fedadagrad, 2 fedyogi, 3 fedadam);
  // v may be 0 for fedavgm
  m.def("server_opt", [](uintptr_t st, uintptr_t x, uintptr_t anchor, uintptr_t mom, uintptr_t v, long n, long n_opt,
                         int kind, float lr, float beta1, float beta2, float tau) {
    if (kind < 0 || kind > 3) throw std::invalid_argument("server_opt: kind must be 0..3");
    if (n < 0 || n_opt < 0 || n_opt > n) throw std::invalid_argument("server_opt: need 0 <= n_opt <= n");
    if (n == 0) return;
    if (!x || !anchor || !mom || (kind != 0 && !v)) throw std::invalid_argument("server_opt: null buffer");
    if ((x | anchor | mom | v) % 16) throw std::invalid_argument("server_opt: buffers must be 16-byte aligned");
    launch_server_opt(S(st), P<float>(x), P<float>(anchor), P<float>(mom), P<float>(v), n, n_opt, kind, lr, beta1,
                      beta2, tau);
    check_last("server_opt");
  }, py::arg("stream"), py::arg("x"), py::arg("anchor"), py::arg("m"), py::arg("v"), py::arg("n"), py::arg("n_opt"),
     py::arg("kind"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("tau"));

  // differentially private FedAvg on the client's update x - anchor over the k trainable entries of the n-entry
  // float state: dp_sumsq, dp_finish and the clip (+ noise when z > 0) apply, stream-ordered with no host sync.
  // partial: dp_partials(k) doubles of scratch; stats: {sumsq, norm, scale} as three doubles.  sigma =
  // (float)(z * clip / sqrt(world)).  stages selects the launches (1 | 2 | 4; the round runs all three).
  m.def("dp_partials", [](long k) {
    if (k < 0) throw std::invalid_argument("dp_partials: need k >= 0");
    return dp_partials(k);
  });
  m.def("dp_privatize", [](uintptr_t st, uintptr_t x, uintptr_t anchor, long n, long k, uintptr_t partial,
                           uintptr_t stats, double clip, double z, int world, uint64_t key, uint64_t draw, int stages) {
    if (n < 0 || k < 0 || k > n) throw std::invalid_argument("dp_privatize: need 0 <= k <= n");
    if (!(clip > 0.0) || !std::isfinite(clip)) throw std::invalid_argument("dp_privatize: need a finite clip norm S > 0");
    if (!(z >= 0.0) || !std::isfinite(z)) throw std::invalid_argument("dp_privatize: need a finite noise multiplier z >= 0");
    if (world < 1) throw std::invalid_argument("dp_privatize: need world >= 1");
    if (stages < 1 || stages > 7) throw std::invalid_argument("dp_privatize: stages must be in 1..7");
    if (k == 0) return;
    if (!x || !anchor || !partial || !stats) throw std::invalid_argument("dp_privatize: null buffer");
    if ((x | anchor) % 16) throw std::invalid_argument("dp_privatize: x and anchor must be 16-byte aligned");
    if ((partial | stats) % 8) throw std::invalid_argument("dp_privatize: partial and stats must be 8-byte aligned");
    const float sigma = (float)(z * clip / std::sqrt((double)world));
    launch_dp(S(st), P<float>(x), P<const float>(anchor), k, P<double>(partial), P<double>(stats), clip, sigma, key,
              draw, stages);
    check_last("dp_privatize");
  }, py::arg("stream"), py::arg("x"), py::arg("anchor"), py::arg("n"), py::arg("k"), py::arg("partial"),
     py::arg("stats"), py::arg("clip"), py::arg("z"), py::arg("world"), py::arg("key"), py::arg("draw"),
     py::arg("stages") = 7);

  // Byzantine-robust aggregation (csrc/kernels/robust.hip): out[i] = the coordinate-wise trimmed mean (b_eff entries
  // cut on either side; the median at b_eff = (W - 1) / 2) of rows[0][i] .. rows[W-1][i], rows ld floats apart;
  // stats[r], r < W = the number of coordinates at which rank r was cut.  partial: robust_partials(n) x 16 int64.
  m.def("robust_partials", [](long n) {
    if (n < 0) throw std::invalid_argument("robust_partials: need n >= 0");
    return robust_partials(n);
  });
  // the contract the gathered-rows kernels share: W rows of ld floats, n used; `last` is the 8-byte-aligned buffer after
  // partial (stats or history)
  auto rows_check = [](const char* who, uintptr_t rows, long ld, int W, long n, uintptr_t out, uintptr_t partial,
                       uintptr_t last) {
    const std::string p = std::string(who) + ": ";
    if (W < 2 || W > 16) throw std::invalid_argument(p + "W must be in 2..16");
    if (n < 0) throw std::invalid_argument(p + "need n >= 0");
    if (ld < n || ld % 4) throw std::invalid_argument(p + "the row stride ld must be >= n and a multiple of 4");
    if (!rows || !out || !partial || !last) throw std::invalid_argument(p + "null buffer");
    if ((rows | out) % 16) throw std::invalid_argument(p + "rows and out must be 16-byte aligned");
    if ((partial | last) % 8) throw std::invalid_argument(p + "partial and stats / history must be 8-byte aligned");
    const uintptr_t row_bytes = ((uintptr_t)(W - 1) * (uintptr_t)ld + (uintptr_t)n) * 4, out_bytes = (uintptr_t)n * 4;
    if (out < rows + row_bytes && rows < out + out_bytes) throw std::invalid_argument(p + "out must not alias rows");
  };
  m.def("robust_reduce", [rows_check](uintptr_t st, uintptr_t rows, long ld, int W, long n, int b_eff, uintptr_t out,
                                      uintptr_t partial, uintptr_t stats) {
    rows_check("robust_reduce", rows, ld, W, n, out, partial, stats);
    if (b_eff < 0 || b_eff > (W - 1) / 2) throw std::invalid_argument("robust_reduce: need 0 <= b_eff <= (W - 1) / 2");
    if (n == 0) return;
    launch_robust_reduce(S(st), P<const float>(rows), ld, W, n, b_eff, P<float>(out), P<long long>(partial),
                         P<long long>(stats));
    check_last("robust_reduce");
  }, py::arg("stream"), py::arg("rows"), py::arg("ld"), py::arg("W"), py::arg("n"), py::arg("b_eff"), py::arg("out"),
     py::arg("partial"), py::arg("stats"));

  // geometric-median aggregation (csrc/kernels/geomed.hip): out = the smoothed-Weiszfeld iterate after `iters`
  // weighted passes over rows[0] .. rows[W-1] (ld floats apart), started from the mean of the finite entries.
  // partial: geomed_partials(n) x 16 doubles of scratch; history: (iters + 1) x 3 x 16 doubles, row t = {sumsq, dist,
  // w} of every rank after pass t (row iters - 1's w formed out, row iters' dist measures it).
  m.def("geomed_partials", [](long n) {
    if (n < 0) throw std::invalid_argument("geomed_partials: need n >= 0");
    return geomed_partials(n);
  });
  auto geomed_check = [rows_check](const char* who, uintptr_t rows, long ld, int W, long n, double nu, uintptr_t out,
                                   uintptr_t partial, uintptr_t history) {
    rows_check(who, rows, ld, W, n, out, partial, history);
    if (!(nu > 0.0) || !std::isfinite(nu)) throw std::invalid_argument(std::string(who) + ": need a finite nu > 0");
  };
  m.def("geomed", [geomed_check](uintptr_t st, uintptr_t rows, long ld, int W, long n, int iters, double nu,
                                 uintptr_t out, uintptr_t partial, uintptr_t history) {
    geomed_check("geomed", rows, ld, W, n, nu, out, partial, history);
    if (iters < 1 || iters > 64) throw std::invalid_argument("geomed: iters must be in 1..64");
    if (n == 0) return;
    launch_geomed(S(st), P<const float>(rows), ld, W, n, iters, nu, P<float>(out), P<double>(partial),
                  P<double>(history));
    check_last("geomed");
  }, py::arg("stream"), py::arg("rows"), py::arg("ld"), py::arg("W"), py::arg("n"), py::arg("iters"), py::arg("nu"),
     py::arg("out"), py::arg("partial"), py::arg("history"));
  // one pass and its finish from caller-supplied fp32 weights (first: pass 0, the weights are not read and may be
  // null); history_row: 3 x 16 doubles.  geomed is a loop over the same launcher.
  m.def("geomed_pass", [geomed_check](uintptr_t st, uintptr_t rows, long ld, int W, long n, bool first,
                                      uintptr_t weights, uintptr_t out, uintptr_t partial, uintptr_t history_row,
                                      double nu) {
    geomed_check("geomed_pass", rows, ld, W, n, nu, out, partial, history_row);
    if (!first && (!weights || weights % 4))
      throw std::invalid_argument("geomed_pass: a weighted pass needs W fp32 weights, 4-byte aligned");
    if (n == 0) return;
    launch_geomed_pass(S(st), P<const float>(rows), ld, W, n, first, P<const float>(weights), nullptr, nu,
                       P<float>(out), P<double>(partial), P<double>(history_row), 0);
    check_last("geomed_pass");
  }, py::arg("stream"), py::arg("rows"), py::arg("ld"), py::arg("W"), py::arg("n"), py::arg("first"),
     py::arg("weights"), py::arg("out"), py::arg("partial"), py::arg("history_row"), py::arg("nu") = 1e-6);

  // Krum / multi-Krum aggregation (csrc/kernels/krum.hip): out = the client of lowest score (multi: the mean of the
  // W - F_eff lowest), a client's score being the sum of its k smallest squared distances to the others, F_eff =
  // max(0, min(byz, (W - 3) / 2)), k = max(1, W - F_eff - 2).  partial: krum_partials(n) x 256 doubles of scratch;
  // stats: 18 x 16 doubles = score, selected (1.0 / 0.0) and the 16 x 16 squared distances.
  m.def("krum_partials", [](long n) {
    if (n < 0) throw std::invalid_argument("krum_partials: need n >= 0");
    return krum_partials(n);
  });
  m.def("krum", [rows_check](uintptr_t st, uintptr_t rows, long ld, int W, long n, int byz, bool multi, uintptr_t out,
                             uintptr_t partial, uintptr_t stats) {
    rows_check("krum", rows, ld, W, n, out, partial, stats);
    if (byz < 0) throw std::invalid_argument("krum: need byz >= 0");
    if (n == 0) return;
    launch_krum(S(st), P<const float>(rows), ld, W, n, byz, multi, P<float>(out), P<double>(partial), P<double>(stats));
    check_last("krum");
  }, py::arg("stream"), py::arg("rows"), py::arg("ld"), py::arg("W"), py::arg("n"), py::arg("byz"), py::arg("multi"),
     py::arg("out"), py::arg("partial"), py::arg("stats"));
  // the Gram pass and its fold alone: gram = G = X X^T as 16 x 16 doubles, 0 outside W x W (nothing else is written)
  m.def("krum_gram", [rows_check](uintptr_t st, uintptr_t rows, long ld, int W, long n, uintptr_t partial,
                                  uintptr_t gram) {
    rows_check("krum_gram", rows, ld, W, n, gram, partial, gram);
    if (n == 0) return;
    launch_krum_gram(S(st), P<const float>(rows), ld, W, n, P<double>(partial), P<double>(gram));
    check_last("krum_gram");
  }, py::arg("stream"), py::arg("rows"), py::arg("ld"), py::arg("W"), py::arg("n"), py::arg("partial"),
     py::arg("gram"));

  // Bulyan aggregation (csrc/kernels/bulyan.hip): Krum, iterated over the one Gram matrix, selects theta = W - 2 F_eff
  // clients, F_eff = max(0, min(byz, (W - 3) / 4)); out = per coordinate the mean of the theta - 2 F_eff of their values
  // closest to the median.  partial: bulyan_partials(n) x 256 doubles of scratch; stats: 19 x 16 doubles = the score
  // when picked, the round picked (0: never), the 16 x 16 squared distances and the per-client cut counts.
  m.def("bulyan_partials", [](long n) {
    if (n < 0) throw std::invalid_argument("bulyan_partials: need n >= 0");
    return bulyan_partials(n);
  });
  m.def("bulyan", [rows_check](uintptr_t st, uintptr_t rows, long ld, int W, long n, int byz, uintptr_t out,
                               uintptr_t partial, uintptr_t stats) {
    rows_check("bulyan", rows, ld, W, n, out, partial, stats);
    if (byz < 0) throw std::invalid_argument("bulyan: need byz >= 0");
    if (n == 0) return;
    launch_bulyan(S(st), P<const float>(rows), ld, W, n, byz, P<float>(out), P<double>(partial), P<double>(stats));
    check_last("bulyan");
  }, py::arg("stream"), py::arg("rows"), py::arg("ld"), py::arg("W"), py::arg("n"), py::arg("byz"), py::arg("out"),
     py::arg("partial"), py::arg("stats"));
  // the fold and its cut counts alone over the rows named by `record` (the selected ranks, ascending), dropping c values
  // per coordinate: out and stats row 18 (nothing else of stats is written)
  m.def("bulyan_fold", [rows_check](uintptr_t st, uintptr_t rows, long ld, int W, long n, const std::vector<int>& record,
                                    int c, uintptr_t out, uintptr_t partial, uintptr_t stats) {
    rows_check("bulyan_fold", rows, ld, W, n, out, partial, stats);
    const int theta = (int)record.size();
    if (theta < 2 || theta > W) throw std::invalid_argument("bulyan_fold: the record must name 2..W clients");
    for (int s = 0; s < theta; ++s)
      if (record[s] < 0 || record[s] >= W || (s > 0 && record[s] <= record[s - 1]))
        throw std::invalid_argument("bulyan_fold: the record must hold ascending ranks below W");
    if (c < 0 || c > 6 || c % 2 || c >= theta)
      throw std::invalid_argument("bulyan_fold: c must be 0, 2, 4 or 6 and leave one value");
    if (n == 0) return;
    launch_bulyan_fold(S(st), P<const float>(rows), ld, W, n, record.data(), theta, c, P<float>(out),
                       P<double>(partial), P<double>(stats));
    check_last("bulyan_fold");
  }, py::arg("stream"), py::arg("rows"), py::arg("ld"), py::arg("W"), py::arg("n"), py::arg("record"), py::arg("c"),
     py::arg("out"), py::arg("partial"), py::arg("stats"));

  // Divide-and-Conquer aggregation (csrc/kernels/dnc.hip): every client is scored by its squared projection on the top
  // principal direction of the centred rows, read off the centred fp64 Gram matrix; out = the fp32 mean of the W - F_eff
  // clients of lowest score, F_eff = max(0, min(byz, (W - 1) / 2)).  partial: dnc_partials(n) x 256 doubles of scratch;
  // stats: 18 x 16 doubles = score, selected (1.0 / 0.0) and the 16 x 16 double-centred Gram.
  m.def("dnc_partials", [](long n) {
    if (n < 0) throw std::invalid_argument("dnc_partials: need n >= 0");
    return dnc_partials(n);
  });
  m.def("dnc", [rows_check](uintptr_t st, uintptr_t rows, long ld, int W, long n, int byz, uintptr_t out,
                            uintptr_t partial, uintptr_t stats) {
    rows_check("dnc", rows, ld, W, n, out, partial, stats);
    if (byz < 0) throw std::invalid_argument("dnc: need byz >= 0");
    if (n == 0) return;
    launch_dnc(S(st), P<const float>(rows), ld, W, n, byz, P<float>(out), P<double>(partial), P<double>(stats));
    check_last("dnc");
  }, py::arg("stream"), py::arg("rows"), py::arg("ld"), py::arg("W"), py::arg("n"), py::arg("byz"), py::arg("out"),
     py::arg("partial"), py::arg("stats"));
  // the centred Gram pass and its fold alone: gram = G = Y Y^T, y = x - the column pivot, as 16 x 16 doubles, 0 outside
  // W x W (nothing else is written)
  m.def("dnc_gram", [rows_check](uintptr_t st, uintptr_t rows, long ld, int W, long n, uintptr_t partial,
                                 uintptr_t gram) {
    rows_check("dnc_gram", rows, ld, W, n, gram, partial, gram);
    if (n == 0) return;
    launch_dnc_gram(S(st), P<const float>(rows), ld, W, n, P<double>(partial), P<double>(gram));
    check_last("dnc_gram");
  }, py::arg("stream"), py::arg("rows"), py::arg("ld"), py::arg("W"), py::arg("n"), py::arg("partial"),
     py::arg("gram"));

  // secure aggregation by pairwise masking (csrc/kernels/secagg.hip).  secagg_mask: u[i] = the fixed-point word of
  // x[i] - anchor[i] at frac_bits fraction bits plus the ChaCha20 masks of the W - 1 pairs of `rank` (keys: W x 8
  // uint32, row `rank` unused; nonce = draw), stats[0] = the number of clamped or NaN entries.  partial:
  // secagg_partials(n) x 16 int64.  secagg_unmask: out[i] = anchor[i] + (float)(sum_r rows[r][i] * 2^-frac_bits / W),
  // the sum over the W gathered payload rows mod 2^32, read as int32.
  m.def("secagg_partials", [](long n) {
    if (n < 0) throw std::invalid_argument("secagg_partials: need n >= 0");
    return secagg_partials(n);
  });
  auto secagg_check = [](const char* who, int W, long n, int frac_bits) {
    const std::string p = std::string(who) + ": ";
    if (W < 2 || W > 16) throw std::invalid_argument(p + "W must be in 2..16");
    if (n < 0) throw std::invalid_argument(p + "need n >= 0");
    if (frac_bits < 19 || frac_bits > 35) throw std::invalid_argument(p + "frac_bits must be in 19..35 (27 - log2 R)");
  };
  m.def("secagg_mask", [secagg_check](uintptr_t st, uintptr_t x, uintptr_t anchor, uintptr_t keys, int W, int rank,
                                      uint64_t draw, long n, int frac_bits, uintptr_t u, uintptr_t partial,
                                      uintptr_t stats) {
    secagg_check("secagg_mask", W, n, frac_bits);
    if (rank < 0 || rank >= W) throw std::invalid_argument("secagg_mask: need 0 <= rank < W");
    if (n == 0) return;
    if (!x || !anchor || !keys || !u || !partial || !stats) throw std::invalid_argument("secagg_mask: null buffer");
    if ((x | anchor | u) % 16) throw std::invalid_argument("secagg_mask: x, anchor and u must be 16-byte aligned");
    if (keys % 4 || (partial | stats) % 8)
      throw std::invalid_argument("secagg_mask: keys must be 4-byte, partial and stats 8-byte aligned");
    const uintptr_t bytes = (uintptr_t)n * 4;
    if ((u < x + bytes && x < u + bytes) || (u < anchor + bytes && anchor < u + bytes))
      throw std::invalid_argument("secagg_mask: u must not alias x or anchor");
    launch_secagg_mask(S(st), P<const float>(x), P<const float>(anchor), P<const uint32_t>(keys), W, rank, draw, n,
                       frac_bits, P<uint32_t>(u), P<long long>(partial), P<long long>(stats));
    check_last("secagg_mask");
  }, py::arg("stream"), py::arg("x"), py::arg("anchor"), py::arg("keys"), py::arg("W"), py::arg("rank"),
     py::arg("draw"), py::arg("n"), py::arg("frac_bits"), py::arg("u"), py::arg("partial"), py::arg("stats"));
  m.def("secagg_unmask", [secagg_check](uintptr_t st, uintptr_t rows, long ld, int W, uintptr_t anchor, long n,
                                        int frac_bits, uintptr_t out) {
    secagg_check("secagg_unmask", W, n, frac_bits);
    if (ld < n || ld % 4) throw std::invalid_argument("secagg_unmask: the row stride ld must be >= n and a multiple of 4");
    if (n == 0) return;
    if (!rows || !anchor || !out) throw std::invalid_argument("secagg_unmask: null buffer");
    if ((rows | anchor | out) % 16)
      throw std::invalid_argument("secagg_unmask: rows, anchor and out must be 16-byte aligned");
    const uintptr_t row_bytes = ((uintptr_t)(W - 1) * (uintptr_t)ld + (uintptr_t)n) * 4, bytes = (uintptr_t)n * 4;
    if ((out < rows + row_bytes && rows < out + bytes) || (out < anchor + bytes && anchor < out + bytes))
      throw std::invalid_argument("secagg_unmask: out must not alias rows or anchor");
    launch_secagg_unmask(S(st), P<const float>(rows), ld, W, P<const float>(anchor), n, frac_bits, P<float>(out));
    check_last("secagg_unmask");
  }, py::arg("stream"), py::arg("rows"), py::arg("ld"), py::arg("W"), py::arg("anchor"), py::arg("n"),
     py::arg("frac_bits"), py::arg("out"));

  // client-side drift correction of the flat gradient, between the backward pass and the SGD tail (kind: 0
  // fedprox -- g, p, anchor, mu; 1 scaffold -- g, corr, acc); the other kind's buffers may be 0
  m.def("drift_grad", [](uintptr_t st, int kind, uintptr_t g, uintptr_t p, uintptr_t anchor, uintptr_t corr,
                         uintptr_t acc, float mu, long n) {
    if (kind < 0 || kind > 1) throw std::invalid_argument("drift_grad: kind must be 0 (fedprox) or 1 (scaffold)");
    if (n < 0) throw std::invalid_argument("drift_grad: need n >= 0");
    if (n == 0) return;
    if (!g || (kind == 0 ? (!p || !anchor) : (!corr || !acc))) throw std::invalid_argument("drift_grad: null buffer");
    if ((g | p | anchor | corr | acc) % 16) throw std::invalid_argument("drift_grad: buffers must be 16-byte aligned");
    launch_drift_grad(S(st), kind, P<float>(g), P<const float>(p), P<const float>(anchor), P<const float>(corr),
                      P<float>(acc), mu, n);
    check_last("drift_grad");
  }, py::arg("stream"), py::arg("kind"), py::arg("g"), py::arg("p"), py::arg("anchor"), py::arg("corr"),
     py::arg("acc"), py::arg("mu"), py::arg("n"));
  m.def("scaffold_finish", [](uintptr_t st, uintptr_t acc, uintptr_t ci, uintptr_t delta, long K, long n) {
    if (K < 1) throw std::invalid_argument("scaffold_finish: need K >= 1 (no SGD step was counted this round)");
    if (n < 0) throw std::invalid_argument("scaffold_finish: need n >= 0");
    if (n == 0) return;
    if (!acc || !ci || !delta) throw std::invalid_argument("scaffold_finish: null buffer");
    if ((acc | ci | delta) % 16) throw std::invalid_argument("scaffold_finish: buffers must be 16-byte aligned");
    launch_scaffold_finish(S(st), P<const float>(acc), P<float>(ci), P<float>(delta), K, n);
    check_last("scaffold_finish");
  }, py::arg("stream"), py::arg("acc"), py::arg("ci"), py::arg("delta"), py::arg("K"), py::arg("n"));
  m.def("scaffold_begin", [](uintptr_t st, uintptr_t c, uintptr_t dmean, uintptr_t ci, uintptr_t corr, uintptr_t acc,
                             long n) {
    if (n < 0) throw std::invalid_argument("scaffold_begin: need n >= 0");
    if (n == 0) return;
    if (!c || !dmean || !ci || !corr || !acc) throw std::invalid_argument("scaffold_begin: null buffer");
    if ((c | dmean | ci | corr | acc) % 16) throw std::invalid_argument("scaffold_begin: buffers must be 16-byte aligned");
    launch_scaffold_begin(S(st), P<float>(c), P<const float>(dmean), P<const float>(ci), P<float>(corr),
                          P<float>(acc), n);
    check_last("scaffold_begin");
  }, py::arg("stream"), py::arg("c"), py::arg("dmean"), py::arg("ci"), py::arg("corr"), py::arg("acc"), py::arg("n"));

  // ---- compression ---------------------------------------------------------------
  m.def("topk_state_bytes", &topk_state_bytes);
  m.def("topk_overflow_offset", &topk_overflow_offset);
  m.def("topk_ef", [](uintptr_t st, uintptr_t x, uintptr_t g, uintptr_t residual, long n, int k, uintptr_t state,
                      uintptr_t cidx, uintptr_t ckey, uintptr_t idx, uintptr_t val) {
    if (k <= 0 || k > n) throw std::invalid_argument("topk_ef: need 0 < k <= n");
    if (n >= (1L << 30)) throw std::invalid_argument("topk_ef: n must be < 2^30 (int32 indices, 2n scratch)");
    if (!x || !g || !residual || !state || !cidx || !ckey || !idx || !val) throw std::invalid_argument("topk_ef: null buffer");
    launch_topk_ef(S(st), P<const float>(x), P<const float>(g), P<float>(residual), n, k, P<void>(state), P<int>(cidx),
                   P<unsigned>(ckey), P<int>(idx), P<float>(val));
    check_last("topk_ef");
  }, py::arg("stream"), py::arg("x"), py::arg("g"), py::arg("residual"), py::arg("n"), py::arg("k"), py::arg("state"),
     py::arg("cidx"), py::arg("ckey"), py::arg("idx"), py::arg("val"));
  // the four below: n (m) < 0, R <= 0 or a null required buffer is an error; n == 0 (m == 0) returns without a launch
  m.def("ef_delta", [](uintptr_t st, uintptr_t local, uintptr_t global, uintptr_t residual, uintptr_t d, long n) {
    if (n < 0) throw std::invalid_argument("ef_delta: need n >= 0");
    if (n == 0) return;
    if (!local || !global || !d) throw std::invalid_argument("ef_delta: null buffer (only residual may be 0)");
    launch_ef_delta(S(st), P<const float>(local), P<const float>(global), P<const float>(residual), P<float>(d), n);
    check_last("ef_delta");
  });
  m.def("scatter_add_ranked", [](uintptr_t st, uintptr_t out, uintptr_t idx, uintptr_t val, int R, long m_, float scale,
                                 long n) {
    if (R <= 0) throw std::invalid_argument("scatter_add_ranked: R must be > 0");
    if (m_ < 0 || n < 0) throw std::invalid_argument("scatter_add_ranked: need m >= 0 and n >= 0");
    if (m_ == 0 || n == 0) return;
    if (!out || !idx || !val) throw std::invalid_argument("scatter_add_ranked: null buffer");
    launch_scatter_add_ranked(S(st), P<float>(out), P<const int>(idx), P<const float>(val), R, m_, scale, n);
    check_last("scatter_add_ranked");
  });
  m.def("quant_int8", [](uintptr_t st, uintptr_t d, long n, uintptr_t q, uintptr_t scales, uintptr_t residual) {
    if (n < 0) throw std::invalid_argument("quant_int8: need n >= 0");
    if (n == 0) return;
    if (!d || !q || !scales) throw std::invalid_argument("quant_int8: null buffer (only residual may be 0)");
    launch_quant_int8(S(st), P<const float>(d), n, P<signed char>(q), P<float>(scales), P<float>(residual));
    check_last("quant_int8");
  });
  m.def("dequant_accum", [](uintptr_t st, uintptr_t q, uintptr_t scales, int R, long n, uintptr_t out, float scale) {
    if (R <= 0) throw std::invalid_argument("dequant_accum: R must be > 0");
    if (n < 0) throw std::invalid_argument("dequant_accum: need n >= 0");
    if (n == 0) return;
    if (!q || !scales || !out) throw std::invalid_argument("dequant_accum: null buffer");
    launch_dequant_accum(S(st), P<const signed char>(q), P<const float>(scales), R, n, P<float>(out), scale);
    check_last("dequant_accum");
  });

  // PowerSGD (csrc/kernels/powersgd.hip).  segs / tiles / folds are the device tables fedmi.parallel.compress.psgd_tables
  // builds and checks against the buffers' sizes (the kernels trust them); a launch covers every segment.  part: the
  // pass's partial buffer (may be 0 when nfolds == 0: no matrix was split).
  m.def("psgd_geometry", []() {
    int geo[11];
    psgd_geometry(geo);
    py::dict d;
    const char* names[11] = {"threads", "max_rank", "slab", "tile_rows", "back_rows", "back_cols", "dense", "fold",
                             "seg_bytes", "tile_bytes", "fold_bytes"};
    for (int i = 0; i < 11; ++i) d[names[i]] = geo[i];
    return d;
  });
  auto psgd_check = [](const char* who, int R, int ntiles, int nfolds, uintptr_t part, uintptr_t folds) {
    if (R < 1 || R > 8) throw std::invalid_argument(std::string(who) + ": need 1 <= R <= 8");
    if (ntiles < 0 || nfolds < 0) throw std::invalid_argument(std::string(who) + ": need ntiles >= 0 and nfolds >= 0");
    if (nfolds > 0 && (!part || !folds)) throw std::invalid_argument(std::string(who) + ": folds need their table and the partial buffer");
  };
  m.def("psgd_qinit", [](uintptr_t st, uintptr_t q, long n, uint64_t key) {
    if (n < 0) throw std::invalid_argument("psgd_qinit: need n >= 0");
    if (n == 0) return;
    if (!q || q % 16) throw std::invalid_argument("psgd_qinit: q must be a 16-byte aligned buffer");
    launch_psgd_qinit(S(st), P<float>(q), n, key);
    check_last("psgd_qinit");
  }, py::arg("stream"), py::arg("q"), py::arg("n"), py::arg("key"));
  m.def("psgd_project", [psgd_check](uintptr_t st, uintptr_t x, uintptr_t g, uintptr_t residual, uintptr_t segs,
                                     uintptr_t tiles, int ntiles, uintptr_t q, int R, uintptr_t send, uintptr_t part,
                                     uintptr_t folds, int nfolds) {
    psgd_check("psgd_project", R, ntiles, nfolds, part, folds);
    if (ntiles == 0) return;
    if (!x || !g || !residual || !segs || !tiles || !q || !send) throw std::invalid_argument("psgd_project: null buffer");
    if ((x | g | residual) % 16) throw std::invalid_argument("psgd_project: x, g and residual must be 16-byte aligned");
    launch_psgd_project(S(st), P<const float>(x), P<const float>(g), P<float>(residual), P<const void>(segs),
                        P<const void>(tiles), ntiles, P<const float>(q), R, P<float>(send), P<float>(part),
                        P<const void>(folds), nfolds);
    check_last("psgd_project");
  }, py::arg("stream"), py::arg("x"), py::arg("g"), py::arg("residual"), py::arg("segs"), py::arg("tiles"),
     py::arg("ntiles"), py::arg("q"), py::arg("R"), py::arg("send"), py::arg("part"), py::arg("folds"), py::arg("nfolds"));
  m.def("psgd_orth", [](uintptr_t st, uintptr_t segs, int nseg, uintptr_t p, int R) {
    if (R < 1 || R > 8) throw std::invalid_argument("psgd_orth: need 1 <= R <= 8");
    if (nseg < 0) throw std::invalid_argument("psgd_orth: need nseg >= 0");
    if (nseg == 0) return;
    if (!segs || !p) throw std::invalid_argument("psgd_orth: null buffer");
    launch_psgd_orth(S(st), P<const void>(segs), nseg, P<float>(p), R);
    check_last("psgd_orth");
  }, py::arg("stream"), py::arg("segs"), py::arg("nseg"), py::arg("p"), py::arg("R"));
  m.def("psgd_backproject", [psgd_check](uintptr_t st, uintptr_t d, uintptr_t segs, uintptr_t tiles, int ntiles,
                                         uintptr_t p, int R, uintptr_t q, uintptr_t part, uintptr_t folds, int nfolds) {
    psgd_check("psgd_backproject", R, ntiles, nfolds, part, folds);
    if (ntiles == 0) return;
    if (!d || !segs || !tiles || !p || !q) throw std::invalid_argument("psgd_backproject: null buffer");
    launch_psgd_backproject(S(st), P<const float>(d), P<const void>(segs), P<const void>(tiles), ntiles,
                            P<const float>(p), R, P<float>(q), P<float>(part), P<const void>(folds), nfolds);
    check_last("psgd_backproject");
  }, py::arg("stream"), py::arg("d"), py::arg("segs"), py::arg("tiles"), py::arg("ntiles"), py::arg("p"), py::arg("R"),
     py::arg("q"), py::arg("part"), py::arg("folds"), py::arg("nfolds"));
  m.def("psgd_apply", [psgd_check](uintptr_t st, uintptr_t x, uintptr_t g, uintptr_t residual, uintptr_t segs,
                                   uintptr_t tiles, int ntiles, uintptr_t p, uintptr_t q, uintptr_t send, int R) {
    psgd_check("psgd_apply", R, ntiles, 0, 0, 0);
    if (ntiles == 0) return;
    if (!x || !g || !residual || !segs || !tiles || !p || !q || !send) throw std::invalid_argument("psgd_apply: null buffer");
    if ((x | g | residual) % 16) throw std::invalid_argument("psgd_apply: x, g and residual must be 16-byte aligned");
    launch_psgd_apply(S(st), P<float>(x), P<float>(g), P<float>(residual), P<const void>(segs), P<const void>(tiles),
                      ntiles, P<const float>(p), P<const float>(q), P<const float>(send), R);
    check_last("psgd_apply");
  }, py::arg("stream"), py::arg("x"), py::arg("g"), py::arg("residual"), py::arg("segs"), py::arg("tiles"),
     py::arg("ntiles"), py::arg("p"), py::arg("q"), py::arg("send"), py::arg("R"));
}

// the module name carries the build variant (fedmi/_build.py VARIANTS): -DFEDMI_MODULE=_fedmi_native_<v>
#ifndef FEDMI_MODULE
#define FEDMI_MODULE _fedmi_native
#endif
PYBIND11_MODULE(FEDMI_MODULE, m) { fedmi_bind(m); }
