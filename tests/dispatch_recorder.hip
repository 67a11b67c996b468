// Records every host-side conv routing decision without a GPU (tests/test_conv_dispatch.py).
//
//   dispatch_recorder SHAPES.txt > record.txt
//
// conv_igemm.hip is compiled into this program with hipLaunchKernelGGL replaced by a recorder, so the launchers
// run their real code and no kernel starts.  Per launch: the resolved kernel instantiation, grid, block, dynamic
// LDS bytes, every integer argument, the integer fields of the geometry structs and each pointer as an offset
// from a fake base.  The CU count is pinned to 256 (the MI355X's) whatever device is present.
// SHAPES.txt: one "N H W C O R stride pad" per line; '#' starts a comment.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <map>
#include <sstream>
#include <string>
#include <typeinfo>

static hipError_t rec_device_attr(int* v, hipDeviceAttribute_t, int) {
  *v = 256;
  return hipSuccess;
}
#define hipDeviceGetAttribute rec_device_attr

// The instantiation a launch resolved to, from the mangled name of KName<&kernel<args>> (the kernels are local
// symbols of this program; integer and bool template arguments are all they take): "conv_tap<64, 8, false>".
template <auto K>
struct KName {
  static std::string get() {
    const std::string m = typeid(KName).name();   // 5KNameIXadL_ZN12_GLOBAL__N_18conv_tapILi64ELi8ELb0EEEv...
    size_t p = m.find("_GLOBAL__N_1");
    if (p == std::string::npos) return m;
    p += 12;
    size_t len = 0;
    while (std::isdigit((unsigned char)m[p])) len = len * 10 + (m[p++] - '0');
    std::string s = m.substr(p, len);
    p += len;
    if (m[p] != 'I') return s;
    s += '<';
    for (++p; m[p] == 'L'; ++p) {   // L <type> <value> E
      const char ty = m[p + 1];
      const size_t e = m.find('E', p);
      std::string v = m.substr(p + 2, e - p - 2);
      if (ty == 'b') v = v == "0" ? "false" : "true";
      if (s.back() != '<') s += ", ";
      s += v;
      p = e;
    }
    return s + '>';
  }
};

template <class... A>
static void rec_launch(const std::string& name, dim3 grid, dim3 block, size_t lds, hipStream_t, const A&... a);

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, l, s, ...) rec_launch(KName<(k)>::get(), g, b, l, s, __VA_ARGS__)

#include "kernels/conv_igemm.hip"

namespace fedmi {
void launch_dw_wgrad_reduce(hipStream_t, const WredItem&) {}   // dwconv.hip; no depthwise item is recorded
}

static std::ostringstream g_out;

// pointers: fake bases 1 << 44 apart, printed as p<base>+<byte offset>
static void rec(const void* p) {
  const unsigned long v = (unsigned long)p;
  if (!v) g_out << " 0";
  else g_out << " p" << (v >> 44) << "+" << (v & ((1ul << 44) - 1));
}
template <class T>
static void rec(T* p) { rec((const void*)p); }
static void rec(int v) { g_out << ' ' << v; }
static void rec(long v) { g_out << ' ' << v; }
static void rec(float v) { g_out << ' ' << v; }
static void rec(const FastDiv& f) { g_out << " /" << f.d; }   // (m, s follow from d: make_div)
// the shape being recorded: geometry fields that repeat it print as "="
static int g_shape[11];   // N H W C O P Q R S st pad
static void rec_shape_part(std::initializer_list<int> v, std::initializer_list<int> pads) {
  bool same = std::equal(v.begin(), v.end(), g_shape);
  for (int p : pads) same = same && p == g_shape[10];
  if (same) { g_out << " ="; return; }
  for (int x : v) rec(x);
  for (int x : pads) rec(x);
}
static void rec(const ConvGeom& g) {
  g_out << " CG[";
  rec_shape_part({g.N, g.H, g.W, g.C, g.O, g.P, g.Q, g.R, g.S, g.st}, {g.pad});
  for (int v : {g.M, g.NC, g.K, g.Cw, g.ph, g.pw, g.r0, g.s0, g.nr, g.ns, g.Hp, g.Wp}) rec(v);
  rec(g.dNS); rec(g.dWp); rec(g.dHWp);
  g_out << " ]";
}
static void rec(const RowMap& r) {
  if (!r.on) { g_out << " RM0"; return; }
  g_out << " RM[";
  for (int v : {r.on, r.P, r.Q, r.OH, r.OW, r.st, r.ph, r.pw}) rec(v);
  g_out << " ]";
}
static void rec(const TapGeom& g) {
  g_out << " TG[";
  rec_shape_part({g.N, g.H, g.W, g.C, g.O, g.P, g.Q, g.R, g.S, g.st}, {g.pad_h, g.pad_w});
  rec(g.M); rec(g.K);
  g_out << " ]";
}
static void rec(const TapMulti& t) {
  g_out << " TM[ n=" << t.n;
  for (int k = 0; k < t.n; ++k) {
    g_out << " {";
    rec(t.g[k]); rec(t.rm[k]); rec(t.woff[k]); rec(t.wsoff[k]); rec(t.kps[k]); rec(t.splits[k]); rec(t.tile0[k]);
    g_out << " }";
  }
  rec(t.tile0[t.n]);
  g_out << " ]";
}
static void rec(const HaloGeom& h) {
  g_out << " HG[";
  for (int v : {h.N, h.H, h.W, h.C, h.O, h.M, h.K, h.TH, h.IMGS, h.PW, h.NPR, h.nchunks}) rec(v);
  g_out << " ]";
}
static void rec(const StemGeom& s) {
  g_out << " SG[";
  for (int v : {s.N, s.H, s.W, s.O, s.M}) rec(v);
  g_out << " ]";
}
static void rec(const fedmi::BnSums& b) {
  if (!b.rep) { g_out << " BS0"; return; }
  g_out << " BS[";
  rec(b.rep); rec(b.z); rec(b.y); rec(b.mean); rec(b.inv); rec(b.reps); rec(b.zb); rec(b.meanb); rec(b.invb);
  rec(b.msc); rec(b.msc_ld);
  g_out << " ]";
}
static void rec(const DPackTable& t) {
  g_out << " DP[ n=" << t.n << " cb=" << t.cb;
  for (int k = 0; k < t.n; ++k) {
    const DPackEntry& e = t.e[k];
    g_out << " {";
    rec(e.w); rec(e.wd);
    for (int v : {e.O, e.Cw, e.Cpad, e.R, e.S, e.r0, e.s0, e.nr, e.ns, e.step, e.blk0}) rec(v);
    g_out << " }";
  }
  g_out << " ]";
}
static void rec(const WredTable& t) { g_out << " WT[ n=" << t.n << " ]"; }   // (multi-item tables are not recorded)
static void rec(const PackTable& t) { g_out << " PT[ n=" << t.n << " ]"; }

template <class... A>
static void rec_launch(const std::string& name, dim3 grid, dim3 block, size_t lds, hipStream_t, const A&... a) {
  g_out << "  " << name << " g=" << grid.x << ',' << grid.y << ',' << grid.z << " b=" << block.x << " lds=" << lds
        << " |";
  (rec(a), ...);
  g_out << '\n';
}

// ---- the record of one shape -------------------------------------------------------------------------------------
template <class T>
static T* base(int k) { return reinterpret_cast<T*>((unsigned long)k << 44); }

static std::map<std::string, std::string> g_seen;   // launches text -> first label with it (per shape)

template <class F>
static void variant(const std::string& label, F&& f) {
  g_out.str("");
  try {
    f();
  } catch (const std::exception& e) {
    g_out << "  throw: " << e.what() << '\n';
  }
  const std::string text = g_out.str();
  const auto it = g_seen.find(text);
  if (it != g_seen.end()) {
    std::printf(" %s == %s\n", label.c_str(), it->second.c_str());
    return;
  }
  g_seen.emplace(text, label);
  std::printf(" %s\n%s", label.c_str(), text.c_str());
}

static void record(int N, int H, int W, int C, int O, int R, int st, int pad) {
  using namespace fedmi;
  ConvShape s{};
  s.N = N; s.H = H; s.W = W; s.C = C; s.Cw = C == 8 ? 3 : C; s.O = O; s.R = R; s.S = R; s.st = st; s.pad = pad;
  s.P = (H + 2 * pad - R) / st + 1; s.Q = (W + 2 * pad - R) / st + 1;
  std::printf("shape %d %d %d %d %d %d %d %d\n", N, H, W, C, O, R, st, pad);
  const int sh[11] = {N, H, W, C, O, s.P, s.Q, R, R, st, pad};
  std::copy(sh, sh + 11, g_shape);
  g_seen.clear();
  long fd = 0, wg = 0;
  try {
    fd = conv_fd_ws_floats(s);
    wg = conv_wgrad_ws_floats(s);
    std::printf(" ws fd=%ld wgrad=%ld fusable=%d,%d\n", fd, wg, conv_dgrad_fusable(s, 0), conv_dgrad_fusable(s, 1));
  } catch (const std::exception& e) {
    std::printf(" ws throw: %s\n", e.what());
    return;
  }
  const bf16 *x = base<const bf16>(1), *w = base<const bf16>(2), *dy = base<const bf16>(8), *wd = base<const bf16>(9);
  bf16 *y = base<bf16>(3), *dx = base<bf16>(10);
  double* stats = base<double>(4);
  const float* shift = base<const float>(5);
  float *ws = base<float>(6), *dw = base<float>(12);
  const long big = 4 * std::max(fd, 1l << 20) + 12345;
  hipStream_t q = nullptr;

  variant("fwd.nows", [&] { launch_conv_fwd(q, s, x, w, y, stats, shift, nullptr, 0, nullptr); });
  variant("fwd.exact", [&] { launch_conv_fwd(q, s, x, w, y, stats, shift, ws, fd, nullptr); });
  variant("fwd.big", [&] { launch_conv_fwd(q, s, x, w, y, stats, shift, ws, big, nullptr); });
  variant("fwd.big.nostats", [&] { launch_conv_fwd(q, s, x, w, y, nullptr, nullptr, ws, big, nullptr); });
  for (int has_wd = 0; has_wd < 2; ++has_wd)
    for (int acc = 0; acc < 2; ++acc)
      variant("dgrad.wd" + std::to_string(has_wd) + ".acc" + std::to_string(acc), [&] {
        launch_conv_dgrad(q, s, dy, w, dx, ws, big, has_wd ? wd : nullptr, acc, nullptr, nullptr);
      });
  variant("dgrad.wd1.exact", [&] { launch_conv_dgrad(q, s, dy, w, dx, ws, fd, wd, 0, nullptr, nullptr); });
  variant("dgrad.wd1.nows", [&] { launch_conv_dgrad(q, s, dy, w, dx, nullptr, 0, wd, 0, nullptr, nullptr); });
  variant("dgrad.wd0.exact", [&] { launch_conv_dgrad(q, s, dy, w, dx, ws, fd, nullptr, 0, nullptr, nullptr); });
  variant("dgrad.wd1.add.bs", [&] {
    BnSums bs{};
    bs.rep = base<double>(13); bs.z = base<const bf16>(14); bs.y = base<const bf16>(15);
    bs.mean = base<const float>(16); bs.inv = base<const float>(17); bs.reps = 4;
    launch_conv_dgrad(q, s, dy, w, dx, ws, big, wd, 0, base<const bf16>(11), &bs);
  });
  const long plane = (long)O * R * R * C;
  for (int a1 = 0; a1 < 2; ++a1) {
    const std::string t = "wgrad.auto.1x1_" + std::to_string(a1);
    variant(t + ".exact", [&] { launch_conv_wgrad(q, s, x, dy, dw, ws, wg, 0, 0, 0, 1, nullptr, a1); });
    variant(t + ".plane", [&] { launch_conv_wgrad(q, s, x, dy, dw, ws, plane, 0, 0, 0, 1, nullptr, a1); });
  }
  variant("wgrad.splits1", [&] { launch_conv_wgrad(q, s, x, dy, dw, ws, 7 * plane, 1, 0, 0, 1, nullptr, 1); });
  variant("wgrad.splits7", [&] { launch_conv_wgrad(q, s, x, dy, dw, ws, 7 * plane, 7, 1, 0, 1, nullptr, 1); });
  variant("dgrad_pack", [&] {
    const DPackItem it{base<const float>(18), base<bf16>(9), O, s.Cw, C, R, R, st, pad};
    launch_dgrad_pack_multi(q, &it, 1);
  });
  variant("sgd_pack", [&] {
    const SgdPackConv c{64, base<bf16>(2), base<bf16>(9), O, s.Cw, C, R, R, st, pad};
    const long segs[2] = {0, 64};
    const SgdPackPlan p = build_sgd_pack_plan(&c, 1, segs, 1);
    g_out << "  plan n=" << p.n_entries << " blocks=" << p.n_blocks << " lds=" << p.lds_bytes << '\n';
    const SgdPackEntry* e = reinterpret_cast<const SgdPackEntry*>(p.table.data());
    for (int k = 0; k < p.n_entries; ++k) {
      g_out << "  entry";
      rec(e[k].off); rec(e[k].wr);
      for (int v : {e[k].kind, e[k].O, e[k].Cw, e[k].C, e[k].R, e[k].S, e[k].cb, e[k].nph, e[k].step, e[k].blk0}) rec(v);
      for (int i = 0; i < e[k].nph; ++i) {
        g_out << " {";
        rec(e[k].wd[i]); rec(e[k].r0[i]); rec(e[k].s0[i]); rec(e[k].nr[i]); rec(e[k].ns[i]);
        g_out << " }";
      }
      g_out << '\n';
    }
  });
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char line[256];
  while (std::fgets(line, sizeof line, f)) {
    int v[8];
    if (line[0] == '#' || std::sscanf(line, "%d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7) != 8)
      continue;
    record(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
  }
  std::fclose(f);
  return 0;
}
