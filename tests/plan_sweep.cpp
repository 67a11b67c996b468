// Sweeps the host conv planner (csrc/kernels/conv_plan.h, plain C++) over a grid of shapes, CU counts and workspace
// caps and checks the invariants the launchers and kernels rely on.  Built by tests/test_conv_dispatch.py with
// -fsanitize=address,undefined: a stand-alone host program, nothing of it runs on a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kernels/conv_plan.h"

using namespace fedmi;

static long g_checks = 0;
static ConvShape g_s;
static int g_cus;
static long g_cap;

#define CHECK(c)                                                                                                   \
  do {                                                                                                             \
    ++g_checks;                                                                                                    \
    if (!(c)) {                                                                                                    \
      std::printf("FAILED %s (line %d): N%d H%d W%d C%d O%d R%d st%d pad%d cus %d cap %ld\n", #c, __LINE__, g_s.N,  \
                  g_s.H, g_s.W, g_s.C, g_s.O, g_s.R, g_s.st, g_s.pad, g_cus, g_cap);                               \
      std::exit(1);                                                                                                \
    }                                                                                                              \
  } while (0)

// splits * kps >= ksteps > (splits - 1) * kps: every split owns a step, the splits cover K
static void check_split(int ksteps, int kps, int splits) {
  CHECK(kps >= 1 && splits >= 1);
  if (ksteps == 0) { CHECK(splits == 1); return; }
  CHECK((long)splits * kps >= ksteps && ksteps > (long)(splits - 1) * kps);
}

static void check_fd(const FdPlan& p, long cap) {
  long need = 0;
  if (p.route == ROUTE_TAP_PHASES) {
    const TapMulti& tm = p.tm;
    CHECK(tm.n >= 2 && tm.n <= MAX_TAP_PHASES && tm.tile0[0] == 0);
    int maxsp = 1;
    long end = 0;   // the split phases' slices follow one another: disjoint, inside ws_need
    for (int k = 0; k < tm.n; ++k) {
      check_split(tm.g[k].K / 64, tm.kps[k], tm.splits[k]);
      const long tiles = (long)((tm.g[k].M + 127) / 128) * ((tm.g[k].O + p.bn - 1) / p.bn);
      CHECK(tm.tile0[k + 1] == tm.tile0[k] + tiles && tiles > 0);
      maxsp = tm.splits[k] > maxsp ? tm.splits[k] : maxsp;
      if (tm.splits[k] > 1) {
        CHECK(tm.g[k].O <= SPLITK_MAX_NC);   // the combine's one-row-per-block layout
        CHECK(tm.wsoff[k] == end);
        end += (long)tm.splits[k] * tm.g[k].M * tm.g[k].O;
      } else {
        CHECK(tm.wsoff[k] == -1);
      }
    }
    CHECK(p.maxsp == maxsp);   // grid.z
    CHECK(end == p.ws_need);
    need = end;
  } else if (p.route != ROUTE_STEM) {
    CHECK(p.n >= 1 && p.n <= MAX_TAP_PHASES);
    for (int i = 0; i < p.n; ++i) {
      const Gemm& l = p.g[i];
      const bool tap = p.route != ROUTE_GENERIC;
      check_split(tap ? (l.tg.K + 63) / 64 : (l.cg.K + BK - 1) / BK, l.kps, l.splits);
      CHECK(l.tiles == (unsigned)((long)((l.M + l.tile.BM - 1) / l.tile.BM) * ((l.NC + l.tile.BN - 1) / l.tile.BN)));
      if (l.splits > 1) {
        CHECK(l.NC <= SPLITK_MAX_NC && l.NC % 8 == 0);   // the combine's one-row-per-block layout
        const Combine c = combine_geom(l.M, l.NC, true);
        CHECK(c.tb > 0 && c.tb <= 256 && c.tb % (l.NC / 8) == 0 && (long)c.nblk * c.rows_per_block >= l.M);
      }
      need = gemm_ws(l) > need ? gemm_ws(l) : need;
    }
    CHECK(need == p.ws_need);
  }
  if (need > 0) CHECK(need <= cap);   // a planned split fits the workspace
}

static bool same_fd(const FdPlan& a, const FdPlan& b) {
  if (a.route != b.route || a.n != b.n || a.ws_need != b.ws_need || a.bn != b.bn || a.maxsp != b.maxsp) return false;
  for (int i = 0; i < a.n; ++i)
    if (a.g[i].kps != b.g[i].kps || a.g[i].splits != b.g[i].splits || a.g[i].tiles != b.g[i].tiles ||
        a.g[i].tile.BM != b.g[i].tile.BM || a.g[i].tile.BN != b.g[i].tile.BN)
      return false;
  for (int k = 0; k < a.tm.n; ++k)
    if (a.tm.kps[k] != b.tm.kps[k] || a.tm.splits[k] != b.tm.splits[k] || a.tm.wsoff[k] != b.tm.wsoff[k] ||
        a.tm.tile0[k + 1] != b.tm.tile0[k + 1])
      return false;
  return a.tm.n == b.tm.n;
}

static void check_wgrad(const WgradPlan& p, long cap) {
  const bool halo = p.route != ROUTE_GENERIC;
  check_split(halo ? p.h.M / 128 : (p.cg.K + BK - 1) / BK, p.kps, p.splits);
  CHECK(p.ws_need == (long)p.splits * p.plane);
  if (cap >= p.plane) CHECK(p.ws_need <= cap);
  if (halo) CHECK(p.h.M % 128 == 0 && p.h.NPR <= 208 && p.tiles == (unsigned)((p.h.O / 64) * (p.h.C / 64)));
}

// the phases' weight-image blocks tile [0, O * R * S * C) without overlap, and every tap belongs to one phase
static void check_phases(const ConvShape& s) {
  Phase ph[MAX_TAP_PHASES];
  const int np = dgrad_phases(s.R, s.S, s.st, s.pad, ph);
  CHECK(np == (s.st == 1 ? 1 : 4));
  long taps = 0;
  int hit[7][7] = {};
  for (int i = 0; i < np; ++i) {
    CHECK(ph[i].tap0 == taps && ph[i].nr >= 0 && ph[i].ns >= 0);
    taps += (long)ph[i].nr * ph[i].ns;
    for (int a = 0; a < ph[i].nr; ++a)
      for (int b = 0; b < ph[i].ns; ++b) {
        const int r = ph[i].r0 + s.st * a, c = ph[i].s0 + s.st * b;
        CHECK(r < s.R && c < s.S);
        ++hit[r][c];
      }
  }
  CHECK(taps * s.C * s.O == (long)s.O * s.R * s.S * s.C);
  for (int r = 0; r < s.R; ++r)
    for (int c = 0; c < s.S; ++c) CHECK(hit[r][c] == 1);
}

int main() {
  const int Ns[] = {1, 2, 3, 16, 128}, HWs[] = {1, 2, 4, 7, 9, 32}, Cs[] = {8, 16, 24, 48, 64, 160, 512, 2048, 2056};
  const int Rs[] = {1, 3, 5, 7}, cus_list[] = {256, 1};
  long shapes = 0;
  for (int N : Ns) for (int H : HWs) for (int W : HWs) for (int C : Cs) for (int O : Cs) for (int R : Rs)
    for (int st = 1; st <= 2; ++st)
      for (int pad = 0; pad <= R / 2; pad += R / 2 ? R / 2 : 1) {
        if (H + 2 * pad < R || W + 2 * pad < R) continue;
        ConvShape s{N, H, W, C, C, O, (H + 2 * pad - R) / st + 1, (W + 2 * pad - R) / st + 1, R, R, st, pad};
        if ((long)N * H * W * C >= (1l << 31) || (long)N * s.P * s.Q * O >= (1l << 31)) continue;
        g_s = s;
        ++shapes;
        g_cus = 0; g_cap = 0;
        check_phases(s);
        for (int cus : cus_list) {
          g_cus = cus;
          const long plane = (long)s.N * s.P * s.Q * s.O, wplane = (long)s.O * s.R * s.S * s.C;
          const FdPlan uf = plan_fwd(s, WS_UNBOUNDED, cus), ud1 = plan_dgrad(s, true, WS_UNBOUNDED, cus),
                       ud0 = plan_dgrad(s, false, WS_UNBOUNDED, cus);
          const WgradPlan uw = plan_wgrad(s, WS_UNBOUNDED, 0, true, cus), uw0 = plan_wgrad(s, WS_UNBOUNDED, 0, false, cus);
          // a plan made at exactly the floats the unbounded plan uses is the unbounded plan
          CHECK(same_fd(plan_fwd(s, uf.ws_need, cus), uf));
          CHECK(same_fd(plan_dgrad(s, true, ud1.ws_need, cus), ud1));
          CHECK(same_fd(plan_dgrad(s, false, ud0.ws_need, cus), ud0));
          const WgradPlan ew = plan_wgrad(s, uw.ws_need, 0, true, cus);
          CHECK(ew.route == uw.route && ew.splits == uw.splits && ew.kps == uw.kps);
          CHECK(ud0.route == ROUTE_GENERIC && !ud0.fusable);
          const long caps[] = {0, plane, uf.ws_need, ud1.ws_need, WS_UNBOUNDED};
          for (long cap : caps) {
            g_cap = cap;
            check_fd(plan_fwd(s, cap, cus), cap);
            check_fd(plan_dgrad(s, true, cap, cus), cap);
            check_fd(plan_dgrad(s, false, cap, cus), cap);
          }
          const long wcaps[] = {wplane, uw.ws_need, uw0.ws_need, WS_UNBOUNDED};
          for (long cap : wcaps) {
            g_cap = cap;
            check_wgrad(plan_wgrad(s, cap, 0, true, cus), cap);
            check_wgrad(plan_wgrad(s, cap, 0, false, cus), cap);
            check_wgrad(plan_wgrad(s, 7 * wplane, 7, true, cus), 7 * wplane);
          }
        }
      }
  std::printf("plan sweep ok: %ld shapes, %ld checks\n", shapes, g_checks);
  return 0;
}
