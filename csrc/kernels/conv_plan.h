// fedmi — host planning of the convolution launches (conv_igemm.hip): the ONLY place a routing decision is made.
//
// plan_fwd / plan_dgrad / plan_wgrad turn a ConvShape, a workspace capacity and the CU count into everything a
// launch needs: the route, the tile, the grid, K steps per split, the split count, the workspace offsets and the
// floats the plan uses.  The launchers issue exactly what a plan says, and the workspace queries
// (conv_fd_ws_floats / conv_wgrad_ws_floats) and conv_dgrad_fusable read the same plans with an unbounded
// capacity -- so a workspace sized by the one can never disagree with the split counts of the other.  Every sum
// downstream is fixed-order: a changed split count changes results bitwise (tests/test_conv_dispatch.py pins the
// plans of every zoo shape).
//
// Plain C++17, no HIP runtime: the CU count is an argument.
#pragma once
#include <algorithm>
#include <stdexcept>

#include "conv_geom.h"

namespace fedmi {
namespace {

enum Route { ROUTE_STEM, ROUTE_TAP, ROUTE_TAP_GEN, ROUTE_TAP_PHASES, ROUTE_GENERIC, ROUTE_HALO, ROUTE_HALO_1X1 };

constexpr long WS_UNBOUNDED = 1l << 40;   // "as much workspace as the plan wants"

inline RowMap make_rowmap(int P, int Q, int OH, int OW, int st, int ph, int pw) {
  RowMap r{};
  r.on = 1;
  r.P = P; r.Q = Q; r.OH = OH; r.OW = OW; r.st = st; r.ph = ph; r.pw = pw;
  r.dPQ = make_div(P * Q); r.dQ = make_div(Q);
  return r;
}

inline ConvGeom make_geom(const ConvShape& s) {
  ConvGeom g{};
  g.N = s.N; g.H = s.H; g.W = s.W; g.C = s.C; g.O = s.O; g.P = s.P; g.Q = s.Q;
  g.R = s.R; g.S = s.S; g.st = s.st; g.pad = s.pad; g.Cw = s.Cw;
  g.dC = make_div(s.C); g.dO = make_div(s.O); g.dS = make_div(s.S); g.dQ = make_div(s.Q);
  g.dPQ = make_div(s.P * s.Q); g.dW = make_div(s.W); g.dHW = make_div(s.H * s.W);
  g.ph = g.pw = 0; g.r0 = g.s0 = 0; g.nr = s.R; g.ns = s.S; g.Hp = s.H; g.Wp = s.W;
  g.dNS = make_div(s.S); g.dWp = make_div(s.W); g.dHWp = make_div(s.H * s.W);
  return g;
}

inline TapGeom make_tap(int N, int H, int W, int C, int O, int P, int Q, int R, int S, int st, int pad_h, int pad_w) {
  TapGeom g{};
  g.N = N; g.H = H; g.W = W; g.C = C; g.O = O; g.P = P; g.Q = Q;
  g.R = R; g.S = S; g.st = st; g.pad_h = pad_h; g.pad_w = pad_w;
  g.M = N * P * Q; g.K = R * S * C;
  g.dPQ = make_div(P * Q); g.dQ = make_div(Q);
  return g;
}

inline void check_shape(const ConvShape& s) {
  if (s.C % 8 || s.O % 8 || s.C < s.Cw || s.st < 1 || s.st > 2 || s.R < 1 || s.S < 1)
    throw std::invalid_argument("conv_igemm: need C % 8 == 0, O % 8 == 0, stride 1|2");
  if (s.P != (s.H + 2 * s.pad - s.R) / s.st + 1 || s.Q != (s.W + 2 * s.pad - s.S) / s.st + 1)
    throw std::invalid_argument("conv_igemm: inconsistent output size");
  if ((long)s.N * s.H * s.W * s.C >= (1l << 31) || (long)s.N * s.P * s.Q * s.O >= (1l << 31))
    throw std::invalid_argument("conv_igemm: tensor too large for 32-bit index math");
}

// ---- split-K ----------------------------------------------------------------------------------------------------
// `want` splits over `ksteps` K steps -> K steps per split and the splits that own at least one step.
struct SplitK {
  int kps, splits;
};
inline SplitK split_k(int ksteps, long want) {
  const int sp = (int)std::max<long>(1, std::min<long>(want, ksteps));
  SplitK k;
  k.kps = std::max(1, (ksteps + sp - 1) / sp);
  k.splits = std::max(1, (ksteps + k.kps - 1) / k.kps);
  return k;
}

// Launch geometry of the split-K combine (conv_splitk_reduce): each lane owns one 8-channel vector of a row.
// Plain combine: ~4 blocks per CU; with BN statistics / BN-backward sums fewer blocks (their per-channel atomics
// contend on 2 x NC addresses).
struct Combine {
  int tb, rows_per_block, nblk;
};
inline Combine combine_geom(int M, int NC, bool sums) {
  const int VR = NC / 8;
  Combine c;
  c.tb = (256 / VR) * VR;
  const int rstep = c.tb / VR;
  c.rows_per_block = sums ? std::max(2 * rstep, (M + 255) / 256) : std::max(rstep, (M + 1023) / 1024);
  c.nblk = (M + c.rows_per_block - 1) / c.rows_per_block;
  return c;
}

// ---- tiles and split choosers (formulas, thresholds and measurements as they were tuned) ------------------------
struct TileCfg {
  int BM, BN;
};

inline TileCfg pick_tiles(int M, int NC, int cus) {
  const int BN = NC <= 64 ? 64 : 128;
  const long t128 = (long)((M + 127) / 128) * ((NC + BN - 1) / BN);
  return TileCfg{(M > 64 && t128 >= cus) ? 128 : 64, BN};
}

// WGRAD always splits K, so the tile count never has to fill the chip: take the 128 x 128 tile
// (twice the MFMA work per loaded byte) for O >= 256 -- measured 44 -> 38 us (256x256 3x3) and
// 51 -> 47 us (512x512) at batch 128, but slower at O = 128.
inline TileCfg pick_tiles_wgrad(int M, int NC, int cus) {
  TileCfg t = pick_tiles(M, NC, cus);
  if (M >= 256 && NC > 64) t.BM = 128;
  return t;
}

// FWD / DGRAD split-K: GEMMs with fewer output tiles than CUs and a long K loop
// (ResNet layer3/4 at batch 128: 128-256 tiles, 36-72 K steps) leave most of
// the chip idle behind a serial K chain.  Split K so that ~3 workgroups per CU
// run >= 8 K steps each, partials into ``ws``; 1 = no split.
// The split-K combine (conv_splitk_reduce) gives each lane one 8-channel vector of a row and needs a
// whole row in one 256-lane block: rows wider than 2048 channels never split.
constexpr int SPLITK_MAX_NC = 2048;

inline int fd_splits(const ConvGeom& g, long ws_floats, int cus) {
  if (ws_floats <= 0 || g.NC > SPLITK_MAX_NC) return 1;
  const TileCfg t = pick_tiles(g.M, g.NC, cus);
  const long tiles = (long)((g.M + t.BM - 1) / t.BM) * ((g.NC + t.BN - 1) / t.BN);
  const int ksteps = (g.K + BK - 1) / BK;
  if (tiles >= 2l * cus || ksteps < 16) return 1;
  long sp = std::min<long>((3l * cus + tiles - 1) / tiles, ksteps / 8);
  sp = std::min<long>(sp, ws_floats / ((long)g.M * g.NC));
  if (sp < 2) return 1;
  return split_k(ksteps, sp).splits;
}

// conv_tap tile width: 128 columns (96 KiB of LDS stages, 1 workgroup per CU) while the 128-wide tiles fill the
// chip; 64 (72 KiB, 2 per CU) for O <= 64 and for problems whose 128-wide tiles would leave CUs idle (ResNet-18 l3 /
// l4: 128 / 64 tiles -> 256 / 128; -19 % / -8 % per conv, while l2's 256 tiles stay faster at 128: +7 % at 64,
// profiles/r5_cnn/).  m_tiles: 128-row tiles of the problem.
inline int tap_bn_for(int O, long m_tiles, int cus) {
  if (O <= 64) return 64;
  return m_tiles * ((O + 127) / 128) < cus ? 64 : 128;
}
inline int tap_bn(const TapGeom& g, int cus) { return tap_bn_for(g.O, (g.M + 127) / 128, cus); }

// conv_tap reads its operands through 32-bit buffer offsets (out-of-range lanes read zeros) and keeps a
// per-row tap-validity mask of R * S <= 64 bits
inline bool tap_fits(long in_elems, long w_elems, int R, int S) {
  return in_elems * 2 < (1l << 31) && w_elems * 2 < (1l << 31) && R * S <= 64;
}

// Split K only to fill one wave of workgroups: conv_tap keeps 1 (BN 128, 96 KiB
// LDS) or 2 (BN 64) workgroups per CU, and a split costs an fp32 round trip.
// With 8-wave workgroups a half-filled chip without split-K beats split-K + combine (ResNet-18 l3 forward:
// 24.7 vs 28.8 us, profiles/r5_cnn/): split only when the tiles fill at most a quarter of one wave of
// workgroups.
inline int tap_splits(const TapGeom& g, long ws_floats, int cus) {
  if (ws_floats <= 0 || g.O > SPLITK_MAX_NC) return 1;
  const int bn = tap_bn(g, cus);
  const long tiles = (long)((g.M + 127) / 128) * ((g.O + bn - 1) / bn);
  const long target = (bn == 128 ? 1l : 2l) * cus;
  const int ksteps = (g.K + 63) / 64;
  // (a 40-step threshold saved 2.4 us on ResNet-18's layer-4 stride-2 forward but moved EfficientNetB0's
  // 3-epoch trajectory outside its parity bound -- profiles/r5_cnn/splits/; kept at 16)
  if (4 * tiles > target || ksteps < 16) return 1;
  long sp = std::min<long>((target + tiles / 2) / tiles, ksteps / 8);
  sp = std::min<long>(sp, ws_floats / ((long)g.M * g.O));
  if (sp < 2) return 1;
  return split_k(ksteps, sp).splits;
}

// K-split count for the weight gradient: at most one wave of two workgroups per CU (rounded down: ResNet-18's
// layer-4 3x3 WGRAD, 144 tiles, 48.0 -> 40.5 us with 3 splits instead of 4 -- the fourth made a second, 64-workgroup
// wave; profiles/r5_cnn/experiments/wgrad_splits.jsonl), at least 8 K steps per split, a bounded workspace.
inline int wgrad_splits(const ConvGeom& g, long ws_cap_floats, int cus) {
  const TileCfg t = pick_tiles_wgrad(g.M, g.NC, cus);
  const long tiles = (long)((g.M + t.BM - 1) / t.BM) * ((g.NC + t.BN - 1) / t.BN);
  const int ksteps = (g.K + BK - 1) / BK;
  long sp = std::max<long>(1, 2l * cus / tiles);
  sp = std::min<long>(sp, std::max(1, ksteps / 8));
  if (ws_cap_floats > 0) sp = std::min<long>(sp, ws_cap_floats / ((long)g.M * g.NC));
  sp = std::max<long>(1, sp);
  return split_k(ksteps, sp).splits;
}

// K splits of the halo WGRAD: about one workgroup per CU over the (O / 64) x (C / 64) tiles -- fewer
// splits mean fewer fp32 partial bytes to write and reduce.
inline int wgrad_halo_splits(const HaloGeom& h, long ws_cap_floats, int cus) {
  const long want = cus;
  const long tiles = (long)(h.O / 64) * h.nchunks;
  const int nblk = h.M / 128;
  long sp = std::max<long>(1, (want + tiles / 2) / tiles);
  sp = std::min<long>(sp, nblk);
  if (ws_cap_floats > 0) sp = std::min<long>(sp, ws_cap_floats / ((long)h.O * h.K));   // K = taps * C
  sp = std::max<long>(1, sp);
  return split_k(nblk, sp).splits;
}

// ---- DGRAD sub-pixel phases -------------------------------------------------------------------------------------
// Stride 2 runs as one sub-problem per output parity (ph, pw), each summing only the taps r = r0 + 2i, s = s0 + 2j
// that land on it (nr x ns of them; none for e.g. three parities of a 1x1); stride 1 is the one phase of all taps.
// A function of the filter alone: the DGRAD weight image concatenates the phases' blocks in this order, phase k
// starting tap0 * C * O elements in.  Whether a parity has output rows at all (Hp, Wp > 0) is for the caller that
// has spatial sizes.
struct Phase {
  int ph, pw, r0, s0, nr, ns;
  long tap0;
};
inline int dgrad_phases(int R, int S, int st, int pad, Phase* out) {
  if (st == 1) {
    out[0] = Phase{0, 0, 0, 0, R, S, 0};
    return 1;
  }
  int n = 0;
  long taps = 0;
  for (int ph = 0; ph < 2; ++ph)
    for (int pw = 0; pw < 2; ++pw) {
      const int r0 = (ph + pad) & 1, s0 = (pw + pad) & 1;
      const int nr = std::max(0, (R - r0 + 1) / 2), ns = std::max(0, (S - s0 + 1) / 2);
      out[n++] = Phase{ph, pw, r0, s0, nr, ns, taps};
      taps += (long)nr * ns;
    }
  return n;
}

// ---- FWD / DGRAD plans ------------------------------------------------------------------------------------------
// One kernel launch of the generic (conv_igemm) or tap (conv_tap) path; splits > 1: fp32 partials into the
// workspace, then the combine over M x NC through rm.
struct Gemm {
  ConvGeom cg;       // generic
  TapGeom tg;        // tap
  RowMap rm;         // output row scatter (a stride-2 DGRAD phase), else off
  long woff;         // tap DGRAD: weight-image offset of the phase (elements)
  TileCfg tile;
  unsigned tiles;    // grid.x
  int kps, splits;   // grid.z = splits
  int M, NC;
};

struct FdPlan {
  Route route;
  int n;                       // TAP / TAP_GEN: 1; GENERIC: one per phase, run in order through the same workspace
  Gemm g[MAX_TAP_PHASES];
  TapMulti tm;                 // TAP_PHASES: the one launch; grid = tm.tile0[tm.n] x 1 x maxsp, tile width bn
  int bn, maxsp;
  StemGeom sg;                 // STEM
  unsigned stem_blocks;
  bool fusable;                // DGRAD: the epilogue can take add / BN sums (tap path, no tap-less phase)
  long ws_need;                // floats of workspace the plan uses
};

inline Gemm plan_generic(const ConvGeom& g, const RowMap& rm, long ws_cap, int cus) {
  Gemm l{};
  l.cg = g; l.rm = rm; l.M = g.M; l.NC = g.NC;
  l.tile = pick_tiles(g.M, g.NC, cus);
  l.tiles = (unsigned)((long)((g.M + l.tile.BM - 1) / l.tile.BM) * ((g.NC + l.tile.BN - 1) / l.tile.BN));
  const SplitK k = split_k((g.K + BK - 1) / BK, fd_splits(g, ws_cap, cus));
  l.kps = k.kps; l.splits = k.splits;
  return l;
}

inline Gemm plan_tap(const TapGeom& g, const RowMap& rm, long woff, long ws_cap, int cus) {
  Gemm l{};
  l.tg = g; l.rm = rm; l.woff = woff; l.M = g.M; l.NC = g.O;
  l.tile = TileCfg{128, tap_bn(g, cus)};
  l.tiles = (unsigned)((long)((g.M + 127) / 128) * ((g.O + l.tile.BN - 1) / l.tile.BN));
  const SplitK k = split_k((g.K + 63) / 64, tap_splits(g, ws_cap, cus));
  l.kps = k.kps; l.splits = k.splits;
  return l;
}

inline long gemm_ws(const Gemm& l) { return l.splits > 1 ? (long)l.splits * l.M * l.NC : 0; }

// One-launch plan for the phases of a stride-2 DGRAD: no K split while their tiles fill the
// chip (the phases run side by side instead of one small launch after another); otherwise split the
// phase with the longest per-split K first (>= 8 K steps per split) until about one wave of workgroups,
// within the workspace.  empty[i]: no tap lands on phase i.
inline void plan_tap_phases(FdPlan& pl, const TapGeom* pg, const RowMap* prm, const long* woff, const bool* empty, int n,
                            long ws_cap, int cus) {
  TapMulti& tm = pl.tm;
  long tiles[MAX_TAP_PHASES], total = 0;
  int ks[MAX_TAP_PHASES];
  long m_tiles = 0;
  for (int i = 0; i < n; ++i)
    if (!empty[i]) m_tiles += (pg[i].M + 127) / 128;
  int bn = 64;
  for (int i = 0; i < n; ++i)
    if (!empty[i]) { bn = tap_bn_for(pg[i].O, m_tiles, cus); break; }
  pl.bn = bn;
  // tap-less parities (1x1 stride 2) ride along as K = 0 phases: their tiles only write zeros (or leave an
  // accumulated dX as it is) -- one launch instead of one zero-fill launch per empty parity
  for (int i = 0; i < n; ++i) {
    const int k = tm.n++;
    tiles[k] = (long)((pg[i].M + 127) / 128) * ((pg[i].O + bn - 1) / bn);
    ks[k] = empty[i] ? 0 : pg[i].K / 64;
    tm.splits[k] = 1;
    if (!empty[i]) total += tiles[k];
  }
  // floats a trial uses: of the splits that will own a K step (split_k), as the launch stores them -- so a plan made
  // at exactly the floats the unbounded plan uses is the unbounded plan
  auto need = [&](const int* sp) {
    long w = 0;
    for (int k = 0; k < tm.n; ++k) {
      const int own = split_k(ks[k], sp[k]).splits;
      if (own > 1) w += (long)own * pg[k].M * pg[k].O;
    }
    return w;
  };
  const long target = (bn == 128 ? 1l : 2l) * cus;
  if (4 * total < 3 * target) {
    long wgs = total;
    for (;;) {
      int best = -1;
      double bestv = 0.0;
      for (int k = 0; k < tm.n; ++k) {
        const double v = (double)ks[k] / tm.splits[k];
        if (pg[k].O > SPLITK_MAX_NC) continue;   // (the combine needs a whole row in one block, as in tap_splits)
        if (ks[k] / (tm.splits[k] + 1) >= 8 && v > bestv) { best = k; bestv = v; }
      }
      if (best < 0 || wgs + tiles[best] > target) break;
      int trial[MAX_TAP_PHASES];
      for (int k = 0; k < tm.n; ++k) trial[k] = tm.splits[k] + (k == best ? 1 : 0);
      if (need(trial) > ws_cap) break;
      tm.splits[best] = trial[best];
      wgs += tiles[best];
    }
  }
  long off = 0, t0 = 0;
  pl.maxsp = 1;
  for (int k = 0; k < tm.n; ++k) {
    const SplitK sk = split_k(ks[k], tm.splits[k]);
    tm.kps[k] = sk.kps;
    tm.splits[k] = sk.splits;
    tm.g[k] = pg[k];
    if (empty[k]) tm.g[k].K = 0;
    tm.rm[k] = prm[k];
    tm.woff[k] = woff[k];
    tm.wsoff[k] = tm.splits[k] > 1 ? off : -1;
    if (tm.splits[k] > 1) off += (long)tm.splits[k] * pg[k].M * pg[k].O;
    tm.tile0[k] = (int)t0;
    t0 += tiles[k];
    pl.maxsp = std::max(pl.maxsp, tm.splits[k]);
  }
  tm.tile0[tm.n] = (int)t0;
  pl.ws_need = off;
}

// the forward runs on conv_tap for C % 64 == 0, and (GEN) for any C % 8 == 0 from 16 channels with O % 8 == 0
inline bool fwd_tap_ok(const ConvShape& s) {
  const long K = (long)s.R * s.S * s.C;
  return s.O % 8 == 0 && (s.C % 64 == 0 || (s.C % 8 == 0 && s.C >= 16)) &&
         tap_fits((long)s.N * s.H * s.W * s.C, (long)s.O * K, s.R, s.S);
}

// The generic implicit-GEMM forward: after the tap and stem routes only C = 8 shapes that are not the stem
// pattern run it, but conv_fd_ws_floats counts it for every shape (see there).
inline FdPlan plan_fwd_generic(const ConvShape& s, long ws_cap, int cus) {
  FdPlan p{};
  ConvGeom g = make_geom(s);
  g.M = s.N * s.P * s.Q; g.NC = s.O; g.K = s.R * s.S * s.C;
  p.route = ROUTE_GENERIC;
  p.n = 1;
  p.g[0] = plan_generic(g, RowMap{}, ws_cap, cus);
  p.ws_need = gemm_ws(p.g[0]);
  return p;
}

// Y[N,P,Q,O] = conv(X[N,H,W,C], W_rsc)
inline FdPlan plan_fwd(const ConvShape& s, long ws_cap, int cus) {
  check_shape(s);
  if (fwd_tap_ok(s)) {
    FdPlan p{};
    p.route = s.C % 64 ? ROUTE_TAP_GEN : ROUTE_TAP;   // GEN: several taps per K step
    p.n = 1;
    p.g[0] = plan_tap(make_tap(s.N, s.H, s.W, s.C, s.O, s.P, s.Q, s.R, s.S, s.st, s.pad, s.pad), RowMap{}, 0, ws_cap,
                      cus);
    p.ws_need = gemm_ws(p.g[0]);
    return p;
  }
  if (s.C == 8 && s.R == 3 && s.S == 3 && s.st == 1 && s.pad == 1 && (s.O == 32 || s.O == 64)) {
    // the network-input conv (conv_stem_kernel): ~4 pixel tiles of 16 per wave
    FdPlan p{};
    p.route = ROUTE_STEM;
    p.sg = StemGeom{s.N, s.H, s.W, s.O, s.N * s.H * s.W};
    const long ntiles = (p.sg.M + 15) / 16;
    p.stem_blocks = (unsigned)std::max<long>(1, std::min<long>(2048, (ntiles + 15) / 16));
    return p;
  }
  return plan_fwd_generic(s, ws_cap, cus);
}

// The tap-major DGRAD reads dY as its input operand through the DGRAD weight image: O % 64 == 0 (every stride:
// conv_tap / conv_tap_phases), or stride 1 with O % 8 == 0 from 16 channels: one phase, a plain conv_tap problem
// over dY with O input channels -> conv_tap<GEN> (the GoogLeNet / zoo narrow branches)
inline bool dgrad_tap_ok(const ConvShape& s) {
  const bool gen = s.st == 1 && s.O % 8 == 0 && s.O >= 16;
  return (s.O % 64 == 0 || gen) && tap_fits((long)s.N * s.P * s.Q * s.O, (long)s.C * s.R * s.S * s.O, s.R, s.S);
}

// dX[N,H,W,C] = conv_transpose(dY[N,P,Q,O], W_rsc)   (every element written).
// Stride 2 runs as 4 sub-pixel phases so no MFMA multiplies a structural zero.
// has_wd: the caller holds the conv's DGRAD weight image (without one only the generic route is open).
inline FdPlan plan_dgrad(const ConvShape& s, bool has_wd, long ws_cap, int cus) {
  check_shape(s);
  FdPlan p{};
  Phase ph[MAX_TAP_PHASES];
  const int np = dgrad_phases(s.R, s.S, s.st, s.pad, ph);
  if (has_wd && dgrad_tap_ok(s)) {   // the phases as conv_tap problems over dY
    TapGeom tg[MAX_TAP_PHASES];
    RowMap rm[MAX_TAP_PHASES];
    long woff[MAX_TAP_PHASES];
    bool empty[MAX_TAP_PHASES];
    int n = 0;
    p.fusable = true;
    for (int i = 0; i < np; ++i) {
      const Phase& q = ph[i];
      if (s.st == 1) {
        tg[n] = make_tap(s.N, s.P, s.Q, s.O, s.C, s.H, s.W, s.R, s.S, 1, s.R - 1 - s.pad, s.S - 1 - s.pad);
        rm[n] = RowMap{};
      } else {
        const int Hp = (s.H - q.ph + 1) / 2, Wp = (s.W - q.pw + 1) / 2;
        if (Hp <= 0 || Wp <= 0) continue;
        const int d0 = (q.ph + s.pad - q.r0) / 2, e0 = (q.pw + s.pad - q.s0) / 2;
        tg[n] = make_tap(s.N, s.P, s.Q, s.O, s.C, Hp, Wp, std::max(q.nr, 1), std::max(q.ns, 1), 1, q.nr - 1 - d0,
                         q.ns - 1 - e0);
        rm[n] = make_rowmap(Hp, Wp, s.H, s.W, 2, q.ph, q.pw);
      }
      woff[n] = q.tap0 * s.C * s.O;
      empty[n] = q.nr * q.ns == 0;   // (1x1 stride 2): output rows must be zero
      if (empty[n]) p.fusable = false;
      ++n;
    }
    if (n > 1) {   // stride 2: every parity in one launch (tap-less parities as K = 0 phases that write zeros)
      p.route = ROUTE_TAP_PHASES;
      plan_tap_phases(p, tg, rm, woff, empty, n, ws_cap, cus);
    } else {
      p.route = tg[0].C % 64 ? ROUTE_TAP_GEN : ROUTE_TAP;
      p.n = 1;
      p.g[0] = plan_tap(tg[0], rm[0], woff[0], ws_cap, cus);
      p.ws_need = gemm_ws(p.g[0]);
    }
    return p;
  }
  p.route = ROUTE_GENERIC;
  ConvGeom g = make_geom(s);
  g.NC = s.C;
  for (int i = 0; i < np; ++i) {
    ConvGeom q = g;
    RowMap rm{};
    if (s.st == 1) {
      q.M = s.N * s.H * s.W; q.K = s.R * s.S * s.O;
    } else {
      q.ph = ph[i].ph; q.pw = ph[i].pw; q.r0 = ph[i].r0; q.s0 = ph[i].s0; q.nr = ph[i].nr; q.ns = ph[i].ns;
      q.Hp = (s.H - q.ph + 1) / 2; q.Wp = (s.W - q.pw + 1) / 2;
      if (q.Hp <= 0 || q.Wp <= 0) continue;
      q.dNS = make_div(std::max(q.ns, 1)); q.dWp = make_div(q.Wp); q.dHWp = make_div(q.Hp * q.Wp);
      q.M = s.N * q.Hp * q.Wp; q.K = q.nr * q.ns * s.O;
      rm = make_rowmap(q.Hp, q.Wp, s.H, s.W, s.st, q.ph, q.pw);
    }
    // a phase with no taps (1x1 stride 2, odd parity) never splits: the kernel just writes zeros
    p.g[p.n] = plan_generic(q, rm, q.K == 0 ? 0 : ws_cap, cus);
    p.ws_need = std::max(p.ws_need, gemm_ws(p.g[p.n]));
    ++p.n;
  }
  return p;
}

// ---- WGRAD plan -------------------------------------------------------------------------------------------------
struct WgradPlan {
  Route route;         // GENERIC (split-K conv_igemm), HALO (3x3) or HALO_1X1
  ConvGeom cg;         // generic
  TileCfg tile;
  HaloGeom h;          // halo
  unsigned tiles;      // grid.x
  int kps;             // K steps (generic) / 128-pixel blocks (halo) per split
  int splits;          // grid.z; every split stores one O x RSC plane
  long plane;
  bool reduce_tiled;   // the partial reduction: coalesced (o, channel-block) tiles, else one lane per column
  long ws_need;
};

// conv_wgrad_halo applies to 3x3 / stride 1 / pad 1 with C and O % 64 and 128-pixel blocks; every other
// shape takes the generic WGRAD (split-K conv_igemm).
inline bool wgrad_halo_geom(const ConvShape& s, HaloGeom* h, bool allow_1x1) {
  if (allow_1x1 && s.R == 1 && s.S == 1 && s.st == 1 && s.pad == 0 && s.C % 64 == 0 && s.O % 64 == 0) {
    // 1x1 / stride 1: conv_wgrad_halo<1> over 128-pixel blocks (K = C marks the one-tap form).  Its 64 x 64
    // tiles re-read each operand chunk twice as often as the generic kernel's 128 x 128 ones, which the L2 absorbs
    // only for small problems: 1.3-2x faster at MobileNet's 16x16 / 8x8 pointwise shapes, 7-65 % slower from
    // M * (C + O) ~ 2e7 on (GoogLeNet 32x32 256 -> 128, 16x16 512 -> 192, 8x8 832 -> 256;
    // profiles/r6_cnn/wgrad1x1_halo/)
    const long M = (long)s.N * s.H * s.W;
    if (M % 128 || M >= (1l << 31) || M * (s.C + s.O) > 3l * (1l << 22)) return false;
    HaloGeom x{};
    x.N = s.N; x.H = s.H; x.W = s.W; x.C = s.C; x.O = s.O; x.M = (int)M; x.K = s.C;
    x.NPR = 128; x.nchunks = s.C / 64;
    *h = x;
    return true;
  }
  if (s.R != 3 || s.S != 3 || s.st != 1 || s.pad != 1 || s.C % 64 || s.O % 64) return false;
  const int M = s.N * s.H * s.W, HW = s.H * s.W;
  if (M % 128) return false;
  HaloGeom x{};
  x.N = s.N; x.H = s.H; x.W = s.W; x.C = s.C; x.O = s.O; x.M = M; x.K = 9 * s.C;
  if (HW <= 128) {
    if (128 % HW) return false;
    x.IMGS = 128 / HW; x.TH = s.H;
  } else {
    if (128 % s.W || s.H % (128 / s.W)) return false;
    x.IMGS = 1; x.TH = 128 / s.W;
  }
  x.PW = s.W + 2;
  x.NPR = x.IMGS * (x.TH + 2) * x.PW;
  x.nchunks = s.C / 64;
  // (a 288-row window, 4x4 images, would spill the kernel's per-lane fragment offset tables: generic path)
  if (x.NPR > 208) return false;
  x.dPI = make_div((x.TH + 2) * x.PW); x.dPW = make_div(x.PW); x.dTHW = make_div(x.TH * s.W);
  x.dW = make_div(s.W); x.dHW = make_div(HW);
  *h = x;
  return true;
}

inline ConvGeom wgrad_geom(const ConvShape& s) {
  check_shape(s);
  ConvGeom g = make_geom(s);
  g.M = s.O; g.NC = s.R * s.S * s.C; g.K = s.N * s.P * s.Q;
  return g;
}

inline WgradPlan wgrad_finish(WgradPlan p, const ConvShape& s) {
  p.plane = (long)s.O * s.R * s.S * s.C;
  p.ws_need = (long)p.splits * p.plane;
  // enough (o, channel-block) tiles: coalesced tile writes; else one lane per workspace column
  p.reduce_tiled = (long)s.O * ((s.C + 63) / 64) >= 1024;
  return p;
}

// The generic split-K WGRAD; splits <= 0 picks automatically within ws_cap floats (<= 0: unbounded).
inline WgradPlan plan_wgrad_generic(const ConvShape& s, long ws_cap, int splits, int cus) {
  WgradPlan p{};
  p.route = ROUTE_GENERIC;
  p.cg = wgrad_geom(s);
  p.tile = pick_tiles_wgrad(p.cg.M, p.cg.NC, cus);
  p.tiles = (unsigned)((long)((p.cg.M + p.tile.BM - 1) / p.tile.BM) * ((p.cg.NC + p.tile.BN - 1) / p.tile.BN));
  const SplitK k = split_k((p.cg.K + BK - 1) / BK, splits > 0 ? splits : wgrad_splits(p.cg, ws_cap, cus));
  p.kps = k.kps; p.splits = k.splits;
  return wgrad_finish(p, s);
}

// dW = X^T dY.  An explicit split count always takes the generic kernel; allow_1x1 = false closes the 1x1 halo route.
inline WgradPlan plan_wgrad(const ConvShape& s, long ws_cap, int splits, bool allow_1x1, int cus) {
  check_shape(s);
  WgradPlan p{};
  if (splits > 0 || !wgrad_halo_geom(s, &p.h, allow_1x1)) return plan_wgrad_generic(s, ws_cap, splits, cus);
  p.route = p.h.K == p.h.C ? ROUTE_HALO_1X1 : ROUTE_HALO;
  p.tiles = (unsigned)((p.h.O / 64) * p.h.nchunks);
  const SplitK k = split_k(p.h.M / 128, wgrad_halo_splits(p.h, ws_cap, cus));
  p.kps = k.kps; p.splits = k.splits;
  return wgrad_finish(p, s);
}

}  // namespace
}  // namespace fedmi
