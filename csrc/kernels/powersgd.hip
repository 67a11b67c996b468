// fedmi — PowerSGD (Vogels, Karimireddy, Jaggi 2019): rank-R compression of the FedAvg update on the client's flat
// state (fedmi/parallel/compress.py PowerSGDCompressor).  The float state is cut into SEGMENTS: a compressed segment is
// a row-major matrix M = d[off .. off + rows * cols) with factors P [rows, R] and Q [cols, R] at poff / qoff of the P
// and Q buffers; every other entry belongs to the DENSE part and travels as it is, behind P in the same send buffer.
//
// One round, d = (x - global) + residual, four launches (plus one fold per GEMM pass when a matrix was split):
//   psgd_project     : d = __fadd_rn(__fsub_rn(x, g), residual), written over residual;  P = M Q;  dense d -> send
//   (all-reduce-mean of the send buffer)
//   psgd_orth        : P^ = orth(P-): per column i in order,  col_i /= (float)(sqrt(sum col_i^2) + 1e-8), then
//                      col_k = fma(-(float)<col_i, col_k>, col_i, col_k) for every k > i  (the paper's code: modified
//                      Gram-Schmidt).  Sums of squares and dot products are fp64 sums of exact fp64 products.
//   psgd_backproject : Q = M^T P^  (reads d only)
//   (all-reduce-mean of Q)
//   psgd_apply       : u = sum_j P^[row][j] Q-[col][j] as R __fmaf_rn in j order from 0;  g = __fadd_rn(g, u), x = g,
//                      residual = __fsub_rn(d, u).  Dense entries: g = __fadd_rn(g, mean d), x = g, residual = 0.
//
// The GEMM passes run on v_mfma_f32_16x16x4_f32 (A lane l = A[l % 16][l / 16], B lane l = B[l / 16][l % 16], C lane l =
// C[4 (l / 16) + r][l % 16], r = 0..3) with the R factor columns padded to the instruction's 16.  A padded operand is the
// constant 0 and is never read from memory, so nothing past a row, a slab or a segment can leak into a result; a
// padded output is never written.
//
//   project: a workgroup owns 16 rows x one column slab (<= PS_SLAB columns; the host cuts long rows into slabs of
//   equal width).  Q's slab is staged in LDS.  The k index inside one wave load is free: lane (row = l % 16, kg = l / 16)
//   loads the 16 B M[row][c .. c + 3], c = cbase + 16 step + 4 kg, and feeds four MFMAs (kk = 0..3) whose B operand is
//   Q[c + kk][l % 16] -- the same permutation of k on both sides.  cbase is the slab's start moved down to the 16-B
//   boundary of the tile's first row, so rows whose length is a multiple of 4 take the vector path whatever the
//   segment's offset; any other lane takes four guarded scalar loads.  The four waves take the slab's steps round
//   robin; their tiles are added in wave order 0..3 through LDS.
//   backproject: a workgroup owns 64 columns x one row chunk (<= PB_ROWS rows); A = M^T comes from coalesced loads (lane
//   l holds M[r + l / 16][c0 + 16 wave + l % 16]), P^'s rows are staged in LDS.
//   A matrix cut into several slabs (row chunks) writes one partial per slab; psgd_fold adds them in slab order from
//   slab 0.  Every sum's order is a function of the shapes only and there are no atomics: the same inputs give the same
//   bits on every run and every client.
//
// The tables (segments, tiles, folds) are built on the host once (fedmi/parallel/compress.py psgd_tables) and live on
// the device; a launch covers every segment.
#include "flat_map.h"
#include "philox.h"

namespace fedmi {

constexpr int PS_THREADS = 256;
constexpr int PS_MAXR = 8;
constexpr int PS_SLAB = 1024;       // columns of one project / apply tile (Q's slab in LDS: PS_SLAB x R floats)
constexpr int PS_TILE_ROWS = 16;    // rows of one project / apply tile
constexpr int PB_ROWS = 256;        // rows of one backproject tile
constexpr int PB_COLS = 64;         // columns of one backproject tile
constexpr int PS_DENSE = 4096;      // dense entries of one tile
constexpr int PS_FOLD = 1024;       // entries of one fold job
constexpr int PS_ORTH_LDS = 8192;   // floats of P- that psgd_orth keeps in LDS (larger factors stay in global memory)

struct PsgdSeg { long off, poff, qoff; int rows, cols; };
// compressed: rows [r0, r1) x columns [c0, c1) of segment seg; part = where the tile's matrix partial starts in the
// partial buffer, or -1 to write the factor itself.  Dense (seg < 0): c1 entries from flat offset part to send[aux].
struct PsgdTile { int seg, r0, r1, c0, c1, pad; long part, aux; };
struct PsgdFold { long dst, src, stride; int cnt, nparts; };

}  // namespace fedmi

namespace {

using namespace fedmi;

FEDMI_DEV f32x4 mfma4(float a, float b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

FEDMI_DEV float ef_delta(float x, float g, float r) { return __fadd_rn(__fsub_rn(x, g), r); }

__global__ __launch_bounds__(PS_THREADS) void psgd_project_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                  float* __restrict__ res, const PsgdSeg* __restrict__ segs,
                                                                  const PsgdTile* __restrict__ tiles,
                                                                  const float* __restrict__ Q, int R,
                                                                  float* __restrict__ send, float* __restrict__ ppart) {
  __shared__ float qs[PS_SLAB * PS_MAXR];
  __shared__ float cw[4][256];
  const PsgdTile t = tiles[blockIdx.x];
  const int tid = threadIdx.x;
  if (t.seg < 0) {
    for (int i = tid; i < t.c1; i += PS_THREADS) {
      const long e = t.part + i;
      send[t.aux + i] = ef_delta(x[e], g[e], res[e]);
    }
    return;
  }
  const PsgdSeg s = segs[t.seg];
  const int w = t.c1 - t.c0;
  for (int i = tid; i < w * R; i += PS_THREADS) qs[i] = Q[s.qoff + (long)t.c0 * R + i];
  __syncthreads();
  const int l = lane_id(), wv = wave_id(), kg = l >> 4, j = l & 15;
  const int row = t.r0 + j;
  const bool row_ok = row < t.r1;
  const long rbase = s.off + (long)row * s.cols;
  const int cbase = t.c0 - (int)((s.off + (long)t.r0 * s.cols + t.c0) & 3);
  const int nsteps = (t.c1 - cbase + 15) >> 4;
  f32x4 acc = zero4();
  for (int st = wv; st < nsteps; st += 4) {
    const int c = cbase + 16 * st + 4 * kg;
    float dv[4] = {0.f, 0.f, 0.f, 0.f};
    if (row_ok) {
      const long e = rbase + c;
      if (c >= t.c0 && c + 4 <= t.c1 && !(e & 3)) {
        const auto xv = flat_load<4>(x, e), gv = flat_load<4>(g, e);
        auto rv = flat_load<4>(res, e);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) dv[kk] = rv[kk] = ef_delta(xv[kk], gv[kk], rv[kk]);
        flat_store<4>(res, e, rv);
      } else {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          if (c + kk >= t.c0 && c + kk < t.c1) res[e + kk] = dv[kk] = ef_delta(x[e + kk], g[e + kk], res[e + kk]);
      }
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int cl = c + kk - t.c0;
      const float b = (j < R && cl >= 0 && cl < w) ? qs[cl * R + j] : 0.f;
      acc = mfma4(dv[kk], b, acc);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) cw[wv][(4 * kg + r) * 16 + j] = acc[r];
  __syncthreads();
  const int orow = t.r0 + (tid >> 4), oj = tid & 15;
  if (orow < t.r1 && oj < R) {
    float v = cw[0][tid];
#pragma unroll
    for (int k = 1; k < 4; ++k) v = __fadd_rn(v, cw[k][tid]);
    if (t.part >= 0)
      ppart[t.part + (long)orow * R + oj] = v;
    else
      send[s.poff + (long)orow * R + oj] = v;
  }
}

__global__ __launch_bounds__(PS_THREADS) void psgd_backproject_kernel(const float* __restrict__ d,
                                                                      const PsgdSeg* __restrict__ segs,
                                                                      const PsgdTile* __restrict__ tiles,
                                                                      const float* __restrict__ Ph, int R,
                                                                      float* __restrict__ Q, float* __restrict__ qpart) {
  __shared__ float ps[PB_ROWS * PS_MAXR];
  const PsgdTile t = tiles[blockIdx.x];
  const PsgdSeg s = segs[t.seg];
  const int tid = threadIdx.x, nr = t.r1 - t.r0;
  for (int i = tid; i < nr * R; i += PS_THREADS) ps[i] = Ph[s.poff + (long)t.r0 * R + i];
  __syncthreads();
  const int l = lane_id(), wv = wave_id(), kg = l >> 4, j = l & 15;
  const int cw0 = t.c0 + 16 * wv;
  if (cw0 >= t.c1) return;
  const int c = cw0 + j;
  const bool col_ok = c < t.c1;
  const float* col = d + s.off + c;
  f32x4 acc = zero4();
  for (int r = t.r0; r < t.r1; r += 16) {       // four k steps a turn: the loads are in flight together
    float a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int rr = r + 4 * u + kg;
      const bool ok = rr < t.r1;
      a[u] = (ok && col_ok) ? col[(long)rr * s.cols] : 0.f;
      b[u] = (ok && j < R) ? ps[(rr - t.r0) * R + j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = mfma4(a[u], b[u], acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int oc = cw0 + 4 * kg + r;
    if (oc < t.c1 && j < R) {
      if (t.part >= 0)
        qpart[t.part + (long)oc * R + j] = acc[r];
      else
        Q[s.qoff + (long)oc * R + j] = acc[r];
    }
  }
}

// dst[i] = part[src + i] + part[src + stride + i] + ..  in part order from 0
__global__ __launch_bounds__(PS_THREADS) void psgd_fold_kernel(const PsgdFold* __restrict__ jobs,
                                                               const float* __restrict__ part, float* __restrict__ dst) {
  const PsgdFold f = jobs[blockIdx.x];
  for (int i = threadIdx.x; i < f.cnt; i += PS_THREADS) {
    float a = part[f.src + i];
    for (int p = 1; p < f.nparts; ++p) a = __fadd_rn(a, part[f.src + (long)p * f.stride + i]);
    dst[f.dst + i] = a;
  }
}

// K fixed-order fp64 sums over the workgroup at once (entries k with lo <= k < hi); every lane returns with all of them
template <int K>
FEDMI_DEV void block_sums(double (&v)[K], int lo, int hi, double (*sh)[PS_THREADS]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (k >= lo && k < hi) sh[k][tid] = v[k];
  __syncthreads();
  for (int s = PS_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (k >= lo && k < hi) sh[k][tid] += sh[k][tid + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (k >= lo && k < hi) v[k] = sh[k][0];
  __syncthreads();
}

// one workgroup per segment; lane t owns rows t, t + 256, .. of the factor for the whole kernel, so only the sums
// cross lanes
__global__ __launch_bounds__(PS_THREADS) void psgd_orth_kernel(const PsgdSeg* __restrict__ segs, float* __restrict__ P,
                                                               int R) {
  __shared__ float pl[PS_ORTH_LDS];
  __shared__ double sh[PS_MAXR][PS_THREADS];
  const PsgdSeg s = segs[blockIdx.x];
  const int tid = threadIdx.x, rows = s.rows;
  float* const pg = P + s.poff;
  const bool in_lds = (long)rows * R <= PS_ORTH_LDS;
  float* const p = in_lds ? pl : pg;
  if (in_lds)
    for (int r = tid; r < rows; r += PS_THREADS)
      for (int k = 0; k < R; ++k) pl[r * R + k] = pg[(long)r * R + k];
  for (int i = 0; i < R; ++i) {
    double v[PS_MAXR] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = tid; r < rows; r += PS_THREADS) {
      const double a = (double)p[(long)r * R + i];
      v[0] += a * a;
    }
    block_sums(v, 0, 1, sh);
    const float den = (float)(__dsqrt_rn(v[0]) + 1e-8);
#pragma unroll
    for (int k = 0; k < PS_MAXR; ++k) v[k] = 0.0;
    for (int r = tid; r < rows; r += PS_THREADS) {
      float* pr = p + (long)r * R;
      const float c = __fdiv_rn(pr[i], den);
      pr[i] = c;
#pragma unroll
      for (int k = 1; k < PS_MAXR; ++k)
        if (k > i && k < R) v[k] += (double)c * (double)pr[k];
    }
    if (i + 1 == R) break;
    block_sums(v, i + 1, R, sh);
    for (int r = tid; r < rows; r += PS_THREADS) {
      float* pr = p + (long)r * R;
      const float c = pr[i];
#pragma unroll
      for (int k = 1; k < PS_MAXR; ++k)
        if (k > i && k < R) pr[k] = __fmaf_rn(-(float)v[k], c, pr[k]);
    }
  }
  if (in_lds)
    for (int r = tid; r < rows; r += PS_THREADS)
      for (int k = 0; k < R; ++k) pg[(long)r * R + k] = pl[r * R + k];
}

template <int R>
FEDMI_DEV float low_rank_entry(const float* pr, const float* q) {
  float u = 0.f;
#pragma unroll
  for (int j = 0; j < R; ++j) u = __fmaf_rn(pr[j], q[j], u);
  return u;
}

// A row's share of the slab is walked in groups: group 0 is the head up to the row's first 16-B boundary, every later
// group one aligned vector (the last may be a shorter tail), so the vector width follows the row's actual address.
template <int R>
__global__ __launch_bounds__(PS_THREADS) void psgd_apply_kernel(float* __restrict__ x, float* __restrict__ g,
                                                                float* __restrict__ res, const PsgdSeg* __restrict__ segs,
                                                                const PsgdTile* __restrict__ tiles,
                                                                const float* __restrict__ Ph, const float* __restrict__ Qb,
                                                                const float* __restrict__ send) {
  __shared__ float qs[PS_SLAB * R];
  __shared__ float ps[PS_TILE_ROWS * R];
  const PsgdTile t = tiles[blockIdx.x];
  const int tid = threadIdx.x;
  if (t.seg < 0) {
    for (int i = tid; i < t.c1; i += PS_THREADS) {
      const long e = t.part + i;
      const float v = __fadd_rn(g[e], send[t.aux + i]);
      g[e] = v;
      x[e] = v;
      res[e] = 0.f;
    }
    return;
  }
  const PsgdSeg s = segs[t.seg];
  const int w = t.c1 - t.c0, nr = t.r1 - t.r0;
  for (int i = tid; i < w * R; i += PS_THREADS) qs[i] = Qb[s.qoff + (long)t.c0 * R + i];
  for (int i = tid; i < nr * R; i += PS_THREADS) ps[i] = Ph[s.poff + (long)t.r0 * R + i];
  __syncthreads();
  const int groups = (w >> 2) + 2;
  for (int idx = tid; idx < nr * groups; idx += PS_THREADS) {
    const int ri = idx / groups, cg = idx - ri * groups;
    const long base = s.off + (long)(t.r0 + ri) * s.cols + t.c0;
    int h = (int)((-base) & 3);
    if (h > w) h = w;
    const int ca = cg == 0 ? 0 : h + 4 * (cg - 1);
    int cb = cg == 0 ? h : ca + 4;
    if (cb > w) cb = w;
    if (ca >= cb) continue;
    float pr[R];
#pragma unroll
    for (int j = 0; j < R; ++j) pr[j] = ps[ri * R + j];
    const long e = base + ca;
    if (cb - ca == 4 && cg > 0) {
      auto dv = flat_load<4>(res, e);
      auto gv = flat_load<4>(g, e);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float u = low_rank_entry<R>(pr, qs + (ca + kk) * R);
        gv[kk] = __fadd_rn(gv[kk], u);
        dv[kk] = __fsub_rn(dv[kk], u);
      }
      flat_store<4>(g, e, gv);
      flat_store<4>(x, e, gv);
      flat_store<4>(res, e, dv);
    } else {
      for (int kk = 0; kk < cb - ca; ++kk) {
        const float u = low_rank_entry<R>(pr, qs + (ca + kk) * R);
        const float v = __fadd_rn(g[e + kk], u);
        g[e + kk] = v;
        x[e + kk] = v;
        res[e + kk] = __fsub_rn(res[e + kk], u);
      }
    }
  }
}

// Q's start: entry i of the Q buffer is the standard normal of Philox entry i under the caller's fixed key, so every
// client holds the same Q with nothing exchanged
struct PsgdQInit {
  float* q;
  Philox rng;

  template <int W>
  FEDMI_DEV void run(long e) const {
    FlatVec<W> v;
    if (W == 4) {
      uint32_t r[4];
      rng.block(e >> 2, r);
      box_muller(r[0], r[1], v[0], v[1]);
      box_muller(r[2], r[3], v[2], v[3]);
    } else {
      v[0] = philox_normal(rng, e);
    }
    flat_store<W>(q, e, v);
  }
};

template <int R>
void apply_r(hipStream_t st, int ntiles, float* x, float* g, float* res, const PsgdSeg* segs, const PsgdTile* tiles,
             const float* Ph, const float* Qb, const float* send) {
  hipLaunchKernelGGL(psgd_apply_kernel<R>, dim3(ntiles), dim3(PS_THREADS), 0, st, x, g, res, segs, tiles, Ph, Qb, send);
}

}  // namespace

namespace fedmi {

// the tile rules the host's table builder follows: {threads, max R, slab, tile rows, backproject rows, backproject
// columns, dense entries per tile, entries per fold job, sizeof(PsgdSeg), sizeof(PsgdTile), sizeof(PsgdFold)}
void psgd_geometry(int (&geo)[11]) {
  const int v[11] = {PS_THREADS, PS_MAXR, PS_SLAB, PS_TILE_ROWS, PB_ROWS, PB_COLS, PS_DENSE, PS_FOLD,
                     (int)sizeof(PsgdSeg), (int)sizeof(PsgdTile), (int)sizeof(PsgdFold)};
  for (int i = 0; i < 11; ++i) geo[i] = v[i];
}

void launch_psgd_qinit(hipStream_t st, float* q, long n, uint64_t key) {
  flat_map(st, n, PsgdQInit{q, Philox{(uint32_t)key, (uint32_t)(key >> 32), 0u, 0u}});
}

static void fold(hipStream_t st, const void* folds, int nfolds, const float* part, float* dst) {
  if (nfolds > 0)
    hipLaunchKernelGGL(psgd_fold_kernel, dim3(nfolds), dim3(PS_THREADS), 0, st, (const PsgdFold*)folds, part, dst);
}

void launch_psgd_project(hipStream_t st, const float* x, const float* g, float* res, const void* segs, const void* tiles,
                         int ntiles, const float* Q, int R, float* send, float* ppart, const void* folds, int nfolds) {
  if (ntiles <= 0) return;
  hipLaunchKernelGGL(psgd_project_kernel, dim3(ntiles), dim3(PS_THREADS), 0, st, x, g, res, (const PsgdSeg*)segs,
                     (const PsgdTile*)tiles, Q, R, send, ppart);
  fold(st, folds, nfolds, ppart, send);
}

void launch_psgd_orth(hipStream_t st, const void* segs, int nseg, float* P, int R) {
  if (nseg <= 0) return;
  hipLaunchKernelGGL(psgd_orth_kernel, dim3(nseg), dim3(PS_THREADS), 0, st, (const PsgdSeg*)segs, P, R);
}

void launch_psgd_backproject(hipStream_t st, const float* d, const void* segs, const void* tiles, int ntiles,
                             const float* Ph, int R, float* Q, float* qpart, const void* folds, int nfolds) {
  if (ntiles <= 0) return;
  hipLaunchKernelGGL(psgd_backproject_kernel, dim3(ntiles), dim3(PS_THREADS), 0, st, d, (const PsgdSeg*)segs,
                     (const PsgdTile*)tiles, Ph, R, Q, qpart);
  fold(st, folds, nfolds, qpart, Q);
}

void launch_psgd_apply(hipStream_t st, float* x, float* g, float* res, const void* segs, const void* tiles, int ntiles,
                       const float* Ph, const float* Qb, const float* send, int R) {
  if (ntiles <= 0) return;
  const PsgdSeg* sg = (const PsgdSeg*)segs;
  const PsgdTile* tl = (const PsgdTile*)tiles;
  switch (R) {
    case 1: apply_r<1>(st, ntiles, x, g, res, sg, tl, Ph, Qb, send); break;
    case 2: apply_r<2>(st, ntiles, x, g, res, sg, tl, Ph, Qb, send); break;
    case 3: apply_r<3>(st, ntiles, x, g, res, sg, tl, Ph, Qb, send); break;
    case 4: apply_r<4>(st, ntiles, x, g, res, sg, tl, Ph, Qb, send); break;
    case 5: apply_r<5>(st, ntiles, x, g, res, sg, tl, Ph, Qb, send); break;
    case 6: apply_r<6>(st, ntiles, x, g, res, sg, tl, Ph, Qb, send); break;
    case 7: apply_r<7>(st, ntiles, x, g, res, sg, tl, Ph, Qb, send); break;
    case 8: apply_r<8>(st, ntiles, x, g, res, sg, tl, Ph, Qb, send); break;
    default: break;   // the binding refuses R outside 1..8
  }
}

}  // namespace fedmi
