"""The fp64 numpy reference of the geometric-median rule (fedmi/parallel/geomed.py) and the bounds its tests use.

Bounds, with their derivation.

* ``z``.  A weighted pass is W fp32 fmas in rank order, each with one rounding of relative size u = 2^-24 on a partial
  sum whose magnitude is at most S = sum_r |w_r x_r[i]|: the error is at most ((1 + u)^W - 1) S < (W + 1) u S for
  W <= 16.  Pass 0 is ``count`` adds and one divide: (count + 1) u sum|x_r[i]| / count by the same argument.
* ``sumsq_r``.  (x_r[i] - z[i]) is an fp32 number, so its square is exact in fp64 and only the additions round, each by
  at most 2^-53 of a partial sum of non-negative terms, i.e. of at most sumsq_r.  No path from a term to the result is
  longer than a lane's chain (< n) plus the workgroup's tree (16 + 16 < 256) plus the fold of at most 2048 partials:
  (n + 256 + 2048) 2^-53 sumsq_r, taken against the sum of the squared fp32 differences from the z under test (in
  extended precision, whose own error is far below the bound).
* ``dist`` and ``w`` are one sqrt, one max, W + 1 adds and two divides of correctly rounded fp64 operations on
  positive numbers, then one rounding to fp32: 4 ulp of the reference formulas applied to the sumsq under test.
"""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53


def inputs(W: int, n: int) -> np.ndarray:
    """``[W, n]`` fp32: a common vector plus per-client noise."""
    rng = np.random.default_rng(1000 * W + n)
    return (rng.standard_normal(n) + 0.5 * rng.standard_normal((W, n))).astype(np.float32)


def inputs_mixed(W: int, n: int) -> np.ndarray:
    """:func:`inputs` with every coordinate scaled by its own power of two in 2^-3 .. 2^3: sums of squares whose
    roundings depend on the order of the additions."""
    scale = 2.0 ** np.random.default_rng(7000 * W + n).integers(-3, 4, n)
    return (inputs(W, n) * scale).astype(np.float32)


def weights(W: int) -> np.ndarray:
    """W fp32 weights summing to about 1; from 3 clients on, rank 1's is exactly 0."""
    w = np.random.default_rng(W).random(W) + 0.1
    if W >= 3:
        w[1] = 0.0
    return (w / w.sum()).astype(np.float32)


def z_ref(rows: np.ndarray, w=None):
    """One pass's ``z`` in fp64 and its bound: pass 0 (``w`` None) or the weighted pass."""
    x = rows.astype(np.float64)
    with np.errstate(all="ignore"):
        if w is None:
            ok = np.isfinite(rows)
            count = ok.sum(0)
            mag = np.where(ok, np.abs(x), 0.0).sum(0) / count
            return np.where(ok, x, 0.0).sum(0) / count, (count + 1) * U32 * mag
        use = np.asarray(w) != 0
        terms = np.asarray(w, dtype=np.float64)[use, None] * x[use]
        return terms.sum(0), (len(w) + 1) * U32 * np.abs(terms).sum(0)


def sumsq_ref(rows: np.ndarray, z32: np.ndarray) -> np.ndarray:
    """Per rank, the sum of the squared fp32 differences from the fp32 ``z32``."""
    with np.errstate(all="ignore"):
        d = (rows - z32[None, :].astype(np.float32)).astype(np.longdouble)
        return (d * d).sum(1).astype(np.float64)


def flat_grid(n: int) -> int:
    """The workgroups of a pass (csrc/kernels/flat_map.h): one float4 per lane up to 2048 workgroups of 256."""
    return min(max((n // 4 + 255) // 256, 1), 2048)


def squares(rows: np.ndarray, z32: np.ndarray) -> np.ndarray:
    """``[W, n]`` fp64: the exact squares of the fp32 differences, the terms the kernel's fmas add."""
    d = (rows.astype(np.float32) - np.asarray(z32, dtype=np.float32)[None, :]).astype(np.float64)
    return d * d


def sumsq_in_kernel_order(rows: np.ndarray, z32: np.ndarray, grid: int = None) -> np.ndarray:
    """``sumsq_r`` with every fp64 addition in the order geomed.hip documents, so equal to the kernels' bit for bit
    (finite rows).  The terms are exact, so each ``fma(d, d, acc)`` is the one fp64 addition numpy does.

    * lane ``t`` of ``grid * 256``: the vectors ``i = t, t + stride, ..`` with ``c = 0..3`` inside each, then the tail
      entries ``4 (n // 4) + t, ..``;
    * workgroup: lane ``(r, j)`` adds the slots ``j, j + 16, .., j + 240`` of rank ``r``, lane ``(r, 0)`` the 16 results;
    * finish: lane ``(g, r)`` adds the partials ``g, g + 64, ..`` from 0, then the binary tree 512 -> 16 over ``g``.

    Vectorised over the lanes.  The finish's groups are padded with ``+0.0``, which changes no bit of a non-negative
    sum.  ``grid`` is ``flat_grid(n)`` as in the launcher; a test may pass a smaller one."""
    W, n = rows.shape
    grid = flat_grid(n) if grid is None else grid
    sq, n4, lanes = squares(rows, z32), n // 4, grid * 256
    acc = np.zeros((W, lanes))
    for first in range(0, n4, lanes):                   # one trip of the lanes first .. first + lanes - 1
        trip = sq[:, 4 * first:4 * min(first + lanes, n4)].reshape(W, -1, 4)
        for c in range(4):
            acc[:, :trip.shape[1]] += trip[:, :, c]
    for i in range(n4 * 4, n):                          # n % 4 <= 3 < lanes: lane i - 4 n4, one entry each
        acc[:, i - n4 * 4] += sq[:, i]
    sh = acc.reshape(W, grid, 16, 16)                   # [rank, workgroup, k, j]: lane slot 16 k + j
    s = sh[:, :, 0, :]
    for k in range(1, 16):
        s = s + sh[:, :, k, :]
    partial = s[:, :, 0]
    for k in range(1, 16):
        partial = partial + s[:, :, k]
    groups = np.zeros((W, -(-grid // 64) * 64))
    groups[:, :grid] = partial
    groups = groups.reshape(W, -1, 64)
    f = np.zeros((W, 64))
    for m in range(groups.shape[1]):
        f = f + groups[:, m, :]
    for h in (32, 16, 8, 4, 2, 1):                      # LDS slots s = 16 h: 512 .. 16
        f = f[:, :h] + f[:, h:2 * h]
    return f[:, 0]


def sumsq_in_kernel_order_loops(rows: np.ndarray, z32: np.ndarray, grid: int) -> np.ndarray:
    """:func:`sumsq_in_kernel_order` as the kernels' own loops, lane by lane in Python floats: what pins it."""
    W, n = rows.shape
    sq, n4, stride = squares(rows, z32).tolist(), n // 4, grid * 256
    out = []
    for r in range(W):
        partial = []
        for wg in range(grid):
            sh = []
            for lane in range(256):
                t, acc = wg * 256 + lane, 0.0
                for i in range(t, n4, stride):
                    for c in range(4):
                        acc += sq[r][4 * i + c]
                for i in range(4 * n4 + t, n, stride):
                    acc += sq[r][i]
                sh.append(acc)
            for j in range(16):
                s = sh[j]
                for k in range(1, 16):
                    s += sh[j + 16 * k]
                sh[j] = s
            s = sh[0]
            for k in range(1, 16):
                s += sh[k]
            partial.append(s)
        sh = []
        for g in range(64):
            acc = 0.0
            for i in range(g, grid, 64):
                acc += partial[i]
            sh.append(acc)
        h = 32
        while h >= 1:
            for g in range(h):
                sh[g] += sh[g + h]
            h //= 2
        out.append(sh[0])
    return np.array(out, dtype=np.float64)


def finish_ref(sumsq: np.ndarray, nu: float):
    """``(dist, w)`` of the rule's finish: ``w`` in fp32."""
    with np.errstate(all="ignore"):
        dist = np.sqrt(sumsq)
        beta = np.where(np.isfinite(dist), 1.0 / np.maximum(nu, dist), 0.0)
    B = 0.0
    for b in beta:
        B += b
    w = (beta / B).astype(np.float32) if B > 0 else np.full(len(beta), np.float32(1.0) / np.float32(len(beta)))
    return dist, w


def iterate(rows: np.ndarray, iters: int, nu: float):
    """The whole iteration with every sum in fp64: ``(z, weights that formed it)``."""
    z, w = z_ref(rows)[0], None
    for _ in range(iters):
        w = finish_ref(((rows.astype(np.float64) - z) ** 2).sum(1), nu)[1]
        z = z_ref(rows, w)[0]
    return z, w


def near(got, want, tol) -> bool:
    """Every entry within ``tol``, or the same non-finite value."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(all="ignore"):
        return bool(((np.abs(got - want) <= tol) | (got == want) | (np.isnan(got) & np.isnan(want))).all())


def check_pass(rows, w, z, hist, nu, tag=""):
    """One pass under test -- its ``z`` (fp32) and history row ``hist`` ``[3, >= W]`` -- against the reference."""
    W, n = rows.shape
    want_z, bound = z_ref(rows, w)
    assert near(z, want_z, bound), f"{tag}: z outside its bound"
    want_sq = sumsq_ref(rows, np.asarray(z, dtype=np.float32))
    assert near(hist[0][:W], want_sq, (n + 256 + 2048) * U64 * want_sq), f"{tag}: sumsq {hist[0][:W]} != {want_sq}"
    dist, w_next = finish_ref(np.asarray(hist[0][:W], dtype=np.float64), nu)
    assert near(hist[1][:W], dist, 4 * np.spacing(np.abs(dist))), f"{tag}: dist {hist[1][:W]} != {dist}"
    assert near(hist[2][:W], w_next, 4 * np.spacing(np.abs(w_next))), f"{tag}: w {hist[2][:W]} != {w_next}"
