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
