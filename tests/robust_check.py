"""The exact reference of the robust aggregation rule (fedmi/parallel/robust.py) in numpy, the inputs of its tests
and their comparison helpers.  Shared by tests/test_robust.py (CPU) and tests/test_robust_gpu.py.

Reference: the sort key as a uint32, a stable argsort along the clients (ties to the lower rank), sequential fp32
adds through the kept window in position order, one IEEE fp32 divide, and the cut counts.  Nothing here calls the
code under test.
"""
from __future__ import annotations

import functools

import numpy as np

CASES = ("randn", "ties", "extremes", "nan")
NS = (1, 3, 4, 5, 1027)
EPS32 = 2.0 ** -24                   # unit roundoff of fp32 (round to nearest)


def b_max(W: int) -> int:
    return (W - 1) // 2


def b_eff(kind: str, trim: int, W: int) -> int:
    return b_max(W) if kind == "median" else min(trim, b_max(W))


def sort_key(x: np.ndarray) -> np.ndarray:
    """uint32 key: NaN (either sign) -> 0xFFFFFFFF, sign bit set -> ~u, else u ^ 0x80000000."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def reference(rows: np.ndarray, b: int):
    """``rows``: [W, n] fp32.  Returns ``(out[n] fp32, cut[W] int64)``."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    W, n = rows.shape
    assert 0 <= b <= b_max(W)
    order = np.argsort(sort_key(rows), axis=0, kind="stable")
    v = np.take_along_axis(rows, order, axis=0)
    with np.errstate(all="ignore"):
        s = v[b].copy()
        for j in range(b + 1, W - b):
            s = (s + v[j]).astype(np.float32)
        out = (s / np.float32(W - 2 * b)).astype(np.float32)
    outside = np.concatenate((order[:b], order[W - b:])).reshape(-1)
    return out, np.bincount(outside, minlength=W).astype(np.int64)


@functools.lru_cache(maxsize=None)
def inputs(case: str, W: int, n: int, b: int = 0, seed: int = 0) -> np.ndarray:
    """The [W, n] fp32 rows of one data case (cached; never written).  ``nan`` scatters NaNs of both signs over at
    most ``b`` rows; ``nan+`` over ``b + 1`` rows, so that a NaN survives the trim somewhere."""
    rng = np.random.default_rng(1_000_003 * seed + 7919 * W + 31 * n + 3 * b + CASES.index(case.rstrip("+")))
    if case == "randn":
        x = rng.standard_normal((W, n)).astype(np.float32)
    elif case == "ties":
        x = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32), size=(W, n))
    elif case == "extremes":
        pool = np.array([np.inf, -np.inf, 3e38, -3e38, 1e-45, -1e-45, 5e-39, -5e-39, 1.17549435e-38, 0.0, -0.0, 1.0,
                         -2.5], dtype=np.float32)
        x = rng.choice(pool, size=(W, n))
    elif case in ("nan", "nan+"):
        x = rng.standard_normal((W, n)).astype(np.float32)
        k = min(W, b + (case == "nan+"))
        bad = rng.permutation(W)[:k]
        nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
        for r in bad:
            hit = rng.random(n) < 0.5
            if case == "nan+":
                hit[0] = True                      # coordinate 0 has b + 1 NaNs: one survives
            x[r, hit] = rng.choice(nans, size=int(hit.sum()))
    else:
        raise KeyError(case)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def data_cases(W: int, b: int):
    """The case names to run at ``(W, b)``: every case, plus ``nan+`` where ``b + 1`` rows fit."""
    return CASES + (("nan+",) if b + 1 <= W else ())


def same_bits(got: np.ndarray, want: np.ndarray) -> str:
    """'' if ``got`` and ``want`` have equal NaN masks and equal bits elsewhere, else a description of the first
    difference."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32)))
    if not bad.any():
        return ""
    i = int(np.flatnonzero(bad)[0])
    return f"{int(bad.sum())} of {got.size} entries differ, first at {i}: {got.flat[i]!r} != {want.flat[i]!r}"


def mean_bound(m: int) -> float:
    """Relative rounding bound of the rule's ``m``-term fp32 mean.  The ``m - 1`` sequential adds and the divide are
    ``m`` roundings, each a factor ``1 + d``, ``|d| <= u = 2^-24`` (no underflow in an add; the tests' garbage-free
    rows are normal numbers), so the result is ``sum_j v_j (1 + t_j) / m`` with ``|t_j| <= g_m = m u / (1 - m u)``
    (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1).  For kept values all inside ``[lo, hi]``
    the exact mean lies in ``[lo, hi]``, so the computed one lies within ``g_m * max(|lo|, |hi|)`` of it."""
    return m * EPS32 / (1.0 - m * EPS32)


def zero_one(W: int) -> np.ndarray:
    """[W, 2^W]: column j holds the bits of j (row r = bit r).  By the zero-one principle a network that sorts all
    of these sorts everything; the many ties pin the rank tie-break through the cut counts."""
    j = np.arange(1 << W, dtype=np.int64)
    x = ((j[None, :] >> np.arange(W, dtype=np.int64)[:, None]) & 1).astype(np.float32)
    x.setflags(write=False)
    return x
