"""The Bulyan rule (fedmi/parallel/bulyan.py) in plain Python and numpy: the reference of tests/test_bulyan.py and
tests/test_bulyan_gpu.py.  The selection runs on Python floats (IEEE fp64); the fold is written per position and per
greedy step with every fp32 operation rounded through np.float32.  Nothing here calls the code under test."""
import math

import numpy as np

from tests.krum_check import dist_bound, gram, inputs  # noqa: F401  (the tests take them from here)
from tests.robust_check import sort_key


def counts(W, byz):
    """``(F_eff, theta, c, beta)``."""
    f = max(0, min(byz, (W - 3) // 4))
    return f, W - 2 * f, 2 * f, W - 4 * f


def select(G, W, byz):
    """``(stats[19][16] with row 18 zero, selected ascending, rounds)`` from the Gram matrix; ``rounds`` holds, per
    round, ``(k, the alive clients' scores ascending)`` for the tests' precondition."""
    f, theta, _, _ = counts(W, byz)
    G = np.asarray(G, dtype=np.float64).tolist()
    stats = np.zeros((19, 16))
    for i in range(W):
        for j in range(W):
            if i != j:
                v = (G[i][i] + G[j][j]) - 2.0 * G[i][j]
                stats[2 + i][j] = max(v, 0.0) if math.isfinite(v) else math.inf
    alive, rounds = list(range(W)), []
    for rnd in range(1, theta + 1):
        k = max(1, len(alive) - f - 2)
        for i in alive:
            near = sorted((stats[2 + i][j], j) for j in alive if j != i)[:k]
            s = near[0][0] if near else 0.0
            for v, _ in near[1:]:
                s = s + v
            stats[0][i] = s
        ranked = sorted((stats[0][i], i) for i in alive)
        rounds.append((k, [s for s, _ in ranked]))
        stats[1][ranked[0][1]] = rnd
        alive.remove(ranked[0][1])
    return stats, [r for r in range(W) if r not in alive], rounds


def fold(rows, record, c):
    """``(out[n] fp32, cut[W] int64)``: the fold of ``rows[record]`` with ``c`` values dropped per coordinate; ``cut``
    is indexed by original rank."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    x = rows[list(record)]
    theta, n = x.shape
    order = np.argsort(sort_key(x), axis=0, kind="stable")
    v = np.take_along_axis(x, order, axis=0)
    with np.errstate(all="ignore"):
        if theta % 2:
            med = v[theta // 2]
        else:
            med = ((v[theta // 2 - 1] + v[theta // 2]).astype(np.float32) / np.float32(2)).astype(np.float32)
        dist = sort_key(np.abs((v - med).astype(np.float32)))
        col = np.arange(n)
        lo, hi = np.zeros(n, dtype=np.int64), np.full(n, theta - 1, dtype=np.int64)
        for _ in range(c):
            drop_hi = dist[hi, col] >= dist[lo, col]
            hi, lo = hi - drop_hi, lo + ~drop_hi
        s = v[lo, col]
        for t in range(1, theta - c):
            s = (s + v[lo + t, col]).astype(np.float32)
        out = (s / np.float32(theta - c)).astype(np.float32)
    pos = np.arange(theta)[:, None]
    cut = np.zeros(rows.shape[0], dtype=np.int64)
    cut[list(record)] = np.bincount(order[(pos < lo) | (pos > hi)], minlength=theta)
    return out, cut


def fold_inputs(n, record, c):
    """``inputs(16, n)`` with its first columns overwritten by the fold's edge cases among the selected rows (column i
    holds case (i + n) % 10, so a 1-column input has one too); the unselected rows of those columns hold NaN or inf."""
    rows = inputs(16, n).copy()
    sel, theta = list(record), len(record)
    rest = [r for r in range(16) if r not in sel]
    half = theta // 2 + 1
    for i in range(min(n, 20)):
        case = (i + n) % 10
        rows[rest, i] = np.nan if case % 2 else np.inf
        if case == 0:
            rows[sel[i % theta], i] = np.nan                    # one NaN
        elif case == 1:
            rows[sel[:c], i] = np.nan                           # c NaNs: all dropped
        elif case == 2:
            rows[sel[-(c + 1):], i] = np.nan                    # c + 1 NaNs: one survives
        elif case == 3:
            rows[sel[0], i], rows[sel[-1], i] = np.inf, -np.inf     # inf at both ends
        elif case == 4:
            rows[sel[:half], i] = -np.inf                       # median -inf: NaN distances next to it, inf further out
        elif case == 5:
            rows[sel[:half], i] = np.inf                        # median +inf
        elif case == 6:
            rows[sel, i] = np.where(np.arange(theta) % 2, -0.0, 0.0)
        elif case == 7:
            rows[:, i] = 1.5                                    # all equal: the rank decides
        else:                                                   # every drop falls on one side
            rows[sel[:c], i] = (100.0 + np.arange(c)) * (1 if case == 8 else -1)
    return rows


def reference(rows, G, byz):
    """The whole rule from ``rows`` and a Gram matrix of them: ``(out, stats[19][16], selected)``."""
    W = rows.shape[0]
    stats, selected, _ = select(G, W, byz)
    out, cut = fold(rows, selected, counts(W, byz)[2])
    stats[18, :W] = cut
    return out, stats, selected
