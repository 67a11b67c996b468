"""The DnC rule (fedmi/parallel/dnc.py) in fp64 numpy and plain Python floats: the reference of tests/test_dnc.py and
tests/test_dnc_gpu.py, written from the rule's text, not from the twin."""
import math

import numpy as np

from tests.krum_check import U64, select  # noqa: F401  (select: the fp32 mean of the kept rows, shared with Krum)

U32 = 2.0 ** -24
SQUARINGS = 12


def counts(W, byz):
    f = max(0, min(byz, (W - 1) // 2))
    return f, W - f


def centre(G):
    """Double-centring in numpy fp64; a vector common to all clients drops out of it exactly (in exact arithmetic)."""
    G = np.asarray(G, dtype=np.float64)
    return G - G.mean(1, keepdims=True) - G.mean(0, keepdims=True) + G.mean()


def gram(rows):
    """The exact centred Gram: centred on the column mean in fp64, then double-centred (the mean's own rounding is a
    common vector)."""
    x = np.asarray(rows, dtype=np.float64)
    y = x - x.mean(0)
    return centre(y @ y.T)


def gram_bound(rows, keep=None):
    """Per entry of the double-centred kernel G over the clients ``keep`` (default: all) against :func:`gram` of those
    rows.  Derived, never measured:
    * pivot: exactly, the kernel's pivot is q = (the sum of the finite entries of ALL rows) / W.  In fp32 it is a
      butterfly of at most 4 roundings on every path, one rounding of 1 / W and one of the product: |p - q| <= gamma32_6
      mean_r |x_r| =: a.  The kernel's exact y is the reference's plus a common vector, |y_kernel| <= |x - q| + a =: z;
    * (double)x - (double)p rounds once per operand of a product, and an fp64 sum of n products in any order, rounded
      or fused, carries gamma_n: gamma_{n+2}; the same again for numpy's Gram, whose y is no larger: E = 2 gamma z z^T;
    * double-centring: the common vector drops out and the error is centred with it, at most E[i][j] + mean_i E +
      mean_j E + mean E; its own arithmetic (two means of at most W entries, a sum and a divide each, three additions,
      of values <= 4 max |G|, on the kernel's side and on numpy's) adds at most 4 (W + 6) u64 max (z z^T)."""
    x = np.asarray(rows, dtype=np.float64)
    W, n = x.shape
    keep = np.ones(W, dtype=bool) if keep is None else np.asarray(keep)
    finite = np.where(np.isfinite(x), x, 0.0)
    z = np.abs(x[keep] - finite.sum(0) / W) + 6 * U32 / (1.0 - 6 * U32) * np.abs(finite).sum(0) / W
    S = z @ z.T
    E = 2.0 * ((n + 2) * U64 / (1.0 - (n + 2) * U64)) * S
    return E + E.mean(1, keepdims=True) + E.mean(0, keepdims=True) + E.mean() + 4 * (W + 6) * U64 * S.max()


def score_bound(rows):
    """Of a score = lambda_1 w_i^2, (lambda_1, w) the top eigenpair of C, from C's bound alone: with e = |E|_F >= |E|_2,
    lambda_1 moves by at most e and w by at most 2 sqrt(2) e / (lambda_1 - lambda_2) (Davis-Kahan as in Yu, Wang and
    Samworth); 12 squarings leave (lambda_2 / lambda_1)^4096 of the rest in a column whose own entry of w is at least
    1 / sqrt(W).  With tau their sum, |lambda~ w~_i^2 - lambda w_i^2| <= e + lambda_1 (2 tau + tau^2)."""
    lam = np.sort(np.linalg.eigvalsh(gram(rows)))[::-1]
    e = float(np.linalg.norm(gram_bound(rows)))
    tau = 2.0 * math.sqrt(2.0) * e / (lam[0] - lam[1]) + math.sqrt(len(rows)) * (lam[1] / lam[0]) ** (2 ** SQUARINGS)
    return float(e + lam[0] * (2.0 * tau + tau * tau))


def add(terms):
    s = 0.0
    for v in terms:
        s = s + v
    return s


def finish(G, W, byz):
    """``(stats[18][16], selected ranks)`` from the centred Gram (read from its upper triangle), in Python floats."""
    m = counts(W, byz)[1]
    G = np.asarray(G, dtype=np.float64).tolist()
    up = lambda i, j: G[i][j] if i <= j else G[j][i]  # noqa: E731
    A = [i for i in range(W) if math.isfinite(G[i][i])]
    C = np.zeros((16, 16))
    score = [0.0] * W
    if A:
        rbar = {i: add(up(i, j) for j in A) / len(A) for i in A}
        gbar = add(rbar[i] for i in A) / len(A)
        for i in A:
            for j in A:
                lo, hi = min(i, j), max(i, j)
                C[i][j] = ((up(lo, hi) - rbar[lo]) - rbar[hi]) + gbar
    c = C.tolist()
    tr = add(c[i][i] for i in range(16))
    if len(A) >= 2 and 0.0 < tr < math.inf:
        B = [[v / tr for v in row] for row in c]
        for _ in range(SQUARINGS):
            T = [[add(B[i][k] * B[k][j] for k in range(16)) for j in range(16)] for i in range(16)]
            t = add(T[k][k] for k in range(16))
            B = [[v / t for v in row] for row in T]
        top = max(range(W), key=lambda o: (B[o][o], -o))
        u = [B[k][top] for k in range(16)]
        cu = [add(c[i][k] * u[k] for k in range(16)) for i in range(16)]
        den = add(u[k] * cu[k] for k in range(16))
        for i in A:
            s = (cu[i] * cu[i]) / den if den > 0.0 else 0.0
            score[i] = math.inf if math.isnan(s) else s
    for i in range(W):
        if i not in A:
            score[i] = math.inf
    selected = sorted(r for _, r in sorted((score[r], r) for r in range(W))[:m])
    stats = np.zeros((18, 16))
    stats[0, :W] = score
    stats[1, selected] = 1.0
    stats[2:] = C
    return stats, selected


def inputs(W, n, attackers=None):
    """A common part about 1e4 times the clients' differences.  ``attackers`` None: differences of distinct scale per
    client, 1e-4 (r + 1) randn (a transposed or permuted tile layout shows); else honest differences 1e-4 randn and the
    last ``attackers`` clients shifted by 1e-3 along ONE common unit-scale direction, each by its own amount."""
    rng = np.random.default_rng(7000 * W + n)
    common = 1.0 + np.abs(rng.standard_normal(n))
    if attackers is None:
        return (common + 1e-4 * (np.arange(W)[:, None] + 1) * rng.standard_normal((W, n))).astype(np.float32)
    push = np.where(np.arange(W) >= W - attackers, 1e-3 * (1.0 + 0.25 * np.arange(W)), 0.0)[:, None]
    return (common + 1e-4 * rng.standard_normal((W, n)) + push * rng.standard_normal(n)).astype(np.float32)
