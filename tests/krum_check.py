"""The Krum rule (fedmi/parallel/krum.py) in fp64 numpy with plain loops: the reference of tests/test_krum.py and
tests/test_krum_gpu.py."""
import math

import numpy as np

U64 = 2.0 ** -53


def gram(rows):
    x = np.asarray(rows, dtype=np.float64)
    return x @ x.T


def gram_bound(rows):
    """Per entry: 2 gamma_n sum_k |x_i[k] x_j[k]| -- gamma_n for a sum of n exact products in ANY order (the kernel's)
    plus gamma_n for numpy's own fp64 sum."""
    x = np.abs(np.asarray(rows, dtype=np.float64))
    n = x.shape[1]
    return 2.0 * (n * U64 / (1.0 - n * U64)) * (x @ x.T)


def dist_bound(rows):
    """Of a distance: 4 gamma_n max_r sum_k x_r[k]^2 (G[i][i] + G[j][j] + 2 |G[i][j]| <= 4 max_r G[r][r])."""
    return float(2.0 * gram_bound(rows).diagonal().max())


def counts(W, byz, multi):
    f = max(0, min(byz, (W - 3) // 2))
    return f, max(1, W - f - 2), (W - f if multi else 1)


def finish(G, W, byz, multi):
    """``(stats[18][16], selected)`` -- the kernels' layout and the selected ranks ascending -- from the Gram matrix."""
    _, k, m = counts(W, byz, multi)
    G = np.asarray(G, dtype=np.float64).tolist()            # Python floats: IEEE fp64, no warnings on inf - inf
    stats = np.zeros((18, 16))
    for i in range(W):
        for j in range(W):
            if i != j:
                v = (G[i][i] + G[j][j]) - 2.0 * G[i][j]
                stats[2 + i][j] = max(v, 0.0) if math.isfinite(v) else math.inf
        near = sorted((stats[2 + i][j], j) for j in range(W) if j != i)[:k]
        s = near[0][0]
        for v, _ in near[1:]:
            s = s + v
        stats[0][i] = s
    selected = sorted(r for _, r in sorted((stats[0][r], r) for r in range(W))[:m])
    stats[1, selected] = 1.0
    return stats, selected


def select(rows, selected):
    z = np.array(rows[selected[0]], dtype=np.float32)
    for r in selected[1:]:
        z = (z + np.asarray(rows[r], dtype=np.float32)).astype(np.float32)
    return (z / np.float32(len(selected))).astype(np.float32)


def inputs(W, n, attackers=None):
    """``attackers`` None: rows of distinct scale per client, (r + 1) randn (a transposed or permuted tile layout
    shows); else honest rows c + 0.1 randn followed by ``attackers`` rows c + 10 randn."""
    rng = np.random.default_rng(1000 * W + n)
    if attackers is None:
        return ((np.arange(W)[:, None] + 1) * rng.standard_normal((W, n))).astype(np.float32)
    scale = np.where(np.arange(W) < W - attackers, 0.1, 10.0)[:, None]
    return (rng.standard_normal(n) + scale * rng.standard_normal((W, n))).astype(np.float32)
