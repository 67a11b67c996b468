"""A plain numpy fp64 reference of the PowerSGD rule (fedmi/parallel/compress.py, csrc/kernels/powersgd.hip) and the
bounds its tests use, each derived here and none tuned.  ``U = 2**-24`` is the fp32 unit roundoff."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24


def worth(rows, cols, R):
    """The segment rule: both factors are defined and together no larger than half the matrix."""
    return min(rows, cols) > R and 2 * R * (rows + cols) <= rows * cols


def delta(x, g, r):
    """d = (x - g) + r: two fp32 roundings, in this order."""
    return ((x.astype(F32) - g.astype(F32)).astype(F32) + r.astype(F32)).astype(F32)


def gemm(a, b):
    """``(a @ b, bound)`` in fp64.  An fp32 sum of k products in ANY order (tests/zoo_check.py ``around``) lies within
    (k + c) U sum|term| of the exact value: each product is rounded at most once, each of the k - 1 additions once on a
    partial sum no larger than sum|term| (1 + U)^k; c = 2 covers the second-order terms while k U < 2**-8.  The bound
    knows nothing of slabs, row chunks, waves or fold order."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return a @ b, (a.shape[1] + 2) * U * (np.abs(a) @ np.abs(b))


def orth(p, dtype=np.float64):
    """Modified Gram-Schmidt in column order (the paper's ``orthogonalize``): column i is divided by ``||col|| + 1e-8``,
    then every later column loses its component along it.  ``dtype`` float32 evaluates the same formulas in fp32."""
    p = np.array(p, dtype=dtype)
    for i in range(p.shape[1]):
        p[:, i] = p[:, i] / dtype(np.sqrt(np.sum(p[:, i] * p[:, i], dtype=dtype)) + dtype(1e-8))
        for k in range(i + 1, p.shape[1]):
            p[:, k] = p[:, k] - np.sum(p[:, i] * p[:, k], dtype=dtype) * p[:, i]
    return p


def orth_bound(pbar, dot_u=2.0 ** -53):
    """Bound on ``max |orth_fp32(P-) - orth_fp64(P-)|`` from rows, R and the condition number of P-.
    u = U + rows * dot_u is one rounding of a value that came out of a sum over the rows (the kernel sums in fp64; the
    fp32 numpy evaluation has dot_u = U).  Column k goes through k projections -- a rounded coefficient (u), its
    product and the subtraction (2 U, one for an fma), on vectors no longer than the column itself -- and one
    normalisation (the rounded denominator u, the division U): the computed factor is the exact Gram-Schmidt factor of
    P- + E with ||E||_F <= (3 R + 2) u ||P-||_F (Bjorck 1967; Higham, Accuracy and Stability, thm 19.13, constants counted
    for this code).  The orthonormal factor of a perturbed matrix moves by at most sqrt(2) kappa_2 ||E||_F / ||P-||_2 (Sun
    1991), ||P-||_F <= sqrt(R) ||P-||_2, and the computed factor's own departure from orthonormality is of the same size,
    hence the 2.  Zero columns stay zero and leave the others alone: kappa is over the non-zero columns; with more
    columns than rows the later ones are pure cancellation and nothing is claimed.  ||.||_F bounds the largest entry."""
    pbar = np.asarray(pbar, dtype=np.float64)
    live = pbar[:, np.any(pbar != 0, axis=0)]
    if live.shape[0] < live.shape[1]:
        return np.inf
    kappa = np.linalg.cond(live) if live.size else 1.0
    R = pbar.shape[1]
    return 2 * np.sqrt(2.0) * (3 * R + 2) * np.sqrt(R) * kappa * (U + pbar.shape[0] * dot_u)


def fma32(a, b, c):
    """fp32 fma(a, b, c), one rounding: the product is exact in fp64; the fp64 sum is rounded to odd (TwoSum gives what
    the addition dropped), after which rounding to fp32 equals rounding the exact sum."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    hi = p + c
    t = hi - p
    lo = (p - (hi - t)) + (c - t)
    odd_up = (lo != 0) & ((hi.view(np.int64) & 1) == 0)
    return np.where(odd_up, np.nextafter(hi, np.where(lo > 0, np.inf, -np.inf)), hi).astype(F32)


def low_rank(ph, qb):
    """u[row][col] = sum_j P^[row][j] Q-[col][j] as R fp32 fmas in j order from 0: the bits of step 4."""
    u = np.zeros((ph.shape[0], qb.shape[0]), dtype=F32)
    for j in range(ph.shape[1]):
        u = fma32(ph[:, j:j + 1].astype(F32), qb[None, :, j].astype(F32), u)
    return u
