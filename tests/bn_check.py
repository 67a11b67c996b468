"""The EXACT reference of csrc/kernels/bn_math.h in numpy, shared by tests/test_bn_math.py (the header compiled for
the host) and tests/test_cnn_kernels_gpu.py (the BN kernels of both grids).  Every comparison against it is bit for
bit; there are no tolerances.

Each function below is the sequence of its namesake in bn_math.h, one rounding (to nearest, ties to even) per step:

* ``+ - * /`` and ``sqrt`` of numpy on fp32 (fp64) operands are single IEEE-754 operations, correctly rounded,
  subnormals included.
* ``fma`` on fp32 is the error-free construction of tests/int8_check.py (exact fp64 product, TwoSum, one rounding).
* ``fma`` on fp64 (the batch variance) has no error-free numpy form: it is evaluated per channel in rational
  arithmetic and rounded once by Python's correctly rounded int / int division.

:func:`self_check` recomputes rows in ``fractions.Fraction`` with one explicit rounding per step and compares.
:func:`forward` / :func:`backward` chain the functions the way bn_apply / bn_bwd_apply do, for whole tensors.
Finite inputs only.
"""
from fractions import Fraction

import numpy as np

from int8_check import fma, round_f32

F32 = np.float32
STAT_REP = 16      # csrc/kernels/common.h


# ---------------------------------------------------------------------------------------------------------------
# bn_math.h, function by function (fp32 numpy arrays or scalars in, fp32 out)
# ---------------------------------------------------------------------------------------------------------------
def _f(*xs):
    return [np.asarray(x, dtype=F32) for x in xs]


def affine(z, sc, sh):
    return fma(z, sc, sh)


def add(a, r):
    a, r = _f(a, r)
    return a + r


def relu(x):
    return np.maximum(np.asarray(x, dtype=F32), F32(0))


def sum_term(s, g, z, mean, inv):
    s, g, z, mean, inv = _f(s, g, z, mean, inv)
    return fma(g * (z - mean), inv, s)


def dz(k, g, b, z, c):
    return fma(k, g, fma(b, z, c))


dz_add = add
unshift = add


def fma64(a: float, b: float, c: float) -> float:
    """One rounding of a * b + c on fp64 scalars."""
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return v.numerator / v.denominator       # int / int: correctly rounded


def batch_stats(s1, s2, M: int):
    """fp64 sums -> (mean of (z - shift), biased variance), fp32 arrays."""
    s1, s2 = np.atleast_1d(np.asarray(s1, np.float64)), np.atleast_1d(np.asarray(s2, np.float64))
    msd = s1 / np.float64(M)
    q = s2 / np.float64(M)
    var = np.array([max(fma64(-m, m, v), 0.0) for m, v in zip(msd, q)], dtype=np.float64)
    return msd.astype(F32), var.astype(F32)


def inv_std(var, eps):
    var, eps = _f(var, eps)
    with np.errstate(divide="ignore"):
        return F32(1) / np.sqrt(var + eps)


def running_mean(mom, old, mean, cbias):
    mom, old, mean, cbias = _f(mom, old, mean, cbias)
    return fma(F32(1) - mom, old, mom * (mean + cbias))


def running_var(mom, old, var, M: int):
    mom, old, var = _f(mom, old, var)
    unbias = F32(M) / F32(max(M - 1, 1))
    return fma(F32(1) - mom, old, mom * var * unbias)


def eval_mean(rmean, cbias):
    rmean, cbias = _f(rmean, cbias)
    return rmean - cbias


def scale(gamma, inv):
    gamma, inv = _f(gamma, inv)
    return gamma * inv


def shift(beta, mean, sc):
    return fma(-np.asarray(mean, dtype=F32), sc, beta)


def inv_count(M: int):
    return F32(1) / F32(M)


def bwd_b(k, sgx, invM, inv):
    k, sgx, invM, inv = _f(k, sgx, invM, inv)
    return -k * sgx * invM * inv


def bwd_c(k, sg, invM, b, mean):
    k, sg, invM, b, mean = _f(k, sg, invM, b, mean)
    return fma(-b, mean, -k * sg * invM)


# ---------------------------------------------------------------------------------------------------------------
# bf16 (the kernels' activations) as fp32 arrays
# ---------------------------------------------------------------------------------------------------------------
def bf16_round(x) -> np.ndarray:
    """fp32 -> the nearest bf16 (ties to even), returned as fp32."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(F32)


# ---------------------------------------------------------------------------------------------------------------
# whole passes, as the kernels chain the functions
# ---------------------------------------------------------------------------------------------------------------
def coeffs(p: dict, M: int, eps: float, mom: float, train: bool) -> dict:
    """bn_coeffs of one BN.  p: gamma, beta [C]; train: stats [STAT_REP, 2, C] fp64, optional rmean / rvar / shift /
    cbias; eval: rmean, rvar, optional cbias.  -> sc, sh, and in train mode smean, sinv (and rmean, rvar updated)."""
    C = len(p["gamma"])
    zero = np.zeros(C, F32)
    cbias = p.get("cbias")
    cbias = zero if cbias is None else cbias
    out = {}
    if train:
        s1, s2 = np.zeros(C), np.zeros(C)
        for r in range(STAT_REP):               # the kernel's order
            s1 = s1 + p["stats"][r, 0]
            s2 = s2 + p["stats"][r, 1]
        ms, var = batch_stats(s1, s2, M)
        mean = unshift(ms, zero if p.get("shift") is None else p["shift"])
        inv = inv_std(var, F32(eps))
        out.update(smean=mean, sinv=inv)
        if p.get("rmean") is not None:
            out.update(rmean=running_mean(F32(mom), p["rmean"], mean, cbias), rvar=running_var(F32(mom), p["rvar"], var, M))
    else:
        mean = eval_mean(p["rmean"], cbias)
        inv = inv_std(p["rvar"], F32(eps))
    out["sc"] = scale(p["gamma"], inv)
    out["sh"] = shift(p["beta"], mean, out["sc"])
    return out


def forward(z, A: dict, M: int, eps: float, mom: float, train: bool, do_relu: bool, res=None, z2=None, B: dict = None):
    """bn_apply.  z, res, z2: [M, C] fp32 arrays holding bf16 values.  -> (y as fp32 holding bf16 values, coeffs of A,
    coeffs of B or None)."""
    ca = coeffs(A, M, eps, mom, train)
    x = affine(z, ca["sc"], ca["sh"])
    cb = None
    if B is not None:
        cb = coeffs(B, M, eps, mom, train)
        x = add(x, affine(z2, cb["sc"], cb["sh"]))
    elif res is not None:
        x = add(x, res)
    if do_relu:
        x = relu(x)
    return bf16_round(x), ca, cb


def masked_grad(dya, dyb=None, y=None, z=None, msc=None):
    """g of the backward: (dya [+ dyb]) where the ReLU mask holds (y > 0, or bn_affine(z, msc[0], msc[1]) > 0)."""
    g = np.asarray(dya, dtype=F32)
    if dyb is not None:
        g = add(g, dyb)
    if y is not None:
        g = np.where(y > 0, g, F32(0))
    elif msc is not None:
        g = np.where(affine(z, msc[0], msc[1]) > 0, g, F32(0))
    return g.astype(F32)


def bwd_coeffs(sums, M: int, gamma, mean, inv, qx: int) -> dict:
    """One branch of bn_bwd_coeffs.  sums: [reps, 3, C] fp64 replicas (chained mode, summed in order) or [3, C];
    qx: 1 (branch A) or 2 (branch B)."""
    sums = np.asarray(sums, np.float64)
    if sums.ndim == 3:
        tot = np.zeros(sums.shape[1:])
        for r in range(sums.shape[0]):
            tot = tot + sums[r]
    else:
        tot = sums
    sg, sgx = tot[0].astype(F32), tot[qx].astype(F32)
    invM = inv_count(M)
    k = scale(gamma, inv)
    b = bwd_b(k, sgx, invM, inv)
    return dict(k=k, b=b, c=bwd_c(k, sg, invM, b, mean), dgamma=sgx, dbeta=sg, shift=np.asarray(mean, F32))


def backward(g, z, co: dict, dadd=None):
    """One branch of the backward apply: g from :func:`masked_grad`, co from :func:`bwd_coeffs` -> dz (bf16 values)."""
    d = dz(co["k"], g, co["b"], z, co["c"])
    if dadd is not None:
        d = dz_add(d, dadd)
    return bf16_round(d)


# ---------------------------------------------------------------------------------------------------------------
# the committed inputs of the host program (tests/golden/bn_math_inputs.txt) and the reference of its output
# ---------------------------------------------------------------------------------------------------------------
ROW_F32, ROW_F64 = 6, 2     # a row: six fp32 (hex), two fp64 (hex), M (decimal)


def make_inputs(seed: int = 17) -> list:
    """How the committed input file was made (the FILE is the authority: numpy's generator streams may change
    between versions; tests/test_bn_math.py checks that the file still holds the cases).  The rows:
    random values; c = -fp32(a * b), the rounding-distance case of bn_affine; products that are exact ties in fp32
    (25 significant bits, the last one set), alone, against a zero addend and against one far below the tie;
    subnormal results; the inv operand across 20 decades."""
    rng = np.random.default_rng(seed)
    rows = []

    def rnd(n, lo=-20, hi=20):
        return (rng.standard_normal(n) * np.exp2(rng.integers(lo, hi, n))).astype(F32)

    def emit(f, s1=None, s2=None, M=None):
        n = len(f[0])
        s1 = rng.standard_normal(n) * 1e3 if s1 is None else s1
        Ms = rng.integers(1, 200000, n) if M is None else M
        s2 = (s1 * s1 / Ms) * (1 + np.abs(rng.standard_normal(n))) if s2 is None else s2
        for i in range(n):
            rows.append(([F32(c[i]) for c in f], [float(s1[i]), float(s2[i])], int(Ms[i])))

    n = 160
    emit([rnd(n) for _ in range(6)])                                            # random
    a, b = rnd(n, -4, 4), rnd(n, -4, 4)
    emit([a, b, -(a * b), rnd(n, -4, 4), rnd(n, -4, 4), rnd(n, -4, 4)])        # rounding distance (affine, dz, shift)
    emit([rnd(n, -4, 4), rnd(n, -4, 4), a, b, -(a * b), rnd(n, -4, 4)])        # ... of dz's inner fma, of bwd_c
    # exact ties: two odd 13-bit integers whose product has 25 bits and is odd
    ta, tb = [], []
    while len(ta) < n:
        x, y = int(rng.integers(2048, 4096)) * 2 + 1, int(rng.integers(2048, 4096)) * 2 + 1
        if (x * y).bit_length() == 25:
            ta.append(x)
            tb.append(y)
    sa, sb = np.exp2(rng.integers(-30, 30, n)), np.exp2(rng.integers(-30, 30, n))
    ta, tb = (np.array(ta) * sa).astype(F32), (np.array(tb) * sb).astype(F32)
    sign = np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
    tiny = (sign * np.abs(ta * tb).astype(np.float64) * 2.0 ** -60).astype(F32)
    third = np.where(np.arange(n) % 3 == 0, F32(0), np.where(np.arange(n) % 3 == 1, tiny, rnd(n, -2, 2))).astype(F32)
    emit([ta, tb, third, tb, third, ta])
    emit([third, ta, tb, ta, tb, third])
    # subnormal results
    sm = lambda: (rng.standard_normal(n) * np.exp2(rng.integers(-75, -62, n))).astype(F32)
    emit([sm(), sm(), (rng.standard_normal(n) * 2.0 ** -140).astype(F32), sm(), sm(), sm()],
         s1=rng.standard_normal(n) * 1e-20, M=rng.integers(1, 100, n))
    # inv across 20 decades (operand e of sum_term, d of bwd_b, b of scale / inv_std)
    dec = (10.0 ** (np.arange(n) % 21 - 10)).astype(F32)
    emit([rnd(n, -6, 6), dec, rnd(n, -6, 6), dec, dec, rnd(n, -6, 6)])
    # variances that cancel: s2 / M == (s1 / M)^2 up to rounding, either side (the clamp at zero)
    s1 = rng.standard_normal(n) * 1e4
    Ms = rng.integers(2, 5000, n)
    emit([rnd(n) for _ in range(6)], s1=s1, s2=(s1 * s1 / Ms) * (1 + rng.integers(-2, 3, n) * 2.0 ** -52), M=Ms)
    return rows


def format_inputs(rows) -> str:
    out = []
    for f, d, M in rows:
        out.append(" ".join("%08x" % np.asarray(v, F32).view(np.uint32) for v in f) + " "
                   + " ".join("%016x" % np.asarray(v, np.float64).view(np.uint64) for v in d) + " %d" % M)
    return "\n".join(out) + "\n"


def parse_inputs(text: str):
    """-> (f [n, 6] fp32, d [n, 2] fp64, M [n] int)."""
    f, d, Ms = [], [], []
    for ln in text.split("\n"):
        if not ln.strip():
            continue
        w = ln.split()
        f.append([int(v, 16) for v in w[:ROW_F32]])
        d.append([int(v, 16) for v in w[ROW_F32:ROW_F32 + ROW_F64]])
        Ms.append(int(w[-1]))
    return (np.array(f, dtype=np.uint32).view(F32), np.array(d, dtype=np.uint64).view(np.float64),
            np.array(Ms, dtype=np.int64))


# the host program prints these, in this order, per row (tests/bn_math_host.cpp)
OUTPUTS = ("affine", "add", "relu", "sum_term", "dz", "dz_add", "batch_mean", "batch_var", "unshift", "inv_std",
           "running_mean", "running_var", "eval_mean", "scale", "shift", "inv_count", "bwd_b", "bwd_c")


def evaluate(f, d, Ms) -> np.ndarray:
    """The reference of the host program's output: [n, len(OUTPUTS)] fp32."""
    a, b, c, dd, e, _ = (f[:, i] for i in range(6))
    out = np.zeros((len(f), len(OUTPUTS)), dtype=F32)
    with np.errstate(all="ignore"):
        out[:, 0], out[:, 1], out[:, 2] = affine(a, b, c), add(a, b), relu(a)
        out[:, 3], out[:, 4], out[:, 5] = sum_term(a, b, c, dd, e), dz(a, b, c, dd, e), dz_add(a, b)
        for i in range(len(f)):
            m, v = batch_stats(d[i, 0], d[i, 1], int(Ms[i]))
            out[i, 6], out[i, 7] = m[0], v[0]
            out[i, 11] = running_var(a[i], b[i], c[i], int(Ms[i]))
            out[i, 15] = inv_count(int(Ms[i]))
        out[:, 8], out[:, 9] = unshift(a, b), inv_std(np.abs(a), np.abs(b))
        out[:, 10] = running_mean(a, b, c, dd)
        out[:, 12], out[:, 13], out[:, 14] = eval_mean(a, b), scale(a, b), shift(a, b, c)
        out[:, 16], out[:, 17] = bwd_b(a, b, c, dd), bwd_c(a, b, c, dd, e)
    return out


# ---------------------------------------------------------------------------------------------------------------
# self-check against exact rational arithmetic
# ---------------------------------------------------------------------------------------------------------------
def _R(v: Fraction) -> Fraction:
    return Fraction(round_f32(v))


def exact_row(f, d, M: int) -> list:
    """One row in ``fractions.Fraction``, one explicit fp32 rounding per step of bn_math.h (fp64 steps: Python's
    correctly rounded float arithmetic and :func:`fma64`).  inv_std is left out (no rational square root)."""
    a, b, c, dd, e, _ = (Fraction(float(v)) for v in f)
    one = Fraction(1)
    msd = d[0] / float(M)
    var = max(fma64(-msd, msd, d[1] / float(M)), 0.0)
    unb = _R(Fraction(M) / Fraction(max(M - 1, 1)))
    invM = _R(one / M)
    res = {
        "affine": _R(a * b + c), "add": _R(a + b), "relu": max(a, Fraction(0)),
        "sum_term": _R(_R(b * _R(c - dd)) * e + a), "dz": _R(a * b + _R(c * dd + e)), "dz_add": _R(a + b),
        "batch_mean": Fraction(float(F32(msd))), "batch_var": Fraction(float(F32(var))), "unshift": _R(a + b),
        "running_mean": _R(_R(one - a) * b + _R(a * _R(c + dd))),
        "running_var": _R(_R(one - a) * b + _R(_R(a * c) * unb)),
        "eval_mean": _R(a - b), "scale": _R(a * b), "shift": _R(-b * c + a), "inv_count": invM,
        "bwd_b": _R(_R(_R(-a * b) * c) * dd), "bwd_c": _R(-dd * e + _R(_R(-a * b) * c)),
    }
    return [res.get(k) for k in OUTPUTS]


def self_check(f, d, Ms, rows) -> int:
    """:func:`evaluate` against :func:`exact_row` on the given row indices; -> values compared."""
    got = evaluate(f[rows], d[rows], Ms[rows])
    n = 0
    for i, r in enumerate(rows):
        want = exact_row(f[r], d[r], int(Ms[r]))
        for k, w in enumerate(want):
            if w is None:
                continue
            assert float(got[i, k]) == float(w), (int(r), OUTPUTS[k], float(got[i, k]), float(w))
            n += 1
    return n
