"""Shared by tests/test_int8_check.py (CPU twin), tests/test_flat_ops_gpu.py and tests/test_peer_comm_gpu.py (HIP
kernels): named inputs and an EXACT reference of the int8 + error-feedback data plane and of the rank-ordered
scatter-add.  Every comparison against it is bit for bit (``torch.equal``); there are no tolerances.

The formulas are the ones listed under "Roundings" in csrc/kernels/compress.hip.  The reference is written in
numpy, separately from the PyTorch twin in fedmi/parallel/compress.py, and every fp32 value it produces is ONE
rounding (to nearest, ties to even) of the exact real result:

* ``x - g``, ``(x - g) + r``, ``amax / 127`` and ``v / s`` are single IEEE-754 binary32 operations of numpy on
  fp32 operands: the CPU rounds each of them once, correctly (subnormals included; nothing here flushes them).
* ``rint`` of an fp32 value and the clamp to +-127 are exact.
* ``fma(a, b, c)``: the product of two fp32 values (an int8 is one) has at most 48 significant bits and lies far
  inside the fp64 range, so ``p = a * b`` is exact in fp64.  ``p + c`` need not be exact in fp64 (the exponents
  may lie more than 53 bits apart), so it is formed with the error-free TwoSum: ``hi + lo == p + c`` exactly,
  ``hi = fl64(p + c)``.  Every fp32 number and every midpoint of two neighbouring fp32 numbers (25 bits) is an
  fp64 number, and ``hi`` is the fp64 nearest to the exact sum, so the exact sum and ``hi`` lie on the same side
  of every midpoint unless ``hi`` IS a midpoint.  Rounding ``hi`` to fp32 is therefore the correct single
  rounding except when ``hi`` is a midpoint and ``lo != 0``; then the exact sum lies strictly on ``lo``'s side of
  the midpoint and the neighbour on that side is taken (:func:`_round_sum`).

:func:`self_check` recomputes whole chunks in exact rational arithmetic (``fractions.Fraction``, one explicit
round-to-nearest-even per formula) and compares; tests/test_int8_check.py runs it on every data case.

Finite inputs only: what a NaN or an infinite update does is described in the README's open issues and is not
asserted anywhere.
"""
import functools
import math
from fractions import Fraction

import numpy as np

CHUNK = 256
CASES = ("randn", "decades", "zero_chunks", "one_nonzero", "ties", "subnormal")
F32 = np.float32


def f32(v: float) -> float:
    """``v`` rounded to fp32, as a Python float (what a ``float`` kernel argument receives)."""
    return float(F32(v))


def nchunks(n: int) -> int:
    return (n + CHUNK - 1) // CHUNK


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def _round_sum(p: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fp32 nearest-even rounding of the exact p + c (fp64 arrays holding exact values); see the module docstring."""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = p + c
        t = hi - p
        lo = (p - (hi - t)) + (c - t)                     # TwoSum (Knuth): hi + lo == p + c exactly
        f = hi.astype(F32)
        back = f.astype(np.float64)
        nb = np.nextafter(f, np.where(hi > back, F32(np.inf), F32(-np.inf)))   # the fp32 on hi's other side
        nb64 = nb.astype(np.float64)
        mid = 0.5 * (back + nb64)                         # exact: 25 significant bits
        tie = (back != hi) & (mid == hi) & (lo != 0.0)
        to_nb = tie & ((lo > 0.0) == (nb64 > back))
    return np.where(to_nb, nb, f).astype(F32)


def fma(a, b, c) -> np.ndarray:
    """One rounding of a * b + c.  a, b: fp32 or int8 values (the product is exact in fp64), c: fp32."""
    p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    p, c = np.broadcast_arrays(p, np.asarray(c, dtype=np.float64))
    return _round_sum(p, c)


def delta(x: np.ndarray, g: np.ndarray, r=None) -> np.ndarray:
    """d = (x - g) + r: two fp32 operations, two roundings (r = 0 without a residual)."""
    d = x.astype(F32) - g.astype(F32)
    return d + (r.astype(F32) if r is not None else F32(0.0))


def quantise(d: np.ndarray):
    """-> q (int8, n), scales (fp32, one per 256-entry chunk), residual (fp32, n)."""
    n = d.size
    nch = nchunks(n)
    pad = np.zeros(nch * CHUNK, dtype=F32)
    pad[:n] = d
    blocks = pad.reshape(nch, CHUNK)
    amax = np.abs(blocks).max(axis=1)                     # exact
    with np.errstate(under="ignore"):
        t = amax / F32(127.0)                             # one fp32 division
    s = np.where(t > 0, t, F32(1.0)).astype(F32)          # t == 0: zero chunk, or the quotient underflowed
    with np.errstate(over="ignore", under="ignore"):
        quo = blocks / s[:, None]                         # one fp32 division
    q = np.clip(np.rint(quo), -127.0, 127.0)              # ties to even; exact
    res = fma(-q, s[:, None], blocks)
    return q.reshape(-1)[:n].astype(np.int8), s, res.reshape(-1)[:n]


def dequant_accum(q_all: np.ndarray, s_all: np.ndarray, out: np.ndarray, scale: float) -> np.ndarray:
    """out' = fma(scale, acc, out), acc = fma(q_p, s_p, acc) over the ranks p = 0..R-1 in order from 0."""
    R, n = q_all.shape
    chunk = np.arange(n) // CHUNK
    acc = np.zeros(n, dtype=F32)
    for p in range(R):
        acc = fma(q_all[p], s_all[p][chunk], acc)
    return fma(F32(scale), acc, out)


def scatter_add(out: np.ndarray, idx: np.ndarray, val: np.ndarray, scale: float) -> np.ndarray:
    """out[idx[p, i]] = fma(scale, val[p, i], out[...]) for the ranks p in order; a rank's in-range indices are
    unique; indices outside [0, n) are ignored."""
    out = out.astype(F32).copy()
    n = out.size
    for p in range(idx.shape[0]):
        j = idx[p].astype(np.int64)
        ok = (j >= 0) & (j < n)
        j, v = j[ok], val[p][ok]
        assert np.unique(j).size == j.size, "indices must be unique within a rank"
        out[j] = fma(F32(scale), v, out[j])
    return out


def int8_round(xs, g, rs, scale=None):
    """One ``-c Y`` aggregation.  xs / rs: every rank's model / residual, g: the common anchor; scale defaults to
    fp32(1 / world).  -> (new g, every rank's new residual); every rank's model becomes the new g."""
    w = len(xs)
    scale = f32(1.0 / w) if scale is None else scale
    qs, ss, new_rs = [], [], []
    for x, r in zip(xs, rs):
        q, s, res = quantise(delta(x, g, r))
        qs.append(q)
        ss.append(s)
        new_rs.append(res)
    return dequant_accum(np.stack(qs), np.stack(ss), g, scale), new_rs


# ---------------------------------------------------------------------------------------------------------------
# named data cases
# ---------------------------------------------------------------------------------------------------------------
ROUNDS = 3


def _gen(case: str, n: int, *key: int):
    import torch

    seed = 7919 * CASES.index(case) + n
    for k in key:
        seed = seed * 1009 + k + 1
    return torch.Generator().manual_seed(seed % (1 << 62))


def _randn(case, n, *key) -> np.ndarray:
    import torch

    return torch.randn(n, generator=_gen(case, n, *key)).numpy().astype(np.float64)


def _randint(case, n, lo, hi, count, *key) -> np.ndarray:
    import torch

    return torch.randint(lo, hi, (count,), generator=_gen(case, n, *key)).numpy()


def special_chunks(n: int):
    """Chunks the zero_chunks / subnormal cases single out: the second, one in the middle and the tail chunk."""
    nch = nchunks(n)
    return sorted({min(1, nch - 1), nch // 2, nch - 1})


def inputs(case: str, n: int, world: int, rounds: int = ROUNDS):
    """-> (g0, r0[rank], upd[round][rank]) as fp32 numpy arrays, rebuilt identically by every process from the
    seeded CPU generator.  Round k runs on x_rank = g_k + upd[k][rank] (one fp32 addition), with the anchor g_k and
    the residuals carried from round k - 1.  The designed cases start from g0 = 0 and r0 = 0, so their round 0
    quantises exactly d = upd[0][rank]."""
    assert case in CASES, case
    nch = nchunks(n)
    chunk = np.arange(n) // CHUNK
    lane = np.arange(n) % CHUNK
    valid = np.minimum(CHUNK, n - CHUNK * np.arange(nch))            # entries of each chunk
    zeros = np.zeros(n, dtype=F32)

    def base(scale, *key):
        return scale * _randn(case, n, *key)

    if case in ("randn", "decades", "zero_chunks"):
        mag = np.ones(n)
        if case == "decades":                                      # one exponent per chunk, the same on every rank
            mag = (10.0 ** _randint(case, n, -30, 31, nch, 50).astype(np.float64))[chunk]
        g0 = (mag * base(1.0, 0)).astype(F32)
        r0 = [(mag * base(1e-3, 1, r)).astype(F32) for r in range(world)]
        upd = [[(mag * base(1e-2, 2, k, r)).astype(F32) for r in range(world)] for k in range(rounds)]
        if case == "zero_chunks":
            sp = special_chunks(n)
            everywhere = np.isin(chunk, sp)                          # d == 0 on every rank in every round
            rank0 = (chunk == 0) & (nch > 1)                         # d == 0 on rank 0 only (x == g, r == 0)
            g0[everywhere] = 0.0
            for r in range(world):
                r0[r][everywhere | (rank0 & (r == 0))] = 0.0
                for k in range(rounds):
                    upd[k][r][everywhere | (rank0 & (r == 0))] = 0.0
        return g0, r0, upd
    if case == "one_nonzero":
        def one(k, r):
            c = np.arange(nch)
            ln = np.where(c % 3 == 0, 0, np.where(c % 3 == 1, CHUNK - 1, (37 * c + 11 * r + k) % CHUNK))
            ln = np.minimum(ln, valid - 1)
            out = zeros.copy()
            out[c * CHUNK + ln] = _randn(case, nch, 3, k, r).astype(F32)
            return out
        return zeros.copy(), [zeros.copy() for _ in range(world)], [[one(k, r) for r in range(world)] for k in range(rounds)]
    if case == "ties":
        def ties(k, r):
            e = _randint(case, n, -20, 21, nch, 60, k).astype(np.float64)        # the same on every rank
            m = _randint(case, n, -127, 127, n, 61, k, r).astype(np.float64)     # (m + 1/2) in [-126.5, 126.5]
            out = (m + 0.5) * (2.0 ** e)[chunk]
            c = np.arange(nch)
            at = c * CHUNK + (c + r) % valid                                    # the absmax lane moves with the chunk
            sign = np.where((c + r + k) % 2 == 0, 1.0, -1.0)
            out[at] = sign * 127.0 * 2.0 ** e                                   # amax = 127 * 2^e -> s = 2^e
            return out.astype(F32)
        return zeros.copy(), [zeros.copy() for _ in range(world)], [[ties(k, r) for r in range(world)] for k in range(rounds)]
    # subnormal: the special chunks hold only multiples of 2^-149 of at most 50 * 2^-149 (amax / 127 rounds to 0);
    # chunk 0 (where it is not one of them) has amax = 100 * 2^-149 (amax / 127 rounds to 2^-149: the smallest
    # nonzero scale)
    sp = special_chunks(n)
    near = 0
    tiny = 2.0 ** -149

    def sub(k, r):
        out = base(1e-2, 4, k, r)
        j = _randint(case, n, -50, 51, n, 70, k, r).astype(np.float64)
        j[lane % 5 != 0] = 0.0                                                 # mostly zeros
        c = np.arange(nch)
        top = c * CHUNK + (3 * c + r) % valid
        j[top] = 50.0                                                          # the absmax: 50 * 2^-149 exactly
        in_sp = np.isin(chunk, sp)
        out[in_sp] = (j * tiny)[in_sp]
        if near not in sp:
            jn = j.copy()
            jn[top] = -100.0
            out[chunk == near] = (jn * tiny)[chunk == near]
        return out.astype(F32)

    g0 = base(1.0, 0).astype(F32)
    g0[np.isin(chunk, sp + [near])] = 0.0
    r0 = [zeros.copy() for _ in range(world)]
    return g0, r0, [[sub(k, r) for r in range(world)] for k in range(rounds)]


def model(g: np.ndarray, upd: np.ndarray) -> np.ndarray:
    """A rank's model before an aggregation: x = g + upd, one fp32 addition."""
    return g.astype(F32) + upd.astype(F32)


@functools.lru_cache(maxsize=None)
def run_rounds(case: str, n: int, world: int, rounds: int = ROUNDS):
    """The reference over ``rounds`` aggregations of ``inputs(case, n, world)``.  -> a list, one entry per round,
    of (xs, g_before, rs_before, g_after, rs_after).  Computed once per process and shared: callers copy, never
    write into it."""
    g, rs, upd = inputs(case, n, world, rounds)
    out = []
    for k in range(rounds):
        xs = [model(g, upd[k][r]) for r in range(world)]
        g1, rs1 = int8_round(xs, g, rs)
        out.append((xs, g, rs, g1, rs1))
        g, rs = g1, rs1
    return out


# ---------------------------------------------------------------------------------------------------------------
# self-check against exact rational arithmetic
# ---------------------------------------------------------------------------------------------------------------
def round_f32(v: Fraction) -> float:
    """The fp32 nearest to the rational v, ties to even, subnormals included (no overflow expected)."""
    if v == 0:
        return 0.0
    a = abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()          # 2^(e-1) < a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1                                                          # 2^e <= a < 2^(e+1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    k = a / quantum
    lo = k.numerator // k.denominator
    rem = k - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    out = float(lo * quantum)                                           # exact: <= 25 bits
    assert out < 2.0 ** 128
    return -out if v < 0 else out


def _rint_even(v: float) -> int:
    fl = math.floor(v)
    rem = Fraction(v) - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return fl


def exact_round_chunk(xs, g, rs, scale: float):
    """One aggregation of ONE chunk in rational arithmetic.  xs, rs: per rank lists of Python floats (fp32
    values), g: list.  -> (g', per rank (q, s, r'))."""
    ranks = []
    for x, r in zip(xs, rs):
        d = [round_f32(Fraction(round_f32(Fraction(xi) - Fraction(gi))) + Fraction(ri)) for xi, gi, ri in zip(x, g, r)]
        amax = max(abs(v) for v in d)
        t = round_f32(Fraction(amax) / 127)
        s = t if t > 0 else 1.0
        q = [max(-127, min(127, _rint_even(round_f32(Fraction(v) / Fraction(s))))) for v in d]
        res = [round_f32(Fraction(v) - qi * Fraction(s)) for v, qi in zip(d, q)]
        ranks.append((q, s, res))
    g1 = []
    for i, gi in enumerate(g):
        acc = 0.0
        for q, s, _ in ranks:
            acc = round_f32(q[i] * Fraction(s) + Fraction(acc))
        g1.append(round_f32(Fraction(scale) * Fraction(acc) + Fraction(gi)))
    return g1, ranks


def check_chunks(n: int):
    """Up to six chunks spread over the state: the first three, the special ones and the last two."""
    nch = nchunks(n)
    return sorted({0, min(2, nch - 1), max(nch - 2, 0)} | set(special_chunks(n)))


def self_check(case: str, n: int, world: int = 3, rounds=(0, 1)) -> int:
    """The vectorised reference against :func:`exact_round_chunk` on :func:`check_chunks` of ``rounds``; every
    round is judged on the inputs the reference itself had.  -> entries compared (per rank)."""
    scale = f32(1.0 / world)
    hist = run_rounds(case, n, world, max(rounds) + 1)
    seen = 0
    for k in rounds:
        xs, g, rs, g1, rs1 = hist[k]
        payload = [quantise(delta(x, g, r)) for x, r in zip(xs, rs)]
        for c in check_chunks(n):
            sl = slice(c * CHUNK, min(n, (c + 1) * CHUNK))
            eg, ranks = exact_round_chunk([x[sl].tolist() for x in xs], g[sl].tolist(), [r[sl].tolist() for r in rs], scale)
            assert np.array_equal(np.array(eg, dtype=F32), g1[sl]), (case, n, k, c, "g")
            for p, (q, s, res) in enumerate(ranks):
                assert np.array_equal(np.array(q, dtype=np.int8), payload[p][0][sl]), (case, n, k, c, p, "q")
                assert F32(s) == payload[p][1][c], (case, n, k, c, p, "scale")
                assert np.array_equal(np.array(res, dtype=F32), rs1[p][sl]), (case, n, k, c, p, "residual")
                assert np.array_equal(payload[p][2][sl], rs1[p][sl])
            seen += sl.stop - sl.start
    return seen
