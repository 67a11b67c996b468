"""Shared by tests/test_zoo_check.py (CPU) and tests/test_zoo_kernels_gpu.py (HIP kernels): fp64 references,
derived error bounds and the seeded cases of the zoo kernels (csrc/kernels/zoo_ops.hip).

References.  One plain numpy-fp64 function per kernel family.  Operands arrive "as stored": the bf16 / fp32
values the kernel reads, widened exactly to fp64 (a bf16 value travels as an fp32 array that holds it exactly).

Bounds are derived, not tuned.  Every reference returns an INTERVAL ``(lo, hi)`` of fp64 arrays that contains
every fp32 evaluation of the op:

* An output that accumulates ``n`` products or terms in fp32, in any order, lies within
  ``(n + c) * 2**-24 * sum|term|`` of the exact value (:func:`around`); ``c`` counts the roundings of the
  epilogue and is stated beside each family.  The bound holds for every summation order, so it knows nothing
  of slabs, splits or fold trees.
* Where a rounded value feeds further arithmetic (the ``s1`` bf16 rounding of a BN term, the BN finalizes)
  the interval is carried through that arithmetic (:func:`widen`, :func:`imul` ...): a rounding of a value in
  ``[lo, hi]`` lands in ``[lo - u*m, hi + u*m]`` with ``m = max(|lo|, |hi|)`` and ``u = 2**-24``.
* A bf16 output is checked as ``bf16_rne(lo) <= y <= bf16_rne(hi)`` (rounding is monotone): sharper than a
  relative tolerance, no constant of its own.
* Exact families (copies, selects, maxima, the Bernoulli mask, NLL backward) have ``lo == hi`` and are
  compared bit for bit.
* Three kernels use fast intrinsics (``__expf``, ``__logf``, ``rsqrtf``) whose error follows neither from the
  source nor from the project: ``EW_SIGMOID``, ``log_softmax`` / ``ce_stats`` and the BN finalizes.  Their error
  was measured ONCE against the fp64 reference (profiles/r18_zoo_pin/README.md) and the constants below are
  four times the measured value, rounded up to a power of two, in fp32 ulps of the reference value.

Finite inputs only; nothing here depends on the order of workgroups.
"""
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24          # fp32 unit roundoff

# Fast-intrinsic terms, in fp32 ulps of the reference value (4 x the measured worst error, rounded up to a
# power of two; measured on an MI355X, see profiles/r18_zoo_pin/README.md):
SIGMOID_ULP = 64.0       # measured 10.6 (inputs to +-25: the argument's rounding grows with |x| through __expf)
LSE_ULP = 32.0           # measured 3.7 forward (ulps of |max| + |log sum|), 4.9 backward (ulps of exp(y) * |sum g|)
RSQRT_ULP = 4.0          # measured 0.77 (rsqrtf(rvar + eps) over 1000 values across ten decades)

EW_COPY, EW_ADD, EW_MUL, EW_MULS, EW_RELU, EW_THR_BWD, EW_SIGMOID, EW_SIG_BWD, EW_FILL, EW_FMA = range(10)
EW_BNB, EW_BERN, EW_SUB, EW_DIV, EW_ADDS, EW_FMA_RELU, EW_BNB_THR = 11, 12, 13, 14, 15, 16, 17
EW_FMA_ADD, EW_FMA_ADD_RELU, EW_BNB_ADD, EW_BNB_THR_ADD = 18, 19, 20, 21
RD_SUM, RD_SUMSQ_SHIFT, RD_DOT_SHIFT, RD_DOT_R = 0, 1, 2, 3


# ---------------------------------------------------------------------------------------------------------------
# number formats and intervals
# ---------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """fp64 -> the nearest bf16 value (8 significant bits, ties to even), as fp64.  Normal range only."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def as_bf16(x):
    """Values rounded to bf16, carried as fp32 (exact)."""
    return bf16_rne(x).astype(F32)


def ulp32(x):
    """The fp32 ulp of |x| (fp64; 2**-149 at 0)."""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def around(ref, terms, k):
    """(lo, hi) = ref -+ k * u * sum|term|."""
    b = k * U * terms
    return ref - b, ref + b


def widen(iv, k=1.0):
    lo, hi = iv
    m = np.maximum(np.abs(lo), np.abs(hi)) * (k * U)
    return lo - m, hi + m


def iadd(a, b):
    return a[0] + b[0], a[1] + b[1]


def isub(a, b):
    return a[0] - b[1], a[1] - b[0]


def ineg(a):
    return -a[1], -a[0]


def imul(a, b):
    p = np.stack(np.broadcast_arrays(a[0] * b[0], a[0] * b[1], a[1] * b[0], a[1] * b[1]))
    return p.min(0), p.max(0)


def pt(x):
    x = np.asarray(x, dtype=np.float64)
    return x, x


def inside(y, iv, bf16_out=False):
    """Worst violation of the interval by y (0.0 = inside), and where; bf16 outputs against the rounded ends."""
    lo, hi = iv
    if bf16_out:
        lo, hi = bf16_rne(lo), bf16_rne(hi)
    y = np.asarray(y, dtype=np.float64)
    lo, hi = np.broadcast_to(lo, y.shape), np.broadcast_to(hi, y.shape)
    v = np.maximum(np.maximum(lo - y, y - hi), 0.0)
    if not np.all(np.isfinite(y)):
        return np.inf, None
    if v.size == 0 or v.max() == 0.0:
        return 0.0, None
    i = np.unravel_index(int(np.argmax(v)), v.shape)
    return float(v.max()), (i, float(y[i]), float(lo[i]), float(hi[i]))


def assert_inside(y, iv, bf16_out=False, what=""):
    v, where = inside(y, iv, bf16_out)
    assert v == 0.0, (what, "outside by", v, "at (index, y, lo, hi)", where)


def _seed(*key):
    # a stable seed from a readable key (str hashes vary per process: fold the characters instead)
    s = 0
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % 2147483629
    return s


def draw(key, shape, scale=1.0, bf16=True, offset=0.0):
    x = np.random.default_rng(_seed(*key)).standard_normal(shape) * scale + offset
    return as_bf16(x) if bf16 else x.astype(F32)


# ---------------------------------------------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------------------------------------------
EW_NIN = {EW_COPY: 1, EW_ADD: 2, EW_MUL: 2, EW_MULS: 1, EW_RELU: 1, EW_THR_BWD: 2, EW_SIGMOID: 1, EW_SIG_BWD: 2,
          EW_FILL: 0, EW_FMA: 3, EW_BNB: 5, EW_SUB: 2, EW_DIV: 2, EW_ADDS: 1, EW_FMA_RELU: 3, EW_BNB_THR: 6,
          EW_FMA_ADD: 4, EW_FMA_ADD_RELU: 4, EW_BNB_ADD: 6, EW_BNB_THR_ADD: 7}
EW_OPS = sorted(EW_NIN)
# operands that are per-channel coefficients in the op's use ('C'), the rest are activations ('A')
EW_ROLES = {EW_ADD: "AC", EW_SUB: "AC", EW_MUL: "AC", EW_DIV: "AC", EW_FMA: "ACC", EW_FMA_RELU: "ACC", EW_BNB: "ACACC",
            EW_BNB_THR: "ACACCA", EW_FMA_ADD: "ACCA", EW_FMA_ADD_RELU: "ACCA", EW_BNB_ADD: "ACACCA",
            EW_BNB_THR_ADD: "ACACCAA"}
EW_EXACT = (EW_COPY, EW_FILL, EW_RELU, EW_THR_BWD)
EW_S1_OPS = (EW_FMA_ADD, EW_FMA_ADD_RELU, EW_BNB_ADD, EW_BNB_THR_ADD)


def _sum_terms(terms, k):
    """Interval of an fp32 sum of exact terms with k roundings in all (n terms + c epilogue roundings)."""
    ref = functools.reduce(np.add, terms)
    mag = functools.reduce(np.add, [np.abs(t) for t in terms])
    return around(ref, mag, k)


def ew_ref(op, xs, s0=0.0, s1=0.0):
    """Interval of the fp32 value ew_apply computes.  xs: fp64 operands (broadcastable), s0 exact in fp32.

    Roundings counted (k = n terms + c):  ADD / SUB: 2 terms + 1 (the s0 product).  MUL / MULS / DIV: 1 + 1.
    ADDS: 2 + 0.  SIG_BWD: 1 term, 3 roundings + 1.  FMA: 2 + 1.  BNB: 3 + 2.  The *_ADD forms: the BN term as
    FMA / BNB, rounded to bf16 when s1 (the interval's ends are rounded: rounding is monotone), then one
    add of 2 terms + 0.  Without s1 the add joins the sum: one more term.
    """
    x = [np.asarray(v, dtype=np.float64) for v in xs]
    if op == EW_COPY:
        return pt(x[0])
    if op == EW_FILL:
        return pt(np.float64(s0))
    if op == EW_RELU:
        return pt(np.maximum(x[0], 0.0))
    if op == EW_THR_BWD:
        return pt(np.where(x[1] > s0, x[0], 0.0))
    if op in (EW_ADD, EW_SUB):
        return _sum_terms([x[0], (s0 if op == EW_ADD else -s0) * x[1]], 3)
    if op == EW_MUL:
        return _sum_terms([x[0] * x[1]], 2)
    if op == EW_MULS:
        return _sum_terms([x[0] * s0], 2)
    if op == EW_DIV:
        return _sum_terms([x[0] / x[1]], 2)
    if op == EW_ADDS:
        return _sum_terms([x[0], np.float64(s0) + 0.0 * x[0]], 2)
    if op == EW_SIGMOID:
        # -x exact; __expf, 1 + e, 1 / (.): the intrinsic term (measured) plus 2 roundings of the result
        ref = 1.0 / (1.0 + np.exp(-x[0]))
        b = SIGMOID_ULP * ulp32(ref) + 2 * U * ref
        return ref - b, ref + b
    if op == EW_SIG_BWD:
        return _sum_terms([x[0] * x[1] * (1.0 - x[1])], 4)
    if op in (EW_FMA, EW_FMA_RELU):
        lo, hi = _sum_terms([x[0] * x[1], x[2]], 3)
        return (np.maximum(lo, 0.0), np.maximum(hi, 0.0)) if op == EW_FMA_RELU else (lo, hi)
    if op in (EW_BNB, EW_BNB_THR):
        g = np.where(x[5] > s0, x[0], 0.0) if op == EW_BNB_THR else x[0]
        return _sum_terms([g * x[1], x[2] * x[3], x[4]], 5)
    if op in (EW_FMA_ADD, EW_FMA_ADD_RELU):
        terms, k, add = [x[0] * x[1], x[2]], 3, x[3]
    elif op in (EW_BNB_ADD, EW_BNB_THR_ADD):
        g = np.where(x[5] > s0, x[0], 0.0) if op == EW_BNB_THR_ADD else x[0]
        terms, k, add = [g * x[1], x[2] * x[3], x[4]], 5, (x[6] if op == EW_BNB_THR_ADD else x[5])
    else:
        raise ValueError(op)
    if s1 != 0.0:
        lo, hi = _sum_terms(terms, k)
        lo, hi = bf16_rne(lo), bf16_rne(hi)
        e = 2 * U * (np.maximum(np.abs(lo), np.abs(hi)) + np.abs(add))
        lo, hi = lo + add - e, hi + add + e
    else:
        lo, hi = _sum_terms(terms + [add], k + 1)
    if op == EW_FMA_ADD_RELU:
        lo, hi = np.maximum(lo, 0.0), np.maximum(hi, 0.0)
    return lo, hi


def ew_f32(op, xs, s0=0.0, s1=0.0):
    """The op as a plain numpy-float32 computation (each operation rounded once, no fused multiply-add)."""
    x = [np.asarray(v, dtype=F32) for v in xs]
    s0 = F32(s0)
    r = (lambda v: as_bf16(v)) if s1 != 0.0 else (lambda v: v)
    with np.errstate(all="ignore"):
        if op == EW_COPY: return x[0]
        if op == EW_FILL: return s0
        if op == EW_RELU: return np.maximum(x[0], F32(0))
        if op == EW_THR_BWD: return np.where(x[1] > s0, x[0], F32(0))
        if op == EW_ADD: return x[0] + s0 * x[1]
        if op == EW_SUB: return x[0] - s0 * x[1]
        if op == EW_MUL: return x[0] * x[1]
        if op == EW_MULS: return x[0] * s0
        if op == EW_DIV: return x[0] / x[1]
        if op == EW_ADDS: return x[0] + s0
        if op == EW_SIGMOID: return F32(1) / (F32(1) + np.exp(-x[0]))
        if op == EW_SIG_BWD: return x[0] * x[1] * (F32(1) - x[1])
        if op == EW_FMA: return x[0] * x[1] + x[2]
        if op == EW_FMA_RELU: return np.maximum(x[0] * x[1] + x[2], F32(0))
        if op == EW_BNB: return x[0] * x[1] + x[2] * x[3] + x[4]
        if op == EW_BNB_THR: return np.where(x[5] > s0, x[0], F32(0)) * x[1] + x[2] * x[3] + x[4]
        if op == EW_FMA_ADD: return r(x[0] * x[1] + x[2]) + x[3]
        if op == EW_FMA_ADD_RELU: return np.maximum(r(x[0] * x[1] + x[2]) + x[3], F32(0))
        if op == EW_BNB_ADD: return r(x[0] * x[1] + x[2] * x[3] + x[4]) + x[5]
        if op == EW_BNB_THR_ADD:
            return r(np.where(x[5] > s0, x[0], F32(0)) * x[1] + x[2] * x[3] + x[4]) + x[6]
    raise ValueError(op)


def ew_s0(op):
    return {EW_ADD: 0.75, EW_SUB: 1.5, EW_MULS: -0.375, EW_FILL: 2.5, EW_ADDS: 0.625}.get(op, 0.0)


def ew_operand(op, k, shape, key, bf16=True):
    """Seeded operand k of an op: generic values, except a divisor (kept away from 0), a sigmoid output (in (0, 1))
    and a threshold source (exact zeros and ties with s0 = 0 included)."""
    x = draw(("ew", op, k) + tuple(key), shape, bf16=False).astype(np.float64)
    if op == EW_DIV and k == 1:
        x = np.sign(x) * (np.abs(x) + 0.5)
    if op == EW_SIG_BWD and k == 1:
        x = 1.0 / (1.0 + np.exp(-x))
    if op == EW_SIGMOID:
        x = x * 6.0
    if (op in (EW_THR_BWD,) and k == 1) or (op in (EW_BNB_THR, EW_BNB_THR_ADD) and k == 5):
        x = np.where(np.abs(x) < 0.3, 0.0, x)
    return as_bf16(x) if bf16 else x.astype(F32)


# (name, logical shape): the three innermost widths -- 7 scalar, 12 four-wide, 24 eight-wide
EW_FLAT = (("inner7", (3, 7)), ("inner12", (3, 12)), ("inner24", (3, 24)))
EW_CL_C = 16            # channels of the channels-last cases: 16 of the 23 + 9 = 32 channels of a [2, 32, 3, 5]
EW_CL_WIDE = 32         # buffer, sliced at offset 3 (falls to scalar) or 8 (stays vector: rows of 64 bytes)
EW_CL_SHAPE = (2, EW_CL_C, 3, 5)
EW_GRID_N = 4096 * 256 + 257    # just past the grid-stride cap of 4096 blocks of 256 threads


def ew_cases(op):
    """(name, shape, [operand shapes], [operand is fp32]) of every elementwise case of an op."""
    nin = EW_NIN[op]
    out = [(name, shp, [shp] * nin, [False] * nin) for name, shp in EW_FLAT]
    roles = EW_ROLES.get(op, "A" * nin)
    chan = [(1, EW_CL_C, 1, 1) if r == "C" else EW_CL_SHAPE for r in roles]
    out.append(("cl", EW_CL_SHAPE, chan, [r == "C" for r in roles]))
    if nin >= 2:   # the last operand 0-dim
        out.append(("zerodim", EW_CL_SHAPE, chan[:-1] + [()], [r == "C" for r in roles[:-1]] + [True]))
    return out


def ew_inputs(op, case):
    name, shape, shapes, f32s = case
    return [ew_operand(op, k, s, (name,), bf16=not f) for k, (s, f) in enumerate(zip(shapes, f32s))]


def hash3(a, b, c):
    a, b, c = (np.asarray(v).astype(np.uint32) for v in (a, b, c))
    with np.errstate(over="ignore"):
        h = a * np.uint32(0x9E3779B1)
        h = h ^ ((b + np.uint32(0x7F4A7C15)) * np.uint32(0x85EBCA77))
        h = h ^ ((c + np.uint32(0x165667B1)) * np.uint32(0xC2B2AE3D))
        h = h ^ (h >> np.uint32(15)); h = h * np.uint32(0x2C1B3C6D)
        h = h ^ (h >> np.uint32(12)); h = h * np.uint32(0x297A2D39)
        h = h ^ (h >> np.uint32(15))
    return h


def bernoulli_ref(seed, ctr, n, p):
    """Mask of the n logical elements: (h >> 8) * 2**-24 < p, every step exact in fp32."""
    h = hash3(seed & 0xFFFFFFFF, ctr, np.arange(n, dtype=np.uint64) & np.uint64(0xFFFFFFFF))
    return ((h >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 < float(F32(p))).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------
# reductions: a [outer, inner] (any op), shift per outer
# ---------------------------------------------------------------------------------------------------------------
def reduce_ref(op, a, b=None, shift=None, acc=(0.0, 0.0), scale=1.0, mask=None):
    """Sums over the LAST axis of a (fp64).  -> (iv1, iv2): intervals of  acc + sums  (scale = 1), or of
    scale * sums (direct output).  n = a.shape[-1] terms; c: SUM 2 (acc add or scale, and slack for the split
    sum); SUMSQ_SHIFT 2 / 4 (the subtraction, its square counted twice, the product); DOT_SHIFT 2 / 4;
    DOT_R 2 / 2 (the bf16 product of two bf16 operands is exact before its rounding)."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[-1]
    if mask is not None:
        a = np.where(mask, a, 0.0)
    sh = 0.0 if shift is None else np.asarray(shift, dtype=np.float64)[..., None]
    if op == RD_SUM:
        t1, t2, c1, c2 = a, None, 2, 0
    elif op == RD_SUMSQ_SHIFT:
        d = a - sh
        t1, t2, c1, c2 = d, d * d, 2, 4
    elif op == RD_DOT_SHIFT:
        t1, t2, c1, c2 = a, a * (np.asarray(b, dtype=np.float64) - sh), 2, 4
    else:
        t1, t2, c1, c2 = a, bf16_rne(a * np.asarray(b, dtype=np.float64)), 2, 2
    out = []
    for t, c, a0 in ((t1, c1, acc[0]), (t2, c2, acc[1])):
        if t is None:
            out.append(None)
            continue
        ref = scale * t.sum(-1) + a0
        mag = abs(scale) * np.abs(t).sum(-1) + np.abs(a0)
        out.append(around(ref, mag, n + c))
    return out[0], out[1]


def _seq_sum(t):
    return np.cumsum(t.astype(F32), axis=-1, dtype=F32)[..., -1]


def reduce_f32(op, a, b=None, shift=None, acc=(0.0, 0.0), scale=1.0, mask=None):
    a = np.asarray(a, dtype=F32)
    if mask is not None:
        a = np.where(mask, a, F32(0))
    sh = F32(0) if shift is None else np.asarray(shift, dtype=F32)[..., None]
    if op == RD_SUM:
        t1, t2 = a, None
    elif op == RD_SUMSQ_SHIFT:
        d = a - sh
        t1, t2 = d, d * d
    elif op == RD_DOT_SHIFT:
        t1, t2 = a, a * (np.asarray(b, dtype=F32) - sh)
    else:
        t1, t2 = a, as_bf16(a * np.asarray(b, dtype=F32))
    f = lambda t, a0: None if t is None else (F32(scale) * _seq_sum(t) + np.asarray(a0, dtype=F32)).astype(F32)  # noqa: E731
    return f(t1, acc[0]), f(t2, acc[1])


RD_OUTER = (1, 63, 65)
RD_INNER = (1, 3, 31, 33, 257, 70001)     # 257: two splits; 70001: the 256-split cap (at outer <= 256)


def reduce_inputs(op, no, ni, bf16=True):
    a = draw(("rd", op, no, ni, "a"), (no, ni), bf16=bf16)
    b = draw(("rd", op, no, ni, "b"), (no, ni), bf16=bf16)
    shift = draw(("rd", op, no, ni, "s"), (no,), scale=0.25, bf16=False)
    return a, b, shift


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm finalizes (the row kernels' epilogues and the z_bn_*_coeffs kernels)
# ---------------------------------------------------------------------------------------------------------------
def bn_fwd_ref(x, shift, w, b, rmean, rvar, eps, mom):
    """x [M, C] (fp64).  -> (ref, iv): dicts of save_mean, save_invstd, rmean, rvar, scale, bias.  ref is the
    exact statistic (mean, biased variance about the mean); iv carries the kernel's own formula --
    ms = s1 / M, var = max(s2 / M - ms^2, 0), inv = rsqrt(var + eps) -- from the intervals of the two row sums
    through every rounding (c = 1 per operation; rsqrtf: RSQRT_ULP ulps of the value)."""
    x = np.asarray(x, dtype=np.float64)
    M = x.shape[0]
    shift = np.zeros(x.shape[1]) if shift is None else np.asarray(shift, dtype=np.float64)
    w64 = np.ones(x.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    b64 = np.zeros(x.shape[1]) if b is None else np.asarray(b, dtype=np.float64)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    unb = var * (M / max(M - 1, 1))
    inv = 1.0 / np.sqrt(var + eps)
    ref = {"save_mean": mean, "save_invstd": inv, "scale": w64 * inv, "bias": b64 - mean * w64 * inv}
    if rmean is not None:
        ref["rmean"] = (1 - mom) * np.asarray(rmean, dtype=np.float64) + mom * mean
        ref["rvar"] = (1 - mom) * np.asarray(rvar, dtype=np.float64) + mom * unb
    s1, s2 = reduce_ref(RD_SUMSQ_SHIFT, x.T, shift=shift)
    return ref, bn_fwd_fin_iv(s1, s2, M, shift, w64, b64, rmean, rvar, eps, mom)


def bn_fwd_fin_iv(s1, s2, M, shift, w64, b64, rmean, rvar, eps, mom):
    """The forward finalize carried over the intervals s1 = sum(x - shift), s2 = sum((x - shift)^2)."""
    eps32, mom32 = float(F32(eps)), float(F32(mom))
    ms = widen((s1[0] / M, s1[1] / M))
    q = widen((s2[0] / M, s2[1] / M))
    v = widen(isub(q, widen(imul(ms, ms))))
    v = (np.maximum(v[0], 0.0), np.maximum(v[1], 0.0))
    imean = widen(iadd(ms, pt(shift)))
    ve = widen(iadd(v, pt(eps32)))
    iinv = (1.0 / np.sqrt(ve[1]), 1.0 / np.sqrt(ve[0]))
    iinv = (iinv[0] - RSQRT_ULP * ulp32(iinv[0]), iinv[1] + RSQRT_ULP * ulp32(iinv[1]))
    sc = widen(imul(pt(w64), iinv))
    iv = {"save_mean": imean, "save_invstd": iinv, "scale": sc,
          "bias": widen(isub(pt(b64), widen(imul(imean, sc))))}
    if rmean is not None:
        c1 = pt(float(F32(1.0) - F32(mom)))
        fac = widen(pt(M / max(M - 1, 1)))
        iv["rmean"] = widen(iadd(widen(imul(c1, pt(rmean))), widen(imul(pt(mom32), imean))))
        iv["rvar"] = widen(iadd(widen(imul(c1, pt(rvar))), widen(imul(widen(imul(pt(mom32), v)), fac))))
    return iv


def bn_fwd_f32(x, shift, w, b, rmean, rvar, eps, mom):
    x = np.asarray(x, dtype=F32)
    M = x.shape[0]
    z = np.zeros(x.shape[1], dtype=F32)
    shift = z if shift is None else np.asarray(shift, dtype=F32)
    s1, s2 = reduce_f32(RD_SUMSQ_SHIFT, x.T, shift=shift)
    ms = s1 / F32(M)
    var = np.maximum(s2 / F32(M) - ms * ms, F32(0))
    mean = ms + shift
    inv = (F32(1) / np.sqrt(var + F32(eps))).astype(F32)
    sc = (z + 1 if w is None else np.asarray(w, dtype=F32)) * inv
    out = {"save_mean": mean, "save_invstd": inv, "scale": sc,
           "bias": (z if b is None else np.asarray(b, dtype=F32)) - mean * sc}
    if rmean is not None:
        c1 = F32(1) - F32(mom)
        out["rmean"] = c1 * np.asarray(rmean, dtype=F32) + F32(mom) * mean
        out["rvar"] = c1 * np.asarray(rvar, dtype=F32) + F32(mom) * var * (F32(M) / F32(max(M - 1, 1)))
    return out


def bn_bwd_ref(g, x, mean, invstd, w, mask=None):
    """g, x [M, C]; mean / invstd / w the fp32 arrays the kernel reads.  -> (ref, iv) of k, bb, cc, dw, db with
    sg = sum g, sgx = sum g (x - mean);  k = w inv,  bb = -k inv^2 sgx / M,  cc = -k sg / M - bb mean,
    dw = sgx inv,  db = sg  (c = 1 per operation of the finalize)."""
    g, x = np.asarray(g, dtype=np.float64), np.asarray(x, dtype=np.float64)
    M, C = g.shape
    mean, inv = np.asarray(mean, dtype=np.float64), np.asarray(invstd, dtype=np.float64)
    w64 = np.ones(C) if w is None else np.asarray(w, dtype=np.float64)
    if mask is not None:
        g = np.where(mask, g, 0.0)
    sg, sgx = g.sum(0), (g * (x - mean)).sum(0)
    k = w64 * inv
    bb = -k * inv * inv * sgx / M
    ref = {"k": k, "bb": bb, "cc": -k * sg / M - bb * mean, "dw": sgx * inv, "db": sg}
    isg, isgx = reduce_ref(RD_DOT_SHIFT, g.T, b=x.T, shift=mean)
    return ref, bn_bwd_fin_iv(isg, isgx, M, mean, inv, w64)


def bn_bwd_fin_iv(isg, isgx, M, mean, inv, w64):
    """The backward finalize carried over the intervals sg = sum g, sgx = sum g (x - mean)."""
    ik = widen(imul(pt(w64), pt(inv)))
    t = widen(imul(widen(imul(widen(imul(ineg(ik), pt(inv))), pt(inv))), isgx))
    ibb = widen((t[0] / M, t[1] / M))
    t = widen(imul(ineg(ik), isg))
    icc = widen(isub(widen((t[0] / M, t[1] / M)), widen(imul(ibb, pt(mean)))))
    return {"k": ik, "bb": ibb, "cc": icc, "dw": widen(imul(isgx, pt(inv))), "db": isg}


def bn_bwd_f32(g, x, mean, invstd, w, mask=None):
    g = np.asarray(g, dtype=F32)
    M, C = g.shape
    mean, inv = np.asarray(mean, dtype=F32), np.asarray(invstd, dtype=F32)
    w32 = np.ones(C, dtype=F32) if w is None else np.asarray(w, dtype=F32)
    sg, sgx = reduce_f32(RD_DOT_SHIFT, g.T, b=np.asarray(x, dtype=F32).T, shift=mean,
                         mask=None if mask is None else mask.T)
    k = w32 * inv
    bb = -k * inv * inv * sgx / F32(M)
    return {"k": k, "bb": bb, "cc": -k * sg / F32(M) - bb * mean, "dw": sgx * inv, "db": sg}


ROWS_C = (4, 8, 12, 36, 64, 72)
ROWS_M = (1, 3, 67, 1031)


def rows_inputs(C, M, bf16=True, mean=0.0):
    x = draw(("rows", C, M, "x"), (M, C), bf16=bf16, offset=mean)
    g = draw(("rows", C, M, "g"), (M, C), bf16=bf16)
    f = np.maximum(draw(("rows", C, M, "f"), (M, C), bf16=bf16), F32(0))
    p = {k: draw(("rows", C, "p", k), (C,), scale=s, bf16=False) for k, s in
         (("w", 1.0), ("b", 1.0), ("rmean", 0.5), ("mean", 0.25))}
    p["rvar"] = np.abs(draw(("rows", C, "p", "rvar"), (C,), bf16=False)) + F32(0.5)
    p["invstd"] = np.abs(draw(("rows", C, "p", "inv"), (C,), bf16=False)) + F32(0.5)
    return x, g, f, p


# ---------------------------------------------------------------------------------------------------------------
# pad_rows, pooling
# ---------------------------------------------------------------------------------------------------------------
def pad_rows_ref(src, C8):
    rows, C = src.shape
    out = np.zeros((rows, C8), dtype=src.dtype)
    out[:, :C] = src
    return out


def pool_out(n, k, s, p, ceil_mode):
    o = -(-(n + 2 * p - k) // s) + 1 if ceil_mode else (n + 2 * p - k) // s + 1
    if ceil_mode and (o - 1) * s >= n + p:
        o -= 1
    return o


# (name, is_max, kernel, stride, pad, ceil_mode, count_include_pad, divisor)
POOLS = (("max3s2p1", 1, (3, 3), (2, 2), (1, 1), False, True, 0), ("max2", 1, (2, 2), (2, 2), (0, 0), False, True, 0),
         ("max3s1p1", 1, (3, 3), (1, 1), (1, 1), False, True, 0),
         ("avg2", 0, (2, 2), (2, 2), (0, 0), False, True, 0), ("avg3s1p1", 0, (3, 3), (1, 1), (1, 1), False, True, 0),
         ("avg3s2p1ceil_cip", 0, (3, 3), (2, 2), (1, 1), True, True, 0),
         ("avg3s2p1ceil_nocip", 0, (3, 3), (2, 2), (1, 1), True, False, 0),
         ("avg3s1p1_div5", 0, (3, 3), (1, 1), (1, 1), False, True, 5),
         ("avg2x3", 0, (2, 3), (1, 2), (0, 1), False, True, 0), ("avg2x3_nocip", 0, (2, 3), (1, 2), (0, 1), False, False, 0),
         ("max2x3", 1, (2, 3), (1, 2), (0, 1), False, True, 0))
POOL_HW = ((5, 5), (7, 6), (6, 7))     # 7 x 6 clips a ceil-mode window at the padded right edge, 6 x 7 at the bottom


def _pool_windows(H, W, cfg):
    _, is_max, (kh, kw), (sh, sw), (ph, pw), ceil_mode, cip, div = cfg
    P, Q = pool_out(H, kh, sh, ph, ceil_mode), pool_out(W, kw, sw, pw, ceil_mode)
    for p in range(P):
        for q in range(Q):
            hs, ws = p * sh - ph, q * sw - pw
            he, we = min(hs + kh, H + ph), min(ws + kw, W + pw)
            pool = (he - hs) * (we - ws)                       # the window clipped to the padded input
            h0, w0, h1, w1 = max(hs, 0), max(ws, 0), min(he, H), min(we, W)
            cnt = div if div else (pool if cip else (h1 - h0) * (w1 - w0))
            yield p, q, h0, h1, w0, w1, max(cnt, 1)


def pool_inputs(H, W, cfg):
    P, Q = pool_out(H, cfg[2][0], cfg[3][0], cfg[4][0], cfg[5]), pool_out(W, cfg[2][1], cfg[3][1], cfg[4][1], cfg[5])
    rng = np.random.default_rng(_seed("pool", H, W, cfg[0]))
    if cfg[1]:   # five bf16 values: ties in most windows
        x = rng.choice(np.array([-1.0, -0.25, 0.0, 0.5, 2.0], dtype=F32), size=(2, 3, H, W))
    else:
        x = as_bf16(rng.standard_normal((2, 3, H, W)))
    return x, as_bf16(rng.standard_normal((2, 3, P, Q)))


def pool_fwd_ref(x, cfg):
    """-> (iv of y, idx or None).  avg: n = window elements summed, c = 1 (the division)."""
    x = np.asarray(x, dtype=np.float64)
    N, C, H, W = x.shape
    wins = list(_pool_windows(H, W, cfg))
    P, Q = wins[-1][0] + 1, wins[-1][1] + 1
    y, mag = np.zeros((N, C, P, Q)), np.zeros((N, C, P, Q))
    idx = np.zeros((N, C, P, Q), dtype=np.int64) if cfg[1] else None
    nmax = cfg[2][0] * cfg[2][1]
    for p, q, h0, h1, w0, w1, cnt in wins:
        win = x[:, :, h0:h1, w0:w1].reshape(N, C, -1)
        if cfg[1]:
            am = win.argmax(-1)                                  # the first maximum in scan order
            y[:, :, p, q] = np.take_along_axis(win, am[..., None], -1)[..., 0]
            idx[:, :, p, q] = (h0 + am // (w1 - w0)) * W + w0 + am % (w1 - w0)
        else:
            y[:, :, p, q] = win.sum(-1) / cnt
            mag[:, :, p, q] = np.abs(win).sum(-1) / cnt
    return (pt(y) if cfg[1] else around(y, mag, nmax + 1)), idx


def pool_fwd_f32(x, cfg):
    x = np.asarray(x, dtype=F32)
    N, C, H, W = x.shape
    wins = list(_pool_windows(H, W, cfg))
    y = np.zeros((N, C, wins[-1][0] + 1, wins[-1][1] + 1), dtype=F32)
    for p, q, h0, h1, w0, w1, cnt in wins:
        win = x[:, :, h0:h1, w0:w1].reshape(N, C, -1)
        y[:, :, p, q] = win.max(-1) if cfg[1] else _seq_sum(win) / F32(cnt)
    return y


def pool_bwd_ref(dy, cfg, H, W, idx=None):
    """dx interval: every input element sums the gradients of the windows covering it (avg: each divided by the
    window's count first).  n = windows covering an element (<= kh * kw), c = 1."""
    dy = np.asarray(dy, dtype=np.float64)
    N, C = dy.shape[:2]
    dx, mag = np.zeros((N, C, H, W)), np.zeros((N, C, H, W))
    for p, q, h0, h1, w0, w1, cnt in _pool_windows(H, W, cfg):
        if cfg[1]:
            hit = np.zeros((N, C, H * W))
            np.put_along_axis(hit, idx[:, :, p, q][..., None], 1.0, -1)
            hit = hit.reshape(N, C, H, W)
            dx += hit * dy[:, :, p, q][..., None, None]
            mag += hit * np.abs(dy[:, :, p, q])[..., None, None]
        else:
            dx[:, :, h0:h1, w0:w1] += (dy[:, :, p, q] / cnt)[..., None, None]
            mag[:, :, h0:h1, w0:w1] += (np.abs(dy[:, :, p, q]) / cnt)[..., None, None]
    return around(dx, mag, cfg[2][0] * cfg[2][1] + 1)


def pool_bwd_f32(dy, cfg, H, W, idx=None):
    dy = np.asarray(dy, dtype=F32)
    N, C = dy.shape[:2]
    dx = np.zeros((N, C, H, W), dtype=F32)
    for p, q, h0, h1, w0, w1, cnt in _pool_windows(H, W, cfg):
        if cfg[1]:
            hit = np.zeros((N, C, H * W), dtype=F32)
            np.put_along_axis(hit, idx[:, :, p, q][..., None], F32(1), -1)
            dx += hit.reshape(N, C, H, W) * dy[:, :, p, q][..., None, None]
        else:
            dx[:, :, h0:h1, w0:w1] += (dy[:, :, p, q] / F32(cnt))[..., None, None]
    return dx


# ---------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------
GEMM_F32 = ((1, 1, 1), (16, 16, 16), (17, 33, 15))
GEMM_MFMA = ((1, 33, 1), (64, 32, 64), (65, 31, 63), (77, 300, 65))


def gemm_inputs(M, K, N, a_bf16=True, b_bf16=True):
    return (draw(("gemm", M, K, N, "a"), (M, K), bf16=a_bf16), draw(("gemm", M, K, N, "b"), (K, N), bf16=b_bf16),
            draw(("gemm", M, K, N, "bias1"), (N,), bf16=True), draw(("gemm", M, K, N, "bias2"), (M, N), bf16=True))


def gemm_ref(A, B, bias=None, alpha=1.0, beta=1.0):
    """alpha A B + beta bias.  n = K products, c = 3 (the alpha and beta products, the bias add)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ref, mag = alpha * (A @ B), abs(alpha) * (np.abs(A) @ np.abs(B))
    if bias is not None:
        ref, mag = ref + beta * np.asarray(bias, dtype=np.float64), mag + np.abs(beta * np.asarray(bias, dtype=np.float64))
    return around(ref, mag, A.shape[1] + 3)


def gemm_f32(A, B, bias=None, alpha=1.0, beta=1.0):
    A, B = np.asarray(A, dtype=F32), np.asarray(B, dtype=F32)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=F32)
    for k in range(A.shape[1]):
        acc += A[:, k:k + 1] * B[k:k + 1, :]
    v = F32(alpha) * acc
    return v if bias is None else v + F32(beta) * np.asarray(bias, dtype=F32)


# ---------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------
LSM_R, LSM_J = (1, 257), (1, 10, 33)


def lsm_inputs(R, J):
    x = draw(("lsm", R, J, "x"), (R, J), scale=2.0)
    x[::3, 0] += F32(60.0)              # rows whose logits spread over 60
    x = as_bf16(x)
    return x, draw(("lsm", R, J, "g"), (R, J))


def _lse(x):
    mx = x.max(-1, keepdims=True)
    se = np.exp(x - mx).sum(-1, keepdims=True)
    return mx, se, mx + np.log(se)


def lse_err(x):
    """Error interval half-width of the kernel's  mx + __logf(sum __expf(x - mx))  per row: the intrinsic term
    (LSE_ULP ulps of |mx| + |log se|, measured) plus one rounding of the sum."""
    mx, se, lse = _lse(np.asarray(x, dtype=np.float64))
    return LSE_ULP * ulp32(np.abs(mx) + np.abs(np.log(se))) + U * np.abs(lse)


def log_softmax_ref(x):
    x = np.asarray(x, dtype=np.float64)
    lse = _lse(x)[2]
    ref = x - lse
    b = lse_err(x) + U * np.abs(ref)
    return ref - b, ref + b


def log_softmax_f32(x):
    x = np.asarray(x, dtype=F32)
    mx = x.max(-1, keepdims=True)
    return x - (mx + np.log(_seq_sum(np.exp(x - mx))[..., None]))


def log_softmax_bwd_exact(y, gy):
    y, gy = np.asarray(y, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    return gy - np.exp(y) * gy.sum(-1, keepdims=True)


def log_softmax_bwd_ref(y, gy):
    """gy - exp(y) * sum(gy), y the stored log-probabilities.  sum: n = J terms; __expf: LSE_ULP ulps of its
    value; then the product and the subtraction (c = 2 on both terms)."""
    y, gy = np.asarray(y, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    J = y.shape[1]
    sg = around(gy.sum(-1, keepdims=True), np.abs(gy).sum(-1, keepdims=True), J)
    e = np.exp(y)
    ie = (e - LSE_ULP * ulp32(e), e + LSE_ULP * ulp32(e))
    return widen(isub(pt(gy), widen(imul(ie, sg))))


def log_softmax_bwd_f32(y, gy):
    y, gy = np.asarray(y, dtype=F32), np.asarray(gy, dtype=F32)
    return gy - np.exp(y) * _seq_sum(gy)[..., None]


def nll_fwd_ref(lp, tgt, ignore, mean):
    """-> (iv of the loss, total weight).  n = R terms, c = 2 (negation free; the division, slack)."""
    lp = np.asarray(lp, dtype=np.float64)
    ok = tgt != ignore
    t = -lp[np.arange(lp.shape[0]), np.where(ok, tgt, 0)] * ok
    cnt = float(ok.sum())
    d = max(cnt, 1.0) if mean else 1.0
    return around(t.sum() / d, np.abs(t).sum() / d, lp.shape[0] + 2), cnt


def nll_fwd_f32(lp, tgt, ignore, mean):
    lp = np.asarray(lp, dtype=F32)
    ok = tgt != ignore
    t = -lp[np.arange(lp.shape[0]), np.where(ok, tgt, 0)] * ok.astype(F32)
    s = _seq_sum(t)
    return s / F32(max(ok.sum(), 1)) if mean else s


def nll_bwd_ref(R, J, g, tw, tgt, ignore, mean):
    """Exact: one fp32 division (correctly rounded) placed at the target column."""
    v = (-F32(g)) / F32(max(tw, 1.0)) if mean else -F32(g)
    out = np.zeros((R, J), dtype=F32)
    ok = tgt != ignore
    out[np.arange(R)[ok], tgt[ok]] = v
    return out


NLL_RJ = ((1, 10), (257, 10), (257, 33))
NLL_KINDS = ("plain", "ignore", "all_ignored")
CE_RJ = tuple((R, J) for R in (1, 255, 257) for J in (10, 33))


def nll_inputs(R, J, bf16, kind):
    """Stored log-probabilities (fp32 or bf16) and targets; -100 is the ignore index."""
    lp = log_softmax_f32(lsm_inputs(R, J)[0])
    tgt = np.random.default_rng(_seed("nll", R, J)).integers(0, J, R)
    if kind == "ignore":
        tgt[::3] = -100
    if kind == "all_ignored":
        tgt[:] = -100
    return (as_bf16(lp) if bf16 else lp), tgt


def ce_inputs(R, J):
    """Logits with exact ties of the maximum in every fourth row (the label on either tied column)."""
    x = lsm_inputs(R, J)[0].copy()
    rng = np.random.default_rng(_seed("ce", R, J))
    y = rng.integers(0, J, R)
    for r in range(0, R, 4):
        j = np.sort(rng.permutation(J)[:2])
        x[r, j] = x[r].max() + F32(1.0)
        y[r] = j[r // 4 % 2]
    return as_bf16(x), y                     # still tied after the rounding


def ce_stats_ref(x, y, stats0):
    """stats += (sum of CE, correct, rows).  Per row the lse error and 2 roundings; the sum of R rows onto the
    previous value: n = R + 1 terms, c = 1."""
    x = np.asarray(x, dtype=np.float64)
    R = x.shape[0]
    lse = _lse(x)[2][:, 0]
    xt = x[np.arange(R), y]
    l = lse - xt
    row_err = lse_err(x)[:, 0] + 2 * U * (np.abs(lse) + np.abs(xt))
    ref = l.sum() + stats0[0]
    b = row_err.sum() + (R + 2) * U * (np.abs(l).sum() + row_err.sum() + abs(stats0[0]))
    correct = float((x.argmax(-1) == y).sum())        # numpy, like the kernel and torch: the first maximum
    return (ref - b, ref + b), stats0[1] + correct, stats0[2] + R


def ce_stats_f32(x, y, stats0):
    x = np.asarray(x, dtype=F32)
    R = x.shape[0]
    mx = x.max(-1)
    l = (mx + np.log(_seq_sum(np.exp(x - mx[:, None])))) - x[np.arange(R), y]
    return _seq_sum(l) + F32(stats0[0])


# ---------------------------------------------------------------------------------------------------------------
# direct grouped convolution
# ---------------------------------------------------------------------------------------------------------------
# name: (N, C, O, G, (R, S), (sth, stw), (padh, padw), (H, W), layout) -- layout: "cl" bf16 channels-last,
# "slice" the same through a channel slice of a wider buffer (vectors off), "nchw32" fp32 NCHW
GCONV = {
    "a_partial_gt": (2, 12, 20, 4, (3, 3), (1, 1), (1, 1), (6, 5), "cl"),
    "b_fast": (2, 16, 32, 2, (3, 3), (1, 1), (1, 1), (6, 5), "cl"),
    "c_fast_sliced": (2, 16, 32, 2, (3, 3), (1, 1), (1, 1), (6, 5), "slice"),
    "d_two_chunks": (1, 20, 8, 1, (7, 7), (1, 1), (3, 3), (7, 7), "cl"),
    "e_1x3": (2, 8, 8, 1, (1, 3), (2, 1), (0, 1), (7, 5), "cl"),
    "e_3x1": (2, 8, 8, 1, (3, 1), (1, 1), (1, 0), (7, 5), "cl"),
    "f_s2p0": (2, 8, 16, 2, (3, 3), (2, 2), (0, 0), (7, 5), "cl"),
    "f_s2p1": (2, 8, 16, 2, (3, 3), (2, 2), (1, 1), (7, 5), "cl"),
    "f_s2p3": (2, 8, 16, 2, (3, 3), (2, 2), (3, 3), (7, 5), "cl"),
    "g_fp32": (2, 12, 20, 4, (3, 3), (1, 1), (1, 1), (6, 5), "nchw32"),
    "h_q4": (4, 8, 8, 1, (3, 3), (1, 1), (1, 1), (17, 4), "cl"),
    "h_q5": (4, 8, 8, 1, (3, 3), (1, 1), (1, 1), (17, 5), "cl"),
    "h_q9": (4, 8, 8, 1, (3, 3), (1, 1), (1, 1), (17, 9), "cl"),
    "k11": (1, 8, 8, 1, (11, 11), (1, 1), (5, 5), (12, 12), "cl"),
}


def gconv_geom(cfg):
    N, C, O, G, (R, S), (sth, stw), (ph, pw), (H, W), _ = cfg
    return (H + 2 * ph - R) // sth + 1, (W + 2 * pw - S) // stw + 1


def gconv_inputs(name):
    cfg = GCONV[name]
    key = "b_fast" if name == "c_fast_sliced" else name        # (c) is (b)'s data through another layout
    N, C, O, G, (R, S), _, _, (H, W), layout = cfg
    P, Q = gconv_geom(cfg)
    bf = layout != "nchw32"
    return (draw(("gc", key, "x"), (N, C, H, W), bf16=bf), draw(("gc", key, "w"), (O, C // G, R, S), scale=0.2, bf16=False),
            draw(("gc", key, "dy"), (N, O, P, Q), bf16=bf))


def _gconv_taps(cfg):
    N, C, O, G, (R, S), (sth, stw), (ph, pw), (H, W), _ = cfg
    P, Q = gconv_geom(cfg)
    for r in range(R):
        for s in range(S):
            # output rows / columns whose tap (r, s) falls inside the input
            ps = [p for p in range(P) if 0 <= p * sth - ph + r < H]
            qs = [q for q in range(Q) if 0 <= q * stw - pw + s < W]
            if ps and qs:
                yield r, s, np.array(ps), np.array(qs), np.array(ps) * sth - ph + r, np.array(qs) * stw - pw + s


def _gconv_all(x, w, dy, cfg, dt):
    """fwd, dgrad, wgrad and their sums of absolute terms, accumulated tap by tap in dtype dt."""
    N, C, O, G, (R, S), _, _, (H, W), _ = cfg
    P, Q = gconv_geom(cfg)
    Cg, Og = C // G, O // G
    x, w, dy = (np.asarray(v, dtype=dt) for v in (x, w, dy))
    out = [np.zeros(s, dtype=dt) for s in ((N, O, P, Q), (N, C, H, W), w.shape) * 2]
    for absolute in (0, 1):
        xa, wa, da = (np.abs(v) if absolute else v for v in (x, w, dy))
        y, dx, dw = out[3 * absolute:3 * absolute + 3]
        for r, s, ps, qs, hs, ws in _gconv_taps(cfg):
            for g in range(G):
                xs = xa[:, g * Cg:(g + 1) * Cg][:, :, hs][:, :, :, ws]          # [N, Cg, p, q]
                ds = da[:, g * Og:(g + 1) * Og][:, :, ps][:, :, :, qs]          # [N, Og, p, q]
                wt = wa[g * Og:(g + 1) * Og, :, r, s]                           # [Og, Cg]
                for c in range(Cg):     # one channel at a time: a sequential sum in dt
                    y[np.ix_(range(N), range(g * Og, (g + 1) * Og), ps, qs)] += xs[:, None, c] * wt[None, :, c, None, None]
                for o in range(Og):
                    dx[np.ix_(range(N), range(g * Cg, (g + 1) * Cg), hs, ws)] += ds[:, None, o] * wt[None, o, :, None, None]
                t = ds[:, :, None] * xs[:, None]                                   # [N, Og, Cg, p, q]
                dw[g * Og:(g + 1) * Og, :, r, s] += t.reshape(N, Og, Cg, -1).sum(-1, dtype=dt).sum(0, dtype=dt) \
                    if dt == np.float64 else _seq_sum(np.moveaxis(t, 0, 2).reshape(Og, Cg, -1))
    return out


def gconv_ref(x, w, dy, cfg):
    """Intervals of y, dx, dw.  n = Cg R S (fwd), Og R S (dgrad: an upper bound of the taps that land),
    N P Q (wgrad); c = 2 (the product of a bf16 / fp32 value and an fp32 weight rounds; slack for the slab sum)."""
    N, C, O, G, (R, S), _, _, _, _ = cfg
    P, Q = gconv_geom(cfg)
    y, dx, dw, ya, dxa, dwa = _gconv_all(x, w, dy, cfg, np.float64)
    return (around(y, ya, C // G * R * S + 2), around(dx, dxa, O // G * R * S + 2), around(dw, dwa, N * P * Q + 2))


def gconv_f32(x, w, dy, cfg):
    return _gconv_all(x, w, dy, cfg, F32)[:3]


# ---------------------------------------------------------------------------------------------------------------
# the launch planner's index decode (zoo_ops.hip zcoords / zoff, scalar and vector forms), on the CPU
# ---------------------------------------------------------------------------------------------------------------
def decode_offsets(shape, strides):
    """Element offsets of every linear index i of the iteration space `shape` in an operand with `strides`
    (zcoords: the innermost dim varies fastest; zoff: the dot product with the strides)."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    off = np.zeros(n, dtype=np.int64)
    for d in range(len(shape) - 1, 0, -1):
        q = i // shape[d]
        off += (i - q * shape[d]) * strides[d]
        i = q
    return off + i * strides[0]


def emulate_ew(descs, vmask, vw, op, s0, s1, storage):
    """Execute a recorded z_ew launch on flat numpy storages.  descs: [(key, dtype, shape, strides)] with descs[0]
    the output and key -> (flat fp32 array, base element offset) in `storage`; returns nothing, writes the output
    storage.  The vector form reads vw consecutive elements of the operands whose vmask bit is set and ONE
    element (broadcast) of the others, and stores vw consecutive outputs."""
    o = descs[0]
    shape = o[2]
    lanes = vw if vmask >= 0 else 1
    offs = [decode_offsets(shape, d[3]) for d in descs]
    xs = []
    for k, d in enumerate(descs[1:]):
        buf, base = storage[d[0]]
        vec = vmask >= 0 and (vmask >> k) & 1
        idx = base + offs[k + 1][:, None] + (np.arange(lanes) if vec else np.zeros(lanes, dtype=np.int64))[None, :]
        xs.append(buf[idx].astype(np.float64))
    val = ew_f32(op, xs, s0, s1) if xs or op == EW_FILL else None
    buf, base = storage[o[0]]
    idx = base + offs[0][:, None] + np.arange(lanes)[None, :]
    assert len(np.unique(idx)) == idx.size, "two lanes store to one element"
    val = np.broadcast_to(np.asarray(val, dtype=F32), idx.shape)
    buf[idx] = as_bf16(val) if o[1] == 1 else val
