"""Shared by tests/test_conv_check.py (CPU) and tests/test_conv_pin_gpu.py (HIP kernels): fp64 references, derived
error bounds and the case tables of the dense conv kernels (csrc/kernels/conv_igemm.hip) and the depthwise ones
(csrc/kernels/dwconv.hip).  No GPU code here.  The number formats, intervals and seeded draws are zoo_check's.

References.  One fp64 function per operation (dense forward / DGRAD / WGRAD, depthwise forward / DGRAD / WGRAD).
Operands arrive "as stored": bf16 values (carried exactly in fp32 arrays) or the fp32 depthwise weights, widened
exactly.  Each returns ``(exact result, sum of |terms|)``; the second is the same operation on ``|x|`` and ``|w|``.
torch's fp64 CPU convolutions do the bulk work; ``loop_*`` are direct nested-loop numpy versions that fix the
padding, stride, flip and layout conventions independently of them (tests/test_conv_check.py holds the two together).

Bounds are derived, not tuned.  ``u = 2**-24``.

* Accumulation.  An output that accumulates ``n`` products in fp32 lies within ``2 * (n + c) * u * sum|term|`` of the
  exact value (:func:`acc_iv`).  Any summation tree over n terms passes each term through at most n - 1 adds that
  round (adding an exact zero -- a masked K-tail product, an empty split group -- does not), so ``n * u * sum|term|``
  holds for every order, tile and split to first order in u; the factor 2 makes it hold for any rounding direction of
  each add (nobody here has measured the bf16 MFMA's adder) and swallows the second-order terms.  bf16 x bf16
  products are exact in fp32.  ``n`` is the number of products that can be non-zero, ``c`` the further roundings:

  - dense forward: ``n = R*S*Cw``.  Unsplit (conv_tap / conv_igemm / conv_stem_kernel epilogues,
    ``ct[..] = (bf16)acc`` at conv_igemm.hip:378, :710, :1216): ``c = 1``.  Split-K (conv_splitk_reduce,
    ``v += partial`` in split order at :1500): ``c = splits`` (the splits - 1 combine adds are already inside
    the any-order argument; they are counted again on purpose, the table states them).
  - dense DGRAD: ``n = taps(phase) * O`` -- at stride 2 the input pixel's parity selects the taps that reach it
    (:func:`dgrad_taps`); a tap-less parity has n = 0 and an exactly zero output.  ``c`` as for the forward.
  - dense WGRAD: ``n = N*P*Q``, ``c = 2`` (fp32 partials by plain stores, conv_igemm.hip:363; the reduce bodies of
    wgrad_reduce.h add splits and the four split groups, all inside the any-order argument; nothing rounds after
    the last add).  ``accumulate=True`` is ``out[e] + s`` (wgrad_reduce.h:69, :105, :133): one more rounding on
    ``|base + dw|`` (:func:`widen`).
  - depthwise forward / DGRAD: ``acc += v * wt`` (dwconv.hip:100, :114): bf16 x fp32 is not exact in fp32, so every
    tap counts its product's rounding and its add (a contracted fma has one; the bound takes both):
    ``n = 2*R*S``, ``c = 1``.
  - depthwise WGRAD: x and dy are both bf16, products exact: ``n = N*P*Q``, ``c = 2``, ``accumulate`` as above.

* A bf16 output is checked as ``bf16_rne(lo) <= y <= bf16_rne(hi)`` (zoo_check.inside, rounding is monotone).
* A residual (forward ``res``), second grad (DGRAD ``add``) or ``accumulate`` operand r follows its path:

  - unsplit tap / generic epilogue: ``t = (bf16)((float)t + (float)r)`` on the already rounded tile
    (conv_igemm.hip:395, :787): two roundings -> ``bf16_rne`` of the ends, ``+ r``, :func:`widen`, then the bf16
    check (:func:`add_unsplit`);
  - split-K combine: ``v += (float)r`` before the one ``(bf16)v`` (conv_igemm.hip:1526-1530): one rounding ->
    ``+ r``, :func:`widen`, then the bf16 check (:func:`add_split`).

  Both are legitimate and both are modelled; the case tables say which path a case takes.
* BN statistics (``stats``, with and without ``shift``) are checked against the kernel's OWN stored y: the reference
  is the fp64 sum of ``v = y - shift`` and of ``v*v`` over the M pixels, the bound ``2 * (M + 2) * u * sum|v|`` and
  the same form with ``v*v`` (:func:`stats_iv`): M adds, the subtraction and the square, any order, any tile.  The
  fp64 replica atomics add nothing that matters.  A column whose y is all zero and shift 0 is exact.
* Channel padding (``Cw < C``) is exactly zero in a DGRAD output; filters beyond ``Ow`` stay untouched in a WGRAD
  output (marker pattern, bit for bit); every split-K and WGRAD workspace is NaN-filled before the call.

Case tables.  One readable row per case: shape ``(N, H, W, C, O, R, stride, pad)``, the call variant, and ``launches``:
what the planner does with it at 256 CUs -- kernel instantiation, grid z (the split count), K steps per split, the
reduce kernel and its split count -- in the notation of :func:`launch_labels`.  tests/test_conv_check.py runs
tests/dispatch_recorder.hip over the tables and asserts every label, so a row cannot claim a route it does not take.
``why`` says what the row is there for.  Finite inputs only.
"""
import functools
import re
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from zoo_check import U, around, bf16_rne, draw, inside, widen  # noqa: F401  (U, draw: re-exported for the tests)

F64 = np.float64


# ---------------------------------------------------------------------------------------------------------------
# fp64 references (torch CPU) -- NHWC activations, PyTorch weight layouts
# ---------------------------------------------------------------------------------------------------------------
def out_hw(H, W, R, st, pad):
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F64))


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _both(f, a, b):
    return f(a, b), f(a.abs(), b.abs())


def fwd_ref(x, w, st, pad, groups=1):
    """y[N,P,Q,O] of x[N,H,W,C >= Cw*groups] and w[O,Cw,R,S]: (exact, sum |terms|)."""
    Cw = w.shape[1] * groups
    y, ya = _both(lambda a, b: F.conv2d(a, b, stride=st, padding=pad, groups=groups), _nchw(x[..., :Cw]), _t(w))
    return _nhwc(y), _nhwc(ya)


def dgrad_ref(dy, w, x_shape, st, pad, groups=1):
    """dx[N,H,W,Cw*groups] of dy[N,P,Q,O] and w[O,Cw,R,S]."""
    N, H, W, _ = x_shape
    Cw = w.shape[1] * groups
    dx, dxa = _both(lambda g, b: torch.nn.grad.conv2d_input((N, Cw, H, W), b, g, stride=st, padding=pad, groups=groups),
                    _nchw(dy), _t(w))
    return _nhwc(dx), _nhwc(dxa)


def wgrad_ref(x, dy, R, st, pad, Cw=None, groups=1):
    """dw[O,Cw,R,R] of x[N,H,W,C] and dy[N,P,Q,O]; groups > 1 (only with ``groups=C``, depthwise): Cw = 1."""
    C, O = x.shape[3], dy.shape[3]
    Cw = (C if Cw is None else Cw) if groups == 1 else C // groups
    dw, dwa = _both(lambda a, g: torch.nn.grad.conv2d_weight(a, (O, Cw, R, R), g, stride=st, padding=pad, groups=groups),
                    _nchw(x[..., :Cw * groups]), _nchw(dy))
    return dw.numpy(), dwa.numpy()


def wgrad_grouped(full, G, Cw):
    """The block-diagonal read of a densified grouped conv: filter o keeps channels [g*Cw, (g+1)*Cw) of its group g."""
    O = full.shape[0]
    return np.stack([full[o, (o // (O // G)) * Cw:(o // (O // G) + 1) * Cw] for o in range(O)])


def dw_fwd_ref(x, w, st, pad):
    return fwd_ref(x, w, st, pad, groups=x.shape[3])


def dw_dgrad_ref(dy, w, x_shape, st, pad):
    return dgrad_ref(dy, w, x_shape, st, pad, groups=x_shape[3])


def dw_wgrad_ref(x, dy, R, st, pad):
    return wgrad_ref(x, dy, R, st, pad, groups=x.shape[3])


# ---- the same six operations as direct nested loops (numpy fp64): the conventions, independently of torch ------
def loop_fwd(x, w, st, pad):
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    N, H, W, _ = x.shape
    O, Cw, R, S = w.shape
    P, Q = out_hw(H, W, R, st, pad)
    y = np.zeros((N, P, Q, O))
    for n in range(N):
        for p in range(P):
            for q in range(Q):
                for r in range(R):
                    for s in range(S):
                        h, ww = p * st - pad + r, q * st - pad + s
                        if 0 <= h < H and 0 <= ww < W:
                            y[n, p, q] += w[:, :, r, s] @ x[n, h, ww, :Cw]
    return y


def loop_dgrad(dy, w, x_shape, st, pad):
    dy, w = np.asarray(dy, F64), np.asarray(w, F64)
    N, H, W, _ = x_shape
    O, Cw, R, S = w.shape
    _, P, Q, _ = dy.shape
    dx = np.zeros((N, H, W, Cw))
    for n in range(N):
        for p in range(P):
            for q in range(Q):
                for r in range(R):
                    for s in range(S):
                        h, ww = p * st - pad + r, q * st - pad + s
                        if 0 <= h < H and 0 <= ww < W:
                            dx[n, h, ww] += dy[n, p, q] @ w[:, :, r, s]
    return dx


def loop_wgrad(x, dy, R, st, pad, Cw):
    x, dy = np.asarray(x, F64), np.asarray(dy, F64)
    N, H, W, _ = x.shape
    _, P, Q, O = dy.shape
    dw = np.zeros((O, Cw, R, R))
    for n in range(N):
        for p in range(P):
            for q in range(Q):
                for r in range(R):
                    for s in range(R):
                        h, ww = p * st - pad + r, q * st - pad + s
                        if 0 <= h < H and 0 <= ww < W:
                            dw[:, :, r, s] += np.outer(dy[n, p, q], x[n, h, ww, :Cw])
    return dw


def loop_dw_fwd(x, w, st, pad):
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    N, H, W, C = x.shape
    R = w.shape[2]
    P, Q = out_hw(H, W, R, st, pad)
    y = np.zeros((N, P, Q, C))
    for n in range(N):
        for p in range(P):
            for q in range(Q):
                for r in range(R):
                    for s in range(R):
                        h, ww = p * st - pad + r, q * st - pad + s
                        if 0 <= h < H and 0 <= ww < W:
                            y[n, p, q] += w[:, 0, r, s] * x[n, h, ww]
    return y


def loop_dw_dgrad(dy, w, x_shape, st, pad):
    dy, w = np.asarray(dy, F64), np.asarray(w, F64)
    N, H, W, C = x_shape
    R = w.shape[2]
    _, P, Q, _ = dy.shape
    dx = np.zeros((N, H, W, C))
    for n in range(N):
        for p in range(P):
            for q in range(Q):
                for r in range(R):
                    for s in range(R):
                        h, ww = p * st - pad + r, q * st - pad + s
                        if 0 <= h < H and 0 <= ww < W:
                            dx[n, h, ww] += dy[n, p, q] * w[:, 0, r, s]
    return dx


def loop_dw_wgrad(x, dy, R, st, pad):
    x, dy = np.asarray(x, F64), np.asarray(dy, F64)
    N, H, W, C = x.shape
    _, P, Q, _ = dy.shape
    dw = np.zeros((C, 1, R, R))
    for n in range(N):
        for p in range(P):
            for q in range(Q):
                for r in range(R):
                    for s in range(R):
                        h, ww = p * st - pad + r, q * st - pad + s
                        if 0 <= h < H and 0 <= ww < W:
                            dw[:, 0, r, s] += dy[n, p, q] * x[n, h, ww]
    return dw


# ---------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------
def acc_iv(ref, terms, n, c):
    """n products accumulated in fp32 in any order and rounding direction, c further roundings."""
    return around(ref, terms, 2.0 * (np.asarray(n, F64) + c))


def add_unsplit(iv, r):
    """bf16(bf16(acc) + r): the unsplit tap / generic epilogues (the bf16 check rounds the second time)."""
    r = np.asarray(r, F64)
    return widen((bf16_rne(iv[0]) + r, bf16_rne(iv[1]) + r))


def add_split(iv, r):
    """bf16(sum + r): the split-K combine."""
    r = np.asarray(r, F64)
    return widen((iv[0] + r, iv[1] + r))


def add_path(iv, r, splits):
    return add_split(iv, r) if splits > 1 else add_unsplit(iv, r)


def stats_iv(y, shift=None):
    """Intervals of the per-channel sum and sum of squares of (y - shift) over the rows of the STORED y [..., O]."""
    v = np.asarray(y, F64).reshape(-1, np.shape(y)[-1])
    if shift is not None:
        v = v - np.asarray(shift, F64)
    k = 2.0 * (v.shape[0] + 2)
    return around(v.sum(0), np.abs(v).sum(0), k), around((v * v).sum(0), (v * v).sum(0), k)


def dgrad_taps(H, W, R, st, pad):
    """[1, H, W, 1]: how many filter taps reach each input pixel (its sub-pixel phase at stride 2)."""
    def per(n):
        return np.array([sum(1 for r in range(R) if (i + pad - r) % st == 0) for i in range(n)], F64)
    return np.outer(per(H), per(W))[None, :, :, None]


def outside(y, iv, bf16_out=False):
    """(count of elements outside, zoo_check.inside's worst (index, y, lo, hi) or None); a NaN is outside."""
    v, worst = inside(y, iv, bf16_out)
    if v == 0.0:
        return 0, None
    lo, hi = (bf16_rne(iv[0]), bf16_rne(iv[1])) if bf16_out else iv
    y = np.asarray(y, F64)
    bad = ~((y >= np.broadcast_to(lo, y.shape)) & (y <= np.broadcast_to(hi, y.shape)))
    if worst is None:                        # a non-finite output: point at the first one
        i = tuple(int(k) for k in np.argwhere(~np.isfinite(y))[0])
        worst = (i, float(y[i]), float(np.broadcast_to(lo, y.shape)[i]), float(np.broadcast_to(hi, y.shape)[i]))
    return int(bad.sum()), worst


def check(y, iv, bf16_out, what, tile=None):
    """Every element inside, or a message with the case, the worst element, the count and its tile."""
    n, worst = outside(y, iv, bf16_out)
    if n:
        where = tile(worst[0]) if tile is not None else ""
        raise AssertionError("%s: %d of %d outside; worst (index, y, lo, hi) = %s %s"
                             % (what, n, np.size(y), worst, where))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


# ---------------------------------------------------------------------------------------------------------------
# operands (stored values, seeded by readable keys)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_operands(key, shape, Cw):
    """x [N,H,W,C] (channels Cw.. zero), w [O,Cw,R,R] (bf16 values: the packed image holds them exactly),
    dy / res [N,P,Q,O], base [N,H,W,C] (an accumulate / add operand, zero in the channel pad), shift [O] fp32."""
    N, H, W, C, O, R, st, pad = shape
    P, Q = out_hw(H, W, R, st, pad)
    x = np.zeros((N, H, W, C), np.float32)
    x[..., :Cw] = draw((key, "x"), (N, H, W, Cw))
    base = np.zeros((N, H, W, C), np.float32)
    base[..., :Cw] = draw((key, "base"), (N, H, W, Cw))
    return dict(x=x, w=draw((key, "w"), (O, Cw, R, R), scale=(Cw * R * R) ** -0.5), dy=draw((key, "dy"), (N, P, Q, O)),
                res=draw((key, "res"), (N, P, Q, O)), base=base,
                shift=draw((key, "shift"), (O,), scale=0.1, bf16=False))


@functools.lru_cache(maxsize=None)
def dw_operands(key, shape):
    N, H, W, C, R, st = shape
    P, Q = out_hw(H, W, R, st, R // 2)
    return dict(x=draw((key, "x"), (N, H, W, C)), w=draw((key, "w"), (C, 1, R, R), scale=1.0 / R, bf16=False),
                dy=draw((key, "dy"), (N, P, Q, C)), shift=draw((key, "shift"), (C,), scale=0.1, bf16=False),
                base=draw((key, "base"), (C, 1, R, R), bf16=False))


@functools.lru_cache(maxsize=None)
def fwd_exact(key, shape, Cw):
    op = dense_operands(key, shape, Cw)
    return fwd_ref(op["x"], op["w"], shape[6], shape[7])


@functools.lru_cache(maxsize=None)
def dgrad_exact(key, shape, Cw):
    op = dense_operands(key, shape, Cw)
    return dgrad_ref(op["dy"], op["w"], shape[:4], shape[6], shape[7])


@functools.lru_cache(maxsize=None)
def wgrad_exact(key, shape):
    """Over all C stored channels (a case slices its Cw / group / Ow part)."""
    op = dense_operands(key, shape, shape[3])
    return wgrad_ref(op["x"], op["dy"], shape[5], shape[6], shape[7])


def fwd_interval(row, res=False):
    op = dense_operands(row.key, row.shape, row.Cw)
    y, ya = fwd_exact(row.key, row.shape, row.Cw)
    iv = acc_iv(y, ya, row.shape[5] ** 2 * row.Cw, row.splits)
    return add_path(iv, op["res"], row.splits) if res else iv


def dgrad_interval(row, variant="plain"):
    """[N,H,W,Cw]; variant 'acc' / 'add': + base on the path of the row."""
    N, H, W, C, O, R, st, pad = row.shape
    op = dense_operands(row.key, row.shape, row.Cw)
    dx, dxa = dgrad_exact(row.key, row.shape, row.Cw)
    iv = acc_iv(dx, dxa, dgrad_taps(H, W, R, st, pad) * O, row.splits)
    return add_path(iv, op["base"][..., :row.Cw], row.splits) if variant != "plain" else iv


def wgrad_interval(row, acc=False):
    """[Ow, Cw, R, R] of the row (its channel, group and filter slice); acc: + base with one more rounding."""
    N, H, W, C, O, R, st, pad = row.shape
    P, Q = out_hw(H, W, R, st, pad)
    dw, dwa = wgrad_exact(row.key, row.shape)
    if row.groups > 1:
        dw, dwa = wgrad_grouped(dw, row.groups, row.Cw), wgrad_grouped(dwa, row.groups, row.Cw)
    dw, dwa = dw[:row.Ow, :row.Cw], dwa[:row.Ow, :row.Cw]
    iv = acc_iv(dw, dwa, N * P * Q, 2)
    return widen((iv[0] + wgrad_base(row), iv[1] + wgrad_base(row))) if acc else iv


def wgrad_base(row):
    return draw((row.key, "dwbase"), (row.Ow, row.Cw, row.shape[5], row.shape[5]), bf16=False).astype(F64)


def dw_intervals(row):
    """fwd [N,P,Q,C] (bf16), dgrad [N,H,W,C] (bf16), wgrad [C,1,R,R] (fp32) and wgrad + base."""
    N, H, W, C, R, st = row.shape
    pad = R // 2
    P, Q = out_hw(H, W, R, st, pad)
    op = dw_operands(row.key, row.shape)
    dw, dwa = dw_wgrad_ref(op["x"], op["dy"], R, st, pad)
    wg = acc_iv(dw, dwa, N * P * Q, 2)
    return dict(fwd=acc_iv(*dw_fwd_ref(op["x"], op["w"], st, pad), 2 * R * R, 1),
                dgrad=acc_iv(*dw_dgrad_ref(op["dy"], op["w"], (N, H, W, C), st, pad), 2 * R * R, 1),
                wgrad=wg, wgrad_acc=widen((wg[0] + op["base"], wg[1] + op["base"])))


# ---------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------
TAP, TAPG = "conv_tap<64, 8, false>", "conv_tap<64, 8, true>"
PHASES = "conv_tap_phases<64, 8>"
COMBINE = "conv_splitk_reduce"

# key, shape (N,H,W,C,O,R,stride,pad), Cw, ws (a NaN workspace of exactly fd_ws_floats), splits (1: unsplit path),
# launches at 256 CUs, variants, why
Fwd = namedtuple("Fwd", "key shape Cw ws splits launches variants why")
_ALL = ("plain", "stats", "stats0", "res", "res+stats")      # stats: with shift; stats0: without
_NORES = ("plain", "stats")                                  # C % 64 != 0 or off the tap route: no fused residual

FWD = [
    Fwd("f_tap_m105", (3, 7, 5, 64, 64, 3, 1, 1), 64, False, 1, (TAP + " z=1 kps=9",), _ALL,
        "M = 105: one partial 128-row tile"),
    Fwd("f_tap_o72", (1, 13, 11, 64, 72, 3, 1, 1), 64, False, 1, (TAP + " z=1 kps=9",), _ALL,
        "M = 143: two M tiles, the second partial; O = 72: a partial second column tile"),
    Fwd("f_tap_1x1", (2, 5, 5, 64, 64, 1, 1, 0), 64, False, 1, (TAP + " z=1 kps=1",), _ALL, "1x1: a single K step"),
    Fwd("f_tap_5x5s2", (2, 9, 9, 64, 8, 5, 2, 2), 64, False, 1, (TAP + " z=1 kps=25",), _ALL, "5x5 stride 2, O = 8"),
    Fwd("f_tap_5x5s2_split", (2, 9, 9, 64, 8, 5, 2, 2), 64, True, 3, (TAP + " z=3 kps=9", COMBINE + " z=3"), _ALL,
        "25 steps in splits of 9, 9, 7: the last split shorter"),
    Fwd("f_tap_64taps", (1, 10, 10, 64, 8, 8, 1, 3), 64, False, 1, (TAP + " z=1 kps=64",), _ALL,
        "64 taps: the last bit of the tap mask"),
    Fwd("f_tap_64taps_split", (1, 10, 10, 64, 8, 8, 1, 3), 64, True, 8, (TAP + " z=8 kps=8", COMBINE + " z=8"), _ALL,
        "64 taps in 8 splits of one filter row each"),
    Fwd("f_gen_81taps", (1, 10, 10, 64, 8, 9, 1, 4), 64, False, 1, ("conv_igemm<0, 64, 64> z=1 kps=81",), _NORES,
        "81 taps do not fit the tap mask: the generic implicit GEMM"),
    Fwd("f_gen_81taps_split", (1, 10, 10, 64, 8, 9, 1, 4), 64, True, 9,
        ("conv_igemm<0, 64, 64> z=9 kps=9", COMBINE + " z=9"), _NORES, "the generic kernel's split-K partials"),
    Fwd("f_tapg_3x3", (2, 6, 6, 16, 24, 3, 1, 1), 16, False, 1, (TAPG + " z=1 kps=3",), _NORES,
        "GEN: four taps of 16 channels per K step, K tail 144 - 128"),
    Fwd("f_tapg_k16", (2, 6, 6, 16, 24, 1, 1, 0), 16, False, 1, (TAPG + " z=1 kps=1",), _NORES,
        "K = 16: one masked K step"),
    Fwd("f_tapg_c72", (2, 5, 5, 72, 24, 3, 1, 1), 72, False, 1, (TAPG + " z=1 kps=11",), _NORES,
        "C = 72: a tap crosses a 64-channel chunk"),
    Fwd("f_split_2x9", (1, 4, 4, 128, 64, 3, 1, 1), 128, True, 2, (TAP + " z=2 kps=9", COMBINE + " z=2"), _ALL,
        "2 splits of 9 steps"),
    Fwd("f_split_9_8", (1, 4, 4, 1088, 64, 1, 1, 0), 1088, True, 2, (TAP + " z=2 kps=9", COMBINE + " z=2"), _ALL,
        "17 steps: splits of 9 and 8"),
    Fwd("f_split_12", (2, 2, 2, 256, 256, 5, 1, 2), 256, True, 12, (TAP + " z=12 kps=9", COMBINE + " z=12"), _ALL,
        "100 steps: 12 splits, the last a single step; four column tiles"),
    Fwd("f_split_gen", (16, 4, 4, 160, 320, 3, 1, 1), 160, True, 2, (TAPG + " z=2 kps=12", COMBINE + " z=2"), _NORES,
        "GEN with splits (12 + 11 steps), a 22-block combine"),
    Fwd("f_stem32", (3, 7, 5, 8, 32, 3, 1, 1), 3, False, 1, ("conv_stem_kernel<2> z=1",), _NORES,
        "stem, O = 32, M = 105 not a multiple of 16"),
    Fwd("f_stem64", (3, 7, 5, 8, 64, 3, 1, 1), 3, False, 1, ("conv_stem_kernel<4> z=1",), _NORES, "stem, O = 64"),
    Fwd("f_c8_s2", (2, 5, 5, 8, 72, 3, 2, 1), 3, False, 1, ("conv_igemm<0, 64, 128> z=1 kps=2",), _NORES,
        "C = 8 off the stem pattern: 64 x 128 tile with an N tail (72), K tail 72 - 64"),
    Fwd("f_c8_1x1", (2, 8, 8, 8, 24, 1, 1, 0), 3, False, 1, ("conv_igemm<0, 64, 64> z=1 kps=1",), _NORES,
        "C = 8, 1x1: K = 8, two row tiles"),
]

# wd: with the DGRAD weight image (the tap routes); launches: the record of dgrad.wd{0,1}.exact
Dgrad = namedtuple("Dgrad", "key shape Cw wd splits launches variants why")
_IG = "conv_igemm<1, 64, 64>"
_P = ("plain",)
_PA = ("plain", "acc")            # accumulate=True into a drawn base
_PAA = ("plain", "acc", "add")    # and add= (tap path, conv.dgrad_fusable)

DGRAD = [
    Dgrad("d_tap", (3, 7, 5, 64, 64, 3, 1, 1), 64, True, 1, (TAP + " z=1 kps=9",), _PAA, "stride 1 on conv_tap"),
    Dgrad("d_tap_nowd", (3, 7, 5, 64, 64, 3, 1, 1), 64, False, 1, (_IG + " z=1 kps=9",), _PA,
          "the generic kernel; accumulate is its partial & 2 epilogue"),
    Dgrad("d_tapg", (1, 13, 11, 64, 72, 3, 1, 1), 64, True, 1, (TAPG + " z=1 kps=11",), _PAA,
          "O = 72 input channels of dY: GEN, a tap crosses a chunk"),
    Dgrad("d_tapg_nowd", (1, 13, 11, 64, 72, 3, 1, 1), 64, False, 1, (_IG + " z=1 kps=11",), _P, "generic, K tail 648 - 640"),
    Dgrad("d_c3of8", (3, 7, 5, 8, 64, 3, 1, 1), 3, True, 1, (TAP + " z=1 kps=9",), _P,
          "Cw = 3 of 8: the channel pad of dx is exactly zero"),
    Dgrad("d_c3of8_nowd", (3, 7, 5, 8, 64, 3, 1, 1), 3, False, 1, (_IG + " z=1 kps=9",), _P, "the same on the generic kernel"),
    Dgrad("d_ph_odd", (3, 7, 5, 64, 64, 3, 2, 1), 64, True, 1, (PHASES + " z=1 phases=4 splits=1,1,1,1",), _PAA,
          "stride 2, odd H and W: four parities of different sizes"),
    Dgrad("d_ph_odd_nowd", (3, 7, 5, 64, 64, 3, 2, 1), 64, False, 1,
          (_IG + " z=1 kps=1", _IG + " z=1 kps=2", _IG + " z=1 kps=2", _IG + " z=1 kps=4"), _PA,
          "one generic launch per parity (1, 2, 2 and 4 taps)"),
    Dgrad("d_ph_2x2", (2, 6, 6, 64, 64, 2, 2, 0), 64, True, 1, (PHASES + " z=1 phases=4 splits=1,1,1,1",), _P,
          "one tap per parity, pad 0"),
    Dgrad("d_ph_2x2_nowd", (2, 6, 6, 64, 64, 2, 2, 0), 64, False, 1, (_IG + " z=1 kps=1",) * 4, _P, "generic"),
    Dgrad("d_ph_5x5", (2, 9, 11, 16, 64, 5, 2, 2), 16, True, 1, (PHASES + " z=1 phases=4 splits=1,1,1,1",), _P,
          "5x5 stride 2: 9, 6, 6 and 4 taps; C = 16 output columns"),
    Dgrad("d_ph_5x5_nowd", (2, 9, 11, 16, 64, 5, 2, 2), 16, False, 1,
          (_IG + " z=1 kps=9", _IG + " z=1 kps=6", _IG + " z=1 kps=6", _IG + " z=1 kps=4"), _P, "generic"),
    Dgrad("d_ph_4x4", (2, 8, 8, 64, 64, 4, 2, 1), 64, True, 1, (PHASES + " z=1 phases=4 splits=1,1,1,1",), _P,
          "4x4 filter, pad 1: four taps per parity"),
    Dgrad("d_ph_4x4_nowd", (2, 8, 8, 64, 64, 4, 2, 1), 64, False, 1, (_IG + " z=1 kps=4",) * 4, _P, "generic"),
    Dgrad("d_ph_1x1", (4, 9, 9, 64, 128, 1, 2, 0), 64, True, 1, (PHASES + " z=1 phases=4 splits=1,1,1,1",), _PA,
          "1x1 stride 2: three tap-less parities -- exactly zero, or the base bit for bit"),
    Dgrad("d_ph_1x1_nowd", (4, 9, 9, 64, 128, 1, 2, 0), 64, False, 1,
          (_IG + " z=1 kps=2", _IG + " z=1 kps=1", _IG + " z=1 kps=1", _IG + " z=1 kps=1"), _PA, "generic"),
    Dgrad("d_ph_two", (1, 1, 8, 64, 64, 3, 2, 1), 64, True, 1, (PHASES + " z=1 phases=2 splits=1,1",), _P,
          "H = 1: two phases"),
    Dgrad("d_ph_two_nowd", (1, 1, 8, 64, 64, 3, 2, 1), 64, False, 1, (_IG + " z=1 kps=1", _IG + " z=1 kps=2"), _P,
          "generic: two launches"),
    Dgrad("d_ph_one", (1, 1, 1, 64, 64, 3, 2, 1), 64, True, 1, (TAP + " z=1 kps=1 rowmap",), _P,
          "one pixel: one phase, a plain conv_tap launch with the row map on"),
    Dgrad("d_ph_one_nowd", (1, 1, 1, 64, 64, 3, 2, 1), 64, False, 1, (_IG + " z=1 kps=1",), _P, "generic: one launch"),
    Dgrad("d_split2", (1, 8, 16, 64, 128, 3, 1, 1), 64, True, 2, (TAP + " z=2 kps=9", COMBINE + " z=2"), _PAA,
          "18 steps in 2 splits, a four-block combine"),
    Dgrad("d_split2_nowd", (1, 8, 16, 64, 128, 3, 1, 1), 64, False, 2, (_IG + " z=2 kps=9", COMBINE + " z=2"), _PA,
          "the same on the generic kernel"),
    Dgrad("d_split9", (2, 2, 2, 128, 512, 3, 1, 1), 128, True, 9, (TAP + " z=9 kps=8", COMBINE + " z=9"), _PAA,
          "72 steps in 9 splits on conv_tap"),
    Dgrad("d_split9_nowd", (2, 2, 2, 128, 512, 3, 1, 1), 128, False, 9,
          ("conv_igemm<1, 64, 128> z=9 kps=8", COMBINE + " z=9"), _PA, "9 splits on the generic kernel"),
    Dgrad("d_ph_split", (2, 4, 4, 64, 128, 5, 2, 2), 64, True, 2, (PHASES + " z=2 phases=4 splits=2,1,1,1", COMBINE + " z=2"),
          _P, "the 9-tap phase of four split, inside one launch"),
    Dgrad("d_ph_split_nowd", (2, 4, 4, 64, 128, 5, 2, 2), 64, False, 2,
          (_IG + " z=2 kps=9", COMBINE + " z=2", _IG + " z=1 kps=12", _IG + " z=1 kps=12", _IG + " z=1 kps=8"), _P,
          "generic: the first parity split"),
    Dgrad("d_gen_s2_o24", (2, 6, 6, 24, 24, 3, 2, 1), 24, False, 1,
          (_IG + " z=1 kps=1", _IG + " z=1 kps=1", _IG + " z=1 kps=1", _IG + " z=1 kps=2"), _P,
          "stride 2 with O % 64 != 0: no tap route, K = 24 .. 96"),
]

# splits: the explicit argument (0: automatic); lib: lib_gemm; launches: wgrad.auto.1x1_{lib}.exact, wgrad.splits1,
# wgrad.splits7, or for another explicit count the splits7 kernel with split_k's answer (see test_conv_check.py).
# Every row runs with accumulate off and on.
Wgrad = namedtuple("Wgrad", "key shape Cw Ow groups splits lib launches why")
_RC, _RT = "conv_wgrad_reduce_cols", "conv_wgrad_reduce"
_W64, _W128, _WBIG = "conv_igemm<2, 64, 64>", "conv_igemm<2, 64, 128>", "conv_igemm<2, 128, 128>"
_H3, _H1 = "conv_wgrad_halo<3>", "conv_wgrad_halo<1>"


def _wg(key, shape, launches, why, Cw=None, Ow=None, groups=1, splits=0, lib=False):
    return Wgrad(key, shape, shape[3] if Cw is None else Cw, shape[4] if Ow is None else Ow, groups, splits, lib,
                 launches, why)


WGRAD = [
    _wg("wg_64x64", (2, 6, 6, 16, 24, 1, 1, 0), (_W64 + " z=1 kps=2", _RC + " splits=1"),
        "64 x 64 tile; 72 pixels: one K step and a tail of 8"),
    _wg("wg_64x128", (3, 7, 5, 64, 64, 3, 1, 1), (_W128 + " z=1 kps=2", _RC + " splits=1"), "64 x 128 tile, 105 pixels"),
    _wg("wg_64x128_s1", (3, 7, 5, 64, 64, 3, 1, 1), (_W128 + " z=1 kps=2", _RC + " splits=1"), "splits=1", splits=1),
    _wg("wg_64x128_s7", (3, 7, 5, 64, 64, 3, 1, 1), (_W128 + " z=2 kps=1", _RC + " splits=2"),
        "splits=7 over 2 K steps: clamped to 2", splits=7),
    _wg("wg_s2", (3, 7, 5, 64, 64, 3, 2, 1), (_W128 + " z=1 kps=1", _RC + " splits=1"), "stride 2: 36 pixels"),
    _wg("wg_1px", (1, 1, 1, 64, 64, 1, 1, 0), (_W64 + " z=1 kps=1", _RC + " splits=1"), "one pixel"),
    _wg("wg_tiled9", (2, 2, 2, 128, 512, 3, 1, 1), (_WBIG + " z=1 kps=1", _RT + " splits=1"),
        "128 x 128 tile; tiled reduce, the RS <= 9 path"),
    _wg("wg_tiled25", (2, 2, 2, 256, 256, 5, 1, 2), (_WBIG + " z=1 kps=1", _RT + " splits=1"),
        "tiled reduce, RS = 25: the general loop"),
    _wg("wg_tiled_s13", (13, 8, 8, 64, 1024, 1, 1, 0), (_W64 + " z=13 kps=1", _RT + " splits=13"),
        "tiled reduce with 13 splits: the general loop's four-load step", splits=13),
    _wg("wg_s7_short", (1, 32, 32, 64, 64, 3, 1, 1), (_W128 + " z=6 kps=3", _RC + " splits=6"),
        "splits=7 over 16 K steps: 6 splits of 3, the last a single step", splits=7),
    _wg("wg_c3of8", (3, 7, 5, 8, 32, 3, 1, 1), (_W128 + " z=1 kps=2", _RC + " splits=1"), "Cw = 3 of 8", Cw=3),
    _wg("wg_c20of24", (2, 6, 6, 24, 24, 3, 1, 1), (_W128 + " z=1 kps=2", _RC + " splits=1"), "Cw = 20 of 24", Cw=20),
    _wg("wg_ow20", (2, 6, 6, 16, 24, 3, 1, 1), (_W128 + " z=1 kps=2", _RC + " splits=1"),
        "Ow = 20 of 24: filters 20.. of the buffer keep their marker", Ow=20),
    _wg("wg_ow_tiled", (2, 2, 2, 128, 512, 3, 1, 1), (_WBIG + " z=1 kps=1", _RT + " splits=1"), "Ow = 500 of 512, tiled reduce",
        Ow=500),
    _wg("wg_g2_cols", (2, 6, 6, 16, 24, 3, 1, 1), (_W128 + " z=1 kps=2", _RC + " splits=1"), "2 groups of 8 channels", Cw=8,
        groups=2),
    _wg("wg_g4_cols", (2, 6, 6, 16, 24, 3, 1, 1), (_W128 + " z=1 kps=2", _RC + " splits=1"), "4 groups of 4 channels", Cw=4,
        groups=4),
    _wg("wg_g2_tiled", (2, 2, 2, 128, 512, 3, 1, 1), (_WBIG + " z=1 kps=1", _RT + " splits=1"), "2 groups, tiled reduce", Cw=64,
        groups=2),
    _wg("wg_g4_tiled", (2, 2, 2, 128, 512, 3, 1, 1), (_WBIG + " z=1 kps=1", _RT + " splits=1"), "4 groups, tiled reduce", Cw=32,
        groups=4),
    _wg("wg_7x7", (2, 6, 6, 16, 24, 7, 1, 3), (_W128 + " z=1 kps=2", _RC + " splits=1"), "a 7x7 window is accepted"),
    _wg("wg_halo", (2, 8, 8, 64, 64, 3, 1, 1), (_H3 + " z=1 kps=1", _RC + " splits=1"),
        "halo 3x3: one 128-pixel block of two images"),
    _wg("wg_halo_w16", (1, 8, 16, 64, 128, 3, 1, 1), (_H3 + " z=1 kps=1", _RC + " splits=1"), "halo: W = 16, two filter tiles"),
    _wg("wg_halo_c128", (1, 16, 8, 128, 64, 3, 1, 1), (_H3 + " z=1 kps=1", _RC + " splits=1"), "halo: two channel chunks"),
    _wg("wg_halo_8", (1, 32, 32, 64, 64, 3, 1, 1), (_H3 + " z=8 kps=1", _RC + " splits=8"),
        "halo: 8 splits, a 204-row window against the limit of 208"),
    _wg("wg_halo_miss_4x4", (8, 4, 4, 64, 64, 3, 1, 1), (_W128 + " z=1 kps=2", _RC + " splits=1"),
        "halo near miss (a 288-row window): generic"),
    _wg("wg_halo_miss_m192", (3, 8, 8, 64, 64, 3, 1, 1), (_W128 + " z=1 kps=3", _RC + " splits=1"),
        "halo near miss (M = 192): generic"),
    _wg("wg_halo_1x1", (17, 8, 16, 64, 64, 1, 1, 0), (_H1 + " z=17 kps=1", _RC + " splits=17"),
        "halo 1x1 route (lib_gemm=True with WGRAD_GEMM_PIXELS = 0): 17 splits", lib=True),
]
WGRAD_8X8 = _wg("wg_8x8", (2, 6, 6, 16, 24, 8, 1, 3), (_W128 + " z=1 kps=1", "throw: conv_wgrad: window larger than 7x7"),
                "an 8x8 window raises")
WGRAD_DEFERRED = ("wg_tiled25", "wg_s7_short", "wg_g2_cols")      # one wgrad_reduce_multi: tiled, columns, grouped


def split_k(ksteps, want):
    """conv_plan.h split_k: (K steps per split, splits)."""
    sp = max(1, min(want, ksteps))
    kps = max(1, -(-ksteps // sp))
    return kps, max(1, -(-ksteps // kps))


# (N, H, W, C, R, stride), pad = R // 2; nblk: partial blocks of the WGRAD (dwconv_ws_floats / (C R R)); every row runs
# forward (plain, statistics with shift: sum and sum of squares), DGRAD and WGRAD (accumulate off / on)
Dw = namedtuple("Dw", "key shape nblk why")
DW = [
    Dw("dw_3s1_odd", (3, 7, 7, 64, 3, 1), 3, "dw_fwd3<1>, dw_dgrad3s1 and the pair WGRAD with an odd width; 3 partial blocks"),
    Dw("dw_3s2_odd", (2, 9, 9, 32, 3, 2), 1, "dw_fwd3<2> with an odd output width, dw_dgrad3s2 with odd H and W"),
    Dw("dw_5s2_c24", (2, 9, 9, 24, 5, 2), 1, "generic forward / DGRAD / WGRAD, 5x5 stride 2; C/8 = 3 does not divide 256"),
    Dw("dw_7_c40", (2, 8, 8, 40, 7, 1), 2, "7x7; C/8 = 5"),
    Dw("dw_c296", (2, 5, 5, 296, 3, 1), 1, "C/8 = 37, prime above 32: the WGRAD chunk width falls to 1"),
    Dw("dw_c296_s2", (2, 5, 5, 296, 3, 2), 1, "the same on the generic WGRAD"),
    Dw("dw_c2048", (1, 2, 2, 2048, 3, 1), 1, "C = 2048 on a 2x2 image"),
    Dw("dw_blocks96", (3, 16, 32, 256, 3, 1), 96, "96 partial blocks: the unrolled loop of wred_dw_body"),
    Dw("dw_blocks18_gen", (2, 24, 24, 256, 3, 2), 18, "generic 3x3 WGRAD at stride 2, 18 partial blocks"),
]
DW_DEFERRED = ("dw_3s1_odd", "dw_blocks96")


def dw_blocks(shape):
    """dwconv.hip dw_wgrad_blocks."""
    N, H, W, C, R, st = shape
    P, Q = out_hw(H, W, R, st, R // 2)
    vc = C // 8
    vcb = next((d for d in range(min(vc, 32), 1, -1) if vc % d == 0), 1)
    pstep = (256 // vcb * vcb) // vcb
    pair = R == 3 and st == 1
    npix = N * P * ((Q + 1) // 2) if pair else N * P * Q
    per = pstep * (1 if pair else 2)
    return max(1, min(512, -(-npix // per)))


# ---------------------------------------------------------------------------------------------------------------
# the dispatch recorder's text -> labels
# ---------------------------------------------------------------------------------------------------------------
def parse_record(text):
    """{(N,H,W,C,O,R,st,pad): {variant: [launch line, ...], 'ws': the workspace / fusable line}} of
    dispatch_recorder's output ('a == b' resolved)."""
    rec = {}
    for block in text.split("shape ")[1:]:
        lines = block.splitlines()
        shape = tuple(int(v) for v in lines[0].split())
        variants, cur = {"ws": lines[1].strip()}, None
        for ln in lines[2:]:
            if ln.startswith("  "):
                variants[cur].append(ln.strip())
            elif " == " in ln:
                a, b = ln.strip().split(" == ")
                variants[a] = variants[b]
            else:
                cur = ln.strip()
                variants[cur] = []
        rec[shape] = variants
    return rec


def launch_labels(lines):
    """A variant's launches in the tables' notation: 'kernel z=<grid z> kps=<K steps per split>[ rowmap]',
    'conv_tap_phases<..> z= phases= splits=<per phase>', 'conv_splitk_reduce z=<splits>',
    'conv_wgrad_reduce[_cols] splits=', 'throw: ...'."""
    out = []
    for ln in lines:
        if ln.startswith("throw"):
            out.append(ln)
            continue
        name = ln.split(" g=")[0]
        z = re.search(r" g=\d+,\d+,(\d+)", ln).group(1)
        args = ln.split("|", 1)[1]
        if name.startswith("conv_igemm"):
            out.append("%s z=%s kps=%s" % (name, z, args.rsplit("]", 1)[1].split()[0]))
        elif name.startswith("conv_tap<"):
            m = re.search(r"\] (RM0|RM\[[^\]]*\]) (\d+) ", args)
            out.append("%s z=%s kps=%s%s" % (name, z, m.group(2), "" if m.group(1) == "RM0" else " rowmap"))
        elif name.startswith("conv_tap_phases"):
            n = re.search(r"TM\[ n=(\d+)", args).group(1)
            sp = [g.split()[-2] for g in re.findall(r"\{([^}]*)\}", args)]
            out.append("%s z=%s phases=%s splits=%s" % (name, z, n, ",".join(sp)))
        elif name.startswith("conv_wgrad_halo"):
            out.append("%s z=%s kps=%s" % (name, z, args.rsplit("]", 1)[1].split()[0]))
        elif name == COMBINE:
            out.append("%s z=%s" % (name, args.split()[1]))
        elif name.startswith("conv_wgrad_reduce"):
            out.append("%s splits=%s" % (name, args.split()[1]))
        else:
            out.append("%s z=%s" % (name, z))
    return tuple(out)


def kernels_of(labels):
    return {lb.split(" z=")[0].split(" splits=")[0] for lb in labels if not lb.startswith("throw")}


def tile_of(label, shape_out):
    """index -> '(M tile, N tile) of <kernel>' for a dense [.., rows.., NC] output of the launch ``label``."""
    name = label.split(" z=")[0]
    m = re.match(r"conv_igemm<\d, (\d+), (\d+)>", name)
    bm, bn = (int(m.group(1)), int(m.group(2))) if m else (16, 64) if name.startswith("conv_stem") else \
        (128, int(re.match(r"conv_tap\w*<(\d+)", name).group(1)))

    def f(idx):
        row = int(np.ravel_multi_index(idx[:-1], shape_out[:-1]))
        return "(row %d: M tile %d of %d rows, N tile %d of %d columns, %s; every split adds to every element)" % (
            row, row // bm, bm, idx[-1] // bn, bn, label)
    return f
