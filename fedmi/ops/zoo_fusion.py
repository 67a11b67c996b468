"""Results of the native aten backend whose pass has not run yet -- the state of its peephole fusions.

A producer impl (:mod:`fedmi.ops.native_mode`) hands the mode a pending result instead of launching its pass:

* ``joins(func, args, kwargs)``: what the consumer needs (the partner tensor, or ``True``) when the op
  ``func(*args)`` will consume this result, else ``None``.  Each join condition is written here, once: the mode
  asks it before the op runs and hands the answer to the consuming impl.
* ``materialize()``: run the pass as if nothing had fused (``order``: the rank among several before one op).

A consumed result leaves a tensor nobody wrote: it waits in the mode's map of deferred tensors until something
reads that tensor.  :class:`_PendingSliceBwd` is deferred from the start.
"""
import torch

from . import zoo_launch as ZL
from .zoo_launch import (EW_ADDS, EW_BNB, EW_BNB_ADD, EW_BNB_THR, EW_BNB_THR_ADD, EW_COPY, EW_FMA, EW_FMA_ADD,
                         EW_FMA_ADD_RELU, EW_FMA_RELU, EW_MUL, EW_THR_BWD, _same, _same_geom)

aten = torch.ops.aten

_BN_FWD = (aten.native_batch_norm.default, aten.miopen_batch_norm.default)


def _add_partner(out, args, kwargs):
    """The other operand of ``add(a, b)`` / ``a.add_(b)`` when one operand is the unwritten ``out`` (plain sum of
    two distinct tensors of one dtype); else None."""
    if len(args) != 2 or kwargs.get("alpha", 1) != 1:
        return None
    a, b = args
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
        return None
    o = b if _same(a, out) else a if _same(b, out) else None
    if o is None or _same(o, out) or o.dtype != out.dtype:
        return None
    return o


class _PendingCtr:
    """BatchNorm's ``num_batches_tracked += 1`` not applied yet: the BN forward that follows bumps the counter in
    its finalizing workgroup."""
    __slots__ = ("t",)
    order = 0

    def __init__(self, t):
        self.t = t

    def joins(self, func, args, kwargs):
        return True if func in _BN_FWD else None

    def materialize(self):
        ZL.ew(self.t, [self.t], EW_ADDS, 1.0)


class _PendingMul:
    """a * b (same shapes) not computed yet: if the next op sums it over some dims (autograd's backward of a
    broadcast multiply -- the SE gate's gradient), the product is folded into that reduction (RD_DOT_SHIFT,
    no shift) and never stored; any other op materialises it."""
    __slots__ = ("out", "a", "b")
    order = 1

    def __init__(self, out, a, b):
        self.out, self.a, self.b = out, a, b

    def joins(self, func, args, kwargs):
        return True if func in (aten.sum.dim_IntList, aten.mean.dim) and args and _same(args[0], self.out) else None

    def materialize(self):
        ZL.ew(self.out, [self.a, self.b], EW_MUL)


class _PendingBNB:
    """A BatchNorm input gradient whose apply pass has not run: when autograd next sums it with the tensor's
    other incoming gradient (DenseNet: the concat's slice; residual nets: the shortcut), the sum joins the
    pass (EW_BNB[_THR]_ADD, the gradient rounded as the unfused pair stores it); any other op materialises it."""
    __slots__ = ("out", "ins", "thr")
    order = 2

    def __init__(self, out, ins, thr):
        self.out, self.ins, self.thr = out, ins, thr

    def joins(self, func, args, kwargs):
        if func not in (aten.add.Tensor, aten.add_.Tensor):
            return None
        o = _add_partner(self.out, args, kwargs)
        return o if o is not None and o.shape == self.out.shape else None

    def materialize(self):
        ZL.ew(self.out, self.ins, EW_BNB_THR if len(self.ins) == 6 else EW_BNB, self.thr)

    def add(self, out, other):
        rnd = 1.0 if self.out.dtype == torch.bfloat16 else 0.0
        return ZL.ew(out, self.ins + [other], EW_BNB_THR_ADD if len(self.ins) == 6 else EW_BNB_ADD, self.thr, rnd)


class _PendingBN:
    """A BatchNorm output whose apply pass (x * scale + shift [+ res]) has not run yet: if the next op is
    a residual add of it (identity or projection shortcut), the add joins the pending pass; if the next
    op is its ReLU, everything becomes one pass (EW_FMA_RELU / EW_FMA_ADD_RELU); any other op
    materialises it first."""
    __slots__ = ("out", "x", "scale", "shift", "res")
    order = 3

    def __init__(self, out, x, scale, shift, res=None):
        self.out, self.x, self.scale, self.shift, self.res = out, x, scale, shift, res

    def joins(self, func, args, kwargs):
        if func in (aten.relu.default, aten.relu_.default):
            return True if args and _same(args[0], self.out) else None
        if func is not aten.add.Tensor or self.res is not None:
            return None
        o = _add_partner(self.out, args, kwargs)
        return o if o is not None and _same_geom(o, self.out) else None

    def inputs(self):
        return [self.x, self.scale, self.shift] + ([] if self.res is None else [self.res])

    def rounding(self) -> float:
        # the unfused BN stores its output before the add reads it: round there too (bit-identical results)
        return 1.0 if self.res is not None and self.out.dtype == torch.bfloat16 else 0.0

    def materialize(self):
        ZL.ew(self.out, self.inputs(), EW_FMA if self.res is None else EW_FMA_ADD, 0.0, self.rounding())

    def relu(self, out):
        return ZL.ew(out, self.inputs(), EW_FMA_RELU if self.res is None else EW_FMA_ADD_RELU, 0.0, self.rounding())


class _PendingThr:
    """threshold_backward(grad, relu_out) not yet computed: its consumer (BN backward) masks on the fly."""
    __slots__ = ("out", "grad", "relu_out", "thr")
    order = 4

    def __init__(self, out, grad, relu_out, thr):
        self.out, self.grad, self.relu_out, self.thr = out, grad, relu_out, thr

    def joins(self, func, args, kwargs):
        if func is aten.native_batch_norm_backward.default:
            g = args[0] if args else None
        elif func is aten.miopen_batch_norm_backward.default:
            g = args[1] if len(args) > 1 else None
        else:
            return None
        return True if _same(g, self.out) else None

    def materialize(self):
        ZL.ew(self.out, [self.grad, self.relu_out], EW_THR_BWD, self.thr)


class _PendingSliceBwd:
    """slice_backward not computed yet (zeros + the gradient in its slice): autograd's sum of two of them that
    tile the sliced dim (DPN's dual path: y[:, :d] and y[:, d:]) becomes two copies into one tensor -- no zero
    fills, no add pass; any other read materialises it."""
    __slots__ = ("out", "grad", "dim", "start", "end")

    def __init__(self, out, grad, dim, start, end):
        self.out, self.grad, self.dim, self.start, self.end = out, grad, dim, start, end

    def materialize(self):
        ZL.fill_(self.out, 0.0)
        ZL.ew(self.out.narrow(self.dim, self.start, self.end - self.start), [self.grad], EW_COPY)


def _sb_pair(dead, args, kwargs):
    """The two deferred slice_backwards (lower slice first) an ``add(a, b)`` sums when their slices tile the dim
    exactly, else None.  ``dead``: the mode's map of deferred tensors -- a slice gradient that something read was
    materialised and left the map, so it cannot pair."""
    if not dead or len(args) != 2 or kwargs.get("alpha", 1) != 1:
        return None
    a, b = args
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
        return None
    pa = dead.get(a.untyped_storage().data_ptr())
    pb = dead.get(b.untyped_storage().data_ptr())
    if (not (isinstance(pa, _PendingSliceBwd) and isinstance(pb, _PendingSliceBwd)) or pa is pb
            or not (_same(a, pa.out) and _same(b, pb.out)) or pa.dim != pb.dim):
        return None
    lo, hi = (pa, pb) if pa.start <= pb.start else (pb, pa)
    if lo.start != 0 or lo.end != hi.start or hi.end != pa.out.shape[pa.dim]:
        return None
    return lo, hi


class _CatBuf:
    """A reverse-filled concat buffer: NHWC [N, H, W, K], channels [front, K) live.  ``cat([y, x], 1)`` with x
    the live tail writes y in front of it and returns the longer tail -- x is never copied again (DenseNet's
    growing feature map, src/models/densenet.py:20-24: the reference copies the whole map per layer)."""
    __slots__ = ("buf", "front", "head")

    def __init__(self, buf, front, head):
        self.buf, self.front, self.head = buf, front, head

    def tail(self):
        return self.buf[..., self.front:].permute(0, 3, 1, 2)
