"""Launch planning for the zoo kernels (``zoo_ops.hip``): tensor descriptors, the coalescing of iteration
spaces, the vector / row-path eligibility tests, and the three launchers every op of the native aten backend is
built from -- :func:`ew` (elementwise with broadcasting), :func:`fill_` and :func:`reduce_sum`.

Nothing here knows an aten op: :mod:`fedmi.ops.zoo_fusion` (results whose pass is still pending) and
:mod:`fedmi.ops.native_mode` (the op table and the dispatch mode) build on it, in that order.
"""
import math
from typing import Optional

import torch

from .. import native

# dtype codes (zoo_ops.hip ZDtype)
_DT = {torch.float32: 0, torch.bfloat16: 1, torch.int64: 2}

# elementwise op codes (zoo_ops.hip EwOp)
EW_COPY, EW_ADD, EW_MUL, EW_MULS, EW_RELU, EW_THR_BWD, EW_SIGMOID, EW_SIG_BWD, EW_FILL, EW_FMA = range(10)
EW_BNB, EW_BERN, EW_SUB, EW_DIV, EW_ADDS, EW_FMA_RELU, EW_BNB_THR = 11, 12, 13, 14, 15, 16, 17
EW_FMA_ADD, EW_FMA_ADD_RELU, EW_BNB_ADD, EW_BNB_THR_ADD = 18, 19, 20, 21
# reduction op codes (zoo_ops.hip RdOp)
RD_SUM, RD_SUMSQ_SHIFT, RD_DOT_SHIFT, RD_DOT_R = 0, 1, 2, 3

_current = None     # the NativeMode whose block is running (its __enter__ / __exit__ set it), else None


def current_mode():
    return _current


def set_current_mode(mode):     # returns the mode it replaces
    global _current
    prev, _current = _current, mode
    return prev


def _nat():
    return native.require()


def _st(dev) -> int:
    return native.stream_handle(dev)


def zd(t: Optional[torch.Tensor]):
    """(ptr, dtype code, sizes, strides) descriptor of a CUDA tensor (None passes through)."""
    if t is None:
        return None
    if t.dtype not in _DT:
        raise TypeError(f"native_mode: unsupported dtype {t.dtype}")
    if t.numel() >= (1 << 31):
        raise ValueError("native_mode: tensors must have < 2^31 elements")
    if t.dim() == 0:
        return (t.data_ptr(), _DT[t.dtype], [1], [1])
    return (t.data_ptr(), _DT[t.dtype], list(t.shape), list(t.stride()))


def _bcast(t: torch.Tensor, shape) -> torch.Tensor:
    if tuple(t.shape) == tuple(shape):
        return t
    return t.expand(shape) if t.dim() == len(shape) else t.reshape((1,) * (len(shape) - t.dim()) + tuple(t.shape)).expand(shape)


def coalesce(shape, strides):
    """Merge the dims of an iteration space shared by several operands (``strides``: one stride list per
    operand, operand 0 decides the order): size-1 dims drop, dims are ordered by operand 0's strides and
    neighbours that are contiguous in EVERY operand merge -- a channels-last activation with a
    per-channel operand becomes [N*H*W, C], a pure elementwise op one flat dim."""
    dims = [d for d in range(len(shape)) if shape[d] != 1]
    if not dims:
        return [1], [[0] for _ in strides]
    dims.sort(key=lambda d: -abs(strides[0][d]))
    nshape = [shape[dims[0]]]
    nstr = [[s[dims[0]]] for s in strides]
    for d in dims[1:]:
        if all(ns[-1] == s[d] * shape[d] for ns, s in zip(nstr, strides)):
            nshape[-1] *= shape[d]
            for ns, s in zip(nstr, strides):
                ns[-1] = s[d]
        else:
            nshape.append(shape[d])
            for ns, s in zip(nstr, strides):
                ns.append(s[d])
    return nshape, nstr


def ew(out: torch.Tensor, ins, op: int, s0: float = 0.0, s1: float = 0.0, seed: int = 0, ctr=None) -> torch.Tensor:
    """out[...] = op(ins...) with broadcasting of every input to out's shape."""
    if out.numel() == 0:
        return out
    if out.numel() >= (1 << 31):
        raise ValueError("native_mode: tensors must have < 2^31 elements")
    shape = list(out.shape) if out.dim() else [1]
    o = out if out.dim() else out.view(1)
    ts = [_bcast(t if t.dim() else t.view(1), shape) for t in ins]
    for t in ts:
        if t.dtype not in _DT:
            raise TypeError(f"native_mode: unsupported dtype {t.dtype}")
    if op == EW_BERN:
        # the counter-based mask is a function of the logical element index: keep the logical order
        nshape, nstr = shape, [list(o.stride())] + [list(t.stride()) for t in ts]
    else:
        nshape, nstr = coalesce(shape, [list(o.stride())] + [list(t.stride()) for t in ts])
    allt = [o] + ts
    vw, vmask = 8, -1
    if op != EW_BERN:
        for vw in (8, 4):
            vmask = _vec_mask(nshape, nstr, allt, vw)
            if vmask >= 0:
                break
    if vmask >= 0:
        nshape = nshape[:-1] + [nshape[-1] // vw]
        nstr = [st[:-1] + [st[-1] * vw] for st in nstr]
    mode = _current
    if mode is not None and mode.diag:   # passes per op code, and which miss the vector launch
        mode.ew_ops[(mode._func_name(), op)] += 1
        if vmask < 0:
            mode.scalar_ew[(op, tuple(out.shape), tuple(out.stride()), tuple(tuple(t.stride()) for t in ts))] += 1
    descs = [(t.data_ptr(), _DT[t.dtype], nshape, st) for t, st in zip(allt, nstr)]
    _nat().z_ew(_st(out.device), descs[0], descs[1:], op, float(s0), float(s1), int(seed) & 0xFFFFFFFF,
                0 if ctr is None else ctr.data_ptr(), vmask, vw)
    return out


def _vec_mask(shape, strides, ts, vw: int = 8) -> int:
    """Bit k (input k) set if that operand is contiguous over groups of ``vw`` innermost elements, bit
    clear = a broadcast operand; -1 = the vector launch does not apply (odd sizes, misalignment,
    int64, an output that is not unit-stride innermost, fp32 with vw 4 below 16-byte alignment)."""
    if shape[-1] % vw:
        return -1
    mask = 0
    for k, (t, st) in enumerate(zip(ts, strides)):
        inner = st[-1]
        if inner == 0 and k > 0:
            continue
        align = 16 if (t.dtype == torch.float32 or vw == 8) else 8
        if inner != 1 or t.dtype == torch.int64 or t.data_ptr() % align or any(v % vw for v in st[:-1]):
            return -1
        if k > 0:
            mask |= 1 << (k - 1)
    return mask


def fill_(t: torch.Tensor, v: float) -> torch.Tensor:
    return ew(t, [], EW_FILL, v)


def _rowmajor_out(out: torch.Tensor) -> bool:
    """out's elements sit at their row-major index (size-1 dims ignored): a reduction can store into it by the
    accumulator index."""
    if out.dtype not in (torch.float32, torch.bfloat16):
        return False
    expect = 1
    for d in range(out.dim() - 1, -1, -1):
        if out.shape[d] == 1:
            continue
        if out.stride(d) != expect:
            return False
        expect *= out.shape[d]
    return True


def reduce_sum(a: torch.Tensor, dims, acc: Optional[torch.Tensor], op: int = RD_SUM, b: Optional[torch.Tensor] = None,
               shift: Optional[torch.Tensor] = None, acc2: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, scale: float = 1.0) -> None:
    """acc (fp32, ZEROED, one entry per kept element in order) += sum over ``dims`` of f(a[, b]); or, with
    ``out`` (RD_SUM, :func:`_rowmajor_out`), out = scale * sum stored directly (no zeroed accumulator, no copy:
    the bias gradients, spatial means of SE gates, sums of autograd's broadcast backward)."""
    dims = sorted(d % a.dim() for d in dims)
    kept = [d for d in range(a.dim()) if d not in dims]
    ops = [a] if b is None else [a, b]

    def space(ds, order_by_acc):
        if not ds:
            return [1], [[0] for _ in ops]
        shp = [a.shape[d] for d in ds]
        strs = [[t.stride(d) for d in ds] for t in ops]
        if order_by_acc:
            # kept dims: the accumulator index is row-major over them -- merge only, never reorder
            acc_str = [1] * len(ds)
            for j in range(len(ds) - 2, -1, -1):
                acc_str[j] = acc_str[j + 1] * shp[j + 1]
            ns, nst = coalesce(shp, [acc_str] + strs)
            return ns, nst[1:]
        return coalesce(shp, strs)

    oshape, ostr = space(kept, True)
    ishape, istr = space(dims, False)
    if op != RD_DOT_R and _rows_ok(oshape, ostr, ishape, istr, ops):
        # channels-last moments / bias gradients: [M, C] rows, 16-byte channel vectors, deterministic
        C, M = oshape[0], ishape[0]
        nat = _nat()
        part = torch.empty(int(nat.z_reduce_rows_ws_floats(M, C)), dtype=torch.float32, device=a.device)
        nat.z_reduce_rows(_st(a.device), a.data_ptr(), _DT[a.dtype], istr[0][0],
                          b.data_ptr() if b is not None else 0, _DT[b.dtype] if b is not None else 0,
                          istr[1][0] if b is not None else 0, shift.data_ptr() if shift is not None else 0, C, M, op,
                          part.data_ptr(), part.numel(), acc.data_ptr() if acc is not None else 0,
                          acc2.data_ptr() if acc2 is not None else 0, out.data_ptr() if out is not None else 0,
                          _DT[out.dtype] if out is not None else 0, float(scale))
        return
    outer = (0, 0, oshape, ostr[0])
    inner = (0, 0, ishape, istr[0])
    outer_b = (0, 0, oshape, ostr[1]) if b is not None else None
    inner_b = (0, 0, ishape, istr[1]) if b is not None else None
    nat = _nat()
    # split partials summed in a fixed order afterwards (no float atomics: bitwise-reproducible steps)
    nws = int(nat.z_reduce_ws_floats(math.prod(oshape), math.prod(ishape)))
    part = torch.empty(max(nws, 1), dtype=torch.float32, device=a.device)
    nat.z_reduce(_st(a.device), outer, inner, outer_b, inner_b, a.data_ptr(), _DT[a.dtype],
                 b.data_ptr() if b is not None else 0, _DT[b.dtype] if b is not None else 0,
                 shift.data_ptr() if shift is not None else 0, acc.data_ptr() if acc is not None else 0,
                 acc2.data_ptr() if acc2 is not None else 0, op, part.data_ptr(), nws,
                 out.data_ptr() if out is not None else 0, _DT[out.dtype] if out is not None else 0, float(scale))


def _rows_ok(oshape, ostr, ishape, istr, ops) -> bool:
    if len(oshape) != 1 or len(ishape) != 1 or oshape[0] % 4 or ishape[0] < 1:
        return False
    vw = 8 if oshape[0] % 8 == 0 else 4
    for t, os_, is_ in zip(ops, ostr, istr):
        align = 16 if (t.dtype == torch.float32 or vw == 8) else 8
        if os_[0] != 1 or is_[0] % vw or t.dtype not in (torch.float32, torch.bfloat16) or t.data_ptr() % align:
            return False
    return True


def _row_stride(t: torch.Tensor) -> Optional[int]:
    """Row stride (elements) when ``t`` [..., C] is evenly spaced rows of unit-stride channels (a compact tensor
    or a channel slice of one), else None."""
    if t.dim() < 2 or t.stride(-1) != 1:
        return None
    ld = expect = None
    for d in range(t.dim() - 2, -1, -1):
        if t.shape[d] == 1:
            continue
        if ld is None:
            ld, expect = t.stride(d), t.stride(d) * t.shape[d]
        elif t.stride(d) != expect:
            return None
        else:
            expect *= t.shape[d]
    return int(ld) if ld is not None else int(t.shape[-1])


def _rows_ld(t: torch.Tensor) -> Optional[int]:
    """Row stride (elements) when t is an [M, C] row matrix in memory -- channels-last 4-D or 2-D with unit-stride
    channels, compact or a channel slice of a wider one (a concat buffer's tail, a padded conv output's first C
    channels) -- with 16-B channel vectors (8-B for bf16 C % 8 != 0); else None."""
    if t.dim() == 4:
        ld = _row_stride(t.permute(0, 2, 3, 1))
    elif t.dim() == 2 and t.stride(1) == 1:
        ld = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    else:
        return None
    C = t.shape[1]
    if ld is None or C % 4 or ld < C or t.dtype not in (torch.float32, torch.bfloat16) or t.numel() == 0:
        return None
    align = 16 if (t.dtype == torch.float32 or C % 8 == 0) else 8
    if t.data_ptr() % align or (ld * t.element_size()) % align:
        return None
    return int(ld)


def _cl_rows(t: torch.Tensor) -> bool:
    return _rows_ld(t) is not None


def _same_geom(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.stride() == b.stride()


def _same(a, b) -> bool:
    return isinstance(a, torch.Tensor) and a.data_ptr() == b.data_ptr() and _same_geom(a, b) and a.dtype == b.dtype
