"""The dense conv kernels (csrc/kernels/conv_igemm.hip) and the depthwise ones (csrc/kernels/dwconv.hip) against the
fp64 interval references of tests/conv_check.py, over its case tables: every element of every output inside its
derived interval, bit for bit where the reference is exact (channel padding, tap-less parities, untouched filters,
deferred against immediate reductions).  The tables' routes are asserted on the CPU by tests/test_conv_check.py for
a 256-CU device; test_device_is_the_one_the_labels_were_recorded_for makes another device a visible failure.

Each check prints one figure (``pin <family> <case> <figure>``, with -s; see _margin) for
profiles/conv_pin/README.md; no test reads it.
"""
import numpy as np
import pytest
import torch

import conv_check as cc
from fedmi.ops import conv

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _bf(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).bfloat16().contiguous()


def _fp(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _np(t):
    return t.detach().to(torch.float64 if t.dtype == torch.float64 else torch.float32).cpu().numpy()


def _nan(shape, dtype, dev):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _margin(family, what, y, iv, bf16_out):
    """fp32 outputs: the worst |y - middle| in units of the interval's half width (<= 1 inside).  bf16 outputs: the
    share of elements whose interval holds ONE bf16 value (both ends round to it: y has no freedom left)."""
    lo, hi = (cc.bf16_rne(iv[0]), cc.bf16_rne(iv[1])) if bf16_out else iv
    lo, hi = np.broadcast_to(lo, y.shape), np.broadcast_to(hi, y.shape)
    half = (hi - lo) / 2
    ok = half > 0
    if bf16_out:
        fig = 1.0 - float(ok.mean())
    else:
        fig = float(np.max(np.abs(y - (lo + hi) / 2)[ok] / half[ok])) if ok.any() else 0.0
    print("pin %s %s %.3f" % (family, what, fig))


def _check(family, what, y, iv, bf16_out, tile=None):
    y = np.asarray(y, np.float64)
    cc.check(y, iv, bf16_out, what, tile)
    _margin(family, what, y, iv, bf16_out)


def _check_stats(family, what, rep, y, shift):
    got = _np(rep).sum(0)                                                    # [2, O] fp64 over the replicas
    iv1, iv2 = cc.stats_iv(y, shift)
    _check(family + "-stats", what + " sum", got[0], iv1, False)
    _check(family + "-stats", what + " sum of squares", got[1], iv2, False)


def test_device_is_the_one_the_labels_were_recorded_for():
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256


def _packed(w, C, dev):
    """The fp32 master on the device and its bf16 [O, R, S, C] image, which holds the drawn bf16 values exactly."""
    wt = _fp(w, dev)
    wr = conv.pack_weight(wt, c_pad=C, out=_nan((w.shape[0], w.shape[2], w.shape[3], C), torch.bfloat16, dev))
    img = np.zeros((w.shape[0], w.shape[2], w.shape[3], C), np.float32)
    img[..., :w.shape[1]] = w.transpose(0, 2, 3, 1)
    assert cc.bits_equal(_np(wr), img), "pack_weight"
    return wt, wr


FWD_CASES = [(r, v) for r in cc.FWD for v in r.variants]


@pytest.mark.parametrize("row,variant", FWD_CASES, ids=["%s-%s" % (r.key, v) for r, v in FWD_CASES])
def test_dense_forward(gpu_device, row, variant):
    dev = gpu_device
    N, H, W, C, O, R, st, pad = row.shape
    P, Q = cc.out_hw(H, W, R, st, pad)
    op = cc.dense_operands(row.key, row.shape, row.Cw)
    x = _bf(op["x"], dev)
    _, wr = _packed(op["w"], C, dev)
    ws = None
    if row.ws:
        need = conv.fd_ws_floats(x.shape, O, R, R, st, pad, row.Cw)
        assert need > 0
        ws = _nan((need,), torch.float32, dev)                               # every partial must be written
    stats = "stats" in variant
    rep = conv.stats_buffer(O, dev) if stats else None
    shift = op["shift"] if stats and "stats0" not in variant else None
    res = "res" in variant
    y = conv.conv2d_fwd(x, wr, st, pad, Cw=row.Cw, stats=rep, out=_nan((N, P, Q, O), torch.bfloat16, dev),
                        shift=_fp(shift, dev) if shift is not None else None, ws=ws,
                        res=_bf(op["res"], dev) if res else None)
    torch.cuda.synchronize()
    what = "%s %s %s [%s] %s" % (row.key, variant, row.shape, "; ".join(row.launches), row.why)
    yh = _np(y)
    _check("fwd", what, yh, cc.fwd_interval(row, res), True, cc.tile_of(row.launches[0], yh.shape))
    if stats:
        _check_stats("fwd", what, rep, yh, shift)


DGRAD_CASES = [(r, v) for r in cc.DGRAD for v in r.variants]


@pytest.mark.parametrize("row,variant", DGRAD_CASES, ids=["%s-%s" % (r.key, v) for r, v in DGRAD_CASES])
def test_dense_dgrad(gpu_device, row, variant):
    dev = gpu_device
    N, H, W, C, O, R, st, pad = row.shape
    op = cc.dense_operands(row.key, row.shape, row.Cw)
    dy = _bf(op["dy"], dev)
    wt, wr = _packed(op["w"], C, dev)
    xs = (N, H, W, C)
    wd = None
    if row.wd:
        wd = _nan((conv.dgrad_image_numel(wt.shape, C),), torch.bfloat16, dev)
        conv.dgrad_pack_weights([(wt, wd, st, pad, C)])
    need = conv.fd_ws_floats(xs, O, R, R, st, pad, row.Cw)
    assert (need > 0) or row.splits == 1
    ws = _nan((need,), torch.float32, dev) if need else None
    base = _bf(op["base"], dev)
    kw = {}
    if variant == "acc":
        out, kw = base.clone(), dict(accumulate=True)
    else:
        out = _nan(xs, torch.bfloat16, dev)
        if variant == "add":
            assert conv.dgrad_fusable(xs, O, R, R, st, pad, row.Cw, has_wd=row.wd)
            kw = dict(add=base)
    dx = conv.conv2d_dgrad(dy, wr, xs, st, pad, Cw=row.Cw, out=out, ws=ws, wd=wd, **kw)
    torch.cuda.synchronize()
    what = "%s %s %s [%s] %s" % (row.key, variant, row.shape, "; ".join(row.launches), row.why)
    dxh = _np(dx)
    _check("dgrad", what, dxh[..., :row.Cw], cc.dgrad_interval(row, variant), True,
           cc.tile_of(row.launches[0], (N, H, W, row.Cw)))
    assert not dxh[..., row.Cw:].any(), what + ": the channel pad of dx is not zero"
    tapless = np.broadcast_to(cc.dgrad_taps(H, W, R, st, pad) == 0, (N, H, W, 1))[..., 0]
    if tapless.any():                                                        # exact: nothing is summed there
        want = op["base"][..., :row.Cw] if variant == "acc" else np.zeros((N, H, W, row.Cw), np.float32)
        assert cc.bits_equal(dxh[..., :row.Cw][tapless], want[tapless]), what + ": tap-less parities"


WGRAD_CASES = [(r, a) for r in cc.WGRAD for a in (False, True)]


def _wgrad_call(row, dev, acc, deferred=None):
    N, H, W, C, O, R, st, pad = row.shape
    op = cc.dense_operands(row.key, row.shape, C)
    x, dy = _bf(op["x"], dev), _bf(op["dy"], dev)
    plane = O * R * R * C
    need = conv.wgrad_ws_floats(x.shape, O, R, R, st, pad, row.Cw) if row.splits == 0 else max(7, row.splits) * plane
    ws = _nan((need,), torch.float32, dev)
    buf = _nan((O, row.Cw, R, R), torch.float32, dev)                        # filters Ow.. keep the marker
    out = buf[:row.Ow]
    if acc:
        out.copy_(_fp(cc.wgrad_base(row), dev))
    conv.conv2d_wgrad(x, dy, R, R, st, pad, Cw=row.Cw, out=out, accumulate=acc, splits=row.splits, ws=ws, Ow=row.Ow,
                      groups=row.groups, deferred=deferred, lib_gemm=row.lib)
    return buf, out, ws


def _wgrad_judge(row, acc, buf, out, what):
    _check("wgrad-acc" if acc else "wgrad", what, _np(out), cc.wgrad_interval(row, acc), False)
    if row.Ow < row.shape[4]:
        rest = _bits(buf[row.Ow:])
        assert bool((rest == _bits(torch.full_like(buf[row.Ow:], NAN))).all()), what + ": filters beyond Ow were written"


@pytest.mark.parametrize("row,acc", WGRAD_CASES, ids=["%s-%s" % (r.key, "acc" if a else "plain") for r, a in WGRAD_CASES])
def test_dense_wgrad(gpu_device, row, acc, monkeypatch):
    if row.lib:
        monkeypatch.setattr(conv, "WGRAD_GEMM_PIXELS", 0)                    # no library GEMM: the 1x1 halo kernel
    buf, out, _ = _wgrad_call(row, gpu_device, acc)
    torch.cuda.synchronize()
    what = "%s %s %s Cw=%d Ow=%d groups=%d [%s] %s" % (row.key, "acc" if acc else "plain", row.shape, row.Cw, row.Ow,
                                                        row.groups, "; ".join(row.launches), row.why)
    _wgrad_judge(row, acc, buf, out, what)


def test_dense_wgrad_window_limit(gpu_device):
    row = cc.WGRAD_8X8
    with pytest.raises((ValueError, RuntimeError), match="window larger than 7x7"):
        _wgrad_call(row, gpu_device, False)
    torch.cuda.synchronize()


def _dw_call(row, dev, acc, deferred=None):
    N, H, W, C, R, st = row.shape
    op = cc.dw_operands(row.key, row.shape)
    x, dy = _bf(op["x"], dev), _bf(op["dy"], dev)
    need = conv.dwconv_ws_floats(x.shape, R, st, R // 2)
    assert need == row.nblk * C * R * R, "partial blocks of the depthwise WGRAD"
    ws = _nan((need,), torch.float32, dev)
    out = _fp(op["base"], dev) if acc else _nan((C, 1, R, R), torch.float32, dev)
    conv.dwconv_wgrad(x, dy, R, st, R // 2, out=out, accumulate=acc, ws=ws, deferred=deferred)
    return out, ws


def test_deferred_reductions_are_the_immediate_ones(gpu_device):
    """Tiled, column, grouped and depthwise reductions through ONE wgrad_reduce_multi: bit-identical to the immediate
    reductions and inside the intervals; nothing is written before the multi launch."""
    dev = gpu_device
    rows = [(next(r for r in cc.WGRAD if r.key == k), i == 1) for i, k in enumerate(cc.WGRAD_DEFERRED)]
    dws = [(next(r for r in cc.DW if r.key == k), i == 1) for i, k in enumerate(cc.DW_DEFERRED)]
    now = [_wgrad_call(r, dev, acc)[1] for r, acc in rows] + [_dw_call(r, dev, acc)[0] for r, acc in dws]
    items, later, keep = [], [], []
    for r, acc in rows:
        buf, out, ws = _wgrad_call(r, dev, acc, deferred=items)
        later.append((r, acc, buf, out))
        keep.append(ws)
    for r, acc in dws:
        out, ws = _dw_call(r, dev, acc, deferred=items)
        later.append((r, acc, None, out))
        keep.append(ws)
    torch.cuda.synchronize()
    assert len(items) == len(rows) + len(dws)
    for (r, acc, _, out) in later:                                           # not reduced yet: NaN, or the base
        want = torch.full_like(out, NAN) if not acc else _fp(cc.wgrad_base(r) if isinstance(r, cc.Wgrad)
                                                             else cc.dw_operands(r.key, r.shape)["base"], dev)
        assert bool((_bits(out) == _bits(want)).all()), r.key + ": written before the deferred reduction"
    conv.wgrad_reduce_multi(items, dev)
    torch.cuda.synchronize()
    for (r, acc, buf, out), ref in zip(later, now):
        assert bool((_bits(out) == _bits(ref)).all()), r.key + ": deferred != immediate"
        if isinstance(r, cc.Wgrad):
            _wgrad_judge(r, acc, buf, out, r.key + " deferred")
        else:
            _check("dw-wgrad-acc" if acc else "dw-wgrad", r.key + " deferred", _np(out),
                   cc.dw_intervals(r)["wgrad_acc" if acc else "wgrad"], False)


@pytest.mark.parametrize("row", cc.DW, ids=lambda r: r.key)
def test_depthwise(gpu_device, row):
    dev = gpu_device
    N, H, W, C, R, st = row.shape
    pad = R // 2
    P, Q = cc.out_hw(H, W, R, st, pad)
    op = cc.dw_operands(row.key, row.shape)
    iv = cc.dw_intervals(row)
    x, dy, w = _bf(op["x"], dev), _bf(op["dy"], dev), _fp(op["w"], dev)
    what = "%s %s nblk=%d %s" % (row.key, row.shape, row.nblk, row.why)
    y0 = conv.dwconv_fwd(x, w, st, pad, out=_nan((N, P, Q, C), torch.bfloat16, dev))
    runs = []
    for shift in (op["shift"], None):
        rep = conv.stats_buffer(C, dev)
        y = conv.dwconv_fwd(x, w, st, pad, stats=rep, out=_nan((N, P, Q, C), torch.bfloat16, dev),
                            shift=_fp(shift, dev) if shift is not None else None)
        runs.append((y, rep, shift))
    dx = conv.dwconv_dgrad(dy, w, (N, H, W, C), st, pad, out=_nan((N, H, W, C), torch.bfloat16, dev))
    dw, _ = _dw_call(row, dev, False)
    dwa, _ = _dw_call(row, dev, True)
    torch.cuda.synchronize()
    _check("dw-fwd", what + " forward", _np(y0), iv["fwd"], True)
    for y, rep, shift in runs:
        assert bool((_bits(y) == _bits(y0)).all()), what + ": the statistics change y"
        _check_stats("dw-fwd", what + (" shift" if shift is not None else " no shift"), rep, _np(y), shift)
    _check("dw-dgrad", what + " dgrad", _np(dx), iv["dgrad"], True)
    _check("dw-wgrad", what + " wgrad", _np(dw), iv["wgrad"], False)
    _check("dw-wgrad-acc", what + " wgrad accumulate", _np(dwa), iv["wgrad_acc"], False)
