"""The zoo kernels (csrc/kernels/zoo_ops.hip) driven directly, against the fp64 references and derived bounds of
tests/zoo_check.py.

No dispatch mode: the ``z_*`` bindings and ``zoo_launch.ew`` / ``reduce_sum`` are called with torch's stream
handle.  Every output lives inside a larger buffer pre-filled with a canary -- the guard elements around it and
the skipped channels of a slice -- and the canary is asserted untouched after each launch.  Shapes are the
smallest that cross each tile / vector / split edge; tests/test_zoo_check.py shows on the CPU that a plain fp32
evaluation of every case here falls inside its bound.  No test feeds non-finite values or depends on the order of
workgroups.
"""
import itertools
import math

import numpy as np
import pytest
import torch

import zoo_check as zc
from fedmi import native
from fedmi.ops import zoo_launch as zl

pytestmark = pytest.mark.gpu

CANARY = 12288.0        # exact in bf16, far from every value the cases draw
ICANARY = -7777
BF, F32, I64, I32 = torch.bfloat16, torch.float32, torch.int64, torch.int32
MEASURED = {}           # worst fast-intrinsic errors seen, in fp32 ulps (printed; see zoo_check's constants)


def _measure(name, v):
    MEASURED[name] = max(MEASURED.get(name, 0.0), float(v))
    print(f"[zoo-pin] measured {name}: {MEASURED[name]:.3f} ulp")


class Dev:
    """A device buffer with guard elements around it and a view of its middle; `check` asserts that everything
    outside the view still holds the canary."""

    def __init__(self, dev, shape, dtype, layout="contig", data=None, shift=0, pad=64):
        shape = tuple(shape)
        if layout == "contig":
            numel, fn = max(math.prod(shape), 1), (lambda b: b.view(shape))
        elif layout[0] == "cl":           # logical NCHW, memory N H W Cw, channels [off, off + C)
            (_, off, Cw), (N, C, H, W) = layout, shape
            numel, fn = N * H * W * Cw, (lambda b: b.view(N, H, W, Cw)[..., off:off + C].permute(0, 3, 1, 2))
        elif layout[0] == "rows":         # [M, C] rows of stride ld
            (_, ld), (M, C) = layout, shape
            numel, fn = M * ld, (lambda b: b.view(M, ld)[:, :C])
        elif layout[0] == "t":            # [M, C] stored transposed
            M, C = shape
            numel, fn = M * C, (lambda b: b.view(C, M).t())
        elif layout[0] == "step":         # 1-D with an element stride
            numel, fn = shape[0] * layout[1], (lambda b: b.view(shape[0], layout[1])[:, 0])
        else:
            raise ValueError(layout)
        self.canary = CANARY if dtype.is_floating_point else ICANARY
        self.buf = torch.full((numel + 2 * pad + shift,), self.canary, dtype=dtype, device=dev)
        self._fn = lambda b: fn(b[pad + shift:pad + shift + numel])
        self.v = self._fn(self.buf)
        self.dtype = dtype
        if data is not None:
            self.set(data)

    def set(self, data):
        data = np.array(np.broadcast_to(data, self.v.shape))          # a writable copy; keeps a 0-dim shape
        self.v.copy_(torch.from_numpy(data.reshape(-1)).to(self.dtype).view(self.v.shape))
        return self

    def get(self):
        t = self.v.cpu()
        return (t.double() if t.dtype.is_floating_point else t).numpy()

    def check(self, what=""):
        c = self.buf.clone()
        self._fn(c).fill_(self.canary)
        assert bool((c == self.canary).all()), ("canary overwritten", what)
        return self

    @property
    def ptr(self):
        return self.v.data_ptr()

    @property
    def d(self):
        return zl.zd(self.v)

    @property
    def is_bf(self):
        return self.dtype == BF


def ok(out, iv, what):
    out.check(what)
    zc.assert_inside(out.get(), iv, out.is_bf, what)


class Spy:
    def __init__(self, nat):
        self.nat, self.calls = nat, []

    def __getattr__(self, name):
        f = getattr(self.nat, name)

        def call(*a, **k):
            self.calls.append((name, a, k))
            return f(*a, **k)
        return call


@pytest.fixture
def nat():
    return native.require()


@pytest.fixture
def st(gpu_device):
    return native.stream_handle(gpu_device)


@pytest.fixture
def spy(monkeypatch, nat):
    s = Spy(nat)
    monkeypatch.setattr(zl, "_nat", lambda: s)
    return s


# ---------------------------------------------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------------------------------------------
def _ew_layouts(case):
    name, shape, shapes, f32s = case
    if name.startswith("inner"):
        return [("contig", {7: -1, 12: 4, 24: 8}[shape[1]])]
    return [(("cl", 3, zc.EW_CL_WIDE), -1), (("cl", 8, zc.EW_CL_WIDE), 8)]


@pytest.mark.parametrize("op", zc.EW_OPS)
def test_ew(gpu_device, spy, op):
    s0 = zc.ew_s0(op)
    for case in zc.ew_cases(op):
        name, shape, shapes, f32s = case
        xs = zc.ew_inputs(op, case)
        for (lay, want_vw), out_dt, s1 in itertools.product(_ew_layouts(case), (BF, F32),
                                                             (0.0, 1.0) if op in zc.EW_S1_OPS else (0.0,)):
            ins = [Dev(gpu_device, s, F32 if f else BF, lay if tuple(s) == tuple(shape) else "contig", x)
                   for s, f, x in zip(shapes, f32s, xs)]
            out = Dev(gpu_device, shape, out_dt, lay)
            spy.calls.clear()
            zl.ew(out.v, [t.v for t in ins], op, s0, s1)
            (_, a, _), = spy.calls
            vmask, vw = a[8], a[9]
            assert (vw if vmask >= 0 else -1) == want_vw, (op, name, lay, vmask, vw)
            assert len(a[2]) == zc.EW_NIN[op]
            iv = zc.ew_ref(op, xs, s0, s1)
            ok(out, iv, (op, name, lay, out_dt, s1))
            if op == zc.EW_SIGMOID and out_dt == F32:
                ref = 0.5 * (iv[0] + iv[1])
                _measure("sigmoid", np.max(np.abs(out.get() - ref) / zc.ulp32(ref)))


def test_ew_grid_stride(gpu_device, spy):
    """One launch per kernel form just past 4096 blocks x 256 threads: the grid-stride loop's second trip."""
    for bf, n, want_vw in ((False, zc.EW_GRID_N, -1), (True, 8 * zc.EW_GRID_N, 8)):
        xs = [zc.draw(("ewgrid", bf, k), (n,), bf16=bf) for k in range(2)]
        ins = [Dev(gpu_device, (n,), BF if bf else F32, data=x) for x in xs]
        out = Dev(gpu_device, (n,), BF if bf else F32)
        spy.calls.clear()
        zl.ew(out.v, [t.v for t in ins], zc.EW_ADD, 0.75)
        a = spy.calls[0][1]
        assert (a[9] if a[8] >= 0 else -1) == want_vw
        ok(out, zc.ew_ref(zc.EW_ADD, xs, 0.75), ("grid", bf))


def test_bernoulli_and_counter(gpu_device, nat, st):
    for (seed, c), (shape, lay, dt) in itertools.product(
            itertools.product((1, 0xDEADBEEF), (0, 41)),
            (((5, 37), "contig", F32), ((2, 8, 3, 5), ("cl", 0, 8), BF))):
        ctr = Dev(gpu_device, (4,), I32, data=np.array([c, 9, 9, 9]))
        out = Dev(gpu_device, shape, dt, lay)
        zl.ew(out.v, [], zc.EW_BERN, 0.3, seed=seed, ctr=ctr.v)
        n = math.prod(shape)
        out.check()
        assert np.array_equal(out.get().reshape(-1), zc.bernoulli_ref(seed, c, n, 0.3)), (seed, c, shape)
        nat.z_ctr_bump(st, ctr.ptr)
        ctr.check()
        assert ctr.get().tolist() == [c + 1, 9, 9, 9]


# ---------------------------------------------------------------------------------------------------------------
# generic reduction
# ---------------------------------------------------------------------------------------------------------------
def _reduce_variants(gpu_device, spy, op, a, b, sh, ah, bh, dims, no, what):
    """acc += into a non-zero accumulator; direct out with a scale, fp32 and bf16."""
    use_b = op in (zc.RD_DOT_SHIFT, zc.RD_DOT_R)
    shd = Dev(gpu_device, (no,), F32, data=sh) if sh is not None else None
    acc0 = (zc.draw(("rdacc", no, 1), (no,), bf16=False), zc.draw(("rdacc", no, 2), (no,), bf16=False))
    acc, acc2 = Dev(gpu_device, (no,), F32, data=acc0[0]), Dev(gpu_device, (no,), F32, data=acc0[1])
    spy.calls.clear()
    zl.reduce_sum(ah.v, dims, acc.v, op, b=bh.v if use_b else None, shift=shd.v if shd else None,
                  acc2=acc2.v if op != zc.RD_SUM else None)
    assert [c[0] for c in spy.calls if c[0].startswith("z_reduce") and not c[0].endswith("floats")] == ["z_reduce"], what
    iv = zc.reduce_ref(op, a, b, sh, acc=acc0)
    ok(acc, iv[0], what + ("acc",))
    if op == zc.RD_SUM:
        acc2.check()
        assert np.array_equal(acc2.get(), acc0[1].astype(np.float64)), "the second accumulator is not this op's"
    else:
        ok(acc2, iv[1], what + ("acc2",))
    if op == zc.RD_SUMSQ_SHIFT:
        return
    for dt in (F32, BF):
        out = Dev(gpu_device, (no,), dt)
        zl.reduce_sum(ah.v, dims, None, op, b=bh.v if use_b else None, shift=shd.v if shd else None, out=out.v, scale=0.5)
        iv = zc.reduce_ref(op, a, b, sh, scale=0.5)
        ok(out, iv[0] if op == zc.RD_SUM else iv[1], what + ("out", dt))


@pytest.mark.parametrize("op", (zc.RD_SUM, zc.RD_SUMSQ_SHIFT, zc.RD_DOT_SHIFT, zc.RD_DOT_R))
def test_reduce(gpu_device, spy, nat, op):
    for no, ni in itertools.product(zc.RD_OUTER, zc.RD_INNER):
        a, b, sh = zc.reduce_inputs(op, no, ni)
        sh = sh if op in (zc.RD_SUMSQ_SHIFT, zc.RD_DOT_SHIFT) else None
        ah = Dev(gpu_device, (no, ni), BF, data=a)
        bh = Dev(gpu_device, (no, ni), BF, ("t",), data=b)       # b's strides differ from a's
        _reduce_variants(gpu_device, spy, op, a, b, sh, ah, bh, [1], no, (op, no, ni))
    assert nat.z_reduce_ws_floats(65, 257) == 2 * 2 * 65 and nat.z_reduce_ws_floats(65, 70001) == 2 * 256 * 65


@pytest.mark.parametrize("op", (zc.RD_SUM, zc.RD_DOT_SHIFT))
def test_reduce_nchw_over_batch_and_space(gpu_device, spy, op):
    """An NCHW operand reduced over (0, 2, 3): two inner dims; b channels-last; fp32 a."""
    N, C, H, W = 3, 6, 5, 7
    for bf in (True, False):
        a = zc.draw(("rdn", op, "a", bf), (N, C, H, W), bf16=bf)
        b = zc.draw(("rdn", op, "b", bf), (N, C, H, W), bf16=True)
        sh = zc.draw(("rdn", op, "s"), (C,), scale=0.25, bf16=False) if op == zc.RD_DOT_SHIFT else None
        ah = Dev(gpu_device, (N, C, H, W), BF if bf else F32, data=a)
        bh = Dev(gpu_device, (N, C, H, W), BF, ("cl", 0, C), data=b)
        flat = lambda t: np.moveaxis(t, 1, 0).reshape(C, -1)   # noqa: E731
        _reduce_variants(gpu_device, spy, op, flat(a), flat(b), sh, ah, bh, [0, 2, 3], C, (op, "nchw", bf))


# ---------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------
def _rows_combos():
    for M, bf, wide in itertools.product(zc.ROWS_M, (True, False), (False, True)):
        yield M, bf, wide, 0
    for M in (67, 1031):
        yield M, True, True, 1            # many slabs at a small M


class _Tuned:
    def __init__(self, nat, per_lane):
        self.nat, self.per_lane = nat, per_lane

    def __enter__(self):
        self.prev = self.nat.z_rows_tune(self.per_lane) if self.per_lane else None

    def __exit__(self, *exc):
        if self.per_lane:
            self.nat.z_rows_tune(self.prev)


def _part(gpu_device, nat, M, C):
    return Dev(gpu_device, (int(nat.z_reduce_rows_ws_floats(M, C)),), F32)      # sized after tuning


@pytest.mark.parametrize("C", zc.ROWS_C)
def test_reduce_rows(gpu_device, nat, st, C):
    for M, bf, wide, tune in _rows_combos():
        x, g, f, p = zc.rows_inputs(C, M, bf)
        dt, lay = (BF if bf else F32), ("rows", C + 8 if wide else C)
        xh, gh = Dev(gpu_device, (M, C), dt, lay, x), Dev(gpu_device, (M, C), dt, lay, g)
        sh = Dev(gpu_device, (C,), F32, data=p["mean"])
        acc0 = (p["w"], p["b"])
        with _Tuned(nat, tune):
            if tune and M == 1031:
                assert nat.z_reduce_rows_ws_floats(M, C) > 2 * C, "more than one slab"
            for op in (zc.RD_SUM, zc.RD_SUMSQ_SHIFT, zc.RD_DOT_SHIFT):
                part = _part(gpu_device, nat, M, C)
                acc, acc2 = Dev(gpu_device, (C,), F32, data=acc0[0]), Dev(gpu_device, (C,), F32, data=acc0[1])
                nat.z_reduce_rows(st, gh.ptr, int(bf), lay[1], xh.ptr, int(bf), lay[1],
                                  sh.ptr if op != zc.RD_SUM else 0, C, M, op, part.ptr, part.v.numel(), acc.ptr, acc2.ptr)
                iv = zc.reduce_ref(op, g.T, x.T, p["mean"] if op != zc.RD_SUM else None, acc=acc0)
                what = ("rows", C, M, bf, wide, tune, op)
                part.check(what)
                ok(acc, iv[0], what)
                if op != zc.RD_SUM:
                    ok(acc2, iv[1], what)
            for out_dt, op in itertools.product((F32, BF), (zc.RD_SUM, zc.RD_DOT_SHIFT)):
                part, out = _part(gpu_device, nat, M, C), Dev(gpu_device, (C,), out_dt)
                nat.z_reduce_rows(st, gh.ptr, int(bf), lay[1], xh.ptr, int(bf), lay[1],
                                  sh.ptr if op != zc.RD_SUM else 0, C, M, op, part.ptr, part.v.numel(), 0, 0, out.ptr,
                                  int(out_dt == BF), 0.5)
                iv = zc.reduce_ref(op, g.T, x.T, p["mean"] if op != zc.RD_SUM else None, scale=0.5)
                part.check()
                ok(out, iv[0] if op == zc.RD_SUM else iv[1], ("rows out", C, M, bf, wide, tune, op, out_dt))


_FWD_KEYS = ("rmean", "rvar", "save_mean", "save_invstd", "scale", "bias")


@pytest.mark.parametrize("C", zc.ROWS_C)
def test_bn_rows_fwd(gpu_device, nat, st, C):
    for (M, bf, wide, tune), mean in itertools.product(_rows_combos(), (0.0, 100.0)):
        x, _, _, p = zc.rows_inputs(C, M, bf, mean)
        shift = p["mean"] if mean == 0.0 else None        # near the data mean; or 0 under a mean of 100
        lay = ("rows", C + 8 if wide else C)
        xh = Dev(gpu_device, (M, C), BF if bf else F32, lay, x)
        par = {k: Dev(gpu_device, (C,), F32, data=p[k]) for k in ("w", "b", "mean")}
        o = {k: Dev(gpu_device, (C,), F32, data=p.get(k)) for k in _FWD_KEYS}
        ctr = Dev(gpu_device, (1,), I64, data=np.array([6]))
        with _Tuned(nat, tune):
            part = _part(gpu_device, nat, M, C)
            nat.z_bn_rows_fwd(st, xh.ptr, int(bf), lay[1], par["mean"].ptr if shift is not None else 0, C, M,
                              part.ptr, part.v.numel(), par["w"].ptr, par["b"].ptr, o["rmean"].ptr, o["rvar"].ptr,
                              1e-5, 0.1, o["save_mean"].ptr, o["save_invstd"].ptr, o["scale"].ptr, o["bias"].ptr, ctr.ptr)
        _, iv = zc.bn_fwd_ref(x, shift, p["w"], p["b"], p["rmean"], p["rvar"], 1e-5, 0.1)
        part.check()
        for k in _FWD_KEYS:
            ok(o[k], iv[k], ("bn_rows_fwd", C, M, bf, wide, tune, mean, k))
        ctr.check()
        assert ctr.get().tolist() == [7]


@pytest.mark.parametrize("C", zc.ROWS_C)
def test_bn_rows_bwd(gpu_device, nat, st, C):
    keys = ("k", "bb", "cc", "dw", "db")
    for M, bf, wide, tune in _rows_combos():
        x, g, f, p = zc.rows_inputs(C, M, bf)
        dt, lay = (BF if bf else F32), ("rows", C + 8 if wide else C)
        gm = np.where(f > 0, g, np.float32(0))
        xh, gh, fh, gmh = (Dev(gpu_device, (M, C), dt, lay, v) for v in (x, g, f, gm))
        par = {k: Dev(gpu_device, (C,), F32, data=p[k]) for k in ("mean", "invstd", "w")}
        res = {}
        with _Tuned(nat, tune):
            for name, a, ff in (("masked", gh, fh), ("premasked", gmh, None), ("plain", gh, None)):
                part = _part(gpu_device, nat, M, C)
                o = {k: Dev(gpu_device, (C,), F32) for k in keys}
                nat.z_bn_rows_bwd(st, a.ptr, int(bf), lay[1], xh.ptr, int(bf), lay[1], ff.ptr if ff else 0,
                                  int(bf), lay[1], 0.0, par["mean"].ptr, par["invstd"].ptr, par["w"].ptr, C, M,
                                  part.ptr, part.v.numel(), *[o[k].ptr for k in keys])
                part.check()
                _, iv = zc.bn_bwd_ref(g, x, p["mean"], p["invstd"], p["w"], None if name == "plain" else f > 0)
                for k in keys:
                    ok(o[k], iv[k], ("bn_rows_bwd", name, C, M, bf, wide, tune, k))
                res[name] = o
        for k in keys:      # the fused mask and the pre-masked gradient: bit-identical
            assert torch.equal(res["masked"][k].v, res["premasked"][k].v), (C, M, bf, wide, tune, k)


def test_bn_coeff_kernels(gpu_device, nat, st):
    """z_bn_fwd_coeffs (train and eval) and z_bn_bwd_coeffs from given sums; the eval form with no weight stores
    rsqrtf(rvar + eps) itself: the measurement of the intrinsic's error."""
    C, M = 1000, 77
    rvar = np.exp(zc.draw(("coef", "rv"), (C,), scale=4.0, bf16=False).astype(np.float64)).astype(np.float32)
    rmean = zc.draw(("coef", "rm"), (C,), bf16=False)
    o = {k: Dev(gpu_device, (C,), F32, data={"rmean": rmean, "rvar": rvar}.get(k)) for k in _FWD_KEYS}
    nat.z_bn_fwd_coeffs(st, 0, 0, 0, C, M, 0, 0, o["rmean"].ptr, o["rvar"].ptr, 1e-5, 0.1, 0, 0, 0, o["scale"].ptr,
                        o["bias"].ptr)
    v = (rvar + np.float32(1e-5)).astype(np.float64)          # one fp32 addition, as the kernel's
    ref = 1.0 / np.sqrt(v)
    o["scale"].check()
    _measure("rsqrt", np.max(np.abs(o["scale"].get() - ref) / zc.ulp32(ref)))
    b = zc.RSQRT_ULP * zc.ulp32(ref)
    ok(o["scale"], (ref - b, ref + b), "eval scale")
    ok(o["bias"], zc.widen(zc.imul(zc.pt(-rmean.astype(np.float64)), (ref - b, ref + b))), "eval bias")
    assert np.array_equal(o["rvar"].get(), rvar.astype(np.float64)) and np.all(o["save_mean"].get() == CANARY)
    # train: the sums of a real activation, given as fp32
    x, g, _, p = zc.rows_inputs(64, M)
    d = x.astype(np.float64) - p["mean"]
    s1, s2 = d.sum(0).astype(np.float32), (d * d).sum(0).astype(np.float32)
    h = {k: Dev(gpu_device, (64,), F32, data=v_) for k, v_ in dict(p, s1=s1, s2=s2).items()}
    o = {k: Dev(gpu_device, (64,), F32, data=p.get(k)) for k in _FWD_KEYS}
    nat.z_bn_fwd_coeffs(st, h["s1"].ptr, h["s2"].ptr, h["mean"].ptr, 64, M, h["w"].ptr, h["b"].ptr, o["rmean"].ptr,
                        o["rvar"].ptr, 1e-5, 0.1, 1, o["save_mean"].ptr, o["save_invstd"].ptr, o["scale"].ptr, o["bias"].ptr)
    iv = zc.bn_fwd_fin_iv(zc.pt(s1), zc.pt(s2), M, p["mean"].astype(np.float64), p["w"].astype(np.float64),
                          p["b"].astype(np.float64), p["rmean"], p["rvar"], 1e-5, 0.1)
    for k in _FWD_KEYS:
        ok(o[k], iv[k], ("fwd_coeffs", k))
    keys = ("k", "bb", "cc", "dw", "db")
    o = {k: Dev(gpu_device, (64,), F32) for k in keys}
    nat.z_bn_bwd_coeffs(st, h["s1"].ptr, h["s2"].ptr, h["mean"].ptr, h["invstd"].ptr, h["w"].ptr, 64, M,
                        *[o[k].ptr for k in keys])
    iv = zc.bn_bwd_fin_iv(zc.pt(s1), zc.pt(s2), M, p["mean"].astype(np.float64), p["invstd"].astype(np.float64),
                          p["w"].astype(np.float64))
    for k in keys:
        ok(o[k], iv[k], ("bwd_coeffs", k))


# ---------------------------------------------------------------------------------------------------------------
# pad_rows, pools
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (3, 7, 12, 58))
def test_pad_rows(gpu_device, nat, st, C):
    rows, C8 = 37, (C + 7) // 8 * 8
    for lds, shift in itertools.product((C, C + 5, C8 + 8), (0, 1)):      # lds > C; aligned and odd-offset base
        src = zc.draw(("pad", C, lds), (rows, C))
        s = Dev(gpu_device, (rows, C), BF, ("rows", lds), src, shift=shift)
        dst = Dev(gpu_device, (rows, C8), BF)
        nat.z_pad_rows(st, s.ptr, lds, C, dst.ptr, C8, rows)
        dst.check()
        assert np.array_equal(dst.get(), zc.pad_rows_ref(src, C8).astype(np.float64)), (C, lds, shift)


@pytest.mark.parametrize("cfg", zc.POOLS, ids=[c[0] for c in zc.POOLS])
def test_pool(gpu_device, nat, st, cfg):
    _, is_max, (kh, kw), (sh, sw), (ph, pw), ceil_mode, cip, div = cfg
    for (H, W), cl in itertools.product(zc.POOL_HW, (False, True)):
        x, dy = zc.pool_inputs(H, W, cfg)
        lay = (lambda c: ("cl", 0, c)) if cl else (lambda c: "contig")
        dt = BF if cl else F32
        xh = Dev(gpu_device, x.shape, dt, lay(3), x)
        y = Dev(gpu_device, dy.shape, dt, lay(3))
        idx = Dev(gpu_device, dy.shape, I64, lay(3)) if is_max else None
        args = (kh, kw, sh, sw, ph, pw, int(cip), div, is_max)
        nat.z_pool_fwd(st, xh.d, y.d, idx.d if idx else None, *args)
        iy, ridx = zc.pool_fwd_ref(x, cfg)
        ok(y, iy, ("pool", cfg[0], H, W, cl))
        if is_max:
            idx.check()
            assert np.array_equal(idx.get(), ridx), (cfg[0], H, W, cl)
        dyh = Dev(gpu_device, dy.shape, dt, lay(3), dy)
        dx = Dev(gpu_device, x.shape, dt, lay(3))
        nat.z_pool_bwd(st, dx.d, dyh.d, idx.d if idx else None, *args)
        ok(dx, zc.pool_bwd_ref(dy, cfg, H, W, ridx), ("pool_bwd", cfg[0], H, W, cl))


# ---------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------
def _gemm_case(gpu_device, nat, st, M, K, N, a_bf, b_bf, ta, tb, bias_kind, bias_dt, out_dt, alpha, beta):
    A, B, b1, b2 = zc.gemm_inputs(M, K, N, a_bf16=a_bf, b_bf16=b_bf)
    Ah = Dev(gpu_device, (M, K), BF if a_bf else F32, ("t",) if ta else "contig", A)
    Bh = Dev(gpu_device, (K, N), BF if b_bf else F32, ("t",) if tb else "contig", B)
    bias = {0: None, 1: b1, 2: b2}[bias_kind]
    bh = Dev(gpu_device, bias.shape, bias_dt, data=bias) if bias is not None else None
    out = Dev(gpu_device, (M, N), out_dt)
    nat.z_gemm(st, Ah.d, Bh.d, out.d, bh.d if bh else None, alpha, beta)
    ok(out, zc.gemm_ref(A, B, bias, alpha, beta), ("gemm", M, K, N, a_bf, b_bf, ta, tb, bias_kind, bias_dt, out_dt))


@pytest.mark.parametrize("shape", zc.GEMM_F32, ids=str)
def test_gemm_fp32(gpu_device, nat, st, shape):
    for a_bf, (ta, tb), (bias_kind, alpha, beta), out_dt in itertools.product(
            (False, True), ((False, False), (True, True), (True, False)), ((0, 1.0, 1.0), (1, 1.0, 1.0), (2, 2.0, 0.5)),
            (F32, BF)):
        _gemm_case(gpu_device, nat, st, *shape, a_bf, False, ta, tb, bias_kind, F32, out_dt, alpha, beta)


@pytest.mark.parametrize("shape", zc.GEMM_MFMA, ids=str)
def test_gemm_mfma(gpu_device, nat, st, shape):
    for (ta, tb), (bias_kind, bias_dt, alpha, beta), out_dt in itertools.product(
            ((False, False), (True, False), (False, True), (True, True)),
            ((0, F32, 1.0, 1.0), (1, F32, 1.0, 1.0), (1, BF, 2.0, 0.5), (2, BF, 2.0, 0.5)), (BF, F32)):
        _gemm_case(gpu_device, nat, st, *shape, True, True, ta, tb, bias_kind, bias_dt, out_dt, alpha, beta)


# ---------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------
def test_log_softmax(gpu_device, nat, st):
    for (R, J), dt in itertools.product(itertools.product(zc.LSM_R, zc.LSM_J), (BF, F32)):
        x, g = zc.lsm_inputs(R, J)
        xh, y = Dev(gpu_device, (R, J), BF, data=x), Dev(gpu_device, (R, J), dt)
        nat.z_log_softmax(st, xh.d, y.d, 0, None)
        ok(y, zc.log_softmax_ref(x), ("lsm", R, J, dt))
        yv = y.get()
        if dt == F32:
            mx, se, lse = zc._lse(x.astype(np.float64))
            _measure("log_softmax", np.max(np.abs(yv - (x - lse)) / zc.ulp32(np.abs(mx) + np.abs(np.log(se)))))
        gh, gx = Dev(gpu_device, (R, J), BF, data=g), Dev(gpu_device, (R, J), dt)
        nat.z_log_softmax(st, y.d, gx.d, 1, gh.d)
        ok(gx, zc.log_softmax_bwd_ref(yv, g), ("lsm_bwd", R, J, dt))
        if dt == F32:
            e, sg = np.exp(yv), np.abs(g.astype(np.float64).sum(-1, keepdims=True))
            _measure("log_softmax_bwd_exp", np.max(np.abs(gx.get() - zc.log_softmax_bwd_exact(yv, g))
                                                   / np.maximum(zc.ulp32(e * sg), zc.ulp32(g))))


def test_nll(gpu_device, nat, st):
    for (R, J), bf, mean, kind in itertools.product(zc.NLL_RJ, (False, True), (1, 0), zc.NLL_KINDS):
        lp, tgt = zc.nll_inputs(R, J, bf, kind)
        dt = BF if bf else F32
        lph = Dev(gpu_device, (R, J), dt, data=lp)
        th = Dev(gpu_device, (R,), I64, ("step", 2), tgt)                  # target stride 2
        out, tw = Dev(gpu_device, (1,), dt), Dev(gpu_device, (1,), dt)
        nat.z_nll_fwd(st, lph.d, th.ptr, 2, -100, mean, out.ptr, int(bf), tw.ptr, int(bf))
        iv, cnt = zc.nll_fwd_ref(lp, tgt, -100, bool(mean))
        what = ("nll", R, J, bf, mean, kind)
        ok(out, (np.reshape(iv[0], (1,)), np.reshape(iv[1], (1,))), what)
        ok(tw, zc.pt(np.array([cnt])), what)
        g = np.float32(-1.375)
        gh = Dev(gpu_device, (1,), dt, data=np.array([g]))
        gx = Dev(gpu_device, (R, J), dt)
        nat.z_nll_bwd(st, gx.d, gh.ptr, int(bf), tw.ptr, int(bf), th.ptr, 2, -100, mean)
        gx.check(what)
        want = zc.nll_bwd_ref(R, J, g, float(tw.get()[0]), tgt, -100, bool(mean))
        assert np.array_equal(gx.get(), (zc.as_bf16(want) if bf else want).astype(np.float64)), what


def test_ce_stats(gpu_device, nat, st):
    for R, J in zc.CE_RJ:
        x, y = zc.ce_inputs(R, J)
        xh = Dev(gpu_device, (R, J), BF, data=x)
        yh = Dev(gpu_device, (R,), I64, data=y)
        stats = Dev(gpu_device, (3,), F32, data=np.array([3.5, 2.0, 7.0]))      # accumulates into non-zero stats
        nat.z_ce_stats(st, xh.d, yh.ptr, stats.ptr)
        iv, correct, rows = zc.ce_stats_ref(x, y, (3.5, 2.0, 7.0))
        stats.check()
        got = stats.get()
        zc.assert_inside(got[:1], (np.reshape(iv[0], (1,)), np.reshape(iv[1], (1,))), False, ("ce", R, J))
        assert got[1] == correct and got[2] == rows, (R, J, got, correct, rows)


# ---------------------------------------------------------------------------------------------------------------
# direct grouped conv
# ---------------------------------------------------------------------------------------------------------------
def _gconv_run(gpu_device, nat, st, name):
    cfg = zc.GCONV[name]
    N, C, O, G, (R, S), (sth, stw), (ph, pw), (H, W), layout = cfg
    x, w, dy = zc.gconv_inputs(name)
    dt = F32 if layout == "nchw32" else BF
    lay = {"cl": lambda c: ("cl", 0, c), "slice": lambda c: ("cl", 3, c + 9), "nchw32": lambda c: "contig"}[layout]
    xh, dyh = Dev(gpu_device, x.shape, dt, lay(C), x), Dev(gpu_device, dy.shape, dt, lay(O), dy)
    wh = Dev(gpu_device, w.shape, F32, data=w)
    y, dx, dw = Dev(gpu_device, dy.shape, dt, lay(O)), Dev(gpu_device, x.shape, dt, lay(C)), Dev(gpu_device, w.shape, F32)
    nat.z_gconv(st, 0, xh.d, wh.d, y.d, G, sth, stw, ph, pw)
    nat.z_gconv(st, 1, dx.d, wh.d, dyh.d, G, sth, stw, ph, pw)
    P, Q = zc.gconv_geom(cfg)
    ws = Dev(gpu_device, (int(nat.z_gconv_wgrad_ws_floats(N, P, Q, w.size)),), F32)
    nat.z_gconv(st, 2, xh.d, dw.d, dyh.d, G, sth, stw, ph, pw, ws.ptr, ws.v.numel())
    ws.check(name)
    for t, iv, what in zip((y, dx, dw), zc.gconv_ref(x, w, dy, cfg), ("y", "dx", "dw")):
        ok(t, iv, (name, what))
    return [t.get() for t in (y, dx, dw)]


@pytest.mark.parametrize("name", sorted(zc.GCONV))
def test_gconv(gpu_device, nat, st, name):
    got = _gconv_run(gpu_device, nat, st, name)
    if name == "c_fast_sliced":       # the sums do not depend on which path a layout takes
        for a, b, what in zip(got, _gconv_run(gpu_device, nat, st, "b_fast"), ("y", "dx", "dw")):
            assert np.array_equal(a, b), what
    if name.startswith("h_"):
        N, P, Q = zc.GCONV[name][0], *zc.gconv_geom(zc.GCONV[name])
        assert N * P == 68 and nat.z_gconv_wgrad_ws_floats(N, P, Q, 8 * 8 * 9) >= 2 * 8 * 8 * 9, "two slabs at least"


def test_gconv_rejects_an_oversized_filter(gpu_device, nat, st):
    """R * S * 8 * GT floats must fit the 8192-float LDS weight chunk: 12 x 12 raises on the host, nothing is
    launched (the tensors are real and correctly sized all the same); 11 x 11 runs (GCONV['k11'])."""
    x = Dev(gpu_device, (1, 8, 12, 12), BF, ("cl", 0, 8), zc.draw(("big", "x"), (1, 8, 12, 12)))
    w = Dev(gpu_device, (8, 8, 12, 12), F32, data=zc.draw(("big", "w"), (8, 8, 12, 12), bf16=False))
    y = Dev(gpu_device, (1, 8, 1, 1), BF, ("cl", 0, 8), zc.draw(("big", "y"), (1, 8, 1, 1)))
    ws = Dev(gpu_device, (int(nat.z_gconv_wgrad_ws_floats(1, 1, 1, 8 * 8 * 144)),), F32)
    for mode in (0, 1, 2):
        with pytest.raises(ValueError, match="filter too large"):
            nat.z_gconv(st, mode, x.d, w.d, y.d, 1, 1, 1, 0, 0, ws.ptr, ws.v.numel())
    torch.cuda.synchronize()
    for t in (x, w, y, ws):
        t.check()
