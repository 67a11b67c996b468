"""tests/zoo_check.py and the zoo launch planner, checked on the CPU before any kernel runs.

1. The fp64 references agree with an independent authority, torch's CPU ops in fp64 (to ~1e-12; indices and
   masks exactly).
2. Every GPU case of tests/test_zoo_kernels_gpu.py, with its actual seeded inputs, evaluated as a plain
   sequential numpy-float32 computation, falls inside its bound: no bound is tighter than fp32 itself allows.
3. The launch planner (fedmi/ops/zoo_launch.py): the descriptors ``ew`` and ``reduce_sum`` would pass to the
   kernels are recorded, executed on CPU tensors through a numpy re-statement of the kernels' index decode, and
   compared with the op's broadcasting semantics; every planned vector launch meets the kernel's alignment
   preconditions.  ``coalesce`` enumerates the same offsets as the space it merged.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import zoo_check as zc
from fedmi.ops import native_mode as nm
from fedmi.ops import zoo_launch as zl

T64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))   # noqa: E731


def mid(iv):
    return 0.5 * (iv[0] + iv[1])


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max(initial=0.0) <= tol * max(1.0, np.abs(b).max(initial=0.0)), np.abs(a - b).max()


# ---------------------------------------------------------------------------------------------------------------
# 1. references against torch fp64
# ---------------------------------------------------------------------------------------------------------------
def test_bf16_rne_is_torch_bfloat16():
    x = np.random.default_rng(0).standard_normal(20000) * np.exp(np.random.default_rng(1).uniform(-20, 20, 20000))
    x = np.concatenate([x, [1.00390625, 1.01171875, -1.00390625, 0.0, 257.0, 255.0]])   # ties
    x32 = x.astype(np.float32)
    assert np.array_equal(zc.as_bf16(x32), torch.from_numpy(x32).bfloat16().float().numpy())
    assert zc.ulp32(1.0) == 2.0 ** -23 and zc.ulp32(0.75) == 2.0 ** -24 and zc.ulp32(2.0) == 2.0 ** -22


def test_hash3_is_the_integer_function():
    def h3(a, b, c):
        m = 0xFFFFFFFF
        h = (a * 0x9E3779B1) & m
        h ^= ((b + 0x7F4A7C15) * 0x85EBCA77) & m
        h ^= ((c + 0x165667B1) * 0xC2B2AE3D) & m
        h ^= h >> 15; h = (h * 0x2C1B3C6D) & m
        h ^= h >> 12; h = (h * 0x297A2D39) & m
        return h ^ (h >> 15)
    for seed, ctr in ((1, 0), (0xDEADBEEF, 7)):
        got = zc.hash3(seed, ctr, np.arange(300))
        assert [int(v) for v in got] == [h3(seed, ctr, i) for i in range(300)]
    m = zc.bernoulli_ref(5, 3, 100000, 0.25)
    assert abs(m.mean() - 0.25) < 0.01 and set(np.unique(m)) == {0.0, 1.0}


@pytest.mark.parametrize("name", sorted(zc.GCONV))
def test_gconv_reference(name):
    cfg = zc.GCONV[name]
    x, w, dy = zc.gconv_inputs(name)
    xt, wt = T64(x).requires_grad_(True), T64(w).requires_grad_(True)
    y = F.conv2d(xt, wt, None, cfg[5], cfg[6], 1, cfg[3])
    y.backward(T64(dy))
    iy, idx, idw = zc.gconv_ref(x, w, dy, cfg)
    close(mid(iy), y.detach().numpy())
    close(mid(idx), xt.grad.numpy())
    close(mid(idw), wt.grad.numpy())
    for iv in (iy, idx, idw):
        assert np.all(iv[1] >= iv[0])


@pytest.mark.parametrize("hw", zc.POOL_HW)
@pytest.mark.parametrize("cfg", zc.POOLS, ids=[c[0] for c in zc.POOLS])
def test_pool_reference(cfg, hw):
    _, is_max, k, s, p, ceil_mode, cip, div = cfg
    x, dy = zc.pool_inputs(*hw, cfg)
    xt = T64(x).requires_grad_(True)
    iy, idx = zc.pool_fwd_ref(x, cfg)
    if is_max:
        y, ti = F.max_pool2d(xt, k, s, p, ceil_mode=ceil_mode, return_indices=True)
        assert np.array_equal(idx, ti.numpy())
        assert np.array_equal(mid(iy), y.detach().numpy())
        wins = np.lib.stride_tricks.sliding_window_view(x, (2, 2), axis=(2, 3))
        assert (wins.reshape(-1, 4).max(1, keepdims=True) == wins.reshape(-1, 4)).sum(1).max() > 1, "no ties drawn"
    else:
        y = F.avg_pool2d(xt, k, s, p, ceil_mode=ceil_mode, count_include_pad=cip, divisor_override=div or None)
        close(mid(iy), y.detach().numpy())
    assert y.shape == dy.shape
    y.backward(T64(dy))
    close(mid(zc.pool_bwd_ref(dy, cfg, *hw, idx)), xt.grad.numpy())


@pytest.mark.parametrize("M", zc.ROWS_M)
def test_bn_reference(M):
    C = 12
    x, g, f, p = zc.rows_inputs(C, M, bf16=True, mean=0.25)
    ref, iv = zc.bn_fwd_ref(x, p["mean"], p["w"], p["b"], p["rmean"], p["rvar"], 1e-5, 0.1)
    xt, wt, bt = (T64(v).requires_grad_(True) for v in (x, p["w"], p["b"]))
    rm, rv = T64(p["rmean"]).clone(), T64(p["rvar"]).clone()
    if M > 1:
        y = F.batch_norm(xt, rm, rv, wt, bt, True, 0.1, 1e-5)
        close(x.astype(np.float64) * ref["scale"] + ref["bias"], y.detach().numpy(), 1e-10)
        close(ref["rmean"], rm.numpy())
        close(ref["rvar"], rv.numpy())
        # backward: dx = g k + x bb + cc with the statistics of the forward pass
        y.backward(T64(g))
        mean64, inv64 = ref["save_mean"], ref["save_invstd"]
        r, _ = zc.bn_bwd_ref(g, x, mean64, inv64, p["w"])
        close(g.astype(np.float64) * r["k"] + x.astype(np.float64) * r["bb"] + r["cc"], xt.grad.numpy(), 1e-9)
        close(r["dw"], wt.grad.numpy(), 1e-10)
        close(r["db"], bt.grad.numpy(), 1e-10)
    else:   # one row: variance 0, the unbiased factor M / (M - 1) taken as 1 (torch refuses to train on one value)
        close(ref["save_mean"], x[0])
        close(ref["save_invstd"], np.full(C, 1e-5 ** -0.5))
        close(ref["rvar"], 0.9 * p["rvar"].astype(np.float64))
    for k_ in ref:
        assert np.all(iv[k_][0] <= iv[k_][1])


def test_loss_references():
    for R, J in itertools.product(zc.LSM_R, zc.LSM_J):
        x, g = zc.lsm_inputs(R, J)
        xt = T64(x).requires_grad_(True)
        y = torch.log_softmax(xt, 1)
        close(mid(zc.log_softmax_ref(x)), y.detach().numpy())
        y.backward(T64(g))
        close(zc.log_softmax_bwd_exact(y.detach().numpy(), g), xt.grad.numpy())
        zc.assert_inside(xt.grad.numpy(), zc.log_softmax_bwd_ref(y.detach().numpy(), g))
        rng = np.random.default_rng(R * 100 + J)
        tgt = rng.integers(0, J, R)
        ign = tgt.copy()
        ign[::2] = -100
        for t, mean in itertools.product((tgt, ign), (True, False)):
            iv, cnt = zc.nll_fwd_ref(y.detach().numpy(), t, -100, mean)
            if cnt > 0 or not mean:
                want = F.nll_loss(y.detach(), torch.from_numpy(t), ignore_index=-100, reduction="mean" if mean else "sum")
                close(mid(iv), want.numpy())
            lp = y.detach().clone().requires_grad_(True)
            F.nll_loss(lp, torch.from_numpy(t), ignore_index=-100, reduction="mean" if mean else "sum").backward()
            if cnt > 0:
                close(zc.nll_bwd_ref(R, J, 1.0, cnt, t, -100, mean), lp.grad.numpy(), 1e-7)
        iv, correct, rows = zc.ce_stats_ref(x, tgt, (0.0, 0.0, 0.0))
        close(mid(iv), F.cross_entropy(T64(x), torch.from_numpy(tgt), reduction="sum").numpy())
        assert correct == float((T64(x).argmax(1).numpy() == tgt).sum()) and rows == R
    iv, cnt = zc.nll_fwd_ref(np.zeros((3, 4)) - 1.0, np.full(3, -100), -100, True)     # all rows ignored
    assert cnt == 0 and mid(iv) == 0.0


def test_gemm_and_reduce_references():
    for M, K, N in zc.GEMM_F32 + zc.GEMM_MFMA:
        A, B, b1, b2 = zc.gemm_inputs(M, K, N)
        close(mid(zc.gemm_ref(A, B, b2, 2.0, 0.5)), torch.addmm(T64(b2), T64(A), T64(B), beta=0.5, alpha=2.0).numpy())
        close(mid(zc.gemm_ref(A, B, b1)), torch.addmm(T64(b1), T64(A), T64(B)).numpy())
    a, b, sh = zc.reduce_inputs(zc.RD_DOT_SHIFT, 5, 33)
    s1, s2 = zc.reduce_ref(zc.RD_DOT_SHIFT, a, b, sh)
    close(mid(s1), T64(a).sum(1).numpy())
    close(mid(s2), (T64(a) * (T64(b) - T64(sh)[:, None])).sum(1).numpy())
    s1, s2 = zc.reduce_ref(zc.RD_SUMSQ_SHIFT, a, None, sh)
    close(mid(s2), ((T64(a) - T64(sh)[:, None]) ** 2).sum(1).numpy())
    s1, s2 = zc.reduce_ref(zc.RD_DOT_R, a, b)
    close(mid(s2), (torch.from_numpy(a) * torch.from_numpy(b)).bfloat16().double().sum(1).numpy())


def test_ew_references():
    x = [zc.ew_operand(zc.EW_BNB_THR_ADD, k, (4, 24), ("t",)) for k in range(7)]
    t = [T64(v) for v in x]
    bf = lambda v: v.float().bfloat16().double()   # noqa: E731
    want = {
        zc.EW_ADD: t[0] + 0.75 * t[1], zc.EW_SUB: t[0] - 0.75 * t[1], zc.EW_MUL: t[0] * t[1], zc.EW_MULS: t[0] * 0.75,
        zc.EW_RELU: torch.relu(t[0]), zc.EW_THR_BWD: torch.where(t[1] > 0.75, t[0], 0.0), zc.EW_SIGMOID: torch.sigmoid(t[0]),
        zc.EW_SIG_BWD: t[0] * t[1] * (1 - t[1]), zc.EW_FMA: t[0] * t[1] + t[2], zc.EW_BNB: t[0] * t[1] + t[2] * t[3] + t[4],
        zc.EW_DIV: t[0] / t[1], zc.EW_ADDS: t[0] + 0.75, zc.EW_FMA_RELU: torch.relu(t[0] * t[1] + t[2]),
        zc.EW_BNB_THR: torch.where(t[5] > 0.75, t[0], 0.0) * t[1] + t[2] * t[3] + t[4],
        zc.EW_FMA_ADD: t[0] * t[1] + t[2] + t[3], zc.EW_FMA_ADD_RELU: torch.relu(t[0] * t[1] + t[2] + t[3]),
        zc.EW_BNB_ADD: t[0] * t[1] + t[2] * t[3] + t[4] + t[5],
        zc.EW_BNB_THR_ADD: torch.where(t[5] > 0.75, t[0], 0.0) * t[1] + t[2] * t[3] + t[4] + t[6],
        zc.EW_COPY: t[0], zc.EW_FILL: torch.full_like(t[0], 0.75)}
    assert sorted(want) == zc.EW_OPS
    for op, w in want.items():
        got = np.broadcast_to(mid(zc.ew_ref(op, x[:zc.EW_NIN[op]], 0.75)), (4, 24))
        close(got, w.numpy())
    # s1: the BN term rounded to bf16 before the add -- the interval holds torch's own two-step evaluation
    for op in zc.EW_S1_OPS:
        iv = zc.ew_ref(op, x[:zc.EW_NIN[op]], 0.0, 1.0)
        if op in (zc.EW_FMA_ADD, zc.EW_FMA_ADD_RELU):
            two = bf(t[0] * t[1] + t[2]) + t[3]
        else:
            g = torch.where(t[5] > 0, t[0], 0.0) if op == zc.EW_BNB_THR_ADD else t[0]
            two = bf(g * t[1] + t[2] * t[3] + t[4]) + (t[6] if op == zc.EW_BNB_THR_ADD else t[5])
        two = torch.relu(two) if op == zc.EW_FMA_ADD_RELU else two
        zc.assert_inside(two.numpy(), iv, what=op)
        assert (iv[1] - iv[0]).max() < 2.0 ** -6 * 16     # at most ~ one bf16 ulp of the term wide


# ---------------------------------------------------------------------------------------------------------------
# 2. plain fp32 inside every bound, for every GPU case
# ---------------------------------------------------------------------------------------------------------------
def _both(y32, iv, what):
    zc.assert_inside(y32, iv, False, what)
    zc.assert_inside(zc.as_bf16(y32), iv, True, what)


@pytest.mark.parametrize("op", zc.EW_OPS)
def test_fp32_inside_ew(op):
    for case in zc.ew_cases(op):
        xs = zc.ew_inputs(op, case)
        for s1 in ((0.0, 1.0) if op in zc.EW_S1_OPS else (0.0,)):
            iv = zc.ew_ref(op, xs, zc.ew_s0(op), s1)
            y = np.broadcast_to(zc.ew_f32(op, xs, zc.ew_s0(op), s1), case[1])
            _both(y, iv, (op, case[0], s1))
            if op in zc.EW_EXACT:
                assert np.array_equal(iv[0], iv[1])


def test_fp32_inside_ew_grid_stride():
    for bf, n in ((False, zc.EW_GRID_N), (True, 8 * zc.EW_GRID_N)):
        xs = [zc.draw(("ewgrid", bf, k), (n,), bf16=bf) for k in range(2)]
        _both(zc.ew_f32(zc.EW_ADD, xs, 0.75), zc.ew_ref(zc.EW_ADD, xs, 0.75), ("grid", bf))


@pytest.mark.parametrize("op", (zc.RD_SUM, zc.RD_SUMSQ_SHIFT, zc.RD_DOT_SHIFT, zc.RD_DOT_R))
def test_fp32_inside_reduce(op):
    for no, ni in itertools.product(zc.RD_OUTER, zc.RD_INNER):
        a, b, sh = zc.reduce_inputs(op, no, ni)
        sh = sh if op in (zc.RD_SUMSQ_SHIFT, zc.RD_DOT_SHIFT) else None
        acc = (zc.draw(("rdacc", no, 1), (no,), bf16=False), zc.draw(("rdacc", no, 2), (no,), bf16=False))
        for kw in (dict(acc=acc), dict(scale=0.5)):
            iv = zc.reduce_ref(op, a, b, sh, **kw)
            y = zc.reduce_f32(op, a, b, sh, **kw)
            for k in (0, 1):
                if iv[k] is not None:
                    _both(y[k], iv[k], (op, no, ni, k, sorted(kw)))


@pytest.mark.parametrize("C", zc.ROWS_C)
def test_fp32_inside_rows(C):
    for M, bf, mean in itertools.product(zc.ROWS_M, (True, False), (0.0, 100.0)):
        x, g, f, p = zc.rows_inputs(C, M, bf, mean)
        for shift in ((p["mean"] + np.float32(mean)), None):
            _, iv = zc.bn_fwd_ref(x, shift, p["w"], p["b"], p["rmean"], p["rvar"], 1e-5, 0.1)
            y = zc.bn_fwd_f32(x, shift, p["w"], p["b"], p["rmean"], p["rvar"], 1e-5, 0.1)
            for k in iv:
                zc.assert_inside(y[k], iv[k], False, ("bn_fwd", C, M, bf, mean, shift is None, k))
        if mean:
            continue
        for mask in (None, f > 0):
            _, iv = zc.bn_bwd_ref(g, x, p["mean"], p["invstd"], p["w"], mask)
            y = zc.bn_bwd_f32(g, x, p["mean"], p["invstd"], p["w"], mask)
            for k in iv:
                zc.assert_inside(y[k], iv[k], False, ("bn_bwd", C, M, bf, mask is None, k))


def test_fp32_inside_pool_gemm_losses():
    for cfg, hw in itertools.product(zc.POOLS, zc.POOL_HW):
        x, dy = zc.pool_inputs(*hw, cfg)
        iy, idx = zc.pool_fwd_ref(x, cfg)
        _both(zc.pool_fwd_f32(x, cfg), iy, ("pool", cfg[0], hw))
        _both(zc.pool_bwd_f32(dy, cfg, *hw, idx), zc.pool_bwd_ref(dy, cfg, *hw, idx), ("pool_bwd", cfg[0], hw))
    for (M, K, N), a_bf in [(s, False) for s in zc.GEMM_F32] + [(s, True) for s in zc.GEMM_F32 + zc.GEMM_MFMA]:
        A, B, b1, b2 = zc.gemm_inputs(M, K, N, a_bf16=a_bf, b_bf16=a_bf and (M, K, N) in zc.GEMM_MFMA)
        for bias, al, be in ((None, 1.0, 1.0), (b1, 1.0, 1.0), (b1, 2.0, 0.5), (b2, 2.0, 0.5)):
            _both(zc.gemm_f32(A, B, bias, al, be), zc.gemm_ref(A, B, bias, al, be), ("gemm", M, K, N))
    for R, J in itertools.product(zc.LSM_R, zc.LSM_J):
        x, g = zc.lsm_inputs(R, J)
        y = zc.log_softmax_f32(x)
        _both(y, zc.log_softmax_ref(x), ("lsm", R, J))
        _both(zc.log_softmax_bwd_f32(y, g), zc.log_softmax_bwd_ref(y, g), ("lsm_bwd", R, J))
    for (R, J), bf, mean, kind in itertools.product(zc.NLL_RJ, (False, True), (True, False), zc.NLL_KINDS):
        lp, tgt = zc.nll_inputs(R, J, bf, kind)
        _both(zc.nll_fwd_f32(lp, tgt, -100, mean), zc.nll_fwd_ref(lp, tgt, -100, mean)[0], ("nll", R, J, bf, mean, kind))
    for R, J in zc.CE_RJ:
        x, y = zc.ce_inputs(R, J)
        assert (x[0] == x[0].max()).sum() == 2, "a tie of the maximum"
        _both(zc.ce_stats_f32(x, y, (3.5, 2.0, 7.0)), zc.ce_stats_ref(x, y, (3.5, 2.0, 7.0))[0], ("ce", R, J))


@pytest.mark.parametrize("name", sorted(zc.GCONV))
def test_fp32_inside_gconv(name):
    x, w, dy = zc.gconv_inputs(name)
    ivs = zc.gconv_ref(x, w, dy, zc.GCONV[name])
    bf = zc.GCONV[name][8] != "nchw32"
    for what, y, iv, is_bf in zip(("y", "dx", "dw"), zc.gconv_f32(x, w, dy, zc.GCONV[name]), ivs, (bf, bf, False)):
        zc.assert_inside(zc.as_bf16(y) if is_bf else y, iv, is_bf, (name, what))


# ---------------------------------------------------------------------------------------------------------------
# 3. the launch planner
# ---------------------------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name == "z_reduce_ws_floats":
            return lambda no, ni: 2 * 256 * no
        if name == "z_reduce_rows_ws_floats":
            return lambda M, C: 2 * C
        return lambda *a: self.calls.append((name, a))


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(zl, "_nat", lambda: r)
    monkeypatch.setattr(zl, "_st", lambda dev: 0)
    return r


class _Buf:
    """A flat CPU buffer and a view of it; `index` maps the view's logical elements to buffer elements."""

    def __init__(self, numel, dtype, view_fn, fill=None):
        self.base = torch.zeros(numel, dtype=dtype)
        if fill is not None:
            self.base.copy_(torch.from_numpy(zc.draw(fill, (numel,), bf16=dtype == torch.bfloat16)))
        self.view = view_fn(self.base)
        self.index = view_fn(torch.arange(numel))
        self.arr = self.base.float().numpy().copy()

    def at(self, ptr):
        off = ptr - self.base.data_ptr()
        assert 0 <= off < self.base.numel() * self.base.element_size() and off % self.base.element_size() == 0
        return off // self.base.element_size()


def _storage(bufs, descs):
    st = {}
    for d in descs:
        if d is None:
            continue
        owner = [b for b in bufs if b.base.data_ptr() <= d[0] < b.base.data_ptr() + b.base.numel() * b.base.element_size()]
        assert len(owner) == 1
        st[d[0]] = (owner[0].arr, owner[0].at(d[0]))
    return st


_DIMS = (1, 2, 3, 4, 5, 7, 8, 12, 16, 24)


def _layout(rng, shape, dtype, key):
    """A buffer whose view has `shape`: contiguous, permuted (channels-last for 4-D) or a channel slice at offset
    3 / 4 / 8 of a wider buffer."""
    kind = rng.choice(["contig", "perm", "slice3", "slice4", "slice8"]) if len(shape) >= 2 else "contig"
    n = len(shape)
    if kind == "contig":
        return _Buf(int(np.prod(shape)), dtype, lambda b: b.view(*shape), key)
    order = [0] + list(range(2, n)) + [1]          # memory order: channels innermost
    off = {"perm": 0, "slice3": 3, "slice4": 4, "slice8": 8}[kind]
    wide = [shape[d] for d in order]
    wide[-1] += off + (5 if off else 0)
    inv = [order.index(d) for d in range(n)]
    C = shape[1]
    return _Buf(int(np.prod(wide)), dtype, lambda b: b.view(*wide)[..., off:off + C].permute(*inv), key)


def _ew_sweep():
    rng = np.random.default_rng(20240)
    ops = (zc.EW_ADD, zc.EW_FMA, zc.EW_COPY, zc.EW_BNB_THR_ADD, zc.EW_FMA_ADD)
    for i in range(160):
        rank = int(rng.integers(1, 6))
        shape = tuple(int(rng.choice(_DIMS)) for _ in range(rank))
        if i % 4 == 0 and rank == 4:
            shape = (2, int(rng.choice((8, 12, 16, 24))), 3, 5)
        yield i, ops[i % len(ops)], shape, rng


def _operand(rng, shape, i, k):
    dt = torch.float32 if rng.random() < 0.4 else torch.bfloat16
    kind = rng.choice(["full", "full", "chan", "zerodim", "ones"])
    if kind == "zerodim":
        return _Buf(1, torch.float32, lambda b: b.view(()), ("pl", i, k))
    if kind == "chan" and len(shape) >= 2:
        s = tuple(shape[1] if d == 1 else 1 for d in range(len(shape)))
        return _Buf(shape[1], torch.float32, lambda b: b.view(*s), ("pl", i, k))
    if kind == "ones":       # size-1 dims that broadcast, fewer dims than the output
        s = tuple(v if rng.random() < 0.5 else 1 for v in shape)[int(rng.integers(0, len(shape))):]
        return _Buf(int(np.prod(s)) if s else 1, dt, (lambda b: b.view(*s)) if s else (lambda b: b.view(())), ("pl", i, k))
    return _layout(rng, shape, dt, ("pl", i, k))


def test_planner_elementwise(rec):
    vec = {8: 0, 4: 0, 1: 0}
    for i, op, shape, rng in _ew_sweep():
        out = _layout(rng, shape, torch.float32 if rng.random() < 0.3 else torch.bfloat16, None)
        ins = [_operand(rng, shape, i, k) for k in range(zc.EW_NIN[op])]
        rec.calls.clear()
        zl.ew(out.view, [b.view for b in ins], op, 0.0, float(i % 2))
        (name, (st, odesc, idescs, op_, s0, s1, seed, ctr, vmask, vw)), = rec.calls
        assert name == "z_ew" and op_ == op
        descs = [odesc] + list(idescs)
        assert all(len(d[2]) <= 6 and d[2] == odesc[2] for d in descs)
        n = int(np.prod(odesc[2])) * (vw if vmask >= 0 else 1)
        assert n == out.view.numel()                      # the innermost size was divisible by vw
        if vmask >= 0:
            vec[vw] += 1
            for k, (d, b) in enumerate(zip(descs, [out] + ins)):
                es = b.base.element_size()
                is_vec = k == 0 or (vmask >> (k - 1)) & 1
                assert is_vec == (d[3][-1] != 0), "mask bit clear exactly for the stride-0 operands"
                if is_vec:
                    align = 16 if (d[1] == 0 or vw == 8) else 8
                    assert d[3][-1] == vw and vw * es >= align
                    assert d[0] % align == 0 and all((s * es) % align == 0 for s in d[3][:-1]), (i, k, d)
        else:
            vec[1] += 1
        zc.emulate_ew(descs, vmask, vw, op, s0, s1, _storage([out] + ins, descs))
        xs = [torch.from_numpy(b.arr)[b.index].numpy() for b in ins]
        want = np.broadcast_to(zc.ew_f32(op, xs, s0, s1), shape if shape else ())
        want = zc.as_bf16(want) if out.base.dtype == torch.bfloat16 else want
        got = torch.from_numpy(out.arr)[out.index].numpy()
        assert np.array_equal(got, want), (i, op, shape)
        untouched = np.ones(out.arr.size, dtype=bool)
        untouched[out.index.reshape(-1).numpy()] = False
        assert not out.arr[untouched].any(), "a store outside the output view"
    assert min(vec.values()) >= 8, vec     # the sweep reaches the 8-wide, 4-wide and scalar launches


def _emulate_reduce(call, bufs, kept_numel):
    name, a = call
    if name == "z_reduce_rows":
        st, ap, adt, lda, bp, bdt, ldb, shift, C, M, op = a[:11]
        outer = (0, 0, [C], [1]); inner = (0, 0, [M], [lda]); outer_b = (0, 0, [C], [1]); inner_b = (0, 0, [M], [ldb])
        vw = 8 if C % 8 == 0 else 4
        assert C % 4 == 0
        for p, dt, ld in ((ap, adt, lda),) + (((bp, bdt, ldb),) if bp else ()):
            es = 4 if dt == 0 else 2
            align = 16 if (dt == 0 or vw == 8) else 8
            assert p % align == 0 and (ld * es) % align == 0 and vw * es >= align, (p % 16, ld, dt, vw)
    else:
        st, outer, inner, outer_b, inner_b, ap, adt, bp, bdt = a[:9]
    assert int(np.prod(outer[2])) == kept_numel
    out = []
    for ptr, od, idesc in ((ap, outer, inner),) + (((bp, outer_b, inner_b),) if bp else ()):
        arr, base = _storage(bufs, [(ptr,)])[ptr]
        offs = base + zc.decode_offsets(od[2], od[3])[:, None] + zc.decode_offsets(idesc[2], idesc[3])[None, :]
        out.append(arr[offs].astype(np.float64))
    return out, name


def test_planner_reduce(rec):
    rng = np.random.default_rng(77)
    rows = 0
    for i in range(120):
        rank = int(rng.integers(2, 5))
        shape = tuple(int(rng.choice((1, 2, 3, 4, 5, 8, 12, 16))) for _ in range(rank))
        if i % 3 == 0:
            shape = (2, int(rng.choice((4, 8, 12, 16))), 3, 5)
        a = _layout(rng, shape, torch.bfloat16 if i % 2 else torch.float32, ("pr", i, "a"))
        b = _layout(rng, shape, torch.bfloat16 if i % 2 else torch.float32, ("pr", i, "b"))
        if i % 3 == 0:
            dims = [0, 2, 3]
        else:
            dims = sorted(rng.choice(rank, size=int(rng.integers(1, rank)), replace=False).tolist())
        kept = [d for d in range(rank) if d not in dims]
        kept_numel = int(np.prod([shape[d] for d in kept])) if kept else 1
        acc = torch.zeros(kept_numel)
        rec.calls.clear()
        zl.reduce_sum(a.view, dims, acc, zc.RD_DOT_SHIFT, b=b.view, acc2=acc)
        vals, name = _emulate_reduce(rec.calls[0], [a, b], kept_numel)
        rows += name == "z_reduce_rows"
        at, bt = a.view.double(), b.view.double()
        close(vals[0].sum(1), at.sum(dims).reshape(-1).numpy(), 1e-12)      # accumulator index: row-major over the kept dims
        close((vals[0] * vals[1]).sum(1), (at * bt).sum(dims).reshape(-1).numpy(), 1e-12)
    assert 5 <= rows < 120, rows


def test_rows_ld_is_a_row_matrix():
    rng = np.random.default_rng(5)
    hits = 0
    for i in range(200):
        C = int(rng.choice((3, 4, 6, 8, 12, 16, 20)))
        shape = (int(rng.choice((1, 2, 3))), C, int(rng.choice((1, 2, 3))), int(rng.choice((1, 3))))
        if i % 5 == 0:
            shape = shape[:2]
        b = _layout(rng, shape, torch.bfloat16 if i % 2 else torch.float32, None)
        ld = zl._rows_ld(b.view)
        if ld is None:
            continue
        hits += 1
        es = b.base.element_size()
        align = 16 if (es == 4 or C % 8 == 0) else 8
        assert C % 4 == 0 and b.view.data_ptr() % align == 0 and (ld * es) % align == 0
        idx = (b.index.permute(0, 2, 3, 1) if len(shape) == 4 else b.index).reshape(-1, C)
        base = b.at(b.view.data_ptr())
        assert torch.equal(idx, base + torch.arange(idx.shape[0])[:, None] * ld + torch.arange(C)[None, :])
    assert hits >= 20


def _enumerate(shape, strides):
    return [tuple(int(zc.decode_offsets(list(shape), list(s))[i]) for s in strides) for i in range(int(np.prod(shape)))]


def test_coalesce_enumerates_the_same_offsets():
    rng = np.random.default_rng(11)
    merged = 0
    for i in range(300):
        rank = int(rng.integers(1, 6))
        shape = [int(rng.choice((1, 2, 3, 4))) for _ in range(rank)]
        perm = rng.permutation(rank)
        def strides(kind):
            if kind == "bcast":
                keep = rng.random(rank) < 0.5
            st, run = [0] * rank, 1 + (int(rng.integers(0, 3)) if kind == "gap" else 0)
            for d in (perm[::-1] if kind != "rowmajor" else range(rank - 1, -1, -1)):
                st[d] = run
                run *= shape[d] + (1 if kind == "gap" and rng.random() < 0.3 else 0)
            if kind == "bcast":
                st = [s if k else 0 for s, k in zip(st, keep)]
            return st
        ops = [strides(k) for k in (["perm", "rowmajor", "gap", "bcast"][i % 4], "perm", "bcast")]
        ns, nst = zl.coalesce(shape, ops)
        assert len(ns) <= max(1, sum(s != 1 for s in shape)) and all(len(s) == len(ns) for s in nst)
        merged += len(ns) < sum(s != 1 for s in shape)
        assert sorted(_enumerate(ns, nst)) == sorted(_enumerate(shape, ops)), (shape, ops, ns, nst)
        # operand 0 the row-major accumulator of a reduction's kept dims: merged only, never reordered
        acc = [1] * rank
        for d in range(rank - 2, -1, -1):
            acc[d] = acc[d + 1] * shape[d + 1]
        ns, nst = zl.coalesce(shape, [acc] + ops)
        assert _enumerate(ns, nst) == _enumerate(shape, [acc] + ops)
    assert merged > 30


# ---------------------------------------------------------------------------------------------------------------
# the direct grouped conv's filter guard
# ---------------------------------------------------------------------------------------------------------------
def test_conv_with_an_oversized_filter_is_not_native():
    """A 12 x 12 filter routes to the direct grouped conv, whose LDS weight chunk holds at most 128 taps of 8
    channels: _conv / _conv_bwd decline (None) before anything is launched, so the mode falls back or reports."""
    x, w = torch.randn(1, 4, 16, 16), torch.randn(8, 4, 12, 12)
    assert nm._conv_kind(4, 8, 1, (12, 12), (1, 1), (0, 0), (1, 1)) == "gconv"
    assert nm._conv(None, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1) is None
    gy = torch.randn(1, 8, 5, 5)
    assert nm._conv_bwd(None, gy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [True, True, False]) is None
    assert nm._gconv_fits((11, 11)) and nm._gconv_fits((8, 16)) and not nm._gconv_fits((12, 12))
