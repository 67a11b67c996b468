"""The pending-result protocol of the native aten backend (fedmi/ops/zoo_fusion.py and NativeMode's bookkeeping),
on CPU tensors: which op joins which pending result, in which order the others are materialised, what a block's
exit writes.  ``zoo_launch.ew`` is replaced by a recorder, so nothing launches; the numerics of the fused passes
are GPU tests (tests/test_native_mode_gpu.py, tests/test_zoo_steps_gpu.py).
"""
import pytest
import torch

from fedmi.ops import native_mode as nm
from fedmi.ops import zoo_fusion as zf
from fedmi.ops import zoo_launch as zl

aten = torch.ops.aten
BF16, F32 = torch.bfloat16, torch.float32
BN_BWD, BN_BWD_MIOPEN = aten.native_batch_norm_backward.default, aten.miopen_batch_norm_backward.default


def cl(c=8, dtype=BF16, fill=0.0):
    """The smallest activation the row kernels take: channels-last [2, c, 4, 4]."""
    t = torch.full((2, c, 4, 4), fill, dtype=dtype).contiguous(memory_format=torch.channels_last)
    assert zl._cl_rows(t) or c % 4
    return t


def coef(dtype=F32):
    return torch.zeros(1, 8, 1, 1, dtype=dtype)


class Recorder:
    """Stands in for ``zoo_launch.ew``: keeps (op code, output) and runs ``on[op](out, ins)`` if one is set."""

    def __init__(self):
        self.calls, self.on = [], {}

    def __call__(self, out, ins, op, s0=0.0, s1=0.0, seed=0, ctr=None):
        self.calls.append((op, out))
        if op in self.on:
            self.on[op](out, ins)
        return out

    def ops(self):
        return [op for op, _ in self.calls]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(zl, "ew", r)
    return r


def bn(out=None, res=None):
    return zf._PendingBN(cl() if out is None else out, cl(), coef(), coef(), res)


def bnb(out=None):
    return zf._PendingBNB(cl() if out is None else out, [cl(), coef(), cl(), coef(), coef()], 0.0)


def thr(out=None):
    return zf._PendingThr(cl() if out is None else out, cl(), cl(), 0.0)


def mul(out=None):
    return zf._PendingMul(cl() if out is None else out, cl(), cl())


def ctr():
    return zf._PendingCtr(torch.zeros((), dtype=torch.int64))


def sb(out, start, end, dim=1):
    shape = list(out.shape)
    shape[dim] = end - start
    return zf._PendingSliceBwd(out, torch.zeros(shape, dtype=out.dtype), dim, start, end)


# ---- join predicates, case by case ---------------------------------------------------------------------------
def test_bn_joins():
    p, r = bn(), cl()
    out = p.out
    for relu in (aten.relu.default, aten.relu_.default):
        assert p.joins(relu, (out,), {}) is True
        assert p.joins(relu, (r,), {}) is None
    add = aten.add.Tensor
    assert p.joins(add, (out, r), {}) is r and p.joins(add, (r, out), {}) is r
    assert p.joins(add, (out, r), {"alpha": 1}) is r
    assert p.joins(add, (out, out), {}) is None
    assert p.joins(add, (out, r), {"alpha": 2}) is None
    assert p.joins(add, (out, cl(dtype=F32)), {}) is None                       # another dtype
    assert p.joins(add, (out, torch.zeros(2, 8, 4, 4, dtype=BF16)), {}) is None   # other strides (NCHW)
    assert p.joins(add, (out, 1.0), {}) is None
    assert p.joins(aten.add_.Tensor, (out, r), {}) is None and p.joins(aten.sub.Tensor, (out, r), {}) is None
    taken = bn(res=r)                       # a residual has joined already: a second add does not
    assert taken.joins(add, (taken.out, cl()), {}) is None
    assert taken.joins(aten.relu.default, (taken.out,), {}) is True


def test_bn_backward_joins():
    p, o = bnb(), cl()
    out = p.out
    for add in (aten.add.Tensor, aten.add_.Tensor):
        assert p.joins(add, (out, o), {}) is o and p.joins(add, (o, out), {}) is o
        assert p.joins(add, (out, torch.zeros(1, 8, 1, 1, dtype=BF16)), {}) is None   # a broadcast-shaped partner
        assert p.joins(add, (out, o), {"alpha": 2}) is None
        assert p.joins(add, (out, cl(dtype=F32)), {}) is None
        assert p.joins(add, (o, cl()), {}) is None
        assert p.joins(add, (out, out), {}) is None
    assert p.joins(aten.sub.Tensor, (out, o), {}) is None and p.joins(aten.relu.default, (out,), {}) is None


def test_threshold_joins():
    p, x, other = thr(), cl(), cl()
    g = p.out
    rest = (None, None, None, None, None, True, 1e-5, [True, True, True])
    assert p.joins(BN_BWD, (g, x) + rest, {}) is True                   # the gradient is args[0] ...
    assert p.joins(BN_BWD_MIOPEN, (x, g) + rest[:-3] + (1e-5,), {}) is True   # ... and args[1] of the MIOpen variant
    assert p.joins(BN_BWD, (other, x) + rest, {}) is None
    assert p.joins(BN_BWD_MIOPEN, (g, other) + rest[:-3] + (1e-5,), {}) is None
    assert p.joins(BN_BWD, (), {}) is None
    assert p.joins(aten.relu.default, (g,), {}) is None and p.joins(aten.add.Tensor, (g, other), {}) is None


def test_mul_joins():
    p = mul()
    assert p.joins(aten.sum.dim_IntList, (p.out, [2, 3]), {}) is True
    assert p.joins(aten.mean.dim, (p.out, [2, 3]), {"keepdim": True}) is True
    assert p.joins(aten.sum.dim_IntList, (cl(), [2, 3]), {}) is None
    assert p.joins(aten.sum.default, (p.out,), {}) is None and p.joins(aten.relu.default, (p.out,), {}) is None


def test_counter_joins():
    p = ctr()
    assert p.joins(aten.native_batch_norm.default, (cl(),), {}) is True
    assert p.joins(aten.miopen_batch_norm.default, (cl(),), {}) is True
    assert p.joins(aten.add_.Tensor, (p.t, 1), {}) is None and p.joins(BN_BWD, (cl(),), {}) is None


def _dead(*pends):
    return {p.out.untyped_storage().data_ptr(): p for p in pends}


def test_slice_pair():
    lo, hi = sb(cl(), 0, 3), sb(cl(), 3, 8)
    d = _dead(lo, hi)
    assert zf._sb_pair(d, (lo.out, hi.out), {}) == (lo, hi)
    assert zf._sb_pair(d, (hi.out, lo.out), {"alpha": 1}) == (lo, hi)     # lower slice first, in either order
    assert zf._sb_pair(d, (lo.out, hi.out), {"alpha": 2}) is None
    assert zf._sb_pair(d, (lo.out, lo.out), {}) is None                   # the same object twice
    assert zf._sb_pair(d, (lo.out, cl()), {}) is None and zf._sb_pair({}, (lo.out, hi.out), {}) is None
    gap, over = sb(cl(), 4, 8), sb(cl(), 2, 8)
    assert zf._sb_pair(_dead(lo, gap), (lo.out, gap.out), {}) is None     # [0,3) + [4,8)
    assert zf._sb_pair(_dead(lo, over), (lo.out, over.out), {}) is None   # [0,3) + [2,8)
    short = sb(cl(), 3, 7)
    assert zf._sb_pair(_dead(lo, short), (lo.out, short.out), {}) is None   # does not reach the end
    other_dim = sb(cl(), 0, 2, dim=2)
    assert zf._sb_pair(_dead(lo, other_dim), (lo.out, other_dim.out), {}) is None
    assert zf._sb_pair(_dead(lo, bn(out=hi.out)), (lo.out, hi.out), {}) is None   # another kind of deferred tensor


def test_slice_pair_member_already_materialised(rec):
    lo, hi = sb(cl(), 0, 3), sb(cl(), 3, 8)
    mode = nm.NativeMode()
    with mode:
        mode._defer(lo)
        mode._defer(hi)
        mode._touch(aten.relu.default, (lo.out,), {})        # something reads lo: written, no longer deferred
        assert rec.ops() == [zl.EW_FILL, zl.EW_COPY] and rec.calls[0][1] is lo.out
        mode._touch(aten.add.Tensor, (lo.out, hi.out), {})   # so the add cannot pair: hi is written for it as well
        assert mode.take_pair() is None
        assert rec.ops() == [zl.EW_FILL, zl.EW_COPY] * 2 and rec.calls[2][1] is hi.out
        assert not mode._blk.dead


def test_slice_pair_stays_deferred(rec):
    lo, hi = sb(cl(), 0, 3), sb(cl(), 3, 8)
    mode = nm.NativeMode()
    with mode:
        mode._defer(lo)
        mode._defer(hi)
        mode._touch(aten.add.Tensor, (hi.out, lo.out), {})
        assert rec.calls == [] and mode.take_pair() == (lo, hi) and mode.take_pair() is None
        mode._settle((hi.out, lo.out), {})
        assert rec.calls == [] and len(mode._blk.dead) == 2      # both operands stay deferred after the fusion
    assert rec.ops() == [zl.EW_FILL, zl.EW_COPY] * 2             # ... and are written at the block's exit


def test_untaken_pair_is_written_before_the_add_runs(rec):
    lo, hi = sb(cl(), 0, 3), sb(cl(), 3, 8)
    mode = nm.NativeMode()
    with mode:
        mode._defer(lo)
        mode._defer(hi)
        mode._touch(aten.add.Tensor, (lo.out, hi.out), {})
        mode._settle((lo.out, hi.out), {})                       # no impl took the pair
        assert rec.ops() == [zl.EW_FILL, zl.EW_COPY] * 2 and not mode._blk.dead


# ---- sequencing ------------------------------------------------------------------------------------------------
def test_unrelated_op_materialises_pending_bn_first(rec):
    p, other = bn(), cl()
    mode = nm.NativeMode()
    with mode:
        mode.pend(p)
        mode._touch(aten.sigmoid.default, (other,), {})
        assert rec.ops() == [zl.EW_FMA] and rec.calls[0][1] is p.out
        assert mode.take(zf._PendingBN) == (None, None) and not mode._blk.pending


def test_dispatched_op_reads_the_written_tensor(rec):
    """Through the dispatcher: the op that does not join runs after the pending pass has written its operand."""
    p = bn(out=cl(dtype=F32))
    rec.on[zl.EW_FMA] = lambda out, ins: out.fill_(2.0)
    mode = nm.NativeMode()
    with mode:
        mode.pend(p)
        y = torch.sigmoid(p.out)
    assert rec.ops() == [zl.EW_FMA] and torch.equal(y, torch.sigmoid(torch.full_like(y, 2.0)))


def test_relu_claims_pending_bn(rec):
    p = bn()
    mode = nm.NativeMode()
    with mode:
        mode.pend(p)
        mode._touch(aten.relu.default, (p.out,), {})
        assert rec.calls == []                                   # nothing from the pre-op step
        assert mode.take(zf._PendingBNB) == (None, None)
        assert mode.take(zf._PendingBN) == (p, True) and mode.take(zf._PendingBN) == (None, None)
        mode._settle((p.out,), {})
        assert rec.calls == []                                   # taken: the impl owns it now


def test_add_claims_pending_bn_with_its_partner(rec):
    p, r = bn(), cl()
    mode = nm.NativeMode()
    with mode:
        mode.pend(p)
        mode._touch(aten.add.Tensor, (r, p.out), {})
        got, partner = mode.take(zf._PendingBN)
        assert got is p and partner is r and rec.calls == []


def test_claim_not_taken_is_materialised(rec):
    p = bn()
    mode = nm.NativeMode()
    with mode:
        mode.pend(p)
        mode._touch(aten.relu.default, (p.out,), {})
        mode._settle((p.out,), {})
        assert rec.ops() == [zl.EW_FMA] and not mode._blk.claimed and not mode._blk.pending
    assert rec.ops() == [zl.EW_FMA]


ORDER = [zl.EW_ADDS, zl.EW_MUL, zl.EW_BNB, zl.EW_FMA, zl.EW_THR_BWD]      # counter, mul, bnb, bn, thr


def test_several_kinds_flush_in_fixed_order(rec):
    mode = nm.NativeMode()
    with mode:
        for p in (thr(), bn(), bnb(), mul(), ctr()):
            mode.pend(p)
        mode._touch(aten.sigmoid.default, (cl(),), {})
        assert rec.ops() == ORDER
        for p in (bn(), ctr(), thr(), mul(), bnb()):
            mode.pend(p)
        mode._flush()
        assert rec.ops() == ORDER * 2 and not mode._blk.pending


def test_join_is_asked_once_per_op(rec, monkeypatch):
    p, asked = bn(), []
    real = zf._PendingBN.joins
    monkeypatch.setattr(zf._PendingBN, "joins", lambda self, *a: asked.append(a[0]) or real(self, *a))
    mode = nm.NativeMode()
    with mode:
        mode.pend(p)
        mode._touch(aten.relu.default, (p.out,), {})
        mode.take(zf._PendingBN)
        mode._settle((p.out,), {})
    assert asked == [aten.relu.default]


# ---- a block's exit --------------------------------------------------------------------------------------------
def _block_with_leftovers(mode, fail=False):
    with mode:
        mode._defer(sb(cl(), 0, 3))
        mode.pend(bn())
        mode._blk.wcache["k"] = mode._blk.catbufs["k"] = mode._blk.cat_src["k"] = 1
        mode._blk.grad_taken.add(0)
        if fail:
            raise ValueError("leaves the block")


def test_exit_materialises_deferred(rec):
    mode = nm.NativeMode(discard_unread=False)
    _block_with_leftovers(mode)
    assert rec.ops() == [zl.EW_FMA, zl.EW_FILL, zl.EW_COPY] and mode._blk is None and zl.current_mode() is None


def test_exit_discards_unread(rec):
    mode = nm.NativeMode(discard_unread=True)
    _block_with_leftovers(mode)
    assert rec.ops() == [zl.EW_FMA] and mode._blk is None and zl.current_mode() is None


def test_exit_through_exception_leaves_deferred_unwritten(rec):
    mode = nm.NativeMode(discard_unread=False)
    with pytest.raises(ValueError):
        _block_with_leftovers(mode, fail=True)
    assert rec.ops() == [zl.EW_FMA] and mode._blk is None and zl.current_mode() is None


def test_second_block_starts_clean_and_keeps_the_plans(rec):
    mode = nm.NativeMode()
    mode._cat_plan["head"], mode._pack_plan["key"], mode._wd_plan["key"] = 24, "w", "w"
    _block_with_leftovers(mode)
    with mode:
        blk = mode._blk
        assert not (blk.wcache or blk.catbufs or blk.cat_src or blk.grad_taken or blk.dead or blk.pending
                    or blk.claimed or blk.wred or blk.wred_keep or blk.wred_ptrs)
        assert blk.pair is None and not blk.prepacked and not blk.prepacked_wd
        assert zl.current_mode() is mode
    assert mode._cat_plan == {"head": 24} and mode._pack_plan == {"key": "w"} and mode._wd_plan == {"key": "w"}
    assert not [k for k in vars(mode) if k.startswith("_pend")]


# ---- the fallback rule -----------------------------------------------------------------------------------------
def test_pending_is_written_before_aten_runs_the_op(rec):
    """An eval-mode BN backward claims the pending ReLU gradient, but no native impl takes it (``train`` is false:
    ATen's op): the gradient is written before ATen reads it."""
    torch.manual_seed(0)
    grad, relu_out, x = (torch.randn(2, 8, 4, 4).contiguous(memory_format=torch.channels_last) for _ in range(3))
    w, rm, rv = torch.rand(8) + 0.5, torch.randn(8), torch.rand(8) + 0.5
    masked = grad * (relu_out > 0)
    want = BN_BWD(masked, x, w, rm, rv, None, None, False, 1e-5, [True, True, True])
    p = zf._PendingThr(torch.full_like(grad, float("nan")), grad, relu_out, 0.0)
    rec.on[zl.EW_THR_BWD] = lambda out, ins: out.copy_(ins[0] * (ins[1] > 0))
    mode = nm.NativeMode()
    with mode:
        mode.pend(p)
        got = BN_BWD(p.out, x, w, rm, rv, None, None, False, 1e-5, [True, True, True])
    assert rec.ops() == [zl.EW_THR_BWD] and rec.calls[0][1] is p.out
    for g, wnt in zip(got, want):
        assert torch.equal(g, wnt)
