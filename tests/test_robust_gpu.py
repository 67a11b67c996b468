"""The robust-aggregation HIP kernels (csrc/kernels/robust.hip, peer_robust_f32_kernel in csrc/comm/peer_comm.hip,
the fold of csrc/kernels/robust_fold.h) against the exact numpy reference of tests/robust_check.py, bit for bit, and
the LeNet engine end to end on a robust aggregate."""
import functools
import hashlib
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi import native
from fedmi.parallel.robust import RobustConfig, make_robust
from tests import robust_check as rc

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
STAT_SENTINEL = -7
WORLDS = tuple(range(2, 17))             # every width is its own kernel with its own sorting network
BIG_N = 2048 * 256 * 4 + 5               # past the grid cap: every lane strides, and a tail


@pytest.fixture(scope="module")
def nat(gpu_device):
    return native.require()


def _trims(W: int):
    return sorted({0, min(1, rc.b_max(W)), rc.b_max(W)})


@functools.lru_cache(maxsize=None)
def _want(case: str, W: int, n: int, b: int):
    """The reference's (out, cut) of one input, computed once."""
    return rc.reference(rc.inputs(case, W, n, b), b)


def _reduce(nat, dev, rows_np: np.ndarray, b: int):
    """robust_reduce on ``rows_np`` ([W, n]); the row padding, out past n and the stats row past W hold sentinels,
    which must survive.  Returns (out[n], cut[W]) as numpy."""
    W, n = rows_np.shape
    ld = (n + 3) & ~3
    rows = torch.full((W, ld), SENTINEL, dtype=torch.float32, device=dev)
    rows[:, :n].copy_(torch.from_numpy(np.array(rows_np, dtype=np.float32)))       # (a writable copy)
    out = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=dev)
    partial = torch.zeros((nat.robust_partials(n), 16), dtype=torch.int64, device=dev)
    stats = torch.full((16,), STAT_SENTINEL, dtype=torch.int64, device=dev)
    nat.robust_reduce(native.stream_handle(), rows.data_ptr(), ld, W, n, b, out.data_ptr(), partial.data_ptr(),
                      stats.data_ptr())
    torch.cuda.synchronize()
    out, stats = out.cpu(), stats.cpu()
    assert bool((out[n:] == SENTINEL).all()), "out was written past n"
    assert bool((stats[W:] == STAT_SENTINEL).all()), "the stats row was written past W"
    assert bool((partial.cpu()[:, W:] == 0).all())
    return out[:n].numpy(), stats[:W].numpy()


def _check(nat, dev, case, W, n, b):
    want, want_cut = _want(case, W, n, b)
    got, cut = _reduce(nat, dev, rc.inputs(case, W, n, b), b)
    assert rc.same_bits(got, want) == "", (case, W, n, b)
    assert cut.tolist() == want_cut.tolist(), (case, W, n, b)


def test_partials_follow_the_grid_rule(nat):
    assert [nat.robust_partials(n) for n in (0, 1, 3, 1027, 1028, 2048 * 1024, BIG_N, 1 << 33)] == \
        [0, 1, 1, 1, 2, 2048, 2048, 2048]
    with pytest.raises(ValueError):
        nat.robust_partials(-1)


@pytest.mark.parametrize("W", WORLDS)
def test_local_kernel_matches_reference_bit_for_bit(nat, gpu_device, W):
    for b in _trims(W):
        for case in rc.data_cases(W, b):
            for n in rc.NS:
                _check(nat, gpu_device, case, W, n, b)


@pytest.mark.parametrize("case,b", [("randn", 0), ("randn", 1), ("ties", 1), ("extremes", 1), ("nan", 1), ("nan+", 1)])
def test_local_kernel_past_the_grid_cap(nat, gpu_device, case, b):
    _check(nat, gpu_device, case, 3, BIG_N, b)


@pytest.mark.parametrize("W", WORLDS)
def test_zero_one_exhaustive(nat, gpu_device, W):
    """Every 0/1 column: by the zero-one principle a network that sorts all of these sorts everything, and the
    columns full of ties pin the rank tie-break through the cut counts.  Every b_eff."""
    rows = rc.zero_one(W)
    for b in range(rc.b_max(W) + 1):
        want, want_cut = rc.reference(rows, b)
        got, cut = _reduce(nat, gpu_device, rows, b)
        assert rc.same_bits(got, want) == "", (W, b)
        assert cut.tolist() == want_cut.tolist(), (W, b)


def test_two_runs_same_bits(nat, gpu_device):
    rows = rc.inputs("nan+", 9, 1027, 2)
    a, b = _reduce(nat, gpu_device, rows, 2), _reduce(nat, gpu_device, rows, 2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist()


def test_binding_rejects_bad_arguments(nat, gpu_device):
    """Refused before any launch: W outside 2..16, b_eff outside 0..(W-1)//2, n < 0, a bad row stride, a null or
    misaligned buffer."""
    rows = torch.zeros(4 * 16, device=gpu_device)
    out = torch.full((16,), SENTINEL, device=gpu_device)
    w = torch.zeros(64, dtype=torch.int64, device=gpu_device)
    p, o, q, s = rows.data_ptr(), out.data_ptr(), w.data_ptr(), native.stream_handle()
    good = dict(rows=p, ld=16, W=4, n=13, b_eff=1, out=o, partial=q + 128, stats=q)
    for bad in (dict(W=1), dict(W=17), dict(W=0), dict(b_eff=-1), dict(b_eff=2), dict(W=2, b_eff=1), dict(n=-1),
                dict(ld=12), dict(ld=15), dict(n=14, ld=14), dict(rows=0), dict(out=0), dict(partial=0), dict(stats=0),
                dict(rows=p + 4), dict(out=o + 8), dict(partial=q + 4), dict(stats=q + 4)):
        with pytest.raises(ValueError):
            nat.robust_reduce(s, **{**good, **bad})
    nat.robust_reduce(s, **{**good, "n": 0})             # nothing to do
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and not w.any()
    nat.robust_reduce(s, **good)
    torch.cuda.synchronize()
    assert not out[:13].any() and bool((out[13:] == SENTINEL).all())
    assert w[:4].tolist() == [13, 0, 0, 13]              # all ties: ranks 0 and 3 are the ends of the order


# ---- the fused peer kernel ------------------------------------------------------------------------------------------------
PEER_SIZES = (1, 5, 1027, 4 * 256 * 256 + 259)            # the last: past the block cap, with a tail
PEER_CASES = ("randn", "ties", "nan", "nan+")


def _dense(rank: int, it: int, n: int = 4099) -> torch.Tensor:
    return torch.randn(n, generator=torch.Generator().manual_seed(1000 * it + 17 * rank))


def _dense_mean(world: int, it: int) -> torch.Tensor:
    acc = _dense(0, it).clone()
    for r in range(1, world):
        acc = acc + _dense(r, it)
    return acc * (1.0 / world)


class _GpuStub:
    """Minimal LocalTrainer surface on the GPU: a float state and one int64 counter."""

    def __init__(self, flat: torch.Tensor, count: int = 0):
        self.flat = flat
        self.ints = [torch.tensor([count], dtype=torch.int64, device=flat.device)]
        self.packs = 0

    def float_state(self):
        return self.flat

    def n_params(self):
        return self.flat.numel()

    def int_state(self):
        return self.ints

    def after_aggregate(self):
        self.packs += 1


def _peer_worker(rank, world, path, q):
    import torch.distributed as dist

    torch.cuda.set_device(0)
    from fedmi.parallel.fedavg import FedAvg
    from fedmi.parallel.peer import PeerAllReduce

    store = dist.FileStore(path, world)
    dev = torch.device("cuda", 0)
    nat = native.require()
    res = {"ok": True, "msgs": []}
    digest = hashlib.sha256()

    def fail(msg):
        res["ok"] = False
        if len(res["msgs"]) < 20:
            res["msgs"].append(msg)

    def dense(it):
        x = _dense(rank, it).to(dev)
        pc.allreduce_mean_(x)
        if not torch.equal(x.cpu(), _dense_mean(world, it)):
            fail(f"allreduce_f32 call {it} (same communicator) != its expected mean")

    try:
        pc = PeerAllReduce(rank, world, 4 * max(PEER_SIZES) + 4096, store, tag="rb")
        partials = torch.zeros((nat.PEER_MAX_BLOCKS, 16), dtype=torch.int64, device=dev)
        dense(0)                                              # shared epoch and slot counter: one dense call before
        for n in PEER_SIZES:
            for b in _trims(world):
                for case in PEER_CASES:
                    rows = rc.inputs(case, world, n, b)       # every rank's inputs rebuilt here
                    want, want_cut = rc.reference(rows, b)
                    x = torch.from_numpy(rows[rank].copy()).to(dev)
                    stats = torch.full((16,), STAT_SENTINEL, dtype=torch.int64, device=dev)
                    gathered = pc.all_gather(x)               # before x is overwritten in place
                    pc.allreduce_robust_(x, b, partials, stats)
                    torch.cuda.synchronize()
                    got, cut = x.cpu().numpy(), stats.cpu()
                    tag = f"{case} W={world} n={n} b={b}"
                    diff = rc.same_bits(got, want)
                    if diff:
                        fail(f"{tag}: out != reference: {diff}")
                    if cut[:world].tolist() != want_cut.tolist() or not bool((cut[world:] == STAT_SENTINEL).all()):
                        fail(f"{tag}: cut {cut.tolist()} != reference {want_cut.tolist()}")
                    # and the local kernel on the all-gathered rows
                    ld = (n + 3) & ~3
                    buf = torch.zeros((world, ld), dtype=torch.float32, device=dev)
                    buf[:, :n].copy_(gathered)
                    out = torch.empty(n, dtype=torch.float32, device=dev)
                    lp = torch.zeros((nat.robust_partials(n), 16), dtype=torch.int64, device=dev)
                    ls = torch.zeros(16, dtype=torch.int64, device=dev)
                    nat.robust_reduce(native.stream_handle(dev), buf.data_ptr(), ld, world, n, b, out.data_ptr(),
                                      lp.data_ptr(), ls.data_ptr())
                    torch.cuda.synchronize()
                    diff = rc.same_bits(out.cpu().numpy(), got)
                    if diff or ls[:world].tolist() != cut[:world].tolist():
                        fail(f"{tag}: local kernel on the gathered rows != fused kernel: {diff}")
                    digest.update(got.tobytes())
                    digest.update(cut.numpy().tobytes())
        # the product path: FedAvg(robust=..., transport=pc).average() on a GPU trainer, then the lagged stats row
        n = 1027
        for kind in ("median", "trimmed"):
            b = rc.b_eff(kind, 1, world)
            rows = rc.inputs("nan", world, n, b)
            want, want_cut = rc.reference(rows, b)
            t = _GpuStub(torch.from_numpy(rows[rank].copy()).to(dev), 10 + 3 * rank)
            fa = FedAvg(robust=make_robust(kind, t, 1), transport=pc)
            fa.average(t)
            torch.cuda.synchronize()
            diff = rc.same_bits(t.flat.cpu().numpy(), want)
            ints = sum(10 + 3 * r for r in range(world)) // world
            if diff or t.ints[0].item() != ints or t.packs != 1:
                fail(f"FedAvg.average {kind} W={world}: {diff} ints {t.ints[0].item()} != {ints} packs {t.packs}")
            stats = fa.robust.round_stats()
            if stats != {"robust_kind": kind, "robust_trim": b, "robust_cut": want_cut.tolist()}:
                fail(f"FedAvg.average {kind} W={world}: round_stats {stats} != cut {want_cut.tolist()}")
            if fa.label() != f"peer-oneshot-hipipc+{kind}":
                fail(f"label {fa.label()}")
        dense(1)                                              # ... and one after
        res["err"] = pc.error()
        pc.close()
    except Exception as e:  # pragma: no cover - reported to the parent
        fail(repr(e))
        res["err"] = -1
    res["x"] = digest.hexdigest()
    q.put((rank, res))


@pytest.mark.parametrize("world", [2, 3, 4, 5, 8])
def test_fused_peer_kernel_matches_reference_and_local_kernel(world):
    """Every rank's out and cut equal the reference on the rebuilt inputs and the local kernel on the all-gathered
    rows, at every size and case; the dense all-reduce before and after in the same communicator still matches."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "store")
        procs = [ctx.Process(target=_peer_worker, args=(r, world, path, q)) for r in range(world)]
        for p in procs:
            p.start()
        out = dict(q.get(timeout=200) for _ in procs)
        for p in procs:
            p.join(timeout=60)
    for r in range(world):
        assert out[r]["ok"] and out[r]["err"] == 0, (r, out[r]["msgs"])
        assert out[r]["x"] == out[0]["x"], r


# ---- RobustAgg.aggregate over torch.distributed on a GPU -------------------------------------------------------------------
class _FakeFedAvg:
    """What RobustAgg.aggregate asks of its FedAvg: the world, no transport, a group and an abort flag."""

    transport = group = abort = None

    def __init__(self, world: int):
        self._world = world

    def world(self) -> int:
        return self._world


def test_aggregate_gathers_then_reduces_natively(nat, gpu_device, monkeypatch):
    """The torch.distributed branch of RobustAgg.aggregate on a GPU: the all-gather into the row views of the
    persistent [W, ld] buffer, native robust_reduce with that row stride, the buffer's re-allocation when W changes and
    the lagged stats row.  One process: the collective itself is replaced by a copy of the other clients' known
    states into the rows it was handed (gloo has no all-gather of GPU tensors, RCCL needs one GPU per rank)."""
    from fedmi.parallel.robust import RobustAgg

    n, rank = 1027, 1
    state = {}

    def fake_all_gather(rows, x, group, abort):
        assert len(rows) == state["rows"].shape[0] and all(r.is_contiguous() and r.numel() == n for r in rows)
        assert rc.same_bits(x.cpu().numpy(), state["rows"][rank]) == ""     # (the rows hold NaNs)
        for r, row in enumerate(rows):
            row.copy_(torch.from_numpy(state["rows"][r].copy()))

    monkeypatch.setattr(RobustAgg, "_all_gather", staticmethod(fake_all_gather))
    t = _GpuStub(torch.zeros(n, device=gpu_device))
    agg = make_robust("trimmed", t, 2)
    seen = []
    for W in (5, 5, 3, 9):
        b = rc.b_eff("trimmed", 2, W)
        state["rows"] = rc.inputs("nan", W, n, b)
        want, want_cut = rc.reference(state["rows"], b)
        t.flat.copy_(torch.from_numpy(state["rows"][rank].copy()))
        agg.aggregate(t, _FakeFedAvg(W))
        torch.cuda.synchronize()
        assert tuple(agg._rows.shape) == (W, 1028)
        seen.append(agg._rows.data_ptr())
        assert rc.same_bits(t.flat.cpu().numpy(), want) == "", W
        assert agg.round_stats() == {"robust_kind": "trimmed", "robust_trim": b, "robust_cut": want_cut.tolist()}
    assert seen[0] == seen[1]                            # the same world: the same buffer


# ---- the LeNet engine end to end ------------------------------------------------------------------------------------------
def test_lenet_four_clients_signflip_attacker(nat, gpu_device):
    """Four LeNet trainers, one epoch each; client 3 is rewritten by the signflip rule (A = 10).  The stacked states
    go through robust_reduce (trimmed, b = 1) into every trainer, then after_aggregate(): evaluate() equals, bit for
    bit, a fresh trainer loaded from the REFERENCE aggregate's state dict (the repacked weights are the robust ones),
    and the attacker is the client cut most often."""
    from fedmi.engine import build_trainer
    from fedmi.engine.base import TrainerConfig
    from fedmi.engine.data import make_dataset, strided_schedule

    W = 4
    data = make_dataset("synthetic-cifar10", device=gpu_device, n_train=384, n_test=128, seed=0)
    clients, init = [], None
    for r in range(W):
        tr = build_trainer("lenet", data, gpu_device, TrainerConfig(seed=1), init_state=init)
        if init is None:
            init = {k: v.detach().cpu().clone() for k, v in tr.state_dict().items()}
        tr.set_schedule(*strided_schedule(384, 32, r, W))
        clients.append(tr)
    start = clients[0].float_state().clone()
    for tr in clients:
        tr.train_epoch()
    torch.cuda.synchronize()
    x3 = clients[3].float_state()
    x3.copy_(start - 10.0 * (x3 - start))
    rows = np.stack([tr.float_state().cpu().numpy() for tr in clients])
    robust = make_robust("trimmed", clients[0], 1)
    assert robust.cfg.b_eff(W) == 1 and RobustConfig("median").b_eff(W) == 1
    want, want_cut = rc.reference(rows, 1)
    got, cut = _reduce(nat, gpu_device, rows, 1)
    assert rc.same_bits(got, want) == "" and cut.tolist() == want_cut.tolist()
    assert int(np.argmax(cut)) == 3 and cut[3] > rows.shape[1] // 2
    for tr in clients:
        tr.float_state().copy_(torch.from_numpy(got))
        tr.after_aggregate()
    clients[1].evaluate()
    ev = clients[1].eval_stats()
    carrier = build_trainer("lenet", data, gpu_device, TrainerConfig(seed=3), init_state=init)
    carrier.float_state().copy_(torch.from_numpy(want))
    fresh = build_trainer("lenet", data, gpu_device, TrainerConfig(seed=2),
                          init_state={k: v.clone() for k, v in carrier.state_dict().items()})
    fresh.evaluate()
    ref = fresh.eval_stats()
    assert ev.count == 128 and (ev.loss_sum, ev.correct, ev.count) == (ref.loss_sum, ref.correct, ref.count)
