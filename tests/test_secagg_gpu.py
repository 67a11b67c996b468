"""The secure-aggregation HIP kernels (csrc/kernels/secagg.hip) against the numpy rule of tests/secagg_check.py, bit
for bit: the RFC 8439 known answer through the kernel's word map, secagg_mask and secagg_unmask at every width and
edge, SecAgg.aggregate on a GPU and over the peer transport."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi import native
from fedmi.parallel import secagg as sa
from tests import secagg_check as sc
from tests.test_robust_gpu import _FakeFedAvg, _GpuStub, _dense, _dense_mean
from tests.test_secagg import RFC_BLOCK, RFC_KEY

pytestmark = pytest.mark.gpu

SENTINEL, SEED, DRAW, R = -12345, 5, (0x1234 << 32) | 0xFFFFFFFE, 8.0
F = sa.frac_bits(R)
BIG_N = 2048 * 256 * 4 + 3 * 16 + 5      # past the grid cap: every lane strides, then whole blocks and a tail
CASES = ("randn", "half", "edge")


@pytest.fixture(scope="module")
def nat(gpu_device):
    return native.require()


def pair(r: int, j: int, n: int) -> bytes:
    """The pair's key: its own below BIG_N.  At BIG_N one of five (every reference stream there costs 0.1 s, and
    W = 16 has 42 pairs at three ranks): what only that size can break -- the stride, the block counter, 64-bit
    indices -- does not depend on which row holds which key; the sizes below pin the rows with 120 distinct keys."""
    return sa.seeded_key(SEED, min(r, j), max(r, j)) if n != BIG_N else sa.seeded_key(SEED, (r + j) % 5, 16)


def table(W: int, rank: int, n: int = 0) -> np.ndarray:
    return sa.key_table([None if j == rank else pair(rank, j, n) for j in range(W)])


@functools.lru_cache(maxsize=None)
def stream(key: bytes, n: int, draw: int = DRAW) -> np.ndarray:
    return sc.keystream(np.frombuffer(key, dtype="<u4"), draw, n)


def inputs(case: str, n: int, rank: int):
    """``(x, a, q, clamped)`` of one client (at BIG_N every client holds client 0's: the ranks differ in their masks)."""
    return _inputs(case, n, 0 if n == BIG_N else rank)


@functools.lru_cache(maxsize=None)
def _inputs(case: str, n: int, rank: int):
    rng = np.random.default_rng(1000 * rank + n % 997 + len(case))
    if case == "randn":
        a = rng.standard_normal(n).astype(np.float32)
        x = (a + 0.1 * R * rng.standard_normal(n)).astype(np.float32)
    elif case == "half":                                  # x - a = (k + 1/2) 2^-f exactly: ties go to even
        m, k = rng.integers(-2 ** 10, 2 ** 10, n), rng.integers(-2 ** 20, 2 ** 20, n)
        a, x = (m * 2.0 ** -F).astype(np.float32), ((m + k + 0.5) * 2.0 ** -F).astype(np.float32)
    else:
        a = np.zeros(n, dtype=np.float32)
        x = np.resize(np.array([R, -R, 2 * R, -2 * R, np.inf, -np.inf, np.nan, -np.nan, -0.0, 0.25], np.float32), n)
        x = np.roll(x, rank)
    return (x, a) + sc.encode(x, a, F)


def want_mask(case: str, W: int, rank: int, n: int, draw: int = DRAW):
    _, _, q, clamped = inputs(case, n, rank)
    u = (q & sc.M32).astype(np.uint32)                    # uint32 arrays add and subtract mod 2^32
    for j in range(W):
        if j != rank:
            u = u + stream(pair(rank, j, n), n, draw) if j > rank else u - stream(pair(rank, j, n), n, draw)
    return u, clamped


def run_mask(nat, dev, x, a, keys, W, rank, draw, f=F):
    n = x.size
    xd, ad = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(a.copy()).to(dev)
    kd = torch.from_numpy(keys.view(np.int32).copy()).to(dev)
    u = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device=dev)
    partial = torch.zeros((nat.secagg_partials(n), 16), dtype=torch.int64, device=dev)
    stats = torch.full((2,), SENTINEL, dtype=torch.int64, device=dev)
    nat.secagg_mask(native.stream_handle(), xd.data_ptr(), ad.data_ptr(), kd.data_ptr(), W, rank, draw, n, f,
                    u.data_ptr(), partial.data_ptr(), stats.data_ptr())
    torch.cuda.synchronize()
    assert bool((u[n:] == SENTINEL).all()) and int(stats[1]) == SENTINEL, "written past the end"
    return u[:n].cpu().numpy().view(np.uint32), int(stats[0])


def test_known_answer_rfc8439_through_the_word_map(nat, gpu_device):
    """q = 0, so the payload is the keystream: block 1 of the RFC's key and nonce, word 4 k + c at coordinate 4 c + k;
    rank 1 subtracts the same mask."""
    keys = np.stack([RFC_KEY, RFC_KEY]).astype(np.uint32)
    x = np.linspace(-1, 1, 32, dtype=np.float32)
    want = [RFC_BLOCK[4 * (i & 3) + (i >> 2)] for i in range(16)]
    u0, c0 = run_mask(nat, gpu_device, x, x, keys, 2, 0, 0x4A00000009000000)
    u1, c1 = run_mask(nat, gpu_device, x, x, keys, 2, 1, 0x4A00000009000000)
    assert u0[16:].tolist() == want and u1[16:].tolist() == [(-w) & sc.M32 for w in want] and c0 == c1 == 0


@pytest.mark.parametrize("n", [1, 3, 15, 16, 17, 67, 1027, BIG_N])
@pytest.mark.parametrize("W", [2, 3, 8, 16])
def test_mask_matches_the_rule(nat, gpu_device, W, n):
    for rank in sorted({0, W // 2, W - 1}):
        for case in CASES:
            x, a = inputs(case, n, rank)[:2]
            want, clamped = want_mask(case, W, rank, n)
            got, count = run_mask(nat, gpu_device, x, a, table(W, rank, n), W, rank, DRAW)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0 and count == clamped, (case, rank, bad[:5], count, clamped)
    if n == BIG_N:                                        # (hundreds of MB of reference streams)
        stream.cache_clear(), _inputs.cache_clear()


@pytest.mark.parametrize("n", [1, 5, 1027])
@pytest.mark.parametrize("W", range(2, 17))
def test_unmask_matches_the_rule(nat, gpu_device, W, n):
    """Rows from the rule's mask (uniform words: their sums wrap through 2^32), sentinels around every buffer."""
    a = inputs("randn", n, 0)[1]
    rows_np = np.stack([want_mask("randn", W, r, n)[0] for r in range(W)])
    assert (rows_np.astype(np.int64).sum(0) >= 2 ** 32).any() or n < 1027
    ld = (n + 3) & ~3
    rows = torch.full((W, ld), SENTINEL, dtype=torch.int32, device=gpu_device)
    rows[:, :n].copy_(torch.from_numpy(rows_np.view(np.int32).copy()))
    out = torch.full((n + 8,), float(SENTINEL), dtype=torch.float32, device=gpu_device)
    ad = torch.from_numpy(a.copy()).to(gpu_device)
    nat.secagg_unmask(native.stream_handle(), rows.data_ptr(), ld, W, ad.data_ptr(), n, F, out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all())
    assert out[:n].cpu().numpy().tobytes() == sc.decode(rows_np, a, F).tobytes()


def test_aggregate_masks_gathers_and_unmasks_natively(nat, gpu_device, monkeypatch):
    """SecAgg.aggregate on a GPU with the collective replaced by the other clients' payloads from the rule: the row
    it sends is the rule's, the result is the rule's decode, x is written only by the decode, the draw advances."""
    n, rank, W = 1027, 1, 3
    state = {}

    def fake_all_gather(rows, x, group, abort):
        assert x.cpu().numpy().view(np.uint32).tobytes() == state["rows"][rank].tobytes()
        for r, row in enumerate(rows):
            row.copy_(torch.from_numpy(state["rows"][r].view(np.float32).copy()))

    monkeypatch.setattr(sa.SecAgg, "_all_gather", staticmethod(fake_all_gather))
    a = inputs("edge", n, 0)[1]
    guard = sa.make_secagg(True, _GpuStub(torch.from_numpy(a.copy()).to(gpu_device)), R, seed=SEED)
    fake = _FakeFedAvg(W)
    fake.rank = lambda: rank
    for draw in (0, 1):
        state["rows"] = np.stack([want_mask("edge", W, r, n, draw)[0] for r in range(W)])
        t = _GpuStub(torch.from_numpy(inputs("edge", n, rank)[0].copy()).to(gpu_device))
        guard.aggregate(t, fake)
        torch.cuda.synchronize()
        assert t.flat.cpu().numpy().tobytes() == sc.decode(state["rows"], a, F).tobytes()
        assert guard.round_stats() == {"secagg_draw": draw + 1, "secagg_clamped": inputs("edge", n, rank)[3]}


def _peer_worker(rank, world, path, q):
    import torch.distributed as dist

    torch.cuda.set_device(0)
    from fedmi.parallel.fedavg import FedAvg
    from fedmi.parallel.peer import PeerAllReduce

    dev, n, msgs = torch.device("cuda", 0), 1027, []
    try:
        pc = PeerAllReduce(rank, world, 4 * 4099 + 4096, dist.FileStore(path, world), tag="sa")

        def dense(it):
            x = _dense(rank, it).to(dev)
            pc.allreduce_mean_(x)
            if not torch.equal(x.cpu(), _dense_mean(world, it)):
                msgs.append(f"dense all-reduce {it} on the same communicator != its mean")

        dense(0)
        a = inputs("randn", n, 0)[1]
        guard = sa.make_secagg(True, _GpuStub(torch.from_numpy(a.copy()).to(dev)), R)     # keys by X25519 over the peers
        fa = FedAvg(secagg=guard, transport=pc)
        t = _GpuStub(torch.from_numpy(inputs("randn", n, rank)[0].copy()).to(dev), 10 + 3 * rank)
        fa.average(t)
        torch.cuda.synchronize()
        got = t.flat.cpu().numpy()
        qs = [sc.encode(inputs("randn", n, r)[0], a, F)[0] for r in range(world)]        # every update from the one anchor
        total = sum(qs)
        want = a + (total.astype(np.float64) * 2.0 ** -F / world).astype(np.float32)      # the masks are gone
        if got.tobytes() != want.tobytes() or t.ints[0].item() != sum(10 + 3 * r for r in range(world)) // world:
            msgs.append("the aggregate is not the rule's decode of the sum of q")
        seen = guard._rows[1, :n].cpu().numpy().view(np.uint32)      # what rank 1 put on the wire
        if rank == 0 and (seen != (qs[1] & sc.M32)).mean() < 0.99:
            msgs.append("rank 1's row is readable")
        if fa.label() != "peer-oneshot-hipipc+pairwise" or guard.round_stats() != {"secagg_draw": 1, "secagg_clamped": 0}:
            msgs.append(f"label {fa.label()} stats {guard.round_stats()}")
        dense(1)
        err = pc.error()
        pc.close()
    except Exception as e:  # pragma: no cover - reported to the parent
        msgs.append(repr(e))
        got, err = np.zeros(1), -1
    q.put((rank, (msgs, err, got.tobytes())))


@pytest.mark.parametrize("world", [2, 3])
def test_peer_transport_round(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as td:
        procs = [ctx.Process(target=_peer_worker, args=(r, world, os.path.join(td, "store"), q)) for r in range(world)]
        for p in procs:
            p.start()
        out = dict(q.get(timeout=200) for _ in procs)
        for p in procs:
            p.join(timeout=60)
    for r in range(world):
        assert out[r][:2] == ([], 0), (r, out[r][0])
        assert out[r][2] == out[0][2], r
