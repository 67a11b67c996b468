"""Secure aggregation on the CPU (fedmi/parallel/secagg.py): the ChaCha20 block and X25519 against their RFCs, the
package's numpy twin against tests/secagg_check.py, the masks' cancellation, the decode's bound, three gloo ranks,
the draw counter, the config and the CLI guards.  The HIP kernels: tests/test_secagg_gpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmi.parallel import secagg as sa
from fedmi.parallel.fedavg import FedAvg
from fedmi.parallel.server_opt import make_server_opt
from tests import secagg_check as sc
from tests.helpers import free_port
from tests.test_robust import _Stub

# RFC 8439 section 2.3.2: key 00..1f, counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00
RFC_KEY = np.frombuffer(bytes(range(32)), dtype="<u4")
RFC_NONCE = (0x09000000, 0x4A000000, 0)
RFC_BLOCK = [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3, 0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
             0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9, 0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]


def tables(W: int, seed: int = 5) -> np.ndarray:
    """``[W, W, 8]``: rank r's key table."""
    return np.stack([sa.key_table([None if j == r else sa.seeded_key(seed, r, j) for j in range(W)]) for r in range(W)])


def states(W: int, n: int, R: float = 8.0, seed: int = 0):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(np.float32)
    return (a + 0.1 * R * rng.standard_normal((W, n))).astype(np.float32), a


def test_chacha20_block_is_rfc8439():
    assert sc.chacha20_block(RFC_KEY, [1], RFC_NONCE)[0].tolist() == RFC_BLOCK
    got = sa.chacha20_blocks(RFC_KEY, np.array([0, 1, 2]), RFC_NONCE)
    assert got.tobytes() == sc.chacha20_block(RFC_KEY, [0, 1, 2], RFC_NONCE).tobytes() and got[1].tolist() == RFC_BLOCK


def test_x25519_is_rfc7748():
    nine = (9).to_bytes(32, "little")
    assert sa.x25519(nine, nine).hex() == "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
    a, b = bytes(range(1, 33)), bytes(range(101, 133))
    assert sa.x25519(a, sa.x25519(b, nine)) == sa.x25519(b, sa.x25519(a, nine))
    ka, kb = sa.pair_key(a, sa.x25519(b, nine), 2, 0), sa.pair_key(b, sa.x25519(a, nine), 0, 2)
    assert ka == kb and len(ka) == 32 and ka != sa.pair_key(a, sa.x25519(b, nine), 2, 1)


@pytest.mark.parametrize("W", [2, 3, 16])
def test_masks_cancel_hide_and_decode_within_the_bound(W):
    n, f, draw = 1027, 24, (7 << 32) | 3
    x, a = states(W, n)
    keys = tables(W)
    us = [sc.mask(x[r], a, keys[r], r, draw, f) for r in range(W)]
    q = np.stack([sc.encode(x[r], a, f)[0] for r in range(W)])
    assert all(c == 0 for _, c in us)
    rows = np.stack([u for u, _ in us])
    assert ((rows.astype(np.int64).sum(0) - q.sum(0)) & sc.M32 == 0).all()
    assert (rows[0] != (q[0] & sc.M32)).mean() >= 0.99
    # the package's twin is the same function
    for r in (0, W - 1):
        u, c = sa.mask_np(x[r], a, keys[r], r, draw, f)
        assert u.tobytes() == rows[r].tobytes() and c == 0
    got = sa.unmask_np(rows, a, f)
    assert got.tobytes() == sc.decode(rows, a, f).tobytes()
    # derived: 2^-(f+1) of the rounding to fixed point, half an ulp of m, half an ulp of a + m
    mean = (x - a).astype(np.float64).mean(0)
    bound = 2.0 ** -(f + 1) + 0.5 * np.spacing(np.abs(mean).astype(np.float32)) + 0.5 * np.spacing(np.abs(got))
    assert (np.abs(got.astype(np.float64) - (a.astype(np.float64) + mean)) <= bound * (1 + 1e-6)).all()


def test_encode_clamps_and_counts():
    a = np.zeros(10, dtype=np.float32)
    x = np.array([8, -8, 16, -16, np.inf, -np.inf, np.nan, -np.nan, -0.0, 1.5 * 2.0 ** -24], dtype=np.float32)
    q, clamped = sc.encode(x, a, 24)
    assert q.tolist() == [sc.Q_MAX, -sc.Q_MAX] * 3 + [0, 0, 0, 2] and clamped == 8
    u, c = sa.encode_np(x, a, 24)
    assert u.tolist() == (q & sc.M32).tolist() and c == 8


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    plain = _Stub(rank)
    plain.flat = 0.5 * plain.flat + _Stub(99).flat        # updates of size 0.5 around a common model
    FedAvg(secagg=sa.make_secagg(True, _Stub(99))).average(plain)       # keys from the X25519 exchange over gloo
    t = _Stub(rank)
    t.flat = 0.5 * t.flat + _Stub(99).flat
    guard = sa.make_secagg(True, _Stub(99))
    fa = FedAvg(secagg=guard, server_opt=make_server_opt("fedavgm", _Stub(99)))
    fa.snapshot_opts()
    fa.average(t)
    first = t.flat.numpy().copy()
    fa.rollback_opts()                                    # a void round: the anchor returns, the draw does not
    rolled = (guard.draw, guard.anchor.numpy().tobytes() == _Stub(99).flat.numpy().tobytes())
    fa.average(t)
    q.put((rank, (plain.flat.numpy().copy(), first, t.flat.numpy().copy(), rolled, guard.round_stats(), fa.label(),
                  t.ints[0].tolist())))
    dist.destroy_process_group()


def test_three_gloo_ranks_hold_the_same_bits():
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), free_port()
    procs = [ctx.Process(target=_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    a = _Stub(99).flat.numpy()
    x = np.stack([0.5 * _Stub(r).flat.numpy() + a for r in range(3)])
    q_sum = sum(sc.encode(x[r], a, 24)[0] for r in range(3))
    mean = a + (q_sum.astype(np.float64) * 2.0 ** -24 / 3.0).astype(np.float32)       # the masks are gone: sum of q
    for r in range(3):
        plain, first, second, rolled, stats, label, ints = res[r]
        assert plain.tobytes() == mean.tobytes()
        assert first.tobytes() == res[0][1].tobytes() and second.tobytes() == res[0][2].tobytes()
        assert np.allclose(first, mean, rtol=0, atol=1e-6)            # fedavgm at lr 1, first step: a + (mean - a)
        assert rolled == (1, True) and stats == {"secagg_draw": 2, "secagg_clamped": 0}
        assert label == "gloo-allreduce+fedavgm+pairwise" and ints == [13, -8]


def test_config():
    assert [sa.frac_bits(R) for R in (2.0 ** -8, 1.0, 8.0, 256.0)] == [35, 27, 24, 19]
    for bad in (0.0, 3.0, 512.0, 2.0 ** -9, -8.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sa.SecAggConfig("pairwise", bad)
    guard = sa.make_secagg(True, _Stub(), 4.0)
    assert guard.cfg.as_vector().tolist() == [0.0, 4.0] and sa.make_secagg(False) is None
    with pytest.raises(RuntimeError, match="'range'"):
        guard.check_config(sa.SecAggConfig("pairwise", 8.0).as_vector(), 0)
    guard.draw = 41                                       # a joining client takes the survivors' draw
    (t,) = guard.state_tensors()
    t.fill_(77)
    guard.reset(_Stub())
    assert guard.draw == 77 and guard._rolled() == [guard.anchor]


@pytest.mark.parametrize("argv,word", [
    (["--secagg", "--agg", "grpc"], "--agg collective"),
    (["--secagg", "--compress", "int8"], "compression"),
    (["--secagg", "-c", "Y"], "compression"),
    (["--secagg", "--robust", "median"], "--robust"),
    (["--secagg", "--client-opt", "scaffold"], "scaffold"),
    (["--secagg", "--secagg-range", "3"], "power of two"),
    (["--secagg", "--secagg-range", "512"], "power of two"),
])
def test_cli_guards(capsys, argv, word):
    from fedmi.cli import client

    with pytest.raises(SystemExit) as e:
        client.main(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err
    a = client.build_parser().parse_args(["--secagg", "--secagg-range", "0.5", "--secagg-seed", "3"])
    assert (a.secagg, a.secagg_range, a.secagg_seed) == (True, 0.5, 3)
    assert "VOIDS" in client.build_parser().format_help() and not client.build_parser().parse_args([]).secagg
