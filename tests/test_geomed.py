"""Geometric-median aggregation on the CPU (fedmi/parallel/geomed.py): the torch twin against the fp64 reference of
tests/geomed_check.py link by link, the rule's properties, the config, the CLI guards, two gloo ranks and the drill.
The HIP kernels: tests/test_geomed_gpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmi.parallel.fedavg import FedAvg
from fedmi.parallel.geomed import GeoMedAgg, GeoMedConfig, geomed_torch
from fedmi.parallel.robust import RobustConfig, make_robust
from tests import geomed_check as gc
from tests.helpers import free_port
from tests.test_robust import _Stub

NU = 1e-6


def drill_rows() -> np.ndarray:
    """Five clients: four honest ``g + 0.1 randn``, the last sends ``-10 g``; row 5 is ``g`` itself (not a client)."""
    rng = np.random.default_rng(7)
    g = rng.standard_normal(1027)
    return np.stack([g + 0.1 * rng.standard_normal(1027) for _ in range(4)] + [-10.0 * g, g]).astype(np.float32)


def drill_errors(rows6: np.ndarray, z) -> tuple:
    """The distances of ``z`` and of the clients' plain mean from the honest mean, in units of ``|g|``."""
    x = rows6.astype(np.float64)
    honest, scale = x[:4].mean(0), np.linalg.norm(x[5])
    return (np.linalg.norm(np.asarray(z, dtype=np.float64) - honest) / scale,
            np.linalg.norm(x[:5].mean(0) - honest) / scale)


@pytest.mark.parametrize("W", [2, 3, 5, 16])
@pytest.mark.parametrize("n", [1, 5, 1027])
def test_twin_matches_reference_link_by_link(W, n):
    """Every pass of the twin is pinned from its own intermediates: row 0 from the rows, every row's dist and w from
    its sumsq, the final z from row T - 1's weights, row T's sumsq from the final z."""
    rows, T = gc.inputs(W, n), 4
    z, hist = geomed_torch(torch.from_numpy(rows.copy()), T, NU)
    z, hist = z.numpy(), hist.numpy()
    z0, h0 = geomed_torch(torch.from_numpy(rows.copy()), 0, NU)    # pass 0 alone
    gc.check_pass(rows, None, z0.numpy(), h0.numpy()[0], NU, f"pass 0 W={W} n={n}")
    assert np.array_equal(h0.numpy()[0], hist[0])
    for t in range(T + 1):
        dist_t, w_t = gc.finish_ref(hist[t][0], NU)
        assert gc.near(hist[t][1], dist_t, 4 * np.spacing(dist_t)) and gc.near(hist[t][2], w_t, 4 * np.spacing(w_t))
    gc.check_pass(rows, hist[T - 1][2].astype(np.float32), z, hist[T], NU, f"W={W} n={n}")


def test_four_points_approach_their_centre():
    """c +- a u, c +- b v with u orthogonal to v: the geometric median is c."""
    rng = np.random.default_rng(1)
    c, u, v = rng.standard_normal((3, 64))
    v -= u * (u @ v) / (u @ u)
    rows = np.stack([c + 3 * u, c - 3 * u, c + 0.5 * v, c - 0.5 * v]).astype(np.float32)
    z, hist = geomed_torch(torch.from_numpy(rows), 32, NU)
    assert np.linalg.norm(z.numpy() - c) < 1e-4 * np.linalg.norm(c)
    assert np.linalg.norm(gc.iterate(rows, 32, NU)[0] - c) < 1e-4 * np.linalg.norm(c)
    assert gc.near(hist[31, 2].numpy(), gc.iterate(rows, 32, NU)[1], 1e-4)


def test_config_and_factory():
    cfg = GeoMedConfig("geomed", 6, 1e-3)
    assert cfg.as_vector().tolist() == [0.0, 6.0, 1e-3] and GeoMedConfig().as_vector().tolist() == [0.0, 8.0, 1e-6]
    for bad in (("krum",), ("geomed", 0), ("geomed", 65), ("geomed", 8, 0.0), ("geomed", 8, -1.0), ("median",)):
        with pytest.raises(ValueError):
            GeoMedConfig(*bad)
    agg = make_robust("geomed", _Stub(), iters=6, nu=1e-3)
    assert isinstance(agg, GeoMedAgg) and agg.cfg == cfg and agg._rolled() == [] and agg.state_tensors() == []
    fa = FedAvg(robust=agg)
    fa.snapshot_opts(), fa.rollback_opts(), fa.reset_opts(_Stub())
    assert fa.label() == "none (single client)+geomed"
    assert agg.round_stats() == {"robust_kind": "geomed", "robust_iters": 6}
    with pytest.raises(RuntimeError, match="'iters'"):
        agg.check_config(GeoMedConfig("geomed", 8, 1e-3).as_vector(), 0)
    with pytest.raises(RuntimeError, match="'nu'"):
        agg.check_config(GeoMedConfig("geomed", 6, 1e-6).as_vector(), 0)
    # the coordinate-wise rules are what they were
    assert RobustConfig.KINDS == ("median", "trimmed") and RobustConfig.FIELDS == ("kind", "trim")
    assert RobustConfig("trimmed", 2).as_vector().tolist() == [1.0, 2.0]
    with pytest.raises(ValueError):
        RobustConfig("geomed")


@pytest.mark.parametrize("argv,word", [
    (["--robust", "geomed", "--robust-iters", "0"], "--robust-iters"),
    (["--robust", "geomed", "--robust-iters", "65"], "--robust-iters"),
    (["--robust", "geomed", "--robust-nu", "0"], "--robust-nu"),
    (["--robust", "geomed", "--agg", "grpc"], "--agg collective"),
    (["--robust", "geomed", "--compress", "int8"], "compression"),
    (["--robust", "geomed", "--client-opt", "scaffold"], "scaffold"),
    (["--robust", "geomed", "--dp-clip", "1", "--dp-noise", "0.5"], "--dp-noise"),
])
def test_cli_guards(capsys, argv, word):
    from fedmi.cli import client

    with pytest.raises(SystemExit) as e:
        client.main(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err
    a = client.build_parser().parse_args(["--robust", "geomed", "--robust-iters", "3", "--robust-nu", "1e-4"])
    assert (a.robust, a.robust_iters, a.robust_nu) == ("geomed", 3, 1e-4)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = _Stub(rank)
    fa = FedAvg(robust=make_robust("geomed", t, iters=3))
    fa.average(t)
    q.put((rank, (t.flat.numpy().copy(), t.ints[0].tolist(), fa.robust.round_stats(), fa.label())))
    dist.destroy_process_group()


def test_two_gloo_ranks_hold_the_same_bits():
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    rows = torch.stack([_Stub(0).flat, _Stub(1).flat])
    z, hist = geomed_torch(rows, 3, NU)
    for r in range(2):
        x, ints, stats, label = res[r]
        assert x.tobytes() == z.numpy().tobytes() and ints == [11, -8] and label == "gloo-allreduce+geomed"
        assert stats == {"robust_kind": "geomed", "robust_iters": 3, "robust_weight": hist[2, 2].tolist(),
                         "robust_dist": hist[3, 1].tolist()}


def test_drill_one_attacker_in_five():
    rows6 = drill_rows()
    rows = rows6[:5].copy()
    ref, plain = drill_errors(rows6, gc.iterate(rows, 6, NU)[0])
    z, hist = geomed_torch(torch.from_numpy(rows), 6, NU)
    got, _ = drill_errors(rows6, z.numpy())
    print(f"drill: reference {ref:.4f}, twin {got:.4f}, plain mean {plain:.4f}, weights {hist[5, 2].tolist()}")
    assert ref < 0.1 and got < 0.1 and plain > 1.0
    assert int(hist[5, 2].argmin()) == 4                 # the attacker is the client with the smallest weight


@pytest.mark.parametrize("n,grid", [(5, 1), (1027, 1), (3077, 4), (3077, 2), (4103, 1)])
def test_the_emulated_order_is_the_kernels_loops(n, grid):
    """The vectorised emulation of the kernels' summation order equals the plain loops bit for bit, at the launcher's
    grid and at smaller ones, where every lane strides two or five times."""
    rows = gc.inputs_mixed(3, n)
    z = gc.z_ref(rows)[0].astype(np.float32)
    assert grid <= gc.flat_grid(n) == (4 if n == 3077 else 1 if n < 4103 else 5)
    assert gc.sumsq_in_kernel_order(rows, z, grid).tobytes() == gc.sumsq_in_kernel_order_loops(rows, z, grid).tobytes()
    assert gc.near(gc.sumsq_in_kernel_order(rows, z), gc.sumsq_ref(rows, z), (n + 256 + 2048) * gc.U64 * gc.sumsq_ref(rows, z))


@pytest.mark.parametrize("W", [2, 5, 16])
@pytest.mark.parametrize("n", [1027, 3077])
def test_a_reordered_sum_is_caught(W, n):
    """On the inputs of the GPU test of the order, a pairwise tree over the same exact terms (numpy's sum) and the
    lanes' chains in rank-major blocks differ from the kernels' order in at least one bit: the bit-for-bit comparison
    can tell a reordered sum from the original.  (At n = 5 one lane adds five terms in index order: nothing to reorder.)"""
    rows = gc.inputs_mixed(W, n)
    for w in (None, gc.weights(W)):
        z = gc.z_ref(rows, w)[0].astype(np.float32)
        right = gc.sumsq_in_kernel_order(rows, z)
        assert gc.squares(rows, z).sum(1).tobytes() != right.tobytes()
        assert np.cumsum(gc.squares(rows, z), axis=1)[:, -1].tobytes() != right.tobytes()     # one chain in index order
