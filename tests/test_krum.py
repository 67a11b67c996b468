"""Krum / multi-Krum on the CPU (fedmi/parallel/krum.py): the torch twin against the numpy reference of
tests/krum_check.py bit for bit, the counts, the config, the CLI guards, three gloo ranks and the drill.
The HIP kernels: tests/test_krum_gpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmi.parallel.fedavg import FedAvg
from fedmi.parallel.krum import KrumAgg, KrumConfig, krum_counts, krum_finish_torch, krum_torch
from fedmi.parallel.robust import RobustConfig, make_robust
from tests import krum_check as kc
from tests.helpers import free_port
from tests.test_geomed import drill_rows
from tests.test_robust import _Stub


@pytest.mark.parametrize("W", [2, 3, 5, 8, 16])
@pytest.mark.parametrize("multi", [False, True])
def test_twin_matches_reference_bit_for_bit(W, multi):
    for n, byz in ((1, 1), (5, 1), (1027, 1), (1027, 3)):
        rows = kc.inputs(W, n, attackers=min(byz, (W - 1) // 2))
        G = kc.gram(rows)
        got = krum_finish_torch(torch.from_numpy(G), byz, multi).numpy()
        assert got.tobytes() == kc.finish(G, W, byz, multi)[0].tobytes()
        z, stats = krum_torch(torch.from_numpy(rows), byz, multi)        # (torch's Gram: other last bits than numpy's)
        sel = [r for r in range(W) if stats[1, r] == 1.0]
        assert len(sel) == kc.counts(W, byz, multi)[2] and z.numpy().tobytes() == kc.select(rows, sel).tobytes()


def test_counts_config_and_factory():
    for W in range(2, 17):
        for F in (1, 2, 3, 7):
            f, k, m = krum_counts(W, F, True)
            assert f == max(0, min(F, (W - 3) // 2)) and k == max(1, W - f - 2) and m == W - f and 1 <= k <= W - 1
            assert (f, k, m) == kc.counts(W, F, True) == KrumConfig("multikrum", F).counts(W)
            assert krum_counts(W, F, False) == (f, k, 1)
    assert krum_counts(2, 1, True) == (0, 1, 2) and krum_counts(5, 1, True) == (1, 2, 4)
    cfg = KrumConfig("multikrum", 2)
    assert cfg.as_vector().tolist() == [1.0, 2.0] and KrumConfig().as_vector().tolist() == [0.0, 1.0]
    assert KrumConfig.KINDS == ("krum", "multikrum") and KrumConfig.FIELDS == ("kind", "byz")
    for bad in (("median",), ("geomed",), ("krum", 0), ("multikrum", -1)):
        with pytest.raises(ValueError):
            KrumConfig(*bad)
    agg = make_robust("multikrum", _Stub(), byz=2)
    assert isinstance(agg, KrumAgg) and agg.cfg == cfg and agg._rolled() == [] and agg.state_tensors() == []
    assert make_robust("krum", _Stub()).cfg == KrumConfig("krum", 1)
    assert FedAvg(robust=agg).label() == "none (single client)+multikrum"
    assert agg.round_stats() == {"robust_kind": "multikrum"}
    with pytest.raises(RuntimeError, match="'byz'"):
        agg.check_config(KrumConfig("multikrum", 1).as_vector(), 0)
    assert RobustConfig.KINDS == ("median", "trimmed")               # the coordinate-wise rules are what they were
    with pytest.raises(ValueError):
        RobustConfig("krum")


@pytest.mark.parametrize("argv,word", [
    (["--robust", "krum", "--robust-byz", "0"], "--robust-byz"),
    (["--robust", "krum", "--agg", "grpc"], "--agg collective"),
    (["--robust", "multikrum", "--compress", "int8"], "compression"),
    (["--robust", "krum", "--client-opt", "scaffold"], "scaffold"),
    (["--robust", "multikrum", "--dp-clip", "1", "--dp-noise", "0.5"], "--dp-noise"),
])
def test_cli_guards(capsys, argv, word):
    from fedmi.cli import client

    with pytest.raises(SystemExit) as e:
        client.main(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err
    a = client.build_parser().parse_args(["--robust", "multikrum", "--robust-byz", "2"])
    assert (a.robust, a.robust_byz) == ("multikrum", 2) and client.build_parser().parse_args([]).robust_byz == 1


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = _Stub(rank)
    fa = FedAvg(robust=make_robust("multikrum", t))
    fa.average(t)
    q.put((rank, (t.flat.numpy().copy(), t.ints[0].tolist(), fa.robust.round_stats(), fa.label())))
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
    z, stats = krum_torch(torch.stack([_Stub(r).flat for r in range(3)]), 1, True)
    for r in range(3):
        x, ints, got, label = res[r]
        assert x.tobytes() == z.numpy().tobytes() and ints == [13, -8] and label == "gloo-allreduce+multikrum"
        assert got == {"robust_kind": "multikrum", "robust_byz": 0, "robust_selected": [0, 1, 2],
                       "robust_score": stats[0, :3].tolist()}


@pytest.mark.parametrize("attack", ["scale -10", "all-nan"])
def test_drill_one_attacker_in_five(attack):
    rows = drill_rows()[:5].copy()
    if attack == "all-nan":
        rows[4] = np.nan
    for multi in (False, True):
        z, stats = krum_torch(torch.from_numpy(rows), 1, multi)
        assert stats[1, 4] == 0.0 and int(stats[1].sum()) == (4 if multi else 1) and torch.isfinite(z).all()
        assert stats[0, 4] == stats[0, :5].max() and (attack != "all-nan" or bool(torch.isinf(stats[2 + 4, :4]).all()))
    assert z.numpy().tobytes() == kc.select(rows, [0, 1, 2, 3]).tobytes()     # the mean of the other four
