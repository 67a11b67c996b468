"""DnC on the CPU (fedmi/parallel/dnc.py): the twin's finish against the reference of tests/dnc_check.py bit for bit,
the counts, the config, the factory, the CLI guards, three gloo ranks and the drill.  The kernels: tests/test_dnc_gpu.py."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmi.parallel.fedavg import FedAvg
from fedmi.parallel.krum import KrumConfig
from fedmi.parallel.robust import RobustConfig, make_robust
from tests import dnc_check as dc
from tests.helpers import free_port
from tests.test_geomed import drill_rows
from tests.test_robust import _Stub


@pytest.mark.parametrize("W", [2, 3, 5, 8, 16])
def test_twin_matches_reference_bit_for_bit(W):
    from fedmi.parallel.dnc import centred_gram_torch, dnc_finish_torch, dnc_torch

    for n, byz in ((1, 1), (5, 1), (1027, 1), (1027, 3)):
        rows = dc.inputs(W, n, attackers=dc.counts(W, byz)[0])
        for G in (dc.gram(rows), centred_gram_torch(torch.from_numpy(rows)).numpy()):    # centred twice, and once
            got, chosen = dnc_finish_torch(torch.from_numpy(G), byz)
            want, selected = dc.finish(G, W, byz)
            assert got.numpy().tobytes() == want.tobytes() and chosen == selected
        z, stats = dnc_torch(torch.from_numpy(rows), byz)
        assert stats.numpy().tobytes() == want.tobytes() and z.numpy().tobytes() == dc.select(rows, selected).tobytes()
        assert n == 1 or selected == list(range(dc.counts(W, byz)[1]))       # (one column: every score is 0 or equal)


def test_counts_config_and_factory():
    from fedmi.parallel.dnc import DncAgg, DncConfig, dnc_counts

    for W in range(2, 17):
        for F in (1, 2, 3, 7):
            f, m = dnc_counts(W, F)
            assert f == max(0, min(F, (W - 1) // 2)) and m == W - f and 2 * m > W
            assert (f, m) == dc.counts(W, F) == DncConfig("dnc", F).counts(W)
    assert dnc_counts(2, 1) == (0, 2) and dnc_counts(3, 1) == (1, 2) and dnc_counts(16, 9) == (7, 9)
    cfg = DncConfig("dnc", 2)
    assert cfg.as_vector().tolist() == [0.0, 2.0] and DncConfig() == DncConfig("dnc", 1)
    assert (DncConfig.KINDS, DncConfig.RULE, DncConfig.FIELDS) == (("dnc",), "DnC", ("kind", "byz"))
    assert RobustConfig.KINDS == ("median", "trimmed") and KrumConfig.KINDS == ("krum", "multikrum")
    for cls, bad in ((DncConfig, ("krum",)), (DncConfig, ("dnc", 0)), (RobustConfig, ("dnc",)), (KrumConfig, ("dnc",))):
        with pytest.raises(ValueError):
            cls(*bad)
    agg = make_robust("dnc", _Stub(), byz=2)
    assert isinstance(agg, DncAgg) and agg.cfg == cfg and agg._rolled() == [] and agg.state_tensors() == []
    assert FedAvg(robust=agg).label() == "none (single client)+dnc" and agg.round_stats() == {"robust_kind": "dnc"}
    with pytest.raises(RuntimeError, match="'byz'"):
        agg.check_config(DncConfig("dnc", 1).as_vector(), 0)


@pytest.mark.parametrize("argv,word", [(["--robust-byz", "0"], "--robust-byz"), (["--agg", "grpc"], "--agg collective"),
                                       (["--compress", "int8"], "compression")])
def test_cli_guards(capsys, argv, word):
    from fedmi.cli import client

    with pytest.raises(SystemExit) as e:
        client.main(["--robust", "dnc", *argv])
    assert e.value.code == 2 and word in capsys.readouterr().err
    a = client.build_parser().parse_args(["--robust", "dnc", "--robust-byz", "2"])
    assert (a.robust, a.robust_byz) == ("dnc", 2)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = _Stub(rank)
    fa = FedAvg(robust=make_robust("dnc", t))
    fa.average(t)
    q.put((rank, (t.flat.numpy().copy(), t.ints[0].tolist(), fa.robust.round_stats(), fa.label())))
    dist.destroy_process_group()


def test_three_gloo_ranks_hold_the_same_bits():
    from fedmi.parallel.dnc import dnc_torch

    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), free_port()
    procs = [ctx.Process(target=_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    z, stats = dnc_torch(torch.stack([_Stub(r).flat for r in range(3)]), 1)
    selected = [r for r in range(3) if stats[1, r] == 1.0]
    for r in range(3):
        x, ints, got, label = res[r]
        assert x.tobytes() == z.numpy().tobytes() and ints == [13, -8] and label == "gloo-allreduce+dnc"
        assert len(selected) == 2 and got == {"robust_kind": "dnc", "robust_byz": 1, "robust_selected": selected,
                                              "robust_score": stats[0, :3].tolist()}


@pytest.mark.parametrize("attack", ["scale -10", "all-nan"])
def test_drill_one_attacker_in_five(attack):
    from fedmi.parallel.dnc import dnc_torch

    rows = drill_rows()[:5].copy()
    if attack == "all-nan":
        rows[4] = np.nan
    z, stats = dnc_torch(torch.from_numpy(rows), 1)
    assert stats[1].tolist() == [1.0] * 4 + [0.0] * 12 and torch.isfinite(z).all()
    assert stats[0, 4] == stats[0, :5].max() and (attack != "all-nan" or bool(torch.isinf(stats[0, 4])))
    assert z.numpy().tobytes() == dc.select(rows, [0, 1, 2, 3]).tobytes()     # the mean of the other four
