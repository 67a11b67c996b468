"""Bulyan on the CPU (fedmi/parallel/bulyan.py): the torch twin against the reference of tests/bulyan_check.py bit for
bit, the CLI guards, BulyanAgg's round_stats on a stub and a simulated federation under attack.
The HIP kernels: tests/test_bulyan_gpu.py."""
import json

import numpy as np
import pytest
import torch

from fedmi.parallel.bulyan import (BulyanAgg, BulyanConfig, bulyan_counts, bulyan_fold_torch, bulyan_select_torch,
                                   bulyan_torch)
from fedmi.parallel.krum import gram_select_torch
from fedmi.parallel.robust import GatheredAgg, make_robust
from tests import bulyan_check as bc
from tests import krum_check as kc
from tests.robust_check import same_bits
from tests.test_robust import _sim, _Stub


@pytest.mark.parametrize("W", [2, 7, 11, 16])
@pytest.mark.parametrize("n", [3, 1027])
def test_twin_matches_reference_bit_for_bit(W, n):
    f, theta, c, beta = bc.counts(W, 3)
    assert (f, theta, c, beta) == bulyan_counts(W, 3) == BulyanConfig("bulyan", 3).counts(W) and beta >= 1
    rows = bc.inputs(W, n, attackers=f)
    G = bc.gram(rows)
    want, want_sel, _ = bc.select(G, W, 3)
    got, sel = bulyan_select_torch(torch.from_numpy(G), 3)
    assert got.numpy().tobytes() == want.tobytes() and sel == want_sel and len(sel) == theta
    z, stats = bulyan_torch(torch.from_numpy(rows), 3)                   # (torch's Gram: other last bits than numpy's)
    out, ref, _ = bc.reference(rows, G, 3)
    assert z.numpy().tobytes() == out.tobytes() and stats.numpy()[[1, 18]].tobytes() == ref[[1, 18]].tobytes()
    assert not set(sel) & set(range(W - f, W))                           # no attacker is selected


@pytest.mark.parametrize("W", [2, 3, 7, 9, 16])
@pytest.mark.parametrize("F", [1, 3])
def test_one_selection_loop_is_both_rules(W, F):
    """The shared loop with Krum's counts (one round of m picks) and with Bulyan's (theta rounds of one) equals either
    rule's own reference: stats bytes and picked ranks; a tail alone, a long row, and a long row with one NaN client."""
    for n, nan_client in ((1, None), (1027, None), (1027, W // 2)):
        rows = bc.inputs(W, n).copy()
        if nan_client is not None:
            rows[nan_client] = np.nan
        G = bc.gram(rows)
        for multi in (False, True):
            f, _, m = kc.counts(W, F, multi)
            want, want_sel = kc.finish(G, W, F, multi)
            got, sel = gram_select_torch(torch.from_numpy(G), f, 1, m)
            assert got.numpy().tobytes() == want.tobytes() and sel == want_sel and len(sel) == m
        f, theta, _, _ = bc.counts(W, F)
        want, want_sel, _ = bc.select(G, W, F)
        got, sel = gram_select_torch(torch.from_numpy(G), f, theta, 1, 19)
        assert got.numpy().tobytes() == want.tobytes() and sel == want_sel and len(sel) == theta


@pytest.mark.parametrize("theta,c", [(2, 0), (3, 2), (5, 4), (8, 2), (9, 6), (16, 6)])
def test_twin_fold_on_the_edge_columns(theta, c):
    record = sorted(np.random.default_rng(theta).permutation(16)[:theta].tolist())
    rows = bc.fold_inputs(1027, record, c)
    out, cut = bulyan_fold_torch(torch.from_numpy(rows[record]), c)
    want, want_cut = bc.fold(rows, record, c)
    assert same_bits(out.numpy(), want) == "" and cut.tolist() == want_cut[record].tolist()
    assert int(want_cut.sum()) == c * 1027 and np.isnan(want).sum() >= (1 if c else 2)


@pytest.mark.parametrize("argv,word", [
    (["--robust", "bulyan", "--robust-byz", "0"], "--robust-byz"),
    (["--robust", "bulyan", "--agg", "grpc"], "--agg collective"),
    (["--robust", "bulyan", "--compress", "int8"], "compression"),
    (["--robust", "bulyan", "--client-opt", "scaffold"], "scaffold"),
    (["--robust", "bulyan", "--dp-clip", "1", "--dp-noise", "0.5"], "--dp-noise"),
])
def test_cli_guards(capsys, argv, word):
    from fedmi.cli import client

    with pytest.raises(SystemExit) as e:
        client.main(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err
    a = client.build_parser().parse_args(["--robust", "bulyan", "--robust-byz", "2"])
    assert (a.robust, a.robust_byz) == ("bulyan", 2)


def test_factory_and_round_stats_on_a_stub(monkeypatch):
    rows = bc.inputs(7, 1027, attackers=1)
    monkeypatch.setattr(GatheredAgg, "_all_gather", staticmethod(
        lambda views, x, group, abort: [v.copy_(torch.from_numpy(rows[r].copy())) for r, v in enumerate(views)]))
    t = _Stub(2)
    agg = make_robust("bulyan", t, byz=2)
    assert isinstance(agg, BulyanAgg) and agg.cfg == BulyanConfig("bulyan", 2) and agg.round_stats() == {
        "robust_kind": "bulyan"}
    fedavg = type("F", (), {"transport": None, "group": None, "abort": None, "world": lambda self: 7})()
    agg.aggregate(t, fedavg)
    z, stats = bulyan_torch(torch.from_numpy(rows), 2)
    assert t.flat.numpy().tobytes() == z.numpy().tobytes()
    assert agg.round_stats() == {"robust_kind": "bulyan", "robust_byz": 1, "robust_selected": [0, 1, 2, 3, 4],
                                 "robust_score": stats[0, :7].tolist(),
                                 "robust_cut": [int(v) for v in stats[18, :7].tolist()]}
    assert sum(agg.round_stats()["robust_cut"]) == 2 * 1027 and agg.round_stats()["robust_cut"][5:] == [0, 0]


def test_simulated_federation_keeps_the_attacker_out(tmp_path, monkeypatch):
    monkeypatch.setenv("FEDMI_TORCH_PATH", "1")                          # (main sets it for --engine fp32: restored here)
    out = tmp_path / "sim.jsonl"
    assert _sim().main(["--model", "lenet", "--engine", "fp32", "--clients", "7", "--rounds", "1", "--n-train", "1792",
                        "--n-test", "64", "--robust", "bulyan", "--attack", "signflip", "--attackers", "1",
                        "--out", str(out)]) == 0
    rec = json.loads(out.read_text().splitlines()[-1])
    assert rec["robust_kind"] == "bulyan" and rec["robust_byz"] == 1 and rec["finite"]
    assert len(rec["robust_selected"]) == 5 and 6 not in rec["robust_selected"] and rec["robust_cut"][6] == 0
