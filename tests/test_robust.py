"""Byzantine-robust aggregation on the CPU (fedmi/parallel/robust.py): the torch twin against the exact numpy
reference of tests/robust_check.py bit for bit, the rule's properties, FedAvg over three gloo ranks, the CLI guards
and the attack drill.  The HIP kernels: tests/test_robust_gpu.py."""
import fractions
import importlib.util
import os
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmi.parallel.fedavg import FedAvg
from fedmi.parallel.robust import RobustAgg, RobustConfig, make_robust, robust_reduce_torch, sort_key
from fedmi.parallel.server_opt import make_server_opt
from tests import robust_check as rc
from tests.helpers import free_port

WORLDS = tuple(range(2, 17))


def _sim():
    spec = importlib.util.spec_from_file_location("fedavg_sim", Path(__file__).resolve().parent.parent / "tools" /
                                                  "fedavg_sim.py")
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    return sim


class _Stub:
    """Minimal LocalTrainer surface used by FedAvg / RobustAgg / ServerOpt."""

    def __init__(self, rank: int = 0, n: int = 1027, k: int = 800):
        self.flat = torch.randn(n, generator=torch.Generator().manual_seed(100 + rank))
        self.ints = [torch.tensor([10 + 3 * rank, -7 - rank], dtype=torch.int64)]
        self.k = k
        self.packs = 0

    def float_state(self):
        return self.flat

    def n_params(self):
        return self.k

    def int_state(self):
        return self.ints

    def after_aggregate(self):
        self.packs += 1


# ---- 1. the reference itself -------------------------------------------------------------------------------------------------
def test_reference_order_is_sorted_by_value_then_rank():
    """The reference's sort step against Python's ``sorted`` on (exact value, rank)."""
    pool = np.array([-3e38, -2.5, -1.0, -1e-40, 1e-45, 1e-40, 0.5, 1.0, 1.0000001, 3e38], dtype=np.float32)
    rng = np.random.default_rng(5)
    for W in (2, 3, 5, 8, 16):
        x = rng.choice(pool, size=(W, 40))
        order = np.argsort(rc.sort_key(x), axis=0, kind="stable")
        for i in range(x.shape[1]):
            want = sorted(range(W), key=lambda r: (fractions.Fraction(float(x[r, i])), r))
            assert order[:, i].tolist() == want, (W, i)
    # what exact values cannot say: -0 sorts before +0, the infinities at the ends, every NaN last
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 3e38, -3e38], dtype=np.float32)
    k = rc.sort_key(sp).tolist()
    assert k[3] < k[7] < k[1] < k[0] < k[6] < k[2] < k[4] == k[5] == 0xFFFFFFFF
    assert k[1] == 0x7FFFFFFF and k[0] == 0x80000000


def test_reference_small_example():
    rows = np.array([[1.0, np.nan], [5.0, 2.0], [-4.0, 2.0], [2.0, -1.0], [100.0, 0.0]], dtype=np.float32)
    out, cut = rc.reference(rows, 1)
    assert out.tolist() == [np.float32(np.float32(1.0 + 2.0) + 5.0) / np.float32(3.0), np.float32(4.0) / np.float32(3.0)]
    assert cut.tolist() == [1, 0, 1, 1, 1]          # coordinate 1's tie at 2.0: rank 1 before rank 2, both kept
    out, cut = rc.reference(rows, 2)
    assert out.tolist() == [2.0, 2.0] and cut.tolist() == [2, 1, 2, 1, 2]


# ---- 2. the torch twin against the reference ---------------------------------------------------------------------------------
def test_twin_key_matches_reference():
    x = rc.inputs("extremes", 16, 1027)
    nan = rc.inputs("nan", 16, 1027, 7)
    for a in (x, nan):
        assert np.array_equal(sort_key(torch.from_numpy(a.copy())).numpy().astype(np.uint32), rc.sort_key(a))


@pytest.mark.parametrize("W", WORLDS)
def test_twin_matches_reference_bit_for_bit(W):
    for b in range(rc.b_max(W) + 1):
        for case in rc.data_cases(W, b):
            for n in rc.NS:
                rows = rc.inputs(case, W, n, b)
                want, want_cut = rc.reference(rows, b)
                got, cut = robust_reduce_torch(torch.from_numpy(rows.copy()), b)
                assert rc.same_bits(got.numpy(), want) == "", (case, W, b, n)
                assert cut.dtype == torch.int64 and cut.tolist() == want_cut.tolist(), (case, W, b, n)
                assert int(cut.sum()) == 2 * b * n
                if case == "nan+" and b + 1 <= W:
                    assert np.isnan(want[0]), "a NaN that survives the trim must propagate"


@pytest.mark.parametrize("W", [3, 4, 9, 16])
def test_row_permutation_keeps_the_bits_and_permutes_cut(W):
    n = 1027
    rows = rc.inputs("randn", W, n)                       # tie-free
    assert all(len(np.unique(rows[:, i])) == W for i in range(n))
    perm = np.random.default_rng(W).permutation(W)
    for b in range(rc.b_max(W) + 1):
        out, cut = robust_reduce_torch(torch.from_numpy(rows.copy()), b)
        out_p, cut_p = robust_reduce_torch(torch.from_numpy(rows[perm].copy()), b)
        assert torch.equal(out, out_p)
        assert cut_p.tolist() == cut[torch.from_numpy(perm)].tolist()


@pytest.mark.parametrize("W", WORLDS)
def test_garbage_rows_cannot_leave_the_honest_range(W):
    """At most b_eff rows replaced by NaN / inf / 1e30 of either sign: the result is finite and lies in the honest
    rows' per-coordinate [min, max], up to the rounding of the m-term fp32 mean (robust_check.mean_bound)."""
    n = 1027
    garbage = np.array([np.nan, -np.nan, np.inf, -np.inf, 1e30, -1e30], dtype=np.float32)
    rng = np.random.default_rng(100 + W)
    for b in range(1, rc.b_max(W) + 1):
        for k in range(1, b + 1):
            rows = rc.inputs("randn", W, n).copy()
            bad = rng.permutation(W)[:k]
            rows[bad] = rng.choice(garbage, size=(k, n))
            honest = np.delete(rows, bad, axis=0).astype(np.float64)
            lo, hi = honest.min(0), honest.max(0)
            out, _ = robust_reduce_torch(torch.from_numpy(rows), b)
            out = out.numpy().astype(np.float64)
            slack = rc.mean_bound(W - 2 * b) * np.maximum(np.abs(lo), np.abs(hi))
            assert np.isfinite(out).all(), (W, b, k)
            assert (out >= lo - slack).all() and (out <= hi + slack).all(), (W, b, k)


@pytest.mark.parametrize("W", [3, 5, 7, 9, 15])
def test_median_of_an_odd_world_is_an_input_value(W):
    for case in ("randn", "ties", "extremes"):
        rows = rc.inputs(case, W, 1027)
        out, cut = robust_reduce_torch(torch.from_numpy(rows.copy()), RobustConfig("median").b_eff(W))
        want = np.sort(rows.astype(np.float64), axis=0)[W // 2].astype(np.float32)    # ties and +-0: any order, same value
        assert np.array_equal(out.numpy(), want)
        hit = (out.numpy().view(np.uint32)[None, :] == rows.view(np.uint32)).any(0)
        assert hit.all()


# ---- 3. configuration ------------------------------------------------------------------------------------------------------
def test_b_eff_follows_a_shrinking_world():
    t = RobustConfig("trimmed", 2)
    assert [t.b_eff(w) for w in (8, 5, 4, 3, 2, 1)] == [2, 2, 1, 1, 0, 0]
    m = RobustConfig("median")
    assert [m.b_eff(w) for w in (8, 5, 3, 2)] == [3, 2, 1, 0]
    for kind, trim in (("median", 1), ("trimmed", 1), ("trimmed", 3)):
        for w in range(2, 17):
            assert RobustConfig(kind, trim).b_eff(w) == rc.b_eff(kind, trim, w)
    with pytest.raises(ValueError):
        RobustConfig("trimmed", 0)
    with pytest.raises(ValueError):
        RobustConfig("krum")
    with pytest.raises(ValueError):
        robust_reduce_torch(torch.zeros(4, 3), 2)


class _FakeFedAvg:
    """What RobustAgg.aggregate asks of its FedAvg: the world, no transport, a group and an abort flag."""

    transport = group = abort = None

    def __init__(self, world: int):
        self._world = world

    def world(self) -> int:
        return self._world


def test_aggregate_follows_a_shrinking_world(monkeypatch, capsys):
    """One RobustAgg through worlds 5 -> 3 -> 2 -> 2 (the collective replaced by a copy of the other clients' known
    states): the gather buffer is re-allocated when W changes and kept when it does not, b_eff follows, the result is
    the reference's at every world, and the note that nothing can be trimmed at 2 clients is logged once."""
    n, rank = 1027, 1
    state = {}

    def fake_all_gather(rows, x, group, abort):
        assert len(rows) == state["rows"].shape[0]
        for r, row in enumerate(rows):
            row.copy_(torch.from_numpy(state["rows"][r].copy()))

    monkeypatch.setattr(RobustAgg, "_all_gather", staticmethod(fake_all_gather))
    t = _Stub(n=n)
    agg = make_robust("trimmed", t, 2)
    bufs = []
    for W, b in ((5, 2), (3, 1), (2, 0), (2, 0)):
        state["rows"] = rc.inputs("randn", W, n)
        want, want_cut = rc.reference(state["rows"], b)
        t.flat.copy_(torch.from_numpy(state["rows"][rank].copy()))
        agg.aggregate(t, _FakeFedAvg(W))
        assert tuple(agg._rows.shape) == (W, 1028)
        bufs.append(agg._rows)
        assert rc.same_bits(t.flat.numpy(), want) == "", W
        assert agg.round_stats() == {"robust_kind": "trimmed", "robust_trim": b, "robust_cut": want_cut.tolist()}
    assert bufs[0] is not bufs[1] and bufs[1] is not bufs[2] and bufs[2] is bufs[3]
    assert capsys.readouterr().out.count("nothing can be trimmed") == 1
    agg.aggregate(t, _FakeFedAvg(1))                           # world 1: nothing happens
    with pytest.raises(ValueError):
        agg.aggregate(t, _FakeFedAvg(17))


def test_factory_and_the_replicated_contract():
    t = _Stub()
    assert make_robust("none", t) is None and make_robust(None, t) is None and FedAvg().robust is None
    r = make_robust("trimmed", t, 2)
    assert isinstance(r, RobustAgg) and r.cfg.as_vector().tolist() == [1.0, 2.0]
    assert r._rolled() == [] and r.state_tensors() == []
    fa = FedAvg(robust=r)
    assert fa.opts() == [r]
    fa.snapshot_opts()
    fa.rollback_opts()
    fa.reset_opts(t)
    with pytest.raises(RuntimeError, match="'trim'"):
        r.check_config(RobustConfig("trimmed", 1).as_vector(), 0)
    with pytest.raises(RuntimeError, match="'kind'"):
        r.check_config(RobustConfig("median", 2).as_vector(), 0)


def test_world1_is_bit_identical_to_plain_fedavg():
    a, b = _Stub(3), _Stub(3)
    fa = FedAvg(robust=make_robust("median", a))
    fa.average(a)
    FedAvg().average(b)
    assert torch.equal(a.flat, b.flat) and torch.equal(a.ints[0], b.ints[0]) and a.packs == b.packs == 1
    assert fa.label() == "none (single client)+median"
    assert fa.robust.round_stats() == {"robust_kind": "median"}      # nothing was launched, nothing was cut


# ---- 4. three gloo ranks -------------------------------------------------------------------------------------------------------
GLOO_WORLD = 3


def _state(rank: int) -> torch.Tensor:
    x = _Stub(rank).flat
    if rank == 2:
        x = x.clone()
        x[::7] = float("nan")
        x[1::7] = 1e30
    return x


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for tag, kind, trim in (("med", "median", 1), ("trim", "trimmed", 1)):
        t = _Stub(rank)
        t.flat.copy_(_state(rank))
        fa = FedAvg(robust=make_robust(kind, t, trim))
        fa.average(t)
        out.update({f"{tag}_x": t.flat.clone(), f"{tag}_ints": t.ints[0].clone(), f"{tag}_packs": t.packs,
                    f"{tag}_stats": fa.robust.round_stats(), f"{tag}_label": fa.label()})
    # a server optimizer on top: the step takes the robust aggregate as its end point
    t = _Stub(rank)
    t.flat.copy_(_Stub(0).flat)                                  # the common starting model: fedavgm's anchor
    fa = FedAvg(robust=make_robust("trimmed", t, 1), server_opt=make_server_opt("fedavgm", t, 0.7, 0.9))
    t.flat.copy_(_state(rank))
    fa.average(t)
    out["avgm_x"] = t.flat.clone()
    # a client with another --robust-trim must not join quietly
    t = _Stub(rank)
    try:
        FedAvg(robust=make_robust("trimmed", t, 1 if rank != 1 else 2)).resync(t, 0)
        out["mismatch"] = ""
    except RuntimeError as e:
        out["mismatch"] = str(e)
    q.put((rank, {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()}))
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def three_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, GLOO_WORLD, port, q)) for r in range(GLOO_WORLD)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def _stacked() -> np.ndarray:
    return np.stack([_state(r).numpy() for r in range(GLOO_WORLD)])


@pytest.mark.parametrize("tag,kind", [("med", "median"), ("trim", "trimmed")])
def test_gloo_every_rank_holds_the_reference_bits(three_ranks, tag, kind):
    b = rc.b_eff(kind, 1, GLOO_WORLD)
    want, want_cut = rc.reference(_stacked(), b)
    assert np.isfinite(want).all()                               # rank 2's NaN and 1e30 entries were cut
    for r in range(GLOO_WORLD):
        d = three_ranks[r]
        assert rc.same_bits(d[f"{tag}_x"], want) == "", r
        ints = [[10 + 3 * q for q in range(GLOO_WORLD)], [-7 - q for q in range(GLOO_WORLD)]]
        assert d[f"{tag}_ints"].tolist() == [sum(v) // GLOO_WORLD for v in ints]          # floor mean, as ever
        assert d[f"{tag}_packs"] == 1
        assert d[f"{tag}_stats"] == {"robust_kind": kind, "robust_trim": b, "robust_cut": want_cut.tolist()}
        assert d[f"{tag}_label"] == f"gloo-allreduce+{kind}"
    assert int(np.argmax(want_cut)) == 2


def test_gloo_server_step_takes_the_robust_aggregate(three_ranks):
    agg, _ = rc.reference(_stacked(), 1)
    t = _Stub(0)
    so = make_server_opt("fedavgm", t, 0.7, 0.9)
    t.flat.copy_(torch.from_numpy(agg))
    so.step(t)
    for r in range(GLOO_WORLD):
        assert rc.same_bits(three_ranks[r]["avgm_x"], t.flat.numpy()) == "", r


def test_gloo_resync_rejects_other_settings(three_ranks):
    assert three_ranks[0]["mismatch"] == "" and three_ranks[2]["mismatch"] == ""
    msg = three_ranks[1]["mismatch"]
    assert "'trim'" in msg and "rank 0" in msg and "--robust" in msg


# ---- 5. CLI ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,word", [
    (["--robust", "median", "--agg", "grpc"], "--agg collective"),
    (["--robust", "trimmed", "-c", "Y"], "compression"),
    (["--robust", "trimmed", "--compress", "int8"], "compression"),
    (["--robust", "median", "--compress", "topk"], "compression"),
    (["--robust", "median", "--client-opt", "scaffold"], "scaffold"),
    (["--robust", "trimmed", "--dp-clip", "1", "--dp-noise", "0.5"], "--dp-noise"),
    (["--robust", "trimmed", "--robust-trim", "0"], "--robust-trim"),
])
def test_cli_guards(capsys, argv, word):
    from fedmi.cli import client

    with pytest.raises(SystemExit) as e:
        client.main(argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_cli_flags_and_sim_guards(capsys):
    from fedmi.cli import client
    from fedmi.parallel.robust import check_robust_flags

    a = client.build_parser().parse_args([])
    assert (a.robust, a.robust_trim) == ("none", 1) and make_robust(a.robust, None, a.robust_trim) is None
    check_robust_flags(a, pytest.fail)
    a = client.build_parser().parse_args(["--robust", "trimmed", "--robust-trim", "2", "--dp-clip", "0.5",
                                          "--client-opt", "fedprox", "--server-opt", "fedavgm", "--compress", "none",
                                          "-c", "Y"])
    assert (a.robust, a.robust_trim) == ("trimmed", 2)
    check_robust_flags(a, pytest.fail)                # --dp-clip alone, fedprox and a server optimizer compose
    help_text = client.build_parser().format_help()
    assert "--robust" in help_text and "--robust-trim" in help_text and "--attack" not in help_text
    sim = _sim()
    for argv, word in ((["--robust", "median", "--client-opt", "scaffold"], "scaffold"),
                       (["--robust", "trimmed", "--robust-trim", "0"], "--robust-trim"),
                       (["--robust", "trimmed", "--dp-clip", "1", "--dp-noise", "1"], "--dp-noise"),
                       (["--attack", "scale", "--attackers", "3", "--clients", "2"], "--attackers")):
        with pytest.raises(SystemExit) as e:
            sim.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


# ---- 6. the attack drill -----------------------------------------------------------------------------------------------------
def _drill(attack: str, robust, rounds: int = 6):
    """Five clients on a small least-squares problem, gradient descent from the shared model; the last client
    attacks.  Returns the honest clients' mean loss before round 1 and after every round."""
    sim = _sim()
    g = torch.Generator().manual_seed(3)
    W, d, rows = 5, 8, 64
    w_true = torch.randn(d, generator=g)
    A = [torch.randn(rows, d, generator=g) for _ in range(W)]
    y = [a @ w_true + 0.01 * torch.randn(rows, generator=g) for a in A]

    def loss(w):
        return float(sum(((A[r] @ w - y[r]) ** 2).mean() for r in range(W - 1)) / (W - 1))

    w = torch.zeros(d)
    losses = [loss(w)]
    cuts = torch.zeros(W, dtype=torch.int64)
    for _ in range(rounds):
        states = []
        for r in range(W):
            x = w.clone()
            for _ in range(5):
                x = x - 0.05 * (2.0 / rows) * (A[r].T @ (A[r] @ x - y[r]))
            states.append(x)
        if attack != "none":
            states[-1] = sim.attack_state(attack, w, states[-1], -10.0)
        if robust is None:
            w = torch.stack(states).mean(0)
        else:
            w, cut = sim.robust_stack(robust, states)
            cuts += cut
        losses.append(loss(w))
    return losses, cuts


@pytest.mark.parametrize("attack", ["scale", "nan"])
def test_attack_drill(attack):
    trimmed = make_robust("trimmed", _Stub(), 1)
    plain, _ = _drill(attack, None)
    robust, cuts = _drill(attack, trimmed)
    print(f"{attack}: plain {plain[0]:.4g} -> {plain[-1]:.4g}, trimmed {robust[0]:.4g} -> {robust[-1]:.4g}, "
          f"cut {cuts.tolist()}")
    assert plain[0] == robust[0]
    if attack == "scale":
        assert plain[-1] > plain[0]                  # the mean update is -1.2 x the honest one: the loss climbs
        assert robust[-1] < plain[-1]
    else:
        assert not np.isfinite(plain[1])             # one all-NaN client: the plain mean is gone in round 1
    assert np.isfinite(robust).all() and robust[-1] < robust[0]
    assert int(cuts.argmax()) == 4                   # the attacker is the client the rule rejects


def test_attack_rules():
    sim = _sim()
    start, x = torch.tensor([1.0, 2.0]), torch.tensor([1.5, 1.0])
    assert sim.attack_state("signflip", start, x, 10.0).tolist() == [-4.0, 12.0]
    assert sim.attack_state("scale", start, x, -10.0).tolist() == [-4.0, 12.0]
    assert sim.attack_state("scale", start, x, 2.0).tolist() == [2.0, 0.0]
    assert torch.isnan(sim.attack_state("nan", start, x, 1.0)).all()
    with pytest.raises(ValueError):
        sim.attack_state("none", start, x, 1.0)


# ---- 7. three client agents over gloo ----------------------------------------------------------------------------------------
@pytest.mark.slow
def test_three_client_agents_log_robust_cut(tmp_path):
    """Three client processes + coordinator, ``--robust trimmed``: every round record carries ``robust_cut``, the same
    list on every client, with 2 b_eff n cuts in all."""
    from fedmi.control.coordinator import Coordinator, CoordinatorConfig
    from tests.helpers import read_jsonl, spawn_client, stop_proc, wait_heartbeat

    addrs = [f"127.0.0.1:{free_port()}" for _ in range(3)]
    procs = [spawn_client(a, tmp_path, "--agg", "collective", "--model", "mlp", "--data", "synthetic-mnist",
                          "--n-train", "512", "--n-test", "256", "--backend", "gloo", "--lr", "0.05",
                          "--robust", "trimmed", "--metrics", str(tmp_path / f"m{i}.jsonl"),
                          log_path=tmp_path / f"client{i}.log") for i, a in enumerate(addrs)]
    try:
        for a in addrs:
            wait_heartbeat(a, timeout=120)
        coord = Coordinator(CoordinatorConfig(clients=addrs, rounds=2, agg="collective", root=str(tmp_path / "srv"),
                                              train_timeout_s=120, rpc_timeout_s=10, heartbeat_s=0.2))
        coord.run()
        coord.close()
        assert coord.round == 2
    finally:
        for p in procs:
            stop_proc(p)
    recs = [[r for r in read_jsonl(tmp_path / f"m{i}.jsonl") if "robust_cut" in r] for i in range(3)]
    assert all(len(r) == 2 for r in recs), [(tmp_path / f"client{i}.log").read_text()[-2000:] for i in range(3)]
    for rnd in range(2):
        cut = recs[0][rnd]["robust_cut"]
        assert len(cut) == 3 and sum(cut) > 0 and sum(cut) % 2 == 0
        assert all(r[rnd]["robust_cut"] == cut and r[rnd]["robust_trim"] == 1 and r[rnd]["robust_kind"] == "trimmed"
                   for r in recs)
