"""Server-side optimizers (fedmi.parallel.server_opt) on the CPU path: the step's math against its fp64
twin, composition with plain FedAvg and the -c Y compressors, replication across two gloo ranks, resync,
rollback, the parameter / buffer split, and the CLI guard."""
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmi.parallel.fedavg import FedAvg
from fedmi.parallel.server_opt import KINDS, ServerOpt, ServerOptConfig, make_server_opt, reference_step
from tests.helpers import free_port, small_trainer
from tests.server_opt_check import YOGI_MAX_SHARE, check_step, draw_inputs, next_round

N, N_OPT = 1500, 1001


class _Stub:
    """Minimal LocalTrainer surface used by FedAvg / compressors / ServerOpt."""

    def __init__(self, rank: int = 0, n: int = 1000, n_opt: int = 800):
        g = torch.Generator().manual_seed(100 + rank)
        self.flat = torch.randn(n, generator=g)
        self.ints = [torch.tensor([10 + 3 * rank], dtype=torch.int64)]
        self.n_opt = n_opt
        self.packs = 0

    def float_state(self):
        return self.flat

    def n_params(self):
        return self.n_opt

    def int_state(self):
        return self.ints

    def after_aggregate(self):
        self.packs += 1


def _state(so):
    return tuple(t.clone() for t in (so.anchor, so.m, so.v))


# ---- 1. math -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_match_fp64_twin(kind):
    x, anchor, m, v, g = draw_inputs(N, 0)
    t = _Stub(n=N, n_opt=N_OPT)
    t.flat.copy_(anchor)
    so = ServerOpt(t, ServerOptConfig(kind))
    so.m.copy_(m)
    so.v.copy_(v)
    t.flat.copy_(x)
    left_out = torch.zeros(N_OPT, dtype=torch.bool)
    for _ in range(3):
        mean = t.flat.clone()
        pre = (mean, so.anchor.clone(), so.m.clone(), so.v.clone())
        so.step(t)
        left_out |= check_step(so.cfg, pre, (t.flat, so.anchor, so.m, so.v), N_OPT)
        assert torch.equal(t.flat[N_OPT:], mean[N_OPT:])      # float buffers: bitwise the mean
        t.flat.copy_(next_round(t.flat, g))
    assert left_out.float().mean().item() <= YOGI_MAX_SHARE
    assert so.steps == 3


@pytest.mark.parametrize("kind", KINDS)
def test_twin_is_the_formula_entry_by_entry(kind):
    """reference_step (vectorised torch) against the formulas written out per entry in Python floats."""
    n, k = 12, 9
    x, anchor, m, v, _ = draw_inputs(n, 1)
    v[2] = float(x[2] - anchor[2]) ** 2          # sgn(0) = 0 is reachable
    cfg = ServerOptConfig(kind, lr=0.25, beta1=0.5, beta2=0.75, tau=0.125)     # exact in fp32
    rx, ra, rm, rv = reference_step(x, anchor, m, v, k, cfg, torch.float64)
    for i in range(n):
        xi, ai, mi, vi = (float(t[i]) for t in (x, anchor, m, v))
        if i < k:
            d = xi - ai
            if kind == "fedavgm":
                mi = cfg.beta1 * mi + d
                xi = ai + cfg.lr * mi
            else:
                mi = cfg.beta1 * mi + (1 - cfg.beta1) * d
                if kind == "fedadagrad":
                    vi = vi + d * d
                elif kind == "fedyogi":
                    s = vi - d * d
                    vi = vi - (1 - cfg.beta2) * d * d * ((s > 0) - (s < 0))
                else:
                    vi = cfg.beta2 * vi + (1 - cfg.beta2) * d * d
                xi = ai + cfg.lr * mi / (math.sqrt(vi) + cfg.tau)
        assert float(rx[i]) == pytest.approx(xi, rel=1e-14, abs=1e-300)
        assert float(ra[i]) == float(rx[i])
        assert float(rm[i]) == pytest.approx(mi, rel=1e-14, abs=1e-300)
        assert float(rv[i]) == pytest.approx(vi, rel=1e-14, abs=1e-300)


def test_config_defaults_and_initial_state():
    assert ServerOptConfig("fedavgm").lr == 1.0
    for kind in KINDS[1:]:
        assert ServerOptConfig(kind).lr == 0.01
    c = ServerOptConfig("fedadam")
    assert (c.beta1, c.beta2, c.tau) == (0.9, 0.99, 1e-3)
    with pytest.raises(ValueError):
        ServerOptConfig("fedsgd")
    t = _Stub()
    assert make_server_opt("none", t) is None
    so = make_server_opt("fedyogi", t, tau=0.5)
    assert torch.equal(so.anchor, t.flat) and not so.m.any() and torch.equal(so.v, torch.full_like(so.v, 0.25))
    assert [id(s) for s in so.state_tensors()] == [id(so.m), id(so.v)]


# ---- 2. composition with plain FedAvg --------------------------------------------------------------------------
def test_fedavgm_without_momentum_is_the_mean():
    """beta1 = 0, lr = 1: x = anchor + (mean - anchor).  Where the update does not cancel the weight
    (|mean - anchor| <= |anchor| / 2, the FedAvg regime) the difference is exact (Sterbenz) and x is within
    1 ulp of the mean; in general the error is one rounding of d plus one of the sum."""
    g = torch.Generator().manual_seed(7)
    n = 1000
    anchor = (0.5 + 1.5 * torch.rand(n, generator=g)) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    mean = anchor + 1e-2 * torch.randn(n, generator=g)
    t = _Stub(n=n, n_opt=n)
    t.flat.copy_(anchor)
    fa = FedAvg(server_opt=make_server_opt("fedavgm", t, lr=1.0, beta1=0.0))
    t.flat.copy_(mean)
    fa.average(t)
    ulp = torch.nextafter(mean.abs(), torch.full_like(mean, float("inf"))) - mean.abs()
    assert ((t.flat - mean).abs() <= ulp).all()
    assert t.packs == 1
    # any inputs (here the mean can cancel the anchor): half an ulp of d and half an ulp of the result
    x, anchor, _, _, _ = draw_inputs(n, 2)
    mean = torch.randn(n, generator=g)
    t.flat.copy_(anchor)
    so = make_server_opt("fedavgm", t, lr=1.0, beta1=0.0)
    t.flat.copy_(mean)
    so.step(t)
    eps = 2.0 ** -24
    assert ((t.flat.double() - mean.double()).abs() <= eps * ((mean - anchor).abs() + mean.abs()).double() * 1.0001).all()


def test_no_server_opt_is_todays_fedavg():
    a, b = _Stub(), _Stub()
    FedAvg().average(a)
    FedAvg(server_opt=None).average(b)
    assert torch.equal(a.flat, b.flat) and torch.equal(a.flat, _Stub().flat) and a.packs == b.packs == 1
    assert FedAvg().server_opt is None
    assert FedAvg().label() == "none (single client)"
    assert FedAvg(server_opt=make_server_opt("fedyogi", a)).label() == "none (single client)+fedyogi"


# ---- 3 / 4 / 6. two gloo ranks -----------------------------------------------------------------------------------
def _prior(so, seed: int) -> None:
    g = torch.Generator().manual_seed(seed)
    so.m.copy_(1e-2 * torch.randn(so.n, generator=g))
    so.v.copy_(1e-6 + 1e-3 * torch.rand(so.n, generator=g))


def _delta(rank: int, n: int) -> torch.Tensor:
    return torch.linspace(-1, 1, n) * (rank + 1) * 1e-2


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fedmi.parallel.compress import Int8Compressor

    out = {}
    common = _Stub(0).flat.clone()
    n = common.numel()
    # today's dense path, field left at None
    t = _Stub(rank)
    FedAvg(server_opt=None).average(t)
    out["dense_none"] = t.flat.clone()
    # 3. average(): different local models, equal prior state
    t = _Stub(rank)
    t.flat.copy_(common)
    so = make_server_opt("fedadam", t)
    _prior(so, 5)
    t.flat.add_(_delta(rank, n))
    FedAvg(server_opt=so).average(t)
    out.update(avg_x=t.flat.clone(), avg_m=so.m.clone(), avg_v=so.v.clone(), avg_anchor=so.anchor.clone(),
               avg_packs=t.packs)
    # 4. resync(): rank 1's m / v differ, its model too
    t = _Stub(rank)
    so = make_server_opt("fedyogi", t)
    _prior(so, 20 + rank)
    FedAvg(server_opt=so).resync(t, 0)
    out.update(rs_x=t.flat.clone(), rs_m=so.m.clone(), rs_v=so.v.clone(), rs_anchor=so.anchor.clone())
    # 6. int8 + error feedback, with and without fedavgm: same residual, anchor == stepped model
    for tag, kind in (("plain", "none"), ("opt", "fedavgm")):
        t = _Stub(rank)
        t.flat.copy_(common)
        comp = Int8Compressor(t)
        so = make_server_opt(kind, t, lr=0.7)
        t.flat.add_(_delta(rank, n))
        FedAvg(compressor=comp, server_opt=so).average(t)
        out.update({f"c_{tag}_x": t.flat.clone(), f"c_{tag}_ref": comp.global_ref.clone(),
                    f"c_{tag}_res": comp.residual.clone()})
    # 4b. a client with another --server-lr must not join quietly.  Rank 0 cannot know and goes on to send
    # m and v: rank 1 receives them into scratch so that rank 0's resync completes.
    t = _Stub(rank)
    so = make_server_opt("fedavgm", t, lr=1.0 if rank == 0 else 0.5)
    try:
        FedAvg(server_opt=so).resync(t, 0)
        out["mismatch"] = ""
    except RuntimeError as e:
        out["mismatch"] = str(e)
        for _ in so.state_tensors():
            dist.broadcast(torch.empty(n), src=0)
    # tensors travel by value (numpy pickles): torch's fd-sharing reducer races the worker's exit
    q.put((rank, {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()}))
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return {r: {k: (torch.from_numpy(v) if hasattr(v, "dtype") else v) for k, v in d.items()} for r, d in res.items()}


@pytest.mark.slow
def test_gloo_average_is_replicated(two_ranks):
    r0, r1 = two_ranks[0], two_ranks[1]
    common = _Stub(0).flat
    n, k = common.numel(), _Stub(0).n_opt
    mean = ((common + _delta(0, n)) + (common + _delta(1, n))) / 2
    assert torch.equal(r0["dense_none"], (_Stub(0).flat + _Stub(1).flat) / 2)
    for key in ("avg_x", "avg_m", "avg_v", "avg_anchor"):
        assert torch.equal(r0[key], r1[key]), key
    t = _Stub(0)
    so = make_server_opt("fedadam", t)
    _prior(so, 5)
    pre = (mean, common, so.m, so.v)
    check_step(so.cfg, pre, (r0["avg_x"], r0["avg_anchor"], r0["avg_m"], r0["avg_v"]), k)
    assert not torch.equal(r0["avg_x"][:k], mean[:k])        # the optimizer did move the parameters
    assert r0["avg_packs"] == r1["avg_packs"] == 1


@pytest.mark.slow
def test_gloo_resync_hands_over_state(two_ranks):
    t = _Stub(0)
    so = make_server_opt("fedyogi", t)
    _prior(so, 20)
    for r in (0, 1):
        d = two_ranks[r]
        assert torch.equal(d["rs_m"], so.m) and torch.equal(d["rs_v"], so.v)
        assert torch.equal(d["rs_x"], t.flat) and torch.equal(d["rs_anchor"], d["rs_x"])


@pytest.mark.slow
def test_gloo_resync_rejects_other_settings(two_ranks):
    assert two_ranks[0]["mismatch"] == ""
    msg = two_ranks[1]["mismatch"]
    assert "'lr'" in msg and "0.5" in msg and "rank 0" in msg


@pytest.mark.slow
def test_gloo_int8_keeps_residual_and_reanchors(two_ranks):
    for r in (0, 1):
        d = two_ranks[r]
        assert torch.equal(d["c_opt_ref"], d["c_opt_x"])
        assert torch.equal(d["c_opt_res"], d["c_plain_res"])
        assert d["c_plain_res"].abs().sum() > 0
        assert not torch.equal(d["c_opt_x"], d["c_plain_x"])      # lr = 0.7: not the plain mean
    assert torch.equal(two_ranks[0]["c_opt_x"], two_ranks[1]["c_opt_x"])


def test_reanchor_keeps_residual_reset_clears_it():
    from fedmi.parallel.compress import Int8Compressor

    t = _Stub()
    comp = Int8Compressor(t)
    comp.residual.fill_(0.25)
    x = torch.arange(t.flat.numel(), dtype=torch.float32)
    comp.reanchor(x)
    assert torch.equal(comp.global_ref, x) and bool((comp.residual == 0.25).all())
    comp.reset(t)
    assert torch.equal(comp.global_ref, t.flat) and not comp.residual.any()


# ---- 5. rollback -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fedavgm", "fedadam"])
def test_snapshot_rollback_bitwise(kind):
    t = _Stub()
    so = make_server_opt(kind, t)
    _prior(so, 3)
    so.snapshot()
    before = _state(so)
    t.flat.copy_(torch.randn(t.flat.numel()) * 1e3)            # garbage "mean"
    so.step(t)
    assert not torch.equal(so.anchor, before[0]) and not torch.equal(so.m, before[1])
    so.rollback()
    for got, want in zip(_state(so), before):
        assert torch.equal(got, want)
    with pytest.raises(RuntimeError):
        make_server_opt(kind, t).rollback()


def test_agent_restore_round_start_rolls_the_optimizer_back(tmp_path):
    from fedmi.control.client_agent import ClientAgent

    tr = small_trainer("mlp", n_train=64, n_test=32)
    so = make_server_opt("fedadam", tr)
    ag = ClientAgent(tr, "127.0.0.1:1", root=tmp_path, agg="collective", fedavg=FedAvg(server_opt=so), verbose=False)
    try:
        _prior(so, 4)
        model = tr.float_state().clone()
        ag._snapshot_round_start()
        before = _state(so)
        tr.float_state().add_(0.5)                              # a local epoch, then a half-applied aggregation
        so.step(tr)
        assert not torch.equal(so.m, before[1])
        ag._restore_round_start()
        assert torch.equal(tr.float_state(), model)
        for got, want in zip(_state(so), before):
            assert torch.equal(got, want)
        assert torch.equal(so.anchor, tr.float_state())
    finally:
        ag.close()


# ---- 7. n_params() ---------------------------------------------------------------------------------------------------
def test_n_params_splits_parameters_from_float_buffers():
    tr = small_trainer("mobilenet", n_train=64, n_test=32)
    k = tr.n_params()
    assert k == sum(p.numel() for p in tr.model.parameters())
    bufs = torch.cat([b.reshape(-1) for b in tr.model.buffers() if b.is_floating_point()])
    assert bufs.numel() > 0 and torch.equal(tr.float_state()[k:], bufs)
    assert torch.equal(tr.float_state()[:k], torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()]))
    assert small_trainer("mlp", n_train=64, n_test=32).n_params() == small_trainer(
        "mlp", n_train=64, n_test=32).float_state().numel()
    # a step with a large server lr moves the parameters and leaves the buffers the mean: running_var > 0
    so = make_server_opt("fedadam", tr, lr=10.0)
    mean = tr.float_state() - 0.05
    mean[k:] = tr.float_state()[k:] * 0.5 + 0.01
    tr.float_state().copy_(mean)
    so.step(tr)
    assert torch.equal(tr.float_state()[k:], mean[k:])
    assert not torch.equal(tr.float_state()[:k], mean[:k])
    var = torch.cat([v.reshape(-1) for n, v in tr.state_dict().items() if n.endswith("running_var")])
    assert var.numel() > 0 and bool((var > 0).all())


# ---- 8. CLI ------------------------------------------------------------------------------------------------------------
def test_cli_rejects_server_opt_with_grpc_aggregation(capsys):
    from fedmi.cli import client

    with pytest.raises(SystemExit) as e:
        client.main(["--server-opt", "fedadam", "--agg", "grpc"])
    assert e.value.code == 2
    assert "--server-opt" in capsys.readouterr().err
    a = client.build_parser().parse_args([])
    assert (a.server_opt, a.server_lr, a.server_beta1, a.server_beta2, a.server_tau) == ("none", None, 0.9, 0.99, 1e-3)
    a = client.build_parser().parse_args(["--server-opt", "fedyogi", "--server-lr", "0.1", "--server-tau", "0.01"])
    assert (a.server_opt, a.server_lr, a.server_tau) == ("fedyogi", 0.1, 0.01)
