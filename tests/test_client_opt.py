"""Client-side drift correction (fedmi.parallel.client_opt) on the CPU path: the torch twins against the
references, SCAFFOLD's fixed point on a heterogeneous least-squares federation, FedProx's proximal pull,
replication across two gloo ranks, resync, rollback, the engine hook and the CLI guards."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmi.parallel.client_opt import (KINDS, ClientOpt, ClientOptConfig, make_client_opt, reference_begin,
                                       reference_drift, reference_finish)
from fedmi.parallel.fedavg import FedAvg
from fedmi.parallel.server_opt import make_server_opt
from tests.client_opt_check import (check_begin, check_fedprox, check_finish, check_scaffold_drift, draw_inputs)
from tests.helpers import free_port, small_trainer

D, K_LOCAL, ROUNDS, LR, MOMENTUM = 8, 5, 200, 0.05, 0.9


class _Stub:
    """Minimal LocalTrainer surface used by FedAvg / ClientOpt: a flat state with float buffers past n_opt and a
    fake local epoch whose raw gradients depend on (rank, round, step) only."""

    def __init__(self, rank: int = 0, n: int = 1000, n_opt: int = 800, steps: int = 3):
        g = torch.Generator().manual_seed(100 + rank)
        self.rank, self.steps, self.epochs = rank, steps, 0
        self.flat = torch.randn(n, generator=g)
        self.n_opt = n_opt
        self.grad = torch.zeros(n_opt)
        self.raw = []                       # every raw gradient of the current epoch
        self.co = None

    def float_state(self):
        return self.flat

    def n_params(self):
        return self.n_opt

    def int_state(self):
        return []

    def after_aggregate(self):
        pass

    def set_client_opt(self, co):
        self.co = co

    def train_epoch(self):
        self.raw = []
        for s in range(self.steps):
            g = torch.Generator().manual_seed(7919 * self.rank + 101 * self.epochs + s)
            self.grad.copy_(1e-2 * torch.randn(self.n_opt, generator=g) + 1e-2 * (self.rank + 1))
            self.raw.append(self.grad.clone())
            if self.co is not None:
                self.co.apply(self.grad, self.flat[:self.n_opt])
            self.flat[:self.n_opt].sub_(self.grad, alpha=0.1)
        if self.co is not None:
            self.co.count(self.steps)
        self.epochs += 1


# ---- the least-squares federation ------------------------------------------------------------------------------------
def lsq_problem(seed: int):
    """Two clients with f_i(w) = ||A_i w - b_i||^2 / (2 m), d = 8, m = 32: different column scalings (Hessians)
    and different minimisers, so the mean of K-step local end points is not the joint optimum.  Returns
    (A, b, joint optimum in fp64)."""
    g = torch.Generator().manual_seed(seed)
    m = 32
    scale = torch.linspace(0.6, 1.6, D)
    A = [torch.randn(m, D, generator=g) * s for s in (scale, scale.flip(0))]
    w = [torch.randn(D, generator=g) + o for o in (1.0, -1.0)]
    b = [A[i] @ w[i] for i in range(2)]
    H = sum(a.double().T @ a.double() for a in A)
    w_star = torch.linalg.solve(H, sum(a.double().T @ v.double() for a, v in zip(A, b)))
    return A, b, w_star


def rel_err(w: torch.Tensor, w_star: torch.Tensor) -> float:
    return float((w.double() - w_star).norm() / w_star.norm())


class _LSQ:
    """fp32 flat-state trainer on one client's least-squares objective: K full-batch momentum-SGD steps per epoch
    (torch.optim.SGD's update, momentum kept across rounds), with the client-optimizer hook where the engines
    have it -- between the gradient and the update."""

    def __init__(self, A, b, lr=LR, momentum=MOMENTUM, K=K_LOCAL):
        self.A, self.b, self.lr, self.m, self.K = A, b, lr, momentum, K
        self.flat = torch.zeros(A.shape[1])
        self.grad = torch.zeros_like(self.flat)
        self.mom = torch.zeros_like(self.flat)
        self.co = None

    def float_state(self):
        return self.flat

    def n_params(self):
        return self.flat.numel()

    def int_state(self):
        return []

    def after_aggregate(self):
        pass

    def set_client_opt(self, co):
        self.co = co

    def train_epoch(self):
        for _ in range(self.K):
            self.grad.copy_(self.A.T @ (self.A @ self.flat - self.b) / self.A.shape[0])
            if self.co is not None:
                self.co.apply(self.grad, self.flat)
            self.mom.mul_(self.m).add_(self.grad)
            self.flat.sub_(self.mom, alpha=self.lr)
        if self.co is not None:
            self.co.count(self.K)


def _federate(rank: int, seed: int, kind: str, mu: float = 0.01, rounds: int = ROUNDS) -> torch.Tensor:
    """This rank's client of the federation through FedAvg.average(); returns the final global model."""
    A, b, _ = lsq_problem(seed)
    t = _LSQ(A[rank], b[rank])
    fa = FedAvg(client_opt=make_client_opt(kind, t, mu))
    for _ in range(rounds):
        t.train_epoch()
        fa.average(t)
    return t.flat.clone()


# ---- 1. the twins against the references ---------------------------------------------------------------------------------
def _opt(kind: str, n: int, mu: float = 0.01):
    t = _Stub(n=n + 7, n_opt=n)
    return t, ClientOpt(t, ClientOptConfig(kind, mu))


@pytest.mark.parametrize("n", [3, 1027, 4099])
def test_scaffold_twins_are_the_fp32_expressions(n):
    x = draw_inputs(n, 0)
    t, co = _opt("scaffold", n)
    assert co.anchor is None and all(not s.any() for s in (co.c, co.ci, co.corr, co.acc, co.delta)) and co.K == 0
    co.corr.copy_(x["corr"])
    co.acc.copy_(x["acc"])
    co.ci.copy_(x["ci"])
    co.c.copy_(x["c"])
    g = x["g"].clone()
    flat0 = t.flat.clone()
    co.apply(g, t.flat[:n])
    check_scaffold_drift(x["g"], x["corr"], x["acc"], g, co.acc)
    assert torch.equal(t.flat, flat0)                          # scaffold never touches the parameters
    co.count(3)
    acc = co.acc.clone()
    co.finish_round()
    check_finish(acc, x["ci"], 3, co.ci, co.delta)
    ci = co.ci.clone()
    co.begin_round(t, x["dmean"])
    check_begin(x["c"], x["dmean"], ci, co.c, co.corr, co.acc)
    assert co.K == 0


@pytest.mark.parametrize("n", [3, 1027, 4099])
def test_fedprox_twin_matches_fp64_reference(n):
    x = draw_inputs(n, 1)
    for mu in (0.01, 1.0, 0.3):
        t, co = _opt("fedprox", n, mu)
        assert co.c is None and co.acc is None and torch.equal(co.anchor, t.flat[:n])
        t.flat[:n].copy_(x["p"])
        co.anchor.copy_(x["anchor"])
        g = x["g"].clone()
        co.apply(g, t.flat[:n])
        check_fedprox(mu, x["g"], x["p"], x["anchor"], g)
        assert not torch.equal(g, x["g"])
        assert torch.equal(co.anchor, x["anchor"]) and torch.equal(t.flat[:n], x["p"])
        co.finish_round()                                      # nothing to finish, K irrelevant
        co.begin_round(t)
        assert torch.equal(co.anchor, t.flat[:n])


def test_fma32_is_one_rounding_of_the_exact_value():
    """fma32 (the CPU twin of the kernel's __fmaf_rn) against exact rational arithmetic, and on a case where
    rounding through fp64 first goes the wrong way."""
    import struct
    from fractions import Fraction

    from fedmi.parallel.client_opt import fma32

    def bits(v: float) -> int:
        return struct.unpack("I", struct.pack("f", v))[0]

    def rn32(q: Fraction) -> float:
        """Nearest fp32 to the rational q, ties to even: the better of float(q)'s fp32 rounding and its neighbours."""
        best = struct.unpack("f", struct.pack("f", float(q)))[0]
        for side in (float("inf"), float("-inf")):
            cand = float(torch.nextafter(torch.tensor(best), torch.tensor(side)))
            dc, db = abs(Fraction(cand) - q), abs(Fraction(best) - q)
            if dc < db or (dc == db and bits(cand) & 1 == 0):
                best = cand
        return best

    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, generator=g)
    y = 1e-2 * torch.randn(300, generator=g)
    y[:4] = torch.tensor([-0.0, 0.0, 3.0, -x[3] * 0.5])
    for a in (0.1, 0.5, 1.0):
        af = Fraction(float(torch.tensor(a, dtype=torch.float32)))
        got = fma32(a, x, y)
        for i in range(x.numel()):
            assert float(got[i]) == rn32(af * Fraction(float(x[i])) + Fraction(float(y[i]))), (a, i)
    # (2^-12 + 2^-32) * (2^-12 - 2^-32) = 2^-24 - 2^-64: added to 1 + 2^-23 the exact sum sits 2^-64 BELOW the fp32
    # tie, so it rounds down to 1 + 2^-23; fp64 rounds the sum onto the tie first, which then goes to even (up)
    a, xv, yv = 2.0 ** -12 + 2.0 ** -32, torch.tensor([2.0 ** -12 - 2.0 ** -32]), torch.tensor([1.0 + 2.0 ** -23])
    assert float(torch.tensor(a, dtype=torch.float32)) == a
    assert float((a * xv.double() + yv.double()).float()) == 1.0 + 2.0 ** -22
    assert float(fma32(a, xv, yv)) == 1.0 + 2.0 ** -23
    assert float(fma32(a, -xv, -yv)) == -(1.0 + 2.0 ** -23)


def test_references_are_the_formulas_entry_by_entry():
    n = 9
    x = draw_inputs(n, 2)
    mu = 0.25                                                  # exact in fp32
    g, _ = reference_drift(ClientOptConfig("fedprox", mu), x["g"], x["p"], x["anchor"])
    gs, acc = reference_drift(ClientOptConfig("scaffold"), x["g"], corr=x["corr"], acc=x["acc"])
    ci, delta = reference_finish(x["acc"], x["ci"], 5)
    c, corr, zero = reference_begin(x["c"], x["dmean"], x["ci"])
    for i in range(n):
        v = {k: float(t[i]) for k, t in x.items()}
        d = float(torch.tensor(v["p"]) - torch.tensor(v["anchor"]))          # fp32 subtraction
        assert float(g[i]) == mu * d + v["g"]
        assert float(gs[i]) == v["g"] + v["corr"] and float(acc[i]) == v["acc"] + v["g"]
        assert float(ci[i]) == v["acc"] / 5 and float(delta[i]) == v["acc"] / 5 - v["ci"]
        assert float(c[i]) == v["c"] + v["dmean"] and float(corr[i]) == v["c"] + v["dmean"] - v["ci"]
    assert not zero.any()


def test_config_and_factory():
    assert ClientOptConfig("fedprox").mu == 0.01
    assert ClientOptConfig("scaffold").as_vector().tolist() == [1.0, 0.01]
    for bad in (lambda: ClientOptConfig("fedsgd"), lambda: ClientOptConfig("fedprox", -0.1),
                lambda: ClientOptConfig("fedprox", float("nan"))):
        with pytest.raises(ValueError):
            bad()
    t = _Stub()
    assert make_client_opt("none", t) is None and t.co is None
    co = make_client_opt("scaffold", t)
    assert t.co is co and co.n == t.n_opt
    assert [id(s) for s in co.state_tensors()] == [id(co.c)]
    assert make_client_opt("fedprox", t).state_tensors() == []
    assert FedAvg().client_opt is None
    assert FedAvg(client_opt=co).label() == "none (single client)+scaffold"
    with pytest.raises(ValueError):
        co.apply(torch.zeros(5), torch.zeros(5))


# ---- 2. what the correction does ---------------------------------------------------------------------------------------
def test_fedprox_mu0_is_the_plain_trajectory_and_mu1_pulls_back():
    A, b, _ = lsq_problem(0)
    ends = {}
    for mu in (None, 0.0, 1.0):
        t = _LSQ(A[0], b[0])
        fa = FedAvg(client_opt=None if mu is None else make_client_opt("fedprox", t, mu))
        for _ in range(3):
            t.train_epoch()
            fa.average(t)                                      # world 1: re-anchors on the client's own model
        anchor = t.flat.clone()
        t.train_epoch()
        ends[mu] = (t.flat.clone(), t.mom.clone(), float((t.flat - anchor).norm()))
        if mu is not None:
            assert torch.equal(fa.client_opt.anchor, anchor)
    assert torch.equal(ends[0.0][0], ends[None][0]) and torch.equal(ends[0.0][1], ends[None][1])
    assert 0 < ends[1.0][2] < ends[0.0][2]


def test_scaffold_world1_round():
    """At world 1 the client's own delta is the mean: c == c_i and the correction vanishes."""
    t = _Stub(steps=4)
    fa = FedAvg(client_opt=make_client_opt("scaffold", t))
    co = fa.client_opt
    for _ in range(2):
        t.train_epoch()
        raw = t.raw
        fa.average(t)
        s = torch.zeros_like(raw[0])
        for g in raw:
            s = s + g
        assert torch.equal(co.ci, s / torch.full_like(s, 4.0))      # the in-order fp32 sum of the RAW gradients / K
        assert co.K == 0 and not co.acc.any()
    assert float((co.c - co.ci).abs().max()) <= 2 ** -22 * float(co.ci.abs().max())
    assert torch.equal(co.corr, co.c - co.ci)


def test_finish_round_without_a_step_raises():
    t = _Stub()
    co = make_client_opt("scaffold", t)
    with pytest.raises(ValueError):
        co.finish_round()
    with pytest.raises(ValueError):
        FedAvg(client_opt=co).average(t)
    with pytest.raises(ValueError):
        co.begin_round(t)                                      # no mean of the deltas


# ---- 3. two gloo ranks -------------------------------------------------------------------------------------------------
def _both(rank: int, start=None, tau: float = 1e-3, mu: float = 0.01):
    """A stub trainer with ``rank``'s gradients (and ``_Stub(start)``'s model) and one FedAvg with fedadam and
    scaffold attached."""
    t = _Stub(rank)
    if start is not None:
        t.flat.copy_(_Stub(start).flat)
    return t, FedAvg(server_opt=make_server_opt("fedadam", t, tau=tau), client_opt=make_client_opt("scaffold", t, mu))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    out = {}
    # fixed point: plain FedAvg against scaffold, seeds 0-2
    for seed in range(3):
        out[f"plain_{seed}"] = _federate(rank, seed, "none")
        out[f"scaffold_{seed}"] = _federate(rank, seed, "scaffold")
    # replication: c after 3 rounds, and what it is the sum of
    t = _Stub(rank)
    t.flat.copy_(_Stub(0).flat)
    fa = FedAvg(client_opt=make_client_opt("scaffold", t))
    co = fa.client_opt
    for r in range(3):
        t.train_epoch()
        ci_before = co.ci.clone()
        fa.average(t)
        out[f"delta_{r}"] = co.ci - ci_before                  # this rank's delta, as finish_round() formed it
        out[f"c_{r}"] = co.c.clone()
    out.update(rep_c=co.c.clone(), rep_ci=co.ci.clone(), rep_corr=co.corr.clone(), rep_x=t.flat.clone())
    # resync: rank 0 holds a trained c, rank 1 is a fresh client with another model
    if rank == 0:
        t2, fa2 = t, fa
    else:
        t2 = _Stub(5)
        fa2 = FedAvg(client_opt=make_client_opt("scaffold", t2))
        fa2.client_opt.acc.fill_(1.0)                          # gradients summed on the model about to be replaced
        fa2.client_opt.K = 2
    fa2.resync(t2, 0)
    c2 = fa2.client_opt
    out.update(rs_x=t2.flat.clone(), rs_c=c2.c.clone(), rs_ci=c2.ci.clone(), rs_corr=c2.corr.clone(),
               rs_acc=c2.acc.clone(), rs_K=c2.K)
    # a client with another --client-mu must not join quietly (fedprox hands nothing over: no broadcast is left open)
    t3 = _Stub(rank)
    fa3 = FedAvg(client_opt=make_client_opt("fedprox", t3, 0.01 if rank == 0 else 0.5))
    try:
        fa3.resync(t3, 0)
        out["mismatch"] = ""
    except RuntimeError as e:
        out["mismatch"] = str(e)
    out["rs_anchor_ok"] = bool(torch.equal(fa3.client_opt.anchor, t3.flat[:t3.n_opt])) if rank == 0 else True
    # both optimizers on one FedAvg: two rounds together, then rank 1 is replaced by a fresh client with another model
    t4, fa4 = _both(rank, start=0)
    for _ in range(2):
        t4.train_epoch()
        fa4.average(t4)
    out.update(both_m=fa4.server_opt.m.clone(), both_v=fa4.server_opt.v.clone(), both_c=fa4.client_opt.c.clone())
    if rank == 1:
        t4, fa4 = _both(5)
    fa4.resync(t4, 0)
    out.update(both_rs_m=fa4.server_opt.m.clone(), both_rs_v=fa4.server_opt.v.clone(),
               both_rs_c=fa4.client_opt.c.clone(), both_rs_x=t4.flat.clone(),
               both_rs_anchor=fa4.server_opt.anchor.clone())
    # a mismatch in either configuration.  Rank 0 cannot know and goes on to send what follows the compared
    # vector: rank 1 receives it into scratch so that rank 0's resync completes.
    for key, kw in (("both_bad_server", dict(tau=1e-3 if rank == 0 else 1e-2)),
                    ("both_bad_client", dict(mu=0.01 if rank == 0 else 0.5))):
        t5, fa5 = _both(rank, **kw)
        try:
            fa5.resync(t5, 0)
            out[key] = ""
        except RuntimeError as e:
            out[key] = str(e)
            # in FedAvg._hand_over's order: the state of the optimizer whose vector differed, then every later
            # optimizer's vector and state
            opts = fa5.opts()
            bad = next(i for i, o in enumerate(opts) if o.cfg.FLAG in str(e))
            rest = opts[bad].state_tensors()
            for o in opts[bad + 1:]:
                rest = rest + [o.cfg.as_vector()] + o.state_tensors()
            for t in rest:
                dist.broadcast(torch.empty_like(t), src=0)
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
    res = dict(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return {r: {k: (torch.from_numpy(v) if hasattr(v, "dtype") else v) for k, v in d.items()} for r, d in res.items()}


@pytest.mark.slow
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scaffold_reaches_the_joint_optimum_fedavg_does_not(two_ranks, seed):
    """d = 8, K = 5, 200 rounds, momentum 0.9 kept across rounds.  Measured with these problems (fp32): plain
    FedAvg 0.27 / 0.40 / 0.23 relative error for seeds 0 / 1 / 2, scaffold 4.5e-8 / 6.3e-8 / 3.1e-8."""
    _, _, w_star = lsq_problem(seed)
    r0, r1 = two_ranks[0], two_ranks[1]
    assert torch.equal(r0[f"plain_{seed}"], r1[f"plain_{seed}"])
    assert torch.equal(r0[f"scaffold_{seed}"], r1[f"scaffold_{seed}"])
    plain, scaf = rel_err(r0[f"plain_{seed}"], w_star), rel_err(r0[f"scaffold_{seed}"], w_star)
    print(f"seed {seed}: plain FedAvg {plain:.3g}, scaffold {scaf:.3g}")
    assert plain >= 0.03
    assert scaf <= 1e-4


@pytest.mark.slow
def test_gloo_c_is_replicated_and_the_mean_of_ci(two_ranks):
    r0, r1 = two_ranks[0], two_ranks[1]
    assert torch.equal(r0["rep_c"], r1["rep_c"]) and torch.equal(r0["rep_x"], r1["rep_x"])
    assert not torch.equal(r0["rep_ci"], r1["rep_ci"]) and r0["rep_c"].abs().sum() > 0
    for r in (r0, r1):
        assert torch.equal(r["rep_corr"], r["rep_c"] - r["rep_ci"])
    # c = sum over rounds of fl(fl(d0 + d1) / 2) with d_i = fl(new_i - ci_i): per round one rounding of each d_i
    # (halved by the mean), one of their sum (halved) and one of c's addition, each <= 2^-24 of its magnitude, so
    # |c - mean(ci)| <= 2^-24 * sum_r (|d0| + |d1| + |c_r|); 4x that is allowed
    mean_ci = (r0["rep_ci"].double() + r1["rep_ci"].double()) / 2
    mag = sum(r0[f"delta_{r}"].abs().double() + r1[f"delta_{r}"].abs().double() + r0[f"c_{r}"].abs().double()
              for r in range(3))
    err = (r0["rep_c"].double() - mean_ci).abs()
    print(f"c vs mean(ci): worst ratio to the bound {float((err / (4 * 2.0 ** -24 * mag)).max()):.3g}")
    assert bool((err <= 4 * 2.0 ** -24 * mag).all())


@pytest.mark.slow
def test_gloo_resync_hands_c_to_a_fresh_client(two_ranks):
    r0, r1 = two_ranks[0], two_ranks[1]
    assert torch.equal(r1["rs_c"], r0["rep_c"]) and torch.equal(r0["rs_c"], r0["rep_c"])
    assert not r1["rs_ci"].any() and torch.equal(r1["rs_corr"], r1["rs_c"])
    assert torch.equal(r0["rs_ci"], r0["rep_ci"]) and torch.equal(r0["rs_corr"], r0["rep_corr"])
    assert torch.equal(r1["rs_x"], r0["rs_x"])
    assert not r1["rs_acc"].any() and r1["rs_K"] == 0


@pytest.mark.slow
def test_gloo_resync_rejects_other_settings(two_ranks):
    assert two_ranks[0]["mismatch"] == "" and two_ranks[0]["rs_anchor_ok"]
    msg = two_ranks[1]["mismatch"]
    assert "'mu'" in msg and "0.5" in msg and "rank 0" in msg


@pytest.mark.slow
def test_gloo_resync_with_both_optimizers_hands_over_m_v_and_c(two_ranks):
    r0, r1 = two_ranks[0], two_ranks[1]
    for key in ("m", "v", "c"):
        trained = r0[f"both_{key}"]
        assert torch.equal(r1[f"both_{key}"], trained) and trained.max() > trained.min()    # replicated, not initial
        assert torch.equal(r1[f"both_rs_{key}"], trained) and torch.equal(r0[f"both_rs_{key}"], trained)
    assert torch.equal(r1["both_rs_x"], r0["both_rs_x"])
    for r in (r0, r1):
        assert torch.equal(r["both_rs_anchor"], r["both_rs_x"])


@pytest.mark.slow
@pytest.mark.parametrize("key,flag,name", [("both_bad_server", "--server-opt", "'tau'"),
                                           ("both_bad_client", "--client-opt", "'mu'")])
def test_gloo_resync_with_both_optimizers_names_the_flag_that_differs(two_ranks, key, flag, name):
    assert two_ranks[0][key] == ""
    msg = two_ranks[1][key]
    assert flag in msg and name in msg and "rank 0" in msg
    assert ("--client-opt" if flag == "--server-opt" else "--server-opt") not in msg


# ---- 4. rollback ---------------------------------------------------------------------------------------------------------
def test_both_optimizers_snapshot_average_rollback_bitwise():
    """snapshot_opts() -> average() -> rollback_opts() at world 1: anchor, m, v and c, ci, corr come back bit for
    bit, and the void round's gradient sum is dropped."""
    t, fa = _both(0)
    t.train_epoch()
    fa.average(t)                                              # non-trivial m, v and c / ci / corr
    rolled = [s for o in fa.opts() for s in o._rolled()]
    assert [id(o) for o in fa.opts()] == [id(fa.server_opt), id(fa.client_opt)] and len(rolled) == 6
    fa.snapshot_opts()
    before = [s.clone() for s in rolled]
    t.train_epoch()
    fa.average(t)
    assert all(not torch.equal(a, b) for a, b in zip(rolled, before))
    t.train_epoch()                                            # the void round got as far as summing gradients
    assert fa.client_opt.acc.any() and fa.client_opt.K == t.steps
    fa.rollback_opts()
    for got, want in zip(rolled, before):
        assert torch.equal(got, want)
    assert fa.client_opt.K == 0 and not fa.client_opt.acc.any()
    fa.reset_opts(t)
    assert torch.equal(fa.server_opt.anchor, t.flat)


@pytest.mark.parametrize("kind", KINDS)
def test_snapshot_train_rollback_bitwise(kind):
    t = _Stub()
    fa = FedAvg(client_opt=make_client_opt(kind, t, 0.1))
    co = fa.client_opt
    t.train_epoch()
    fa.average(t)                                              # a non-trivial c / ci / corr, anchor == model
    co.snapshot()
    before = [s.clone() for s in co._rolled()]
    t.train_epoch()
    if kind == "scaffold":
        assert co.acc.any() and co.K == t.steps
    fa.average(t)
    assert all(not torch.equal(a, b) for a, b in zip(co._rolled(), before))
    t.train_epoch()                                            # the void round got as far as summing gradients
    co.rollback()
    for got, want in zip(co._rolled(), before):
        assert torch.equal(got, want)
    assert co.K == 0 and (co.acc is None or not co.acc.any())
    with pytest.raises(RuntimeError):
        ClientOpt(t, ClientOptConfig(kind)).rollback()


def test_agent_round_start_snapshot_and_rollback(tmp_path):
    from fedmi.control.client_agent import ClientAgent

    tr = small_trainer("mlp", n_train=64, n_test=32)
    co = make_client_opt("scaffold", tr)
    ag = ClientAgent(tr, "127.0.0.1:1", root=tmp_path, agg="collective", fedavg=FedAvg(client_opt=co), verbose=False)
    try:
        tr.set_schedule([0, 32], [32, 32])
        tr.train_epoch()
        ag.fedavg.average(tr)
        ag._snapshot_round_start()
        before = [s.clone() for s in co._rolled()]
        model = tr.float_state().clone()
        tr.train_epoch()
        assert co.K == 2 and co.acc.any()
        ag.fedavg.average(tr)
        assert not torch.equal(co.ci, before[1])
        ag._restore_round_start()
        assert torch.equal(tr.float_state(), model)
        for got, want in zip(co._rolled(), before):
            assert torch.equal(got, want)
        assert co.K == 0 and not co.acc.any()
    finally:
        ag.close()


# ---- 5. the engine hook ----------------------------------------------------------------------------------------------------
def test_base_trainer_has_no_hook():
    from fedmi.engine.base import LocalTrainer

    class Bare(LocalTrainer):
        state_dict = load_state_dict = set_schedule = train_epoch = train_stats = evaluate = eval_stats = None
        device = torch.device("cpu")

        def float_state(self):
            return torch.zeros(4)

    with pytest.raises(NotImplementedError):
        Bare().set_client_opt(object())
    with pytest.raises(NotImplementedError):
        make_client_opt("fedprox", Bare())


def test_torch_trainer_cpu_applies_the_correction():
    """The CPU TorchTrainer: scaffold's first round (corr = 0) and fedprox mu = 0 leave the trajectory bit for
    bit; acc is the in-order sum of the raw gradients; mu = 1 ends closer to the anchor."""
    def run(kind, mu=0.0):
        tr = small_trainer("mlp", n_train=96, n_test=32)
        tr.set_schedule([0, 32, 64], [32, 32, 32])
        co = make_client_opt(kind, tr, mu)
        start = tr.float_state().clone()
        tr.train_epoch()
        return tr, co, float((tr.float_state() - start).norm())

    plain, _, d_plain = run("none")
    prox0, _, _ = run("fedprox", 0.0)
    scaf, co, _ = run("scaffold")
    _, _, d_prox1 = run("fedprox", 1.0)
    for tr in (prox0, scaf):
        assert torch.equal(tr.float_state(), plain.float_state())
        assert torch.equal(tr.momentum_state(), plain.momentum_state())
    assert co.K == 3
    assert 0 < d_prox1 < d_plain
    # the raw gradients, recomputed step by step on a twin without a client optimizer
    twin = small_trainer("mlp", n_train=96, n_test=32)
    acc = torch.zeros_like(co.acc)
    twin.model.train()
    for s in (0, 32, 64):
        twin.train_step(s, 32)
        acc = acc + twin.fs.grad
    assert torch.equal(co.acc, acc)


# ---- 6. CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_guards(capsys):
    from fedmi.cli import client

    with pytest.raises(SystemExit) as e:
        client.main(["--client-opt", "scaffold", "--agg", "grpc"])
    assert e.value.code == 2
    assert "--client-opt" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        client.main(["--client-opt", "fedprox", "--client-mu", "-0.5"])
    assert e.value.code == 2
    assert "--client-mu" in capsys.readouterr().err
    a = client.build_parser().parse_args([])
    assert (a.client_opt, a.client_mu) == ("none", 0.01)
    a = client.build_parser().parse_args(["--client-opt", "fedprox", "--client-mu", "0.1"])
    assert (a.client_opt, a.client_mu) == ("fedprox", 0.1)
