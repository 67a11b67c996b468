"""Differentially private FedAvg (fedmi.parallel.dp) on the CPU path: the generator's known answers, the Gaussian
twin's moments, the clip, the accounting, replication across two gloo ranks, rollback, the config check and the CLI
guards.  Bounds and inputs: tests/dp_check.py."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fedmi.parallel.dp import (DpConfig, DpGuard, derive_key, draw_words, epsilon, gaussian, make_dp, philox4x32,
                               reference_privatize, sigma32)
from fedmi.parallel.fedavg import FedAvg
from tests.dp_check import (CLIP_SLACK, GAUSS_ABS, GAUSS_MAX, PHILOX_KAT, SHAPES, check_clip, check_stats, draw_inputs,
                            mean_bound, update_norm, var_bound)
from tests.helpers import free_port, small_trainer

KEY = 0x0123456789ABCDEF
N_NOISE = 1 << 18


class _Stub:
    """Minimal LocalTrainer surface used by FedAvg / compressors / DpGuard."""

    def __init__(self, rank: int = 0, n: int = 1000, k: int = 800):
        g = torch.Generator().manual_seed(100 + rank)
        self.flat = torch.randn(n, generator=g)
        self.ints = [torch.tensor([10 + 3 * rank], dtype=torch.int64)]
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


# ---- 1. the generator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", PHILOX_KAT)
def test_philox_known_answers(ctr, key, want):
    got = philox4x32(np.array(ctr, dtype=np.uint64), key)
    assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]


def test_draw_words_counter_layout():
    """Block b of (key, draw) is Philox at counter (b lo, b hi, draw lo, draw hi) under key (lo, hi)."""
    draw = (7 << 32) | 5
    w = draw_words(KEY, draw, 4 * 3 + 1)
    assert w.shape == (4, 4)
    for b in range(4):
        one = philox4x32(np.array([b, 0, 5, 7], dtype=np.uint64), (KEY & 0xFFFFFFFF, KEY >> 32))
        assert np.array_equal(w[b], one)


@pytest.fixture(scope="module")
def draws():
    return gaussian(KEY, 0, 1 << 20)


def test_gaussian_twin_moments(draws):
    n = draws.numel()
    assert draws.dtype == torch.float64 and n == 1 << 20
    mean, var, top = float(draws.mean()), float(draws.var(unbiased=False)), float(draws.abs().max())
    print(f"gaussian twin n={n}: mean {mean:.3g} (bound {mean_bound(n):.3g}), var-1 {var - 1:.3g} "
          f"(bound {var_bound(n):.3g}), max {top:.4g}")
    assert abs(mean) <= mean_bound(n)
    assert abs(var - 1.0) <= var_bound(n)
    assert top <= GAUSS_MAX
    assert bool(torch.isfinite(draws).all())


def test_gaussian_twin_lanes_draws_keys(draws):
    # entry i is lane i & 3 of block i >> 2 whatever the length: a shorter request is a prefix
    for m in (1, 2, 3, 5, 1027):
        assert torch.equal(gaussian(KEY, 0, m), draws[:m])
    # lanes 0, 1 are the cos / sin of one pair: g0^2 + g1^2 = -2 ln u(r0)
    w = draw_words(KEY, 0, 8).astype(np.float64)
    r2 = -2.0 * np.log((np.floor(w[:, 0::2] / 512.0) + 0.5) * 2.0 ** -23)
    g = draws[:8].reshape(2, 2, 2).numpy()
    assert np.allclose((g ** 2).sum(-1), r2, rtol=1e-12)
    other_draw, other_key = gaussian(KEY, 1, 4096), gaussian(KEY ^ 1, 0, 4096)
    assert not torch.equal(other_draw, draws[:4096]) and not torch.equal(other_key, draws[:4096])
    # no entry repeats between draws or keys beyond chance (2^-23 per pair of entries)
    assert int((other_draw == draws[:4096]).sum()) <= 1 and int((other_key == draws[:4096]).sum()) <= 1
    assert derive_key(3, "a:1") != derive_key(3, "a:2") and derive_key(3, "a:1") == derive_key(3, "a:1")
    assert derive_key(None, "a:1") != derive_key(None, "a:1")      # os.urandom


# ---- 2. the step on the CPU path ---------------------------------------------------------------------------------------
def _guard(x, anchor, k, clip, noise=0.0, key=KEY):
    t = _Stub(n=x.numel(), k=k)
    t.flat = anchor.clone()
    dp = DpGuard(t, DpConfig(clip, noise), key)
    t.flat = x.clone()
    return t, dp


@pytest.mark.parametrize("n,k", SHAPES[:4])
def test_clip_shrinks_to_the_bound(n, k):
    x, anchor = draw_inputs(n)
    clip = 0.37 * update_norm(x, anchor, k) if k else 0.05
    t, dp = _guard(x, anchor, k, clip)
    dp.privatize(t, 1)
    scale = check_stats(x, anchor, k, clip, dp.stats)
    assert (scale < 1.0) == (k > 0)
    check_clip(x, anchor, t.flat, k, dp.cfg, scale)
    assert dp.draw == 1


@pytest.mark.parametrize("n,k", SHAPES[:4])
def test_unclipped_update_keeps_its_bits(n, k):
    x, anchor = draw_inputs(n, 1)
    norm = update_norm(x, anchor, k)
    for clip in (2.0 * norm + 1.0, norm if norm else 1.0):          # also ||d|| == S exactly: not clipped
        t, dp = _guard(x, anchor, k, clip)
        dp.privatize(t, 1)
        assert torch.equal(t.flat, x)
        assert float(dp.stats[2]) == 1.0


def test_noise_is_the_twins_draw():
    """x = anchor = 0, sigma = 1: the CPU path's fp32 output is g, within GAUSS_ABS of the fp64 twin; the entries at
    and past k are never written; the next call uses the next draw."""
    n, k = 1500, 1001
    t, dp = _guard(torch.zeros(n), torch.zeros(n), k, 1.0, 1.0)
    t.flat[k:] = -12345.0
    dp.privatize(t, 1)
    assert sigma32(1.0, 1.0, 1) == 1.0
    err = (t.flat[:k].double() - gaussian(KEY, 0, k)).abs().max()
    assert float(err) <= GAUSS_ABS
    assert bool((t.flat[k:] == -12345.0).all())
    first = t.flat.clone()
    t.flat[:k] = 0.0
    dp.privatize(t, 1)
    assert dp.draw == 2 and not torch.equal(t.flat, first)
    assert float((t.flat[:k].double() - gaussian(KEY, 1, k)).abs().max()) <= GAUSS_ABS


def test_twin_is_the_formula_entry_by_entry():
    n, k = 12, 9
    x, anchor = draw_inputs(n, 2)
    cfg = DpConfig(0.01, 0.5)
    out, sumsq, norm, scale = reference_privatize(x, anchor, k, cfg, 4, KEY, 3)
    d = [float(np.float32(float(x[i]) - float(anchor[i]))) for i in range(k)]
    assert sumsq == pytest.approx(math.fsum(v * v for v in d), rel=1e-15)
    assert norm == math.sqrt(sumsq) and norm > cfg.clip
    assert scale == float(np.float32(cfg.clip / norm))
    sigma = float(np.float32(0.5 * 0.01 / 2.0))
    g = gaussian(KEY, 3, k)
    for i in range(n):
        want = scale * d[i] + float(anchor[i]) + sigma * float(g[i]) if i < k else float(x[i])
        assert float(out[i]) == pytest.approx(want, rel=1e-14, abs=1e-300)


def test_config_and_factory():
    assert DpConfig(1.0).kind == "clip" and DpConfig(1.0, 0.5).kind == "gaussian"
    assert DpConfig(2.0, 0.5).as_vector().tolist() == [1.0, 2.0, 0.5]
    for bad in ((0.0, 0.0), (-1.0, 0.0), (1.0, -0.1), (float("inf"), 0.0)):
        with pytest.raises(ValueError):
            DpConfig(*bad)
    t = _Stub()
    assert make_dp(0.0, t) is None
    dp = make_dp(1.5, t, 0.3, seed=7, who="h:1")
    assert torch.equal(dp.anchor, t.flat[:t.k]) and dp.state_tensors() == [] and dp.draw == 0
    assert dp.key == derive_key(7, "h:1") != make_dp(1.5, t, 0.3, seed=7, who="h:2").key
    assert FedAvg(dp=dp).label() == "none (single client)+gaussian"
    assert FedAvg().dp is None and FedAvg().label() == "none (single client)"


# ---- 3. accounting ------------------------------------------------------------------------------------------------------------
def test_epsilon_closed_form():
    for z, T, delta in ((1.0, 1, 1e-5), (0.3, 20, 1e-5), (4.0, 500, 1e-6)):
        want = T / (2 * z * z) + math.sqrt(2 * T * math.log(1 / delta)) / z
        assert epsilon(z, T, delta) == pytest.approx(want, rel=1e-15)
        # it is the RDP conversion alpha T / (2 z^2) + ln(1/delta) / (alpha - 1) at its best order: no alpha does better
        best = 1 + z * math.sqrt(2 * math.log(1 / delta) / T)
        conv = lambda alpha: alpha * T / (2 * z * z) + math.log(1 / delta) / (alpha - 1)   # noqa: E731
        assert conv(best) == pytest.approx(want, rel=1e-12)
        for alpha in (1.01, 1.5, 2.0, 0.9 * best + 0.1, 1.1 * best, 16.0, 64.0):
            assert conv(alpha) >= want * (1 - 1e-12)
    assert epsilon(0.5, 10) > epsilon(1.0, 10) > epsilon(2.0, 10)
    assert epsilon(1.0, 5) < epsilon(1.0, 10) < epsilon(1.0, 20)
    assert epsilon(1.0, 0) == 0.0 and epsilon(0.0, 3) == math.inf
    assert epsilon(1.0, 10, 1e-5) > epsilon(1.0, 10, 1e-3)


# ---- 4. FedAvg at world 1, rollback -----------------------------------------------------------------------------------------
def test_average_world1_clips_then_reanchors():
    t = _Stub()
    anchor = t.flat.clone()
    dp = make_dp(0.05, t)
    fa = FedAvg(dp=dp)
    t.flat[:] = anchor + 1e-2 * torch.randn(1000, generator=torch.Generator().manual_seed(5))
    tail = t.flat[t.k:].clone()
    fa.average(t)
    assert update_norm(t.flat, anchor, t.k) <= 0.05 * CLIP_SLACK
    assert torch.equal(t.flat[t.k:], tail)                      # float buffers: untouched
    assert torch.equal(dp.anchor, t.flat[:t.k]) and t.packs == 1 and dp.draw == 1
    rec = dp.round_stats()
    assert rec["dp_rounds"] == 1 and rec["dp_epsilon"] is None and rec["dp_scale"] < 1.0 < rec["dp_norm"] / 0.05


def test_rollback_restores_the_anchor_not_the_draw():
    t = _Stub(n=4096, k=4096)
    dp = make_dp(0.05, t, 1.0, seed=1)
    fa = FedAvg(dp=dp)
    start = t.flat.clone()
    trained = start + 1e-2 * torch.randn(4096, generator=torch.Generator().manual_seed(6))
    fa.snapshot_opts()
    t.flat.copy_(trained)
    fa.average(t)
    first = t.flat.clone()
    assert not torch.equal(dp.anchor, start) and dp.draw == 1
    # the round is void: the model and the anchor go back, the draw counter does not
    t.flat.copy_(start)
    fa.rollback_opts()
    assert torch.equal(dp.anchor, start) and dp.draw == 1
    t.flat.copy_(trained)                                       # the re-run round trains to the same model ...
    fa.average(t)
    assert dp.draw == 2 and not torch.equal(t.flat, first)      # ... and publishes it under fresh noise
    want, _, _, _ = reference_privatize(trained, start, 4096, dp.cfg, 1, dp.key, 1)
    assert float((t.flat.double() - want).abs().max()) <= 0.05 * GAUSS_ABS + 1e-6
    with pytest.raises(RuntimeError):
        make_dp(1.0, t).rollback()


def test_agent_restore_round_start_rolls_the_anchor_back(tmp_path):
    from fedmi.control.client_agent import ClientAgent

    tr = small_trainer("mlp", n_train=64, n_test=32)
    dp = make_dp(0.01, tr, 0.5, seed=2)
    ag = ClientAgent(tr, "127.0.0.1:1", root=tmp_path, agg="collective", fedavg=FedAvg(dp=dp), verbose=False)
    try:
        model = tr.float_state().clone()
        ag._snapshot_round_start()
        tr.float_state().add_(0.5)                              # a local epoch, then a half-applied aggregation
        ag.fedavg.average(tr)
        assert not torch.equal(dp.anchor, model[:dp.k]) and dp.draw == 1
        ag._restore_round_start()
        assert torch.equal(tr.float_state(), model) and torch.equal(dp.anchor, model[:dp.k]) and dp.draw == 1
    finally:
        ag.close()


# ---- 5. two gloo ranks ---------------------------------------------------------------------------------------------------------
def _delta(rank: int, n: int) -> torch.Tensor:
    return torch.linspace(-1, 1, n) * (rank + 1) * 1e-2


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fedmi.parallel.compress import Int8Compressor

    out = {}
    common = _Stub(0).flat.clone()
    n = common.numel()
    # clip only, S well below both updates' norms
    t = _Stub(rank)
    t.flat.copy_(common)
    dp = make_dp(0.05, t)
    t.flat.add_(_delta(rank, n))
    FedAvg(dp=dp).average(t)
    out.update(clip_x=t.flat.clone(), clip_anchor=dp.anchor.clone(), clip_scale=float(dp.stats[2]))
    # noise on a zero update: what arrives is the mean of the two shares
    t = _Stub(rank, n=N_NOISE, k=N_NOISE)
    t.flat.zero_()
    dp = make_dp(0.5, t, 2.0, seed=11, who=f"rank{rank}")
    FedAvg(dp=dp).average(t)
    out.update(noise_x=t.flat.clone(), noise_key=dp.key)
    # -c Y: int8 + error feedback on the privatised update; with S out of reach the DP step changes nothing
    for tag, clip in (("off", 0.0), ("far", 1e6), ("on", 0.05)):
        t = _Stub(rank)
        t.flat.copy_(common)
        comp, dp = Int8Compressor(t), make_dp(clip, t)
        t.flat.add_(_delta(rank, n))
        FedAvg(compressor=comp, dp=dp).average(t)
        out.update({f"c_{tag}_x": t.flat.clone(), f"c_{tag}_ref": comp.global_ref.clone(),
                    f"c_{tag}_res": comp.residual.clone()})
    # a client with another --dp-noise must not join quietly
    t = _Stub(rank)
    dp = make_dp(1.0, t, 1.0 if rank == 0 else 0.5, seed=1)
    try:
        FedAvg(dp=dp).resync(t, 0)
        out["mismatch"] = ""
    except RuntimeError as e:
        out["mismatch"] = str(e)
    out["resync_anchor_ok"] = bool(torch.equal(dp.anchor, t.flat[:t.k])) if rank == 0 else True
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
def test_gloo_clipped_mean_is_replicated_and_bounded(two_ranks):
    r0, r1 = two_ranks[0], two_ranks[1]
    common = _Stub(0).flat
    k = _Stub(0).k
    assert torch.equal(r0["clip_x"], r1["clip_x"]) and torch.equal(r0["clip_anchor"], r1["clip_anchor"])
    assert r0["clip_scale"] < 1.0 and r1["clip_scale"] < r0["clip_scale"]       # rank 1's update is twice as long
    assert update_norm(r0["clip_x"], common, k) <= 0.05 * CLIP_SLACK
    assert torch.equal(r0["clip_anchor"], r0["clip_x"][:k])
    # the float buffers past k are the plain mean of the raw states
    n = common.numel()
    raw = ((common + _delta(0, n)) + (common + _delta(1, n))) / 2
    assert torch.equal(r0["clip_x"][k:], raw[k:])


@pytest.mark.slow
def test_gloo_noise_shares_add_up(two_ranks):
    r0, r1 = two_ranks[0], two_ranks[1]
    assert torch.equal(r0["noise_x"], r1["noise_x"]) and r0["noise_key"] != r1["noise_key"]
    x = r0["noise_x"].double()
    n, z, S, N = x.numel(), 2.0, 0.5, 2
    want = z * z * S * S / (N * N)
    var = float((x ** 2).mean())
    print(f"mean of {N} noise shares, n={n}: var {var:.6g}, want {want:.6g}, rel {var / want - 1:.3g} "
          f"(bound {var_bound(n):.3g})")
    assert abs(var / want - 1.0) <= var_bound(n)
    assert abs(float(x.mean())) <= mean_bound(n) * math.sqrt(want)
    # and it is the two clients' own draws
    s = sigma32(S, z, N)
    g = [gaussian(derive_key(11, f"rank{r}"), 0, n) for r in range(2)]
    assert float((x - s * (g[0] + g[1]) / 2).abs().max()) <= 2 * s * GAUSS_ABS


@pytest.mark.slow
def test_gloo_int8_keeps_its_residual(two_ranks):
    for r in (0, 1):
        d = two_ranks[r]
        for key in ("x", "ref", "res"):
            assert torch.equal(d[f"c_far_{key}"], d[f"c_off_{key}"]), key     # no clip, no noise: every path as before
        assert d["c_on_res"].abs().sum() > 0 and torch.equal(d["c_on_ref"], d["c_on_x"])
        assert not torch.equal(d["c_on_x"], d["c_off_x"])
    assert torch.equal(two_ranks[0]["c_on_x"], two_ranks[1]["c_on_x"])


@pytest.mark.slow
def test_gloo_resync_rejects_other_settings(two_ranks):
    assert two_ranks[0]["mismatch"] == "" and two_ranks[0]["resync_anchor_ok"]
    msg = two_ranks[1]["mismatch"]
    assert "'noise'" in msg and "0.5" in msg and "rank 0" in msg and "--dp-noise" in msg


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,word", [
    (["--dp-clip", "1", "--agg", "grpc"], "--agg collective"),
    (["--dp-clip", "1", "--client-opt", "scaffold"], "scaffold"),
    (["--dp-clip", "-1"], ">= 0"),
    (["--dp-clip", "1", "--dp-noise", "-0.5"], ">= 0"),
    (["--dp-noise", "1"], "--dp-noise needs --dp-clip"),
    (["--dp-clip", "1", "--dp-delta", "2"], "--dp-delta"),
])
def test_cli_guards(capsys, argv, word):
    from fedmi.cli import client

    with pytest.raises(SystemExit) as e:
        client.main(argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_cli_flags_and_sim_guards(capsys):
    import importlib.util
    from pathlib import Path

    from fedmi.cli import client

    a = client.build_parser().parse_args([])
    assert (a.dp_clip, a.dp_noise, a.dp_delta, a.dp_seed) == (0.0, 0.0, 1e-5, None)
    a = client.build_parser().parse_args(["--dp-clip", "0.5", "--dp-noise", "1.1", "--dp-seed", "3",
                                          "--client-opt", "fedprox", "--server-opt", "fedavgm", "-c", "Y"])
    assert (a.dp_clip, a.dp_noise, a.dp_seed) == (0.5, 1.1, 3)
    from fedmi.parallel.dp import check_dp_flags

    check_dp_flags(a, pytest.fail)                    # fedprox, a server optimizer and -c Y compose
    assert "voids" in client.build_parser().format_help().lower()
    spec = importlib.util.spec_from_file_location("fedavg_sim", Path(__file__).resolve().parent.parent / "tools" /
                                                  "fedavg_sim.py")
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    for argv, word in ((["--dp-noise", "1"], "--dp-noise needs --dp-clip"),
                       (["--dp-clip", "1", "--client-opt", "scaffold"], "scaffold")):
        with pytest.raises(SystemExit) as e:
            sim.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
