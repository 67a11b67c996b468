"""The DP-FedAvg HIP kernels (csrc/kernels/dp.hip: dp_sumsq, dp_finish, DpApply) against their fp64 twin, and the
LeNet engine end to end with clipping and noise at world 1.  Bounds and inputs: tests/dp_check.py."""
import functools

import pytest
import torch

from fedmi import native
from fedmi.parallel.dp import DpConfig, gaussian, make_dp, reference_privatize, sigma32
from fedmi.parallel.fedavg import FedAvg
from tests.dp_check import (CLIP_SLACK, GAUSS_ABS, SHAPES, check_clip, check_stats, draw_inputs, ulp32, update_norm)

pytestmark = pytest.mark.gpu

KEY = 0xFEDCBA9876543210            # both key words and both draw words are non-zero
DRAW = (3 << 32) | 7
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def nat(gpu_device):
    return native.require()


@functools.lru_cache(maxsize=None)
def _case(n: int):
    """(x, anchor) of one length, shared by the tests and never written."""
    return draw_inputs(n)


@functools.lru_cache(maxsize=None)
def _twin_draw(key: int, draw: int, k: int) -> torch.Tensor:
    return gaussian(key, draw, k)


class _Dev:
    """The device buffers of one call: x (n entries), anchor (k), the partials and the stats row."""

    def __init__(self, nat, dev, x, anchor, k):
        self.nat, self.n, self.k = nat, x.numel(), k
        self.x = x.to(dev)
        self.anchor = anchor[:k].to(dev)
        self.partial = torch.zeros(max(1, nat.dp_partials(k)), dtype=torch.float64, device=dev)
        self.stats = torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float64, device=dev)

    def run(self, clip, z=0.0, world=1, key=KEY, draw=DRAW):
        self.nat.dp_privatize(native.stream_handle(), self.x.data_ptr(), self.anchor.data_ptr(), self.n, self.k,
                              self.partial.data_ptr(), self.stats.data_ptr(), clip, z, world, key, draw)
        torch.cuda.synchronize()
        return self.x.cpu(), self.stats.cpu()


def test_partials_follow_the_grid_rule(nat):
    assert [nat.dp_partials(k) for k in (0, 1, 3, 1027, 1028, 2048 * 1024, 2048 * 1024 + 5, 1 << 33)] == \
        [0, 1, 1, 1, 2, 2048, 2048, 2048]


@pytest.mark.parametrize("n,k", SHAPES)
def test_sumsq_scale_and_clip(nat, gpu_device, n, k):
    x0, a0 = _case(n)
    clip = 0.37 * update_norm(x0, a0, k) if k else 0.05
    d = _Dev(nat, gpu_device, x0, a0, k)
    x1, stats = d.run(clip)
    scale = check_stats(x0, a0, k, clip, stats)
    assert (scale < 1.0) == (k > 0)
    check_clip(x0, a0, x1, k, DpConfig(clip), scale)


@pytest.mark.parametrize("n,k", SHAPES)
def test_unclipped_update_keeps_its_bits(nat, gpu_device, n, k):
    x0, a0 = _case(n)
    norm = update_norm(x0, a0, k)
    d = _Dev(nat, gpu_device, x0, a0, k)
    x1, stats = d.run(2.0 * norm + 1.0)
    assert torch.equal(x1, x0) and float(stats[2]) == 1.0
    check_stats(x0, a0, k, 2.0 * norm + 1.0, stats)


@pytest.mark.parametrize("n,k", SHAPES)
def test_noise_is_the_twins_draw(nat, gpu_device, n, k):
    """x = anchor = 0 and sigma = 1: the output is g, entry by entry the fp64 twin's draw at the same counters."""
    assert sigma32(1.0, 1.0, 1) == 1.0
    x0 = torch.zeros(n)
    x0[k:] = SENTINEL
    d = _Dev(nat, gpu_device, x0, torch.zeros(n), k)
    x1, stats = d.run(1.0, 1.0)
    assert bool((x1[k:] == SENTINEL).all()), "entries at or past k were written"
    if k == 0:
        return
    assert stats[:3].tolist() == [0.0, 0.0, 1.0]
    err = (x1[:k].double() - _twin_draw(KEY, DRAW, k)).abs()
    print(f"noise k={k}: worst |g - g64| {float(err.max()):.3g} (bound {GAUSS_ABS:.3g}), "
          f"mean {float(x1[:k].mean()):.3g}, var {float(x1[:k].var()):.5g}")
    assert float(err.max()) <= GAUSS_ABS


def test_clip_and_noise_together(nat, gpu_device):
    """Both halves on a real update, four clients' share of the noise: the clipped value is within 1 ulp of the
    twin's (tests/dp_check.py), the noise fma adds half an ulp of the result and sigma * GAUSS_ABS."""
    n, k = 1500, 1001
    x0, a0 = _case(n)
    cfg = DpConfig(0.37 * update_norm(x0, a0, k), 0.7)
    d = _Dev(nat, gpu_device, x0, a0, k)
    x1, stats = d.run(cfg.clip, cfg.noise, world=4)
    scale = check_stats(x0, a0, k, cfg.clip, stats)
    ref, _, _, _ = reference_privatize(x0, a0, k, cfg, 4, KEY, DRAW, scale=scale)
    assert torch.equal(x1[k:], x0[k:])
    sigma = sigma32(cfg.clip, cfg.noise, 4)
    assert sigma == pytest.approx(0.7 * cfg.clip / 2.0, rel=1e-7)
    clipped, _, _, _ = reference_privatize(x0, a0, k, DpConfig(cfg.clip), 4, KEY, DRAW, scale=scale)
    bound = ulp32(clipped[:k].float()).double() + 0.5 * ulp32(ref[:k].float()).double() + sigma * GAUSS_ABS
    err = (x1[:k].double() - ref[:k]).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float((x1[:k].double() - clipped[:k]).abs().max()) > 10 * sigma * GAUSS_ABS     # noise was added


def test_same_key_and_draw_same_bits(nat, gpu_device):
    n = k = 2048 * 256 * 4 + 5
    x0, a0 = _case(n)
    clip = 0.37 * update_norm(x0, a0, k)
    runs = {}
    for tag, key, draw in (("a", KEY, DRAW), ("b", KEY, DRAW), ("draw", KEY, DRAW + 1), ("key", KEY ^ (1 << 40), DRAW),
                           ("draw_hi", KEY, DRAW + (1 << 32))):
        runs[tag], stats = _Dev(nat, gpu_device, x0, a0, k).run(clip, 1.0, 2, key, draw)
        if tag == "a":
            first = stats
        assert torch.equal(stats, first)               # the sum's order is fixed: the same bits on every run
    assert torch.equal(runs["a"], runs["b"])
    for tag in ("draw", "key", "draw_hi"):
        same = int((runs[tag] == runs["a"]).sum())
        assert same <= n // 1000, (tag, same)          # fresh noise everywhere (equal fp32 results happen by chance)


def test_binding_rejects_bad_arguments(nat, gpu_device):
    """Refused before any launch: k outside [0, n], a null or misaligned buffer, S <= 0, z < 0, world < 1."""
    t = torch.zeros(64, device=gpu_device)
    w = torch.zeros(8, dtype=torch.float64, device=gpu_device)
    p, q, s = t.data_ptr(), w.data_ptr(), native.stream_handle()
    good = dict(x=p, anchor=p, n=16, k=16, partial=q + 32, stats=q, clip=1.0, z=0.0, world=1, key=1, draw=0)
    for bad in (dict(k=17), dict(k=-1), dict(n=-1, k=0), dict(x=0), dict(anchor=0), dict(partial=0), dict(stats=0),
                dict(x=p + 4), dict(anchor=p + 8), dict(stats=q + 4), dict(clip=0.0), dict(clip=-1.0),
                dict(clip=float("nan")), dict(z=-0.5), dict(z=float("inf")), dict(world=0), dict(stages=0),
                dict(stages=8)):
        with pytest.raises(ValueError):
            nat.dp_privatize(s, **{**good, **bad})
    with pytest.raises(ValueError):
        nat.dp_partials(-1)
    nat.dp_privatize(s, **{**good, "k": 0, "x": 0, "anchor": 0})     # k = 0: nothing to do
    nat.dp_privatize(s, **good)
    torch.cuda.synchronize()
    assert not t.any() and w[:3].tolist() == [0.0, 0.0, 1.0]


# ---- the LeNet engine end to end ------------------------------------------------------------------------------------------
CLIP = 0.02


def _lenet_rounds(gpu_device, noise: float, seed=None):
    from fedmi.engine import build_trainer
    from fedmi.engine.base import TrainerConfig
    from fedmi.engine.data import make_dataset, strided_schedule

    data = make_dataset("synthetic-cifar10", device=gpu_device, n_train=384, n_test=128, seed=0)
    tr = build_trainer("lenet", data, gpu_device, TrainerConfig(seed=1))
    assert tr.n_params() == tr.float_state().numel()
    dp = make_dp(CLIP, tr, noise, seed=seed, who="test")
    fa = FedAvg(dp=dp)
    tr.set_schedule(*strided_schedule(384, 128, 0, 1))
    moved = []
    for _ in range(2):
        tr.train_epoch()
        torch.cuda.synchronize()
        start, trained = dp.anchor.cpu(), tr.float_state().cpu()
        fa.average(tr)
        torch.cuda.synchronize()
        moved.append((start, trained, tr.float_state().cpu(), dp.stats.cpu()))
        assert torch.equal(dp.anchor, tr.float_state())
    return data, tr, dp, moved


def test_lenet_two_rounds_clipped_world1(gpu_device):
    """train_epoch() + FedAvg(dp=clip).average() twice at world 1: the model never moves farther than S from the
    round's start, and after_aggregate re-packed the PRIVATISED weights -- a fresh trainer loaded from the state dict
    evaluates to the same bits."""
    from fedmi.engine import build_trainer
    from fedmi.engine.base import TrainerConfig

    data, tr, dp, moved = _lenet_rounds(gpu_device, 0.0)
    n = tr.float_state().numel()
    for start, trained, after, stats in moved:
        scale = check_stats(trained, start, n, CLIP, stats)
        assert scale < 1.0, f"S = {CLIP} did not clip an update of norm {float(stats[1]):.4g}"
        check_clip(trained, start, after, n, dp.cfg, scale)
        assert update_norm(after, start, n) <= CLIP * CLIP_SLACK
    assert dp.draw == 2
    rec = dp.round_stats()
    assert rec["dp_scale"] == float(moved[-1][3][2]) and rec["dp_epsilon"] is None
    tr.evaluate()
    got = tr.eval_stats()
    fresh = build_trainer("lenet", data, gpu_device, TrainerConfig(seed=2),
                          init_state={k: v.clone() for k, v in tr.state_dict().items()})
    fresh.evaluate()
    want = fresh.eval_stats()
    assert got.count == 128 and (got.loss_sum, got.correct, got.count) == (want.loss_sum, want.correct, want.count)


def test_lenet_two_rounds_noised_reproducible_with_a_seed(gpu_device):
    runs = [_lenet_rounds(gpu_device, 0.5, seed=5) for _ in range(2)]
    (_, tr_a, dp_a, moved_a), (_, tr_b, dp_b, moved_b) = runs
    assert dp_a.key == dp_b.key and dp_a.draw == dp_b.draw == 2
    assert torch.equal(tr_a.float_state(), tr_b.float_state())
    n = tr_a.float_state().numel()
    for (start, trained, after, stats), (_, _, after_b, _) in zip(moved_a, moved_b):
        assert torch.equal(after, after_b)
        # the noise is there: sigma = z * S on every entry, far above the clip's own rounding
        noise = after.double() - reference_privatize(trained, start, n, DpConfig(CLIP), 1, 0, 0,
                                                     scale=float(stats[2]))[0]
        assert float(noise.std()) == pytest.approx(0.5 * CLIP, rel=0.05)
    assert dp_a.round_stats()["dp_epsilon"] == pytest.approx(2 / (2 * 0.25) + (2 * 2 * 11.512925464970229) ** 0.5 / 0.5)
