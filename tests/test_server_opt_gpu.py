"""The server-optimizer HIP kernel (csrc/kernels/server_opt.hip) against its fp64 twin, and the LeNet engine
end to end with FedAvgM at world 1.  Bounds and inputs: tests/server_opt_check.py."""
import functools

import pytest
import torch

from fedmi import native
from fedmi.parallel.fedavg import FedAvg
from fedmi.parallel.server_opt import KINDS, ServerOptConfig, make_server_opt
from tests.server_opt_check import YOGI_MAX_SHARE, check_step, draw_inputs, next_round

pytestmark = pytest.mark.gpu

BIG = 2048 * 256 * 4 + 5          # past the 2048-block grid cap: the grid-stride loop and the tail both run
# (n, n_opt): tail only; no straddle with everything / nothing optimised; a straddling vector; past the grid cap
SHAPES = [(3, 3), (1027, 1027), (1027, 0), (1500, 1001), (BIG, BIG)]
SEEDS = (0, 1, 2)
STEPS = 3


@pytest.fixture(scope="module")
def nat(gpu_device):
    return native.require()


@functools.lru_cache(maxsize=None)
def _case(n: int, seed: int):
    """The inputs of one (n, seed) and the client progress added before steps 2 and 3; shared by the four
    kinds and never written."""
    x, anchor, m, v, g = draw_inputs(n, seed)
    noise = [next_round(torch.zeros(n), g) for _ in range(STEPS - 1)]
    return x, anchor, m, v, noise


def _launch(nat, cfg, x, anchor, m, v, n, n_opt):
    nat.server_opt(native.stream_handle(), x.data_ptr(), anchor.data_ptr(), m.data_ptr(),
                   0 if v is None else v.data_ptr(), n, n_opt, cfg.kind_id, cfg.lr, cfg.beta1, cfg.beta2, cfg.tau)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,n_opt", SHAPES)
def test_kernel_matches_fp64_twin(nat, gpu_device, n, n_opt, kind):
    cfg = ServerOptConfig(kind)
    for seed in SEEDS:
        x0, a0, m0, v0, noise = _case(n, seed)
        x, a, m, v = (t.to(gpu_device) for t in (x0, a0, m0, v0))
        left_out = torch.zeros(n_opt, dtype=torch.bool)
        for step in range(STEPS):
            pre = tuple(t.cpu() for t in (x, a, m, v))
            _launch(nat, cfg, x, a, m, v, n, n_opt)
            torch.cuda.synchronize()
            left_out |= check_step(cfg, pre, tuple(t.cpu() for t in (x, a, m, v)), n_opt)
            if step < STEPS - 1:
                x.add_(noise[step].to(gpu_device))
        if n_opt:
            assert left_out.float().mean().item() <= YOGI_MAX_SHARE, (seed, int(left_out.sum()))


def test_fedavgm_never_touches_v(nat, gpu_device):
    n, n_opt = 1500, 1001
    cfg = ServerOptConfig("fedavgm")
    x0, a0, m0, _, _ = _case(n, 0)
    xa, aa, ma = (t.to(gpu_device) for t in (x0, a0, m0))
    _launch(nat, cfg, xa, aa, ma, None, n, n_opt)                 # v null
    xb, ab, mb = (t.to(gpu_device) for t in (x0, a0, m0))
    sentinel = torch.full((n,), -12345.0, device=gpu_device)
    _launch(nat, cfg, xb, ab, mb, sentinel, n, n_opt)
    torch.cuda.synchronize()
    assert bool((sentinel == -12345.0).all())
    for p, q in ((xa, xb), (aa, ab), (ma, mb)):
        assert torch.equal(p, q)
    check_step(cfg, (x0, a0, m0, None), (xa.cpu(), aa.cpu(), ma.cpu(), None), n_opt)


def test_binding_rejects_bad_arguments(nat, gpu_device):
    """Refused before any launch: an unknown kind, n_opt outside [0, n], a null or misaligned buffer."""
    t = torch.zeros(64, device=gpu_device)
    p, s = t.data_ptr(), native.stream_handle()
    for args in ((p, p, p, p, 16, 16, 4), (p, p, p, p, 16, 17, 3), (p, p, p, p, 16, -1, 3), (p, p, p, 0, 16, 16, 3),
                 (0, p, p, p, 16, 16, 0), (p + 4, p, p, p, 16, 16, 0), (p, p, p, p + 8, 16, 16, 1)):
        with pytest.raises(ValueError):
            nat.server_opt(s, *args, 1.0, 0.9, 0.99, 1e-3)
    nat.server_opt(s, p, p, p, 0, 0, 0, 0, 1.0, 0.9, 0.99, 1e-3)   # n = 0: nothing to do
    torch.cuda.synchronize()
    assert not t.any()


def test_lenet_two_rounds_fedavgm_world1(gpu_device):
    """train_epoch() + FedAvg(server_opt=fedavgm).average() twice at world 1 (the pseudo-gradient is the
    client's own update): float_state() follows the twin, and after_aggregate re-packed the STEPPED weights --
    a fresh trainer loaded from the state dict evaluates to the same bits."""
    from fedmi.engine import build_trainer
    from fedmi.engine.base import TrainerConfig
    from fedmi.engine.data import make_dataset, strided_schedule

    data = make_dataset("synthetic-cifar10", device=gpu_device, n_train=384, n_test=128, seed=0)
    tr = build_trainer("lenet", data, gpu_device, TrainerConfig(seed=1))
    n = tr.float_state().numel()
    assert tr.n_params() == n
    so = make_server_opt("fedavgm", tr)
    fa = FedAvg(server_opt=so)
    tr.set_schedule(*strided_schedule(384, 128, 0, 1))
    for rnd in range(2):
        tr.train_epoch()
        torch.cuda.synchronize()
        pre = (tr.float_state().cpu(), so.anchor.cpu(), so.m.cpu(), None)
        assert not torch.equal(pre[0], pre[1])                    # the epoch moved the model off the anchor
        fa.average(tr)
        torch.cuda.synchronize()
        check_step(so.cfg, pre, (tr.float_state().cpu(), so.anchor.cpu(), so.m.cpu(), None), n)
        if rnd == 1:
            assert not torch.equal(tr.float_state().cpu(), pre[0])   # momentum: not the plain mean any more
    assert so.steps == 2 and fa.timer.calls == 2
    tr.evaluate()
    got = tr.eval_stats()
    fresh = build_trainer("lenet", data, gpu_device, TrainerConfig(seed=2),
                          init_state={k: v.clone() for k, v in tr.state_dict().items()})
    fresh.evaluate()
    want = fresh.eval_stats()
    assert got.count == 128 and (got.loss_sum, got.correct, got.count) == (want.loss_sum, want.correct, want.count)
