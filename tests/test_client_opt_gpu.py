"""The client-optimizer HIP kernels (csrc/kernels/client_opt.hip) against their twins, and the engines' hook:
the correction sits between the backward pass and the unchanged SGD tail, is captured into the step graph, and
the capture's warm-up step leaves nothing in SCAFFOLD's gradient sum.  Inputs and checks: tests/client_opt_check.py."""
import functools

import pytest
import torch

from fedmi import native
from fedmi.parallel.client_opt import ClientOpt, ClientOptConfig, fma32, make_client_opt
from tests.client_opt_check import (SEEDS, SIZES, check_begin, check_fedprox, check_finish, check_scaffold_drift,
                                    draw_inputs)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def nat(gpu_device):
    return native.require()


@functools.lru_cache(maxsize=None)
def _case(n: int, seed: int) -> dict:
    """The CPU inputs of one (n, seed): shared by every kernel test and never written."""
    return draw_inputs(n, seed)


def _dev(x: dict, dev, *names):
    return [x[k].to(dev) for k in names]


def _drift(nat, kind, g, p=None, anchor=None, corr=None, acc=None, mu=0.0):
    ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
    nat.drift_grad(native.stream_handle(), kind, g.data_ptr(), ptr(p), ptr(anchor), ptr(corr), ptr(acc), mu, g.numel())


# ---- 1. the kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_drift_grad_fedprox(nat, gpu_device, n):
    for seed in SEEDS:
        x = _case(n, seed)
        for mu in (0.01, 0.1):
            g, p, a = _dev(x, gpu_device, "g", "p", "anchor")
            _drift(nat, 0, g, p, a, mu=mu)
            torch.cuda.synchronize()
            got = g.cpu()
            check_fedprox(mu, x["g"], x["p"], x["anchor"], got)
            assert torch.equal(p.cpu(), x["p"]) and torch.equal(a.cpu(), x["anchor"])
            # the CPU twin is the same single rounding: the engines' CPU and GPU paths agree bit for bit
            assert torch.equal(got, fma32(mu, x["p"] - x["anchor"], x["g"]))


@pytest.mark.parametrize("n", SIZES)
def test_scaffold_kernels_bitwise(nat, gpu_device, n):
    s = native.stream_handle()
    for seed in SEEDS:
        x = _case(n, seed)
        g, corr, acc, ci, c, dmean = _dev(x, gpu_device, "g", "corr", "acc", "ci", "c", "dmean")
        _drift(nat, 1, g, corr=corr, acc=acc)
        torch.cuda.synchronize()
        check_scaffold_drift(x["g"], x["corr"], x["acc"], g.cpu(), acc.cpu())
        assert torch.equal(corr.cpu(), x["corr"])
        for K in (1, 3, 391):
            acc, ci = _dev(x, gpu_device, "acc", "ci")
            delta = torch.full((n,), SENTINEL, device=gpu_device)
            nat.scaffold_finish(s, acc.data_ptr(), ci.data_ptr(), delta.data_ptr(), K, n)
            torch.cuda.synchronize()
            check_finish(x["acc"], x["ci"], K, ci.cpu(), delta.cpu())
            assert torch.equal(acc.cpu(), x["acc"])
        acc, ci = _dev(x, gpu_device, "acc", "ci")
        corr = torch.full((n,), SENTINEL, device=gpu_device)
        nat.scaffold_begin(s, c.data_ptr(), dmean.data_ptr(), ci.data_ptr(), corr.data_ptr(), acc.data_ptr(), n)
        torch.cuda.synchronize()
        check_begin(x["c"], x["dmean"], x["ci"], c.cpu(), corr.cpu(), acc.cpu())
        assert torch.equal(ci.cpu(), x["ci"]) and torch.equal(dmean.cpu(), x["dmean"])


def test_a_kind_never_touches_the_other_kinds_buffers(nat, gpu_device):
    n = 1027
    x = _case(n, 0)
    sent = lambda: torch.full((n,), SENTINEL, device=gpu_device)   # noqa: E731
    # fedprox: corr / acc null, then sentinels
    g0, p, a = _dev(x, gpu_device, "g", "p", "anchor")
    _drift(nat, 0, g0, p, a, mu=0.1)
    g1, = _dev(x, gpu_device, "g")
    s1, s2 = sent(), sent()
    _drift(nat, 0, g1, p, a, corr=s1, acc=s2, mu=0.1)
    torch.cuda.synchronize()
    assert torch.equal(g0, g1) and bool((s1 == SENTINEL).all()) and bool((s2 == SENTINEL).all())
    # scaffold: p / anchor null, then NaN-filled (a read would poison g) and checked unwritten
    g0, corr, acc0 = _dev(x, gpu_device, "g", "corr", "acc")
    _drift(nat, 1, g0, corr=corr, acc=acc0)
    g1, acc1 = _dev(x, gpu_device, "g", "acc")
    s1, s2 = sent(), sent()
    _drift(nat, 1, g1, p=s1, anchor=s2, corr=corr, acc=acc1, mu=float("nan"))
    torch.cuda.synchronize()
    assert torch.equal(g0, g1) and torch.equal(acc0, acc1)
    assert bool((s1 == SENTINEL).all()) and bool((s2 == SENTINEL).all())
    check_scaffold_drift(x["g"], x["corr"], x["acc"], g1.cpu(), acc1.cpu())


def test_bindings_reject_bad_arguments(nat, gpu_device):
    """Refused before any launch: an unknown kind, a null or misaligned buffer the kind uses, K < 1, n < 0."""
    t = torch.zeros(64, device=gpu_device)
    p, s = t.data_ptr(), native.stream_handle()
    for args in ((2, p, p, p, p, p), (-1, p, p, p, p, p), (0, 0, p, p, 0, 0), (0, p, 0, p, 0, 0), (0, p, p, 0, 0, 0),
                 (1, p, 0, 0, 0, p), (1, p, 0, 0, p, 0), (1, 0, 0, 0, p, p), (0, p + 4, p, p, 0, 0),
                 (0, p, p, p + 8, 0, 0), (1, p, 0, 0, p + 4, p), (1, p, 0, 0, p, p + 12)):
        with pytest.raises(ValueError):
            nat.drift_grad(s, *args, 0.1, 16)
    with pytest.raises(ValueError):
        nat.drift_grad(s, 0, p, p, p, 0, 0, 0.1, -1)
    for args in ((p, p, p, 0, 16), (p, p, p, -3, 16), (0, p, p, 1, 16), (p, 0, p, 1, 16), (p, p, 0, 1, 16),
                 (p + 4, p, p, 1, 16), (p, p, p + 8, 1, 16), (p, p, p, 1, -1)):
        with pytest.raises(ValueError):
            nat.scaffold_finish(s, *args)
    for args in ((0, p, p, p, p, 16), (p, 0, p, p, p, 16), (p, p, 0, p, p, 16), (p, p, p, 0, p, 16),
                 (p, p, p, p, 0, 16), (p, p + 4, p, p, p, 16), (p, p, p, p, p, -1)):
        with pytest.raises(ValueError):
            nat.scaffold_begin(s, *args)
    nat.drift_grad(s, 0, 0, 0, 0, 0, 0, 0.1, 0)                 # n = 0: nothing to do, nothing dereferenced
    nat.drift_grad(s, 1, 0, 0, 0, 0, 0, 0.1, 0)
    nat.scaffold_finish(s, 0, 0, 0, 1, 0)
    nat.scaffold_begin(s, 0, 0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert not t.any()


# ---- 2. CNNNativeTrainer("resnet18") -------------------------------------------------------------------------------------
NB = 128


@pytest.fixture(scope="module")
def cnn(gpu_device):
    """256 synthetic images, one shared init, and the plain engine's two eager steps: every step's raw gradient,
    the model and the momentum after the epoch."""
    from fedmi.engine.cnn_native import CNNNativeTrainer
    from fedmi.engine.data import make_dataset
    from fedmi.models import build_model

    data = make_dataset("synthetic-cifar10-easy", device=gpu_device, n_train=256, n_test=64, seed=0)
    init = build_model("ResNet18").state_dict()

    def make(graph: bool):
        from fedmi.engine.base import TrainerConfig

        tr = CNNNativeTrainer("resnet18", data, gpu_device, TrainerConfig(batch_size=NB, lr=0.05, use_graph=graph, seed=3),
                              init_state=init)
        tr.set_schedule([0, NB], [NB, NB])
        return tr

    plain = make(False)
    plain.model.train()
    plain.stats[0].zero_()
    plain.counter.zero_()
    raw = []
    for _ in range(2):                      # train_epoch()'s eager loop, with a look at the gradient in between
        plain._train_step(NB)
        raw.append(plain.fs.grad.clone())
    torch.cuda.synchronize()
    return dict(make=make, raw=raw, x=plain.float_state().clone(), mom=plain.momentum_state().clone())


def _perturb(co, seed: int = 11) -> None:
    """A correction that matters: fedprox's anchor moved off the model, scaffold's corr non-zero."""
    g = torch.Generator().manual_seed(seed)
    t = co.anchor if co.cfg.kind == "fedprox" else co.corr
    t.add_((1e-2 if co.cfg.kind == "fedprox" else 1e-3) * torch.randn(t.numel(), generator=g).to(t.device))


@pytest.mark.parametrize("kind", ["fedprox", "scaffold"])
def test_cnn_noop_correction_is_the_plain_epoch(cnn, kind):
    """fedprox with mu = 0 and scaffold's first round (corr = 0) change nothing, through graph replay; scaffold's
    acc is the in-order fp32 sum of the two RAW gradients -- the capture's warm-up step left nothing in it."""
    tr = cnn["make"](True)
    co = make_client_opt(kind, tr, 0.0)
    tr.train_epoch()
    torch.cuda.synchronize()
    assert ("train", NB) in tr._graphs and co.K == 2
    assert torch.equal(tr.float_state(), cnn["x"])
    assert torch.equal(tr.momentum_state(), cnn["mom"])
    if kind == "scaffold":
        assert torch.equal(co.acc, (torch.zeros_like(cnn["raw"][0]) + cnn["raw"][0]) + cnn["raw"][1])
        assert not co.corr.any() and not co.ci.any()


@pytest.mark.parametrize("kind", ["fedprox", "scaffold"])
def test_cnn_graph_replay_equals_eager_with_a_live_correction(cnn, kind):
    runs = []
    for graph in (False, True):
        tr = cnn["make"](graph)
        co = make_client_opt(kind, tr, 0.1)
        _perturb(co)
        tr.train_epoch()
        torch.cuda.synchronize()
        runs.append((tr.float_state().clone(), tr.momentum_state().clone(), None if co.acc is None else co.acc.clone()))
    (xe, me, ae), (xg, mg, ag) = runs
    assert not torch.equal(xe, cnn["x"])                       # the correction did move the trajectory
    assert torch.equal(xe, xg) and torch.equal(me, mg)
    if kind == "scaffold":
        assert torch.equal(ae, ag) and ae.any()


def test_cnn_one_fedprox_step_is_grad_then_twin_then_sgd_flat(cnn, nat, gpu_device):
    """One step with anchor perturbed and mu = 0.1 against the same thing assembled by hand: grads_for_batch ->
    the CPU twin's correction -> sgd_flat on copies."""
    mu = 0.1
    a = cnn["make"](False)
    n = a.n_params()
    a.grads_for_batch(0, NB)
    torch.cuda.synchronize()
    ref = ClientOpt(a, ClientOptConfig("fedprox", mu))
    _perturb(ref)
    p = a.fs.params.clone()
    g = fma32(mu, p.cpu() - ref.anchor.cpu(), a.fs.grad.cpu()).to(gpu_device)
    assert not torch.equal(g, a.fs.grad)
    mom = a.momentum_state().clone()
    c = a.cfg
    nat.sgd_flat(native.stream_handle(gpu_device), p.data_ptr(), g.data_ptr(), mom.data_ptr(), n, c.lr, c.momentum,
                 c.weight_decay, 0.0, False, False)
    b = cnn["make"](False)
    b.set_schedule([0], [NB])
    co = make_client_opt("fedprox", b, mu)
    _perturb(co)
    assert torch.equal(co.anchor, ref.anchor)
    b.train_epoch()
    torch.cuda.synchronize()
    assert torch.equal(b.fs.params, p)
    assert torch.equal(b.momentum_state(), mom)
    assert co.K == 1


# ---- 3. TorchTrainer, hybrid ----------------------------------------------------------------------------------------------
def test_hybrid_scaffold_graph_equals_eager_and_acc_is_the_raw_sum(gpu_device):
    from fedmi.engine import build_trainer
    from fedmi.engine.base import TrainerConfig
    from fedmi.engine.data import make_dataset

    nb = 128
    data = make_dataset("synthetic-mnist", device=gpu_device, n_train=2 * nb, n_test=64, seed=0)

    def make(graph: bool, init=None):
        tr = build_trainer("mlp", data, gpu_device, TrainerConfig(batch_size=nb, lr=0.05, seed=3, use_graph=graph),
                           init_state=init)
        assert tr.hybrid and tr.use_graph == graph
        tr.set_schedule([0, nb], [nb, nb])
        return tr

    plain = make(False)
    init = {k: v.detach().clone() for k, v in plain.state_dict().items()}
    plain.model.train()
    raw = []
    for s in (0, nb):
        plain.train_step(s, nb)
        raw.append(plain.fs.grad.clone())
    # first round (corr = 0): the plain trajectory, acc = the raw sum, through the captured graph
    tr = make(True, init)
    co = make_client_opt("scaffold", tr)
    tr.train_epoch()
    torch.cuda.synchronize()
    assert tr._graph is not None and co.K == 2
    assert torch.equal(tr.float_state(), plain.float_state())
    assert torch.equal(co.acc, (torch.zeros_like(raw[0]) + raw[0]) + raw[1])
    # a live correction: graph replay == eager
    runs = []
    for graph in (False, True):
        tr = make(graph, init)
        co = make_client_opt("scaffold", tr)
        _perturb(co)
        tr.train_epoch()
        torch.cuda.synchronize()
        runs.append((tr.float_state().clone(), tr.momentum_state().clone(), co.acc.clone()))
    for e, g in zip(*runs):
        assert torch.equal(e, g)
    assert not torch.equal(runs[0][0], plain.float_state())


# ---- 4. LeNet -----------------------------------------------------------------------------------------------------------------
def test_lenet_native_engine_has_no_hook(gpu_device):
    from fedmi.engine import build_trainer
    from fedmi.engine.base import TrainerConfig
    from fedmi.engine.data import make_dataset
    from fedmi.engine.lenet_native import LeNetNativeTrainer

    data = make_dataset("synthetic-cifar10", device=gpu_device, n_train=128, n_test=64, seed=0)
    tr = build_trainer("lenet", data, gpu_device, TrainerConfig(seed=1))
    assert isinstance(tr, LeNetNativeTrainer)
    with pytest.raises(NotImplementedError):
        tr.set_client_opt(object())
    with pytest.raises(NotImplementedError):
        make_client_opt("scaffold", tr)
