"""The fused LeNet step (KS1 lenet_sample_step + KS2 lenet_sgd2) at the batch sizes and buffer states
the main parametrisation of tests/test_lenet_kernels_gpu.py does not reach.

* the torch-math comparison of ``test_step_matches_torch_math`` (same 2e-2 per-tensor bound, same loss /
  correct checks: it is that function, called at other shapes) at nb = 1, nb = 7 (inside one 8-sample
  fragment of KS2's column mask), nb = 120 (last fragment empty) and nb = 128 right after an nb = 7 step on
  the same buffers (the unmasked full-batch KS2 path over scratch that held a partial batch);
* bitwise determinism at nb = 7 and nb = 128, and eager vs graph replay of a schedule ending in a partial batch;
* the conv backward's partial LDS clear: a step must not depend on what the previous step left behind, at
  the crop offsets that put real pixels next to every pad of the shifted image copies.
"""
import numpy as np
import pytest
import torch

from fedmi.engine.base import TrainerConfig
from fedmi.engine.data import crop_flip_params
from fedmi.engine.lenet_native import LeNetNativeTrainer
from tests import test_lenet_kernels_gpu as base
from tests.test_lenet_kernels_gpu import env  # noqa: F401  (module-scoped fixture: dataset, reference model, trainer)

pytestmark = pytest.mark.gpu

SEED = base.SEED


@pytest.mark.parametrize("start,nb", [(5, 1), (640, 7), (256, 120)])
def test_step_matches_torch_math_small(env, start, nb):  # noqa: F811
    base.test_step_matches_torch_math(env, start, nb, True)


def test_full_batch_after_partial_batch(env):  # noqa: F811
    nat, dev, ds, ref, tr = env
    tr.load_state_dict(ref.state_dict())
    tr.round_ctr.zero_()
    base._step_grad(tr, 384, 7)          # leaves a 7-column batch in the KS1 -> KS2 operand buffers
    base.test_step_matches_torch_math(env, 512, 128, True)


@pytest.mark.parametrize("nb", [7, 128])
def test_step_is_deterministic_small(env, nb):  # noqa: F811
    nat, dev, ds, ref, tr = env
    res = []
    for _ in range(2):
        tr.load_state_dict(ref.state_dict())
        tr.round_ctr.zero_()
        g, st = base._step_grad(tr, 128, nb)
        res.append((tr.params.clone(), tr.mom.clone(), st))
    (p0, m0, s0), (p1, m1, s1) = res
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(s0, s1)
    tr.load_state_dict(ref.state_dict())
    tr.mom.zero_()


def test_graph_replay_is_bitwise_eager_partial_tail(env):  # noqa: F811
    nat, dev, ds, ref, tr = env
    starts, sizes = [0, 128, 256], [128, 128, 40]
    res = []
    try:
        for use_graph in (False, True):
            tr.load_state_dict(ref.state_dict())
            tr.mom.zero_()
            tr.round_ctr.zero_()
            tr.cfg.use_graph = use_graph
            tr.set_schedule(starts, sizes)
            tr.train_epoch()
            torch.cuda.synchronize()
            res.append((tr.params.clone(), tr.mom.clone(), tr.stats[0].clone()))
    finally:
        tr.cfg.use_graph = True
        tr.set_schedule([], [])
        tr.load_state_dict(ref.state_dict())
        tr.mom.zero_()
        tr.round_ctr.zero_()
    (pe, me, se), (pg, mg, sg) = res
    assert int(se[2]) == sum(sizes)
    assert torch.equal(pe, pg) and torch.equal(me, mg) and torch.equal(se, sg)


def _round_with(gidx, i0, j0, flip):
    """A round counter at which sample gidx draws exactly this crop / flip."""
    r = np.arange(1, 40000)
    a, b, f = crop_flip_params(SEED, r, np.full_like(r, gidx))
    hit = np.nonzero((a == i0) & (b == j0) & (f == flip))[0]
    assert len(hit), (gidx, i0, j0, flip)
    return int(r[hit[0]])


def _fresh(ds, dev, ref):
    tr = LeNetNativeTrainer(ds, dev, TrainerConfig(seed=SEED), init_state=ref.state_dict())
    torch.cuda.synchronize()
    return tr


def _one(tr, ref, rnd, start, nb):
    tr.load_state_dict(ref.state_dict())
    tr.mom.zero_()
    tr.stats.zero_()
    tr.round_ctr.fill_(rnd)
    tr.train_step(start, nb)
    torch.cuda.synchronize()
    return tr.params.clone(), tr.mom.clone(), tr.stats[0].clone()


@pytest.mark.parametrize("i0,j0,flip", [(0, 0, 0), (0, 8, 1), (8, 0, 1), (8, 8, 0)])
def test_step_ignores_previous_steps_lds(env, i0, j0, flip):  # noqa: F811
    """Step 2 (one sample B at crop (i0, j0)) after step 1 (a full batch on every CU whose first sample A has
    the opposite crop corner and the opposite flip, so A's shifted copies differ from B's everywhere) equals,
    bit for bit, the same step 2 run first in a fresh engine: nothing the partial clear leaves uncleared in
    LDS is read."""
    nat, dev, ds, ref, tr = env
    a, b = 128, 700
    ra = _round_with(a, 8 - i0, 8 - j0, 1 - flip)
    rb = _round_with(b, i0, j0, flip)
    t1 = _fresh(ds, dev, ref)
    _one(t1, ref, ra, a, 128)
    after = _one(t1, ref, rb, b, 1)
    first = _one(_fresh(ds, dev, ref), ref, rb, b, 1)
    for x, y in zip(after, first):
        assert torch.equal(x, y)
