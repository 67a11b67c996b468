"""The FC tail of the fused LeNet step (KS1): fc3, cross-entropy, dZ3 and dH2 use one or two waves between
workgroup barriers, and the conv backward's shifted copies are built around them.  Any other thread mapping of
that tail (round 19 tried the whole tail in wave 0 with the builders beside it, `profiles/r19_lenet_fc_tail/`)
has to reproduce the step at these edges:

* the step is the recorded step: ``tests/golden/lenet_fc_tail_parent.json``
  (``tools/record_lenet_fc_tail.py``, recorded twice at the commit before the change, both records
  identical) holds SHA-256 of params || momentum and the stats row for batch sizes 1, 2, 33 and 128 -- class 0
  and class 9, the first and last cross-entropy lanes, at the single-sample steps -- on three parameter sets:
  fc3 zeroed, fc2 dead, random; two eager steps and one graph epoch of the schedule sizes [128, 1, 33] each;
* with fc3.weight = fc3.bias = 0 all logits tie: argmax is class 0, ``correct`` counts the label-0 samples,
  the mean loss is ln 10;
* with fc2.bias = -10 every h2 is dead: dZ2 is zero, so from zero momentum every gradient but fc3.bias's is
  weight decay alone (momentum == wd * p, exactly);
* a step does not depend on what the previous step left in the shifted copies: a full batch whose first sample
  has crop (8, 8) flipped, then a step at crop (0, 0) unflipped on another sample, equals that second step in a
  fresh engine, bit for bit.
"""
import importlib.util
import json
import math
from pathlib import Path

import pytest
import torch

from fedmi.engine.base import TrainerConfig
from fedmi.engine.lenet_native import LeNetNativeTrainer
from tests.test_lenet_kernels_gpu import env  # noqa: F401  (module-scoped fixture: dataset, reference model, trainer)
from tests.test_lenet_step_small_gpu import _fresh, _one, _round_with

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _tool():
    spec = importlib.util.spec_from_file_location("record_lenet_fc_tail", ROOT / "tools" / "record_lenet_fc_tail.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool()


def test_fc_tail_hashes_match_parent_record(gpu_device, tool):
    want = json.loads((ROOT / "tests" / "golden" / "lenet_fc_tail_parent.json").read_text())
    got = tool.compute(gpu_device)
    assert got["dataset"] == want["dataset"], "the record's inputs are not reproduced"
    assert got["eager_steps"] == want["eager_steps"] and got["schedule"] == want["schedule"]
    assert sorted(want["cases"]) == sorted(tool.CASES)
    for case in tool.CASES:
        g, w = got["cases"][case], want["cases"][case]
        assert g["init"] == w["init"], case
        assert len(w["eager"]) == 2 and len(w["graph"]) == 1
        for kind in ("eager", "graph"):
            for i, (a, b) in enumerate(zip(g[kind], w[kind])):
                assert a == b, (case, kind, i)
    assert got == want


def test_record_plan_covers_the_edges(tool):
    ds = tool.dataset()
    y = ds.train.y
    eager, starts, sizes = tool.plan(ds)
    assert sorted({nb for _, nb in eager} | set(sizes)) == [1, 2, 33, 128]
    (s0, n0), (s1, n1) = eager
    assert n0 == 1 and int(y[s0]) == 0                      # class 0 alone: the first CE lane
    assert n1 == 2 and int(y[s1 + 1]) == 9                  # class 9: the last CE lane
    assert sizes[1] == 1 and int(y[starts[1]]) == 9
    seen = set()
    for s, n in zip(starts, sizes):
        seen |= set(y[s:s + n].tolist())
    assert seen == set(range(10))


@pytest.fixture(scope="module")
def steps(tool):
    """(start, nb) at the four batch sizes, from the record's plan."""
    eager, starts, sizes = tool.plan(tool.dataset())
    return [eager[0], eager[1], (starts[2], sizes[2]), (starts[0], sizes[0])]


def _single_step(tool, ds, dev, case, start, nb):
    """One eager step of a fresh engine (zero momentum) on the parameter set 'case'."""
    tr = LeNetNativeTrainer(ds, dev, TrainerConfig(seed=tool.SEED), init_state=tool.init_state(case))
    p0 = tr.params.clone()
    tr.round_ctr.fill_(3)
    tr.train_step(start, nb)
    torch.cuda.synchronize()
    return tr, p0


@pytest.mark.parametrize("k", range(4), ids=["nb1", "nb2", "nb33", "nb128"])
def test_all_logits_tie_argmax_is_class_0(env, tool, steps, k):  # noqa: F811
    nat, dev, ds, ref, _ = env
    start, nb = steps[k]
    tr, _p0 = _single_step(tool, ds, dev, "zero_fc3", start, nb)
    st = tr.train_stats()
    labels = ds.train.y[start:start + nb]
    assert st.count == nb
    assert st.correct == int((labels == 0).sum())
    # every sample's loss is ln 10 (fp32 exp / log of exact zeros: a few ulp of 1.2e-7 * 2.3); st.loss is the mean
    assert abs(st.loss - math.log(10.0)) < 1e-5


@pytest.mark.parametrize("k", range(4), ids=["nb1", "nb2", "nb33", "nb128"])
def test_dead_fc2_leaves_weight_decay_alone(env, tool, steps, k):  # noqa: F811
    nat, dev, ds, ref, _ = env
    start, nb = steps[k]
    tr, p0 = _single_step(tool, ds, dev, "dead_fc2", start, nb)
    wd = torch.tensor(tr.cfg.weight_decay, dtype=torch.float32, device=dev)
    assert torch.isfinite(tr.mom).all()
    for name, view in tr.state_dict().items():
        lo, n = view.storage_offset(), view.numel()
        m, want = tr.mom[lo:lo + n], p0[lo:lo + n] * wd
        if name == "fc3.bias":               # the only gradient that reaches the parameters: dZ3
            assert not torch.equal(m, want)
        else:                                # from zero momentum: m = wd * p + 0, one rounding
            assert torch.equal(m, want), name


@pytest.mark.parametrize("nb2", [1, 2])
def test_step_ignores_previous_steps_shifted_copies(env, nb2):  # noqa: F811
    nat, dev, ds, ref, _ = env
    a, b = 128, 700
    ra = _round_with(a, 8, 8, 1)
    rb = _round_with(b, 0, 0, 0)
    t1 = _fresh(ds, dev, ref)
    _one(t1, ref, ra, a, 128)
    after = _one(t1, ref, rb, b, nb2)
    first = _one(_fresh(ds, dev, ref), ref, rb, b, nb2)
    for x, y in zip(after, first):
        assert torch.equal(x, y)
