"""The KS2 -> KS1 seam of the fused LeNet step.

* KS2's FC tiles store their packed bf16 images from the tile's own (n, f) instead of through the generic
  ``pack_one``: after any step ``pk`` must equal, bit for bit and padding included, ``lenet_pack(params)``
  into a zeroed buffer (the generic pack is the reference).
* the augmented bf16 image KS1 stages is prepared a step ahead (``lenet_prep_batch``, and the extra workgroups
  of the previous KS2): its geometry is checked exactly and its values to one bf16 ulp against a numpy
  reference built from ``fedmi.engine.data.crop_flip_params`` (the exact bits are pinned by the record below).
* graph replay of an irregular schedule (partial batch in the middle, non-contiguous starts, partial tail)
  over two epochs equals the same steps issued one by one; an eager step after a graph epoch, and a graph
  epoch after a schedule change, depend on nothing an earlier launch left behind.
* the step is the recorded step: ``tests/golden/lenet_steps_parent.json`` holds SHA-256 of params || momentum
  and the stats row after each of 12 eager steps and 2 graph epochs, recorded by
  ``tools/record_lenet_steps.py`` at the commit before the seam work.  The record is re-made only by a change
  that is MEANT to alter the step's arithmetic; a change to how the step is scheduled has to reproduce it.
"""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from fedmi import native
from fedmi.engine.base import TrainerConfig
from fedmi.engine.data import CIFAR_MEAN, CIFAR_STD, crop_flip_params
from fedmi.engine.lenet_native import LeNetNativeTrainer
from tests import test_lenet_kernels_gpu as base
from tests.test_lenet_kernels_gpu import env  # noqa: F401  (module-scoped fixture: dataset, reference model, trainer)

pytestmark = pytest.mark.gpu

SEED = base.SEED
ROOT = Path(__file__).resolve().parent.parent
STARTS, SIZES = [0, 640, 256, 384], [128, 7, 128, 40]


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _reset(tr, ref, rnd=0):
    tr.load_state_dict(ref.state_dict())
    tr.mom.zero_()
    tr.stats.zero_()
    tr.round_ctr.fill_(rnd)


def _state(tr):
    torch.cuda.synchronize()
    return tr.params.clone(), tr.mom.clone(), tr.stats[0].clone()


# ---- 1. pack equivalence ----------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [[(5, 1)], [(640, 7)], [(256, 128)], [(0, 128), (640, 7), (256, 128)]],
                         ids=["nb1", "nb7", "nb128", "seq128_7_128"])
def test_pk_is_generic_pack_of_params(env, steps):  # noqa: F811
    nat, dev, ds, ref, tr = env
    _reset(tr, ref)
    try:
        for start, nb in steps:          # momentum carries over the sequence
            tr.train_step(start, nb)
        torch.cuda.synchronize()
        fresh = torch.zeros_like(tr.pk)
        nat.lenet_pack(native.stream_handle(), tr.params.data_ptr(), fresh.data_ptr())
        torch.cuda.synchronize()
        L = tr.L
        assert tr.pk.numel() == L["PK_TOTAL"]
        names = ["PK_W1C", "PK_W2C", "PK_W2DG", "PK_FC1", "PK_FC2", "PK_FC2T", "PK_FC3"]
        edges = [L[n] for n in names] + [L["PK_TOTAL"]]
        for n, lo, hi in zip(names, edges[:-1], edges[1:]):
            assert _same(tr.pk[lo:hi], fresh[lo:hi]), n
        assert _same(tr.pk, fresh)
        assert not _same(fresh, torch.zeros_like(fresh))
    finally:
        _reset(tr, ref)


# ---- 2. the prepared image ----------------------------------------------------------------------------------
def _round_with(gidx, i0, j0, flip):
    """A round counter at which sample gidx draws exactly this crop / flip."""
    r = np.arange(1, 40000)
    a, b, f = crop_flip_params(SEED, r, np.full_like(r, gidx))
    hit = np.nonzero((a == i0) & (b == j0) & (f == flip))[0]
    assert len(hit), (gidx, i0, j0, flip)
    return int(r[hit[0]])


def _source_map(i0, j0, flip):
    """Per sample: source row of every output row, source column of every output column, and validity."""
    ar = np.arange(32)
    ys = ar[None, :] + i0[:, None] - 4
    xs = np.where(flip[:, None] != 0, 31 - ar[None, :], ar[None, :]) + j0[:, None] - 4
    valid = ((ys >= 0) & (ys < 32))[:, :, None] & ((xs >= 0) & (xs < 32))[:, None, :]
    return ys, xs, valid


def _reference_image(x_u8, i0, j0, flip):
    """fp64 crop / flip / normalise of uint8 [nb, 3, 32, 32] as the padded channels-last [nb, 36, 40, 4]."""
    nb = x_u8.shape[0]
    ys, xs, valid = _source_map(i0, j0, flip)
    g = x_u8[np.arange(nb)[:, None, None, None], np.arange(3)[None, :, None, None],
             np.clip(ys, 0, 31)[:, None, :, None], np.clip(xs, 0, 31)[:, None, None, :]].astype(np.float64)
    v = np.where(valid[:, None], g / 255.0, 0.0)           # the crop pads with pixel 0 BEFORE normalising
    mean = np.asarray(CIFAR_MEAN, dtype=np.float64)[None, :, None, None]
    std = np.asarray(CIFAR_STD, dtype=np.float64)[None, :, None, None]
    full = np.zeros((nb, 36, 40, 4))
    full[:, :32, :32, :3] = ((v - mean) / std).transpose(0, 2, 3, 1)
    return full


def _prep(nat, tr, images, start, nb, rnd, augment):
    B, L = tr.L["MAX_TRAIN_BATCH"], tr.L
    assert (L["XP_H"], L["XP_W"], L["XP_C"]) == (36, 40, 4)
    fill = torch.full((B, L["XP_ELEMS"]), 1.5, dtype=torch.bfloat16, device=images.device)
    out = fill.clone()
    ctr = torch.full((4,), rnd, dtype=torch.int32, device=images.device)
    nat.lenet_prep_batch(native.stream_handle(), images.data_ptr(), start, nb, SEED, ctr.data_ptr(), int(augment),
                         out.data_ptr())
    torch.cuda.synchronize()
    assert _same(out[nb:], fill[nb:]), "samples >= nb of the buffer are untouched"
    return out[:nb].view(nb, 36, 40, 4)


PREP_CASES = [(0, 1, True, 1), (640, 7, True, 1), (256, 128, True, 2), (1024 - 40, 40, True, 1), (128, 7, False, 1),
              (700, 3, True, (0, 0, 0)), (700, 3, True, (0, 8, 1)), (700, 3, True, (8, 0, 1)), (700, 3, True, (8, 8, 0))]


@pytest.mark.parametrize("start,nb,augment,rnd", PREP_CASES)
def test_prepared_image_matches_numpy_reference(env, start, nb, augment, rnd):  # noqa: F811
    nat, dev, ds, ref, tr = env
    n_train = len(tr.train_set)
    assert start + nb <= n_train
    corner = rnd if isinstance(rnd, tuple) else None
    if corner:
        rnd = _round_with(start, *corner)
    gidx = np.arange(start, start + nb)
    if augment:
        i0, j0, flip = crop_flip_params(SEED, rnd, gidx)
    else:
        i0, j0, flip = np.full(nb, 4), np.full(nb, 4), np.zeros(nb, dtype=np.int64)
    if corner:
        assert (int(i0[0]), int(j0[0]), int(flip[0])) == corner

    # values: within one bf16 ulp of the fp64 formula; channel 3 and the pad exactly zero
    got_t = _prep(nat, tr, tr.train_set.x, start, nb, rnd, augment)
    zero = torch.zeros((), dtype=torch.bfloat16, device=dev)
    for pad in (got_t[:, 32:], got_t[:, :, 32:], got_t[..., 3]):
        assert _same(pad, zero.expand_as(pad)), "pad / channel 3 must be +0"
    got = got_t.double().cpu().numpy()
    want = _reference_image(tr.train_set.x[start:start + nb].cpu().numpy(), i0, j0, flip)
    inner_g, inner_w = got[:, :32, :32, :3], want[:, :32, :32, :3]
    ulp = 2.0 ** (np.floor(np.log2(np.abs(inner_w))) - 7)          # bf16: 8 significant bits
    assert np.all(np.abs(inner_g - inner_w) <= ulp)

    # geometry, exactly: images whose bytes name their own (row, column, sample), 8 codes apart (a bf16 value
    # here is within +-1 of its byte), pad pixels decode to byte 0
    ar = torch.arange(32, device=dev)
    coded = torch.empty(n_train, 3, 32, 32, dtype=torch.uint8, device=dev)
    coded[:, 0] = (8 * ar + 7).to(torch.uint8)[None, :, None]
    coded[:, 1] = (8 * ar + 7).to(torch.uint8)[None, None, :]
    tag = lambda g: (g * 37) % 31 * 8 + 7  # noqa: E731
    coded[:, 2] = tag(torch.arange(n_train, device=dev)).to(torch.uint8)[:, None, None]
    gc = _prep(nat, tr, coded, start, nb, rnd, augment).double().cpu().numpy()[:, :32, :32, :3]
    mean, std = np.asarray(CIFAR_MEAN), np.asarray(CIFAR_STD)
    byte = np.rint((gc * std + mean) * 255.0).astype(np.int64)
    ys, xs, valid = _source_map(i0, j0, flip)
    exp = np.zeros_like(byte)
    exp[..., 0] = np.where(valid, 8 * ys[:, :, None] + 7, 0)
    exp[..., 1] = np.where(valid, 8 * xs[:, None, :] + 7, 0)
    exp[..., 2] = np.where(valid, tag(gidx)[:, None, None], 0)
    assert np.all(np.abs(byte - exp) <= 1)


# ---- 3. graph == eager on an irregular schedule, two epochs -----------------------------------------------
def _eager_epoch(tr, starts, sizes):
    tr.stats.zero_()                     # the graph epoch's first node zeroes the train row
    for i, (s, n) in enumerate(zip(starts, sizes)):
        tr.train_step(s, n, bump_round=(i + 1 == len(starts)))
    return _state(tr)


def _graph_epoch(tr):
    tr.train_epoch()
    return _state(tr)


def test_graph_is_bitwise_eager_irregular_schedule_two_epochs(env):  # noqa: F811
    nat, dev, ds, ref, tr = env
    try:
        _reset(tr, ref)
        eager = [_eager_epoch(tr, STARTS, SIZES) for _ in range(2)]
        assert int(tr.round_ctr[0]) == 2
        _reset(tr, ref)
        tr.cfg.use_graph = True
        tr.set_schedule(STARTS, SIZES)
        graph = [_graph_epoch(tr) for _ in range(2)]
        assert int(tr.round_ctr[0]) == 2
    finally:
        tr.set_schedule([], [])
        _reset(tr, ref)
    for ep, (e, g) in enumerate(zip(eager, graph)):
        assert int(e[2][2]) == sum(SIZES)
        for x, y in zip(e, g):
            assert _same(x, y), ep
    assert not _same(eager[0][0], eager[1][0])


# ---- 4. nothing stale crosses from one launch sequence into the next -------------------------------------
def _fresh(ds, dev, ref):
    tr = LeNetNativeTrainer(ds, dev, TrainerConfig(seed=SEED), init_state=ref.state_dict())
    torch.cuda.synchronize()
    return tr


def _one(tr, ref, rnd, start, nb):
    _reset(tr, ref, rnd)
    tr.train_step(start, nb)
    return _state(tr)


def test_eager_step_after_graph_epoch_equals_fresh_engine(env):  # noqa: F811
    """After a graph epoch over the irregular schedule, an eager step on a batch that no step of that
    schedule would have followed with equals, bit for bit, the same step as a fresh engine's first."""
    nat, dev, ds, ref, tr = env
    t1 = _fresh(ds, dev, ref)
    t1.set_schedule(STARTS, SIZES)
    t1.train_epoch()
    torch.cuda.synchronize()
    after = _one(t1, ref, 5, 800, 100)
    first = _one(_fresh(ds, dev, ref), ref, 5, 800, 100)
    for x, y in zip(after, first):
        assert _same(x, y)


def test_graph_epoch_after_set_schedule_equals_eager(env):  # noqa: F811
    nat, dev, ds, ref, tr = env
    starts2, sizes2 = [896, 128, 1017], [128, 40, 7]
    t1 = _fresh(ds, dev, ref)
    t1.set_schedule(STARTS, SIZES)
    t1.train_epoch()
    torch.cuda.synchronize()
    _reset(t1, ref, 9)
    t1.set_schedule(starts2, sizes2)
    graph = _graph_epoch(t1)
    t2 = _fresh(ds, dev, ref)
    _reset(t2, ref, 9)
    eager = _eager_epoch(t2, starts2, sizes2)
    assert int(eager[2][2]) == sum(sizes2)
    for x, y in zip(graph, eager):
        assert _same(x, y)


# ---- 5. the step is the recorded step ---------------------------------------------------------------------
def test_step_hashes_match_parent_record(gpu_device):
    """Recomputes tools/record_lenet_steps.py's figures and compares them with the committed record.  The record
    is re-made only by a change that is meant to alter the step's arithmetic."""
    spec = importlib.util.spec_from_file_location("record_lenet_steps", ROOT / "tools" / "record_lenet_steps.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = json.loads((ROOT / "tests" / "golden" / "lenet_steps_parent.json").read_text())
    got = mod.compute(gpu_device)
    assert got["dataset"] == want["dataset"] and got["init"] == want["init"], "the record's inputs are not reproduced"
    assert len(want["eager"]) == 12 and len(want["graph"]) == 2
    for kind in ("eager", "graph"):
        for i, (g, w) in enumerate(zip(got[kind], want[kind])):
            assert g == w, (kind, i)
    assert got == want


# ---- engine argument checks -------------------------------------------------------------------------------
def test_engine_rejects_batches_out_of_range(env):  # noqa: F811
    nat, dev, ds, ref, tr = env
    n = len(tr.train_set)
    for start, nb in [(0, 0), (0, 129), (-1, 4), (n - 3, 4), (n, 1)]:
        with pytest.raises(ValueError):
            tr.train_step(start, nb)
        with pytest.raises(ValueError):
            tr.engine.set_schedule([0, start], [128, nb])
    torch.cuda.synchronize()
