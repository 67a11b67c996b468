"""The Bulyan HIP kernels (csrc/kernels/bulyan.hip) against the reference of tests/bulyan_check.py, bit for bit: the
iterated selection from the kernel's own Gram, the fold of any record, the whole rule with non-finite clients, and
BulyanAgg end to end."""
import numpy as np
import pytest
import torch

from fedmi import native
from fedmi.parallel.robust import GatheredAgg, make_robust
from tests import bulyan_check as bc
from tests import krum_check as kc
from tests.robust_check import same_bits
from tests.test_robust_gpu import _FakeFedAvg, _GpuStub

pytestmark = pytest.mark.gpu

CANARY = -12345.0
BIG_N = 2 * 1024 * 1024 + 7                  # past the fold's grid cap (2048 x 256 lanes x 4): every lane strides


@pytest.fixture(scope="module")
def nat(gpu_device):
    return native.require()


def _run(nat, dev, rows_np, byz=None, record=None, c=0):
    """``record`` given: ``bulyan_fold``; ``byz`` given: the whole ``bulyan``; neither: ``krum_gram``, returns G.
    Every row is followed by 4 to 7 NaNs; out lies between canaries.  Returns ``(z[n], stats[19, 16], record)``."""
    W, n = rows_np.shape
    ld = ((n + 3) & ~3) + 4
    rows = torch.full((W, ld), float("nan"), dtype=torch.float32, device=dev)
    rows[:, :n].copy_(torch.from_numpy(np.array(rows_np, dtype=np.float32)))
    partial = torch.zeros((nat.bulyan_partials(n), 256), dtype=torch.float64, device=dev)
    buf = torch.full((n + 8,), CANARY, dtype=torch.float32, device=dev)
    res = torch.full((19, 16), CANARY, dtype=torch.float64, device=dev)
    args = (native.stream_handle(), rows.data_ptr(), ld, W, n)
    if record is not None:
        nat.bulyan_fold(*args, list(record), c, buf[4:4 + n].data_ptr(), partial.data_ptr(), res.data_ptr())
    elif byz is not None:
        nat.bulyan(*args, byz, buf[4:4 + n].data_ptr(), partial.data_ptr(), res.data_ptr())
    else:
        nat.krum_gram(*args, partial.data_ptr(), res.data_ptr())
    torch.cuda.synchronize()
    buf, res = buf.cpu().numpy(), res.cpu().numpy()
    assert (buf[:4] == CANARY).all() and (buf[4 + n:] == CANARY).all(), "out was written outside [0, n)"
    if record is None and byz is None:
        return res[:16]
    rec = partial[nat.krum_partials(n) - 1].cpu().view(torch.int32)[:17].tolist()
    return buf[4:4 + n].copy(), res, rec[1:1 + rec[0]]


@pytest.mark.parametrize("W,F", [(2, 1), (5, 1), (7, 1), (10, 1), (11, 2), (15, 3), (16, 3), (16, 1)])
@pytest.mark.parametrize("n", [3, 1027])
def test_selection_bit_for_bit(nat, gpu_device, W, F, n):
    """Stats rows 0 .. 17 and the record equal the reference applied to the kernel's own G; the selected set is the
    fp64 numpy Gram's.  On the reference alone: in every round the picked score and the next greater one lie further
    apart than 2 k times the distances' error bound, and equal scores occur only at k = 1 (the mutually nearest pair)."""
    f, theta, _, _ = bc.counts(W, F)
    rows = bc.inputs(W, n, attackers=f)
    _, ref_selected, rounds = bc.select(bc.gram(rows), W, F)
    for k, scores in rounds:
        above = [s for s in scores if s > scores[0]]
        gap = above[0] - scores[0] if above else np.inf
        assert gap > 2 * k * bc.dist_bound(rows) and (k == 1 or len(set(scores)) == len(scores))
    assert not set(ref_selected) & set(range(W - f, W))
    _, stats, record = _run(nat, gpu_device, rows, F)
    want, selected, _ = bc.select(_run(nat, gpu_device, rows)[:W, :W], W, F)
    assert stats[:18].tobytes() == want[:18].tobytes() and record == selected == ref_selected and len(record) == theta


@pytest.mark.parametrize("W", [9, 16])
@pytest.mark.parametrize("F", [1, 3])
def test_selection_when_every_score_ties(nat, gpu_device, W, F):
    """All W rows are one row: every distance and so every score is the same number, and the rank alone decides --
    several picks in ONE round (krum, multikrum) and one pick in each of many rounds (bulyan).  Stats rows 0 .. 17 and
    the record equal the references applied to the kernel's own G; the picked are the lowest ranks; Bulyan's round
    numbers count up in rank order."""
    n = 5
    rows = torch.randn(n, generator=torch.Generator().manual_seed(W)).repeat(W, 1).numpy()
    G = _run(nat, gpu_device, rows)[:W, :W]
    padded = torch.zeros((W, 8), dtype=torch.float32, device=gpu_device)
    padded[:, :n].copy_(torch.from_numpy(rows))
    for multi in (False, True):
        partial = torch.zeros((nat.krum_partials(n), 256), dtype=torch.float64, device=gpu_device)
        out = torch.empty(8, dtype=torch.float32, device=gpu_device)
        res = torch.full((18, 16), CANARY, dtype=torch.float64, device=gpu_device)
        nat.krum(native.stream_handle(), padded.data_ptr(), 8, W, n, F, multi, out.data_ptr(), partial.data_ptr(),
                 res.data_ptr())
        torch.cuda.synchronize()
        rec = partial[-1].cpu().view(torch.int32)[:17].tolist()
        want, selected = kc.finish(G, W, F, multi)
        assert res.cpu().numpy().tobytes() == want.tobytes()
        assert rec[1:1 + rec[0]] == selected == list(range(kc.counts(W, F, multi)[2]))
        assert out[:n].cpu().numpy().tobytes() == kc.select(rows, selected).tobytes()
    theta = bc.counts(W, F)[1]
    _, stats, record = _run(nat, gpu_device, rows, F)
    want, selected, _ = bc.select(G, W, F)
    assert stats[:18].tobytes() == want[:18].tobytes() and record == selected == list(range(theta))
    assert stats[1].tolist() == [float(r + 1) for r in range(theta)] + [0.0] * (16 - theta)


@pytest.mark.parametrize("theta", [2, 3, 5, 8, 9, 14, 16])
def test_fold_bit_for_bit(nat, gpu_device, theta):
    """Any non-contiguous record out of 16 rows, every c that leaves a value, whole vectors and tails; the edge columns
    of bulyan_check.fold_inputs (NaNs up to c + 1, infinities, a median of -inf, signed zeros, ties, one-sided drops)."""
    record = sorted(np.random.default_rng(theta).permutation(16)[:theta].tolist())
    for c in [c for c in (0, 2, 4, 6) if theta - c >= 1]:
        for n in (1, 3, 4, 1027) + ((BIG_N,) if (theta, c) == (5, 2) else ()):
            rows = bc.fold_inputs(n, record, c)
            want, want_cut = bc.fold(rows, record, c)
            z, stats, rec = _run(nat, gpu_device, rows, record=record, c=c)
            assert same_bits(z, want) == "", (theta, c, n)
            assert stats[18].tolist() == want_cut.tolist() and rec == record and (stats[:18] == CANARY).all()


@pytest.mark.parametrize("W,F", [(7, 1), (11, 2), (16, 3)])
def test_whole_rule_and_non_finite_clients(nat, gpu_device, W, F):
    rows = bc.inputs(W, 1027, attackers=bc.counts(W, F)[0])
    z, stats, record = _run(nat, gpu_device, rows, F)
    want, want_stats, selected = bc.reference(rows, _run(nat, gpu_device, rows)[:W, :W], F)
    assert z.tobytes() == want.tobytes() and stats.tobytes() == want_stats.tobytes() and record == selected
    again = _run(nat, gpu_device, rows, F)
    assert again[0].tobytes() == z.tobytes() and again[1].tobytes() == stats.tobytes()       # the same bits every run
    rest = np.arange(W) != 3
    for where, poison in ((slice(None), np.nan), (5, np.inf)):           # a row all NaN; a client with one inf
        bad = bc.inputs(W, 1027, attackers=0)
        bad[3, where] = poison
        z, stats, record = _run(nat, gpu_device, bad, F)
        d = stats[2:2 + W, :W]
        assert np.isinf(d[3, rest]).all() and np.isinf(d[rest, 3]).all() and np.isfinite(z).all()
        assert 3 not in record and stats[1, 3] == 0 and stats[18, 3] == 0
        assert z.tobytes() == bc.reference(bad, _run(nat, gpu_device, bad)[:W, :W], F)[0].tobytes()


def test_aggregate_stats_and_bindings(nat, gpu_device, monkeypatch):
    """BulyanAgg.aggregate (the gather replaced by a copy of the clients' known states) equals the direct native call
    bit for bit and its lagged round_stats are the stats'; then the bindings' argument checks."""
    rows = bc.inputs(7, 1027, attackers=1)
    monkeypatch.setattr(GatheredAgg, "_all_gather", staticmethod(
        lambda views, x, group, abort: [v.copy_(torch.from_numpy(rows[r].copy())) for r, v in enumerate(views)]))
    t = _GpuStub(torch.from_numpy(rows[1].copy()).to(gpu_device))
    agg = make_robust("bulyan", t, byz=1)
    agg.aggregate(t, _FakeFedAvg(7))
    torch.cuda.synchronize()
    z, stats, record = _run(nat, gpu_device, rows, 1)
    assert t.flat.cpu().numpy().tobytes() == z.tobytes() and tuple(agg._rows.shape) == (7, 1028)
    assert agg.round_stats() == {"robust_kind": "bulyan", "robust_byz": 1, "robust_selected": record,
                                 "robust_score": stats[0, :7].tolist(), "robust_cut": stats[18, :7].astype(int).tolist()}
    out = torch.full((16,), CANARY, device=gpu_device)
    d = torch.zeros(2048, dtype=torch.float64, device=gpu_device)
    zeros = torch.zeros(4 * 16, device=gpu_device)
    p, o, q, s = zeros.data_ptr(), out.data_ptr(), d.data_ptr(), native.stream_handle()
    good = dict(rows=p, ld=16, W=4, n=13, byz=1, out=o, partial=q, stats=q + 8 * 3 * 256)
    common = (dict(W=1), dict(W=17), dict(n=-1), dict(ld=12), dict(ld=15), dict(rows=0), dict(out=0), dict(partial=0),
              dict(stats=0), dict(rows=p + 4), dict(out=o + 8), dict(partial=q + 4), dict(stats=q + 4),
              dict(out=p + 64), dict(out=p + 3 * 64 + 32))
    fold = {k: v for k, v in good.items() if k != "byz"}
    fold.update(record=[0, 2, 3], c=2)
    for bad in common + (dict(byz=-1),):
        with pytest.raises(ValueError):
            nat.bulyan(s, **{**good, **bad})
    for bad in common + (dict(c=1), dict(c=4), dict(c=-2), dict(record=[0]), dict(record=[0, 4]), dict(record=[2, 1]),
                         dict(record=[1, 1]), dict(record=[-1, 1]), dict(record=[0, 1, 2, 3, 3])):
        with pytest.raises(ValueError):
            nat.bulyan_fold(s, **{**fold, **bad})
    nat.bulyan(s, **{**good, "n": 0})                                    # nothing to do
    nat.bulyan_fold(s, **{**fold, "n": 0})
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and not d.any() and nat.bulyan_partials(13) == 3 and nat.bulyan_partials(0) == 0
    nat.bulyan(s, **good)                                                # four zero rows: F_eff = 0, all four picked
    torch.cuda.synchronize()
    assert not out[:13].any() and bool((out[13:] == CANARY).all())
    assert d[768 + 16:768 + 21].tolist() == [1, 2, 3, 4, 0] and not d[768 + 288:].any()
