"""The DnC HIP kernels (csrc/kernels/dnc.hip) against the fp64 reference and the bounds of tests/dnc_check.py: the
centred MFMA Gram pass, the finish and the kept rows' mean bit for bit, non-finite clients, and DncAgg end to end."""
import numpy as np
import pytest
import torch

from fedmi import native
from fedmi.parallel.robust import GatheredAgg, make_robust
from tests import dnc_check as dc
from tests import krum_check as kc
from tests.test_robust_gpu import _FakeFedAvg, _GpuStub

pytestmark = pytest.mark.gpu

CANARY = -12345.0
BIG_N = 2 * 1024 * 1024 + 7                  # past the grid cap (1024 workgroups of 1024 columns): every wave strides


@pytest.fixture(scope="module")
def nat(gpu_device):
    return native.require()


def _run(nat, dev, rows_np, byz=None):
    """``byz`` None: ``dnc_gram``, G[16, 16]; else ``dnc``, ``(z[n], stats[18, 16])``.  Every row is followed by 4 to 7
    NaNs (ld > n: an entry read past n poisons the pivot or the Gram); out lies between canaries."""
    W, n = rows_np.shape
    ld = ((n + 3) & ~3) + 4
    rows = torch.full((W, ld), float("nan"), dtype=torch.float32, device=dev)
    rows[:, :n].copy_(torch.from_numpy(np.array(rows_np, dtype=np.float32)))
    partial = torch.zeros((nat.dnc_partials(n), 256), dtype=torch.float64, device=dev)
    buf = torch.full((n + 8,), CANARY, dtype=torch.float32, device=dev)
    res = torch.full((18, 16), CANARY, dtype=torch.float64, device=dev)
    if byz is None:
        nat.dnc_gram(native.stream_handle(), rows.data_ptr(), ld, W, n, partial.data_ptr(), res.data_ptr())
    else:
        nat.dnc(native.stream_handle(), rows.data_ptr(), ld, W, n, byz, buf[4:4 + n].data_ptr(), partial.data_ptr(),
                res.data_ptr())
    torch.cuda.synchronize()
    buf, res = buf.cpu().numpy(), res.cpu().numpy()
    assert (buf[:4] == CANARY).all() and (buf[4 + n:] == CANARY).all(), "out was written outside [0, n)"
    return res[:16] if byz is None else (buf[4:4 + n].copy(), res)


@pytest.mark.parametrize("W", [2, 3, 4, 5, 8, 9, 16])
def test_centred_gram_within_the_bound_symmetric_and_repeatable(nat, gpu_device, W):
    """Every tile size P = 4, 8, 16, full and partly filled; a common part 1e4 times the differences, of distinct scale
    per client.  Double-centred as the reference is, the kernel's G meets the derived bound of the exact centred Gram."""
    for n in (1, 3, 4, 63, 257, 1027) + ((BIG_N,) if W == 3 else ()):
        rows = dc.inputs(W, n)
        G = _run(nat, gpu_device, rows)
        C, bound = dc.gram(rows), dc.gram_bound(rows)
        err = np.abs(dc.centre(G[:W, :W]) - C)
        size = np.abs(C).max()
        print(f"W={W} n={n}: worst error / bound {float((err / bound).max()):.3f}; bound / max|C|: centred "
              f"{float(bound.max() / size):.2e}, Krum's uncentred {float(kc.gram_bound(rows).max() / size):.2e}")
        assert (err <= bound).all(), (W, n, G[:W, :W])
        assert np.array_equal(G, G.T) and not G[W:].any() and not G[:, W:].any()
        assert _run(nat, gpu_device, rows).tobytes() == G.tobytes()          # the same bits every run


@pytest.mark.parametrize("W", [2, 5, 8, 16])
@pytest.mark.parametrize("byz", [1, 3])
def test_finish_and_select_bit_for_bit(nat, gpu_device, W, byz):
    """stats and out equal the reference applied to the kernel's own G, bit for bit; F_eff attackers are shifted along
    one direction.  On the reference alone the m-th and (m + 1)-th score lie further apart than twice the score error
    that the Gram's bound implies: the selection is well defined (W = 2, where nothing is removed, is exempt)."""
    f, m = dc.counts(W, byz)
    for n in (3, 1027):
        rows = dc.inputs(W, n, attackers=f)
        ref, ref_selected = dc.finish(dc.gram(rows), W, byz)
        by_score = sorted(ref[0, :W])
        gap = by_score[m] - by_score[m - 1] if m < W else np.inf
        print(f"W={W} byz={byz} n={n}: score gap {gap:.3e}, 2 x bound {2 * dc.score_bound(rows):.3e}")
        assert gap > 2 * dc.score_bound(rows) or W == 2
        z, stats = _run(nat, gpu_device, rows, byz)
        want, selected = dc.finish(_run(nat, gpu_device, rows)[:W, :W], W, byz)
        assert stats.tobytes() == want.tobytes() and selected == ref_selected == list(range(W - f))
        assert z.tobytes() == dc.select(rows, selected).tobytes()


@pytest.mark.parametrize("W,bad", [(3, 0), (5, 4), (16, 7)])
@pytest.mark.parametrize("poison", ["nan-row", "one-inf"])
def test_a_non_finite_client_scores_infinity_and_stays_out(nat, gpu_device, W, bad, poison):
    rows = dc.inputs(W, 1027)
    rows[bad, slice(None) if poison == "nan-row" else 5] = np.nan if poison == "nan-row" else np.inf
    rest = np.arange(W) != bad
    z, stats = _run(nat, gpu_device, rows, 1)
    C = stats[2:2 + W, :W]
    assert np.isposinf(stats[0, bad]) and stats[1, bad] == 0.0 and np.isfinite(stats[0, :W][rest]).all()
    assert np.isfinite(z).all() and stats[1].sum() == dc.counts(W, 1)[1] and not C[bad].any() and not C[:, bad].any()
    err, bound = np.abs(C[rest][:, rest] - dc.gram(rows[rest])), dc.gram_bound(rows, rest)
    print(f"W={W} {poison}: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("world,kept", [(2, 2), (4, 3)])
def test_every_row_nan_keeps_the_lowest_ranks_and_propagates(nat, gpu_device, world, kept):
    z, stats = _run(nat, gpu_device, np.full((world, 1027), np.nan, dtype=np.float32), 1)
    assert np.isnan(z).all() and np.isposinf(stats[0, :world]).all()
    assert stats[1].tolist() == [1.0] * kept + [0.0] * (16 - kept) and not stats[2:].any()


def test_aggregate_stats_and_bindings(nat, gpu_device, monkeypatch):
    """DncAgg.aggregate (the gather replaced by a copy of the clients' known states) equals the direct native call
    bit for bit and its lagged round_stats are the stats'; then the bindings refuse bad arguments as Krum's do."""
    rows = dc.inputs(5, 1027, attackers=1)
    monkeypatch.setattr(GatheredAgg, "_all_gather", staticmethod(
        lambda views, x, group, abort: [v.copy_(torch.from_numpy(rows[r].copy())) for r, v in enumerate(views)]))
    t = _GpuStub(torch.from_numpy(rows[1].copy()).to(gpu_device))
    agg = make_robust("dnc", t, byz=1)
    agg.aggregate(t, _FakeFedAvg(5))
    torch.cuda.synchronize()
    z, stats = _run(nat, gpu_device, rows, 1)
    assert t.flat.cpu().numpy().tobytes() == z.tobytes() and tuple(agg._rows.shape) == (5, 1028)
    assert agg.round_stats() == {"robust_kind": "dnc", "robust_byz": 1, "robust_selected": [0, 1, 2, 3],
                                 "robust_score": stats[0, :5].tolist()}
    out = torch.full((16,), CANARY, device=gpu_device)
    d = torch.zeros(1024, dtype=torch.float64, device=gpu_device)
    zeros = torch.zeros(4 * 16, device=gpu_device)
    p, o, q, s = zeros.data_ptr(), out.data_ptr(), d.data_ptr(), native.stream_handle()
    good = dict(rows=p, ld=16, W=4, n=13, byz=1, out=o, partial=q, stats=q + 8 * 512)
    for bad in (dict(W=17), dict(ld=15), dict(byz=-1), dict(partial=0), dict(out=p + 3 * 64 + 32)):   # Krum's rows_check
        with pytest.raises(ValueError):
            nat.dnc(s, **{**good, **bad})
    with pytest.raises(ValueError):
        nat.dnc_gram(s, p, 16, 17, 13, q, q + 8 * 512)
    nat.dnc(s, **{**good, "n": 0})                                       # nothing to do
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and not d.any()
    nat.dnc(s, **good)                                                   # four zero rows: tr C = 0, the 3 lowest ranks
    torch.cuda.synchronize()
    assert not out[:13].any() and bool((out[13:] == CANARY).all()) and d[512 + 16:512 + 21].tolist() == [1, 1, 1, 0, 0]
    assert nat.dnc_partials(13) == 2 and nat.dnc_partials(0) == 0
