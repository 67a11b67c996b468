"""The Krum HIP kernels (csrc/kernels/krum.hip) against the fp64 reference and the bounds of tests/krum_check.py: the
MFMA Gram pass, the finish and the selected rows' mean bit for bit, non-finite clients, and KrumAgg end to end."""
import numpy as np
import pytest
import torch

from fedmi import native
from fedmi.parallel.robust import GatheredAgg, make_robust
from tests import krum_check as kc
from tests.test_robust_gpu import _FakeFedAvg, _GpuStub

pytestmark = pytest.mark.gpu

CANARY = -12345.0
BIG_N = 2 * 1024 * 1024 + 7                  # past the grid cap (1024 workgroups of 1024 columns): every wave strides


@pytest.fixture(scope="module")
def nat(gpu_device):
    return native.require()


def _run(nat, dev, rows_np, byz=None, multi=False):
    """``byz`` None: ``krum_gram``, returns G[16, 16]; else the whole ``krum``, returns ``(z[n], stats[18, 16])``.
    Every row is followed by 4 to 7 NaNs (ld > n: an entry read past n poisons the Gram); out lies between canaries."""
    W, n = rows_np.shape
    ld = ((n + 3) & ~3) + 4
    rows = torch.full((W, ld), float("nan"), dtype=torch.float32, device=dev)
    rows[:, :n].copy_(torch.from_numpy(np.array(rows_np, dtype=np.float32)))
    partial = torch.zeros((nat.krum_partials(n), 256), dtype=torch.float64, device=dev)
    buf = torch.full((n + 8,), CANARY, dtype=torch.float32, device=dev)
    res = torch.full((18, 16), CANARY, dtype=torch.float64, device=dev)
    if byz is None:
        nat.krum_gram(native.stream_handle(), rows.data_ptr(), ld, W, n, partial.data_ptr(), res.data_ptr())
    else:
        nat.krum(native.stream_handle(), rows.data_ptr(), ld, W, n, byz, multi, buf[4:4 + n].data_ptr(),
                 partial.data_ptr(), res.data_ptr())
    torch.cuda.synchronize()
    buf, res = buf.cpu().numpy(), res.cpu().numpy()
    assert (buf[:4] == CANARY).all() and (buf[4 + n:] == CANARY).all(), "out was written outside [0, n)"
    return res[:16] if byz is None else (buf[4:4 + n].copy(), res)


@pytest.mark.parametrize("W", [2, 3, 4, 5, 8, 9, 16])
def test_gram_within_the_bound_symmetric_and_repeatable(nat, gpu_device, W):
    """Every tile size P = 4, 8, 16, full and partly filled; rows of distinct scale, so a transposed or permuted tile
    layout misses the bound by orders of magnitude."""
    for n in (1, 3, 4, 63, 257, 1027) + ((BIG_N,) if W == 3 else ()):
        rows = kc.inputs(W, n)
        G = _run(nat, gpu_device, rows)
        err, bound = np.abs(G[:W, :W] - kc.gram(rows)), kc.gram_bound(rows)
        print(f"W={W} n={n}: worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (W, n, G[:W, :W])
        assert np.array_equal(G, G.T) and not G[W:].any() and not G[:, W:].any()
        assert _run(nat, gpu_device, rows).tobytes() == G.tobytes()          # the same bits every run


@pytest.mark.parametrize("W", [2, 5, 8, 16])
@pytest.mark.parametrize("byz", [1, 3])
@pytest.mark.parametrize("multi", [False, True])
def test_finish_and_select_bit_for_bit(nat, gpu_device, W, byz, multi):
    """stats and out equal the reference applied to the kernel's own G, bit for bit; n = 3 is a tail alone.  On the
    reference alone the m-th and the (m + 1)-th score lie further apart than twice the distances' error bound, so the
    selection is well defined -- except krum at W = 2, where both scores ARE the one number d[0][1] (no gap can be
    asked for) and the rule's tie-break keeps rank 0."""
    f, k, m = kc.counts(W, byz, multi)
    for n in (3, 1027):
        rows = kc.inputs(W, n, attackers=f)
        ref, ref_selected = kc.finish(kc.gram(rows), W, byz, multi)
        by_score = sorted(ref[0, :W])
        gap = by_score[m] - by_score[m - 1] if m < W else np.inf
        print(f"W={W} byz={byz} multi={multi} n={n}: score gap {gap:.3e}, 2 x bound {2 * kc.dist_bound(rows):.3e}")
        assert gap > 2 * kc.dist_bound(rows) or (W == 2 and m == 1)
        z, stats = _run(nat, gpu_device, rows, byz, multi)
        want, selected = kc.finish(_run(nat, gpu_device, rows)[:W, :W], W, byz, multi)
        assert stats.tobytes() == want.tobytes() and selected == (ref_selected if W > 2 else [0, 1][:m])
        assert z.tobytes() == kc.select(rows, selected).tobytes()
        assert m > 1 or z.tobytes() == rows[selected[0]].tobytes()


@pytest.mark.parametrize("W,bad", [(3, 0), (5, 4), (16, 7)])
@pytest.mark.parametrize("poison", ["nan-row", "one-inf"])
def test_a_non_finite_client_is_at_infinite_distance_and_stays_out(nat, gpu_device, W, bad, poison):
    rows = kc.inputs(W, 1027)
    rows[bad, slice(None) if poison == "nan-row" else 5] = np.nan if poison == "nan-row" else np.inf
    rest = np.arange(W) != bad
    for multi in (False, True) if kc.counts(W, 1, True)[0] else (False,):     # (at W = 3 multikrum keeps everyone)
        z, stats = _run(nat, gpu_device, rows, 1, multi)
        d = stats[2:2 + W, :W]
        assert np.isinf(d[bad, rest]).all() and np.isinf(d[rest, bad]).all() and stats[1, bad] == 0.0
        assert np.isfinite(z).all() and stats[1, :W].sum() == kc.counts(W, 1, multi)[2]
    x = rows[rest].astype(np.float64)
    want = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    # the kernel's 4 gamma_n max G and the reference's, and three roundings of a value <= 4 max G each
    tol = 2 * kc.dist_bound(rows[rest]) + 24 * kc.U64 * float((x * x).sum(1).max())
    assert np.isfinite(d[rest][:, rest]).all() and (np.abs(d[rest][:, rest] - want) <= tol).all()
    z, stats = _run(nat, gpu_device, np.full((4, 1027), np.nan, dtype=np.float32), 1, True)    # every row NaN
    assert np.isnan(z).all() and np.isinf(stats[0, :4]).all() and stats[1].tolist() == [1.0] * 4 + [0.0] * 12


def test_aggregate_stats_and_bindings(nat, gpu_device, monkeypatch):
    """KrumAgg.aggregate (the gather replaced by a copy of the clients' known states) equals the direct native call
    bit for bit and its lagged round_stats are the stats'; then the bindings' argument checks."""
    rows = kc.inputs(5, 1027, attackers=1)
    monkeypatch.setattr(GatheredAgg, "_all_gather", staticmethod(
        lambda views, x, group, abort: [v.copy_(torch.from_numpy(rows[r].copy())) for r, v in enumerate(views)]))
    t = _GpuStub(torch.from_numpy(rows[1].copy()).to(gpu_device))
    agg = make_robust("multikrum", t, byz=1)
    agg.aggregate(t, _FakeFedAvg(5))
    torch.cuda.synchronize()
    z, stats = _run(nat, gpu_device, rows, 1, True)
    assert t.flat.cpu().numpy().tobytes() == z.tobytes() and tuple(agg._rows.shape) == (5, 1028)
    assert agg.round_stats() == {"robust_kind": "multikrum", "robust_byz": 1, "robust_selected": [0, 1, 2, 3],
                                 "robust_score": stats[0, :5].tolist()}
    out = torch.full((16,), CANARY, device=gpu_device)
    d = torch.zeros(1024, dtype=torch.float64, device=gpu_device)
    zeros = torch.zeros(4 * 16, device=gpu_device)
    p, o, q, s = zeros.data_ptr(), out.data_ptr(), d.data_ptr(), native.stream_handle()
    good = dict(rows=p, ld=16, W=4, n=13, byz=1, multi=True, out=o, partial=q, stats=q + 8 * 512)
    for bad in (dict(W=1), dict(W=17), dict(n=-1), dict(ld=12), dict(ld=15), dict(byz=-1), dict(rows=0), dict(out=0),
                dict(partial=0), dict(stats=0), dict(rows=p + 4), dict(out=o + 8), dict(partial=q + 4),
                dict(stats=q + 4), dict(out=p + 64), dict(out=p + 3 * 64 + 32)):
        with pytest.raises(ValueError):
            nat.krum(s, **{**good, **bad})
    with pytest.raises(ValueError):
        nat.krum_gram(s, p, 16, 17, 13, q, q + 8 * 512)
    nat.krum(s, **{**good, "n": 0})                                      # nothing to do
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and not d.any() and nat.krum_partials(13) == 2 and nat.krum_partials(0) == 0
    nat.krum(s, **good)                                                  # four zero rows: F_eff = 0, all four kept
    torch.cuda.synchronize()
    assert not out[:13].any() and bool((out[13:] == CANARY).all()) and d[512 + 16:512 + 21].tolist() == [1, 1, 1, 1, 0]
