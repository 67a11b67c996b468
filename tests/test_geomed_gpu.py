"""The geometric-median HIP kernels (csrc/kernels/geomed.hip) against the fp64 reference and the bounds of
tests/geomed_check.py: one pass, the zero-weight select, the chained call link by link, and GeoMedAgg end to end."""
import numpy as np
import pytest
import torch

from fedmi import native
from fedmi.parallel.robust import make_robust
from tests import geomed_check as gc
from tests.test_geomed import NU, drill_errors, drill_rows
from tests.test_robust_gpu import _FakeFedAvg, _GpuStub

pytestmark = pytest.mark.gpu

CANARY = -12345.0
BIG_N = 256 * 4 * 2048 + 7                   # past the grid cap: every lane strides, and a tail


@pytest.fixture(scope="module")
def nat(gpu_device):
    return native.require()


def _run(nat, dev, rows_np, weights=None, first=True, iters=0):
    """One ``geomed_pass`` (``iters`` 0) or the chained ``geomed`` on ``rows_np`` ([W, n]).  Every row is followed by
    4 to 7 NaNs (ld > n: a read past a row's end poisons its sumsq) and out lies between canaries.  Returns
    ``(z[n], history)`` as numpy: ``[3, 16]`` of the pass, ``[iters + 1, 3, 16]`` of the chain."""
    W, n = rows_np.shape
    ld = ((n + 3) & ~3) + 4
    rows = torch.full((W, ld), float("nan"), dtype=torch.float32, device=dev)
    rows[:, :n].copy_(torch.from_numpy(np.array(rows_np, dtype=np.float32)))
    buf = torch.full((n + 8,), CANARY, dtype=torch.float32, device=dev)
    out = buf[4:4 + n]
    partial = torch.zeros((nat.geomed_partials(n), 16), dtype=torch.float64, device=dev)
    hist = torch.full((iters + 1, 3, 16), CANARY, dtype=torch.float64, device=dev)
    s = native.stream_handle()
    if iters:
        nat.geomed(s, rows.data_ptr(), ld, W, n, iters, NU, out.data_ptr(), partial.data_ptr(), hist.data_ptr())
    else:
        w = torch.from_numpy(np.asarray(weights, dtype=np.float32)).to(dev) if not first else None
        nat.geomed_pass(s, rows.data_ptr(), ld, W, n, first, 0 if first else w.data_ptr(), out.data_ptr(),
                        partial.data_ptr(), hist.data_ptr(), nu=NU)
    torch.cuda.synchronize()
    buf, hist = buf.cpu().numpy(), hist.cpu().numpy()
    assert (buf[:4] == CANARY).all() and (buf[4 + n:] == CANARY).all(), "out was written outside [0, n)"
    assert (hist[:, :, W:] == CANARY).all(), "a history row was written past W"
    return buf[4:4 + n].copy(), hist if iters else hist[0]


@pytest.mark.parametrize("W", range(2, 17))
def test_one_pass_within_the_bounds(nat, gpu_device, W):
    for n in (1, 3, 4, 5, 1027) + ((BIG_N,) if W in (2, 16) else ()):
        rows = gc.inputs(W, n)
        for w in (None, gc.weights(W)):
            z, hist = _run(nat, gpu_device, rows, w, first=w is None)
            gc.check_pass(rows, w, z, hist, NU, f"W={W} n={n} first={w is None}")


@pytest.mark.parametrize("W", [2, 5, 16])
def test_sumsq_is_added_in_the_documented_order(nat, gpu_device, W):
    """The history's sumsq column equals, bit for bit, the kernel's own squared differences added in the order
    geomed.hip documents (tests/geomed_check.py emulates it; tests/test_geomed.py shows that a reordered sum differs
    on these inputs).  n = 5: one lane and a tail; 1027: one workgroup, a partly filled last wave, tail 3; 3077: four
    workgroups, the last with a single vector, tail 1; BIG_N: every lane strides."""
    for n in (5, 1027, 3077) + ((BIG_N,) if W in (2, 16) else ()):
        rows = gc.inputs_mixed(W, n)
        for w in (None, gc.weights(W)):
            z, hist = _run(nat, gpu_device, rows, w, first=w is None)
            want = gc.sumsq_in_kernel_order(rows, z)
            print(f"W={W} n={n} first={w is None}: sumsq {hist[0][:W].tolist()} emulated {want.tolist()}")
            assert hist[0][:W].tobytes() == want.tobytes(), f"W={W} n={n} first={w is None}"
            gc.check_pass(rows, w, z, hist, NU, f"W={W} n={n} first={w is None} (mixed magnitudes)")


@pytest.mark.parametrize("W,bad", [(3, 0), (5, 4), (16, 7)])
@pytest.mark.parametrize("poison", ["nan-row", "one-inf"])
def test_a_non_finite_row_gets_weight_zero_and_stays_out(nat, gpu_device, W, bad, poison):
    rows = gc.inputs(W, 1027)
    if poison == "nan-row":
        rows[bad] = np.nan
    else:
        rows[bad, 5] = np.inf
    z0, hist = _run(nat, gpu_device, rows)
    w = hist[2][:W].astype(np.float32)
    assert w[bad] == 0.0 and (w[np.arange(W) != bad] > 0).all() and np.isfinite(z0).all()
    rest = np.delete(rows, bad, axis=0)
    if poison == "nan-row":                              # pass 0 skips every entry of the row: the others' mean
        assert z0.tobytes() == _run(nat, gpu_device, rest)[0].tobytes()
    z1, _ = _run(nat, gpu_device, rows, w, first=False)
    z1_rest, _ = _run(nat, gpu_device, rest, np.delete(w, bad), first=False)
    assert np.isfinite(z1).all() and z1.tobytes() == z1_rest.tobytes()
    gc.check_pass(rest, np.delete(w, bad), z1, np.delete(_run(nat, gpu_device, rows, w, first=False)[1], bad, axis=1),
                  NU, f"W={W} {poison}")


def test_all_rows_nan(nat, gpu_device):
    z, hist = _run(nat, gpu_device, np.full((4, 1027), np.nan, dtype=np.float32))
    assert np.isnan(z).all() and hist[2][:4].tolist() == [0.25] * 4
    z, _ = _run(nat, gpu_device, np.full((4, 1027), np.nan, dtype=np.float32), [0.25] * 4, first=False)
    assert np.isnan(z).all()


@pytest.mark.parametrize("W", [2, 5, 16])
@pytest.mark.parametrize("T", [1, 6])
def test_chain_link_by_link(nat, gpu_device, W, T):
    """The chained call equals, bit for bit, its passes replayed one by one from its own history's weights, and
    every replayed pass meets the reference's bounds: no tolerance has to absorb the iteration's sensitivity."""
    rows = gc.inputs(W, 1027)
    z, hist = _run(nat, gpu_device, rows, iters=T)
    again = _run(nat, gpu_device, rows, iters=T)
    assert z.tobytes() == again[0].tobytes() and hist.tobytes() == again[1].tobytes()
    for t in range(T + 1):
        w = hist[t - 1][2][:W].astype(np.float32) if t else None
        z_t, row = _run(nat, gpu_device, rows, w, first=t == 0)
        gc.check_pass(rows, w, z_t, row, NU, f"W={W} T={T} pass {t}")
        assert row.tobytes() == hist[t].tobytes(), t
    assert z_t.tobytes() == z.tobytes()


def test_aggregate_stats_and_drill(nat, gpu_device, monkeypatch):
    """GeoMedAgg.aggregate (the gather replaced by a copy of the clients' known states) equals the direct native call
    bit for bit, its lagged round_stats are the history's, and the drill's thresholds hold on the GPU."""
    from fedmi.parallel.robust import GatheredAgg

    rows6 = drill_rows()
    rows = rows6[:5].copy()

    def fake_all_gather(views, x, group, abort):
        for r, v in enumerate(views):
            v.copy_(torch.from_numpy(rows[r].copy()))

    monkeypatch.setattr(GatheredAgg, "_all_gather", staticmethod(fake_all_gather))
    t = _GpuStub(torch.from_numpy(rows[1].copy()).to(gpu_device))
    agg = make_robust("geomed", t, iters=6)
    agg.aggregate(t, _FakeFedAvg(5))
    torch.cuda.synchronize()
    z, hist = _run(nat, gpu_device, rows, iters=6)
    assert t.flat.cpu().numpy().tobytes() == z.tobytes() and tuple(agg._rows.shape) == (5, 1028)
    assert agg.round_stats() == {"robust_kind": "geomed", "robust_iters": 6, "robust_weight": hist[5][2][:5].tolist(),
                                 "robust_dist": hist[6][1][:5].tolist()}
    got, plain = drill_errors(rows6, z)
    print(f"drill on the GPU: geomed {got:.4f}, plain mean {plain:.4f}, weights {hist[5][2][:5].tolist()}")
    assert got < 0.1 and plain > 1.0


def test_binding_rejects_bad_arguments(nat, gpu_device):
    rows = torch.zeros(4 * 16, device=gpu_device)
    out = torch.full((16,), CANARY, device=gpu_device)
    d = torch.zeros(512, dtype=torch.float64, device=gpu_device)
    p, o, q, s = rows.data_ptr(), out.data_ptr(), d.data_ptr(), native.stream_handle()
    good = dict(rows=p, ld=16, W=4, n=13, iters=2, nu=NU, out=o, partial=q, history=q + 1024)
    for bad in (dict(W=1), dict(W=17), dict(n=-1), dict(ld=12), dict(ld=15), dict(iters=0), dict(iters=65), dict(nu=0.0),
                dict(nu=-1.0), dict(rows=0), dict(out=0), dict(partial=0), dict(history=0), dict(rows=p + 4),
                dict(out=o + 8), dict(partial=q + 4), dict(history=q + 4), dict(out=p + 64), dict(out=p + 3 * 64 + 32)):
        with pytest.raises(ValueError):
            nat.geomed(s, **{**good, **bad})
    with pytest.raises(ValueError):
        nat.geomed_pass(s, p, 16, 4, 13, False, 0, o, q, q + 1024)      # a weighted pass without weights
    nat.geomed(s, **{**good, "n": 0})                                    # nothing to do
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and not d.any()
    nat.geomed(s, **good)
    torch.cuda.synchronize()
    assert not out[:13].any() and bool((out[13:] == CANARY).all()) and d[128 + 32:128 + 36].tolist() == [0.25] * 4
