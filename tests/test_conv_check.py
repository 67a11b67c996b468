"""The conv references of tests/conv_check.py, checked without a GPU.

* the six fp64 references against direct nested-loop numpy versions (padding, stride, flip and layout conventions);
* the bounds reject wrong kernels: on cases spanning forward, DGRAD, WGRAD and depthwise an honest fp32 evaluation
  (torch fp32 on the CPU, tests/emulate.py where it applies) has no element outside its interval, and every mutant of
  MUTANTS -- an error the old ``max|a-b| / max|b| < 1e-2`` rule let through, or a lost term -- has at least one;
* the labels of the case tables are what the planner does: tests/dispatch_recorder.hip, built host-only, run over
  every dense shape of the tables; and the tables together reach every kernel instantiation of
  tests/golden/conv_dispatch_cus256.txt.gz but the ones that need a workload-size problem.
"""
import gzip
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_check as cc
import emulate

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


# ---------------------------------------------------------------------------------------------------------------
# conventions
# ---------------------------------------------------------------------------------------------------------------
def _close(a, b, terms, n):
    """fp64 rounding only: both sides sum n terms in some order."""
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= 2.0 * n * 2.0 ** -53 * terms + 1e-300)


TINY = (2, 5, 4, 3, 4, 3, 2, 1)      # N H W C O R stride pad: odd height, stride 2 that does not divide, pad 1


@pytest.mark.parametrize("shape", [TINY, (1, 4, 5, 2, 3, 2, 1, 0), (1, 3, 3, 2, 2, 5, 2, 2)], ids=str)
def test_dense_references_agree_with_nested_loops(shape):
    N, H, W, C, O, R, st, pad = shape
    P, Q = cc.out_hw(H, W, R, st, pad)
    x, w, dy = cc.draw(("loop", "x"), (N, H, W, C)), cc.draw(("loop", "w"), (O, C, R, R)), cc.draw(("loop", "dy"), (N, P, Q, O))
    y, ya = cc.fwd_ref(x, w, st, pad)
    _close(y, cc.loop_fwd(x, w, st, pad), ya, R * R * C)
    _close(ya, cc.loop_fwd(np.abs(x), np.abs(w), st, pad), ya, R * R * C)
    dx, dxa = cc.dgrad_ref(dy, w, (N, H, W, C), st, pad)
    _close(dx, cc.loop_dgrad(dy, w, (N, H, W, C), st, pad), dxa, R * R * O)
    dw, dwa = cc.wgrad_ref(x, dy, R, st, pad)
    _close(dw, cc.loop_wgrad(x, dy, R, st, pad, C), dwa, N * P * Q)
    dw2, _ = cc.wgrad_ref(x, dy, R, st, pad, Cw=C - 1)                      # Cw < C: the leading channels
    _close(dw2, cc.loop_wgrad(x, dy, R, st, pad, C - 1), dwa[:, :C - 1], N * P * Q)


@pytest.mark.parametrize("shape", [(2, 5, 4, 8, 3, 2), (1, 4, 4, 8, 5, 1)], ids=str)
def test_depthwise_references_agree_with_nested_loops(shape):
    N, H, W, C, R, st = shape
    pad = R // 2
    P, Q = cc.out_hw(H, W, R, st, pad)
    x, dy = cc.draw(("dwloop", "x"), (N, H, W, C)), cc.draw(("dwloop", "dy"), (N, P, Q, C))
    w = cc.draw(("dwloop", "w"), (C, 1, R, R), bf16=False)
    y, ya = cc.dw_fwd_ref(x, w, st, pad)
    _close(y, cc.loop_dw_fwd(x, w, st, pad), ya, R * R)
    dx, dxa = cc.dw_dgrad_ref(dy, w, (N, H, W, C), st, pad)
    _close(dx, cc.loop_dw_dgrad(dy, w, (N, H, W, C), st, pad), dxa, R * R)
    dw, dwa = cc.dw_wgrad_ref(x, dy, R, st, pad)
    _close(dw, cc.loop_dw_wgrad(x, dy, R, st, pad), dwa, N * P * Q)


def test_grouped_read_and_tap_counts():
    full = np.arange(4 * 6 * 1 * 1, dtype=np.float64).reshape(4, 6, 1, 1)
    g = cc.wgrad_grouped(full, 2, 3)                                          # filters 0, 1: channels 0-2; 2, 3: 3-5
    assert g.shape == (4, 3, 1, 1) and g[1, 0, 0, 0] == full[1, 0, 0, 0] and g[2, 0, 0, 0] == full[2, 3, 0, 0]
    t = cc.dgrad_taps(3, 3, 1, 2, 0)[0, :, :, 0]                              # 1x1 stride 2: only even / even has a tap
    assert t.tolist() == [[1, 0, 1], [0, 0, 0], [1, 0, 1]]
    assert cc.dgrad_taps(4, 4, 3, 2, 1)[0, :2, :2, 0].tolist() == [[1, 2], [2, 4]]
    assert cc.dgrad_taps(2, 2, 3, 1, 1).max() == 9
    assert cc.split_k(16, 7) == (3, 6) and cc.split_k(2, 7) == (1, 2) and cc.split_k(13, 13) == (1, 13)


def test_tables_are_well_formed():
    keys = [r.key for t in (cc.FWD, cc.DGRAD, cc.WGRAD, cc.DW) for r in t]
    assert len(keys) == len(set(keys))
    for r in cc.FWD:
        N, H, W, C, O, R, st, pad = r.shape
        assert ("res" in r.variants) == (C % 64 == 0 and r.launches[0].startswith("conv_tap")), r.key
        assert (r.splits > 1) == (len(r.launches) == 2) == r.ws, r.key
        P, Q = cc.out_hw(H, W, R, st, pad)
        assert N * P * Q * R * R * C * O <= 1.2e8, r.key      # reference products per case (the largest: the GEN split)
    for r in cc.DGRAD + cc.WGRAD:
        N, H, W, C, O, R, st, pad = r.shape
        P, Q = cc.out_hw(H, W, R, st, pad)
        assert N * P * Q * R * R * C * O <= 1e8, r.key
    for r in cc.DGRAD:
        if r.variants != ("plain",):     # one path for every element: the variant's operand is modelled on it
            assert all(" splits=" not in lb or len(set(lb.split("splits=")[1].split(","))) == 1 for lb in r.launches), r.key
    for r in cc.DW:
        assert cc.dw_blocks(r.shape) == r.nblk, r.key
    assert max(r.nblk for r in cc.DW) > 64 and min(r.nblk for r in cc.DW) < 16
    assert all(k in keys for k in cc.WGRAD_DEFERRED + cc.DW_DEFERRED)


# ---------------------------------------------------------------------------------------------------------------
# the bounds reject wrong kernels
# ---------------------------------------------------------------------------------------------------------------
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


def _rne(a):
    """fp32 -> bf16, round to nearest even (torch's conversion), as fp32."""
    return _f32(a).bfloat16().float().numpy()


def _trunc(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _add32(a, b):
    return (np.asarray(a, np.float32) + np.asarray(b, np.float32)).astype(np.float32)


def _fwd32(x, w, st, pad, groups=1):
    Cw = w.shape[1] * groups
    y = F.conv2d(_f32(x[..., :Cw]).permute(0, 3, 1, 2), _f32(w), stride=st, padding=pad, groups=groups)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def _dgrad32(dy, w, xs, st, pad, groups=1):
    N, H, W, _ = xs
    dx = torch.nn.grad.conv2d_input((N, w.shape[1] * groups, H, W), _f32(w), _f32(dy).permute(0, 3, 1, 2), stride=st,
                                    padding=pad, groups=groups)
    return dx.permute(0, 2, 3, 1).contiguous().numpy()


def _wgrad32(x, dy, R, st, pad, groups=1):
    C, O = x.shape[3], dy.shape[3]
    return torch.nn.grad.conv2d_weight(_f32(x).permute(0, 3, 1, 2), (O, C // groups, R, R), _f32(dy).permute(0, 3, 1, 2),
                                       stride=st, padding=pad, groups=groups).numpy()


def _drop_k(w, C, first):
    """w [O,Cw,R,S] with the GEMM-K elements k = (r*S + s)*C + c >= first zeroed (the forward's K order)."""
    O, Cw, R, S = w.shape
    k = (np.arange(R * S)[:, None] * C + np.arange(Cw)[None, :]).reshape(R, S, Cw).transpose(2, 0, 1)
    return np.where(k[None] >= first, np.float32(0), w)


def _drop_ko(w, first):
    """w with the DGRAD's K elements k = (r*S + s)*O + o >= first zeroed."""
    O, Cw, R, S = w.shape
    k = (np.arange(R * S)[None, :] * O + np.arange(O)[:, None]).reshape(O, 1, R, S)
    return np.where(k >= first, np.float32(0), w)


def _drop_pixels(dy, first, last=None):
    d = dy.copy().reshape(-1, dy.shape[-1])
    d[first:last] = 0
    return d.reshape(dy.shape)


def _ksteps(k):
    return -(-k // 64)


def _split_first(row, ksteps, unit=64):
    """First K element of the last split of a row whose first launch is '... z=<splits> kps=<kps>'."""
    z, kps = (int(f.split("=")[1]) for f in row.launches[0].split()[-2:])
    assert z > 1 and (z - 1) * kps < ksteps
    return (z - 1) * kps * unit


MUT_FWD = ("f_tap_m105", "f_tapg_3x3", "f_split_2x9", "f_tap_5x5s2_split", "f_stem32")
MUT_DGRAD = ("d_tap", "d_ph_odd", "d_split2")
MUT_WGRAD = ("wg_64x128", "wg_s7_short", "wg_halo_8")
MUT_DW = ("dw_3s1_odd", "dw_5s2_c24")
MUTANTS = ("truncated to bf16", "one (tap, 8 channels) dropped at one output row", "last K step dropped",
           "one pixel dropped from a WGRAD sum", "last split dropped", "statistics of the unrounded accumulator",
           "residual added with the other path's rounding")
MATRIX = {}      # (case, mutant) -> elements outside (filled by the tests below; printed by the last one)


def _row(table, key):
    return next(r for r in table if r.key == key)


def _stats32(y, shift):
    """An honest fp32 statistics pass over the stored y: sequential fp32 sums of (y - shift) and its square."""
    v = (np.asarray(y, np.float32).reshape(-1, y.shape[-1]) - np.asarray(shift, np.float32)).astype(np.float32)
    return np.cumsum(v, 0, dtype=np.float32)[-1], np.cumsum(v * v, 0, dtype=np.float32)[-1]


def _stats64(y, shift):
    v = np.asarray(y, np.float64).reshape(-1, y.shape[-1]) - np.asarray(shift, np.float64)
    return v.sum(0), (v * v).sum(0)


def _judge(case, honest, mutants, iv, bf16_out):
    n, worst = cc.outside(honest, iv, bf16_out)
    assert n == 0, (case, "the honest fp32 evaluation is outside", n, worst)
    for name, y in mutants.items():
        n, _ = cc.outside(y, iv, bf16_out)
        MATRIX[(case, name)] = n
        assert n > 0, (case, name, "passes the interval check")


def _judge_stats(case, acc, shift):
    y = _rne(acc)
    iv1, iv2 = cc.stats_iv(y, shift)
    s1, s2 = _stats32(y, shift)
    assert cc.outside(s1, iv1)[0] == 0 and cc.outside(s2, iv2)[0] == 0, (case, "honest statistics outside")
    m1, m2 = _stats64(acc, shift)                                           # of the accumulator, not the stored value
    n = cc.outside(m1, iv1)[0] + cc.outside(m2, iv2)[0]
    MATRIX[(case, MUTANTS[5])] = n
    assert n > 0, (case, MUTANTS[5], "passes")


@pytest.mark.parametrize("key", MUT_FWD)
def test_forward_bounds_reject_mutants(key):
    r = _row(cc.FWD, key)
    N, H, W, C, O, R, st, pad = r.shape
    op = cc.dense_operands(r.key, r.shape, r.Cw)
    x, w = op["x"], op["w"]
    acc = _fwd32(x, w, st, pad)
    n0, p0, t0, c0 = N - 1, 1, R // 2, 8 * ((r.Cw - 1) // 8 // 2)            # an interior row, the centre tap
    cut = acc.copy()
    h = p0 * st - pad + t0
    for q in range(acc.shape[2]):
        ww = q * st - pad + t0
        if 0 <= ww < W:
            cut[n0, p0, q] -= w[:, c0:c0 + 8, t0, t0] @ x[n0, h, ww, c0:min(c0 + 8, r.Cw)]
    K = R * R * C
    mut = {MUTANTS[0]: _trunc(acc), MUTANTS[1]: _rne(cut),
           MUTANTS[2]: _rne(_fwd32(x, _drop_k(w, C, 64 * (_ksteps(K) - 1)), st, pad))}
    if r.splits > 1:
        mut[MUTANTS[4]] = _rne(_fwd32(x, _drop_k(w, C, _split_first(r, _ksteps(K))), st, pad))
    _judge(key, _rne(acc), mut, cc.fwd_interval(r), True)
    if key == "f_tap_m105":                                                  # the emulation is an honest evaluation too
        xt, wt = _f32(x).bfloat16(), torch.from_numpy(w)
        y = emulate.conv2d_fwd(xt, emulate.pack_weight(wt, C), st, pad, Cw=r.Cw)
        assert cc.outside(y.float().numpy(), cc.fwd_interval(r), True)[0] == 0
    _judge_stats(key, acc, op["shift"])
    if "res" in r.variants:
        one, two = _rne(_add32(acc, op["res"])), _rne(_add32(_rne(acc), op["res"]))
        assert not np.array_equal(one, two), "a case where the two roundings differ"
        honest, other = (one, two) if r.splits > 1 else (two, one)
        _judge(key + "+res", honest, {MUTANTS[6]: other}, cc.fwd_interval(r, res=True), True)


@pytest.mark.parametrize("key", MUT_DGRAD)
def test_dgrad_bounds_reject_mutants(key):
    r = _row(cc.DGRAD, key)
    N, H, W, C, O, R, st, pad = r.shape
    op = cc.dense_operands(r.key, r.shape, r.Cw)
    dy, w = op["dy"], op["w"]
    xs = r.shape[:4]
    acc = _dgrad32(dy, w, xs, st, pad)
    # one (tap, 8 filters of dY) dropped at one dx row: the tap (t0, t0) reaches row h0 from dY row p0
    n0, p0, t0, o0 = N - 1, 0, R // 2, 8
    h0 = p0 * st - pad + t0
    cut = acc.copy()
    hit = 0
    for q in range(dy.shape[2]):
        ww = q * st - pad + t0
        if 0 <= ww < W:
            cut[n0, h0, ww] -= dy[n0, p0, q, o0:o0 + 8] @ w[o0:o0 + 8, :, t0, t0]
            hit += 1
    assert 0 <= h0 < H and hit
    K = R * R * O
    mut = {MUTANTS[0]: _trunc(acc), MUTANTS[1]: _rne(cut),
           MUTANTS[2]: _rne(_dgrad32(dy, _drop_ko(w, 64 * (_ksteps(K) - 1)), xs, st, pad))}
    if r.splits > 1:
        mut[MUTANTS[4]] = _rne(_dgrad32(dy, _drop_ko(w, _split_first(r, _ksteps(K))), xs, st, pad))
    _judge(key, _rne(acc), mut, cc.dgrad_interval(r), True)
    if key == "d_tap":
        dx = emulate.conv2d_dgrad(_f32(dy).bfloat16(), emulate.pack_weight(torch.from_numpy(w), C), xs, st, pad, Cw=r.Cw)
        assert cc.outside(dx.float().numpy()[..., :r.Cw], cc.dgrad_interval(r), True)[0] == 0
    if "add" in r.variants:
        base = op["base"][..., :r.Cw]
        one, two = _rne(_add32(acc, base)), _rne(_add32(_rne(acc), base))
        assert not np.array_equal(one, two)
        honest, other = (one, two) if r.splits > 1 else (two, one)
        _judge(key + "+add", honest, {MUTANTS[6]: other}, cc.dgrad_interval(r, "add"), True)


@pytest.mark.parametrize("key", MUT_WGRAD)
def test_wgrad_bounds_reject_mutants(key):
    r = _row(cc.WGRAD, key)
    N, H, W, C, O, R, st, pad = r.shape
    op = cc.dense_operands(r.key, r.shape, C)
    x, dy = op["x"], op["dy"]
    npix = dy.shape[0] * dy.shape[1] * dy.shape[2]
    unit = 128 if "halo" in r.launches[0] else 64                           # pixels per K step
    steps = -(-npix // unit)
    mut = {MUTANTS[2]: _wgrad32(x, _drop_pixels(dy, unit * (steps - 1)), R, st, pad),
           MUTANTS[3]: _wgrad32(x, _drop_pixels(dy, npix // 2, npix // 2 + 1), R, st, pad)}
    if "z=1 " not in r.launches[0]:
        mut[MUTANTS[4]] = _wgrad32(x, _drop_pixels(dy, _split_first(r, steps, unit)), R, st, pad)
    iv = cc.wgrad_interval(r)
    _judge(key, _wgrad32(x, dy, R, st, pad), mut, iv, False)
    dw = emulate.conv2d_wgrad(_f32(x).bfloat16(), _f32(dy).bfloat16(), R, R, st, pad)
    assert cc.outside(dw.numpy(), iv)[0] == 0
    base = cc.wgrad_base(r).astype(np.float32)
    honest = _add32(base, _wgrad32(x, dy, R, st, pad))
    _judge(key + "+acc", honest, {MUTANTS[3]: _add32(base, mut[MUTANTS[3]])}, cc.wgrad_interval(r, acc=True), False)


@pytest.mark.parametrize("key", MUT_DW)
def test_depthwise_bounds_reject_mutants(key):
    r = _row(cc.DW, key)
    N, H, W, C, R, st = r.shape
    pad = R // 2
    op = cc.dw_operands(r.key, r.shape)
    x, w, dy = op["x"], op["w"], op["dy"]
    iv = cc.dw_intervals(r)
    acc = _fwd32(x, w, st, pad, groups=C)
    n0, p0, t0, c0 = N - 1, 1, R // 2, 8
    cut = acc.copy()
    for q in range(acc.shape[2]):
        ww = q * st - pad + t0
        if 0 <= ww < W:
            cut[n0, p0, q, c0:c0 + 8] -= x[n0, p0 * st - pad + t0, ww, c0:c0 + 8] * w[c0:c0 + 8, 0, t0, t0]
    wl = w.copy()
    wl[:, 0, R - 1, R - 1] = 0
    _judge(key + " fwd", _rne(acc), {MUTANTS[0]: _trunc(acc), MUTANTS[1]: _rne(cut),
                                     MUTANTS[2]: _rne(_fwd32(x, wl, st, pad, groups=C))}, iv["fwd"], True)
    y = emulate.dwconv_fwd(_f32(x).bfloat16(), torch.from_numpy(w), st, pad)
    assert cc.outside(y.float().numpy(), iv["fwd"], True)[0] == 0
    _judge_stats(key + " fwd", acc, op["shift"])
    dacc = _dgrad32(dy, w, (N, H, W, C), st, pad, groups=C)
    _judge(key + " dgrad", _rne(dacc), {MUTANTS[0]: _trunc(dacc),
                                        MUTANTS[2]: _rne(_dgrad32(dy, wl, (N, H, W, C), st, pad, groups=C))},
           iv["dgrad"], True)
    npix = dy.shape[0] * dy.shape[1] * dy.shape[2]
    _judge(key + " wgrad", _wgrad32(x, dy, R, st, pad, groups=C),
           {MUTANTS[3]: _wgrad32(x, _drop_pixels(dy, npix // 2, npix // 2 + 1), R, st, pad, groups=C)}, iv["wgrad"], False)


def test_mutant_matrix_is_complete():
    """Every mutant was judged (and rejected: the tests above assert it) on at least one case of each family it
    applies to; prints the matrix (profiles/conv_pin/README.md)."""
    for keys, test in ((MUT_FWD, test_forward_bounds_reject_mutants), (MUT_DGRAD, test_dgrad_bounds_reject_mutants),
                       (MUT_WGRAD, test_wgrad_bounds_reject_mutants), (MUT_DW, test_depthwise_bounds_reject_mutants)):
        for k in keys:
            if not any(c.split("+")[0].split(" ")[0] == k for c, _ in MATRIX):     # run alone or out of order
                test(k)
    for m in MUTANTS:
        cases = sorted(c for c, name in MATRIX if name == m)
        assert cases, m
        print("%-52s %s" % (m, ", ".join("%s: %d" % (c, MATRIX[(c, m)]) for c in cases)))
    fam = {"f_": MUTANTS[:3] + MUTANTS[4:], "d_": MUTANTS[:3] + (MUTANTS[4], MUTANTS[6]), "wg_": MUTANTS[2:5],
           "dw_": MUTANTS[:4] + (MUTANTS[5],)}
    for prefix, ms in fam.items():
        for m in ms:
            assert any(c.startswith(prefix) and name == m for c, name in MATRIX), (prefix, m)


# ---------------------------------------------------------------------------------------------------------------
# the labels are true
# ---------------------------------------------------------------------------------------------------------------
R18_B128_TAP128 = {      # instantiations test_resnet18_batch128_conv_shapes reaches: (shape C padded to 8, variant)
    "conv_tap<128, 8, false>": ((128, 32, 32, 64, 128, 3, 2, 1), "fwd.big"),
    "conv_tap_phases<128, 8>": ((128, 16, 16, 128, 256, 3, 2, 1), "dgrad.wd1.acc0"),
}
# Not reached by the tables: each needs a workload-size problem (128-row tiles are planned only when there are more
# tiles than CUs).  The two above run in tests/test_cnn_kernels_gpu.py::test_resnet18_batch128_conv_shapes; the
# generic 128-row tiles (the forward of GoogLeNet's 8 -> 192 stem, the DGRAD without a weight image) and the GEN tap
# kernel's 128-column tile run in the batch-128 zoo rounds of tests/test_cnn_native_gpu.py and per launch in
# tests/test_cnn_shadow_gpu.py.
WORKLOAD_SIZE_ONLY = set(R18_B128_TAP128) | {"conv_igemm<0, 128, 128>", "conv_igemm<1, 128, 128>",
                                             "conv_igemm<1, 128, 64>", "conv_tap<128, 8, true>"}


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("conv_pin")
    exe, table = d / "dispatch_recorder", d / "shapes.txt"
    shapes = sorted({r.shape for r in cc.FWD + cc.DGRAD + cc.WGRAD + [cc.WGRAD_8X8]} | {s for s, _ in R18_B128_TAP128.values()})
    table.write_text("".join(" ".join(str(v) for v in s) + "\n" for s in shapes))
    subprocess.run([HIPCC, "-O0", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", str(ROOT / "csrc"),
                    str(ROOT / "tests" / "dispatch_recorder.hip"), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe), str(table)], check=True, capture_output=True, text=True).stdout
    rec = cc.parse_record(out)
    assert set(rec) == set(shapes)
    return rec


@pytest.mark.parametrize("row", cc.FWD, ids=lambda r: r.key)
def test_forward_labels(record, row):
    got = cc.launch_labels(record[row.shape]["fwd.exact" if row.ws else "fwd.nows"])
    assert got == row.launches
    assert int(got[0].split("z=")[1].split()[0]) == row.splits
    if row.ws:       # a split row plans nothing without its workspace, and the exact size is enough
        assert len(record[row.shape]["fwd.nows"]) == 1
        assert cc.launch_labels(record[row.shape]["fwd.big"]) == row.launches


@pytest.mark.parametrize("row", cc.DGRAD, ids=lambda r: r.key)
def test_dgrad_labels(record, row):
    got = cc.launch_labels(record[row.shape]["dgrad.wd%d.exact" % row.wd])
    assert got == row.launches
    assert max(int(v) for lb in got for v in lb.split("z=")[1].split()[0:1]) == row.splits
    if "add" in row.variants:
        assert record[row.shape]["ws"].split("fusable=")[1].split(",")[1] == "1"      # conv.dgrad_fusable with an image
    # accumulate changes no launch: the same kernels, grids and K steps
    acc = cc.launch_labels(record[row.shape]["dgrad.wd%d.acc1" % row.wd])
    if "acc" in row.variants:
        assert acc == row.launches


@pytest.mark.parametrize("row", cc.WGRAD + [cc.WGRAD_8X8], ids=lambda r: r.key)
def test_wgrad_labels(record, row):
    rec = record[row.shape]
    N, H, W, C, O, R, st, pad = row.shape
    P, Q = cc.out_hw(H, W, R, st, pad)
    steps = -(-N * P * Q // 64)
    for want in (1, 7):      # the Python mirror of split_k against the planner, on every shape of the table
        lb = cc.launch_labels(rec["wgrad.splits%d" % want])[0]
        assert lb.split(" z=")[1] == "%d kps=%d" % cc.split_k(steps, want)[::-1], (row.key, want)
    if row.splits in (0, 1, 7):
        got = cc.launch_labels(rec["wgrad.auto.1x1_%d.exact" % row.lib if row.splits == 0 else "wgrad.splits%d" % row.splits])
    else:                    # another explicit count: the generic kernel of this shape, split_k's answer
        k7 = cc.launch_labels(rec["wgrad.splits7"])
        kps, sp = cc.split_k(steps, row.splits)
        got = ("%s z=%d kps=%d" % (k7[0].split(" z=")[0], sp, kps), "%s splits=%d" % (k7[1].split(" splits=")[0], sp))
    assert got == row.launches


def test_tables_reach_every_instantiation_of_the_golden_record(record):
    golden = gzip.decompress((ROOT / "tests" / "golden" / "conv_dispatch_cus256.txt.gz").read_bytes()).decode()
    want = {ln.split(" g=")[0].strip() for ln in golden.splitlines() if ln.startswith("  ") and " g=" in ln}
    have = set()
    for r in cc.FWD + cc.DGRAD + cc.WGRAD:
        have |= cc.kernels_of(r.launches)
    for r in cc.DGRAD:       # the rows with a weight image pack it with dgrad_pack_weights
        if r.wd:
            have |= cc.kernels_of(cc.launch_labels(record[r.shape]["dgrad_pack"]))
    assert want - have == WORKLOAD_SIZE_ONLY, (sorted(want - have), sorted(have - want))
    for name, (shape, variant) in R18_B128_TAP128.items():
        assert name in cc.kernels_of(cc.launch_labels(record[shape][variant])), name
    # every shape of the golden record that reaches one of them has a GEMM of at least 2**20 outputs (hundreds of
    # tiles: the planner takes 128-row tiles only with more tiles than CUs), most a reference beyond 1e8 products
    for block in golden.split("shape ")[1:]:
        lines = block.splitlines()
        N, H, W, C, O, R, st, pad = (int(v) for v in lines[0].split())
        P, Q = cc.out_hw(H, W, R, st, pad)
        if any(ln.split(" g=")[0].strip() in WORKLOAD_SIZE_ONLY for ln in lines if ln.startswith("  ")):
            assert max(N * P * Q * O, N * H * W * C) >= 1 << 20, lines[0]
