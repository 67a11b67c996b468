"""Numerics of the flat-buffer and compression HIP kernels vs PyTorch fp32."""
import numpy as np
import pytest
import torch

import int8_check as ic
from fedmi import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat(gpu_device):
    return native.require()


def S():
    return native.stream_handle()


@pytest.mark.parametrize("n", [1, 7, 1027, 4096, 100003, 2048 * 256 * 4 + 5])   # 1027: vectors plus tail; the last: past the grid cap
def test_sgd_flat(nat, gpu_device, n):
    torch.manual_seed(n)
    p = torch.randn(n, device=gpu_device)
    g = torch.randn(n, device=gpu_device)
    b = torch.randn(n, device=gpu_device)
    pr, br = p.clone(), b.clone()
    nat.sgd_flat(S(), p.data_ptr(), g.data_ptr(), b.data_ptr(), n, 0.1, 0.9, 5e-4, 0.0, False, False)
    d = g + 5e-4 * pr
    br = 0.9 * br + d
    pr = pr - 0.1 * br
    torch.cuda.synchronize()
    assert torch.allclose(b, br, rtol=1e-6, atol=1e-6)
    assert torch.allclose(p, pr, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("n,k,ties", [(62006, 620, False), (5000, 1, False), (5000, 5000, False),
                                       (1 << 20, 10000, False), (11173962, 111740, False), (70001, 700, True),
                                       (4099, 17, True), (1 << 21, 5000, "sparse")])
def test_topk_ef_exact(nat, gpu_device, n, k, ties):
    """Fused error-feedback top-k: d = x - g + r built in r, exactly the k largest |d| selected (ties:
    smallest indices), r keeps the rest; called twice on the same state (it must leave it reusable)."""
    torch.manual_seed(k)
    for rep in range(2):
        x = torch.randn(n, device=gpu_device)
        g = torch.randn(n, device=gpu_device) * 0.5
        r = torch.randn(n, device=gpu_device) * 0.1
        if ties == "sparse":                  # 100 nonzeros, k = 5000: the rest are ties at 0 (huge candidate lists)
            x.zero_(); g.zero_(); r.zero_()
            x[torch.randperm(n, device=gpu_device)[:100]] = torch.randn(100, device=gpu_device)
        elif ties:                            # many exact ties at the threshold magnitude
            x[::3] = 0.75
            g[::3] = 0.0
            r[::3] = 0.0
            x[1::7] = -0.75
            g[1::7] = 0.0
            r[1::7] = 0.0
        x[::97] = 0.0
        g[::97] = 0.0
        r[::97] = 0.0
        d = x - g + r
        if rep == 0:
            state = torch.zeros(nat.topk_state_bytes(), dtype=torch.uint8, device=gpu_device)
            cidx = torch.empty(2 * n, dtype=torch.int32, device=gpu_device)
            ckey = torch.empty(2 * n, dtype=torch.int32, device=gpu_device)
        idx = torch.full((k,), -1, dtype=torch.int32, device=gpu_device)
        val = torch.zeros(k, device=gpu_device)
        nat.topk_ef(S(), x.data_ptr(), g.data_ptr(), r.data_ptr(), n, k, state.data_ptr(), cidx.data_ptr(),
                    ckey.data_ptr(), idx.data_ptr(), val.data_ptr())
        torch.cuda.synchronize()
        assert int(idx.min()) >= 0
        sel = idx.long()
        assert len(set(sel.tolist())) == k
        assert torch.equal(d[sel], val)
        ref = d.abs().topk(k).values
        assert torch.equal(val.abs().sort(descending=True).values, ref)
        thr = ref[-1]
        tied = (d.abs() == thr).nonzero().flatten()
        chosen_tied = sel[d[sel].abs() == thr].sort().values
        assert torch.equal(chosen_tied, tied[: chosen_tied.numel()])     # smallest indices win ties
        mask = torch.ones(n, dtype=torch.bool, device=gpu_device)
        mask[sel] = False
        assert torch.equal(r[mask], d[mask])
        assert r[~mask].abs().sum().item() == 0
        off = nat.topk_overflow_offset()
        assert int(state[off:off + 4].view(torch.int32).item()) == 0      # no select ever exceeded k


def test_scatter_add_ranked_is_rank_ordered(nat, gpu_device):
    """Two ranks' top-k payloads (unique indices within a rank, overlapping across ranks) are
    applied in rank order without atomics: the result equals the sequential fp32 sum."""
    n, m = 1000, 4
    base = torch.randn(n, device=gpu_device)
    out = base.clone()
    idx = torch.tensor([[1, 5, 7, 999], [5, 2, 999, 0]], dtype=torch.int32, device=gpu_device)
    val = torch.randn(2, m, device=gpu_device)
    nat.scatter_add_ranked(S(), out.data_ptr(), idx.data_ptr(), val.data_ptr(), 2, m, 0.5, n)
    torch.cuda.synchronize()
    exp = base.clone().cpu()
    for r in range(2):
        for i in range(m):
            exp[int(idx[r, i])] += 0.5 * float(val[r, i])
    assert torch.equal(out.cpu(), exp)


def test_int8_roundtrip(nat, gpu_device):
    n = 62006
    torch.manual_seed(1)
    d = torch.randn(n, device=gpu_device)
    nch = (n + 255) // 256
    q = torch.empty(n, dtype=torch.int8, device=gpu_device)
    sc = torch.empty(nch, device=gpu_device)
    res = torch.empty(n, device=gpu_device)
    nat.quant_int8(S(), d.data_ptr(), n, q.data_ptr(), sc.data_ptr(), res.data_ptr())
    out = torch.zeros(n, device=gpu_device)
    nat.dequant_accum(S(), q.data_ptr(), sc.data_ptr(), 1, n, out.data_ptr(), 1.0)
    torch.cuda.synchronize()
    # reference quantizer
    pad = torch.zeros(nch * 256, device=gpu_device)
    pad[:n] = d
    amax = pad.view(nch, 256).abs().amax(1)
    s_ref = torch.where(amax > 0, amax / 127, torch.ones_like(amax))
    assert torch.allclose(sc, s_ref)
    deq = (torch.round(pad.view(nch, 256) / s_ref[:, None]).clamp(-127, 127) * s_ref[:, None]).view(-1)[:n]
    assert torch.allclose(out, deq, atol=1e-6)
    assert torch.allclose(res, d - deq, atol=1e-6)


def test_topk_ef_state_alternates_paths(nat, gpu_device):
    """One state reused across calls that alternate between the 2-level (< 1 M entries) and 3-level paths
    and between histogram parities: every call still selects exactly the top k."""
    torch.manual_seed(3)
    state = torch.zeros(nat.topk_state_bytes(), dtype=torch.uint8, device=gpu_device)
    for n, k in ((1 << 21, 20000), (70001, 700), (300000, 3000), (1 << 21, 9000), (62006, 620)):
        x = torch.randn(n, device=gpu_device)
        g = torch.zeros(n, device=gpu_device)
        r = torch.zeros(n, device=gpu_device)
        cidx = torch.empty(2 * n, dtype=torch.int32, device=gpu_device)
        ckey = torch.empty(2 * n, dtype=torch.int32, device=gpu_device)
        idx = torch.full((k,), -1, dtype=torch.int32, device=gpu_device)
        val = torch.zeros(k, device=gpu_device)
        nat.topk_ef(S(), x.data_ptr(), g.data_ptr(), r.data_ptr(), n, k, state.data_ptr(), cidx.data_ptr(),
                    ckey.data_ptr(), idx.data_ptr(), val.data_ptr())
        torch.cuda.synchronize()
        assert int(idx.min()) >= 0 and len(set(idx.tolist())) == k, n
        assert torch.equal(val.abs().sort(descending=True).values, x.abs().topk(k).values), n


# ---------------------------------------------------------------------------------------------------------------
# The int8 / scatter-add kernels against the exact reference (tests/int8_check.py): torch.equal, no tolerances.
# ---------------------------------------------------------------------------------------------------------------
PAST_CAP = 2048 * 256          # entries one full grid of the capped kernels covers: beyond it they grid-stride


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _quant(nat, dev, d, with_residual=True):
    n = d.size
    dd = _dev(d, dev)
    q = torch.full((n,), 77, dtype=torch.int8, device=dev)
    sc = torch.full((ic.nchunks(n),), -5.0, device=dev)
    res = torch.full((n,), -5.0, device=dev)
    nat.quant_int8(S(), dd.data_ptr(), n, q.data_ptr(), sc.data_ptr(), res.data_ptr() if with_residual else 0)
    torch.cuda.synchronize()
    return q.cpu(), sc.cpu(), res.cpu()


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1027, 62006])
@pytest.mark.parametrize("case", ic.CASES)
def test_quant_int8_exact(nat, gpu_device, case, n):
    """q, scales and residual equal the reference bit for bit: rank 1's d of rounds 0 (the designed values) and 1
    (a carried residual) of every data case; once more without a residual buffer."""
    for k, (xs, g, rs, _, _) in enumerate(ic.run_rounds(case, n, 3)[:2]):
        d = ic.delta(xs[1], g, rs[1])
        q_ref, s_ref, res_ref = ic.quantise(d)
        q, sc, res = _quant(nat, gpu_device, d)
        assert torch.equal(sc, torch.from_numpy(s_ref)), (k, "scales")
        assert torch.equal(q, torch.from_numpy(q_ref)), (k, "q")
        assert torch.equal(res, torch.from_numpy(res_ref)), (k, "residual")
        if k == 0:
            q, sc, res = _quant(nat, gpu_device, d, with_residual=False)
            assert torch.equal(sc, torch.from_numpy(s_ref)) and torch.equal(q, torch.from_numpy(q_ref))
            assert (res == -5.0).all()
    if case == "subnormal":                     # amax / 127 underflows: scale 1, nothing sent, nothing lost
        xs, g, rs, _, _ = ic.run_rounds(case, n, 3)[0]
        d = ic.delta(xs[1], g, rs[1])
        q, sc, res = _quant(nat, gpu_device, d)
        for c in ic.special_chunks(n):
            sl = slice(c * 256, min(n, (c + 1) * 256))
            assert sc[c].item() == 1.0 and not q[sl].any() and torch.equal(res[sl], torch.from_numpy(d[sl]))


@pytest.mark.parametrize("n", [257, 62006, PAST_CAP + 257])
@pytest.mark.parametrize("scale", [1.0, ic.f32(1.0 / 3.0)], ids=["one", "third"])
@pytest.mark.parametrize("R", [1, 3])
def test_dequant_accum_exact(nat, gpu_device, R, scale, n):
    gen = torch.Generator().manual_seed(100 * R + n)
    nch = ic.nchunks(n)
    q = torch.randint(-127, 128, (R, n), generator=gen, dtype=torch.int8)
    sc = torch.randn(R, nch, generator=gen).abs() * 1e-2 + 1e-6
    out0 = torch.randn(n, generator=gen)
    exp = ic.dequant_accum(q.numpy(), sc.numpy(), out0.numpy(), scale)
    out = out0.to(gpu_device)
    qd, sd = q.to(gpu_device), sc.to(gpu_device)
    nat.dequant_accum(S(), qd.data_ptr(), sd.data_ptr(), R, n, out.data_ptr(), scale)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(exp))


@pytest.mark.parametrize("n", [1, 1027, PAST_CAP + 5])
@pytest.mark.parametrize("with_residual", [True, False])
def test_ef_delta_exact(nat, gpu_device, with_residual, n):
    gen = torch.Generator().manual_seed(n)
    mag = 10.0 ** torch.randint(-6, 7, (n,), generator=gen).double()
    g = (mag * torch.randn(n, generator=gen).double()).float()
    x = (g.double() + 1e-2 * mag * torch.randn(n, generator=gen).double()).float()
    r = (1e-3 * mag * torch.randn(n, generator=gen).double()).float()
    exp = ic.delta(x.numpy(), g.numpy(), r.numpy() if with_residual else None)
    xd, gd, rd = x.to(gpu_device), g.to(gpu_device), r.to(gpu_device)
    d = torch.full((n,), -5.0, device=gpu_device)
    nat.ef_delta(S(), xd.data_ptr(), gd.data_ptr(), rd.data_ptr() if with_residual else 0, d.data_ptr(), n)
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), torch.from_numpy(exp))


@pytest.mark.parametrize("m", [17, PAST_CAP + 5])
def test_scatter_add_ranked_exact(nat, gpu_device, m):
    """Three ranks, scale fp32(1/3) (scale * val is not exact: an fma differs from a multiply and an add), indices
    unique within a rank and overlapping across ranks, a few out-of-range ones (-1 and n) that must be ignored."""
    R, n = 3, m + 3
    scale = ic.f32(1.0 / 3.0)
    gen = torch.Generator().manual_seed(m)
    idx = torch.stack([torch.randperm(n, generator=gen)[:m] for _ in range(R)]).to(torch.int32)
    for r in range(R):
        idx[r, (5 * r + 1) % m] = -1
        idx[r, (7 * r + 3) % m] = n
    val = torch.randn(R, m, generator=gen)
    out0 = torch.randn(n, generator=gen)
    exp = ic.scatter_add(out0.numpy(), idx.numpy(), val.numpy(), scale)
    # guard words around the model: an index of -1 or n must not be written either
    buf = torch.full((n + 8,), 123.0, device=gpu_device)
    out = buf[4:4 + n]
    out.copy_(out0)
    idxd, vald = idx.to(gpu_device), val.to(gpu_device)
    nat.scatter_add_ranked(S(), out.data_ptr(), idxd.data_ptr(), vald.data_ptr(), R, m, scale, n)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(exp))
    assert (buf[:4] == 123.0).all() and (buf[4 + n:] == 123.0).all()


def _sgd_reference(p, g, b, lr, mo, wd, damp, nesterov, first):
    """fp64 evaluation of torch.optim.SGD's update on the fp32 inputs (scalars as the kernel receives them, in
    fp32), and the bound of each output.  -> (p64, b64, Ep, Eb).

        d  = g + wd*p
        b' = d                      (first)     or   mo*b + (1 - damp)*d         (momentum != 0; else b' = b)
        d' = d + mo*b' (nesterov),  b' (momentum != 0),  d (momentum == 0)
        p' = p - lr*d'

    The kernel's sgd_elem evaluates this in fp32 and leaves contraction to the compiler, so it is not bit-exact.
    The longest chain (dampening and nesterov) has 10 fp32 roundings of <= 0.5 ulp of a partial result each, and
    every partial result is bounded by the SUM OF THE MAGNITUDES of the terms it is formed from (sums can cancel,
    magnitudes cannot); 5 ulp at most, and the project's rule (server_opt_check.py) allows 16 ulp = 2e-6 of that sum:

        D  = |g| + |wd*p|                                   magnitudes behind d
        B  = D (first)  or  |mo*b| + (1 - damp)*D           magnitudes behind b'        ->  |b' - b64| <= 2e-6 * B
        D' = D + mo*B (nesterov),  B (momentum),  D (none)  magnitudes behind d'
                                                            ->  |p' - p64| <= 2e-6 * (|p| + lr*D')
    """
    lr, mo, wd, damp = (ic.f32(v) for v in (lr, mo, wd, damp))
    p, g, b = p.double(), g.double(), b.double()
    d = g + wd * p
    D = g.abs() + (wd * p).abs()
    if mo != 0.0:
        if first:
            b1, B = d, D
        else:
            b1 = mo * b + (1.0 - damp) * d
            B = (mo * b).abs() + (1.0 - damp) * D
        d1, D1 = (d + mo * b1, D + mo * B) if nesterov else (b1, B)
    else:
        b1, B, d1, D1 = b, torch.zeros_like(b), d, D
    return p - lr * d1, b1, 2e-6 * (p.abs() + lr * D1), 2e-6 * B


@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("damp", [0.0, 0.1])
@pytest.mark.parametrize("mo", [0.0, 0.9])
@pytest.mark.parametrize("n", [7, 1027])
def test_sgd_flat_branches(nat, gpu_device, n, mo, damp, nesterov, first, wd):
    """Every branch of sgd_elem against the fp64 update within the derived bounds; without momentum the buffer is
    not touched."""
    gen = torch.Generator().manual_seed(n)
    p0, g0, b0 = (torch.randn(n, generator=gen) for _ in range(3))
    p, g, b = p0.to(gpu_device), g0.to(gpu_device), b0.to(gpu_device)
    nat.sgd_flat(S(), p.data_ptr(), g.data_ptr(), b.data_ptr(), n, 0.1, mo, wd, damp, nesterov, first)
    torch.cuda.synchronize()
    p64, b64, ep, eb = _sgd_reference(p0, g0, b0, 0.1, mo, wd, damp, nesterov, first)
    assert torch.equal(g.cpu(), g0)
    if mo == 0.0:
        assert torch.equal(b.cpu(), b0)
    else:
        err = (b.cpu().double() - b64).abs()
        assert (err <= eb).all(), f"buf: worst ratio {float((err / eb).max()):.3g}"
    err = (p.cpu().double() - p64).abs()
    assert (err <= ep).all(), f"p: worst ratio {float((err / ep).max()):.3g}"


def test_compression_bindings_check_their_arguments(nat, gpu_device):
    """n == 0 (m == 0) returns before anything is launched -- null pointers are fine there -- and a negative size, a
    null required buffer or R <= 0 raise ValueError instead of reaching a kernel."""
    a = torch.zeros(512, device=gpu_device)
    i = torch.zeros(512, dtype=torch.int32, device=gpu_device)
    q = torch.zeros(512, dtype=torch.int8, device=gpu_device)
    A, I, Q = a.data_ptr(), i.data_ptr(), q.data_ptr()
    nat.ef_delta(S(), 0, 0, 0, 0, 0)
    nat.quant_int8(S(), 0, 0, 0, 0, 0)
    nat.dequant_accum(S(), 0, 0, 1, 0, 0, 1.0)
    nat.scatter_add_ranked(S(), 0, 0, 0, 1, 0, 1.0, 10)
    nat.scatter_add_ranked(S(), 0, 0, 0, 1, 10, 1.0, 0)
    torch.cuda.synchronize()
    bad = [
        lambda: nat.ef_delta(S(), A, A, 0, A, -1),
        lambda: nat.ef_delta(S(), 0, A, 0, A, 4),
        lambda: nat.ef_delta(S(), A, 0, 0, A, 4),
        lambda: nat.ef_delta(S(), A, A, 0, 0, 4),
        lambda: nat.quant_int8(S(), A, -1, Q, A, 0),
        lambda: nat.quant_int8(S(), 0, 4, Q, A, 0),
        lambda: nat.quant_int8(S(), A, 4, 0, A, 0),
        lambda: nat.quant_int8(S(), A, 4, Q, 0, 0),
        lambda: nat.dequant_accum(S(), Q, A, 1, -1, A, 1.0),
        lambda: nat.dequant_accum(S(), Q, A, 0, 4, A, 1.0),
        lambda: nat.dequant_accum(S(), Q, A, -2, 4, A, 1.0),
        lambda: nat.dequant_accum(S(), 0, A, 1, 4, A, 1.0),
        lambda: nat.dequant_accum(S(), Q, 0, 1, 4, A, 1.0),
        lambda: nat.dequant_accum(S(), Q, A, 1, 4, 0, 1.0),
        lambda: nat.scatter_add_ranked(S(), A, I, A, 0, 4, 1.0, 16),
        lambda: nat.scatter_add_ranked(S(), A, I, A, 1, -1, 1.0, 16),
        lambda: nat.scatter_add_ranked(S(), A, I, A, 1, 4, 1.0, -1),
        lambda: nat.scatter_add_ranked(S(), 0, I, A, 1, 4, 1.0, 16),
        lambda: nat.scatter_add_ranked(S(), A, 0, A, 1, 4, 1.0, 16),
        lambda: nat.scatter_add_ranked(S(), A, I, 0, 1, 4, 1.0, 16),
        lambda: nat.topk_ef(S(), 0, A, A, 16, 4, A, I, I, I, A),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert not a.any() and not i.any() and not q.any()          # nothing was launched on them
