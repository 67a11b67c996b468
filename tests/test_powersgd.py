"""--compress powersgd on the CPU: the segment rule, the phases driven side by side on in-process clients, an update of
exact low rank, one aggregate() over gloo, the refusals.  Reference and bounds: tests/powersgd_check.py."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import powersgd_check as pc
from fedmi.engine.lenet_native import LENET_SPEC
from fedmi.parallel.compress import PowerSGDCompressor, make_compressor, psgd_segments
from tests.helpers import free_port

SPEC = [("b0", (6,)), ("w1", (20, 33)), ("b1", (5,)), ("w2", (12, 7, 3)), ("small", (4, 5))]   # R = 2 compresses w1, w2


def views_of(flat, spec):
    offs = np.concatenate([[0], np.cumsum([int(np.prod(shape)) for _, shape in spec])])
    return OrderedDict((name, flat[offs[i]:offs[i + 1]].view(shape)) for i, (name, shape) in enumerate(spec))


class _Stub:
    """Minimal LocalTrainer surface: a flat float state and a state dict of views into it."""

    def __init__(self, spec=SPEC):
        n = sum(int(np.prod(shape)) for _, shape in spec)
        self.flat = torch.randn(n, generator=torch.Generator().manual_seed(0))
        self.views = views_of(self.flat, spec)
        self.float_state, self.state_dict = lambda: self.flat, lambda: self.views
        self.int_state, self.after_aggregate = lambda: [], lambda: None


def _update(rank, n):
    return 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(50 + rank))


def _np(t):
    return t.detach().cpu().numpy().copy()


def test_segment_rule_on_lenet():
    comp, dense = psgd_segments(_Stub(LENET_SPEC), 4)
    offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for _, s in LENET_SPEC])])
    at = {name: int(offs[i]) for i, (name, _) in enumerate(LENET_SPEC)}
    assert comp == [(at["conv2.weight"], 16, 150), (at["fc1.weight"], 120, 400), (at["fc2.weight"], 84, 120),
                    (at["fc3.weight"], 10, 84)]
    assert all(pc.worth(r, c, 4) for _, r, c in comp) and not pc.worth(6, 75, 4)
    # conv1 and its bias merge into one dense range; the other biases stand alone
    assert dense == [(0, 456), (at["conv2.bias"], 16), (at["fc1.bias"], 120), (at["fc2.bias"], 84), (at["fc3.bias"], 10)]
    gap = _Stub(LENET_SPEC)
    del gap.views["fc1.bias"]
    with pytest.raises(ValueError, match="does not tile"):
        psgd_segments(gap, 4)


def check_phases(stubs, R):
    """One round phase by phase on in-process clients that start from the same model, a plain mean between the phases,
    every stage against the fp64 rule evaluated on the stage's own inputs (the GPU test runs it on the kernels)."""
    W, dev = len(stubs), stubs[0].flat.device
    comps = [PowerSGDCompressor(s, rank=R) for s in stubs]
    c0 = comps[0]
    g0, q0 = _np(c0.global_ref), _np(c0.q)
    assert all(np.array_equal(_np(c.q), q0) for c in comps)              # the same start with nothing exchanged
    for r, s in enumerate(stubs):
        s.flat.add_(_update(r, s.flat.numel()).to(dev))
    xs = [_np(s.flat) for s in stubs]
    sends = [c.phase1(s.flat) for c, s in zip(comps, stubs)]
    ds = [_np(c.residual) for c in comps]
    for r, c in enumerate(comps):                        # d: in the residual where compressed, in the send buffer where dense
        for (off, ln), dst in zip(c.dense_ranges, c.doffs):
            ds[r][off:off + ln] = _np(sends[r])[dst:dst + ln]
        assert np.array_equal(ds[r], pc.delta(xs[r], g0, np.zeros_like(g0)))
    pbar = _np(torch.stack(sends).sum(0) / W)
    qs = [_np(c.phase2(torch.from_numpy(pbar.copy()).to(dev))) for c in comps]
    qbar = (torch.from_numpy(np.stack(qs)).sum(0) / W).numpy()
    for c, s in zip(comps, stubs):
        c.phase3(s.flat, torch.from_numpy(qbar.copy()).to(dev))
    g1 = _np(c0.global_ref)
    for c, s in zip(comps, stubs):                                       # identical bits everywhere
        assert np.array_equal(_np(c.global_ref), g1) and np.array_equal(_np(s.flat), g1)
    dmean = np.mean(np.stack(ds).astype(np.float64), axis=0)

    def mean_bound(ms, f):      # each client's GEMM within its bound, then the mean's W - 1 additions and one division
        return sum(pc.gemm(m, f)[1] + W * pc.U * (np.abs(m).astype(np.float64) @ np.abs(f)) for m in ms) / W

    for i, (off, rows, cols) in enumerate(c0.segments):
        sl = slice(off, off + rows * cols)
        ph = _np(c0._p(c0.send, i))
        p_in = pbar[c0.poffs[i]:c0.poffs[i] + rows * R].reshape(rows, R)
        q_in, q_out = (q[c0.qoffs[i]:c0.qoffs[i] + cols * R].reshape(cols, R) for q in (q0, qbar))
        m, mm = [d[sl].reshape(rows, cols) for d in ds], dmean[sl].reshape(rows, cols)
        # linearity: the averaged factors are the factors of the mean update
        assert np.all(np.abs(p_in - pc.gemm(mm, q_in)[0]) <= mean_bound(m, q_in))
        assert np.max(np.abs(ph - pc.orth(p_in))) <= pc.orth_bound(p_in)
        assert np.all(np.abs(q_out - pc.gemm(mm.T, ph)[0]) <= mean_bound([mk.T for mk in m], ph))
        u = pc.low_rank(ph, q_out)
        assert np.array_equal(g1[sl].reshape(rows, cols), g0[sl].reshape(rows, cols) + u)
        for c, d in zip(comps, m):                                       # error feedback: residual + u is d, one rounding
            res = _np(c.residual)[sl].reshape(rows, cols)
            assert np.array_equal(res, d - u)
            assert np.all(np.abs(res.astype(np.float64) + u - d) <= pc.U * np.abs(d.astype(np.float64) - u))
    for off, ln in c0.dense_ranges:                                      # the dense part: its mean, no residual
        sl = slice(off, off + ln)
        assert np.all(np.abs(g1[sl] - (g0[sl] + dmean[sl])) <= (W + 1) * pc.U * (np.abs(g0[sl]) + np.abs(dmean[sl])))
        assert all(not _np(c.residual)[sl].any() for c in comps)


def test_phases_are_linear_and_identical_across_clients():
    check_phases([_Stub() for _ in range(3)], 2)


def test_update_of_exact_low_rank_leaves_a_rounding_level_residual():
    R, rows, cols = 2, 24, 40
    gen = torch.Generator().manual_seed(3)
    stub = _Stub([("w", (rows, cols))])
    stub.flat.zero_()                                    # global = 0: d is the update itself, bit for bit
    comp = PowerSGDCompressor(stub, rank=R)
    q0 = _np(comp.q).reshape(cols, R)
    stub.flat.copy_((torch.randn(rows, R, generator=gen).double() @ torch.randn(R, cols, generator=gen).double()).view(-1))
    d = _np(stub.flat).reshape(rows, cols).astype(np.float64)           # rank R up to the rounding of its entries
    comp.phase3(stub.flat, comp.phase2(comp.phase1(stub.flat)))
    # P^ = B + D for an exact basis B of d's range: ||D||_F <= orth's error + the factor's shift under P's GEMM error
    # (sqrt(2) kappa ||E||_F / ||P||_2, Sun 1991), and d - P^ P^T d = -(D B^T + B D^T + D D^T) d.  To that come d's own
    # distance from rank R, the second GEMM's error through P^ (||P^||_F <= sqrt(R)) and step 4's R + 1 roundings.
    p, p_bound = pc.gemm(d, q0)
    dd = pc.orth_bound(p) + np.sqrt(2.0) * np.linalg.cond(p) * np.linalg.norm(p_bound) / np.linalg.norm(p, 2)
    ph, qb = _np(comp._p(comp.send, 0)), _np(comp.q).reshape(cols, R)
    bound = ((2 * dd + dd * dd + (R + 1) * pc.U) * np.linalg.norm(d) + np.sqrt(R) * np.linalg.norm(pc.gemm(d.T, ph)[1])
             + (R + 2) * pc.U * np.linalg.norm(np.abs(ph) @ np.abs(qb).T))
    worst = float(np.abs(_np(comp.residual)).max())
    print(f"exact rank {R}: max |residual| {worst:.3e}, bound {bound:.3e}, max |d| {np.abs(d).max():.3e}")
    assert worst <= bound < 1e-2 * np.abs(d).max()       # a lost direction would leave a residual of the size of d


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fedmi.parallel.fedavg import FedAvg

    stub = _Stub()
    comp = PowerSGDCompressor(stub, rank=2)
    stub.flat.add_(_update(rank, stub.flat.numel()))
    FedAvg(compressor=comp).average(stub)
    q.put((rank, stub.flat.numpy(), comp.global_ref.numpy(), comp.bytes_sent, comp.dense_bytes))
    dist.destroy_process_group()


@pytest.mark.slow
def test_aggregate_over_gloo_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r[0]: r[1:] for r in (q.get(timeout=120) for _ in procs)}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])    # identical bits
    assert np.array_equal(res[0][0], res[0][1]) and np.isfinite(res[0][0]).all()
    assert not np.array_equal(res[0][0], _Stub().flat.numpy())           # the model moved
    assert res[0][2] == res[1][2] == 4 * (2 * (20 + 33) + 2 * (12 + 21) + (6 + 5 + 20))
    assert res[0][3] == 4 * _Stub().flat.numel()


@pytest.mark.parametrize("rank", [0, 9, -1])
def test_rank_outside_1_to_8_is_refused(rank, capsys):
    from fedmi.cli import client

    with pytest.raises(ValueError, match="rank"):
        make_compressor("powersgd", 0.2, _Stub(), 0, powersgd_rank=rank)
    with pytest.raises(SystemExit):
        client.main(["--compress", "powersgd", "--powersgd-rank", str(rank)])
    assert "--powersgd-rank" in capsys.readouterr().err
