"""The PowerSGD kernels (csrc/kernels/powersgd.hip) through their bindings against tests/powersgd_check.py at the edges
of their tiles, in one table that ignores the worth rule; then the compressor end to end on two in-process clients."""
import numpy as np
import pytest
import torch

import powersgd_check as pc
from fedmi import native
from fedmi.engine.lenet_native import LENET_SPEC
from fedmi.parallel.compress import psgd_tables
from test_powersgd import check_phases, views_of
from test_robust_gpu import _GpuStub

pytestmark = pytest.mark.gpu

# rows 1 / 5 / 16 / 17 / 33 and one past the row chunk; columns 3 / 4 / 63 / 65 / 257 and one past the column slab
SHAPES = [(1, 3), (5, 4), (16, 63), (17, 65), (33, 257), (5, 1025), (257, 7)]
CANARY, PAD = 12345.0, 16                # 16 floats: the payload between the canaries stays 16-byte aligned
ZERO_SEG = 3                             # orth: this segment's P- has a zero column


class _Case:
    """x / global / residual: segment i starts at an offset congruent to (0, 1, 3)[i % 3] mod 4, behind a dense range
    (even i) or a gap of NaNs that no table names (odd i).  Row r and column c of every matrix carry the scales 2^(r % 5)
    and 3^(c % 3), column j of Q and P^ the scale j + 1: a transposed or permuted fragment misses the bounds by orders of
    magnitude."""

    def __init__(self, R, dev):
        self.R, self.dev, self.nat = R, dev, native.require()
        rng = np.random.default_rng(7)
        self.comp, self.dense, gaps, end = [], [], [], 0
        for i, (rows, cols) in enumerate(SHAPES):
            off = end + 5
            off += ((0, 1, 3)[i % 3] - off) % 4
            (self.dense if i % 2 == 0 else gaps).append((end, off - end))
            self.comp.append((off, rows, cols))
            end = off + rows * cols
        self.n, self.host = end, {}
        for name in ("x", "g", "res"):
            v = rng.standard_normal(self.n).astype(np.float32)
            for off, rows, cols in self.comp:
                v[off:off + rows * cols] *= np.outer(2.0 ** (np.arange(rows) % 5), 3.0 ** (np.arange(cols) % 3)).reshape(-1)
            for off, ln in gaps:
                v[off:off + ln] = np.nan
            for off, ln in self.dense if name == "res" else []:
                v[off:off + ln] = 0.0
            self.host[name] = v
        self.covered = ~np.isnan(self.host["x"])
        self.tb = tb = psgd_tables(self.comp, self.dense, R, self.n, self.nat.psgd_geometry())
        assert len(tb["pfolds"]) and len(tb["qfolds"])                     # both splits are in the table
        self.tab = {k: (torch.from_numpy(v.view(np.uint8).reshape(-1).copy()).to(dev), len(v))
                    for k, v in tb.items() if isinstance(v, np.ndarray)}
        cols_scale = lambda m: np.tile(np.arange(1, R + 1, dtype=np.float32), m // R)   # noqa: E731
        self.q = rng.standard_normal(tb["n_q"]).astype(np.float32) * cols_scale(tb["n_q"])
        self.ph = rng.standard_normal(tb["n_p"]).astype(np.float32) * cols_scale(tb["n_p"])
        self.part = {k: torch.full((tb[k],), np.nan, device=dev) for k in ("n_ppart", "n_qpart")}
        self.d = pc.delta(self.host["x"], self.host["g"], self.host["res"])

    def up(self, v):
        buf = torch.full((v.size + 2 * PAD,), CANARY, device=self.dev)
        buf[PAD:PAD + v.size] = torch.from_numpy(v).to(self.dev)
        return buf

    def down(self, buf):
        """The payload on the host, once the canaries around it are seen to be intact."""
        torch.cuda.synchronize()
        v = buf.cpu().numpy()
        assert (v[:PAD] == CANARY).all() and (v[-PAD:] == CANARY).all()
        return v[PAD:-PAD]

    def segs(self):
        poff = qoff = 0
        for off, rows, cols in self.comp:
            yield slice(off, off + rows * cols), rows, cols, slice(poff, poff + rows * self.R), slice(qoff, qoff + cols * self.R)
            poff, qoff = poff + rows * self.R, qoff + cols * self.R

    def call(self, fn, *args):
        """``fn(stream, ...)``: canaried buffers go as the payload's address, a table name as its address and length."""
        flat = []
        for a in args:
            if isinstance(a, str):
                flat += [self.tab[a][0].data_ptr(), self.tab[a][1]]
            else:
                flat.append(a[PAD:].data_ptr() if torch.is_tensor(a) else a)
        getattr(self.nat, fn)(native.stream_handle(self.dev), *flat)

    def project(self):
        b = {k: self.up(v) for k, v in self.host.items()}
        send = self.up(np.full(self.tb["n_p"] + self.tb["n_dense"], np.nan, dtype=np.float32))
        segs = self.tab["segs"][0].data_ptr()
        self.call("psgd_project", b["x"], b["g"], b["res"], segs, "project", self.up(self.q), self.R, send,
                  self.part["n_ppart"].data_ptr(), "pfolds")
        return [self.down(v) for v in (b["x"], b["g"], b["res"], send)]

    def backproject(self):
        q = self.up(np.full(self.tb["n_q"], np.nan, dtype=np.float32))
        self.call("psgd_backproject", self.up(self.d), self.tab["segs"][0].data_ptr(), "backproject", self.up(self.ph),
                  self.R, q, self.part["n_qpart"].data_ptr(), "qfolds")
        return self.down(q)


@pytest.fixture(scope="module", params=[1, 3, 4, 8])
def case(request, gpu_device):
    return _Case(request.param, gpu_device)


def test_project_and_backproject_within_their_bounds(case):
    x, g, res, p = case.project()
    q = case.backproject()
    for a, b in zip((x, g, res, p, q), case.project() + [case.backproject()]):       # repeatable bit for bit
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(x, case.host["x"], equal_nan=True) and np.array_equal(g, case.host["g"], equal_nan=True)
    assert not np.isnan(p).any() and not np.isnan(q).any()                 # no gap leaked in, nothing left unwritten
    worst = 0.0
    for sl, rows, cols, ps, qs in case.segs():
        m = case.d[sl].reshape(rows, cols)
        assert np.array_equal(res[sl], case.d[sl])                         # d over the residual, two roundings
        for got, (ref, bound) in ((p[ps].reshape(rows, -1), pc.gemm(m, case.q[qs].reshape(cols, -1))),
                                  (q[qs].reshape(cols, -1), pc.gemm(m.T, case.ph[ps].reshape(rows, -1)))):
            assert np.all(np.abs(got - ref) <= bound)
            worst = max(worst, float(np.max(np.abs(got - ref) / np.maximum(bound, 1e-300))))
    print(f"R={case.R}: worst GEMM error / bound {worst:.3f}")
    at = case.tb["n_p"]
    for off, ln in case.dense:                                             # the dense part behind P, its residual untouched
        assert np.array_equal(p[at:at + ln], case.d[off:off + ln]) and not res[off:off + ln].any()
        at += ln
    assert np.isnan(res[~case.covered]).all()


def test_orth_within_its_bound(case):
    R, pbar = case.R, case.ph.copy()
    zero = [ps for i, (_, rows, _, ps, _) in enumerate(case.segs()) if i == ZERO_SEG and R > 1]
    for ps in zero:
        pbar[ps].reshape(-1, R)[:, 1] = 0.0
    buf = case.up(pbar)
    case.call("psgd_orth", "segs", buf, R)
    out, worst = case.down(buf), 0.0
    for _, rows, _, ps, _ in case.segs():
        pin, got = pbar[ps].reshape(rows, R), out[ps].reshape(rows, R)
        ref, bound = pc.orth(pin), pc.orth_bound(pin)
        # the bound is not tuned to the kernel: the fp32 numpy evaluation of the same formulas sits inside it
        assert np.max(np.abs(pc.orth(pin, np.float32) - ref)) <= pc.orth_bound(pin, dot_u=pc.U)
        assert np.isfinite(got).all() and np.max(np.abs(got - ref)) <= bound
        worst = max(worst, float(np.max(np.abs(got - ref)) / bound))
    assert all(not out[ps].reshape(-1, R)[:, 1].any() for ps in zero)      # a zero column stays zero, never NaN
    print(f"R={R}: worst orth error / bound {worst:.3e}")


def test_apply_bit_for_bit(case):
    R, host = case.R, dict(case.host, res=case.d.copy())
    for off, ln in case.dense:
        host["res"][off:off + ln] = 7.0                                    # must come back as 0
    send_h = np.concatenate([case.ph, np.random.default_rng(11).standard_normal(case.tb["n_dense"]).astype(np.float32)])
    b = {k: case.up(v) for k, v in host.items()}
    send = case.up(send_h)
    case.call("psgd_apply", b["x"], b["g"], b["res"], case.tab["segs"][0].data_ptr(), "project", send, case.up(case.q),
              send, R)
    want = {k: v.copy() for k, v in host.items()}
    for sl, rows, cols, ps, qs in case.segs():
        u = pc.low_rank(send_h[ps].reshape(rows, R), case.q[qs].reshape(cols, R)).reshape(-1)
        want["g"][sl], want["res"][sl] = host["g"][sl] + u, host["res"][sl] - u
    at = case.tb["n_p"]
    for off, ln in case.dense:                                             # the dense part: the averaged entries
        want["g"][off:off + ln], want["res"][off:off + ln] = host["g"][off:off + ln] + send_h[at:at + ln], 0.0
        at += ln
    want["x"] = np.where(case.covered, want["g"], host["x"])
    for k in want:                                                         # gaps and canaries untouched, the rest exact
        assert np.array_equal(case.down(b[k]), want[k], equal_nan=True), k


class _Stub(_GpuStub):
    def __init__(self, spec, dev):
        n = sum(int(np.prod(shape)) for _, shape in spec)
        super().__init__(torch.randn(n, generator=torch.Generator().manual_seed(0)).to(dev))
        self.state_dict = lambda: views_of(self.flat, spec)


@pytest.mark.parametrize("R", [2, 4])
def test_compressor_end_to_end_on_two_clients(R, gpu_device):
    check_phases([_Stub(LENET_SPEC, gpu_device) for _ in range(2)], R)
