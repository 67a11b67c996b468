"""CPU side of the exact int8 / scatter-add reference (tests/int8_check.py): the reference agrees with exact
rational arithmetic, and the PyTorch twin in fedmi/parallel/compress.py (what a CPU client runs) gives the
reference's bits -- q, scales, residual and the new global model -- on every named data case, with one and three
simulated ranks, over three rounds with the residual carried."""
import numpy as np
import pytest
import torch

import int8_check as ic
from fedmi.parallel.compress import Int8Compressor, TopKCompressor

SIZES = [1, 255, 256, 257, 1027, 62006]


class _Flat:
    def __init__(self, t):
        self.t = t

    def float_state(self):
        return self.t


class _Gathered:
    """Stands in for a transport: all_gather returns every simulated rank's payload of this round."""

    def __init__(self, world):
        self.world = world
        self.rows = {}

    def all_gather(self, t):
        return self.rows[t.dtype].clone()


def T(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("case", ic.CASES)
def test_reference_matches_exact_rational(case):
    seen = sum(ic.self_check(case, n) for n in SIZES)
    assert seen >= 2000, seen


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", ic.CASES)
def test_twin_equals_reference_bit_for_bit(case, n, world):
    g0, r0, upd = ic.inputs(case, n, world)
    ref = ic.run_rounds(case, n, world)
    comps, scouts = [], []
    for r in range(world):
        for group in (comps, scouts):
            c = Int8Compressor(_Flat(T(g0).clone()))
            c.residual.copy_(T(r0[r]))
            group.append(c)
    tr = _Gathered(world)
    for k in range(ic.ROUNDS):
        xs_ref, g_ref, rs_ref, g1_ref, rs1_ref = ref[k]
        xs = [T(ic.model(g_ref, upd[k][r])) for r in range(world)]
        # every rank's payload first (on a copy of its state), then each rank's real aggregation
        for r in range(world):
            assert torch.equal(comps[r].global_ref, T(g_ref))
            scouts[r].global_ref.copy_(comps[r].global_ref)
            scouts[r].residual.copy_(comps[r].residual)
            scouts[r].compress(xs[r])
            q_ref, s_ref, res_ref = ic.quantise(ic.delta(xs_ref[r], g_ref, rs_ref[r]))
            assert torch.equal(scouts[r].q, T(q_ref)), (k, r, "q")
            assert torch.equal(scouts[r].scales, T(s_ref)), (k, r, "scales")
            assert torch.equal(scouts[r].residual, T(res_ref)), (k, r, "residual")
        tr.rows = {torch.int8: torch.stack([s.q for s in scouts]), torch.float32: torch.stack([s.scales for s in scouts])}
        for r in range(world):
            comps[r].aggregate(_Flat(xs[r]), transport=tr)
            assert torch.equal(comps[r].global_ref, T(g1_ref)), (k, r, "global model")
            assert torch.equal(xs[r], T(g1_ref)), (k, r, "x")
            assert torch.equal(comps[r].residual, T(rs1_ref[r])), (k, r, "residual after the round")
            assert comps[r].bytes_sent == (k + 1) * (n + 4 * ic.nchunks(n))


class _Solo:
    world = 1

    @staticmethod
    def all_gather(t):
        return t.clone().unsqueeze(0)


def test_subnormal_chunk_keeps_a_finite_residual():
    """A zero chunk with one entry of 50 * 2^-149: amax / 127 rounds to 0.  The scale must fall back to 1 (q = 0,
    the residual keeps d bit for bit); dividing by the zero scale made the residual NaN for good."""
    n, tiny = 300, 2.0 ** -149
    d0 = np.zeros(n, dtype=np.float32)
    d0[17] = 50 * tiny
    q_ref, s_ref, res_ref = ic.quantise(d0)
    assert s_ref[0] == 1.0 and not q_ref.any() and np.array_equal(res_ref, d0)
    comp = Int8Compressor(_Flat(torch.zeros(n)))
    # round 0: nothing can be sent, the update waits in the residual
    x = T(d0).clone()
    comp.aggregate(_Flat(x), transport=_Solo)
    assert comp.scales[0].item() == 1.0 and not comp.q.any()
    assert torch.equal(comp.residual, T(d0))
    assert not comp.global_ref.any() and not x.any()
    # round 1: the same update again; 100 * 2^-149 has the smallest nonzero scale and goes out whole
    x = comp.global_ref + T(d0)
    comp.aggregate(_Flat(x), transport=_Solo)
    assert comp.scales[0].item() == tiny and comp.q[17].item() == 100
    assert not comp.residual.any()
    assert comp.global_ref[17].item() == 100 * tiny and torch.isfinite(comp.global_ref).all()
    # round 2: no update, nothing pending
    comp.aggregate(_Flat(comp.global_ref.clone()), transport=_Solo)
    assert not comp.residual.any() and comp.global_ref[17].item() == 100 * tiny


@pytest.mark.parametrize("world", [1, 3])
def test_topk_twin_scatter_equals_reference(world):
    """The CPU top-k path folds the gathered (idx, val) rows into the global model rank after rank with one fma
    per entry, like scatter_add_rank_kernel."""
    n, k = 1027, 103
    gen = torch.Generator().manual_seed(11 + world)
    g0 = torch.randn(n, generator=gen)
    comps = [TopKCompressor(_Flat(g0.clone()), ratio=k / n) for _ in range(world)]
    assert comps[0].k == k
    xs = [g0 + 0.01 * torch.randn(n, generator=gen) for _ in range(world)]
    for c, x in zip(comps, xs):
        c.compress(x)
    idx = torch.stack([c.idx for c in comps])
    val = torch.stack([c.val for c in comps])
    exp = ic.scatter_add(g0.numpy(), idx.numpy(), val.numpy(), ic.f32(1.0 / world))
    tr = _Gathered(world)
    tr.rows = {torch.int32: idx, torch.float32: val}
    for r, c in enumerate(comps):
        c.residual.zero_()                                      # aggregate() compresses again from the same state
        c.aggregate(_Flat(xs[r]), transport=tr)
        assert torch.equal(c.global_ref, T(exp)), r
        assert torch.equal(xs[r], T(exp)), r
