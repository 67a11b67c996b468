"""Shared by tests/test_client_opt.py (CPU path) and tests/test_client_opt_gpu.py (HIP kernels): seeded inputs and
the checks of the four client-optimizer operations (fedmi/parallel/client_opt.py).

SCAFFOLD.  Every output of drift_grad<scaffold>, scaffold_finish and scaffold_begin is ONE correctly rounded fp32
operation on fp32 inputs (an addition, a subtraction, an IEEE division by (float)K): no multiply sits next to an
add, so nothing can be contracted, and the result is defined bit for bit.  The checks are ``torch.equal`` against
the fp32 torch expression evaluated on the CPU.

FedProx.  The kernel computes d = fl32(p - a), then g' = fma(mu, d, g) = RN32(mu*d + g) with ONE rounding of the
exact value e = mu*d + g.  The fp64 twin computes t = RN32(RN64(e')) with e' = fp64(mu)*fp64(d) + fp64(g): the
product of two 24-bit significands is exact in fp64's 53 bits, so RN64 rounds the same exact e once, to within
2^-53 |e|.  The second rounding to fp32 can then differ from RN32(e) only when RN64 moved e onto or across an
fp32 rounding boundary (a tie point), in which case the two results are NEIGHBOURING fp32 numbers.  Hence
|g' - t| <= 1 ulp(t), with ulp(t) the spacing of fp32 above |t|; nothing else is allowed.
"""
import torch

from fedmi.parallel.client_opt import ClientOptConfig, reference_begin, reference_drift, reference_finish

BIG = 2048 * 256 * 4 + 5          # past the 2048-block grid cap: the grid-stride loop and the tail both run
SIZES = (3, 1027, BIG)            # tail only; vectors plus tail; past the grid cap
SEEDS = (0, 1, 2)
NAMES = ("g", "p", "anchor", "corr", "acc", "ci", "c", "dmean")


def draw_inputs(n: int, seed: int) -> dict:
    """fp32 CPU tensors drawn in the order of NAMES from Generator().manual_seed(2000 + seed): g, corr, ci, c
    ~ 1e-2 N(0,1); p ~ N(0,1); anchor = p + 1e-2 N(0,1); acc ~ 1e-1 N(0,1); dmean ~ 1e-3 N(0,1)."""
    gen = torch.Generator().manual_seed(2000 + seed)
    r = lambda s: s * torch.randn(n, generator=gen)   # noqa: E731
    g = r(1e-2)
    p = r(1.0)
    anchor = p + r(1e-2)
    return dict(g=g, p=p, anchor=anchor, corr=r(1e-2), acc=r(1e-1), ci=r(1e-2), c=r(1e-2), dmean=r(1e-3))


def ulp32(t: torch.Tensor) -> torch.Tensor:
    a = t.abs()
    return torch.nextafter(a, torch.full_like(a, float("inf"))) - a


def check_fedprox(mu: float, g0, p, anchor, g1) -> float:
    """``g1`` (fp32 CPU) after drift_grad<fedprox> on ``g0``: within 1 ulp of the fp64 twin.  Returns the worst
    error in ulp."""
    ref, _ = reference_drift(ClientOptConfig("fedprox", mu), g0, p, anchor, dtype=torch.float64)
    t = ref.float()
    err = (g1.double() - t.double()).abs() / ulp32(t).double()
    worst = float(err.max()) if err.numel() else 0.0
    print(f"fedprox mu={mu} n={g0.numel()}: worst {worst:.3g} ulp, {int((err > 0).sum())} entries differ")
    assert worst <= 1.0, f"fedprox: {int((err > 1.0).sum())} entries off by more than 1 ulp, worst {worst:.3g}"
    return worst


def check_scaffold_drift(g0, corr, acc0, g1, acc1) -> None:
    rg, ra = reference_drift(ClientOptConfig("scaffold"), g0, corr=corr, acc=acc0, dtype=torch.float32)
    assert torch.equal(acc1, ra), "acc != acc + g (raw gradient)"
    assert torch.equal(g1, rg), "g != g + corr"
    assert torch.equal(rg, g0 + corr) and torch.equal(ra, acc0 + g0)


def check_finish(acc, ci0, K: int, ci1, delta) -> None:
    rc, rd = reference_finish(acc, ci0, K, torch.float32)
    assert torch.equal(ci1, rc), "ci != acc / K"
    assert torch.equal(delta, rd), "delta != acc / K - ci"
    assert torch.equal(rc, acc / torch.full_like(acc, float(K)))


def check_begin(c0, dmean, ci, c1, corr, acc) -> None:
    rc, rr, _ = reference_begin(c0, dmean, ci, torch.float32)
    assert torch.equal(c1, rc), "c != c + dmean"
    assert torch.equal(corr, rr), "corr != c - ci"
    assert not acc.any(), "acc not cleared"
    assert torch.equal(rc, c0 + dmean) and torch.equal(rr, (c0 + dmean) - ci)
