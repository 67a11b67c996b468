"""Shared by tests/test_server_opt.py (CPU path) and tests/test_server_opt_gpu.py (HIP kernel): inputs and the
derived error bounds of one server-optimizer step against its fp64 twin.

Bounds (derived, not measured).  Each output is a chain of fewer than 8 fp32 roundings of <= 0.5 ulp each,
i.e. <= 4 ulp before counting that the device sqrt / division need not be correctly rounded; 16 ulp (2e-6) of
the SUM OF THE MAGNITUDES of the terms that form an output is allowed -- not of the output itself, because the
sums can cancel:

    |m - m64| <= 2e-6 * (|beta1*m_prev| + |c*d|)             c = 1 (fedavgm) or 1 - beta1
    |v - v64| <= 2e-6 * (|v_prev| + d*d)
    |x - x64| <= 2e-6 * (|anchor| + |step|) + the m / v bounds propagated through step = lr*m/(sqrt(v)+tau):
                 lr*Em/(sqrt(v)+tau) + |step|/(sqrt(v)+tau) * Ev/(2*sqrt(v))      (first order; Ev/v <= 2e-4 here)

The twin runs on the SAME fp32 state the step under test started from, so every step is judged on its own.

FedYogi's sgn(v - d*d) may legitimately differ between fp32 and fp64 where the two are nearly equal (FMA
contraction decides), so entries with |v_prev - d*d| <= 1e-5*(v_prev + d*d) are left out; the callers cap
the share left out at 0.1 % per case.
"""
import torch

from fedmi.parallel.server_opt import ServerOptConfig, reference_step

ULP16 = 2e-6
YOGI_BAND = 1e-5
YOGI_MAX_SHARE = 1e-3


def draw_inputs(n: int, seed: int):
    """anchor ~ N(0,1); x = anchor + 1e-2 N(0,1); m = 1e-2 N(0,1); v ~ U(1e-6, 1e-3), drawn in this order from
    Generator().manual_seed(1000 + seed).  The generator is returned: :func:`next_round` continues it."""
    g = torch.Generator().manual_seed(1000 + seed)
    anchor = torch.randn(n, generator=g)
    x = anchor + 1e-2 * torch.randn(n, generator=g)
    m = 1e-2 * torch.randn(n, generator=g)
    v = 1e-6 + (1e-3 - 1e-6) * torch.rand(n, generator=g)
    return x, anchor, m, v, g


def next_round(x: torch.Tensor, g: torch.Generator) -> torch.Tensor:
    """The next aggregation's mean: the new global model plus another 1e-2 N(0,1) of client progress (after a
    step anchor == x, so without it the second and third steps would see a zero pseudo-gradient)."""
    return x + 1e-2 * torch.randn(x.numel(), generator=g)


def _f32(s: float) -> float:
    return float(torch.tensor(s, dtype=torch.float32))


def check_step(cfg: ServerOptConfig, pre, post, n_opt: int) -> torch.Tensor:
    """``pre`` / ``post``: (x, anchor, m, v) as fp32 CPU tensors before / after ONE step (v may be None for
    fedavgm).  Asserts the bounds above on the entries < n_opt, and bit-exactly that the entries >= n_opt of x,
    m, v are untouched and anchor == x everywhere.  Returns the mask of FedYogi entries left out."""
    x0, a0, m0, v0 = pre
    x1, a1, m1, v1 = post
    k = int(n_opt)
    assert torch.equal(a1, x1), "anchor != x after the step"
    assert torch.equal(x1[k:], x0[k:]), "entries >= n_opt of x changed"
    assert torch.equal(m1[k:], m0[k:]), "entries >= n_opt of m changed"
    if v0 is not None and v1 is not None:
        assert torch.equal(v1[k:], v0[k:]), "entries >= n_opt of v changed"
    adaptive = cfg.kind != "fedavgm"
    if not adaptive and v0 is not None and v1 is not None:
        assert torch.equal(v1, v0), "fedavgm wrote v"
    rx, _, rm, rv = reference_step(x0, a0, m0, v0 if adaptive else None, k, cfg, torch.float64)
    lr, b1, tau = _f32(cfg.lr), _f32(cfg.beta1), _f32(cfg.tau)
    a = a0[:k].double()
    d = x0[:k].double() - a
    c = (1.0 - b1) if adaptive else 1.0
    em = ULP16 * ((b1 * m0[:k].double()).abs() + (c * d).abs())
    step = rx[:k] - a
    out = torch.zeros(k, dtype=torch.bool)
    if adaptive:
        vp = v0[:k].double()
        dd = d * d
        if cfg.kind == "fedyogi":
            out = (vp - dd).abs() <= YOGI_BAND * (vp + dd)
        ev = ULP16 * (vp.abs() + dd)
        den = torch.sqrt(rv[:k]) + tau
        ex = ULP16 * (a.abs() + step.abs()) + lr * em / den + step.abs() / den * ev / (2.0 * torch.sqrt(rv[:k]))
        bad = ((v1[:k].double() - rv[:k]).abs() > ev) & ~out
        assert not bad.any(), f"v: {int(bad.sum())} entries off, worst ratio {float(((v1[:k].double() - rv[:k]).abs() / ev)[~out].max()):.3g}"
    else:
        ex = ULP16 * (a.abs() + step.abs()) + lr * em
    keep = ~out
    for name, got, ref, bound in (("m", m1, rm, em), ("x", x1, rx, ex)):
        err = (got[:k].double() - ref[:k]).abs()
        bad = (err > bound) & keep
        assert not bad.any(), f"{name}: {int(bad.sum())} entries off, worst ratio {float((err / bound)[keep].max()):.3g}"
    return out
