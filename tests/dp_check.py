"""Shared by tests/test_dp.py (CPU path) and tests/test_dp_gpu.py (HIP kernels, csrc/kernels/dp.hip): inputs, known
answers and the derived bounds of the DP-FedAvg step against its fp64 twin (fedmi.parallel.dp).

Bounds (derived, not measured).

``sumsq``.  d = x - a is formed in fp32 on both sides and its square is exact in fp64 (24 + 24 <= 53 bits), so the
device and the twin add the same n exact terms, all >= 0, in different orders.  Reordering an fp64 sum of n such terms
moves it by at most n * 2^-53 relative (SUMSQ_REL).

``scale``.  norm = sqrt(sumsq) and S / norm are correctly rounded fp64 operations on a sumsq that differs by the above,
then one rounding to fp32: the two fp32 results are equal or neighbours (1 ulp).

Clip.  y = fma(scale, d, a) with the DEVICE's scale is one fp32 rounding of the exact scale * d + a; the fp64 twin
rounds the same exact value once to within 2^-53 and then to fp32, which can differ from the single rounding only by
landing on the neighbouring fp32 number (the argument of tests/client_opt_check.py): 1 ulp, nothing else.  The
distance of the clipped x from the anchor is S up to the rounding of scale (2^-24 relative) and the fma's rounding
e_i of every entry (<= half an ulp of x_i <= 2^-24 |x_i|): at worst S (1 + 2^-24) + 2^-24 ||x||.  The result has to be
an fp32 number near x, so this is a property of the format, not of the kernel, and the issue's CLIP_SLACK = 1 + 2^-20
can hold for every sign of the roundings only where 2^-24 ||x|| <= (2^-20 - 2^-24) S, i.e. ||x|| <= 15 S.
draw_inputs keeps the weights within that: ||x|| ~ 3.2 ||d|| and the tests clip at S = 0.37 ||d||, so ||x|| ~ 8.6 S
(a three-entry case cannot count on the roundings cancelling).  The end-to-end tests run real weights, where the
roundings of tens of thousands of entries enter the norm in quadrature and the same bound holds with room.

Noise, GAUSS_ABS.  g = radius * trig with radius = sqrtf(-2 * logf(u0)) <= sqrt(-2 ln 2^-24) = 5.77 and |trig| <= 1.
u0, u1 and 2 * u1 are exact in fp32.  With e = 2^-24 (half an ulp, relative) and the usual library bounds of 1 ulp for
logf, 1 ulp for sqrtf and 2 ulp for sincospif (no table of ROCm's own bounds is installed beside the toolchain, so
these are assumed, generously: sqrtf is correctly rounded in practice):
    -2 * logf(u0):  relative 2e (the multiplication by 2 is exact);   sqrtf of it:  e from the argument + 2e
    trig:           absolute 4e  (2 ulp of a value <= 1)
    the product:    one more rounding, e
so |g - g64| <= 5.77 * (3e + 4e + e) = 5.77 * 8 * 2^-24 = 2.8e-6.  A kernel that goes through sincosf(2 pi u1)
instead adds half an ulp of the angle (<= 6.28): 6.28 * 2^-24 * 5.77 = 2.2e-6, together 5e-6.  The issue's bound is
1e-5 absolute; any wrong Philox round, lane order or tail index misses it by five orders of magnitude.

Moments of n standard normal draws: the mean has std 1/sqrt(n), the sample variance sqrt(2/n); five sigma each.
"""
import math

import torch

from fedmi.parallel.dp import DpConfig, reference_privatize

BIG = 2048 * 256 * 4 + 5          # past the 2048-block grid cap: the grid-stride loops and the tail both run
# (n, k): tail only; vectors plus tail; nothing to do; a vector straddling k; past the grid cap
SHAPES = [(3, 3), (1027, 1027), (1027, 0), (1500, 1001), (BIG, BIG)]

# Philox4x32-10 known answers (Salmon et al. 2011, Random123 kat_vectors): counter, key, output
PHILOX_KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

CLIP_SLACK = 1.0 + 2.0 ** -20
GAUSS_ABS = 1e-5
GAUSS_MAX = math.sqrt(-2.0 * math.log(2.0 ** -24))      # 5.77: u >= 2^-24


def sumsq_rel(n: int) -> float:
    return n * 2.0 ** -53


def mean_bound(n: int) -> float:
    return 5.0 / math.sqrt(n)


def var_bound(n: int) -> float:
    return 5.0 * math.sqrt(2.0 / n)


def draw_inputs(n: int, seed: int = 0):
    """anchor ~ 3e-2 N(0, 1); x = anchor + 1e-2 N(0, 1), drawn in this order from Generator().manual_seed(2000 + seed):
    an update of norm about 1e-2 * sqrt(n) on weights three times as large (see CLIP_SLACK above)."""
    g = torch.Generator().manual_seed(2000 + seed)
    anchor = 3e-2 * torch.randn(n, generator=g)
    x = anchor + 1e-2 * torch.randn(n, generator=g)
    return x, anchor


def update_norm(x: torch.Tensor, anchor: torch.Tensor, k: int) -> float:
    """The twin's norm: ``sqrt(((x - a).float().double()^2).sum())`` over the first k entries."""
    return math.sqrt(float(((x[:k].float() - anchor[:k].float()).double() ** 2).sum())) if k else 0.0


def ulp32(t: torch.Tensor) -> torch.Tensor:
    a = t.abs()
    return torch.nextafter(a, torch.full_like(a, float("inf"))) - a


def check_stats(x0, anchor, k: int, clip: float, stats) -> float:
    """``stats`` = (sumsq, norm, scale) of the step under test on (x0, anchor): sumsq within SUMSQ_REL of the twin's,
    scale within 1 fp32 ulp of ``(float)(S / norm)``.  Returns the device's scale."""
    sumsq, norm, scale = (float(v) for v in stats[:3])
    want = float(((x0[:k].float() - anchor[:k].float()).double() ** 2).sum()) if k else 0.0
    rel = abs(sumsq - want) / want if want else abs(sumsq)
    print(f"sumsq k={k}: device {sumsq!r} twin {want!r} rel {rel:.3g} (bound {sumsq_rel(max(k, 1)):.3g})")
    assert rel <= sumsq_rel(max(k, 1)), (sumsq, want, rel)
    wn = math.sqrt(want)
    assert abs(norm - wn) <= 2.0 * sumsq_rel(max(k, 1)) * wn + 2.0 ** -52 * wn, (norm, wn)
    ws = torch.tensor(clip / wn if wn > clip else 1.0, dtype=torch.float64).float()
    got = torch.tensor(scale, dtype=torch.float64)
    assert float(got.float()) == scale, "scale is not an fp32 value"
    assert abs(scale - float(ws)) <= float(ulp32(ws)), (scale, float(ws))
    return scale


def check_clip(x0, anchor, x1, k: int, cfg: DpConfig, scale: float) -> float:
    """``x1`` after a clip-only step (z = 0) on ``x0`` with the step's own ``scale``: the first k entries within 1 ulp
    of the fp64 twin (bit for bit when nothing was clipped), the rest untouched, and the result no farther than
    S * CLIP_SLACK from the anchor.  Returns the worst error in ulp."""
    assert torch.equal(x1[k:], x0[k:]), "entries at or past k changed"
    if scale == 1.0:
        assert torch.equal(x1, x0), "an unclipped update was rewritten"
        return 0.0
    ref, _, _, _ = reference_privatize(x0, anchor, k, DpConfig(cfg.clip, 0.0), 1, 0, 0, scale=scale)
    t = ref[:k].float()
    err = (x1[:k].double() - t.double()).abs() / ulp32(t).double()
    worst = float(err.max())
    print(f"clip k={k} scale={scale!r}: worst {worst:.3g} ulp, {int((err > 0).sum())} entries differ")
    assert worst <= 1.0, f"{int((err > 1.0).sum())} entries off by more than 1 ulp, worst {worst:.3g}"
    dist = update_norm(x1, anchor, k)
    assert dist <= cfg.clip * CLIP_SLACK, (dist, cfg.clip)
    return worst
