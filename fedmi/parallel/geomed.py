"""Geometric-median aggregation (``--robust geomed``): the smoothed Weiszfeld iteration in place of FedAvg's mean.

The coordinate-wise rules of :mod:`.robust` bound every coordinate inside the honest clients' range but not the
aggregate's norm or direction.  The geometric median (RFA, Pillutla et al. 2022, "Robust Aggregation for Federated
Learning") minimises the sum of the Euclidean distances to the clients' whole models: the aggregate is a convex
combination of them (so non-negative BN statistics stay non-negative), its breakdown point is 1/2, and it reports one
weight per client.

The rule, exactly.  ``W`` clients (2..16), rank ``r`` holds ``x_r[i]``, ``i < n``, the whole ``float_state()``;
``T = --robust-iters``, ``nu = --robust-nu``.

* pass 0: ``z[i]`` = the fp32 mean over the ranks whose entry ``i`` is finite (sequential adds in rank order from 0,
  one divide by the count; NaN if none is finite);
* pass ``t``, ``1 <= t <= T``: ``s = 0``, then for ``r`` ascending ``s = fma(w_r, x_r[i], s)`` if ``w_r != 0`` else
  ``s``; ``z[i] = s``.  The select is part of the rule: a NaN row of weight 0 does not reach ``z``;
* in every pass, for every rank: ``sumsq_r = sum_i (double)(x_r[i] - z[i])^2`` (the subtraction in fp32, the sum in
  fp64, in a fixed order);
* finish after pass ``t``: ``dist_r = sqrt(sumsq_r)``, ``beta_r = 1 / max(nu, dist_r)`` if ``dist_r`` is finite else 0,
  ``B = sum beta_r`` in rank order, ``w_r = (float)(beta_r / B)`` if ``B > 0`` else ``1 / W`` (every client non-finite:
  NaN propagates as in dense FedAvg); row ``t`` of the history ``[T + 1][3][16]`` (fp64) = ``sumsq, dist, w``.

The result is ``z`` after pass ``T``: history row ``T - 1``'s ``w`` formed it, row ``T``'s ``dist`` measures it.

The float state is gathered into a persistent ``[W, ld]`` buffer (over ``torch.distributed`` by all-gather, with the
peer transport by its all-gather and a copy) and reduced by ``geomed`` (csrc/kernels/geomed.hip: ``2 (T + 1)``
launches, no host sync) on a GPU or by :func:`geomed_torch` on the CPU.  Every client computes the same bits from the
same rows.  Not built: a fused multi-pass peer kernel, and client subsampling.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Tuple

import torch

from .. import native
from .replicated import ReplicatedConfig
from .robust import MAX_RANKS, GatheredAgg

KINDS = ("geomed",)
MAX_ITERS = 64


@dataclass
class GeoMedConfig(ReplicatedConfig):
    kind: str = "geomed"
    iters: int = 8                   # --robust-iters T: weighted passes after the mean
    nu: float = 1e-6                 # --robust-nu: the smoothing floor of a client's distance

    KINDS = KINDS
    FIELDS = ("kind", "iters", "nu")
    ROLE, FLAG = "robust aggregation", "--robust / --robust-iters / --robust-nu"
    MISMATCH_TAIL = ", or the clients iterate to different aggregates and their models drift apart"

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"geometric-median aggregation: kind must be one of {KINDS}, not {self.kind!r}")
        self.iters, self.nu = int(self.iters), float(self.nu)
        if not 1 <= self.iters <= MAX_ITERS:
            raise ValueError(f"geometric-median aggregation: the iteration count must lie in 1..{MAX_ITERS}")
        if not (self.nu > 0 and math.isfinite(self.nu)):
            raise ValueError("geometric-median aggregation: nu must be a finite number > 0")


def geomed_torch(rows: torch.Tensor, iters: int, nu: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernels' twin in torch: ``rows`` is ``[W, n]`` fp32; returns ``(z[n] fp32, history[iters + 1, 3, W]
    fp64)``.  The same formulas; the fp64 sums run in torch's order, not the kernels'."""
    W, n = rows.shape
    hist = torch.zeros((iters + 1, 3, W), dtype=torch.float64, device=rows.device)
    w = None
    for t in range(iters + 1):
        z = torch.zeros(n, dtype=torch.float32, device=rows.device)
        if t == 0:
            count = torch.zeros(n, dtype=torch.float32, device=rows.device)
            for r in range(W):
                ok = torch.isfinite(rows[r])
                z = torch.where(ok, z + rows[r], z)
                count += ok
            z = z / count
        else:
            for r in range(W):
                if float(w[r]) != 0.0:                      # (the fma, up to a double rounding)
                    z = torch.addcmul(z.double(), rows[r].double(), w[r].double()).float()
        sumsq = ((rows - z).double() ** 2).sum(1)
        dist = sumsq.sqrt()
        beta = torch.where(torch.isfinite(dist), 1.0 / dist.clamp_min(nu), torch.zeros_like(dist))
        B = beta.sum()
        w = (beta / B).float() if float(B) > 0 else torch.full((W,), 1.0 / W, dtype=torch.float32, device=rows.device)
        hist[t, 0], hist[t, 1], hist[t, 2] = sumsq, dist, w.double()
    return z, hist


class GeoMedAgg(GatheredAgg):
    """The geometric-median rule in the ``robust`` slot of a :class:`fedmi.parallel.fedavg.FedAvg`, with
    :class:`fedmi.parallel.robust.RobustAgg`'s interface; ``history`` is ``[T + 1][3][16]`` of the last call."""

    def __init__(self, trainer, cfg: GeoMedConfig):
        self.history = torch.zeros((cfg.iters + 1, 3, MAX_RANKS), dtype=torch.float64,
                                   device=trainer.float_state().device)
        super().__init__(trainer, cfg, self.history)

    def _reduce(self, rows, x, W, n):
        T = self.cfg.iters
        if self._nat is not None:
            self._nat.geomed(native.stream_handle(self.dev), rows.data_ptr(), rows.shape[1], W, n, T, self.cfg.nu,
                             x.data_ptr(), self._partials(self._nat.geomed_partials(n), torch.float64).data_ptr(),
                             self.history.data_ptr())
        else:
            with torch.no_grad():
                z, hist = geomed_torch(rows[:, :n], T, self.cfg.nu)
                x.copy_(z)
                self.history[:, :, :W] = hist
        return W

    def _raw(self, W):
        return self.history[:, :, :W]

    def _decode(self, W, h) -> dict:
        """``robust_weight`` (the weights that formed the aggregate) and ``robust_dist`` (every client's distance to it)."""
        T = self.cfg.iters
        return {"robust_weight": [float(v) for v in h[T - 1, 2, :W].tolist()],
                "robust_dist": [float(v) for v in h[T, 1, :W].tolist()]}

    def round_stats(self) -> dict:
        return {**super().round_stats(), "robust_iters": self.cfg.iters}
