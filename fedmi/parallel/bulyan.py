"""Bulyan aggregation (``--robust bulyan``): Krum, iterated, picks the clients; a coordinate-wise rule folds only them.

A coordinate-wise rule bounds every coordinate and says nothing about the vector; Krum bounds the vector, and an
attacker who stays close in L2 and spends all of its budget on a few coordinates is still selected -- in dimension
``n`` ~ 1e7 that budget is large (El Mhamdi, Guerraoui and Rouault 2018, "The Hidden Vulnerability of Distributed
Learning in Byzantium").  Bulyan composes the two: the selected set is Krum's, the value of every coordinate is the mean
of the selected values closest to their median.

The rule, exactly.  ``W`` clients (2..16), rank ``r`` holds ``x_r[i]``, ``i < n``, the whole ``float_state()``;
``F = --robust-byz``.

* counts: ``F_eff = max(0, min(F, (W - 3) // 4))`` from the current world, ``theta = W - 2 F_eff`` clients selected,
  ``c = 2 F_eff`` values cut per coordinate, ``beta = theta - c`` kept.  Below 7 clients ``F_eff = 0``: everyone is
  selected, nothing is cut, the aggregate is the plain mean in sorted order;
* Gram and distances: exactly Krum's (:mod:`fedmi.parallel.krum`), ``d[i][j] == d[j][i]`` bit for bit;
* selection: the alive set ``A`` starts as all clients; ``theta`` rounds.  In each, ``k = max(1, |A| - F_eff - 2)``,
  ``score[i]`` for ``i`` in ``A`` is the sum of the ``k`` smallest ``d[i][j]``, ``j`` in ``A \\ {i}``, added in fp64 in
  ascending ``(d, j)`` order (a lone client scores 0.0), and the client of lowest ``(score, rank)`` is picked and
  leaves ``A``;
* fold, per coordinate, over the selected rows: order the ``theta`` values by ``(sort key, rank)`` as the
  coordinate-wise rules do, ``v[0..theta)``; ``med = v[theta / 2]`` (odd) or ``(v[theta/2 - 1] + v[theta/2]) / 2`` in
  fp32 (even); ``dist_p`` = the sort key of ``|v[p] - med|`` (fp32); the window starts as ``[0, theta - 1]`` and ``c``
  times drops its high end if ``dist_hi >= dist_lo``, else its low end; the result is the window added in fp32 in
  position order (the first kept value starts the sum), then one divide by ``(float)beta``.  NaN sorts last and its
  distance key is the largest: up to ``c`` non-finite values per coordinate are dropped first, a surviving NaN
  propagates as in dense FedAvg;
* ``stats`` is fp64 ``[19][16]``: row 0 the score with which a client was picked (never picked: its score in the last
  round), row 1 the round in which it was picked (1-based, 0 = never), rows 2..17 ``d``, row 18 ``cut[r]`` = the number
  of coordinates at which selected client ``r``'s value was dropped (0 for an unselected client).

The float state is gathered as for the other rules (:class:`fedmi.parallel.robust.GatheredAgg`) and reduced by
``bulyan`` (csrc/kernels/bulyan.hip: Krum's Gram pass, a one-workgroup finish that runs all rounds from LDS, the row
sweep over the selected rows, the cut counts' fold; four launches, no host sync) on a GPU or by :func:`bulyan_torch` on
the CPU.  Not built: a fused peer kernel, a centred Gram, client subsampling, Bulyan over compressed deltas or
SCAFFOLD's variate.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import torch

from .krum import SelectAgg, SelectConfig, gram_select_torch, gram_torch
from .robust import MAX_RANKS, sort_key

KINDS = ("bulyan",)
STATS_ROWS = 3 + MAX_RANKS
CUT_ROW = 2 + MAX_RANKS


@dataclass
class BulyanConfig(SelectConfig):
    kind: str = "bulyan"

    KINDS, RULE = KINDS, "Bulyan"

    def counts(self, world: int) -> Tuple[int, int, int, int]:
        return bulyan_counts(world, self.byz)


def bulyan_counts(world: int, byz: int) -> Tuple[int, int, int, int]:
    """``(F_eff, theta, c, beta)`` at ``world`` clients."""
    f = max(0, min(int(byz), (int(world) - 3) // 4))
    return f, world - 2 * f, 2 * f, world - 4 * f


def bulyan_select_torch(G: torch.Tensor, byz: int) -> Tuple[torch.Tensor, List[int]]:
    """``stats[19, 16]`` (fp64, row 18 still 0) and the selected ranks, ascending, from the symmetric ``[W, W]`` Gram."""
    f, theta, _, _ = bulyan_counts(G.shape[0], byz)
    return gram_select_torch(G, f, theta, 1, STATS_ROWS)


def bulyan_fold_torch(rows: torch.Tensor, c: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The fold of ``rows`` (``[theta, n]`` fp32, the selected clients in rank order) with ``c`` values cut per
    coordinate: ``(out[n] fp32, cut[theta] int64)``."""
    theta, n = rows.shape
    beta = theta - int(c)
    if c < 0 or beta < 1:
        raise ValueError(f"c = {c} outside 0..{theta - 1} at {theta} selected clients")
    order = torch.sort(sort_key(rows), dim=0, stable=True).indices
    v = torch.gather(rows, 0, order)
    two = torch.tensor(2.0, dtype=torch.float32, device=rows.device)
    med = v[theta // 2] if theta % 2 else (v[theta // 2 - 1] + v[theta // 2]) / two
    dist = sort_key((v - med).abs())
    lo = torch.zeros((1, n), dtype=torch.int64, device=rows.device)
    hi = torch.full((1, n), theta - 1, dtype=torch.int64, device=rows.device)
    for _ in range(int(c)):
        drop_hi = torch.gather(dist, 0, hi) >= torch.gather(dist, 0, lo)
        hi = hi - drop_hi.to(torch.int64)
        lo = lo + (~drop_hi).to(torch.int64)
    s = torch.gather(v, 0, lo)[0]
    for t in range(1, beta):
        s = s + torch.gather(v, 0, lo + t)[0]
    out = s / torch.tensor(float(beta), dtype=torch.float32, device=rows.device)
    pos = torch.arange(theta, device=rows.device)[:, None]
    outside = order[(pos < lo) | (pos > hi)]
    return out, torch.bincount(outside, minlength=theta).to(torch.int64)


def bulyan_torch(rows: torch.Tensor, byz: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernels' twin in torch: ``rows`` is ``[W, n]`` fp32; returns ``(z[n] fp32, stats[19, 16] fp64)``.  The same
    formulas; the Gram's fp64 sums run in torch's order, not the kernels'."""
    stats, selected = bulyan_select_torch(gram_torch(rows), byz)
    z, cut = bulyan_fold_torch(rows[selected], bulyan_counts(rows.shape[0], byz)[2])
    stats[CUT_ROW, selected] = cut.cpu().double()
    return z, stats


class BulyanAgg(SelectAgg):
    """Bulyan; ``stats`` is ``[19][16]`` of the last call."""

    STATS_ROWS = STATS_ROWS
    BINDING, TWIN = "bulyan", staticmethod(bulyan_torch)

    def _run(self, x, W, fedavg):
        if self.cfg.counts(W)[0] == 0:
            self._log_once(f"{W} clients: nothing can be withstood (F_eff = 0), --robust bulyan selects everyone and is "
                           f"the plain mean until the federation has 7 or more")
        return super()._run(x, W, fedavg)

    def _decode(self, tag, stats) -> dict:
        """:class:`fedmi.parallel.krum.SelectAgg`'s keys and ``robust_cut`` (per client, the coordinates at which its
        value was dropped)."""
        return {**super()._decode(tag, stats), "robust_cut": [int(v) for v in stats[CUT_ROW, :tag[1]].tolist()]}
