"""Krum and multi-Krum aggregation (``--robust krum | multikrum``): the client nearest to its peers replaces the mean.

Krum (Blanchard et al. 2017, "Machine Learning with Adversaries: Byzantine Tolerant Gradient Descent") scores every
client by its squared distances to its nearest peers and keeps the best-scored client, or averages the best ``m``:
a whole-model guarantee from ONE sweep of the gathered buffer plus a small copy, and the metrics say which clients were
kept.

The rule, exactly.  ``W`` clients (2..16), rank ``r`` holds ``x_r[i]``, ``i < n``, the whole ``float_state()``;
``F = --robust-byz`` is the number of arbitrary clients to withstand (default 1).

* Gram: ``G[i][j] = sum_k (double)x_i[k] * (double)x_j[k]``, summed in fp64 in a fixed order that is a function of
  ``W`` and ``n`` only.  No centring row is subtracted; a client's NaN or Inf reaches only its own row and column;
* distances: for ``i != j``, ``d[i][j] = (G[i][i] + G[j][j]) - 2 G[i][j]`` (three IEEE fp64 operations in that order),
  clamped below at 0, replaced by ``+inf`` if it is not finite;
* effective counts: ``F_eff = max(0, min(F, (W - 3) // 2))``, from the current world (a shrinking federation degrades
  and does not fail, like ``b_eff``); ``k = max(1, W - F_eff - 2)``;
* scores: ``score[i]`` = the sum of the ``k`` smallest ``d[i][j]``, ``j != i``, added in fp64 in ascending ``(d, j)``
  order;
* selection: the ``m`` clients of lowest ``(score, rank)``; ``krum``: ``m = 1``; ``multikrum``: ``m = W - F_eff``;
* output: ``z[i]`` = the selected rows added in fp32 in rank order (the first selected row starts the sum), then one
  divide by ``(float)m``; ``m = 1`` is a bit-exact copy of the winner;
* non-finite inputs: a client with any non-finite entry has all its distances ``+inf``; it is selected only if fewer
  than ``m`` finite clients exist, and NaN then propagates as in dense FedAvg;
* ``stats`` is fp64 ``[18][16]``: row 0 ``score``, row 1 ``selected`` (1.0 or 0.0), rows 2..17 ``d``.

A distance carries an absolute error of at most ``4 gamma_n max_r sum_k x_r[k]^2``, ``gamma_n = n 2^-53 / (1 - n
2^-53)``: the choice can differ from exact arithmetic only between clients whose scores are closer than that.  Every
client still computes the same bits from the same rows.

The float state is gathered as for the other rules (:class:`fedmi.parallel.robust.GatheredAgg`) and reduced by ``krum``
(csrc/kernels/krum.hip: the Gram as fp64 MFMA tiles, a one-workgroup finish, a copy of the selected rows; three
launches, no host sync) on a GPU or by :func:`krum_torch` on the CPU.  Bulyan builds on the same Gram pass
(:mod:`fedmi.parallel.bulyan`).  Not built: a fused peer kernel, client subsampling, the distances from a centred Gram
(:mod:`fedmi.parallel.dnc` has the centred pass).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Tuple

import torch

from .. import native
from .replicated import ReplicatedConfig
from .robust import MAX_RANKS, GatheredAgg

KINDS = ("krum", "multikrum")
STATS_ROWS = 2 + MAX_RANKS


@dataclass
class SelectConfig(ReplicatedConfig):
    """Base of the configs of the rules that select clients by Krum's scores; a subclass names its ``KINDS`` and its
    ``RULE`` (the word in the messages) and supplies ``counts(world)``."""
    kind: str
    byz: int = 1                     # --robust-byz F: arbitrary clients to withstand

    RULE = ""
    FIELDS = ("kind", "byz")
    ROLE, FLAG = "robust aggregation", "--robust / --robust-byz"
    MISMATCH_TAIL = ", or the clients select different peers and their models drift apart"

    def __post_init__(self):
        if self.kind not in self.KINDS:
            raise ValueError(f"{self.RULE} aggregation: kind must be one of {self.KINDS}, not {self.kind!r}")
        self.byz = int(self.byz)
        if self.byz < 1:
            raise ValueError(f"{self.RULE} aggregation: the Byzantine count F must be >= 1")


@dataclass
class KrumConfig(SelectConfig):
    kind: str = "krum"

    KINDS, RULE = KINDS, "Krum"

    @property
    def multi(self) -> bool:
        return self.kind == "multikrum"

    def counts(self, world: int) -> Tuple[int, int, int]:
        return krum_counts(world, self.byz, self.multi)


def krum_counts(world: int, byz: int, multi: bool) -> Tuple[int, int, int]:
    """``(F_eff, k, m)`` at ``world`` clients."""
    f = max(0, min(int(byz), (int(world) - 3) // 2))
    return f, max(1, world - f - 2), world - f if multi else 1


def gram_torch(rows: torch.Tensor) -> torch.Tensor:
    """The symmetric ``[W, W]`` fp64 Gram matrix of ``rows`` (``[W, n]`` fp32), on the CPU, read from its upper triangle
    as the kernel reads it; the sums run in torch's order, not the kernels'."""
    x = rows.double()
    G = torch.triu(x @ x.T)
    return (G + torch.triu(G, 1).T).cpu()


def gram_select_torch(G: torch.Tensor, f: int, rounds: int, picks: int,
                      stats_rows: int = STATS_ROWS) -> Tuple[torch.Tensor, List[int]]:
    """The loop of both finish kernels (``krum_finish``: one round of ``m`` picks; ``bulyan_finish``: ``theta`` rounds of
    one): from the symmetric ``[W, W]`` Gram matrix, ``rounds`` rounds over the alive set that pick the ``picks``
    clients of lowest ``(score, rank)`` each, with ``F_eff = f``.  Returns ``stats[stats_rows,
    16]`` (fp64: row 0 the score in the client's last round alive, row 1 the round in which it was picked, rows 2..17
    ``d``, any further row 0) and the picked ranks, ascending."""
    W = G.shape[0]
    g = G.tolist()
    stats = torch.zeros((stats_rows, MAX_RANKS), dtype=torch.float64)
    d = [[0.0] * W for _ in range(W)]
    for i in range(W):
        for j in range(W):
            if i != j:
                v = (g[i][i] + g[j][j]) - 2.0 * g[i][j]
                d[i][j] = (0.0 if v < 0.0 else v) if math.isfinite(v) else math.inf
        stats[2 + i, :W] = torch.tensor(d[i], dtype=torch.float64)
    alive = list(range(W))
    for rnd in range(1, rounds + 1):
        k = max(1, len(alive) - f - 2)
        score = {}
        for i in alive:
            near = sorted((d[i][j], j) for j in alive if j != i)[:k]
            s = near[0][0] if near else 0.0
            for v, _ in near[1:]:
                s = s + v
            score[i] = s
            stats[0, i] = s
        for i in sorted(alive, key=lambda i: (score[i], i))[:picks]:
            stats[1, i] = float(rnd)
            alive.remove(i)
    return stats, [r for r in range(W) if r not in alive]


def krum_finish_torch(G: torch.Tensor, byz: int, multi: bool) -> torch.Tensor:
    """``stats[18, 16]`` (fp64) from the symmetric ``[W, W]`` Gram matrix: one round of ``m`` picks."""
    f, _, m = krum_counts(G.shape[0], byz, multi)
    return gram_select_torch(G, f, 1, m)[0]


def krum_torch(rows: torch.Tensor, byz: int, multi: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernels' twin in torch: ``rows`` is ``[W, n]`` fp32; returns ``(z[n] fp32, stats[18, 16] fp64)``.  The same
    formulas; the Gram's fp64 sums run in torch's order, not the kernels'."""
    f, _, m = krum_counts(rows.shape[0], byz, multi)
    stats, chosen = gram_select_torch(gram_torch(rows), f, 1, m)
    z = rows[chosen[0]].clone()
    for r in chosen[1:]:
        z = z + rows[r]
    return z / torch.tensor(float(len(chosen)), dtype=torch.float32, device=rows.device), stats


class SelectAgg(GatheredAgg):
    """Base of the rules built on the Gram pass and Krum's selection, in the ``robust`` slot of a
    :class:`fedmi.parallel.fedavg.FedAvg` with :class:`fedmi.parallel.robust.RobustAgg`'s interface; ``stats`` is
    ``[STATS_ROWS][16]`` (fp64) of the last call.  A subclass names its ``BINDING`` (``<BINDING>_partials(n)`` sizes its
    scratch) and its ``TWIN`` in torch; both take the rows and then :meth:`_rule_args`."""

    STATS_ROWS = STATS_ROWS
    BINDING, TWIN = "", None

    def __init__(self, trainer, cfg: SelectConfig):
        self.stats = torch.zeros((self.STATS_ROWS, MAX_RANKS), dtype=torch.float64,
                                 device=trainer.float_state().device)
        super().__init__(trainer, cfg, self.stats)

    def _rule_args(self) -> tuple:
        return (self.cfg.byz,)

    def _reduce(self, rows, x, W, n):
        if self._nat is not None:
            # one allocation; the partials are rows of 256 doubles: 16 rows of the shared [*, 16] buffer each
            blocks = MAX_RANKS * getattr(self._nat, self.BINDING + "_partials")(n)
            getattr(self._nat, self.BINDING)(native.stream_handle(self.dev), rows.data_ptr(), rows.shape[1], W, n,
                                             *self._rule_args(), x.data_ptr(),
                                             self._partials(blocks, torch.float64).data_ptr(), self.stats.data_ptr())
        else:
            with torch.no_grad():
                z, stats = self.TWIN(rows[:, :n], *self._rule_args())
                x.copy_(z)
                self.stats.copy_(stats)
        return self.cfg.counts(W)[0], W

    def _decode(self, tag, stats) -> dict:
        """``robust_byz`` (the effective one), ``robust_selected`` (the ranks picked) and ``robust_score``."""
        f_eff, W = tag
        return {"robust_byz": f_eff, "robust_selected": [r for r in range(W) if float(stats[1, r]) > 0.0],
                "robust_score": [float(v) for v in stats[0, :W].tolist()]}


class KrumAgg(SelectAgg):
    """The Krum rules; ``stats`` is ``[18][16]`` of the last call."""

    BINDING, TWIN = "krum", staticmethod(krum_torch)

    def _rule_args(self) -> tuple:
        return self.cfg.byz, self.cfg.multi
