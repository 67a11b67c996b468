"""Divide-and-Conquer aggregation (``--robust dnc``): clients that stand out along the top principal direction are dropped.

The coordinate-wise rules judge a client by coordinate ranks, Krum and Bulyan by pairwise L2 distances.  Colluding
attackers that stay inside the honest clients' spread and all push in ONE common direction ("a little is enough", the
Fang-style attacks) pass both.  DnC (Shejwalkar and Houmansadr 2021, "Manipulating the Byzantine: Optimizing Model
Poisoning Attacks and Defenses for Federated Learning") is the spectral answer: score every client by its squared
projection on the top principal direction of the centred updates and drop the highest scores.  With at most 16 clients
that direction is fully determined by the ``W x W`` centred Gram matrix: no coordinate subsampling, no SVD of anything
large -- one sweep of the gathered buffer on the fp64 matrix cores, a tiny eigen-solve, the mean of the kept rows.

The rule, exactly.  ``W`` clients (2..16), rank ``r`` holds ``x_r[k]``, ``k < n``, the whole ``float_state()``;
``F = --robust-byz``.

* counts: ``F_eff = max(0, min(F, (W - 1) // 2))`` from the current world, ``m = W - F_eff`` clients are kept.  At
  ``W = 2`` nothing is removed, and the client says so once;
* column pivot: ``p[k]``, an fp32 value that is the same for all clients of column ``k``: the fp32 sum of the clients'
  entries (a non-finite entry contributing 0) in the fixed cross-lane order, times ``1 / W``; 0 if that sum is not
  finite.  The pivot only has to be near the mean: the finish removes what is left of the common part, so the pivot's
  rounding never enters the result's meaning;
* centred Gram: ``y_r[k] = (double)x_r[k] - (double)p[k]`` (a non-finite ``x`` stays non-finite and reaches only its own
  row and column), ``G[i][j] = sum_k y_i[k] * y_j[k]`` in fp64, in an order that is a function of ``W`` and ``n`` only;
* finish.  A client is *bad* if ``G[i][i]`` is not finite; ``A`` is the set of the others.  Every sum below runs from
  0.0 in ascending index order, every operation is one IEEE fp64 operation, nothing is contracted:

  - double-centring over ``A``: ``rbar_i`` = the sum of ``G[i][j]``, ``j`` in ``A``, divided by ``|A|``; ``gbar`` = the
    sum of the ``rbar_i`` divided by ``|A|``; for ``i <= j`` in ``A``, ``C[i][j] = ((G[i][j] - rbar_i) - rbar_j) +
    gbar`` and ``C[j][i]`` is the same number; ``C`` is 0 outside ``A x A``;
  - top eigenvector by repeated squaring: ``B = C / tr C``, then 12 times ``B <- B B / tr(B B)``; what is left of the
    second eigenvector is ``(lambda_2 / lambda_1)^4096``.  ``u`` is the column of ``B`` with the largest diagonal entry,
    ties to the lower rank;
  - ``score_i = ((C u)_i)^2 / (u^T C u)``: the squared projection of ``y_i - ybar`` on the unit vector ``Y_c^T u /
    |Y_c^T u|``, whatever ``u`` is.  A NaN (an overflow) counts as ``+inf``; if ``u^T C u`` is not positive the score
    is 0;
  - if ``tr C`` is not positive and finite, or ``|A| < 2``, every score in ``A`` is 0.  A bad client's score is ``+inf``;

* selection: the ``m`` clients of lowest ``(score, rank)``;
* output: the selected rows added in fp32 in rank order (the first selected row starts the sum), then one divide by
  ``(float)m`` -- Krum's select.  A bad client is kept only if fewer than ``m`` finite clients exist, and NaN then
  propagates as in dense FedAvg;
* ``stats`` is fp64 ``[18][16]``: row 0 ``score``, row 1 ``selected`` (1.0 or 0.0), rows 2..17 ``C``.

An entry of the centred Gram carries an error of about ``gamma_n sum_k |y_i[k] y_j[k]|`` -- of the clients'
DIFFERENCES.  The uncentred ``G = X X^T`` that Krum and Bulyan use carries ``gamma_n sum_k |x_i[k] x_j[k]|``, of the
whole models: federated models share a common part that dwarfs their differences.  With a common part 1e4 times the
differences the uncentred bound is 1e6 times the centred one (still below the entries: 0.037 of the largest at 2 M
entries), and a spectral rule reads the small eigen-gaps of exactly those entries.

The float state is gathered as for the other rules (:class:`fedmi.parallel.robust.GatheredAgg`) and reduced by ``dnc``
(csrc/kernels/dnc.hip: the centred Gram as fp64 MFMA tiles with the pivot formed in registers across lanes, a
one-workgroup finish, Krum's mean of the selected rows; three launches, no host sync) on a GPU or by :func:`dnc_torch` on
the CPU.  Not built: a fused peer kernel, coordinate subsampling, several DnC iterations, Krum or Bulyan on the centred
Gram.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Tuple

import torch

from .krum import STATS_ROWS, SelectAgg, SelectConfig
from .robust import MAX_RANKS

KINDS = ("dnc",)
SQUARINGS = 12


@dataclass
class DncConfig(SelectConfig):
    kind: str = "dnc"

    KINDS, RULE = KINDS, "DnC"

    def counts(self, world: int) -> Tuple[int, int]:
        return dnc_counts(world, self.byz)


def dnc_counts(world: int, byz: int) -> Tuple[int, int]:
    """``(F_eff, m)`` at ``world`` clients."""
    f = max(0, min(int(byz), (int(world) - 1) // 2))
    return f, world - f


def centred_gram_torch(rows: torch.Tensor) -> torch.Tensor:
    """The symmetric ``[W, W]`` fp64 Gram matrix of ``rows`` (``[W, n]`` fp32) minus their column pivot, on the CPU,
    read from its upper triangle as the kernel reads it.  The pivot is the fp64 mean with non-finite entries counting 0,
    and the sums run in torch's order: other last bits than the kernel's."""
    x = rows.double()
    p = torch.where(torch.isfinite(x), x, torch.zeros_like(x)).sum(0) / x.shape[0]
    y = x - torch.where(torch.isfinite(p), p, torch.zeros_like(p))
    G = torch.triu(y @ y.T)
    return (G + torch.triu(G, 1).T).cpu()


def dnc_finish_torch(G: torch.Tensor, byz: int) -> Tuple[torch.Tensor, List[int]]:
    """The finish kernel in Python floats (IEEE fp64, one rounding per operation, the kernel's order): from the
    symmetric ``[W, W]`` centred Gram matrix, ``stats[18, 16]`` (fp64) and the selected ranks, ascending."""
    W, R = G.shape[0], MAX_RANKS
    m = dnc_counts(W, byz)[1]
    g = G.tolist()
    A = [i for i in range(W) if math.isfinite(g[i][i])]
    rbar = [0.0] * R
    for i in A:
        s = 0.0
        for j in A:
            s = s + g[min(i, j)][max(i, j)]
        rbar[i] = s / len(A)
    gbar = 0.0
    for i in A:
        gbar = gbar + rbar[i]
    if A:
        gbar = gbar / len(A)
    C = [[0.0] * R for _ in range(R)]
    for i in A:
        for j in A:
            if i <= j:
                C[i][j] = C[j][i] = ((g[i][j] - rbar[i]) - rbar[j]) + gbar
    score = [0.0] * R
    tr = _trace(C)
    if len(A) >= 2 and 0.0 < tr < math.inf:
        B = [[c / tr for c in row] for row in C]
        for _ in range(SQUARINGS):
            T = [[_dot(B[i], [B[o][j] for o in range(R)]) for j in range(R)] for i in range(R)]
            tt = _trace(T)
            B = [[v / tt for v in row] for row in T]
        top = 0
        for o in range(1, W):
            if B[o][o] > B[top][top]:
                top = o
        u = [B[o][top] for o in range(R)]
        cu = [_dot(C[i], u) for i in range(R)]
        den = _dot(u, cu)
        for i in range(R):
            s = (cu[i] * cu[i]) / den if den > 0.0 else 0.0
            score[i] = s if s == s else math.inf
    for i in range(W):
        if i not in A:
            score[i] = math.inf
    selected = sorted(sorted(range(W), key=lambda r: (score[r], r))[:m])
    stats = torch.zeros((STATS_ROWS, R), dtype=torch.float64)
    stats[0, :W] = torch.tensor(score[:W], dtype=torch.float64)
    stats[1, selected] = 1.0
    stats[2:] = torch.tensor(C, dtype=torch.float64)
    return stats, selected


def _dot(a, b) -> float:
    s = 0.0
    for x, y in zip(a, b):
        s = s + x * y
    return s


def _trace(M) -> float:
    s = 0.0
    for o in range(len(M)):
        s = s + M[o][o]
    return s


def dnc_torch(rows: torch.Tensor, byz: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernels' twin in torch: ``rows`` is ``[W, n]`` fp32; returns ``(z[n] fp32, stats[18, 16] fp64)``.  The same
    formulas; the pivot and the Gram's fp64 sums are torch's, not the kernels'."""
    stats, chosen = dnc_finish_torch(centred_gram_torch(rows), byz)
    z = rows[chosen[0]].clone()
    for r in chosen[1:]:
        z = z + rows[r]
    return z / torch.tensor(float(len(chosen)), dtype=torch.float32, device=rows.device), stats


class DncAgg(SelectAgg):
    """Divide-and-Conquer; ``stats`` is ``[18][16]`` of the last call."""

    BINDING, TWIN = "dnc", staticmethod(dnc_torch)

    def _run(self, x, W, fedavg):
        if self.cfg.counts(W)[0] == 0:
            self._log_once(f"{W} clients: nothing can be removed (F_eff = 0), --robust dnc keeps everyone and is the "
                           f"plain mean until the federation has 3 or more")
        return super()._run(x, W, fedavg)
