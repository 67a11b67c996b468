"""Byzantine-robust aggregation: the coordinate-wise median and trimmed mean in place of FedAvg's plain mean.

A plain mean lets one client decide the global model: a diverged epoch, a NaN, a sign-flipped or scaled update
reaches every client in the same round.  The coordinate-wise trimmed mean / median (Yin et al. 2018,
"Byzantine-Robust Distributed Learning: Towards Optimal Statistical Rates") cuts, per coordinate, the ``b`` smallest
and the ``b`` largest of the ``W`` clients' values and averages the rest, so up to ``b`` arbitrary clients -- NaN
included -- cannot move a coordinate outside the honest clients' range.

The rule, exactly (the tests compare bits).  ``W`` clients, rank ``r`` holds ``x_r[i]``, ``i < n``; the whole
``float_state()`` is aggregated, BN running statistics included (a trimmed mean of non-negative values is
non-negative); the int state keeps its floor-mean.

* sort key of an fp32 ``v`` with bits ``u``: ``0xFFFFFFFF`` if ``v`` is NaN (either sign), ``u ^ 0xFFFFFFFF`` if the
  sign bit is set, ``u ^ 0x80000000`` otherwise: ``-inf < ... < -0 < +0 < ... < +inf < NaN`` as unsigned integers;
* per coordinate the ``W`` entries are ordered by ``(key, rank)`` ascending (ties to the lower rank: a total order);
* the kept window is positions ``[b_eff, W - b_eff)``, ``m = W - 2 b_eff`` entries: ``median`` has ``b_eff =
  (W - 1) // 2`` (1 entry at odd ``W``, 2 at even), ``trimmed`` with ``--robust-trim b`` has ``b_eff = min(b,
  (W - 1) // 2)`` -- a federation that shrinks after a client loss degrades towards the median and does not fail;
  ``b_eff`` is computed on the host from the current world (at ``W = 2`` nothing can be trimmed);
* result: ``s = v[b_eff]``, then ``s = s + v[j]`` in fp32 for ``j`` ascending through the window, then ``s / (float)m``
  (exact for ``m = 1``).  A NaN that survives the trim propagates, as in dense FedAvg;
* ``cut[r]`` (int64) = the number of coordinates where rank ``r``'s entry fell outside the window: the same on every
  rank, ``sum(cut) = 2 b_eff n``.  It is the operator's signal for which client is being rejected.

The fold runs over a sorted order, not over rank order or arrival order, so it is bit-identical on every rank by
construction.  With the peer transport it is ONE kernel (``peer_robust_f32_kernel``: the one-shot all-reduce with the
sum replaced by the fold); with ``torch.distributed`` the float state is all-gathered into a persistent ``[W, n]``
buffer (4 W n bytes: 358 MB for ResNet-18 at 8 clients) and reduced by ``robust_reduce`` (csrc/kernels/robust.hip) on
a GPU or by :func:`robust_reduce_torch` on the CPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.distributed as dist

from .. import native
from .replicated import ReplicatedConfig, ReplicatedState

KINDS = ("median", "trimmed")
MAX_RANKS = 16
_NAN_KEY = 0xFFFFFFFF


@dataclass
class RobustConfig(ReplicatedConfig):
    kind: str
    trim: int = 1                    # --robust-trim b (trimmed); the median ignores it

    KINDS = KINDS
    FIELDS = ("kind", "trim")
    ROLE, FLAG = "robust aggregation", "--robust / --robust-trim"
    MISMATCH_TAIL = ", or the clients fold different windows and their models drift apart"

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"robust aggregation: kind must be one of {KINDS}, not {self.kind!r}")
        self.trim = int(self.trim)
        if self.trim < 1:
            raise ValueError("robust aggregation: the trim count b must be >= 1")

    def b_eff(self, world: int) -> int:
        """The number of entries cut on either side at ``world`` clients."""
        most = (int(world) - 1) // 2
        return most if self.kind == "median" else min(self.trim, most)


def sort_key(x: torch.Tensor) -> torch.Tensor:
    """The rule's sort key of every fp32 entry, as int64 in ``[0, 2^32)``."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(u >= 0x80000000, u ^ 0xFFFFFFFF, u ^ 0x80000000)
    return torch.where(torch.isnan(x), torch.full_like(key, _NAN_KEY), key)


def robust_reduce_torch(rows: torch.Tensor, b_eff: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernels' twin in torch: ``rows`` is ``[W, n]`` fp32; returns ``(out[n], cut[W] int64)``.  A stable sort of
    the key along dim 0 orders by ``(key, rank)``; the window is folded by sequential fp32 adds and one divide."""
    W, n = rows.shape
    b = int(b_eff)
    if not 0 <= b <= (W - 1) // 2:
        raise ValueError(f"b_eff = {b} outside 0..{(W - 1) // 2} at {W} clients")
    order = torch.sort(sort_key(rows), dim=0, stable=True).indices
    v = torch.gather(rows, 0, order)
    s = v[b].clone()
    for j in range(b + 1, W - b):
        s = s + v[j]
    out = s / torch.tensor(float(W - 2 * b), dtype=torch.float32, device=rows.device)
    outside = torch.cat((order[:b], order[W - b:])).reshape(-1)
    return out, torch.bincount(outside, minlength=W).to(torch.int64)


class RobustAgg(ReplicatedState):
    """The robust rule attached to a :class:`fedmi.parallel.fedavg.FedAvg`.  Stateless: nothing is rolled back or
    handed over; the class exists so that ``resync`` compares the settings across clients and raises on the one that
    differs.  Holds the gather buffer, the cut partials and the device stats row ``cut[0..16)`` of the last call."""

    def __init__(self, trainer, cfg: RobustConfig):
        super().__init__(trainer.float_state(), cfg)
        self.stats = torch.zeros(MAX_RANKS, dtype=torch.int64, device=self.dev)
        self._rows = None                # [W, ld] gather buffer (torch.distributed path), ld = n rounded up to 4
        self._partial = None             # int64 [blocks, 16]
        self._host = self._copied = None
        if self._nat is not None:
            self._host = torch.zeros(MAX_RANKS, dtype=torch.int64).pin_memory()
            self._copied = torch.cuda.Event()
        self._flying = None              # (b_eff, world) of the stats row on its way to the host
        self._seen = None                # (b_eff, [cut]) of the newest row known on the host
        self._warned = False

    def _rolled(self) -> List[torch.Tensor]:
        return []

    def state_tensors(self) -> List[torch.Tensor]:
        return []

    def reset(self, trainer) -> None:
        pass

    def _partials(self, rows: int) -> torch.Tensor:
        if self._partial is None or self._partial.shape[0] < rows:
            self._partial = torch.zeros((max(1, rows), MAX_RANKS), dtype=torch.int64, device=self.dev)
        return self._partial

    def aggregate(self, trainer, fedavg) -> None:
        """``float_state()`` holds the client's model on entry and the robust aggregate of all clients' on return
        (the same bits on every client).  ``fedavg`` supplies the world, the transport or group, and the abort flag."""
        W = fedavg.world()
        if W < 2:
            return
        if W > MAX_RANKS:
            raise ValueError(f"robust aggregation handles at most {MAX_RANKS} clients, the federation has {W}")
        x = trainer.float_state()
        n, b = x.numel(), self.cfg.b_eff(W)
        if b == 0 and not self._warned:
            from ..utils.metrics import log

            self._warned = True
            log("robust", f"{W} clients: nothing can be trimmed (b_eff = 0), --robust {self.cfg.kind} is the plain "
                          f"mean until the federation has 3 or more")
        self._collect()                             # the previous call's row, before this one overwrites it
        tp = fedavg.transport
        if tp is not None:
            tp.allreduce_robust_(x, b, self._partials(self._nat.PEER_MAX_BLOCKS), self.stats)
        else:
            ld = (n + 3) & ~3                       # every row 16-byte aligned
            if self._rows is None or tuple(self._rows.shape) != (W, ld):
                self._rows = None                   # (the old one first: ResNet-18 at 8 clients is 358 MB)
                self._rows = torch.zeros((W, ld), dtype=torch.float32, device=self.dev)
            self._all_gather([self._rows[r, :n] for r in range(W)], x, fedavg.group, fedavg.abort)
            if self._nat is not None:
                self._nat.robust_reduce(native.stream_handle(self.dev), self._rows.data_ptr(), ld, W, n, b,
                                        x.data_ptr(), self._partials(self._nat.robust_partials(n)).data_ptr(),
                                        self.stats.data_ptr())
            else:
                with torch.no_grad():
                    out, cut = robust_reduce_torch(self._rows[:, :n], b)
                    x.copy_(out)
                    self.stats[:W] = cut
        self._flying = (b, W)
        if self._nat is not None:
            # the row reaches the host behind the launches; read at the next round's start (round_stats)
            self._host.copy_(self.stats, non_blocking=True)
            self._copied.record(torch.cuda.current_stream(self.dev))

    @staticmethod
    def _all_gather(rows, x, group, abort) -> None:
        """Rank r's ``x`` into ``rows[r]`` on every rank.  RCCL is stream-ordered; a host-blocking backend (gloo) runs
        ``async_op`` and stops waiting when ``abort`` is set, like :func:`fedmi.parallel.fedavg._run`."""
        from .fedavg import _supports_avg

        if abort is None or _supports_avg(group):
            dist.all_gather(rows, x, group=group)
            return
        from .group import wait_work

        wait_work(dist.all_gather(rows, x, group=group, async_op=True), abort, "all_gather")

    def _collect(self) -> None:
        """Pick up the last call's cut counts if they have reached the host.  Never waits."""
        if self._flying is None:
            return
        b, W = self._flying
        if self._nat is None:
            self._seen = (b, self.stats[:W].tolist())
        elif self._copied.query():
            self._seen = (b, self._host[:W].tolist())

    def round_stats(self) -> dict:
        """``robust_kind``, and ``robust_trim`` (the effective one) / ``robust_cut`` (one count per client) of the
        newest call whose stats row has reached the host (on a GPU at worst the previous round's: no sync is added)."""
        self._collect()
        rec = {"robust_kind": self.cfg.kind}
        if self._seen is not None:
            rec["robust_trim"], rec["robust_cut"] = self._seen[0], [int(c) for c in self._seen[1]]
        return rec


def add_robust_flags(ap) -> None:
    """``--robust`` and ``--robust-trim`` (fedmi.cli.client, tools/fedavg_sim.py)."""
    ap.add_argument("--robust", default="none", choices=["none", *KINDS],
                    help="Byzantine-robust aggregation (fedmi.parallel.robust): the coordinate-wise median or trimmed "
                         "mean of the clients' models replaces the plain mean; every client must pass the same settings")
    ap.add_argument("--robust-trim", type=int, default=1, metavar="B",
                    help="trimmed: cut the B smallest and the B largest values of every coordinate (at most "
                         "(clients - 1) // 2 are cut: a shrinking federation degrades towards the median)")


def check_robust_flags(a, error) -> None:
    """The flag combinations a robust rule cannot serve, each refused through ``error`` (``ArgumentParser.error``)."""
    if getattr(a, "robust", "none") == "none":
        return
    if a.robust_trim < 1:
        error("--robust-trim must be >= 1 (the number of values cut on either side of every coordinate)")
    if getattr(a, "agg", "collective") == "grpc":
        error("--robust needs --agg collective: with --agg grpc the coordinator averages the clients' models "
              "(reference peers), nothing folds them robustly")
    compress = getattr(a, "compress", None)
    if (compress is not None and compress != "none") or (compress is None and getattr(a, "compressFlag", None) == "Y"):
        error("--robust cannot be combined with compression (-c Y / --compress): the compressors aggregate sums of "
              "quantised deltas, not the clients' models")
    if getattr(a, "client_opt", "none") == "scaffold":
        error("--robust cannot be combined with --client-opt scaffold: its second collective is a plain mean that "
              "an outlier can pull")
    if getattr(a, "dp_noise", 0.0) > 0:
        error("--robust cannot be combined with --dp-noise > 0: the accounting is for the released sum, and an order "
              "statistic of individually noised updates is not a post-processing of the sum (--dp-clip alone is fine)")


def make_robust(kind: Optional[str], trainer=None, trim: int = 1) -> Optional[RobustAgg]:
    """None for ``none`` (nothing new is launched)."""
    if kind in (None, "", "none"):
        return None
    return RobustAgg(trainer, RobustConfig(kind, trim))
