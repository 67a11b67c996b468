"""The contract of state that :class:`fedmi.parallel.fedavg.FedAvg` keeps replicated across clients.

A server optimizer (:mod:`.server_opt`) and a client optimizer (:mod:`.client_opt`) both hold tensors that every
client must compute to the same bits without a server, and FedAvg and the client agent ask the same of either (the
classes below).  The DP guard (:mod:`.dp`) uses the same contract for its anchor and its settings check; its key and
draw counter are per client and deliberately outside it.  The compressors (:mod:`.compress`) stay outside: they have no snapshot and nothing of theirs is
handed over.
"""
from __future__ import annotations

import torch

from .. import native


class ReplicatedConfig:
    """Base of the optimizers' config dataclasses.  A subclass declares ``KINDS`` (index == the kernels' ``kind``
    argument), ``FIELDS`` (``"kind"`` first, then its numeric fields), and ``ROLE`` / ``FLAG`` for the messages."""

    KINDS = FIELDS = ()
    ROLE = FLAG = MISMATCH_TAIL = ""     # the tail is appended to check()'s message

    @property
    def kind_id(self) -> int:
        return self.KINDS.index(self.kind)

    def as_vector(self) -> torch.Tensor:
        """``FIELDS`` in fp64 (the kind as its id): what :meth:`FedAvg.resync` compares across clients."""
        return torch.tensor([self.kind_id, *(getattr(self, f) for f in self.FIELDS[1:])], dtype=torch.float64)

    def check(self, other: torch.Tensor, src: int) -> None:
        """Raise if rank ``src``'s :meth:`as_vector` differs from the local one, naming the first such field."""
        mine, kinds = self.as_vector(), self.KINDS
        other = other.detach().cpu().to(torch.float64)
        for i, name in enumerate(self.FIELDS):
            if float(mine[i]) != float(other[i]):
                show = (lambda t: kinds[int(t)] if 0 <= int(t) < len(kinds) else int(t)) if i == 0 else float
                raise RuntimeError(f"{self.ROLE} configuration differs from rank {src}'s in {name!r}: "
                                   f"local {show(mine[i])}, rank {src} {show(other[i])} -- every client must run "
                                   f"the same {self.FLAG} settings{self.MISMATCH_TAIL}")


class ReplicatedState:
    """Base of ``ServerOpt``, ``ClientOpt`` and ``DpGuard``, built from the trainer's flat float state ``x`` (it decides the
    device and whether the HIP kernels run).  A subclass says in ``_rolled()`` which tensors a void round must
    restore and in ``_after_rollback()`` what else it must undo, and adds ``state_tensors()`` (what a joining
    client receives from the survivors) and ``reset(trainer)`` (re-anchor on a model installed from outside)."""

    def __init__(self, x: torch.Tensor, cfg: ReplicatedConfig):
        self.cfg = cfg
        self.dev = x.device
        self._nat = native.require() if x.is_cuda else None
        self._snap = None

    def _rolled(self) -> list:
        raise NotImplementedError

    def _after_rollback(self) -> None:
        pass

    def snapshot(self) -> None:
        """Device copy of :meth:`_rolled` (the client agent takes it at the start of every round)."""
        if self._snap is None:
            self._snap = tuple(torch.empty_like(t) for t in self._rolled())
        for d, s in zip(self._snap, self._rolled()):
            d.copy_(s, non_blocking=True)

    def rollback(self) -> None:
        """Back to the last :meth:`snapshot`, bit for bit (a void round must not leave a trace in the state)."""
        if self._snap is None:
            raise RuntimeError(f"{type(self).__name__}.rollback() without a snapshot()")
        for d, s in zip(self._rolled(), self._snap):
            d.copy_(s)
        self._after_rollback()

    def check_config(self, other: torch.Tensor, src: int) -> None:
        """Raise if rank ``src``'s configuration (:meth:`ReplicatedConfig.as_vector`) differs from the local one."""
        self.cfg.check(other, src)
