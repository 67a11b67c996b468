"""Client-side drift correction inside the local SGD step: FedProx and SCAFFOLD.

With a few labels per client the damage is done during the local epoch: every client's iterates walk toward
its own optimum, and the mean of those end points is not the federation's optimum.  A server optimizer
(:mod:`fedmi.parallel.server_opt`) only rescales that biased mean; these two act on the gradient each SGD step
consumes, between the backward pass and the engine's unchanged SGD tail.  For every trainable entry, in fp32::

    fedprox  (Li et al. 2020)           every step:   g = fma(mu, w - anchor, g)      anchor = the round's start
    scaffold (Karimireddy et al. 2020)  every step:   acc = acc + g;   g = g + corr   corr = c - c_i
                                 before the collective:   new = acc / K;   delta = new - c_i;   c_i = new
                                  after the collective:   c = c + mean(delta);   corr = c - c_i;   acc = 0

``c_i`` is the mean of the round's K *raw* gradients.  The paper's option II, ``(w_global - y_K) / (K*lr)``,
equals that mean only for plain SGD; fedmi's clients run momentum that persists across rounds, which would
inflate it by up to ``1/(1 - momentum)``.  Summing ``g`` in the pass that already reads it is exact for any
optimizer.

``delta`` travels as a second dense all-reduce per round (:meth:`FedAvg.average`); its mean is the same bits on
every rank, so ``c`` stays replicated without a server.  All clients take part in every round here, so
``c = mean(c_i)`` up to rounding; the ``c_i`` of a client that is lost stays inside ``c``.

On a GPU the four launches are HIP kernels (csrc/kernels/client_opt.hip) on the trainer's stream -- the per-step
one is captured into the engine's step graph; elsewhere the same operations run in torch.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from .. import native
from .replicated import ReplicatedConfig, ReplicatedState

KINDS = ("fedprox", "scaffold")      # index == the kernels' ``kind`` argument


def _f32(s: float) -> float:
    return float(torch.tensor(s, dtype=torch.float32))


@dataclass
class ClientOptConfig(ReplicatedConfig):
    kind: str
    mu: float = 0.01                 # FedProx's proximal weight (unused by scaffold)

    KINDS = KINDS
    FIELDS = ("kind", "mu")
    ROLE, FLAG = "client optimizer", "--client-opt"

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"unknown client optimizer {self.kind!r} (one of {', '.join(KINDS)})")
        self.mu = float(self.mu)
        if not self.mu >= 0:
            raise ValueError("client optimizer: mu must be >= 0")


def fma32(a: float, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``RN32(a*x + y)`` for an fp32 scalar ``a`` and fp32 tensors, with ONE rounding like the kernel's fma.

    In fp64 the product of two fp32 numbers is exact; TwoSum gives the sum's rounding error exactly.  Where the
    sum is inexact the fp64 value is replaced by its odd neighbour on the side of the exact value (round to odd),
    after which the rounding to fp32 cannot be a double rounding (53 >= 2*24 + 2 bits)."""
    s = _f32(a) * x.double()
    g = y.double()
    hi = s + g
    bb = hi - s
    lo = (s - (hi - bb)) + (g - bb)
    toward = torch.where(lo > 0, torch.full_like(hi, float("inf")), torch.full_like(hi, float("-inf")))
    odd = (hi.view(torch.int64) & 1).bool()
    return torch.where((lo == 0) | odd, hi, torch.nextafter(hi, toward)).float()


# ---- the four operations in plain torch at a chosen dtype (inputs untouched) --------------------------------------
def reference_drift(cfg: ClientOptConfig, g: torch.Tensor, p: Optional[torch.Tensor] = None,
                    anchor: Optional[torch.Tensor] = None, corr: Optional[torch.Tensor] = None,
                    acc: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.float64):
    """One per-step correction: returns ``(g, acc)`` (``acc`` None for fedprox).

    fedprox: ``d = p - anchor`` is formed in fp32 as the kernel forms it (one rounding, part of the definition),
    then ``mu*d + g`` at ``dtype`` with ``mu`` rounded to fp32 first (it reaches the kernel as an fp32 argument).
    At fp64 the product is exact, so the result rounded to fp32 is the kernel's fma up to double rounding."""
    if cfg.kind == "fedprox":
        d = (p.float() - anchor.float()).to(dtype)
        return _f32(cfg.mu) * d + g.to(dtype), None
    return g.to(dtype) + corr.to(dtype), acc.to(dtype) + g.to(dtype)


def reference_finish(acc: torch.Tensor, ci: torch.Tensor, K: int, dtype: torch.dtype = torch.float64):
    """End of the local epoch: returns the new ``(ci, delta)``."""
    new = acc.to(dtype) / torch.full((1,), float(K), dtype=dtype, device=acc.device)   # a true division, not *(1/K)
    return new, new - ci.to(dtype)


def reference_begin(c: torch.Tensor, dmean: torch.Tensor, ci: torch.Tensor, dtype: torch.dtype = torch.float64):
    """After the collective: returns the new ``(c, corr, acc)``."""
    cn = c.to(dtype) + dmean.to(dtype)
    return cn, cn - ci.to(dtype), torch.zeros_like(cn)


class ClientOpt(ReplicatedState):
    """Drift-correction state of one client.  FedProx: ``anchor``.  SCAFFOLD: ``c`` (replicated), ``ci``,
    ``corr = c - ci``, the raw-gradient sum ``acc``, the round's ``delta``, and the host step count ``K``."""

    def __init__(self, trainer, cfg: ClientOptConfig):
        x = trainer.float_state()
        super().__init__(x, cfg)
        self.n = int(trainer.n_params())
        if not 0 <= self.n <= x.numel():
            raise ValueError(f"n_params() = {self.n} outside the float state of {x.numel()} entries")
        self.anchor = self.c = self.ci = self.corr = self.acc = self.delta = None
        if cfg.kind == "fedprox":
            self.anchor = x[:self.n].detach().clone()
        else:
            self.c, self.ci, self.corr, self.acc, self.delta = (
                torch.zeros(self.n, dtype=torch.float32, device=self.dev) for _ in range(5))
        self.K = 0

    def _stream(self) -> int:
        return native.stream_handle(self.dev)

    def _rolled(self) -> List[torch.Tensor]:
        return [self.anchor] if self.cfg.kind == "fedprox" else [self.c, self.ci, self.corr]

    # ---- per step (the engines call these) -----------------------------------------------------------------------
    def apply(self, grad: torch.Tensor, params: torch.Tensor) -> None:
        """Correct the flat gradient in place, after the backward pass and before the SGD tail."""
        if grad.numel() != self.n or params.numel() != self.n:
            raise ValueError(f"gradient / parameters of {grad.numel()} / {params.numel()} entries, the client "
                             f"optimizer was built for {self.n}")
        c = self.cfg
        prox = c.kind == "fedprox"
        if self._nat is not None:
            # a kind never touches the other kind's buffers: the kernel gets null pointers for them
            self._nat.drift_grad(self._stream(), c.kind_id, grad.data_ptr(),
                                 params.data_ptr() if prox else 0, self.anchor.data_ptr() if prox else 0,
                                 0 if prox else self.corr.data_ptr(), 0 if prox else self.acc.data_ptr(), c.mu, self.n)
            return
        with torch.no_grad():
            if prox:
                grad.copy_(fma32(c.mu, params - self.anchor, grad))
            else:
                self.acc.add_(grad)
                grad.add_(self.corr)

    def count(self, steps: int) -> None:
        """``steps`` more SGD steps ran (or were enqueued) since :meth:`begin_round`."""
        self.K += int(steps)

    def save_acc(self):
        """What an engine's capture warm-up step must not leave a trace in (restored by :meth:`restore_acc`)."""
        return None if self.acc is None else self.acc.clone()

    def restore_acc(self, saved) -> None:
        if saved is not None:
            self.acc.copy_(saved)

    # ---- per round (FedAvg calls these) ---------------------------------------------------------------------------
    def finish_round(self) -> None:
        """Before the collective.  SCAFFOLD: ``ci`` becomes the mean raw gradient, ``delta`` its change."""
        if self.cfg.kind != "scaffold":
            return
        if self.K < 1:
            raise ValueError("scaffold: finish_round() without a counted SGD step (K = 0): the client did not train "
                             "this round, so it has no gradient mean to report")
        if self._nat is not None:
            self._nat.scaffold_finish(self._stream(), self.acc.data_ptr(), self.ci.data_ptr(), self.delta.data_ptr(),
                                      self.K, self.n)
        else:
            with torch.no_grad():
                new, d = reference_finish(self.acc, self.ci, self.K, torch.float32)
                self.delta.copy_(d)
                self.ci.copy_(new)

    def begin_round(self, trainer, dmean: Optional[torch.Tensor] = None) -> None:
        """After the collective (and any server step): ``float_state()`` holds the next round's starting model,
        ``dmean`` the mean of the clients' ``delta`` (SCAFFOLD)."""
        if self.cfg.kind == "fedprox":
            self.anchor.copy_(trainer.float_state()[:self.n])
            self.K = 0
            return
        if dmean is None or dmean.numel() != self.n:
            raise ValueError("scaffold: begin_round() needs the mean of the clients' delta")
        if self._nat is not None:
            self._nat.scaffold_begin(self._stream(), self.c.data_ptr(), dmean.data_ptr(), self.ci.data_ptr(),
                                     self.corr.data_ptr(), self.acc.data_ptr(), self.n)
        else:
            with torch.no_grad():
                cn, corr, _ = reference_begin(self.c, dmean, self.ci, torch.float32)
                self.c.copy_(cn)
                self.corr.copy_(corr)
                self.acc.zero_()
        self.K = 0

    def reset(self, trainer) -> None:
        """The model was replaced from outside (resync, load): re-anchor and forget the gradients summed on the
        old one; ``c`` and ``ci`` are kept, and ``corr`` follows a ``c`` that :meth:`FedAvg.resync` just delivered
        (the same fp32 subtraction as ``scaffold_begin``'s, so it is a no-op when ``c`` did not change)."""
        if self.anchor is not None:
            self.anchor.copy_(trainer.float_state()[:self.n])
        if self.acc is not None:
            torch.sub(self.c, self.ci, out=self.corr)
            self.acc.zero_()
        self.K = 0

    def _after_rollback(self) -> None:
        """``acc`` and ``K`` restart from zero (a void round's gradients must not leave a trace in ``ci``)."""
        if self.acc is not None:
            self.acc.zero_()
        self.K = 0

    def state_tensors(self) -> List[torch.Tensor]:
        """What a joining client must receive from the survivors: ``c``.  Its own ``ci`` starts at zero."""
        return [] if self.c is None else [self.c]


def add_client_opt_flags(ap) -> None:
    """``--client-opt`` and ``--client-mu`` (fedmi.cli.client, tools/fedavg_sim.py)."""
    ap.add_argument("--client-opt", default="none", choices=["none", *KINDS],
                    help="drift correction inside the local SGD step (fedmi.parallel.client_opt): fedprox adds "
                         "mu*(w - w_global) to every gradient, scaffold adds c - c_i; every client must pass the "
                         "same settings")
    ap.add_argument("--client-mu", type=float, default=0.01, help="FedProx proximal weight mu (>= 0)")


def make_client_opt(kind: Optional[str], trainer=None, mu: float = 0.01) -> Optional[ClientOpt]:
    """Build the state and hand it to the trainer (:meth:`LocalTrainer.set_client_opt`; an engine without the hook
    raises NotImplementedError)."""
    if kind in (None, "", "none"):
        return None
    co = ClientOpt(trainer, ClientOptConfig(kind, mu))
    trainer.set_client_opt(co)
    return co
