"""Server-side optimizers on the aggregated model: FedAvgM, FedAdagrad, FedYogi, FedAdam.

Plain FedAvg installs ``mean(clients)`` as the new global model.  A server optimizer treats
``d = mean(clients) - previous global`` as a pseudo-gradient (Hsu et al. 2019, "Measuring the Effects of
Non-Identical Data Distribution for Federated Visual Classification"; Reddi et al. 2021, "Adaptive Federated
Optimization").  For every trainable entry, in fp32::

    fedavgm :   m = beta1*m + d                                x = anchor + lr*m
    adaptive:   m = beta1*m + (1-beta1)*d
      fedadagrad: v = v + d*d
      fedyogi   : v = v - (1-beta2)*d*d*sgn(v - d*d)
      fedadam   : v = beta2*v + (1-beta2)*d*d
                                                               x = anchor + lr*m / (sqrt(v) + tau)

with ``m`` starting at 0 and ``v`` at ``tau**2``; neither paper has a bias correction or a step counter.
Floating buffers (BN running statistics, the entries past :meth:`LocalTrainer.n_params`) stay the plain mean.

fedmi has no server: after the all-reduce every client holds the mean and a copy of the previous global
model (``anchor``), so the step is *replicated* -- each client runs the same one-launch kernel
(csrc/kernels/server_opt.hip) on the same inputs and gets the same bits, which keeps ``anchor``, ``m`` and
``v`` in lockstep without any extra traffic.  A client that joins later receives ``m`` / ``v`` from the
survivors (:meth:`FedAvg.resync`).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from .. import native
from .replicated import ReplicatedConfig, ReplicatedState

KINDS = ("fedavgm", "fedadagrad", "fedyogi", "fedadam")      # index == the kernel's ``kind`` argument
DEFAULT_LR = {"fedavgm": 1.0, "fedadagrad": 0.01, "fedyogi": 0.01, "fedadam": 0.01}   # the papers' starting points


@dataclass
class ServerOptConfig(ReplicatedConfig):
    kind: str
    lr: Optional[float] = None       # None: DEFAULT_LR[kind]
    beta1: float = 0.9
    beta2: float = 0.99
    tau: float = 1e-3

    KINDS = KINDS
    FIELDS = ("kind", "lr", "beta1", "beta2", "tau")
    ROLE, FLAG, MISMATCH_TAIL = "server optimizer", "--server-opt", ", or the replicated state drifts apart"

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"unknown server optimizer {self.kind!r} (one of {', '.join(KINDS)})")
        self.lr = DEFAULT_LR[self.kind] if self.lr is None else float(self.lr)
        self.beta1, self.beta2, self.tau = float(self.beta1), float(self.beta2), float(self.tau)
        if self.tau <= 0:
            raise ValueError("server optimizer: tau must be > 0")


def reference_step(x: torch.Tensor, anchor: torch.Tensor, m: torch.Tensor, v: Optional[torch.Tensor], n_opt: int,
                   cfg: ServerOptConfig, dtype: torch.dtype = torch.float64):
    """The step in plain torch ops at ``dtype``: returns new ``(x, anchor, m, v)``, inputs untouched.

    Same formulas in the same operation order as the kernel.  The hyperparameters are rounded to fp32 first
    (they reach the kernel as fp32 arguments, so they are inputs, not part of the arithmetic under test);
    ``1 - beta`` is then formed at ``dtype`` as the kernel forms it in fp32.  ``v`` may be None for fedavgm."""
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))   # noqa: E731
    lr, b1, b2, tau = f32(cfg.lr), f32(cfg.beta1), f32(cfg.beta2), f32(cfg.tau)
    k = int(n_opt)
    xo, mo = x.to(dtype).clone(), m.to(dtype).clone()
    vo = None if v is None else v.to(dtype).clone()
    a = anchor.to(dtype)[:k]
    d = xo[:k] - a
    if cfg.kind == "fedavgm":
        mk = b1 * mo[:k] + d
        xk = a + lr * mk
    else:
        mk = b1 * mo[:k] + (1.0 - b1) * d
        dd = d * d
        vk = vo[:k]
        if cfg.kind == "fedadagrad":
            vk = vk + dd
        elif cfg.kind == "fedyogi":
            vk = vk - (1.0 - b2) * dd * torch.sign(vk - dd)
        else:
            vk = b2 * vk + (1.0 - b2) * dd
        vo[:k] = vk
        xk = a + lr * mk / (torch.sqrt(vk) + tau)
    mo[:k] = mk
    xo[:k] = xk
    return xo, xo.clone(), mo, vo


class ServerOpt(ReplicatedState):
    """Replicated server optimizer state of one client: ``anchor`` (the previous global model), ``m``, ``v``."""

    def __init__(self, trainer, cfg: ServerOptConfig):
        x = trainer.float_state()
        super().__init__(x, cfg)
        self.n = x.numel()
        self.n_opt = int(trainer.n_params())
        if not 0 <= self.n_opt <= self.n:
            raise ValueError(f"n_params() = {self.n_opt} outside the float state of {self.n} entries")
        self.anchor = x.detach().clone()
        self.m = torch.zeros_like(self.anchor)
        self.v = torch.full_like(self.anchor, cfg.tau * cfg.tau)
        self.steps = 0

    def _rolled(self) -> List[torch.Tensor]:
        return [self.anchor, self.m, self.v]

    def step(self, trainer) -> None:
        """``float_state()`` holds the aggregated mean on entry and the new global model on return."""
        x = trainer.float_state()
        if x.numel() != self.n:
            raise ValueError(f"float state has {x.numel()} entries, the server optimizer was built for {self.n}")
        c = self.cfg
        if self._nat is not None:
            # fedavgm never touches v: the kernel gets a null pointer for it
            self._nat.server_opt(native.stream_handle(self.dev), x.data_ptr(), self.anchor.data_ptr(),
                                 self.m.data_ptr(), 0 if c.kind == "fedavgm" else self.v.data_ptr(), self.n,
                                 self.n_opt, c.kind_id, c.lr, c.beta1, c.beta2, c.tau)
        else:
            k = self.n_opt
            with torch.no_grad():
                xo, _, mo, vo = reference_step(x, self.anchor, self.m, None if c.kind == "fedavgm" else self.v, k,
                                               c, torch.float32)
                x[:k] = xo[:k]               # the float buffers past n_opt are never written
                self.m[:k] = mo[:k]
                if vo is not None:
                    self.v[:k] = vo[:k]
                self.anchor.copy_(x)
        self.steps += 1

    def reset(self, trainer) -> None:
        """The model was replaced from outside (resync, load): it is the new anchor; ``m`` and ``v`` are kept."""
        self.anchor.copy_(trainer.float_state())

    def state_tensors(self) -> List[torch.Tensor]:
        """What a joining client must receive from the survivors (the anchor is the model itself)."""
        return [self.m, self.v]


def add_server_opt_flags(ap) -> None:
    """``--server-opt`` and its hyperparameters (fedmi.cli.client, tools/fedavg_sim.py)."""
    ap.add_argument("--server-opt", default="none", choices=["none", *KINDS],
                    help="server-side optimizer applied to the aggregated model (fedmi.parallel.server_opt), "
                         "replicated on every client; every client must pass the same settings")
    ap.add_argument("--server-lr", type=float, default=None,
                    help="server learning rate (default: 1.0 for fedavgm, 0.01 for the adaptive kinds)")
    ap.add_argument("--server-beta1", type=float, default=0.9, help="server momentum")
    ap.add_argument("--server-beta2", type=float, default=0.99, help="second-moment decay (fedyogi, fedadam)")
    ap.add_argument("--server-tau", type=float, default=1e-3, help="adaptivity floor added to sqrt(v)")


def make_server_opt(kind: Optional[str], trainer=None, lr: Optional[float] = None, beta1: float = 0.9,
                    beta2: float = 0.99, tau: float = 1e-3) -> Optional[ServerOpt]:
    if kind in (None, "", "none"):
        return None
    return ServerOpt(trainer, ServerOptConfig(kind, lr, beta1, beta2, tau))
