"""Differentially private FedAvg: per-client update clipping and Gaussian noise.

DP-FedAvg (McMahan et al. 2018, "Learning Differentially Private Recurrent Language Models") bounds what one
client's round update reveals: the update is clipped to L2 norm ``S`` and Gaussian noise calibrated to ``S`` is
added.  Per round, on each client, after the local epoch and before the collective, with ``x = float_state()``,
``a`` the round's starting global model, ``k = n_params()`` and ``N`` clients::

    d_i    = x_i - a_i                       (fp32, i < k)
    norm   = sqrt(sum_i d_i^2)               (the sum in fp64, fixed order)
    scale  = norm > S ? (float)(S / norm) : 1
    y_i    = scale == 1 ? x_i : fma(scale, d_i, a_i)      (an unclipped update keeps its exact bits)
    x_i    = z > 0 ? fma(sigma, g_i, y_i) : y_i           sigma = (float)(z * S / sqrt(N)),  g_i ~ N(0, 1)

The entries at and past ``k`` (BN running statistics) and the int state are not touched: noise on a running variance
can make it negative.  The guarantee therefore covers the trainable parameters only; it is complete for models without
such buffers (LeNet, MLP).

fedmi has no server, so each client adds its own share of the noise: N shares of std ``z*S/sqrt(N)`` sum to std
``z*S`` on the sum of the updates, the central DP-FedAvg mechanism.  A curious peer knows its own share, so towards a
peer the effective noise variance is ``(N-1)/N`` of it.  Compression, a server optimizer and FedProx act on the privatised
``x`` and are post-processing.

``g`` comes from Philox4x32-10 (Salmon et al. 2011) keyed by a 64-bit per-client secret, counter ``(block lo, block
hi, draw lo, draw hi)`` with ``block = i >> 2``; entry ``i`` takes lane ``i & 3``.  The outputs ``r0..r3`` give two
Box-Muller pairs from ``u(r) = ((r >> 9) + 0.5) * 2^-23``.  ``draw`` is a host counter advanced on every call and NOT
rolled back with a void round: reusing noise on a retrained update would publish the difference of the two updates
without noise.

On a GPU the round is three HIP launches (csrc/kernels/dp.hip) on the trainer's stream without a host sync; elsewhere
the same formulas and draws run in torch / numpy.
"""
from __future__ import annotations

import hashlib
import math
import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from .. import native
from .client_opt import fma32
from .replicated import ReplicatedConfig, ReplicatedState

KINDS = ("clip", "gaussian")
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_U64 = (1 << 64) - 1


@dataclass
class DpConfig(ReplicatedConfig):
    clip: float                      # S > 0
    noise: float = 0.0               # the noise multiplier z >= 0
    delta: float = 1e-5              # used only for the reported epsilon

    KINDS = KINDS
    FIELDS = ("kind", "clip", "noise")
    ROLE, FLAG = "differential privacy", "--dp-clip / --dp-noise"
    MISMATCH_TAIL = ", or the federation's noise does not add up to the level the accounting assumes"

    def __post_init__(self):
        self.clip, self.noise, self.delta = float(self.clip), float(self.noise), float(self.delta)
        if not (self.clip > 0 and math.isfinite(self.clip)):
            raise ValueError("differential privacy: the clip norm S must be finite and > 0")
        if not (self.noise >= 0 and math.isfinite(self.noise)):
            raise ValueError("differential privacy: the noise multiplier z must be finite and >= 0")
        if not 0 < self.delta < 1:
            raise ValueError("differential privacy: delta must lie in (0, 1)")

    @property
    def kind(self) -> str:
        return "gaussian" if self.noise > 0 else "clip"


def epsilon(z: float, rounds: int, delta: float = 1e-5) -> float:
    """Client-level epsilon after ``rounds`` rounds with every client taking part in each (no subsampling
    amplification).  One round of the Gaussian mechanism at noise multiplier ``z`` is ``(alpha, alpha / (2 z^2))``-RDP;
    T rounds compose to ``alpha T / (2 z^2)``, which converts to ``(eps, delta)`` with ``eps = alpha T / (2 z^2) +
    ln(1/delta) / (alpha - 1)``.  At the optimal order ``alpha = 1 + z sqrt(2 ln(1/delta) / T)``::

        eps = T / (2 z^2) + sqrt(2 T ln(1/delta)) / z

    Neighbouring federations differ in one client.  ``z = 0`` (clipping alone) gives ``inf``."""
    if rounds <= 0:
        return 0.0
    if not z > 0:
        return math.inf
    return rounds / (2.0 * z * z) + math.sqrt(2.0 * rounds * math.log(1.0 / delta)) / z


def sigma32(clip: float, noise: float, world: int) -> float:
    """``(float)(z * S / sqrt(N))``, the same fp64 operations as the binding's."""
    return float(np.float32(noise * clip / math.sqrt(float(world))))


# ---- the generator in numpy / torch (the kernels' twin) --------------------------------------------------------------
def philox4x32(counter, key) -> np.ndarray:
    """Philox4x32-10.  ``counter``: uint32 words ``[..., 4]``, ``key``: two uint32 words; returns ``[..., 4]``
    uint32."""
    c = [np.asarray(counter, dtype=np.uint64)[..., j] & _MASK for j in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]          # 32 x 32 bits: no overflow in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def draw_words(key: int, draw: int, n: int) -> np.ndarray:
    """The ``[ceil(n / 4), 4]`` uint32 outputs of blocks ``0 .. ceil(n / 4) - 1`` under a 64-bit ``key`` and ``draw``."""
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.empty((blocks.size, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = blocks & _MASK, blocks >> np.uint64(32)
    ctr[:, 2], ctr[:, 3] = draw & 0xFFFFFFFF, (draw >> 32) & 0xFFFFFFFF
    return philox4x32(ctr, (key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF))


def gaussian(key: int, draw: int, n: int, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """``g_0 .. g_{n-1}`` at ``dtype``: entry ``i`` is lane ``i & 3`` of block ``i >> 2``; lanes 0, 1 =
    ``sqrt(-2 ln u(r0)) * {cos, sin}(2 pi u(r1))``, lanes 2, 3 the same from ``r2, r3``.  ``u`` is exact in fp32, so
    the fp64 result is the exact-arithmetic value of the kernel's draw to fp64 accuracy."""
    r = torch.from_numpy((draw_words(key, draw, n) >> np.uint32(9)).astype(np.int64))
    u = (r.to(dtype) + 0.5) * 2.0 ** -23
    radius = torch.sqrt(-2.0 * torch.log(u[:, 0::2]))
    angle = (2.0 * math.pi) * u[:, 1::2]
    g = torch.stack((radius * torch.cos(angle), radius * torch.sin(angle)), dim=-1)     # [blocks, pair, cos | sin]
    return g.reshape(-1)[:n]


def reference_privatize(x: torch.Tensor, anchor: torch.Tensor, k: int, cfg: DpConfig, world: int, key: int, draw: int,
                        scale: Optional[float] = None, dtype: torch.dtype = torch.float64):
    """The round's step in plain torch at ``dtype``: returns ``(x_new, sumsq, norm, scale)``, inputs untouched.

    ``d`` is formed in fp32 as the kernel forms it (part of the definition); ``sumsq`` is the fp64 sum of its exact
    squares.  ``scale`` (an fp32 value) replaces the twin's own when given: a test judges the apply on the device's
    scale.  ``scale`` and ``sigma`` reach the fma as fp32 numbers."""
    k = int(k)
    out = x.to(dtype).clone()
    d32 = x[:k].float() - anchor[:k].float()
    sumsq = float((d32.double() ** 2).sum()) if k else 0.0
    norm = math.sqrt(sumsq)
    if scale is None:
        scale = float(np.float32(cfg.clip / norm)) if norm > cfg.clip else 1.0
    y = out[:k] if scale == 1.0 else scale * d32.to(dtype) + anchor[:k].to(dtype)
    if cfg.noise > 0 and k:
        y = sigma32(cfg.clip, cfg.noise, world) * gaussian(key, draw, k, dtype).to(x.device) + y
    out[:k] = y
    return out, sumsq, norm, scale


def derive_key(seed: Optional[int], who: str) -> int:
    """The client's 64-bit Philox key: fresh from ``os.urandom``, or (``seed`` given: reproducible, which voids the
    guarantee) a hash of the seed and the client's address or rank, so clients never share a key."""
    if seed is None:
        return int.from_bytes(os.urandom(8), "little")
    return int.from_bytes(hashlib.sha256(f"fedmi-dp/{int(seed)}/{who}".encode()).digest()[:8], "little")


class DpGuard(ReplicatedState):
    """Per-client DP state: ``anchor`` (the round's starting global model, the first ``k`` entries), the secret
    ``key``, the host draw counter and the device stats row ``{sumsq, norm, scale}`` of the last call."""

    def __init__(self, trainer, cfg: DpConfig, key: Optional[int] = None):
        x = trainer.float_state()
        super().__init__(x, cfg)
        self.n = x.numel()
        self.k = int(trainer.n_params())
        if not 0 <= self.k <= self.n:
            raise ValueError(f"n_params() = {self.k} outside the float state of {self.n} entries")
        self.key = (derive_key(None, "") if key is None else int(key)) & _U64
        self.draw = 0
        self.anchor = x[:self.k].detach().clone()
        self.stats = torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float64, device=self.dev)
        self._partial = self._host = self._copied = None
        if self._nat is not None:
            self._partial = torch.zeros(max(1, self._nat.dp_partials(self.k)), dtype=torch.float64, device=self.dev)
            self._host = torch.zeros(4, dtype=torch.float64).pin_memory()
            self._copied = torch.cuda.Event()
        self._seen = None                # (norm, scale) of the newest stats row known on the host

    def _rolled(self) -> List[torch.Tensor]:
        return [self.anchor]

    def privatize(self, trainer, world: int) -> None:
        """``float_state()`` holds the client's locally trained model on entry and its clipped (and noised) one on
        return.  Advances ``draw``."""
        x = trainer.float_state()
        if x.numel() != self.n:
            raise ValueError(f"float state has {x.numel()} entries, the DP guard was built for {self.n}")
        self._collect()                             # the previous round's row, before this one overwrites it
        c, draw = self.cfg, self.draw
        self.draw = (self.draw + 1) & _U64          # before anything can fail: a draw is never used twice
        if self._nat is not None:
            self._nat.dp_privatize(native.stream_handle(self.dev), x.data_ptr(), self.anchor.data_ptr(), self.n,
                                   self.k, self._partial.data_ptr(), self.stats.data_ptr(), c.clip, c.noise,
                                   int(world), self.key, draw)
            # the row reaches the host behind the launches; read at the next round's start (round_stats)
            self._host.copy_(self.stats, non_blocking=True)
            self._copied.record(torch.cuda.current_stream(self.dev))
            return
        with torch.no_grad():
            k = self.k
            d = x[:k] - self.anchor
            sumsq = float((d.double() ** 2).sum()) if k else 0.0
            norm = math.sqrt(sumsq)
            scale = float(np.float32(c.clip / norm)) if norm > c.clip else 1.0
            if scale != 1.0:
                x[:k] = fma32(scale, d, self.anchor)
            if c.noise > 0 and k:
                g = gaussian(self.key, draw, k, torch.float32).to(x.device)
                x[:k] = fma32(sigma32(c.clip, c.noise, world), g, x[:k])
            self.stats.copy_(torch.tensor([sumsq, norm, scale, 0.0], dtype=torch.float64))

    def _collect(self) -> None:
        """Pick up the last call's stats row if it has reached the host.  Never waits: a row still in flight is
        picked up by a later call."""
        if self.draw == 0:
            return
        if self._nat is None:
            self._seen = (float(self.stats[1]), float(self.stats[2]))
        elif self._copied.query():
            self._seen = (float(self._host[1]), float(self._host[2]))

    def round_stats(self) -> dict:
        """``dp_norm`` / ``dp_scale`` of the newest call whose stats row has reached the host (on a GPU at worst the
        previous round's: no sync is added), and the epsilon spent by all ``draw`` calls so far."""
        self._collect()
        eps = epsilon(self.cfg.noise, self.draw, self.cfg.delta)
        rec = {"dp_rounds": self.draw, "dp_epsilon": eps if math.isfinite(eps) else None}   # clip only: no epsilon
        if self._seen is not None:
            rec["dp_norm"], rec["dp_scale"] = self._seen
        return rec

    def begin_round(self, trainer) -> None:
        """After the collective (and any server step): ``float_state()`` is the next round's starting model."""
        self.anchor.copy_(trainer.float_state()[:self.k])

    def reset(self, trainer) -> None:
        """The model was replaced from outside (resync, load): it is the new anchor.  ``draw`` goes on."""
        self.anchor.copy_(trainer.float_state()[:self.k])

    def state_tensors(self) -> List[torch.Tensor]:
        """Nothing is handed over: the anchor is the model itself, and the key never leaves the client."""
        return []


def add_dp_flags(ap) -> None:
    """``--dp-clip``, ``--dp-noise``, ``--dp-delta``, ``--dp-seed`` (fedmi.cli.client, tools/fedavg_sim.py)."""
    ap.add_argument("--dp-clip", type=float, default=0.0, metavar="S",
                    help="clip every client's round update (trainable parameters) to L2 norm S before it is "
                         "aggregated (fedmi.parallel.dp); 0 = off; every client must pass the same settings")
    ap.add_argument("--dp-noise", type=float, default=0.0, metavar="Z",
                    help="Gaussian noise multiplier z: every client adds N(0, (z*S)^2 / clients) to its clipped "
                         "update, std z*S on the sum (DP-FedAvg); needs --dp-clip > 0")
    ap.add_argument("--dp-delta", type=float, default=1e-5, help="delta of the reported (epsilon, delta)")
    ap.add_argument("--dp-seed", type=int, default=None,
                    help="derive the noise key from this seed and the client's address instead of os.urandom: "
                         "reproducible runs for tests only -- a known key VOIDS the privacy guarantee")


def check_dp_flags(a, error) -> None:
    """The flag combinations that cannot be private, each refused through ``error`` (``ArgumentParser.error``)."""
    if a.dp_clip < 0 or a.dp_noise < 0:
        error("--dp-clip and --dp-noise must be >= 0 (a norm bound and a noise multiplier)")
    if a.dp_noise > 0 and not a.dp_clip > 0:
        error("--dp-noise needs --dp-clip > 0: the noise is calibrated to the clip norm, and an unclipped update "
              "has no bounded sensitivity")
    if not a.dp_clip > 0:
        return
    if not 0 < a.dp_delta < 1:
        error("--dp-delta must lie in (0, 1)")
    if getattr(a, "agg", "collective") == "grpc":
        error("--dp-clip needs --agg collective: with --agg grpc the coordinator averages the clients' raw models "
              "(reference peers), nothing clips or noises them first")
    if getattr(a, "client_opt", "none") == "scaffold":
        error("--dp-clip cannot be combined with --client-opt scaffold: its second collective carries every client's "
              "mean gradient, which is neither clipped nor noised")


def make_dp(clip: float, trainer=None, noise: float = 0.0, delta: float = 1e-5, seed: Optional[int] = None,
            who: str = "") -> Optional[DpGuard]:
    """None when ``clip`` is 0 (nothing new is launched); ``who`` (address or rank) separates the clients' keys under
    ``seed``."""
    if not clip:
        return None
    return DpGuard(trainer, DpConfig(clip, noise, delta), derive_key(seed, who))
