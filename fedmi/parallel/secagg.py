"""Secure aggregation (``--secagg``): FedAvg's mean over pairwise-masked fixed-point updates.

fedmi has no server, and the collectives let every peer read every client's contribution.  With pairwise masking
(Bonawitz et al. 2017, "Practical Secure Aggregation for Privacy-Preserving Machine Learning") a client's update leaves
it only under masks that every pair of clients shares and that cancel in the sum: a peer sees uniform words and, after
the sum, the mean -- nothing else.  A lost client voids the round here (the survivors roll back), so the protocol's
mask recovery (secret shares of a dropped client's seeds) is not needed: a round completes with every mask cancelled
or not at all.

The rule, exactly (the tests compare bits).  ``W`` clients (2..16), rank ``r`` holds ``x_r[i]``, ``i < n``, the whole
``float_state()``; ``a[i]`` is the round's starting global model, the guard's own anchor over all ``n`` entries.
``R = --secagg-range`` is a power of two in ``2^-8 .. 2^8`` and ``f = 27 - log2 R``, so ``R 2^f = 2^27`` whatever ``W``
is.

* encode: ``d = x - a`` (fp32), ``s = d 2^f`` (exact), clamped to ``+-(2^27 - 1)``, a NaN becomes 0; ``q = (int32)
  rint(s)`` (ties to even).  A clamped or NaN entry counts into ``clamped``.  ``|q| <= 2^27 - 1``: the sum over 16
  clients fits an int32;
* mask: ``u_r[i] = (uint32) q + sum_{j > r} m_rj[i] - sum_{j < r} m_rj[i]  mod 2^32``.  ``m_rj[i]`` is a ChaCha20
  keystream word (RFC 8439 block function, 20 rounds) under the pair's key ``k_rj = k_jr``, block counter ``i >> 4``,
  nonce words ``(draw lo, draw hi, 0)``; coordinate ``16 B + 4 c + k`` takes output word ``4 k + c`` of block ``B``
  (the kernel's lane ``c`` of a quad holds exactly those four words, csrc/kernels/secagg.hip).  ``draw`` is a 64-bit
  round counter, the same on all clients, advanced on every call and NOT rolled back with a void round: a mask used
  twice would publish the difference of the two updates it covered;
* decode: ``S[i] = sum_r u_r[i] mod 2^32`` read as int32, ``m = (float)((double) S 2^-f / W)`` (product and division
  in fp64, one rounding to fp32), ``x[i] = a[i] + m`` (fp32).  The masks cancel exactly, ``S = sum_r q_r``: every
  client computes the same bits.  Where nothing is clamped ``|mean_r q_r 2^-f - mean_r d_r| <= 2^-(f+1)``.

Keys.  Every client draws an X25519 secret (``secrets``); when the world or the group changes the clients all-gather
their 32-byte public keys over the data plane, and ``k_rj = HKDF-SHA256(X25519(sk_r, pk_j), info = b"fedmi-secagg" +
min rank + max rank)``.  The keys never leave the client; the public keys are NOT authenticated: the threat model is
honest-but-curious peers, an active man in the middle is out of scope.  X25519 is the RFC 7748 ladder in plain Python
(not constant-time).  ``--secagg-seed`` derives the pair keys from a hash of the seed: reproducible, and no secret.

On a GPU a round is 3 launches (mask, its count fold, unmask) around the gather of ``u`` on the trainer's stream, no
host sync; elsewhere the numpy twin below runs the same rule.
"""
from __future__ import annotations

import hashlib
import hmac
import math
import secrets
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import native
from .replicated import ReplicatedConfig
from .robust import MAX_RANKS, GatheredAgg, compression_on

KINDS = ("pairwise",)
Q_MAX = (1 << 27) - 1
_U64 = (1 << 64) - 1
_P = (1 << 255) - 19
_BASE = (9).to_bytes(32, "little")
_SIGMA = np.array([0x61707865, 0x3320646E, 0x79622D32, 0x6B206574], dtype=np.uint32)


def frac_bits(R: float) -> int:
    """``f = 27 - log2 R``; raises unless ``R`` is a power of two in ``2^-8 .. 2^8``."""
    m, e = math.frexp(float(R)) if R and math.isfinite(R) else (0.0, 0)
    if m != 0.5 or not -8 <= e - 1 <= 8:
        raise ValueError(f"secure aggregation: the range R must be a power of two in 2^-8 .. 2^8, not {R!r}")
    return 27 - (e - 1)


@dataclass
class SecAggConfig(ReplicatedConfig):
    kind: str = "pairwise"
    range: float = 8.0               # --secagg-range R: an update entry beyond +-R is clamped

    KINDS = KINDS
    FIELDS = ("kind", "range")
    ROLE, FLAG = "secure aggregation", "--secagg / --secagg-range"
    MISMATCH_TAIL = ", or the clients encode at different scales and the decoded mean is wrong"

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"secure aggregation: kind must be one of {KINDS}, not {self.kind!r}")
        self.range = float(self.range)
        self.frac_bits = frac_bits(self.range)


# ---- keys ------------------------------------------------------------------------------------------------------------
def x25519(k: bytes, u: bytes) -> bytes:
    """RFC 7748 section 5: the Montgomery ladder on Curve25519, scalar ``k`` (clamped here) times the point ``u``."""
    kb = bytearray(k)
    kb[0] &= 248
    kb[31] = (kb[31] & 127) | 64
    kn = int.from_bytes(kb, "little")
    x1 = int.from_bytes(u, "little") & ((1 << 255) - 1)
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        bit = (kn >> t) & 1
        if swap ^ bit:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = bit
        A, B, C, D = x2 + z2, x2 - z2, x3 + z3, x3 - z3
        AA, BB, DA, CB = A * A % _P, B * B % _P, D * A % _P, C * B % _P
        E = AA - BB
        x3, z3 = (DA + CB) ** 2 % _P, x1 * (DA - CB) ** 2 % _P
        x2, z2 = AA * BB % _P, E * (AA + 121665 * E) % _P
    if swap:
        x2, z2 = x3, z3
    return (x2 * pow(z2, _P - 2, _P) % _P).to_bytes(32, "little")


def pair_key(sk: bytes, pk_peer: bytes, rank: int, peer: int) -> bytes:
    """``k_rj``: HKDF-SHA256 (RFC 5869, empty salt, one block) of the X25519 shared secret, bound to the pair."""
    shared = x25519(sk, pk_peer)
    if not any(shared):
        raise ValueError(f"secure aggregation: rank {peer}'s public key is a low-order point (all-zero shared secret)")
    prk = hmac.new(bytes(32), shared, hashlib.sha256).digest()
    info = b"fedmi-secagg" + bytes([min(rank, peer), max(rank, peer)])
    return hmac.new(prk, info + b"\x01", hashlib.sha256).digest()


def seeded_key(seed: int, rank: int, peer: int) -> bytes:
    """``--secagg-seed``: the pair's key from a hash anyone can compute (tests only)."""
    return hashlib.sha256(f"fedmi-secagg/{int(seed)}/{min(rank, peer)}/{max(rank, peer)}".encode()).digest()


def key_table(keys: Sequence[Optional[bytes]]) -> np.ndarray:
    """``[W, 8]`` uint32, row ``j`` = the little-endian words of the key shared with rank ``j`` (own row: zeros)."""
    table = np.zeros((len(keys), 8), dtype=np.uint32)
    for j, k in enumerate(keys):
        if k is not None:
            table[j] = np.frombuffer(k, dtype="<u4")
    return table


# ---- the kernels' twin in numpy --------------------------------------------------------------------------------------
def chacha20_blocks(key: np.ndarray, counters: np.ndarray, nonce: Sequence[int]) -> np.ndarray:
    """RFC 8439 section 2.3 for every counter at once: ``key`` 8 words, ``nonce`` 3 words; ``[len(counters), 16]``."""
    counters = np.asarray(counters, dtype=np.uint32)
    init = np.empty((16, counters.size), dtype=np.uint32)
    init[0:4] = _SIGMA[:, None]
    init[4:12] = np.asarray(key, dtype=np.uint32)[:, None]
    init[12] = counters
    init[13:16] = np.array([int(w) & 0xFFFFFFFF for w in nonce], dtype=np.uint32)[:, None]
    s = [init[i].copy() for i in range(16)]

    def rotl(v, k):
        return (v << np.uint32(k)) | (v >> np.uint32(32 - k))

    def quarter(a, b, c, d):
        s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 16)
        s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 12)
        s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 8)
        s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 7)

    for _ in range(10):
        for col in range(4):
            quarter(col, 4 + col, 8 + col, 12 + col)
        for col in range(4):
            quarter(col, 4 + (col + 1) % 4, 8 + (col + 2) % 4, 12 + (col + 3) % 4)
    return np.stack(s, axis=1) + init.T


def pair_mask(key: np.ndarray, draw: int, n: int) -> np.ndarray:
    """``m[i]``, ``i < n``, of one pair: coordinate ``16 B + 4 c + k`` is word ``4 k + c`` of block ``B``."""
    nb = (n + 15) // 16
    words = chacha20_blocks(key, np.arange(nb, dtype=np.uint64).astype(np.uint32), (draw, draw >> 32, 0))
    return np.ascontiguousarray(words.reshape(nb, 4, 4).transpose(0, 2, 1)).reshape(-1)[:n]


def encode_np(x: np.ndarray, a: np.ndarray, f: int) -> Tuple[np.ndarray, int]:
    """``(q as uint32, clamped)``."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = (x.astype(np.float32) - a.astype(np.float32)) * np.float32(2.0 ** f)
        inside = np.abs(s) < np.float32(2.0 ** 27)
        edge = np.where(np.isnan(s), 0.0, np.where(s < 0, -float(Q_MAX), float(Q_MAX)))
        q = np.where(inside, np.rint(s.astype(np.float64)), edge).astype(np.int64)
    return q.astype(np.uint32), int((~inside).sum())


def mask_np(x: np.ndarray, a: np.ndarray, keys: np.ndarray, rank: int, draw: int, f: int) -> Tuple[np.ndarray, int]:
    """``secagg_mask`` in numpy: ``keys`` is the ``[W, 8]`` table; returns ``(u uint32[n], clamped)``."""
    u, clamped = encode_np(x, a, f)
    for j in range(keys.shape[0]):
        if j != rank:
            m = pair_mask(keys[j], draw, u.size)
            u = u + m if j > rank else u - m
    return u, clamped


def unmask_np(rows: np.ndarray, a: np.ndarray, f: int) -> np.ndarray:
    """``secagg_unmask`` in numpy: ``rows`` is ``[W, n]`` uint32."""
    total = rows.sum(axis=0, dtype=np.uint32).view(np.int32)
    m = (total.astype(np.float64) * 2.0 ** -f / float(rows.shape[0])).astype(np.float32)
    return a.astype(np.float32) + m


# ---- the guard -------------------------------------------------------------------------------------------------------
class SecAgg(GatheredAgg):
    """The masked mean in the ``secagg`` slot of a :class:`fedmi.parallel.fedavg.FedAvg`.  Holds the anchor (rolled
    back with a void round), the draw counter (never rolled back; handed to a joining client), the client's X25519
    secret and the device table of its pair keys for the current world."""

    def __init__(self, trainer, cfg: SecAggConfig, seed: Optional[int] = None):
        x = trainer.float_state()
        self.stats = torch.zeros(1, dtype=torch.int64, device=x.device)
        super().__init__(trainer, cfg, self.stats)
        self.n = x.numel()
        self.anchor = x.detach().clone()
        self.draw = 0
        self._draw_t = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self._handed = False
        self._u = torch.zeros(self.n, dtype=torch.int32, device=self.dev)     # the payload: x stays intact until the decode
        self._seed = seed
        self._sk = secrets.token_bytes(32)
        self.public_key = x25519(self._sk, _BASE)
        self._keys = None                # [W, 8] int32 (uint32 words) on the device
        self._peers = None               # (W, rank, transport, group) the table was made for

    def _rolled(self) -> List[torch.Tensor]:
        return [self.anchor]

    def state_tensors(self) -> List[torch.Tensor]:
        """``draw``: one int64 that every client must share.  The keys never leave the client."""
        self._draw_t.fill_(self.draw - (1 << 64) if self.draw >> 63 else self.draw)
        self._handed = True
        return [self._draw_t]

    def begin_round(self, trainer) -> None:
        """After the collective (and any server step): ``float_state()`` is the next round's starting model."""
        self.anchor.copy_(trainer.float_state())

    def reset(self, trainer) -> None:
        """The model was replaced from outside: it is the new anchor.  After a hand-over the draw is the source's;
        the pair keys are exchanged again at the next call."""
        self.anchor.copy_(trainer.float_state())
        if self._handed:
            self.draw = int(self._draw_t.item()) & _U64
            self._handed = False
        self._peers = None

    # -- keys
    def set_peers(self, W: int, rank: int, public_keys: Optional[Sequence[bytes]]) -> None:
        """Build the key table for ``W`` clients from their public keys (None: ``--secagg-seed``)."""
        if self._seed is not None:
            keys = [None if j == rank else seeded_key(self._seed, rank, j) for j in range(W)]
        else:
            if bytes(public_keys[rank]) != self.public_key:
                raise RuntimeError("secure aggregation: the gathered public keys do not hold this client's at its rank")
            keys = [None if j == rank else pair_key(self._sk, bytes(public_keys[j]), rank, j) for j in range(W)]
        self._keys = torch.from_numpy(key_table(keys).view(np.int32)).to(self.dev)

    def _exchange(self, W: int, rank: int, fedavg) -> None:
        peers = (W, rank, fedavg.transport, fedavg.group)
        if self._peers is not None and self._peers[:2] == peers[:2] and self._peers[2] is peers[2] \
                and self._peers[3] is peers[3]:
            return
        pks = None
        if self._seed is None:
            mine = torch.frombuffer(bytearray(self.public_key), dtype=torch.uint8).to(self.dev)
            if fedavg.transport is not None:
                got = fedavg.transport.all_gather(mine)
            else:
                rows = [torch.empty_like(mine) for _ in range(W)]
                self._all_gather(rows, mine, fedavg.group, fedavg.abort)
                got = torch.stack(rows)
            pks = [bytes(row) for row in got.cpu().numpy()]          # once per generation: the only host sync
        self.set_peers(W, rank, pks)
        self._peers = peers

    # -- the two kernels or their twin
    def mask(self, x: torch.Tensor, W: int, rank: int) -> torch.Tensor:
        """``u`` of this client's ``x`` under the current draw, which it consumes."""
        if x.numel() != self.n:
            raise ValueError(f"float state has {x.numel()} entries, the secure-aggregation guard was built for {self.n}")
        if self._keys is None or self._keys.shape[0] != W:
            raise RuntimeError("secure aggregation: no key table for this world (set_peers)")
        draw = self.draw
        self.draw = (self.draw + 1) & _U64          # before anything can fail: a mask is never used twice
        f = self.cfg.frac_bits
        if self._nat is not None:
            self._nat.secagg_mask(native.stream_handle(self.dev), x.data_ptr(), self.anchor.data_ptr(),
                                  self._keys.data_ptr(), W, rank, draw, self.n, f, self._u.data_ptr(),
                                  self._partials(self._nat.secagg_partials(self.n), torch.int64).data_ptr(),
                                  self.stats.data_ptr())
        else:
            with torch.no_grad():
                u, clamped = mask_np(x.detach().numpy(), self.anchor.numpy(), self._keys.numpy().view(np.uint32), rank, draw, f)
                self._u.copy_(torch.from_numpy(u.view(np.int32)))
                self.stats[0] = clamped
        return self._u

    def unmask(self, rows: torch.Tensor, x: torch.Tensor, W: int) -> None:
        """``x`` <- the decode of the ``[W, ld]`` payload rows (fp32 storage holding the uint32 words)."""
        f = self.cfg.frac_bits
        if self._nat is not None:
            self._nat.secagg_unmask(native.stream_handle(self.dev), rows.data_ptr(), rows.shape[1], W,
                                    self.anchor.data_ptr(), self.n, f, x.data_ptr())
        else:
            with torch.no_grad():
                words = rows[:, :self.n].contiguous().numpy().view(np.uint32)
                x.copy_(torch.from_numpy(unmask_np(words, self.anchor.numpy(), f)))

    def _run(self, x, W, fedavg):
        rank = fedavg.rank()
        self._exchange(W, rank, fedavg)
        u = self.mask(x, W, rank)
        self.unmask(self._gather(u.view(torch.float32), W, fedavg), x, W)
        return True

    def _decode(self, tag, stats) -> dict:
        return {"secagg_clamped": int(stats[0])}

    def round_stats(self) -> dict:
        """``secagg_draw`` (the calls so far) and ``secagg_clamped`` of the newest call whose count has reached the
        host (on a GPU at worst the previous round's: no sync is added)."""
        self._collect()
        return {"secagg_draw": self.draw, **self._seen}


def add_secagg_flags(ap) -> None:
    """``--secagg``, ``--secagg-range``, ``--secagg-seed`` (fedmi.cli.client, tools/fedavg_sim.py)."""
    ap.add_argument("--secagg", action="store_true",
                    help="secure aggregation (fedmi.parallel.secagg): every client's update leaves it as fixed-point "
                         "words under pairwise ChaCha20 masks that cancel in the sum, so a peer sees only the mean; "
                         "every client must pass the same settings")
    ap.add_argument("--secagg-range", type=float, default=8.0, metavar="R",
                    help="an update entry beyond +-R is clamped (counted in secagg_clamped); a power of two in "
                         "2^-8 .. 2^8; the resolution is R * 2^-27")
    ap.add_argument("--secagg-seed", type=int, default=None,
                    help="derive the pair keys from this seed instead of an X25519 exchange: reproducible runs for "
                         "tests only -- a known key VOIDS the secrecy of the updates")


def check_secagg_flags(a, error) -> None:
    """The flag combinations the masked sum cannot serve, each refused through ``error`` (``ArgumentParser.error``)."""
    if not getattr(a, "secagg", False):
        return
    try:
        frac_bits(a.secagg_range)
    except ValueError:
        error("--secagg-range must be a power of two in 2^-8 .. 2^8 (the fixed-point scale is 2^27 / R)")
    if getattr(a, "agg", "collective") == "grpc":
        error("--secagg needs --agg collective: with --agg grpc the coordinator receives and averages the clients' "
              "raw models (reference peers), nothing masks them")
    if compression_on(a):
        error("--secagg cannot be combined with compression (-c Y / --compress): the compressors send quantised "
              "deltas of their own, which the masks do not cover")
    if getattr(a, "robust", "none") != "none":
        error("--secagg cannot be combined with --robust: a robust rule needs the clients' individual models, which "
              "the masks hide")
    if getattr(a, "client_opt", "none") == "scaffold":
        error("--secagg cannot be combined with --client-opt scaffold: its second collective carries every client's "
              "mean gradient unmasked")


def make_secagg(on: bool, trainer=None, R: float = 8.0, seed: Optional[int] = None) -> Optional[SecAgg]:
    """None when off (nothing new is launched)."""
    if not on:
        return None
    return SecAgg(trainer, SecAggConfig("pairwise", R), seed)


def secagg_stack(guards: Sequence[SecAgg], states: Sequence[torch.Tensor]) -> torch.Tensor:
    """The masked mean of simulated clients in one process (tools/fedavg_sim.py): guard ``r`` masks ``states[r]``,
    the payloads are stacked as the gather would and guard 0 decodes.  Returns the aggregate (a new tensor)."""
    W, n = len(states), states[0].numel()
    if W > MAX_RANKS:
        raise ValueError(f"secure aggregation handles at most {MAX_RANKS} clients, the federation has {W}")
    pks = [g.public_key for g in guards]
    rows = torch.zeros((W, (n + 3) & ~3), dtype=torch.float32, device=states[0].device)
    for r, (g, x) in enumerate(zip(guards, states)):
        if g._keys is None or g._keys.shape[0] != W:
            g.set_peers(W, r, pks)
        rows[r, :n].copy_(g.mask(x, W, r).view(torch.float32))
    out = torch.empty_like(states[0])
    guards[0].unmask(rows, out, W)
    return out
