"""``-c Y``: compressed FedAvg updates on the data plane.

Reference -c Y = gRPC gzip of base64 fp32 checkpoints (src/server.py:103-107,
src/client.py:39-43): 0.98-0.99x of the raw size at 16 ms-3 s of CPU per
message.  fedmi keeps the flag (and gzip on the gRPC control
channel) and compresses the *update* instead:

* ``topk``  — each client sends the k largest-magnitude entries of
  d = (w_local - w_global) + e (error feedback e carries the rest to the next
  round); selection is exact, on the GPU in 3 launches (6 from 1 M entries) and
  2 passes over the state (csrc/kernels/compress.hip ``launch_topk_ef``: fused
  delta + 11-bit histogram, wave-aggregated compaction of the certain winners and
  the boundary-bin candidates with the bin pick inside it, exact candidate
  select); (idx, val) pairs are all-gathered (RCCL, or the
  hipIpc peer kernels of :mod:`fedmi.parallel.peer`) and applied to the global
  model in rank order without atomics, so every client holds a bit-identical
  global model.  Payload per client: 8k bytes.
* ``int8``  — per-256-element absmax int8 quantisation with error feedback;
  payload n + 4n/256 bytes (~3.9x smaller than fp32).

* ``powersgd`` -- rank-R PowerSGD (Vogels, Karimireddy, Jaggi 2019), the one compressor that is LINEAR in the
  update: every weight matrix M of d = (w_local - w_global) + e that is worth it sends P = M Q and Q = M^T orth(mean P)
  ([rows, R] and [cols, R]); both factors are averaged by the plain all-reduce (RCCL, gloo or the peer transport), the
  global model moves by orth(mean P) (mean Q)^T and e keeps what the rank dropped.  Everything else (1-D tensors, BN
  statistics, matrices too small to gain) travels as its exact mean behind P in the same buffer.  mean Q is the next
  round's Q (warm start); Q starts from the same Philox normals on every client.  Four launches a round
  (csrc/kernels/powersgd.hip: the two GEMM passes on the fp32 matrix instruction), payload
  4 (sum R (rows + cols) + n_dense) bytes whatever the world size.  Its CPU branch follows the same formulas but not
  the matrix passes' summation order (tests/powersgd_check.py is the fp64 reference, with derived bounds).

The top-k and int8 CPU branches below are the kernels' twin: they follow the single-rounding
formulas in the header of csrc/kernels/compress.hip and give the kernels' bits
(tests/int8_check.py is the independent exact reference of both).

After aggregation every client holds w_global' = w_global + mean(sparse d),
exactly like dense FedAvg when k = n.

Every client must hold the same anchor ``global_ref``.  It is re-anchored
(:meth:`reset`) whenever the model is replaced from outside — a rank-0 init
broadcast, a SendModel resync, a new membership generation — and a client
that trains alone (world 1) simply adopts its local model.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from .. import native


def _world(group) -> int:
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fp32 ``fma(a, b, c)``: ONE rounding of a * b + c, like the kernels' ``__fmaf_rn`` (the roundings are listed
    in the header of csrc/kernels/compress.hip).  The product of two fp32 (or int8) values is exact in fp64; the
    fp64 sum is rounded to odd (TwoSum gives the sign of what the addition dropped), after which the final
    rounding to fp32 is the same as rounding the exact sum (fp64 carries more than 2 extra bits)."""
    p = a.double() * b.double()
    c = c.double()
    hi = p + c
    t = hi - p
    lo = (p - (hi - t)) + (c - t)                       # hi + lo == p + c exactly
    even = (hi.view(torch.int64) & 1) == 0
    side = torch.where(lo > 0, torch.full_like(hi, float("inf")), torch.full_like(hi, float("-inf")))
    hi = torch.where((lo != 0) & even, torch.nextafter(hi, side), hi)
    return hi.float()


PROBE = None          # diagnostics hook (client agent, FEDMI_DEBUG_STATS=1): called with a phase tag


def _probe(tag: str) -> None:
    if PROBE is not None:
        PROBE(tag)


def _all_gather_flat(t: torch.Tensor, group, transport=None) -> torch.Tensor:
    if transport is not None:
        return transport.all_gather(t)
    w = _world(group)
    if w == 1:
        return t.clone().unsqueeze(0)
    out = torch.empty((w,) + tuple(t.shape), dtype=t.dtype, device=t.device)
    if t.is_cuda:
        dist.all_gather_into_tensor(out.view(-1), t.contiguous().view(-1), group=group)
    else:
        dist.all_gather(list(out.unbind(0)), t.contiguous(), group=group)
    return out


class _EFCompressor:
    """``warmup``: the first ``warmup`` aggregations are dense FedAvg (the largest updates of a run come
    first, when a 1 % selection defers most of them); compression starts from the dense global model
    with an empty residual."""

    def __init__(self, trainer, warmup: int = 0):
        self.warmup = int(warmup)
        self.dense_rounds = 0
        x = trainer.float_state()
        self.n = x.numel()
        self.dev = x.device
        self.global_ref = x.detach().clone()
        self.residual = torch.zeros_like(self.global_ref)
        self.d = torch.empty_like(self.global_ref)
        self._nat = native.require() if x.is_cuda else None
        self.bytes_sent = 0          # this client's compressed payload bytes, summed over rounds
        self.dense_bytes = 0         # what dense fp32 FedAvg would have sent
        self.rounds = 0

    def reset(self, trainer) -> None:
        """Re-anchor on the trainer's current model (after a resync/load)."""
        self.global_ref.copy_(trainer.float_state())
        self.residual.zero_()

    def reanchor(self, x: torch.Tensor) -> None:
        """``x`` is the new global model on every client (a server optimizer moved it after the aggregation):
        it becomes the anchor.  Unlike :meth:`reset` the error-feedback residual is kept."""
        self.global_ref.copy_(x)

    def _dense(self, x: torch.Tensor, group, transport) -> bool:
        """Dense FedAvg of ``x`` while in warm-up; True if it ran (the anchor follows, residual empty)."""
        if self.dense_rounds >= self.warmup:
            return False
        if transport is not None:
            transport.allreduce_mean_(x)
        else:
            from .fedavg import allreduce_mean_

            allreduce_mean_(x, group)
        self.global_ref.copy_(x)
        self.residual.zero_()
        self.dense_rounds += 1
        self.bytes_sent += 4 * self.n
        self.dense_bytes += 4 * self.n
        self.rounds += 1
        return True

    def _delta(self, x: torch.Tensor) -> None:
        if self._nat is not None:
            self._nat.ef_delta(native.stream_handle(self.dev), x.data_ptr(), self.global_ref.data_ptr(),
                               self.residual.data_ptr(), self.d.data_ptr(), self.n)
        else:
            torch.sub(x, self.global_ref, out=self.d)
            self.d.add_(self.residual)


class TopKCompressor(_EFCompressor):
    def __init__(self, trainer, ratio: float = 0.01, warmup: int = 0):
        super().__init__(trainer, warmup)
        self.k = max(1, min(self.n, int(round(self.n * ratio))))
        self.idx = torch.empty(self.k, dtype=torch.int32, device=self.dev)
        self.val = torch.empty(self.k, dtype=torch.float32, device=self.dev)
        if self._nat is not None:
            self.state = torch.zeros(self._nat.topk_state_bytes(), dtype=torch.uint8, device=self.dev)
            # boundary-bin candidates (index, key) + the level-3 list: sized for the worst case (every
            # entry in one bin)
            self.cidx = torch.empty(2 * self.n, dtype=torch.int32, device=self.dev)
            self.ckey = torch.empty(2 * self.n, dtype=torch.int32, device=self.dev)

    def overflowed(self, clear: bool = True) -> bool:
        """True if a select ever produced more than k entries (the excess was dropped, never written
        past the payload; a kernel bug, not a data condition).  Synchronous; read at end of run."""
        if self._nat is None:
            return False
        off = int(self._nat.topk_overflow_offset())
        word = self.state[off:off + 4].view(torch.int32)
        hit = bool(word.item())
        if clear and hit:
            word.zero_()
        return hit

    def compress(self, x: torch.Tensor) -> None:
        if self._nat is not None:
            # d = x - global + residual is built IN the residual buffer; the winners are zeroed there
            self._nat.topk_ef(native.stream_handle(self.dev), x.data_ptr(), self.global_ref.data_ptr(),
                              self.residual.data_ptr(), self.n, self.k, self.state.data_ptr(), self.cidx.data_ptr(),
                              self.ckey.data_ptr(), self.idx.data_ptr(), self.val.data_ptr())
            return
        self._delta(x)
        sel = self.d.abs().topk(self.k, sorted=False).indices
        self.idx.copy_(sel.to(torch.int32))
        self.val.copy_(self.d[sel])
        self.residual.copy_(self.d)
        self.residual[sel] = 0.0

    def aggregate(self, trainer, group=None, transport=None) -> None:
        x = trainer.float_state()
        if self._dense(x, group, transport):
            return
        self.compress(x)
        _probe("topk")
        w = transport.world if transport is not None else _world(group)
        idx_all = _all_gather_flat(self.idx, group, transport)
        _probe("gather-idx")
        val_all = _all_gather_flat(self.val, group, transport)
        _probe("gather-val")
        self.bytes_sent += 8 * self.k
        self.dense_bytes += 4 * self.n
        self.rounds += 1
        if self._nat is not None:
            self._nat.scatter_add_ranked(native.stream_handle(self.dev), self.global_ref.data_ptr(),
                                         idx_all.data_ptr(), val_all.data_ptr(), w, self.k, 1.0 / w, self.n)
        else:
            scale = torch.tensor(1.0 / w, dtype=torch.float32, device=self.dev)
            for r in range(w):                 # rank order and one fma per entry, like the GPU path
                j = idx_all[r].long()          # (unique within a rank)
                self.global_ref[j] = _fma32(scale, val_all[r], self.global_ref[j])
        x.copy_(self.global_ref)
        _probe("scatter")


class Int8Compressor(_EFCompressor):
    CHUNK = 256

    def __init__(self, trainer, warmup: int = 0):
        super().__init__(trainer, warmup)
        self.nchunks = (self.n + self.CHUNK - 1) // self.CHUNK
        self.q = torch.empty(self.n, dtype=torch.int8, device=self.dev)
        self.scales = torch.empty(self.nchunks, dtype=torch.float32, device=self.dev)

    def compress(self, x: torch.Tensor) -> None:
        self._delta(x)
        if self._nat is not None:
            self._nat.quant_int8(native.stream_handle(self.dev), self.d.data_ptr(), self.n, self.q.data_ptr(),
                                 self.scales.data_ptr(), self.residual.data_ptr())
        else:
            pad = torch.zeros(self.nchunks * self.CHUNK, device=self.dev)
            pad[:self.n] = self.d
            blocks = pad.view(self.nchunks, self.CHUNK)
            amax = blocks.abs().amax(1)
            t = amax / torch.full_like(amax, 127.0)      # a true fp32 division (not a product with 1 / 127)
            s = torch.where(t > 0, t, torch.ones_like(t))   # t == 0: a zero chunk, or amax / 127 underflowed
            q = torch.round(blocks / s[:, None]).clamp_(-127, 127)
            self.q.copy_(q.view(-1)[:self.n].to(torch.int8))
            self.scales.copy_(s)
            self.residual.copy_(_fma32(-q, s[:, None], blocks).view(-1)[:self.n])

    # the fused peer kernel (quantise + exchange + dequantise-average in one launch); False: the unfused
    # reference path (tests compare the two bit for bit)
    fused = True

    def aggregate(self, trainer, group=None, transport=None) -> None:
        x = trainer.float_state()
        if self._dense(x, group, transport):
            return
        if self.fused and transport is not None and hasattr(transport, "int8_ef_allreduce_"):
            transport.int8_ef_allreduce_(x, self.global_ref, self.residual)
            self.bytes_sent += self.n + 4 * self.nchunks
            self.dense_bytes += 4 * self.n
            self.rounds += 1
            return
        self.compress(x)
        w = transport.world if transport is not None else _world(group)
        q_all = _all_gather_flat(self.q, group, transport)
        s_all = _all_gather_flat(self.scales, group, transport)
        self.bytes_sent += self.n + 4 * self.nchunks
        self.dense_bytes += 4 * self.n
        self.rounds += 1
        if self._nat is not None:
            self._nat.dequant_accum(native.stream_handle(self.dev), q_all.data_ptr(), s_all.data_ptr(), w, self.n,
                                    self.global_ref.data_ptr(), 1.0 / w)
        else:
            idx = torch.arange(self.n, device=self.dev) // self.CHUNK
            acc = torch.zeros_like(self.global_ref)
            for r in range(w):                 # rank order, one fma per rank and entry, like the kernels
                acc = _fma32(q_all[r], s_all[r][idx], acc)
            scale = torch.tensor(1.0 / w, dtype=torch.float32, device=self.dev)
            self.global_ref.copy_(_fma32(scale, acc, self.global_ref))
        x.copy_(self.global_ref)


DEFAULT_POWERSGD_RANK = 4
MAX_POWERSGD_RANK = 8
_PSGD_KEY = 0x706F776572736764        # "powersgd": the fixed Philox key of Q's start


def check_powersgd_rank(rank) -> int:
    if int(rank) != rank or not 1 <= int(rank) <= MAX_POWERSGD_RANK:
        raise ValueError(f"powersgd rank must be an integer in 1..{MAX_POWERSGD_RANK}, got {rank!r}")
    return int(rank)


def psgd_segments(trainer, rank: int) -> Tuple[List[Tuple[int, int, int]], List[Tuple[int, int]]]:
    """``(compressed, dense)`` of the trainer's float state: compressed = [(offset, rows, cols)] of the state dict's
    matrices that are worth a rank-``rank`` factorisation (min(rows, cols) > rank and
    2 rank (rows + cols) <= rows cols), dense = [(offset, length)] of everything else, merged, both in offset order."""
    flat = trainer.float_state()
    base, n = flat.data_ptr(), flat.numel()
    views = []
    for name, t in trainer.state_dict().items():
        if not torch.is_floating_point(t):
            continue
        byte_off = t.data_ptr() - base
        if (t.dtype != torch.float32 or t.device != flat.device or not t.is_contiguous() or byte_off % 4
                or byte_off < 0 or byte_off // 4 + t.numel() > n):
            raise ValueError(f"powersgd: state dict entry {name!r} is not a contiguous fp32 view into the trainer's "
                             "float state, so its matrices cannot be located")
        views.append((byte_off // 4, name, t))
    views.sort(key=lambda v: v[0])
    end = 0
    comp, dense = [], []
    for off, name, t in views:
        if off != end:
            raise ValueError(f"powersgd: the state dict does not tile the float state ({name!r} starts at entry {off}, "
                             f"the entry before it ends at {end})")
        end = off + t.numel()
        rows = t.shape[0] if t.ndim >= 2 else 0
        cols = t.numel() // rows if rows else 0
        if rows and min(rows, cols) > rank and 2 * rank * (rows + cols) <= rows * cols:
            comp.append((off, rows, cols))
        elif t.numel():
            if dense and dense[-1][0] + dense[-1][1] == off:
                dense[-1] = (dense[-1][0], dense[-1][1] + t.numel())
            else:
                dense.append((off, t.numel()))
    if end != n:
        raise ValueError(f"powersgd: the state dict does not tile the float state (it ends at entry {end} of {n})")
    return comp, dense


def psgd_layout(comp, dense, rank: int):
    """Offsets of every segment's P and Q in their buffers and of every dense range behind P in the send buffer:
    ``(poffs, qoffs, doffs, n_p, n_q, n_dense)``."""
    poffs, qoffs, doffs = [], [], []
    n_p = n_q = 0
    for _, rows, cols in comp:
        poffs.append(n_p)
        qoffs.append(n_q)
        n_p += rows * rank
        n_q += cols * rank
    n_dense = 0
    for _, ln in dense:
        doffs.append(n_p + n_dense)
        n_dense += ln
    return poffs, qoffs, doffs, n_p, n_q, n_dense


def _ceil(a: int, b: int) -> int:
    return -(-a // b)


def psgd_tables(comp, dense, rank: int, n: int, geo: dict) -> dict:
    """The device tables of csrc/kernels/powersgd.hip as numpy records (``geo``: the extension's ``psgd_geometry()``).
    Every segment and dense range must lie inside ``[0, n)`` and none may overlap another: the kernels trust the
    tables.  Work is handed out in tiles of about slab x tile_rows (back_cols x back_rows) entries; a row longer than
    one slab (a matrix taller than one row chunk) is cut into pieces of equal size whose partials a fold job adds."""
    spans = sorted([(o, o + r * c) for o, r, c in comp] + [(o, o + ln) for o, ln in dense])
    for i, (a, b) in enumerate(spans):
        if a < 0 or b > n or b <= a or (i and a < spans[i - 1][1]):
            raise ValueError(f"powersgd: segment [{a}, {b}) is empty, outside the {n} entries or overlaps its neighbour")
    seg_t = np.dtype([("off", "<i8"), ("poff", "<i8"), ("qoff", "<i8"), ("rows", "<i4"), ("cols", "<i4")])
    tile_t = np.dtype([("seg", "<i4"), ("r0", "<i4"), ("r1", "<i4"), ("c0", "<i4"), ("c1", "<i4"), ("pad", "<i4"),
                       ("part", "<i8"), ("aux", "<i8")])
    fold_t = np.dtype([("dst", "<i8"), ("src", "<i8"), ("stride", "<i8"), ("cnt", "<i4"), ("nparts", "<i4")])
    if (seg_t.itemsize, tile_t.itemsize, fold_t.itemsize) != (geo["seg_bytes"], geo["tile_bytes"], geo["fold_bytes"]):
        raise RuntimeError("powersgd: the table records do not match the extension's")
    poffs, qoffs, doffs, n_p, n_q, n_dense = psgd_layout(comp, dense, rank)
    segs = [(o, poffs[i], qoffs[i], r, c) for i, (o, r, c) in enumerate(comp)]
    ptiles, btiles, pfolds, qfolds = [], [], [], []
    n_ppart = n_qpart = 0

    def folds(out, dst, src, cnt, nparts):
        for k in range(0, cnt, geo["fold"]):
            out.append((dst + k, src + k, cnt, min(geo["fold"], cnt - k), nparts))

    for i, (_, rows, cols) in enumerate(comp):
        nslab = _ceil(cols, geo["slab"])
        wslab = _ceil(_ceil(cols, nslab), 16) * 16
        for r0 in range(0, rows, geo["tile_rows"]):
            for sl in range(nslab):
                if sl * wslab < cols:
                    part = n_ppart + sl * rows * rank if nslab > 1 else -1
                    ptiles.append((i, r0, min(rows, r0 + geo["tile_rows"]), sl * wslab, min(cols, (sl + 1) * wslab), 0,
                                   part, 0))
        if nslab > 1:
            folds(pfolds, poffs[i], n_ppart, rows * rank, nslab)
            n_ppart += nslab * rows * rank
        nchunk = _ceil(rows, geo["back_rows"])
        chunk = _ceil(_ceil(rows, nchunk), 4) * 4
        for c0 in range(0, cols, geo["back_cols"]):
            for ch in range(nchunk):
                if ch * chunk < rows:
                    part = n_qpart + ch * cols * rank if nchunk > 1 else -1
                    btiles.append((i, ch * chunk, min(rows, (ch + 1) * chunk), c0, min(cols, c0 + geo["back_cols"]), 0,
                                   part, 0))
        if nchunk > 1:
            folds(qfolds, qoffs[i], n_qpart, cols * rank, nchunk)
            n_qpart += nchunk * cols * rank
    for (off, ln), dst in zip(dense, doffs):
        for k in range(0, ln, geo["dense"]):
            ptiles.append((-1, 0, 0, 0, min(geo["dense"], ln - k), 0, off + k, dst + k))
    return {"segs": np.array(segs, dtype=seg_t), "project": np.array(ptiles, dtype=tile_t),
            "backproject": np.array(btiles, dtype=tile_t), "pfolds": np.array(pfolds, dtype=fold_t),
            "qfolds": np.array(qfolds, dtype=fold_t), "n_p": n_p, "n_q": n_q, "n_dense": n_dense,
            "n_ppart": n_ppart, "n_qpart": n_qpart}


class PowerSGDCompressor(_EFCompressor):
    """Rank-``rank`` PowerSGD with error feedback (module docstring).  The three phases are methods so that several
    in-process compressors can be driven side by side with a plain mean between them; :meth:`aggregate` strings them
    together with the two collectives."""

    def __init__(self, trainer, rank: int = DEFAULT_POWERSGD_RANK, warmup: int = 0):
        self.rank = check_powersgd_rank(rank)
        super().__init__(trainer, warmup)
        self.segments, self.dense_ranges = psgd_segments(trainer, self.rank)
        self.poffs, self.qoffs, self.doffs, self.n_p, self.n_q, self.n_dense = psgd_layout(
            self.segments, self.dense_ranges, self.rank)
        self.send = torch.zeros(self.n_p + self.n_dense, dtype=torch.float32, device=self.dev)   # P, then the dense part
        self.q = torch.zeros(max(self.n_q, 1), dtype=torch.float32, device=self.dev)[:self.n_q]
        if self._nat is not None:
            tb = psgd_tables(self.segments, self.dense_ranges, self.rank, self.n, self._nat.psgd_geometry())
            self._tb = {k: torch.from_numpy(v.view(np.uint8).reshape(-1).copy()).to(self.dev)
                        for k, v in tb.items() if isinstance(v, np.ndarray)}
            self._cnt = {k: len(v) for k, v in tb.items() if isinstance(v, np.ndarray)}
            self.ppart = torch.empty(tb["n_ppart"], dtype=torch.float32, device=self.dev)
            self.qpart = torch.empty(tb["n_qpart"], dtype=torch.float32, device=self.dev)
        self._fill_q()

    @property
    def payload_bytes(self) -> int:
        return 4 * (self.n_p + self.n_q + self.n_dense)

    def _fill_q(self) -> None:
        """Standard normals under a fixed key: the same Q on every client, nothing exchanged."""
        if self._nat is not None:
            self._nat.psgd_qinit(native.stream_handle(self.dev), self.q.data_ptr(), self.n_q, _PSGD_KEY)
        else:
            self.q.copy_(torch.randn(self.n_q, generator=torch.Generator().manual_seed(_PSGD_KEY)))

    def reset(self, trainer) -> None:
        super().reset(trainer)
        self._fill_q()

    def _mat(self, buf: torch.Tensor, i: int) -> torch.Tensor:
        off, rows, cols = self.segments[i]
        return buf[off:off + rows * cols].view(rows, cols)

    def _p(self, buf: torch.Tensor, i: int) -> torch.Tensor:
        return buf[self.poffs[i]:self.poffs[i] + self.segments[i][1] * self.rank].view(-1, self.rank)

    def _q(self, buf: torch.Tensor, i: int) -> torch.Tensor:
        return buf[self.qoffs[i]:self.qoffs[i] + self.segments[i][2] * self.rank].view(-1, self.rank)

    def phase1(self, x: torch.Tensor) -> torch.Tensor:
        """d = (x - global) + residual (left in ``residual``), P = M Q and the dense entries of d into :attr:`send`."""
        if self._nat is not None:
            t, c = self._tb, self._cnt
            self._nat.psgd_project(native.stream_handle(self.dev), x.data_ptr(), self.global_ref.data_ptr(),
                                   self.residual.data_ptr(), t["segs"].data_ptr(), t["project"].data_ptr(), c["project"],
                                   self.q.data_ptr(), self.rank, self.send.data_ptr(), self.ppart.data_ptr(),
                                   t["pfolds"].data_ptr(), c["pfolds"])
            return self.send
        self._delta(x)
        self.residual.copy_(self.d)
        for i in range(len(self.segments)):
            torch.mm(self._mat(self.residual, i), self._q(self.q, i), out=self._p(self.send, i))
        for (off, ln), dst in zip(self.dense_ranges, self.doffs):
            self.send[dst:dst + ln] = self.residual[off:off + ln]
        return self.send

    def phase2(self, pbar: torch.Tensor) -> torch.Tensor:
        """``pbar``: the averaged send buffer.  P^ = orth(P-) in place, Q = M^T P^ into :attr:`q`."""
        if pbar.data_ptr() != self.send.data_ptr():
            self.send.copy_(pbar)
        if self._nat is not None:
            t, c, s = self._tb, self._cnt, native.stream_handle(self.dev)
            self._nat.psgd_orth(s, t["segs"].data_ptr(), c["segs"], self.send.data_ptr(), self.rank)
            self._nat.psgd_backproject(s, self.residual.data_ptr(), t["segs"].data_ptr(), t["backproject"].data_ptr(),
                                       c["backproject"], self.send.data_ptr(), self.rank, self.q.data_ptr(),
                                       self.qpart.data_ptr(), t["qfolds"].data_ptr(), c["qfolds"])
            return self.q
        for i in range(len(self.segments)):
            p = self._p(self.send, i)
            for a in range(self.rank):           # modified Gram-Schmidt in column order (the paper's orthogonalize)
                col = p[:, a]
                col.div_((col.double().square().sum().sqrt() + 1e-8).float())
                for b in range(a + 1, self.rank):
                    dot = (col.double() * p[:, b].double()).sum().float()
                    p[:, b] = _fma32(-dot.expand_as(col), col, p[:, b])
            torch.mm(self._mat(self.residual, i).t(), p, out=self._q(self.q, i))
        return self.q

    def phase3(self, x: torch.Tensor, qbar: torch.Tensor) -> None:
        """``qbar``: the averaged Q (kept as the next round's).  global += P^ Q-^T (dense: += the averaged entries),
        x = global, residual = d - P^ Q-^T (dense: 0)."""
        if qbar.data_ptr() != self.q.data_ptr():
            self.q.copy_(qbar)
        if self._nat is not None:
            t, c = self._tb, self._cnt
            self._nat.psgd_apply(native.stream_handle(self.dev), x.data_ptr(), self.global_ref.data_ptr(),
                                 self.residual.data_ptr(), t["segs"].data_ptr(), t["project"].data_ptr(), c["project"],
                                 self.send.data_ptr(), self.q.data_ptr(), self.send.data_ptr(), self.rank)
            return
        for i in range(len(self.segments)):
            p, q = self._p(self.send, i), self._q(self.q, i)
            g, r = self._mat(self.global_ref, i), self._mat(self.residual, i)
            u = torch.zeros_like(g)
            for j in range(self.rank):           # R fmas in j order from 0
                u = _fma32(p[:, j:j + 1].expand_as(u), q[:, j].expand_as(u), u)
            g.add_(u)
            r.sub_(u)
        for (off, ln), dst in zip(self.dense_ranges, self.doffs):
            self.global_ref[off:off + ln] += self.send[dst:dst + ln]
            self.residual[off:off + ln] = 0.0
        x.copy_(self.global_ref)

    def aggregate(self, trainer, group=None, transport=None) -> None:
        x = trainer.float_state()
        if self._dense(x, group, transport):
            return

        def mean_(t):
            if transport is not None:
                transport.allreduce_mean_(t)
            else:
                from .fedavg import allreduce_mean_

                allreduce_mean_(t, group)

        mean_(self.phase1(x))
        _probe("psgd-p")
        mean_(self.phase2(self.send))
        _probe("psgd-q")
        self.phase3(x, self.q)
        self.bytes_sent += self.payload_bytes
        self.dense_bytes += 4 * self.n
        self.rounds += 1


# What ``-c Y`` selects: the compressor that stays within 3 points of dense FedAvg at the fewest bytes on the
# 8-rank rehearsal (profiles/r5_dataplane/: 3 seeds x 23 rounds) -- int8 + error feedback, a quarter of the dense
# bytes; top-k needs ~20 % of the entries (40 % of the dense bytes: 8 B per kept entry) to get as close.
DEFAULT_Y = "int8"
DEFAULT_TOPK_RATIO = 0.2


def make_compressor(kind: Optional[str], ratio: float, trainer, warmup: int = 0,
                    powersgd_rank: int = DEFAULT_POWERSGD_RANK):
    if kind == "powersgd":
        return PowerSGDCompressor(trainer, powersgd_rank, warmup)
    if kind in (None, "", "none", "n", "N"):
        return None
    if kind in ("Y", "y"):
        kind = DEFAULT_Y
    if kind == "topk":
        return TopKCompressor(trainer, ratio, warmup)
    if kind == "int8":
        return Int8Compressor(trainer, warmup)
    raise ValueError(f"unknown compression {kind!r}")
