"""Op-by-op shadow of the CNN kernels (tests only).

:func:`shadow` wraps whatever is bound to the kernel entry points of
:mod:`fedmi.ops.conv` / :mod:`fedmi.ops.cnn` (the names :func:`emulate.emulated`
swaps).  Every call then runs twice on the same inputs: the bound function on
the real buffers, untouched, and the PyTorch emulation (tests/emulate.py) on
snapshots of everything the op reads and writes.  All outputs and all mutated
state are compared, per call, so an error cannot compound through the network
and exactly the launches an engine issues are covered: shapes, strides, flags,
channel-slice views, in-place destinations.

The engine never sees a difference: the real buffers hold what the bound call
wrote, the emulation only touches clones.

Tolerances (none of them new, see the tests they come from):

* bf16 tensors and fp32 gradients: ``max|a-b| / (max|b| + 1e-6) < 1e-2`` (``_rel`` of
  test_cnn_kernels_gpu.py) and a relative L2 error < 1e-2.  Both sides round to bf16 at the same
  points; at most three roundings separate them.
* conv / depthwise statistics: the delta of the replica totals against fp64 sums of the op's own
  output, within 1e-3 of sum|v| (first row) and of sum v^2 (second row), per channel.
* BN saved / running statistics, dgamma, dbeta, the stored scale / shift: ``allclose(rtol=1e-3,
  atol=1e-5)`` (the wiring test); num_batches_tracked, the statistics shift and untouched state exact.
* prep_input: ``allclose(atol=2e-2)`` as its kernel test; padded channels exactly 0.
* head: loss within 1e-3 * max(1, |loss|), count exact, correct count within the number of rows whose
  top-two logits lie within 1e-2 of the row's max |logit|; gradients by the bf16 / fp32 rule.
* pools: forwards and ``maxpool2_bwd`` exact (first maximum, torch's rule); ``maxpool3_bwd`` sums up to
  nine bf16 grads per element, so it takes the bf16 rule.
* ``bn_bwd`` with ``mask_bn``: elements with ``|z*sc+sh| <= 1e-5 * (|z*sc| + |sh|)`` (the mask can flip
  between an fma and an unfused evaluation) are left out of the dz / gout comparison; their share per call
  must stay <= 1e-3.
"""
from __future__ import annotations

import contextlib
import functools
import inspect
import json
import sys
from pathlib import Path

import torch

if __name__ == "__main__":     # run as a script from anywhere: the package lives one level up
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import emulate
from fedmi.ops import cnn, conv

CONV_OPS = ("conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad", "wgrad_reduce_multi", "dwconv_fwd", "dwconv_dgrad",
            "dwconv_wgrad")
CNN_OPS = ("prep_input", "bn_apply", "bn_bwd", "head", "maxpool2", "maxpool2_bwd", "maxpool3", "maxpool3_bwd")
ALL_OPS = CONV_OPS + CNN_OPS

_BN_STATE = ("stats", "smean", "sinv", "rmean", "rvar", "nbt", "shift")


class ShadowMismatch(AssertionError):
    pass


def _span(t: torch.Tensor):
    """[lo, hi) byte range a (possibly strided) tensor can touch."""
    if t.numel() == 0:
        return 0, 0
    n = sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1
    return t.data_ptr(), t.data_ptr() + n * t.element_size()


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    (la, ha), (lb, hb) = _span(a), _span(b)
    return la < hb and lb < ha


def _sig(**kw) -> str:
    parts = []
    for k, v in kw.items():
        if v is None:
            continue
        if isinstance(v, torch.Tensor):
            s = "x".join(map(str, v.shape))
            parts.append(f"{k}={s}" if v.is_contiguous() else f"{k}={s}/ld{v.stride(-2)}")
        elif k == "opt":
            if v:
                parts.append("+" + "+".join(v))
        elif isinstance(v, (tuple, list, torch.Size)):
            parts.append(f"{k}=" + "x".join(str(int(i)) for i in v))
        else:
            parts.append(f"{k}={v}")
    return " ".join(parts)


def _present(A: dict, names) -> list:
    def on(v):
        return v is not None and (isinstance(v, (torch.Tensor, dict, list)) or bool(v))

    return [n for n in names if on(A.get(n))]


def _worse(old, v):
    if old is None or v != v:
        return v
    return old if (old != old or old >= v) else v


class Shadow:
    """State of one ``shadow()`` block: the per-(op, signature) table, the mismatches, pending comparisons."""

    def __init__(self, collect: bool = False, ref_device=None):
        self.collect = collect
        self.ref_device = torch.device(ref_device) if ref_device is not None else None
        self.table: dict = {}        # (op, sig) -> {"count": calls, "worst": {"tensor:metric": value}}
        self.failures: list = []
        self._checks: list = []
        self._pending: list = []     # deferred WGRADs: (op, sig, out, expected)
        self._pool_in: dict = {}     # maxpool3 idx.data_ptr() -> clone of the pool's input
        self._native = False         # the bound functions are not the emulation: weights from the packed image

    # ---- bookkeeping -----------------------------------------------------------------------
    def ops(self) -> set:
        return {op for op, _ in self.table}

    def signatures(self, op: str) -> list:
        return [s for o, s in self.table if o == op]

    def dump(self) -> list:
        return [[op, sig, e["count"], e["worst"]] for (op, sig), e in self.table.items()]

    def _fail(self, msg: str) -> None:
        if not self.collect:
            raise ShadowMismatch(msg)
        self.failures.append(msg)

    def _check(self, name: str, metric: str, value: torch.Tensor, limit, lt: bool = False) -> None:
        self._checks.append((name, metric, value.detach().double().reshape(()), limit, lt))

    def _flush(self, op: str, sig: str) -> None:
        ent = self.table.setdefault((op, sig), {"count": 0, "worst": {}})
        ent["count"] += 1
        checks, self._checks = self._checks, []
        if not checks:
            return
        dev = checks[0][2].device
        vals = torch.stack([c[2].to(dev) for c in checks]).tolist()     # one sync per op
        for (name, metric, _, limit, lt), v in zip(checks, vals):
            key = f"{name}:{metric}"
            ent["worst"][key] = _worse(ent["worst"].get(key), v)
            if not (v < limit if lt else v <= limit):
                self._fail(f"{op} [{sig}] {name}: {metric} = {v:.4g} (limit {'<' if lt else '<='} {limit:g})")

    # ---- snapshots / reference placement ----------------------------------------------------
    def _R(self, t):
        if t is None or self.ref_device is None or not isinstance(t, torch.Tensor):
            return t
        return t.detach().to(self.ref_device)

    def _snap(self, t):
        return None if t is None else self._R(t.detach().clone())

    def _inputs(self, ins: dict, outs) -> dict:
        """Reference-side inputs; one that overlaps an output is cloned before the bound call can change it."""
        outs = [o for o in outs if isinstance(o, torch.Tensor)]
        res = {}
        for k, t in ins.items():
            if isinstance(t, torch.Tensor) and any(_overlap(t, o) for o in outs):
                t = t.detach().clone()
            res[k] = t
        return res

    def _bn_copy(self, p):
        if p is None:
            return None
        kw = {k: getattr(p, k) for k in cnn.BNParams.__slots__}
        for k in kw:
            kw[k] = self._snap(kw[k]) if k in _BN_STATE else self._R(kw[k])
        return cnn.BNParams(**kw)

    def _emul(self, name: str, *a, **k):
        saved, lib = emulate._MASTER, torch.backends.cudnn.enabled
        if self._native:
            emulate._MASTER = {}
        try:
            # torch's own im2col / depthwise kernels on the GPU, not the vendor convolution library: its solver
            # search runs candidate kernels per new shape (slow on first use, and one of them faulted on a 1x1
            # data gradient with 160 channels fed a channels-last fp32 view)
            torch.backends.cudnn.enabled = False
            return getattr(emulate, name)(*a, **k)
        finally:
            emulate._MASTER, torch.backends.cudnn.enabled = saved, lib

    # ---- comparisons -------------------------------------------------------------------------
    @staticmethod
    def _pair(got, ref):
        return got.detach().double(), ref.detach().to(got.device).double()

    def _close(self, name, got, ref, excl=None) -> None:
        """bf16 tensors / fp32 gradients: max error relative to the reference's max, and relative L2."""
        if tuple(got.shape) != tuple(ref.shape):
            return self._check(name, "shape_mismatch", torch.ones(()), 0)
        if got.numel() == 0:
            return
        a, b = self._pair(got, ref)
        if excl is not None:
            a = torch.where(excl.reshape(a.shape), b, a)
        d = a - b
        self._check(name, "rel_max", d.abs().max() / (b.abs().max() + 1e-6), 1e-2, lt=True)
        self._check(name, "rel_l2", d.norm() / (b.norm() + 1e-6), 1e-2, lt=True)

    @staticmethod
    def _diff(a, b):
        """|a - b|, 0 where both hold the same value (equal NaNs of never-written state included)."""
        same = (a == b) | (a.isnan() & b.isnan())
        return torch.where(same, torch.zeros_like(a), (a - b).abs()), same

    def _allclose(self, name, got, ref, rtol=1e-3, atol=1e-5) -> None:
        if got.numel() == 0:
            return
        a, b = self._pair(got, ref)
        d, _ = self._diff(a, b)
        r = d / (atol + rtol * b.abs())
        self._check(name, "tol_ratio", torch.where(r.isnan(), torch.full_like(r, float("inf")), r).max(), 1.0)

    def _exact(self, name, got, ref, metric="mismatches") -> None:
        if got.numel() == 0:
            return
        a, b = self._pair(got, ref)
        self._check(name, metric, (~self._diff(a, b)[1]).sum(), 0)

    def _stats(self, name, stats, st0, y, shift) -> None:
        """Delta of the replica totals vs fp64 sums of the op's own output, scale-free per channel."""
        R = conv.STAT_REP
        delta = (stats.view(R, 2, -1).double() - st0.to(stats.device).view(R, 2, -1).double()).sum(0)
        ref = emulate.stats_sums(y, shift)
        v = y.double().reshape(-1, y.shape[-1])
        if shift is not None:
            v = v - shift.double()
        err = (delta - ref).abs()
        err = torch.where(err.isnan(), torch.full_like(err, float("inf")), err)
        self._check(name, "stats_sum", (err[0] / v.abs().sum(0).clamp_min(1e-300)).max(), 1e-3)
        self._check(name, "stats_sq", (err[1] / ref[1].clamp_min(1e-300)).max(), 1e-3)

    def _bn_cmp(self, name, p, pe) -> None:
        for k in ("smean", "sinv", "rmean", "rvar"):
            if getattr(p, k) is not None:
                self._allclose(f"{name}.{k}", getattr(p, k), getattr(pe, k))
        for k in ("nbt", "shift", "stats"):
            if getattr(p, k) is not None:
                self._exact(f"{name}.{k}", getattr(p, k), getattr(pe, k))

    # ---- the ops ---------------------------------------------------------------------------------
    def _run_emul(self, op, sig, name, *a, **k):
        try:
            return self._emul(name, *a, **k), True
        except ValueError as e:      # the emulation's mirror of a host-side check disagrees with the bound call
            self._check("emulation", "rejected", torch.ones(()), 0)
            self._flush(op, sig + f" ({e})")
            return None, False

    def conv2d_fwd(self, call, A):
        x, wr, out, stats, shift, res = A["x"], A["wrsc"], A["out"], A["stats"], A["shift"], A["res"]
        sig = _sig(x=x, w=wr, stride=A["stride"], pad=A["pad"], Cw=A["Cw"],
                   opt=_present(A, ("stats", "shift", "ws", "res")))
        out0, st0 = self._snap(out), self._snap(stats)
        ins = self._inputs(dict(x=x, wr=wr, res=res), (out, stats))
        y = call()
        e = self._emul("conv2d_fwd", self._R(ins["x"]), self._R(ins["wr"]), A["stride"], A["pad"], Cw=A["Cw"], out=out0,
                       res=self._R(ins["res"]))
        self._close("out", y, e)
        if stats is not None:
            self._stats("stats", stats, st0, y, shift)
        self._flush("conv2d_fwd", sig)
        return y

    def dwconv_fwd(self, call, A):
        x, w, out, stats, shift = A["x"], A["w"], A["out"], A["stats"], A["shift"]
        sig = _sig(x=x, w=w, stride=A["stride"], pad=A["pad"], opt=_present(A, ("stats", "shift")))
        out0, st0 = self._snap(out), self._snap(stats)
        ins = self._inputs(dict(x=x), (out, stats))
        y = call()
        e = self._emul("dwconv_fwd", self._R(ins["x"]), self._R(w), A["stride"], A["pad"], out=out0)
        self._close("out", y, e)
        if stats is not None:
            self._stats("stats", stats, st0, y, shift)
        self._flush("dwconv_fwd", sig)
        return y

    def conv2d_dgrad(self, call, A):
        dy, wr, out, add = A["dy"], A["wrsc"], A["out"], A["add"]
        sig = _sig(dy=dy, w=wr, x=tuple(A["x_shape"]), stride=A["stride"], pad=A["pad"], Cw=A["Cw"],
                   opt=_present(A, ("ws", "wd", "accumulate", "add", "bn_sums"))
                   + (["msc"] if A["bn_sums"] and A["bn_sums"].get("msc") is not None else [])
                   + (["zb"] if A["bn_sums"] and A["bn_sums"].get("zb") is not None else []))
        out0 = self._snap(out)
        ins = self._inputs(dict(dy=dy, add=add), (out,))
        dx = call()
        e, ok = self._run_emul("conv2d_dgrad", sig, "conv2d_dgrad", self._R(ins["dy"]), self._R(wr),
                               tuple(A["x_shape"]), A["stride"], A["pad"], Cw=A["Cw"], out=out0, wd=A["wd"],
                               accumulate=A["accumulate"], add=self._R(ins["add"]), bn_sums=A["bn_sums"])
        if ok:
            # accumulate / add: the sum is rounded once more than a plain dx (still <= 3 bf16 roundings apart)
            self._close("dx", dx, e)
            self._flush("conv2d_dgrad", sig)
        return dx

    def dwconv_dgrad(self, call, A):
        dy, w, out = A["dy"], A["w"], A["out"]
        sig = _sig(dy=dy, w=w, x=tuple(A["x_shape"]), stride=A["stride"], pad=A["pad"],
                   opt=_present(A, ("bn_sums",)))
        out0 = self._snap(out)
        ins = self._inputs(dict(dy=dy), (out,))
        dx = call()
        e = self._emul("dwconv_dgrad", self._R(ins["dy"]), self._R(w), tuple(A["x_shape"]), A["stride"], A["pad"],
                       out=out0)
        self._close("dx", dx, e)
        self._flush("dwconv_dgrad", sig)
        return dx

    def _wgrad(self, op, sig, call, A, dw_of):
        """Shared by the dense and depthwise WGRAD: ``dw_of()`` is the emulated dW of this call.  A call that
        defers its reduction leaves ``out`` unwritten: the comparison waits for wgrad_reduce_multi."""
        out, deferred = A["out"], A["deferred"]
        out0 = self._snap(out)
        dw = dw_of()                     # now: the engine reuses x / dy before the deferred reduction runs
        n0 = len(deferred) if deferred is not None else 0
        ret = call()
        want = out0 + dw if (A["accumulate"] and out is not None) else dw
        if deferred is not None and len(deferred) > n0:
            self._pending.append((op, sig + " +deferred", ret, want))
        else:
            self._close("dw", ret, want)
            self._flush(op, sig)
        return ret

    def conv2d_wgrad(self, call, A):
        if A.get("Ow") is not None or A.get("groups", 1) != 1:
            raise NotImplementedError("shadow: conv2d_wgrad Ow / groups have no emulation")
        x, dy = A["x"], A["dy"]
        sig = _sig(x=x, dy=dy, R=A["R"], S=A["S"], stride=A["stride"], pad=A["pad"], Cw=A["Cw"],
                   opt=_present(A, ("accumulate", "splits", "ws")) + ([] if A["lib_gemm"] else ["no_lib_gemm"]))
        return self._wgrad("conv2d_wgrad", sig, call, A,
                           lambda: self._emul("conv2d_wgrad", self._R(x), self._R(dy), A["R"], A["S"], A["stride"],
                                              A["pad"], Cw=A["Cw"]))

    def dwconv_wgrad(self, call, A):
        x, dy = A["x"], A["dy"]
        sig = _sig(x=x, dy=dy, R=A["R"], stride=A["stride"], pad=A["pad"], opt=_present(A, ("accumulate", "ws")))
        return self._wgrad("dwconv_wgrad", sig, call, A,
                           lambda: self._emul("dwconv_wgrad", self._R(x), self._R(dy), A["R"], A["stride"], A["pad"]))

    def wgrad_reduce_multi(self, call, A):
        n = len(A["items"])
        ret = call()
        pend, self._pending = self._pending, []
        for op, sig, out, want in pend:
            self._close("dw", out, want)
            self._flush(op, sig)
        self._flush("wgrad_reduce_multi", f"items={'0' if not n else '1-32' if n <= 32 else '>32'}")
        return ret

    def prep_input(self, call, A):
        sig = _sig(nb=A["nb"], augment=bool(A["augment"]), opt=_present(A, ("dbase",)))
        out = call()
        e = self._emul("prep_input", self._R(A["images_u8"]), A["base"], A["nb"], A["augment"], A["seed"],
                       self._R(A["round_ctr"]), dbase=self._R(A["dbase"]))
        self._allclose("rgb", out[..., :3], e[..., :3], rtol=1e-5, atol=2e-2)
        self._check("pad", "max_abs", out[..., 3:].double().abs().max(), 0)
        self._flush("prep_input", sig)
        return out

    @staticmethod
    def _row_frame(y):
        """(full rows of the wider buffer a channel-slice view lives in, boolean mask of the columns outside it)."""
        if y is None or y.is_contiguous() or y.dim() < 2:
            return None
        C, ld = y.shape[-1], y.stride(-2)
        col0 = y.storage_offset() % ld
        if col0 + C > ld:
            return None
        try:
            full = torch.as_strided(y, (y.numel() // C, ld), (ld, 1), y.storage_offset() - col0)
        except RuntimeError:
            return None
        outside = torch.ones(ld, dtype=torch.bool, device=y.device)
        outside[col0:col0 + C] = False
        return full, outside

    def bn_apply(self, call, A):
        z, a, y, z2, b, res, co = A["z"], A["a"], A["y"], A["z2"], A["b"], A["res"], A["co_out"]
        sig = _sig(z=z, y=y, train=bool(A["train"]), relu=bool(A["relu"]),
                   opt=_present(A, ("z2", "res", "co_out")) + (["cbias"] if a.cbias is not None else []))
        ae, be, y0, co0 = self._bn_copy(a), self._bn_copy(b), self._snap(y), self._snap(co)
        frame = self._row_frame(y)
        frame0 = frame[0].clone() if frame else None
        ins = self._inputs(dict(z=z, z2=z2, res=res), (y, co))
        ret = call()
        self._emul("bn_apply", self._R(ins["z"]), ae, y0, A["train"], A["relu"], z2=self._R(ins["z2"]), b=be,
                   res=self._R(ins["res"]), eps=A["eps"], momentum=A["momentum"], co_out=co0)
        self._close("y", y, y0)
        if frame:     # a channel-slice write leaves the other branches' columns alone
            self._exact("y", frame[0][:, frame[1]], frame0[:, frame[1]], "outside_slice")
        self._bn_cmp("a", a, ae)
        if b is not None:
            self._bn_cmp("b", b, be)
        if co is not None:
            self._allclose("co_out", co, co0)
        self._flush("bn_apply", sig)
        return ret

    def bn_bwd(self, call, A):
        za, a, zb, b, msc = A["za"], A["a"], A["zb"], A["b"], A["mask_bn"]
        sig = _sig(dya=A["dya"], za=za, y=A["y"],
                   opt=_present(A, ("dyb", "zb", "gout", "ws", "dadd", "chained", "mask_bn", "presummed"))
                   + (["relu_y"] if A["y"] is not None else []))
        outs = ("dgamma_a", "dbeta_a", "dza", "dgamma_b", "dbeta_b", "dzb", "gout")
        E = {k: self._snap(A[k]) for k in outs}
        ae, be = self._bn_copy(a), self._bn_copy(b)
        ins = self._inputs({k: A[k] for k in ("dya", "za", "dyb", "y", "zb", "dadd", "mask_bn")},
                           [A[k] for k in outs] + [A["red"], A["ws"]])
        ret = call()
        self._emul("bn_bwd", self._R(ins["dya"]), self._R(ins["za"]), ae, E["dgamma_a"], E["dbeta_a"], E["dza"], None,
                   dyb=self._R(ins["dyb"]), y=self._R(ins["y"]), zb=self._R(ins["zb"]), b=be,
                   dgamma_b=E["dgamma_b"], dbeta_b=E["dbeta_b"], dzb=E["dzb"], gout=E["gout"],
                   dadd=self._R(ins["dadd"]), chained=A["chained"], mask_bn=self._R(ins["mask_bn"]),
                   presummed=A["presummed"])
        excl = None
        if msc is not None:
            C = za.shape[-1]
            t = ins["za"].double().reshape(-1, C) * ins["mask_bn"][0].double()
            sh = ins["mask_bn"][1].double()
            excl = (t + sh).abs() <= 1e-5 * (t.abs() + sh.abs())
            self._check("mask_bn", "excluded_share", excl.double().mean(), 1e-3)
        # the sums behind dgamma / dbeta / dz are the kernels' own (a reduce pass, or the DGRAD epilogue that
        # wrote dya: presummed); the emulation always recomputes them from dya
        for k in ("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b"):
            if A[k] is not None and (k.endswith("_a") or zb is not None):
                self._allclose(k, A[k], E[k])
        self._close("dza", A["dza"], E["dza"], excl)
        if zb is not None:
            self._close("dzb", A["dzb"], E["dzb"], excl)
        if A["gout"] is not None:
            self._close("gout", A["gout"], E["gout"], excl)
        self._bn_cmp("a", a, ae)
        if b is not None:
            self._bn_cmp("b", b, be)
        self._flush("bn_bwd", sig)
        return ret

    def head(self, call, A):
        y, W, bias, stats, train, zero = A["y"], A["W"], A["b"], A["stats"], A["train"], A["zero"]
        sig = _sig(y=y, J=W.shape[0], train=bool(train), opt=_present(A, ("dbase", "zero", "lossv")))
        outs = ("pooled", "dlog", "dy", "dW", "db")
        E = {k: self._snap(A[k]) for k in outs}
        st0 = stats.detach().clone()
        se = self._snap(stats)
        ret = call()
        self._emul("head", self._R(y), self._R(A["labels"]), A["base"], self._R(W), self._R(bias), se, train,
                   E["pooled"], E["dlog"], E["dy"], E["dW"], E["db"], dbase=self._R(A["dbase"]))
        se = se.to(stats.device)
        loss, loss_e = stats[0].double() - st0[0].double(), se[0].double() - st0[0].double()
        self._check("loss", "rel_to_max1", (loss - loss_e).abs() / loss_e.abs().clamp_min(1.0), 1e-3)
        iv, ie, i0 = stats.view(torch.int32), se.view(torch.int32), st0.view(torch.int32)
        self._exact("count", iv[2] - i0[2], ie[2] - i0[2])
        logits = y.detach().float().mean((1, 2)) @ W.detach().float().t() + bias.detach().float()
        top = logits.topk(2, dim=1).values
        near = ((top[:, 0] - top[:, 1]) <= 1e-2 * logits.abs().max(1).values).sum()
        dc = ((iv[1] - i0[1]) - (ie[1] - i0[1])).abs()
        self._check("correct", "beyond_near_ties", (dc - near).clamp_min(0), 0)
        if train:
            for k in outs:
                if A[k] is not None:
                    self._close(k, A[k], E[k])
        if zero is not None:
            self._check("zero", "nonzero", (zero != 0).sum(), 0)
        self._flush("head", sig)
        return ret

    def maxpool2(self, call, A):
        x, out = A["x"], A["out"]
        out0 = self._snap(out)
        ins = self._inputs(dict(x=x), (out,))
        y = call()
        self._exact("out", y, self._emul("maxpool2", self._R(ins["x"]), out=out0))
        self._flush("maxpool2", _sig(x=x))
        return y

    def maxpool2_bwd(self, call, A):
        x, dy, out = A["x"], A["dy"], A["out"]
        out0 = self._snap(out)
        ins = self._inputs(dict(x=x, dy=dy), (out,))
        dx = call()
        # first maximum of each window, the rule the kernel declares and torch's max_pool2d follows
        self._exact("dx", dx, self._emul("maxpool2_bwd", self._R(ins["x"]), self._R(ins["dy"]), out=out0))
        self._flush("maxpool2_bwd", _sig(x=x))
        return dx

    def maxpool3(self, call, A):
        x, out = A["x"], A["out"]
        out0 = self._snap(out)
        xin = self._snap(x)
        y, idx = call()
        self._pool_in[idx.data_ptr()] = xin
        self._exact("out", y, self._emul("maxpool3", xin, A["stride"], out=out0)[0])
        self._flush("maxpool3", _sig(x=x, stride=A["stride"]))
        return y, idx

    def maxpool3_bwd(self, call, A):
        dy, idx, out = A["dy"], A["idx"], A["out"]
        sig = _sig(dy=dy, x=tuple(A["x_shape"]), stride=A["stride"], opt=_present(A, ("accumulate",)))
        xin = self._pool_in.get(idx.data_ptr())
        out0 = self._snap(out)
        ins = self._inputs(dict(dy=dy), (out,))
        dx = call()
        if xin is None:
            self._check("idx", "unknown_forward", torch.ones(()), 0)
        else:
            # up to nine bf16 grads (and the accumulate destination) are summed per element: the bf16 rule,
            # against torch's first-maximum routing
            self._close("dx", dx, self._emul("maxpool3_bwd", self._R(ins["dy"]), xin, tuple(A["x_shape"]),
                                             A["stride"], out=out0, accumulate=A["accumulate"]))
        self._flush("maxpool3_bwd", sig)
        return dx

    # ---- wrapping ------------------------------------------------------------------------------------
    def wrap(self, name: str, fn):
        sg = inspect.signature(fn)
        handler = getattr(self, name)

        @functools.wraps(fn)
        def wrapper(*args, **kw):
            bound = sg.bind(*args, **kw)
            bound.apply_defaults()
            grad = torch.is_grad_enabled()

            def call():      # the bound function as the engine would have called it
                with torch.set_grad_enabled(grad):
                    return fn(*args, **kw)

            with torch.no_grad():
                return handler(call, dict(bound.arguments))

        return wrapper


@contextlib.contextmanager
def shadow(collect: bool = False, ref_device=None):
    """Shadow every kernel entry point bound in fedmi.ops.conv / fedmi.ops.cnn with its emulation.

    A mismatch raises :class:`ShadowMismatch` naming the op, the signature, the tensor and the error;
    ``collect=True`` gathers them in ``.failures`` instead.  ``ref_device``: where the emulation runs
    (default: where the op's tensors live)."""
    S = Shadow(collect, ref_device)
    S._native = conv.pack_weight is not emulate.pack_weight
    saved = []
    for mod, names in ((conv, CONV_OPS), (cnn, CNN_OPS)):
        for name in names:
            fn = getattr(mod, name)
            saved.append((mod, name, fn))
            setattr(mod, name, S.wrap(name, fn))
    try:
        yield S
        if S._pending:
            S._fail(f"{len(S._pending)} deferred WGRADs were never reduced (first: {S._pending[0][0]} "
                    f"[{S._pending[0][1]}])")
    finally:
        for mod, name, fn in reversed(saved):
            setattr(mod, name, fn)


# ---- results table ---------------------------------------------------------------------------------
def report_markdown(cases: list) -> str:
    """Markdown table of dumped cases (dicts: arch, nb, seconds, table = Shadow.dump())."""
    lines = ["| arch | nb | seconds | op | signatures | calls | worst error per metric |", "|---|---|---|---|---|---|---|"]
    for c in sorted(cases, key=lambda c: (c["arch"], c["nb"])):
        per_op: dict = {}
        for op, sig, count, worst in c["table"]:
            e = per_op.setdefault(op, {"sigs": 0, "calls": 0, "worst": {}})
            e["sigs"] += 1
            e["calls"] += count
            for k, v in worst.items():
                m = k.split(":")[-1]
                e["worst"][m] = _worse(e["worst"].get(m), v)
        for op in ALL_OPS:
            if op in per_op:
                e = per_op[op]
                w = ", ".join(f"{m} {v:.2e}" for m, v in sorted(e["worst"].items()))
                lines.append(f"| {c['arch']} | {c['nb']} | {c['seconds']:.1f} | {op} | {e['sigs']} | {e['calls']} "
                             f"| {w} |")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":     # python tests/shadow.py DIR: the table of the case files a GPU run dumped there
    print(report_markdown([json.loads(p.read_text()) for p in sorted(Path(sys.argv[1]).glob("*.json"))]), end="")
