#!/usr/bin/env python
"""-c Y kernel timings (csrc/kernels/compress.hip) at the LeNet and ResNet-18 state sizes.

For n = 62,006 (LeNet) and 11,173,962 (ResNet-18): device time of the
error-feedback delta + exact top-k (k = 1 % and 20 % of n, FEDMI_TOPK_RATIOS: the fused path ``topk_us``, and one
read+write pass over the state for scale ``rw_pass_us``), of the rank-ordered
scatter of 4 ranks' payloads, of int8 quantisation and of a 4-rank dequant
accumulate; plus payload bytes vs dense fp32.  One JSON line per size.

The powersgd arm (csrc/kernels/powersgd.hip) runs on the real layouts of LeNet, ResNet-18 and MobileNet at the ranks of
FEDMI_PSGD_RANKS (default 2,4): device time of each of the round's four launches and of the round without its two
collectives, the bytes each moves (16 / 4 / 20 B per entry) over that time beside ``sgd_flat`` on the same state
(20 B per entry), and the payload per round and client.  One JSON line per model and rank.
"""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _time(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


class _Layout:
    """A trainer's float state with the model's state dict laid over it (what PowerSGDCompressor reads)."""

    def __init__(self, model: str, dev):
        from fedmi.models import build_model

        shapes = [(k, tuple(v.shape)) for k, v in build_model(model).state_dict().items() if v.is_floating_point()]
        sizes = [int(torch.Size(s).numel()) for _, s in shapes]
        self.flat = torch.randn(sum(sizes), device=dev)
        self.views, off = {}, 0
        for (k, s), m in zip(shapes, sizes):
            self.views[k] = self.flat[off:off + m].view(s)
            off += m

    def float_state(self):
        return self.flat

    def state_dict(self):
        return self.views


def powersgd_arm(nat, dev, S, out) -> None:
    from fedmi.parallel.compress import PowerSGDCompressor

    ranks = [int(v) for v in os.environ.get("FEDMI_PSGD_RANKS", "2,4").split(",")]
    for model in os.environ.get("FEDMI_PSGD_MODELS", "lenet,resnet18,mobilenet").split(","):
        tr = _Layout(model, dev)
        n = tr.flat.numel()
        iters = 200 if n < 1e6 else 20
        grad, mom = torch.randn(n, device=dev) * 0.01, torch.zeros(n, device=dev)
        t_sgd = _time(lambda: nat.sgd_flat(S(), tr.flat.data_ptr(), grad.data_ptr(), mom.data_ptr(), n, 0.01, 0.9, 5e-4,
                                           0.0, False, False), iters)
        for R in ranks:
            c = PowerSGDCompressor(tr, rank=R)
            x = tr.flat
            x.copy_(c.global_ref).add_(grad)
            t, k = c._tb, c._cnt
            n_comp = sum(r * cl for _, r, cl in c.segments)
            launches = {
                "project": lambda: c.phase1(x),
                "orth": lambda: nat.psgd_orth(S(), t["segs"].data_ptr(), k["segs"], c.send.data_ptr(), R),
                "backproject": lambda: nat.psgd_backproject(
                    S(), c.residual.data_ptr(), t["segs"].data_ptr(), t["backproject"].data_ptr(), k["backproject"],
                    c.send.data_ptr(), R, c.q.data_ptr(), c.qpart.data_ptr(), t["qfolds"].data_ptr(), k["qfolds"]),
                "apply": lambda: c.phase3(x, c.q),
            }
            c.phase2(c.phase1(x))                       # every timed launch starts from a finite, typical state
            us = {name: _time(fn, iters) for name, fn in launches.items()}
            c.residual.zero_()
            t_round = _time(lambda: c.phase3(x, c.phase2(c.phase1(x))), iters)
            moved = {"project": 16 * n_comp + 12 * c.n_dense, "backproject": 4 * n_comp, "apply": 20 * n}
            rec = {"bench": "powersgd_kernels", "payload": model, "n": n, "rank": R, "segments": len(c.segments),
                   "n_compressed": n_comp, "n_dense": c.n_dense, "tiles_project": k["project"],
                   "tiles_backproject": k["backproject"], "folds": [k["pfolds"], k["qfolds"]],
                   **{f"{name}_us": round(v, 2) for name, v in us.items()}, "round_us": round(t_round, 2),
                   **{f"{name}_GBps": round(moved[name] / us[name] / 1e3, 1) for name in moved},
                   "sgd_flat_us": round(t_sgd, 2), "sgd_flat_GBps": round(20 * n / t_sgd / 1e3, 1),
                   "bytes_dense": 4 * n, "bytes_powersgd": c.payload_bytes,
                   "ratio_powersgd": round(4 * n / c.payload_bytes, 1)}
            print(json.dumps(rec), flush=True)
            out.append(rec)


def main() -> int:
    from fedmi import native

    nat = native.require()
    dev = torch.device("cuda", 0)
    S = lambda: native.stream_handle(dev)   # noqa: E731
    out = []
    ratios = [float(v) for v in os.environ.get("FEDMI_TOPK_RATIOS", "0.01,0.2").split(",")]
    for (name, n), ratio in [(p, r) for p in (("lenet", 62006), ("resnet18", 11173962)) for r in ratios]:
        iters = 200 if n < 1e6 else 20
        k = max(1, int(round(n * ratio)))
        R = 4
        local = torch.randn(n, device=dev)
        glob = torch.randn(n, device=dev)
        resid = torch.zeros(n, device=dev)
        d = torch.empty(n, device=dev)
        idx = torch.empty(k, dtype=torch.int32, device=dev)
        val = torch.empty(k, device=dev)
        tstate = torch.zeros(nat.topk_state_bytes(), dtype=torch.uint8, device=dev)
        cidx = torch.empty(2 * n, dtype=torch.int32, device=dev)
        ckey = torch.empty(2 * n, dtype=torch.int32, device=dev)

        def topk_ef():
            nat.topk_ef(S(), local.data_ptr(), glob.data_ptr(), resid.data_ptr(), n, k, tstate.data_ptr(),
                        cidx.data_ptr(), ckey.data_ptr(), idx.data_ptr(), val.data_ptr())

        t_topk = _time(topk_ef, iters)
        # realistic rounds: a fresh update every call (the residual carries the unsent part forward)
        ups = [torch.randn(n, device=dev) * 0.01 for _ in range(4)]
        calls = [0]

        def topk_ef_fresh():
            local.copy_(glob).add_(ups[calls[0] % 4])
            calls[0] += 1
            topk_ef()

        resid.zero_()
        t_topk_fresh = _time(topk_ef_fresh, iters) - _time(lambda: local.copy_(glob).add_(ups[0]), iters)
        st_words = tstate.view(torch.int32).cpu()
        cand = int(st_words[2048 + 4])
        dense = torch.randn(n, device=dev)
        t_copy = _time(lambda: dense.mul_(1.0), iters)     # one read + write pass over the state
        idx_all = torch.stack([torch.randperm(n, device=dev)[:k].to(torch.int32) for _ in range(R)])
        val_all = torch.randn(R, k, device=dev)
        acc = torch.zeros(n, device=dev)
        t_scatter = _time(lambda: nat.scatter_add_ranked(S(), acc.data_ptr(), idx_all.data_ptr(), val_all.data_ptr(),
                                                          R, k, 1.0 / R, n), iters)
        nch = (n + 255) // 256
        q = torch.empty(n, dtype=torch.int8, device=dev)
        sc = torch.empty(nch, device=dev)
        t_q = _time(lambda: nat.quant_int8(S(), d.data_ptr(), n, q.data_ptr(), sc.data_ptr(), resid.data_ptr()), iters)
        q_all = q.repeat(R)
        s_all = sc.repeat(R)
        t_dq = _time(lambda: nat.dequant_accum(S(), q_all.data_ptr(), s_all.data_ptr(), R, n, acc.data_ptr(), 1.0 / R),
                     iters)
        rec = {"bench": "compress_kernels", "payload": name, "n": n, "k": k, "ratio": ratio,
               "topk_us": round(t_topk, 2), "topk_fresh_update_us": round(t_topk_fresh, 2), "candidates_last": cand,
               "rw_pass_us": round(t_copy, 2), "scatter_ranked_4rank_us": round(t_scatter, 2),
               "quant_int8_us": round(t_q, 2), "dequant_accum_4rank_us": round(t_dq, 2),
               "bytes_dense": 4 * n, "bytes_topk": 8 * k, "bytes_int8": n + 4 * nch,
               "ratio_topk": round(4 * n / (8 * k), 2), "ratio_int8": round(4 * n / (n + 4 * nch), 2)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    powersgd_arm(nat, dev, S, out)
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text("".join(json.dumps(r) + "\n" for r in out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
