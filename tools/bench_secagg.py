#!/usr/bin/env python
"""Time the secure-aggregation kernels (csrc/kernels/secagg.hip) next to sgd_flat at the same sizes.

    python tools/bench_secagg.py [--sizes 62006 11173962] [--worlds 2 4 8 16] [--iters 100] [--reps 3]

One JSON line per (size, W, kernel): microseconds per call (HIP-graph replay of `iters` calls, device events; the
variants alternate `reps` times in one run and the median is kept), the bytes moved per entry, the resulting GB/s and
the time as a multiple of sgd_flat's in the same run.  `secagg_mask` is the mask kernel and its count fold (12 B per
entry, W - 1 ChaCha20 words per entry: issue-bound), `secagg_unmask` the decode of the W gathered rows ((W + 2) * 4 B
per entry).  The middle rank masks: half its streams are added, half subtracted.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402
from bench_robust import LENET, RESNET18, _time  # noqa: E402

from fedmi import native  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[LENET, RESNET18])
    ap.add_argument("--worlds", nargs="+", type=int, default=[2, 4, 8, 16])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    nat = native.require()
    dev = torch.device("cuda:0")

    def S():
        return native.stream_handle(dev)

    for n in a.sizes:
        ld = (n + 3) & ~3
        p, g, m = (torch.randn(n, device=dev) for _ in range(3))
        x = p + 0.1 * g
        u = torch.zeros(n, dtype=torch.int32, device=dev)
        rows = torch.randint(-2 ** 31, 2 ** 31, (max(a.worlds), ld), dtype=torch.int32, device=dev)
        keys = torch.randint(-2 ** 31, 2 ** 31, (16, 8), dtype=torch.int32, device=dev)
        out = torch.empty(n, device=dev)
        part = torch.zeros((nat.secagg_partials(n), 16), dtype=torch.int64, device=dev)
        stats = torch.zeros(1, dtype=torch.int64, device=dev)
        runs = [("sgd_flat", 0, 20, lambda: nat.sgd_flat(S(), p.data_ptr(), g.data_ptr(), m.data_ptr(), n, 0.0, 0.9,
                                                         0.0, 0.0, False, False))]
        for W in a.worlds:
            runs += [
                ("secagg_mask", W, 12,
                 lambda W=W: nat.secagg_mask(S(), x.data_ptr(), p.data_ptr(), keys.data_ptr(), W, W // 2, 7, n, 24,
                                             u.data_ptr(), part.data_ptr(), stats.data_ptr())),
                ("secagg_unmask", W, 4 * (W + 2),
                 lambda W=W: nat.secagg_unmask(S(), rows.data_ptr(), ld, W, g.data_ptr(), n, 24, out.data_ptr()))]
        us = {i: [] for i in range(len(runs))}
        for _ in range(a.reps):                                  # the variants alternate in one run
            for i, run in enumerate(runs):
                us[i].append(_time(run[3], a.iters))
        flat = statistics.median(us[0])
        for i, (name, W, bpe, _) in enumerate(runs):
            t = statistics.median(us[i])
            print(json.dumps({"kernel": name, "n": n, "W": W, "us": round(t, 2), "min": round(min(us[i]), 2),
                              "max": round(max(us[i]), 2), "bytes_per_entry": bpe,
                              "GBps": round(n * bpe / t / 1e3, 1), "x_sgd_flat": round(t / flat, 2),
                              "keystream_Gwords_per_s": round(n * (W - 1) / t / 1e3, 1) if name == "secagg_mask" else None,
                              "iters": a.iters, "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
