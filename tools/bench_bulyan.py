#!/usr/bin/env python
"""Time the Bulyan kernels (csrc/kernels/bulyan.hip) next to robust_reduce, krum, multikrum and geomed.

    python tools/bench_bulyan.py [--sizes 11173962] [--worlds 8 16] [--byz 1 3] [--iters 50] [--reps 3] [--T 8]

One JSON line per (size, W, kernel): microseconds per call (HIP-graph replay of `iters` calls, device events; the
variants alternate `reps` times in one run and the median is kept), the bytes moved per entry and the resulting GB/s.
`krum_gram` is launch 1 (with Krum's own fold of the tiles), `bulyan_fold` launches 3 and 4 over the first theta rows
(plus the one-thread record write of the test entry), `bulyan` all four; `robust_reduce` is the coordinate-wise trimmed
mean over theta rows with b = F_eff -- the fold's yardstick: the same rows, the same sort, no window choice.
`x_robust_reduce` is the time as a multiple of it in the same run.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402
from bench_robust import RESNET18, _time  # noqa: E402

from fedmi import native  # noqa: E402
from fedmi.parallel.bulyan import bulyan_counts  # noqa: E402
from fedmi.parallel.krum import krum_counts  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[RESNET18])
    ap.add_argument("--worlds", nargs="+", type=int, default=[8, 16])
    ap.add_argument("--byz", nargs="+", type=int, default=[1, 3], help="F per world")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--T", type=int, default=8)
    a = ap.parse_args()
    nat = native.require()
    dev = torch.device("cuda:0")

    def S():
        return native.stream_handle(dev)

    for n in a.sizes:
        ld = (n + 3) & ~3
        rows = torch.randn((max(a.worlds), ld), device=dev)
        out = torch.empty(n, device=dev)
        tiles = torch.zeros((nat.bulyan_partials(n), 256), dtype=torch.float64, device=dev)
        part = torch.zeros((max(nat.geomed_partials(n), nat.robust_partials(n)), 16), dtype=torch.float64, device=dev)
        gram = torch.zeros((16, 16), dtype=torch.float64, device=dev)
        stats = torch.zeros((19, 16), dtype=torch.float64, device=dev)
        cut = torch.zeros(16, dtype=torch.int64, device=dev)
        hist = torch.zeros((a.T + 1, 3, 16), dtype=torch.float64, device=dev)
        R, O, TL, ST = rows.data_ptr(), out.data_ptr(), tiles.data_ptr(), stats.data_ptr()
        runs = []
        for W, F in zip(a.worlds, a.byz):
            f, theta, c, _ = bulyan_counts(W, F)
            kept = krum_counts(W, F, True)[2]
            runs += [
                ("krum_gram", W, theta, 4 * W, lambda W=W: nat.krum_gram(S(), R, ld, W, n, TL, gram.data_ptr())),
                ("bulyan_fold", W, theta, 4 * (theta + 1),
                 lambda W=W, theta=theta, c=c: nat.bulyan_fold(S(), R, ld, W, n, list(range(theta)), c, O, TL, ST)),
                ("bulyan", W, theta, 4 * (W + theta + 1), lambda W=W, F=F: nat.bulyan(S(), R, ld, W, n, F, O, TL, ST)),
                ("robust_reduce", W, theta, 4 * (theta + 1),
                 lambda theta=theta, f=f: nat.robust_reduce(S(), R, ld, theta, n, f, O, part.data_ptr(), cut.data_ptr())),
                ("krum", W, theta, 4 * (W + 2), lambda W=W, F=F: nat.krum(S(), R, ld, W, n, F, False, O, TL, ST)),
                ("multikrum", W, theta, 4 * (W + kept + 1),
                 lambda W=W, F=F: nat.krum(S(), R, ld, W, n, F, True, O, TL, ST)),
                ("geomed", W, theta, 4 * (W + 1) * (a.T + 1),
                 lambda W=W: nat.geomed(S(), R, ld, W, n, a.T, 1e-6, O, part.data_ptr(), hist.data_ptr()))]
        us = {i: [] for i in range(len(runs))}
        for _ in range(a.reps):                                  # the variants alternate in one run
            for i, run in enumerate(runs):
                us[i].append(_time(run[4], a.iters))
        yard = {W: statistics.median(us[i]) for i, (name, W, *_) in enumerate(runs) if name == "robust_reduce"}
        for i, (name, W, theta, bpe, _) in enumerate(runs):
            t = statistics.median(us[i])
            print(json.dumps({"kernel": name, "n": n, "W": W, "theta": theta, "us": round(t, 2),
                              "min": round(min(us[i]), 2), "max": round(max(us[i]), 2), "bytes_per_entry": bpe,
                              "GBps": round(n * bpe / t / 1e3, 1), "x_robust_reduce": round(t / yard[W], 2),
                              "iters": a.iters, "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
