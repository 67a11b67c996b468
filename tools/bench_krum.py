#!/usr/bin/env python
"""Time the Krum kernels (csrc/kernels/krum.hip) next to geomed_pass, geomed and sgd_flat at the same sizes.

    python tools/bench_krum.py [--sizes 62006 11173962] [--worlds 2 4 8 16] [--iters 100] [--reps 3] [--T 8]

One JSON line per (size, W, kernel): microseconds per call (HIP-graph replay of `iters` calls, device events; the
variants alternate `reps` times in one run and the median is kept), the bytes moved per entry, the resulting GB/s and
the time as a multiple of what sgd_flat (20 B per entry) takes per byte in the same run.  `krum_gram` is the Gram pass
and its fold (W * 4 B per entry), `krum` / `multikrum` the whole aggregation (the Gram, the finish and the mean of the m
selected rows: (W + m + 1) * 4 B per entry), `geomed_pass` one weighted pass and its finish -- the yardstick: it moves
the same row bytes -- and `geomed` the whole T-pass aggregation.  `x_geomed_pass` is the time as a multiple of
geomed_pass at the same size and W in the same run.
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
from fedmi.parallel.krum import krum_counts  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[LENET, RESNET18])
    ap.add_argument("--worlds", nargs="+", type=int, default=[2, 4, 8, 16])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--T", type=int, default=8)
    a = ap.parse_args()
    nat = native.require()
    dev = torch.device("cuda:0")

    def S():
        return native.stream_handle(dev)

    for n in a.sizes:
        ld = (n + 3) & ~3
        p, g, m = (torch.randn(n, device=dev) for _ in range(3))
        rows = torch.randn((max(a.worlds), ld), device=dev)
        out = torch.empty(n, device=dev)
        part = torch.zeros((nat.geomed_partials(n), 16), dtype=torch.float64, device=dev)
        tiles = torch.zeros((nat.krum_partials(n), 256), dtype=torch.float64, device=dev)
        gram = torch.zeros((16, 16), dtype=torch.float64, device=dev)
        stats = torch.zeros((18, 16), dtype=torch.float64, device=dev)
        hist = torch.zeros((a.T + 1, 3, 16), dtype=torch.float64, device=dev)
        runs = [("sgd_flat", 0, 20, lambda: nat.sgd_flat(S(), p.data_ptr(), g.data_ptr(), m.data_ptr(), n, 0.0, 0.9,
                                                         0.0, 0.0, False, False))]
        for W in a.worlds:
            w = torch.full((W,), 1.0 / W, device=dev)
            kept = krum_counts(W, 1, True)[2]
            runs += [
                ("krum_gram", W, 4 * W,
                 lambda W=W: nat.krum_gram(S(), rows.data_ptr(), ld, W, n, tiles.data_ptr(), gram.data_ptr())),
                ("krum", W, 4 * (W + 2),
                 lambda W=W: nat.krum(S(), rows.data_ptr(), ld, W, n, 1, False, out.data_ptr(), tiles.data_ptr(),
                                      stats.data_ptr())),
                ("multikrum", W, 4 * (W + kept + 1),
                 lambda W=W: nat.krum(S(), rows.data_ptr(), ld, W, n, 1, True, out.data_ptr(), tiles.data_ptr(),
                                      stats.data_ptr())),
                ("geomed_pass", W, 4 * (W + 1),
                 lambda W=W, w=w: nat.geomed_pass(S(), rows.data_ptr(), ld, W, n, False, w.data_ptr(), out.data_ptr(),
                                                  part.data_ptr(), hist.data_ptr())),
                ("geomed", W, 4 * (W + 1) * (a.T + 1),
                 lambda W=W: nat.geomed(S(), rows.data_ptr(), ld, W, n, a.T, 1e-6, out.data_ptr(), part.data_ptr(),
                                        hist.data_ptr()))]
        us = {i: [] for i in range(len(runs))}
        for _ in range(a.reps):                                  # the variants alternate in one run
            for i, run in enumerate(runs):
                us[i].append(_time(run[3], a.iters))
        flat = statistics.median(us[0]) / (n * 20)               # us per byte of a streaming kernel, this run
        yard = {W: statistics.median(us[i]) for i, (name, W, _, _) in enumerate(runs) if name == "geomed_pass"}
        for i, (name, W, bpe, _) in enumerate(runs):
            t = statistics.median(us[i])
            print(json.dumps({"kernel": name, "n": n, "W": W, "T": a.T if name == "geomed" else None,
                              "us": round(t, 2), "min": round(min(us[i]), 2), "max": round(max(us[i]), 2),
                              "bytes_per_entry": bpe, "GBps": round(n * bpe / t / 1e3, 1),
                              "x_sgd_flat_per_byte": round(t / (n * bpe) / flat, 2),
                              "x_geomed_pass": round(t / yard[W], 2) if W else None, "iters": a.iters,
                              "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
