#!/usr/bin/env python
"""Time the DnC kernels (csrc/kernels/dnc.hip) next to Krum's at the same sizes: both Gram sweeps read the same bytes.

    python tools/bench_dnc.py [--sizes 11173962] [--worlds 8 16] [--iters 100] [--reps 3]

One JSON line per (size, W, kernel): microseconds per call (HIP-graph replay of `iters` calls, device events; the
variants alternate `reps` times in one run and the median is kept), the bytes moved per entry, the resulting GB/s and
the time as a multiple of what sgd_flat (20 B per entry) takes per byte in the same run.  `dnc_gram` is the centred
Gram pass and its fold, `krum_gram` the uncentred one (W * 4 B per entry each); `dnc` and `multikrum` (F = 1) are the
whole aggregations (the Gram, the finish and the mean of the m kept rows: (W + m + 1) * 4 B per entry).  `x_krum` is the
time as a multiple of the Krum counterpart (dnc_gram / krum_gram, dnc / multikrum) at the same size and W in the same
run.
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
from fedmi.parallel.dnc import dnc_counts  # noqa: E402
from fedmi.parallel.krum import krum_counts  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[RESNET18])
    ap.add_argument("--worlds", nargs="+", type=int, default=[8, 16])
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
        # a federation's rows: a common part and small differences (the timings do not depend on the values)
        rows = torch.randn(ld, device=dev) + 1e-3 * torch.randn((max(a.worlds), ld), device=dev)
        out = torch.empty(n, device=dev)
        tiles = torch.zeros((max(nat.krum_partials(n), nat.dnc_partials(n)), 256), dtype=torch.float64, device=dev)
        gram = torch.zeros((16, 16), dtype=torch.float64, device=dev)
        stats = torch.zeros((18, 16), dtype=torch.float64, device=dev)
        runs = [("sgd_flat", 0, 20, None, lambda: nat.sgd_flat(S(), p.data_ptr(), g.data_ptr(), m.data_ptr(), n, 0.0,
                                                               0.9, 0.0, 0.0, False, False))]
        for W in a.worlds:
            runs += [
                ("krum_gram", W, 4 * W, None,
                 lambda W=W: nat.krum_gram(S(), rows.data_ptr(), ld, W, n, tiles.data_ptr(), gram.data_ptr())),
                ("dnc_gram", W, 4 * W, "krum_gram",
                 lambda W=W: nat.dnc_gram(S(), rows.data_ptr(), ld, W, n, tiles.data_ptr(), gram.data_ptr())),
                ("multikrum", W, 4 * (W + krum_counts(W, 1, True)[2] + 1), None,
                 lambda W=W: nat.krum(S(), rows.data_ptr(), ld, W, n, 1, True, out.data_ptr(), tiles.data_ptr(),
                                      stats.data_ptr())),
                ("dnc", W, 4 * (W + dnc_counts(W, 1)[1] + 1), "multikrum",
                 lambda W=W: nat.dnc(S(), rows.data_ptr(), ld, W, n, 1, out.data_ptr(), tiles.data_ptr(),
                                     stats.data_ptr()))]
        us = {i: [] for i in range(len(runs))}
        for _ in range(a.reps):                                  # the variants alternate in one run
            for i, run in enumerate(runs):
                us[i].append(_time(run[4], a.iters))
        flat = statistics.median(us[0]) / (n * 20)               # us per byte of a streaming kernel, this run
        med = {(name, W): statistics.median(us[i]) for i, (name, W, _, _, _) in enumerate(runs)}
        for i, (name, W, bpe, yard, _) in enumerate(runs):
            t = med[(name, W)]
            print(json.dumps({"kernel": name, "n": n, "W": W, "us": round(t, 2), "min": round(min(us[i]), 2),
                              "max": round(max(us[i]), 2), "bytes_per_entry": bpe,
                              "GBps": round(n * bpe / t / 1e3, 1), "x_sgd_flat_per_byte": round(t / (n * bpe) / flat, 2),
                              "x_krum": round(t / med[(yard, W)], 2) if yard else None, "iters": a.iters,
                              "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
