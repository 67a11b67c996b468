"""Time the client-optimizer step kernels (csrc/kernels/client_opt.hip) against sgd_flat at the same length,
and a ResNet-18 local epoch with each kind on.

    python tools/bench_client_opt.py [--sizes 62006 11173962] [--iters 200] [--cold]
    python tools/bench_client_opt.py --epoch [--batches 391] [--rounds 5]

Kernel mode prints one JSON line per (size, kernel): microseconds per launch (HIP-graph replay of `iters`
launches), the bytes it moves per entry (sgd_flat 20: reads p, g, buf and writes p, buf; fedprox 16: reads g, p,
anchor and writes g; scaffold 20: reads g, corr, acc and writes g, acc) and the time relative to sgd_flat.
--cold: every launch follows a 1 GiB streaming pass that evicts the 256 MB last-level cache; the pass alone is
timed and subtracted.

Epoch mode prints one JSON line per kind (none, fedprox, scaffold): milliseconds per local epoch of `batches`
batches of 128 on the native ResNet-18 engine (graph replay), FedAvg.average() at world 1 included, median of
`rounds` timed rounds after 2 untimed ones.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from fedmi import native  # noqa: E402

LENET, RESNET18 = 62006, 11173962      # n_params() (ResNet-18: parameters only)


def _time(fn, iters: int) -> float:
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def kernels(a) -> None:
    nat = native.require()
    dev = torch.device("cuda:0")
    flush = torch.zeros(1 << 28, device=dev) if a.cold else None   # 1 GiB
    t_flush = _time(lambda: flush.add_(1.0), a.iters) if a.cold else 0.0
    for n in a.sizes:
        # lr 0, mu 0 and corr 0 keep the values fixed over hundreds of replays; the traffic is the same
        p, anchor, g, mom = (torch.randn(n, device=dev) for _ in range(4))
        corr, acc = torch.zeros(n, device=dev), torch.zeros(n, device=dev)

        def S():
            return native.stream_handle(dev)

        runs = [("sgd_flat", 20, lambda: nat.sgd_flat(S(), p.data_ptr(), g.data_ptr(), mom.data_ptr(), n, 0.0, 0.9,
                                                      0.0, 0.0, False, False)),
                ("drift_grad<fedprox>", 16, lambda: nat.drift_grad(S(), 0, g.data_ptr(), p.data_ptr(), anchor.data_ptr(),
                                                                   0, 0, 0.0, n)),
                ("drift_grad<scaffold>", 20, lambda: nat.drift_grad(S(), 1, g.data_ptr(), 0, 0, corr.data_ptr(),
                                                                    acc.data_ptr(), 0.0, n))]
        base = None
        for name, bpe, fn in runs:
            mom.normal_()                       # decays by 0.9 per launch: restart it well above the denormals
            g.normal_()
            acc.zero_()
            step = (lambda fn=fn: (flush.add_(1.0), fn())) if a.cold else fn
            us = _time(step, a.iters) - t_flush
            base = us if base is None else base
            print(json.dumps({"kernel": name, "n": n, "us": round(us, 2), "vs_sgd_flat": round(us / base, 3),
                              "bytes_per_entry": bpe, "ns_per_KiB": round(us * 1e3 / (n * bpe / 1024), 3),
                              "GBps": round(n * bpe / us / 1e3, 1), "cold": a.cold, "flush_us": round(t_flush, 2)}),
                  flush=True)


def epoch(a) -> None:
    from fedmi.engine import build_trainer
    from fedmi.engine.base import TrainerConfig
    from fedmi.engine.data import contiguous_schedule, make_dataset
    from fedmi.parallel.client_opt import make_client_opt
    from fedmi.parallel.fedavg import FedAvg

    dev = torch.device("cuda:0")
    n_train = 128 * a.batches
    data = make_dataset("synthetic-cifar10", device=dev, n_train=n_train, n_test=128, seed=0)
    for kind in ("none", "fedprox", "scaffold"):
        tr = build_trainer("resnet18", data, dev, TrainerConfig(seed=1, lr=0.02))
        tr.set_schedule(*contiguous_schedule(n_train, 128))
        fa = FedAvg(client_opt=make_client_opt(kind, tr, 0.01))
        ms = []
        for r in range(a.rounds + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train_epoch()
            fa.average(tr)
            torch.cuda.synchronize()
            if r >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"model": "resnet18", "client_opt": kind, "batches": a.batches,
                          "ms_per_round": round(statistics.median(ms), 2), "min": round(min(ms), 2),
                          "max": round(max(ms), 2), "rounds": a.rounds,
                          "finite": bool(torch.isfinite(tr.float_state()).all())}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[LENET, RESNET18])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--cold", action="store_true")
    ap.add_argument("--epoch", action="store_true", help="time a ResNet-18 local epoch with each kind instead")
    ap.add_argument("--batches", type=int, default=391)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    epoch(a) if a.epoch else kernels(a)


if __name__ == "__main__":
    main()
