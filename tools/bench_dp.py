"""Time the DP-FedAvg launches (csrc/kernels/dp.hip) against sgd_flat at the same length.

    python tools/bench_dp.py [--sizes 62006 11173962] [--iters 200] [--cold]
    python tools/bench_dp.py --epoch [--models lenet resnet18] [--batches 391] [--rounds 5]

Prints one JSON line per (size, kernel): microseconds per launch (HIP-graph replay of `iters` launches), the bytes
it moves per entry and the resulting GB/s, so the launches can be compared per byte with a streaming kernel:
sgd_flat 20, dp_sumsq 8, dp_finish 0 (it reads at most 2048 partials), the apply 12 when it clips and adds noise
(x and anchor in, x out), 8 for noise alone (scale == 1: the anchor is not read), 12 for the clip alone, and `round` =
the three launches of one round (20).  An apply that stays far below sgd_flat's GB/s is bound by the Philox rounds and
the transcendentals, not by memory.  --cold: every launch follows a 1 GiB streaming pass that evicts the 256 MB
last-level cache (after a local epoch the model state is cold); the pass alone is timed and subtracted.

Epoch mode prints one JSON line per (model, setting): milliseconds per round (a local epoch of `batches` batches of
128 on the native engine, graph replay, FedAvg.average() at world 1 and the evaluation of 10,000 test images) with the
DP flags off, with the clip alone and with clip and noise; median of `rounds` timed rounds after 2 untimed ones.
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

LENET, RESNET18 = 62006, 11173962      # float_state() entries (ResNet-18: parameters only)
SUMSQ, FINISH, APPLY = 1, 2, 4


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


def epoch(a) -> None:
    from fedmi.engine import build_trainer
    from fedmi.engine.base import TrainerConfig
    from fedmi.engine.data import contiguous_schedule, make_dataset
    from fedmi.parallel.dp import make_dp
    from fedmi.parallel.fedavg import FedAvg

    dev = torch.device("cuda:0")
    n_train = 128 * a.batches
    data = make_dataset("synthetic-cifar10", device=dev, n_train=n_train, n_test=10000, seed=0)
    for model in a.models:
        for clip, z in ((0.0, 0.0), (0.5, 0.0), (0.5, 0.01)):     # the work does not depend on z; a small one keeps the state finite
            tr = build_trainer(model, data, dev, TrainerConfig(seed=1, lr=0.02))
            tr.set_schedule(*contiguous_schedule(n_train, 128))
            dp = make_dp(clip, tr, z, seed=1, who="bench")
            fa = FedAvg(dp=dp)
            ms = []
            for r in range(a.rounds + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.train_epoch()
                fa.average(tr)
                tr.evaluate()
                torch.cuda.synchronize()
                if r >= 2:
                    ms.append((time.perf_counter() - t0) * 1e3)
            med = statistics.median(ms)
            rec = {"model": model, "dp_clip": clip, "dp_noise": z, "batches": a.batches, "ms_per_round": round(med, 3),
                   "rounds_per_s": round(1e3 / med, 3), "min": round(min(ms), 3), "max": round(max(ms), 3),
                   "rounds": a.rounds, "finite": bool(torch.isfinite(tr.float_state()).all())}
            if dp is not None:
                rec.update(dp.round_stats())
            print(json.dumps(rec), flush=True)


def kernels(a) -> None:
    nat = native.require()
    dev = torch.device("cuda:0")
    flush = torch.zeros(1 << 28, device=dev) if a.cold else None   # 1 GiB
    t_flush = _time(lambda: flush.add_(1.0), a.iters) if a.cold else 0.0
    for n in a.sizes:
        anchor, g, m = (torch.randn(n, device=dev) for _ in range(3))
        x = anchor + 1e-2 * torch.randn(n, device=dev)
        x0 = x.clone()
        partial = torch.zeros(max(1, nat.dp_partials(n)), dtype=torch.float64, device=dev)
        stats = torch.zeros(4, dtype=torch.float64, device=dev)
        norm = float((x - anchor).double().norm())

        def S():
            return native.stream_handle(dev)

        def dp(stages, clip, z):
            # the apply reads the scale the last dp_finish left in the stats row
            return lambda: nat.dp_privatize(S(), x.data_ptr(), anchor.data_ptr(), n, n, partial.data_ptr(),
                                            stats.data_ptr(), clip, z, 1, 0x1234567887654321, 7, stages)

        lo, hi = 0.5 * norm, 4.0 * norm      # a clip that bites and one out of reach
        runs = [("sgd_flat", 20, None, lambda: nat.sgd_flat(S(), x.data_ptr(), g.data_ptr(), m.data_ptr(), n, 0.0, 0.9,
                                                            0.0, 0.0, False, False)),
                ("dp_sumsq", 8, None, dp(SUMSQ, lo, 0.0)),
                ("dp_finish", 0, None, dp(FINISH, lo, 0.0)),
                ("apply_clip", 12, (lo, 0.0), dp(APPLY, lo, 0.0)),
                ("apply_unclipped", 0, (hi, 0.0), dp(APPLY, hi, 0.0)),
                ("apply_noise", 8, (hi, 1e-3), dp(APPLY, hi, 1e-3)),
                ("apply_clip_noise", 12, (lo, 1e-3), dp(APPLY, lo, 1e-3)),
                # z = 0.01 lengthens the update by more than the clip shortens it, so every replay clips again (a
                # clip-only round would find norm == S from its second replay on and store nothing)
                ("round_clip_noise", 20, (lo, 1e-2), dp(SUMSQ | FINISH | APPLY, lo, 1e-2))]
        for name, bpe, prime, fn in runs:
            m.normal_()                         # decays by 0.9 per launch: restart it well above the denormals
            x.copy_(x0)
            if prime is not None:               # the stats row the timed apply reads: this case's scale
                dp(SUMSQ | FINISH, prime[0], 0.0)()
            step = (lambda fn=fn: (flush.add_(1.0), fn())) if a.cold else fn
            us = _time(step, a.iters) - t_flush
            rec = {"kernel": name, "n": n, "us": round(us, 2), "bytes_per_entry": bpe, "cold": a.cold,
                   "flush_us": round(t_flush, 2)}
            if bpe:
                rec.update(ns_per_KiB=round(us * 1e3 / (n * bpe / 1024), 3), GBps=round(n * bpe / us / 1e3, 1))
            print(json.dumps(rec), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[LENET, RESNET18])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--cold", action="store_true")
    ap.add_argument("--epoch", action="store_true", help="time whole rounds with the DP flags off and on instead")
    ap.add_argument("--models", nargs="+", default=["lenet", "resnet18"])
    ap.add_argument("--batches", type=int, default=391)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    epoch(a) if a.epoch else kernels(a)


if __name__ == "__main__":
    main()
