#!/usr/bin/env python
"""Time the robust-aggregation kernels (csrc/kernels/robust.hip, peer_robust_f32_kernel) against their dense
counterparts at the same sizes.

    python tools/bench_robust.py [--sizes 62006 11173962] [--worlds 2 4 8 16] [--iters 200] [--reps 3]
    python tools/bench_robust.py --peer [--worlds 2 4] [--iters 200]

Kernel mode prints one JSON line per (size, W, kind): microseconds per robust_reduce + robust_finish (HIP-graph
replay of `iters` launches, device events; the variants alternate `reps` times in one run and the median is kept),
the (W + 1) * 4 bytes it moves per entry, the resulting GB/s, and the time as a multiple of what sgd_flat (20 B per
entry) takes per byte in the same run.  A width far above 1x does not run at the streaming rate.

Peer mode spawns W ranks on the visible GPUs (all on cuda:0 on a one-GPU box, without the host gate, as
tools/bench_peer.py --no-gate) and prints, per (W, size), the fused robust all-reduce next to the dense one-shot
all-reduce: the difference is the price of the rule on the data plane.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from fedmi import native  # noqa: E402

LENET, RESNET18 = 62006, 11173962      # float_state() entries (ResNet-18: parameters only)


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

    def S():
        return native.stream_handle(dev)

    for n in a.sizes:
        ld = (n + 3) & ~3
        iters = a.iters
        p, g, m = (torch.randn(n, device=dev) for _ in range(3))
        rows = torch.randn((max(a.worlds), ld), device=dev)
        out = torch.empty(n, device=dev)
        partial = torch.zeros((nat.robust_partials(n), 16), dtype=torch.int64, device=dev)
        stats = torch.zeros(16, dtype=torch.int64, device=dev)
        runs = [("sgd_flat", 0, 0, 20, lambda: nat.sgd_flat(S(), p.data_ptr(), g.data_ptr(), m.data_ptr(), n, 0.0,
                                                            0.9, 0.0, 0.0, False, False))]
        for W in a.worlds:
            for kind, b in (("trimmed", min(1, (W - 1) // 2)), ("median", (W - 1) // 2)):
                runs.append((kind, W, b, 4 * (W + 1),
                             lambda W=W, b=b: nat.robust_reduce(S(), rows.data_ptr(), ld, W, n, b, out.data_ptr(),
                                                                partial.data_ptr(), stats.data_ptr())))
        us = {i: [] for i in range(len(runs))}
        for _ in range(a.reps):                                  # the variants alternate in one run
            for i, (name, W, b, bpe, fn) in enumerate(runs):
                m.normal_()
                us[i].append(_time(fn, iters))
        flat = statistics.median(us[0]) / (n * 20)               # us per byte of a streaming kernel, this run
        for i, (name, W, b, bpe, fn) in enumerate(runs):
            t = statistics.median(us[i])
            rec = {"kernel": name, "n": n, "W": W, "b_eff": b, "us": round(t, 2), "min": round(min(us[i]), 2),
                   "max": round(max(us[i]), 2), "bytes_per_entry": bpe, "GBps": round(n * bpe / t / 1e3, 1),
                   "x_sgd_flat_per_byte": round(t / (n * bpe) / flat, 2), "iters": iters, "reps": a.reps}
            print(json.dumps(rec), flush=True)


def _peer_worker(rank, world, path, sizes, iters, q):
    import torch.distributed as dist

    from fedmi.parallel.peer import PeerAllReduce

    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    nat = native.require()
    store = dist.FileStore(path, world)
    pc = PeerAllReduce(rank, world, 4 * max(sizes) + 4096, store, tag="bench", device=dev)
    pc.comm.set_timeout_ms(float(os.environ.get("FEDMI_BENCH_PEER_TIMEOUT_MS", "30000")))
    partials = torch.zeros((nat.PEER_MAX_BLOCKS, 16), dtype=torch.int64, device=dev)
    stats = torch.zeros(16, dtype=torch.int64, device=dev)
    res = []
    for n in sizes:
        x0 = torch.randn(n, device=dev)
        x = x0.clone()
        it = iters
        variants = [("dense_oneshot", 0, lambda: pc.allreduce_mean_(x)),
                    ("trimmed", min(1, (world - 1) // 2),
                     lambda: pc.allreduce_robust_(x, min(1, (world - 1) // 2), partials, stats)),
                    ("median", (world - 1) // 2, lambda: pc.allreduce_robust_(x, (world - 1) // 2, partials, stats))]
        times = {name: [] for name, _, _ in variants}
        for _ in range(3):                                       # alternate the variants in one run
            for name, b, fn in variants:
                x.copy_(x0)
                for _ in range(5):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(it):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / it)
        for name, b, _ in variants:
            res.append((name, b, n, statistics.median(times[name])))
    err = pc.error()
    pc.close()
    q.put((rank, res, err))


def peer(a) -> None:
    os.environ["FEDMI_PEER_GATE"] = "0"
    os.environ["FEDMI_BENCH_PEER_TIMEOUT_MS"] = "2000"
    for world in a.worlds:
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "store")
            procs = [ctx.Process(target=_peer_worker, args=(r, world, path, a.sizes, a.iters, q)) for r in range(world)]
            for p in procs:
                p.start()
            got = [q.get(timeout=600) for _ in procs]
            for p in procs:
                p.join(timeout=60)
        errs = [e for _, _, e in got]
        dense = {}
        for i, (name, b, n, _) in enumerate(got[0][1]):
            us = max(g[1][i][3] for g in got)
            if name == "dense_oneshot":
                dense[n] = us
            rec = {"bench": "peer_robust", "world": world, "numel": n, "algo": name, "b_eff": b,
                   "us_per_call": round(us, 2), "over_dense_us": round(us - dense[n], 2),
                   "gpus": torch.cuda.device_count(), "errors": errs, "host_gate": False}
            print(json.dumps(rec), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[LENET, RESNET18])
    ap.add_argument("--worlds", nargs="+", type=int, default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--peer", action="store_true", help="time the fused peer kernel against the dense one-shot")
    a = ap.parse_args()
    if a.worlds is None:
        a.worlds = [2, 4] if a.peer else [2, 4, 8, 16]
    peer(a) if a.peer else kernels(a)


if __name__ == "__main__":
    main()
