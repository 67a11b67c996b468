"""Time the server-optimizer step (csrc/kernels/server_opt.hip) against sgd_flat at the same length.

    python tools/bench_server_opt.py [--sizes 62006 11173962] [--iters 200] [--cold]

Prints one JSON line per (size, kernel): microseconds per launch (HIP-graph replay of `iters` launches), the
bytes it moves per entry (sgd_flat 20, fedavgm 24, adaptive 32) and the resulting ns per KiB, so the streaming
kernels can be compared per byte.  --cold: every launch follows a 1 GiB streaming pass that evicts the 256 MB
last-level cache (after a local epoch the model state is cold); the pass alone is timed and subtracted.
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from fedmi import native  # noqa: E402
from fedmi.parallel.server_opt import KINDS  # noqa: E402

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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[LENET, RESNET18])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--cold", action="store_true")
    a = ap.parse_args()
    nat = native.require()
    dev = torch.device("cuda:0")
    flush = torch.zeros(1 << 28, device=dev) if a.cold else None   # 1 GiB
    t_flush = _time(lambda: flush.add_(1.0), a.iters) if a.cold else 0.0
    for n in a.sizes:
        # lr 0 / a zero pseudo-gradient keep the values finite over hundreds of replays; the traffic is the same
        x, anchor, m, g = (torch.randn(n, device=dev) for _ in range(4))
        anchor.copy_(x)
        v = torch.rand(n, device=dev) + 1e-3

        def S():
            return native.stream_handle(dev)

        runs = [("sgd_flat", 20, lambda: nat.sgd_flat(S(), x.data_ptr(), g.data_ptr(), m.data_ptr(), n, 0.0, 0.9, 0.0,
                                                      0.0, False, False))]
        for k, kind in enumerate(KINDS):
            runs.append((kind, 24 if kind == "fedavgm" else 32,
                         lambda k=k: nat.server_opt(S(), x.data_ptr(), anchor.data_ptr(), m.data_ptr(),
                                                    0 if k == 0 else v.data_ptr(), n, n, k, 0.0, 0.9, 0.99, 1e-3)))
        for name, bpe, fn in runs:
            m.normal_()                         # decays by 0.9 per launch: restart it well above the denormals
            step = (lambda fn=fn: (flush.add_(1.0), fn())) if a.cold else fn
            us = _time(step, a.iters) - t_flush
            print(json.dumps({"kernel": name, "n": n, "us": round(us, 2), "bytes_per_entry": bpe,
                              "ns_per_KiB": round(us * 1e3 / (n * bpe / 1024), 3), "GBps": round(n * bpe / us / 1e3, 1),
                              "cold": a.cold, "flush_us": round(t_flush, 2)}), flush=True)


if __name__ == "__main__":
    main()
