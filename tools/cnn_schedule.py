"""Ordered launch trace of the native CNN engine under the CPU emulation (no GPU needed).

    python tools/cnn_schedule.py ARCH [--nb 8] > file

One line per call of a kernel entry point of fedmi.ops.conv / fedmi.ops.cnn: the op, then every argument by
name.  A tensor prints as b<k>:<shape>/<strides>, k numbering the distinct data_ptr() values in order of first
appearance, so the trace does not depend on where the allocator put things but does on which buffer feeds which
launch.  Two trees issue the same schedule exactly when ``diff`` of their traces is empty.  The run is that of
tests/test_cnn_shadow_cpu.py: two training passes of one batch, then an evaluation.
"""
import argparse
import functools
import inspect
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import emulate  # noqa: E402
from fedmi.engine.base import TrainerConfig  # noqa: E402
from fedmi.engine.cnn_native import CNNNativeTrainer  # noqa: E402
from fedmi.engine.data import make_dataset  # noqa: E402
from fedmi.ops import cnn, conv  # noqa: E402
from shadow import CNN_OPS, CONV_OPS  # noqa: E402

_bufs = {}


def fmt(v) -> str:
    if isinstance(v, torch.Tensor):
        k = _bufs.setdefault(v.data_ptr(), len(_bufs))
        return f"b{k}:{'x'.join(map(str, v.shape))}/{','.join(map(str, v.stride()))}"
    if isinstance(v, cnn.BNParams):
        return "BN(" + " ".join(f"{k}={fmt(getattr(v, k))}" for k in v.__slots__) + ")"
    if isinstance(v, dict):
        return "{" + " ".join(f"{k}={fmt(x)}" for k, x in v.items()) + "}"
    if isinstance(v, (list, tuple)):
        return "[" + " ".join(map(fmt, v)) + "]"
    return repr(v)


def traced(name, fn):
    sg = inspect.signature(fn)

    @functools.wraps(fn)
    def f(*a, **k):
        b = sg.bind(*a, **k)
        b.apply_defaults()
        print(name, *(f"{n}={fmt(v)}" for n, v in b.arguments.items()))
        return fn(*a, **k)

    return f


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("arch")
    ap.add_argument("--nb", type=int, default=8)
    args = ap.parse_args()
    torch.manual_seed(0)
    data = make_dataset("synthetic-cifar10", device="cpu", n_train=16, n_test=40, seed=0)
    with emulate.emulated():     # restores the modules' own entry points on exit, the wrappers with them
        for mod, names in ((conv, CONV_OPS), (cnn, CNN_OPS + ("sched_next",))):
            for n in names:
                setattr(mod, n, traced(n, getattr(mod, n)))
        tr = CNNNativeTrainer(args.arch, data, torch.device("cpu"),
                              TrainerConfig(batch_size=args.nb, eval_batch_size=16, augment=False, use_graph=False))
        tr.grads_for_batch(0, args.nb)
        tr.grads_for_batch(0, args.nb)
        tr.evaluate()


if __name__ == "__main__":
    main()
