"""Record what the native aten backend computes and launches for the zoo families, as hashes and counters
(tests/golden/zoo_steps_parent.json).

For each family in FAMILIES, from a CPU-seeded init on a CPU-generated dataset, the script runs three eager
batch-64 steps of the hybrid trainer (the first learns the concat and pack plans, the second uses them, the third
is the steady state) with the backend's diagnostics on, and after each step keeps

* SHA-256 of float_state() || momentum_state() and the train-stats row, and
* the backend's counters: ``fused``, ``native_ops``, ``packs``, ``fallbacks``, ``ew_ops``, ``scalar_ew`` (the
  last two count every elementwise launch, the materialisations at the block's exit included).

It also runs a tiny block (conv, BN, ReLU, a residual add, two channel slices and their cat) forward and backward
under a plain ``NativeMode(strict=True)`` -- the exit path outside a trainer, where tensors left unwritten by a
fusion are materialised when the block ends -- and hashes the output and every gradient read after the block.

``tests/test_zoo_steps_gpu.py`` recomputes the same figures and compares them, so a change to the backend's host
logic has to reproduce the recorded steps bit for bit AND launch for launch.

The record is re-made (``python tools/record_zoo_steps.py --write``, on the GPU, at the commit whose behaviour is
the reference) only by a change that is MEANT to alter the steps' arithmetic or their launch sequence.
"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "zoo_steps_parent.json"
FAMILIES = ["densenet_cifar", "ResNeXt29_2x64d", "DPN26", "SENet18", "EfficientNetB0", "ShuffleNetV2"]
SEED = 1234
BATCH = 64
STEPS = 3
COUNTERS = ("fused", "native_ops", "packs", "fallbacks", "ew_ops", "scalar_ew")


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _counters(mode) -> dict:
    return {name: {str(k): int(v) for k, v in sorted(getattr(mode, name).items(), key=lambda kv: str(kv[0]))}
            for name in COUNTERS}


def _dataset():
    from fedmi.engine.data import make_dataset

    return make_dataset("synthetic-cifar10", n_train=BATCH * STEPS, n_test=BATCH, device="cpu", seed=3)


def compute_family(name: str, dev) -> dict:
    from fedmi.engine import build_trainer
    from fedmi.engine.base import TrainerConfig
    from fedmi.models import build_model

    ds = _dataset()
    torch.manual_seed(0)
    init = build_model(name).state_dict()
    cfg = TrainerConfig(seed=SEED, batch_size=BATCH, augment=False, use_graph=False)
    tr = build_trainer(name, ds, dev, cfg, init_state=init)
    tr.mode.diag = True
    tr.model.train()
    out = {"dataset": _sha(ds.train.x, ds.train.y), "init": _sha(*init.values()), "steps": []}
    for i in range(STEPS):
        tr.train_step(BATCH * i, BATCH)
        torch.cuda.synchronize()
        st = tr.train_stats()
        out["steps"].append({"state": _sha(tr.float_state(), tr.momentum_state()),
                             "stats": [float(st.loss_sum), int(st.correct), int(st.count)],
                             **_counters(tr.mode)})
    return out


def compute_block(dev) -> dict:
    """conv -> BN -> (+ x) -> ReLU -> two channel slices -> cat, forward and backward under a plain strict mode."""
    import torch.nn as nn

    from fedmi.ops.native_mode import NativeMode

    torch.manual_seed(7)
    conv = nn.Conv2d(8, 8, 3, padding=1, bias=False)
    bn = nn.BatchNorm2d(8)
    x = torch.randn(4, 8, 8, 8)
    w = torch.randn(4, 8, 8, 8)
    conv, bn = conv.to(dev), bn.to(dev)
    bn.train()
    x = x.to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = w.to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    torch.cuda.synchronize()
    mode = NativeMode(strict=True)
    mode.diag = True
    with mode:
        y = torch.relu(bn(conv(x)) + x)
        z = torch.cat([y[:, 3:], y[:, :3]], 1)
        (z * w).sum().backward()
    torch.cuda.synchronize()
    params = list(conv.parameters()) + list(bn.parameters())
    return {"out": _sha(z), "grads": [_sha(p.grad) for p in params] + [_sha(x.grad)],
            "buffers": _sha(*bn.buffers()), **_counters(mode)}


def compute(dev, families=FAMILIES) -> dict:
    return {"families": {name: compute_family(name, dev) for name in families}, "block": compute_block(dev)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--write", action="store_true", help=f"write {GOLDEN.relative_to(ROOT)} (default: compare with it)")
    ap.add_argument("--out", default=None, help="write the record to this file instead")
    a = ap.parse_args()
    rec = compute(torch.device("cuda", 0))
    if a.write or a.out:
        path = Path(a.out) if a.out else GOLDEN
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {path}")
        return 0
    same = rec == json.loads(GOLDEN.read_text())
    print("record matches" if same else "record DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
