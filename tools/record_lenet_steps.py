"""Record what the fused LeNet step computes, as hashes (tests/golden/lenet_steps_parent.json).

From a fixed init on a fixed (CPU-generated) dataset the script runs

* 12 eager steps with momentum that mix batch sizes 128 / 7 / 40 / 1 over two round-counter values
  (step 6 bumps the counter), and
* two graph epochs of the irregular schedule starts [0, 640, 256, 384], sizes [128, 7, 128, 40],

and after each step / epoch keeps SHA-256 of params || momentum and the raw train-stats row.
``tests/test_lenet_seam_gpu.py`` recomputes the same figures and compares them, so a change to the
step's kernels or to how the engine issues them has to reproduce the recorded step bit for bit.

The record is re-made (``python tools/record_lenet_steps.py --write``, on the GPU, at the commit whose
arithmetic is the reference) only by a change that is MEANT to alter the step's arithmetic.
"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "lenet_steps_parent.json"
SEED = 1234
EAGER_STEPS = [(0, 128), (640, 7), (256, 128), (384, 40), (5, 1), (128, 128),
               (896, 128), (1017, 7), (512, 40), (640, 128), (1023, 1), (256, 128)]
BUMP_AFTER = 6            # the 6th step bumps the round counter: steps 7..12 draw other crops
SCHED_STARTS, SCHED_SIZES = [0, 640, 256, 384], [128, 7, 128, 40]


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def compute(dev) -> dict:
    from fedmi.engine.base import TrainerConfig
    from fedmi.engine.data import make_dataset
    from fedmi.engine.lenet_native import LeNetNativeTrainer
    from fedmi.models.small import LeNet

    ds = make_dataset("synthetic-cifar10", n_train=1024, n_test=512, device="cpu", seed=3)
    torch.manual_seed(0)
    init = LeNet().state_dict()
    tr = LeNetNativeTrainer(ds, dev, TrainerConfig(seed=SEED), init_state=init)
    torch.cuda.synchronize()
    out = {"dataset": _sha(ds.train.x, ds.train.y), "init": _sha(tr.params), "eager": [], "graph": []}

    def snap():
        torch.cuda.synchronize()
        return {"state": _sha(tr.params, tr.mom), "stats": [int(v) for v in tr.stats[0].cpu()]}

    tr.round_ctr.fill_(3)
    for i, (start, nb) in enumerate(EAGER_STEPS):
        tr.train_step(start, nb, bump_round=(i + 1 == BUMP_AFTER))
        out["eager"].append(snap())

    tr.load_state_dict(init)
    tr.mom.zero_()
    tr.stats.zero_()
    tr.round_ctr.zero_()
    tr.cfg.use_graph = True
    tr.set_schedule(SCHED_STARTS, SCHED_SIZES)
    for _ in range(2):
        tr.train_epoch()
        out["graph"].append(snap())
    return out


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
