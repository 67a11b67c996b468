"""Record the fused LeNet step at the edges of its FC tail (tests/golden/lenet_fc_tail_parent.json).

A sibling of ``record_lenet_steps.py`` (same dataset, same hashing) with a second case set: batch sizes
1, 2, 33 and 128 on three parameter sets written through the engine's state and ``pack``:

* ``zero_fc3``  fc3.weight = 0 and fc3.bias = 0: all logits tie, argmax must be class 0;
* ``dead_fc2``  fc2.bias = -10: every h2 is dead, dZ2 is zero, the fc1 / conv gradients are weight decay alone;
* ``random``    the fixed random init.

Per set: two eager steps (one sample of class 0; two samples ending in one of class 9), then from the same
init one graph epoch of the schedule sizes [128, 1, 33] (the single sample is of class 9; the 128 cover every
class).  After each step / epoch it keeps SHA-256 of params || momentum and the raw train-stats row.
``tests/test_lenet_fc_tail_gpu.py`` recomputes and compares.

The record is made on the GPU at the commit whose arithmetic is the reference
(``python tools/record_lenet_fc_tail.py --write``): twice, and the two records must be identical.
"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "lenet_fc_tail_parent.json"
SEED = 1234
CASES = ("zero_fc3", "dead_fc2", "random")
SCHED_SIZES = [128, 1, 33]


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def dataset():
    from fedmi.engine.data import make_dataset

    return make_dataset("synthetic-cifar10", n_train=1024, n_test=512, device="cpu", seed=3)


def init_state(case: str):
    from fedmi.models.small import LeNet

    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in LeNet().state_dict().items()}
    if case == "zero_fc3":
        sd["fc3.weight"].zero_()
        sd["fc3.bias"].zero_()
    elif case == "dead_fc2":
        sd["fc2.bias"].fill_(-10.0)
    else:
        assert case == "random", case
    return sd


def plan(ds):
    """Eager steps and the graph schedule, chosen from the labels: class 0 and class 9 at the single-sample steps."""
    y = ds.train.y.cpu().numpy()
    i0 = int((y == 0).nonzero()[0][0])
    i9 = int((y[1:] == 9).nonzero()[0][0]) + 1
    eager = [(i0, 1), (i9 - 1, 2)]
    starts = [0, i9, 512]
    assert set(y[:128].tolist()) == set(range(10)), "the full batch covers every class"
    assert y[i0] == 0 and y[i9] == 9 and 512 + 33 <= len(y)
    return eager, starts, list(SCHED_SIZES)


def compute(dev, probe=None) -> dict:
    """probe(case, kind, index, trainer, (start, nb) or (starts, sizes)) is called after each recorded point."""
    from fedmi.engine.base import TrainerConfig
    from fedmi.engine.lenet_native import LeNetNativeTrainer

    ds = dataset()
    eager, starts, sizes = plan(ds)
    out = {"dataset": _sha(ds.train.x, ds.train.y), "eager_steps": [list(e) for e in eager],
           "schedule": [starts, sizes], "cases": {}}
    for case in CASES:
        init = init_state(case)
        tr = LeNetNativeTrainer(ds, dev, TrainerConfig(seed=SEED), init_state=init)
        torch.cuda.synchronize()
        rec = {"init": _sha(tr.params), "eager": [], "graph": []}

        def snap():
            torch.cuda.synchronize()
            return {"state": _sha(tr.params, tr.mom), "stats": [int(v) for v in tr.stats[0].cpu()]}

        tr.round_ctr.fill_(3)
        for i, (start, nb) in enumerate(eager):
            tr.stats.zero_()
            tr.train_step(start, nb)
            rec["eager"].append(snap())
            if probe:
                probe(case, "eager", i, tr, (start, nb))

        tr.load_state_dict(init)
        tr.mom.zero_()
        tr.stats.zero_()
        tr.round_ctr.zero_()
        tr.cfg.use_graph = True
        tr.set_schedule(starts, sizes)
        tr.train_epoch()
        rec["graph"].append(snap())
        if probe:
            probe(case, "graph", 0, tr, (starts, sizes))
        out["cases"][case] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--write", action="store_true", help=f"write {GOLDEN.relative_to(ROOT)} (default: compare with it)")
    ap.add_argument("--out", default=None, help="write the record to this file instead")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rec = compute(dev)
    if rec != compute(dev):
        print("two records of the same build DIFFER")
        return 2
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
