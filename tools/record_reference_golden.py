"""Record the facts about the reference project that the CPU tests compare against, as small data files
under tests/golden/ (no reference source is copied):

  model_zoo.json       per model factory: the logits the reference model gives in float64 for the seeded weights
                       and input of tests/helpers.py (``seeded_state`` / ``seeded_input``), and the sorted
                       keys / shapes / dtypes of its state dict (``pack_layout``)
  wire_reference.json  the reference's generated protobuf module read back at run time: package, syntax,
                       messages and fields, service methods, and the bytes it serializes sample messages to

usage:  python tools/record_reference_golden.py --ref <reference checkout>
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests.helpers import pack_layout, seeded_input, seeded_state, state_layout  # noqa: E402
from tests.test_models import CASES  # noqa: E402
from tests.test_wire import SAMPLES  # noqa: E402


def record_models(src: Path) -> dict:
    out = {}
    for name, fname, expr in CASES:
        spec = importlib.util.spec_from_file_location(f"_ref_{fname}", src / "models" / f"{fname}.py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        ref = eval(expr, vars(mod))  # noqa: S307  (reference factory call, e.g. "ResNet18()")
        layout = state_layout(ref.state_dict())
        ref.load_state_dict(seeded_state(layout))
        ref.double().eval()
        with torch.no_grad():
            y = ref(seeded_input())
        assert torch.isfinite(y).all(), name
        out[name] = {"logits": y.tolist(), "layout": pack_layout(layout)}
        print(f"{name}: {len(layout)} entries, |logits| max {float(y.abs().max()):.4f}")
    return out


def record_wire(src: Path) -> dict:
    from google.protobuf import descriptor_pb2

    sys.path.insert(0, str(src))
    try:
        import federated_pb2 as R  # noqa: N812
    finally:
        sys.path.remove(str(src))
    fd = descriptor_pb2.FileDescriptorProto.FromString(R.DESCRIPTOR.serialized_pb)
    (svc,) = fd.service
    return {
        "name": fd.name, "package": fd.package, "syntax": fd.syntax,
        "messages": [{"name": m.name, "fields": [[f.name, f.number, f.type, f.label] for f in m.field]}
                     for m in fd.message_type],
        "service": {"name": svc.name, "methods": [[m.name, m.input_type, m.output_type] for m in svc.method]},
        "samples": {name: getattr(R, name)(**kw).SerializeToString().hex() for name, kw in SAMPLES},
    }


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", required=True, type=Path, help="checkout of the reference project")
    ap.add_argument("--out", type=Path, default=ROOT / "tests" / "golden")
    a = ap.parse_args()
    a.out.mkdir(parents=True, exist_ok=True)
    for name, rec in (("wire_reference", record_wire(a.ref / "src")), ("model_zoo", record_models(a.ref / "src"))):
        rows = ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in rec.items())     # one line per entry
        (a.out / f"{name}.json").write_text("{\n" + rows + "\n}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
