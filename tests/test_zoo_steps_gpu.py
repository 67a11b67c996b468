"""The native aten backend computes and launches what the committed record says (tests/golden/zoo_steps_parent.json,
made by tools/record_zoo_steps.py): three eager batch-64 steps per family -- state hash, train-stats row and every
counter of the backend (fusions, native ops, packs, fallbacks, elementwise launches per op code) -- and a tiny block
under a plain strict mode, whose unread deferred tensors are written at the block's exit.  A change to the backend's
host logic has to reproduce all of it; the record is re-made only by a change meant to alter it.
"""
import importlib.util
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
WANT = json.loads((ROOT / "tests" / "golden" / "zoo_steps_parent.json").read_text())


def _recorder():
    spec = importlib.util.spec_from_file_location("record_zoo_steps", ROOT / "tools" / "record_zoo_steps.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_record_covers_the_families():
    assert sorted(WANT["families"]) == sorted(_recorder().FAMILIES)
    assert all(len(f["steps"]) == 3 for f in WANT["families"].values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WANT["families"]))
def test_zoo_steps_match_parent_record(gpu_device, name):
    want = WANT["families"][name]
    got = _recorder().compute_family(name, gpu_device)
    assert got["dataset"] == want["dataset"] and got["init"] == want["init"], "the record's inputs are not reproduced"
    for i, (g, w) in enumerate(zip(got["steps"], want["steps"])):
        for key in w:
            assert g[key] == w[key], (name, "step", i, key)
    assert got == want


@pytest.mark.gpu
def test_exit_path_block_matches_parent_record(gpu_device):
    want = WANT["block"]
    got = _recorder().compute_block(gpu_device)
    for key in want:
        assert got[key] == want[key], key
    assert got == want
