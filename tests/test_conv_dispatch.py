"""Host-side conv routing, pinned without a GPU.

``dispatch_recorder.hip`` compiles csrc/kernels/conv_igemm.hip with the launch macro replaced by a recorder and
runs the real launchers on fake pointers: per launch the kernel instantiation, grid, block, K steps per split,
workspace offsets and geometry.  ``golden/conv_dispatch_cus256.txt.gz`` is that record for every shape of
``golden/conv_dispatch_shapes.txt`` (the zoo's dense convs at batch 128 and 8, the shapes of
test_cnn_kernels_gpu.py, three small split-K shapes), taken from the commit BEFORE the planner (conv_plan.h)
existed; only the two ``conv_wgrad_halo`` instantiation names were rewritten to their one-parameter form.  Every sum
in these kernels is fixed-order, so a changed split count or tile changes training results bitwise: a routing change
has to show up here, and be meant.

To re-record after a deliberate change: build the recorder as below, run it on the shape table and gzip the output.
"""
import difflib
import gzip
import shutil
import subprocess
from pathlib import Path

import pytest

import emulate
from fedmi.ops import conv

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)
CLANGXX = shutil.which("clang++") or next(
    (str(p) for p in (Path("/opt/rocm/lib/llvm/bin/clang++"), Path("/opt/rocm/llvm/bin/clang++")) if p.exists()), None)


def _golden() -> str:
    return gzip.decompress((GOLDEN / "conv_dispatch_cus256.txt.gz").read_bytes()).decode()


@pytest.fixture(scope="module")
def record(tmp_path_factory) -> str:
    if HIPCC is None:
        pytest.skip("hipcc not found")
    exe = tmp_path_factory.mktemp("dispatch") / "dispatch_recorder"
    # host side only: the launchers run, no kernel is compiled or started
    subprocess.run([HIPCC, "-O0", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", str(ROOT / "csrc"),
                    str(ROOT / "tests" / "dispatch_recorder.hip"), "-o", str(exe)], check=True, capture_output=True)
    return subprocess.run([str(exe), str(GOLDEN / "conv_dispatch_shapes.txt")], check=True, capture_output=True,
                          text=True).stdout


def test_dispatch_record_is_the_recorded_one(record):
    want = _golden()
    if record != want:
        diff = list(difflib.unified_diff(want.splitlines(), record.splitlines(), "golden", "this tree", n=1, lineterm=""))
        pytest.fail("conv routing changed (%d diff lines):\n%s" % (len(diff), "\n".join(diff[:60])))
    assert record.count("\nshape ") + 1 >= 288


def test_python_mirrors_agree_with_the_planner(record):
    """tests/emulate.py::dgrad_fusable and conv.dgrad_eligible against the C++ answers of every shape in the table."""
    blocks = record.split("shape ")[1:]
    assert len(blocks) >= 288
    for b in blocks:
        lines = b.splitlines()
        N, H, W, C, O, R, st, pad = (int(v) for v in lines[0].split())
        fus = [int(v) for v in lines[1].split("fusable=")[1].split(",")]
        for has_wd in (0, 1):
            assert emulate.dgrad_fusable((N, H, W, C), O, R, R, st, pad, has_wd=bool(has_wd)) == bool(fus[has_wd]), lines[0]
        # with a DGRAD image the launch takes the tap path exactly where Python says a conv gets an image
        # (a record equal to an earlier variant's prints as "label == earlier label": the same launches without an image)
        i = next(k for k, ln in enumerate(lines) if ln.startswith(" dgrad.wd1.acc0"))
        tap = "==" not in lines[i] and lines[i + 1].lstrip().startswith("conv_tap")
        assert conv.dgrad_eligible(O, st) == tap, lines[0]


def test_planner_sweep_under_sanitizers(tmp_path):
    """plan_sweep.cpp: the planner's invariants over a grid of shapes, CU counts and workspace caps, as a stand-alone
    host program built with AddressSanitizer and UndefinedBehaviorSanitizer."""
    if CLANGXX is None:
        pytest.skip("clang++ not found")
    exe = tmp_path / "plan_sweep"
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "csrc"), str(ROOT / "tests" / "plan_sweep.cpp"), "-o", str(exe)], check=True,
                   capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "plan sweep ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
