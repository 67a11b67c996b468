"""csrc/kernels/bn_math.h without a GPU: its numpy reference (tests/bn_check.py) against rational arithmetic, and the
header itself, compiled for the host, against the reference -- bit for bit, on the committed inputs of
tests/golden/bn_math_inputs.txt (random values, the rounding-distance case sh = -fp32(z * sc), products that are exact
fp32 ties, subnormal results, inv across 20 decades, cancelling variances)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bn_check

ROOT = Path(__file__).resolve().parent.parent
INPUTS = ROOT / "tests" / "golden" / "bn_math_inputs.txt"
CLANGXX = shutil.which("clang++") or next(
    (str(p) for p in (Path("/opt/rocm/lib/llvm/bin/clang++"), Path("/opt/rocm/llvm/bin/clang++")) if p.exists()), None)


@pytest.fixture(scope="module")
def rows():
    return bn_check.parse_inputs(INPUTS.read_text())


def test_committed_inputs_parse(rows):
    f, d, Ms = rows
    assert len(f) >= 1000 and np.isfinite(f).all() and np.isfinite(d).all() and (Ms >= 1).all()
    assert bn_check.format_inputs(zip(f, d, Ms)) == INPUTS.read_text()


def test_inputs_hold_the_cases_they_claim(rows):
    f, d, Ms = rows
    a, b, c = (f[:, i].astype(np.float64) for i in range(3))
    with np.errstate(all="ignore"):
        prod32 = (f[:, 0] * f[:, 1]).astype(np.float64)
    exact = a * b                                               # exact in fp64
    assert int(((c == -prod32) & (exact != prod32)).sum()) >= 50            # at rounding distance: fma != 0, unfused == 0
    tie = (exact != prod32) & (np.abs(exact - prod32) == np.abs(np.spacing(prod32.astype(np.float32)).astype(np.float64)) / 2)
    assert int(tie.sum()) >= 100                                            # products half way between two fp32
    ref = bn_check.evaluate(f, d, Ms)
    tiny = np.finfo(np.float32).tiny
    assert int(((np.abs(ref[:, 0]) < tiny) & (ref[:, 0] != 0)).sum()) >= 50  # subnormal results
    e = np.abs(f[:, 4])
    assert e.max() >= 1e10 and e[e > 0].min() <= 1e-10                      # inv over 20 decades
    assert int((ref[:, 7] == 0).sum()) >= 10                                # variances clamped at zero


def test_reference_matches_rational_arithmetic(rows):
    f, d, Ms = rows
    n = len(f)
    idx = np.unique(np.concatenate([np.arange(0, n, 7), np.arange(480, 800, 3)]))    # every case, all the tie rows' kin
    assert bn_check.self_check(f, d, Ms, idx) >= 17 * len(idx)


def test_bf16_round_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8], dtype=np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0], dtype=np.float32)
    assert np.array_equal(bn_check.bf16_round(x), want)


def test_header_on_the_host_matches_the_reference(rows, tmp_path):
    """bn_math.h compiled as plain host C++ (a stand-alone program, under AddressSanitizer and
    UndefinedBehaviorSanitizer) evaluates every function on the committed rows; the bits equal the reference's."""
    if CLANGXX is None:
        pytest.skip("clang++ not found")
    exe = tmp_path / "bn_math_host"
    subprocess.run([CLANGXX, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "csrc"), str(ROOT / "tests" / "bn_math_host.cpp"), "-o", str(exe)], check=True,
                   capture_output=True)
    out = subprocess.run([str(exe)], input=INPUTS.read_text(), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.array([[int(v, 16) for v in ln.split()] for ln in out.stdout.splitlines()], dtype=np.uint32)
    f, d, Ms = rows
    want = bn_check.evaluate(f, d, Ms).view(np.uint32)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(r), bn_check.OUTPUTS[k], hex(got[r, k]), hex(want[r, k])) for r, k in bad[:10]]
