"""KS1's cross-lane helpers (csrc/kernels/xlane.h: DPP, permlane swaps, readlane) against the shuffle
formulations they replaced, bit for bit.

``lenet_xlane_probe`` runs one wave per input row of 64 floats and writes, for every helper KS1 uses, the
helper's result and that of the ``__shfl_xor`` / ``__shfl`` butterfly of the parent (for fc1's row sums: the
separate ``mov_dpp`` + add), which is kept in the probe only.  The two are compared as int32 bit patterns in
all 64 lanes -- a superset of the lanes the call sites consume (lane 0 of a group for the sums, lanes 0..15
of the cross-entropy block, any lane for the label lookup).  One wave is the smallest shape at which a wrong
partner lane, a wrong step order or a missing wait state shows.

Rows: normals over 2^-100..2^100 with mixed signs; rows mixing +-0, denormals and infinities; rows whose
maximum (minimum) sits in several lanes -- the first-index rule of the CE block's ``cand``; rows with all 16
values of a DPP row equal; CE-shaped rows (-inf in lanes 10..15 of every 16); every label 0..9 (and the other
54 lanes) for the broadcast.  No NaN inputs: the step feeds none, and max / min operand order with NaN is
not part of the helpers' contract.  For the same reason a row holds infinities of one sign only (the sums
of a row with both would be NaN from the second step on); both signs occur, in different rows.
"""
import numpy as np
import pytest
import torch

from fedmi import native

pytestmark = pytest.mark.gpu

HELPERS = ["sum8", "sum16", "max16", "min16", "sum32", "add_xor16+add_xor32", "row_sum16", "bcast"]


def _rows():
    rng = np.random.default_rng(20)
    rows = []

    def normals(n):
        mag = np.exp2(rng.uniform(-100.0, 100.0, size=(n, 64)))
        return (mag * rng.choice([-1.0, 1.0], size=(n, 64))).astype(np.float32)

    rows.append(normals(96))
    # like magnitudes (sums that cancel and round at every step)
    rows.append((rng.standard_normal((64, 64)) * np.exp2(rng.integers(-20, 20, size=(64, 1)))).astype(np.float32))
    # +-0, denormals, infinities of one sign per row, normals
    tiny = np.float32(1.401298464324817e-45)
    for sign in (1.0, -1.0):
        pool = np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, -5 * tiny, 1.1754942e-38, -1.1754942e-38,
                         sign * np.inf, 1.0, -2.5, 3e-39, -3e-39], dtype=np.float32)
        rows.append(pool[rng.integers(0, len(pool), size=(24, 64))])
    zeros = np.array([0.0, -0.0], dtype=np.float32)
    rows.append(zeros[rng.integers(0, 2, size=(16, 64))])                     # only signed zeros
    rows.append(np.array([0.0, -0.0, tiny, -tiny], dtype=np.float32)[rng.integers(0, 4, size=(16, 64))])
    # the maximum / minimum in several lanes of a 16-lane row
    few = rng.integers(-3, 4, size=(48, 64)).astype(np.float32)
    rows.append(few)
    rows.append(few[:16] * np.float32(0.1))
    # all 16 values of a DPP row equal (one value per row of 16, and one per wave)
    rows.append(np.repeat(normals(16)[:, :4], 16, axis=1))
    rows.append(np.repeat(normals(8)[:, :1], 64, axis=1))
    # CE-shaped: logits in lanes 0..9 of every 16, -inf in lanes 10..15; with ties and with all logits equal
    ce = (rng.standard_normal((48, 64)) * 4).astype(np.float32)
    ce[16:32] = np.round(ce[16:32])
    ce[32:40] = ce[32:40, :1]
    ce[40:48] = 0.0
    ce.reshape(48, 4, 16)[:, :, 10:] = -np.inf
    rows.append(ce)
    x = np.ascontiguousarray(np.concatenate(rows, axis=0), dtype=np.float32)
    assert not np.isnan(x).any()
    # broadcast source lanes: every label 0..9 first, then every other lane of the wave
    labels = (np.arange(len(x)) % 64).astype(np.int32)
    return x, labels


@pytest.fixture(scope="module")
def probe(gpu_device):
    nat = native.require()
    x, labels = _rows()
    n = nat.XLANE_PROBE_HELPERS
    assert n == len(HELPERS)
    xd = torch.from_numpy(x).to(gpu_device)
    ld = torch.from_numpy(labels).to(gpu_device)
    out = torch.full((len(x), n, 2, 64), float("nan"), dtype=torch.float32, device=gpu_device)
    nat.lenet_xlane_probe(torch.cuda.current_stream().cuda_stream, xd.data_ptr(), ld.data_ptr(), len(x), out.data_ptr())
    torch.cuda.synchronize()
    return x, labels, out.cpu().numpy()


@pytest.mark.parametrize("h", range(len(HELPERS)), ids=HELPERS)
def test_helper_has_the_shuffle_butterflys_bits(probe, h):
    x, labels, out = probe
    got, ref = out[:, h, 0].view(np.int32), out[:, h, 1].view(np.int32)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (f"{HELPERS[h]}: {len(bad)} lanes differ, first (row, lane) {bad[0].tolist()}: "
                           f"{out[bad[0][0], h, 0, bad[0][1]]!r} vs {out[bad[0][0], h, 1, bad[0][1]]!r}")


def test_reference_formulations_are_what_they_claim(probe):
    """The reference side of the probe against numpy where that is exact: max / min over each 16 lanes (as
    values; +-0 compare equal), the broadcast of lane label, and the rows came through unchanged."""
    x, labels, out = probe
    assert not np.isnan(out[:, [2, 3, 7]]).any()
    x16 = x.reshape(len(x), 4, 16)
    assert np.array_equal(out[:, 2, 1].reshape(len(x), 4, 16), np.broadcast_to(x16.max(axis=2, keepdims=True), x16.shape))
    assert np.array_equal(out[:, 3, 1].reshape(len(x), 4, 16), np.broadcast_to(x16.min(axis=2, keepdims=True), x16.shape))
    want = x[np.arange(len(x)), labels]
    assert np.array_equal(out[:, 7, 1].view(np.int32), np.broadcast_to(want.view(np.int32)[:, None], (len(x), 64)))
    assert set(labels[:64].tolist()) >= set(range(10))
