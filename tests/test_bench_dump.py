"""bench.py --dump-outputs: the arrays of the last round as float32 / float64 .npy files, the same for the
same seeded run, a model over the size limit cut to a fixed sample, every BatchNorm counter of a model
that has some."""
import numpy as np
import torch

import bench
from tests.helpers import small_trainer


def _round(seed=0, **kw):
    tr = small_trainer(seed=seed, **kw)
    tr.set_schedule([0, 32], [32, 32])
    tr.train_epoch()
    tr.evaluate()
    return tr


def _dump(out_dir, tr, eval_stats):
    bench.dump_outputs(out_dir, bench.collect_outputs(tr, eval_stats))


def test_dump_writes_state_and_stats(tmp_path):
    tr = _round()
    _dump(tmp_path / "a", tr, tr.eval_stats())
    _dump(tmp_path / "b", _round(), tr.eval_stats())
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["eval_stats.npy", "float_state.npy", "train_stats.npy"]      # the MLP has no integer buffers
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all()
        assert np.array_equal(a, b), f                               # same seed, same inputs, same outputs
    w = np.load(tmp_path / "a" / "float_state.npy")
    assert w.dtype == np.float32 and np.array_equal(w, tr.float_state().numpy().reshape(-1))
    st = tr.train_stats()
    assert np.load(tmp_path / "a" / "train_stats.npy").tolist() == [st.loss_sum, st.correct, st.count]
    assert np.load(tmp_path / "a" / "eval_stats.npy")[2] == 256


def test_dump_writes_every_batchnorm_counter(tmp_path):
    tr = _round(model="pnasneta", n_train=64, n_test=32)
    counters = [b for k, b in tr.model.state_dict().items() if k.endswith("num_batches_tracked")]
    assert len(counters) > 2
    _dump(tmp_path / "a", tr, tr.eval_stats())
    ints = np.load(tmp_path / "a" / "int_state.npy")
    assert ints.dtype == np.float64 and ints.shape == (len(counters),)
    assert np.array_equal(ints, torch.stack(counters).numpy()) and (ints == 2).all()      # two training steps
    w = np.load(tmp_path / "a" / "float_state.npy")
    assert w.dtype == np.float32 and np.array_equal(w, tr.float_state().numpy().reshape(-1))


def test_dump_samples_a_state_over_the_limit(tmp_path, monkeypatch):
    tr = _round()
    n = tr.float_state().numel()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", (1 << 20) + 4 * (n // 3))
    _dump(tmp_path / "a", tr, None)
    _dump(tmp_path / "b", tr, None)
    a = np.load(tmp_path / "a" / "float_state.npy")
    assert a.size == n // 3 and np.array_equal(a, np.load(tmp_path / "b" / "float_state.npy"))
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= bench.DUMP_MAX_BYTES
    assert not (tmp_path / "a" / "eval_stats.npy").exists()
