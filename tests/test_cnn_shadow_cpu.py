"""The op-by-op shadow harness (tests/shadow.py) on a CPU-only host: it must be transparent, and it must be
able to fail.

* Transparency: the emulation shadowed by itself gives exactly zero error at every comparison, and the engine's
  gradients, buffers and statistics are bit-identical to the same run without the shadow (no state applied
  twice, no snapshot leaking into a live buffer).
* Sensitivity: one subtly wrong stand-in at a time; the shadow must raise and name that op.
* Coverage: every wrapped entry point (and every flag combination the harness treats specially) is exercised.
"""
import contextlib
import functools
import inspect

import pytest
import torch

import emulate
from emulate import emulated
from fedmi.engine.base import TrainerConfig
from fedmi.engine.data import make_dataset
from fedmi.ops import cnn, conv
from shadow import ALL_OPS, ShadowMismatch, shadow

ARCHS = ["ResNet18", "ResNet50", "MobileNet", "MobileNetV2", "VGG11", "PreActResNet18", "PreActResNet50", "GoogLeNet"]


@contextlib.contextmanager
def _bound(*patches):
    """Bind stand-ins (module, name, fn) inside an ``emulated()`` block, restored before it exits."""
    saved = [(m, n, getattr(m, n)) for m, n, _ in patches]
    for m, n, fn in patches:
        setattr(m, n, fn)
    try:
        yield
    finally:
        for m, n, fn in reversed(saved):
            setattr(m, n, fn)


def _engine_run(name, nb, shadowed, patches=(), evaluate=True, collect=True):
    """Two training passes (the second with shifted BN statistics) and an evaluation (16 / 16 / 8) of a fresh
    engine under emulation; returns (trainer, Shadow or None)."""
    from fedmi.engine.cnn_native import CNNNativeTrainer

    torch.manual_seed(0)
    data = make_dataset("synthetic-cifar10", device="cpu", n_train=16, n_test=40, seed=0)
    with emulated(), _bound(*patches):
        with (shadow(collect=collect) if shadowed else contextlib.nullcontext()) as S:
            tr = CNNNativeTrainer(name, data, torch.device("cpu"),
                                  TrainerConfig(batch_size=nb, eval_batch_size=16, augment=False, use_graph=False))
            tr.grads_for_batch(0, nb)
            tr.grads_for_batch(0, nb)
            if evaluate:
                tr.evaluate()
    return tr, S


@functools.lru_cache(maxsize=None)
def _transparent(name):
    return _engine_run(name, 8, True)


def _state(tr):
    st = {"grad": tr.fs.grad, "stats": tr.stats, "stats_all": tr.stats_all}
    st.update({"buf." + k: v for k, v in tr.model.named_buffers()})
    st.update({f"shift.{i}": u.shift for i, u in enumerate(tr.units)})
    return st


@pytest.mark.parametrize("name", ARCHS)
def test_shadow_is_transparent(name):
    tr, S = _transparent(name)
    assert not S.failures, S.failures[:5]
    # every comparison exactly zero (the mask_bn excluded share is a count of skipped elements, not an error)
    nonzero = {(op, sig, k): v for (op, sig), e in S.table.items() for k, v in e["worst"].items()
               if v != 0.0 and not k.endswith(":excluded_share")}
    assert not nonzero, list(nonzero.items())[:5]
    plain, _ = _engine_run(name, 8, False)
    a, b = _state(tr), _state(plain)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert tr.eval_stats() == plain.eval_stats() and tr.train_stats() == plain.train_stats()


# ---- sensitivity ---------------------------------------------------------------------------------------
def _standin(name, body):
    """``body(fn, A)`` with the emulated ``fn`` and the call's arguments by name, under the emulation's signature."""
    fn = getattr(emulate, name)
    sg = inspect.signature(fn)

    @functools.wraps(fn)
    def f(*a, **k):
        b = sg.bind(*a, **k)
        b.apply_defaults()
        return body(fn, dict(b.arguments))

    return f


def _fwd_stats_miss_border_row(fn, A):
    out = fn(**dict(A, stats=None))
    if A["stats"] is not None:
        emulate._stats_add(A["stats"], out[:, 1:], A["shift"])      # the first output row never reaches the sums
    return out


def _bn_apply_keeps_rvar(fn, A):
    rv = A["a"].rvar.clone()
    r = fn(**A)
    A["a"].rvar.copy_(rv)
    return r


def _dw_dgrad_wrong_phase(fn, A):
    out = fn(**A)
    if A["stride"] == 2:
        out.copy_(torch.roll(out, shifts=(1, 1), dims=(1, 2)))
    return out


def _maxpool2_bwd_last_maximum(fn, A):
    # post-ReLU windows of zeros hold equal maxima: the LAST one takes the gradient instead of the first
    dx = fn(A["x"].flip(1, 2), A["dy"].flip(1, 2)).flip(1, 2)
    return dx if A["out"] is None else A["out"].copy_(dx)


def _head_miscounts(fn, A):
    r = fn(**A)
    A["stats"].view(torch.int32)[1] += 3
    return r


SENSITIVITY = {
    "dgrad_ignores_accumulate": ("GoogLeNet", conv, "conv2d_dgrad", lambda fn, A: fn(**dict(A, accumulate=False)),
                                 "accumulate"),
    "fwd_drops_res": ("PreActResNet18", conv, "conv2d_fwd", lambda fn, A: fn(**dict(A, res=None)), "res"),
    "fwd_stats_miss_border_row": ("ResNet18", conv, "conv2d_fwd", _fwd_stats_miss_border_row, "stats"),
    "bn_apply_skips_running_var": ("ResNet18", cnn, "bn_apply", _bn_apply_keeps_rvar, "train=True"),
    "bn_bwd_drops_dadd": ("PreActResNet18", cnn, "bn_bwd", lambda fn, A: fn(**dict(A, dadd=None)), "dadd"),
    "wgrad_drops_last_image": ("ResNet18", conv, "conv2d_wgrad",
                               lambda fn, A: fn(**dict(A, x=A["x"][:-1], dy=A["dy"][:-1])), "x=2x"),
    "dw_dgrad_wrong_stride_phase": ("MobileNet", conv, "dwconv_dgrad", _dw_dgrad_wrong_phase, "stride=2"),
    "maxpool3_bwd_ignores_accumulate": ("GoogLeNet", cnn, "maxpool3_bwd",
                                        lambda fn, A: fn(**dict(A, accumulate=False)), "accumulate"),
    "maxpool2_bwd_last_maximum": ("VGG11", cnn, "maxpool2_bwd", _maxpool2_bwd_last_maximum, "x="),
    "head_miscounts_correct": ("ResNet18", cnn, "head", _head_miscounts, "train=True"),
}


@pytest.mark.parametrize("case", sorted(SENSITIVITY))
def test_shadow_catches_a_wrong_kernel(case):
    arch, mod, op, body, flag = SENSITIVITY[case]
    with pytest.raises(ShadowMismatch) as ei:
        _engine_run(arch, 2, True, patches=[(mod, op, _standin(op, body))], evaluate=False, collect=False)
    msg = str(ei.value)
    assert msg.startswith(op + " ["), msg          # names the op that is wrong, not a consumer of its output
    assert flag in msg, msg                        # ... at a call site that uses the broken feature


def test_collect_gathers_every_mismatch():
    _, S = _engine_run("PreActResNet18", 2, True, evaluate=False,
                       patches=[(conv, "conv2d_fwd", _standin("conv2d_fwd", lambda fn, A: fn(**dict(A, res=None))))])
    assert len(S.failures) > 4 and all(f.startswith("conv2d_fwd [") and "res" in f for f in S.failures), S.failures


# ---- deferred WGRAD reductions ---------------------------------------------------------------------------
def _deferring(name, wrong=False):
    """A WGRAD stand-in that defers like the native one: ``out`` stays unwritten until the reduce launch."""

    def body(fn, A):
        if A["deferred"] is None or A["out"] is None:
            return fn(**A)
        src = dict(A, out=None, deferred=None)
        if wrong:
            src.update(x=A["x"][:-1], dy=A["dy"][:-1])
        A["deferred"].append((A["out"], fn(**src), A["accumulate"]))
        return A["out"]

    return _standin(name, body)


def _reduce_deferred(items, device):
    for out, dw, acc in items:
        out.add_(dw) if acc else out.copy_(dw)


@functools.lru_cache(maxsize=None)
def _deferred_run():
    return _engine_run("MobileNet", 2, True, evaluate=False,
                       patches=[(conv, "conv2d_wgrad", _deferring("conv2d_wgrad")),
                                (conv, "dwconv_wgrad", _deferring("dwconv_wgrad")),
                                (conv, "wgrad_reduce_multi", _reduce_deferred)])


def test_deferred_wgrad_is_compared_after_the_reduction():
    tr, S = _deferred_run()
    assert not S.failures and not S._pending
    for op in ("conv2d_wgrad", "dwconv_wgrad"):
        sigs = S.signatures(op)
        assert sigs and all(s.endswith("+deferred") for s in sigs), sigs
    assert "wgrad_reduce_multi" in S.ops()
    plain, _ = _engine_run("MobileNet", 2, False, evaluate=False)
    assert torch.equal(tr.fs.grad, plain.fs.grad)


@pytest.mark.parametrize("op", ["conv2d_wgrad", "dwconv_wgrad"])
def test_deferred_wgrad_mismatch_is_caught(op):
    patches = [(conv, "conv2d_wgrad", _deferring("conv2d_wgrad", wrong=op == "conv2d_wgrad")),
               (conv, "dwconv_wgrad", _deferring("dwconv_wgrad", wrong=op == "dwconv_wgrad")),
               (conv, "wgrad_reduce_multi", _reduce_deferred)]
    with pytest.raises(ShadowMismatch) as ei:
        _engine_run("MobileNet", 2, True, patches=patches, evaluate=False, collect=False)
    assert str(ei.value).startswith(op + " [") and "+deferred" in str(ei.value)


# ---- coverage ----------------------------------------------------------------------------------------------
def test_every_wrapped_op_and_special_case_is_exercised():
    runs = [_transparent(n)[1] for n in ARCHS]
    ops = set().union(*(S.ops() for S in runs))
    # the emulated WGRAD reduces at once, so the engine never calls wgrad_reduce_multi under plain emulation:
    # the deferring stand-ins above cover it
    assert ops == set(ALL_OPS) - {"wgrad_reduce_multi"}, set(ALL_OPS) ^ ops
    assert "wgrad_reduce_multi" in _deferred_run()[1].ops()
    sigs = {op: " | ".join(s for S in runs for s in S.signatures(op)) for op in ALL_OPS}
    for op, flags in {"conv2d_fwd": ["stats", "shift", "res"],
                      "conv2d_dgrad": ["accumulate", "add", "bn_sums", "msc", "zb", "wd"],
                      "dwconv_fwd": ["stats", "shift"],
                      "bn_apply": ["/ld", "z2", "res", "co_out", "cbias", "train=False", "relu=False"],
                      "bn_bwd": ["/ld", "dyb", "zb", "gout", "dadd", "chained", "mask_bn", "presummed", "relu_y"],
                      "head": ["train=True", "train=False", "zero"],
                      "maxpool3": ["stride=1", "stride=2"],
                      "maxpool3_bwd": ["accumulate", "stride=2"]}.items():
        for f in flags:
            assert f in sigs[op], (op, f)
