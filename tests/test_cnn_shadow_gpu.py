"""Every kernel launch the native CNN engine issues, against the fp32 emulation of the same op on the same
inputs (tests/shadow.py): eight architectures at the batch sizes where path selection differs.

* nb=8: the deep layers' M (= N*H*W) is below one MFMA tile;
* nb=80: the ragged last batch of a 50000-sample epoch at batch 128;
* nb=128: the production batch (path selection reads N*H*W).

Each case runs two training passes (the second with shifted BN statistics), a third with augmentation and a
non-zero round counter, and an evaluation in batches of 16 / 16 / 8, all under ``shadow()``: no comparison may
fail, the engine's results must be bit-identical to the same engine without the shadow, and the set of ops
exercised must be what the architecture implies.  Errors are per op, so nothing compounds through the network
and the tolerances are the per-kernel tests' (see tests/shadow.py).

FEDMI_SHADOW_REPORT=<dir>: each case also dumps its table there (``python tests/shadow.py <dir>`` renders
profiles/tests_shadow/README.md from them).  FEDMI_SHADOW_REF=cpu computes the references on the host.
"""
import contextlib
import functools
import json
import os
import time
from pathlib import Path

import pytest
import torch

from fedmi.engine.base import TrainerConfig
from fedmi.engine.data import make_dataset
from fedmi.models import build_model
from shadow import shadow

pytestmark = pytest.mark.gpu

ARCHS = ["ResNet18", "ResNet50", "MobileNet", "MobileNetV2", "VGG11", "PreActResNet18", "PreActResNet50", "GoogLeNet"]
COMMON = {"prep_input", "conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad", "wgrad_reduce_multi", "bn_apply", "bn_bwd", "head"}
DEPTHWISE = {"dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad"}
EXTRA = {"MobileNet": DEPTHWISE, "MobileNetV2": DEPTHWISE, "GoogLeNet": {"maxpool3", "maxpool3_bwd"},
         "VGG11": {"maxpool2", "maxpool2_bwd"}}


def _run(name, nb, dev, init, data, shadowed):
    from fedmi.engine.cnn_native import CNNNativeTrainer

    tr = CNNNativeTrainer(name, data, dev, TrainerConfig(batch_size=nb, eval_batch_size=16, augment=False,
                                                         use_graph=False), init_state=init)
    ref = os.environ.get("FEDMI_SHADOW_REF") or None
    with (shadow(collect=True, ref_device=ref) if shadowed else contextlib.nullcontext()) as S:
        tr.grads_for_batch(0, nb)
        tr.grads_for_batch(0, nb)            # statistics shifted by the first pass's batch means
        tr.augment = True                    # crop / flip in prep_input, keyed by a non-zero round counter
        tr.round_ctr[0] = 3
        tr.grads_for_batch(256 - nb, nb)
        tr.evaluate()                        # 16 / 16 / 8: the eval branches of bn_apply and head
        torch.cuda.synchronize(dev)
    return tr, S


def _state(tr):
    st = {"grad": tr.fs.grad, "stats": tr.stats, "stats_all": tr.stats_all}
    st.update({"buf." + k: v for k, v in tr.model.named_buffers()})
    st.update({f"shift.{i}": u.shift for i, u in enumerate(tr.units)})
    return st


@pytest.mark.parametrize("nb", [8, 80, 128])
@pytest.mark.parametrize("name", ARCHS)
def test_every_engine_launch_matches_emulation(gpu_device, name, nb):
    t0 = time.perf_counter()
    torch.manual_seed(0)
    init = build_model(name).state_dict()
    data = make_dataset("synthetic-cifar10", device=gpu_device, n_train=256, n_test=40, seed=0)
    tr, S = _run(name, nb, gpu_device, init, data, True)
    plain, _ = _run(name, nb, gpu_device, init, data, False)
    seconds = time.perf_counter() - t0
    out = os.environ.get("FEDMI_SHADOW_REPORT")
    if out:
        Path(out).mkdir(parents=True, exist_ok=True)
        (Path(out) / f"{name}_{nb:03d}.json").write_text(json.dumps(
            {"arch": name, "nb": nb, "seconds": seconds, "failures": S.failures, "table": S.dump()}))
    assert not S.failures, (len(S.failures), S.failures[:8])
    a, b = _state(tr), _state(plain)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert tr.eval_stats() == plain.eval_stats() and tr.train_stats() == plain.train_stats()
    assert S.ops() == COMMON | EXTRA.get(name, set()), S.ops() ^ (COMMON | EXTRA.get(name, set()))
    assert tr.eval_stats().count == 40 and tr.train_stats().count == 3 * nb


def test_shadow_fails_on_a_wrong_native_launch(gpu_device, monkeypatch):
    """The harness can fail on the GPU too: a forward whose last image never lands is named, with its signature
    (the CPU file holds the full sensitivity set)."""
    from fedmi.engine.cnn_native import CNNNativeTrainer
    from fedmi.ops import conv
    from shadow import ShadowMismatch

    native = conv.conv2d_fwd

    @functools.wraps(native)
    def fwd_loses_last_image(*a, **k):
        out = native(*a, **k)
        out[-1].zero_()
        return out

    monkeypatch.setattr(conv, "conv2d_fwd", fwd_loses_last_image)
    data = make_dataset("synthetic-cifar10", device=gpu_device, n_train=256, n_test=40, seed=0)
    tr = CNNNativeTrainer("ResNet18", data, gpu_device, TrainerConfig(batch_size=8, eval_batch_size=16, augment=False,
                                                                      use_graph=False))
    with pytest.raises(ShadowMismatch, match=r"^conv2d_fwd \[x=8x32x32x8 .*\] (out|stats): "):
        with shadow():
            tr.grads_for_batch(0, 8)
