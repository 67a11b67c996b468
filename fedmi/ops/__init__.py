"""Torch-facing wrappers over fedmi's hand-written HIP/CDNA4 kernels.

* :mod:`fedmi.ops.conv` — implicit-GEMM MFMA convolution fwd / dgrad / wgrad (NHWC bf16), depthwise
* :mod:`fedmi.ops.cnn`  — BatchNorm (+ReLU, +residual) fwd/bwd, classifier head + CE, input prep, pooling
* :mod:`fedmi.ops.native_mode` — the aten backend (TorchDispatchMode) for the zoo families without a
  whole-network engine: the op table, the conv routing and the mode.  It builds on
  :mod:`fedmi.ops.zoo_launch` (descriptors, launch planner, ``ew`` / ``fill_`` / ``reduce_sum``, op codes) and
  :mod:`fedmi.ops.zoo_fusion` (results whose pass is pending: the peephole fusions' join conditions)

Every wrapper launches on torch's current stream (graph-capturable) and raises
if the native extension is missing: there is no silent PyTorch fallback.
"""
from . import cnn, conv  # noqa: F401
