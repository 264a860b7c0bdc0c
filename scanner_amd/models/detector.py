"""Detector model family support: the conv topology restated in Python and
weight generation for the numerics tests (tests/test_dnn_models_*.py).

Layer naming and the [out][r][s][in] (OHWI) weight layout mirror
csrc/ops/detector.cpp; BN is pre-folded into per-channel scale/bias.

Topology (input 320 x 320, feature stride 8): b1..b6 3x3 pad 1 with stride
2 at b2/b4/b6 -> 40 x 40 x 128; head 3x3 -> 128; loc (4 anchors x 4 deltas)
and cls (4 anchors x 8 classes), both 3x3 on `head`, no relu.
"""
from .pose import conv_spec, generate_tensors
from .resnet50 import write_tensor_file  # noqa: F401  (re-exported)

IN_HW = 320
FEAT_HW = 40
ANCHORS = (16.0, 32.0, 64.0, 128.0)
CLASSES = 8


def conv_specs():
    return [conv_spec("b1", 8, 64, 3, 1, True),
            conv_spec("b2", 64, 64, 3, 2, True),
            conv_spec("b3", 64, 128, 3, 1, True),
            conv_spec("b4", 128, 128, 3, 2, True),
            conv_spec("b5", 128, 128, 3, 1, True),
            conv_spec("b6", 128, 128, 3, 2, True),
            conv_spec("head", 128, 128, 3, 1, True),
            conv_spec("loc", 128, len(ANCHORS) * 4, 3, 1, False),
            conv_spec("cls", 128, len(ANCHORS) * CLASSES, 3, 1, False)]


def generate_weights(seed=0, b1_channels=8):
    """See models.pose.generate_tensors."""
    return generate_tensors(conv_specs(), seed, b1_channels)
