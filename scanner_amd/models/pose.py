"""Pose model family support: the conv topology restated in Python and
weight generation for the numerics tests (tests/test_dnn_models_*.py compare
the engine layer by layer against float64 references built from these).

Layer naming and the [out][r][s][in] (OHWI) weight layout mirror
csrc/ops/pose.cpp; BN is pre-folded into per-channel scale/bias.

Topology (input 368 x 368, feature stride 8):
  backbone b1..b8, 3x3 pad 1, stride 2 at b2/b4/b6 -> F: 46 x 46 x 128
  stage t, branch L (38 PAF channels) and S (19 heatmap channels):
    _1.._3 3x3 -> 128, _4 1x1 -> 512 (t = 1) or 128, _5 1x1 -> out, no relu
  stage t >= 2 reads concat(F[128], L[38], S[19]) padded with 7 zero
  channels to 192; b1 reads RGB padded with 5 zero channels to 8.
"""
import numpy as np

from .resnet50 import write_tensor_file  # noqa: F401  (re-exported)

PAF_C = 38
HEAT_C = 19
IN_HW = 368
FEAT_HW = 46
CAT_LIVE = 128 + PAF_C + HEAT_C  # 185 of the 192 concat channels


def conv_spec(name, in_c, out_c, k, stride, relu):
    return dict(name=name, in_c=in_c, out_c=out_c, r=k, s=k, stride=stride,
                pad=k // 2, relu=relu)


def conv_specs(stages=3):
    """The convs in engine order; in_c is what the engine's conv consumes
    (zero-padded channels included)."""
    specs = [conv_spec("b1", 8, 64, 3, 1, True),
             conv_spec("b2", 64, 64, 3, 2, True),
             conv_spec("b3", 64, 128, 3, 1, True),
             conv_spec("b4", 128, 128, 3, 2, True),
             conv_spec("b5", 128, 256, 3, 1, True),
             conv_spec("b6", 256, 256, 3, 2, True),
             conv_spec("b7", 256, 256, 3, 1, True),
             conv_spec("b8", 256, 128, 3, 1, True)]
    for t in range(1, stages + 1):
        for br, out_c in (("L", PAF_C), ("S", HEAT_C)):
            p = f"s{t}{br}"
            mid = 512 if t == 1 else 128
            in_c = 128 if t == 1 else 192
            specs += [conv_spec(f"{p}_1", in_c, 128, 3, 1, True),
                      conv_spec(f"{p}_2", 128, 128, 3, 1, True),
                      conv_spec(f"{p}_3", 128, 128, 3, 1, True),
                      conv_spec(f"{p}_4", 128, mid, 1, 1, True),
                      conv_spec(f"{p}_5", mid, out_c, 1, 1, False)]
    return specs


def generate_tensors(specs, seed, b1_channels=8):
    """He-normal OHWI weights, scale ~ U(0.7, 1.3), bias ~ N(0, 0.05) for
    every conv of `specs`: a complete file, nothing left to the engine's own
    fallback initialisation. The weights that meet zero-padded input
    channels (b1 channels 3..7, stage >= 2 `_1` channels 185..191) are
    non-zero like the rest, so the engine's zero lanes are load-bearing.
    b1_channels=3 gives the natural 64 x 3 x 3 x 3 b1.weight that the engine
    expands on load."""
    assert b1_channels in (3, 8)
    rng = np.random.RandomState(seed)
    ts = {}
    for sp in specs:
        fan_in = sp["in_c"] * sp["r"] * sp["s"]
        w = rng.normal(0, np.sqrt(2.0 / fan_in),
                       size=(sp["out_c"], sp["r"], sp["s"], sp["in_c"]))
        if sp["name"] == "b1" and b1_channels == 3:
            w = w[..., :3]
        ts[sp["name"] + ".weight"] = np.ascontiguousarray(w, np.float32)
        ts[sp["name"] + ".scale"] = rng.uniform(
            0.7, 1.3, sp["out_c"]).astype(np.float32)
        ts[sp["name"] + ".bias"] = rng.normal(
            0, 0.05, sp["out_c"]).astype(np.float32)
    return ts


def generate_weights(seed=0, stages=3, b1_channels=8):
    return generate_tensors(conv_specs(stages), seed, b1_channels)
