"""Pose and Detector on the GPU, layer by layer, through
`_core.op_kernel_test` and the ops' `debug_tap`.

Every conv tap is compared with the float64 reference of that one layer fed
the GPU's *own* previous tap (dnn_models_ref.py), every live element of
both frames within dnn_ref.tolerance(ref, mag, K = r * s * in_c); pad
columns must be exactly +0, concats bit-equal, and the ops' real outputs
equal to the keypoint / post-process references applied to the final taps.
test_dnn_models_cpu.py shows that this comparator flags a wrong offset, relu
flag, concat order, weight block or dirty pad channel.

Inputs: two different 45 x 61 x 3 frames in one batch, weights from
generated files. A tap is fetched once per module and reused; the tap of
one layer per model is fetched twice and must be bit-equal, which is what
teacher forcing across calls rests on. Worst err/tol per layer is printed
(`pytest -rP`) and tabulated in docs/testing.md; no bound is tuned from it.
The `Net` helper and the checks live in dnn_models_net.py, shared with
test_resnet_layers_gpu.py.
"""
import numpy as np
import pytest

import dnn_models_ref as M
import scanner_amd as sp
from dnn_models_net import FRAMES, Net, check_conv, check_pre
from scanner_amd import _core
from scanner_amd.models import detector, pose

pytestmark = pytest.mark.gpu

IH, IW = FRAMES.shape[1:3]

# The detector head whose float64 post-process keeps a few dozen boxes with
# every decision >= 1e-3 from its threshold: cls.bias of seed DET_SEED
# lowered by DET_BIAS_DROP. Chosen on an MI355X from the reference's
# margins alone, among drops of 2.0 .. 3.25 on seeds 21 .. 24: the reference
# has 33 + 7 candidates on the two frames and keeps 12 + 7 boxes, smallest
# margin 1.9e-3 / 1.5e-3 (|score - 0.5|; |IoU - 0.5| >= 5.3e-3, extent
# >= 2.07). About one choice in six clears 1e-3: 12 800 bf16 logits have
# to stay 0.004 away from 0.
DET_SEED = 21
DET_BIAS_DROP = 2.90


def keypoints_of(rows):
    return np.stack([np.frombuffer(r, np.float32).reshape(19, 3)
                     for r in rows])


# ---- Pose, stages = 3 ----

POSE_NODES = M.pose_nodes(3)


@pytest.fixture(scope="module")
def pose3(tmp_path_factory):
    return Net("Pose", POSE_NODES, pose.conv_specs(3),
               pose.generate_weights(seed=31, stages=3),
               tmp_path_factory.mktemp("pose3") / "w.bin", stages=3)


def test_pose_pre(pose3):
    check_pre(pose3, pose.IN_HW)


@pytest.mark.parametrize("name",
                         [n[0] for n in POSE_NODES if n[1] == "conv"])
def test_pose_layer(pose3, name):
    check_conv(pose3, name)


@pytest.mark.parametrize("t", [2, 3])
def test_pose_concat(pose3, t):
    got = pose3.tap(f"cat{t}")
    want = M.cat_ref(pose3.tap("b8"), pose3.tap(f"s{t - 1}L_5"),
                     pose3.tap(f"s{t - 1}S_5"))
    assert got.shape == want.shape == (2, 46, 46, 192)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_pose_keypoints_are_the_argmax_of_the_last_stage(pose3):
    got = keypoints_of(pose3.output())
    assert np.array_equal(got, M.keypoints_ref(pose3.tap("s3S_5")))
    # not those of stage 2
    assert not np.array_equal(got, M.keypoints_ref(pose3.tap("s2S_5")))


def test_pose_tap_is_repeatable(pose3):
    a = pose3.tap("s2L_3")
    assert np.array_equal(a.view(np.uint32),
                          pose3.fetch("s2L_3").view(np.uint32))


def test_pose_single_stage(tmp_path):
    net = Net("Pose", M.pose_nodes(1), pose.conv_specs(1),
              pose.generate_weights(seed=32, stages=1), tmp_path / "w.bin",
              stages=1)
    check_conv(net, "s1S_5")
    assert np.array_equal(keypoints_of(net.output()),
                          M.keypoints_ref(net.tap("s1S_5")))
    with pytest.raises(Exception, match="unknown debug_tap 'cat2'"):
        net.fetch("cat2")   # no second stage here
    with pytest.raises(Exception, match="unknown debug_tap 's2S_5'"):
        net.fetch("s2S_5")


def test_pose_three_channel_b1_weight(tmp_path):
    ts = pose.generate_weights(seed=33, stages=3, b1_channels=3)
    assert ts["b1.weight"].shape == (64, 3, 3, 3)
    net = Net("Pose", POSE_NODES, pose.conv_specs(3), ts, tmp_path / "w.bin",
              stages=3)
    check_conv(net, "b1")


def test_unknown_tap_is_rejected_by_name(pose3, det):
    for net in (pose3, det):
        with pytest.raises(Exception, match="unknown debug_tap 'b9'"):
            net.run(debug_tap="b9")


# ---- Detector ----

DET_NODES = M.detector_nodes()


@pytest.fixture(scope="module")
def det(tmp_path_factory):
    return Net("Detector", DET_NODES, detector.conv_specs(),
               detector.generate_weights(seed=DET_SEED),
               tmp_path_factory.mktemp("det") / "w.bin")


def head_maps(net, f):
    return (net.tap("loc")[f].reshape(1600, 64),
            net.tap("cls")[f].reshape(1600, 64))


def test_detector_pre(det):
    check_pre(det, detector.IN_HW)


@pytest.mark.parametrize("name",
                         [n[0] for n in DET_NODES if n[1] == "conv"])
def test_detector_layer(det, name):
    check_conv(det, name)


def test_detector_tap_is_repeatable(det):
    a = det.tap("head")
    assert np.array_equal(a.view(np.uint32),
                          det.fetch("head").view(np.uint32))


def test_detector_output_is_the_postprocess_of_its_taps(det):
    blobs = det.output()
    assert len(blobs) == 2
    for f in range(2):
        loc, cls = head_maps(det, f)
        assert blobs[f] == _core.detector_postprocess(loc, cls, IH, IW), f
    assert blobs[0] != blobs[1]


def test_detector_boxes_match_the_float64_postprocess(tmp_path):
    ts = detector.generate_weights(seed=DET_SEED)
    ts["cls.bias"] = (ts["cls.bias"] - np.float32(DET_BIAS_DROP)).astype(
        np.float32)
    net = Net("Detector", DET_NODES, detector.conv_specs(), ts,
              tmp_path / "w.bin")
    check_conv(net, "cls")
    blobs = net.output()
    total = 0
    for f in range(2):
        loc, cls = head_maps(net, f)
        kept, m = M.detector_post_ref(loc, cls, IH, IW)
        cand = M.detector_post_ref(loc, cls, IH, IW, nms=False)[0]
        print(f"frame {f}: the reference has {len(cand)} candidates and "
              f"keeps {len(kept)} boxes, margins {m}")
        assert m["min"] >= 1e-3, \
            f"frame {f}: the reference's own decisions are marginal ({m}); " \
            f"another DET_SEED / DET_BIAS_DROP is needed"
        assert m["order"] >= 2.0 ** -20, (f, m)
        M.assert_boxes_match(blobs[f], kept, f"frame {f}")
        assert blobs[f] == _core.detector_postprocess(loc, cls, IH, IW)
        assert len(kept) > 0, f"frame {f}: nothing to compare"
        total += len(cand)
    assert 24 <= total <= 120, \
        f"the reference has {total} candidates, not a few dozen"


# ---- default weights, no file ----

def test_pose_default_weights():
    net = Net("Pose", POSE_NODES, pose.conv_specs(3), None, None)
    got = keypoints_of(net.output())
    assert np.array_equal(got, M.keypoints_ref(net.tap("s3S_5")))
    assert net.run() == net.output()


def test_detector_default_weights():
    net = Net("Detector", DET_NODES, detector.conv_specs(), None, None)
    blobs = net.output()
    for f in range(2):
        loc, cls = head_maps(net, f)
        assert blobs[f] == _core.detector_postprocess(loc, cls, IH, IW), f
    assert net.run() == blobs


# ---- mixed frame geometries are rejected before any launch ----

@pytest.mark.parametrize("op", ["Pose", "ResNet50"])
def test_mixed_frame_geometries_are_rejected(sc, tmp_path, op):
    """Files -> ImageDecoder hands on a batch whose rows alternate between
    two shapes; both ops size their reads by frame 0 alone."""
    from test_image_decode_cpu import write_files
    from test_image_decode_gpu import case_file
    blobs = [case_file("17x33_420" if s % 2 else "40x56_420_rst1", "noise",
                       75, s) for s in range(6)]
    col = sc.sources.Files(write_files(tmp_path, blobs))
    frames = sc.ops.ImageDecoder(img=col, device=sp.DeviceType.GPU)
    res = getattr(sc.ops, op)(frame=frames, device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, f"mixed_{op}")
    with pytest.raises(Exception,
                       match=f"{op} batch has mixed frame geometries"):
        sc.run(sc.io.Output(res, [out]), sp.PerfParams.manual(6, 6),
               cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
