"""CPU half of the layer-by-layer Pose / Detector tests: the Python
restatement of the two topologies against the engine's own ConvSpec lists,
the float64 references of dnn_models_ref.py run as a network of their own,
and the per-layer comparator against bugs seeded into the reference.

The comparator is the one the GPU tests use (dnn_ref.tolerance with K =
r * s * in_c, every element). A mutation counts as caught when at least 10 %
of the elements it changes are flagged, the rule of dnn_ref.mutation_rates;
the measured rates are tabulated in docs/testing.md.
"""
import numpy as np
import pytest

import dnn_models_ref as M
import dnn_ref as R
from scanner_amd import _core
from scanner_amd.models import detector, pose

SPEC_KEYS = ("name", "in_c", "out_c", "r", "s", "stride", "pad", "relu")


def _pad64(v):
    return -(-v // 64) * 64


def _check_parity(py_specs, model):
    cc = _core.dnn_model_specs(model)
    assert [{k: d[k] for k in SPEC_KEYS} for d in cc] == py_specs
    w_off = sb_off = 0
    for d in cc:
        assert d["kp"] == _pad64(d["r"] * d["s"] * d["in_c"]), d["name"]
        assert d["np"] == _pad64(d["out_c"]), d["name"]
        assert (d["w_off"], d["sb_off"]) == (w_off, sb_off), d["name"]
        w_off += d["np"] * d["kp"]
        sb_off += 2 * d["np"]


@pytest.mark.parametrize("stages", [1, 3, 6])
def test_pose_spec_parity(stages):
    _check_parity(pose.conv_specs(stages), f"pose{stages}")


def test_detector_spec_parity():
    _check_parity(detector.conv_specs(), "detector")


def test_unknown_model_rejected_by_name():
    for name in ("pose0", "pose7", "pose", "resnet", "resnet500", ""):
        with pytest.raises(Exception, match="unknown model"):
            _core.dnn_model_specs(name)


@pytest.mark.parametrize("model", ["pose", "detector"])
def test_generated_tensor_shapes(model):
    mod = pose if model == "pose" else detector
    specs = mod.conv_specs()
    ts = mod.generate_weights(seed=1)
    assert set(ts) == {s["name"] + suffix for s in specs
                       for suffix in (".weight", ".scale", ".bias")}
    for s in specs:
        n = s["name"]
        assert ts[n + ".weight"].shape == (s["out_c"], s["r"], s["s"],
                                           s["in_c"])
        assert ts[n + ".scale"].shape == ts[n + ".bias"].shape \
            == (s["out_c"],)
        assert all(ts[n + k].dtype == np.float32
                   for k in (".weight", ".scale", ".bias"))
        assert 0.7 <= ts[n + ".scale"].min() and ts[n + ".scale"].max() <= 1.3
    # the weights that meet the engine's zero-padded channels are non-zero
    assert np.all(ts["b1.weight"][..., 3:] != 0)
    if model == "pose":
        for t in (2, 3):
            for br in "LS":
                assert np.all(ts[f"s{t}{br}_1.weight"][..., 185:] != 0)
    w3 = mod.generate_weights(seed=1, b1_channels=3)["b1.weight"]
    assert w3.shape == (64, 3, 3, 3)
    assert np.array_equal(w3, ts["b1.weight"][..., :3])


# ---- the references as a network ----

@pytest.fixture(scope="module")
def frame():
    return M.frames_45x61()[1:]  # the noise frame


@pytest.fixture(scope="module")
def pose_run(frame):
    specs = pose.conv_specs(2)
    ts = pose.generate_weights(seed=11, stages=2)
    nodes = M.pose_nodes(2)
    return nodes, specs, ts, M.emulate(nodes, specs, ts, frame, pose.IN_HW)


@pytest.fixture(scope="module")
def det_run(frame):
    specs = detector.conv_specs()
    ts = detector.generate_weights(seed=12)
    nodes = M.detector_nodes()
    return nodes, specs, ts, M.emulate(nodes, specs, ts, frame,
                                       detector.IN_HW)


def test_pose_reference_shapes(pose_run):
    nodes, specs, _, taps = pose_run
    hw = {"pre": 368, "b1": 368, "b2": 184, "b3": 184, "b4": 92, "b5": 92,
          "b6": 46}
    ch = {s["name"]: s["out_c"] for s in specs}
    ch.update(pre=8, cat2=192)
    assert [n[0] for n in nodes] == list(taps)
    assert set(taps) == set(ch)
    for name, x in taps.items():
        side = hw.get(name, 46)
        assert x.shape == (1, side, side, ch[name]), name
        assert np.isfinite(x).all()
    assert taps["s1L_4"].shape[3] == 512 and taps["s2L_4"].shape[3] == 128
    assert taps["s2L_5"].shape[3] == 38 and taps["s2S_5"].shape[3] == 19
    assert not taps["cat2"][..., 185:].any()
    assert M.keypoints_ref(taps["s2S_5"]).shape == (1, 19, 3)


def test_detector_reference_shapes(det_run):
    _, specs, _, taps = det_run
    hw = {"pre": 320, "b1": 320, "b2": 160, "b3": 160, "b4": 80, "b5": 80}
    ch = {s["name"]: s["out_c"] for s in specs}
    ch["pre"] = 8
    assert set(taps) == set(ch)
    for name, x in taps.items():
        side = hw.get(name, 40)
        assert x.shape == (1, side, side, ch[name]), name
    assert ch["loc"] == 16 and ch["cls"] == 32


# ---- the comparator: passes the emulation, flags seeded bugs ----

def _layer(run, name):
    nodes, spec_list, ts, taps = run
    specs = {s["name"]: s for s in spec_list}
    node = next(n for n in nodes if n[0] == name)
    return specs, ts, taps, node, M.source_of(node, taps, specs)


@pytest.mark.parametrize("model", ["pose", "detector"])
def test_comparator_passes_the_emulation(model, pose_run, det_run):
    run = pose_run if model == "pose" else det_run
    nodes = run[0]
    for node in nodes:
        if node[1] != "conv":
            continue
        specs, ts, taps, _, x = _layer(run, node[0])
        sp = specs[node[0]]
        ref, mag = M.layer_ref(sp, x, ts)
        worst = R.assert_within(taps[node[0]], ref,
                                M.layer_tolerance(sp, ref, mag),
                                f"{model} {node[0]}")
        assert worst < 1.0
        print(f"emulation err/tol {model} {node[0]}: {worst:.3f}")


def _rate(spec, ref, mag, mutated, what):
    """Fraction of the elements the mutation changes that the comparator
    flags."""
    affected = mutated != ref
    assert affected.any(), f"mutation {what} changed nothing"
    flagged = R.err_over_tol(mutated, ref,
                             M.layer_tolerance(spec, ref, mag)) > 1.0
    rate = float((flagged & affected).sum() / affected.sum())
    print(f"mutation {what}: {rate:.1%} of {int(affected.sum())} changed "
          f"elements flagged")
    assert rate >= 0.10, f"comparator flags only {rate:.1%} of {what}"
    return rate


def _mutation(run, name, what, x=None, **kw):
    specs, ts, _, _, x0 = _layer(run, name)
    sp = specs[name]
    ref, mag = M.layer_ref(sp, x0, ts)
    mutated, _ = M.layer_ref(sp, x0 if x is None else x, ts, **kw)
    return _rate(sp, ref, mag, mutated, f"{what} at {name}")


def test_mutation_relu_on_final_layers(pose_run, det_run):
    _mutation(pose_run, "s2S_5", "relu", relu=True)
    _mutation(det_run, "cls", "relu", relu=True)


@pytest.mark.parametrize("model,name,nxt", [("pose", "b1", "b2"),
                                            ("pose", "s2L_1", "s2L_2"),
                                            ("detector", "head", "loc")])
def test_mutation_scale_bias_of_following_conv(model, name, nxt, pose_run,
                                               det_run):
    """What a wrong sb_off does: the next conv's scale/bias block, as far
    as it reaches (loc has 16 channels; the rest of its padded block is
    zero)."""
    run = pose_run if model == "pose" else det_run
    specs, ts, _, _, _ = _layer(run, name)
    out_c = specs[name]["out_c"]
    pad = np.zeros(out_c, np.float32)
    scale = np.concatenate([ts[nxt + ".scale"], pad])[:out_c]
    bias = np.concatenate([ts[nxt + ".bias"], pad])[:out_c]
    _mutation(run, name, f"scale/bias of {nxt}", scale=scale, bias=bias)


def test_mutation_concat_order(pose_run):
    _, _, _, taps = pose_run
    good = taps["cat2"]
    bad = M.cat_ref(taps["b8"], np.concatenate(
        [taps["s1S_5"], taps["s1L_5"]], axis=3), taps["s1L_5"][..., 19:])
    # F | S | L: the 57 branch channels in the other order
    assert np.array_equal(bad[..., 128:147], taps["s1S_5"])
    assert np.array_equal(bad[..., 147:185], taps["s1L_5"])
    changed = bad != good
    assert changed.any() and not changed[..., :128].any()
    # cat is compared bit for bit, so every changed element is flagged; the
    # conv that reads it must notice as well
    for name in ("s2L_1", "s2S_1"):
        _mutation(pose_run, name, "concat order F, S, L", x=bad)


def test_mutation_other_branch_weights(pose_run):
    specs, ts, _, _, _ = _layer(pose_run, "s2L_1")
    _mutation(pose_run, "s2L_1", "weights of s2S_1",
              weight=M.weight_ohwi(specs["s2S_1"], ts))


def test_mutation_garbage_in_concat_pad_channels(pose_run):
    bad = pose_run[3]["cat2"].copy()
    bad[..., 185:] = 1.0
    for name in ("s2L_1", "s2S_1"):
        _mutation(pose_run, name, "cat2 channels 185..191 = 1", x=bad)


@pytest.mark.parametrize("model", ["pose", "detector"])
def test_mutation_garbage_in_pre_pad_channels(model, pose_run, det_run):
    run = pose_run if model == "pose" else det_run
    bad = run[3]["pre"].copy()
    bad[..., 3:] = 1.0
    _mutation(run, "b1", f"{model} pre channels 3..7 = 1", x=bad)


def test_mutation_b1_expansion_transposed(pose_run):
    """A 64 x 3 x 3 x 3 b1.weight read as [o][c][r*s] instead of
    [o][r*s][c] when it is expanded to 8 input channels."""
    specs, ts, _, _, x = _layer(pose_run, "b1")
    w3 = np.ascontiguousarray(ts["b1.weight"][..., :3])
    ts3 = dict(ts, **{"b1.weight": w3})
    sp = specs["b1"]
    ref, mag = M.layer_ref(sp, x, ts3)
    bad3 = w3.reshape(64, 3, 9).transpose(0, 2, 1).reshape(64, 3, 3, 3)
    assert not np.array_equal(bad3, w3)
    bad = M.weight_ohwi(sp, {"b1.weight": bad3})
    mutated, _ = M.layer_ref(sp, x, ts3, weight=bad)
    _rate(sp, ref, mag, mutated, "b1 expansion read as [o][c][r*s]")
