"""CPU half of the layer-by-layer ResNet-50 tests: the Python restatement
of the topology against the engine's own ConvSpec list, the float64
references of dnn_models_ref.py run as a network of their own, the per-layer
comparator against bugs seeded into the reference, and the dispatch plans of
the layers at the two batch sizes test_resnet_layers_gpu.py runs.

The comparator is the one the GPU tests use (dnn_ref.tolerance with K =
r * s * in_c, |residual| in mag, every element). A mutation counts as caught
when at least 10 % of the elements it changes are flagged, the rule of
dnn_ref.mutation_rates; the measured rates are tabulated in docs/testing.md.

The emulation walks pre .. block3 on one 45 x 61 frame: that stretch has
both kinds of downsample (stride 1 and 2), both kinds of identity
(downsample tap, previous block) and a stride-2 conv2.
"""
import numpy as np
import pytest

import dnn_models_ref as M
import dnn_ref as R
from scanner_amd import _core
from scanner_amd.models import resnet50
from test_dnn_models_cpu import _check_parity, _rate

NODES = M.resnet_nodes()
SPECS = {s["name"]: s for s in resnet50.layer_specs()}
LAST = "block3.conv3"


def _node(name):
    return next(n for n in NODES if n[0] == name)


# ---- specs, nodes, weights ----

def test_spec_parity():
    _check_parity(resnet50.layer_specs(), "resnet50")
    # the tuple form the older tests use says the same, conv1's in_c apart
    for t, d in zip(resnet50.conv_specs(), resnet50.layer_specs()):
        assert t == (d["name"], 3 if d["name"] == "conv1" else d["in_c"],
                     d["out_c"], d["r"], d["stride"], d["pad"], d["relu"])
        assert d["r"] == d["s"]
    assert SPECS["conv1"]["in_c"] == 8


def test_node_list_covers_every_spec_once():
    convs = [n[0] for n in NODES if n[1] == "conv"]
    assert sorted(convs) == sorted(SPECS) and len(convs) == 54
    assert len({n[0] for n in NODES}) == len(NODES)
    assert [n[1] for n in NODES if n[1] != "conv"] == \
        ["pre", "maxpool", "avgpool"]
    seen = set()
    for node in NODES:
        name, kind, srcs = node
        assert all(s in seen for s in srcs), f"{name} reads a later tap"
        seen.add(name)
        if kind != "conv":
            continue
        sp = SPECS[name]
        assert M.live_channels(_node(srcs[0]), SPECS) == sp["in_c"], name
        assert len(srcs) == (2 if name.endswith(".conv3") else 1), name
        if len(srcs) == 2:
            assert M.live_channels(_node(srcs[1]), SPECS) == sp["out_c"], name
    # identities: the block's downsample where it has one, else the previous
    # block's output, maxpool never (block 0 has a downsample)
    ident = {n[0]: n[2][1] for n in NODES if len(n[2]) == 2}
    for b in range(16):
        want = f"block{b}.downsample" if b in (0, 3, 7, 13) \
            else f"block{b - 1}.conv3"
        assert ident[f"block{b}.conv3"] == want
        assert (f"block{b}.downsample" in SPECS) == (b in (0, 3, 7, 13))
    sides = M.resnet_tap_sides()
    assert [sides[k] for k in ("pre", "conv1", "maxpool", "block2.conv3",
                               "block3.conv1", "block3.conv2",
                               "block3.downsample", "block7.conv2",
                               "block13.conv1", "block13.downsample",
                               "block15.conv3", "avgpool", "fc")] == \
        [224, 112, 56, 56, 56, 28, 28, 14, 14, 7, 7, 1, 1]


def test_generated_tensor_shapes():
    ts = resnet50.generate_layer_weights(seed=1)
    assert set(ts) == {n + suffix for n in SPECS
                       for suffix in (".weight", ".scale", ".bias")}
    for n, s in SPECS.items():
        assert ts[n + ".weight"].shape == (s["out_c"], s["r"], s["s"],
                                           s["in_c"])
        assert ts[n + ".scale"].shape == ts[n + ".bias"].shape \
            == (s["out_c"],)
        assert all(ts[n + k].dtype == np.float32
                   for k in (".weight", ".scale", ".bias"))
        assert 0.7 <= ts[n + ".scale"].min() and ts[n + ".scale"].max() <= 1.3
    # the weights that meet the engine's zero-padded channels are non-zero
    assert np.all(ts["conv1.weight"][..., 3:] != 0)
    w3 = resnet50.generate_layer_weights(seed=1, conv1_channels=3)
    assert w3["conv1.weight"].shape == (64, 7, 7, 3)
    assert np.array_equal(w3["conv1.weight"], ts["conv1.weight"][..., :3])
    assert all(np.array_equal(w3[k], ts[k]) for k in ts
               if k != "conv1.weight")


# ---- the reference as a network ----

@pytest.fixture(scope="module")
def frame():
    return M.frames_45x61()[1:]  # the noise frame


@pytest.fixture(scope="module")
def run(frame):
    ts = resnet50.generate_layer_weights(seed=41)
    taps = M.emulate(NODES, resnet50.layer_specs(), ts, frame,
                     resnet50.IN_HW, last=LAST)
    return ts, taps


def test_reference_shapes(run):
    _, taps = run
    stretch = [n for n in NODES[:[n[0] for n in NODES].index(LAST) + 1]]
    assert list(taps) == [n[0] for n in stretch]
    sides = M.resnet_tap_sides()
    for node in stretch:
        x = taps[node[0]]
        assert x.shape == (1, sides[node[0]], sides[node[0]],
                           M.live_channels(node, SPECS)), node[0]
        assert np.isfinite(x).all()
        assert np.array_equal(R.bf16_round(x), x)
    assert taps["block3.conv2"].shape == (1, 28, 28, 128)
    assert taps["block3.conv1"].shape == (1, 56, 56, 128)
    assert not taps["pre"][..., 3:].any()


def _operands(run, name):
    ts, taps = run
    node = _node(name)
    return (SPECS[name], ts, M.source_of(node, taps, SPECS),
            M.residual_of(node, taps, SPECS))


def test_comparator_passes_the_emulation(run):
    _, taps = run
    for node in NODES:
        if node[0] not in taps or node[1] != "conv":
            continue
        sp, ts, x, res = _operands(run, node[0])
        assert (res is not None) == node[0].endswith(".conv3")
        ref, mag = M.layer_ref(sp, x, ts, residual=res)
        worst = R.assert_within(taps[node[0]], ref,
                                M.layer_tolerance(sp, ref, mag), node[0])
        assert worst < 1.0
        print(f"emulation err/tol resnet50 {node[0]}: {worst:.3f}")
    assert np.array_equal(taps["maxpool"], R.maxpool_ref(taps["conv1"]))


def test_emulation_agrees_with_the_fp32_torch_reference(frame):
    """Ties the new reference to the old one: torch_reference's fp32 taps
    against the bf16 emulation on the same 3-channel conv1.weight file,
    within the budgets test_resnet50_per_stage_activations uses for the
    engine."""
    ts = resnet50.generate_layer_weights(seed=41, conv1_channels=3)
    taps = M.emulate(NODES, resnet50.layer_specs(), ts, frame,
                     resnet50.IN_HW, last="block2.conv3")
    budgets = {"conv1": 0.03, "maxpool": 0.03, "block2": 0.05}
    for tap, budget in budgets.items():
        got = taps[tap if tap in taps else tap + ".conv3"]
        ref = resnet50.torch_reference(ts, frame, tap=tap)
        assert got.shape == ref.shape, (tap, got.shape, ref.shape)
        e = float(np.sqrt(np.mean((got - ref) ** 2)) /
                  (np.sqrt(np.mean(ref ** 2)) + 1e-6))
        corr = np.corrcoef(got.ravel(), ref.ravel())[0, 1]
        print(f"emulation vs fp32 torch at {tap}: rel RMS {e:.4f}, "
              f"corr {corr:.5f}")
        assert e < budget, f"{tap}: rel RMS err {e:.4f} > {budget}"
        assert corr > 0.99, f"{tap}: corr {corr:.5f}"


# ---- seeded bugs ----

def _mutation(run, name, what, x=None, **kw):
    sp, ts, x0, res = _operands(run, name)
    ref, mag = M.layer_ref(sp, x0, ts, residual=res)
    kw.setdefault("residual", res)
    mutated, _ = M.layer_ref(sp, x0 if x is None else x, ts, **kw)
    return _rate(sp, ref, mag, mutated, f"{what} at {name}")


def test_mutation_residual_dropped(run):
    _mutation(run, "block1.conv3", "residual dropped", residual=None)


def test_mutation_block_input_as_identity(run):
    """block3.conv3 adds the block's input, every other pixel, instead of
    its projection: the 256 channels that exist land in columns 0..255, the
    rest get nothing (the parameter-free shortcut)."""
    _, taps = run
    x = taps["block2.conv3"][:, ::2, ::2]
    bad = np.concatenate([x, np.zeros_like(x)], axis=3)
    assert bad.shape == taps["block3.downsample"].shape
    _mutation(run, "block3.conv3", "block input [::2, ::2] as identity",
              residual=bad)


def test_mutation_downsample_samples_odd_pixels(run):
    _, taps = run
    x = np.ascontiguousarray(taps["block2.conv3"][:, 1:, 1:])
    _mutation(run, "block3.downsample", "sampling [1::2, 1::2]", x=x)


def test_mutation_stride_on_conv1_instead_of_conv2(run):
    """The v1 / v1.5 ambiguity, seen at block3.conv2: conv1 strided, conv2
    not."""
    sp1, ts, x1, _ = _operands(run, "block3.conv1")
    y1 = R.bf16_round(M.layer_ref(sp1, x1, ts, stride=2)[0])
    assert y1.shape == (1, 28, 28, 128)
    _mutation(run, "block3.conv2", "stride on conv1", x=y1, stride=1)


@pytest.mark.parametrize("name", ["block0.downsample", "block3.downsample"])
def test_mutation_relu_on_downsample(run, name):
    _mutation(run, name, "relu", relu=True)


def test_mutation_relu_before_the_residual_add(run):
    sp, ts, x, res = _operands(run, "block1.conv3")
    ref, mag = M.layer_ref(sp, x, ts, residual=res)
    early, _ = M.layer_ref(sp, x, ts, relu=True)
    mutated = np.maximum(early + res.astype(np.float64), 0.0)
    _rate(sp, ref, mag, mutated, "relu before the residual add at "
          "block1.conv3")


@pytest.mark.parametrize("name,nxt", [("block1.conv2", "block1.conv3"),
                                      ("block0.conv3", "block0.downsample"),
                                      ("block3.conv1", "block3.conv2")])
def test_mutation_scale_bias_of_following_conv(run, name, nxt):
    """What a wrong sb_off does: the scale/bias block of the conv that
    follows in spec order."""
    ts, _ = run
    out_c = SPECS[name]["out_c"]
    assert SPECS[nxt]["out_c"] >= out_c
    _mutation(run, name, f"scale/bias of {nxt}",
              scale=ts[nxt + ".scale"][:out_c], bias=ts[nxt + ".bias"][:out_c])


def test_mutation_garbage_in_pre_pad_channels(run):
    bad = run[1]["pre"].copy()
    bad[..., 3:] = 1.0
    _mutation(run, "conv1", "pre channels 3..7 = 1", x=bad)


def test_mutation_conv1_expansion_transposed(run):
    """A 64 x 7 x 7 x 3 conv1.weight read as [o][c][r*s] instead of
    [o][r*s][c] when it is expanded to 8 input channels."""
    sp, ts, x, _ = _operands(run, "conv1")
    w3 = np.ascontiguousarray(ts["conv1.weight"][..., :3])
    ts3 = dict(ts, **{"conv1.weight": w3})
    ref, mag = M.layer_ref(sp, x, ts3)
    bad3 = w3.reshape(64, 3, 49).transpose(0, 2, 1).reshape(64, 7, 7, 3)
    assert not np.array_equal(bad3, w3)
    bad = M.weight_ohwi(sp, {"conv1.weight": bad3})
    mutated, _ = M.layer_ref(sp, x, ts3, weight=bad)
    _rate(sp, ref, mag, mutated, "conv1 expansion read as [o][c][r*s]")


def test_mutation_avgpool_divides_by_64(run):
    """The 7 x 7 mean taken with the next power of two. The 7 x 7 windows
    are cut from the block3 tap, the deepest the walk has."""
    x = np.ascontiguousarray(run[1]["block3.conv3"][:, 3:24:3, 3:24:3])
    assert x.shape == (1, 7, 7, 512)
    ref, tol = R.avgpool_ref(x)
    mutated, _ = R.avgpool_ref(x, divisor=64)
    affected = mutated != ref
    assert affected.any()
    flagged = R.err_over_tol(mutated, ref, tol) > 1.0
    rate = float((flagged & affected).sum() / affected.sum())
    print(f"mutation avgpool / 64: {rate:.1%} of {int(affected.sum())} "
          f"changed elements flagged")
    assert rate >= 0.10


def test_maxpool_padding_value_cannot_show(run):
    """A bug that cannot show: the maxpool border padded with 0 instead of
    -inf. conv1 ends in a relu, so every window already holds a value >= 0
    and the two pools are the same function of any conv1 tap; no test of
    the network can tell them apart (test_dnn_kernels_gpu.py::test_maxpool
    does, on an all-negative input)."""
    conv1 = run[1]["conv1"]
    assert conv1.min() >= 0 and (conv1 == 0).any()
    assert np.array_equal(R.maxpool_ref(conv1),
                          R.maxpool_ref(conv1, pad_value=0.0))
    neg = -np.abs(conv1) - 1.0
    assert not np.array_equal(R.maxpool_ref(neg),
                              R.maxpool_ref(neg, pad_value=0.0))


# ---- the dispatch plans at the two batch sizes ----

@pytest.mark.parametrize("name", list(M.RESNET_PLANS))
def test_plan_table(name):
    """The in-network dispatch paths test_resnet_layers_gpu.py covers: at
    batch 2 every layer, at batch 64 the plans the benchmark runs. A planner
    change shows here as the layer whose path lost its coverage."""
    side = M.resnet_tap_sides()[name]
    for batch, want in M.RESNET_PLANS[name].items():
        shape = M.resnet_gemm_shape(SPECS[name], side, batch)
        assert R.plan_of(_core, *shape) == want, (name, batch, shape)


def test_plan_table_is_where_the_batches_differ():
    """Outside the table, batch 64 changes the grid and the swizzle and
    nothing else."""
    sides = M.resnet_tap_sides()
    for name, sp in SPECS.items():
        a, b = (R.plan_of(_core, *M.resnet_gemm_shape(sp, sides[name], n))
                for n in (2, 64))
        if name in M.RESNET_PLANS:
            continue
        for k in ("kernel", "splits", "ksteps_per_split", "tiles_per_wg",
                  "atomic", "fused"):
            assert a[k] == b[k], (name, k, a, b)
        assert b["swizzle"] or b["kernel"] in ("splitk", "smallk"), name
