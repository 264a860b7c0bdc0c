"""ResNet-50 on the GPU, layer by layer, through `_core.op_kernel_test` and
the op's `debug_tap`.

Every conv tap (53 convs and fc) is compared with the float64 reference of
that one layer fed the GPU's *own* source taps (dnn_models_ref.py): conv ->
scale, bias -> + bf16-exact residual -> relu, every live element within
dnn_ref.tolerance(ref, mag, K = r * s * in_c) with |residual| in mag; pad
columns must be exactly +0, maxpool equal to its reference, avgpool within
the bound of test_dnn_kernels_gpu.py::test_avgpool, and the op's real output
bit-equal to the fc tap. test_resnet_layers_cpu.py shows that this
comparator flags a dropped or wrong residual, a wrong stride or sampling
phase, a misplaced relu, a wrong scale/bias block, a dirty pad channel and a
transposed conv1 expansion.

The op's internal size is 224 x 224 whatever the frames; the frames are
45 x 61 and the frame count is the batch (the harness sets max_batch to it).

Batch 2: every layer, both frames. Batch 64: the dispatch plans the
benchmark runs and batch 2 does not (dnn_models_ref.RESNET_PLANS), each
asserted through `_core.gemm_plan` before the layer is compared, with the
reference computed for frames 0, 37 and 63 alone; teacher forcing makes the
frames independent. Only those three frames of a 64-frame tap are kept.

Worst err/tol per layer is printed (`pytest -rP`) and tabulated in
docs/testing.md; no bound is tuned from it.
"""
import numpy as np
import pytest

import dnn_models_ref as M
import dnn_ref as R
from dnn_models_net import Net, check_conv, check_pre, conv_reference
from scanner_amd import _core
from scanner_amd.models import resnet50

pytestmark = pytest.mark.gpu

NODES = M.resnet_nodes()
SPECS = resnet50.layer_specs()
CONVS = [n[0] for n in NODES if n[1] == "conv"]
SIDES = M.resnet_tap_sides()
SEED = 51


@pytest.fixture(scope="module")
def net2(tmp_path_factory):
    return Net("ResNet50", NODES, SPECS,
               resnet50.generate_layer_weights(seed=SEED),
               tmp_path_factory.mktemp("resnet") / "w.bin")


def check_maxpool(net):
    got, src = net.tap("maxpool"), net.tap("conv1")
    assert got.shape == (len(net.keep), 56, 56, 64)
    assert np.array_equal(got, R.maxpool_ref(src).astype(np.float32))
    assert not np.signbit(got).any()
    print(f"{net.op} maxpool equals its reference")


def check_avgpool(net):
    got, src = net.tap("avgpool"), net.tap("block15.conv3")
    assert src.shape == (len(net.keep), 7, 7, 2048)
    assert got.shape == (len(net.keep), 1, 1, 2048)
    ref, tol = R.avgpool_ref(src)
    worst = R.assert_within(got.reshape(ref.shape), ref, tol,
                            f"{net.op} avgpool")
    print(f"worst err/tol {net.op} avgpool: {worst:.3f}")


# ---- batch 2: every layer ----

def test_pre(net2):
    check_pre(net2, resnet50.IN_HW)


@pytest.mark.parametrize("name", CONVS)
def test_layer(net2, name):
    check_conv(net2, name)
    assert net2.tap(name).shape[1] == SIDES[name]


def test_maxpool(net2):
    check_maxpool(net2)


def test_avgpool(net2):
    check_avgpool(net2)


def test_block_alias_is_the_conv3_tap(net2):
    a = net2.tap("block5.conv3")
    rows = net2.run(debug_tap="block5")
    b = np.stack([np.frombuffer(r, np.float32) for r in rows])
    assert np.array_equal(a.reshape(2, -1).view(np.uint32),
                          b.view(np.uint32))


def test_output_is_the_fc_tap(net2):
    rows = net2.output()
    assert len(rows) == 2
    out = np.stack([np.frombuffer(r, np.float32) for r in rows])
    fc = net2.tap("fc")
    assert out.shape == (2, 1000) and fc.shape == (2, 1, 1, 1024)
    assert np.array_equal(out.view(np.uint32),
                          fc[:, 0, 0, :1000].view(np.uint32))
    assert not np.array_equal(out[0], out[1])


def test_tap_is_repeatable(net2):
    a = net2.tap("block9.conv2")
    assert np.array_equal(a.view(np.uint32),
                          net2.fetch("block9.conv2").view(np.uint32))


def test_three_channel_conv1_weight(tmp_path):
    ts = resnet50.generate_layer_weights(seed=SEED + 1, conv1_channels=3)
    assert ts["conv1.weight"].shape == (64, 7, 7, 3)
    # the layers after conv1 are not run here: leave them to the engine
    ts = {k: v for k, v in ts.items() if k.startswith("conv1.")}
    net = Net("ResNet50", NODES, SPECS, ts, tmp_path / "w.bin")
    check_conv(net, "conv1")


def test_unknown_tap_is_rejected_by_name(net2):
    for name in ("block16", "block3.conv4", "block1.downsample"):
        with pytest.raises(Exception, match=f"unknown debug_tap '{name}'"):
            net2.run(debug_tap=name)


def test_skipped_residual_fails_the_layer_check(net2, monkeypatch):
    """The op's mutation seam at layer granularity: with block13's residual
    add dropped, the check that passes in test_layer[block13.conv3] fails,
    on at least 10 % of the elements."""
    monkeypatch.setenv("SCANNER_RESNET_SKIP_RESIDUAL", "block13")
    got = net2.fetch("block13.conv3")
    monkeypatch.delenv("SCANNER_RESNET_SKIP_RESIDUAL")
    with pytest.raises(AssertionError, match="elements outside tol"):
        check_conv(net2, "block13.conv3", got=got)
    _, ref, tol = conv_reference(net2, "block13.conv3")
    rate = float((R.err_over_tol(got, ref, tol) > 1.0).mean())
    print(f"residual skipped at block13.conv3: {rate:.1%} of the elements "
          f"out of bound")
    assert rate >= 0.10
    # and the seam leaves nothing behind
    check_conv(net2, "block13.conv3", got=net2.fetch("block13.conv3"))


# ---- batch 64: the plans the benchmark runs ----

BATCH = 64
KEEP = (0, 37, 63)
B64_LAYERS = ["conv1", "block0.downsample", "block0.conv3", "block2.conv3",
              "block3.conv2", "block4.conv2", "block7.conv2", "block8.conv2",
              "block13.downsample", "block13.conv1", "block13.conv3", "fc"]
B64_TWICE = ("block7.conv2", "fc")


@pytest.fixture(scope="module")
def net64(net2):
    """The weight file of net2, written once, at batch 64."""
    frames = M.noise_and_gradient_frames(BATCH)
    assert len({f.tobytes() for f in frames}) == BATCH
    net = Net("ResNet50", NODES, SPECS, None, None, frames=frames, keep=KEEP,
              weights_file=net2.args["weights_file"])
    net.ts = net2.ts
    return net


def test_batch64_pre(net64):
    check_pre(net64, resnet50.IN_HW)


@pytest.mark.parametrize("name", B64_LAYERS)
def test_batch64_layer(net64, name):
    sp = net64.specs[name]
    shape = M.resnet_gemm_shape(sp, SIDES[name], BATCH)
    assert R.plan_of(_core, *shape) == M.RESNET_PLANS[name][BATCH], name
    check_conv(net64, name)
    if name in B64_TWICE:  # split-K is deterministic by construction
        assert np.array_equal(net64.tap(name).view(np.uint32),
                              net64.fetch(name).view(np.uint32)), name


def test_batch64_maxpool(net64):
    check_maxpool(net64)


def test_batch64_avgpool(net64):
    check_avgpool(net64)
