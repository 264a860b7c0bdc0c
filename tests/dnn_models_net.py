"""What the layer-by-layer GPU tests share (test_dnn_models_gpu.py,
test_resnet_layers_gpu.py): one op with one weight file, its taps through
`_core.op_kernel_test` and `debug_tap`, and the per-layer checks against the
float64 references of dnn_models_ref.py fed the GPU's own source taps.
"""
import msgpack
import numpy as np

import dnn_models_ref as M
import dnn_ref as R
from scanner_amd import _core
from scanner_amd.models import detector, pose, resnet50

GPU = 1
FRAMES = M.frames_45x61()

SIDE = {"Pose": pose.IN_HW, "Detector": detector.IN_HW,
        "ResNet50": resnet50.IN_HW}


class Net:
    """One op with one weight file: its taps (each fetched once) and its
    real output. `frames` is the batch (FRAMES by default); with `keep`, a
    list of frame indices, only those frames of a fetched tap are kept and
    compared, so a large batch is never held whole."""

    def __init__(self, op, nodes, specs, tensors, path, frames=None,
                 keep=None, **args):
        self.op, self.nodes = op, nodes
        self.specs = {s["name"]: s for s in specs}
        self.ts = tensors
        self.args = dict(args)
        self.batch = FRAMES if frames is None else frames
        self.keep = list(range(len(self.batch))) if keep is None \
            else list(keep)
        self.frames = self.batch[self.keep]
        if tensors is not None:
            pose.write_tensor_file(str(path), tensors)
            self.args["weights_file"] = str(path)
        self._taps = {}
        self._out = None

    def run(self, **extra):
        return _core.op_kernel_test(
            self.op, GPU, msgpack.packb(dict(self.args, **extra)),
            list(self.batch))

    def fetch(self, name):
        side = SIDE[self.op]
        rows = self.run(debug_tap=name)
        assert len(rows) == len(self.batch)
        x = np.stack([np.frombuffer(rows[f], np.float32) for f in self.keep])
        del rows
        node = self.node(name)
        c = M.live_channels(node, self.specs)
        if node[1] == "conv":
            c = -(-c // 64) * 64
        assert x.shape[1] % c == 0
        hw = int(round((x.shape[1] // c) ** 0.5))
        assert hw * hw * c == x.shape[1] and side % hw == 0, (name, x.shape)
        return x.reshape(len(self.keep), hw, hw, c)

    def tap(self, name):
        if name not in self._taps:
            self._taps[name] = self.fetch(name)
        return self._taps[name]

    def output(self):
        if self._out is None:
            self._out = self.run()
        return self._out

    def node(self, name):
        return next(n for n in self.nodes if n[0] == name)

    def conv_names(self):
        return [n[0] for n in self.nodes if n[1] == "conv"]


def check_pre(net, ohw):
    got = net.tap("pre")
    assert got.shape == (len(net.keep), ohw, ohw, 8)
    ref, tol = M.pre_ref(net.frames, ohw)
    worst = R.assert_within(got[..., :3], ref, tol, f"{net.op} pre")
    assert not got[..., 3:].view(np.uint32).any(), "pre pad channels not +0"
    print(f"worst err/tol {net.op} pre: {worst:.3f}")


def conv_reference(net, name, tensors=None):
    """(spec, ref, tol) of one conv node from the net's own source taps."""
    sp_ = net.specs[name]
    node = net.node(name)
    taps = {s: net.tap(s) for s in node[2]}
    ref, mag = M.layer_ref(sp_, M.source_of(node, taps, net.specs),
                           tensors or net.ts,
                           residual=M.residual_of(node, taps, net.specs))
    return sp_, ref, M.layer_tolerance(sp_, ref, mag)


def check_conv(net, name, tensors=None, got=None):
    """Every live element of every kept frame within the layer's tolerance,
    pad columns exactly +0. `got` replaces the net's own tap of the layer."""
    sp_, ref, tol = conv_reference(net, name, tensors)
    got = net.tap(name) if got is None else got
    assert got.shape[:3] == ref.shape[:3], (name, got.shape, ref.shape)
    assert got.shape[3] == -(-sp_["out_c"] // 64) * 64
    worst = []
    for i, f in enumerate(net.keep):  # frame 1 always, frame 0 as well
        worst.append(R.assert_within(got[i, ..., :sp_["out_c"]], ref[i],
                                     tol[i], f"{net.op} {name} frame {f}"))
    pad = got[..., sp_["out_c"]:]
    assert not pad.view(np.uint32).any(), \
        f"{net.op} {name}: pad columns >= {sp_['out_c']} are not +0"
    print(f"worst err/tol {net.op} {name}: " + ", ".join(
        f"frame {f} {v:.3f}" for f, v in zip(net.keep, worst)))
    return max(worst)
