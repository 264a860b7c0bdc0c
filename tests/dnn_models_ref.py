"""Per-layer float64 references for the Pose, Detector and ResNet-50
networks (test_dnn_models_cpu.py, test_dnn_models_gpu.py,
test_detector_post_cpu.py, test_resnet_layers_cpu.py,
test_resnet_layers_gpu.py).

Written from the topology comments at the top of csrc/ops/pose.cpp and
csrc/ops/detector.cpp and from resnet50_specs() with the bottleneck
topology stated at resnet_nodes() below, not from the ops' loops: a layer is
torch.nn.functional.conv2d in float64 on the bf16-exact previous activation
and the bf16-rounded weights, then the f32 scale and bias as float64, then
the bf16-exact residual where the node names one, then relu where the spec
says so. Each layer is checked against the reference
fed the *engine's own* previous activation (teacher forcing), so the bound
is the single-GEMM bound of dnn_ref.tolerance with K = r * s * in_c and no
error accumulates across layers.
"""
import numpy as np

import dnn_ref as R

# Box coordinates: 16 float32 roundings of the largest intermediate,
# 128 * e^2 = 946 (the widest anchor at the clamp).
BOX_TOL = 16 * 2.0 ** -24 * 946


# ---- inputs ----

def frames_45x61():
    """Two different frames of an odd size: 0 smooth (three gradients), 1
    noise (batch index 1 is the one indexing bugs show on)."""
    yy, xx = np.mgrid[0:45, 0:61]
    smooth = np.stack([20 + 3 * xx, 30 + 3 * yy, 25 + 3 * (xx + yy) // 2],
                      axis=-1)
    noise = np.random.RandomState(61).randint(0, 256, (45, 61, 3))
    return np.stack([smooth, noise]).astype(np.uint8)


# ---- the graphs: (tap name, kind, source taps), in forward order ----

def pose_nodes(stages):
    nodes = [("pre", "pre", ())]
    prev = "pre"
    for k in range(1, 9):
        nodes.append((f"b{k}", "conv", (prev,)))
        prev = f"b{k}"
    for t in range(1, stages + 1):
        if t == 1:
            src = "b8"
        else:
            src = f"cat{t}"
            nodes.append((src, "cat", ("b8", f"s{t - 1}L_5", f"s{t - 1}S_5")))
        for br in "LS":
            prev = src
            for k in range(1, 6):
                nodes.append((f"s{t}{br}_{k}", "conv", (prev,)))
                prev = f"s{t}{br}_{k}"
    return nodes


def detector_nodes():
    nodes = [("pre", "pre", ())]
    prev = "pre"
    for name in ("b1", "b2", "b3", "b4", "b5", "b6", "head"):
        nodes.append((name, "conv", (prev,)))
        prev = name
    nodes += [("loc", "conv", ("head",)), ("cls", "conv", ("head",))]
    return nodes


# ResNet-50 v1.5: (blocks, mid channels, out channels, stride of the first
# block) per stage. A bottleneck block is conv1 1x1 -> mid, conv2 3x3 -> mid
# (the block's stride is here, not on conv1), conv3 1x1 -> out; the first
# block of a stage projects its input with `downsample`, 1x1 at the block's
# stride, no relu. out = relu(conv3(conv2(conv1(x))) * scale + bias + id),
# id = downsample(x) where there is one, else x.
RESNET_STAGES = ((3, 64, 256, 1), (4, 128, 512, 2), (6, 256, 1024, 2),
                 (3, 512, 2048, 2))


def resnet_nodes():
    """pre -> conv1 7x7 s2 -> maxpool 3x3 s2 p1 -> 16 bottleneck blocks ->
    global average -> fc. A conv3 node names two sources: its conv2 tap and
    its identity. The downsample node comes first within its block, where
    resnet50_specs() has it last: it is ready before conv3 needs it."""
    nodes = [("pre", "pre", ()), ("conv1", "conv", ("pre",)),
             ("maxpool", "maxpool", ("conv1",))]
    prev = "maxpool"
    b = 0
    for count, _, _, _ in RESNET_STAGES:
        for i in range(count):
            p = f"block{b}"
            identity = prev
            if i == 0:
                identity = p + ".downsample"
                nodes.append((identity, "conv", (prev,)))
            nodes += [(p + ".conv1", "conv", (prev,)),
                      (p + ".conv2", "conv", (p + ".conv1",)),
                      (p + ".conv3", "conv", (p + ".conv2", identity))]
            prev = p + ".conv3"
            b += 1
    nodes += [("avgpool", "avgpool", (prev,)), ("fc", "conv", ("avgpool",))]
    return nodes


def resnet_tap_sides():
    """{tap: h (= w)} of every node, walked from the 224 x 224 input."""
    from scanner_amd.models import resnet50
    specs = {s["name"]: s for s in resnet50.layer_specs()}
    side = {}
    for name, kind, srcs in resnet_nodes():
        if kind == "pre":
            side[name] = resnet50.IN_HW
        elif kind == "avgpool":
            side[name] = 1
        else:
            k, stride, pad = (3, 2, 1) if kind == "maxpool" else (
                specs[name]["r"], specs[name]["stride"], specs[name]["pad"])
            side[name] = (side[srcs[0]] + 2 * pad - k) // stride + 1
    return side


RESNET_SCRATCH = 64 << 20  # the op's split-K scratch


def resnet_gemm_shape(spec, side, batch):
    """(M, N, K, scratch, is_conv) as the op hands the layer to gemm_plan:
    a 1x1 stride-1 conv (and fc) is a plain GEMM, every other conv takes
    the implicit path."""
    direct = spec["r"] == 1 and spec["stride"] == 1 and spec["pad"] == 0
    return (batch * side * side, -(-spec["out_c"] // 64) * 64,
            -(-spec["r"] * spec["s"] * spec["in_c"] // 64) * 64,
            RESNET_SCRATCH, not direct)


def _resnet_plans():
    """{layer: {batch: plan}}: the dispatch paths that differ between the
    batch the tests could afford everywhere (2) and the batch the benchmark
    runs (64), as _core.gemm_plan gives them. Where the planner changes,
    test_resnet_layers_cpu.py says which in-network path lost its test."""
    p = R.plan
    t = {}
    for name in ("block0.downsample", "block0.conv3", "block1.conv3",
                 "block2.conv3"):
        # K = 64, N = 256; M = 200 704 at batch 64 walks two tiles per
        # workgroup at the default SCANNER_SMALLK_WGS
        t[name] = {2: p("smallk", 98, 64), 64: p("smallk", 1568, 64, tpw=2)}
    for b in range(3, 7):       # 3x3, c = 128; block3 is stride 2
        t[f"block{b}.conv2"] = {
            2: p("splitk", 52, 1152, splits=4, kps=5),
            64: p("tile128", 392, 1152, swizzle=True)}
    for b in range(7, 13):      # 3x3, c = 256; block7 is stride 2
        # batch 64: 6 splits wanted, 5 partials of 12 544 * 256 * 4 B fit
        # the scratch: 8, 8, 8, 8, 4 k-steps
        t[f"block{b}.conv2"] = {
            2: p("splitk", 48, 2304, splits=6, kps=6),
            64: p("splitk", 980, 2304, splits=5, kps=8)}
    t["block13.downsample"] = {2: p("splitk", 64, 1024, splits=4, kps=4),
                               64: p("tile128", 400, 1024, swizzle=True)}
    t["block13.conv1"] = {2: p("splitk", 64, 1024, splits=4, kps=4),
                          64: p("tile128", 392, 1024, swizzle=True)}
    t["block13.conv3"] = {2: p("tile128", 16, 512, swizzle=True),
                          64: p("tile128", 400, 512, swizzle=True)}
    t["conv1"] = {2: p("tile64", 392, 448, swizzle=True),
                  64: p("tile64", 12544, 448, swizzle=True)}
    t["fc"] = {2: p("splitk", 48, 2048, splits=6, kps=6),
               64: p("splitk", 48, 2048, splits=6, kps=6)}
    return t


RESNET_PLANS = _resnet_plans()


def live_channels(node, specs):
    """How many channels of a node's tap carry data."""
    name, kind, srcs = node
    if kind == "conv":
        return specs[name]["out_c"]
    return {"pre": 8, "cat": 192, "maxpool": 64, "avgpool": 2048}[kind]


def noise_and_gradient_frames(n):
    """n distinct 45 x 61 frames: the two of frames_45x61(), then seeded
    noise (odd indices) and gradients of varying slope and offset (even)."""
    yy, xx = np.mgrid[0:45, 0:61]
    out = list(frames_45x61())
    for i in range(2, n):
        if i % 2:
            out.append(np.random.RandomState(1000 + i).randint(
                0, 256, (45, 61, 3)))
        else:
            a, b = 1 + i % 4, 1 + (i // 4) % 4
            out.append(np.stack([(3 * i + a * xx) % 256,
                                 (5 * i + b * yy) % 256,
                                 (7 * i + (a * xx + b * yy) // 2) % 256],
                                axis=-1))
    return np.stack(out).astype(np.uint8)


# ---- references ----

def pre_ref(frames, ohw):
    """(ref [n][ohw][ohw][3] float64, tol): the reference and tolerance of
    test_dnn_kernels_gpu.py::test_preprocess."""
    ref = R.preprocess_ref(frames, ohw)
    return ref, R.preprocess_tolerance(ref, frames.shape[1], frames.shape[2])


def weight_ohwi(spec, tensors):
    """The conv's bf16-rounded weights as [out][r][s][in_c]; a 3-channel b1
    (ResNet: conv1) tensor is zero-extended to the 8 input channels the
    entry conv reads."""
    w = np.asarray(tensors[spec["name"] + ".weight"], np.float32)
    w = w.reshape(spec["out_c"], spec["r"], spec["s"], -1)
    if w.shape[3] != spec["in_c"]:
        assert spec["name"] in ("b1", "conv1") and w.shape[3] == 3
        w = np.concatenate(
            [w, np.zeros(w.shape[:3] + (spec["in_c"] - 3,), np.float32)], 3)
    return R.bf16_round(w)


def layer_ref(spec, x_prev, tensors, weight=None, scale=None, bias=None,
              relu=None, residual=None, stride=None):
    """(ref, mag) of one conv as float64 [n][oh][ow][out_c]. x_prev is the
    bf16-exact input [n][h][w][in_c], residual the bf16-exact
    [n][oh][ow][out_c] operand added before the relu; mag = |scale| * (|x|
    conv |w|) + |bias| + |residual|. The other keyword arguments replace an
    operand (the seeded bugs of the comparator test)."""
    import torch
    import torch.nn.functional as F
    assert x_prev.shape[3] == spec["in_c"], (spec["name"], x_prev.shape)
    assert np.array_equal(R.bf16_round(x_prev), x_prev)
    w = weight_ohwi(spec, tensors) if weight is None else weight
    name = spec["name"]
    scale = tensors[name + ".scale"] if scale is None else scale
    bias = tensors[name + ".bias"] if bias is None else bias
    relu = spec["relu"] if relu is None else relu
    stride = spec["stride"] if stride is None else stride
    if residual is not None:
        assert np.array_equal(R.bf16_round(residual), residual)
    x = torch.from_numpy(x_prev.astype(np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2)

    def run(xx, ww):
        y = F.conv2d(xx, ww, stride=stride, padding=spec["pad"])
        return y.permute(0, 2, 3, 1).numpy()

    return R.epilogue_ref(run(x, wt), run(x.abs(), wt.abs()),
                          scale=np.asarray(scale, np.float32),
                          bias=np.asarray(bias, np.float32),
                          residual=residual, relu=relu)


def layer_tolerance(spec, ref, mag):
    return R.tolerance(ref, mag, spec["r"] * spec["s"] * spec["in_c"])


def cat_ref(F, L, S):
    """F[:128] | L[:38] | S[:19] | 7 zeros, per pixel."""
    zeros = np.zeros(F.shape[:3] + (7,), np.float32)
    return np.concatenate([F[..., :128], L[..., :38], S[..., :19], zeros],
                          axis=3).astype(np.float32)


def keypoints_ref(S):
    """[n][19][3] f32 {x, y, peak}: per-channel argmax of the heatmaps
    [n][h][w][>=19], the lowest flat index on ties."""
    n, h, w, _ = S.shape
    out = np.zeros((n, 19, 3), np.float32)
    for f in range(n):
        for ch in range(19):
            m = S[f, :, :, ch].reshape(-1)
            i = int(np.argmax(m))
            out[f, ch] = (i % w, i // w, m[i])
    return out


# ---- teacher-forced walk over a graph ----

def source_of(node, taps, specs):
    """The reference's input for a conv node, from the taps of its source:
    the first in_c channels (a tap carries the GEMM-padded count)."""
    name, kind, srcs = node
    assert kind == "conv"
    return np.ascontiguousarray(taps[srcs[0]][..., :specs[name]["in_c"]])


def residual_of(node, taps, specs):
    """The residual operand of a conv node: the first out_c channels of its
    second source, None where it has one source."""
    name, kind, srcs = node
    assert kind == "conv"
    if len(srcs) < 2:
        return None
    return np.ascontiguousarray(taps[srcs[1]][..., :specs[name]["out_c"]])


def emulate(nodes, spec_list, tensors, frames, ohw, last=None):
    """The network run by the references themselves: every node's output
    rounded to bf16 feeds the next, as far as node `last`. Returns {tap: f32
    [n][h][w][c]} with c = 8 for pre, out_c for a conv, 192 for a concat and
    the source's for a pool."""
    specs = {s["name"]: s for s in spec_list}
    taps = {}
    for node in nodes:
        name, kind, srcs = node
        if kind == "pre":
            pre = np.zeros((len(frames), ohw, ohw, 8), np.float32)
            pre[..., :3] = R.bf16_round(pre_ref(frames, ohw)[0])
            taps[name] = pre
        elif kind == "cat":
            taps[name] = cat_ref(*(taps[s] for s in srcs))
        elif kind == "maxpool":
            taps[name] = R.maxpool_ref(taps[srcs[0]]).astype(np.float32)
        elif kind == "avgpool":
            ref = R.avgpool_ref(taps[srcs[0]])[0]
            taps[name] = R.bf16_round(ref).reshape(len(frames), 1, 1, -1)
        else:
            ref, _ = layer_ref(specs[name], source_of(node, taps, specs),
                               tensors,
                               residual=residual_of(node, taps, specs))
            taps[name] = R.bf16_round(ref)
        if name == last:
            break
    return taps


# ---- detector post-process ----

DET_IN = 320
DET_FEAT = 40
DET_ANCHORS = (16.0, 32.0, 64.0, 128.0)
DET_CLASSES = 8
DET_TOPK = 1000


def _iou64(a, b):
    ix = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    iy = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = ix * iy
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) \
        - inter
    return inter / union if union > 0 else 0.0


def detector_post_ref(loc, cls, ih, iw, nms=True):
    """float64 post-process of one frame's [1600][64] head maps, from the
    header comment of detector.cpp: per cell (row-major over the 40 x 40
    map, centre (x + 0.5) * 8) and anchor a (sizes 16, 32, 64, 128): the
    score is the sigmoid of the largest of the anchor's 8 class logits
    (the first on ties), kept when >= 0.5; centre = cell centre + tanh(d0,
    d1) * size, extent = size * exp(min(2, d2, d3)); scaled by iw/320 and
    ih/320 and clipped to the frame; empty boxes dropped. Candidates are
    ordered by score descending, ties by (cell, anchor) ascending, cut to
    the first 1000, then greedy NMS: a box is dropped when its IoU with an
    earlier kept box is >= 0.5, whatever the labels.

    Returns (boxes, margins). boxes: [(x1, y1, x2, y2, score, label, cell,
    anchor)] in output order. margins: the smallest distance of every
    decision taken from its threshold -- 'score' |score - 0.5| (anchors
    whose logit is exactly 0 excepted: their sigmoid is exactly 0.5 in
    every IEEE format, so that decision cannot flip), 'cut' the score gap
    at the top-1000 cut when it falls between different scores, 'iou'
    |IoU - 0.5| over every pair evaluated, 'extent' the smallest |x2 - x1|,
    |y2 - y1| after clipping, and 'order' the smallest gap between
    different scores of candidates (informational: the order is decided on
    float32 sigmoids, which are a few 2^-24 from these). A margin no
    decision contributed to is inf; 'min' is the smallest of the first
    four. nms=False stops after the cut and returns the candidates in
    visiting order."""
    loc = np.asarray(loc, np.float64).reshape(DET_FEAT * DET_FEAT, 64)
    cls = np.asarray(cls, np.float64).reshape(DET_FEAT * DET_FEAT, 64)
    sx, sy = iw / DET_IN, ih / DET_IN
    m = dict(score=np.inf, cut=np.inf, iou=np.inf, extent=np.inf,
             order=np.inf)
    cand = []
    for cell in range(DET_FEAT * DET_FEAT):
        cxg = (cell % DET_FEAT + 0.5) * 8.0
        cyg = (cell // DET_FEAT + 0.5) * 8.0
        for a, size in enumerate(DET_ANCHORS):
            logits = cls[cell, a * DET_CLASSES:(a + 1) * DET_CLASSES]
            label = int(np.argmax(logits))  # first on ties
            logit = float(logits[label])
            score = 1.0 / (1.0 + np.exp(-logit))
            if logit != 0.0:
                m["score"] = min(m["score"], abs(score - 0.5))
            if score < 0.5:
                continue
            d = loc[cell, a * 4:a * 4 + 4]
            cx = cxg + np.tanh(d[0]) * size
            cy = cyg + np.tanh(d[1]) * size
            bw = size * np.exp(min(2.0, d[2]))
            bh = size * np.exp(min(2.0, d[3]))
            x1 = max(0.0, (cx - bw / 2) * sx)
            y1 = max(0.0, (cy - bh / 2) * sy)
            x2 = min(float(iw), (cx + bw / 2) * sx)
            y2 = min(float(ih), (cy + bh / 2) * sy)
            m["extent"] = min(m["extent"], abs(x2 - x1), abs(y2 - y1))
            if x2 <= x1 or y2 <= y1:
                continue
            cand.append((x1, y1, x2, y2, score, label, cell, a))
    cand.sort(key=lambda b: (-b[4], b[6], b[7]))
    for p, q in zip(cand, cand[1:]):
        if p[4] != q[4]:
            m["order"] = min(m["order"], p[4] - q[4])
    if len(cand) > DET_TOPK:
        gap = cand[DET_TOPK - 1][4] - cand[DET_TOPK][4]
        if gap > 0:
            m["cut"] = gap
        cand = cand[:DET_TOPK]
    if not nms:
        m["min"] = min(m["score"], m["cut"], m["extent"])
        return cand, m
    alive = [True] * len(cand)
    kept = []
    for i, b in enumerate(cand):
        if not alive[i]:
            continue
        kept.append(b)
        for j in range(i + 1, len(cand)):
            if alive[j]:
                v = _iou64(b, cand[j])
                m["iou"] = min(m["iou"], abs(v - 0.5))
                if v >= 0.5:
                    alive[j] = False
    m["min"] = min(m["score"], m["cut"], m["iou"], m["extent"])
    return kept, m


def unpack_boxes(blob):
    """BoundingBoxList blob -> [(x1, y1, x2, y2, score, label)] as float32
    values and int, read with numpy alone."""
    n = int(np.frombuffer(blob, "<u4", 1)[0])
    assert len(blob) == 4 + 24 * n, (len(blob), n)
    rec = np.frombuffer(blob, np.dtype([("b", "<f4", 5), ("l", "<i4")]), n, 4)
    return [tuple(r["b"]) + (int(r["l"]),) for r in rec]


def assert_boxes_match(blob, kept, what):
    """The blob holds the reference's boxes, box for box: coordinates
    within BOX_TOL, score within 4 * 2^-24 (float32 exp, add and divide on
    values <= 1), label equal."""
    got = unpack_boxes(blob)
    assert len(got) == len(kept), \
        f"{what}: {len(got)} boxes, reference keeps {len(kept)}"
    for i, (g, r) in enumerate(zip(got, kept)):
        assert g[5] == r[5], f"{what}: box {i} label {g[5]} != {r[5]}"
        assert abs(float(g[4]) - r[4]) <= 4 * 2.0 ** -24, \
            f"{what}: box {i} score {g[4]!r} vs {r[4]!r}"
        for k in range(4):
            assert abs(float(g[k]) - r[k]) <= BOX_TOL, \
                f"{what}: box {i} (cell {r[6]}, anchor {r[7]}) coordinate " \
                f"{k}: {g[k]!r} vs {r[k]!r}"
