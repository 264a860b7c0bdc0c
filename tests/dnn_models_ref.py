"""Per-layer float64 references for the Pose and Detector networks
(test_dnn_models_cpu.py, test_dnn_models_gpu.py, test_detector_post_cpu.py).

Written from the topology comments at the top of csrc/ops/pose.cpp and
csrc/ops/detector.cpp, not from the ops' loops: a layer is
torch.nn.functional.conv2d in float64 on the bf16-exact previous activation
and the bf16-rounded weights, then the f32 scale and bias as float64, then
relu where the spec says so. Each layer is checked against the reference
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


# ---- the two graphs: (tap name, kind, source taps), in forward order ----

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


# ---- references ----

def pre_ref(frames, ohw):
    """(ref [n][ohw][ohw][3] float64, tol): the reference and tolerance of
    test_dnn_kernels_gpu.py::test_preprocess."""
    ref = R.preprocess_ref(frames, ohw)
    return ref, R.preprocess_tolerance(ref, frames.shape[1], frames.shape[2])


def weight_ohwi(spec, tensors):
    """The conv's bf16-rounded weights as [out][r][s][in_c]; a 3-channel b1
    tensor is zero-extended to the 8 input channels the entry conv reads."""
    w = np.asarray(tensors[spec["name"] + ".weight"], np.float32)
    w = w.reshape(spec["out_c"], spec["r"], spec["s"], -1)
    if w.shape[3] != spec["in_c"]:
        assert spec["name"] == "b1" and w.shape[3] == 3
        w = np.concatenate(
            [w, np.zeros(w.shape[:3] + (spec["in_c"] - 3,), np.float32)], 3)
    return R.bf16_round(w)


def layer_ref(spec, x_prev, tensors, weight=None, scale=None, bias=None,
              relu=None):
    """(ref, mag) of one conv as float64 [n][oh][ow][out_c]. x_prev is the
    bf16-exact input [n][h][w][in_c]; mag = |scale| * (|x| conv |w|) +
    |bias|. The keyword arguments replace an operand (the seeded bugs of
    the comparator test)."""
    import torch
    import torch.nn.functional as F
    assert x_prev.shape[3] == spec["in_c"], (spec["name"], x_prev.shape)
    assert np.array_equal(R.bf16_round(x_prev), x_prev)
    w = weight_ohwi(spec, tensors) if weight is None else weight
    name = spec["name"]
    scale = tensors[name + ".scale"] if scale is None else scale
    bias = tensors[name + ".bias"] if bias is None else bias
    relu = spec["relu"] if relu is None else relu
    x = torch.from_numpy(x_prev.astype(np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2)

    def run(xx, ww):
        y = F.conv2d(xx, ww, stride=spec["stride"], padding=spec["pad"])
        return y.permute(0, 2, 3, 1).numpy()

    return R.epilogue_ref(run(x, wt), run(x.abs(), wt.abs()),
                          scale=np.asarray(scale, np.float32),
                          bias=np.asarray(bias, np.float32), relu=relu)


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


def emulate(nodes, spec_list, tensors, frames, ohw):
    """The network run by the references themselves: every node's output
    rounded to bf16 feeds the next. Returns {tap: f32 [n][h][w][c]} with
    c = 8 for pre, out_c for a conv and 192 for a concat."""
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
        else:
            ref, _ = layer_ref(specs[name], source_of(node, taps, specs),
                               tensors)
            taps[name] = R.bf16_round(ref)
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
