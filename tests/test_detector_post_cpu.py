"""The Detector op's host post-process (`_core.detector_postprocess`: sigmoid,
anchor decode, clip, top-k, NMS, blob) on crafted head maps, against the
float64 reference of dnn_models_ref.detector_post_ref.

Inputs are bf16-exact; every logit not set is -8. Every case asserts that
no decision the reference took was closer than 1e-3 to its threshold (the
float32 post-process is 1e-6 from float64 at the worst), then compares box
for box: coordinates within 16 * 2^-24 * 946, score within 4 * 2^-24 (and
exactly where the sigmoid is exact), label exactly. A 480 x 360 frame makes
sx = 1.5 and sy = 1.125 different.
"""
import numpy as np
import pytest

import dnn_models_ref as M
import dnn_ref as R
from scanner_amd import _core, types

IH, IW = 360, 480


class Maps:
    def __init__(self):
        self.loc = np.zeros((1600, 64), np.float32)
        self.cls = np.full((1600, 64), -8.0, np.float32)

    def put(self, x, y, a, logit, label=0, d=(0, 0, 0, 0)):
        cell = y * 40 + x
        self.cls[cell, a * 8 + label] = logit
        self.loc[cell, a * 4:a * 4 + 4] = d
        return cell

    def run(self, what, ih=IH, iw=IW):
        assert np.array_equal(R.bf16_round(self.loc), self.loc)
        assert np.array_equal(R.bf16_round(self.cls), self.cls)
        kept, m = M.detector_post_ref(self.loc, self.cls, ih, iw)
        assert m["min"] >= 1e-3, f"{what}: a decision is marginal: {m}"
        assert m["order"] >= 2.0 ** -20, f"{what}: scores too close: {m}"
        blob = _core.detector_postprocess(self.loc, self.cls, ih, iw)
        M.assert_boxes_match(blob, kept, what)
        return kept, M.unpack_boxes(blob), blob


def _ids(kept):
    return [(b[6], b[7]) for b in kept]


def test_one_candidate_per_anchor_size():
    mp = Maps()
    cells = [mp.put(10, 10, 0, 1.0, 1, (0.25, -0.5, 0.5, -0.25)),
             mp.put(30, 10, 1, 1.5, 2),
             mp.put(10, 30, 2, 2.0, 3, (-0.25, 0.125, -0.5, 0.75)),
             mp.put(28, 28, 3, 2.5, 4, (0.125, -0.125, 0.25, 0.125))]
    kept, got, _ = mp.run("per-anchor")
    assert _ids(kept) == [(cells[3], 3), (cells[2], 2), (cells[1], 1),
                          (cells[0], 0)]
    assert [g[5] for g in got] == [4, 3, 2, 1]
    # anchor 32 at cell (30, 10) with zero deltas, in closed form: centre
    # (244, 84), +-16, times (1.5, 1.125) -- every value exact in float32
    assert got[2][:4] == (342.0, 76.5, 390.0, 112.5)


def test_score_threshold_is_inclusive():
    mp = Maps()
    keep = mp.put(5, 5, 1, 0.0, 2)
    mp.put(20, 20, 1, -2.0 ** -7, 2)
    kept, got, _ = mp.run("threshold")
    assert _ids(kept) == [(keep, 1)]
    assert got[0][4] == 0.5 and got[0][5] == 2  # sigmoid(0) is exact


def test_class_ties_take_the_first_class():
    mp = Maps()
    mp.put(7, 9, 2, 1.0, 5)
    mp.put(7, 9, 2, 1.0, 3)
    mp.put(7, 9, 2, 0.5, 1)
    kept, got, _ = mp.run("class tie")
    assert len(got) == 1 and got[0][5] == 3


def test_anchor_reads_its_own_classes_and_deltas():
    mp = Maps()
    cell = 12 * 40 + 17
    for a in range(4):  # other anchors: distinct deltas, no score
        mp.loc[cell, a * 4:a * 4 + 4] = (0.5 * a - 1, 0.25 * a, 1 - a, a - 2)
    mp.cls[cell, 2 * 8 + 6] = 1.0
    kept, got, _ = mp.run("own columns")
    assert _ids(kept) == [(cell, 2)] and got[0][5] == 6
    # anchor 2 (64): d = (0, 0.5, -1, 0)
    cx, cy = 17 * 8 + 4, 12 * 8 + 4 + np.tanh(0.5) * 64
    bw, bh = 64 * np.exp(-1.0), 64.0
    want = ((cx - bw / 2) * 1.5, (cy - bh / 2) * 1.125,
            (cx + bw / 2) * 1.5, (cy + bh / 2) * 1.125)
    assert np.abs(np.array(got[0][:4], np.float64) - want).max() <= M.BOX_TOL


def test_extent_clamp_at_two():
    mp = Maps()
    mp.put(8, 8, 0, 3.0, 0, (0, 0, 2, 2))
    mp.put(30, 30, 0, 2.0, 0, (0, 0, 3, 3))
    mp.put(8, 30, 0, 1.0, 0, (0, 0, -3, -3))
    kept, got, _ = mp.run("clamp")
    assert len(got) == 3
    w = [g[2] - g[0] for g in got]
    h = [g[3] - g[1] for g in got]
    e2 = 16 * np.exp(2.0)
    for i in (0, 1):  # d = 3 gives what d = 2 gives
        assert abs(w[i] - e2 * 1.5) <= 2 * M.BOX_TOL
        assert abs(h[i] - e2 * 1.125) <= 2 * M.BOX_TOL
    assert abs(w[2] - 16 * np.exp(-3.0) * 1.5) <= 2 * M.BOX_TOL


def test_tanh_saturation():
    mp = Maps()
    mp.put(20, 20, 1, 1.0, 0, (8, -8, 0, 0))
    mp.put(10, 30, 2, 2.0, 0, (-8, 8, 0, 0))
    kept, got, _ = mp.run("tanh")
    assert len(got) == 2
    # centre moved by one anchor size, to float32 accuracy
    assert abs(got[1][0] - (164 + 32 - 16) * 1.5) <= M.BOX_TOL
    assert abs(got[1][1] - (164 - 32 - 16) * 1.125) <= M.BOX_TOL


def test_clipped_at_each_border():
    mp = Maps()
    mp.put(0, 20, 3, 4.0)
    mp.put(39, 20, 3, 3.0)
    mp.put(20, 0, 3, 2.0)
    mp.put(20, 39, 3, 1.0)
    kept, got, _ = mp.run("clip")
    assert len(got) == 4
    assert got[0][0] == 0.0 and got[0][2] == 68 * 1.5
    assert got[1][2] == float(IW) and got[1][0] == 252 * 1.5
    assert got[2][1] == 0.0 and got[2][3] == 68 * 1.125
    assert got[3][3] == float(IH) and got[3][1] == 252 * 1.125


def test_box_outside_the_frame_is_dropped():
    mp = Maps()
    mp.put(39, 20, 3, 3.0, 0, (8, 0, 0, 0))   # x from 570 on, frame ends 480
    mp.put(20, 0, 3, 2.0, 0, (0, -8, 0, 0))   # y up to -67.5
    ok = mp.put(12, 12, 1, 1.0)
    kept, got, _ = mp.run("outside")
    assert _ids(kept) == [(ok, 1)]


def test_nms_is_class_agnostic():
    mp = Maps()
    a = mp.put(10, 10, 2, 2.0, 1)
    mp.put(11, 10, 2, 1.0, 5)     # IoU 56/72 = 0.78 with a: suppressed
    big = mp.put(10, 10, 3, 0.5, 5)  # IoU 0.25 with a: kept
    kept, got, _ = mp.run("nms")
    assert _ids(kept) == [(a, 2), (big, 3)]
    assert [g[5] for g in got] == [1, 5]


def test_nms_chain_keeps_what_only_a_suppressed_box_overlaps():
    mp = Maps()
    a = mp.put(10, 20, 2, 3.0, 0)
    mp.put(11, 20, 2, 2.0, 0)      # IoU 0.78 with a
    c = mp.put(13, 20, 2, 1.0, 0)  # IoU 0.6 with b, 40/88 = 0.45 with a
    kept, _, _ = mp.run("chain")
    assert _ids(kept) == [(a, 2), (c, 2)]


def _bf16_values(lo_bits, hi_bits):
    bits = np.arange(lo_bits, hi_bits, dtype=np.uint32) << 16
    return bits.view(np.float32)


def _many(rng, n):
    """n (cell, anchor) sites on the two small anchors of shuffled cells,
    every box shrunk by exp(-3) to under 2 pixels: concentric anchors have
    IoU 0.25 and neighbouring cells do not touch, so NMS drops nothing."""
    cells = rng.permutation(1600)[:(n + 1) // 2]
    sites = [(int(c), a) for c in cells for a in (0, 1)][:n]
    return [sites[i] for i in rng.permutation(n)]


def _put_site(mp, site, logit):
    cell, a = site
    mp.put(cell % 40, cell // 40, a, logit, a + 1, (0, 0, -3, -3))


def test_top_1000_of_distinct_scores():
    rng = np.random.RandomState(1003)
    sites = _many(rng, 1003)
    high = _bf16_values(0x3D00, 0x4100)[-1000:]   # 1000 values in [0.03, 8)
    low = _bf16_values(0x3C00, 0x3C60)[::32]      # 3 values near 0.01
    assert len(high) == 1000 and len(low) == 3 and low.max() < high.min()
    mp = Maps()
    logits = rng.permutation(np.concatenate([high, low]))
    for site, v in zip(sites, logits):
        _put_site(mp, site, float(v))
    kept, got, _ = mp.run("top-1000")
    assert len(got) == 1000
    want = sorted(zip(-logits, sites))[:1000]
    assert _ids(kept) == [s for _, s in want]
    m = M.detector_post_ref(mp.loc, mp.cls, IH, IW, nms=False)[1]
    assert 1e-3 <= m["cut"] < np.inf


@pytest.fixture(scope="module")
def tied():
    """1003 candidates, 500 at logit 2 and 503 at logit 1: the cut falls
    inside the second tie."""
    rng = np.random.RandomState(503)
    sites = _many(rng, 1003)
    mp = Maps()
    for i, site in enumerate(sites):
        _put_site(mp, site, 2.0 if i < 500 else 1.0)
    return mp, sites


def test_ties_across_the_cut_keep_cell_anchor_order(tied):
    mp, sites = tied
    kept, got, _ = mp.run("tied cut")
    want = sorted(sites[:500]) + sorted(sites[500:])[:500]
    assert _ids(kept) == want
    assert len(got) == 1000
    m = M.detector_post_ref(mp.loc, mp.cls, IH, IW, nms=False)[1]
    assert m["cut"] == np.inf  # a tie at the cut: decided by order alone


def test_python_nms_best_visits_ties_in_the_given_order(tied):
    mp, _ = tied
    pairs = Maps()
    pairs.loc, pairs.cls = mp.loc.copy(), mp.cls.copy()
    # tied neighbours on the 64 anchor, IoU 0.78: the first of each survives
    for x in range(4, 36, 4):
        for y in (3, 21):
            pairs.put(x, y, 2, 1.0, 7)
            pairs.put(x + 1, y, 2, 1.0, 7)
    kept, _, _ = pairs.run("nms_best")
    cand, _ = M.detector_post_ref(pairs.loc, pairs.cls, IH, IW, nms=False)
    assert len(cand) == 1000
    by_site = sorted(cand, key=lambda b: (b[6], b[7]))  # generation order
    boxes = [types.BoundingBox(*b[:6]) for b in by_site]
    out = types.nms_best(boxes)
    index = {id(b): c for b, c in zip(boxes, by_site)}
    assert _ids([index[id(b)] for b in out]) == _ids(kept)
    assert len(out) < len(cand)  # the tied neighbours did meet


def test_empty_result_is_a_four_byte_blob():
    mp = Maps()
    kept, got, blob = mp.run("empty")
    assert kept == [] and blob == b"\x00\x00\x00\x00"


def test_blob_round_trips_through_types():
    mp = Maps()
    mp.put(10, 10, 2, 2.0, 1, (0.25, 0.5, -0.25, 0.125))
    mp.put(30, 25, 1, 0.0, 6)
    _, got, blob = mp.run("round trip")
    boxes = types.loads("BoundingBoxList", blob)
    assert len(boxes) == 2
    assert types.dumps("BoundingBoxList", boxes) == blob
    for b, g in zip(boxes, got):
        assert (np.float32(b.x1), np.float32(b.y1), np.float32(b.x2),
                np.float32(b.y2), np.float32(b.score), b.label) == g


def test_bad_shapes_are_rejected():
    ok = np.zeros((1600, 64), np.float32)
    with pytest.raises(Exception, match=r"\[1600\]\[64\]"):
        _core.detector_postprocess(ok[:100], ok, IH, IW)
    with pytest.raises(Exception, match="bad frame size"):
        _core.detector_postprocess(ok, ok, 0, IW)
