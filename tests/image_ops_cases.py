"""The cases of the image, colour and optical-flow kernel tests, written once
and run on either device through `_core.op_kernel_test`:
test_image_ops_ref.py holds the CPU kernels to them, test_image_ops_gpu.py
the HIP kernels. References and bounds are in image_ref.py and flow_ref.py.
"""
import functools

import msgpack
import numpy as np

import flow_ref as F
import image_ref as I
from scanner_amd import _core

CPU, GPU = 0, 1


def run(op, dev, frames, args=None, **kw):
    blob = msgpack.packb(args) if args else b""
    return _core.op_kernel_test(op, dev, blob, list(frames), **kw)


def rand_frames(n, h, w, c, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, c)).astype(np.uint8) for _ in range(n)]


# ----------------------------------------------------------------- Histogram

HIST_SHAPES = [(1, 1, 3), (5, 7, 3), (13, 17, 3), (16, 16, 3)]
HIST_BATCHES = [1, 3, 16]
HIST_CASES = [(s, b, p) for s in HIST_SHAPES for b in HIST_BATCHES
              for p in (True, False)]


def hist_contents(shape, batch):
    """random / one constant (one bin holds h*w) / a constant per frame."""
    h, w, c = shape
    return {
        "random": rand_frames(batch, h, w, c, 11),
        "constant": [np.full(shape, 200, np.uint8) for _ in range(batch)],
        "per-frame": [np.full(shape, 7 + 13 * i, np.uint8)
                      for i in range(batch)],
    }


def hist_of(blob, c):
    return np.frombuffer(blob, np.uint32).reshape(c, 256)


def check_histogram(dev, frames, packed, what):
    c = frames[0].shape[2]
    got = run("Histogram", dev, frames, packed=packed)
    assert len(got) == len(frames)
    for i, (g, f) in enumerate(zip(got, frames)):
        I.assert_exact(hist_of(g, c), I.histogram(f), f"{what} frame {i}")
    return got


# -------------------------------------------------------------------- Resize

RESIZE_SHAPES = [((5, 7), (16, 16)), ((37, 53), (20, 32)),
                 ((64, 96), (32, 48)), ((8, 8), (8, 8)), ((1, 1), (4, 4)),
                 ((9, 9), (1, 1))]
RESIZE_CASES = [(s, d, c) for s, d in RESIZE_SHAPES for c in (1, 3)] + \
    [((3, 420), (420, 420), 3)]   # 529 200 outputs > 2048 * 256


def check_resize(dev, src, dst, c):
    (sh, sw), (dh, dw) = src, dst
    n = 1 if dh * dw > 10000 else 2
    frames = rand_frames(n, sh, sw, c, 5)
    got = run("Resize", dev, frames, {"width": dw, "height": dh})
    worst = -1.0
    for g, f in zip(got, frames):
        assert g.dtype == np.uint8
        worst = max(worst, I.assert_rounded(
            g, I.resize(f, dh, dw), I.delta_resize(sh, sw),
            f"resize {sh}x{sw}->{dh}x{dw} c={c}"))
        if src == dst:
            I.assert_exact(g, f, "identity resize")
    return worst


# ---------------------------------------------------------------------- Blur

BLUR_KS = [1, 2, 3, 5, 7, 9]
BLUR_SHAPES = [(1, 1), (1, 9), (5, 3), (33, 47)]
BLUR_CASES = [(s, c) for s in BLUR_SHAPES for c in (1, 3)]


# A 5x3 frame under ks = 9 is one window: whether floor and nearest differ
# there is a coin toss per channel. With this seed they differ on every
# shape and size (test_seeded_blur requires it).
BLUR_SEED = 2


def check_blur(dev, shape, c, ks_list=BLUR_KS):
    frames = rand_frames(2 if shape[0] * shape[1] < 10000 else 1,
                         shape[0], shape[1], c, BLUR_SEED)
    for ks in ks_list:
        got = run("Blur", dev, frames, {"kernel_size": ks})
        for g, f in zip(got, frames):
            I.assert_exact(g, I.blur(f, ks), f"blur {shape} c={c} ks={ks}")


# -------------------------------------------------------------- ColorConvert

def colour_lattice():
    """The 8 corner colours, every (r,g,b) of a 32-step lattice closed with
    255, and 4096 random pixels: 4833 pixels as 9 x 537 x 3."""
    corners = [(r, g, b) for r in (0, 255) for g in (0, 255)
               for b in (0, 255)]
    steps = list(range(0, 256, 32)) + [255]
    lattice = [(r, g, b) for r in steps for g in steps for b in steps]
    rnd = np.random.RandomState(3).randint(0, 256, (4096, 3))
    px = np.concatenate([np.array(corners), np.array(lattice), rnd])
    assert px.shape == (4833, 3)
    return px.astype(np.uint8).reshape(9, 537, 3)


def colour_frames():
    # 1025 x 1024 > 4096 * 256 pixels: the stride loop takes a second pass
    return {"lattice": colour_lattice(),
            "1025x1024": rand_frames(1, 1025, 1024, 3, 4)[0]}


def check_colour(dev, fmt, frame, what):
    (got,) = run("ColorConvert", dev, [frame], {"format": fmt})
    real = I.gray(frame) if fmt == "gray" else I.yuv(frame)
    return I.assert_rounded(got, real, I.DELTA_COLOR, f"{fmt} {what}")


PLANAR_CASES = [(s, c) for s in ((13, 17), (33, 65)) for c in (1, 3, 4)]


def check_planar(dev, shape, c):
    frames = rand_frames(2, shape[0], shape[1], c, 6)
    got = run("ColorConvert", dev, frames, {"format": "planar"})
    for g, f in zip(got, frames):
        I.assert_exact(g, I.planar(f), f"planar {shape} c={c}")


# (x, y, width, height) on 48 x 64: flush right/bottom, last pixel, whole
CROP_WINDOWS = [(40, 30, 24, 18), (63, 47, 1, 1), (0, 0, 64, 48)]
CROP_REJECTED = [((60, 0, 8, 8), "Crop outside frame bounds"),
                 ((0, 44, 8, 8), "Crop outside frame bounds"),
                 ((-1, 0, 8, 8), "Crop x/y must be >= 0"),
                 ((0, -3, 8, 8), "Crop x/y must be >= 0")]


def crop_args(win):
    return dict(zip(("x", "y", "width", "height"), win))


def check_crop(dev, h, w, c, win):
    frames = rand_frames(2 if h * w < 10000 else 1, h, w, c, 8)
    got = run("Crop", dev, frames, crop_args(win))
    for g, f in zip(got, frames):
        I.assert_exact(g, np.ascontiguousarray(I.crop(f, *win)),
                       f"crop {win} of {h}x{w}x{c}")


# --------------------------------------------------------------- OpticalFlow

def _pair(h, w, c, sigma, seed):
    return F.textured_pair(h, w, dx=2, dy=1, c=c, sigma=sigma, seed=seed)


FLOW_SPECS = {}
for _r in (2, 3, 4):
    for _c in (3, 1):
        # one step from zero flow: LDS tile, gradients, window sums, border
        FLOW_SPECS[f"single-r{_r}-c{_c}"] = dict(
            shape=(40, 56), c=_c, sigma=1.2 + 0.2 * _r, seed=_r,
            params=dict(radius=_r, iters=1, levels=1))
        # second step: fractional warps, interior and clamped paths
        FLOW_SPECS[f"two-r{_r}-c{_c}"] = dict(
            shape=(40, 56), c=_c, sigma=1.2 + 0.2 * _r, seed=10 + _r,
            params=dict(radius=_r, iters=2, levels=1))
for _c in (3, 1):
    # 99x131 -> 49x65 -> 24x32 (w/cw = 131/65); 130x72 -> 65x36
    FLOW_SPECS[f"pyramid-99x131-c{_c}"] = dict(
        shape=(99, 131), c=_c, sigma=1.5, seed=20, params={})
    FLOW_SPECS[f"pyramid-130x72-c{_c}"] = dict(
        shape=(130, 72), c=_c, sigma=2.0, seed=21, params={})
# 178x168 -> 89x84 -> 44x42, run as 36 pairs of 37 buffers (rows per thread)
ROWS_SPEC = dict(shape=(178, 168), c=3, sigma=1.5, seed=30, params={})
FLOW_IDS = list(FLOW_SPECS)


@functools.lru_cache(maxsize=None)
def flow_case(name):
    """FlowCase (float64 reference, E32, tolerance) of a spec, once."""
    spec = FLOW_SPECS[name]
    a, b = _pair(*spec["shape"], spec["c"], spec["sigma"], spec["seed"])
    return F.FlowCase(name, a, b, **spec["params"])


@functools.lru_cache(maxsize=None)
def rows_cases():
    a, b = _pair(*ROWS_SPEC["shape"], ROWS_SPEC["c"], ROWS_SPEC["sigma"],
                 ROWS_SPEC["seed"])
    return F.FlowCase("rows-AB", a, b), F.FlowCase("rows-BA", b, a)


def run_flow(dev, frames, params, **kw):
    return run("OpticalFlow", dev, frames, params or None, stencil=[0, 1],
               **kw)


def check_flow(dev, name):
    case = flow_case(name)
    (got,) = run_flow(dev, [case.f0, case.f1], case.params)
    return case.check(got)


def check_flow_rows(dev, what=""):
    """37 frames A,B,A,... in 37 buffers, 36 pairs in one call. On the GPU
    the launch rule gives 2 rows per thread at 178x168 and 89x84 (89 rows:
    the last block's second half-tile is partly outside) and 1 at 44x42;
    with SCANNER_LK_PY=4, 4 and 2. 37*178*168 pixels > 4096*256."""
    ab, ba = rows_cases()
    frames = [(ab.f0 if i % 2 == 0 else ab.f1).copy() for i in range(37)]
    got = run_flow(dev, frames, None, packed=False)
    assert len(got) == 36
    worst = 0.0
    for i, g in enumerate(got):
        case = ab if i % 2 == 0 else ba
        worst = max(worst, case.check(g, f"{what} pair {i}"))
        assert np.array_equal(g.view(np.uint32), got[i % 2].view(np.uint32)), \
            f"pair {i} differs from pair {i % 2} on the same frames"
    return worst


def check_flow_exact(dev):
    a, _ = _pair(40, 56, 3, 1.5, 40)
    c0 = np.full((40, 56, 3), 90, np.uint8)
    c1 = np.full((40, 56, 3), 140, np.uint8)
    (got,) = run_flow(dev, [c0, c1], None)
    assert got.shape == (40, 56, 2) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), np.zeros_like(got, np.uint32)), \
        "constant frames: flow must be +0 everywhere"
    (got,) = run_flow(dev, [a, a.copy()], None)
    assert np.all(got == 0), "a frame against itself: flow must be +-0"


# ----------------------------------------------------------------- FlowStats

STATS_SHAPES = [(3, 5), (16, 16), (130, 72)]   # 9360 px > 32 * 256


def stats_flows(shape, batch, seed=0):
    rng = np.random.RandomState(seed)
    return [(rng.standard_normal(shape + (2,)) * (1 + i)).astype(np.float32)
            for i in range(batch)]


def stats_of(blob):
    return np.frombuffer(blob, np.float32)


def check_flowstats(dev, flows, what, **kw):
    got = run("FlowStats", dev, flows, **kw)
    assert len(got) == len(flows)
    for i, (g, f) in enumerate(zip(got, flows)):
        F.assert_flowstats(stats_of(g), f, f"{what} frame {i}")
