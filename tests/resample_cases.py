"""The cases of the filtered-Resize tests, written once and run on either
device through `_core.op_kernel_test`: test_resize_filters_cpu.py holds the
CPU kernel to them, test_resize_filters_gpu.py the HIP kernels of
kernels/resample.hip. The reference and the bound are in resample_ref.py.
"""
import functools
import io
import os

import msgpack
import numpy as np
from PIL import Image

import image_ref as I
import resample_ref as R
from scanner_amd import _core

CPU, GPU = 0, 1
FILTERS = R.FILTERS

# source -> destination, h x w
SHAPES = [
    ((37, 53), (20, 32)),     # a fractional downscale
    ((64, 96), (9, 13)),      # 42 taps with lanczos3
    ((130, 70), (8, 5)),      # about 100 taps
    ((5, 7), (16, 16)),       # an upscale where edge taps clip
    ((33, 47), (32, 46)),     # near identity
    ((8, 8), (8, 8)),         # must equal the input
    ((1, 1), (4, 4)),
    ((9, 9), (1, 1)),
    ((3, 1500), (2, 700)),    # a row longer than any LDS stage
    ((3, 420), (420, 420)),   # more outputs than one grid pass, batch of 1
]
CHANNELS = [1, 3, 4]
CASES = [(s, d, c) for s, d in SHAPES for c in CHANNELS]
PILLOW_SHAPES = SHAPES[:7]
PILLOW_CASES = [(s, d, c) for s, d in PILLOW_SHAPES for c in CHANNELS]
CONSTANTS = [0, 77, 255]

# 13 x 17 x 3 frames are 663 bytes: packed, every second one starts odd
LAYOUT_SHAPE, LAYOUT_DST = (13, 17, 3), (9, 11)
LAYOUT_CASES = [(b, p) for b in (1, 3, 17) for p in (True, False)]
# 17 frames leave each 2048 // 17 = 120 workgroups; 1200 x 8 -> 600 x 4 has
# 150 horizontal tiles of 8 rows: the tile loop of that pass takes a second
# round (no listed shape has that many rows)
STRIDE_CASE = ((1200, 8), (600, 4), 1, 17)

FIT_CASES = [((48, 64), (32, 32), (24, 32)), ((64, 48), (32, 32), (32, 24)),
             ((1, 100), (32, 32), (1, 32)), ((100, 1), (32, 32), (32, 1)),
             ((10, 10), (7, 32), (7, 7))]


def run(dev, frames, args, **kw):
    return _core.op_kernel_test("Resize", dev, msgpack.packb(args),
                                list(frames), **kw)


def resize_args(dst, flt=None, **kw):
    args = {"width": dst[1], "height": dst[0]}
    if flt is not None:
        args["filter"] = flt
    args.update(kw)
    return args


@functools.lru_cache(maxsize=None)
def content(kind, h, w, c, n=1, seed=0):
    """n frames: "random" 0..255, "bw" 0 or 255 per sample (cubic and
    lanczos3 overshoot both ends, so the final clamp works), "mid" random in
    [64, 191] (no overshoot past [0, 255]: Pillow's u8 intermediate is then
    only a rounding), or a constant."""
    rng = np.random.RandomState(1000 * seed + 10 * h + w + c)
    if kind == "random":
        fr = rng.randint(0, 256, (n, h, w, c))
    elif kind == "bw":
        fr = rng.randint(0, 2, (n, h, w, c)) * 255
    elif kind == "mid":
        fr = rng.randint(64, 192, (n, h, w, c))
    else:
        fr = np.full((n, h, w, c), int(kind))
    fr = fr.astype(np.uint8)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def reference(flt, kind, src, dst, c):
    """float64 result of frame 0 of content(kind, ...), computed once."""
    out = R.resample(content(kind, src[0], src[1], c)[0], dst[0], dst[1], flt)
    out.setflags(write=False)
    return out


def check_filter(dev, flt, src, dst, c):
    """random and black/white noise within 0.5 + delta of the float64
    reference, constants and a same-size resize exact. Returns the outputs
    by content (for the byte comparison of the two devices) and the worst
    excess over a correct rounding."""
    delta = R.delta(flt, *src, *dst)
    assert delta <= 1.0 / 16, f"{flt} {src}->{dst}: derived delta {delta}"
    outs, worst = {}, -1.0
    for kind in ["random", "bw"] + [str(k) for k in CONSTANTS]:
        frame = content(kind, src[0], src[1], c)[0]
        (got,) = run(dev, [frame], resize_args(dst, flt))
        assert got.dtype == np.uint8 and got.shape == dst + (c,)
        what = f"{flt} {src}->{dst} c={c} {kind}"
        if kind in ("random", "bw"):
            worst = max(worst, I.assert_rounded(
                got, reference(flt, kind, src, dst, c), delta, what))
        else:
            I.assert_exact(got, np.full(dst + (c,), int(kind), np.uint8), what)
        if src == dst:
            I.assert_exact(got, frame, what + " same size")
        outs[kind] = got
    return outs, worst


def check_nearest(dev, src, dst, c):
    frame = content("random", src[0], src[1], c)[0]
    (got,) = run(dev, [frame], resize_args(dst, "nearest"))
    I.assert_exact(got, R.nearest(frame, *dst), f"nearest {src}->{dst} c={c}")
    return got


PIL_FILTER = {"box": Image.Resampling.BOX,
              "triangle": Image.Resampling.BILINEAR,
              "cubic": Image.Resampling.BICUBIC,
              "lanczos3": Image.Resampling.LANCZOS}


@functools.lru_cache(maxsize=None)
def pillow(flt, kind, src, dst, c):
    """Pillow's resize of frame 0, channel by channel (as "L" images: an
    RGBA image would be premultiplied by its alpha)."""
    frame = content(kind, src[0], src[1], c)[0]
    chans = [np.asarray(Image.fromarray(np.ascontiguousarray(frame[:, :, k]))
                        .resize((dst[1], dst[0]), PIL_FILTER[flt]))
             for k in range(c)]
    return np.stack(chans, -1)


def check_pillow(dev, flt, src, dst, c):
    """At most 1 per sample: our half unit, Pillow's half-unit intermediate
    rounding times sum |w| <= 1.56, Pillow's final half unit: below 2."""
    kind = "random" if flt in ("box", "triangle") else "mid"
    frame = content(kind, src[0], src[1], c)[0]
    (got,) = run(dev, [frame], resize_args(dst, flt))
    diff = np.abs(got.astype(int) - pillow(flt, kind, src, dst, c).astype(int))
    print(f"pillow {flt} {src}->{dst} c={c}: max diff {diff.max()}")
    assert diff.max() <= 1, f"{flt} {src}->{dst} c={c}: {diff.max()}"
    return int(diff.max())


def check_layout(dev, flt, batch, packed):
    """Packed frames start at odd addresses; 17 is one more than the
    preferred batch. Every frame must equal the one-frame result."""
    h, w, c = LAYOUT_SHAPE
    frames = list(content("random", h, w, c, n=batch, seed=3))
    got = run(dev, frames, resize_args(LAYOUT_DST, flt), packed=packed)
    assert len(got) == batch
    for i, (g, f) in enumerate(zip(got, frames)):
        (alone,) = run(dev, [f], resize_args(LAYOUT_DST, flt), packed=False)
        I.assert_exact(g, alone, f"{flt} x{batch} packed={packed} frame {i}")
    return got


def check_fit(dev, flt, src, box, want, c=3):
    """preserve_aspect gives the size of the integer rule and the pixels of a
    plain resize to that size."""
    assert R.fit(*src, *box) == want
    frame = content("random", src[0], src[1], c)[0]
    (got,) = run(dev, [frame], resize_args(box, flt, preserve_aspect=True))
    assert got.shape == want + (c,), (got.shape, want)
    (plain,) = run(dev, [frame], resize_args(want, flt))
    I.assert_exact(got, plain, f"fit {flt} {src} into {box}")
    return got


def check_memory(dev):
    """Repeated calls, a change of geometry and a rejected argument among
    them, leave the allocators where the first round left them."""
    import pytest
    frames = list(content("random", 13, 17, 3, n=4, seed=4))
    other = list(content("random", 37, 53, 3, n=2, seed=4))

    def calls():
        for flt in FILTERS + ["nearest"]:
            run(dev, frames, resize_args((9, 11), flt))
            run(dev, other, resize_args((20, 32), flt), packed=False)
            run(dev, frames, resize_args((32, 32), flt, preserve_aspect=True))
        with pytest.raises(Exception, match="Resize filter must be one of"):
            run(dev, frames, resize_args((9, 11), "gaussian"))

    def stats():    # the host allocator, and the device's where there is one
        return [_core.mem_stats(d) for d in ([-1, 0] if dev == GPU else [-1])]

    calls()     # the peak settles
    before = stats()
    calls()
    assert stats() == before


# ------------------------------------------------------------------ pipeline

PIPE_SIZES = [(48, 64), (50, 30)]
PIPE_BOX = (32, 32)


def pipeline_frames():
    return [content("random", h, w, 3, seed=7)[0] for h, w in PIPE_SIZES]


def png_bytes(frame):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "PNG")
    return buf.getvalue()


def check_pipeline(sc, tmp_path, dev):
    """Files -> ImageDecoder -> Resize(preserve_aspect, lanczos3) ->
    ImageEncoder(png) -> Files on PNGs of two sizes in one column: each
    output has its own fitted shape and the kernel test's pixels."""
    import scanner_amd as sp
    gpu = dev == GPU
    device = sp.DeviceType.GPU if gpu else sp.DeviceType.CPU
    frames = pipeline_frames()
    paths = []
    for i, f in enumerate(frames):
        p = os.path.join(str(tmp_path), f"in_{i}.png")
        with open(p, "wb") as fh:
            fh.write(png_bytes(f))
        paths.append(p)
    img = sc.sources.Files(paths)
    dec = sc.ops.ImageDecoder(img=img, device=device)
    small = sc.ops.Resize(frame=dec, width=PIPE_BOX[1], height=PIPE_BOX[0],
                          filter="lanczos3", preserve_aspect=True,
                          device=device)
    # PNG is encoded on the host on either device (docs/ops.md)
    enc = sc.ops.ImageEncoder(frame=small, format="png")
    out_dir = os.path.join(str(tmp_path), "out")
    os.makedirs(out_dir)
    sc.run(sc.sinks.Files(enc, out_dir, ext="png"),
           sp.PerfParams.manual(4, 8), cache_mode=sp.CacheMode.Overwrite,
           **({"gpu_ids": [0]} if gpu else {}))
    for i, f in enumerate(frames):
        got = np.asarray(Image.open(os.path.join(out_dir, f"c0_{i}.png")))
        want_hw = R.fit(f.shape[0], f.shape[1], *PIPE_BOX)
        assert got.shape == want_hw + (3,), (i, got.shape)
        (kernel,) = run(dev, [f], resize_args(want_hw, "lanczos3"))
        I.assert_exact(got, kernel, f"pipeline frame {i}")
