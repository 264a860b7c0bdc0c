"""4:2:0 mode of the CPU JPEG encoder (csrc/ops/jpeg_cpu.cpp, jpeg_common.h)
and the ImageEncoder op's subsampling="420". Pillow (libjpeg) is the
independent decoder, scipy's float64 DCT the arithmetic reference. The shapes
and the oracle defined here are reused by test_jpeg420_gpu.py."""
import functools
import io
import struct

import numpy as np
import pytest
from PIL import Image
from scipy.fft import dctn

import scanner_amd as sp
from scanner_amd import _core
from conftest import make_video
from test_jpeg_cpu import ZIGZAG, decode, image, psnr, segments

R420 = 16  # MCUs per restart segment: 96 blocks, as 4:4:4 with R = 32

# (H, W, 3): the smallest shape at which each mechanism can break
SHAPES = [
    (1, 1, 3),      # one MCU, all replication
    (16, 16, 3),    # exactly one MCU, no padding
    (17, 15, 3),    # two MCU rows; odd width and height, so the last chroma
                    # cell averages replicated pixels; 45-byte row stride
    (8, 24, 3),     # half-height MCUs: the lower Y blocks are replication
    (16, 256, 3),   # exactly one full segment
    (185, 170, 3),  # 11 x 12 = 132 MCUs: 9 segments, the last partial;
                    # segments straddle MCU rows; the RST index wraps
]
CONTENTS = ["smooth", "noise", "constant", "basis63", "checker"]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def cpu_jpeg420(shape, content, quality, seed=0):
    """The oracle's bytes, computed once per case."""
    return _core.jpeg_cpu_encode(image(shape, content, seed), quality,
                                 subsampling="420")


def nmcu(shape):
    return -(-shape[0] // 16) * -(-shape[1] // 16)


def sof0_sampling(blob):
    """[(component id, h factor, v factor)] of the SOF0 segment."""
    (p,) = [p for m, p in segments(blob)[0] if m == 0xc0]
    return [(p[6 + 3 * i], p[7 + 3 * i] >> 4, p[7 + 3 * i] & 15)
            for i in range(p[5])]


# ---------------- independent decoder ----------------

@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_pillow_decodes(shape, content):
    h, w, c = shape
    for q in (1, 50, 100):
        blob = cpu_jpeg420(shape, content, q)
        im = decode(blob)
        assert im.format == "JPEG"
        assert im.mode == "RGB"
        assert im.size == (w, h)
        assert sof0_sampling(blob) == [(1, 2, 2), (2, 1, 1), (3, 1, 1)]
        assert [(l[1], l[2]) for l in im.layer] == [(2, 2), (1, 1), (1, 1)]
        assert len(blob) <= _core.jpeg_size_bound(h, w, c, "420")
        assert len(blob) <= _core.jpeg_size_bound(h, w, c, subsampling="420")


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_own_decoder_reads_it(shape, content):
    h, w, c = shape
    blob = cpu_jpeg420(shape, content, 50)
    info = _core.jpeg_decode_info(blob)
    assert info["hs"] == info["vs"] == 2
    assert info["restart_interval"] == R420
    assert (info["h"], info["w"], info["c"]) == shape
    out = _core.jpeg_cpu_decode(blob)
    assert out.shape == shape and out.dtype == np.uint8


def test_size_bound_is_six_blocks_per_mcu():
    for shape in SHAPES:
        h, w, c = shape
        blob = cpu_jpeg420(shape, "constant", 50)
        header = len(blob) - len(segments(blob)[1]) - 2
        nseg = -(-nmcu(shape) // R420)
        assert _core.jpeg_size_bound(h, w, c, "420") == \
            header + nmcu(shape) * 6 * 416 + 2 * nseg
    assert _core.jpeg_restart_interval("420") == R420
    assert _core.jpeg_restart_interval(subsampling="444") == 32
    assert _core.jpeg_restart_interval() == 32


# ---------------- format mechanics ----------------

@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_restart_segments(shape, content):
    for q in (1, 100):
        head, scan = segments(cpu_jpeg420(shape, content, q))
        dri = [p for m, p in head if m == 0xdd]
        assert dri == [struct.pack(">H", R420)]
        rst, i = [], 0
        while i < len(scan):
            if scan[i] == 0xff:
                nxt = scan[i + 1]
                assert nxt == 0 or 0xd0 <= nxt <= 0xd7, hex(nxt)
                if nxt:
                    rst.append(nxt - 0xd0)
                i += 2
            else:
                i += 1
        assert len(rst) + 1 == -(-nmcu(shape) // R420)
        assert rst == [k % 8 for k in range(len(rst))]
    assert -(-nmcu((185, 170, 3)) // R420) == 9


# ---------------- arithmetic ----------------

def float_coefficients_420(frame, quant):
    """round()-free float64 reference of jpeg_quantize_cpu(subsampling="420"):
    edge-pad to a multiple of 16, JFIF colour conversion, 2x2 mean of Cb/Cr,
    -128, orthonormal 8x8 DCT, / q. Returns Y [by, bx, 64] and chroma
    [2, by, bx, 64] in zig-zag order. quant: Pillow's im.quantization."""
    h, w, _ = frame.shape
    f = np.pad(frame.astype(np.float64),
               ((0, -h % 16), (0, -w % 16), (0, 0)), mode="edge")
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb = 128 - 0.168736 * r - 0.331264 * g + 0.5 * b
    cr = 128 + 0.5 * r - 0.418688 * g - 0.081312 * b

    def mean2(p):
        return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] +
                p[1::2, 1::2]) / 4

    def blocks(plane, table):
        # Pillow lists a table in natural (row-major) order
        q = np.array(quant[table], np.float64)[ZIGZAG]
        out = np.zeros((plane.shape[0] // 8, plane.shape[1] // 8, 64))
        for by in range(out.shape[0]):
            for bx in range(out.shape[1]):
                blk = plane[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] - 128
                out[by, bx] = dctn(blk, norm="ortho").ravel()[ZIGZAG] / q
        return out

    return blocks(y, 0), np.stack([blocks(mean2(cb), 1),
                                   blocks(mean2(cr), 1)])


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_coefficients_within_one_of_float_reference(shape, content):
    """The bound of the 4:4:4 test: a value within half a unit before
    rounding can only land on a neighbouring integer."""
    frame = image(shape, content)
    got_y, got_c = _core.jpeg_quantize_cpu(frame, 100, subsampling="420")
    quant = decode(cpu_jpeg420(shape, content, 100)).quantization
    want_y, want_c = (np.round(a)
                      for a in float_coefficients_420(frame, quant))
    for name, got, want in (("Y", got_y, want_y), ("chroma", got_c, want_c)):
        assert got.shape == want.shape and got.dtype == np.int16, name
        diff = np.abs(got - want).max()
        print(f"{name}: max |coefficient - round(float64)| =", diff)
        assert diff <= 1, name


def pillow_jpeg420(frame, quality):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=quality, subsampling=2,
                                optimize=False)
    return buf.getvalue()


# Gap = Pillow's PSNR (subsampling=2) - ours for the same input and tables,
# measured with this file on the CPU path (profiles/jpeg_encode.md):
#   smooth q50 -0.022 dB, smooth q90 +0.008 dB,
#   noise  q50 +0.001 dB, noise  q90 -0.001 dB
# margin = largest gap + 0.1 dB
PSNR_MARGIN_DB = 0.008 + 0.1


@pytest.mark.parametrize("quality", [50, 90])
@pytest.mark.parametrize("content", ["smooth", "noise"])
def test_psnr_close_to_pillow(content, quality):
    shape = (64, 96, 3)
    frame = image(shape, content)
    ours = np.asarray(decode(cpu_jpeg420(shape, content, quality)))
    blob = pillow_jpeg420(frame, quality)
    assert [(l[1], l[2]) for l in decode(blob).layer][0] == (2, 2)
    ref = np.asarray(decode(blob))
    p_ours, p_ref = psnr(ours, frame), psnr(ref, frame)
    print(f"{content} q{quality}: ours {p_ours:.3f} dB, Pillow {p_ref:.3f} "
          f"dB, gap {p_ref - p_ours:+.3f} dB")
    assert p_ours >= p_ref - PSNR_MARGIN_DB


@pytest.mark.parametrize("content", ["smooth", "noise"])
def test_file_is_smaller_than_444(content):
    shape = (64, 96, 3)
    small = cpu_jpeg420(shape, content, 90)
    full = _core.jpeg_cpu_encode(image(shape, content), 90)
    print(f"{content}: 4:2:0 {len(small)} B, 4:4:4 {len(full)} B")
    assert len(small) < len(full)


# ---------------- grey, default, bad values ----------------

@pytest.mark.parametrize("shape", [(16, 24, 1), (1, 1, 1)])
def test_grey_is_unchanged_by_420(shape):
    h, w, c = shape
    for content in ("smooth", "noise"):
        f = image(shape, content)
        assert _core.jpeg_cpu_encode(f, 75, subsampling="420") == \
            _core.jpeg_cpu_encode(f, 75, subsampling="444")
        np.testing.assert_array_equal(
            _core.jpeg_quantize_cpu(f, 75, subsampling="420"),
            _core.jpeg_quantize_cpu(f, 75))
    assert _core.jpeg_size_bound(h, w, c, "420") == \
        _core.jpeg_size_bound(h, w, c)


def test_default_is_444():
    for shape in ((17, 15, 3), (16, 24, 1)):
        f = image(shape, "noise")
        for q in (50, 90):
            assert _core.jpeg_cpu_encode(f, q) == \
                _core.jpeg_cpu_encode(f, q, subsampling="444")
            assert _core.jpeg_cpu_encode(f, q) == \
                _core.jpeg_cpu_encode(f, q, "444")
        np.testing.assert_array_equal(
            _core.jpeg_quantize_cpu(f, 90),
            _core.jpeg_quantize_cpu(f, 90, subsampling="444"))
        h, w, c = shape
        assert _core.jpeg_size_bound(h, w, c) == \
            _core.jpeg_size_bound(h, w, c, "444")


@pytest.mark.parametrize("value", ["422", "411", ""])
def test_binding_rejects_other_values(value):
    f = np.zeros((16, 16, 3), np.uint8)
    for call in (lambda: _core.jpeg_cpu_encode(f, 90, subsampling=value),
                 lambda: _core.jpeg_quantize_cpu(f, 90, subsampling=value),
                 lambda: _core.jpeg_size_bound(16, 16, 3, value),
                 lambda: _core.jpeg_restart_interval(value),
                 lambda: _core.jpeg_gpu_encode(f[None], 90,
                                               subsampling=value)):
        with pytest.raises(Exception, match="subsampling") as e:
            call()
        assert "'444'" in str(e.value) and "'420'" in str(e.value)


# ---------------- op level ----------------

def test_pipeline_resize_to_jpeg420(sc):
    frames = make_video(n=5, h=48, w=64)
    video = sp.NamedVideoStream(sc, "jpg420_in", frames=frames, codec="raw")
    frame = sc.io.Input([video])
    small = sc.ops.Resize(frame=frame, width=40, height=27)
    enc = sc.ops.ImageEncoder(frame=small, format="jpg", quality=80,
                              subsampling="420")
    out = sp.NamedStream(sc, "jpg420_out")
    sc.run(sc.io.Output([enc, small], [out]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite)
    rows = list(sp.NamedStream(sc, "jpg420_out", column="img").load())
    resized = list(sp.NamedVideoStream(sc, "jpg420_out",
                                       column="frame").load())
    assert len(rows) == 5
    for blob, small_frame in zip(rows, resized):
        im = decode(blob)
        assert (im.format, im.mode, im.size) == ("JPEG", "RGB", (40, 27))
        assert blob == _core.jpeg_cpu_encode(small_frame, 80,
                                             subsampling="420")
        assert blob != _core.jpeg_cpu_encode(small_frame, 80)


@pytest.mark.parametrize("value", ["422", "411", ""])
def test_bad_op_subsampling_raises_at_construction(sc, value):
    frames = make_video(n=2, h=16, w=16)
    video = sp.NamedVideoStream(sc, "jpg420_bad", frames=frames, codec="raw")
    enc = sc.ops.ImageEncoder(frame=sc.io.Input([video]), format="jpg",
                              subsampling=value)
    out = sp.NamedStream(sc, "jpg420_bad_out")
    with pytest.raises(Exception, match="subsampling"):
        sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite)


def test_png_ignores_subsampling(sc):
    frames = make_video(n=2, h=16, w=16)
    video = sp.NamedVideoStream(sc, "png420_in", frames=frames, codec="raw")
    rows = {}
    for name, args in (("plain", {}), ("s420", dict(subsampling="420")),
                       ("s_bad", dict(subsampling="422"))):
        enc = sc.ops.ImageEncoder(frame=sc.io.Input([video]), format="png",
                                  **args)
        out = sp.NamedStream(sc, "png420_" + name)
        sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite)
        rows[name] = list(out.load())
    assert rows["plain"] == rows["s420"] == rows["s_bad"]
