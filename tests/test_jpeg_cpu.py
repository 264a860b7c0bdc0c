"""CPU baseline JPEG encoder (csrc/ops/jpeg_cpu.cpp, jpeg_common.h) and the
ImageEncoder op's format="jpg". Pillow (libjpeg) is the independent decoder,
scipy's float64 DCT the arithmetic reference. The shapes and contents defined
here are reused by test_jpeg_gpu.py."""
import functools
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image
from scipy.fft import dctn, idctn

import scanner_amd as sp
from scanner_amd import _core
from conftest import make_video

R = _core.jpeg_restart_interval()

# (H, W, C): the smallest shape at which each mechanism can break
SHAPES = [
    (1, 1, 1),           # one block, all padding
    (8, 8, 1),           # exactly one block, no padding
    (7, 9, 3),           # two blocks, both edges replicated, odd row stride
    (16, 24, 3),         # 6 MCUs, one short segment
    (8, 8 * R, 1),       # exactly one full segment
    (136, 4 * R, 1),     # 8.5 R MCUs: 9 segments, the last partial, so the
                         # RST index wraps
]
CONTENTS = ["smooth", "noise", "constant", "basis63", "checker"]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


@functools.lru_cache(maxsize=None)
def image(shape, content, seed=0):
    """Deterministic test image; `seed` varies the frames of a batch."""
    h, w, c = shape
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "smooth":
        f = np.stack([(2 * xx + yy + 5 * seed) % 256, (3 * yy + seed) % 256,
                      ((xx + 2 * yy) // 2 + 3 * seed) % 256], -1)[..., :c]
    elif content == "noise":
        f = np.random.RandomState(100 + seed).randint(0, 256, (h, w, c))
    elif content == "constant":
        f = np.full((h, w, c), (77 + 60 * seed) % 256)
    elif content == "basis63":
        # every block is the inverse DCT of a single (7,7) coefficient + 128
        coef = np.zeros((8, 8))
        coef[7, 7] = 400 - 20 * (seed % 5)
        block = np.round(idctn(coef, norm="ortho") + 128)
        f = np.tile(block, ((h + 7) // 8, (w + 7) // 8))[:h, :w, None]
        f = np.repeat(f, c, axis=2)
    else:  # black / white 8x8 checker: maximum DC differences
        f = ((((yy // 8) + (xx // 8) + seed) % 2) * 255)[..., None]
        f = np.repeat(f, c, axis=2)
    f = np.ascontiguousarray(f.astype(np.uint8))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def cpu_jpeg(shape, content, quality, seed=0):
    """The oracle's bytes, computed once per case."""
    return _core.jpeg_cpu_encode(image(shape, content, seed), quality)


def pillow_jpeg(frame, quality):
    buf = io.BytesIO()
    im = Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame)
    im.save(buf, "JPEG", quality=quality, subsampling=0, optimize=False)
    return buf.getvalue()


def decode(blob):
    im = Image.open(io.BytesIO(blob))
    im.load()
    return im


def segments(blob):
    """Marker segments before the scan as [(marker, payload)], the entropy
    coded data and what follows it."""
    assert blob[:2] == b"\xff\xd8"
    pos, out = 2, []
    while True:
        assert blob[pos] == 0xff
        marker = blob[pos + 1]
        (ln,) = struct.unpack(">H", blob[pos + 2:pos + 4])
        out.append((marker, blob[pos + 4:pos + 2 + ln]))
        pos += 2 + ln
        if marker == 0xda:
            break
    assert blob[-2:] == b"\xff\xd9"
    return out, blob[pos:-2]


def huffman_tables(blob):
    tabs = {}
    for marker, p in segments(blob)[0]:
        if marker != 0xc4:
            continue
        while p:
            n = sum(p[1:17])
            tabs[p[0]] = (bytes(p[1:17]), bytes(p[17:17 + n]))
            p = p[17 + n:]
    return tabs


def float_coefficients(frame, quant):
    """round()-free float64 reference of jpeg_quantize_cpu: JFIF colour
    conversion, -128, orthonormal 8x8 DCT, / q; [ncomp, by, bx, 64] in
    zig-zag order. quant: Pillow's im.quantization of the same file."""
    h, w, c = frame.shape
    f = np.pad(frame.astype(np.float64),
               ((0, -h % 8), (0, -w % 8), (0, 0)), mode="edge")
    if c == 3:
        r, g, b = f[..., 0], f[..., 1], f[..., 2]
        comps = [0.299 * r + 0.587 * g + 0.114 * b,
                 128 - 0.168736 * r - 0.331264 * g + 0.5 * b,
                 128 + 0.5 * r - 0.418688 * g - 0.081312 * b]
    else:
        comps = [f[..., 0]]
    out = np.zeros((c, f.shape[0] // 8, f.shape[1] // 8, 64))
    for k, comp in enumerate(comps):
        # Pillow lists a table in natural (row-major) order
        q = np.array(quant[0 if k == 0 else 1], np.float64)[ZIGZAG]
        for by in range(out.shape[1]):
            for bx in range(out.shape[2]):
                blk = comp[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] - 128
                out[k, by, bx] = dctn(blk, norm="ortho").ravel()[ZIGZAG] / q
    return out


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / np.mean(d * d))


# ---------------- independent decoder ----------------

@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_pillow_decodes(shape, content):
    h, w, c = shape
    frame = image(shape, content)
    for q in (1, 50, 90, 100):
        blob = cpu_jpeg(shape, content, q)
        im = decode(blob)
        assert im.format == "JPEG"
        assert im.size == (w, h)
        assert im.mode == ("L" if c == 1 else "RGB")
        ref = decode(pillow_jpeg(frame, q))
        assert im.quantization == ref.quantization, q
        assert len(blob) <= _core.jpeg_size_bound(h, w, c)


def test_huffman_tables_are_annex_k():
    """Our DHT segments carry the tables libjpeg writes when it does not
    optimise them."""
    for shape in ((8, 8, 1), (16, 24, 3)):
        frame = image(shape, "noise")
        ours = huffman_tables(cpu_jpeg(shape, "noise", 90))
        assert ours == huffman_tables(pillow_jpeg(frame, 90))
        assert sorted(ours) == ([0x00, 0x10] if shape[2] == 1
                                else [0x00, 0x01, 0x10, 0x11])


# ---------------- arithmetic ----------------

@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_coefficients_within_one_of_float_reference(shape, content):
    """A value within half a unit before rounding can only land on a
    neighbouring integer, so the bound is exactly 1."""
    frame = image(shape, content)
    got = _core.jpeg_quantize_cpu(frame, 100)
    quant = decode(cpu_jpeg(shape, content, 100)).quantization
    want = np.round(float_coefficients(frame, quant))
    assert got.shape == want.shape and got.dtype == np.int16
    diff = np.abs(got - want).max()
    print("max |coefficient - round(float64)| =", diff)
    assert diff <= 1


# Gap = Pillow's PSNR - ours for the same input and tables, measured with
# this file on the CPU path (profiles/jpeg_encode.md):
#   smooth q50 -0.018 dB, smooth q90 -0.049 dB,
#   noise  q50 +0.013 dB, noise  q90 -0.022 dB
# margin = largest gap + 0.1 dB
PSNR_MARGIN_DB = 0.013 + 0.1


@pytest.mark.parametrize("quality", [50, 90])
@pytest.mark.parametrize("content", ["smooth", "noise"])
def test_psnr_close_to_pillow(content, quality):
    shape = (64, 96, 3)
    frame = image(shape, content)
    ours = np.asarray(decode(cpu_jpeg(shape, content, quality)))
    ref = np.asarray(decode(pillow_jpeg(frame, quality)))
    p_ours, p_ref = psnr(ours, frame), psnr(ref, frame)
    print(f"{content} q{quality}: ours {p_ours:.3f} dB, Pillow {p_ref:.3f} "
          f"dB, gap {p_ref - p_ours:+.3f} dB")
    assert p_ours >= p_ref - PSNR_MARGIN_DB


# ---------------- format mechanics ----------------

@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_restart_segments(shape, content):
    h, w, c = shape
    nmcu = ((h + 7) // 8) * ((w + 7) // 8)
    for q in (1, 100):
        head, scan = segments(cpu_jpeg(shape, content, q))
        dri = [p for m, p in head if m == 0xdd]
        assert dri == [struct.pack(">H", R)]
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
        assert len(rst) + 1 == -(-nmcu // R)
        assert rst == [k % 8 for k in range(len(rst))]


def test_noise_at_q100_is_stuffed_and_within_bound():
    shape = (136, 4 * R, 1)
    blob = cpu_jpeg(shape, "noise", 100)
    _, scan = segments(blob)
    assert b"\xff\x00" in scan
    assert len(blob) <= _core.jpeg_size_bound(*shape)


def test_size_bound_covers_header_and_worst_case_blocks():
    for h, w, c in SHAPES:
        nmcu = ((h + 7) // 8) * ((w + 7) // 8)
        header = len(cpu_jpeg((h, w, c), "constant", 50)) - \
            len(segments(cpu_jpeg((h, w, c), "constant", 50))[1]) - 2
        # DC 9+11 bits, 63 x (16+10) bits -> 208 bytes, doubled by stuffing
        assert _core.jpeg_size_bound(h, w, c) >= header + nmcu * c * 416 + 2


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 8],
                         ids=[i for s, i in zip(SHAPES, SHAPE_IDS)
                              if s[0] >= 8])
def test_basis63_triggers_zrl(shape):
    zz = _core.jpeg_quantize_cpu(image(shape, "basis63"), 50)[0, 0, 0]
    assert zz[63] != 0
    nonzero = np.flatnonzero(zz[:63])
    last = nonzero[-1] if len(nonzero) else 0
    assert 63 - last - 1 >= 16
    decode(cpu_jpeg(shape, "basis63", 50))


def test_rejects_bad_arguments():
    f = np.zeros((8, 8, 3), np.uint8)
    for q in (0, 101):
        with pytest.raises(Exception, match="quality"):
            _core.jpeg_cpu_encode(f, q)
    with pytest.raises(Exception, match="1- or 3-channel"):
        _core.jpeg_cpu_encode(np.zeros((8, 8, 2), np.uint8), 90)


# ---------------- op level ----------------

def test_pipeline_resize_to_jpeg(sc):
    frames = make_video(n=5, h=48, w=64)
    video = sp.NamedVideoStream(sc, "jpg_in", frames=frames, codec="raw")
    frame = sc.io.Input([video])
    small = sc.ops.Resize(frame=frame, width=40, height=27)
    enc = sc.ops.ImageEncoder(frame=small, format="jpg", quality=80)
    out = sp.NamedStream(sc, "jpg_out")
    sc.run(sc.io.Output([enc, small], [out]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite)
    rows = list(sp.NamedStream(sc, "jpg_out", column="img").load())
    resized = list(sp.NamedVideoStream(sc, "jpg_out", column="frame").load())
    assert len(rows) == 5
    for blob, small_frame in zip(rows, resized):
        im = decode(blob)
        assert (im.format, im.mode, im.size) == ("JPEG", "RGB", (40, 27))
        assert blob == _core.jpeg_cpu_encode(small_frame, 80)


@pytest.mark.parametrize("args, message", [
    (dict(format="jpg", quality=0), "quality"),
    (dict(format="jpeg", quality=101), "quality"),
    (dict(format="bmp"), "format"),
])
def test_bad_op_arguments_raise_at_construction(sc, args, message):
    frames = make_video(n=2, h=16, w=16)
    video = sp.NamedVideoStream(sc, "jpg_bad", frames=frames, codec="raw")
    enc = sc.ops.ImageEncoder(frame=sc.io.Input([video]), **args)
    out = sp.NamedStream(sc, "jpg_bad_out")
    with pytest.raises(Exception, match=message):
        sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite)


def expected_png(frame):
    """The PNG writer's bytes: filter-0 scanlines, zlib level 6, one IDAT."""
    h, w, c = frame.shape

    def chunk(typ, data):
        body = typ + data
        return struct.pack(">I", len(data)) + body + \
            struct.pack(">I", zlib.crc32(body))

    raw = b"".join(b"\x00" + frame[y].tobytes() for y in range(h))
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0)
    return (b"\x89PNG\r\n\x1a\x0a" + chunk(b"IHDR", ihdr) +
            chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def test_png_output_unchanged_and_ignores_quality(sc):
    from test_engine_cpu import decode_png_filter0
    frames = make_video(n=3, h=24, w=32)
    video = sp.NamedVideoStream(sc, "png_q", frames=frames, codec="raw")
    rows = {}
    for name, args in (("plain", {}), ("q", dict(quality=5)),
                       ("q_bad", dict(quality=0))):
        enc = sc.ops.ImageEncoder(frame=sc.io.Input([video]), format="png",
                                  **args)
        out = sp.NamedStream(sc, "png_q_" + name)
        sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite)
        rows[name] = list(out.load())
    assert rows["plain"] == rows["q"] == rows["q_bad"]
    for blob, frame in zip(rows["plain"], frames):
        np.testing.assert_array_equal(decode_png_filter0(blob), frame)
        assert blob == expected_png(frame)
