"""CPU still-image decoders (csrc/ops/jpeg_decode_cpu.cpp, png_decode.cpp,
jpeg_decode_common.h) and the ImageDecoder op on the CPU. Pillow (libjpeg)
is the independent encoder and decoder, scipy's float64 IDCT the arithmetic
reference. The helpers defined here are reused by test_image_decode_gpu.py."""
import functools
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image
from scipy.fft import idctn

import scanner_amd as sp
from scanner_amd import _core, register_python_op
from test_jpeg_cpu import CONTENTS, SHAPES, SHAPE_IDS, cpu_jpeg, image, segments

PILLOW_SHAPES = [(1, 1, 1), (8, 8, 1), (33, 50, 1),
                 (7, 9, 3), (16, 24, 3), (17, 33, 3), (40, 56, 3)]
PILLOW_IDS = ["x".join(map(str, s)) for s in PILLOW_SHAPES]
PILLOW_CONTENTS = ["smooth", "noise", "checker"]

# max |ours - Pillow| per sample. A float64 decoder built from the same
# formulas differs from Pillow by at most 1 (grey) and 3 (RGB); the integer
# IDCT adds at most 1 per plane sample, so the hard caps are 2 and 6. The
# integer decoder measures 1 (grey) and 3 (RGB, all three samplings) on the
# list below and on our own encoder's files (profiles/jpeg_decode.md); the
# bounds are those maxima + 1.
BOUND_GREY = 1 + 1
BOUND_RGB = 3 + 1
assert BOUND_GREY <= 2 and BOUND_RGB <= 6


def pillow_save(frame, fmt="JPEG", **kw):
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(
        buf, fmt, **kw)
    return buf.getvalue()


def pillow_decode(blob):
    a = np.asarray(Image.open(io.BytesIO(blob)))
    return a[..., None] if a.ndim == 2 else a


@functools.lru_cache(maxsize=None)
def pillow_jpeg(shape, content, quality, subsampling=0, variant="plain",
                seed=0):
    kw = dict(quality=quality)
    if shape[2] == 3:
        kw["subsampling"] = subsampling
    if variant == "rst3_opt":
        kw.update(restart_marker_blocks=3, optimize=True)
    elif variant == "rst2":
        kw.update(restart_marker_blocks=2)
    elif variant == "rst1":
        kw.update(restart_marker_blocks=1)
    elif variant == "rows1_opt":
        kw.update(restart_marker_rows=1, optimize=True)
    elif variant == "rows1":
        kw.update(restart_marker_rows=1)
    else:
        assert variant == "plain"
    return pillow_save(image(shape, content, seed), **kw)


def max_diff(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


# ---------------- IDCT ----------------

def idct_reference(blocks):
    out = [np.clip(np.round(idctn(b.reshape(8, 8).astype(np.float64),
                                  norm="ortho") + 128), 0, 255)
           for b in blocks]
    return np.stack(out).reshape(-1, 64).astype(np.int32)


def idct_cases():
    rs = np.random.RandomState(1180)
    sparse = np.where(rs.rand(500, 64) < 0.1,
                      rs.randint(-20, 21, (500, 64)), 0)
    dense = rs.randint(-300, 301, (500, 64))
    dc = np.zeros((2, 64), np.int64)
    dc[0, 0], dc[1, 0] = -1024, 1016  # every sample 0 / every sample 255
    hf = np.zeros((2, 64), np.int64)
    hf[0, 63], hf[1, 63] = 400, -400  # a single (7,7) coefficient
    return {"sparse": sparse, "dense": dense, "dc_extremes": dc,
            "basis63": hf}


@pytest.mark.parametrize("name", ["sparse", "dense", "dc_extremes",
                                  "basis63"])
def test_idct_within_one_of_float_reference(name):
    """IEEE 1180 peak-error criterion against
    clip(round(idctn(coefs, norm="ortho") + 128), 0, 255) in float64."""
    blocks = idct_cases()[name]
    got = _core.jpeg_idct_blocks(blocks.astype(np.int32)).astype(np.int32)
    want = idct_reference(blocks)
    diff = np.abs(got - want).max()
    print(f"{name}: max |idct - float64 reference| = {diff}")
    assert diff <= 1
    if name == "dc_extremes":
        assert (got[0] == 0).all() and (got[1] == 255).all()


# ---------------- against Pillow's decode of the same file ----------------

@pytest.mark.parametrize("variant", ["plain", "rst3_opt"])
@pytest.mark.parametrize("content", PILLOW_CONTENTS)
@pytest.mark.parametrize("shape", PILLOW_SHAPES, ids=PILLOW_IDS)
def test_matches_pillow_decode(shape, content, variant):
    worst = 0
    for q in (30, 75, 95, 100):
        for sub in ((0, 1, 2) if shape[2] == 3 else (0,)):
            blob = pillow_jpeg(shape, content, q, sub, variant)
            info = _core.jpeg_decode_info(blob)
            assert (info["h"], info["w"], info["c"]) == shape
            if shape[2] == 3:
                assert (info["hs"], info["vs"]) == [(1, 1), (2, 1),
                                                    (2, 2)][sub]
            assert (info["restart_interval"] != 0) == (variant != "plain")
            d = max_diff(_core.jpeg_cpu_decode(blob), pillow_decode(blob))
            worst = max(worst, d)
            assert d <= (BOUND_GREY if shape[2] == 1 else BOUND_RGB), (q, sub)
    print(f"{shape} {content} {variant}: max |ours - Pillow| = {worst}")


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_own_encoder_round_trip(shape, content):
    for q in (1, 50, 90, 100):
        blob = cpu_jpeg(shape, content, q)
        got = _core.jpeg_cpu_decode(blob)
        assert got.shape == shape
        d = max_diff(got, pillow_decode(blob))
        assert d <= (BOUND_GREY if shape[2] == 1 else BOUND_RGB), q
    R = _core.jpeg_restart_interval()
    info = _core.jpeg_decode_info(cpu_jpeg(shape, content, 50))
    assert info["restart_interval"] == R
    assert len(info["segments"]) == -(-info["mcus"] // R)
    assert [s[2] for s in info["segments"]] == \
        list(range(0, info["mcus"], R))


def test_image_cpu_decode_dispatches_on_magic():
    f = image((16, 24, 3), "smooth")
    jpg, png = pillow_save(f, quality=90), pillow_save(f, "PNG")
    np.testing.assert_array_equal(_core.image_cpu_decode(jpg),
                                  _core.jpeg_cpu_decode(jpg))
    np.testing.assert_array_equal(_core.image_cpu_decode(png), f)
    with pytest.raises(Exception, match="unknown image format"):
        _core.image_cpu_decode(b"GIF89a" + bytes(64))


def test_dqt_16_bit_precision_gives_the_same_pixels():
    blob = pillow_jpeg((17, 33, 3), "noise", 75, 2)
    out, pos = bytearray(blob[:2]), 2
    rewritten = 0
    while True:
        marker = blob[pos + 1]
        (ln,) = struct.unpack(">H", blob[pos + 2:pos + 4])
        payload = blob[pos + 4:pos + 2 + ln]
        if marker == 0xdb:
            wide = bytearray()
            while payload:
                assert payload[0] >> 4 == 0
                wide.append(0x10 | payload[0])
                for v in payload[1:65]:
                    wide += struct.pack(">H", v)
                payload = payload[65:]
                rewritten += 1
            payload = bytes(wide)
        out += b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2)
        out += payload
        pos += 2 + ln
        if marker == 0xda:
            break
    out += blob[pos:]
    assert rewritten == 2 and len(out) == len(blob) + 128
    np.testing.assert_array_equal(_core.jpeg_cpu_decode(bytes(out)),
                                  _core.jpeg_cpu_decode(blob))


# ---------------- PNG ----------------

def png_chunk(typ, data):
    body = typ + data
    return struct.pack(">I", len(data)) + body + \
        struct.pack(">I", zlib.crc32(body))


def build_png(raw, w, h, ctype, depth=8, interlace=0, idat_pieces=1,
              extra=b""):
    ihdr = struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)
    comp = zlib.compress(raw, 6)
    step = -(-len(comp) // idat_pieces)
    idat = b"".join(png_chunk(b"IDAT", comp[i:i + step])
                    for i in range(0, len(comp), step))
    return (b"\x89PNG\r\n\x1a\x0a" + png_chunk(b"IHDR", ihdr) + extra + idat +
            png_chunk(b"IEND", b""))


def png_filter_rows(frame, ftype):
    """Scanlines of `frame` with filter `ftype` applied (PNG spec 9.2)."""
    h, w, c = frame.shape
    rows = frame.reshape(h, w * c).astype(np.int32)
    out = b""
    for y in range(h):
        cur = rows[y]
        up = rows[y - 1] if y else np.zeros_like(cur)
        left = np.concatenate([np.zeros(c, np.int32), cur[:-c]])
        upleft = np.concatenate([np.zeros(c, np.int32), up[:-c]])
        if ftype == 0:
            pred = np.zeros_like(cur)
        elif ftype == 1:
            pred = left
        elif ftype == 2:
            pred = up
        elif ftype == 3:
            pred = (left + up) // 2
        else:
            p = left + up - upleft
            pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left,
                            np.where(pb <= pc, up, upleft))
        out += bytes([ftype]) + ((cur - pred) % 256).astype(np.uint8).tobytes()
    return out


@pytest.mark.parametrize("mode", ["L", "RGB", "RGBA"])
@pytest.mark.parametrize("hw", [(1, 1), (7, 9), (33, 50)])
def test_png_pillow_files_decode_exactly(hw, mode):
    c = {"L": 1, "RGB": 3, "RGBA": 4}[mode]
    frame = np.random.RandomState(c).randint(0, 256, hw + (c,)).astype(
        np.uint8)
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if c == 1 else frame, mode).save(buf, "PNG")
    got = _core.png_cpu_decode(buf.getvalue())
    np.testing.assert_array_equal(got, frame[..., :3] if c == 4 else frame)


@pytest.mark.parametrize("ftype", [0, 1, 2, 3, 4])
def test_png_each_filter_and_several_idat_chunks(ftype):
    for c, ctype in ((1, 0), (3, 2), (4, 6)):
        frame = image((33, 50, 3), "noise", seed=ftype)
        if c == 1:
            frame = frame[..., :1]
        elif c == 4:
            frame = np.concatenate([frame, frame[..., :1]], -1)
        frame = np.ascontiguousarray(frame)
        raw = png_filter_rows(frame, ftype)
        for pieces in (1, 5):
            blob = build_png(raw, 50, 33, ctype, idat_pieces=pieces)
            assert blob.count(b"IDAT") >= pieces
            np.testing.assert_array_equal(pillow_decode(blob)[..., :3]
                                          if c == 4 else pillow_decode(blob),
                                          frame[..., :3] if c == 4 else frame)
            np.testing.assert_array_equal(_core.png_cpu_decode(blob),
                                          frame[..., :3] if c == 4 else frame)


def test_png_rejections_name_the_cause():
    frame = image((7, 9, 3), "noise")
    raw = png_filter_rows(frame, 0)
    good = build_png(raw, 9, 7, 2)
    np.testing.assert_array_equal(_core.png_cpu_decode(good), frame)
    pal = build_png(png_filter_rows(frame[..., :1], 0), 9, 7, 3,
                    extra=png_chunk(b"PLTE", bytes(768)))
    with pytest.raises(Exception, match="palette"):
        _core.png_cpu_decode(pal)
    with pytest.raises(Exception, match="16-bit"):
        _core.png_cpu_decode(build_png(raw + raw, 9, 7, 2, depth=16))
    with pytest.raises(Exception, match="interlaced"):
        _core.png_cpu_decode(build_png(raw, 9, 7, 2, interlace=1))
    bad = bytearray(good)
    bad[-20] ^= 1  # inside the IDAT payload
    with pytest.raises(Exception, match="CRC"):
        _core.png_cpu_decode(bytes(bad))
    with pytest.raises(Exception, match="truncated"):
        _core.png_cpu_decode(good[:-12])  # no IEND
    with pytest.raises(Exception, match="filter type"):
        _core.png_cpu_decode(build_png(b"\x07" + raw[1:], 9, 7, 2))
    with pytest.raises(Exception, match="does not inflate"):
        _core.png_cpu_decode(build_png(raw[:-5], 9, 7, 2))


# ---------------- JPEG rejections ----------------

def test_progressive_is_rejected():
    blob = pillow_save(image((16, 24, 3), "smooth"), quality=80,
                       progressive=True)
    with pytest.raises(Exception, match="progressive"):
        _core.jpeg_cpu_decode(blob)
    with pytest.raises(Exception, match="progressive"):
        _core.jpeg_decode_info(blob)


def test_four_components_are_rejected():
    cmyk = Image.fromarray(image((16, 24, 3), "smooth")).convert("CMYK")
    buf = io.BytesIO()
    cmyk.save(buf, "JPEG", quality=80)
    with pytest.raises(Exception, match="4-component"):
        _core.jpeg_cpu_decode(buf.getvalue())


def test_twelve_bit_and_bad_sampling_are_rejected():
    blob = bytearray(pillow_jpeg((16, 24, 3), "smooth", 75, 0))
    sof = blob.index(b"\xff\xc0")
    twelve = bytearray(blob)
    twelve[sof + 4] = 12
    with pytest.raises(Exception, match="12-bit"):
        _core.jpeg_cpu_decode(bytes(twelve))
    odd = bytearray(blob)
    odd[sof + 11] = 0x12  # luma 1x2
    with pytest.raises(Exception, match="sampling factors"):
        _core.jpeg_cpu_decode(bytes(odd))


def test_truncation_at_every_marker_is_rejected():
    """Cutting the file at each marker, and in the middle of each segment,
    raises with 'truncated' (or, with nothing but SOI left, any message)."""
    for blob in (pillow_jpeg((17, 33, 3), "noise", 75, 2, "rst3_opt"),
                 cpu_jpeg((16, 24, 3), "noise", 90)):
        head, _ = segments(blob)
        pos, cuts = 2, [2]
        for marker, payload in head:
            cuts += [pos + 2, pos + 3, pos + 4 + len(payload) // 2,
                     pos + 4 + len(payload)]
            pos += 4 + len(payload)
        cuts += [pos + 1, (pos + len(blob)) // 2, len(blob) - 2,
                 len(blob) - 1]
        for cut in cuts:
            with pytest.raises(Exception, match="truncated|marker expected"):
                _core.jpeg_cpu_decode(blob[:cut])
        _core.jpeg_cpu_decode(blob)


def test_restart_markers_out_of_sequence_are_rejected():
    blob = bytearray(cpu_jpeg((136, 128, 1), "noise", 50))
    i = blob.index(b"\xff\xd1")
    blob[i + 1] = 0xd2
    with pytest.raises(Exception, match="out of sequence"):
        _core.jpeg_cpu_decode(bytes(blob))


# ---------------- op ----------------

@register_python_op(name="ImageDecodePackFrame")
def pack_frame(frame: sp.FrameType) -> bytes:
    """Shape and pixels of one frame as bytes: a table's frame column
    stores one shape per task, these tests mix shapes. A null row stays
    null."""
    if frame is None:
        return None
    return struct.pack("<3i", *frame.shape) + frame.tobytes()


def unpack_frame(blob):
    h, w, c = struct.unpack("<3i", blob[:12])
    return np.frombuffer(blob[12:], np.uint8).reshape(h, w, c)


def mixed_files():
    """JPEG (with and without DRI, three samplings, grey) and PNG files of
    different shapes."""
    return [
        pillow_jpeg((17, 33, 3), "smooth", 75, 2),
        pillow_save(image((7, 9, 3), "noise"), "PNG"),
        pillow_jpeg((16, 24, 3), "noise", 95, 1, "rst3_opt"),
        cpu_jpeg((8, 8, 1), "checker", 50),
        pillow_save(image((33, 50, 1), "smooth"), "PNG"),
        pillow_jpeg((40, 56, 3), "checker", 30, 0, "rows1_opt"),
        pillow_jpeg((33, 50, 1), "noise", 75),
    ]


def write_files(tmp_path, blobs):
    paths = []
    for i, b in enumerate(blobs):
        p = tmp_path / f"img{i}.bin"
        p.write_bytes(b)
        paths.append(str(p))
    return paths


def test_op_files_to_frames_mixed_formats_shapes_and_a_null_row(sc, tmp_path):
    blobs = mixed_files()
    col = sc.sources.Files(write_files(tmp_path, blobs))
    spaced = sc.streams.RepeatNull(col, [2])
    frames = sc.ops.ImageDecoder(img=spaced)
    packed = sc.ops.ImageDecodePackFrame(frame=frames)
    out = sp.NamedStream(sc, "imgdec_cpu_out")
    sc.run(sc.io.Output(packed, [out]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite)
    rows = list(out.load())
    assert len(rows) == 2 * len(blobs)
    assert all(r is None for r in rows[1::2])
    for blob, row in zip(blobs, rows[0::2]):
        np.testing.assert_array_equal(unpack_frame(row),
                                      _core.image_cpu_decode(blob))


def test_op_uniform_shape_into_a_frame_column(sc, tmp_path):
    """Files -> ImageDecoder -> frame table."""
    blobs = [pillow_jpeg((40, 56, 3), "smooth", 90, 2, "plain", seed)
             for seed in range(5)]
    col = sc.sources.Files(write_files(tmp_path, blobs))
    frames = sc.ops.ImageDecoder(img=col)
    out = sp.NamedVideoStream(sc, "imgdec_cpu_frames")
    sc.run(sc.io.Output(frames, [out]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite)
    got = list(sp.NamedVideoStream(sc, "imgdec_cpu_frames",
                                   column="frame").load())
    assert len(got) == 5
    for blob, f in zip(blobs, got):
        np.testing.assert_array_equal(f, _core.jpeg_cpu_decode(blob))


def test_op_names_the_corrupt_row(sc, tmp_path):
    blobs = [pillow_jpeg((16, 24, 3), "smooth", 75, 0),
             pillow_save(image((16, 24, 3), "smooth"), quality=75,
                         progressive=True)]
    col = sc.sources.Files(write_files(tmp_path, blobs))
    frames = sc.ops.ImageDecoder(img=col)
    out = sp.NamedVideoStream(sc, "imgdec_cpu_bad")
    with pytest.raises(Exception, match="row 1 .*progressive"):
        sc.run(sc.io.Output(frames, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite)
