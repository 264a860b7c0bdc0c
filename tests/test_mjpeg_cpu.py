"""Motion-JPEG as a video codec, on the CPU: ingest, load, sampling, the
host sink, argument handling, mp4 in and out, and the host reference of the
restart-segment index against jpeg_parse."""
import io

import msgpack
import numpy as np
import pytest
from PIL import Image

import scanner_amd as sp
from scanner_amd import _core

import mjpeg_cases as mc


def items_of(sc, name):
    info = sc._db.table_info(name)
    return [_core.read_video_item(sc._db, name, info["columns"][0][0], i)
            for i in range(len(info["end_rows"]))]


def samples_of(sc, name):
    out = []
    for data, meta in items_of(sc, name):
        for o, s in zip(meta["sample_offsets"], meta["sample_sizes"]):
            out.append(data[o:o + s])
    return out


# ---------------- ingest ----------------

@pytest.mark.parametrize("ss", mc.SUBSAMPLINGS)
@pytest.mark.parametrize("shape", mc.SHAPES)
def test_ingest_samples_are_the_encoders_files(sc, shape, ss):
    h, w, c = shape
    fr = mc.frames(5, h, w, c, seed=h)
    video = sp.NamedVideoStream(sc, "v", frames=fr, codec="mjpeg",
                                quality=80, subsampling=ss)
    (data, meta), = items_of(sc, "v")
    assert meta["codec"] == "mjpeg"
    assert (meta["height"], meta["width"], meta["channels"]) == shape
    assert meta["num_frames"] == 5
    assert meta["keyframe_indices"] == list(range(5))
    files = [_core.jpeg_cpu_encode(f, 80, ss) for f in fr]
    assert meta["sample_sizes"] == [len(f) for f in files]
    assert meta["sample_offsets"] == \
        [sum(len(f) for f in files[:i]) for i in range(5)]
    assert data == b"".join(files)
    loaded = list(video.load())
    for got, f in zip(loaded, files):
        np.testing.assert_array_equal(got, _core.jpeg_cpu_decode(f))
    got = list(video.load(rows=[3, 1]))
    assert len(got) == 2


def test_ingest_default_is_420_quality_90(sc):
    fr = mc.frames(2, 16, 272, 3)
    sp.NamedVideoStream(sc, "v", frames=fr, codec="mjpeg")
    assert samples_of(sc, "v") == \
        [_core.jpeg_cpu_encode(f, 90, "420") for f in fr]


def test_ingest_items(sc):
    fr = mc.frames(10, 16, 272, 3)
    video = sp.NamedVideoStream(sc, "v", frames=fr, codec="mjpeg",
                                io_packet_size=4)
    items = items_of(sc, "v")
    assert [m["num_frames"] for _, m in items] == [4, 4, 2]
    assert all(m["sample_offsets"][0] == 0 for _, m in items)
    assert len(list(video.load())) == 10


def test_ingest_videos_passes_options(sc):
    fr = mc.frames(2, 8, 264, 1)
    streams, failures = sp.storage.ingest_videos(
        sc, [("a", fr)], codec="mjpeg", quality=55, subsampling="444")
    assert not failures
    assert samples_of(sc, "a") == \
        [_core.jpeg_cpu_encode(f, 55, "444") for f in fr]


# ---------------- sampling ----------------

def hist_of(frame):
    return np.stack([np.bincount(frame[:, :, c].ravel(), minlength=256)
                     for c in range(frame.shape[2])]).astype(np.uint32)


@pytest.mark.parametrize("sampling", ["all", "stride", "gather"])
def test_input_histogram(sc, sampling):
    fr = mc.frames(10, 40, 520, 3, seed=4)
    video = sp.NamedVideoStream(sc, "v", frames=fr, codec="mjpeg",
                                io_packet_size=4)
    decoded = list(video.load())
    frame = sc.io.Input([video])
    if sampling == "all":
        rows, col = list(range(10)), sc.streams.All(frame)
    elif sampling == "stride":
        rows, col = list(range(0, 10, 3)), sc.streams.Stride(frame, [3])
    else:
        rows, col = [9, 0, 4], sc.streams.Gather(frame, [[9, 0, 4]])
    hist = sc.ops.Histogram(frame=col)
    out = sp.NamedStream(sc, "h")
    prof = sc.run(sc.io.Output([hist], [out]), sp.PerfParams.manual(4, 4),
                  cache_mode=sp.CacheMode.Overwrite)
    got = [np.frombuffer(r, np.uint32).reshape(3, 256) for r in out.load()]
    assert len(got) == len(rows)
    for g, r in zip(got, rows):
        np.testing.assert_array_equal(g, hist_of(decoded[r]))
    # per-frame random access: only the wanted frames are decoded
    assert prof.counters()["decoded_frames"] == len(rows)


# ---------------- sink ----------------

@sp.register_python_op(name="MjpegCpuInvert")
def mjpeg_cpu_invert(frame: sp.FrameType) -> sp.FrameType:
    return 255 - frame


@pytest.mark.parametrize("ss", mc.SUBSAMPLINGS)
def test_cpu_sink_equals_ingest(sc, ss):
    fr = mc.frames(10, 16, 272, 3, seed=6)
    src = sp.NamedVideoStream(sc, "src", frames=fr, codec="raw")
    inv = sc.ops.MjpegCpuInvert(frame=sc.io.Input([src]))
    inv.compress_video(codec="mjpeg", quality=70, subsampling=ss)
    out = sp.NamedStream(sc, "sunk")
    sc.run(sc.io.Output(inv, [out]), sp.PerfParams.manual(4, 4),
           cache_mode=sp.CacheMode.Overwrite)
    sp.NamedVideoStream(sc, "ingested", frames=255 - fr, codec="mjpeg",
                        quality=70, subsampling=ss, io_packet_size=4)
    assert items_of(sc, "sunk") == items_of(sc, "ingested")


# ---------------- arguments ----------------

def test_ingest_rejections(sc):
    fr = mc.frames(2, 8, 8, 1)
    with pytest.raises(Exception, match="quality"):
        sp.NamedVideoStream(sc, "a", frames=fr, codec="mjpeg", quality=0)
    with pytest.raises(Exception, match="subsampling"):
        sp.NamedVideoStream(sc, "b", frames=fr, codec="mjpeg",
                            subsampling="422")
    with pytest.raises(Exception, match="1- or 3-channel"):
        sp.NamedVideoStream(sc, "c", frames=mc.frames(2, 8, 8, 3)[..., :2],
                            codec="mjpeg")
    with pytest.raises(Exception, match="unknown option 'quality'"):
        sp.NamedVideoStream(sc, "d", frames=fr, codec="svc", quality=50)
    with pytest.raises(Exception, match="unknown codec 'mpeg9'"):
        sp.NamedVideoStream(sc, "e", frames=fr, codec="mpeg9")


def test_compress_video_rejections(sc):
    fr = mc.frames(2, 8, 8, 1)
    src = sp.NamedVideoStream(sc, "src", frames=fr, codec="raw")
    frame = sc.io.Input([src])
    with pytest.raises(sp.ScannerException, match="unknown option 'bitrate'"):
        frame.compress_video(codec="mjpeg", bitrate=5)
    with pytest.raises(sp.ScannerException, match="unknown option 'quality'"):
        frame.compress_video(quality=5)
    with pytest.raises(sp.ScannerException, match="unknown sink codec 'h265'"):
        frame.compress_video(codec="h265")
    with pytest.raises(sp.ScannerException, match="quality"):
        frame.compress_video(codec="mjpeg", quality=101)
    with pytest.raises(sp.ScannerException, match="subsampling"):
        frame.compress_video(codec="mjpeg", subsampling="411")


def output_args(sc, annotate):
    src = sp.NamedVideoStream(sc, "src")
    frame = sc.io.Input([src])
    annotate(frame)
    return sc.io.Output(frame, [sp.NamedStream(sc, "o")])._args


def test_output_args(sc):
    sp.NamedVideoStream(sc, "src", frames=mc.frames(1, 8, 8, 1), codec="raw")
    # compress_video() and lossless() are what they were: this literal is
    # the msgpack of the Output args before the mjpeg codec existed
    literal = b"\x81\xa8compress\x81\xa5frame\xa3svc"
    for annotate in (lambda f: f.compress_video(), lambda f: f.lossless()):
        args = output_args(sc, annotate)
        assert msgpack.packb(args) == literal
    args = output_args(sc, lambda f: f.compress_video(codec="mjpeg"))
    assert args == {"compress": {"frame": "mjpeg"}}
    args = output_args(sc, lambda f: f.compress_video(
        codec="mjpeg", quality=75, subsampling="444"))
    assert args == {"compress": {"frame": "mjpeg"},
                    "compress_opts": {"frame": {"quality": 75,
                                                "subsampling": "444"}}}


@sp.register_python_op(name="MjpegCpuToFloat")
def mjpeg_cpu_to_float(frame: sp.FrameType) -> sp.FrameType:
    return frame.astype(np.float32)


@sp.register_python_op(name="MjpegCpuGrow")
def mjpeg_cpu_grow(frame: sp.FrameType) -> sp.FrameType:
    n = 8 + 8 * int(frame[0, 0, 0] > 100)
    return np.zeros((n, 8, 1), np.uint8)


def run_sink(sc, col, **kw):
    col.compress_video(codec="mjpeg", **kw)
    sc.run(sc.io.Output(col, [sp.NamedStream(sc, "o")]),
           sp.PerfParams.manual(4, 4), cache_mode=sp.CacheMode.Overwrite)


def test_sink_rejections(sc):
    fr = mc.frames(4, 8, 8, 1)
    fr[2:] = 200
    src = sp.NamedVideoStream(sc, "src", frames=fr, codec="raw")
    with pytest.raises(Exception, match="mjpeg compression needs u8 frames"):
        run_sink(sc, sc.ops.MjpegCpuToFloat(frame=sc.io.Input([src])))
    with pytest.raises(Exception, match="uniform frame shapes"):
        run_sink(sc, sc.ops.MjpegCpuGrow(frame=sc.io.Input([src])))
    with pytest.raises(Exception, match="null rows"):
        frame = sc.io.Input([src])
        run_sink(sc, sc.streams.RepeatNull(frame, [2]))
    two = sp.NamedVideoStream(sc, "two", frames=np.zeros((2, 8, 8, 2),
                                                         np.uint8),
                              codec="raw")
    with pytest.raises(Exception, match="1- or 3-channel"):
        run_sink(sc, sc.io.Input([two]))
    # the executor checks the options again: hand it what Python refuses
    frame = sc.io.Input([src])
    frame.compress_video(codec="mjpeg")
    frame.op._compress["frame"]["bitrate"] = 5
    with pytest.raises(Exception,
                       match="unknown option 'bitrate' for sink codec "
                             "'mjpeg'"):
        sc.run(sc.io.Output(frame, [sp.NamedStream(sc, "o")]),
               sp.PerfParams.manual(4, 4), cache_mode=sp.CacheMode.Overwrite)


def test_other_codecs_still_fail_by_name(sc, tmp_path):
    fr = mc.frames(2, 8, 8, 1)
    svc = sp.NamedVideoStream(sc, "svc", frames=fr, codec="svc")
    with pytest.raises(Exception, match="h264"):
        svc.save_mp4(str(tmp_path / "x.mp4"))


# ---------------- mp4 ----------------

@pytest.mark.parametrize("ss", mc.SUBSAMPLINGS)
def test_save_mp4_and_reingest(sc, tmp_path, ss):
    fr = mc.frames(7, 40, 520, 3, seed=8)
    video = sp.NamedVideoStream(sc, "v", frames=fr, codec="mjpeg",
                                quality=85, subsampling=ss, io_packet_size=3)
    path = video.save_mp4(str(tmp_path / "v.mp4"), fps=25.0)
    buf = open(path, "rb").read()
    kind, w, h, esds, has_stss, samples = mc.demux_mp4(buf)
    assert (kind, w, h, has_stss) == (b"mp4v", 520, 40, False)
    # ES_Descriptor -> DecoderConfigDescriptor (OTI 0x6C, visual, no
    # DecoderSpecificInfo) -> SLConfigDescriptor 0x02
    assert esds == bytes([0, 0, 0, 0, 0x03, 21, 0, 1, 0, 0x04, 13, 0x6c,
                          0x11]) + b"\x00" * 11 + bytes([0x06, 1, 0x02])
    assert samples == samples_of(sc, "v")
    for s, got in zip(samples, video.load()):
        img = Image.open(io.BytesIO(s))
        img.load()
        assert img.size == (520, 40) and img.mode == "RGB"
        np.testing.assert_array_equal(got, _core.jpeg_cpu_decode(s))
    again = sp.NamedVideoStream(sc, "again", path=path)
    (data, meta), = items_of(sc, "again")
    assert meta["codec"] == "mjpeg" and meta["num_frames"] == 7
    assert samples_of(sc, "again") == samples
    for a, b in zip(again.load(), video.load()):
        np.testing.assert_array_equal(a, b)
    probe = _core.mp4_probe(buf)
    assert probe["codec"] == "mjpeg" and probe["timescale"] == 90000


PILLOW_SETS = {
    "422": dict(quality=85, subsampling=1),
    "optimised": dict(quality=75, subsampling=2, optimize=True),
    "restart": dict(quality=90, subsampling=0, restart_marker_blocks=4),
}


@pytest.mark.parametrize("entry,ext", [("jpeg", ".mov"), ("mp4v", ".mp4")])
@pytest.mark.parametrize("kind", sorted(PILLOW_SETS))
def test_ingest_pillow_files(sc, tmp_path, kind, entry, ext):
    fr = mc.frames(5, 40, 520, 3, seed=10, noise=48)
    samples = [mc.pillow_jpeg(f, **PILLOW_SETS[kind]) for f in fr]
    if kind == "optimised":
        assert len({s[:mc.scan_start(s)] for s in samples}) > 1
    path = tmp_path / ("p" + ext)
    path.write_bytes(mc.mux_mp4(samples, 520, 40, entry=entry, chunk=2))
    video = sp.NamedVideoStream(sc, "p", path=str(path))
    assert samples_of(sc, "p") == samples
    (_, meta), = items_of(sc, "p")
    assert (meta["codec"], meta["height"], meta["width"],
            meta["channels"]) == ("mjpeg", 40, 520, 3)
    for got, s in zip(video.load(), samples):
        np.testing.assert_array_equal(got, _core.jpeg_cpu_decode(s))
    # and through the engine
    hist = sc.ops.Histogram(frame=sc.io.Input([video]))
    out = sp.NamedStream(sc, "ph")
    sc.run(sc.io.Output([hist], [out]), sp.PerfParams.manual(4, 4),
           cache_mode=sp.CacheMode.Overwrite)
    for r, s in zip(out.load(), samples):
        np.testing.assert_array_equal(
            np.frombuffer(r, np.uint32).reshape(3, 256),
            hist_of(_core.jpeg_cpu_decode(s)))


def test_ingest_rejects_by_sample_index(sc, tmp_path):
    fr = mc.frames(4, 16, 272, 3)
    good = [mc.pillow_jpeg(f, quality=80) for f in fr]
    mixed = list(good)
    mixed[2] = mc.pillow_jpeg(mc.frames(1, 16, 264, 3)[0], quality=80)
    path = tmp_path / "mixed.mp4"
    path.write_bytes(mc.mux_mp4(mixed, 272, 16, entry="mp4v"))
    with pytest.raises(Exception, match=r"sample 2: .*differs from sample 0"):
        sp.NamedVideoStream(sc, "m", path=str(path))
    prog = list(good)
    prog[3] = mc.pillow_jpeg(fr[3], quality=80, progressive=True)
    path = tmp_path / "prog.mov"
    path.write_bytes(mc.mux_mp4(prog, 272, 16, entry="jpeg"))
    with pytest.raises(Exception, match=r"sample 3: .*progressive"):
        sp.NamedVideoStream(sc, "g", path=str(path))
    other = tmp_path / "mpeg4.mp4"
    other.write_bytes(mc.mux_mp4(good, 272, 16, entry="mp4v", oti=0x20))
    with pytest.raises(Exception, match="objectTypeIndication is 0x20"):
        sp.NamedVideoStream(sc, "o", path=str(other))


# ---------------- index reference ----------------

def index_cases():
    for shape in mc.SHAPES + [(64, 2080, 1)]:
        for ss in mc.SUBSAMPLINGS:
            h, w, c = shape
            yield [_core.jpeg_cpu_encode(f, 90, ss)
                   for f in mc.frames(2, h, w, c, seed=w)]
    yield [_core.jpeg_cpu_encode(f, 100, "444")
           for f in mc.noise_frames(2, 40, 520, 3, seed=5)]
    fr = mc.frames(2, 40, 520, 3, seed=10, noise=48)
    yield [mc.pillow_jpeg(f, quality=90, subsampling=0,
                          restart_marker_blocks=4) for f in fr]
    yield [mc.pillow_jpeg(f, quality=85, subsampling=1,
                          restart_marker_rows=1) for f in fr]


@pytest.mark.parametrize("samples", list(index_cases()))
def test_index_ref_equals_jpeg_parse(samples):
    info = _core.mjpeg_header_info(samples[0])
    assert info["has_dri"]
    stream, offs, sizes = mc.layout(samples, lead=3, gap=2)
    segs, status = _core.mjpeg_index_ref(stream, offs, sizes,
                                         info["header_len"], info["nseg"])
    assert status.tolist() == [0] * len(samples)
    for i, s in enumerate(samples):
        want = [(b + offs[i], e + offs[i], f, m)
                for b, e, f, m in _core.jpeg_decode_info(s)["segments"]]
        assert [tuple(r) for r in segs[i].tolist()] == want


def test_index_ref_refuses_what_jpeg_parse_refuses():
    good = _core.jpeg_cpu_encode(mc.frames(1, 16, 272, 3, seed=3)[0], 90,
                                 "444")
    info = _core.mjpeg_header_info(good)
    L = info["header_len"]
    rst = [i for i in range(L, len(good) - 1)
           if good[i] == 0xff and 0xd0 <= good[i + 1] <= 0xd7]
    bad = [good[:-10], good[:-1],
           good[:rst[0] + 1] + b"\xd3" + good[rst[0] + 2:],
           good[:rst[1] + 2] + b"\x55\xff\xd2" + good[rst[1] + 2:],
           good[:rst[1]] + good[rst[1] + 2:],
           good[:-2] + b"\xff\xda",
           good[:L + 4] + b"\xff\xd9"]
    stream, offs, sizes = mc.layout([good] + bad)
    _, status = _core.mjpeg_index_ref(stream, offs, sizes, L, info["nseg"])
    assert status.tolist() == [0, 2, 2, 4, 5, 5, 3, 5]
    for b in bad:
        with pytest.raises(Exception):
            _core.jpeg_decode_info(b)
