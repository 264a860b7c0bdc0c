"""Motion-JPEG on the GPU: the device-side restart-segment index
(kernels/mjpeg_index.hip) against its host reference, decode from a
device-resident stream against the CPU decoder, and the engine's mjpeg
decode and sink on a GPU instance against the CPU paths."""
import numpy as np
import pytest

import scanner_amd as sp
from scanner_amd import _core

import mjpeg_cases as mc

pytestmark = pytest.mark.gpu

TILE = 4096  # bytes one workgroup classifies per step
LANE = 16    # bytes per lane; tiles start at a 16-byte aligned address


def encode(fr, quality=90, ss="444"):
    return [_core.jpeg_cpu_encode(f, quality, ss) for f in fr]


def check_index(samples, lead=0, gap=0, nseg=None):
    """gpu == ref on the samples laid out as a stream; returns both."""
    stream, offs, sizes = mc.layout(samples, lead, gap)
    info = _core.mjpeg_header_info(samples[0])
    nseg = info["nseg"] if nseg is None else nseg
    ref = _core.mjpeg_index_ref(stream, offs, sizes, info["header_len"], nseg)
    gpu = _core.mjpeg_index_gpu(stream, offs, sizes, info["header_len"], nseg)
    np.testing.assert_array_equal(gpu[1], ref[1])
    np.testing.assert_array_equal(gpu[0], ref[0])
    return ref, offs


def parse_segments(sample, off):
    return [(b + off, e + off, f, m)
            for b, e, f, m in _core.jpeg_decode_info(sample)["segments"]]


@pytest.mark.parametrize("ss", mc.SUBSAMPLINGS)
@pytest.mark.parametrize("shape", mc.SHAPES + [(64, 2080, 1)])
def test_index_matches_reference(shape, ss):
    h, w, c = shape
    samples = encode(mc.frames(3, h, w, c, seed=h + w), 90, ss)
    (segs, status), offs = check_index(samples)
    assert status.tolist() == [0, 0, 0]
    for i, s in enumerate(samples):
        assert [tuple(r) for r in segs[i].tolist()] == \
            parse_segments(s, offs[i])
    if shape == (64, 2080, 1):
        assert segs.shape[1] == 65  # two entropy workgroups per frame


def test_index_dense_stuffing():
    # noise at quality 100: FF bytes, and so FF 00 pairs, are frequent
    samples = encode(mc.noise_frames(2, 40, 520, 3, seed=5), 100, "444")
    assert sum(s.count(b"\xff\x00") for s in samples) > 500
    (segs, status), offs = check_index(samples)
    assert status.tolist() == [0, 0]
    for i, s in enumerate(samples):
        assert [tuple(r) for r in segs[i].tolist()] == \
            parse_segments(s, offs[i])


@pytest.mark.parametrize("lead", [1, 3, 7, 13, 255])
def test_index_odd_offsets(lead):
    samples = encode(mc.frames(3, 40, 520, 3, seed=lead), 90, "420")
    (segs, status), offs = check_index(samples, lead=lead, gap=lead % 5)
    assert status.tolist() == [0, 0, 0]
    for i, s in enumerate(samples):
        assert [tuple(r) for r in segs[i].tolist()] == \
            parse_segments(s, offs[i])


def test_index_comment_lengths_cover_a_tile_period():
    """The kernel's tiles start at the 16-byte aligned address at or below
    the first entropy byte, so where tile and lane boundaries fall inside
    the scan depends on that address modulo 16 alone: 16 consecutive COM
    lengths are one full period. Four periods are run, on a Pillow stream
    with a restart marker after every MCU, so markers and FF 00 pairs are
    dense (the scan is several tiles long)."""
    base = mc.pillow_jpeg(mc.noise_frames(1, 96, 128, 3, seed=9)[0],
                          quality=97, subsampling=0, restart_marker_blocks=1)
    assert len(base) > 3 * TILE and base.count(b"\xff\x00") > 50
    for k in range(4 * LANE):
        s = mc.with_comment(base, k)
        (segs, status), offs = check_index([s, s], lead=2)
        assert status.tolist() == [0, 0], k
        assert [tuple(r) for r in segs[1].tolist()] == \
            parse_segments(s, offs[1]), k


def crafted(header, nseg, positions, fill, end_at):
    """header + a scan of `end_at` bytes of fill with RSTn at the given
    scan-relative positions, then EOI."""
    scan = bytearray(fill(end_at))
    for k, p in enumerate(positions):
        scan[p:p + 2] = bytes([0xff, 0xd0 + (k & 7)])
    assert len(positions) == nseg - 1
    return header + bytes(scan) + b"\xff\xd9"


@pytest.mark.parametrize("shift", range(LANE))
def test_index_markers_on_every_tile_boundary(shift):
    """Crafted scans (the index reads bytes, it does not decode them): RSTn
    markers and FF 00 pairs that straddle, end at and start at the
    boundaries of the first tiles, at each of the 16 alignments of the
    scan. The index must equal the reference, which the CPU tests hold
    against jpeg_parse."""
    first = encode(mc.frames(1, 64, 2080, 1, seed=1), 90, "444")[0]
    info = _core.mjpeg_header_info(first)
    L, nseg = info["header_len"], info["nseg"]
    header = first[:L]
    # the device copy of the stream is at least 256-byte aligned: with
    # `lead` bytes in front the first entropy byte has address = shift mod 16
    lead = (shift - L) % LANE
    e1, e2, e3 = [t * TILE - shift for t in (1, 2, 3)]  # scan-relative
    positions = [
        e1 - 1,          # FF in one tile, the code in the next
        e1 + LANE - 1,   # the same across a lane boundary
        e2 - 2, e2,      # ends at the boundary, starts at it
        e2 + 2 * LANE,
        e3 + 1,
    ]
    positions += list(range(e3 + 40, e3 + 40 + 3 * (nseg - 1 -
                                                    len(positions)), 3))
    assert len(positions) == nseg - 1

    def fill(n):
        b = bytearray(0x11 + i % 7 for i in range(n))
        # stuffed FF 00 pairs around and across the boundaries
        for p in (e1 + 5, e2 - 5, e2 + LANE - 1, e3 - 1):
            b[p:p + 2] = b"\xff\x00"
        return b

    s = crafted(header, nseg, positions, fill, positions[-1] + 300)
    # a second sample: fill bytes FF FF 00 in front of a boundary marker
    t = bytearray(s)
    t[L + e1 - 4:L + e1 - 1] = b"\xff\xff\x00"
    (segs, status), offs = check_index([s, bytes(t)], lead=lead)
    assert status.tolist() == [0, 0]
    got = segs[0].tolist()
    assert [r[1] for r in got[:-1]] == [offs[0] + L + p for p in positions]
    assert [r[0] for r in got[1:]] == [offs[0] + L + p + 2 for p in positions]


def test_index_status_cases():
    fr = mc.frames(1, 16, 272, 3, seed=3)
    good = encode(fr, 90, "444")[0]
    info = _core.mjpeg_header_info(good)
    L, nseg = info["header_len"], info["nseg"]
    assert nseg == 3
    rst = [i for i in range(L, len(good) - 1)
           if good[i] == 0xff and 0xd0 <= good[i + 1] <= 0xd7]
    assert len(rst) == 2
    out_of_seq = bytearray(good)
    out_of_seq[rst[0] + 1] = 0xd3
    too_many = good[:rst[1] + 2] + b"\x55\xff\xd2" + good[rst[1] + 2:]
    too_few = good[:rst[1]] + good[rst[1] + 2:]
    cases = [
        (good, 0),
        (good[:-10], 2),                      # truncated: no EOI
        (good[:-1], 2),                       # FF is the last byte
        (bytes(out_of_seq), 4),               # RST3 where RST0 belongs
        (too_many, 5),
        (too_few, 5),
        (good + b"\x12\xff\xd0\xff\xc4junk", 0),   # bytes after EOI
        (encode(fr, 60, "444")[0], 1),        # another quality
        (good[:L - 3], 1),                    # shorter than the header
        (good[:-2] + b"\xff\xda", 3),         # the scan ends in SOS, not EOI
    ]
    (segs, status), offs = check_index([c for c, _ in cases], lead=5, gap=3)
    assert status.tolist() == [st for _, st in cases]
    want = parse_segments(good, 0)
    for i, (c, st) in enumerate(cases):
        rows = [tuple(r) for r in segs[i].tolist()]
        if st == 0:
            assert rows == [(b + offs[i], e + offs[i], f, m)
                            for b, e, f, m in want]
        else:
            assert rows == [(0, 0, 0, 0)] * nseg  # a status and no more


@pytest.mark.parametrize("ss", mc.SUBSAMPLINGS)
@pytest.mark.parametrize("shape", mc.SHAPES + [(64, 2080, 1)])
def test_decode_from_device_stream(shape, ss):
    h, w, c = shape
    samples = encode(mc.frames(5, h, w, c, seed=7), 85, ss)
    stream, offs, sizes = mc.layout(samples, lead=3, gap=1)
    want = [0, 2, 4]
    got, on_index, fell_back = _core.mjpeg_gpu_decode(stream, offs, sizes,
                                                      want, h, w, c)
    assert (on_index, fell_back) == (3, 0)
    for k, i in enumerate(want):
        np.testing.assert_array_equal(got[k],
                                      _core.jpeg_cpu_decode(samples[i]))


def test_decode_hands_back_what_the_index_refuses():
    fr = mc.frames(4, 40, 520, 3, seed=11)
    samples = encode(fr, 85, "420")
    samples[1] = encode(fr[1:2], 50, "420")[0]           # another header
    samples[2] = mc.pillow_jpeg(fr[2], quality=80)       # no DRI at all
    stream, offs, sizes = mc.layout(samples)
    got, on_index, fell_back = _core.mjpeg_gpu_decode(
        stream, offs, sizes, [0, 1, 2, 3], 40, 520, 3)
    assert (on_index, fell_back) == (2, 2)
    for i in range(4):
        np.testing.assert_array_equal(got[i],
                                      _core.jpeg_cpu_decode(samples[i]))


def test_decode_corrupt_frame_raises_cpu_error():
    samples = encode(mc.frames(3, 16, 272, 3, seed=2), 90, "444")
    L = _core.mjpeg_header_info(samples[0])["header_len"]
    bad = bytearray(samples[1])
    bad[L + 5:L + 25] = b"\xff\x00" * 10   # markers stay, the codes do not
    samples[1] = bytes(bad)
    with pytest.raises(Exception) as cpu:
        _core.jpeg_cpu_decode(samples[1])
    stream, offs, sizes = mc.layout(samples)
    with pytest.raises(Exception) as gpu:
        _core.mjpeg_gpu_decode(stream, offs, sizes, [0, 1, 2], 16, 272, 3)
    assert "frame 1" in str(gpu.value)
    assert "corrupt JPEG entropy data" in str(gpu.value)
    assert str(cpu.value).split("corrupt JPEG")[1] in str(gpu.value)


# ---------------- engine ----------------

N, H, W = 12, 40, 520


def hist_rows(sc, video, device, gpu_ids, name):
    frame = sc.io.Input([video])
    hist = sc.ops.Histogram(frame=frame, device=device)
    out = sp.NamedStream(sc, name)
    prof = sc.run(sc.io.Output([hist], [out]), sp.PerfParams.manual(4, 8),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=gpu_ids)
    rows = [np.frombuffer(r, np.uint32) for r in out.load()]
    return np.stack(rows), prof.counters()


def test_pipeline_gpu_decode_matches_cpu(sc):
    fr = mc.frames(N, H, W, 3, seed=21)
    video = sp.NamedVideoStream(sc, "clip", frames=fr, codec="mjpeg",
                                quality=85)
    cpu, _ = hist_rows(sc, video, sp.DeviceType.CPU, [], "h_cpu")
    gpu, counters = hist_rows(sc, video, sp.DeviceType.GPU, [0], "h_gpu")
    np.testing.assert_array_equal(gpu, cpu)
    ref = np.stack([np.stack([np.bincount(f[:, :, c].ravel(), minlength=256)
                              for c in range(3)]).ravel()
                    for f in video.load()])
    np.testing.assert_array_equal(gpu, ref)
    assert counters["decoded_frames"] == N
    assert counters["mjpeg_gpu_index_frames"] == N
    assert counters.get("mjpeg_host_fallback_frames", 0) == 0


def test_pipeline_optimised_headers_fall_back(sc, tmp_path):
    """Pillow optimize=True gives every frame its own Huffman tables, so
    every header but sample 0's differs from the reference: sample 0 is
    indexed, the rest fall back, and the pixels are the CPU decoder's."""
    fr = mc.frames(6, H, W, 3, seed=23, noise=64)
    samples = [mc.pillow_jpeg(f, quality=80, subsampling=2, optimize=True,
                              restart_marker_blocks=8) for f in fr]
    assert len({s[:mc.scan_start(s)] for s in samples}) == 6
    path = tmp_path / "opt.mov"
    path.write_bytes(mc.mux_mp4(samples, W, H, entry="jpeg"))
    video = sp.NamedVideoStream(sc, "opt", path=str(path))
    cpu, _ = hist_rows(sc, video, sp.DeviceType.CPU, [], "o_cpu")
    gpu, counters = hist_rows(sc, video, sp.DeviceType.GPU, [0], "o_gpu")
    np.testing.assert_array_equal(gpu, cpu)
    assert counters["mjpeg_gpu_index_frames"] == 1
    assert counters["mjpeg_host_fallback_frames"] == 5


def run_sink(sc, monkeypatch, switch, name, video, ss):
    monkeypatch.setenv("SCANNER_MJPEG_GPU", switch)
    frame = sc.io.Input([video])
    blur = sc.ops.Blur(frame=frame, kernel_size=3, device=sp.DeviceType.GPU)
    blur.compress_video(codec="mjpeg", quality=80, subsampling=ss)
    out = sp.NamedStream(sc, name)
    prof = sc.run(sc.io.Output(blur, [out]), sp.PerfParams.manual(4, 8),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    info = sc._db.table_info(name)
    items = [_core.read_video_item(sc._db, name, info["columns"][0][0], i)
             for i in range(len(info["end_rows"]))]
    return items, prof.counters()


@pytest.mark.parametrize("ss", mc.SUBSAMPLINGS)
def test_pipeline_gpu_sink_matches_host_sink(sc, monkeypatch, ss):
    fr = mc.frames(N, H, W, 3, seed=29)
    video = sp.NamedVideoStream(sc, "src", frames=fr, codec="svc")
    on, c_on = run_sink(sc, monkeypatch, "1", "on_" + ss, video, ss)
    off, c_off = run_sink(sc, monkeypatch, "0", "off_" + ss, video, ss)
    assert len(on) == len(off) == 2
    for (b_on, m_on), (b_off, m_off) in zip(on, off):
        assert m_on == m_off
        assert b_on == b_off
        assert m_on["codec"] == "mjpeg"
    total = sum(len(b) for b, _ in on)
    assert c_on["mjpeg_gpu_encode_frames"] == N
    assert c_on["sink_d2h_bytes"] == total + 4 * N
    assert c_off.get("mjpeg_gpu_encode_frames", 0) == 0
    assert c_off["sink_d2h_bytes"] == N * H * W * 3


def test_pipeline_corrupt_frame_names_the_frame(sc, tmp_path):
    samples = encode(mc.frames(4, 16, 272, 3, seed=31), 90, "444")
    L = _core.mjpeg_header_info(samples[0])["header_len"]
    bad = bytearray(samples[2])
    bad[L + 5:L + 25] = b"\xff\x00" * 10
    samples[2] = bytes(bad)
    path = tmp_path / "bad.mp4"
    path.write_bytes(mc.mux_mp4(samples, 272, 16, entry="mp4v"))
    video = sp.NamedVideoStream(sc, "bad", path=str(path))
    with pytest.raises(Exception) as err:
        hist_rows(sc, video, sp.DeviceType.GPU, [0], "bad_h")
    assert "frame 2" in str(err.value)
    assert "corrupt JPEG entropy data" in str(err.value)
