"""4:2:0 mode of the GPU JPEG encoder (kernels/jpeg_encode.hip) and of the GPU
ImageEncoder op. The contract is byte identity with
jpeg_cpu_encode(subsampling="420"): there is no tolerance anywhere in this
file."""
import numpy as np
import pytest

import scanner_amd as sp
from scanner_amd import _core
from conftest import make_smooth_video
from test_jpeg_cpu import decode, image
from test_jpeg420_cpu import CONTENTS, SHAPE_IDS, SHAPES, cpu_jpeg420

pytestmark = pytest.mark.gpu


def batch(shape, content, n):
    return np.stack([image(shape, content, seed) for seed in range(n)])


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_encode_matches_cpu(shape, content):
    """Batches of 1, 3 and 9 frames (9 crosses the op's preferred batch of
    8); the frames of a batch differ."""
    for n in (1, 3, 9):
        frames = batch(shape, content, n)
        for q in (1, 50, 100):
            got = _core.jpeg_gpu_encode(frames, q, subsampling="420")
            want = [cpu_jpeg420(shape, content, q, seed) for seed in range(n)]
            assert [len(g) for g in got] == [len(w) for w in want], (n, q)
            assert got == want, (n, q)


def test_encode_1080p():
    """68 x 120 MCUs are 510 segments: more than one step of the offset
    scan."""
    h, w = 1080, 1920
    yy, xx = np.mgrid[0:h, 0:w]
    frame = np.stack([(xx + yy) % 256, (2 * yy) % 256, (xx // 2) % 256],
                     -1).astype(np.uint8)
    noise = np.random.RandomState(5).randint(0, 256, (h // 2, w // 2, 3))
    frame[:h // 2, w // 2:] = noise  # one textured quadrant
    (got,) = _core.jpeg_gpu_encode(frame[None], 90, subsampling="420")
    want = _core.jpeg_cpu_encode(frame, 90, subsampling="420")
    assert len(_core.jpeg_decode_info(want)["segments"]) == 510
    assert len(got) == len(want)
    assert got == want
    assert decode(got).size == (w, h)


def test_encode_deterministic():
    frames = batch((185, 170, 3), "noise", 3)
    first = _core.jpeg_gpu_encode(frames, 90, subsampling="420")
    assert _core.jpeg_gpu_encode(frames, 90, subsampling="420") == first


@pytest.mark.parametrize("shape", [(16, 24, 1), (1, 1, 1)])
def test_grey_is_unchanged_by_420(shape):
    frames = batch(shape, "noise", 3)
    got = _core.jpeg_gpu_encode(frames, 75, subsampling="420")
    assert got == _core.jpeg_gpu_encode(frames, 75, subsampling="444")
    assert got == [_core.jpeg_cpu_encode(f, 75) for f in frames]


# ---------------- op and pipeline ----------------

N, H, W = 20, 48, 64
OUT_H, OUT_W = 40, 56  # neither is a multiple of 16


def jpeg420_graph(sc, name, frames, quality=90):
    """SVC GPU decode -> GPU Resize -> GPU ImageEncoder(jpg, 4:2:0)."""
    video = sp.NamedVideoStream(sc, name + "_in", frames=frames, codec="svc")
    small = sc.ops.Resize(frame=sc.io.Input([video]), width=OUT_W,
                          height=OUT_H, device=sp.DeviceType.GPU)
    enc = sc.ops.ImageEncoder(frame=small, format="jpg", quality=quality,
                              subsampling="420", device=sp.DeviceType.GPU)
    return small, enc


def test_pipeline_rows_match_cpu_encoder(sc):
    """The encoded rows equal jpeg_cpu_encode(subsampling="420") of the
    GPU-resized frames, fetched through a second output column."""
    frames = make_smooth_video(n=N, h=H, w=W)
    small, enc = jpeg420_graph(sc, "jpg420_g", frames)
    out = sp.NamedStream(sc, "jpg420_g_out")
    prof = sc.run(sc.io.Output([enc, small], [out]),
                  sp.PerfParams.manual(5, 20),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(sp.NamedStream(sc, "jpg420_g_out", column="img").load())
    resized = list(sp.NamedVideoStream(sc, "jpg420_g_out",
                                       column="frame").load())
    assert len(rows) == len(resized) == N
    for blob, f in zip(rows, resized):
        assert f.shape == (OUT_H, OUT_W, 3)
        assert blob == _core.jpeg_cpu_encode(f, 90, subsampling="420")
    assert prof.counters().get("jpeg_gpu_encode_frames", 0) == N


def test_pipeline_moves_only_compressed_bytes(sc):
    frames = make_smooth_video(n=N, h=H, w=W)
    _, enc = jpeg420_graph(sc, "jpg420_c", frames)
    out = sp.NamedStream(sc, "jpg420_c_out")
    prof = sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(5, 20),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    counters = prof.counters()
    assert counters.get("jpeg_gpu_encode_frames", 0) == N
    assert counters["sink_d2h_bytes"] == sum(len(r) for r in rows)
    for blob in rows:
        info = _core.jpeg_decode_info(blob)
        assert (info["h"], info["w"], info["hs"], info["vs"]) == \
            (OUT_H, OUT_W, 2, 2)


def test_pipeline_round_trip_on_the_device(sc):
    """Our own 4:2:0 files take the decoder's device path."""
    frames = make_smooth_video(n=N, h=H, w=W)
    _, enc = jpeg420_graph(sc, "jpg420_r", frames, quality=85)
    dec = sc.ops.ImageDecoder(img=enc, device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "jpg420_r_out")
    prof = sc.run(sc.io.Output([dec, enc], [out]),
                  sp.PerfParams.manual(5, 20),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(sp.NamedStream(sc, "jpg420_r_out", column="img").load())
    decoded = list(sp.NamedVideoStream(sc, "jpg420_r_out",
                                       column="frame").load())
    assert len(rows) == len(decoded) == N
    for blob, f in zip(rows, decoded):
        info = _core.jpeg_decode_info(blob)
        assert info["hs"] == info["vs"] == 2
        assert info["restart_interval"] == 16
        assert f.shape == (OUT_H, OUT_W, 3)
        np.testing.assert_array_equal(f, _core.jpeg_cpu_decode(blob))
    counters = prof.counters()
    assert counters.get("jpeg_gpu_encode_frames", 0) == N
    assert counters.get("jpeg_gpu_decode_frames", 0) == N
    assert counters.get("image_decode_host_rows", 0) == 0


@pytest.mark.parametrize("value", ["422", "411", ""])
def test_bad_op_subsampling_raises_at_construction(sc, value):
    frames = make_smooth_video(n=2, h=H, w=W)
    video = sp.NamedVideoStream(sc, "jpg420_b_in", frames=frames, codec="svc")
    enc = sc.ops.ImageEncoder(frame=sc.io.Input([video]), format="jpg",
                              subsampling=value, device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "jpg420_b_out")
    with pytest.raises(Exception, match="subsampling"):
        sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
