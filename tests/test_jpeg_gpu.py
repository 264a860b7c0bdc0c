"""GPU JPEG encoder (kernels/jpeg_encode.hip) and the GPU ImageEncoder op.
The contract is byte identity with jpeg_cpu_encode: there is no tolerance
anywhere in this file."""
import os

import numpy as np
import pytest

import scanner_amd as sp
from scanner_amd import FrameType, _core, register_python_op
from conftest import make_smooth_video
from test_jpeg_cpu import CONTENTS, SHAPE_IDS, SHAPES, cpu_jpeg, decode, image

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
            got = _core.jpeg_gpu_encode(frames, q)
            want = [cpu_jpeg(shape, content, q, seed) for seed in range(n)]
            assert [len(g) for g in got] == [len(w) for w in want], (n, q)
            assert got == want, (n, q)


def test_encode_1080p():
    """1020 segments per frame: more than one step of the offset scan."""
    h, w = 1080, 1920
    yy, xx = np.mgrid[0:h, 0:w]
    frame = np.stack([(xx + yy) % 256, (2 * yy) % 256, (xx // 2) % 256],
                     -1).astype(np.uint8)
    noise = np.random.RandomState(5).randint(0, 256, (h // 2, w // 2, 3))
    frame[:h // 2, w // 2:] = noise  # one textured quadrant
    (got,) = _core.jpeg_gpu_encode(frame[None], 90)
    want = _core.jpeg_cpu_encode(frame, 90)
    assert len(got) == len(want)
    assert got == want
    assert decode(got).size == (w, h)


def test_encode_deterministic():
    frames = batch((136, 4 * _core.jpeg_restart_interval(), 1), "noise", 3)
    first = _core.jpeg_gpu_encode(frames, 90)
    assert _core.jpeg_gpu_encode(frames, 90) == first


# ---------------- op and pipeline ----------------

N, H, W = 20, 48, 64
OUT_H, OUT_W = 40, 56
RAW = N * OUT_H * OUT_W * 3


def jpeg_graph(sc, name, frames, quality=90, null_repeat=0):
    """SVC GPU decode -> GPU Resize -> GPU ImageEncoder(jpg)."""
    video = sp.NamedVideoStream(sc, name + "_in", frames=frames, codec="svc")
    frame = sc.io.Input([video])
    small = sc.ops.Resize(frame=frame, width=OUT_W, height=OUT_H,
                          device=sp.DeviceType.GPU)
    src = sc.streams.RepeatNull(small, [null_repeat]) if null_repeat else small
    enc = sc.ops.ImageEncoder(frame=src, format="jpg", quality=quality,
                              device=sp.DeviceType.GPU)
    return small, enc


def test_pipeline_rows_match_cpu_encoder(sc):
    """The encoded rows equal jpeg_cpu_encode of the GPU-resized frames,
    fetched through a second output column of the same run."""
    frames = make_smooth_video(n=N, h=H, w=W)
    small, enc = jpeg_graph(sc, "jpg_g", frames)
    out = sp.NamedStream(sc, "jpg_g_out")
    prof = sc.run(sc.io.Output([enc, small], [out]),
                  sp.PerfParams.manual(5, 20),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(sp.NamedStream(sc, "jpg_g_out", column="img").load())
    resized = list(sp.NamedVideoStream(sc, "jpg_g_out", column="frame").load())
    assert len(rows) == len(resized) == N
    for blob, f in zip(rows, resized):
        assert f.shape == (OUT_H, OUT_W, 3)
        assert blob == _core.jpeg_cpu_encode(f, 90)
    assert prof.counters().get("jpeg_gpu_encode_frames", 0) == N


def test_pipeline_moves_only_compressed_bytes(sc):
    frames = make_smooth_video(n=N, h=H, w=W)
    _, enc = jpeg_graph(sc, "jpg_c", frames)
    out = sp.NamedStream(sc, "jpg_c_out")
    prof = sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(5, 20),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    counters = prof.counters()
    assert counters.get("jpeg_gpu_encode_frames", 0) == N
    assert counters["sink_d2h_bytes"] == sum(len(r) for r in rows)
    assert 0 < counters["sink_d2h_bytes"] < RAW
    for blob in rows:
        assert decode(blob).size == (OUT_W, OUT_H)


def test_pipeline_null_rows_pass_through(sc):
    frames = make_smooth_video(n=6, h=H, w=W)
    _, enc = jpeg_graph(sc, "jpg_n", frames, null_repeat=2)
    out = sp.NamedStream(sc, "jpg_n_out")
    prof = sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(4, 12),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    assert len(rows) == 12
    assert all(r is None for r in rows[1::2])
    for blob in rows[0::2]:
        assert decode(blob).size == (OUT_W, OUT_H)
    assert prof.counters().get("jpeg_gpu_encode_frames", 0) == 6


@register_python_op(name="JpegVaryShape")
def jpeg_vary_shape(frame: FrameType) -> FrameType:
    """Frames alternate between two heights (the first pixel carries the
    frame number)."""
    return np.ascontiguousarray(frame[:40 if frame[0, 0, 0] % 2 else 48])


def test_pipeline_mixed_shapes_in_one_batch(sc):
    """A batch whose frames change shape is encoded as sub-batches."""
    frames = make_smooth_video(n=12, h=H, w=W)
    frames[:, 0, 0, 0] = np.arange(12)
    video = sp.NamedVideoStream(sc, "jpg_m_in", frames=frames, codec="raw")
    varied = sc.ops.JpegVaryShape(frame=sc.io.Input([video]))
    enc = sc.ops.ImageEncoder(frame=varied, format="jpeg", quality=60,
                              device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "jpg_m_out")
    prof = sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(12, 12),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    assert len(rows) == 12
    for i, blob in enumerate(rows):
        assert blob == _core.jpeg_cpu_encode(frames[i, :40 if i % 2 else 48],
                                             60)
    assert prof.counters().get("jpeg_gpu_encode_frames", 0) == 12


def test_pipeline_files_sink_writes_jpg(sc, tmp_path):
    frames = make_smooth_video(n=N, h=H, w=W)
    _, enc = jpeg_graph(sc, "jpg_f", frames, quality=75)
    out_dir = str(tmp_path / "jpgs")
    os.makedirs(out_dir)
    sc.run(sc.sinks.Files(enc, out_dir, ext="jpg"),
           sp.PerfParams.manual(5, 20), cache_mode=sp.CacheMode.Overwrite,
           gpu_ids=[0])
    # the same graph into a table gives the bytes the files must hold
    _, enc2 = jpeg_graph(sc, "jpg_f2", frames, quality=75)
    out = sp.NamedStream(sc, "jpg_f2_out")
    sc.run(sc.io.Output(enc2, [out]), sp.PerfParams.manual(5, 20),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    assert len(rows) == N
    for i, blob in enumerate(rows):
        with open(os.path.join(out_dir, f"c0_{i}.jpg"), "rb") as fh:
            assert fh.read() == blob
        assert decode(blob).size == (OUT_W, OUT_H)


def test_png_on_gpu_is_rejected(sc):
    frames = make_smooth_video(n=2, h=H, w=W)
    video = sp.NamedVideoStream(sc, "jpg_p_in", frames=frames, codec="svc")
    enc = sc.ops.ImageEncoder(frame=sc.io.Input([video]), format="png",
                              device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "jpg_p_out")
    with pytest.raises(Exception, match="format=png has no GPU kernel"):
        sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
