"""GPU writer of the "parallel" PNG format (kernels/png_encode.hip) and the
GPU ImageEncoder op with png_writer="parallel". The contract is byte identity
with the CPU writer: there is no tolerance anywhere in this file."""
import os

import numpy as np
import pytest

import scanner_amd as sp
from scanner_amd import _core
from conftest import make_smooth_video
from png_cases import CASES, CASE_IDS, SPLIT, cpu_png, frame

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,content", CASES, ids=CASE_IDS)
def test_encode_matches_cpu(shape, content):
    (got,) = _core.png_gpu_encode([frame(shape, content)])
    want = cpu_png(shape, content)
    assert len(got) == len(want)
    assert got == want


def test_one_call_mixes_shapes_and_grey_and_colour():
    """The whole case list in one call, ordered so that shapes alternate."""
    order = sorted(range(len(CASES)), key=lambda i: (i % 7, i))
    got = _core.png_gpu_encode([frame(*CASES[i]) for i in order])
    assert len(got) == len(order)
    for blob, i in zip(got, order):
        assert blob == cpu_png(*CASES[i]), CASE_IDS[i]


def test_more_frames_than_one_launch_sequence():
    """35 frames of one shape: three launch sequences of at most 16."""
    contents = [c for s, c in CASES if s == SPLIT]
    frames = [frame(SPLIT, contents[i % len(contents)]) for i in range(35)]
    got = _core.png_gpu_encode(frames)
    assert got == [cpu_png(SPLIT, contents[i % len(contents)])
                   for i in range(35)]


def test_encode_deterministic():
    frames = [frame(*CASES[i]) for i in range(len(CASES)) if i % 5 == 0]
    assert _core.png_gpu_encode(frames) == _core.png_gpu_encode(frames)


# ---------------- op and pipeline ----------------

N, H, W = 20, 48, 64
OUT_H, OUT_W = 40, 56


def png_graph(sc, name, frames, resize=True, null_repeat=0, **args):
    """SVC GPU decode -> (GPU Resize) -> GPU ImageEncoder(png, parallel)."""
    video = sp.NamedVideoStream(sc, name + "_in", frames=frames, codec="svc")
    frame_col = sc.io.Input([video])
    if resize:
        frame_col = sc.ops.Resize(frame=frame_col, width=OUT_W, height=OUT_H,
                                  device=sp.DeviceType.GPU)
    src = (sc.streams.RepeatNull(frame_col, [null_repeat]) if null_repeat
           else frame_col)
    args.setdefault("png_writer", "parallel")
    enc = sc.ops.ImageEncoder(frame=src, format="png",
                              device=sp.DeviceType.GPU, **args)
    return frame_col, enc


def test_pipeline_rows_match_cpu_writer(sc):
    """With a Resize in front: the rows equal the CPU writer's files of the
    GPU-resized frames, fetched through a second column of the same run."""
    frames = make_smooth_video(n=N, h=H, w=W)
    small, enc = png_graph(sc, "pngg_r", frames)
    out = sp.NamedStream(sc, "pngg_r_out")
    prof = sc.run(sc.io.Output([enc, small], [out]),
                  sp.PerfParams.manual(5, 20),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(sp.NamedStream(sc, "pngg_r_out", column="img").load())
    resized = list(sp.NamedVideoStream(sc, "pngg_r_out",
                                       column="frame").load())
    assert len(rows) == len(resized) == N
    for blob, f in zip(rows, resized):
        assert f.shape == (OUT_H, OUT_W, 3)
        assert bytes(blob) == _core.png_cpu_encode(f, "parallel")
    assert prof.counters().get("png_gpu_encode_frames", 0) == N


def test_pipeline_table_and_files_sink(sc, tmp_path):
    """SVC video straight into the encoder. The writer is lossless, so a
    row equals the CPU writer's file of the pixels it decodes to."""
    frames = make_smooth_video(n=N, h=H, w=W)
    _, enc = png_graph(sc, "pngg_t", frames, resize=False)
    out = sp.NamedStream(sc, "pngg_t_out")
    prof = sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(5, 20),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = [bytes(r) for r in out.load()]
    assert len(rows) == N
    assert prof.counters().get("png_gpu_encode_frames", 0) == N
    for blob in rows:
        pix = _core.png_cpu_decode(blob)
        assert pix.shape == (H, W, 3)
        assert blob == _core.png_cpu_encode(pix, "parallel")
    out_dir = str(tmp_path / "pngs")
    os.makedirs(out_dir)
    _, enc2 = png_graph(sc, "pngg_f", frames, resize=False)
    sc.run(sc.sinks.Files(enc2, out_dir, ext="png"),
           sp.PerfParams.manual(5, 20), cache_mode=sp.CacheMode.Overwrite,
           gpu_ids=[0])
    for i, blob in enumerate(rows):
        with open(os.path.join(out_dir, f"c0_{i}.png"), "rb") as fh:
            assert fh.read() == blob


def test_pipeline_null_rows_pass_through(sc):
    frames = make_smooth_video(n=6, h=H, w=W)
    _, enc = png_graph(sc, "pngg_n", frames, null_repeat=2)
    out = sp.NamedStream(sc, "pngg_n_out")
    prof = sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(4, 12),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    assert len(rows) == 12
    assert all(r is None for r in rows[1::2])
    for blob in rows[0::2]:
        pix = _core.png_cpu_decode(bytes(blob))
        assert pix.shape == (OUT_H, OUT_W, 3)
        assert bytes(blob) == _core.png_cpu_encode(pix, "parallel")
    assert prof.counters().get("png_gpu_encode_frames", 0) == 6


@pytest.mark.parametrize("value", ["fast", ""])
def test_bad_writer_is_rejected_on_the_gpu_kernel(sc, value):
    frames = make_smooth_video(n=2, h=H, w=W)
    _, enc = png_graph(sc, "pngg_b", frames, resize=False, png_writer=value)
    out = sp.NamedStream(sc, "pngg_b_out")
    with pytest.raises(Exception, match="png_writer") as e:
        sc.run(sc.io.Output(enc, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    assert "'zlib'" in str(e.value) and "'parallel'" in str(e.value)
