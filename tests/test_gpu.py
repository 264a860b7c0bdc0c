"""GPU tests (run on a real MI355X via gpurun; every HIP kernel is compared
against the CPU reference path)."""
import numpy as np
import pytest

import scanner_amd as sp
from conftest import make_smooth_video, make_video

pytestmark = pytest.mark.gpu


def ref_histogram(frame):
    return np.stack([np.bincount(frame[:, :, c].ravel(), minlength=256)
                     for c in range(3)]).astype(np.uint32)


def test_gpu_available():
    from scanner_amd import _core
    assert _core.have_gpu()
    assert _core.gpu_device_count() >= 1


def test_gpu_histogram_matches_cpu(sc):
    frames = make_video(n=12, h=240, w=320)
    video = sp.NamedVideoStream(sc, "g_h", frames=frames, codec="raw")
    frame = sc.io.Input([video])
    hist = sc.ops.Histogram(frame=frame, device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "g_h_out")
    sc.run(sc.io.Output(hist, [out]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    assert len(rows) == 12
    for i, blob in enumerate(rows):
        got = np.frombuffer(blob, dtype=np.uint32).reshape(3, 256)
        np.testing.assert_array_equal(got, ref_histogram(frames[i]))


def test_gpu_resize_matches_cpu(sc):
    frames = make_video(n=4, h=64, w=96)
    video = sp.NamedVideoStream(sc, "g_r", frames=frames, codec="raw")

    for dev, name in ((sp.DeviceType.CPU, "g_r_cpu"),
                      (sp.DeviceType.GPU, "g_r_gpu")):
        frame = sc.io.Input([video])
        small = sc.ops.Resize(frame=frame, width=48, height=32, device=dev)
        out = sp.NamedStream(sc, name)
        sc.run(sc.io.Output(small, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite,
               gpu_ids=[0] if dev == sp.DeviceType.GPU else [])
    cpu = np.stack(list(sp.NamedVideoStream(sc, "g_r_cpu").load()))
    gpu = np.stack(list(sp.NamedVideoStream(sc, "g_r_gpu").load()))
    # identical bilinear math up to rounding
    assert np.abs(cpu.astype(int) - gpu.astype(int)).max() <= 1


def test_gpu_svc_decode(sc):
    frames = make_smooth_video(n=40, h=72, w=96)
    video = sp.NamedVideoStream(sc, "g_svc", frames=frames, codec="svc")
    frame = sc.io.Input([video])
    hist = sc.ops.Histogram(frame=frame, device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "g_svc_out")
    sc.run(sc.io.Output(hist, [out]), sp.PerfParams.manual(8, 16),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    assert len(rows) == 40
    for i, blob in enumerate(rows):
        got = np.frombuffer(blob, dtype=np.uint32).reshape(3, 256)
        np.testing.assert_array_equal(got, ref_histogram(frames[i]))


def test_gpu_svc_strided_decode(sc):
    frames = make_smooth_video(n=48, h=48, w=64)
    video = sp.NamedVideoStream(sc, "g_svs", frames=frames, codec="svc")
    frame = sc.io.Input([video])
    sampled = sc.streams.Stride(frame, [11])
    hist = sc.ops.Histogram(frame=sampled, device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "g_svs_out")
    sc.run(sc.io.Output(hist, [out]), sp.PerfParams.manual(2, 4),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    assert len(rows) == 5
    for k, blob in enumerate(rows):
        got = np.frombuffer(blob, dtype=np.uint32).reshape(3, 256)
        np.testing.assert_array_equal(got, ref_histogram(frames[k * 11]))


def test_gpu_pool_allocator():
    from scanner_amd import _core
    _core.destroy_memory()
    _core.init_memory(0, 1 << 30, [0])
    # engine allocations now come from the 1 GiB slab; run a small job
    import tempfile
    sc = sp.Client(db_path=tempfile.mkdtemp())
    frames = make_video(n=4, h=64, w=64)
    video = sp.NamedVideoStream(sc, "pool_t", frames=frames, codec="raw")
    frame = sc.io.Input([video])
    hist = sc.ops.Histogram(frame=frame, device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "pool_out")
    sc.run(sc.io.Output(hist, [out]), sp.PerfParams.manual(2, 4),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    assert len(list(out.load())) == 4
    _core.destroy_memory()


def test_gpu_optical_flow_matches_cpu(sc):
    from test_engine_cpu import make_textured_pair
    pair = make_textured_pair(h=96, w=128, dx=2, dy=1)
    # 24 frames: enough stencil windows that the LK launch takes the
    # 2-rows-per-thread (PY=2) path as well as PY=1 on the coarse levels
    frames = np.concatenate([pair, pair[::-1]] * 6)
    n = frames.shape[0]
    video = sp.NamedVideoStream(sc, "g_of", frames=frames, codec="raw")
    for dev, name in ((sp.DeviceType.CPU, "g_of_cpu"),
                      (sp.DeviceType.GPU, "g_of_gpu")):
        frame = sc.io.Input([video])
        flow = sc.ops.OpticalFlow(frame=frame, device=dev)
        out = sp.NamedStream(sc, name)
        sc.run(sc.io.Output(flow, [out]), sp.PerfParams.manual(24, 24),
               cache_mode=sp.CacheMode.Overwrite,
               gpu_ids=[0] if dev == sp.DeviceType.GPU else [])
    cpu = np.stack(list(sp.NamedVideoStream(sc, "g_of_cpu").load()))
    gpu = np.stack(list(sp.NamedVideoStream(sc, "g_of_gpu").load()))
    assert cpu.shape == gpu.shape == (n, 96, 128, 2)
    # same algorithm in f32; differences only from fma contraction
    diff = np.abs(cpu - gpu)
    assert np.median(diff) < 1e-3, np.median(diff)
    assert np.percentile(diff, 99) < 0.1, np.percentile(diff, 99)


def test_gpu_color_ops_match_cpu(sc):
    frames = make_video(n=4, h=48, w=64)
    video = sp.NamedVideoStream(sc, "g_c", frames=frames, codec="raw")

    def run(dev, tag, make_op):
        frame = sc.io.Input([video])
        col = make_op(frame, dev)
        out = sp.NamedStream(sc, tag)
        sc.run(sc.io.Output(col, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite,
               gpu_ids=[0] if dev == sp.DeviceType.GPU else [])
        return np.stack(list(sp.NamedVideoStream(sc, tag).load()))

    cases = {
        "crop": lambda f, d: sc.ops.Crop(frame=f, x=8, y=4, width=32,
                                         height=24, device=d),
        "gray": lambda f, d: sc.ops.ColorConvert(frame=f, format="gray",
                                                 device=d),
        "yuv": lambda f, d: sc.ops.ColorConvert(frame=f, format="yuv",
                                                device=d),
        "planar": lambda f, d: sc.ops.ColorConvert(frame=f, format="planar",
                                                   device=d),
        "blur": lambda f, d: sc.ops.Blur(frame=f, kernel_size=5, device=d),
    }
    for name, mk in cases.items():
        cpu = run(sp.DeviceType.CPU, f"g_c_{name}_cpu", mk)
        gpu = run(sp.DeviceType.GPU, f"g_c_{name}_gpu", mk)
        assert cpu.shape == gpu.shape, name
        diff = np.abs(cpu.astype(int) - gpu.astype(int))
        # crop, planar and blur are integer operations: equal; gray and yuv
        # round a float (held to the float64 value in test_image_ops_gpu.py)
        bound = 1 if name in ("gray", "yuv") else 0
        assert diff.max() <= bound, (name, diff.max())


def test_gpu_to_cpu_device_crossing(sc):
    """GPU Resize feeding the CPU PNG encoder exercises the automatic
    kernel-group D2H transfer (reference: copy_or_ref_elements,
    evaluate_worker.cpp:798-806)."""
    from test_engine_cpu import decode_png_filter0
    frames = make_video(n=4, h=64, w=96)
    video = sp.NamedVideoStream(sc, "g_x", frames=frames, codec="raw")
    frame = sc.io.Input([video])
    small = sc.ops.Resize(frame=frame, width=48, height=32,
                          device=sp.DeviceType.GPU)
    png = sc.ops.ImageEncoder(frame=small, format="png")  # CPU op
    out = sp.NamedStream(sc, "g_x_out")
    sc.run(sc.io.Output(png, [out]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    assert len(rows) == 4
    img = decode_png_filter0(rows[0])
    assert img.shape == (32, 48, 3)


def test_gpu_compressed_output(sc):
    """GPU pipeline with an SVC-compressed output column (sink-side
    encode of device-produced frames)."""
    from conftest import make_smooth_video
    frames = make_smooth_video(n=24, h=48, w=64)
    video = sp.NamedVideoStream(sc, "g_cmp", frames=frames, codec="svc")
    frame = sc.io.Input([video])
    blur = sc.ops.Blur(frame=frame, kernel_size=3, device=sp.DeviceType.GPU)
    blur.compress_video()
    out = sp.NamedStream(sc, "g_cmp_out")
    sc.run(sc.io.Output(blur, [out]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    got = np.stack(list(sp.NamedVideoStream(sc, "g_cmp_out").load()))
    assert got.shape == (24, 48, 64, 3)

    # CPU blur reference: identical box blur math
    frame = sc.io.Input([video])
    blur2 = sc.ops.Blur(frame=frame, kernel_size=3)
    out2 = sp.NamedStream(sc, "g_cmp_ref")
    sc.run(sc.io.Output(blur2, [out2]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite)
    ref = np.stack(list(sp.NamedVideoStream(sc, "g_cmp_ref").load()))
    assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1


def test_gpu_4k_decode_histogram(sc):
    """4K frames through SVC GPU decode + histogram (the pose pipeline's
    decode shape; catches large-frame geometry bugs the 1080p tests
    miss)."""
    from conftest import make_smooth_video
    frames = make_smooth_video(n=6, h=2160, w=3840)
    video = sp.NamedVideoStream(sc, "g_4k", frames=frames, codec="svc")
    frame = sc.io.Input([video])
    hist = sc.ops.Histogram(frame=frame, device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "g_4k_out")
    sc.run(sc.io.Output(hist, [out]), sp.PerfParams.manual(2, 4),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    assert len(rows) == 6
    for i, blob in enumerate(rows):
        got = np.frombuffer(blob, dtype=np.uint32).reshape(3, 256)
        np.testing.assert_array_equal(got, ref_histogram(frames[i]))


def test_gpu_svc_decode_odd_shapes(sc):
    """GPU SVC decode on odd dimensions (tail groups, non-multiple-of-32
    frame bytes) must match ingest exactly."""
    rng = np.random.RandomState(7)
    for i, (h, w) in enumerate([(13, 17), (37, 51), (9, 127)]):
        frames = rng.randint(0, 256, size=(11, h, w, 3)).astype(np.uint8)
        v = sp.NamedVideoStream(sc, f"godd{i}", frames=frames, codec="svc",
                                io_packet_size=5)
        frame = sc.io.Input([v])
        # GPU ColorConvert forces the GPU decode path; planar is lossless
        cc = sc.ops.ColorConvert(frame=frame, format="planar",
                                 device=sp.DeviceType.GPU)
        out = sp.NamedStream(sc, f"godd{i}_out")
        sc.run(sc.io.Output(cc, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
        got = np.stack(list(sp.NamedVideoStream(sc, f"godd{i}_out").load()))
        ref = np.transpose(frames, (0, 3, 1, 2))
        np.testing.assert_array_equal(got, ref)


def test_gpu_span_cache_hits_and_numerics(sc):
    """Second run of the same pipeline decodes from HBM-cached spans (no
    storage re-read, no H2D) and produces identical results (VERDICT r01
    #1: span cache)."""
    from scanner_amd import _core
    frames = make_smooth_video(n=40, h=72, w=96)
    video = sp.NamedVideoStream(sc, "g_sc", frames=frames, codec="svc")

    def run(name):
        frame = sc.io.Input([video])
        hist = sc.ops.Histogram(frame=frame, device=sp.DeviceType.GPU)
        out = sp.NamedStream(sc, name)
        sc.run(sc.io.Output(hist, [out]),
               sp.PerfParams.manual(8, 16, span_cache=256 << 20),
               cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
        return list(out.load())

    _core.span_cache_clear()
    r1 = run("g_sc_1")
    s1 = _core.span_cache_stats()
    r2 = run("g_sc_2")
    s2 = _core.span_cache_stats()
    assert r1 == r2
    for i, blob in enumerate(r1):
        got = np.frombuffer(blob, dtype=np.uint32).reshape(3, 256)
        np.testing.assert_array_equal(got, ref_histogram(frames[i]))
    # run 2 must be served from the cache
    assert s2["hits"] > s1["hits"]
    assert s2["misses"] == s1["misses"]
    assert s2["bytes"] > 0


def test_gpu_span_cache_eviction():
    """A tiny budget forces LRU eviction instead of unbounded growth."""
    from scanner_amd import _core
    _core.span_cache_clear()
    _core.span_cache_set_budget(1 << 20)  # 1 MB
    import tempfile, os
    import scanner_amd as spp
    sc2 = spp.Client(db_path=os.path.join(
        tempfile.mkdtemp(prefix="scse_"), "db"))
    frames = make_smooth_video(n=64, h=72, w=96)  # ~0.4 MB/frame raw
    video = spp.NamedVideoStream(sc2, "g_ev", frames=frames, codec="svc")
    frame = sc2.io.Input([video])
    hist = sc2.ops.Histogram(frame=frame, device=spp.DeviceType.GPU)
    out = spp.NamedStream(sc2, "g_ev_out")
    sc2.run(sc2.io.Output(hist, [out]),
            spp.PerfParams.manual(8, 16, span_cache=1 << 20),
            cache_mode=spp.CacheMode.Overwrite, gpu_ids=[0])
    s = _core.span_cache_stats()
    assert s["bytes"] <= 1 << 20
    rows = list(out.load())
    assert len(rows) == 64


def test_gpu_histogram_4k_raw(sc):
    """Histogram alone on raw-codec 4K frames (no SVC decode in the path)
    — isolates the histogram kernels at large frame sizes."""
    from conftest import make_smooth_video
    frames = make_smooth_video(n=3, h=2160, w=3840)
    video = sp.NamedVideoStream(sc, "g4kr", frames=frames, codec="raw")
    frame = sc.io.Input([video])
    hist = sc.ops.Histogram(frame=frame, device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "g4kr_out")
    sc.run(sc.io.Output(hist, [out]), sp.PerfParams.manual(2, 4),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    for i, blob in enumerate(out.load()):
        got = np.frombuffer(blob, dtype=np.uint32).reshape(3, 256)
        np.testing.assert_array_equal(got, ref_histogram(frames[i]))


def test_gpu_svc_decode_4k_exact(sc):
    """GPU SVC decode of 4K frames compared byte-exactly against the
    ingested frames (lossless codec): isolates the GOP-batched decode
    kernel at large geometry."""
    from conftest import make_smooth_video
    frames = make_smooth_video(n=6, h=2160, w=3840)
    video = sp.NamedVideoStream(sc, "g4kd", frames=frames, codec="svc")
    frame = sc.io.Input([video])
    out = sp.NamedStream(sc, "g4kd_out")
    # sink the decoded frame column itself (raw storage)
    sc.run(sc.io.Output(frame, [out]), sp.PerfParams.manual(2, 4),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    got = np.stack(list(sp.NamedVideoStream(sc, "g4kd_out").load()))
    np.testing.assert_array_equal(got, frames)


def test_gpu_svc_decode_multibatch_chain(sc):
    """Sparse wants over several GOPs make interior frames registers-only.
    Ingest encodes at GOP 16, so through the engine no chain is longer than
    one 16-frame launch; the same clip encoded as ONE 40-frame GOP is then
    decoded directly, which forces the chain across three launches (chain
    state handed over through the scratch buffer: frames 15 and 31 are not
    wanted). tests/test_svc_decode_gpu.py covers that path in full."""
    from conftest import make_smooth_video
    from scanner_amd import _core
    frames = make_smooth_video(n=40, h=120, w=160)
    video = sp.NamedVideoStream(sc, "gmb", frames=frames, codec="svc",
                                io_packet_size=40)
    # gop defaults to 16 at ingest; wants span several batches
    frame = sc.io.Input([video])
    g = sc.streams.Gather(frame, [[0, 7, 18, 19, 33, 39]])
    out = sp.NamedStream(sc, "gmb_out")
    sc.run(sc.io.Output(g, [out]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    got = np.stack(list(sp.NamedVideoStream(sc, "gmb_out").load()))
    np.testing.assert_array_equal(got, frames[[0, 7, 18, 19, 33, 39]])
    stream, sizes = _core.svc_cpu_encode(frames, 40)
    got = _core.svc_gpu_decode(stream, sizes, 120, 160, 3, [0],
                               [0, 7, 18, 19, 33, 39])
    np.testing.assert_array_equal(got, frames[[0, 7, 18, 19, 33, 39]])


def test_gpu_svc_decode_1080p_exact_repeated():
    """Regression for the GOP-batch decode corruption seen past byte 2^20:
    direct kernel round-trip at 1080p, byte-exact, repeated (the failure
    was content/size-conditional and schedule-sensitive)."""
    from conftest import make_smooth_video
    from scanner_amd import _core
    frames = make_smooth_video(n=4, h=1080, w=1920)
    ref = None
    for it in range(5):
        got = _core.svc_gpu_roundtrip(frames, 16, [])
        np.testing.assert_array_equal(got, frames, err_msg=f"iter {it}")
        if ref is None:
            ref = got
        else:
            np.testing.assert_array_equal(got, ref)  # run-to-run identical


def test_gpu_distributed_master_worker(tmp_path_factory):
    """Full distributed stack on GPU: real master + worker processes over
    shared storage, GPU decode + histogram + ResNet-50 pipeline through
    the pull scheduler (the CPU suite covers this path with gloo-era ops;
    this is the first-class GPU run)."""
    import os
    import signal
    import subprocess
    import sys
    import time

    from scanner_amd.master import MasterServer
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("gpud")
    db = str(tmp / "db")
    os.makedirs(db, exist_ok=True)
    master = MasterServer(db, task_timeout=120)
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    proc = subprocess.Popen(
        [sys.executable, "-m", "scanner_amd.worker", "--master",
         master.addr, "--db-path", db, "--instances", "2",
         "--gpu-ids", "0", "--no-watchdog"],
        env=env, start_new_session=True)
    try:
        sc = sp.Client(db_path=db, master=master.addr)
        frames = make_smooth_video(n=32, h=360, w=480)
        video = sp.NamedVideoStream(sc, "gd_clip", frames=frames,
                                    codec="svc")
        frame = sc.io.Input([video])
        hist = sc.ops.Histogram(frame=frame, device=sp.DeviceType.GPU)
        logits = sc.ops.ResNet50(frame=frame, device=sp.DeviceType.GPU)
        out = sp.NamedStream(sc, "gd_out")
        sc.run(sc.io.Output([hist, logits], [out]),
               sp.PerfParams.manual(8, 16, gpu_pool=4 << 30),
               cache_mode=sp.CacheMode.Overwrite)
        rows = list(out.load())
        assert len(rows) == 32
        for i, blob in enumerate(rows):
            got = np.frombuffer(blob, np.uint32).reshape(3, 256)
            np.testing.assert_array_equal(got, ref_histogram(frames[i]))
        info = sc.table_info("gd_out")
        assert [n for n, _ in info["columns"]] == ["histogram", "logits"]
        sc.shutdown()
    finally:
        try:
            os.killpg(proc.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        master.shutdown()
