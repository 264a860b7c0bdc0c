"""GPU JPEG decoder (kernels/jpeg_decode.hip) and the GPU ImageDecoder op.
The contract is byte identity with jpeg_cpu_decode: there is no tolerance
anywhere in this file."""
import numpy as np
import pytest

import scanner_amd as sp
from scanner_amd import _core
from conftest import make_smooth_video
from test_image_decode_cpu import (pillow_jpeg, pillow_save, unpack_frame,
                                   write_files)
from test_image_decode_fuzz import entropy_base, entropy_mutations
from test_jpeg_cpu import cpu_jpeg, image

pytestmark = pytest.mark.gpu

R = _core.jpeg_restart_interval()

# name -> (shape, file variant of pillow_jpeg or "ours", subsampling). Every
# file has a DRI segment, so every one is decoded on the device.
CASES = {
    "1x1_grey": ((1, 1, 1), "rst2", 0),
    "8x8_grey": ((8, 8, 1), "rst2", 0),
    "7x9_444": ((7, 9, 3), "rst2", 0),
    "17x33_420": ((17, 33, 3), "rst2", 2),   # partial MCU on both edges, odd
                                             # chroma extent
    "16x24_422": ((16, 24, 3), "rst2", 1),
    "one_full_segment": ((8, 8 * R, 1), "ours", 0),
    "nine_segments": ((136, 4 * R, 1), "ours", 0),  # the RST index wraps
    "40x56_420_rst1": ((40, 56, 3), "rst1", 2),     # every MCU a segment
    "40x56_rows1_opt": ((40, 56, 3), "rows1_opt", 1),  # non-Annex-K tables
}


def case_file(name, content, quality, seed):
    shape, variant, sub = CASES[name]
    if variant == "ours":
        return cpu_jpeg(shape, content, quality, seed)
    return pillow_jpeg(shape, content, quality, sub, variant, seed)


def gpu_decode(blobs, expect_host_rows=0):
    frames, host_rows = _core.jpeg_gpu_decode(list(blobs), host_rows=True)
    assert host_rows == expect_host_rows
    return frames


def assert_frames_equal(got, blobs):
    assert len(got) == len(blobs)
    for k, (g, b) in enumerate(zip(got, blobs)):
        want = _core.image_cpu_decode(b)
        assert g.shape == want.shape, k
        np.testing.assert_array_equal(g, want, err_msg=f"row {k}")


@pytest.mark.parametrize("content", ["smooth", "noise", "checker"])
@pytest.mark.parametrize("name", list(CASES))
def test_decode_matches_cpu(name, content):
    """Batches of 1, 3 and 9 files (9 crosses the op's preferred batch of
    8); the files of a batch differ."""
    for n in (1, 3, 9):
        for q in (1, 50, 100):
            blobs = [case_file(name, content, q, seed) for seed in range(n)]
            assert _core.jpeg_decode_info(blobs[0])["restart_interval"] > 0
            assert_frames_equal(gpu_decode(blobs), blobs)


def test_mixed_batch_keeps_order_and_counts_host_rows():
    """9 files of different shapes, samplings, qualities and table sets; a
    PNG and a JPEG without DRI sit in the middle and are decoded on the
    host."""
    blobs = [
        case_file("17x33_420", "noise", 50, 0),
        case_file("nine_segments", "smooth", 90, 1),
        case_file("40x56_rows1_opt", "checker", 30, 2),
        case_file("1x1_grey", "noise", 100, 3),
        pillow_save(image((7, 9, 3), "noise"), "PNG"),
        pillow_jpeg((33, 50, 3), "smooth", 75, 2),          # no DRI
        case_file("16x24_422", "smooth", 1, 4),
        case_file("40x56_420_rst1", "noise", 95, 5),
        case_file("7x9_444", "checker", 75, 6),
    ]
    assert _core.jpeg_decode_info(blobs[5])["restart_interval"] == 0
    assert_frames_equal(gpu_decode(blobs, expect_host_rows=2), blobs)
    # host rows only, and an empty batch
    assert_frames_equal(gpu_decode(blobs[4:6], expect_host_rows=2),
                        blobs[4:6])
    assert gpu_decode([]) == []


def frame_1080p():
    h, w = 1080, 1920
    yy, xx = np.mgrid[0:h, 0:w]
    frame = np.stack([(xx + yy) % 256, (2 * yy) % 256, (xx // 2) % 256],
                     -1).astype(np.uint8)
    noise = np.random.RandomState(5).randint(0, 256, (h // 2, w // 2, 3))
    frame[:h // 2, w // 2:] = noise  # one textured quadrant
    return frame


def test_decode_1080p():
    """Our encoder's file has 135 * 240 / 32 -> 1013 segments (16
    workgroups); Pillow's 4:2:0 file with a restart marker per MCU row has
    68 long ones."""
    frame = frame_1080p()
    ours = _core.jpeg_cpu_encode(frame, 90)
    pil = pillow_save(frame, quality=90, subsampling=2, restart_marker_rows=1)
    assert len(_core.jpeg_decode_info(ours)["segments"]) == 1013
    assert len(_core.jpeg_decode_info(pil)["segments"]) == 68
    blobs = [ours, pil]
    assert_frames_equal(gpu_decode(blobs), blobs)


def test_decode_deterministic():
    blobs = [case_file("nine_segments", "noise", 90, s) for s in range(3)] + \
        [case_file("40x56_420_rst1", "noise", 90, 0)]
    first = gpu_decode(blobs)
    second = gpu_decode(blobs)
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)


def outcome(fn, blob):
    try:
        return fn(blob)
    except Exception as e:  # noqa: BLE001 - the class is checked below
        return e


def test_error_parity_on_corrupt_entropy_data():
    """32 corruptions confined to the entropy-coded data of a (16,24,3) DRI
    file — the files test_image_decode_fuzz.py ran through the sanitizer
    build: both decoders return identical pixels or both raise."""
    good = entropy_base()
    raised = 0
    for k, blob in enumerate(entropy_mutations()):
        cpu = outcome(_core.jpeg_cpu_decode, blob)
        gpu = outcome(lambda b: _core.jpeg_gpu_decode([good, b])[1], blob)
        if isinstance(cpu, Exception):
            raised += 1
            assert isinstance(gpu, Exception), k
            assert type(gpu) is type(cpu), k
            assert "row 1" in str(gpu), (k, str(gpu))
            if "corrupt JPEG" in str(cpu):  # same cause, same segment
                assert str(cpu).split("corrupt JPEG")[-1] == \
                    str(gpu).split("corrupt JPEG")[-1], (k, str(gpu))
        else:
            assert not isinstance(gpu, Exception), (k, str(gpu))
            np.testing.assert_array_equal(gpu, cpu, err_msg=f"mutation {k}")
    assert 0 < raised < 32
    # the good file shared batches with bad ones; on its own it is intact
    assert_frames_equal(gpu_decode([good]), [good])


# ---------------- op and pipeline ----------------

N, H, W = 20, 48, 64
OUT_H, OUT_W = 40, 56


def test_pipeline_encoder_to_decoder_on_the_gpu(sc):
    """SVC decode -> Resize -> ImageEncoder(jpg) -> ImageDecoder, all on the
    GPU; the JPEG rows come out through a second column."""
    frames = make_smooth_video(n=N, h=H, w=W)
    video = sp.NamedVideoStream(sc, "imgdec_g_in", frames=frames, codec="svc")
    small = sc.ops.Resize(frame=sc.io.Input([video]), width=OUT_W,
                          height=OUT_H, device=sp.DeviceType.GPU)
    enc = sc.ops.ImageEncoder(frame=small, format="jpg", quality=85,
                              device=sp.DeviceType.GPU)
    dec = sc.ops.ImageDecoder(img=enc, device=sp.DeviceType.GPU)
    out = sp.NamedStream(sc, "imgdec_g_out")
    prof = sc.run(sc.io.Output([dec, enc], [out]),
                  sp.PerfParams.manual(5, 20),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(sp.NamedStream(sc, "imgdec_g_out", column="img").load())
    decoded = list(sp.NamedVideoStream(sc, "imgdec_g_out",
                                       column="frame").load())
    assert len(rows) == len(decoded) == N
    for blob, f in zip(rows, decoded):
        assert f.shape == (OUT_H, OUT_W, 3)
        np.testing.assert_array_equal(f, _core.jpeg_cpu_decode(blob))
    counters = prof.counters()
    assert counters.get("jpeg_gpu_decode_frames", 0) == N
    assert counters.get("image_decode_host_rows", 0) == 0


def colour_files():
    """Files of one shape (the GPU Histogram takes uniform batches) from
    every source: device rows of three kinds, a PNG, a JPEG without DRI."""
    shape = (40, 56, 3)
    return [case_file("40x56_420_rst1", "noise", 75, s) for s in range(3)] + \
        [pillow_save(image(shape, "noise"), "PNG"),
         pillow_jpeg(shape, "smooth", 75, 2),
         cpu_jpeg(shape, "checker", 60),
         case_file("40x56_rows1_opt", "smooth", 95, 1),
         cpu_jpeg(shape, "smooth", 90, 2),
         case_file("40x56_rows1_opt", "noise", 30, 2)]


def test_pipeline_files_to_histogram_matches_cpu_graph(sc, tmp_path):
    blobs = colour_files()
    paths = write_files(tmp_path, blobs)
    hists = {}
    for name, dev, kw in (("cpu", sp.DeviceType.CPU, {}),
                          ("gpu", sp.DeviceType.GPU, dict(gpu_ids=[0]))):
        frames = sc.ops.ImageDecoder(img=sc.sources.Files(paths), device=dev)
        hist = sc.ops.Histogram(frame=frames, device=dev)
        out = sp.NamedStream(sc, "imgdec_h_" + name)
        prof = sc.run(sc.io.Output(hist, [out]), sp.PerfParams.manual(4, 8),
                      cache_mode=sp.CacheMode.Overwrite, **kw)
        hists[name] = list(out.load())
        if name == "gpu":
            host = sum(1 for b in blobs if b[:2] != b"\xff\xd8" or
                       _core.jpeg_decode_info(b)["restart_interval"] == 0)
            counters = prof.counters()
            assert counters.get("image_decode_host_rows", 0) == host > 0
            assert counters.get("jpeg_gpu_decode_frames", 0) == \
                len(blobs) - host > 0
    assert len(hists["cpu"]) == len(blobs)
    assert hists["gpu"] == hists["cpu"]


def test_pipeline_null_rows_and_alternating_shapes(sc, tmp_path):
    """Null rows pass through; a batch whose rows alternate between two
    shapes (and between grey and colour) is decoded in one call."""
    blobs = []
    for s in range(6):
        blobs.append(case_file("17x33_420" if s % 2 else "nine_segments",
                               "noise", 75, s))
    col = sc.sources.Files(write_files(tmp_path, blobs))
    spaced = sc.streams.RepeatNull(col, [2])
    frames = sc.ops.ImageDecoder(img=spaced, device=sp.DeviceType.GPU)
    packed = sc.ops.ImageDecodePackFrame(frame=frames)
    out = sp.NamedStream(sc, "imgdec_n_out")
    prof = sc.run(sc.io.Output(packed, [out]), sp.PerfParams.manual(12, 12),
                  cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    rows = list(out.load())
    assert len(rows) == 12
    assert all(r is None for r in rows[1::2])
    for blob, row in zip(blobs, rows[0::2]):
        np.testing.assert_array_equal(unpack_frame(row),
                                      _core.jpeg_cpu_decode(blob))
    assert prof.counters().get("jpeg_gpu_decode_frames", 0) == 6


def test_pipeline_names_the_corrupt_row(sc, tmp_path):
    bad = next(b for b in entropy_mutations()
               if isinstance(outcome(_core.jpeg_cpu_decode, b), Exception)
               and not isinstance(outcome(_core.jpeg_decode_info, b),
                                  Exception))
    col = sc.sources.Files(write_files(tmp_path, [entropy_base(), bad]))
    frames = sc.ops.ImageDecoder(img=col, device=sp.DeviceType.GPU)
    out = sp.NamedVideoStream(sc, "imgdec_bad_out")
    with pytest.raises(Exception, match="row 1 .*corrupt JPEG entropy data"):
        sc.run(sc.io.Output(frames, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
