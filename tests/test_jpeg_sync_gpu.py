"""GPU decode of JPEG files without restart markers
(kernels/jpeg_sync_decode.hip) and the ImageDecoder argument
serial_scan="device". The contract is byte identity with the CPU decoder,
and the same verdict (device row or fallback) as the CPU model of
test_jpeg_sync_cpu.py; there is no tolerance anywhere in this file. The
corrupt files used here have gone through the sanitizer build of the shared
header in test_jpeg_sync_fuzz.py."""
import numpy as np
import pytest

import scanner_amd as sp
from scanner_amd import _core
from test_image_decode_cpu import (PILLOW_CONTENTS, PILLOW_IDS, PILLOW_SHAPES,
                                   pillow_jpeg, pillow_save, write_files)
from test_jpeg_cpu import cpu_jpeg, image
from test_jpeg_sync_cpu import (QUALITIES, nodri_base, nodri_mutations,
                                outcome, plain_jpeg)

pytestmark = pytest.mark.gpu


def fallbacks(blobs, cb):
    """Rows of the batch the CPU model gives back to the serial decoder."""
    n = 0
    for b in blobs:
        if b[:2] == b"\xff\xd8" and \
                _core.jpeg_decode_info(b)["restart_interval"] == 0:
            n += bool(_core.jpeg_sync_model(b, cb)[1]["fallback"])
    return n


def device_decode(blobs, cb=0, serial_scan="device"):
    """(frames, host_rows, stats) of one call."""
    return _core.jpeg_gpu_decode(list(blobs), host_rows=True,
                                 serial_scan=serial_scan, chunk_bytes=cb,
                                 stats=True)


def assert_frames_equal(got, blobs):
    assert len(got) == len(blobs)
    for k, (g, b) in enumerate(zip(got, blobs)):
        want = _core.image_cpu_decode(b)
        assert g.shape == want.shape, k
        np.testing.assert_array_equal(g, want, err_msg=f"row {k}")


@pytest.mark.parametrize("shape", PILLOW_SHAPES, ids=PILLOW_IDS)
def test_device_equals_cpu(shape):
    """Batches of 1, 3 and 9 different files at 4-byte chunks, 64-byte
    chunks and the default; the rows that fall back are the model's."""
    for content in PILLOW_CONTENTS:
        for q in QUALITIES:
            for opt in (False, True):
                files = [plain_jpeg(shape, content, q, opt, seed)
                         for seed in range(9)]
                for n in (1, 3, 9):
                    for cb in (4, 64, 0):
                        blobs = files[:n]
                        frames, host_rows, stats = device_decode(blobs, cb)
                        key = (content, q, opt, n, cb)
                        assert_frames_equal(frames, blobs)
                        want_host = fallbacks(blobs, cb)
                        assert host_rows == want_host, key
                        assert stats["fallback_rows"] == want_host, key
                        assert stats["sync_rows"] == n - want_host, key
                        if cb != 4:
                            assert want_host == 0, key


def test_mixed_batch_keeps_order_and_counts_host_rows():
    q100 = plain_jpeg((40, 56, 3), "noise", 100)
    blobs = [
        pillow_jpeg((17, 33, 3), "noise", 50, 2, "rst2", 0),       # DRI
        plain_jpeg((7, 9, 3), "noise", 50),                        # 4:4:4
        pillow_save(image((7, 9, 3), "noise"), "PNG"),
        plain_jpeg((16, 24, 3), "smooth", 100),                    # 4:2:2
        q100,                                                      # 4:2:0
        plain_jpeg((33, 50, 1), "noise", 100),                     # grey
        cpu_jpeg((136, 128, 1), "smooth", 90, 1),                  # DRI, grey
        plain_jpeg((17, 33, 3), "checker", 1, True),               # 4:2:0
        pillow_jpeg((40, 56, 3), "noise", 95, 2, "rst1", 5),       # DRI
    ]
    dri = sum(1 for b in blobs if b[:2] == b"\xff\xd8" and
              _core.jpeg_decode_info(b)["restart_interval"] > 0)
    assert dri == 3
    assert _core.jpeg_sync_model(q100, 4)[1]["fallback"]
    want_fb = fallbacks(blobs, 4)
    assert want_fb >= 1
    frames, host_rows, stats = device_decode(blobs, 4)
    assert_frames_equal(frames, blobs)
    assert host_rows == 1 + want_fb
    assert stats == {"sync_rows": 5 - want_fb, "fallback_rows": want_fb}
    # at the default chunk size nothing falls back
    frames, host_rows, stats = device_decode(blobs)
    assert_frames_equal(frames, blobs)
    assert host_rows == 1 and stats == {"sync_rows": 5, "fallback_rows": 0}
    # not asked for: the host rows of today
    frames, host_rows, stats = device_decode(blobs, serial_scan="host")
    assert_frames_equal(frames, blobs)
    assert host_rows == 6 and stats == {"sync_rows": 0, "fallback_rows": 0}
    assert _core.jpeg_gpu_decode(blobs, host_rows=True)[1] == 6


def test_bad_arguments_are_rejected_by_name():
    blob = plain_jpeg((8, 8, 1), "smooth", 50)
    with pytest.raises(Exception, match="serial_scan"):
        _core.jpeg_gpu_decode([blob], serial_scan="gpu")
    with pytest.raises(Exception, match="power of two"):
        _core.jpeg_gpu_decode([blob], serial_scan="device", chunk_bytes=24)


def frame_256():
    h = w = 256
    yy, xx = np.mgrid[0:h, 0:w]
    frame = np.stack([(xx + yy) % 256, (2 * yy) % 256, (xx // 2) % 256],
                     -1).astype(np.uint8)
    noise = np.random.RandomState(5).randint(0, 256, (h // 2, w // 2, 3))
    frame[:h // 2, w // 2:] = noise  # one textured quadrant
    return frame


def test_one_256x256_file_in_several_groups():
    """4:2:0 q90 with one noise quadrant, some 20 KB of scan: at the default
    chunk size, twice, and at 32- and 8-byte chunks, which make several and
    some ten groups of it."""
    blob = pillow_save(frame_256(), quality=90, subsampling=2)
    assert _core.jpeg_sync_model(blob, 32)[1]["groups"] >= 3
    assert _core.jpeg_sync_model(blob, 8)[1]["groups"] >= 8
    first = None
    for cb in (0, 0, 32, 8):
        frames, host_rows, stats = device_decode([blob], cb)
        assert host_rows == fallbacks([blob], cb) == 0, cb
        assert stats["sync_rows"] == 1
        assert_frames_equal(frames, [blob])
        if first is None:
            first = frames
        np.testing.assert_array_equal(first[0], frames[0])


def test_error_parity_on_corrupt_entropy_data():
    """32 corruptions confined to the entropy-coded data of a (16,24,3) file
    without DRI, each behind a good file: the device path returns the CPU
    decoder's pixels or raises its error for row 1."""
    good = nodri_base()
    raised = 0
    for k, blob in enumerate(nodri_mutations()):
        cpu = outcome(_core.jpeg_cpu_decode, blob)
        for cb in (4, 0):
            gpu = outcome(lambda b: _core.jpeg_gpu_decode(
                [good, b], serial_scan="device", chunk_bytes=cb)[1], blob)
            if isinstance(cpu, Exception):
                raised += 1
                assert isinstance(gpu, Exception), (k, cb)
                assert type(gpu) is type(cpu), (k, cb)
                assert "row 1" in str(gpu), (k, str(gpu))
                if "corrupt JPEG" in str(cpu):
                    assert str(cpu).split("corrupt JPEG")[-1] == \
                        str(gpu).split("corrupt JPEG")[-1], (k, str(gpu))
            else:
                assert not isinstance(gpu, Exception), (k, cb, str(gpu))
                np.testing.assert_array_equal(gpu, cpu,
                                              err_msg=f"mutation {k} cb {cb}")
    assert 0 < raised < 64
    frames, host_rows, _ = device_decode([good])
    assert host_rows == 0
    assert_frames_equal(frames, [good])


# ---------------- op and pipeline ----------------

def colour_files():
    """Nine (40,56,3) files of every kind: without DRI in three samplings,
    plain and optimised, with DRI from Pillow and from our encoder, a PNG."""
    shape = (40, 56, 3)
    img = image(shape, "noise", 3)
    return [plain_jpeg(shape, "noise", 75, False, 0),
            pillow_save(img, quality=90, subsampling=0),
            pillow_jpeg(shape, "noise", 75, 2, "rst1", 1),
            pillow_save(image(shape, "noise"), "PNG"),
            pillow_save(img, quality=60, subsampling=1, optimize=True),
            cpu_jpeg(shape, "checker", 60),
            plain_jpeg(shape, "smooth", 100, True, 2),
            pillow_jpeg(shape, "smooth", 95, 1, "rows1_opt", 1),
            plain_jpeg(shape, "checker", 1, False, 1)]


def test_pipeline_files_to_histogram_matches_cpu_graph(sc, tmp_path):
    blobs = colour_files()
    png = sum(1 for b in blobs if b[:2] != b"\xff\xd8")
    nodri = sum(1 for b in blobs if b[:2] == b"\xff\xd8" and
                _core.jpeg_decode_info(b)["restart_interval"] == 0)
    assert png == 1 and nodri == 5
    assert fallbacks(blobs, 0) == 0
    paths = write_files(tmp_path, blobs)
    hists, counters = {}, {}
    for name, dev, kw, args in (
            ("cpu", sp.DeviceType.CPU, {}, dict(serial_scan="device")),
            ("device", sp.DeviceType.GPU, dict(gpu_ids=[0]),
             dict(serial_scan="device")),
            ("default", sp.DeviceType.GPU, dict(gpu_ids=[0]), {})):
        frames = sc.ops.ImageDecoder(img=sc.sources.Files(paths), device=dev,
                                     **args)
        hist = sc.ops.Histogram(frame=frames, device=dev)
        out = sp.NamedStream(sc, "jsync_h_" + name)
        prof = sc.run(sc.io.Output(hist, [out]), sp.PerfParams.manual(4, 8),
                      cache_mode=sp.CacheMode.Overwrite, **kw)
        hists[name] = list(out.load())
        counters[name] = prof.counters()
    assert len(hists["cpu"]) == len(blobs)
    assert hists["device"] == hists["cpu"]
    assert hists["default"] == hists["cpu"]
    c = counters["device"]
    assert c.get("jpeg_gpu_sync_frames", 0) == nodri
    assert c.get("jpeg_sync_fallback_rows", 0) == 0
    assert c.get("image_decode_host_rows", 0) == png
    assert c.get("jpeg_gpu_decode_frames", 0) == len(blobs) - png
    c = counters["default"]
    assert c.get("jpeg_gpu_sync_frames", 0) == 0
    assert c.get("image_decode_host_rows", 0) == png + nodri
    assert c.get("jpeg_gpu_decode_frames", 0) == len(blobs) - png - nodri


def test_op_rejects_an_unknown_serial_scan(sc, tmp_path):
    paths = write_files(tmp_path, [plain_jpeg((40, 56, 3), "smooth", 50)])
    frames = sc.ops.ImageDecoder(img=sc.sources.Files(paths),
                                 device=sp.DeviceType.GPU, serial_scan="both")
    out = sp.NamedVideoStream(sc, "jsync_bad_out")
    with pytest.raises(Exception, match=r"serial_scan=host\|device.*'both'"):
        sc.run(sc.io.Output(frames, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
