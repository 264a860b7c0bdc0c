"""GPU decode of progressive JPEG (kernels/jpeg_progressive_decode.hip) and
the ImageDecoder argument progressive="decode". The contract is byte
identity with the CPU decoder, which test_jpeg_progressive_cpu.py holds to
the baseline file of the same image; there is no tolerance anywhere in this
file. The corrupt files used here have gone through the sanitizer build of
the shared header in test_jpeg_progressive_fuzz.py."""
import numpy as np
import pytest

import scanner_amd as sp
from scanner_amd import _core
import jpeg_progressive_cases as pc
from test_image_decode_cpu import pillow_jpeg, pillow_save, write_files
from test_jpeg_cpu import image

pytestmark = pytest.mark.gpu

DECODE = dict(progressive="decode")


def device_decode(blobs, serial_scan="host"):
    """(frames, host_rows, stats) of one call."""
    return _core.jpeg_gpu_decode(list(blobs), host_rows=True, stats=True,
                                 serial_scan=serial_scan, **DECODE)


def assert_frames_equal(got, blobs):
    assert len(got) == len(blobs)
    for k, (g, b) in enumerate(zip(got, blobs)):
        want = _core.image_cpu_decode(b, **DECODE)
        assert g.shape == want.shape, k
        np.testing.assert_array_equal(g, want, err_msg=f"row {k}")


def outcome(fn, *args):
    try:
        return fn(*args)
    except Exception as e:  # noqa: BLE001 - the class is checked by callers
        return e


def batches_of_1_3_9(files):
    """Every one of 12 files, in batches of 1, 3 and 9."""
    assert len(files) == 12
    return [files[0:1], files[1:4], files[3:12]]


# ---------------- device identity ----------------

@pytest.mark.parametrize("shape", [s for s, _, _ in pc.IDENTITY_SHAPES],
                         ids=lambda s: "x".join(map(str, s)))
def test_device_equals_cpu_with_restart_markers(shape):
    prefix = "x".join(map(str, shape)) + "_"
    files = [prog for name, _, prog in pc.identity_cases(True)
             if name.startswith(prefix)]
    for blobs in batches_of_1_3_9(files):
        frames, host_rows, stats = device_decode(blobs)
        assert host_rows == 0
        assert stats["progressive_rows"] == len(blobs)
        assert_frames_equal(frames, blobs)


def test_device_equals_cpu_on_the_writers_scripts():
    cases = pc.writer_cases()
    dri = [name for name, c in cases.items() if c[4]]
    assert len(dri) >= 7 and "dri_changes_420" in dri
    blobs = [cases[name][1] for name in dri]
    for batch in (blobs[:1], blobs[1:4], (blobs + blobs)[:9]):
        frames, host_rows, stats = device_decode(batch)
        assert host_rows == 0 and stats["progressive_rows"] == len(batch)
        assert_frames_equal(frames, batch)
    # a complete script gives the baseline file's pixels
    for name in dri:
        base, prog, _, stops_early, _ = cases[name]
        if not stops_early:
            np.testing.assert_array_equal(device_decode([prog])[0][0],
                                          _core.jpeg_cpu_decode(base))


# ---------------- files without restart markers ----------------

def nodri_files():
    cases = pc.writer_cases()
    files = [cases[name][1] for name, c in cases.items() if not c[4]]
    assert cases["constant_272_blocks"][1] in files
    assert cases["dri_switched_off_grey"][1] in files
    for shape, sub, _ in pc.IDENTITY_SHAPES:
        files.append(pc.pillow_pair(shape, "noise", 50, sub)[1])
    files.append(pc.pillow_pair((40, 56, 3), "smooth", 90, 1, "optimize")[1])
    return files


def test_files_without_restart_markers_go_where_serial_scan_says():
    files = nodri_files()
    frames, host_rows, stats = device_decode(files, serial_scan="device")
    assert host_rows == 0 and stats["progressive_rows"] == len(files)
    assert_frames_equal(frames, files)
    frames, host_rows, stats = device_decode(files)
    assert host_rows == len(files) and stats["progressive_rows"] == 0
    assert_frames_equal(frames, files)


def test_a_file_with_too_many_scans_is_a_host_row():
    """33 scans, one more than a batch gets launches for: AC bands of one
    coefficient each."""
    base = pc.writer_bases()["grey"]
    script = [pc.scan([0], 0, 0, 0, 0, dri=2)]
    script += [pc.scan([0], k, k, 0, 0) for k in range(1, 32)]
    script.append(pc.scan([0], 32, 63, 0, 0))
    assert len(script) == 33
    prog, _ = pc.write_progressive(base, script)
    np.testing.assert_array_equal(_core.jpeg_cpu_decode(prog, **DECODE),
                                  _core.jpeg_cpu_decode(base))
    fits, _ = pc.write_progressive(base, script[:31] + [
        pc.scan([0], 31, 63, 0, 0)])
    frames, host_rows, stats = device_decode([prog, fits])
    assert host_rows == 1 and stats["progressive_rows"] == 1
    assert_frames_equal(frames, [prog, fits])


# ---------------- mixed batch ----------------

def mixed_batch():
    """(files, progressive rows on the device, host rows) under the default
    serial_scan: baseline and progressive, with and without DRI, PNG, grey,
    and 4, 6, 8, 10 and 16 scans."""
    cases = pc.writer_cases()
    files = [
        pillow_jpeg((40, 56, 3), "noise", 75, 2, "rst1", 1),   # baseline DRI
        pc.pillow_pair((40, 56, 3), "noise", 75, 2, "rst1")[1],  # 10 scans
        pillow_jpeg((17, 33, 3), "smooth", 75, 2),             # baseline
        pc.pillow_pair((17, 33, 3), "smooth", 75, 2)[1],       # host row
        pillow_save(image((7, 9, 3), "noise"), "PNG"),
        pc.pillow_pair((72, 72, 1), "noise", 50, 0, "rst1")[1],  # 6 scans
        cases["dri_changes_420"][1],                           # 8 scans
        cases["successive_from_3_420_dri"][1],                 # 16 scans
        cases["dri_switched_off_grey"][1],                     # host row
        cases["dc_per_component_444_dri"][1],                  # 6 scans
    ]
    return files, 5, 4


def test_mixed_batch_keeps_order_shapes_and_pixels():
    files, on_device, on_host = mixed_batch()
    scans = [len(_core.jpeg_decode_info(f, **DECODE)["scans"])
             for f in files if f[:2] == b"\xff\xd8"]
    assert {0, 4, 6, 8, 10, 16} <= set(scans)
    frames, host_rows, stats = device_decode(files)
    assert host_rows == on_host and stats["progressive_rows"] == on_device
    assert_frames_equal(frames, files)
    # the baseline file without DRI goes to the self-synchronising decoder,
    # whose CPU model says whether it hands the row back
    fell_back = int(_core.jpeg_sync_model(files[2], 0)[1]["fallback"])
    frames, host_rows, stats = device_decode(files, serial_scan="device")
    assert host_rows == 1 + fell_back
    assert stats["progressive_rows"] == on_device + 2
    assert_frames_equal(frames, files)


def test_two_runs_give_equal_bytes():
    files, _, _ = mixed_batch()
    a = device_decode(files, serial_scan="device")[0]
    b = device_decode(files, serial_scan="device")[0]
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_default_still_rejects_and_names_the_row():
    base, prog = pc.pillow_pair((16, 24, 3), "smooth", 75, 0, "rst2")
    with pytest.raises(Exception, match="row 1 .*progressive"):
        _core.jpeg_gpu_decode([base, prog])
    with pytest.raises(Exception,
                       match=r"progressive=reject\|decode, got 'maybe'"):
        _core.jpeg_gpu_decode([base], progressive="maybe")


# ---------------- error parity ----------------

def test_corrupt_scans_give_the_cpu_decoders_verdict():
    """The 32 corruptions of the entropy-coded bytes: the device gives the
    CPU decoder's pixels, or its message with the row named."""
    good = pc.entropy_base()
    info = _core.jpeg_decode_info(good, **DECODE)
    assert all(s["restart_interval"] for s in info["scans"])
    raised = entropy_errors = 0
    for k, blob in enumerate(pc.entropy_mutations()):
        cpu = outcome(lambda b: _core.jpeg_cpu_decode(b, **DECODE), blob)
        gpu = outcome(lambda b: device_decode([good, b])[0][1], blob)
        if isinstance(cpu, Exception):
            raised += 1
            assert isinstance(gpu, Exception), k
            assert type(gpu) is type(cpu), k
            assert "row 1" in str(gpu), (k, str(gpu))
            if "corrupt JPEG" in str(cpu):  # same cause, segment and scan
                entropy_errors += 1
                assert " of scan " in str(cpu)
                assert str(cpu).split("corrupt JPEG")[-1] == \
                    str(gpu).split("corrupt JPEG")[-1], (k, str(gpu))
        else:
            assert not isinstance(gpu, Exception), (k, str(gpu))
            np.testing.assert_array_equal(gpu, cpu, err_msg=f"mutation {k}")
    assert 0 < raised < 32 and entropy_errors > 0
    # the good file shared batches with bad ones; on its own it is intact
    frames, host_rows, _ = device_decode([good])
    assert host_rows == 0
    assert_frames_equal(frames, [good])


# ---------------- pipelines ----------------

def test_pipeline_files_to_histogram_matches_cpu_graph(sc, tmp_path):
    shape = (40, 56, 3)
    blobs = [pc.pillow_pair(shape, "noise", 75, 2, "rst1", 1)[1],
             pillow_jpeg(shape, "noise", 75, 2, "rst1", 1),
             pc.pillow_pair(shape, "smooth", 90, 0, "rows1")[1],
             pillow_save(image(shape, "noise"), "PNG"),
             pc.pillow_pair(shape, "checker", 60, 1)[1],          # no DRI
             pc.pillow_pair(shape, "noise", 30, 1, "rst2", 2)[1],
             pillow_jpeg(shape, "smooth", 75, 0)]                 # no DRI
    paths = write_files(tmp_path, blobs)
    hists, counters = {}, {}
    for name, dev, kw in (("cpu", sp.DeviceType.CPU, {}),
                          ("gpu", sp.DeviceType.GPU, dict(gpu_ids=[0]))):
        frames = sc.ops.ImageDecoder(img=sc.sources.Files(paths), device=dev,
                                     **DECODE)
        hist = sc.ops.Histogram(frame=frames, device=dev)
        out = sp.NamedStream(sc, "jprog_h_" + name)
        prof = sc.run(sc.io.Output(hist, [out]), sp.PerfParams.manual(4, 8),
                      cache_mode=sp.CacheMode.Overwrite, **kw)
        hists[name] = list(out.load())
        counters[name] = prof.counters()
    assert len(hists["cpu"]) == len(blobs)
    assert hists["gpu"] == hists["cpu"]
    c = counters["gpu"]
    assert c.get("jpeg_gpu_progressive_frames", 0) == 3
    assert c.get("jpeg_gpu_decode_frames", 0) == 4
    assert c.get("image_decode_host_rows", 0) == 3


def test_pipeline_default_still_fails_naming_the_row(sc, tmp_path):
    base, prog = pc.pillow_pair((16, 24, 3), "smooth", 75, 0, "rst2")
    col = sc.sources.Files(write_files(tmp_path, [base, prog]))
    frames = sc.ops.ImageDecoder(img=col, device=sp.DeviceType.GPU)
    out = sp.NamedVideoStream(sc, "jprog_bad_out")
    with pytest.raises(Exception, match="row 1 .*progressive"):
        sc.run(sc.io.Output(frames, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
    frames = sc.ops.ImageDecoder(img=col, device=sp.DeviceType.GPU,
                                 progressive="maybe")
    with pytest.raises(Exception,
                       match=r"progressive=reject\|decode, got 'maybe'"):
        sc.run(sc.io.Output(frames, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
