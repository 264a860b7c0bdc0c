"""The self-synchronising JPEG decoder's CPU model (csrc/ops/jpeg_sync_cpu.cpp
over jpeg_sync_common.h): the algorithm of kernels/jpeg_sync_decode.hip run
lane by lane on files without restart markers. The contract is byte identity
with jpeg_cpu_decode, whether the model verified its own result or fell back
to the serial decoder; there is no tolerance anywhere in this file."""
import numpy as np
import pytest

import scanner_amd as sp
from scanner_amd import _core
from test_image_decode_cpu import (PILLOW_CONTENTS, PILLOW_IDS, PILLOW_SHAPES,
                                   pillow_save, write_files)
from test_image_decode_fuzz import _frame, _save, scan_range
from test_jpeg_cpu import image

DEFAULT_CB = _core.jpeg_sync_chunk_bytes() if hasattr(
    _core, "jpeg_sync_chunk_bytes") else 0
CHUNK_BYTES = [4, 16, 64, 0]          # 0: the default
QUALITIES = [1, 50, 100]
# Pillow's subsampling argument per colour shape: 4:4:4, 4:2:2, 4:2:0, 4:2:0
SUBSAMPLING = {(7, 9, 3): 0, (16, 24, 3): 1, (17, 33, 3): 2, (40, 56, 3): 2}


def plain_jpeg(shape, content, quality, optimize=False, seed=0):
    """A Pillow file without a DRI segment."""
    kw = dict(quality=quality, optimize=optimize)
    if shape[2] == 3:
        kw["subsampling"] = SUBSAMPLING[shape]
    return pillow_save(image(shape, content, seed), **kw)


def case_list(shape):
    """(content, quality, optimize, blob) of one shape."""
    return [(content, q, opt, plain_jpeg(shape, content, q, opt))
            for content in PILLOW_CONTENTS for q in QUALITIES
            for opt in (False, True)]


def model(blob, cb=0):
    return _core.jpeg_sync_model(blob, cb)


# The cases the model gives back to the serial decoder. The issue allows at
# most the q100 noise files at 4- and 16-byte chunks; the model needs only
# this one: 1216 chunks in 5 groups, one more than kJpegSyncMaxRounds = 3
# rounds across groups make exact, and its sync distance is longer than a
# group of 256 x 4 bytes.
FALLBACK = {((40, 56, 3), "noise", 100, False, 4)}


def test_feature_bindings_exist():
    assert DEFAULT_CB in (32, 64, 128, 256)
    pix, stats = model(plain_jpeg((8, 8, 1), "smooth", 50))
    assert pix.shape == (8, 8, 1) and pix.dtype == np.uint8
    assert {"chunks", "groups", "group_iterations", "cross_rounds",
            "cross_repairs", "stuffed_starts", "empty_chunks", "verified",
            "fallback"} <= set(stats)


@pytest.mark.parametrize("shape", PILLOW_SHAPES, ids=PILLOW_IDS)
def test_pixels_equal_the_serial_decoder(shape):
    for content, q, opt, blob in case_list(shape):
        assert _core.jpeg_decode_info(blob)["restart_interval"] == 0
        want = _core.jpeg_cpu_decode(blob)
        for cb in CHUNK_BYTES:
            got, stats = model(blob, cb)
            key = (shape, content, q, opt, cb)
            np.testing.assert_array_equal(got, want, err_msg=str(key))
            assert stats["fallback"] == (key in FALLBACK), (key, stats)
            assert stats["verified"] != stats["fallback"]
            assert stats["chunks"] == max(
                1, -(-(np.diff(scan_range(blob))[0]) // (cb or DEFAULT_CB)))
            assert stats["groups"] == -(-stats["chunks"] // 256)


def test_default_chunk_size_is_what_zero_means():
    blob = plain_jpeg((40, 56, 3), "noise", 50)
    assert model(blob, 0)[1] == model(blob, DEFAULT_CB)[1]


def test_bad_chunk_sizes_are_rejected():
    blob = plain_jpeg((8, 8, 1), "smooth", 50)
    for cb in (1, 2, 3, 24, 100):
        with pytest.raises(Exception, match="power of two"):
            model(blob, cb)


def test_files_with_restart_markers_are_rejected():
    blob = pillow_save(image((16, 24, 3), "noise"), quality=75,
                       restart_marker_blocks=2)
    with pytest.raises(Exception, match="without restart markers"):
        model(blob, 16)


# ---- edge cases, each on a named file chosen from the model's stats ----

def grey_noise(q):
    return plain_jpeg((33, 50, 1), "noise", q)


def test_more_than_one_group():
    """(33,50,1) noise q90 at 4-byte chunks: 300-odd chunks, two groups."""
    blob = pillow_save(image((33, 50, 1), "noise"), quality=90)
    got, stats = model(blob, 4)
    assert stats["chunks"] > 256 and stats["groups"] == 2
    assert stats["verified"]
    np.testing.assert_array_equal(got, _core.jpeg_cpu_decode(blob))


def test_chunks_that_start_on_a_stuffed_zero():
    blob = grey_noise(100)
    lo, hi = scan_range(blob)
    on_stuffing = sum(1 for c in range(1, -(-(hi - lo) // 4))
                      if blob[lo + 4 * c] == 0 and blob[lo + 4 * c - 1] == 0xff)
    got, stats = model(blob, 4)
    assert stats["stuffed_starts"] == on_stuffing > 0
    assert stats["verified"]
    np.testing.assert_array_equal(got, _core.jpeg_cpu_decode(blob))


def test_a_chunk_without_a_symbol_boundary():
    """A symbol and its value bits can span a whole 4-byte chunk; the lane of
    that chunk decodes nothing."""
    got, stats = model(grey_noise(100), 4)
    assert stats["empty_chunks"] > 0 and stats["verified"]


def test_one_chunk_file():
    blob = plain_jpeg((1, 1, 1), "smooth", 50)
    for cb in (64, 0):
        got, stats = model(blob, cb)
        assert stats["chunks"] == stats["groups"] == 1
        assert stats["group_iterations"] == 1 and stats["cross_rounds"] == 0
        assert stats["verified"]
        np.testing.assert_array_equal(got, _core.jpeg_cpu_decode(blob))


def test_in_group_loop_iterates_to_its_fixed_point():
    """The sync distance is far longer than a chunk or two: at 4-byte chunks
    the loop runs to its bound, at 64-byte chunks still more than 8 times."""
    blob = plain_jpeg((40, 56, 3), "noise", 100)
    assert model(blob, 4)[1]["group_iterations"] == 256
    got, stats = model(blob, 64)
    assert 8 < stats["group_iterations"] < 256 and stats["verified"]


def test_cross_group_repair():
    got, stats = model(grey_noise(100), 4)
    assert stats["groups"] == 3
    assert stats["cross_repairs"] > 0 and stats["cross_rounds"] > 0
    assert stats["verified"]


def test_the_fallback_case_is_a_verification_failure():
    blob = plain_jpeg((40, 56, 3), "noise", 100)
    got, stats = model(blob, 4)
    assert stats["groups"] == 5 and stats["fallback"]
    assert stats["status"] == 4  # a writing walk missed its recorded exit
    np.testing.assert_array_equal(got, _core.jpeg_cpu_decode(blob))


# ---- the op argument on the CPU kernel: accepted, nothing to choose ----

def test_op_accepts_serial_scan_on_the_cpu(sc, tmp_path):
    blobs = [plain_jpeg((40, 56, 3), "noise", 75),
             plain_jpeg((40, 56, 3), "smooth", 50, True)]
    col = sc.sources.Files(write_files(tmp_path, blobs))
    for k, value in enumerate(("device", "host")):
        frames = sc.ops.ImageDecoder(img=col, serial_scan=value)
        out = sp.NamedVideoStream(sc, f"jsync_cpu_{k}")
        sc.run(sc.io.Output(frames, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite)
        got = list(out.load())
        assert len(got) == len(blobs)
        for f, b in zip(got, blobs):
            np.testing.assert_array_equal(f, _core.jpeg_cpu_decode(b))


def test_op_rejects_an_unknown_serial_scan_by_name(sc, tmp_path):
    col = sc.sources.Files(write_files(
        tmp_path, [plain_jpeg((40, 56, 3), "smooth", 50)]))
    frames = sc.ops.ImageDecoder(img=col, serial_scan="both")
    out = sp.NamedVideoStream(sc, "jsync_cpu_bad")
    with pytest.raises(Exception, match=r"serial_scan=host\|device.*'both'"):
        sc.run(sc.io.Output(frames, [out]), sp.PerfParams.manual(4, 8),
               cache_mode=sp.CacheMode.Overwrite)


# ---- corrupt entropy-coded data ----

def nodri_base():
    """The (16,24,3) file of test_image_decode_fuzz.entropy_base, saved
    without restart markers."""
    return _save(_frame(16, 24, 3, 6), "JPEG", quality=90, subsampling=0)


def nodri_mutations(n=32, seed=11):
    """entropy_mutations() of that file: three in four flip 1..3 bits of the
    entropy-coded data, the fourth cuts a piece out of it."""
    base = nodri_base()
    lo, hi = scan_range(base)
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        b = bytearray(base)
        if i % 4 == 3:
            a = rs.randint(lo, hi)
            e = rs.randint(a, hi) + 1
            del b[a:e]
        else:
            for _ in range(rs.randint(1, 4)):
                b[rs.randint(lo, hi)] ^= 1 << rs.randint(0, 8)
        out.append(bytes(b))
    return out


def outcome(fn, *args):
    try:
        return fn(*args)
    except Exception as e:  # noqa: BLE001 - the class is checked by callers
        return e


def test_corrupt_data_never_gives_other_pixels():
    assert _core.jpeg_decode_info(nodri_base())["restart_interval"] == 0
    raised = verified = 0
    for k, blob in enumerate(nodri_mutations()):
        cpu = outcome(_core.jpeg_cpu_decode, blob)
        for cb in (4, 16, 64, 0):
            got = outcome(model, blob, cb)
            if isinstance(cpu, Exception):
                # fallback is the serial decoder, and that raises
                assert isinstance(got, Exception), (k, cb)
                assert type(got) is type(cpu) and str(got) == str(cpu), (k, cb)
                raised += 1
            else:
                assert not isinstance(got, Exception), (k, cb, str(got))
                np.testing.assert_array_equal(got[0], cpu,
                                              err_msg=f"mutation {k} cb {cb}")
                verified += got[1]["verified"]
    assert raised > 0 and verified > 0
