"""Progressive JPEG (SOF2) in the CPU decoder, opt-in through
progressive="decode". The contract is identity with the baseline file of the
same image: the same quantised coefficients and byte-identical pixels, with
no tolerance anywhere. Inputs: jpeg_progressive_cases.py."""
import numpy as np
import pytest

import scanner_amd as sp
from scanner_amd import _core
import jpeg_progressive_cases as pc
import mjpeg_cases as mc
from test_jpeg_cpu import image
from test_image_decode_cpu import (pillow_jpeg, pillow_save, unpack_frame,
                                   write_files)

DECODE = dict(progressive="decode")


def assert_identical(base, prog, name, expect_coefs=None):
    cb = expect_coefs or _core.jpeg_decode_coefficients(base)
    cp = _core.jpeg_decode_coefficients(prog, **DECODE)
    assert len(cb) == len(cp), name
    for c, (x, y) in enumerate(zip(cb, cp)):
        assert x.dtype == y.dtype == np.int16
        np.testing.assert_array_equal(y, x, err_msg=f"{name} component {c}")
    if expect_coefs is None:
        np.testing.assert_array_equal(_core.jpeg_cpu_decode(prog, **DECODE),
                                      _core.jpeg_cpu_decode(base),
                                      err_msg=name)


# ---------------- identity ----------------

@pytest.mark.parametrize("dri", [True, False], ids=["dri", "nodri"])
@pytest.mark.parametrize("shape", [s for s, _, _ in pc.IDENTITY_SHAPES],
                         ids=lambda s: "x".join(map(str, s)))
def test_progressive_equals_baseline(shape, dri):
    cases = [c for c in pc.identity_cases(dri)
             if c[0].startswith("x".join(map(str, shape)) + "_")]
    assert len(cases) == len(pc.IDENTITY_CONTENTS) * len(pc.IDENTITY_QUALITIES)
    for name, base, prog in cases:
        info = _core.jpeg_decode_info(prog, **DECODE)
        assert info["progressive"] and not info["segments"]
        assert len(info["scans"]) == (10 if shape[2] == 3 else 6), name
        if dri:
            assert all(s["restart_interval"] for s in info["scans"]), name
        assert_identical(base, prog, name)


def test_info_lists_the_scans_in_their_own_units():
    """(37,53,3) 4:2:0 with interval 2: interleaved DC scans count MCUs,
    single-component scans the blocks of the component's own raster; the
    file has 2*5 + 4*17 + 4*5 = 98 RSTn markers."""
    base, prog = pc.pillow_pair((37, 53, 3), "noise", 75, 2, "rst2")
    info = _core.jpeg_decode_info(prog, **DECODE)
    assert (info["h"], info["w"], info["c"]) == (37, 53, 3)
    assert (info["hs"], info["vs"], info["mcus"]) == (2, 2, 12)
    units = {(): 12, (0,): 5 * 7, (1,): 3 * 4, (2,): 3 * 4}
    markers = 0
    for s in info["scans"]:
        comps = tuple(s["components"])
        n = units[() if len(comps) == 3 else comps]
        assert s["units"] == n and s["restart_interval"] == 2
        assert s["segment_count"] == len(s["segments"]) == (n + 1) // 2
        assert [g[2] for g in s["segments"]] == list(range(0, n, 2))
        assert sum(g[3] for g in s["segments"]) == n
        markers += s["segment_count"] - 1
    assert markers == 98
    assert {"ss", "se", "ah", "al"} <= set(info["scans"][0])
    base_info = _core.jpeg_decode_info(base)
    assert base_info["progressive"] is False and base_info["scans"] == []
    assert_identical(base, prog, "37x53")


def test_coefficients_of_a_baseline_file_are_its_dct():
    """The seam itself: dequantised and inverse transformed, the
    coefficients of a baseline file give its pixels."""
    blob = pillow_jpeg((16, 24, 1), "noise", 90)
    (c,) = _core.jpeg_decode_coefficients(blob)
    assert c.shape == (2, 3, 64) and c.dtype == np.int16
    q = np.frombuffer(blob[blob.index(b"\xff\xdb") + 5:][:64], np.uint8)
    nat = np.zeros(64, np.int32)
    nat[pc.ZZ] = q
    deq = np.clip(c.astype(np.int32) * nat, -4096, 4096).reshape(-1, 64)
    pix = _core.jpeg_idct_blocks(deq).reshape(2, 3, 8, 8)
    got = pix.transpose(0, 2, 1, 3).reshape(16, 24, 1)
    np.testing.assert_array_equal(got, _core.jpeg_cpu_decode(blob))


# ---------------- the writer's scripts ----------------

def test_writer_case_list_reaches_every_branch():
    counts = [c for _, _, c, _, _ in pc.writer_cases().values()]
    assert any(c["multi_block_runs"] for c in counts)
    assert max(c["max_eobrun"] for c in counts) >= 256
    assert pc.writer_cases()["constant_272_blocks"][2]["max_eobrun"] == 272
    assert any(c["refine_zrl"] for c in counts)
    assert any(c["refined_history"] for c in counts)
    assert any(c["correction_bits"] for c in counts)
    assert any(c["runs_cut_by_restart"] for c in counts)
    assert any(n >= 8 for c in counts for n in c["eob"])


@pytest.mark.parametrize("name", list(pc.writer_cases()))
def test_writer_round_trip(name):
    base, prog, _, stops_early, all_dri = pc.writer_cases()[name]
    info = _core.jpeg_decode_info(prog, **DECODE)
    assert all(s["restart_interval"] for s in info["scans"]) == all_dri
    if stops_early:
        expect = pc.clear_unrefined_bit(_core.jpeg_decode_coefficients(base))
        assert any((x != y).any() for x, y in zip(
            expect, _core.jpeg_decode_coefficients(base)))
        assert_identical(base, prog, name, expect)
        # what the file holds is what libjpeg reads from it, too: within the
        # hard cap between the two decoders that test_image_decode_cpu.py
        # derives for RGB (3 for a float64 decoder of the same formulas
        # against Pillow, and 1 per plane sample for the integer IDCT)
        ours = _core.jpeg_cpu_decode(prog, **DECODE).astype(int)
        assert np.abs(ours - pc.pillow_pixels(prog)).max() <= 6
    else:
        assert_identical(base, prog, name)
        np.testing.assert_array_equal(pc.pillow_pixels(prog),
                                      pc.pillow_pixels(base))


def test_writer_restart_interval_follows_the_dri_segments():
    _, prog, _, _, _ = pc.writer_cases()["dri_changes_420"]
    info = _core.jpeg_decode_info(prog, **DECODE)
    assert [s["restart_interval"] for s in info["scans"]] == \
        [2, 3, 3, 3, 1, 5, 5, 5]
    _, prog, _, _, _ = pc.writer_cases()["dri_switched_off_grey"]
    info = _core.jpeg_decode_info(prog, **DECODE)
    assert [s["restart_interval"] for s in info["scans"]] == [3, 3, 0, 0]
    assert [s["segment_count"] for s in info["scans"]] == [12, 12, 1, 1]


# ---------------- script validation ----------------

def patch_scan(blob, k, ss=None, se=None, ah=None, al=None):
    """Scan k of a valid file with some of its SOS parameters replaced."""
    info = _core.jpeg_decode_info(blob, **DECODE)
    at = info["scans"][k]["segments"][0][0]
    b = bytearray(blob)
    if ss is not None:
        b[at - 3] = ss
    if se is not None:
        b[at - 2] = se
    if ah is not None:
        b[at - 1] = ah << 4 | (b[at - 1] & 15)
    if al is not None:
        b[at - 1] = (b[at - 1] & 0xf0) | al
    return bytes(b)


def test_invalid_scan_scripts_are_rejected_by_name():
    base = pc.writer_bases()["444"]
    good, _ = pc.write_progressive(base, pc.script_successive(3, 2))
    _core.jpeg_cpu_decode(good, **DECODE)
    # scans of `good`: 0 DC first Al=2, 1..3 AC first Al=2, 4 DC refine 2->1,
    # 5..7 AC refine 2->1, 8 DC refine 1->0, 9..11 AC refine 1->0
    S = pc.scan
    bad = {
        "Se above 63": (patch_scan(good, 1, se=64), "not a band of 0..63"),
        "Ss above Se": (patch_scan(good, 1, ss=9, se=8),
                        "not a band of 0..63"),
        "DC with AC": (patch_scan(good, 0, se=5), "Se must be 0"),
        "interleaved AC": (patch_scan(good, 0, ss=1, se=5),
                           "an AC scan holds one component"),
        "Al 14": (patch_scan(good, 0, al=14), "above 13"),
        "Ah on a first scan": (patch_scan(good, 0, ah=3),
                               "no scan has coded yet"),
        "Ah is not the last Al": (patch_scan(good, 9, ah=3, al=2),
                                  "was last coded with Al = 1"),
        "Al is not Ah - 1": (patch_scan(good, 5, al=0), "Al must be Ah - 1"),
        "AC before DC": (
            pc.write_progressive(base, [S([0], 1, 63, 0, 0),
                                        S(range(3), 0, 0, 0, 0)])[0],
            "comes before its first DC scan"),
        "coded twice": (
            pc.write_progressive(base, [S(range(3), 0, 0, 0, 0),
                                        S([1], 1, 63, 0, 0),
                                        S([1], 6, 9, 0, 0)])[0],
            "coded a second time"),
    }
    for name, (blob, what) in bad.items():
        for fn in (_core.jpeg_cpu_decode, _core.jpeg_decode_info,
                   _core.jpeg_decode_coefficients):
            with pytest.raises(Exception) as e:
                fn(blob, **DECODE)
            assert "invalid progressive scan script" in str(e.value), name
            assert what in str(e.value), (name, str(e.value))


def test_a_scan_of_two_components_is_rejected_by_name():
    base = pc.writer_bases()["444"]
    blob, _ = pc.write_progressive(base, [pc.scan([0, 1], 0, 0, 0, 0)])
    with pytest.raises(Exception, match="scan of 2 of 3 components"):
        _core.jpeg_cpu_decode(blob, **DECODE)


def test_segment_rules_name_the_scan():
    _, prog = pc.pillow_pair((16, 24, 3), "noise", 90, 0, "rst2")
    info = _core.jpeg_decode_info(prog, **DECODE)
    scan3 = info["scans"][3]
    assert scan3["segment_count"] > 2
    b = bytearray(prog)
    first_rst = scan3["segments"][0][1]
    assert b[first_rst:first_rst + 2] == b"\xff\xd0"
    b[first_rst + 1] = 0xd1
    with pytest.raises(Exception, match="out of sequence.* in scan 3"):
        _core.jpeg_cpu_decode(bytes(b), **DECODE)
    b = bytearray(prog)
    last_rst = scan3["segments"][-2][1]
    del b[last_rst:last_rst + 2]
    with pytest.raises(Exception, match="scan 3 has .* restart segments"):
        _core.jpeg_cpu_decode(bytes(b), **DECODE)
    # EOI has to follow the last scan: a marker-free tail is a truncation
    with pytest.raises(Exception, match="truncated"):
        _core.jpeg_cpu_decode(prog[:-2] + b"\x00\x00", **DECODE)


def test_a_dc_scan_too_short_for_the_frame_is_refused():
    """A header that promises more blocks than the DC-first scan's bytes can
    hold is refused before anything is allocated for it."""
    _, prog = pc.pillow_pair((16, 24, 1), "smooth", 50)
    b = bytearray(prog)
    sof = b.index(b"\xff\xc2")
    b[sof + 5:sof + 9] = (4096).to_bytes(2, "big") * 2
    with pytest.raises(Exception, match="truncated JPEG: the scan is too "
                                        "short"):
        _core.jpeg_cpu_decode(bytes(b), **DECODE)


# ---------------- truncation ----------------

def truncation_cuts(blob):
    info = _core.jpeg_decode_info(blob, **DECODE)
    ends = {s["segments"][0][0]: s["segments"][-1][1] for s in info["scans"]}
    pos, cuts = 2, [2]
    while blob[pos + 1] != 0xd9:
        n = int.from_bytes(blob[pos + 2:pos + 4], "big")
        cuts += [pos + 2, pos + 3, pos + 2 + n // 2, pos + 2 + n]
        marker, pos = blob[pos + 1], pos + 2 + n
        if marker == 0xda:  # the scan's bytes: start, middle, last byte
            end = ends[pos]
            cuts += [pos + 1, (pos + end) // 2, end - 1, end, end + 1]
            pos = end
    assert pos == len(blob) - 2 and len(ends) == len(info["scans"])
    return sorted(set(cuts))


@pytest.mark.parametrize("which", ["pillow_420_rst", "pillow_grey",
                                   "writer_dri_changes"])
def test_truncation_at_every_marker_and_inside_every_scan(which):
    blob = {
        "pillow_420_rst": pc.pillow_pair((17, 33, 3), "noise", 75, 2,
                                         "rst2")[1],
        "pillow_grey": pc.pillow_pair((33, 50, 1), "smooth", 75)[1],
        "writer_dri_changes": pc.writer_cases()["dri_changes_420"][1],
    }[which]
    _core.jpeg_cpu_decode(blob, **DECODE)
    cuts = truncation_cuts(blob)
    assert len(cuts) > 9 * len(_core.jpeg_decode_info(blob, **DECODE)["scans"])
    for cut in cuts:
        with pytest.raises(Exception, match="truncated|marker expected"):
            _core.jpeg_cpu_decode(blob[:cut], **DECODE)


# ---------------- the default is unchanged ----------------

def test_default_still_rejects_progressive_files():
    base, prog = pc.pillow_pair((16, 24, 3), "smooth", 80)
    for fn in (_core.jpeg_cpu_decode, _core.jpeg_decode_info,
               _core.image_cpu_decode, _core.jpeg_decode_coefficients):
        with pytest.raises(Exception, match=r"progressive JPEG \(SOF2\) is "
                                            "not supported"):
            fn(prog)
        with pytest.raises(Exception, match=r"progressive JPEG \(SOF2\) is "
                                            "not supported"):
            fn(prog, progressive="reject")
        with pytest.raises(Exception,
                           match=r"progressive=reject\|decode, got 'maybe'"):
            fn(prog, progressive="maybe")
    # a baseline file reads the same with either value
    np.testing.assert_array_equal(_core.jpeg_cpu_decode(base, **DECODE),
                                  _core.jpeg_cpu_decode(base))
    np.testing.assert_array_equal(_core.image_cpu_decode(prog, **DECODE),
                                  _core.jpeg_cpu_decode(base))


def test_mjpeg_ingest_still_rejects_a_progressive_sample(sc, tmp_path):
    fr = mc.frames(4, 16, 272, 3)
    samples = [mc.pillow_jpeg(f, quality=80) for f in fr]
    samples[3] = mc.pillow_jpeg(fr[3], quality=80, progressive=True)
    path = tmp_path / "prog.mov"
    path.write_bytes(mc.mux_mp4(samples, 272, 16, entry="jpeg"))
    with pytest.raises(Exception, match=r"sample 3: .*progressive"):
        sp.NamedVideoStream(sc, "prog_cpu_mjpeg", path=str(path))


# ---------------- op ----------------

def mixed_files():
    return [
        pillow_jpeg((17, 33, 3), "smooth", 75, 2),                  # baseline
        pc.pillow_pair((17, 33, 3), "noise", 75, 2, "rst2")[1],
        pillow_save(image((7, 9, 3), "noise"), "PNG"),
        pillow_jpeg((16, 24, 3), "noise", 95, 1, "rst3_opt"),       # baseline
        pc.pillow_pair((40, 56, 3), "checker", 30, 1, "optimize")[1],
        pc.pillow_pair((33, 50, 1), "noise", 75, 0, "rows1")[1],    # grey
        pc.pillow_pair((33, 50, 1), "smooth", 75)[1],
        pc.writer_cases()["dri_changes_420"][1],
    ]


def test_op_decodes_a_mixed_list_with_a_null_row(sc, tmp_path):
    blobs = mixed_files()
    col = sc.sources.Files(write_files(tmp_path, blobs))
    spaced = sc.streams.RepeatNull(col, [2])
    frames = sc.ops.ImageDecoder(img=spaced, progressive="decode")
    packed = sc.ops.ImageDecodePackFrame(frame=frames)
    out = sp.NamedStream(sc, "prog_cpu_out")
    sc.run(sc.io.Output(packed, [out]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite)
    rows = list(out.load())
    assert len(rows) == 2 * len(blobs)
    assert all(r is None for r in rows[1::2])
    for blob, row in zip(blobs, rows[0::2]):
        np.testing.assert_array_equal(
            unpack_frame(row), _core.image_cpu_decode(blob, **DECODE))


def test_op_rejects_an_unknown_value_and_keeps_the_default(sc, tmp_path):
    blobs = [pillow_jpeg((16, 24, 3), "smooth", 75, 0),
             pc.pillow_pair((16, 24, 3), "smooth", 75)[1]]
    col = sc.sources.Files(write_files(tmp_path, blobs))
    for kw, what in ((dict(progressive="maybe"),
                      r"progressive=reject\|decode, got 'maybe'"),
                     (dict(progressive="reject"), "row 1 .*progressive"),
                     ({}, "row 1 .*progressive")):
        frames = sc.ops.ImageDecoder(img=col, **kw)
        out = sp.NamedVideoStream(sc, "prog_cpu_bad")
        with pytest.raises(Exception, match=what):
            sc.run(sc.io.Output(frames, [out]), sp.PerfParams.manual(4, 8),
                   cache_mode=sp.CacheMode.Overwrite)
