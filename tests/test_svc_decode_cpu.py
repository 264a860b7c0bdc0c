"""The SVC decode case list on the CPU (no GPU needed): the numpy
restatement of the format (svc_ref.py) tied to svc_encode_cpu byte for byte,
both readers against the source frames on every case of svc_cases.py, the
seeded reference defects, and the conditions the case list must meet for
test_svc_decode_gpu.py to reach what it is there for. The codec is
lossless: every comparison is equality."""
import numpy as np
import pytest

import svc_cases as C
import svc_ref as R
from scanner_amd import _core

CASES = C.cases()
ALL_GEOMS = C.SMALL_GEOMS + [C.BIG_GEOM]


def nbytes_of(geom):
    return int(np.prod(geom))


# ------------------------------------------- the restatement is the format

@pytest.mark.parametrize("gop", [1, 5, 16, 40])
@pytest.mark.parametrize("geom", ALL_GEOMS, ids=C.geom_id)
def test_writer_matches_cpu_encoder(geom, gop):
    n = C.BIG_N if geom == C.BIG_GEOM else C.N
    keys = tuple(range(0, n, gop))
    for content in C.ENC_CONTENTS:
        frames = C.clip((n,) + geom, content,
                        keys if content == "widths" else 16)
        ref_stream, ref_sizes = _core.svc_cpu_encode(frames, gop)
        stream, sizes = R.write_stream(frames, keys)
        assert sizes == ref_sizes, content
        assert stream == ref_stream, content


def test_widths_content_is_what_it_says():
    """Conditions on the inputs: `widths` gives group g of frame f exactly
    (g + f) % 9 bits under every key list, overwide8 is 8 everywhere,
    overwide_random lies in [minimal, 8] and exceeds the minimum somewhere,
    one_group is 0 everywhere but the one group."""
    for case in CASES:
        nbytes = nbytes_of(case.geom)
        stream, sizes = C.stream(*case[:4])
        got = R.stream_widths(stream, sizes, nbytes)
        if case.content == "widths":
            np.testing.assert_array_equal(
                got, C.crafted_bits((case.n,) + case.geom))
        elif case.content == "overwide8":
            assert (got == 8).all()
        elif case.content == "overwide_random":
            mins = R.stream_widths(
                *C.stream(case.geom, "smooth", case.keys, case.n), nbytes)
            assert (got >= mins).all() and (got <= 8).all()
            assert (got > mins).any()
        elif case.content == "one_group":
            g = C.one_group_index(nbytes)
            assert (np.delete(got, g, axis=1) == 0).all()
            assert (got[:, g] > 0).any()


# ------------------------------------------------ both readers, every case

@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_readers_return_the_source(case):
    frames = C.frames(*case[:4])
    stream, sizes = C.stream(*case[:4])
    h, w, c = case.geom
    np.testing.assert_array_equal(
        R.read_stream(stream, sizes, h, w, c, case.keys), frames)
    for want in case.wants:
        got = _core.svc_cpu_decode(stream, sizes, h, w, c,
                                   keyframes=list(case.keys),
                                   want=list(want))
        np.testing.assert_array_equal(got, frames[list(want)], str(want))


def test_span_is_minimal():
    """svc_decode_span through its effect: a stream cut down to the packets
    of the python span (every other packet replaced by garbage of the same
    size) still decodes the wanted frames, for each key list and want."""
    geom = (5, 7, 3)
    for keys in C.KEYS:
        frames = C.frames(geom, "noise", keys, C.N)
        stream, sizes = C.stream(geom, "noise", keys, C.N)
        offs = np.cumsum([0] + sizes)
        for want in C.WANTS:
            span = set(R.decode_span(keys, want))
            cut = bytearray(stream)
            for f in range(C.N):
                if f not in span:
                    cut[offs[f]:offs[f + 1]] = b"\xee" * sizes[f]
            got = _core.svc_cpu_decode(bytes(cut), sizes, *geom,
                                       keyframes=list(keys),
                                       want=list(want))
            np.testing.assert_array_equal(got, frames[list(want)])


def test_default_arguments_unchanged():
    frames = C.clip((18, 5, 7, 3), "noise")
    stream, sizes = _core.svc_cpu_encode(frames, 5)
    np.testing.assert_array_equal(
        _core.svc_cpu_decode(stream, sizes, 5, 7, 3, 5), frames)
    np.testing.assert_array_equal(
        _core.svc_cpu_decode(stream, sizes, 5, 7, 3, gop=5, want=[3, 11]),
        frames[[3, 11]])


# ----------------------------------------------------------- seeded defects

def can_show(defect, geom):
    nbytes = nbytes_of(geom)
    ngroups, nsuper = R.geometry(nbytes)
    if defect == "key_pred_across":
        return ngroups > 1
    if defect == "carry_dropped":
        return ngroups > 64
    if defect == "super_off_ignored":
        return nsuper > 1
    if defect == "tail_prev32":
        return nbytes % 32 != 0 and nbytes >= 32
    return True


@pytest.mark.parametrize("geom", ALL_GEOMS, ids=C.geom_id)
def test_seeded_reader_defects_show(geom):
    """Each defect seeded into the *reference reader* changes the decoded
    frames on at least one listed case of every geometry where it can show;
    the first such case is printed (`pytest -rP`)."""
    h, w, c = geom
    mine = [case for case in CASES if case.geom == geom]
    for defect in R.DEFECTS:
        if not can_show(defect, geom):
            continue
        for case in mine:
            stream, sizes = C.stream(*case[:4])
            got = R.read_stream(stream, sizes, h, w, c, case.keys, defect)
            if not np.array_equal(got, C.frames(*case[:4])):
                print(f"{defect}: {C.case_id(case)}")
                break
        else:
            pytest.fail(f"{defect} shows on no case of {C.geom_id(geom)}")


def test_defects_that_cannot_show_do_not():
    """can_show is not an excuse: where it says no, the defective reader is
    in fact right on every listed case of that geometry."""
    for geom in C.SMALL_GEOMS:
        for defect in R.DEFECTS:
            if can_show(defect, geom):
                continue
            for case in CASES:
                if case.geom != geom:
                    continue
                stream, sizes = C.stream(*case[:4])
                got = R.read_stream(stream, sizes, *geom, case.keys, defect)
                np.testing.assert_array_equal(got, C.frames(*case[:4]))


# ------------------------------------------------ conditions on the inputs

def all_launches(batch=16):
    for case in CASES:
        for want in case.wants:
            yield case, want, C.launches(case.keys, want, batch)


def test_case_list_reaches_the_handover():
    wanted_handover = scratch_handover = tail_from_scratch = False
    for case, want, launches in all_launches():
        tail = nbytes_of(case.geom) % 32 != 0
        for i, launch in enumerate(launches):
            if not launch["continues"]:
                continue
            if launch["last_wanted"]:
                wanted_handover = True
            else:
                scratch_handover = True
                assert launches[i + 1]["from_prev"]
                tail_from_scratch |= tail
    # a launch whose last frame is wanted and the chain continues
    assert wanted_handover
    # a launch whose last frame is not wanted: the scratch frame
    assert scratch_handover
    # a launch that starts from the scratch frame with a tail group
    assert tail_from_scratch


def test_case_list_has_more_than_four_chains():
    assert any(sum(not la["from_prev"] for la in launches) > 4
               for _, _, launches in all_launches())


def test_case_list_skips_a_gop_inside_the_span():
    found = False
    for case in CASES:
        for want in case.wants:
            span = R.decode_span(case.keys, want)
            skipped = set(range(span[0], span[-1] + 1)) - set(span)
            # a whole GOP: a key frame and everything up to the next key
            for k, nxt in zip(case.keys, case.keys[1:] + (case.n,)):
                found |= set(range(k, nxt)) <= skipped
    assert found


def test_case_list_starts_mid_gop():
    assert any(want[0] not in case.keys
               for case in CASES for want in case.wants)


def test_one_mb_geometry_is_what_the_table_says():
    nbytes = nbytes_of(C.BIG_GEOM)
    assert nbytes == 1051050 and nbytes > 1 << 20
    assert R.geometry(nbytes) == (32846, 257) and nbytes % 32 == 10
    assert [R.geometry(nbytes_of(g)) for g in C.SMALL_GEOMS] == [
        (1, 1), (4, 1), (64, 1), (65, 1), (65, 1), (128, 1), (129, 2),
        (157, 2)]


# --------------------------------------------------------------- rejections

def test_rejections_by_name():
    geom = (5, 7, 3)
    stream, sizes = C.stream(geom, "smooth", (0,), C.N)
    with pytest.raises(Exception, match="frame beyond stream"):
        _core.svc_cpu_decode(stream, sizes, *geom, keyframes=[0],
                             want=[C.N])
    with pytest.raises(Exception, match="no keyframe before frame"):
        _core.svc_cpu_decode(stream, sizes, *geom, keyframes=[5], want=[3])
    with pytest.raises(Exception, match="not all wanted frames produced"):
        _core.svc_cpu_decode(stream, sizes, *geom, keyframes=[0],
                             want=[5, 5])
    assert _core.svc_cpu_decode(stream, sizes, *geom, keyframes=[0],
                                want=[]).shape == (0,) + geom
