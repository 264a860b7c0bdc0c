"""HIP kernels of kernels/resample.hip (Resize with filter "nearest", "box",
"triangle", "cubic", "lanczos3", and preserve_aspect) on the cases of
resample_cases.py: within 0.5 + delta of the float64 reference of
resample_ref.py, byte for byte equal to the CPU kernel, equal to the integer
rules, within 1 of Pillow. test_resize_filters_cpu.py holds the CPU kernel to
the same cases. Worst figures are printed (`pytest -rP`) and tabulated in
docs/testing.md; no bound is tuned from them.
"""
import numpy as np
import pytest

import image_ref as I
import resample_cases as C
import resample_ref as R

pytestmark = pytest.mark.gpu

DEV = C.GPU


@pytest.mark.parametrize("src,dst,c", C.CASES)
def test_filters_against_float64_and_cpu_bytes(src, dst, c):
    for flt in C.FILTERS:
        gpu, _ = C.check_filter(DEV, flt, src, dst, c)
        cpu, _ = C.check_filter(C.CPU, flt, src, dst, c)
        for kind in gpu:
            I.assert_exact(gpu[kind], cpu[kind],
                           f"GPU against CPU bytes: {flt} {src}->{dst} "
                           f"c={c} {kind}")


@pytest.mark.parametrize("src,dst,c", C.CASES)
def test_nearest(src, dst, c):
    I.assert_exact(C.check_nearest(DEV, src, dst, c),
                   C.check_nearest(C.CPU, src, dst, c), "GPU against CPU")


@pytest.mark.parametrize("src,dst,c", C.PILLOW_CASES)
def test_filters_against_pillow(src, dst, c):
    for flt in C.FILTERS:
        C.check_pillow(DEV, flt, src, dst, c)


@pytest.mark.parametrize("batch,packed", C.LAYOUT_CASES)
def test_layouts_and_two_calls(batch, packed):
    """13x17x3 packed: frames 2, 4, .. start at odd addresses and the group
    takes the byte-wise staging; unpacked, the 16-byte one needs a pitch of
    51 bytes to be a multiple of 16, so bytes again; batch 17 is one more
    than the preferred batch."""
    for flt in C.FILTERS + ["nearest"]:
        a = C.check_layout(DEV, flt, batch, packed)
        b = C.check_layout(DEV, flt, batch, packed)
        cpu = C.check_layout(C.CPU, flt, batch, packed)
        for x, y, z in zip(a, b, cpu):
            I.assert_exact(x, y, f"{flt}: second call")
            I.assert_exact(x, z, f"{flt}: GPU against CPU bytes")


def test_wide_loads_against_bytes():
    """Rows of 64x96x1 (96 bytes) and 64x96x4 (384 bytes) are multiples of
    16 bytes and every frame starts aligned, packed or not: the 16-byte
    staging, with spans that start and end inside a vector. 37x53x3 has a
    pitch of 159 bytes: the byte-wise staging. Black/white noise, against
    the CPU kernel's bytes."""
    for src, dst, c in [((64, 96), (9, 13), 1), ((64, 96), (40, 50), 4),
                        ((37, 53), (20, 32), 3)]:
        frames = list(C.content("bw", src[0], src[1], c, n=3, seed=6))
        for flt in C.FILTERS:
            for packed in (True, False):
                g = C.run(DEV, frames, C.resize_args(dst, flt), packed=packed)
                h = C.run(C.CPU, frames, C.resize_args(dst, flt))
                for x, y in zip(g, h):
                    I.assert_exact(x, y, f"{flt} {src}->{dst} c={c} "
                                         f"packed={packed}")


def test_many_rows_batch_17():
    """The horizontal pass's tile loop takes a second round
    (resample_cases.STRIDE_CASE)."""
    src, dst, c, batch = C.STRIDE_CASE
    frames = list(C.content("random", src[0], src[1], c, n=batch, seed=5))
    for flt in C.FILTERS:
        got = C.run(DEV, frames, C.resize_args(dst, flt))
        cpu = C.run(C.CPU, frames, C.resize_args(dst, flt))
        delta = R.delta(flt, *src, *dst)
        for g, h, f in zip(got, cpu, frames):
            I.assert_exact(g, h, f"{flt}: GPU against CPU bytes")
        I.assert_rounded(got[0], R.resample(frames[0], dst[0], dst[1], flt),
                         delta, f"{flt} {src}->{dst} x{batch}")


def test_unknown_filter_is_rejected_by_name():
    frame = C.content("random", 8, 8, 3)[0]
    with pytest.raises(Exception, match="Resize filter must be one of "
                       "'bilinear', 'nearest', 'box', 'triangle', 'cubic', "
                       "'lanczos3', got 'gaussian'"):
        C.run(DEV, [frame], C.resize_args((4, 4), "gaussian"))
    with pytest.raises(Exception, match="Resize needs width/height args"):
        C.run(DEV, [frame], {"filter": "box"})


def test_f32_frames_are_rejected_by_name():
    frame = np.zeros((8, 8, 2), np.float32)
    with pytest.raises(Exception, match="need.* u8 frames"):
        C.run(DEV, [frame], C.resize_args((4, 4), "box"))


@pytest.mark.parametrize("src,dst", [((37, 53), (20, 32)), ((5, 7), (16, 16))])
def test_default_is_the_bilinear_sampler(src, dst):
    frame = C.content("random", src[0], src[1], 3)[0]
    (absent,) = C.run(DEV, [frame], C.resize_args(dst))
    (named,) = C.run(DEV, [frame], C.resize_args(dst, "bilinear"))
    I.assert_exact(named, absent, "filter='bilinear' against no argument")
    I.assert_rounded(absent, I.resize(frame, *dst), I.delta_resize(*src),
                     f"default resize {src}->{dst}")


@pytest.mark.parametrize("src,box,want", C.FIT_CASES)
def test_preserve_aspect(src, box, want):
    for flt in ["bilinear", "nearest", "lanczos3"]:
        got = C.check_fit(DEV, flt, src, box, want)
        if flt != "bilinear":
            I.assert_exact(got, C.check_fit(C.CPU, flt, src, box, want),
                           f"fit {flt}: GPU against CPU bytes")


def test_pipeline_two_sizes_in_one_column(sc, tmp_path):
    C.check_pipeline(sc, tmp_path, DEV)


def test_repeated_calls_release_everything():
    C.check_memory(DEV)
