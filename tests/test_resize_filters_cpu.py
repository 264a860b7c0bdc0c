"""Resize's filters ("nearest", "box", "triangle", "cubic", "lanczos3") and
preserve_aspect on the CPU kernel, against the float64 reference of
resample_ref.py, the integer rules of docs/ops.md and Pillow. The cases are
in resample_cases.py; test_resize_filters_gpu.py runs the same ones on the HIP
kernels. Every bound is derived (resample_ref.delta, resample_cases
.check_pillow); worst figures are printed (`pytest -rP`) and tabulated in
docs/testing.md.
"""
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import image_ref as I
import resample_cases as C
import resample_ref as R
import scanner_amd as sp

DEV = C.CPU
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------- the reference

def test_reference_rows_sum_to_one_and_identity_is_identity():
    for flt in R.FILTERS:
        for n_src, n_dst in [(53, 32), (7, 16), (130, 8), (1, 4), (9, 1)]:
            w = R.axis_matrix(flt, n_src, n_dst)
            assert np.allclose(w.sum(axis=1), 1.0, atol=1e-12)
        assert np.allclose(R.axis_matrix(flt, 8, 8), np.eye(8), atol=1e-15)


def test_derived_delta_is_small_on_every_case():
    worst = max(R.delta(f, *s, *d) for f in R.FILTERS for s, d in C.SHAPES)
    print(f"largest derived delta {worst:.4f}")
    assert worst <= 1.0 / 16


def _rounded(real):
    return np.clip(np.floor(real + 0.5), 0, 255).astype(np.uint8)


# where each seeded defect must show: (filter, content, source, destination)
SEEDED = {
    "support_unscaled": ("lanczos3", "random", (64, 96), (9, 13)),
    "not_normalised": ("triangle", "random", (37, 53), (20, 32)),
    "clip_intermediate": ("lanczos3", "bw", (37, 53), (20, 32)),
    "no_half_pixel": ("cubic", "random", (5, 7), (16, 16)),
}


@pytest.mark.parametrize("bug", R.BUGS)
def test_seeded_defects_break_the_bound(bug):
    """A correctly rounded output of the defective reference must fail the
    comparison that the kernels pass, on a listed case; the sound reference,
    rounded, passes it."""
    flt, kind, src, dst = SEEDED[bug]
    frame = C.content(kind, src[0], src[1], 3)[0]
    real = C.reference(flt, kind, src, dst, 3)
    delta = R.delta(flt, *src, *dst)
    assert I.rounded_ok(_rounded(real), real, delta)
    bad = _rounded(R.resample(frame, dst[0], dst[1], flt, bug=bug))
    ex = I.rounded_excess(bad, real)
    print(f"{bug}: excess {ex:.3f} over delta {delta:.4f}")
    assert ex > delta


# ------------------------------------------------------------------ kernels

@pytest.mark.parametrize("src,dst,c", C.CASES)
def test_filters_against_float64(src, dst, c):
    for flt in C.FILTERS:
        C.check_filter(DEV, flt, src, dst, c)


@pytest.mark.parametrize("src,dst,c", C.CASES)
def test_nearest(src, dst, c):
    C.check_nearest(DEV, src, dst, c)


@pytest.mark.parametrize("src,dst,c", C.PILLOW_CASES)
def test_filters_against_pillow(src, dst, c):
    for flt in C.FILTERS:
        C.check_pillow(DEV, flt, src, dst, c)


@pytest.mark.parametrize("batch,packed", C.LAYOUT_CASES)
def test_layouts(batch, packed):
    for flt in C.FILTERS + ["nearest"]:
        a = C.check_layout(DEV, flt, batch, packed)
        b = C.check_layout(DEV, flt, batch, packed)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_many_rows_batch_17():
    src, dst, c, batch = C.STRIDE_CASE
    frames = list(C.content("random", src[0], src[1], c, n=batch, seed=5))
    for flt in C.FILTERS:
        got = C.run(DEV, frames, C.resize_args(dst, flt))
        delta = R.delta(flt, *src, *dst)
        for g, f in zip(got, frames):
            I.assert_rounded(g, R.resample(f, dst[0], dst[1], flt), delta,
                             f"{flt} {src}->{dst} x{batch}")


# ---------------------------------------------------------------- arguments

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


# ----------------------------------------------------------------- fit rule

@pytest.mark.parametrize("src,box,want", C.FIT_CASES)
def test_preserve_aspect(src, box, want):
    for flt in ["bilinear", "nearest", "lanczos3"]:
        C.check_fit(DEV, flt, src, box, want)


def test_pipeline_two_sizes_in_one_column(sc, tmp_path):
    C.check_pipeline(sc, tmp_path, DEV)


def test_python_surface_takes_bool_and_string(sc):
    from conftest import make_video
    frames = make_video(n=4, h=48, w=64)
    video = sp.NamedVideoStream(sc, "rf_in", frames=frames, codec="raw")
    small = sc.ops.Resize(frame=sc.io.Input([video]), width=20, height=20,
                          filter="box", preserve_aspect=True)
    out = sp.NamedStream(sc, "rf_out")
    sc.run(sc.io.Output(small, [out]), sp.PerfParams.manual(4, 8),
           cache_mode=sp.CacheMode.Overwrite)
    got = list(sp.NamedVideoStream(sc, "rf_out").load())
    assert len(got) == 4
    for g, f in zip(got, frames):
        (want,) = C.run(DEV, [f], C.resize_args((15, 20), "box"))
        I.assert_exact(np.asarray(g), want, "graph against kernel test")


# ------------------------------------------------------------------- memory

def test_repeated_calls_release_everything():
    C.check_memory(DEV)


# ---------------------------------------------------------------- sanitiser

def test_asan_table_builder_and_cpu_resampler():
    """csrc/ops/resample_common.h (table builder, CPU resampler, fit rule) is
    index arithmetic on caller-chosen sizes: a stand-alone program built with
    g++ -fsanitize=address,undefined sweeps sizes 1..70 in both directions
    over every filter, from exact-size heap buffers."""
    src = os.path.join(REPO, "tests", "cpp", "asan_resample.cpp")
    headers = [os.path.join(REPO, "scanner_amd", "csrc", p)
               for p in ("ops/resample_common.h", "common.h")]
    h = hashlib.sha256()
    for f in [src] + headers:
        with open(f, "rb") as fh:
            h.update(fh.read())
    binp = os.path.join(tempfile.gettempdir(),
                        f"sca_asan_resample_{h.hexdigest()[:16]}")
    if not os.path.exists(binp):
        r = subprocess.run(
            ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", src, "-o", binp],
            capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            pytest.fail(f"asan build failed:\n{r.stderr[-2000:]}")
    r = subprocess.run([binp], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"rc={r.returncode}:\n{out[-3000:]}"
    assert "AddressSanitizer" not in out, out[-3000:]
    assert "runtime error" not in out, out[-3000:]
    assert "asan resample: OK" in out
