"""CPU kernels of Histogram, Resize, Blur, ColorConvert, Crop, OpticalFlow
and FlowStats against the float64/integer references, through
`_core.op_kernel_test(..., CPU, ...)`: the same cases and bounds as
test_image_ops_gpu.py (image_ops_cases.py). Then the comparators
themselves: a defect seeded into the reference must be flagged on every
shape where it can show, and the flow inputs must stay far from the one
discontinuity of the function (det > 1e-4).
"""
import numpy as np
import pytest

import flow_ref as F
import image_ops_cases as C
import image_ref as I
from scanner_amd import _core

DEV = C.CPU


# ------------------------------------------------------------- the binding

def test_op_kernel_test_releases_everything():
    frames = C.rand_frames(4, 13, 17, 3, 1)

    def calls():
        C.run("Histogram", DEV, frames)
        C.run("Histogram", DEV, frames, packed=False)
        C.run("Blur", DEV, frames, {"kernel_size": 3})
        C.run_flow(DEV, frames, None)
        C.run("OpticalFlow", DEV, frames[:2], None, stencil=[0, 1],
              then_op="FlowStats")
        with pytest.raises(Exception, match="Crop outside frame bounds"):
            C.run("Crop", DEV, frames, C.crop_args((10, 10, 20, 20)))

    calls()  # the peak settles
    before = _core.mem_stats(-1)
    calls()
    assert _core.mem_stats(-1) == before


def test_op_kernel_test_rejects_bad_input():
    f = C.rand_frames(2, 4, 5, 3, 1)
    with pytest.raises(Exception, match="differ in shape or type"):
        C.run("Histogram", DEV, [f[0], f[1][:3]])
    with pytest.raises(Exception, match="fewer frames than the stencil"):
        C.run("OpticalFlow", DEV, f[:1], None, stencil=[0, 1])
    with pytest.raises(Exception, match="uint8 or float32"):
        C.run("Histogram", DEV, [f[0].astype(np.int32)])
    # a non-contiguous view is copied, not misread
    wide = C.rand_frames(1, 4, 10, 3, 2)[0]
    (got,) = C.run("Histogram", DEV, [wide[:, ::2]])
    I.assert_exact(C.hist_of(got, 3), I.histogram(wide[:, ::2]), "strided")


# --------------------------------------------------------------- Histogram

@pytest.mark.parametrize("shape,batch,packed", C.HIST_CASES)
def test_histogram(shape, batch, packed):
    for name, frames in C.hist_contents(shape, batch).items():
        C.check_histogram(DEV, frames, packed, f"{shape} x{batch} {name}")


def test_histogram_batch_300():
    C.check_histogram(DEV, C.rand_frames(300, 4, 5, 3, 2), True, "4x5x3 x300")


@pytest.mark.parametrize("c", [1, 4])
def test_histogram_other_channel_counts(c):
    C.check_histogram(DEV, C.rand_frames(3, 9, 11, c, 3), True, f"9x11x{c}")


# ------------------------------------------------------------------ Resize

@pytest.mark.parametrize("src,dst,c", C.RESIZE_CASES)
def test_resize(src, dst, c):
    C.check_resize(DEV, src, dst, c)


# -------------------------------------------------------------------- Blur

@pytest.mark.parametrize("shape,c", C.BLUR_CASES)
def test_blur(shape, c):
    C.check_blur(DEV, shape, c)


def test_blur_600():
    C.check_blur(DEV, (600, 600), 3, [3])


# ------------------------------------------------------------ ColorConvert

@pytest.mark.parametrize("fmt", ["gray", "yuv"])
def test_colour(fmt):
    for what, frame in C.colour_frames().items():
        C.check_colour(DEV, fmt, frame, what)


@pytest.mark.parametrize("fmt", ["gray", "yuv"])
def test_colour_rejects_other_channel_counts(fmt):
    for c in (1, 4):
        with pytest.raises(Exception,
                           match=f"{fmt} conversion needs RGB input"):
            C.run("ColorConvert", DEV, C.rand_frames(1, 4, 4, c, 1),
                  {"format": fmt})


@pytest.mark.parametrize("shape,c", C.PLANAR_CASES)
def test_planar(shape, c):
    C.check_planar(DEV, shape, c)


@pytest.mark.parametrize("c", [1, 3])
def test_crop(c):
    for win in C.CROP_WINDOWS:
        C.check_crop(DEV, 48, 64, c, win)
    for win, msg in C.CROP_REJECTED:
        with pytest.raises(Exception, match=msg):
            C.run("Crop", DEV, C.rand_frames(1, 48, 64, c, 1),
                  C.crop_args(win))


def test_crop_600():
    C.check_crop(DEV, 600, 600, 3, (1, 1, 599, 599))


# ------------------------------------------------------------- OpticalFlow

@pytest.mark.parametrize("name", C.FLOW_IDS)
def test_flow(name):
    C.check_flow(DEV, name)


def test_flow_rows():
    C.check_flow_rows(DEV)


def test_flow_exact_cases():
    C.check_flow_exact(DEV)


def test_flow_two_calls_bit_equal():
    case = C.flow_case("pyramid-99x131-c3")
    a = C.run_flow(DEV, [case.f0, case.f1], None)[0]
    b = C.run_flow(DEV, [case.f0, case.f1], None)[0]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# --------------------------------------------------------------- FlowStats

@pytest.mark.parametrize("shape", C.STATS_SHAPES)
@pytest.mark.parametrize("batch", [1, 5])
def test_flowstats(shape, batch):
    C.check_flowstats(DEV, C.stats_flows(shape, batch), f"{shape} x{batch}")


@pytest.mark.parametrize("where", ["first", "last"])
def test_flowstats_lone_large_value(where):
    fl = C.stats_flows((130, 72), 1, seed=5)[0] * np.float32(0.01)
    fl.reshape(-1, 2)[0 if where == "first" else -1] = (-300.0, 450.0)
    C.check_flowstats(DEV, [fl], f"large value {where}")


def test_flowstats_of_flow_output():
    case = C.flow_case("pyramid-130x72-c3")
    flows, stats = C.run("OpticalFlow", DEV, [case.f0, case.f1], None,
                         stencil=[0, 1], then_op="FlowStats")
    case.check(flows[0])
    F.assert_flowstats(C.stats_of(stats[0]), flows[0], "of OpticalFlow")


# ----------------------------------------- flow: the reference is sensible

def test_flow_reference_recovers_a_translation():
    case = C.flow_case("pyramid-99x131-c3")   # textured, moved by (2, 1)
    inner = case.ref[12:-12, 12:-12]
    assert np.abs(inner - [2.0, 1.0]).max() <= 0.05
    assert abs(inner[..., 0].mean() - 2.0) < 1e-3
    assert abs(inner[..., 1].mean() - 1.0) < 1e-3


def test_flow_inputs_are_far_from_the_singular_guard():
    """min det >= 1 = 1e4 * kDetEps on every input: no pixel's update can
    flip on a rounding error, so the flow is continuous in its arithmetic."""
    cases = [C.flow_case(n) for n in C.FLOW_IDS] + list(C.rows_cases())
    for case in cases:
        print(f"{case.name}: min det {case.min_det:.3e} E32 {case.e32:.3e}")
        assert case.min_det >= 1.0, (case.name, case.min_det)
        assert 0 < case.e32 < 1e-3, (case.name, case.e32)


# ------------------------- the comparators notice a defect in the reference

def _rounded(real, wrap=False):
    v = np.floor(real + 0.5)
    if wrap:                      # what a kernel without the clamp stores
        return (v.astype(np.int64) & 0xff).astype(np.uint8)
    return np.clip(v, 0, 255).astype(np.uint8)


def _resize_can_show(bug, src, dst):
    (sh, sw), (dh, dw) = src, dst
    if bug == "no_half_pixel":    # the offset cancels at 1:1; one source
        return src != dst and sh * sw > 1     # pixel has nowhere to move
    # x1 = x0 + 1 leaves the image only where the last source coordinate
    # lies beyond the last pixel centre: upscaling
    return dh > sh or dw > sw


@pytest.mark.parametrize("bug", ["no_half_pixel", "no_x1_clamp"])
def test_seeded_resize(bug):
    shown = 0
    for src, dst, c in C.RESIZE_CASES:
        f = C.rand_frames(1, src[0], src[1], c, 5)[0]
        real = I.resize(f, *dst)
        delta = I.delta_resize(*src)
        assert I.rounded_ok(_rounded(real), real, delta)
        if _resize_can_show(bug, src, dst):
            assert not I.rounded_ok(_rounded(I.resize(f, *dst, bug=bug)),
                                    real, delta), (bug, src, dst, c)
            shown += 1
    assert shown >= 5


@pytest.mark.parametrize("bug", ["round", "zero_pad"])
def test_seeded_blur(bug):
    shown = 0
    for (h, w), c in C.BLUR_CASES + [((600, 600), 3)]:
        f = C.rand_frames(1, h, w, c, C.BLUR_SEED)[0]
        for ks in C.BLUR_KS if h < 600 else [3]:
            ref = I.blur(f, ks)
            # floor and nearest differ only where a window holds > 1 pixel;
            # zero padding shows wherever a window leaves the frame
            can_show = ks // 2 > 0 and (bug == "zero_pad" or h * w > 1)
            if can_show:
                assert not I.exact_ok(I.blur(f, ks, bug=bug), ref), \
                    (bug, h, w, c, ks)
                shown += 1
    assert shown >= 30


def test_seeded_yuv_clamp():
    """A kernel that stores U or V = 256 unclamped ((0,0,255), (255,0,0))
    is flagged on the frame that holds the corner colours."""
    f = C.colour_frames()["lattice"]
    real = I.yuv(f)
    assert real[..., 1].max() == 255.5 and real[..., 2].max() == 255.5
    assert I.rounded_ok(_rounded(real), real, I.DELTA_COLOR)
    assert not I.rounded_ok(_rounded(real, wrap=True), real, I.DELTA_COLOR)


def test_seeded_yuv_coefficient():
    for what, f in C.colour_frames().items():
        real = I.yuv(f)
        assert I.rounded_ok(_rounded(real), real, I.DELTA_COLOR)
        assert not I.rounded_ok(_rounded(I.yuv(f, bug="coef")), real,
                                I.DELTA_COLOR), what


@pytest.mark.parametrize("bug", ["phase", "drop_tail"])
def test_seeded_histogram(bug):
    shown = 0
    shapes = C.HIST_SHAPES + [(4, 5, 3), (9, 11, 4)]
    for shape in shapes:
        f = C.rand_frames(1, *shape, 11)[0]
        ref = I.histogram(f)
        nbytes = f.size
        # the tail exists where nbytes % 16 != 0; a phase shift shows on
        # any frame whose channels differ
        can_show = nbytes % 16 != 0 if bug == "drop_tail" else True
        if can_show:
            assert not I.exact_ok(I.histogram(f, bug=bug), ref), (bug, shape)
            shown += 1
    assert shown >= (4 if bug == "drop_tail" else 6)


def _flow_can_show(bug, name):
    if bug in ("upsample_noscale", "upsample_2x"):
        if not name.startswith("pyramid"):
            return False          # one level: nothing is upsampled
        # 130x72 -> 65x36 scales by exactly 2 on both axes
        return bug == "upsample_noscale" or "99x131" in name
    return True


@pytest.mark.parametrize("bug", ["grad_no_half", "radius", "upsample_noscale",
                                 "upsample_2x", "wrap", "iters"])
def test_seeded_flow(bug):
    shown = 0
    for name in C.FLOW_IDS:
        if not _flow_can_show(bug, name):
            continue
        case = C.flow_case(name)
        bad, _ = F.flow(case.f0, case.f1, bug=bug, **case.params)
        assert not case.ok(bad.astype(np.float32)), (bug, name)
        shown += 1
    assert shown >= 2
    if bug.startswith("upsample"):    # 178/89 = 2 but 89/44 is not
        ab, _ = C.rows_cases()
        bad, _ = F.flow(ab.f0, ab.f1, bug=bug)
        assert not ab.ok(bad.astype(np.float32)), (bug, "rows")


def test_flow_comparator_accepts_the_float32_emulation():
    for name in C.FLOW_IDS:
        case = C.flow_case(name)
        f32, _ = F.flow(case.f0, case.f1, dtype=np.float32, **case.params)
        assert case.ok(f32)


@pytest.mark.parametrize("bug", ["signed", "drop_chunk"])
def test_seeded_flowstats(bug):
    shown = 0
    for shape in C.STATS_SHAPES:
        for fl in C.stats_flows(shape, 5):
            npix = shape[0] * shape[1]
            ref = F.flowstats(fl)
            mx = np.abs(fl.reshape(-1, 2)).max(axis=0).astype(np.float32)
            assert F.flowstats_ok(ref.astype(np.float32), ref, npix, mx)
            # 16x16 is one whole chunk of 256 pixels: nothing to drop
            if bug == "signed" or npix % 256:
                assert not F.flowstats_ok(
                    F.flowstats(fl, bug=bug).astype(np.float32), ref, npix,
                    mx), (bug, shape)
                shown += 1
    assert shown >= 10
