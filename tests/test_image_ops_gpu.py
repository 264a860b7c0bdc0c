"""HIP kernels of kernels/image_ops.hip (Histogram, Resize), kernels/color.hip
(ColorConvert, Crop, Blur) and kernels/optflow.hip (OpticalFlow, FlowStats)
against the float64/integer references of image_ref.py and flow_ref.py.

Each kernel is run directly through `_core.op_kernel_test` on the smallest
shapes that reach each of its paths (image_ops_cases.py; the same cases hold
the CPU kernels in test_image_ops_ref.py). Integer operations must be equal;
rounded-float operations must lie within 0.5 + delta of the real value, delta
derived from the float32 operation count; optical flow within 16 * E32 of
the float64 flow on every pixel, E32 being the measured cost of single
precision on that input. Worst figures are printed (`pytest -rP`) and
tabulated in docs/testing.md; no bound is tuned from them.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_ref as F
import image_ops_cases as C
import image_ref as I
from scanner_amd import _core

pytestmark = pytest.mark.gpu

DEV = C.GPU
HERE = os.path.dirname(os.path.abspath(__file__))


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
    before = (_core.mem_stats(0), _core.mem_stats(-1))
    calls()
    assert (_core.mem_stats(0), _core.mem_stats(-1)) == before


# --------------------------------------------------------------- Histogram

@pytest.mark.parametrize("shape,batch,packed", C.HIST_CASES)
def test_histogram(shape, batch, packed):
    """1x1x3 and 5x7x3 (105 B: six vectors, then the tail), 13x17x3 (663 B;
    packed, frames 2.. start at odd addresses and take the byte-wise
    kernel), 16x16x3 aligned as the control."""
    for name, frames in C.hist_contents(shape, batch).items():
        C.check_histogram(DEV, frames, packed, f"{shape} x{batch} {name}")


def test_histogram_batch_300():
    """chunks = 2048 // 300 = 6 and 512 // 300 = 1 reduce slice: the reduce
    kernel stores instead of accumulating."""
    C.check_histogram(DEV, C.rand_frames(300, 4, 5, 3, 2), True, "4x5x3 x300")


@pytest.mark.parametrize("c", [1, 4])
def test_histogram_other_channel_counts(c):
    C.check_histogram(DEV, C.rand_frames(3, 9, 11, c, 3), True, f"9x11x{c}")


def test_histogram_two_calls_bit_equal():
    frames = C.rand_frames(16, 13, 17, 3, 4)
    for packed in (True, False):
        a = C.run("Histogram", DEV, frames, packed=packed)
        b = C.run("Histogram", DEV, frames, packed=packed)
        assert a == b


# ------------------------------------------------------------------ Resize

@pytest.mark.parametrize("src,dst,c", C.RESIZE_CASES)
def test_resize(src, dst, c):
    C.check_resize(DEV, src, dst, c)


# -------------------------------------------------------------------- Blur

@pytest.mark.parametrize("shape,c", C.BLUR_CASES)
def test_blur(shape, c):
    C.check_blur(DEV, shape, c)


def test_blur_600():
    """600*600*3 > 4096*256 elements: the stride loop's second pass."""
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


def test_flow_rows_per_thread():
    C.check_flow_rows(DEV, "PY default")


def test_flow_rows_per_thread_py4():
    """The library reads SCANNER_LK_PY once per process: a fresh child."""
    out = subprocess.run(
        [sys.executable, os.path.join(HERE, "image_ops_child.py")],
        env=dict(os.environ, SCANNER_LK_PY="4"), capture_output=True,
        text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, \
        f"child exited {out.returncode}:\n{out.stdout[-2000:]}\n" \
        f"{out.stderr[-4000:]}"
    assert "child OK" in out.stdout


def test_flow_exact_cases():
    C.check_flow_exact(DEV)


def test_flow_rejects_radius_5():
    a, b = C.rand_frames(2, 40, 56, 3, 1)
    with pytest.raises(Exception, match="OpticalFlow radius must be 2, 3 or 4"):
        C.run_flow(DEV, [a, b], {"radius": 5})


def test_flow_two_calls_bit_equal():
    case = C.flow_case("pyramid-99x131-c3")
    a = C.run_flow(DEV, [case.f0, case.f1], None)[0]
    b = C.run_flow(DEV, [case.f0, case.f1], None)[0]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# --------------------------------------------------------------- FlowStats

@pytest.mark.parametrize("shape", C.STATS_SHAPES)
@pytest.mark.parametrize("batch", [1, 5])
def test_flowstats(shape, batch):
    flows = C.stats_flows(shape, batch)
    C.check_flowstats(DEV, flows, f"{shape} x{batch}")
    C.check_flowstats(DEV, flows, f"{shape} x{batch} unpacked", packed=False)


@pytest.mark.parametrize("where", ["first", "last"])
def test_flowstats_lone_large_value(where):
    fl = C.stats_flows((130, 72), 1, seed=5)[0] * np.float32(0.01)
    fl.reshape(-1, 2)[0 if where == "first" else -1] = (-300.0, 450.0)
    C.check_flowstats(DEV, [fl], f"large value {where}")


def test_flowstats_of_flow_output_on_the_device():
    """OpticalFlow -> FlowStats without leaving the device, the `flow`
    benchmark's two ops."""
    case = C.flow_case("pyramid-130x72-c3")
    flows, stats = C.run("OpticalFlow", DEV, [case.f0, case.f1], None,
                         stencil=[0, 1], then_op="FlowStats")
    case.check(flows[0])
    F.assert_flowstats(C.stats_of(stats[0]), flows[0], "of OpticalFlow")
