"""float64 reference of Resize's filtered paths ("box", "triangle", "cubic",
"lanczos3", "nearest") and of the aspect-preserving fit, restated from
docs/ops.md: unquantised weights as dense [n_dst, n_src] matrices, two matrix
products, no intermediate rounding. Nothing here follows a kernel's loops.

`bug` seeds one known defect into the *reference*, for the tests that check
that the bound would notice it (test_resize_filters_cpu.py).

delta() is the distance beyond a correct rounding that the fixed-point formats
of csrc/ops/resample_common.h may cost; it is derived from those formats and
from the weight matrices, not from any result.
"""
import functools

import numpy as np

# the formats csrc/ops/resample_common.h states
WEIGHT_BITS = 22    # fractional bits of a tap weight
INTER_BITS = 6      # fractional bits of the i16 intermediate

RADIUS = {"box": 0.5, "triangle": 1.0, "cubic": 2.0, "lanczos3": 3.0}
FILTERS = list(RADIUS)
BUGS = ["support_unscaled", "not_normalised", "clip_intermediate",
        "no_half_pixel"]


def kernel_function(name, x):
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    if name == "box":
        return ((x > -0.5) & (x <= 0.5)).astype(np.float64)
    if name == "triangle":
        return np.maximum(0.0, 1.0 - a)
    if name == "cubic":     # Keys, a = -0.5
        near = (1.5 * a - 2.5) * a * a + 1.0
        far = -0.5 * (((a - 5.0) * a + 8.0) * a - 4.0)
        return np.where(a < 1.0, near, np.where(a < 2.0, far, 0.0))
    if name == "lanczos3":
        return np.where(a < 3.0, np.sinc(x) * np.sinc(x / 3.0), 0.0)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def axis_matrix(name, n_src, n_dst, bug=None):
    """[n_dst, n_src] weights of one axis; rows sum to one."""
    scale = n_src / n_dst
    fscale = max(1.0, scale)
    if bug == "support_unscaled":   # the filter keeps its upscale width
        fscale = 1.0
    support = RADIUS[name] * fscale
    d = np.arange(n_dst, dtype=np.float64)[:, None]
    k = np.arange(n_src, dtype=np.float64)[None, :]
    center = d * scale if bug == "no_half_pixel" else (d + 0.5) * scale
    lo = np.maximum(0, np.trunc(center - support + 0.5))
    hi = np.minimum(n_src, np.trunc(center + support + 0.5))
    w = kernel_function(name, (k + 0.5 - center) / fscale)
    w = w * ((k >= lo) & (k < hi))
    if bug != "not_normalised":
        total = w.sum(axis=1, keepdims=True)
        # a defect can leave a row without taps; the real definition cannot
        w = w / np.where(total == 0.0, 1.0, total)
    w.setflags(write=False)
    return w


def resample(frame, dh, dw, name, bug=None):
    """float64 [dh, dw, c], before the final rounding and clamp."""
    sh, sw, _ = frame.shape
    wx = axis_matrix(name, sw, dw, bug)
    wy = axis_matrix(name, sh, dh, bug)
    mid = np.einsum("xk,hkc->hxc", wx, frame.astype(np.float64))
    if bug == "clip_intermediate":      # Pillow's u8 intermediate
        mid = np.clip(np.floor(mid + 0.5), 0.0, 255.0)
    return np.einsum("yh,hxc->yxc", wy, mid)


def nearest(frame, dh, dw):
    sh, sw, _ = frame.shape
    ys = [((2 * d + 1) * sh) // (2 * dh) for d in range(dh)]
    xs = [((2 * d + 1) * sw) // (2 * dw) for d in range(dw)]
    return np.ascontiguousarray(frame[ys][:, xs])


def fit(sh, sw, box_h, box_w):
    """(dh, dw): the largest size of the aspect sh x sw inside the box."""
    if box_w * sh <= box_h * sw:
        return min(box_h, max(1, (2 * sh * box_w + sw) // (2 * sw))), box_w
    return box_h, min(box_w, max(1, (2 * sw * box_h + sh) // (2 * sh)))


def delta(name, sh, sw, dh, dw):
    """Bound on |fixed point - real| before the final rounding.

    Weights: each of a row's T taps is rounded to WEIGHT_BITS (error <= half
    a unit), and the largest then absorbs the residue of the row (<= T half
    units), so a row's weights are off by at most T units q = 2^-WEIGHT_BITS
    in sum. Horizontal pass on samples <= 255: 255 * Tx * q, plus half a unit
    of the intermediate, 2^-(INTER_BITS + 1). The vertical pass multiplies
    that by at most the row's sum |w| (Sy) and adds its own weight error on
    intermediates of magnitude <= 255 * Sx. The final rounding is the 0.5 of
    the comparator."""
    wx = axis_matrix(name, sw, dw)
    wy = axis_matrix(name, sh, dh)
    q = 2.0 ** -WEIGHT_BITS
    tx = int((wx != 0).sum(axis=1).max())
    ty = int((wy != 0).sum(axis=1).max())
    # taps whose weight is zero still count where the range holds them
    tx = max(tx, int(np.ceil(2 * RADIUS[name] * max(1.0, sw / dw))) + 1)
    ty = max(ty, int(np.ceil(2 * RADIUS[name] * max(1.0, sh / dh))) + 1)
    sx = float(np.abs(wx).sum(axis=1).max())
    sy = float(np.abs(wy).sum(axis=1).max())
    horizontal = 255.0 * tx * q + 2.0 ** -(INTER_BITS + 1)
    return sy * horizontal + ty * q * (255.0 * sx + horizontal)
