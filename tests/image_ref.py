"""High-precision numpy references for Histogram, Resize, Blur, ColorConvert
and Crop, and the comparators that hold a kernel's output to them.

Every function restates the operation, in float64 or exact integers, from
what docs/ops.md promises; none follows a kernel's loops. The `bug` argument
seeds one known defect into the *reference*, for the tests that check that
the comparators would notice it (test_image_ops_ref.py).
"""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


# ---------------------------------------------------------------- references

def histogram(frame, bug=None):
    """[c,256] uint32 counts of an HWC u8 frame."""
    h, w, c = frame.shape
    flat = frame.reshape(-1)
    if bug == "phase":          # channel of byte i taken as (i+1) % c
        chan = (np.arange(flat.size) + 1) % c
    else:
        chan = np.arange(flat.size) % c
    if bug == "drop_tail":      # the last nbytes % 16 bytes never counted
        keep = flat.size - flat.size % 16
        flat, chan = flat[:keep], chan[:keep]
    out = np.zeros((c, 256), np.uint32)
    for ch in range(c):
        out[ch] = np.bincount(flat[chan == ch], minlength=256)
    return out


def _axis(dst_n, src_n, bug):
    """Source taps and weight of one axis of a half-pixel-centre bilinear
    resize: indices i0, i1 and the fraction of i1."""
    d = np.arange(dst_n, dtype=np.float64)
    if bug == "no_half_pixel":
        s = d * src_n / dst_n
    else:
        s = (d + 0.5) * src_n / dst_n - 0.5
    i0 = np.maximum(0, np.floor(s).astype(np.int64))
    if bug == "no_x1_clamp":    # reads past the edge; modelled as zero
        i1 = i0 + 1
    else:
        i1 = np.minimum(src_n - 1, i0 + 1)
    f = np.clip(s - i0, 0.0, 1.0)
    return i0, i1, f


def resize(frame, dh, dw, bug=None):
    """float64 bilinear resize, before rounding. [dh,dw,c]."""
    sh, sw, c = frame.shape
    src = frame.astype(np.float64)
    if bug == "no_x1_clamp":
        src = np.pad(src, ((0, 1), (0, 1), (0, 0)))
    y0, y1, fy = _axis(dh, sh, bug)
    x0, x1, fx = _axis(dw, sw, bug)
    fy = fy[:, None, None]
    fx = fx[None, :, None]
    top = src[y0][:, x0] * (1 - fx) + src[y0][:, x1] * fx
    bot = src[y1][:, x0] * (1 - fx) + src[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def blur(frame, ks, bug=None):
    """Box mean over the (2*(ks//2)+1)^2 window clipped to the frame, floor
    division by the number of pixels the clipped window holds."""
    h, w, c = frame.shape
    r = ks // 2
    src = np.pad(frame.astype(np.int64), ((r, r), (r, r), (0, 0)))
    one = np.pad(np.ones((h, w, 1), np.int64), ((r, r), (r, r), (0, 0)))
    total = np.zeros((h, w, c), np.int64)
    count = np.zeros((h, w, 1), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            total += src[dy:dy + h, dx:dx + w]
            count += one[dy:dy + h, dx:dx + w]
    if bug == "zero_pad":       # window not clipped: always (2r+1)^2 taps
        count = np.full_like(count, (2 * r + 1) ** 2)
    if bug == "round":
        return ((2 * total + count) // (2 * count)).astype(np.uint8)
    return (total // count).astype(np.uint8)


Y_COEF = (0.299, 0.587, 0.114)
U_COEF = (-0.169, -0.331, 0.5)
V_COEF = (0.5, -0.419, -0.081)


def gray(frame):
    """float64 BT.601 luma, before rounding. [h,w,1]."""
    return (frame.astype(np.float64) @ np.array(Y_COEF))[:, :, None]


def yuv(frame, bug=None):
    """float64 BT.601 full-range YUV, before rounding and clamping."""
    m = np.array([Y_COEF, U_COEF, V_COEF], np.float64)
    if bug == "coef":
        m[2, 1] += 0.001
    out = frame.astype(np.float64) @ m.T
    out[:, :, 1:] += 128.0
    return out


def crop(frame, x, y, width, height):
    return frame[y:y + height, x:x + width]


def planar(frame):
    return np.ascontiguousarray(frame.transpose(2, 0, 1))


# ---------------------------------------------------------------- tolerances

# gray/yuv: 8 float32 operations (3 conversions of exact integers are free;
# 3 products, 3 sums, the +0.5/+128.5 and the conversion of the coefficient
# itself) on magnitudes <= sum|coef|*255 + 128.5 < 384.
DELTA_COLOR = 8 * U * 384


def delta_resize(sh, sw):
    """The source coordinate takes three float32 roundings of magnitude <=
    the source size on each of two axes; the value moves by at most 255 per
    pixel of coordinate error. 16 more roundings of <= 256 cover the blend
    and the +0.5."""
    return 255.0 * (6 * max(sh, sw) * U + 16 * U)


# ---------------------------------------------------------------- comparators

def rounded_excess(got, real, clamp_hi=255.0):
    """max over elements of |got - clip(real)| - 0.5: how far beyond a
    correct rounding (ties either way) the worst element lies."""
    got = np.asarray(got)
    assert got.shape == real.shape, (got.shape, real.shape)
    want = np.clip(real, 0.0, clamp_hi)
    return float(np.max(np.abs(got.astype(np.float64) - want)) - 0.5)


def rounded_ok(got, real, delta, clamp_hi=255.0):
    return rounded_excess(got, real, clamp_hi) <= delta


def assert_rounded(got, real, delta, what):
    ex = rounded_excess(got, real)
    print(f"{what}: worst |got-real|-0.5 = {ex:.3e} (delta {delta:.3e})")
    assert ex <= delta, f"{what}: |got-real| exceeds 0.5 by {ex} > {delta}"
    return ex


def exact_ok(got, ref):
    got = np.asarray(got)
    return got.shape == ref.shape and got.dtype == ref.dtype and \
        bool(np.array_equal(got, ref))


def assert_exact(got, ref, what):
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert got.dtype == ref.dtype, (what, got.dtype, ref.dtype)
    bad = np.flatnonzero(got.reshape(-1) != ref.reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} of {ref.size} elements "
                           f"differ, first at {bad[0]}: "
                           f"{got.reshape(-1)[bad[0]]} != "
                           f"{ref.reshape(-1)[bad[0]]}")
