"""numpy reference for OpticalFlow (dense pyramidal Lucas-Kanade) and
FlowStats, the test inputs, and the tolerance.

`flow(..., dtype=np.float64)` is the reference. `dtype=np.float32` runs the
same statements in single precision, with numpy's summation order; the
difference of the two, E32, is what single precision costs on that input and
is measured without the code under test. A kernel is allowed 16 * E32: the
factor covers what the emulation does not share with a kernel (fma
contraction, another summation order over the 25-81 taps, the compiler's
division).

The algorithm, as csrc/ops/optflow_common.h and the two kernels define it:
luma (c == 3) or the single channel; a 2x2 box pyramid with h//2, w//2 and
num_levels(); per level and iteration, for every pixel, the 2x2 normal
equations over a (2R+1)^2 window of central-difference gradients of the
edge-clamped first image and of the temporal difference against the second
image sampled bilinearly (edge-clamped) at the window position displaced by
the *centre* pixel's flow; the update is applied where det > 1e-4; between
levels the flow is upsampled bilinearly (half-pixel centres, edge-clamped)
and scaled per axis by w/cw and h/ch.

`bug` seeds a defect into the reference for the comparator tests.
"""
import numpy as np

DET_EPS = 1e-4
U = 2.0 ** -24


def num_levels(h, w, maxl):
    n = 1
    while n < maxl and (h >> n) >= 24 and (w >> n) >= 24:
        n += 1
    return n


def _luma(frame, dt):
    f = frame.astype(dt)
    if frame.shape[2] == 3:
        return dt(0.299) * f[:, :, 0] + dt(0.587) * f[:, :, 1] + \
            dt(0.114) * f[:, :, 2]
    return f[:, :, 0]


def _down(img, dt):
    h, w = img.shape[0] // 2, img.shape[1] // 2
    a = img[0:2 * h:2, 0:2 * w:2]
    b = img[0:2 * h:2, 1:2 * w:2]
    c = img[1:2 * h:2, 0:2 * w:2]
    d = img[1:2 * h:2, 1:2 * w:2]
    return dt(0.25) * (a + b + c + d)


def _index(i, n, wrap):
    return np.mod(i, n) if wrap else np.clip(i, 0, n - 1)


def _at(img, y, x, wrap):
    h, w = img.shape[:2]
    return img[_index(y, h, wrap), _index(x, w, wrap)]


def _bilerp(img, fx, fy, dt, wrap):
    """img sampled at real positions (fx, fy); taps clamped to the image."""
    x0 = np.floor(fx)
    y0 = np.floor(fy)
    ax = (fx - x0).astype(dt)
    ay = (fy - y0).astype(dt)
    x0 = x0.astype(np.int64)
    y0 = y0.astype(np.int64)
    if img.ndim == 3:
        ax, ay = ax[..., None], ay[..., None]
    one = dt(1)
    return (_at(img, y0, x0, wrap) * (one - ay) * (one - ax) +
            _at(img, y0, x0 + 1, wrap) * (one - ay) * ax +
            _at(img, y0 + 1, x0, wrap) * ay * (one - ax) +
            _at(img, y0 + 1, x0 + 1, wrap) * ay * ax)


def _lk_iter(i0, i1, uv, radius, dt, bug):
    h, w = i0.shape
    wrap = bug == "wrap"
    half = dt(1.0) if bug == "grad_no_half" else dt(0.5)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = uv[:, :, 0], uv[:, :, 1]
    a11 = np.zeros((h, w), dt)
    a12 = np.zeros((h, w), dt)
    a22 = np.zeros((h, w), dt)
    b1 = np.zeros((h, w), dt)
    b2 = np.zeros((h, w), dt)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            py, px = yy + dy, xx + dx
            ix = half * (_at(i0, py, px + 1, wrap) - _at(i0, py, px - 1, wrap))
            iy = half * (_at(i0, py + 1, px, wrap) - _at(i0, py - 1, px, wrap))
            it = _bilerp(i1, px.astype(dt) + u, py.astype(dt) + v, dt, wrap) \
                - _at(i0, py, px, wrap)
            a11 += ix * ix
            a12 += ix * iy
            a22 += iy * iy
            b1 += ix * it
            b2 += iy * it
    det = a11 * a22 - a12 * a12
    ok = det > dt(DET_EPS)
    safe = np.where(ok, det, dt(1))
    out = np.empty_like(uv)
    out[:, :, 0] = np.where(ok, u - (a22 * b1 - a12 * b2) / safe, u)
    out[:, :, 1] = np.where(ok, v - (a11 * b2 - a12 * b1) / safe, v)
    return out, float(det.min())


def _upsample(uv, h, w, dt, bug):
    ch, cw = uv.shape[:2]
    sx = dt(w) / dt(cw)
    sy = dt(h) / dt(ch)
    if bug == "upsample_2x":
        sx = sy = dt(2)
    yy, xx = np.mgrid[0:h, 0:w]
    fx = (xx.astype(dt) + dt(0.5)) / sx - dt(0.5)
    fy = (yy.astype(dt) + dt(0.5)) / sy - dt(0.5)
    out = _bilerp(uv, fx, fy, dt, False)
    if bug != "upsample_noscale":
        out = out * np.array([sx, sy], dt)
    return out.astype(dt)


def flow(f0, f1, radius=3, iters=2, levels=4, dtype=np.float64, bug=None):
    """Flow from f0 to f1 (HWC u8, c = 1 or 3): ([h,w,2] of dtype, the
    smallest determinant met over all levels and iterations)."""
    dt = np.dtype(dtype).type
    if bug == "radius":
        radius += 1
    if bug == "iters":
        iters -= 1
    h, w = f0.shape[:2]
    n = num_levels(h, w, levels)
    p0, p1 = [_luma(f0, dt)], [_luma(f1, dt)]
    for _ in range(1, n):
        p0.append(_down(p0[-1], dt))
        p1.append(_down(p1[-1], dt))
    uv = np.zeros(p0[-1].shape + (2,), dt)
    min_det = np.inf
    for lv in range(n - 1, -1, -1):
        if lv < n - 1:
            uv = _upsample(uv, p0[lv].shape[0], p0[lv].shape[1], dt, bug)
        for _ in range(iters):
            uv, d = _lk_iter(p0[lv], p1[lv], uv, radius, dt, bug)
            min_det = min(min_det, d)
        assert uv.dtype == np.dtype(dtype)
    return uv, min_det


def flowstats(fl, bug=None):
    """float64 [mean|u|, mean|v|, max|u|, max|v|] of an [h,w,2] flow."""
    a = fl.reshape(-1, 2).astype(np.float64)
    n = a.shape[0]
    if bug != "signed":
        a = np.abs(a)
    if bug == "drop_chunk":     # the last partial chunk of 256 pixels lost
        a = a[:n - n % 256] if n % 256 else a
    mean = a.sum(axis=0) / n
    mx = a.max(axis=0) if a.size else np.zeros(2)
    return np.array([mean[0], mean[1], mx[0], mx[1]])


# ------------------------------------------------------------------- inputs

def _gauss(img, sigma):
    r = int(4 * sigma + 0.5)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    img = np.apply_along_axis(np.convolve, 0, img, k, mode="same")
    return np.apply_along_axis(np.convolve, 1, img, k, mode="same")


def textured_pair(h, w, dx=2, dy=1, c=3, sigma=1.5, seed=0):
    """Two h x w x c u8 views of one band-limited texture (gaussian-filtered
    noise). The pixel at (x, y) of the first is found at (x + dx, y + dy) in
    the second, so the true flow is (dx, dy). Both are cut from a larger
    image with a margin: nothing wraps around."""
    rng = np.random.RandomState(seed)
    m = 16
    big = np.stack([_gauss(rng.standard_normal((h + 2 * m, w + 2 * m)), sigma)
                    for _ in range(c)], axis=2)
    big = (big - big.min()) / (big.max() - big.min())
    big = np.round(255 * big).astype(np.uint8)
    a = big[m:m + h, m:m + w]
    b = big[m - dy:m - dy + h, m - dx:m - dx + w]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


# ----------------------------------------------------------------- tolerance

class FlowCase:
    """One input pair with both reference runs, computed once."""

    def __init__(self, name, f0, f1, **params):
        self.name, self.f0, self.f1, self.params = name, f0, f1, params
        self.ref, self.min_det = flow(f0, f1, dtype=np.float64, **params)
        f32, _ = flow(f0, f1, dtype=np.float32, **params)
        assert f32.dtype == np.float32
        self.e32 = float(np.abs(f32.astype(np.float64) - self.ref).max())
        self.tol = 16.0 * self.e32

    def err(self, got):
        got = np.asarray(got)
        assert got.shape == self.ref.shape and got.dtype == np.float32, \
            (self.name, got.shape, got.dtype)
        return float(np.abs(got.astype(np.float64) - self.ref).max())

    def ok(self, got):
        return self.err(got) <= self.tol

    def check(self, got, what=""):
        e = self.err(got)
        print(f"flow {self.name} {what}: E32 {self.e32:.3e} err {e:.3e} "
              f"err/tol {e / self.tol:.3f} min det {self.min_det:.3e}")
        assert e <= self.tol, (f"{self.name} {what}: max |got - flow64| "
                               f"{e:.3e} > 16*E32 {self.tol:.3e}")
        return e / self.tol


def flowstats_tol(ref4, npix):
    """Any-order float32 summation of npix non-negative terms, then one
    division: relative npix*2^-24 + 2^-24 on the mean; the max is exact."""
    mean = ref4[:2]
    return npix * U * mean + U * mean


def assert_flowstats(got, fl, what):
    got = np.asarray(got, np.float32)
    ref = flowstats(fl)
    npix = fl.shape[0] * fl.shape[1]
    assert got.shape == (4,), (what, got.shape)
    mx = np.abs(fl.reshape(-1, 2)).max(axis=0).astype(np.float32)
    assert got[2] == mx[0] and got[3] == mx[1], (what, got[2:], mx)
    err = np.abs(got[:2].astype(np.float64) - ref[:2])
    tol = flowstats_tol(ref, npix)
    print(f"flowstats {what}: mean err/tol "
          f"{np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol), (what, err, tol)


def flowstats_ok(got, ref4, npix, fl32_max):
    got = np.asarray(got, np.float32)
    return bool(got[2] == fl32_max[0] and got[3] == fl32_max[1] and np.all(
        np.abs(got[:2].astype(np.float64) - ref4[:2])
        <= flowstats_tol(ref4, npix)))
