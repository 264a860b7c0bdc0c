"""Case list shared by test_png_parallel_cpu.py and test_png_parallel_gpu.py:
frames for the "parallel" PNG writer, and helpers that take a PNG file
apart. Frames and the CPU writer's files are computed once per process."""
import functools
import struct
import zlib

import numpy as np

from scanner_amd import _core

K = _core.png_chunk_bytes()


def gradient(h, w, c, i=0):
    """One frame of conftest.make_smooth_video."""
    yy, xx = np.mgrid[0:h, 0:w]
    ch = [(xx + i * 2) % 256, (yy + i) % 256, (xx + yy + i * 3) % 256]
    return np.stack(ch[:c], -1).astype(np.uint8)


def _rng(h, w, c, salt):
    return np.random.RandomState(1000 * salt + 7 * h + 3 * w + c)


def _separable(h, w, c):
    """g(x) + h(y) with random steps: left predicts some pixels of a row
    best and above the others, which is where Paeth wins."""
    r = _rng(h, w, c, 5)
    gx = np.cumsum(r.randint(0, 21, (1, w, c)), 1)
    hy = np.cumsum(r.randint(0, 21, (h, 1, c)), 0)
    return ((gx + hy) % 256).astype(np.uint8)


def _ramp(h, w, c, ax, ay):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat(((ax * xx + ay * yy) % 256)[..., None], c,
                     -1).astype(np.uint8)


CONTENTS = {
    "const77": lambda h, w, c: np.full((h, w, c), 77, np.uint8),
    "const255": lambda h, w, c: np.full((h, w, c), 255, np.uint8),
    "gradient": lambda h, w, c: gradient(h, w, c, 3),
    "gradient3": lambda h, w, c: np.clip(
        gradient(h, w, c, 3).astype(np.int32)
        + _rng(h, w, c, 1).randint(-3, 4, (h, w, c)), 0, 255).astype(np.uint8),
    "noise": lambda h, w, c: _rng(h, w, c, 2).randint(
        0, 256, (h, w, c)).astype(np.uint8),
    "stripes": lambda h, w, c: np.broadcast_to(
        ((np.arange(w) % 2) * 200 + 20).astype(np.uint8)[None, :, None],
        (h, w, c)).copy(),
    "hramp": lambda h, w, c: _ramp(h, w, c, 5, 0),     # Sub
    "vramp": lambda h, w, c: _ramp(h, w, c, 0, 5),     # Up
    "dramp": lambda h, w, c: _ramp(h, w, c, 4, -4),    # Average
    "separable": _separable,                            # Paeth
}

SMALL = [(1, 1, 1), (1, 1, 3), (1, 40, 3), (40, 1, 1), (7, 5, 3)]
# grey, 128 filtered bytes per row: exactly one chunk, one row fewer, one more
EXACT = [(K // 128 + d, 127, 1) for d in (0, -1, 1)]
SPLIT = (105, 104, 3)     # two chunks; the cut falls mid-row and mid-pixel
THREE = (150, 150, 3)     # three chunks
BIG = (256, 256, 3)       # the frames of the size conditions

CASES = (
    [(s, c) for s in SMALL for c in ("gradient", "noise", "const77")]
    + [(s, c) for s in EXACT for c in ("gradient", "gradient3", "noise")]
    + [(SPLIT, c) for c in CONTENTS]
    + [(THREE, c) for c in ("gradient", "gradient3", "noise", "separable",
                            "stripes")]
    + [(BIG, c) for c in ("const77", "const255", "gradient", "gradient3")]
)
CASE_IDS = ["%dx%dx%d-%s" % (s + (c,)) for s, c in CASES]


@functools.lru_cache(maxsize=None)
def frame(shape, content):
    f = CONTENTS[content](*shape)
    assert f.shape == shape and f.dtype == np.uint8
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def cpu_png(shape, content):
    return _core.png_cpu_encode(frame(shape, content), "parallel")


def filtered_size(shape):
    h, w, c = shape
    return h * (1 + w * c)


def chunk_count(shape):
    return -(-filtered_size(shape) // K)


def png_chunks(blob):
    """[(type, data, crc_ok)] of a PNG file; asserts the signature and that
    nothing trails IEND."""
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(blob):
        (n,) = struct.unpack(">I", blob[pos:pos + 4])
        typ = blob[pos + 4:pos + 8]
        data = blob[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])
        out.append((typ, data, crc == zlib.crc32(typ + data)))
        pos += 12 + n
    assert pos == len(blob) and out[-1][0] == b"IEND"
    return out


def idat_payloads(blob):
    return [d for t, d, _ in png_chunks(blob) if t == b"IDAT"]


def inflate(blob):
    """The filtered stream: zlib.decompress of the concatenated IDATs."""
    return zlib.decompress(b"".join(idat_payloads(blob)))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def residual_rows(f):
    """int array [5, h, w*c]: the residuals of every row under each of the
    five PNG filters, as unsigned bytes. bpp = c; row 0 sees zeros above."""
    h, w, c = f.shape
    x = f.reshape(h, w * c).astype(np.int32)
    a = np.zeros_like(x)
    a[:, c:] = x[:, :-c]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, c:] = x[:-1, :-c]
    pred = np.stack([np.zeros_like(x), a, b, (a + b) >> 1, _paeth(a, b, cc)])
    return (x[None] - pred) % 256


def filter_rule(f):
    """Filter type per row by the rule: the smallest sum of |residual as
    signed 8-bit|, ties to the lowest type."""
    r = residual_rows(f)
    score = np.where(r < 128, r, 256 - r).sum(-1)   # [5, h]
    return np.argmin(score, 0)                       # first minimum


def unfilter(stream, shape):
    """Filtered stream -> (types [h], frame [h, w, c])."""
    h, w, c = shape
    rows = np.frombuffer(stream, np.uint8).reshape(h, 1 + w * c)
    types = rows[:, 0].astype(np.int64)
    out = np.zeros((h, w * c), np.int32)
    for y in range(h):
        res = rows[y, 1:].astype(np.int32)
        up = out[y - 1] if y else np.zeros(w * c, np.int32)
        t = types[y]
        if t == 0:
            out[y] = res
        elif t == 1:   # a running sum per channel
            out[y] = (np.cumsum(res.reshape(w, c), 0) % 256).reshape(-1)
        elif t == 2:
            out[y] = (res + up) % 256
        else:          # sequential in x: plain ints
            r, u, o = res.tolist(), up.tolist(), [0] * (w * c)
            for x in range(w * c):
                a = o[x - c] if x >= c else 0
                if t == 3:
                    pred = (a + u[x]) >> 1
                else:
                    ul = u[x - c] if x >= c else 0
                    p = a + u[x] - ul
                    pa, pb, pc = abs(p - a), abs(p - u[x]), abs(p - ul)
                    pred = a if pa <= pb and pa <= pc else (
                        u[x] if pb <= pc else ul)
                o[x] = (r[x] + pred) % 256
            out[y] = o
    return types, out.astype(np.uint8).reshape(h, w, c)
