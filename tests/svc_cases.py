"""SVC test clips and the decode case list, shared by the encoder tests and
by test_svc_decode_cpu.py / test_svc_decode_gpu.py / svc_decode_child.py.
No GPU is touched here."""
import functools
from collections import namedtuple

import numpy as np

import svc_ref as R
from conftest import make_smooth_video, make_video


def residual_for_bits(b):
    """A residual whose zigzag code needs exactly b bits: 0 -> 0, -1 -> 1,
    2^(b-2) -> 2^(b-1) for b >= 2."""
    return 0 if b == 0 else (-1 if b == 1 else 1 << (b - 2))


def crafted_bits(shape):
    n = shape[0]
    ngroups = (int(np.prod(shape[1:])) + 31) // 32
    f, g = np.mgrid[0:n, 0:ngroups]
    return (g + f) % 9


def crafted_widths_clip(shape, gop):
    """Group g of frame f is constant and needs exactly (g + f) % 9 bits:
    a key group holds 128 + r (first residual r, the rest 0), a delta group
    the previous frame's value + r (every residual r). gop is a period or a
    tuple of key frame indices."""
    n = shape[0]
    nbytes = int(np.prod(shape[1:]))
    bits = crafted_bits(shape)
    r = np.vectorize(residual_for_bits)(bits)
    vals = np.zeros(bits.shape, np.int64)
    for f in range(n):
        key = f in gop if isinstance(gop, tuple) else f % gop == 0
        vals[f] = (128 if key else vals[f - 1]) + r[f]
    flat = np.repeat(vals % 256, 32, axis=1)[:, :nbytes]
    return flat.astype(np.uint8).reshape(shape)


@functools.lru_cache(maxsize=None)
def clip(shape, content, gop=16):
    n, h, w, c = shape
    if content == "smooth":
        f = make_smooth_video(n=n, h=h, w=w)[..., :c]
    elif content == "noise":
        f = make_video(n=n, h=h, w=w, c=c, seed=11)
    elif content == "constant":
        f = np.full(shape, 77, np.uint8)
    elif content == "alternate":
        f = np.zeros(shape, np.uint8)
        f[1::2] = 128
    else:
        f = crafted_widths_clip(shape, gop)
    f = np.ascontiguousarray(f)
    f.setflags(write=False)
    return f


# ------------------------------------------------------------ decode cases

# (H, W, C): each the smallest at which its mechanism can break
SMALL_GEOMS = [
    (1, 3, 3),       # 9 B: one group, all tail
    (5, 7, 3),       # 105 B: 4 groups, 9-byte tail
    (1, 2048, 1),    # 64 groups: wave 1 has no valid lane
    (1, 2049, 1),    # 65 groups: wave 1 is one lane, a 1-byte tail
    (1, 2080, 1),    # 65 groups, no tail
    (32, 128, 1),    # 4096 B: exactly one supergroup
    (1, 4128, 1),    # a second supergroup of one group
    (37, 45, 3),     # 4995 B: 157 groups, 2nd supergroup partial, 3-byte tail
]
FULL_GEOMS = [(5, 7, 3), (37, 45, 3)]   # the full keys x want cross product
BIG_GEOM = (350, 1001, 3)   # 1 051 050 B: 257 supergroups, 10-byte tail; the
                            # first size past 2^20 bytes and supergroup 256
N, BIG_N = 40, 18

ENC_CONTENTS = ["smooth", "noise", "constant", "alternate", "widths"]
CONTENTS = ENC_CONTENTS + ["overwide8", "overwide_random", "one_group"]
BIG_CONTENTS = ["smooth", "noise", "widths"]

IRREGULAR = (0, 1, 2, 20, 21, 39)     # GOPs of 1, 1, 18, 1, 18, 1
KEYS = [(0,), tuple(range(0, N, 16)), tuple(range(0, N, 5)),
        tuple(range(N)), IRREGULAR]
ALL = tuple(range(N))
WANTS = [ALL, (39,), (0,), (15,), (16,), (15, 16), (17, 33),
         (0, 7, 18, 19, 33, 39), (2, 23, 38)]
FEW_KEYS = [(0,), IRREGULAR]
FEW_WANTS = [ALL, (39,), (17, 33)]
BIG_WANTS = [tuple(range(BIG_N)), (17,)]

Case = namedtuple("Case", "geom content keys n wants")


def geom_id(geom):
    return "x".join(map(str, geom))


def keys_id(keys):
    if len(keys) > 6:
        return f"k{len(keys)}"
    return "k" + "_".join(map(str, keys))


def case_id(case):
    return f"{geom_id(case.geom)}-{case.content}-{keys_id(case.keys)}"


def cases():
    out = []
    for geom in SMALL_GEOMS:
        full = geom in FULL_GEOMS
        for content in CONTENTS:
            for keys in (KEYS if full else FEW_KEYS):
                out.append(Case(geom, content, keys, N,
                                tuple(WANTS if full else FEW_WANTS)))
    for content in BIG_CONTENTS:
        out.append(Case(BIG_GEOM, content, (0,), BIG_N, tuple(BIG_WANTS)))
    return out


def one_group_index(nbytes):
    """one_group: 127 on shapes with at least 128 groups, otherwise the last
    full group (group 0 where the frame has no full group)."""
    ngroups = (nbytes + 31) // 32
    return 127 if ngroups >= 128 else max(nbytes // 32 - 1, 0)


@functools.lru_cache(maxsize=None)
def frames(geom, content, keys, n):
    """The source frames [n, H, W, C] of a case, read-only."""
    shape = (n,) + tuple(geom)
    if content in ("overwide8", "overwide_random"):
        return clip(shape, "smooth")
    if content == "one_group":
        # 128 everywhere: every key and every delta group needs 0 bits,
        # except group `g`, which is seeded noise in every frame
        nbytes = int(np.prod(geom))
        g = one_group_index(nbytes)
        f = np.full((n, nbytes), 128, np.uint8)
        lo, hi = g * 32, min(g * 32 + 32, nbytes)
        f[:, lo:hi] = np.random.RandomState(5).randint(
            0, 256, size=(n, hi - lo))
        f = f.reshape(shape)
        f.setflags(write=False)
        return f
    return clip(shape, content, keys if content == "widths" else 16)


@functools.lru_cache(maxsize=None)
def stream(geom, content, keys, n):
    """(bytes, sizes) of a case, written by svc_ref.write_stream."""
    widths = None
    if content == "overwide8":
        widths = 8
    elif content == "overwide_random":
        rng = np.random.RandomState(17)

        def widths(f, wmin):
            return wmin + rng.randint(0, 1 << 30, wmin.shape) % (9 - wmin)
    return R.write_stream(frames(geom, content, keys, n), keys, widths)


# How test_svc_decode_gpu.py calls svc_gpu_decode: (resident, first), first
# being 0 or the first frame of the span (a key frame)
PATHS = {
    "host": (False, True),        # stream_offset > 0 when the span starts late
    "resident0": (True, False),   # the whole stream resident, dev_lo = 0
    "resident_key": (True, True),  # resident from the span's key, dev_lo > 0
}


def gpu_decode(geom, content, keys, n, want, path):
    from scanner_amd import _core
    data, sizes = stream(geom, content, keys, n)
    resident, late = PATHS[path]
    first = R.decode_span(keys, want)[0] if late and want else 0
    return _core.svc_gpu_decode(data, sizes, *geom, list(keys), list(want),
                                resident=resident, first=first)


def check_gpu(geom, content, keys, n, want, paths=tuple(PATHS)):
    expect = frames(geom, content, keys, n)[list(want)]
    for path in paths:
        got = gpu_decode(geom, content, keys, n, want, path)
        np.testing.assert_array_equal(
            got, expect, f"{geom} {content} {keys_id(keys)} want={want} "
                         f"{path}")


def launches(keys, want, batch=16):
    """The kernel launches svc_decode_gpu makes for a sorted `want`, from
    the span and the key list alone: a key frame starts a chain, and a
    chain is cut every `batch` frames. Each launch is a dict of its frames,
    whether its first frame is predicted from the previous launch, whether
    the chain goes on after it, and whether its last frame is wanted."""
    keyset, wantset = set(keys), set(want)
    out = []
    for f in R.decode_span(keys, want):
        if f in keyset:
            out.append(dict(frames=[f], from_prev=False))
        elif len(out[-1]["frames"]) == batch:
            out.append(dict(frames=[f], from_prev=True))
        else:
            out[-1]["frames"].append(f)
    for i, launch in enumerate(out):
        launch["continues"] = i + 1 < len(out) and out[i + 1]["from_prev"]
        launch["last_wanted"] = launch["frames"][-1] in wantset
    return out
