"""Inputs shared by the Motion-JPEG tests: frames, Pillow-written files, a
small mp4 muxer and demuxer written for the tests (both Motion-JPEG sample
entries), and streams of samples laid out the way an item is."""
import io
import struct

import numpy as np
from PIL import Image

# the shapes of the issue: one MCU; one row of many MCUs, no multiple of the
# restart interval; colour at two sizes that are no multiple of a 4:2:0 MCU
SHAPES = [(8, 8, 1), (8, 264, 1), (16, 272, 3), (40, 520, 3)]
SUBSAMPLINGS = ["444", "420"]


def frames(n, h, w, c, seed=0, noise=16):
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.RandomState(seed)
    out = np.zeros((n, h, w, c), np.uint8)
    for i in range(n):
        smooth = np.stack([(3 * xx + yy + 5 * i) % 256,
                           (2 * yy + xx + 3 * i) % 256,
                           (xx * yy // 4 + i) % 256], -1)[..., :c]
        out[i] = (smooth + rng.randint(0, noise, (h, w, c))) % 256
    return out


def noise_frames(n, h, w, c, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, c)).astype(
        np.uint8)


def pillow_jpeg(frame, **kw):
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(
        buf, "JPEG", **kw)
    return buf.getvalue()


def with_comment(blob, k):
    """The file with a COM segment of k payload bytes behind SOI."""
    assert blob[:2] == b"\xff\xd8" and 0 <= k <= 65533
    return blob[:2] + b"\xff\xfe" + struct.pack(">H", k + 2) + b"c" * k + \
        blob[2:]


def layout(samples, lead=0, gap=0):
    """(stream, offsets, sizes): the samples back to back behind `lead`
    bytes, `gap` bytes between them."""
    stream = bytearray(b"\x00" * lead)
    offsets, sizes = [], []
    for s in samples:
        offsets.append(len(stream))
        sizes.append(len(s))
        stream += s
        stream += b"\x00" * gap
    return bytes(stream), offsets, sizes


def scan_start(blob):
    """Offset of the first entropy-coded byte of a single-scan file."""
    pos = 2
    while True:
        assert blob[pos] == 0xff
        m = blob[pos + 1]
        ln = struct.unpack(">H", blob[pos + 2:pos + 4])[0]
        pos += 2 + ln
        if m == 0xda:
            return pos


# ---- mp4 ----

def _box(kind, body):
    return struct.pack(">I", 8 + len(body)) + kind + body


def _visual_entry(kind, w, h, extra=b""):
    body = b"\x00" * 6 + struct.pack(">H", 1) + b"\x00" * 16 + \
        struct.pack(">HH", w, h) + struct.pack(">II", 0x480000, 0x480000) + \
        b"\x00" * 4 + struct.pack(">H", 1) + b"\x00" * 32 + \
        struct.pack(">HH", 0x18, 0xffff) + extra
    return _box(kind, body)


def _esds(oti):
    dcd = bytes([oti, 0x11, 0, 0, 0]) + b"\x00" * 8
    sl = bytes([0x06, 1, 0x02])
    es = struct.pack(">HB", 1, 0) + bytes([0x04, len(dcd)]) + dcd + sl
    return _box(b"esds", b"\x00" * 4 + bytes([0x03, len(es)]) + es)


def mux_mp4(samples, w, h, entry="jpeg", oti=0x6c, chunk=3):
    """An mp4 with one video track of the given samples, `chunk` samples per
    chunk (so stsc and stco matter), no stss. entry: 'jpeg' or 'mp4v'."""
    n = len(samples)
    ftyp = _box(b"ftyp", b"qt  " + struct.pack(">I", 0) + b"qt  ")
    mdat_body = b"".join(samples)
    base = len(ftyp) + 8
    offs, p = [], base
    for s in samples:
        offs.append(p)
        p += len(s)
    chunks = list(range(0, n, chunk))
    se = _visual_entry(b"jpeg", w, h) if entry == "jpeg" else \
        _visual_entry(b"mp4v", w, h, _esds(oti))
    stsd = _box(b"stsd", struct.pack(">II", 0, 1) + se)
    stts = _box(b"stts", struct.pack(">IIII", 0, 1, n, 3000))
    runs = [(1, min(chunk, n))]
    if n % chunk and len(chunks) > 1:
        runs.append((len(chunks), n % chunk))
    stsc = _box(b"stsc", struct.pack(">II", 0, len(runs)) + b"".join(
        struct.pack(">III", f, k, 1) for f, k in runs))
    stsz = _box(b"stsz", struct.pack(">III", 0, 0, n) + b"".join(
        struct.pack(">I", len(s)) for s in samples))
    stco = _box(b"stco", struct.pack(">II", 0, len(chunks)) + b"".join(
        struct.pack(">I", offs[c]) for c in chunks))
    stbl = _box(b"stbl", stsd + stts + stsc + stsz + stco)
    minf = _box(b"minf", stbl)
    mdhd = _box(b"mdhd", struct.pack(">IIIIIHH", 0, 0, 0, 90000, n * 3000,
                                     0x55c4, 0))
    hdlr = _box(b"hdlr", struct.pack(">II", 0, 0) + b"vide" + b"\x00" * 12 +
                b"v\x00")
    trak = _box(b"trak", _box(b"mdia", mdhd + hdlr + minf))
    return ftyp + _box(b"mdat", mdat_body) + _box(b"moov", trak)


def _children(buf, off, end):
    out = {}
    while off + 8 <= end:
        size, kind = struct.unpack(">I4s", buf[off:off + 8])
        assert size >= 8 and off + size <= end
        out.setdefault(kind, (off + 8, off + size))
        off += size
    return out


def demux_mp4(buf):
    """(sample entry fourcc, entry width, height, esds body or None, has
    stss, samples) of the first track of a file written by export."""
    top = _children(buf, 0, len(buf))
    moov = _children(buf, *top[b"moov"])
    trak = _children(buf, *moov[b"trak"])
    mdia = _children(buf, *trak[b"mdia"])
    minf = _children(buf, *mdia[b"minf"])
    stbl = _children(buf, *minf[b"stbl"])
    s0, s1 = stbl[b"stsd"]
    esize, kind = struct.unpack(">I4s", buf[s0 + 8:s0 + 16])
    w, h = struct.unpack(">HH", buf[s0 + 16 + 24:s0 + 16 + 28])
    kids = _children(buf, s0 + 16 + 78, s0 + 8 + esize)
    esds = buf[kids[b"esds"][0]:kids[b"esds"][1]] if b"esds" in kids else None
    z0, _ = stbl[b"stsz"]
    fixed, n = struct.unpack(">II", buf[z0 + 4:z0 + 12])
    sizes = [fixed] * n if fixed else list(
        struct.unpack(">%dI" % n, buf[z0 + 12:z0 + 12 + 4 * n]))
    c0, _ = stbl[b"stco"]
    nchunks = struct.unpack(">I", buf[c0 + 4:c0 + 8])[0]
    chunk_off = struct.unpack(">%dI" % nchunks,
                              buf[c0 + 8:c0 + 8 + 4 * nchunks])
    r0, _ = stbl[b"stsc"]
    nruns = struct.unpack(">I", buf[r0 + 4:r0 + 8])[0]
    runs = [struct.unpack(">III", buf[r0 + 8 + 12 * i:r0 + 20 + 12 * i])
            for i in range(nruns)]
    samples, si = [], 0
    for ri, (first, per, _) in enumerate(runs):
        last = runs[ri + 1][0] if ri + 1 < nruns else nchunks + 1
        for ch in range(first, last):
            off = chunk_off[ch - 1]
            for _ in range(per):
                if si == n:
                    break
                samples.append(buf[off:off + sizes[si]])
                off += sizes[si]
                si += 1
    assert si == n
    return kind, w, h, esds, b"stss" in stbl, samples
