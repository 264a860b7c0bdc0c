"""The SVC packet format restated in numpy, from the header comment of
csrc/video/svc.h alone: a writer that may spend more bits on a group than it
needs (the format allows it, the encoders never do it) and a reader
vectorised over the groups of a frame. Neither follows the loops of
svc_cpu.cpp or of the HIP kernel.

One packet per frame:
    u32 'SVC1' | u8 type (0 key, 1 delta) | 3 pad | u32 nbytes | u32 ngroups
    | u32 nsuper | u32 super_off[nsuper] | u8 width[ngroups] | pad to 4
    | packed region: group g holds 32 values of width[g] bits, LSB-first, in
      4 * width[g] bytes; supergroup s (128 groups) starts at super_off[s]

A key frame predicts each byte from the previous byte of its group (the
first from 128), a delta frame from the same byte of the previous frame; the
residual, reduced to a signed byte, is zigzag-mapped to 0..255.
"""
import struct

import numpy as np

BIT_LENGTH = np.array([int(i).bit_length() for i in range(256)], np.int64)

# defects that read_stream can be asked to have (test_svc_decode_cpu.py)
DEFECTS = (
    "msb_first",          # the packed bytes unpacked MSB-first
    "key_pred_0",         # key predictor starts at 0, not 128
    "key_pred_across",    # key predictor runs across the group boundary
    "zigzag_sign",        # zigzag sign flipped
    "carry_dropped",      # groups 64..127 of a supergroup read from offset 0
    "super_off_ignored",  # every supergroup read from the region start
    "tail_prev32",        # the tail group takes 32 bytes of `prev`
    "delta_prev_prev",    # a delta frame predicted from the frame before prev
)


def geometry(nbytes):
    ngroups = -(-nbytes // 32)
    return ngroups, -(-ngroups // 128)


def zigzag(d):
    v = (np.asarray(d, np.int64) + 128) % 256 - 128
    return np.where(v >= 0, 2 * v, -2 * v - 1)


def unzigzag(z):
    z = np.asarray(z, np.int64)
    return np.where(z & 1, -((z + 1) // 2), z // 2)


# the two maps as tables over the byte values; all frame arithmetic below is
# uint8, which wraps modulo 256 as the format's residuals do
ZIGZAG = zigzag(np.arange(256)).astype(np.uint8)
UNZIGZAG = (unzigzag(np.arange(256)) % 256).astype(np.uint8)


def _padded(frame, ngroups):
    out = np.zeros(ngroups * 32, np.uint8)
    out[:frame.size] = frame.reshape(-1)
    return out.reshape(ngroups, 32)


def codes(cur, prev):
    """Zigzag codes [ngroups, 32] of a frame; bytes past the frame code 0."""
    nbytes = cur.size
    ngroups, _ = geometry(nbytes)
    c = _padded(cur, ngroups)
    if prev is None:
        pred = np.concatenate(
            [np.full((ngroups, 1), 128, np.uint8), c[:, :-1]], axis=1)
    else:
        pred = _padded(prev, ngroups)
    z = ZIGZAG[c - pred]
    z.reshape(-1)[nbytes:] = 0
    return z


def minimal_widths(z):
    return BIT_LENGTH[z.max(axis=1)]


def _offsets(widths):
    """Exclusive prefix sum of the group payload sizes, and their total."""
    size = 4 * np.asarray(widths, np.int64)
    end = np.cumsum(size)
    return end - size, int(end[-1])


def write_packet(cur, prev, widths=None):
    """The packet of `cur` (any uint8 array), a key frame when prev is None.
    widths: None (minimal), an int, an array [ngroups], or a callable
    minimal -> array; every entry must lie in [minimal, 8]."""
    cur = np.asarray(cur, np.uint8)
    nbytes = cur.size
    ngroups, nsuper = geometry(nbytes)
    z = codes(cur, prev)
    wmin = minimal_widths(z)
    if widths is None:
        w = wmin
    elif callable(widths):
        w = np.asarray(widths(wmin), np.int64)
    else:
        w = np.broadcast_to(np.asarray(widths, np.int64), wmin.shape)
    assert w.shape == wmin.shape and (w >= wmin).all() and (w <= 8).all()
    excl, total = _offsets(w)
    packed = np.zeros(total, np.uint8)
    for k in np.unique(w):
        if k == 0:
            continue
        idx = np.nonzero(w == k)[0]
        bits = np.unpackbits(z[idx][:, :, None], axis=2,
                             bitorder="little")[:, :, :k]
        by = np.packbits(bits.reshape(len(idx), 32 * k), axis=1,
                         bitorder="little")
        packed[excl[idx][:, None] + np.arange(4 * k)] = by
    head = struct.pack("<4sB3xIII", b"SVC1", 0 if prev is None else 1, nbytes,
                       ngroups, nsuper)
    return b"".join([head, excl[::128].astype("<u4").tobytes(),
                     w.astype(np.uint8).tobytes(), bytes(-ngroups % 4),
                     packed.tobytes()])


def write_stream(frames, keyframes, widths=None):
    """(bytes, sizes) of a clip [N, ...]. widths: as write_packet, or a
    callable (frame index, minimal) -> array."""
    keys = set(keyframes)
    pkts = []
    for f in range(len(frames)):
        wf = widths
        if callable(widths):
            wf = (lambda m, f=f: widths(f, m))
        pkts.append(write_packet(frames[f],
                                 None if f in keys else frames[f - 1], wf))
    return b"".join(pkts), [len(p) for p in pkts]


def stream_widths(stream, sizes, nbytes):
    """The width[] arrays [N, ngroups] of a packet stream."""
    ngroups, nsuper = geometry(nbytes)
    buf = np.frombuffer(stream, np.uint8)
    starts = np.cumsum([0] + list(sizes[:-1])) + 20 + 4 * nsuper
    return np.stack([buf[s:s + ngroups] for s in starts])


def read_stream(stream, sizes, h, w, c, keyframes, defect=None):
    """All frames [N, h, w, c] of a packet stream. Frame f is a key frame
    when f is in `keyframes` (the packet's type byte must agree)."""
    assert defect is None or defect in DEFECTS
    nbytes = h * w * c
    ngroups, nsuper = geometry(nbytes)
    keys = set(keyframes)
    buf = np.frombuffer(stream, np.uint8)
    g = np.arange(ngroups)
    first = g // 128 * 128          # first group of g's supergroup
    out = np.zeros((len(sizes), ngroups * 32), np.uint8)
    off = 0
    for f, size in enumerate(sizes):
        pkt = buf[off:off + size]
        off += size
        magic, typ, nb, ng, ns = struct.unpack("<4sB3xIII", pkt[:20].tobytes())
        assert (magic, nb, ng, ns) == (b"SVC1", nbytes, ngroups, nsuper)
        assert (typ == 0) == (f in keys)
        wo = 20 + 4 * nsuper
        super_off = pkt[20:wo].view("<u4").astype(np.int64)
        width = pkt[wo:wo + ngroups].astype(np.int64)
        assert (width <= 8).all()
        packed = pkt[wo + (ngroups + 3) // 4 * 4:]
        excl, total = _offsets(width)
        assert total == packed.size
        local = excl - excl[first]
        if defect == "carry_dropped":
            up = np.nonzero(g - first >= 64)[0]
            local[up] -= excl[first[up] + 64] - excl[first[up]]
        at = local if defect == "super_off_ignored" \
            else super_off[g // 128] + local
        z = np.zeros((ngroups, 32), np.uint8)
        for k in np.unique(width):
            if k == 0:
                continue
            idx = np.nonzero(width == k)[0]
            by = packed[at[idx][:, None] + np.arange(4 * k)]
            bits = np.unpackbits(
                by, axis=1,
                bitorder="big" if defect == "msb_first" else "little")
            z[idx] = np.packbits(bits.reshape(len(idx), 32, k), axis=2,
                                 bitorder="little")[:, :, 0]
        r = UNZIGZAG[z]
        if defect == "zigzag_sign":
            r = np.negative(r)
        if f in keys:
            start = 0 if defect == "key_pred_0" else 128
            if defect == "key_pred_across":
                cur = np.cumsum(r.reshape(-1), dtype=np.uint8)
            else:
                cur = np.cumsum(r, axis=1, dtype=np.uint8)
            cur = cur + np.uint8(start)
        else:
            src = f - 2 if defect == "delta_prev_prev" else f - 1
            pred = (out[src] if src >= 0 else np.zeros_like(out[0])) \
                .reshape(ngroups, 32).copy()
            if defect == "tail_prev32" and nbytes % 32 and nbytes >= 32:
                pred[-1] = out[f - 1][nbytes - 32:nbytes]
            cur = pred + r
        out[f] = cur.reshape(-1)
    return out[:, :nbytes].reshape(len(sizes), h, w, c)


def decode_span(keyframes, want):
    """The frames that must be decoded for `want`: for each wanted frame,
    everything from the last key frame at or before it."""
    need = set()
    for f in want:
        k = max(k for k in keyframes if k <= f)
        need.update(range(k, f + 1))
    return sorted(need)
