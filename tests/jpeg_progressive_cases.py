"""Progressive JPEG inputs for the ImageDecoder tests.

Two sources. Pillow (libjpeg) writes SOF2 files with its fixed script: 10
scans for colour, 6 for grey, restart markers on request. A small writer
here turns the quantised coefficients of a baseline file
(_core.jpeg_decode_coefficients) and any scan script into a progressive file,
for the scripts Pillow never writes. Its Huffman tables give every symbol a
code of one length and leave the all-ones code unused, so libjpeg reads its
files too.

The oracle everywhere is the baseline file of the same image: libjpeg
computes the same quantised coefficients whatever the entropy mode, so the
decoder must give the same coefficients and the same pixels for both."""
import functools
import io

import numpy as np
from PIL import Image

from scanner_amd import _core
from test_jpeg_cpu import image
from test_image_decode_cpu import pillow_save


# ---------------- Pillow files ----------------

VARIANTS = {
    "plain": {},
    "rst1": dict(restart_marker_blocks=1),
    "rst2": dict(restart_marker_blocks=2),
    "rows1": dict(restart_marker_rows=1),
    "optimize": dict(optimize=True),
}


@functools.lru_cache(maxsize=None)
def pillow_pair(shape, content, quality, subsampling=0, variant="plain",
                seed=0):
    """(baseline file, progressive file) of one image, same quality,
    subsampling and restart setting."""
    kw = dict(quality=quality, **VARIANTS[variant])
    if shape[2] == 3:
        kw["subsampling"] = subsampling
    frame = image(shape, content, seed)
    return (pillow_save(frame, **kw),
            pillow_save(frame, progressive=True, **kw))


# shape, subsampling, restart variant (None: only without restart markers)
IDENTITY_SHAPES = [
    ((1, 1, 1), 0, "rst2"),
    ((8, 8, 1), 0, "rst2"),
    ((7, 9, 3), 0, "rst2"),
    ((17, 33, 3), 2, "rst2"),
    ((16, 24, 3), 1, "rst2"),
    ((40, 56, 3), 2, "rows1"),
    ((72, 72, 1), 0, "rst1"),  # 81 segments per scan: two workgroups, the
                               # RST index wraps
]
IDENTITY_CONTENTS = ["smooth", "noise", "checker", "constant"]
IDENTITY_QUALITIES = [1, 50, 100]


def identity_cases(dri):
    """(id, baseline, progressive) over the shapes, contents and qualities;
    dri False: the files without restart markers."""
    out = []
    for shape, sub, variant in IDENTITY_SHAPES:
        for content in IDENTITY_CONTENTS:
            for q in IDENTITY_QUALITIES:
                v = variant if dri else "plain"
                base, prog = pillow_pair(shape, content, q, sub, v)
                name = "x".join(map(str, shape)) + f"_{sub}_{content}_q{q}_{v}"
                out.append((name, base, prog))
    return out


# ---------------- the writer ----------------

def zigzag():
    zz = []
    for s in range(15):
        for i in range(max(0, s - 7), min(s, 7) + 1):
            r = i if s & 1 else s - i
            zz.append(r * 8 + (s - r))
    return zz


ZZ = zigzag()


class HuffTable:
    """Every symbol gets a code of `length` bits, in the order given: n
    codes 0..n-1 use at most half of the code space, so there is no
    all-ones code."""

    def __init__(self, symbols, length):
        self.symbols = list(symbols)
        assert len(self.symbols) <= min(255, 1 << (length - 1))
        self.length = length
        self.code = {s: i for i, s in enumerate(self.symbols)}

    def dht_payload(self, tc, th):
        bits = [0] * 16
        bits[self.length - 1] = len(self.symbols)
        return bytes([tc << 4 | th]) + bytes(bits) + bytes(self.symbols)


def tables(variant):
    """(DC, AC); variant 1 has other lengths and the reverse order."""
    # a DHT count is one byte, so not all 256 symbols fit one length: the AC
    # tables hold every run with the sizes 0..10 an 8-bit image can need
    ac = [r << 4 | n for r in range(16) for n in range(11)]
    if variant == 0:
        return HuffTable(range(16), 5), HuffTable(ac, 9)
    return (HuffTable(list(reversed(range(16))), 6),
            HuffTable(list(reversed(ac)), 10))


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        if nbits == 0:
            return
        self.acc = self.acc << nbits | (value & ((1 << nbits) - 1))
        self.n += nbits
        while self.n >= 8:
            b = self.acc >> (self.n - 8) & 0xff
            self.out.append(b)
            if b == 0xff:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def marker(code, payload=b""):
    return bytes([0xff, code]) + (len(payload) + 2).to_bytes(2, "big") + payload


def parse_baseline(blob):
    """DQT payloads and the SOF payload of a baseline file."""
    pos, dqt, sof = 2, [], None
    while True:
        assert blob[pos] == 0xff
        m = blob[pos + 1]
        n = int.from_bytes(blob[pos + 2:pos + 4], "big")
        payload = blob[pos + 4:pos + 2 + n]
        if m == 0xdb:
            dqt.append(payload)
        elif m in (0xc0, 0xc1):
            sof = payload
        elif m == 0xda:
            return dqt, sof
        pos += 2 + n


class ScanEncoder:
    """One scan, libjpeg's progressive encoder in outline (T.81 G.1.2)."""

    def __init__(self, scan, dc, ac, counts):
        self.ss, self.se = scan["ss"], scan["se"]
        self.ah, self.al = scan["ah"], scan["al"]
        self.dc, self.ac, self.counts = dc, ac, counts
        self.w = BitWriter()
        self.reset()

    def reset(self):
        self.pred = {}
        self.eobrun = 0
        self.pending = []  # correction bits of the blocks of the EOB run

    def symbol(self, table, s):
        self.w.put(table.code[s], table.length)

    def flush_eobrun(self):
        if self.eobrun:
            n = self.eobrun.bit_length() - 1
            self.symbol(self.ac, n << 4)
            self.w.put(self.eobrun, n)
            self.counts["eob"][n] = self.counts["eob"].get(n, 0) + 1
            self.counts["max_eobrun"] = max(self.counts["max_eobrun"],
                                            self.eobrun)
            self.eobrun = 0
        for b in self.pending:
            self.w.put(b, 1)
        self.counts["correction_bits"] += len(self.pending)
        self.pending = []

    def block(self, comp, blk):
        """blk: 64 coefficients in natural order."""
        if self.ss == 0:
            v = int(blk[0]) >> self.al
            if self.ah:
                self.w.put(v & 1, 1)
                return
            d = v - self.pred.get(comp, 0)
            self.pred[comp] = v
            n = abs(d).bit_length()
            self.symbol(self.dc, n)
            self.w.put(d if d >= 0 else d - 1, n)
            return
        if self.ah == 0:
            self.ac_first(blk)
        else:
            self.ac_refine(blk)

    def ac_first(self, blk):
        r = 0
        for k in range(self.ss, self.se + 1):
            t = int(blk[ZZ[k]])
            a = abs(t) >> self.al
            if a == 0:
                r += 1
                continue
            self.flush_eobrun()
            while r > 15:
                self.symbol(self.ac, 0xf0)
                r -= 16
            n = a.bit_length()
            self.symbol(self.ac, r << 4 | n)
            self.w.put(a if t >= 0 else ~a, n)
            r = 0
        if r > 0:
            self.eobrun += 1
            if self.eobrun == 0x7fff:
                self.flush_eobrun()

    def ac_refine(self, blk):
        absv = {k: abs(int(blk[ZZ[k]])) >> self.al
                for k in range(self.ss, self.se + 1)}
        eob = max([k for k, a in absv.items() if a == 1], default=0)
        if any(a > 1 for a in absv.values()):
            self.counts["refined_history"] += 1
        r, br = 0, []
        for k in range(self.ss, self.se + 1):
            a = absv[k]
            if a == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                self.flush_eobrun()
                self.symbol(self.ac, 0xf0)
                self.counts["refine_zrl"] += 1
                r -= 16
                for b in br:
                    self.w.put(b, 1)
                self.counts["correction_bits"] += len(br)
                br = []
            if a > 1:
                br.append(a & 1)
                continue
            self.flush_eobrun()
            self.symbol(self.ac, r << 4 | 1)
            self.w.put(0 if int(blk[ZZ[k]]) < 0 else 1, 1)
            for b in br:
                self.w.put(b, 1)
            self.counts["correction_bits"] += len(br)
            br = []
            r = 0
        if r > 0 or br:
            self.eobrun += 1
            self.pending += br
            if self.eobrun == 0x7fff or len(self.pending) > 900:
                self.flush_eobrun()

    def end_segment(self, last):
        if self.eobrun and not last:
            self.counts["runs_cut_by_restart"] += 1
        if self.eobrun > 1:
            self.counts["multi_block_runs"] += 1
        self.flush_eobrun()
        self.w.pad()


def new_counts():
    return dict(eob={}, max_eobrun=0, refine_zrl=0, correction_bits=0,
                runs_cut_by_restart=0, multi_block_runs=0,
                refined_history=0)


def write_progressive(base, script, redefine_dht=False):
    """The image of the baseline file `base` as a progressive file that
    follows `script`: a list of scans, each a dict of comps (frame indices),
    ss, se, ah, al and optionally dri, a restart interval that a DRI segment
    in front of the scan sets (0 switches restarts off). With redefine_dht
    every scan is preceded by DHT segments that redefine tables 0, in turn
    with two different sets. Nothing checks the script: invalid ones are
    written as they are. Returns (file, counts)."""
    info = _core.jpeg_decode_info(base)
    coefs = _core.jpeg_decode_coefficients(base)
    h, w, nc, hs, vs = (info[k] for k in ("h", "w", "c", "hs", "vs"))
    mcus_x = -(-w // (8 * hs))
    mcus_y = -(-h // (8 * vs))
    # luma over the MCU-padded raster for the interleaved scans; the padding
    # blocks, which no pixel shows, are zero
    luma = np.zeros((mcus_y * vs, mcus_x * hs, 64), np.int16)
    luma[:coefs[0].shape[0], :coefs[0].shape[1]] = coefs[0]
    dqt, sof = parse_baseline(base)
    counts = new_counts()
    out = bytearray(b"\xff\xd8")
    for p in dqt:
        out += marker(0xdb, p)
    out += marker(0xc2, sof)
    dc, ac = tables(0)
    if not redefine_dht:
        out += marker(0xc4, dc.dht_payload(0, 0))
        out += marker(0xc4, ac.dht_payload(1, 0))
    ri = 0
    for i, scan in enumerate(script):
        if "dri" in scan:
            ri = scan["dri"]
            out += marker(0xdd, ri.to_bytes(2, "big"))
        if redefine_dht:
            dc, ac = tables(i % 2)
            out += marker(0xc4, dc.dht_payload(0, 0))
            out += marker(0xc4, ac.dht_payload(1, 0))
        comps = scan["comps"]
        sos = bytes([len(comps)])
        for c in comps:
            sos += bytes([sof[6 + 3 * c], 0])
        sos += bytes([scan["ss"], scan["se"], scan["ah"] << 4 | scan["al"]])
        out += marker(0xda, sos)
        if len(comps) == 1:
            c = comps[0]
            units = [[(c, blk)] for row in coefs[c] for blk in row]
        else:
            units = []
            for my in range(mcus_y):
                for mx in range(mcus_x):
                    u = [(0, luma[my * vs + b // hs, mx * hs + b % hs])
                         for b in range(hs * vs)]
                    u += [(c, coefs[c][my, mx]) for c in range(1, nc)]
                    units.append(u)
        enc = ScanEncoder(scan, dc, ac, counts)
        per = ri if ri else len(units)
        nseg = -(-len(units) // per)
        for s in range(nseg):
            enc.reset()
            for u in units[s * per:(s + 1) * per]:
                for c, blk in u:
                    enc.block(c, blk)
            enc.end_segment(s == nseg - 1)
            if s < nseg - 1:
                enc.w.out += bytes([0xff, 0xd0 + (s & 7)])
        out += enc.w.out
    out += b"\xff\xd9"
    return bytes(out), counts


def scan(comps, ss, se, ah, al, **kw):
    return dict(comps=list(comps), ss=ss, se=se, ah=ah, al=al, **kw)


def script_spectral_only(nc):
    """Spectral selection alone: every Al is 0."""
    s = [scan(range(nc), 0, 0, 0, 0)]
    for c in range(nc):
        s += [scan([c], 1, 5, 0, 0), scan([c], 6, 63, 0, 0)]
    return s


def script_dc_per_component(nc):
    """DC in single-component scans, the last component first."""
    s = [scan([c], 0, 0, 0, 0) for c in reversed(range(nc))]
    s += [scan([c], 1, 63, 0, 0) for c in range(nc)]
    return s


def script_successive(nc, top=3, stop_early=False):
    """Successive approximation from Al=top down in single steps; with
    stop_early the last AC bit is never refined."""
    s = [scan(range(nc), 0, 0, 0, top)]
    s += [scan([c], 1, 63, 0, top) for c in range(nc)]
    for al in reversed(range(top)):
        s.append(scan(range(nc), 0, 0, al + 1, al))
        if al == 0 and stop_early:
            break
        s += [scan([c], 1, 63, al + 1, al) for c in range(nc)]
    return s


def script_dri_changes(nc):
    """The restart interval set by DRI segments between scans: 2 MCUs for
    the DC scan, 3 blocks, then 1, then 5 for the refinements."""
    s = [scan(range(nc), 0, 0, 0, 1, dri=2)]
    s += [scan([c], 1, 63, 0, 1, **({"dri": 3} if c == 0 else {}))
          for c in range(nc)]
    s.append(scan(range(nc), 0, 0, 1, 0, dri=1))
    s += [scan([c], 1, 63, 1, 0, **({"dri": 5} if c == 0 else {}))
          for c in range(nc)]
    return s


def script_dri_switched_off():
    """Grey: restart interval 3 for the first scans, then a DRI of 0."""
    s = with_dri(script_successive(1, 1), 3)
    s[2] = dict(s[2], dri=0)
    return s


def with_dri(script, ri):
    """The script with restart interval ri from the first scan on."""
    return [dict(script[0], dri=ri)] + script[1:]


@functools.lru_cache(maxsize=None)
def writer_bases():
    """Baseline files the writer recodes: name -> file."""
    return {
        "420": pillow_pair((17, 33, 3), "noise", 90, 2)[0],
        "444": pillow_pair((16, 24, 3), "smooth", 75, 0)[0],
        "grey": pillow_pair((33, 50, 1), "noise", 95, 0)[0],
        # 272 blocks of nothing but DC: one EOB run per AC scan
        "constant": pillow_pair((136, 128, 1), "constant", 75, 0)[0],
    }


@functools.lru_cache(maxsize=None)
def writer_cases():
    """name -> (baseline, progressive, counts, stops_early, every scan has a
    restart interval). The scripts Pillow never writes."""
    b = writer_bases()
    made = {
        "spectral_only_420": (b["420"], script_spectral_only(3), False),
        "spectral_only_420_dri": (
            b["420"], with_dri(script_spectral_only(3), 2), False),
        "dc_per_component_444": (b["444"], script_dc_per_component(3), False),
        "dc_per_component_444_dri": (
            b["444"], with_dri(script_dc_per_component(3), 1), False),
        "successive_from_3_420": (b["420"], script_successive(3), False),
        "successive_from_3_420_dri": (
            b["420"], with_dri(script_successive(3), 3), False),
        "successive_from_3_grey_dri": (
            b["grey"], with_dri(script_successive(1), 4), False),
        "dri_changes_420": (b["420"], script_dri_changes(3), False),
        "dri_switched_off_grey": (b["grey"], script_dri_switched_off(), False),
        "dht_redefined_444": (b["444"], script_successive(3, 2), True),
        "dht_redefined_444_dri": (
            b["444"], with_dri(script_successive(3, 2), 2), True),
        "stops_early_420": (
            b["420"], script_successive(3, 2, stop_early=True), False),
        "stops_early_420_dri": (
            b["420"], with_dri(script_successive(3, 2, stop_early=True), 2),
            False),
        "constant_272_blocks": (b["constant"], script_successive(1, 1), False),
    }
    out = {}
    for name, (base, script, redefine) in made.items():
        prog, counts = write_progressive(base, script, redefine)
        ri, all_dri = 0, True
        for s in script:
            ri = s.get("dri", ri)
            all_dri = all_dri and ri != 0
        out[name] = (base, prog, counts, name.startswith("stops_early"),
                     all_dri)
    return out


def clear_unrefined_bit(coefs, al=0):
    """What a script that never refines AC bit `al` leaves: the AC
    coefficients with that bit cleared, toward zero."""
    out = []
    for c in coefs:
        c = c.astype(np.int32)
        cut = np.sign(c) * ((np.abs(c) >> (al + 1)) << (al + 1))
        cut[..., 0] = c[..., 0]
        out.append(cut.astype(np.int16))
    return out


def pillow_pixels(blob):
    a = np.asarray(Image.open(io.BytesIO(blob)))
    return a[..., None] if a.ndim == 2 else a


# ---------------- corruptions of the entropy-coded bytes ----------------

def entropy_base():
    """The (16,24,3) progressive DRI file whose scans are mutated."""
    return pillow_pair((16, 24, 3), "noise", 90, 0, "rst2", seed=6)[1]


def scan_byte_ranges(blob):
    """[begin, end) of the entropy-coded bytes of every scan."""
    info = _core.jpeg_decode_info(blob, progressive="decode")
    return [(s["segments"][0][0], s["segments"][-1][1])
            for s in info["scans"]]


def entropy_mutations(n=32, seed=17):
    """n corruptions confined to the entropy-coded bytes of the scans of
    entropy_base(): three in four flip 1..3 bits inside one scan, the fourth
    cuts a piece out of one scan. Headers, the markers between the scans and
    EOI stay valid."""
    base = entropy_base()
    ranges = scan_byte_ranges(base)
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        b = bytearray(base)
        lo, hi = ranges[rs.randint(0, len(ranges))]
        if i % 4 == 3:
            a = rs.randint(lo, hi)
            e = rs.randint(a, hi) + 1
            del b[a:e]
        else:
            for _ in range(rs.randint(1, 4)):
                b[rs.randint(lo, hi)] ^= 1 << rs.randint(0, 8)
        out.append(bytes(b))
    return out
