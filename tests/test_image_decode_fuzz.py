"""Memory safety of the still-image decoders on corrupt input: the parse,
CPU-decode and PNG translation units — and with them jpeg_decode_common.h,
the header kernels/jpeg_decode.hip compiles for the GPU — built with plain
g++ -fsanitize=address,undefined into tests/cpp/asan_image_decode.cpp and
run over fixed-seed mutations of five seed files. The corrupt files that
test_image_decode_gpu.py gives to the HIP decoder (entropy_mutations) go
through the same binary first."""
import hashlib
import io
import os
import subprocess
import tempfile

import numpy as np
import pytest
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(h, w, c, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(3 * xx + yy) % 256, (2 * yy + xx) % 256,
                       (xx * yy // 4) % 256], -1)[..., :c]
    noise = np.random.RandomState(seed).randint(0, 64, (h, w, c))
    return ((smooth + noise) % 256).astype(np.uint8)


def _save(frame, fmt, **kw):
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(
        buf, fmt, **kw)
    return buf.getvalue()


def seed_files():
    return {
        "444_dri.jpg": _save(_frame(40, 56, 3, 1), "JPEG", quality=85,
                             subsampling=0, restart_marker_blocks=4),
        "420_nodri.jpg": _save(_frame(41, 57, 3, 2), "JPEG", quality=70,
                               subsampling=2),
        "grey.jpg": _save(_frame(33, 50, 1, 3), "JPEG", quality=90,
                          restart_marker_blocks=2),
        "optimised.jpg": _save(_frame(40, 56, 3, 4), "JPEG", quality=60,
                               subsampling=1, optimize=True,
                               restart_marker_rows=1),
        "rgb.png": _save(_frame(33, 50, 3, 5), "PNG"),
    }


def entropy_base():
    """The (16,24,3) DRI file whose entropy-coded data is mutated."""
    return _save(_frame(16, 24, 3, 6), "JPEG", quality=90, subsampling=0,
                 restart_marker_blocks=2)


def scan_range(blob):
    """[first entropy-coded byte, EOI marker) of a single-scan JPEG."""
    pos = 2
    while blob[pos + 1] != 0xda:
        pos += 2 + int.from_bytes(blob[pos + 2:pos + 4], "big")
    pos += 2 + int.from_bytes(blob[pos + 2:pos + 4], "big")
    assert blob[-2:] == b"\xff\xd9"
    return pos, len(blob) - 2


def entropy_mutations(n=32, seed=11):
    """n corruptions confined to the entropy-coded data of entropy_base():
    three in four flip 1..3 bits, the fourth cuts a piece out (the header
    and the EOI marker stay valid)."""
    base = entropy_base()
    lo, hi = scan_range(base)
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        b = bytearray(base)
        if i % 4 == 3:
            a = rs.randint(lo, hi)
            e = rs.randint(a, hi) + 1
            del b[a:e]
        else:
            for _ in range(rs.randint(1, 4)):
                b[rs.randint(lo, hi)] ^= 1 << rs.randint(0, 8)
        out.append(bytes(b))
    return out


def build_asan_binary():
    src = os.path.join(REPO, "tests", "cpp", "asan_image_decode.cpp")
    ops = os.path.join(REPO, "scanner_amd", "csrc", "ops")
    tus = [os.path.join(ops, f) for f in ("jpeg_decode_cpu.cpp",
                                          "png_decode.cpp")]
    headers = [os.path.join(ops, f) for f in (
        "image_decode.h", "jpeg_decode_common.h", "jpeg_common.h")]
    headers.append(os.path.join(REPO, "scanner_amd", "csrc", "common.h"))
    h = hashlib.sha256()
    for f in [src] + tus + headers:
        with open(f, "rb") as fh:
            h.update(fh.read())
    binp = os.path.join(tempfile.gettempdir(),
                        f"sca_asan_image_{h.hexdigest()[:16]}")
    if not os.path.exists(binp):
        r = subprocess.run(
            ["g++", "-O1", "-g", "-std=c++17",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
             src, *tus, "-lz", "-o", binp],
            capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            pytest.fail(f"asan build failed:\n{r.stderr[-2000:]}")
    return binp


def test_asan_image_decode_fuzz(tmp_path):
    binp = build_asan_binary()
    seeds = []
    for name, blob in seed_files().items():
        p = tmp_path / name
        p.write_bytes(blob)
        seeds.append(str(p))
    exact = []
    for i, blob in enumerate(entropy_mutations()):
        p = tmp_path / f"mut{i}.jpg"
        p.write_bytes(blob)
        exact.append(str(p))
    r = subprocess.run([binp, "1500", *seeds, "--exact", *exact],
                       capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"fuzz binary rc={r.returncode}:\n{out[-3000:]}"
    assert "AddressSanitizer" not in out, out[-3000:]
    assert "runtime error" not in out, out[-3000:]
    assert "asan image decode fuzz: OK" in out
    # the fuzz exercises both outcomes for every seed file
    lines = [ln for ln in out.splitlines() if " iters, " in ln]
    assert len(lines) == len(seeds)
    for ln in lines:
        decoded = int(ln.split(" iters, ")[1].split(" decoded")[0])
        assert decoded < 1500, ln
        # a PNG's CRCs reject nearly every mutation; a JPEG has no checksum
        assert decoded > 0 or ".png:" in ln, ln
    assert "exact: 32 files" in out
