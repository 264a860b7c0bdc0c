"""Memory safety of the self-synchronising JPEG decoder on corrupt input: the
CPU model (jpeg_sync_cpu.cpp) and the serial decoder — and with them
jpeg_sync_common.h, the header kernels/jpeg_sync_decode.hip compiles for the
GPU — built with plain g++ -fsanitize=address,undefined into
tests/cpp/asan_jpeg_sync.cpp and run as a subprocess over fixed-seed
mutations of three seed files without restart markers, at 4- and 64-byte
chunks. The corrupt files that test_jpeg_sync_gpu.py gives to the HIP
decoder (nodri_mutations) go through the same binary first."""
import hashlib
import os
import subprocess
import tempfile

import pytest

from test_image_decode_fuzz import _frame, _save
from test_jpeg_sync_cpu import nodri_mutations

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 400


def seed_files():
    return {
        "420.jpg": _save(_frame(41, 57, 3, 2), "JPEG", quality=70,
                         subsampling=2),
        "grey.jpg": _save(_frame(33, 50, 1, 3), "JPEG", quality=90),
        "optimised_422.jpg": _save(_frame(40, 56, 3, 4), "JPEG", quality=60,
                                   subsampling=1, optimize=True),
    }


def build_asan_binary():
    src = os.path.join(REPO, "tests", "cpp", "asan_jpeg_sync.cpp")
    ops = os.path.join(REPO, "scanner_amd", "csrc", "ops")
    # png_decode.cpp only completes the link: image_decode_cpu names it
    tus = [os.path.join(ops, f) for f in (
        "jpeg_sync_cpu.cpp", "jpeg_decode_cpu.cpp", "png_decode.cpp")]
    headers = [os.path.join(ops, f) for f in (
        "image_decode.h", "jpeg_sync_common.h", "jpeg_decode_common.h",
        "jpeg_common.h")]
    headers.append(os.path.join(REPO, "scanner_amd", "csrc", "common.h"))
    h = hashlib.sha256()
    for f in [src] + tus + headers:
        with open(f, "rb") as fh:
            h.update(fh.read())
    binp = os.path.join(tempfile.gettempdir(),
                        f"sca_asan_jpeg_sync_{h.hexdigest()[:16]}")
    if not os.path.exists(binp):
        r = subprocess.run(
            ["g++", "-O1", "-g", "-std=c++17",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
             src, *tus, "-lz", "-o", binp],
            capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            pytest.fail(f"asan build failed:\n{r.stderr[-2000:]}")
    return binp


def test_asan_jpeg_sync_fuzz(tmp_path):
    binp = build_asan_binary()
    seeds = []
    for name, blob in seed_files().items():
        p = tmp_path / name
        p.write_bytes(blob)
        seeds.append(str(p))
    exact = []
    for i, blob in enumerate(nodri_mutations()):
        p = tmp_path / f"mut{i}.jpg"
        p.write_bytes(blob)
        exact.append(str(p))
    r = subprocess.run([binp, str(ITERS), *seeds, "--exact", *exact],
                       capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"fuzz binary rc={r.returncode}:\n{out[-3000:]}"
    assert "AddressSanitizer" not in out, out[-3000:]
    assert "runtime error" not in out, out[-3000:]
    assert "MISMATCH" not in out, out[-3000:]
    assert "asan jpeg sync fuzz: OK" in out
    # every seed file exercises all three outcomes: the model's own pixels,
    # a fallback that decodes, a fallback that raises
    lines = [ln for ln in out.splitlines() if " iters, " in ln]
    assert len(lines) == len(seeds)
    for ln in lines:
        counts = dict(zip(("equal", "fallback", "raised", "unparsed"),
                          (int(part.split()[0]) for part in
                           ln.split(" iters, ")[1].split(", "))))
        assert counts["equal"] > 0 and counts["fallback"] > 0 and \
            counts["raised"] > 0, ln
        # two chunk sizes per parsed file
        assert counts["equal"] + counts["fallback"] + counts["raised"] == \
            2 * (ITERS - counts["unparsed"]), ln
    tail = next(ln for ln in out.splitlines() if ln.startswith("exact: "))
    assert tail.startswith("exact: 32 files"), tail
