"""Memory safety of the progressive JPEG decoder on corrupt input: the parse
and CPU-decode translation unit — and with it jpeg_progressive_common.h, the
header kernels/jpeg_progressive_decode.hip compiles for the GPU — built with
plain g++ -fsanitize=address,undefined into
tests/cpp/asan_jpeg_progressive.cpp and run as a child process over
fixed-seed mutations of five seed files. The corrupt files that
test_jpeg_progressive_gpu.py gives to the HIP decoder
(jpeg_progressive_cases.entropy_mutations) go through the same binary
first."""
import hashlib
import os
import subprocess
import tempfile

import pytest

import jpeg_progressive_cases as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 1200


def seed_files():
    return {
        "444_nodri.jpg": pc.pillow_pair((40, 56, 3), "noise", 85, 0)[1],
        "444_dri.jpg": pc.pillow_pair((40, 56, 3), "smooth", 85, 0,
                                      "rst2")[1],
        "grey.jpg": pc.pillow_pair((33, 50, 1), "noise", 90, 0, "rst2")[1],
        "420.jpg": pc.pillow_pair((41, 57, 3), "noise", 70, 2, "rows1")[1],
        "writer_dri_changes.jpg": pc.writer_cases()["dri_changes_420"][1],
    }


def build_asan_binary():
    src = os.path.join(REPO, "tests", "cpp", "asan_jpeg_progressive.cpp")
    ops = os.path.join(REPO, "scanner_amd", "csrc", "ops")
    # png_decode.cpp only for the link: image_decode_cpu dispatches to it
    tus = [os.path.join(ops, f) for f in ("jpeg_decode_cpu.cpp",
                                          "png_decode.cpp")]
    headers = [os.path.join(ops, f) for f in (
        "image_decode.h", "jpeg_decode_common.h", "jpeg_progressive_common.h",
        "jpeg_common.h")]
    headers.append(os.path.join(REPO, "scanner_amd", "csrc", "common.h"))
    h = hashlib.sha256()
    for f in [src] + tus + headers:
        with open(f, "rb") as fh:
            h.update(fh.read())
    binp = os.path.join(tempfile.gettempdir(),
                        f"sca_asan_jpeg_prog_{h.hexdigest()[:16]}")
    if not os.path.exists(binp):
        r = subprocess.run(
            ["g++", "-O1", "-g", "-std=c++17",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
             src, *tus, "-lz", "-o", binp],
            capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            pytest.fail(f"asan build failed:\n{r.stderr[-2000:]}")
    return binp


def test_asan_jpeg_progressive_fuzz(tmp_path):
    binp = build_asan_binary()
    seeds = []
    for name, blob in seed_files().items():
        p = tmp_path / name
        p.write_bytes(blob)
        seeds.append(str(p))
    exact = []
    for i, blob in enumerate(pc.entropy_mutations()):
        p = tmp_path / f"mut{i}.jpg"
        p.write_bytes(blob)
        exact.append(str(p))
    assert len(exact) == 32
    r = subprocess.run([binp, str(ITERS), *seeds, "--exact", *exact],
                       capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"fuzz binary rc={r.returncode}:\n{out[-3000:]}"
    assert "AddressSanitizer" not in out, out[-3000:]
    assert "runtime error" not in out, out[-3000:]
    assert "asan jpeg progressive fuzz: OK" in out
    # the fuzz exercises both outcomes for every seed file
    lines = [ln for ln in out.splitlines() if " iters, " in ln]
    assert len(lines) == len(seeds)
    for ln in lines:
        decoded = int(ln.split(" iters, ")[1].split(" decoded")[0])
        assert 0 < decoded < ITERS, ln
    # and the exact files hold both outcomes as well
    line = next(ln for ln in out.splitlines() if ln.startswith("exact: "))
    assert line.startswith("exact: 32 files, ")
    assert 0 < int(line.split("files, ")[1].split(" decoded")[0]) < 32, line
