"""Memory safety of the Motion-JPEG host code on corrupt input, and the
index's agreement with jpeg_parse on it: tests/cpp/asan_mjpeg.cpp, a
stand-alone program built with plain g++ -fsanitize=address,undefined, runs
a fixed-seed mutation pass over mjpeg_index_ref (the rule the HIP kernel
shares, csrc/video/mjpeg_common.h) and over mp4_parse on Motion-JPEG files.
Nothing here runs on a GPU or inside Python."""
import hashlib
import os
import subprocess
import tempfile

import pytest

import mjpeg_cases as mc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 2000


def build_asan_binary():
    src = os.path.join(REPO, "tests", "cpp", "asan_mjpeg.cpp")
    csrc = os.path.join(REPO, "scanner_amd", "csrc")
    tus = [os.path.join(csrc, "ops", "jpeg_decode_cpu.cpp"),
           os.path.join(csrc, "ops", "png_decode.cpp"),
           os.path.join(csrc, "video", "mp4.cpp"),
           os.path.join(csrc, "video", "h264.cpp")]
    headers = [os.path.join(csrc, *p) for p in (
        ("ops", "image_decode.h"), ("ops", "jpeg_decode_common.h"),
        ("ops", "jpeg_common.h"), ("video", "mjpeg_common.h"),
        ("video", "mp4.h"), ("video", "h264.h"), ("common.h",))]
    h = hashlib.sha256()
    for f in [src] + tus + headers:
        with open(f, "rb") as fh:
            h.update(fh.read())
    binp = os.path.join(tempfile.gettempdir(),
                        f"sca_asan_mjpeg_{h.hexdigest()[:16]}")
    if not os.path.exists(binp):
        r = subprocess.run(
            ["g++", "-O1", "-g", "-std=c++17",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
             src, *tus, "-lz", "-o", binp],
            capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            pytest.fail(f"asan build failed:\n{r.stderr[-2000:]}")
    return binp


def test_asan_mjpeg_fuzz(tmp_path):
    binp = build_asan_binary()
    fr = mc.frames(3, 24, 72, 3, seed=12, noise=48)
    jpegs = {
        "444.jpg": mc.pillow_jpeg(fr[0], quality=90, subsampling=0,
                                  restart_marker_blocks=2),
        "420.jpg": mc.pillow_jpeg(fr[1], quality=75, subsampling=2,
                                  restart_marker_blocks=1),
        "grey.jpg": mc.pillow_jpeg(fr[2][..., :1], quality=95,
                                   restart_marker_rows=1),
    }
    samples = [mc.pillow_jpeg(f, quality=60, subsampling=2) for f in fr]
    mp4s = {
        "jpeg.mov": mc.mux_mp4(samples, 72, 24, entry="jpeg", chunk=2),
        "mp4v.mp4": mc.mux_mp4(samples, 72, 24, entry="mp4v", chunk=1),
    }
    args = []
    for name, blob in jpegs.items():
        (tmp_path / name).write_bytes(blob)
        args.append(str(tmp_path / name))
    args.append("--mp4")
    for name, blob in mp4s.items():
        (tmp_path / name).write_bytes(blob)
        args.append(str(tmp_path / name))
    r = subprocess.run([binp, str(ITERS), *args], capture_output=True,
                       text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"fuzz binary rc={r.returncode}:\n{out[-3000:]}"
    assert "AddressSanitizer" not in out, out[-3000:]
    assert "runtime error" not in out, out[-3000:]
    assert "asan mjpeg fuzz: OK" in out
    # both verdicts occur for every seed, so both branches were checked
    lines = [ln for ln in out.splitlines() if " iters, " in ln]
    assert len(lines) == len(jpegs) + len(mp4s)
    for ln in lines[:len(jpegs)]:
        accepted = int(ln.split(" iters, ")[1].split(" accepted")[0])
        refused = int(ln.split(" accepted, ")[1].split(" refused")[0])
        assert accepted > 0 and refused > 0, ln
    for ln in lines[len(jpegs):]:
        parsed = int(ln.split(" iters, ")[1].split(" parsed")[0])
        assert 0 < parsed < ITERS, ln
