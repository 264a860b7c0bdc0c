#!/usr/bin/env python3
"""Still-image source A/B: the GPU JPEG decoder against the host paths.

_core.jpeg_decode_bench on batches of 8 1080p files in host memory, each
timed call ending with the decoded frames resident in HBM:

  gpu     jpeg_parse + jpeg_decode_gpu (compressed H2D inside); files
          without restart markers are decoded on the host inside the call
          (serial_scan="host", the default)
  gpu_sync, gpu_sync_<bytes>
          the same call with serial_scan="device": the self-synchronising
          decoder at the default chunk size, and at 32, 64, 128 and 256
          bytes (only for the files without restart markers)
  cpu     jpeg_decode_cpu on one core + H2D of the raw frames (the same
          pixels as the gpu side)
  pillow  Pillow decode + H2D of the raw frames (informational: a different
          decoder)

Files: our encoder at quality 90 ("smooth" and "noise", restart interval 32),
Pillow 4:2:0 with a restart marker per MCU row, and "pillow420_plain": Pillow
4:2:0 without restart markers, smooth and noise. For the latter the CPU
model's chunk, group and round counts of the first file and the rows that
fell back in one call are reported with each gpu_sync side. The sides
alternate in
one process after a warm-up; each is reported as seconds per batch, median
and spread (min..max) over --reps timed calls. Prints one JSON line per
result and, with --md, appends a markdown table. Needs a GPU: there is no
CPU fallback for a timing.

--progressive measures the progressive decoder instead, on Pillow 4:2:0 files
of the same images, smooth and noise, saved four ways (baseline or
progressive, a restart marker per MCU row or none):

  base_rows1/gpu         baseline, device decode: the yardstick
  prog_rows1/gpu_prog    progressive="decode", every scan on the device, one
                         lane per restart segment
  prog_plain/gpu_prog_serial   progressive without restart markers under
                         serial_scan="device": one lane per scan
  prog_plain/gpu_prog_host     the same files with the default serial_scan:
                         decoded on the host inside the call
  base_plain/gpu         baseline without restart markers, host path, for
                         scale
A build without the progressive option (an older commit) runs the baseline
sides alone, which is how the baseline sides of two commits are compared.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scanner_amd import _core  # noqa: E402


def frames(clip, n, h=1080, w=1920):
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        if clip == "noise":
            f = np.random.RandomState(i).randint(0, 256, (h, w, 3))
        else:
            f = np.stack([(xx + 2 * i) % 256, (yy + i) % 256,
                          ((xx + yy) // 2 + 3 * i) % 256], -1)
        out.append(np.ascontiguousarray(f.astype(np.uint8)))
    return out


def pillow_side(blobs):
    from PIL import Image
    t0 = time.perf_counter()
    raw = [np.asarray(Image.open(io.BytesIO(b))).tobytes() for b in blobs]
    dt = time.perf_counter() - t0
    return dt + _core.jpeg_decode_bench(raw, 1, "upload")[0]


def progressive_main(args):
    """The --progressive sides; see the module docstring."""
    from PIL import Image
    have_prog = "progressive" in (_core.jpeg_decode_bench.__doc__ or "")
    _core.init_memory(4 << 30, 8 << 30, [0])

    def save(f, **kw):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=args.quality,
                                subsampling=2, **kw)
        return buf.getvalue()

    rows = []
    for clip in ("smooth", "noise"):
        fr = frames(clip, args.batch)
        sides = [("base_rows1", "gpu", [save(f, restart_marker_rows=1)
                                        for f in fr], {}),
                 ("base_plain", "gpu", [save(f) for f in fr], {})]
        if have_prog:
            rows1 = [save(f, progressive=True, restart_marker_rows=1)
                     for f in fr]
            plain = [save(f, progressive=True) for f in fr]
            dec = dict(progressive="decode")
            sides += [("prog_rows1", "gpu_prog", rows1, dec),
                      ("prog_plain", "gpu_prog_serial", plain,
                       dict(dec, serial_scan="device")),
                      ("prog_plain", "gpu_prog_host", plain, dec)]
        secs = [[] for _ in sides]
        for _, _, blobs, kw in sides:  # warm-up, every side
            _core.jpeg_decode_bench(blobs, 1, "gpu", **kw)
        for _ in range(args.reps):  # the sides alternate
            for k, (_, _, blobs, kw) in enumerate(sides):
                secs[k].append(_core.jpeg_decode_bench(blobs, 1, "gpu",
                                                       **kw)[0])
        for k, (files, mode, blobs, kw) in enumerate(sides):
            med = statistics.median(secs[k])
            r = {"files": f"{files}_{clip}", "mode": mode,
                 "batch": args.batch, "reps": args.reps,
                 "quality": args.quality,
                 "bytes_per_file": sum(map(len, blobs)) // len(blobs),
                 "seconds": {"median": med, "min": min(secs[k]),
                             "max": max(secs[k])},
                 "frames_per_s": args.batch / med}
            if kw:
                frames_, host_rows, st = _core.jpeg_gpu_decode(
                    blobs, host_rows=True, stats=True, **kw)
                r["host_rows"] = host_rows
                r["progressive_rows"] = st["progressive_rows"]
                info = _core.jpeg_decode_info(blobs[0], progressive="decode")
                r["scans"] = len(info["scans"])
                r["segments_per_file"] = sum(s["segment_count"]
                                             for s in info["scans"])
            rows.append(r)
            print(json.dumps(r), flush=True)
    _core.destroy_memory()
    if args.md:
        with open(args.md, "a") as f:
            f.write("| files | side | median ms/batch | min..max ms | "
                    "frames/s | bytes/file | scans | segments/file | host "
                    "rows |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                s = {k: v * 1e3 for k, v in r["seconds"].items()}
                f.write(f"| {r['files']} | {r['mode']} | {s['median']:.3f} | "
                        f"{s['min']:.3f}..{s['max']:.3f} | "
                        f"{r['frames_per_s']:.1f} | {r['bytes_per_file']} | "
                        f"{r.get('scans', '')} | "
                        f"{r.get('segments_per_file', '')} | "
                        f"{r.get('host_rows', '')} |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--progressive", action="store_true",
                    help="measure the progressive decoder (see above)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--md", help="append a markdown table to this file")
    ap.add_argument("--sets", help="comma-separated file sets to run "
                    "(default: all)")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    if not _core.have_gpu():
        sys.exit("bench_jpeg_decode needs a GPU")
    if args.progressive:
        return progressive_main(args)
    from PIL import Image
    _core.init_memory(4 << 30, 8 << 30, [0])
    sets = {}
    for clip in ("smooth", "noise"):
        sets["ours_" + clip] = [_core.jpeg_cpu_encode(f, args.quality)
                                for f in frames(clip, args.batch)]
    pil = []
    for f in frames("smooth", args.batch):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=args.quality,
                                subsampling=2, restart_marker_rows=1)
        pil.append(buf.getvalue())
    sets["pillow420_rows1_smooth"] = pil
    for clip in ("smooth", "noise"):
        plain = []
        for f in frames(clip, args.batch):
            buf = io.BytesIO()
            Image.fromarray(f).save(buf, "JPEG", quality=args.quality,
                                    subsampling=2)
            plain.append(buf.getvalue())
        sets["pillow420_plain_" + clip] = plain
    if args.sets:
        sets = {k: sets[k] for k in args.sets.split(",")}

    rows = []
    sync = {}  # per gpu mode: seconds waited in the call's synchronise
    sync_chunks = {"gpu_sync": 0, "gpu_sync_32": 32, "gpu_sync_64": 64,
                   "gpu_sync_128": 128, "gpu_sync_256": 256}

    def run(mode, blobs):
        if mode == "pillow":
            return pillow_side(blobs)
        if mode in sync_chunks:
            s = _core.jpeg_decode_bench(blobs, 1, "gpu", serial_scan="device",
                                        chunk_bytes=sync_chunks[mode])[0]
        else:
            s = _core.jpeg_decode_bench(blobs, 1, mode)[0]
        if mode.startswith("gpu"):
            sync[mode].append(_core.jpeg_decode_last_sync_seconds())
        return s

    for name, blobs in sets.items():
        plain = _core.jpeg_decode_info(blobs[0])["restart_interval"] == 0
        modes = ("gpu",) + (tuple(sync_chunks) if plain else ()) + \
            ("cpu", "pillow")
        secs = {m: [] for m in modes}
        sync.clear()
        sync.update({m: [] for m in modes})
        for m in modes:  # warm-up, every side
            run(m, blobs)
        for _ in range(args.reps):
            for m in modes:
                secs[m].append(run(m, blobs))
        info = _core.jpeg_decode_info(blobs[0])
        for m in modes:
            med = statistics.median(secs[m])
            r = {"files": name, "mode": m, "batch": args.batch,
                 "reps": args.reps, "quality": args.quality,
                 "segments_per_file": len(info["segments"]),
                 "bytes_per_file": sum(map(len, blobs)) // len(blobs),
                 "seconds": {"median": med, "min": min(secs[m]),
                             "max": max(secs[m])},
                 "frames_per_s": args.batch / med}
            if sync[m]:  # warm-up call included; the median ignores it
                r["sync_wait_seconds_median"] = statistics.median(sync[m])
            if m in sync_chunks:
                st = _core.jpeg_sync_model(blobs[0], sync_chunks[m])[1]
                r["chunk_bytes"] = sync_chunks[m] or \
                    _core.jpeg_sync_chunk_bytes()
                r["model_first_file"] = {
                    k: st[k] for k in ("chunks", "groups", "group_iterations",
                                       "cross_rounds", "cross_repairs")}
                r["fallback_rows"] = _core.jpeg_gpu_decode(
                    blobs, serial_scan="device", chunk_bytes=sync_chunks[m],
                    stats=True)[1]["fallback_rows"]
            rows.append(r)
            print(json.dumps(r), flush=True)
    _core.destroy_memory()
    if args.md:
        with open(args.md, "a") as f:
            f.write("| files | side | median ms/batch | min..max ms | frames/s "
                    "| segments/file | bytes/file | sync wait ms | chunks, "
                    "groups, in-group iterations, rounds used (first file) "
                    "| fallback rows |\n"
                    "|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                s = {k: v * 1e3 for k, v in r["seconds"].items()}
                f.write(f"| {r['files']} | {r['mode']} | {s['median']:.3f} | "
                        f"{s['min']:.3f}..{s['max']:.3f} | "
                        f"{r['frames_per_s']:.1f} | {r['segments_per_file']} "
                        f"| {r['bytes_per_file']} | "
                        + (f"{r['sync_wait_seconds_median'] * 1e3:.3f}"
                           if "sync_wait_seconds_median" in r else "")
                        + " | "
                        + (", ".join(str(r["model_first_file"][k]) for k in (
                            "chunks", "groups", "group_iterations",
                            "cross_rounds")) + f" | {r['fallback_rows']}"
                           if "model_first_file" in r else " | ")
                        + " |\n")


if __name__ == "__main__":
    main()
