#!/usr/bin/env python3
"""Still-image sink A/B: the GPU JPEG encoder against the two host paths.

_core.jpeg_encode_bench on device-resident 1080p RGB frames, quality 90,
batch 8, each call ending with the files in host memory:

  gpu  jpeg_encode_gpu + D2H of the compressed bytes
  cpu  D2H of the raw frames + jpeg_encode_cpu (one core)
  png  D2H of the raw frames + the PNG writer (the only image path before
       the JPEG encoder existed)

The sides alternate in one process after a warm-up; each is reported as
seconds per batch, median and spread (min..max) over --reps timed calls (a
GPU call times --gpu-iters batches), for a smooth and a noise clip.
--subsampling 444|420 selects the JPEG mode of the gpu and cpu sides (png has
none). Prints one JSON line per result and, with --md, appends a markdown
table. Needs a GPU: there is no CPU fallback for a timing.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scanner_amd import _core  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--gpu-iters", type=int, default=200,
                    help="batches per timed GPU call")
    ap.add_argument("--subsampling", choices=("444", "420"), default="444")
    ap.add_argument("--modes", default="gpu,cpu,png",
                    help="comma-separated sides to time")
    ap.add_argument("--md", help="append a markdown table to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    if not _core.have_gpu():
        sys.exit("bench_jpeg_encode needs a GPU")
    h, w, c = 1080, 1920, 3
    _core.init_memory(4 << 30, 8 << 30, [0])
    rows = []
    modes = tuple(args.modes.split(","))
    if not modes or any(m not in ("gpu", "cpu", "png") for m in modes):
        ap.error("--modes takes gpu, cpu and png")
    for clip in ("smooth", "noise"):
        secs = {m: [] for m in modes}
        size = {}
        for m in modes:  # warm-up, every side
            _core.jpeg_encode_bench(h, w, c, args.quality, args.batch, 1, m,
                                    clip, args.subsampling)
        for _ in range(args.reps):
            for m in modes:
                # a GPU batch takes well under a millisecond: time many
                iters = args.gpu_iters if m == "gpu" else 1
                s, nbytes = _core.jpeg_encode_bench(
                    h, w, c, args.quality, args.batch, iters, m, clip,
                    args.subsampling)
                secs[m].append(s / iters)
                size[m] = nbytes
        for m in modes:
            med = statistics.median(secs[m])
            r = {"shape": f"{h}x{w}x{c}", "clip": clip, "mode": m,
                 "quality": args.quality, "batch": args.batch,
                 "reps": args.reps,
                 "batches_per_rep": args.gpu_iters if m == "gpu" else 1,
                 "seconds": {"median": med, "min": min(secs[m]),
                             "max": max(secs[m])},
                 "frames_per_s": args.batch / med,
                 "bytes_per_frame": size[m] // args.batch,
                 "subsampling": args.subsampling,
                 "restart_interval":
                     _core.jpeg_restart_interval(args.subsampling)}
            rows.append(r)
            print(json.dumps(r), flush=True)
    _core.destroy_memory()
    if args.md:
        with open(args.md, "a") as f:
            f.write("| clip | mode | subsampling | median ms/batch | "
                    "min..max ms | frames/s | bytes/frame |\n"
                    "|---|---|---|---|---|---|---|\n")
            for r in rows:
                s = {k: v * 1e3 for k, v in r["seconds"].items()}
                f.write(f"| {r['clip']} | {r['mode']} | {r['subsampling']} | "
                        f"{s['median']:.3f} | "
                        f"{s['min']:.3f}..{s['max']:.3f} | "
                        f"{r['frames_per_s']:.1f} | {r['bytes_per_frame']} |\n")


if __name__ == "__main__":
    main()
