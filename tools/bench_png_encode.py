#!/usr/bin/env python3
"""PNG sink A/B: the GPU writer of the "parallel" format against the two host
paths.

_core.png_encode_bench on device-resident 1080p RGB frames, batch 8, each
call ending with the files in host memory:

  gpu           png_encode_gpu + D2H of the files
  cpu-parallel  D2H of the raw frames + png_encode_parallel_cpu (one core)
  zlib          D2H of the raw frames + the zlib writer (the default, and the
                only PNG path on a GPU pipeline without png_writer="parallel")

The sides alternate in one process after a warm-up; each is reported as
seconds per batch, median and spread (min..max) over --reps timed calls (a
GPU call times --gpu-iters batches), for a smooth and a noise clip. Then the
file sizes of three 256x256 RGB frames (gradient, gradient +-3 noise,
constant 77) from all three writers. Prints one JSON line per result and,
with --md, appends markdown tables. Needs a GPU: there is no CPU fallback for
a timing.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scanner_amd import _core  # noqa: E402

MODES = ("gpu", "cpu-parallel", "zlib")


def small_frames():
    yy, xx = np.mgrid[0:256, 0:256]
    grad = np.stack([xx % 256, yy % 256, (xx + yy) % 256], -1).astype(np.uint8)
    noise = np.random.RandomState(0).randint(-3, 4, grad.shape)
    return {"gradient": grad,
            "gradient+-3": np.clip(grad.astype(np.int32) + noise, 0,
                                   255).astype(np.uint8),
            "constant77": np.full((256, 256, 3), 77, np.uint8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--gpu-iters", type=int, default=10,
                    help="batches per timed GPU call")
    ap.add_argument("--modes", default=",".join(MODES),
                    help="comma-separated sides to time")
    ap.add_argument("--md", help="append markdown tables to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    if not _core.have_gpu():
        sys.exit("bench_png_encode needs a GPU")
    h, w, c = 1080, 1920, 3
    _core.init_memory(4 << 30, 8 << 30, [0])
    rows = []
    modes = tuple(args.modes.split(","))
    if not modes or any(m not in MODES for m in modes):
        ap.error("--modes takes " + ", ".join(MODES))
    for clip in ("smooth", "noise"):
        secs = {m: [] for m in modes}
        size = {}
        for m in modes:  # warm-up, every side
            _core.png_encode_bench(h, w, c, args.batch, 1, m, clip)
        for _ in range(args.reps):
            for m in modes:
                iters = args.gpu_iters if m == "gpu" else 1
                s, nbytes = _core.png_encode_bench(h, w, c, args.batch, iters,
                                                   m, clip)
                secs[m].append(s / iters)
                size[m] = nbytes
        for m in modes:
            med = statistics.median(secs[m])
            r = {"shape": f"{h}x{w}x{c}", "clip": clip, "mode": m,
                 "batch": args.batch, "reps": args.reps,
                 "batches_per_rep": args.gpu_iters if m == "gpu" else 1,
                 "seconds": {"median": med, "min": min(secs[m]),
                             "max": max(secs[m])},
                 "frames_per_s": args.batch / med,
                 "bytes_per_frame": size[m] // args.batch,
                 "chunk_bytes": _core.png_chunk_bytes()}
            rows.append(r)
            print(json.dumps(r), flush=True)
    sizes = []
    for name, f in small_frames().items():
        (gpu,) = _core.png_gpu_encode([f])
        r = {"frame": "256x256x3 " + name, "raw": int(f.nbytes),
             "gpu": len(gpu),
             "cpu-parallel": len(_core.png_cpu_encode(f, "parallel")),
             "zlib": len(_core.png_cpu_encode(f, "zlib"))}
        sizes.append(r)
        print(json.dumps(r), flush=True)
    _core.destroy_memory()
    if args.md:
        with open(args.md, "a") as f:
            f.write("| clip | mode | median ms/batch | min..max ms | "
                    "frames/s | bytes/frame |\n|---|---|---|---|---|---|\n")
            for r in rows:
                s = {k: v * 1e3 for k, v in r["seconds"].items()}
                f.write(f"| {r['clip']} | {r['mode']} | {s['median']:.3f} | "
                        f"{s['min']:.3f}..{s['max']:.3f} | "
                        f"{r['frames_per_s']:.1f} | {r['bytes_per_frame']} |\n")
            f.write("\n| frame | raw | gpu | cpu-parallel | zlib |\n"
                    "|---|---|---|---|---|\n")
            for r in sizes:
                f.write(f"| {r['frame']} | {r['raw']} | {r['gpu']} | "
                        f"{r['cpu-parallel']} | {r['zlib']} |\n")


if __name__ == "__main__":
    main()
