#!/usr/bin/env python3
"""Resize filters, frames per second on device-resident frames.

_core.resize_bench runs ONE Resize kernel object (tables and workspace
cached, as in a pipeline instance) on a batch of resident RGB noise frames;
every call ends with the stream drained and the outputs released. Per shape
and filter it reports the GPU kernels (kernels/resample.hip; "bilinear" is
the older two-tap kernel of image_ops.hip, the only baseline the project has)
and the CPU kernel (one core), as seconds per batch, median and spread
(min..max) over --reps timed calls of --iters (GPU) batches.

It also prints what the two passes of a convolution filter must move
(horizontal: the u8 source in, the i16 intermediate out; vertical: the
intermediate in, the u8 result out) and how long that takes at --hbm-tbs
(default 6.29 TB/s, what a float4 copy reaches of the 8 TB/s peak), next to
the time measured for both passes together; the passes are not timed apart
here.

Prints one JSON line per result and, with --md, appends a markdown table.
Needs a GPU for the gpu side: there is no fallback for a timing.
"""
import argparse
import json
import os
import statistics
import sys

import msgpack

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scanner_amd import _core  # noqa: E402

SHAPES = [((1080, 1920), (360, 640)), ((1080, 1920), (144, 256)),
          ((2160, 3840), (224, 224))]
FILTERS = ["bilinear", "nearest", "box", "triangle", "cubic", "lanczos3"]
CONVOLUTION = ("box", "triangle", "cubic", "lanczos3")


def pass_bytes(src, dst, c):
    """(horizontal, vertical) bytes per frame of a convolution filter."""
    (sh, sw), (dh, dw) = src, dst
    inter = sh * dw * c * 2
    return sh * sw * c + inter, inter + dh * dw * c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20,
                    help="batches per timed GPU call")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--cpu-batch", type=int, default=2,
                    help="frames per timed CPU call (one call per rep)")
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--devices", default="gpu,cpu")
    ap.add_argument("--hbm-tbs", type=float, default=6.29)
    ap.add_argument("--md", help="append a markdown table to this file")
    args = ap.parse_args()
    devices = args.devices.split(",")
    if any(d not in ("gpu", "cpu") for d in devices):
        ap.error("--devices takes gpu and cpu")
    if "gpu" in devices and not _core.have_gpu():
        sys.exit("bench_resize: the gpu side needs a GPU")
    _core.init_memory(4 << 30, 8 << 30, [0] if "gpu" in devices else [])
    c = 3
    rows = []
    for src, dst in SHAPES:
        for flt in FILTERS:
            blob = msgpack.packb({"width": dst[1], "height": dst[0],
                                  "filter": flt})
            for dev in devices:
                gpu = dev == "gpu"
                batch = args.batch if gpu else args.cpu_batch
                iters = args.iters if gpu else 1
                reps = args.reps if gpu else args.cpu_reps
                secs = [_core.resize_bench(1 if gpu else 0, blob, src[0],
                                           src[1], c, batch, iters) / iters
                        for _ in range(reps)]
                med = statistics.median(secs)
                r = {"src": f"{src[0]}x{src[1]}", "dst": f"{dst[0]}x{dst[1]}",
                     "filter": flt, "device": dev, "batch": batch,
                     "reps": reps, "batches_per_rep": iters,
                     "seconds": {"median": med, "min": min(secs),
                                 "max": max(secs)},
                     "frames_per_s": batch / med}
                if gpu and flt in CONVOLUTION:
                    hb, vb = pass_bytes(src, dst, c)
                    rate = args.hbm_tbs * 1e12
                    r["pass_bytes_per_frame"] = {"h": hb, "v": vb}
                    r["hbm_seconds_per_batch"] = {
                        "h": hb * batch / rate, "v": vb * batch / rate}
                    r["times_hbm_floor"] = med / ((hb + vb) * batch / rate)
                rows.append(r)
                print(json.dumps(r), flush=True)
    _core.destroy_memory()
    if args.md:
        with open(args.md, "a") as f:
            f.write("| source | result | filter | device | batch | "
                    "median ms/batch | min..max ms | frames/s | "
                    "H+V MB/frame | HBM floor ms/batch | x floor |\n"
                    "|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                s = {k: v * 1e3 for k, v in r["seconds"].items()}
                if "pass_bytes_per_frame" in r:
                    pb, hs = r["pass_bytes_per_frame"], \
                        r["hbm_seconds_per_batch"]
                    tail = (f"{pb['h'] / 1e6:.2f}+{pb['v'] / 1e6:.2f} | "
                            f"{hs['h'] * 1e3:.3f}+{hs['v'] * 1e3:.3f} | "
                            f"{r['times_hbm_floor']:.1f}")
                else:
                    tail = "| | "
                f.write(f"| {r['src']} | {r['dst']} | {r['filter']} | "
                        f"{r['device']} | {r['batch']} | {s['median']:.3f} | "
                        f"{s['min']:.3f}..{s['max']:.3f} | "
                        f"{r['frames_per_s']:.0f} | {tail} |\n")


if __name__ == "__main__":
    main()
