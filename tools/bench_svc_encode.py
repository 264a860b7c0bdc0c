#!/usr/bin/env python3
"""A/B of the sink-side SVC encode: GPU encoder vs the host path.

Two measurements, both alternating the two sides in one process after a
warm-up, each reported as median and spread (min..max) over --reps runs:

  kernel   _core.svc_encode_bench on device-resident clips (1080p x 32 and
           4K x 16; a smooth and a noise clip, seeded). "gpu" is
           svc_encode_gpu including the D2H of the compressed bytes, "cpu"
           is the host sink path: raw D2H + svc_encode_cpu. Reported as
           frames/s and bytes/s of raw input.
  pipeline decode -> GPU Blur -> svc-compressed output at 1080p, 40 frames,
           one task in packets of 5, end to end with
           SCANNER_SVC_GPU_ENCODE=0 and =1 (same build, identical bytes).

Prints one JSON line per result and, with --md, appends a markdown table.
Needs a GPU: there is no CPU fallback for a timing.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import scanner_amd as sp  # noqa: E402
from scanner_amd import _core  # noqa: E402


def summarize(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def bench_kernel(reps, rows):
    _core.init_memory(4 << 30, 8 << 30, [0])
    for label, (h, w, n) in (("1080p x32", (1080, 1920, 32)),
                             ("4K x16", (2160, 3840, 16))):
        for clip in ("smooth", "noise"):
            raw = h * w * 3 * n
            secs = {"gpu": [], "cpu": []}
            for mode in ("gpu", "cpu"):  # warm-up, both sides
                _core.svc_encode_bench(h, w, 3, n, 1, mode, clip, 7)
            for _ in range(reps):
                for mode in ("gpu", "cpu"):
                    secs[mode].append(
                        _core.svc_encode_bench(h, w, 3, n, 1, mode, clip, 7))
            for mode in ("gpu", "cpu"):
                s = summarize(secs[mode])
                r = {"bench": "kernel", "shape": label, "clip": clip,
                     "mode": mode, "reps": reps, "seconds": s,
                     "frames_per_s": n / s["median"],
                     "raw_GB_per_s": raw / s["median"] / 1e9}
                rows.append(r)
                print(json.dumps(r), flush=True)
    _core.destroy_memory()


def smooth_clip(n, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.zeros((n, h, w, 3), np.uint8)
    for i in range(n):
        f[i, :, :, 0] = (xx + i * 2) % 256
        f[i, :, :, 1] = (yy + i) % 256
        f[i, :, :, 2] = (xx + yy + i * 3) % 256
    return f


def bench_pipeline(reps, rows, n=40, h=1080, w=1920):
    frames = smooth_clip(n, h, w)
    with tempfile.TemporaryDirectory() as tmp:
        sc = sp.Client(db_path=os.path.join(tmp, "db"))
        video = sp.NamedVideoStream(sc, "benc_in", frames=frames, codec="svc")
        results = {}

        def run(switch):
            os.environ["SCANNER_SVC_GPU_ENCODE"] = switch
            frame = sc.io.Input([video])
            blur = sc.ops.Blur(frame=frame, kernel_size=3,
                               device=sp.DeviceType.GPU)
            blur.compress_video()
            out = sp.NamedStream(sc, "benc_out" + switch)
            t0 = time.perf_counter()
            prof = sc.run(sc.io.Output(blur, [out]),
                          sp.PerfParams.manual(5, n, cpu_pool=4 << 30,
                                               gpu_pool=8 << 30),
                          cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
            dt = time.perf_counter() - t0
            results[switch] = prof.counters()
            return dt

        secs = {"0": [], "1": []}
        for switch in ("0", "1"):
            run(switch)
        for _ in range(reps):
            for switch in ("0", "1"):
                secs[switch].append(run(switch))
        a = np.stack(list(sp.NamedVideoStream(sc, "benc_out0").load()))
        b = np.stack(list(sp.NamedVideoStream(sc, "benc_out1").load()))
        assert np.array_equal(a, b), "the two sink paths disagree"
        for switch in ("0", "1"):
            s = summarize(secs[switch])
            c = results[switch]
            r = {"bench": "pipeline", "shape": f"{h}x{w} x{n}",
                 "switch": switch, "reps": reps, "seconds": s,
                 "frames_per_s": n / s["median"],
                 "raw_GB_per_s": n * h * w * 3 / s["median"] / 1e9,
                 "sink_d2h_bytes": c.get("sink_d2h_bytes", 0),
                 "io_write_bytes": c.get("io_write_bytes", 0),
                 "svc_gpu_encode_frames": c.get("svc_gpu_encode_frames", 0)}
            rows.append(r)
            print(json.dumps(r), flush=True)


def write_md(path, rows):
    with open(path, "a") as f:
        f.write("| bench | shape | clip/switch | median s | min..max s | "
                "frames/s | raw GB/s |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            side = (f"{r['clip']} {r['mode']}" if r["bench"] == "kernel"
                    else f"switch={r['switch']}")
            s = r["seconds"]
            f.write(f"| {r['bench']} | {r['shape']} | {side} | "
                    f"{s['median']:.4f} | {s['min']:.4f}..{s['max']:.4f} | "
                    f"{r['frames_per_s']:.1f} | {r['raw_GB_per_s']:.2f} |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["kernel", "pipeline"])
    ap.add_argument("--md", help="append a markdown table to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be >= 5")
    if not _core.have_gpu():
        sys.exit("bench_svc_encode needs a GPU")
    rows = []
    if args.only in (None, "kernel"):
        bench_kernel(args.reps, rows)
    if args.only in (None, "pipeline"):
        bench_pipeline(args.reps, rows)
    if args.md:
        write_md(args.md, rows)


if __name__ == "__main__":
    main()
