#!/usr/bin/env python3
"""Measurements of the Motion-JPEG codec on a GPU (profiles/mjpeg.md).

  decode    the device-side index path (mjpeg_decode_gpu_dev, stream resident
            in HBM) against jpeg_parse on the host + jpeg_decode_gpu, and the
            index kernel alone
  pipeline  Input -> Histogram(GPU) over an mjpeg table against the same
            clip as SVC
  sink      Blur(GPU) -> compress_video(codec="mjpeg") with the GPU sink
            against the host sink (SCANNER_MJPEG_GPU=0)
  bytes     bytes per frame against SVC

The two sides of each comparison alternate in this one process, after a
warm-up; every timed window ends on a synchronise. Prints one JSON line per
measurement.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import numpy as np

import scanner_amd as sp
from scanner_amd import _core


def clip(kind, n, h, w):
    if kind == "noise":
        return np.random.RandomState(0).randint(0, 256, (n, h, w, 3)).astype(
            np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([np.stack([(xx + 4 * i) % 256, (yy + 2 * i) % 256,
                               (xx + yy + 3 * i) // 2 % 256], -1)
                     for i in range(n)]).astype(np.uint8)


def summary(xs):
    return {"median_ms": round(1e3 * statistics.median(xs), 3),
            "min_ms": round(1e3 * min(xs), 3),
            "max_ms": round(1e3 * max(xs), 3), "windows": len(xs)}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--subsampling", default="420")
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", default="smooth,noise")
    ap.add_argument("--skip", default="", help="comma list of sections")
    args = ap.parse_args()
    assert _core.have_gpu(), "bench_mjpeg.py needs a GPU"
    skip = set(args.skip.split(","))
    n, h, w = args.frames, args.height, args.width
    tmp = tempfile.mkdtemp(prefix="bench_mjpeg_")
    sc = sp.Client(db_path=os.path.join(tmp, "db"))

    for kind in args.clips.split(","):
        fr = clip(kind, n, h, w)
        samples = [_core.jpeg_cpu_encode(f, args.quality, args.subsampling)
                   for f in fr]
        stream = b"".join(samples)
        sizes = [len(s) for s in samples]
        offs = [sum(sizes[:i]) for i in range(n)]
        if "decode" not in skip:
            t = _core.mjpeg_decode_bench(stream, offs, sizes, h, w, 3,
                                         args.windows, args.warmup)
            for mode in ("index", "host", "index_kernel"):
                emit(section="decode", clip=kind, mode=mode, frames=n,
                     **summary(t[mode]))
        mj = sp.NamedVideoStream(sc, f"mj_{kind}", frames=fr, codec="mjpeg",
                                 quality=args.quality,
                                 subsampling=args.subsampling)
        svc = sp.NamedVideoStream(sc, f"svc_{kind}", frames=fr, codec="svc")
        if "bytes" not in skip:
            info = sc._db.table_info(f"svc_{kind}")
            svc_bytes = sum(
                len(_core.read_video_item(sc._db, f"svc_{kind}", "frame",
                                          i)[0])
                for i in range(len(info["end_rows"])))
            emit(section="bytes", clip=kind, raw=h * w * 3,
                 mjpeg_per_frame=len(stream) // n,
                 svc_per_frame=svc_bytes // n)

        def hist(video, name):
            frame = sc.io.Input([video])
            col = sc.ops.Histogram(frame=frame, device=sp.DeviceType.GPU)
            out = sp.NamedStream(sc, name)
            t0 = time.perf_counter()
            sc.run(sc.io.Output([col], [out]), sp.PerfParams.manual(8, 16),
                   cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
            return time.perf_counter() - t0

        if "pipeline" not in skip:
            t = {"mjpeg": [], "svc": []}
            for it in range(args.windows + args.warmup):
                a = hist(mj, "h_mj")
                b = hist(svc, "h_svc")
                if it >= args.warmup:
                    t["mjpeg"].append(a)
                    t["svc"].append(b)
            for mode in t:
                emit(section="pipeline", clip=kind, mode=mode, frames=n,
                     **summary(t[mode]))

        def sink(switch, name):
            os.environ["SCANNER_MJPEG_GPU"] = switch
            frame = sc.io.Input([svc])
            col = sc.ops.Blur(frame=frame, kernel_size=3,
                              device=sp.DeviceType.GPU)
            col.compress_video(codec="mjpeg", quality=args.quality,
                               subsampling=args.subsampling)
            out = sp.NamedStream(sc, name)
            t0 = time.perf_counter()
            sc.run(sc.io.Output(col, [out]), sp.PerfParams.manual(8, 16),
                   cache_mode=sp.CacheMode.Overwrite, gpu_ids=[0])
            os.environ.pop("SCANNER_MJPEG_GPU")
            return time.perf_counter() - t0

        if "sink" not in skip:
            t = {"gpu_sink": [], "host_sink": []}
            for it in range(args.windows + args.warmup):
                a = sink("1", "s_gpu")
                b = sink("0", "s_host")
                if it >= args.warmup:
                    t["gpu_sink"].append(a)
                    t["host_sink"].append(b)
            for mode in t:
                emit(section="sink", clip=kind, mode=mode, frames=n,
                     **summary(t[mode]))


if __name__ == "__main__":
    main()
