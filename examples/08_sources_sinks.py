"""Tutorial 08: user sources and sinks.

Jobs don't have to start or end at database tables: a registered Source
feeds the graph rows from anywhere (here: one row per file in a
directory), and a registered Sink writes results anywhere (here: one file
per output row). Both are C++ classes behind SCA_REGISTER_SOURCE/SINK
(csrc/ops/source.h — parity: scanner/api/source.h, sink.h,
enumerator.h); `Files` ships built in.
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import scanner_amd as sp

tmp = tempfile.mkdtemp(prefix="scanner_tut08_")
sc = sp.Client(db_path=os.path.join(tmp, "db"))

# a directory of blobs to process
in_dir = os.path.join(tmp, "in")
os.makedirs(in_dir)
paths = []
for i in range(6):
    p = os.path.join(in_dir, f"doc{i}.txt")
    with open(p, "w") as f:
        f.write(f"document {i} " * (i + 1))
    paths.append(p)

# Files source -> op -> Files sink: no table anywhere
col = sc.sources.Files(paths)
doubled = sc.ops.ConcatBytes(inputs=[col, col])
out_dir = os.path.join(tmp, "out")
os.makedirs(out_dir)
sink = sc.sinks.Files(doubled, out_dir, ext="txt")
sc.run(sink, sp.PerfParams.manual(2, 4),
       cache_mode=sp.CacheMode.Overwrite)

written = sorted(os.listdir(out_dir))
print(f"wrote {len(written)} files:", written)
assert len(written) == 6
body = open(os.path.join(out_dir, "c0_2.txt")).read()
assert body == "document 2 " * 3 * 2

# The most common sink of all: every frame of a video as a .jpg file.
# ImageEncoder(format="jpg") has a CPU and a GPU kernel with identical
# bytes; on the GPU the frames are resized and encoded on the device and
# only the compressed files cross the host link.
import numpy as np

from scanner_amd import _core

yy, xx = np.mgrid[0:96, 0:128]
frames = np.stack([np.stack([(xx + 4 * i) % 256, (yy + 2 * i) % 256,
                             (xx + yy) // 2 % 256], -1).astype(np.uint8)
                   for i in range(8)])
video = sp.NamedVideoStream(sc, "tut08_video", frames=frames, codec="svc")
gpu = _core.have_gpu()
dev = sp.DeviceType.GPU if gpu else sp.DeviceType.CPU
frame = sc.io.Input([video])
thumb = sc.ops.Resize(frame=frame, width=64, height=48, device=dev)
jpg = sc.ops.ImageEncoder(frame=thumb, format="jpg", quality=85, device=dev)
jpg_dir = os.path.join(tmp, "thumbs")
os.makedirs(jpg_dir)
sc.run(sc.sinks.Files(jpg, jpg_dir, ext="jpg"), sp.PerfParams.manual(4, 8),
       cache_mode=sp.CacheMode.Overwrite, **({"gpu_ids": [0]} if gpu else {}))
thumbs = sorted(os.listdir(jpg_dir))
assert len(thumbs) == 8
first = open(os.path.join(jpg_dir, "c0_0.jpg"), "rb").read()
assert first[:2] == b"\xff\xd8" and first[-2:] == b"\xff\xd9"  # SOI .. EOI
print(f"wrote {len(thumbs)} thumbnails on the {'GPU' if gpu else 'CPU'}, "
      f"{len(first)} bytes each or so")
print("sources/sinks OK")
