"""Tutorial 12: Motion-JPEG, the lossy video codec and the way to mp4.

codec="mjpeg" stores one JPEG file per frame: every frame is a keyframe, so
a strided or gathered sample decodes only the frames it asks for, and the
table is a standard video as soon as it is wrapped in mp4. The chain here:

  frames -> mjpeg table -> Histogram
         -> compress_video(codec="mjpeg") -> save_mp4 -> re-ingest

On a GPU the compressed samples stay in HBM; a kernel finds every frame's
restart segments there and the JPEG decode kernels read them in place
(docs/codec.md, "Motion-JPEG"). The sink encodes on the device too.
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np

import scanner_amd as sp
from scanner_amd import _core

tmp = tempfile.mkdtemp(prefix="scanner_tut12_")
sc = sp.Client(db_path=os.path.join(tmp, "db"))
gpu = _core.have_gpu()
dev = sp.DeviceType.GPU if gpu else sp.DeviceType.CPU
run_kw = {"gpu_ids": [0]} if gpu else {}

# ---- ingest: quality and subsampling are the encoder's ----
yy, xx = np.mgrid[0:96, 0:128]
frames = np.stack([np.stack([(xx + 4 * i) % 256, (yy + 2 * i) % 256,
                             (xx + yy) // 2 % 256], -1).astype(np.uint8)
                   for i in range(12)])
video = sp.NamedVideoStream(sc, "tut12_video", frames=frames, codec="mjpeg",
                            quality=90, subsampling="420")
decoded = list(video.load())
err = np.abs(np.stack(decoded).astype(int) - frames.astype(int)).mean()
print(f"12 frames of {frames[0].nbytes} bytes -> mjpeg, mean abs error "
      f"{err:.2f}")
assert err < 3

# ---- a sampled histogram decodes only the sampled frames ----
frame = sc.io.Input([video])
every_third = sc.streams.Stride(frame, [3])
hist = sc.ops.Histogram(frame=every_third, device=dev)
hists = sp.NamedStream(sc, "tut12_hist")
prof = sc.run(sc.io.Output([hist], [hists]), sp.PerfParams.manual(4, 16),
              cache_mode=sp.CacheMode.Overwrite, **run_kw)
rows = [np.frombuffer(r, np.uint32).reshape(3, 256) for r in hists.load()]
assert len(rows) == 4
assert prof.counters()["decoded_frames"] == 4
np.testing.assert_array_equal(
    rows[1][0], np.bincount(decoded[3][:, :, 0].ravel(), minlength=256))

# ---- a computed column, stored lossy, exported and read back ----
frame = sc.io.Input([video])
small = sc.ops.Resize(frame=frame, width=64, height=48, device=dev)
small.compress_video(codec="mjpeg", quality=80)
thumbs = sp.NamedVideoStream(sc, "tut12_small")
sc.run(sc.io.Output(small, [thumbs]), sp.PerfParams.manual(4, 16),
       cache_mode=sp.CacheMode.Overwrite, **run_kw)
path = thumbs.save_mp4(os.path.join(tmp, "small.mp4"), fps=25.0)
probe = _core.mp4_probe(open(path, "rb").read())
print(f"{os.path.basename(path)}: {probe['codec']} {probe['width']}x"
      f"{probe['height']}, {len(probe['sample_sizes'])} samples, "
      f"{os.path.getsize(path)} bytes")
assert probe["codec"] == "mjpeg" and len(probe["sample_sizes"]) == 12

again = sp.NamedVideoStream(sc, "tut12_again", path=path)
for a, b in zip(again.load(), thumbs.load()):
    np.testing.assert_array_equal(a, b)
print("mjpeg video OK")
