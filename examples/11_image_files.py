"""Tutorial 11: image files in, image files out.

The reference's sources-and-sinks tutorial runs Files -> ImageDecoder ->
Resize -> ImageEncoder -> Files. Here it is in two jobs:

  1. video frames -> ImageEncoder(jpg) -> Files sink: a directory of stills
  2. Files source -> ImageDecoder -> Resize -> ImageEncoder -> Files sink

ImageDecoder reads baseline JPEG (grey or YCbCr, 4:4:4 / 4:2:2 / 4:2:0) and
8-bit PNG. On the GPU, JPEG files with restart markers — every file our own
ImageEncoder writes — are decoded on the device from the compressed bytes;
files without them and PNG files are decoded on the host and uploaded
(docs/ops.md, "Image files").
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np

import scanner_amd as sp
from scanner_amd import _core

tmp = tempfile.mkdtemp(prefix="scanner_tut11_")
sc = sp.Client(db_path=os.path.join(tmp, "db"))
gpu = _core.have_gpu()
dev = sp.DeviceType.GPU if gpu else sp.DeviceType.CPU
run_kw = {"gpu_ids": [0]} if gpu else {}

# ---- job 1: a clip becomes a directory of .jpg stills ----
yy, xx = np.mgrid[0:96, 0:128]
frames = np.stack([np.stack([(xx + 4 * i) % 256, (yy + 2 * i) % 256,
                             (xx + yy) // 2 % 256], -1).astype(np.uint8)
                   for i in range(8)])
video = sp.NamedVideoStream(sc, "tut11_video", frames=frames, codec="svc")
jpg = sc.ops.ImageEncoder(frame=sc.io.Input([video]), format="jpg",
                          quality=90, device=dev)
stills = os.path.join(tmp, "stills")
os.makedirs(stills)
sc.run(sc.sinks.Files(jpg, stills, ext="jpg"), sp.PerfParams.manual(4, 8),
       cache_mode=sp.CacheMode.Overwrite, **run_kw)
paths = [os.path.join(stills, f"c0_{i}.jpg") for i in range(8)]
assert all(os.path.exists(p) for p in paths)

# what the decoder will see: shape, sampling and the restart segments that
# make the file parallel
info = _core.jpeg_decode_info(open(paths[0], "rb").read())
print(f"{os.path.basename(paths[0])}: {info['h']}x{info['w']}x{info['c']}, "
      f"{len(info['segments'])} restart segments of "
      f"{info['restart_interval']} MCUs")

# ---- job 2: the stills come back in, are halved and written out again ----
img = sc.sources.Files(paths)
# serial_scan="device" also decodes JPEG files *without* restart markers on
# the GPU (camera, browser and default Pillow files); the default is "host"
frame = sc.ops.ImageDecoder(img=img, serial_scan="device", device=dev)
thumb = sc.ops.Resize(frame=frame, width=64, height=48, device=dev)
# subsampling="420" halves the chroma resolution, as cameras and browsers
# do: smaller files, same bytes on both devices (the default is "444")
out = sc.ops.ImageEncoder(frame=thumb, format="jpg", quality=85,
                          subsampling="420", device=dev)
thumbs = os.path.join(tmp, "thumbs")
os.makedirs(thumbs)
prof = sc.run(sc.sinks.Files(out, thumbs, ext="jpg"),
              sp.PerfParams.manual(4, 8), cache_mode=sp.CacheMode.Overwrite,
              **run_kw)
written = sorted(os.listdir(thumbs))
assert len(written) == 8
if gpu:
    assert prof.counters().get("jpeg_gpu_decode_frames", 0) == 8

# the decoders are also plain functions: a JPEG frame is close to the
# original, a PNG frame is the original
first = _core.image_cpu_decode(open(paths[0], "rb").read())
assert first.shape == frames[0].shape
err = np.abs(first.astype(int) - frames[0].astype(int)).mean()
small = _core.image_cpu_decode(
    open(os.path.join(thumbs, "c0_0.jpg"), "rb").read())
assert small.shape == (48, 64, 3)
thumb_info = _core.jpeg_decode_info(
    open(os.path.join(thumbs, "c0_0.jpg"), "rb").read())
assert (thumb_info["hs"], thumb_info["vs"]) == (2, 2)
print(f"decoded {len(paths)} stills on the {'GPU' if gpu else 'CPU'} "
      f"(mean abs error of the round trip {err:.2f}), wrote "
      f"{len(written)} thumbnails")
assert err < 3
print("image files OK")
