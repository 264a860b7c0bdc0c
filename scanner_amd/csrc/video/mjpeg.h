// MJPEG — Motion-JPEG as a video codec of the engine.
//
// Context: the image layer already holds a baseline JPEG encoder and decoder
// whose CPU and gfx950 halves produce identical bytes (ops/jpeg_common.h,
// ops/image_decode.h). Motion-JPEG is those files back to back, one per
// frame and every frame a keyframe; cameras, capture cards and ffmpeg
// (-c:v mjpeg) write it, inside mp4 or mov any player opens it. Behind the
// codec slot next to SVC (svc.h) it gives the engine a lossy column format,
// a standard file to export, and per-frame random access: a strided or
// gathered sample decodes only the wanted frames.
//
// Format (VideoMetadata.codec == "mjpeg"):
//   sample i       one complete JPEG file that jpeg_parse accepts: SOI ..
//                  EOI, baseline or extended sequential, 8-bit, one
//                  interleaved scan; grey, or YCbCr 4:4:4, 4:2:2 or 4:2:0
//   item           the samples of its frames, concatenated, nothing between
//   uniform        every sample of an item has the item's height, width and
//                  channels (1 or 3); tables, restart interval and sampling
//                  may differ from sample to sample
//   metadata       keyframe_indices = every frame; sample_offsets and
//                  sample_sizes as for SVC; frame_type = U8;
//                  VideoMetadata::serialize is unchanged
//   encoder        sample i is exactly jpeg_encode_cpu(frame i, h, w, c,
//                  quality, subsampling), so every sample carries a DRI
//                  segment and the same header
//
// Decode. A frame needs only its own sample, so the byte range of an item
// and task runs from the first wanted sample to the end of the last. CPU:
// jpeg_decode_cpu per wanted frame. GPU (mjpeg_decode_gpu_dev): the range
// stays in HBM and is never read by the host. The host knows one header,
// that of the item's sample 0 (MjpegRefHeader), and builds every decode
// descriptor from it; kernels/mjpeg_index.hip checks each wanted sample
// against that header and finds its restart segments (mjpeg_common.h), and
// the entropy and colour kernels of kernels/jpeg_decode.hip read the span
// in place. A sample the device does not take (another header, no DRI, an
// index or entropy failure) is copied back and goes through jpeg_parse and
// jpeg_decode_gpu with the serial-scan decoder on, so its pixels or its
// error are the CPU decoder's.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "../element.h"
#include "../metadata.h"
#include "../ops/image_decode.h"
#include "../ops/jpeg_common.h"
#include "mjpeg_common.h"

namespace sca {

// Encoder options of the codec; the defaults of a column that names none.
struct MjpegOptions {
  i32 quality = 90;
  JpegSubsampling subsampling = JpegSubsampling::k420;
};
constexpr const char* kMjpegDefaultSubsampling = "420";

// Encode n frames (contiguous HWC u8) as one item. Fills vm: codec,
// geometry, num_frames, keyframe_indices, sample_offsets/sizes.
void mjpeg_encode_cpu(const u8* frames, i64 n, i32 h, i32 w, i32 c,
                      const MjpegOptions& opt, std::vector<u8>& stream,
                      VideoMetadata& vm);
// Append one encoded sample of `size` bytes to the metadata of an item that
// is being built (both sinks and the ingest use it).
void mjpeg_append_sample(VideoMetadata& vm, u64 size);

// Decode the given item-local frames; `stream` holds the item's bytes from
// `stream_offset` on. A sample that fails, or whose shape is not the
// item's, raises ScannerError naming the frame.
void mjpeg_decode_cpu(const u8* stream, size_t size, const VideoMetadata& vm,
                      const std::vector<i64>& want,
                      std::vector<std::vector<u8>>& out, u64 stream_offset = 0);

// The parse, up to the start of the scan, of an item's sample 0.
struct MjpegRefHeader {
  std::vector<u8> bytes;  // SOI .. SOS, header_len of them
  JpegInfo info;          // jpeg_parse_header of them; no segments
  MjpegIndexParams params{};
  bool device_ok = false;  // has a DRI segment: the device can index it
};
// From the first bytes of sample 0 (`size` may cover more than the header).
std::shared_ptr<const MjpegRefHeader> mjpeg_ref_header(const u8* sample0,
                                                       size_t size);
// An upper bound of the header length worth reading from storage.
constexpr u64 kMjpegHeaderReadBytes = 64 * 1024;

struct MjpegGpuStats {
  i64 index_frames = 0;     // frames the device index delivered
  i64 fallback_frames = 0;  // frames handed back to the serial path
};

// GPU decode from a device-resident range (the HBM span cache):
// `stream_dev` holds the item's bytes from offset `dev_lo` on and covers
// every wanted sample. Returns engine elements in HBM, index = item-local
// frame. One status copy and one stream synchronise per call (one more when
// a frame fell back); a range of 4 GiB or more is decoded in several parts.
std::vector<Element> mjpeg_decode_gpu_dev(const u8* stream_dev, u64 dev_lo,
                                          const VideoMetadata& vm,
                                          const std::vector<i64>& want,
                                          DeviceHandle dev,
                                          const MjpegRefHeader& ref_header,
                                          MjpegGpuStats* stats = nullptr);
// The same from host bytes: uploads the range once, then the path above.
std::vector<Element> mjpeg_decode_gpu(const u8* stream_host, size_t size,
                                      const VideoMetadata& vm,
                                      const std::vector<i64>& want,
                                      DeviceHandle dev,
                                      const MjpegRefHeader& ref_header,
                                      u64 stream_offset = 0,
                                      MjpegGpuStats* stats = nullptr);

// The index kernel alone (tests, tools): samples [offsets[i], +sizes[i]) of
// the host buffer `stream` are uploaded and indexed against `ref`. segs
// gets nseg records per sample, zero for a sample with a status.
void mjpeg_index_gpu(const u8* stream, size_t stream_size,
                     const std::vector<u64>& offsets,
                     const std::vector<u64>& sizes, const u8* ref_header,
                     const MjpegIndexParams& p, std::vector<MjpegSeg>& segs,
                     std::vector<u32>& status, double* kernel_ms = nullptr,
                     int repeats = 1);

// SCANNER_MJPEG_GPU: 0 forces the host paths of encode and decode.
bool read_mjpeg_gpu_switch();

}  // namespace sca
