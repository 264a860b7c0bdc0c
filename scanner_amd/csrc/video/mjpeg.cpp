// Host half of the MJPEG codec (mjpeg.h): encode and decode of an item on
// the CPU, and the reference header of an item. HIP-free.
#include "mjpeg.h"

#include <cstdlib>
#include <cstring>

namespace sca {

bool read_mjpeg_gpu_switch() {
  const char* e = std::getenv("SCANNER_MJPEG_GPU");
  if (!e || !*e) return true;
  return std::atoi(e) != 0;
}

void mjpeg_append_sample(VideoMetadata& vm, u64 size) {
  u64 off = vm.sample_offsets.empty()
                ? 0
                : vm.sample_offsets.back() + vm.sample_sizes.back();
  vm.keyframe_indices.push_back((i64)vm.sample_offsets.size());
  vm.sample_offsets.push_back(off);
  vm.sample_sizes.push_back(size);
}

void mjpeg_encode_cpu(const u8* frames, i64 n, i32 h, i32 w, i32 c,
                      const MjpegOptions& opt, std::vector<u8>& stream,
                      VideoMetadata& vm) {
  jpeg_check_args(h, w, c, opt.quality);
  vm.codec = "mjpeg";
  vm.height = h;
  vm.width = w;
  vm.channels = c;
  vm.frame_type = FrameType::U8;
  vm.num_frames = n;
  vm.keyframe_indices.clear();
  vm.sample_offsets.clear();
  vm.sample_sizes.clear();
  size_t fsize = (size_t)h * w * c;
  for (i64 i = 0; i < n; ++i) {
    std::vector<u8> file = jpeg_encode_cpu(frames + (size_t)i * fsize, h, w, c,
                                           opt.quality, opt.subsampling);
    stream.insert(stream.end(), file.begin(), file.end());
    mjpeg_append_sample(vm, file.size());
  }
}

void mjpeg_decode_cpu(const u8* stream, size_t size, const VideoMetadata& vm,
                      const std::vector<i64>& want,
                      std::vector<std::vector<u8>>& out, u64 stream_offset) {
  out.clear();
  out.reserve(want.size());
  for (i64 f : want) {
    SCA_CHECK(f >= 0 && (size_t)f < vm.sample_offsets.size(),
              "mjpeg: frame " + std::to_string(f) + " is not in the item");
    u64 off = vm.sample_offsets[f], sz = vm.sample_sizes[f];
    SCA_CHECK(off >= stream_offset && off - stream_offset + sz <= size,
              "mjpeg: the byte range does not cover frame " +
                  std::to_string(f));
    try {
      DecodedImage img = jpeg_decode_cpu(stream + (off - stream_offset), sz);
      SCA_CHECK(img.h == vm.height && img.w == vm.width &&
                    img.c == vm.channels,
                "its shape " + std::to_string(img.h) + "x" +
                    std::to_string(img.w) + "x" + std::to_string(img.c) +
                    " is not the item's");
      out.push_back(std::move(img.pixels));
    } catch (const ScannerError& err) {
      throw ScannerError("mjpeg: frame " + std::to_string(f) + ": " +
                         err.what());
    }
  }
}

std::shared_ptr<const MjpegRefHeader> mjpeg_ref_header(const u8* sample0,
                                                       size_t size) {
  auto ref = std::make_shared<MjpegRefHeader>();
  size_t scan = jpeg_parse_header(sample0, size, ref->info);
  ref->bytes.assign(sample0, sample0 + scan);
  const JpegDecGeom& g = ref->info.g;
  u32 ri = ref->info.restart_interval;
  u32 per_seg = ri ? ri : g.nmcu;
  MjpegIndexParams& p = ref->params;
  p.header_len = (u32)scan;
  p.mcus_per_seg = per_seg;
  p.nmcu = g.nmcu;
  p.nseg = (g.nmcu + per_seg - 1) / per_seg;
  p.min_scan_bytes = (u32)(((u64)g.nmcu * g.blocks_per_mcu * 2 + 7) / 8);
  ref->device_ok = ri != 0;
  return ref;
}

}  // namespace sca
