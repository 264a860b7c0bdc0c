// ImageDecoder op: JPEG or PNG blobs -> u8 frames, the inverse of
// ImageEncoder (capability parity: the reference's ImageDecoder op over
// OpenCV imdecode). Formats and limits: image_decode.h. Every output element
// carries its own frame_info, since shapes may change from row to row. This
// is the CPU kernel; the GPU kernel lives in kernels/jpeg_decode.hip.
#include <cstring>

#include "../memory.h"
#include "../msgpack.h"
#include "image_decode.h"
#include "kernel.h"

namespace sca {

namespace {

class ImageDecoderKernelCPU : public BatchedKernel {
 public:
  explicit ImageDecoderKernelCPU(const KernelConfig& cfg)
      : BatchedKernel(cfg) {
    // where a GPU kernel decodes scans without restart markers; nothing to
    // choose here, but a graph may carry the argument on either device
    image_decoder_serial_scan_on_device(cfg.args);
    parse_.allow_progressive = image_decoder_progressive(cfg.args);
  }
  void execute_batch(const BatchedElements& in, BatchedElements& out) override {
    for (size_t i = 0; i < in[0].size(); ++i) {
      const Element& b = in[0][i];
      Element e;
      if (b.is_null) {
        e.is_null = true;
        out[0].push_back(e);
        continue;
      }
      SCA_CHECK(!b.is_frame, "ImageDecoder needs a bytes input");
      DecodedImage img;
      try {
        img = image_decode_cpu(b.buffer, b.size, parse_);
      } catch (const ScannerError& err) {
        throw ScannerError("ImageDecoder: row " + std::to_string(i) +
                           " of the batch: " + err.what());
      }
      e.is_frame = true;
      e.frame_info.shape[0] = img.h;
      e.frame_info.shape[1] = img.w;
      e.frame_info.shape[2] = img.c;
      e.frame_info.type = FrameType::U8;
      e.size = img.pixels.size();
      e.buffer = new_buffer(config_.device, e.size);
      e.device = config_.device;
      std::memcpy(e.buffer, img.pixels.data(), e.size);
      out[0].push_back(e);
    }
  }

 private:
  JpegParseOptions parse_;
};

}  // namespace

bool image_decoder_serial_scan_on_device(const std::vector<u8>& args) {
  std::string v = mp::decode(args).get_str("serial_scan", "host");
  SCA_CHECK(v == "host" || v == "device",
            "ImageDecoder supports serial_scan=host|device, got '" + v + "'");
  return v == "device";
}

bool image_decoder_progressive(const std::vector<u8>& args) {
  return jpeg_progressive_option(
      mp::decode(args).get_str("progressive", "reject"), "ImageDecoder");
}

void register_image_decoder_op() {
  static bool done = false;
  if (done) return;
  done = true;
  OpInfo o;
  o.name = "ImageDecoder";
  o.input_columns = {{"img", ColumnType::Bytes}};
  o.output_columns = {{"frame", ColumnType::Video}};
  op_registry().add(o);
  KernelFactory f;
  f.op_name = "ImageDecoder";
  f.device_type = DeviceType::CPU;
  f.preferred_batch = 8;
  f.make = [](const KernelConfig& c) -> std::unique_ptr<BaseKernel> {
    return std::make_unique<ImageDecoderKernelCPU>(c);
  };
  kernel_registry().add(f);
}

}  // namespace sca
