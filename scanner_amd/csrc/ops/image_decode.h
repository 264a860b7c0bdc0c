// Still-image decode: baseline and (on request) progressive JPEG and 8-bit
// PNG files -> HWC u8 frames. The CPU decoders (jpeg_decode_cpu.cpp,
// png_decode.cpp) are HIP-free and define the pixels; kernels/jpeg_decode.hip,
// kernels/jpeg_sync_decode.hip and kernels/jpeg_progressive_decode.hip
// reproduce the JPEG ones on the GPU from the same arithmetic
// (jpeg_decode_common.h, jpeg_sync_common.h, jpeg_progressive_common.h).
//
// Accepted JPEG: SOF0, or SOF1 at 8-bit precision; 1 component, or 3
// components taken as YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma
// 1x1; one interleaved scan; any restart interval. With
// JpegParseOptions::allow_progressive also SOF2 at 8 bits under the same
// component and sampling rules: any number of scans, each over all
// components (DC only) or over exactly one, with DHT, DQT and DRI segments
// between them, whose script obeys T.81 G.1.1.1.1; a file whose scans leave
// bits unrefined or bands uncoded decodes to what it holds. Without the
// option a progressive file is rejected by name, as before. Accepted PNG: 8-bit
// grey, RGB or RGBA (alpha dropped), not interlaced. Everything else is
// rejected with a message that names the cause. No parser or decoder reads
// outside the bytes it is given.
#pragma once

#include <string>
#include <vector>

#include "jpeg_decode_common.h"

namespace sca {

// One restart segment of the scan: bytes [begin, end) of the file (the RSTn
// marker that follows is not included) and the MCUs it holds.
struct JpegSegment {
  u32 begin, end;
  u32 first_mcu, mcu_count;
};

// One scan of a progressive file. `segments[].first_mcu/mcu_count` count the
// scan's own units: MCUs for an interleaved scan, blocks of the component's
// own raster (jpeg_prog_comp_blocks) for a single-component scan.
struct JpegScan {
  u32 ncomp = 0;             // 1, or all components of the frame (DC only)
  u32 comp[3] = {0, 0, 0};   // frame indices of its components, in order
  u32 ss = 0, se = 0, ah = 0, al = 0;
  u32 restart_interval = 0;  // units; 0 = no DRI segment in force
  u32 units = 0;             // units in the scan
  u32 blocks_per_unit = 0;   // blocks_per_mcu when interleaved, else 1
  JpegHuff dc[3], ac[3];     // per frame component, as they stood at its SOS
  std::vector<JpegSegment> segments;
};

struct JpegInfo {
  JpegDecGeom g{};
  u32 restart_interval = 0;  // MCUs; 0 = the file has no DRI segment
  u16 q[3][64];              // per component, natural order
  JpegHuff dc[3], ac[3];     // per component
  u8 zz2nat[64];
  std::vector<JpegSegment> segments;  // empty for a progressive file
  bool progressive = false;
  std::vector<JpegScan> scans;  // progressive files only, in file order
};

struct JpegParseOptions {
  bool allow_progressive = false;  // else SOF2 is rejected by name
};
// "reject" (false) or "decode" (true); anything else is rejected by name
// with the supported list. `who` starts the message.
bool jpeg_progressive_option(const std::string& value, const char* who);

JpegInfo jpeg_parse(const u8* data, size_t size, JpegParseOptions opt = {});
// The first half of jpeg_parse: everything up to the start of the (first)
// scan. Fills every field of `info` except `segments` and `scans` and
// returns the offset of the first entropy-coded byte. Same checks, same
// messages. For a progressive file the Huffman tables of `info` stay zero
// (every scan carries its own) and the quantisation tables are those
// defined so far; restart_interval is the last DRI read.
size_t jpeg_parse_header(const u8* data, size_t size, JpegInfo& info,
                         JpegParseOptions opt = {});

struct DecodedImage {
  i32 h = 0, w = 0, c = 0;
  std::vector<u8> pixels;  // HWC
};

// The oracle: serial, from jpeg_decode_common.h (and, for a progressive
// file, jpeg_progressive_common.h: the scans in file order into a zeroed
// coefficient buffer, then dequantisation, IDCT and colour as for baseline).
DecodedImage jpeg_decode_cpu(const u8* data, size_t size,
                             JpegParseOptions opt = {});
// Decode of an already parsed file into h*w*c bytes at `out`.
void jpeg_decode_cpu_into(const u8* data, const JpegInfo& info, u8* out);
// The quantised coefficients of an already parsed file, baseline or
// progressive: nmcu * blocks_per_mcu blocks of 64 in natural order, in the
// MCU order of jpeg_block_pos.
void jpeg_coefficients_cpu(const u8* data, const JpegInfo& info,
                           std::vector<i16>& coef);
// Text of an entropy error, shared with the GPU decoder's report; the second
// form is for a scan of a progressive file.
std::string jpeg_entropy_error(u32 status, u32 segment);
std::string jpeg_entropy_error(u32 status, u32 segment, u32 scan);

// ---- model of the self-synchronising decoder (jpeg_sync_cpu.cpp) ----
struct JpegSyncStats {
  u32 chunks = 0, groups = 0;
  u32 group_iterations = 0;  // most iterations any in-group loop ran
  u32 cross_rounds = 0;      // last round across groups that changed an exit
  u32 cross_repairs = 0;     // groups repaired in those rounds
  u32 stuffed_starts = 0;    // chunks that started on a stuffed 00
  u32 empty_chunks = 0;      // chunks that hold no symbol boundary
  u32 status = 0;            // 0, or JpegBlockStatus / JpegSyncStatus
  bool verified = false;     // else the pixels are jpeg_decode_cpu_into's
};
// The kernels' algorithm on one file without restart markers, lane by lane:
// the same pixels into h*w*c bytes at `out` and the same verdict. A file
// that fails verification is decoded by jpeg_decode_cpu_into (which raises
// on a corrupt one) after *stats has been written. chunk_bytes 0 is the
// default.
void jpeg_decode_sync_model(const u8* data, const JpegInfo& info,
                            u32 chunk_bytes, u8* out,
                            JpegSyncStats* stats = nullptr);

// IHDR only: the output shape (c is 1 or 3), after the same checks
// png_decode makes on the header.
void png_shape(const u8* data, size_t size, i32& h, i32& w, i32& c);
DecodedImage png_decode(const u8* data, size_t size);

bool is_jpeg(const u8* data, size_t size);
bool is_png(const u8* data, size_t size);
// Dispatch on the magic bytes.
DecodedImage image_decode_cpu(const u8* data, size_t size,
                              JpegParseOptions opt = {});

// ---- HIP decoder (kernels/jpeg_decode.hip) ----
struct ImageBlob {
  const u8* data;  // host memory
  size_t size;
};
struct DeviceFrame {
  u8* buffer = nullptr;  // HWC u8 on the device, release with delete_buffer
  i32 h = 0, w = 0, c = 0;
};
// Decodes a batch of files (any mix of shapes, samplings and tables) into
// device frames, in order. infos[i] is jpeg_parse of blobs[i] for a JPEG row
// and is ignored for a PNG row. JPEG rows with a DRI segment are decoded on
// the device, one lane per restart segment. JPEG rows without one are
// decoded by the CPU decoder and uploaded, unless
// opt.serial_scan_on_device asks for the self-synchronising decoder
// (kernels/jpeg_sync_decode.hip, jpeg_sync_common.h): one lane per chunk of
// opt.chunk_bytes, verified on the device; a row that fails the
// verification is decoded by jpeg_decode_cpu_into after the synchronise and
// uploaded, so its pixels or its error are always the CPU decoder's. A
// progressive row (infos[i].progressive; needs opt.progressive) whose every
// scan has a restart interval is decoded on the device by
// kernels/jpeg_progressive_decode.hip, one lane per restart segment of a
// scan and one launch per scan index; one with a scan without a restart
// interval goes there (one lane for that scan) only under
// opt.serial_scan_on_device and is a host row otherwise, and so is a row
// with more than kJpegProgMaxDeviceScans scans. PNG
// rows are decoded by the CPU decoder. *host_rows counts every row the CPU
// decoders handled. Everything is issued on `stream`, which is synchronised
// once, after the per-file status words have been copied back (once more
// when a row fell back); a corrupt row raises ScannerError naming the row
// and no frame of the call survives. The frames share one block buffer:
// release each with delete_buffer(dev, buffer).
// One kernel launch per scan index of a batch: Pillow and libjpeg's default
// script write 10 scans for colour, and a script that codes every bit of
// every band of three components on its own stays below 32. A file with
// more (a hostile one could ask for thousands of launches) is a host row.
constexpr u32 kJpegProgMaxDeviceScans = 32;
struct JpegGpuOptions {
  bool serial_scan_on_device = false;
  u32 chunk_bytes = 0;  // 0: kJpegSyncChunkBytes; else a power of two >= 4
  bool progressive = false;  // the infos were parsed with allow_progressive
};
struct JpegGpuStats {
  i64 sync_rows = 0;      // rows the self-synchronising decoder delivered
  i64 fallback_rows = 0;  // rows it gave back to the CPU decoder
  i64 progressive_rows = 0;  // progressive rows decoded on the device
};
void jpeg_decode_gpu(const std::vector<ImageBlob>& blobs,
                     const std::vector<JpegInfo>& infos, DeviceHandle dev,
                     void* stream, std::vector<DeviceFrame>& out_frames,
                     i64* host_rows = nullptr, JpegGpuOptions opt = {},
                     JpegGpuStats* stats = nullptr);
// The ImageDecoder argument serial_scan ("host", the default, or "device")
// from an op instance's msgpack args; any other value is rejected by name.
bool image_decoder_serial_scan_on_device(const std::vector<u8>& args);
// The ImageDecoder argument progressive ("reject", the default, or "decode"),
// likewise.
bool image_decoder_progressive(const std::vector<u8>& args);
// Seconds the calling thread's last jpeg_decode_gpu spent waiting in its
// stream synchronise.
double jpeg_decode_gpu_last_sync_seconds();

}  // namespace sca
