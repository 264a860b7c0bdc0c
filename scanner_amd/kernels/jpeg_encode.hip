// GPU baseline JPEG encoder for gfx950: device-resident u8 frames become
// JFIF files in HBM, byte-identical to jpeg_encode_cpu, so an image sink
// moves only compressed bytes over the host link. Format and the shared
// integer arithmetic: csrc/ops/jpeg_common.h.
//
// Kernel shape (three launches per chunk of same-shape frames):
//   segment  grid (segments, frames) x 256 lanes, one workgroup per restart
//            segment of R = 32 MCUs (<= 96 blocks):
//              A  lane (row r, MCU m) loads 8 pixels of one image row (lanes
//                 of a wave read neighbouring MCUs, so a wave covers two
//                 contiguous row pieces), converts colour in registers and
//                 runs the row DCT -> int16 in LDS
//              B  lane (MCU m, column u) runs the column DCT, quantises and
//                 stores the zig-zagged int16 coefficients in LDS
//              C  one lane per block walks its 64 coefficients twice: code
//                 lengths -> workgroup exclusive scan -> codes OR-merged
//                 into a zeroed LDS bit image with LDS atomics
//              D  1-bit padding, then 256 bytes per step are byte-stuffed
//                 with a ballot prefix and stored to the segment's slot in
//                 device staging (worst-case stride); byte count -> sizes
//            Coefficients never reach global memory.
//            4:2:0 (S420): the segment is 16 MCUs of 16x16 pixels, again
//            96 blocks, block b = MCU * 6 + {Y00, Y01, Y10, Y11, Cb, Cr}:
//              A  lane (pixel row r of 16, MCU m of 16), tid = r * 16 + m,
//                 loads 16 pixels of one row, runs the two Y row DCTs and
//                 pair-sums Cb/Cr horizontally; the sums of row r ^ 1 come
//                 from 16 lanes away in the same wave by a shuffle, and the
//                 even-row lane rounds (jpeg_downsample4) and runs the
//                 chroma row DCTs of chroma row r / 2
//              B  lane (u, MCU m) x 3 steps covers block kinds 2 per step
//              C  the DC predictor of a block is the previous block of its
//                 component: b-1 (Y01..Y11), b-3 (Y00), b-6 (Cb, Cr)
//              D  as above
//   scan     one workgroup per frame: exclusive scan of (segment size + 2
//            marker bytes) for any segment count -> offsets and file size.
//   gather   grid (segments, frames): header, compacted segments, RSTn
//            markers and EOI into exact-size outputs.
// The host reads the file sizes once per chunk (one stream synchronise),
// allocates exact-size outputs from the slab pool and synchronises once more
// before the staging goes back to the pool.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../csrc/memory.h"
#include "../csrc/msgpack.h"
#include "../csrc/ops/jpeg_common.h"
#include "../csrc/ops/kernel.h"
#include "../csrc/ops/png_common.h"

namespace sca {

namespace {

#define JPEG_ENC_CHECK(expr)                                             \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess) {                                              \
      throw ScannerError(std::string("HIP error in jpeg encode: ") +     \
                         hipGetErrorString(_e));                         \
    }                                                                    \
  } while (0)

constexpr u32 kR = kJpegRestartInterval;
constexpr u32 kThreads = 256;
static_assert(kR * 8 == kThreads, "one lane per (MCU, row) of a segment");
constexpr u32 kR420 = kJpegRestartInterval420;
static_assert(kR420 * 16 == kThreads, "one lane per (MCU, row) in 4:2:0");
static_assert(kR420 * 6 == kR * 3, "both modes code 96 blocks per segment");
static_assert(64 % kR420 == 0 && (64 / kR420) % 2 == 0,
              "rows r and r ^ 1 of an MCU sit in one wave");
constexpr u32 kMaxChunk = 16;  // frames per launch sequence
// staging holds worst-case segments (about 7x the raw frame); frames per
// launch sequence are limited so that it stays below this
constexpr u64 kStagingBudget = 384ull << 20;
// int16 per block in LDS; 33 words, so lanes walking neighbouring blocks
// hit different banks
constexpr u32 kCoefStride = 66;
// bit image of one segment before stuffing, + the word a code may spill into
constexpr u32 kBitWords = kR * 3 * kJpegBlockMaxBytes / 4 + 2;
static_assert(kBitWords * 4 >= kR * 3 * 64 * sizeof(i16),
              "row-pass results alias the bit image");

struct JpegEncArgs {
  const u8* frames[kMaxChunk];
  u8* out[kMaxChunk];        // exact-size files (gather)
  u8* staging;               // segment (f, s) at (f * nseg + s) * seg_stride
  u32* seg_sizes;            // [nframes][nseg] stuffed bytes
  u32* seg_off;              // [nframes][nseg] offset past the header
  u32* sizes;                // [nframes] file sizes
  const JpegTables* tables;
  const u8* header;
  u32 header_len;
  JpegGeom g;
};

// exclusive prefix of v over the 256 lanes; total in `all`
__device__ inline u32 block_excl_scan(u32 v, u32* wave_sum, u32& all) {
  u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32 x = v;
#pragma unroll
  for (u32 d = 1; d < 64; d <<= 1) {
    u32 y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  __syncthreads();  // wave_sum may still be read from an earlier scan
  if (lane == 63) wave_sum[wave] = x;
  __syncthreads();
  u32 before = 0;
  all = 0;
#pragma unroll
  for (u32 k = 0; k < kThreads / 64; ++k) {
    u32 t = wave_sum[k];
    if (k < wave) before += t;
    all += t;
  }
  return before + x - v;
}

struct BitCount {
  u32 bits = 0;
  __device__ void operator()(u32, u32 len) { bits += len; }
};

// OR a code into the MSB-first bit image at bit `pos`
struct BitMerge {
  u32* img;
  u32 pos;
  __device__ void operator()(u32 bits, u32 len) {
    u32 w = pos >> 5, o = pos & 31;
    u64 v = (u64)bits << (64 - len - o);
    atomicOr(&img[w], (u32)(v >> 32));
    u32 lo = (u32)v;
    if (lo) atomicOr(&img[w + 1], lo);
    pos += len;
  }
};

// N (8 or 16) pixels of one row, C bytes each, starting at column x0 of `row`
template <int C, int N = 8>
__device__ inline void load_pixels(const u8* __restrict__ row, u32 x0, i32 w,
                                   u8 (&px)[N * C]) {
  const u8* p = row + (u64)x0 * C;
  if (x0 + N <= (u32)w && ((uintptr_t)p & 3) == 0) {
    const u32* p4 = reinterpret_cast<const u32*>(p);
    u32 v[N * C / 4];
#pragma unroll
    for (int k = 0; k < N * C / 4; ++k) v[k] = p4[k];
#pragma unroll
    for (int k = 0; k < N * C; ++k) px[k] = (u8)(v[k / 4] >> (8 * (k & 3)));
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      u32 x = min(x0 + (u32)k, (u32)w - 1);  // replicate the last column
#pragma unroll
      for (int ch = 0; ch < C; ++ch) px[k * C + ch] = row[(u64)x * C + ch];
    }
  }
}

// S420: the 4:2:0 variant (C == 3), see the file comment
template <int C, bool S420 = false>
__global__ void __launch_bounds__(kThreads) jpeg_segment_kernel(JpegEncArgs a) {
  static_assert(!S420 || C == 3, "4:2:0 needs three channels");
  constexpr u32 R = S420 ? kR420 : kR;     // MCUs per segment
  constexpr u32 MB = S420 ? 6u : (u32)C;   // blocks per MCU
  static_assert(R * MB <= kR * 3, "LDS is sized for 96 blocks");
  __shared__ JpegTables t;
  __shared__ u32 bits[kBitWords];
  __shared__ i16 coef[R * MB * kCoefStride];
  __shared__ u32 wave_sum[kThreads / 64];
  u32 s = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  u32 lane = tid & 63, wave = tid >> 6;
  const JpegGeom& g = a.g;
  u32 m0 = s * R;
  u32 nm = min(R, g.nmcu - m0);  // MCUs in this segment

  for (u32 i = tid; i < sizeof(JpegTables) / 4; i += kThreads)
    reinterpret_cast<u32*>(&t)[i] = reinterpret_cast<const u32*>(a.tables)[i];

  // ---- A: load, colour, row DCT -> rowres[comp][r][m][u] (Q6); a lane
  // writes 16 contiguous bytes next to its neighbour's ----
  i16* rowres = reinterpret_cast<i16*>(bits);
  if constexpr (S420) {
    // rowres[kind][row of the block][m][u], kind = Y00 Y01 Y10 Y11 Cb Cr.
    // m < nm is the same for the lanes of rows r and r ^ 1, and a clamped
    // row only changes the address a lane loads from, so both partners of
    // a shuffle are always active together.
    u32 r = tid / R, m = tid % R;
    if (m < nm) {
      u32 mg = m0 + m;
      u32 bx = mg % g.mcus_x, by = mg / g.mcus_x;
      u32 y = min(by * 16 + r, (u32)g.h - 1);  // replicate the last row
      u8 px[16 * 3];
      load_pixels<3, 16>(a.frames[f] + (u64)y * g.w * 3, bx * 16, g.w, px);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        i32 in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const u8* p = px + (half * 8 + k) * 3;
          in[k] = jpeg_sample_rgb(p[0], p[1], p[2], 0);
        }
        jpeg_dct8(in, out);
        i16* dst =
            rowres + ((((r / 8) * 2 + half) * 8 + r % 8) * R + m) * 8;
#pragma unroll
        for (int u = 0; u < 8; ++u) dst[u] = (i16)jpeg_descale_row(out[u]);
      }
#pragma unroll
      for (int comp = 1; comp < 3; ++comp) {
        i32 in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const u8* p = px + k * 6;
          i32 sum = jpeg_sample_rgb(p[0], p[1], p[2], comp) +
                    jpeg_sample_rgb(p[3], p[4], p[5], comp);
          // the other row of the 2x2 cell; a + b + c + d + 2 >> 2 is
          // jpeg_downsample4 whatever the order of the additions
          in[k] = (sum + __shfl_xor(sum, (int)R, 64) + 2) >> 2;
        }
        if ((r & 1) == 0) {
          jpeg_dct8(in, out);
          i16* dst = rowres + (((3 + comp) * 8 + r / 2) * R + m) * 8;
#pragma unroll
          for (int u = 0; u < 8; ++u) dst[u] = (i16)jpeg_descale_row(out[u]);
        }
      }
    }
  } else {
    u32 r = tid / kR, m = tid % kR;
    if (m < nm) {
      u32 mg = m0 + m;
      u32 bx = mg % g.mcus_x, by = mg / g.mcus_x;
      u32 y = min(by * 8 + r, (u32)g.h - 1);  // replicate the last row
      u8 px[8 * C];
      load_pixels<C>(a.frames[f] + (u64)y * g.w * C, bx * 8, g.w, px);
#pragma unroll
      for (int comp = 0; comp < C; ++comp) {
        i32 in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if constexpr (C == 1) {
            in[k] = jpeg_sample_grey(px[k]);
          } else {
            in[k] = jpeg_sample_rgb(px[k * 3], px[k * 3 + 1], px[k * 3 + 2],
                                    comp);
          }
        }
        jpeg_dct8(in, out);
        i16* dst = rowres + ((comp * 8 + r) * kR + m) * 8;
#pragma unroll
        for (int u = 0; u < 8; ++u) dst[u] = (i16)jpeg_descale_row(out[u]);
      }
    }
  }
  __syncthreads();

  // ---- B: column DCT, quantise, zig-zag -> coef[m * C + comp][64] ----
  if constexpr (S420) {
    u32 u = tid % 8;
#pragma unroll
    for (u32 j = 0; j < 3; ++j) {
      u32 idx = j * 32 + tid / 8;  // kind * R + m, 0..95
      u32 kind = idx / R, m = idx % R;
      if (m < nm) {
        const i16* src = rowres + (kind * 8 * R + m) * 8 + u;
        i32 in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = src[r * R * 8];
        jpeg_dct8(in, out);
        const u16* q = t.q[kind < 4 ? 0 : 1];
        i16* dst = coef + (m * 6 + kind) * kCoefStride;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          u32 nat = v * 8 + u;
          dst[t.nat2zz[nat]] = (i16)jpeg_quantize(out[v], q[nat]);
        }
      }
    }
  } else {
    u32 m = tid / 8, u = tid % 8;
    if (m < nm) {
#pragma unroll
      for (int comp = 0; comp < C; ++comp) {
        const i16* src = rowres + (comp * 8 * kR + m) * 8 + u;
        i32 in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = src[r * kR * 8];
        jpeg_dct8(in, out);
        const u16* q = t.q[comp ? 1 : 0];
        i16* dst = coef + (m * C + comp) * kCoefStride;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          u32 nat = v * 8 + u;
          dst[t.nat2zz[nat]] = (i16)jpeg_quantize(out[v], q[nat]);
        }
      }
    }
  }
  __syncthreads();

  // ---- C: code lengths, scan, OR-merge into the zeroed bit image ----
  for (u32 i = tid; i < kBitWords; i += kThreads) bits[i] = 0;
  u32 nb = nm * MB;
  const i16* zz = coef + tid * kCoefStride;
  i32 pred = 0;
  u32 pos = tid % MB;  // position in the MCU
  // blocks back to the previous one of the same component
  u32 back = !S420 ? MB : pos >= 4 ? 6u : pos ? 1u : 3u;
  bool chroma = S420 ? pos >= 4 : pos != 0;
  const u32* dc = t.dc[chroma ? 1 : 0];
  const u32* ac = t.ac[chroma ? 1 : 0];
  u32 my_bits = 0;
  if (tid < nb) {
    // the first block of a component in the segment predicts from 0
    if (tid >= back) pred = zz[-(i32)(back * kCoefStride)];
    BitCount cnt;
    jpeg_code_block(zz, pred, dc, ac, cnt);
    my_bits = cnt.bits;
  }
  u32 total_bits;
  u32 my_pos = block_excl_scan(my_bits, wave_sum, total_bits);  // syncs
  if (tid < nb) {
    BitMerge mrg{bits, my_pos};
    jpeg_code_block(zz, pred, dc, ac, mrg);
  }
  if (tid == 0 && (total_bits & 7)) {  // pad to a byte with 1-bits
    u32 pad = 8 - (total_bits & 7);
    BitMerge mrg{bits, total_bits};
    mrg((1u << pad) - 1u, pad);
  }
  __syncthreads();

  // ---- D: byte stuffing, 256 bytes per step ----
  u32 nbytes = (total_bits + 7) / 8;
  u8* dst = a.staging + ((u64)f * g.nseg + s) * g.seg_stride;
  u32 carry = 0;  // bytes written by earlier steps
  for (u32 k0 = 0; k0 < nbytes; k0 += kThreads) {
    u32 k = k0 + tid;
    bool valid = k < nbytes;
    u32 byte = valid ? (bits[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu : 0u;
    bool ff = byte == 0xffu;
    u64 mask = __ballot(ff);
    u32 before = (u32)__popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_sum[wave] = (u32)__popcll(mask);
    __syncthreads();
    u32 all = 0;
#pragma unroll
    for (u32 w = 0; w < kThreads / 64; ++w) {
      u32 x = wave_sum[w];
      if (w < wave) before += x;
      all += x;
    }
    if (valid) {
      u32 o = carry + tid + before;
      dst[o] = (u8)byte;
      if (ff) dst[o + 1] = 0;
    }
    carry += min(kThreads, nbytes - k0) + all;
    __syncthreads();
  }
  if (tid == 0) a.seg_sizes[(u64)f * g.nseg + s] = carry;
}

// One workgroup per frame; 256 segments per step, carry kept across steps.
// Every segment is followed by a two-byte marker (RSTn, or EOI after the
// last one).
__global__ void __launch_bounds__(kThreads) jpeg_scan_kernel(JpegEncArgs a) {
  __shared__ u32 wave_sum[kThreads / 64];
  u32 f = blockIdx.x, tid = threadIdx.x;
  u32 nseg = a.g.nseg;
  const u32* sz = a.seg_sizes + (u64)f * nseg;
  u32* off = a.seg_off + (u64)f * nseg;
  u32 carry = 0;
  for (u32 s0 = 0; s0 < nseg; s0 += kThreads) {
    u32 s = s0 + tid;
    u32 val = s < nseg ? sz[s] + 2u : 0u;
    u32 all;
    u32 x = block_excl_scan(val, wave_sum, all);
    if (s < nseg) off[s] = carry + x;
    carry += all;
  }
  if (tid == 0) a.sizes[f] = a.header_len + carry;
}

__global__ void __launch_bounds__(kThreads) jpeg_gather_kernel(JpegEncArgs a) {
  u32 s = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  u32 nseg = a.g.nseg;
  u8* file = a.out[f];
  if (s == 0) {
    for (u32 i = tid; i < a.header_len; i += kThreads) file[i] = a.header[i];
  }
  const u8* src = a.staging + ((u64)f * nseg + s) * a.g.seg_stride;
  u32 n = a.seg_sizes[(u64)f * nseg + s];
  u8* dst = file + a.header_len + a.seg_off[(u64)f * nseg + s];
  for (u32 i = tid; i < n; i += kThreads) dst[i] = src[i];
  if (tid == 0) {
    dst[n] = 0xff;
    dst[n + 1] = s + 1 < nseg ? (u8)(0xd0 + (s & 7)) : (u8)0xd9;
  }
}

u64 align_up(u64 x, u64 a) { return (x + a - 1) / a * a; }

}  // namespace

void jpeg_encode_gpu(const std::vector<const u8*>& frames, i32 h, i32 w,
                     i32 c, i32 quality, DeviceHandle dev, void* stream,
                     std::vector<u8*>& out, std::vector<u64>& sizes,
                     JpegSubsampling ss) {
  jpeg_check_args(h, w, c, quality);
  SCA_CHECK(dev.is_gpu(), "jpeg_encode_gpu needs a GPU device");
  if (frames.empty()) return;
  JPEG_ENC_CHECK(hipSetDevice(dev.id));
  hipStream_t s = (hipStream_t)stream;

  JpegTables tables;
  jpeg_make_tables(c, quality, tables);
  std::vector<u8> header = jpeg_header(h, w, c, tables, ss);
  JpegGeom g = jpeg_geom(h, w, c, ss);
  u64 bound = jpeg_size_bound(h, w, c, ss);

  u64 frame_staging = (u64)g.nseg * g.seg_stride;
  size_t chunk_max = (size_t)std::max<u64>(
      1, std::min<u64>({(u64)kMaxChunk, (u64)frames.size(),
                        kStagingBudget / frame_staging}));
  // one slab-pool allocation: segments, the three u32 arrays, tables, header
  u64 seg_sizes_off = align_up(frame_staging * chunk_max, 256);
  u64 seg_off_off = seg_sizes_off + align_up(chunk_max * g.nseg * 4, 256);
  u64 sizes_off = seg_off_off + align_up(chunk_max * g.nseg * 4, 256);
  u64 tables_off = sizes_off + align_up(chunk_max * 4, 256);
  u64 header_off = tables_off + align_up(sizeof(JpegTables), 256);
  u8* staging = new_buffer(dev, header_off + header.size());
  u32 host_sizes[kMaxChunk];
  size_t first_out = out.size();

  try {
    JPEG_ENC_CHECK(hipMemcpyAsync(staging + tables_off, &tables,
                                  sizeof(JpegTables), hipMemcpyHostToDevice,
                                  s));
    JPEG_ENC_CHECK(hipMemcpyAsync(staging + header_off, header.data(),
                                  header.size(), hipMemcpyHostToDevice, s));
    for (size_t c0 = 0; c0 < frames.size(); c0 += chunk_max) {
      size_t n = std::min(chunk_max, frames.size() - c0);
      JpegEncArgs a{};
      a.staging = staging;
      a.seg_sizes = reinterpret_cast<u32*>(staging + seg_sizes_off);
      a.seg_off = reinterpret_cast<u32*>(staging + seg_off_off);
      a.sizes = reinterpret_cast<u32*>(staging + sizes_off);
      a.tables = reinterpret_cast<const JpegTables*>(staging + tables_off);
      a.header = staging + header_off;
      a.header_len = (u32)header.size();
      a.g = g;
      for (size_t i = 0; i < n; ++i) {
        SCA_CHECK(frames[c0 + i], "jpeg encode: null frame pointer");
        a.frames[i] = frames[c0 + i];
      }
      dim3 grid(g.nseg, (u32)n);
      if (g.ss == JpegSubsampling::k420) {
        jpeg_segment_kernel<3, true><<<grid, kThreads, 0, s>>>(a);
      } else if (c == 3) {
        jpeg_segment_kernel<3><<<grid, kThreads, 0, s>>>(a);
      } else {
        jpeg_segment_kernel<1><<<grid, kThreads, 0, s>>>(a);
      }
      JPEG_ENC_CHECK(hipGetLastError());
      jpeg_scan_kernel<<<(u32)n, kThreads, 0, s>>>(a);
      JPEG_ENC_CHECK(hipGetLastError());
      JPEG_ENC_CHECK(hipMemcpyAsync(host_sizes, a.sizes, n * 4,
                                    hipMemcpyDeviceToHost, s));
      JPEG_ENC_CHECK(hipStreamSynchronize(s));

      // exact-size outputs, 16-byte aligned, in one block buffer
      u64 total = 0;
      for (size_t i = 0; i < n; ++i) {
        SCA_CHECK(host_sizes[i] > header.size() && host_sizes[i] <= bound,
                  "jpeg encode: file size out of range");
        total += align_up(host_sizes[i], 16);
      }
      u8* block = new_block_buffer(dev, total, (i32)n);
      u64 pos = 0;
      for (size_t i = 0; i < n; ++i) {
        a.out[i] = block + pos;
        out.push_back(block + pos);
        sizes.push_back(host_sizes[i]);
        pos += align_up(host_sizes[i], 16);
      }
      jpeg_gather_kernel<<<grid, kThreads, 0, s>>>(a);
      JPEG_ENC_CHECK(hipGetLastError());
    }
    // the staging feeds the last gather
    JPEG_ENC_CHECK(hipStreamSynchronize(s));
  } catch (...) {
    (void)hipStreamSynchronize(s);
    for (size_t i = first_out; i < out.size(); ++i) delete_buffer(dev, out[i]);
    out.resize(first_out);
    sizes.resize(first_out);
    delete_buffer(dev, staging);
    throw;
  }
  delete_buffer(dev, staging);
}

namespace {

// ImageEncoder on the GPU: JPEG, and PNG with png_writer="parallel"
// (kernels/png_encode.hip); the zlib PNG writer stays a CPU kernel.
class ImageEncoderKernelGPU : public BatchedKernel {
 public:
  explicit ImageEncoderKernelGPU(const KernelConfig& cfg)
      : BatchedKernel(cfg) {
    auto a = mp::decode(cfg.args);
    std::string format = a.get_str("format", "png");
    if (format == "png") {
      // like subsampling for JPEG, read for PNG only
      PngWriter writer = png_parse_writer(a.get_str("png_writer", "zlib"));
      SCA_CHECK(writer == PngWriter::kParallel,
                "ImageEncoder format=png has no GPU kernel; run it with "
                "device=CPU (format=jpg is supported on the GPU), or pass "
                "png_writer=\"parallel\"");
      png_ = true;
      return;
    }
    SCA_CHECK(format == "jpg" || format == "jpeg",
              "ImageEncoder supports format=png|jpg|jpeg, got '" + format +
                  "'");
    quality_ = (i32)a.get_int("quality", 90);
    SCA_CHECK(quality_ >= 1 && quality_ <= 100,
              "ImageEncoder quality must be in 1..100, got " +
                  std::to_string(quality_));
    subsampling_ = jpeg_parse_subsampling(a.get_str("subsampling", "444"));
  }

  void execute_batch(const BatchedElements& in, BatchedElements& out) override {
    const ElementVector& col = in[0];
    out[0].resize(col.size());
    // consecutive frames of one shape are encoded together; a null row or
    // a shape change ends the sub-batch
    size_t i = 0;
    while (i < col.size()) {
      if (col[i].is_null) {
        out[0][i].is_null = true;
        ++i;
        continue;
      }
      check(col[i]);
      size_t j = i + 1;
      while (j < col.size() && !col[j].is_null &&
             col[j].frame_info == col[i].frame_info) {
        check(col[j]);
        ++j;
      }
      encode_run(col, i, j, out[0]);
      i = j;
    }
  }

 private:
  void check(const Element& f) const {
    SCA_CHECK(f.is_frame && f.frame_info.type == FrameType::U8,
              "ImageEncoder needs u8 frames");
    SCA_CHECK(f.device.is_gpu(), "GPU ImageEncoder needs GPU frame input");
  }

  void encode_run(const ElementVector& col, size_t i0, size_t i1,
                  ElementVector& out) {
    std::vector<const u8*> frames;
    for (size_t i = i0; i < i1; ++i) frames.push_back(col[i].buffer);
    const FrameInfo& fi = col[i0].frame_info;
    void* stream =
        config_.hip_stream ? config_.hip_stream : per_thread_hip_stream();
    std::vector<u8*> bufs;
    std::vector<u64> sizes;
    if (png_) {
      png_encode_gpu(frames, fi.shape[0], fi.shape[1], fi.shape[2],
                     config_.device, stream, bufs, sizes);
    } else {
      jpeg_encode_gpu(frames, fi.shape[0], fi.shape[1], fi.shape[2], quality_,
                      config_.device, stream, bufs, sizes, subsampling_);
    }
    for (size_t i = i0; i < i1; ++i) {
      Element& e = out[i];
      e.buffer = bufs[i - i0];
      e.size = sizes[i - i0];
      e.device = config_.device;
    }
    if (config_.profiler)
      config_.profiler->increment(
          png_ ? "png_gpu_encode_frames" : "jpeg_gpu_encode_frames",
          (i64)(i1 - i0));
  }

  bool png_ = false;
  i32 quality_ = 90;
  JpegSubsampling subsampling_ = JpegSubsampling::k444;
};

}  // namespace

void register_image_encoder_gpu() {
  static bool done = false;
  if (done) return;
  done = true;
  KernelFactory f;
  f.op_name = "ImageEncoder";
  f.device_type = DeviceType::GPU;
  f.preferred_batch = 8;
  f.make = [](const KernelConfig& c) -> std::unique_ptr<BaseKernel> {
    return std::make_unique<ImageEncoderKernelGPU>(c);
  };
  kernel_registry().add(f);
}

}  // namespace sca
