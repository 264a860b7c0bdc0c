// Baseline JPEG encoder arithmetic shared by the CPU encoder (jpeg_cpu.cpp)
// and the HIP encoder (kernels/jpeg_encode.hip). Written from ITU-T T.81 and
// the JFIF 1.02 specification; every function is integer-only, so the two
// encoders produce the same coefficients and the same codes by construction
// and differ only in how the bits are packed (sequentially vs in parallel).
//
// Format (fixed):
//   SOF0, 8 bit, JFIF APP0; 1 channel -> greyscale, 3 channels -> YCbCr
//   4:4:4 (full-range BT.601); Annex K quantisation tables scaled by the IJG
//   quality rule; the four Annex K Huffman tables; a DRI segment with a
//   restart interval of kJpegRestartInterval MCUs. Each restart segment
//   starts from DC prediction 0, is padded to a byte with 1-bits and is
//   byte-stuffed on its own; segments are separated by RST(n mod 8).
//
// 4:2:0 mode (JpegSubsampling::k420, 3 channels only; a 1-channel frame has
// no chroma and is written exactly as in 4:4:4):
//   SOF0 sampling factors Y 2x2, Cb 1x1, Cr 1x1. One MCU is 16x16 pixels and
//   6 blocks in the order Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr (T.81 A.2.3).
//   The restart interval is kJpegRestartInterval420 = 16 MCUs, 96 blocks, the
//   block count of a 4:4:4 segment; DRI carries 16. DC prediction is per
//   component and starts from 0 in each segment; Y chains through the four Y
//   blocks of an MCU and on into the next MCU. Pixel coordinates past the
//   right or bottom edge clamp to w-1 / h-1 before anything else, so a 1x1
//   image is one MCU of one replicated pixel. A chroma sample is the 2x2 box
//   mean jpeg_downsample4 of the Q4 samples jpeg_sample_rgb returns for the
//   four (clamped) pixels: (a + b + c + d + 2) >> 2, arithmetic shift, with
//   no 8-bit rounding of Cb/Cr before it. DCT, quantisation and entropy
//   coding are those of 4:4:4.
//
// Fixed-point pipeline of one 8x8 block:
//   sample  Q4   level-shifted component value (pixel - 128) * 16
//   row DCT Q4 * Q14 constants -> descaled to Q6 (fits int16)
//   col DCT Q6 * Q14 constants -> Q20 coefficient (|c| <= 2^30)
//   quant   round-half-away-from-zero division by q << 20
// The DCT is the orthonormal 8-point DCT-II of T.81 A.3.3 evaluated with
// the even/odd symmetry of the cosine basis (4+4 products per output).
#pragma once

#include <string>
#include <vector>

#include "../common.h"

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__
#else
#define JPEG_HD
#endif

namespace sca {

constexpr i32 kJpegRestartInterval = 32;     // MCUs per 4:4:4 segment
constexpr i32 kJpegRestartInterval420 = 16;  // MCUs per 4:2:0 segment
enum class JpegSubsampling : i32 { k444 = 0, k420 = 1 };
// Longest code of one block: DC 9 + 11 bits, 63 x (AC 16 + 10 bits) = 1658
// bits -> 208 bytes; every byte can be 0xFF and need a stuffed zero.
constexpr u32 kJpegBlockMaxBytes = 208;
constexpr u32 kJpegBlockMaxStuffed = 2 * kJpegBlockMaxBytes;

// Everything an encoder looks up, built once per (channels, quality) by
// jpeg_make_tables and read by both encoders.
struct JpegTables {
  u16 q[2][64];      // quantisation tables, natural (row-major) order
  u8 zz2nat[64];     // zig-zag position -> natural index
  u8 nat2zz[64];     // natural index -> zig-zag position
  u32 dc[2][16];     // DC Huffman: [category] -> length << 16 | code
  u32 ac[2][256];    // AC Huffman: [run << 4 | size] -> length << 16 | code
};

// ---- colour: full-range BT.601 in Q16, result Q4, level-shifted ----
// comp 0 = Y, 1 = Cb, 2 = Cr. Range: [-2048, 2040].
JPEG_HD inline i32 jpeg_sample_rgb(i32 r, i32 g, i32 b, int comp) {
  i32 v;
  if (comp == 0) {
    v = 19595 * r + 38470 * g + 7471 * b - (128 << 16);
  } else if (comp == 1) {
    v = -11059 * r - 21709 * g + 32768 * b;
  } else {
    v = 32768 * r - 27439 * g - 5329 * b;
  }
  return (v + 2048) >> 12;
}
JPEG_HD inline i32 jpeg_sample_grey(i32 y) { return (y - 128) * 16; }
// 4:2:0 chroma sample: box mean of the Q4 samples of one 2x2 pixel cell
JPEG_HD inline i32 jpeg_downsample4(i32 a, i32 b, i32 c, i32 d) {
  return (a + b + c + d + 2) >> 2;
}

// ---- 8-point DCT-II, orthonormal, constants in Q14 ----
// out[u] = sum_x in[x] * c(u)/2 * cos((2x+1) u pi / 16), not descaled.
// |in| <= 46340/2 keeps every sum inside 32 bits.
JPEG_HD inline void jpeg_dct8(const i32 (&in)[8], i32 (&out)[8]) {
  // round(8192 * cos(n pi / 16)), n = 1..7; n = 4 also serves c(0)/2
  constexpr i32 k1 = 8035, k2 = 7568, k3 = 6811, k4 = 5793, k5 = 4551,
                k6 = 3135, k7 = 1598;
  i32 s0 = in[0] + in[7], s1 = in[1] + in[6], s2 = in[2] + in[5],
      s3 = in[3] + in[4];
  i32 d0 = in[0] - in[7], d1 = in[1] - in[6], d2 = in[2] - in[5],
      d3 = in[3] - in[4];
  out[0] = k4 * (s0 + s1 + s2 + s3);
  out[4] = k4 * (s0 - s1 - s2 + s3);
  out[2] = k2 * (s0 - s3) + k6 * (s1 - s2);
  out[6] = k6 * (s0 - s3) - k2 * (s1 - s2);
  out[1] = k1 * d0 + k3 * d1 + k5 * d2 + k7 * d3;
  out[3] = k3 * d0 - k7 * d1 - k1 * d2 - k5 * d3;
  out[5] = k5 * d0 - k1 * d1 + k7 * d2 + k3 * d3;
  out[7] = k7 * d0 - k5 * d1 + k3 * d2 - k1 * d3;
}

// row pass result Q(4+14) -> Q6, round to nearest
JPEG_HD inline i32 jpeg_descale_row(i32 v) { return (v + (1 << 11)) >> 12; }

// Q20 coefficient / q, round half away from zero
JPEG_HD inline i32 jpeg_quantize(i32 v, u32 q) {
  u32 a = v < 0 ? (u32)(-v) : (u32)v;
  u32 r = (a + (q << 19)) / (q << 20);
  return v < 0 ? -(i32)r : (i32)r;
}

// ---- entropy coding ----
// size category of T.81 F.1.2.1: bits needed for |v|
JPEG_HD inline u32 jpeg_nbits(i32 v) {
  u32 a = v < 0 ? (u32)(-v) : (u32)v;
  return a ? 32u - (u32)__builtin_clz(a) : 0u;
}
// the n appended bits: v, or v - 1 in n-bit two's complement when negative
JPEG_HD inline u32 jpeg_value_bits(i32 v, u32 n) {
  return (u32)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
}

// Code one block of zig-zagged coefficients; emit(bits, length) is called
// once per symbol with the Huffman code and the value bits joined
// (length <= 26).
template <class Emit>
JPEG_HD inline void jpeg_code_block(const i16* zz, i32 pred, const u32* dc,
                                    const u32* ac, Emit& emit) {
  i32 diff = (i32)zz[0] - pred;
  u32 n = jpeg_nbits(diff);
  u32 e = dc[n];
  emit(((e & 0xffffu) << n) | jpeg_value_bits(diff, n), (e >> 16) + n);
  u32 run = 0;
  for (int k = 1; k < 64; ++k) {
    i32 v = zz[k];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run >= 16) {  // ZRL
      emit(ac[0xf0] & 0xffffu, ac[0xf0] >> 16);
      run -= 16;
    }
    n = jpeg_nbits(v);
    e = ac[(run << 4) | n];
    emit(((e & 0xffffu) << n) | jpeg_value_bits(v, n), (e >> 16) + n);
    run = 0;
  }
  if (run) emit(ac[0] & 0xffffu, ac[0] >> 16);  // EOB
}

// ---- geometry ----
struct JpegGeom {
  i32 h, w, c;
  u32 mcus_x, mcus_y, nmcu, nseg;
  u32 seg_stride;  // worst-case bytes of one stuffed restart segment
  u32 mcu_px;      // MCU width and height in pixels: 8, or 16 in 4:2:0
  u32 mcu_blocks;  // blocks per MCU: c, or 6 in 4:2:0
  u32 restart;     // MCUs per restart segment
  JpegSubsampling ss;  // the mode in effect: k444 for every 1-channel frame
};
JPEG_HD inline JpegGeom jpeg_geom(
    i32 h, i32 w, i32 c, JpegSubsampling ss = JpegSubsampling::k444) {
  JpegGeom g;
  g.h = h;
  g.w = w;
  g.c = c;
  bool sub = ss == JpegSubsampling::k420 && c == 3;
  g.ss = sub ? JpegSubsampling::k420 : JpegSubsampling::k444;
  g.mcu_px = sub ? 16 : 8;
  g.mcu_blocks = sub ? 6 : (u32)c;
  g.restart = (u32)(sub ? kJpegRestartInterval420 : kJpegRestartInterval);
  g.mcus_x = ((u32)w + g.mcu_px - 1) / g.mcu_px;
  g.mcus_y = ((u32)h + g.mcu_px - 1) / g.mcu_px;
  g.nmcu = g.mcus_x * g.mcus_y;
  g.nseg = (g.nmcu + g.restart - 1) / g.restart;
  g.seg_stride = g.restart * g.mcu_blocks * kJpegBlockMaxStuffed;
  return g;
}

// ---- host API (jpeg_cpu.cpp) ----
void jpeg_make_tables(i32 c, i32 quality, JpegTables& t);
// "444" | "420" -> mode; anything else (4:2:2 included) is an error that
// lists the supported values
JpegSubsampling jpeg_parse_subsampling(const std::string& name);
// SOI .. SOS, the same for every frame of one shape, quality and mode
std::vector<u8> jpeg_header(i32 h, i32 w, i32 c, const JpegTables& t,
                            JpegSubsampling ss = JpegSubsampling::k444);
// Header, worst-case entropy bytes (stuffing included), restart markers
// and EOI: no h x w x c frame encodes to more.
u64 jpeg_size_bound(i32 h, i32 w, i32 c,
                    JpegSubsampling ss = JpegSubsampling::k444);
// Quantised coefficients of component `comp` of block (bx, by) of the
// full-resolution 8x8 block grid, zig-zag order; pixels past the
// right/bottom edge replicate the last column/row. The Y blocks of a 4:2:0
// file are these too: MCU (mx, my) holds blocks (2mx + j, 2my + i).
void jpeg_block_coefs(const u8* pix, i32 h, i32 w, i32 c, u32 bx, u32 by,
                      int comp, const JpegTables& t, i16 (&zz)[64]);
// The same for a 4:2:0 chroma block: (bx, by) counts blocks of 8x8 chroma
// samples, i.e. 16x16 pixels; comp is 1 (Cb) or 2 (Cr); 3-channel frames.
void jpeg_block_coefs_420(const u8* pix, i32 h, i32 w, u32 bx, u32 by,
                          int comp, const JpegTables& t, i16 (&zz)[64]);
std::vector<u8> jpeg_encode_cpu(const u8* pix, i32 h, i32 w, i32 c,
                                i32 quality,
                                JpegSubsampling ss = JpegSubsampling::k444);
void jpeg_check_args(i32 h, i32 w, i32 c, i32 quality);

// ---- HIP encoder (kernels/jpeg_encode.hip) ----
// Encodes same-shape device frames; out[i] is a device buffer of exactly
// sizes[i] bytes holding the file jpeg_encode_cpu would produce. The
// buffers of one call share block buffers: release each with
// delete_buffer(dev, out[i]). Everything is issued on `stream`.
void jpeg_encode_gpu(const std::vector<const u8*>& frames, i32 h, i32 w,
                     i32 c, i32 quality, DeviceHandle dev, void* stream,
                     std::vector<u8*>& out, std::vector<u64>& sizes,
                     JpegSubsampling ss = JpegSubsampling::k444);

}  // namespace sca
