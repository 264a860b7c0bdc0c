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

constexpr i32 kJpegRestartInterval = 32;  // MCUs per restart segment
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
};
JPEG_HD inline JpegGeom jpeg_geom(i32 h, i32 w, i32 c) {
  JpegGeom g;
  g.h = h;
  g.w = w;
  g.c = c;
  g.mcus_x = ((u32)w + 7) / 8;
  g.mcus_y = ((u32)h + 7) / 8;
  g.nmcu = g.mcus_x * g.mcus_y;
  g.nseg = (g.nmcu + kJpegRestartInterval - 1) / kJpegRestartInterval;
  g.seg_stride = kJpegRestartInterval * (u32)c * kJpegBlockMaxStuffed;
  return g;
}

// ---- host API (jpeg_cpu.cpp) ----
void jpeg_make_tables(i32 c, i32 quality, JpegTables& t);
// SOI .. SOS, the same for every frame of one shape and quality
std::vector<u8> jpeg_header(i32 h, i32 w, i32 c, const JpegTables& t);
// Header, worst-case entropy bytes (stuffing included), restart markers
// and EOI: no h x w x c frame encodes to more.
u64 jpeg_size_bound(i32 h, i32 w, i32 c);
// Quantised coefficients of component `comp` of block (bx, by), zig-zag
// order; pixels past the right/bottom edge replicate the last column/row.
void jpeg_block_coefs(const u8* pix, i32 h, i32 w, i32 c, u32 bx, u32 by,
                      int comp, const JpegTables& t, i16 (&zz)[64]);
std::vector<u8> jpeg_encode_cpu(const u8* pix, i32 h, i32 w, i32 c,
                                i32 quality);
void jpeg_check_args(i32 h, i32 w, i32 c, i32 quality);

// ---- HIP encoder (kernels/jpeg_encode.hip) ----
// Encodes same-shape device frames; out[i] is a device buffer of exactly
// sizes[i] bytes holding the file jpeg_encode_cpu would produce. The
// buffers of one call share block buffers: release each with
// delete_buffer(dev, out[i]). Everything is issued on `stream`.
void jpeg_encode_gpu(const std::vector<const u8*>& frames, i32 h, i32 w,
                     i32 c, i32 quality, DeviceHandle dev, void* stream,
                     std::vector<u8*>& out, std::vector<u64>& sizes);

}  // namespace sca
