// Baseline JPEG decoder arithmetic shared by the CPU decoder
// (jpeg_decode_cpu.cpp) and the HIP decoder (kernels/jpeg_decode.hip).
// Written from ITU-T T.81 and the JFIF 1.02 specification; every function is
// integer-only, so the two decoders produce the same pixels by construction
// and differ only in which lane runs which restart segment.
//
// Pipeline of one 8x8 block:
//   entropy   jpeg_decode_block: Huffman codes (arbitrary DHT tables, T.81
//             F.2.2.3 min/max-code form) -> quantised int16 coefficients in
//             natural (row-major) order
//   dequant   coefficient * q in i32, clamped to +-kJpegCoefLimit
//   IDCT      orthonormal 8-point DCT-III on columns, then on rows, the
//             Q14 constants of jpeg_common.h; the first pass is descaled to
//             Q2
//   output    + 128, round to nearest, clamp to u8
// then per pixel: triangle-filter chroma upsampling (2x1, 2x2) and
// full-range BT.601 YCbCr -> RGB in Q16.
//
// Nothing here reads outside the [begin, end) byte range of the segment it
// is given, or writes outside the 64-entry block it is given, whatever the
// input bytes are.
#pragma once

#include "jpeg_common.h"

#if defined(__HIPCC__)
#define JPEG_UNROLL _Pragma("unroll")
#else
#define JPEG_UNROLL
#endif

namespace sca {

// ---- bit reader over one entropy-coded segment ----
// Bytes [pos, end) of `p`, MSB first. FF 00 is the data byte FF (T.81 B.1.1.5);
// an FF followed by anything else is taken as the data byte FF. Past `end`
// the reader supplies 1-bits; `exhausted` is set once such a bit has been
// consumed (not merely prefetched).
struct JpegBitReader {
  const u8* p;
  u32 pos, end;
  u32 acc;      // next bits, left-aligned
  u32 n;        // bits held in acc
  u32 phantom;  // how many of them (the last ones) lie past `end`
  bool exhausted;
};

JPEG_HD inline void jpeg_bits_init(JpegBitReader& br, const u8* p, u32 begin,
                                   u32 end) {
  br.p = p;
  br.pos = begin;
  br.end = end;
  br.acc = 0;
  br.n = 0;
  br.phantom = 0;
  br.exhausted = false;
}

// at least 25 bits in acc afterwards
JPEG_HD inline void jpeg_bits_fill(JpegBitReader& br) {
  while (br.n <= 24) {
    u32 b = 0xffu;
    if (br.pos < br.end) {
      b = br.p[br.pos++];
      if (b == 0xffu && br.pos < br.end && br.p[br.pos] == 0) ++br.pos;
    } else {
      br.phantom += 8;
    }
    br.acc |= b << (24 - br.n);
    br.n += 8;
  }
}

// the next `k` bits (k <= 16) without consuming them; needs a prior fill
JPEG_HD inline u32 jpeg_bits_peek(const JpegBitReader& br, u32 k) {
  return k ? br.acc >> (32 - k) : 0u;
}

JPEG_HD inline void jpeg_bits_skip(JpegBitReader& br, u32 k) {
  br.acc = k < 32 ? br.acc << k : 0u;
  br.n -= k;
  if (br.n < br.phantom) {
    br.exhausted = true;
    br.phantom = br.n;
  }
}

// ---- Huffman table, T.81 F.2.2.3 ----
// The min/max-code form with the maxima left-aligned to 16 bits: the next 16
// bits `look` start with a code of length l when look < limit[l], where
// limit[l] = (MAXCODE(l) + 1) << (16 - l), or limit[l - 1] when no code has
// length l. Canonical codes make the limits non-decreasing, so the length is
// 1 + the number of limits that look has reached: sixteen independent
// compares instead of a search loop with a load and a branch per length. The
// value is vals[code + delta[l]] with delta = VALPTR - MINCODE. Built and
// validated by jpeg_build_huff.
struct JpegHuff {
  u32 limit[17];
  i32 delta[17];
  u8 vals[256];
};

// BITS (16 counts) and HUFFVAL -> table. False when the counts describe more
// than 256 values or more codes than a length can hold (T.81 Annex C).
JPEG_HD inline bool jpeg_build_huff(const u8* bits, const u8* vals, u32 nvals,
                                    JpegHuff& t) {
  u32 total = 0;
  for (int l = 1; l <= 16; ++l) total += bits[l - 1];
  if (total > 256 || total != nvals) return false;
  u32 code = 0, k = 0;
  t.limit[0] = 0;
  t.delta[0] = 0;
  for (u32 l = 1; l <= 16; ++l) {
    u32 cnt = bits[l - 1];
    if (code + cnt > (1u << l)) return false;
    t.delta[l] = (i32)k - (i32)code;
    t.limit[l] = cnt ? (code + cnt) << (16 - l) : t.limit[l - 1];
    k += cnt;
    code = (code + cnt) << 1;
  }
  for (u32 i = 0; i < 256; ++i) t.vals[i] = i < nvals ? vals[i] : 0;
  return true;
}

// One symbol; -1 when no code of any length matches the next 16 bits.
JPEG_HD inline i32 jpeg_huff_symbol(JpegBitReader& br, const JpegHuff& t) {
  jpeg_bits_fill(br);
  u32 look = jpeg_bits_peek(br, 16);
  u32 len = 1;
  JPEG_UNROLL
  for (u32 l = 1; l <= 16; ++l) len += look >= t.limit[l] ? 1u : 0u;
  if (len > 16) {
    // the 1-bits supplied past the end match no code: that is exhaustion
    if (br.n - br.phantom < 16) br.exhausted = true;
    return -1;
  }
  u32 idx = (u32)((i32)(look >> (16 - len)) + t.delta[len]);
  if (idx > 255u) return -1;
  jpeg_bits_skip(br, len);
  return t.vals[idx];
}

// s additional bits (s <= 15) as a signed value, T.81 F.2.2.1 EXTEND
JPEG_HD inline i32 jpeg_receive_extend(JpegBitReader& br, u32 s) {
  if (s == 0) return 0;
  jpeg_bits_fill(br);
  i32 v = (i32)jpeg_bits_peek(br, s);
  jpeg_bits_skip(br, s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

enum JpegBlockStatus : u32 {
  kJpegBlockOk = 0,
  kJpegBadCode = 1,    // no Huffman code matches, or an impossible size
  kJpegBadIndex = 2,   // a run takes the coefficient index past 63
  kJpegExhausted = 3,  // the segment ended before the block did
};

JPEG_HD inline i32 jpeg_clamp_i16(i32 v) {
  return v < -32768 ? -32768 : v > 32767 ? 32767 : v;
}

// Decode one block into out[64] (natural order, zeroed by the caller).
// `pred` is the component's DC predictor; it is kept inside int16, which no
// valid stream leaves. At most 64 symbols are read. On an error nothing more
// is decoded and the returned status says why.
JPEG_HD inline u32 jpeg_decode_block(JpegBitReader& br, const JpegHuff& dc,
                                     const JpegHuff& ac, const u8* zz2nat,
                                     i32& pred, i16* out) {
  i32 s = jpeg_huff_symbol(br, dc);
  if (s < 0 || s > 15) return br.exhausted ? kJpegExhausted : kJpegBadCode;
  pred = jpeg_clamp_i16(pred + jpeg_receive_extend(br, (u32)s));
  if (br.exhausted) return kJpegExhausted;
  out[0] = (i16)pred;
  u32 k = 1;
  while (k < 64) {
    i32 rs = jpeg_huff_symbol(br, ac);
    if (rs < 0) return br.exhausted ? kJpegExhausted : kJpegBadCode;
    u32 r = (u32)rs >> 4, sz = (u32)rs & 15u;
    if (sz == 0) {
      if (r != 15) {  // EOB (runs 1..14 with size 0 are not baseline codes)
        if (r != 0) return kJpegBadCode;
        break;
      }
      k += 16;  // ZRL
      if (k > 64) return kJpegBadIndex;
      continue;
    }
    k += r;
    if (k > 63) return kJpegBadIndex;
    i32 v = jpeg_receive_extend(br, sz);
    if (br.exhausted) return kJpegExhausted;
    out[zz2nat[k]] = (i16)v;
    ++k;
  }
  return br.exhausted ? kJpegExhausted : kJpegBlockOk;
}

// ---- dequantisation ----
// |coefficient| <= 32768 and q <= 65535, so the product fits i32 exactly.
// An orthonormal DCT of 8-bit samples has |F| <= 1024; the product is
// clamped to +-4096, four times that, which a valid file cannot reach with a
// table below 6144 and which keeps every sum of the IDCT inside 32 bits.
constexpr i32 kJpegCoefLimit = 4096;
JPEG_HD inline i32 jpeg_dequant(i32 coef, u32 q) {
  i32 v = coef * (i32)q;
  return v < -kJpegCoefLimit ? -kJpegCoefLimit
                             : v > kJpegCoefLimit ? kJpegCoefLimit : v;
}

// ---- 8-point DCT-III (inverse of jpeg_dct8), constants in Q14 ----
// out[x] = sum_u in[u] * c(u)/2 * cos((2x+1) u pi / 16) * 2^14, not descaled.
// |out| <= max|in| * 43284, so |in| <= 49613 keeps it inside 32 bits.
JPEG_HD inline void jpeg_idct8(const i32 (&in)[8], i32 (&out)[8]) {
  constexpr i32 k1 = 8035, k2 = 7568, k3 = 6811, k4 = 5793, k5 = 4551,
                k6 = 3135, k7 = 1598;
  i32 e0 = k4 * (in[0] + in[4]), e1 = k4 * (in[0] - in[4]);
  i32 e2 = k2 * in[2] + k6 * in[6], e3 = k6 * in[2] - k2 * in[6];
  i32 a0 = e0 + e2, a1 = e1 + e3, a2 = e1 - e3, a3 = e0 - e2;
  i32 o0 = k1 * in[1] + k3 * in[3] + k5 * in[5] + k7 * in[7];
  i32 o1 = k3 * in[1] - k7 * in[3] - k1 * in[5] - k5 * in[7];
  i32 o2 = k5 * in[1] - k1 * in[3] + k7 * in[5] + k3 * in[7];
  i32 o3 = k7 * in[1] - k5 * in[3] + k3 * in[5] - k1 * in[7];
  out[0] = a0 + o0;
  out[7] = a0 - o0;
  out[1] = a1 + o1;
  out[6] = a1 - o1;
  out[2] = a2 + o2;
  out[5] = a2 - o2;
  out[3] = a3 + o3;
  out[4] = a3 - o3;
}

// first pass Q14 -> Q2: |v| <= 4096 * 43284 gives |result| <= 43285
JPEG_HD inline i32 jpeg_idct_descale_first(i32 v) {
  return (v + (1 << 11)) >> 12;
}
// second pass Q16 -> u8 with the level shift: 43285 * 43284 + (128 << 16) +
// 2^15 < 2^31
JPEG_HD inline u8 jpeg_idct_sample(i32 v) {
  i32 s = (v + (128 << 16) + (1 << 15)) >> 16;
  return (u8)(s < 0 ? 0 : s > 255 ? 255 : s);
}

// Dequantised (already clamped by jpeg_dequant) natural-order block -> 8x8
// u8 samples, row-major. Columns first, so that the second pass finishes one
// output row at a time (the HIP decoder stores each row as it is produced).
JPEG_HD inline void jpeg_idct_block(const i32 (&deq)[64], u8 (&pix)[64]) {
  i32 tmp[64];
  JPEG_UNROLL
  for (int u = 0; u < 8; ++u) {
    i32 in[8], out[8];
    JPEG_UNROLL
    for (int v = 0; v < 8; ++v) in[v] = deq[v * 8 + u];
    jpeg_idct8(in, out);
    JPEG_UNROLL
    for (int y = 0; y < 8; ++y) tmp[y * 8 + u] = jpeg_idct_descale_first(out[y]);
  }
  JPEG_UNROLL
  for (int y = 0; y < 8; ++y) {
    i32 in[8], out[8];
    JPEG_UNROLL
    for (int u = 0; u < 8; ++u) in[u] = tmp[y * 8 + u];
    jpeg_idct8(in, out);
    JPEG_UNROLL
    for (int x = 0; x < 8; ++x) pix[y * 8 + x] = jpeg_idct_sample(out[x]);
  }
}

// ---- chroma upsampling, triangle filter ----
// Sample of a chroma plane (stride bytes per row, valid extent cw x ch) at
// output pixel (x, y) for luma sampling hs x vs (1x1, 2x1 or 2x2) against
// 1x1 chroma. Neighbours outside the valid extent replicate its edge.
JPEG_HD inline i32 jpeg_upsample_at(const u8* plane, u32 stride, u32 cw,
                                    u32 ch, u32 hs, u32 vs, u32 x, u32 y) {
  if (hs == 1) return plane[(size_t)y * stride + x];  // vs == 1 as well
  u32 cx = x >> 1;
  if (vs == 1) {  // h2v1
    const u8* row = plane + (size_t)y * stride;
    i32 p = row[cx];
    if (x & 1) {
      if (cx + 1 >= cw) return p;
      return (3 * p + row[cx + 1] + 2) >> 2;
    }
    if (cx == 0) return p;
    return (3 * p + row[cx - 1] + 1) >> 2;
  }
  // h2v2: vertical pass t = 3 * near + far, then horizontal
  u32 cy = y >> 1;
  u32 fy = (y & 1) ? (cy + 1 < ch ? cy + 1 : cy) : (cy ? cy - 1 : 0);
  const u8* nr = plane + (size_t)cy * stride;
  const u8* fr = plane + (size_t)fy * stride;
  i32 t = 3 * nr[cx] + fr[cx];
  if (x & 1) {
    if (cx + 1 >= cw) return (4 * t + 7) >> 4;
    i32 tr = 3 * nr[cx + 1] + fr[cx + 1];
    return (3 * t + tr + 7) >> 4;
  }
  if (cx == 0) return (4 * t + 8) >> 4;
  i32 tl = 3 * nr[cx - 1] + fr[cx - 1];
  return (3 * t + tl + 8) >> 4;
}

// ---- colour: full-range BT.601 (JFIF), Q16, round to nearest, clamp ----
JPEG_HD inline u8 jpeg_clamp_u8(i32 v) {
  return (u8)(v < 0 ? 0 : v > 255 ? 255 : v);
}
JPEG_HD inline void jpeg_ycc_to_rgb(i32 y, i32 cb, i32 cr, u8* rgb) {
  cb -= 128;
  cr -= 128;
  rgb[0] = jpeg_clamp_u8(y + ((91881 * cr + 32768) >> 16));
  rgb[1] = jpeg_clamp_u8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = jpeg_clamp_u8(y + ((116130 * cb + 32768) >> 16));
}

// ---- geometry of a parsed file ----
// Component planes are padded to whole MCUs, so every decoded block lies
// inside its plane; the valid chroma extent is what the upsampler filters.
struct JpegDecGeom {
  i32 h, w, nc;          // nc: 1 (grey) or 3 (YCbCr)
  u32 hs, vs;            // luma sampling factors; chroma is 1x1
  u32 mcus_x, mcus_y, nmcu;
  u32 blocks_per_mcu;    // hs * vs + 2, or 1
  u32 y_stride, y_rows;  // luma plane, bytes
  u32 c_stride, c_rows;  // each chroma plane
  u32 cw, ch;            // valid chroma extent
};
JPEG_HD inline JpegDecGeom jpeg_dec_geom(i32 h, i32 w, i32 nc, u32 hs,
                                         u32 vs) {
  JpegDecGeom g;
  g.h = h;
  g.w = w;
  g.nc = nc;
  if (nc == 1) hs = vs = 1;  // a single-component scan is never interleaved
  g.hs = hs;
  g.vs = vs;
  g.mcus_x = ((u32)w + 8 * hs - 1) / (8 * hs);
  g.mcus_y = ((u32)h + 8 * vs - 1) / (8 * vs);
  g.nmcu = g.mcus_x * g.mcus_y;
  g.blocks_per_mcu = nc == 1 ? 1 : hs * vs + 2;
  g.y_stride = g.mcus_x * 8 * hs;
  g.y_rows = g.mcus_y * 8 * vs;
  g.c_stride = nc == 1 ? 0 : g.mcus_x * 8;
  g.c_rows = nc == 1 ? 0 : g.mcus_y * 8;
  g.cw = ((u32)w + hs - 1) / hs;
  g.ch = ((u32)h + vs - 1) / vs;
  return g;
}

// Block b of MCU m: component and the top-left sample of the block in that
// component's plane.
JPEG_HD inline void jpeg_block_pos(const JpegDecGeom& g, u32 m, u32 b,
                                   u32& comp, u32& px, u32& py) {
  u32 mx = m % g.mcus_x, my = m / g.mcus_x;
  u32 ny = g.hs * g.vs;
  if (g.nc == 1 || b < ny) {
    comp = 0;
    px = (mx * g.hs + b % g.hs) * 8;
    py = (my * g.vs + b / g.hs) * 8;
  } else {
    comp = b - ny + 1;
    px = mx * 8;
    py = my * 8;
  }
}

// Output pixel (x, y) of a 3-component image from its planes.
JPEG_HD inline void jpeg_pixel_rgb(const JpegDecGeom& g, const u8* yp,
                                   const u8* cbp, const u8* crp, u32 x, u32 y,
                                   u8* rgb) {
  i32 yy = yp[(size_t)y * g.y_stride + x];
  i32 cb = jpeg_upsample_at(cbp, g.c_stride, g.cw, g.ch, g.hs, g.vs, x, y);
  i32 cr = jpeg_upsample_at(crp, g.c_stride, g.cw, g.ch, g.hs, g.vs, x, y);
  jpeg_ycc_to_rgb(yy, cb, cr, rgb);
}

}  // namespace sca
