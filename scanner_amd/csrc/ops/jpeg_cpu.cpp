// Sequential baseline JPEG encoder: the definition of the bytes the HIP
// encoder (kernels/jpeg_encode.hip) has to reproduce. Format and arithmetic:
// jpeg_common.h. Tables are those of ITU-T T.81 Annex K.
#include "jpeg_common.h"

#include <algorithm>

namespace sca {

namespace {

// T.81 Table K.1 / K.2, natural order
const u8 kQuantLuma[64] = {
    16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
    14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
    18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const u8 kQuantChroma[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// T.81 Figure A.6
const u8 kZigzag[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Tables K.3 - K.6: BITS (codes per length 1..16) and HUFFVAL
const u8 kDcBits[2][16] = {
    {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const u8 kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const u8 kAcBits[2][16] = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const u8 kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06,
     0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
     0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
     0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4,
     0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41,
     0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
     0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
     0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4,
     0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// T.81 Annex C: canonical codes from BITS/HUFFVAL, as length << 16 | code
void huff_codes(const u8* bits, const u8* vals, u32* table) {
  u32 code = 0;
  int k = 0;
  for (u32 len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = len << 16 | code++;
    code <<= 1;
  }
}

void put16(std::vector<u8>& v, u32 x) {
  v.push_back((u8)(x >> 8));
  v.push_back((u8)x);
}

void put_dht(std::vector<u8>& v, u8 tc_th, const u8* bits, const u8* vals,
             int nvals) {
  put16(v, 0xffc4);
  put16(v, 2 + 1 + 16 + nvals);
  v.push_back(tc_th);
  v.insert(v.end(), bits, bits + 16);
  v.insert(v.end(), vals, vals + nvals);
}

// MSB-first bit writer of one restart segment, stuffing as it goes
struct BitWriter {
  std::vector<u8>& out;
  u64 acc = 0;  // low `n` bits pending
  u32 n = 0;
  void operator()(u32 bits, u32 len) {
    acc = (acc << len) | bits;
    n += len;
    while (n >= 8) {
      u8 b = (u8)(acc >> (n - 8));
      out.push_back(b);
      if (b == 0xff) out.push_back(0);
      n -= 8;
    }
  }
  void flush() {  // pad to a byte with 1-bits
    if (n) (*this)((1u << (8 - n)) - 1u, 8 - n);
  }
};

}  // namespace

void jpeg_check_args(i32 h, i32 w, i32 c, i32 quality) {
  SCA_CHECK(c == 1 || c == 3, "JPEG encoder supports 1- or 3-channel u8");
  SCA_CHECK(h >= 1 && w >= 1 && h <= 65535 && w <= 65535,
            "JPEG encoder needs 1..65535 rows and columns");
  SCA_CHECK(quality >= 1 && quality <= 100,
            "JPEG quality must be in 1..100, got " + std::to_string(quality));
}

void jpeg_make_tables(i32 c, i32 quality, JpegTables& t) {
  SCA_CHECK(quality >= 1 && quality <= 100,
            "JPEG quality must be in 1..100, got " + std::to_string(quality));
  t = JpegTables{};
  i32 s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    for (int k = 0; k < 2; ++k) {
      i32 v = ((k ? kQuantChroma[i] : kQuantLuma[i]) * s + 50) / 100;
      t.q[k][i] = (u16)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
    t.zz2nat[i] = kZigzag[i];
    t.nat2zz[kZigzag[i]] = (u8)i;
  }
  for (int k = 0; k < (c == 3 ? 2 : 1); ++k) {
    huff_codes(kDcBits[k], kDcVals, t.dc[k]);
    huff_codes(kAcBits[k], kAcVals[k], t.ac[k]);
  }
}

JpegSubsampling jpeg_parse_subsampling(const std::string& name) {
  if (name == "444") return JpegSubsampling::k444;
  if (name == "420") return JpegSubsampling::k420;
  throw ScannerError("JPEG subsampling must be one of '444', '420', got '" +
                     name + "'");
}

std::vector<u8> jpeg_header(i32 h, i32 w, i32 c, const JpegTables& t,
                            JpegSubsampling ss) {
  JpegGeom g = jpeg_geom(h, w, c, ss);
  int ntab = c == 3 ? 2 : 1;
  std::vector<u8> v;
  put16(v, 0xffd8);  // SOI
  put16(v, 0xffe0);  // APP0: JFIF 1.01, no density unit, 1:1, no thumbnail
  put16(v, 16);
  const u8 jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  v.insert(v.end(), jfif, jfif + 14);
  for (int k = 0; k < ntab; ++k) {  // DQT, 8-bit entries in zig-zag order
    put16(v, 0xffdb);
    put16(v, 2 + 1 + 64);
    v.push_back((u8)k);
    for (int i = 0; i < 64; ++i) v.push_back((u8)t.q[k][t.zz2nat[i]]);
  }
  put16(v, 0xffc0);  // SOF0
  put16(v, 8 + 3 * c);
  v.push_back(8);
  put16(v, (u32)h);
  put16(v, (u32)w);
  v.push_back((u8)c);
  for (int i = 0; i < c; ++i) {
    v.push_back((u8)(i + 1));      // component id
    // sampling factors: 1x1, or 2x2 for the Y of a 4:2:0 file
    v.push_back(i == 0 && g.ss == JpegSubsampling::k420 ? 0x22 : 0x11);
    v.push_back(i == 0 ? 0 : 1);   // quantisation table
  }
  for (int k = 0; k < ntab; ++k) {
    put_dht(v, (u8)k, kDcBits[k], kDcVals, 12);
    put_dht(v, (u8)(0x10 | k), kAcBits[k], kAcVals[k], 162);
  }
  put16(v, 0xffdd);  // DRI
  put16(v, 4);
  put16(v, g.restart);
  put16(v, 0xffda);  // SOS
  put16(v, 6 + 2 * c);
  v.push_back((u8)c);
  for (int i = 0; i < c; ++i) {
    v.push_back((u8)(i + 1));
    v.push_back(i == 0 ? 0x00 : 0x11);  // DC/AC Huffman tables
  }
  v.push_back(0);   // Ss
  v.push_back(63);  // Se
  v.push_back(0);   // Ah/Al
  return v;
}

u64 jpeg_size_bound(i32 h, i32 w, i32 c, JpegSubsampling ss) {
  jpeg_check_args(h, w, c, 50);
  JpegTables t;
  jpeg_make_tables(c, 50, t);
  JpegGeom g = jpeg_geom(h, w, c, ss);
  // every segment is followed by a 2-byte marker (RSTn or EOI)
  return jpeg_header(h, w, c, t, ss).size() +
         (u64)g.nmcu * g.mcu_blocks * kJpegBlockMaxStuffed + 2ull * g.nseg;
}

namespace {

// row-pass results (Q6) -> column DCT, quantisation, zig-zag
void column_pass(const i32 (&rows)[8][8], int comp, const JpegTables& t,
                 i16 (&zz)[64]) {
  const u16* q = t.q[comp ? 1 : 0];
  for (int u = 0; u < 8; ++u) {
    i32 in[8], out[8];
    for (int r = 0; r < 8; ++r) in[r] = rows[r][u];
    jpeg_dct8(in, out);
    for (int v = 0; v < 8; ++v) {
      int nat = v * 8 + u;
      zz[t.nat2zz[nat]] = (i16)jpeg_quantize(out[v], q[nat]);
    }
  }
}

}  // namespace

void jpeg_block_coefs(const u8* pix, i32 h, i32 w, i32 c, u32 bx, u32 by,
                      int comp, const JpegTables& t, i16 (&zz)[64]) {
  i32 rows[8][8];
  for (int r = 0; r < 8; ++r) {
    i32 y = std::min<i32>((i32)by * 8 + r, h - 1);
    i32 in[8], out[8];
    for (int k = 0; k < 8; ++k) {
      i32 x = std::min<i32>((i32)bx * 8 + k, w - 1);
      const u8* p = pix + ((size_t)y * w + x) * c;
      in[k] = c == 1 ? jpeg_sample_grey(p[0])
                     : jpeg_sample_rgb(p[0], p[1], p[2], comp);
    }
    jpeg_dct8(in, out);
    for (int u = 0; u < 8; ++u) rows[r][u] = jpeg_descale_row(out[u]);
  }
  column_pass(rows, comp, t, zz);
}

void jpeg_block_coefs_420(const u8* pix, i32 h, i32 w, u32 bx, u32 by,
                          int comp, const JpegTables& t, i16 (&zz)[64]) {
  i32 rows[8][8];
  for (int r = 0; r < 8; ++r) {
    i32 y0 = std::min<i32>(((i32)by * 8 + r) * 2, h - 1);
    i32 y1 = std::min<i32>(((i32)by * 8 + r) * 2 + 1, h - 1);
    i32 in[8], out[8];
    for (int k = 0; k < 8; ++k) {
      i32 x0 = std::min<i32>(((i32)bx * 8 + k) * 2, w - 1);
      i32 x1 = std::min<i32>(((i32)bx * 8 + k) * 2 + 1, w - 1);
      auto sample = [&](i32 y, i32 x) {
        const u8* p = pix + ((size_t)y * w + x) * 3;
        return jpeg_sample_rgb(p[0], p[1], p[2], comp);
      };
      in[k] = jpeg_downsample4(sample(y0, x0), sample(y0, x1), sample(y1, x0),
                               sample(y1, x1));
    }
    jpeg_dct8(in, out);
    for (int u = 0; u < 8; ++u) rows[r][u] = jpeg_descale_row(out[u]);
  }
  column_pass(rows, comp, t, zz);
}

std::vector<u8> jpeg_encode_cpu(const u8* pix, i32 h, i32 w, i32 c,
                                i32 quality, JpegSubsampling ss) {
  jpeg_check_args(h, w, c, quality);
  JpegTables t;
  jpeg_make_tables(c, quality, t);
  JpegGeom g = jpeg_geom(h, w, c, ss);
  std::vector<u8> out = jpeg_header(h, w, c, t, ss);
  i16 zz[64];
  for (u32 s = 0; s < g.nseg; ++s) {
    BitWriter bw{out};
    i32 pred[3] = {0, 0, 0};
    u32 m1 = std::min<u32>(g.nmcu, (s + 1) * g.restart);
    for (u32 m = s * g.restart; m < m1; ++m) {
      u32 mx = m % g.mcus_x, my = m / g.mcus_x;
      if (g.ss == JpegSubsampling::k420) {
        // Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr
        for (u32 k = 0; k < 6; ++k) {
          int comp = k < 4 ? 0 : (int)k - 3;
          if (k < 4) {
            jpeg_block_coefs(pix, h, w, c, 2 * mx + (k & 1), 2 * my + (k >> 1),
                             0, t, zz);
          } else {
            jpeg_block_coefs_420(pix, h, w, mx, my, comp, t, zz);
          }
          int tab = comp ? 1 : 0;
          jpeg_code_block(zz, pred[comp], t.dc[tab], t.ac[tab], bw);
          pred[comp] = zz[0];
        }
        continue;
      }
      for (int comp = 0; comp < c; ++comp) {
        jpeg_block_coefs(pix, h, w, c, mx, my, comp, t, zz);
        int k = comp ? 1 : 0;
        jpeg_code_block(zz, pred[comp], t.dc[k], t.ac[k], bw);
        pred[comp] = zz[0];
      }
    }
    bw.flush();
    put16(out, s + 1 < g.nseg ? 0xffd0 + (s & 7) : 0xffd9);  // RSTn / EOI
  }
  return out;
}

}  // namespace sca
