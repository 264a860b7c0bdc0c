// PNG reader for the ImageDecoder op, over the system zlib: 8-bit grey, RGB
// and RGBA (alpha dropped), non-interlaced, any number of IDAT chunks, all
// five scanline filters; chunk lengths and CRCs are verified. Written from
// the PNG specification (ISO/IEC 15948). HIP-free.
#include <zlib.h>

#include "image_decode.h"

namespace sca {

namespace {

const u8 kPngMagic[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};

u32 be32(const u8* p) {
  return (u32)p[0] << 24 | (u32)p[1] << 16 | (u32)p[2] << 8 | p[3];
}

struct PngHeader {
  i32 h, w;
  int channels;  // in the file: 1, 3 or 4
};

// One chunk at `pos`: checks length and CRC, returns the payload.
const u8* read_chunk(const u8* d, size_t n, size_t& pos, u32& len,
                     char (&type)[5]) {
  SCA_CHECK(pos + 12 <= n, "truncated PNG: chunk header runs past the end");
  len = be32(d + pos);
  SCA_CHECK(len <= 0x7fffffffu && (size_t)len <= n - pos - 12,
            "truncated PNG: chunk length runs past the end");
  for (int i = 0; i < 4; ++i) type[i] = (char)d[pos + 4 + i];
  type[4] = 0;
  u32 crc = (u32)crc32(crc32(0L, Z_NULL, 0), d + pos + 4, (uInt)(4 + len));
  SCA_CHECK(crc == be32(d + pos + 8 + len),
            std::string("PNG chunk ") + "CRC mismatch");
  const u8* payload = d + pos + 8;
  pos += 12 + (size_t)len;
  return payload;
}

PngHeader read_ihdr(const u8* d, size_t n, size_t& pos) {
  SCA_CHECK(is_png(d, n), "not a PNG file (bad signature)");
  pos = 8;
  u32 len;
  char type[5];
  const u8* p = read_chunk(d, n, pos, len, type);
  SCA_CHECK(std::string(type) == "IHDR" && len == 13,
            "PNG does not start with a 13-byte IHDR chunk");
  u32 w = be32(p), h = be32(p + 4);
  SCA_CHECK(w >= 1 && h >= 1 && w <= 65535 && h <= 65535,
            "PNG needs 1..65535 rows and columns");
  u32 depth = p[8], ctype = p[9];
  SCA_CHECK(ctype != 3, "palette PNG (colour type 3) is not supported");
  SCA_CHECK(depth != 16, "16-bit PNG is not supported");
  SCA_CHECK(depth == 8, "PNG bit depth " + std::to_string(depth) +
                            " is not supported, only 8");
  SCA_CHECK(ctype == 0 || ctype == 2 || ctype == 6,
            "PNG colour type " + std::to_string(ctype) +
                " is not supported (grey, RGB and RGBA are)");
  SCA_CHECK(p[10] == 0 && p[11] == 0, "bad PNG compression or filter method");
  SCA_CHECK(p[12] == 0, "interlaced PNG is not supported");
  return {(i32)h, (i32)w, ctype == 0 ? 1 : ctype == 2 ? 3 : 4};
}

int paeth(int a, int b, int c) {
  int p = a + b - c;
  int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p,
      pc = p > c ? p - c : c - p;
  return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

}  // namespace

bool is_png(const u8* d, size_t n) {
  return n >= 8 && std::memcmp(d, kPngMagic, 8) == 0;
}

void png_shape(const u8* data, size_t size, i32& h, i32& w, i32& c) {
  size_t pos;
  PngHeader hd = read_ihdr(data, size, pos);
  h = hd.h;
  w = hd.w;
  c = hd.channels == 1 ? 1 : 3;
}

DecodedImage png_decode(const u8* data, size_t size) {
  SCA_CHECK(data != nullptr, "not a PNG file (no data)");
  size_t pos;
  PngHeader hd = read_ihdr(data, size, pos);
  std::vector<u8> idat;
  bool ended = false;
  while (!ended) {
    u32 len;
    char type[5];
    const u8* p = read_chunk(data, size, pos, len, type);
    std::string t(type);
    if (t == "IDAT") {
      idat.insert(idat.end(), p, p + len);
    } else if (t == "IEND") {
      ended = true;
    } else {
      // an unknown critical chunk (upper-case first letter) cannot be skipped
      SCA_CHECK((type[0] & 0x20) != 0 || t == "PLTE",
                "unknown critical PNG chunk '" + t + "'");
    }
  }
  size_t bpp = (size_t)hd.channels;
  size_t row = (size_t)hd.w * bpp;
  size_t raw_size = (size_t)hd.h * (row + 1);
  // deflate expands by at most 1032:1, so a header promising more than the
  // IDAT data can hold is refused before anything is allocated for it
  SCA_CHECK(raw_size <= idat.size() * 1032 + 64,
            "truncated PNG: IDAT data too short for the image size");
  std::vector<u8> raw(raw_size);
  z_stream zs;
  std::memset(&zs, 0, sizeof(zs));
  SCA_CHECK(inflateInit(&zs) == Z_OK, "zlib inflateInit failed");
  zs.next_in = idat.data();
  zs.avail_in = (uInt)idat.size();
  zs.next_out = raw.data();
  zs.avail_out = (uInt)raw.size();
  int rc = inflate(&zs, Z_FINISH);
  size_t got = zs.total_out;
  inflateEnd(&zs);
  SCA_CHECK(rc == Z_STREAM_END && got == raw_size,
            "corrupt PNG: the zlib stream does not inflate to the image size");

  DecodedImage img;
  img.h = hd.h;
  img.w = hd.w;
  img.c = hd.channels == 1 ? 1 : 3;
  img.pixels.resize((size_t)img.h * img.w * img.c);
  std::vector<u8> zero(row, 0);
  for (i32 y = 0; y < hd.h; ++y) {
    u8* line = raw.data() + (size_t)y * (row + 1);
    u32 filter = line[0];
    u8* cur = line + 1;
    const u8* up = y ? cur - (row + 1) : zero.data();
    SCA_CHECK(filter <= 4, "corrupt PNG: scanline filter type " +
                               std::to_string(filter));
    for (size_t i = 0; i < row; ++i) {
      int a = i >= bpp ? cur[i - bpp] : 0;
      int b = up[i];
      int c = i >= bpp ? up[i - bpp] : 0;
      int pred = filter == 0   ? 0
                 : filter == 1 ? a
                 : filter == 2 ? b
                 : filter == 3 ? (a + b) >> 1
                               : paeth(a, b, c);
      cur[i] = (u8)(cur[i] + pred);
    }
    u8* dst = img.pixels.data() + (size_t)y * img.w * img.c;
    if (hd.channels == 4) {
      for (i32 x = 0; x < hd.w; ++x) {
        dst[3 * x] = cur[4 * x];
        dst[3 * x + 1] = cur[4 * x + 1];
        dst[3 * x + 2] = cur[4 * x + 2];
      }
    } else {
      std::memcpy(dst, cur, row);
    }
  }
  return img;
}

}  // namespace sca
