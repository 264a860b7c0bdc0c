// Reference writer of the "parallel" PNG format: filtering, chunked LZ77,
// one dynamic-Huffman block per chunk. Every choice is made by the functions
// of png_common.h, whose comment is the specification; this file walks the
// data in order and packs the bits. Single-threaded: "parallel" names the
// format, which kernels/png_encode.hip writes a chunk per workgroup.
#include <zlib.h>

#include <cstring>

#include "png_common.h"

namespace sca {

PngWriter png_parse_writer(const std::string& s) {
  if (s == "zlib") return PngWriter::kZlib;
  if (s == "parallel") return PngWriter::kParallel;
  throw ScannerError("ImageEncoder png_writer must be one of 'zlib', "
                     "'parallel', got '" + s + "'");
}

void png_check_args(i32 h, i32 w, i32 c) {
  SCA_CHECK(c == 1 || c == 3, "PNG encoder supports 1- or 3-channel u8");
  SCA_CHECK(h >= 1 && w >= 1, "PNG encoder needs a non-empty frame");
  SCA_CHECK(png_size_bound(h, w, c) < (1ull << 31),
            "PNG encoder: frame too large");
}

namespace {

struct BitWriter {
  std::vector<u8>& out;
  u64 acc = 0;
  u32 fill = 0;
  void operator()(u32 bits, u32 n) {
    acc |= (u64)bits << fill;
    fill += n;
    while (fill >= 8) {
      out.push_back((u8)acc);
      acc >>= 8;
      fill -= 8;
    }
  }
  void align() {
    if (fill) (*this)(0, 8 - fill);
  }
};

struct BitCount {
  u64 bits = 0;
  void operator()(u32, u32 n) { bits += n; }
};

struct Token {
  u16 len;  // 0: literal
  u16 v;    // literal value or distance
};

void filter_frame(const u8* pix, i32 h, i32 w, i32 c, std::vector<u8>& out) {
  size_t rb = (size_t)w * c;
  out.resize((size_t)h * (1 + rb));
  std::vector<u8> zero(rb, 0);
  for (i32 y = 0; y < h; ++y) {
    const u8* cur = pix + (size_t)y * rb;
    const u8* up = y ? cur - rb : zero.data();
    u32 score[5] = {0, 0, 0, 0, 0};
    for (size_t x = 0; x < rb; ++x) {
      i32 a = x >= (size_t)c ? cur[x - c] : 0;
      i32 b = up[x];
      i32 cc = x >= (size_t)c ? up[x - c] : 0;
      for (u32 t = 0; t < 5; ++t)
        score[t] += png_abs8(png_residual(t, cur[x], a, b, cc));
    }
    u32 t = png_pick_filter(score);
    u8* dst = out.data() + (size_t)y * (1 + rb);
    dst[0] = (u8)t;
    for (size_t x = 0; x < rb; ++x) {
      i32 a = x >= (size_t)c ? cur[x - c] : 0;
      i32 b = up[x];
      i32 cc = x >= (size_t)c ? up[x - c] : 0;
      dst[1 + x] = png_residual(t, cur[x], a, b, cc);
    }
  }
}

// deflate data of one chunk: its block and the empty stored block
void deflate_chunk(const u8* d, u32 n, u32 bpp, std::vector<u8>& out) {
  std::vector<u32> head(kPngHashSize, 0);
  std::vector<Token> tokens;
  std::vector<u32> ll_freq(kPngLitLen, 0), d_freq(kPngDist, 0);
  u32 match[kPngWindow];
  u32 cur = 0;
  while (cur < n) {
    u32 wend = n - cur < kPngWindow ? n : cur + kPngWindow;
    for (u32 p = cur; p < wend; ++p) {
      u32 hq = p + kPngMinMatch <= n ? head[png_hash3(d + p)] : 0;
      match[p - cur] = png_best_match(d, n, p, bpp, hq);
    }
    u32 pos = cur;
    while (pos < wend) {
      u32 m = match[pos - cur];
      if (m) {
        u32 len = m >> 16, dist = m & 0xffff, sym, eb, ev;
        tokens.push_back({(u16)len, (u16)dist});
        png_len_symbol(len, sym, eb, ev);
        ++ll_freq[sym];
        png_dist_symbol(dist, sym, eb, ev);
        ++d_freq[sym];
        pos += len;
      } else {
        tokens.push_back({0, d[pos]});
        ++ll_freq[d[pos]];
        pos += 1;
      }
    }
    for (u32 q = cur; q < pos; ++q)
      if (q + kPngMinMatch <= n) head[png_hash3(d + q)] = q + 1;
    cur = pos;
  }
  ++ll_freq[kPngEob];

  PngCodes codes;
  png_build_codes(ll_freq.data(), d_freq.data(), codes);
  BitCount cnt;
  for (const Token& t : tokens) png_code_token(codes, t.len, t.v, cnt);
  u64 dyn_bits = codes.header_bits + cnt.bits + codes.ll_len[kPngEob];

  BitWriter bw{out};
  if (dyn_bits > 8ull * (n + 5)) {
    bw(0, 8);  // BFINAL 0, BTYPE 00, padding
    bw(n, 16);
    bw(~n & 0xffffu, 16);
    out.insert(out.end(), d, d + n);
  } else {
    bw(0, 1);
    bw(2, 2);
    bw(codes.hlit - 257, 5);
    bw(codes.hdist - 1, 5);
    bw(kPngCl - 4, 4);
    for (u32 i = 0; i < kPngCl; ++i) bw(codes.cl_len[png_cl_order(i)], 3);
    for (u32 i = 0; i < codes.hlit; ++i)
      bw(codes.cl_code[codes.ll_len[i]], codes.cl_len[codes.ll_len[i]]);
    for (u32 i = 0; i < codes.hdist; ++i)
      bw(codes.cl_code[codes.d_len[i]], codes.cl_len[codes.d_len[i]]);
    for (const Token& t : tokens) png_code_token(codes, t.len, t.v, bw);
    bw(codes.ll_code[kPngEob], codes.ll_len[kPngEob]);
  }
  bw(0, 3);  // the empty stored block
  bw.align();
  bw(0, 16);
  bw(0xffff, 16);
}

void put_be32(std::vector<u8>& v, u32 x) {
  v.push_back((u8)(x >> 24));
  v.push_back((u8)(x >> 16));
  v.push_back((u8)(x >> 8));
  v.push_back((u8)x);
}

void put_chunk(std::vector<u8>& png, const char type[4], const u8* data,
               size_t n) {
  put_be32(png, (u32)n);
  size_t type_off = png.size();
  png.insert(png.end(), type, type + 4);
  png.insert(png.end(), data, data + n);
  u32 crc = (u32)crc32(crc32(0L, Z_NULL, 0), png.data() + type_off,
                       (uInt)(4 + n));
  put_be32(png, crc);
}

}  // namespace

std::vector<u8> png_encode_parallel_cpu(const u8* pix, i32 h, i32 w, i32 c) {
  png_check_args(h, w, c);
  std::vector<u8> filt;
  filter_frame(pix, h, w, c, filt);

  std::vector<u8> png = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  std::vector<u8> ihdr;
  put_be32(ihdr, (u32)w);
  put_be32(ihdr, (u32)h);
  ihdr.push_back(8);               // bit depth
  ihdr.push_back(c == 3 ? 2 : 0);  // colour type: RGB / grey
  ihdr.insert(ihdr.end(), {0, 0, 0});  // deflate, adaptive filters, no interlace
  put_chunk(png, "IHDR", ihdr.data(), ihdr.size());

  u32 nch = png_chunk_count(h, w, c);
  u32 adler = 1;
  std::vector<u8> idat;
  for (u32 k = 0; k < nch; ++k) {
    const u8* d = filt.data() + (size_t)k * kPngChunkBytes;
    u32 n = (u32)std::min<size_t>(kPngChunkBytes,
                                  filt.size() - (size_t)k * kPngChunkBytes);
    idat.clear();
    if (k == 0) idat.insert(idat.end(), {0x78, 0x01});
    deflate_chunk(d, n, (u32)c, idat);
    u32 a = (u32)adler32(adler32(0L, Z_NULL, 0), d, n);
    adler = k == 0 ? a : png_adler_combine(adler, a, n);
    if (k + 1 == nch) {
      idat.insert(idat.end(), {0x03, 0x00});
      put_be32(idat, adler);
    }
    put_chunk(png, "IDAT", idat.data(), idat.size());
  }
  put_chunk(png, "IEND", nullptr, 0);
  return png;
}

}  // namespace sca
