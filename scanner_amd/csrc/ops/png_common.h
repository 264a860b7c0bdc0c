// The "parallel" PNG format shared by the CPU writer (png_encode_cpu.cpp)
// and the HIP encoder (kernels/png_encode.hip). Written from the PNG
// specification (ISO/IEC 15948), RFC 1950 and RFC 1951. Every choice below is
// a pure function of the frame's bytes, and both writers call the functions
// of this header for it, so they agree byte for byte; they differ only in
// who walks the data (one thread, or a workgroup per chunk).
//
// Frames: 8-bit grey (1 channel) or RGB (3 channels), not interlaced.
//
// Filtering. bpp = channel count; row 0 sees a zero prior row. For every
// scanline each of the five filter types (0 None, 1 Sub, 2 Up, 3 Average,
// 4 Paeth) is scored by the sum over the row of |residual as signed 8-bit|;
// the smallest score wins, ties go to the lowest type. The filtered stream is
// h * (1 + w * c) bytes: a type byte, then the residuals.
//
// Chunks. The filtered stream is cut every kPngChunkBytes = 32768 bytes
// (the last chunk is shorter). A chunk is deflated on its own: no match
// reaches before its first byte. 32 KiB is deflate's whole distance range, so
// a larger chunk would find nothing more, and it is the largest of 16/32/64
// KiB whose working set fits the 160 KiB of LDS of a gfx950 CU: the chunk
// (32 KiB), one u16 per position for the parse (64 KiB), the start bitmap
// (4 KiB) and the bit image that aliases the hash table (32 KiB + 16), about
// 135 KiB. 16 KiB would let two workgroups share a CU but doubles the number
// of block headers and halves the match context.
//
// LZ77 per chunk. Match length 3..258, distance 1..32767. The candidate
// distances of position p are: 1; bpp (if bpp > 1); and one hash candidate.
// hash = png_hash3 of the 3 bytes at p, a table of kPngHashSize heads without
// chains. The parse walks the chunk in windows: a window starts at the
// current parse position `cur` and covers the kPngWindow = 256 positions from
// there. The hash candidate of every position of the window is the latest
// position q < cur with q + 3 <= n and the same hash, so lookups of a window
// never depend on inserts of the same window. A candidate counts if its
// distance is <= p, p + 3 <= n, and it matches >= 3 bytes (at most
// min(258, n - p)); the hash candidate must match >= kPngMinHashMatch = 6,
// since a far match costs about 25 bits and a filtered literal 3 to 4 (on a
// 256x256 gradient +-3 noise the file is 106 KB without this rule and 87 KB
// with it). The longest match wins, ties go to the smallest distance.
// The parse is greedy from left to right: at a position with a match the
// match is taken, otherwise a literal; the next token starts after it. When a
// token ends at or past the window's end (or the chunk's), all positions
// q in [cur, end of that token) with q + 3 <= n are inserted in ascending
// order (the latest wins) and the next window starts there.
//
// Entropy coding. One dynamic-Huffman block per chunk, BFINAL = 0. Code
// lengths come from png_build_lengths, a Kraft-sum rule (no tree):
//   0 used symbols -> all lengths 0; 1 used symbol -> length 1. Otherwise
//   1. len = the smallest l in 1..maxbits with freq << l >= total
//      (Shannon's ceil(log2(total / freq)), cut at maxbits). In units of
//      2^-maxbits the Kraft sum is S = sum(2^(maxbits - len)), full = 2^maxbits.
//   2. while S > full (only possible after the cut): for L = maxbits-1 down
//      to 1, lengthen the first m = min(count(L), ceil(over / 2^(maxbits-L-1)))
//      symbols of length L in index order, until over = S - full <= 0.
//   3. slack = full - S. For L = 2 up to maxbits: shorten the first
//      m = min(count(L), slack >> (maxbits - L)) symbols that have length L
//      at that moment, in index order, to L - 1.
//   4. For L = maxbits down to 2, while slack > 0: the same step. Lengths
//      are now <= L, so slack is a multiple of the step's cost and the loop
//      ends with slack = 0: the code is complete, as inflate requires.
// maxbits is 15 for the literal/length code (286 symbols, EOB counted once)
// and the distance code (30 symbols), 7 for the code-length code. Codes are
// canonical (RFC 1951 3.2.2). The block header sends HLIT = (last used
// literal/length symbol + 1, at least 257), HDIST = (last used distance
// symbol + 1, at least 1), HCLEN = 19, and lists every code length as it is:
// the run-length symbols 16..18 are never used.
// If the dynamic block has more bits than the stored block of the chunk
// (8 * (n + 5)), the stored block is written instead.
//
// Framing. zlib header 78 01. Every chunk's block is followed by an empty
// stored block (three 0 bits, padding to a byte, 00 00 FF FF), so a chunk's
// deflate data is a whole number of bytes: at most n + 10. After the last
// chunk: the final empty fixed block 03 00, then Adler-32 of the filtered
// stream, big-endian, computed per chunk and combined by png_adler_combine.
// File: signature, IHDR, one IDAT per chunk (the first also carries the
// zlib header, the last also 03 00 and the Adler-32), IEND.
// png_size_bound is exact for a frame whose every chunk is stored.
#pragma once

#include <string>
#include <vector>

#include "../common.h"

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__
#else
#define PNG_HD
#endif

namespace sca {

constexpr u32 kPngChunkBytes = 32768;
constexpr u32 kPngWindow = 256;
constexpr u32 kPngHashBits = 12;
constexpr u32 kPngHashSize = 1u << kPngHashBits;
constexpr u32 kPngMinMatch = 3, kPngMaxMatch = 258;
constexpr u32 kPngMinHashMatch = 6;
constexpr u32 kPngLitLen = 286, kPngDist = 30, kPngCl = 19;
constexpr u32 kPngEob = 256;
// deflate bytes of one chunk, worst case, and of the parts around the chunks
constexpr u32 kPngChunkOverhead = 10;
constexpr u32 kPngHeadBytes = 8 + 25;  // signature + IHDR chunk
constexpr u32 kPngZlibHead = 2, kPngZlibTail = 6;

enum class PngWriter : i32 { kZlib = 0, kParallel = 1 };
PngWriter png_parse_writer(const std::string& s);  // throws on anything else

PNG_HD inline u64 png_filtered_size(i32 h, i32 w, i32 c) {
  return (u64)h * (1 + (u64)w * c);
}
PNG_HD inline u32 png_chunk_count(i32 h, i32 w, i32 c) {
  return (u32)((png_filtered_size(h, w, c) + kPngChunkBytes - 1) /
               kPngChunkBytes);
}
PNG_HD inline u64 png_size_bound(i32 h, i32 w, i32 c) {
  return kPngHeadBytes + png_filtered_size(h, w, c) +
         (u64)png_chunk_count(h, w, c) * (12 + kPngChunkOverhead) +
         kPngZlibHead + kPngZlibTail + 12;
}

// ---- filtering ----
PNG_HD inline i32 png_paeth(i32 a, i32 b, i32 c) {
  i32 p = a + b - c;
  i32 pa = p > a ? p - a : a - p;
  i32 pb = p > b ? p - b : b - p;
  i32 pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// residual of byte x under filter `type`; a = left, b = above, c = above left
PNG_HD inline u8 png_residual(u32 type, i32 x, i32 a, i32 b, i32 c) {
  i32 pred = type == 0   ? 0
             : type == 1 ? a
             : type == 2 ? b
             : type == 3 ? (a + b) >> 1
                         : png_paeth(a, b, c);
  return (u8)(x - pred);
}
PNG_HD inline u32 png_abs8(u8 r) { return r < 128 ? r : 256u - r; }
// smallest score, ties to the lowest type
PNG_HD inline u32 png_pick_filter(const u32 score[5]) {
  u32 best = 0;
  for (u32 t = 1; t < 5; ++t)
    if (score[t] < score[best]) best = t;
  return best;
}

// ---- LZ77 ----
PNG_HD inline u32 png_hash3(const u8* p) {
  u32 v = (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16;
  return (v * 2654435761u) >> (32 - kPngHashBits);
}
// common prefix of d[p..] and d[p - dist..], at most maxl
PNG_HD inline u32 png_match_len(const u8* d, u32 p, u32 dist, u32 maxl) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the same number, four bytes per step from aligned words: d is 4-byte
  // aligned and readable for 8 bytes past the chunk (what lies there is
  // cut off by maxl)
  const u32* w = reinterpret_cast<const u32*>(d);
  u32 q = p - dist;
  u32 pa = p >> 2, sa = (p & 3) * 8, qa = q >> 2, sb = (q & 3) * 8;
  u32 k = 0;
  while (k < maxl) {
    u32 x = (u32)(((u64)w[pa + 1] << 32 | w[pa]) >> sa);
    u32 y = (u32)(((u64)w[qa + 1] << 32 | w[qa]) >> sb);
    u32 diff = x ^ y;
    if (diff) {
      k += (u32)__builtin_ctz(diff) >> 3;
      break;
    }
    k += 4;
    ++pa;
    ++qa;
  }
  return k < maxl ? k : maxl;
#else
  const u8* a = d + p;
  const u8* b = a - dist;
  u32 k = 0;
  while (k < maxl && a[k] == b[k]) ++k;
  return k;
#endif
}
// best match at p of the n-byte chunk d: len << 16 | dist, or 0. `head` is
// the hash table's entry for p (position + 1, 0 = none), as of the window's
// start.
PNG_HD inline u32 png_best_match(const u8* d, u32 n, u32 p, u32 bpp,
                                 u32 head) {
  if (p + kPngMinMatch > n) return 0;
  u32 maxl = n - p < kPngMaxMatch ? n - p : kPngMaxMatch;
  u32 cand[3] = {1u, bpp > 1 ? bpp : 0u, head ? p - (head - 1) : 0u};
  u32 best = 0, bd = 0;
  for (u32 k = 0; k < 3; ++k) {
    u32 dist = cand[k];
    if (dist == 0 || dist > p) continue;
    u32 l = png_match_len(d, p, dist, maxl);
    if (l >= (k == 2 ? kPngMinHashMatch : kPngMinMatch) && (l > best || (l == best && dist < bd))) {
      best = l;
      bd = dist;
    }
  }
  return best ? best << 16 | bd : 0u;
}

// ---- deflate symbols ----
PNG_HD inline u32 png_log2(u32 v) { return 31u - (u32)__builtin_clz(v); }
// match length 3..258 -> symbol 257..285, extra bit count and value
PNG_HD inline void png_len_symbol(u32 len, u32& sym, u32& ebits, u32& eval) {
  if (len == kPngMaxMatch) {
    sym = 285;
    ebits = eval = 0;
    return;
  }
  u32 l = len - 3;
  ebits = l < 8 ? 0 : png_log2(l) - 2;
  sym = 257 + 4 * ebits + (l >> ebits);
  eval = l & ((1u << ebits) - 1);
}
// distance 1..32768 -> symbol 0..29
PNG_HD inline void png_dist_symbol(u32 dist, u32& sym, u32& ebits, u32& eval) {
  u32 d = dist - 1;
  ebits = d < 4 ? 0 : png_log2(d) - 1;
  sym = d < 4 ? d : 2 * ebits + 2 + ((d >> ebits) & 1);
  eval = d & ((1u << ebits) - 1);
}

// Code lengths by the rule in the file comment. cnt: 16 words of scratch.
PNG_HD inline void png_build_lengths(const u32* freq, u32 n, u32 maxbits,
                                     u8* len, u32* cnt) {
  u32 used = 0, total = 0, last = 0;
  for (u32 i = 0; i < n; ++i) {
    len[i] = 0;
    if (freq[i]) {
      ++used;
      total += freq[i];
      last = i;
    }
  }
  if (used == 0) return;
  if (used == 1) {
    len[last] = 1;
    return;
  }
  for (u32 l = 0; l < 16; ++l) cnt[l] = 0;
  const u32 full = 1u << maxbits;
  u32 sum = 0;
  for (u32 i = 0; i < n; ++i) {
    if (!freq[i]) continue;
    u32 l = 1;
    while (l < maxbits && (freq[i] << l) < total) ++l;
    len[i] = (u8)l;
    ++cnt[l];
    sum += full >> l;
  }
  while (sum > full) {
    for (u32 L = maxbits - 1; L >= 1 && sum > full; --L) {
      u32 gain = full >> (L + 1), over = sum - full;
      u32 m = (over + gain - 1) / gain;
      if (m > cnt[L]) m = cnt[L];
      cnt[L] -= m;
      cnt[L + 1] += m;
      sum -= m * gain;
      for (u32 i = 0; i < n && m; ++i)
        if (len[i] == L) {
          len[i] = (u8)(L + 1);
          --m;
        }
    }
  }
  u32 slack = full - sum;
  for (u32 pass = 0; pass < 2 && slack; ++pass) {
    for (u32 k = 2; k <= maxbits && slack; ++k) {
      u32 L = pass == 0 ? k : maxbits + 2 - k;
      u32 m = slack >> (maxbits - L);
      if (m > cnt[L]) m = cnt[L];
      if (!m) continue;
      cnt[L] -= m;
      cnt[L - 1] += m;
      slack -= m << (maxbits - L);
      for (u32 i = 0; i < n && m; ++i)
        if (len[i] == L) {
          len[i] = (u8)(L - 1);
          --m;
        }
    }
  }
}

PNG_HD inline u32 png_bit_reverse(u32 code, u32 len) {
  u32 r = 0;
  for (u32 i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}
// canonical codes, already reversed for deflate's LSB-first bit order
template <class Code>
PNG_HD inline void png_canonical(const u8* len, u32 n, Code* code, u32* cnt) {
  u32 next[16];
  for (u32 l = 0; l < 16; ++l) cnt[l] = 0;
  for (u32 i = 0; i < n; ++i) ++cnt[len[i]];
  cnt[0] = 0;
  u32 c = 0;
  next[0] = 0;
  for (u32 l = 1; l < 16; ++l) {
    c = (c + cnt[l - 1]) << 1;
    next[l] = c;
  }
  for (u32 i = 0; i < n; ++i)
    code[i] = len[i] ? (Code)png_bit_reverse(next[len[i]]++, len[i]) : (Code)0;
}

// order in which the code-length code's lengths are sent
PNG_HD inline u32 png_cl_order(u32 i) {
  const u8 order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5,
                        11, 4, 12, 3, 13, 2, 14, 1, 15};
  return order[i];
}

// The three codes of one chunk's dynamic block.
struct PngCodes {
  u16 ll_code[kPngLitLen];
  u16 d_code[kPngDist];
  u8 ll_len[kPngLitLen];
  u8 d_len[kPngDist];
  u8 cl_code[kPngCl];
  u8 cl_len[kPngCl];
  u32 hlit, hdist;   // code lengths sent for the two codes
  u32 header_bits;   // BFINAL .. the last code length
  u32 cl_freq[kPngCl];
  u32 cnt[16];       // scratch
};
constexpr u32 kPngHeaderFixedBits = 3 + 5 + 5 + 4 + 3 * kPngCl;

// ll_freq counts literals, length symbols and one EOB; d_freq the distance
// symbols.
PNG_HD inline void png_build_codes(const u32* ll_freq, const u32* d_freq,
                                   PngCodes& c) {
  png_build_lengths(ll_freq, kPngLitLen, 15, c.ll_len, c.cnt);
  png_build_lengths(d_freq, kPngDist, 15, c.d_len, c.cnt);
  c.hlit = 257;
  for (u32 i = 257; i < kPngLitLen; ++i)
    if (c.ll_len[i]) c.hlit = i + 1;
  c.hdist = 1;
  for (u32 i = 1; i < kPngDist; ++i)
    if (c.d_len[i]) c.hdist = i + 1;
  for (u32 i = 0; i < kPngCl; ++i) c.cl_freq[i] = 0;
  for (u32 i = 0; i < c.hlit; ++i) ++c.cl_freq[c.ll_len[i]];
  for (u32 i = 0; i < c.hdist; ++i) ++c.cl_freq[c.d_len[i]];
  png_build_lengths(c.cl_freq, kPngCl, 7, c.cl_len, c.cnt);
  png_canonical(c.ll_len, kPngLitLen, c.ll_code, c.cnt);
  png_canonical(c.d_len, kPngDist, c.d_code, c.cnt);
  png_canonical(c.cl_len, kPngCl, c.cl_code, c.cnt);
  u32 bits = kPngHeaderFixedBits;
  for (u32 i = 0; i < kPngCl; ++i) bits += c.cl_freq[i] * c.cl_len[i];
  c.header_bits = bits;
}

// One token through sink(bits, count), each call at most 28 bits. len == 0:
// the literal v; otherwise a match of that length at distance v.
template <class Sink>
PNG_HD inline void png_code_token(const PngCodes& c, u32 len, u32 v,
                                  Sink& sink) {
  if (len == 0) {
    sink(c.ll_code[v], c.ll_len[v]);
    return;
  }
  u32 sym, eb, ev;
  png_len_symbol(len, sym, eb, ev);
  sink(c.ll_code[sym] | ev << c.ll_len[sym], c.ll_len[sym] + eb);
  png_dist_symbol(v, sym, eb, ev);
  sink(c.d_code[sym] | ev << c.d_len[sym], c.d_len[sym] + eb);
}

// ---- checksums ----
constexpr u32 kAdlerBase = 65521;
// Adler-32 of A || B from those of A and B and len(B)
PNG_HD inline u32 png_adler_combine(u32 adler1, u32 adler2, u64 len2) {
  u32 rem = (u32)(len2 % kAdlerBase);
  u32 sum1 = adler1 & 0xffff;
  u32 sum2 = (u32)(((u64)rem * sum1) % kAdlerBase);
  sum1 += (adler2 & 0xffff) + kAdlerBase - 1;
  sum2 += (adler1 >> 16) + (adler2 >> 16) + kAdlerBase - rem;
  if (sum1 >= kAdlerBase) sum1 -= kAdlerBase;
  if (sum1 >= kAdlerBase) sum1 -= kAdlerBase;
  if (sum2 >= kAdlerBase * 2) sum2 -= kAdlerBase * 2;
  if (sum2 >= kAdlerBase) sum2 -= kAdlerBase;
  return sum1 | sum2 << 16;
}

// ---- the two writers ----
void png_check_args(i32 h, i32 w, i32 c);  // throws
// one [h, w, c] u8 frame -> file bytes; the reference implementation
std::vector<u8> png_encode_parallel_cpu(const u8* pix, i32 h, i32 w, i32 c);
// device-resident frames of one shape -> exact-size files in device memory
// (kernels/png_encode.hip), appended to out/sizes
void png_encode_gpu(const std::vector<const u8*>& frames, i32 h, i32 w, i32 c,
                    DeviceHandle dev, void* stream, std::vector<u8*>& out,
                    std::vector<u64>& sizes);

}  // namespace sca
