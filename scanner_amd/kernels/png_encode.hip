// GPU writer of the "parallel" PNG format for gfx950: device-resident u8
// frames become PNG files in HBM, byte-identical to png_encode_parallel_cpu.
// The format and every choice in it: csrc/ops/png_common.h.
//
// Kernel shape (four launches per sequence of same-shape frames):
//   filter   grid (rows, frames) x 256 lanes: the five residual scores of a
//            scanline by wave and workgroup reduction, then the chosen
//            filtered row and its type byte -> the filtered stream in HBM
//   deflate  grid (chunks, frames) x 256 lanes, one workgroup per 32 KiB
//            chunk, about 135 KiB of LDS (one workgroup per CU):
//              A  chunk -> LDS; Adler-32 partial sums
//              B  windows of 256 positions: lane t finds the best match at
//                 cur + t (three candidates, png_best_match); wave 0 walks
//                 the greedy parse through the window, 64 lengths per
//                 register: literal runs in one step from ballot masks, a
//                 match's length by readlane; token starts -> bitmap,
//                 length and distance -> tok[], symbols -> LDS histogram;
//                 the window's positions enter the hash table by atomicMax
//              C  lane 0 builds the three codes (png_build_codes, the same
//                 function as on the CPU; 335 symbols)
//              D  code lengths -> workgroup exclusive scan -> codes OR-merged
//                 into a zeroed LDS bit image (LSB first), or the stored
//                 block if that is shorter; image -> the chunk's staging
//                 slot; byte count and Adler-32 -> arrays
//   scan     one workgroup per frame: IDAT offsets and the file size for any
//            chunk count; lane 0 combines the chunks' Adler-32
//   gather   grid (chunks, frames): signature, IHDR, the IDAT of the chunk
//            with its CRC-32 (256 slices, combined by multiplication with
//            x^(8 * bytes behind the slice) in GF(2)[x] / CRC polynomial),
//            IEND -> exact-size outputs
// The host reads the file sizes once per sequence (one stream synchronise),
// allocates exact-size outputs from the slab pool and synchronises once more
// before the staging goes back to the pool.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../csrc/memory.h"
#include "../csrc/ops/png_common.h"

namespace sca {

namespace {

#define PNG_ENC_CHECK(expr)                                              \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess) {                                              \
      throw ScannerError(std::string("HIP error in png encode: ") +      \
                         hipGetErrorString(_e));                         \
    }                                                                    \
  } while (0)

constexpr u32 kThreads = 256;
static_assert(kPngWindow == kThreads, "one lane per position of a window");
constexpr u32 kMaxFrames = 16;  // frames per launch sequence
// filtered stream + staging are about twice the raw frames
constexpr u64 kStagingBudget = 384ull << 20;
// staging bytes of one chunk: its deflate data, rounded up to whole words
constexpr u32 kSlot = kPngChunkBytes + 16;
static_assert(kSlot >= kPngChunkBytes + kPngChunkOverhead && kSlot % 4 == 0,
              "a stored chunk fits its slot");
// bit image of one chunk, + the word a code may spill into
constexpr u32 kBitWords = kSlot / 4 + 2;
static_assert(kBitWords >= kPngHashSize, "the hash heads alias the bit image");
constexpr u32 kCrcPoly = 0xedb88320u;

struct PngEncArgs {
  const u8* frames[kMaxFrames];
  u8* out[kMaxFrames];  // exact-size files (gather)
  u8* filt;             // [nframes][fsz] filtered streams
  u8* staging;          // chunk (f, k) at (f * nch + k) * kSlot
  u32* csize;           // [nframes][nch] deflate bytes
  u32* cadler;          // [nframes][nch] Adler-32 of the chunk
  u32* coff;            // [nframes][nch] IDAT offset past IHDR
  u32* sizes;           // [nframes] file sizes
  u32* adler;           // [nframes] Adler-32 of the filtered stream
  u32 x2n[32];          // x^(2^k) mod the CRC polynomial, reflected
  u64 fsz;              // filtered bytes per frame
  i32 h, w, c;
  u32 nch;
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

__device__ inline u32 wave_sum_u32(u32 v) {
#pragma unroll
  for (u32 d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ inline u32 chunk_len(const PngEncArgs& a, u32 k) {
  u64 left = a.fsz - (u64)k * kPngChunkBytes;
  return left < kPngChunkBytes ? (u32)left : kPngChunkBytes;
}

__global__ void __launch_bounds__(kThreads) png_filter_kernel(PngEncArgs a) {
  __shared__ u32 red[kThreads / 64][5];
  u32 y = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  u32 bpp = (u32)a.c, rb = (u32)a.w * bpp;
  const u8* cur = a.frames[f] + (u64)y * rb;
  const u8* up = cur - rb;  // read for y > 0 only
  u32 s[5] = {0, 0, 0, 0, 0};
  for (u32 x = tid; x < rb; x += kThreads) {
    i32 v = cur[x];
    i32 l = x >= bpp ? cur[x - bpp] : 0;
    i32 u = y ? up[x] : 0;
    i32 ul = (y && x >= bpp) ? up[x - bpp] : 0;
#pragma unroll
    for (u32 t = 0; t < 5; ++t) s[t] += png_abs8(png_residual(t, v, l, u, ul));
  }
#pragma unroll
  for (u32 t = 0; t < 5; ++t) {
    u32 r = wave_sum_u32(s[t]);
    if ((tid & 63) == 0) red[tid >> 6][t] = r;
  }
  __syncthreads();
  u32 score[5];
#pragma unroll
  for (u32 t = 0; t < 5; ++t) {
    score[t] = 0;
#pragma unroll
    for (u32 wv = 0; wv < kThreads / 64; ++wv) score[t] += red[wv][t];
  }
  u32 type = png_pick_filter(score);
  u8* dst = a.filt + (u64)f * a.fsz + (u64)y * (1 + rb);
  if (tid == 0) dst[0] = (u8)type;
  for (u32 x = tid; x < rb; x += kThreads) {
    i32 v = cur[x];
    i32 l = x >= bpp ? cur[x - bpp] : 0;
    i32 u = y ? up[x] : 0;
    i32 ul = (y && x >= bpp) ? up[x - bpp] : 0;
    dst[1 + x] = png_residual(type, v, l, u, ul);
  }
}

struct BitCount {
  u32 bits = 0;
  __device__ void operator()(u32, u32 len) { bits += len; }
};

// OR a code into the LSB-first bit image at bit `pos`
struct BitMerge {
  u32* img;
  u32 pos;
  __device__ void operator()(u32 v, u32 len) {
    u32 w = pos >> 5, o = pos & 31;
    u64 x = (u64)v << o;
    u32 lo = (u32)x, hi = (u32)(x >> 32);
    if (lo) atomicOr(&img[w], lo);
    if (hi) atomicOr(&img[w + 1], hi);
    pos += len;
  }
};

// code length of the i-th entry of the block header's length list
__device__ inline u32 header_len_at(const PngCodes& c, u32 i) {
  return i < c.hlit ? c.ll_len[i] : c.d_len[i - c.hlit];
}

__global__ void __launch_bounds__(kThreads) png_deflate_kernel(PngEncArgs a) {
  // + 8: png_match_len reads whole words
  __shared__ __attribute__((aligned(16))) u8 data[kPngChunkBytes + 8];
  __shared__ u16 tok[kPngChunkBytes];   // at a token's start: 0 (literal) or
                                        // the length; distance at start + 1
  __shared__ u32 smask[kPngChunkBytes / 32];  // token starts
  __shared__ u32 bits[kBitWords];
  __shared__ u32 ll_freq[kPngLitLen];
  __shared__ u32 d_freq[kPngDist];
  __shared__ PngCodes codes;
  __shared__ u32 wmatch[kThreads];
  __shared__ u32 wmask[kThreads / 32];
  __shared__ u32 wnext;
  __shared__ u32 wave_sum[kThreads / 64];
  __shared__ u32 red[2][kThreads / 64];
  u32* head = bits;  // B only; the bit image is zeroed after it
  u32 k = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  u32 bpp = (u32)a.c;
  u32 n = chunk_len(a, k);
  const u8* src = a.filt + (u64)f * a.fsz + (u64)k * kPngChunkBytes;

  // ---- A: load; Adler-32 = (1 + sum d) | (n + sum (n - i) d) << 16 ----
  u32 s1 = 0, s2 = 0;  // <= 128 terms of < 2^23 each
  for (u32 i = tid; i < n; i += kThreads) {
    u32 v = src[i];
    data[i] = (u8)v;
    s1 += v;
    s2 += (n - i) * v;
  }
  s1 = wave_sum_u32(s1 % kAdlerBase);
  s2 = wave_sum_u32(s2 % kAdlerBase);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = s1;
    red[1][tid >> 6] = s2;
  }
  for (u32 i = tid; i < kPngChunkBytes / 32; i += kThreads) smask[i] = 0;
  for (u32 i = tid; i < kPngHashSize; i += kThreads) head[i] = 0;
  for (u32 i = tid; i < kPngLitLen; i += kThreads) ll_freq[i] = 0;
  if (tid < kPngDist) d_freq[tid] = 0;
  __syncthreads();

  // ---- B: matches, greedy parse, histogram ----
  u32 cur = 0;
  while (cur < n) {
    u32 p = cur + tid;
    u32 m = 0;
    if (p < n) {
      u32 hq = p + kPngMinMatch <= n ? head[png_hash3(data + p)] : 0u;
      m = png_best_match(data, n, p, bpp, hq);
    }
    wmatch[tid] = m;
    __syncthreads();
    if (tid < 64) {
      // lengths of positions cur + 64 j + lane in register j
      u32 l0 = wmatch[tid] >> 16, l1 = wmatch[64 + tid] >> 16;
      u32 l2 = wmatch[128 + tid] >> 16, l3 = wmatch[192 + tid] >> 16;
      u32 lim = n - cur < kThreads ? n - cur : kThreads;
      // groups of 64 positions: where a match starts, and the token starts
      u64 b0 = __ballot(l0 != 0), b1 = __ballot(l1 != 0);
      u64 b2 = __ballot(l2 != 0), b3 = __ballot(l3 != 0);
      u64 m0 = 0, m1 = 0, m2 = 0, m3 = 0;
      u32 pos = 0;
      while (pos < lim) {
        u32 q = __builtin_amdgcn_readfirstlane(pos);
        u32 g = q >> 6, ln = q & 63;
        u64 rest = (g == 0 ? b0 : g == 1 ? b1 : g == 2 ? b2 : b3) >> ln;
        // literals up to the next match, the group's end or the limit
        u32 run = rest ? (u32)__builtin_ctzll(rest) : 64u - ln;
        if (run > lim - q) run = lim - q;
        u32 len = 0;
        if (run == 0) {
          len = g == 0   ? __builtin_amdgcn_readlane(l0, ln)
                : g == 1 ? __builtin_amdgcn_readlane(l1, ln)
                : g == 2 ? __builtin_amdgcn_readlane(l2, ln)
                         : __builtin_amdgcn_readlane(l3, ln);
          run = 1;
        }
        u64 span = (run == 64 ? ~0ull : (1ull << run) - 1ull) << ln;
        if (g == 0) m0 |= span;
        else if (g == 1) m1 |= span;
        else if (g == 2) m2 |= span;
        else m3 |= span;
        pos = q + (len ? len : run);
      }
      if (tid == 0) {
        wmask[0] = (u32)m0; wmask[1] = (u32)(m0 >> 32);
        wmask[2] = (u32)m1; wmask[3] = (u32)(m1 >> 32);
        wmask[4] = (u32)m2; wmask[5] = (u32)(m2 >> 32);
        wmask[6] = (u32)m3; wmask[7] = (u32)(m3 >> 32);
        wnext = cur + pos;
      }
    }
    __syncthreads();
    u32 nxt = wnext;
    if ((wmask[tid >> 5] >> (tid & 31)) & 1u) {  // a token starts at p < n
      atomicOr(&smask[p >> 5], 1u << (p & 31));
      if (m) {
        u32 len = m >> 16, dist = m & 0xffffu, sym, eb, ev;
        tok[p] = (u16)len;
        tok[p + 1] = (u16)dist;  // len >= 3: inside the match
        png_len_symbol(len, sym, eb, ev);
        atomicAdd(&ll_freq[sym], 1u);
        png_dist_symbol(dist, sym, eb, ev);
        atomicAdd(&d_freq[sym], 1u);
      } else {
        tok[p] = 0;
        atomicAdd(&ll_freq[data[p]], 1u);
      }
    }
    for (u32 q = cur + tid; q < nxt; q += kThreads)
      if (q + kPngMinMatch <= n) atomicMax(&head[png_hash3(data + q)], q + 1);
    cur = nxt;
    __syncthreads();
  }

  // ---- C: the three codes ----
  if (tid == 0) {
    ll_freq[kPngEob] = 1;
    png_build_codes(ll_freq, d_freq, codes);
  }
  for (u32 i = tid; i < kBitWords; i += kThreads) bits[i] = 0;
  __syncthreads();

  // ---- D: lengths, scans, OR-merge or the stored block ----
  u32 per = (n + kThreads - 1) / kThreads;
  u32 lo = tid * per < n ? tid * per : n;
  u32 hi = lo + per < n ? lo + per : n;
  BitCount cnt;
  for (u32 p = lo; p < hi; ++p)
    if ((smask[p >> 5] >> (p & 31)) & 1u) {
      u32 t = tok[p];
      png_code_token(codes, t, t ? (u32)tok[p + 1] : (u32)data[p], cnt);
    }
  u32 tok_bits;
  u32 tok_pos = block_excl_scan(cnt.bits, wave_sum, tok_bits);
  u32 nlist = codes.hlit + codes.hdist;  // <= 316: two entries per lane
  u32 hb = 0;
  for (u32 i = 2 * tid; i < 2 * tid + 2 && i < nlist; ++i)
    hb += codes.cl_len[header_len_at(codes, i)];
  u32 list_bits;
  u32 list_pos = block_excl_scan(hb, wave_sum, list_bits);
  u32 eob_len = codes.ll_len[kPngEob];
  u32 dyn_bits = codes.header_bits + tok_bits + eob_len;
  bool stored = dyn_bits > 8u * (n + 5u);
  u8* dst = a.staging + ((u64)f * a.nch + k) * kSlot;
  u32 nbytes;
  if (stored) {
    nbytes = n + kPngChunkOverhead;
    if (tid == 0) {
      dst[0] = 0;  // BFINAL 0, BTYPE 00, padding
      dst[1] = (u8)n;
      dst[2] = (u8)(n >> 8);
      dst[3] = (u8)~n;
      dst[4] = (u8)(~n >> 8);
      u8* e = dst + 5 + n;  // the empty stored block
      e[0] = e[1] = e[2] = 0;
      e[3] = e[4] = 0xff;
    }
    for (u32 i = tid; i < n; i += kThreads) dst[5 + i] = data[i];
  } else {
    if (tid == 0) {
      BitMerge mrg{bits, 0};
      mrg(0, 1);
      mrg(2, 2);
      mrg(codes.hlit - 257, 5);
      mrg(codes.hdist - 1, 5);
      mrg(kPngCl - 4, 4);
      for (u32 i = 0; i < kPngCl; ++i) mrg(codes.cl_len[png_cl_order(i)], 3);
      BitMerge eob{bits, codes.header_bits + tok_bits};
      eob(codes.ll_code[kPngEob], eob_len);
    }
    BitMerge lst{bits, kPngHeaderFixedBits + list_pos};
    for (u32 i = 2 * tid; i < 2 * tid + 2 && i < nlist; ++i) {
      u32 l = header_len_at(codes, i);
      lst(codes.cl_code[l], codes.cl_len[l]);
    }
    BitMerge mrg{bits, codes.header_bits + tok_pos};
    for (u32 p = lo; p < hi; ++p)
      if ((smask[p >> 5] >> (p & 31)) & 1u) {
        u32 t = tok[p];
        png_code_token(codes, t, t ? (u32)tok[p + 1] : (u32)data[p], mrg);
      }
    // the empty stored block: 3 zero bits, padding, 00 00 FF FF
    u32 nb = (dyn_bits + 3 + 7) / 8;
    nbytes = nb + 4;
    if (tid == 0) {
      BitMerge ff{bits, (nb + 2) * 8};
      ff(0xffffu, 16);
    }
    __syncthreads();
    u32* dst4 = reinterpret_cast<u32*>(dst);  // slots are word-aligned
    for (u32 i = tid; i < (nbytes + 3) / 4; i += kThreads) dst4[i] = bits[i];
  }
  if (tid == 0) {
    u32 t1 = 0, t2 = 0;
    for (u32 wv = 0; wv < kThreads / 64; ++wv) {
      t1 += red[0][wv];
      t2 += red[1][wv];
    }
    u64 idx = (u64)f * a.nch + k;
    a.csize[idx] = nbytes;
    a.cadler[idx] = (1 + t1) % kAdlerBase | ((n + t2) % kAdlerBase) << 16;
  }
}

// bytes of chunk k's IDAT payload in front of and behind its deflate data
__device__ inline u32 idat_pre(u32 k) { return k == 0 ? kPngZlibHead : 0u; }
__device__ inline u32 idat_post(u32 k, u32 nch) {
  return k + 1 == nch ? kPngZlibTail : 0u;
}

// One workgroup per frame; 256 chunks per step, carry kept across steps.
__global__ void __launch_bounds__(kThreads) png_scan_kernel(PngEncArgs a) {
  __shared__ u32 wave_sum[kThreads / 64];
  u32 f = blockIdx.x, tid = threadIdx.x;
  u32 nch = a.nch;
  const u32* sz = a.csize + (u64)f * nch;
  u32* off = a.coff + (u64)f * nch;
  u32 carry = 0;
  for (u32 k0 = 0; k0 < nch; k0 += kThreads) {
    u32 k = k0 + tid;
    u32 val = k < nch ? 12u + idat_pre(k) + sz[k] + idat_post(k, nch) : 0u;
    u32 all;
    u32 x = block_excl_scan(val, wave_sum, all);
    if (k < nch) off[k] = carry + x;
    carry += all;
  }
  if (tid == 0) {
    a.sizes[f] = kPngHeadBytes + carry + 12;
    const u32* ad = a.cadler + (u64)f * nch;
    u32 v = ad[0];
    for (u32 k = 1; k < nch; ++k)
      v = png_adler_combine(v, ad[k], chunk_len(a, k));
    a.adler[f] = v;
  }
}

// product of two reflected polynomials modulo the CRC polynomial
__host__ __device__ inline u32 crc_mul(u32 x, u32 y) {
  u32 p = 0;
  for (u32 i = 0; i < 32; ++i) {
    if (x & (0x80000000u >> i)) p ^= y;
    y = (y & 1u) ? (y >> 1) ^ kCrcPoly : y >> 1;
  }
  return p;
}

// x^(8 * nbytes) modulo the CRC polynomial
__device__ inline u32 crc_shift(const u32* x2n, u32 nbytes) {
  u32 p = 0x80000000u;  // 1
  for (u32 j = 0; nbytes; ++j, nbytes >>= 1)
    if (nbytes & 1u) p = crc_mul(x2n[(j + 3) & 31], p);
  return p;
}

__device__ inline void store_be32(u8* p, u32 v) {
  p[0] = (u8)(v >> 24);
  p[1] = (u8)(v >> 16);
  p[2] = (u8)(v >> 8);
  p[3] = (u8)v;
}

__global__ void __launch_bounds__(kThreads) png_gather_kernel(PngEncArgs a) {
  __shared__ u32 crc_tab[256];
  __shared__ u32 red[kThreads / 64];
  u32 k = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  u32 nch = a.nch;
  {
    u32 v = tid;
    for (u32 i = 0; i < 8; ++i) v = (v & 1u) ? (v >> 1) ^ kCrcPoly : v >> 1;
    crc_tab[tid] = v;
  }
  __syncthreads();
  u8* file = a.out[f];
  if (k == 0 && tid == 0) {
    const u8 sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (u32 i = 0; i < 8; ++i) file[i] = sig[i];
    u8* h = file + 8;
    store_be32(h, 13);
    h[4] = 'I'; h[5] = 'H'; h[6] = 'D'; h[7] = 'R';
    store_be32(h + 8, (u32)a.w);
    store_be32(h + 12, (u32)a.h);
    h[16] = 8;
    h[17] = a.c == 3 ? 2 : 0;
    h[18] = h[19] = h[20] = 0;
    u32 crc = 0xffffffffu;
    for (u32 i = 4; i < 21; ++i) crc = crc_tab[(crc ^ h[i]) & 0xff] ^ (crc >> 8);
    store_be32(h + 21, ~crc);
  }
  u64 idx = (u64)f * nch + k;
  u32 n = a.csize[idx], pre = idat_pre(k), post = idat_post(k, nch);
  u32 payload = pre + n + post;
  const u8* src = a.staging + idx * kSlot;
  u8* ch = file + kPngHeadBytes + a.coff[idx];
  u8 tail[kPngZlibTail] = {0x03, 0x00, 0, 0, 0, 0};
  if (post) store_be32(tail + 2, a.adler[f]);
  // byte i of what the CRC covers: type, payload
  auto byte_at = [&](u32 i) -> u32 {
    if (i < 4) return (u32)"IDAT"[i];
    i -= 4;
    if (i < pre) return i == 0 ? 0x78u : 0x01u;
    i -= pre;
    if (i < n) return src[i];
    return tail[i - n];
  };
  u32 total = 4 + payload;
  u32 per = (total + kThreads - 1) / kThreads;
  u32 lo = tid * per < total ? tid * per : total;
  u32 hi = lo + per < total ? lo + per : total;
  u32 crc = 0xffffffffu;
  u8* body = ch + 4;
  for (u32 i = lo; i < hi; ++i) {
    u32 b = byte_at(i);
    body[i] = (u8)b;
    crc = crc_tab[(crc ^ b) & 0xff] ^ (crc >> 8);
  }
  crc = ~crc;  // of the slice; 0 for an empty one
  // CRC(A || B) = CRC(A) * x^(8 len B) + CRC(B)
  u32 part = crc_mul(crc_shift(a.x2n, total - hi), crc);
#pragma unroll
  for (u32 d = 32; d >= 1; d >>= 1) part ^= __shfl_xor(part, d, 64);
  if ((tid & 63) == 0) red[tid >> 6] = part;
  __syncthreads();
  if (tid == 0) {
    store_be32(ch, payload);
    store_be32(ch + 8 + payload, red[0] ^ red[1] ^ red[2] ^ red[3]);
    if (k + 1 == nch) {
      const u8 iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D',
                           0xae, 0x42, 0x60, 0x82};
      u8* e = ch + 12 + payload;
      for (u32 i = 0; i < 12; ++i) e[i] = iend[i];
    }
  }
}

u64 align_up(u64 x, u64 a) { return (x + a - 1) / a * a; }

}  // namespace

void png_encode_gpu(const std::vector<const u8*>& frames, i32 h, i32 w, i32 c,
                    DeviceHandle dev, void* stream, std::vector<u8*>& out,
                    std::vector<u64>& sizes) {
  png_check_args(h, w, c);
  SCA_CHECK(dev.is_gpu(), "png_encode_gpu needs a GPU device");
  if (frames.empty()) return;
  PNG_ENC_CHECK(hipSetDevice(dev.id));
  hipStream_t s = (hipStream_t)stream;

  u64 fsz = png_filtered_size(h, w, c);
  u32 nch = png_chunk_count(h, w, c);
  u64 bound = png_size_bound(h, w, c);
  u64 frame_bytes = align_up(fsz, 256) + (u64)nch * kSlot;
  size_t seq_max = (size_t)std::max<u64>(
      1, std::min<u64>({(u64)kMaxFrames, (u64)frames.size(),
                        kStagingBudget / frame_bytes}));
  // one slab-pool allocation: staging, filtered streams, the u32 arrays
  u64 filt_off = align_up((u64)nch * kSlot * seq_max, 256);
  u64 csize_off = filt_off + align_up(fsz * seq_max, 256);
  u64 cadler_off = csize_off + align_up(seq_max * nch * 4, 256);
  u64 coff_off = cadler_off + align_up(seq_max * nch * 4, 256);
  u64 sizes_off = coff_off + align_up(seq_max * nch * 4, 256);
  u64 adler_off = sizes_off + align_up(seq_max * 4, 256);
  u8* staging = new_buffer(dev, adler_off + align_up(seq_max * 4, 256));
  u32 host_sizes[kMaxFrames];
  size_t first_out = out.size();

  try {
    for (size_t c0 = 0; c0 < frames.size(); c0 += seq_max) {
      size_t n = std::min(seq_max, frames.size() - c0);
      PngEncArgs a{};
      a.staging = staging;
      a.filt = staging + filt_off;
      a.csize = reinterpret_cast<u32*>(staging + csize_off);
      a.cadler = reinterpret_cast<u32*>(staging + cadler_off);
      a.coff = reinterpret_cast<u32*>(staging + coff_off);
      a.sizes = reinterpret_cast<u32*>(staging + sizes_off);
      a.adler = reinterpret_cast<u32*>(staging + adler_off);
      a.x2n[0] = 0x40000000u;  // x
      for (u32 k = 1; k < 32; ++k) a.x2n[k] = crc_mul(a.x2n[k - 1], a.x2n[k - 1]);
      a.fsz = fsz;
      a.h = h;
      a.w = w;
      a.c = c;
      a.nch = nch;
      for (size_t i = 0; i < n; ++i) {
        SCA_CHECK(frames[c0 + i], "png encode: null frame pointer");
        a.frames[i] = frames[c0 + i];
      }
      png_filter_kernel<<<dim3((u32)h, (u32)n), kThreads, 0, s>>>(a);
      PNG_ENC_CHECK(hipGetLastError());
      dim3 grid(nch, (u32)n);
      png_deflate_kernel<<<grid, kThreads, 0, s>>>(a);
      PNG_ENC_CHECK(hipGetLastError());
      png_scan_kernel<<<(u32)n, kThreads, 0, s>>>(a);
      PNG_ENC_CHECK(hipGetLastError());
      PNG_ENC_CHECK(hipMemcpyAsync(host_sizes, a.sizes, n * 4,
                                   hipMemcpyDeviceToHost, s));
      PNG_ENC_CHECK(hipStreamSynchronize(s));

      // exact-size outputs, 16-byte aligned, in one block buffer
      u64 total = 0;
      for (size_t i = 0; i < n; ++i) {
        SCA_CHECK(host_sizes[i] > kPngHeadBytes && host_sizes[i] <= bound,
                  "png encode: file size out of range");
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
      png_gather_kernel<<<grid, kThreads, 0, s>>>(a);
      PNG_ENC_CHECK(hipGetLastError());
    }
    // the staging feeds the last gather
    PNG_ENC_CHECK(hipStreamSynchronize(s));
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

}  // namespace sca
