// Self-synchronising parallel Huffman decode of a JPEG scan that has no
// restart markers (Klein & Wiseman; Weissenberger & Schmidt, "Accelerating
// JPEG Decompression on GPUs", 2021), shared by the CPU model
// (jpeg_sync_cpu.cpp) and the HIP kernels (kernels/jpeg_sync_decode.hip).
// Integer-only, host and device, on top of jpeg_decode_common.h.
//
// The scan is cut into chunks of `chunk_bytes` raw (still byte-stuffed)
// bytes. A decoder state at a symbol boundary is (bit position in the scan,
// block index inside the MCU, zig-zag index); zig-zag index 0 means the next
// symbol is a DC code. Every chunk is decoded speculatively from a guessed
// state, then again from its predecessor's exit state until the exit states
// stop changing; a writing pass from the final states stores the
// coefficients and verifies that every chunk ends where the speculative
// pass said it would. Soundness rests on that verification alone: chunk 0
// starts from the true state, so if every chunk's writing walk ends at its
// recorded exit, every chunk started from the true state.
//
// Bit positions are relative to the first byte of the scan. Byte i of the
// scan is a stuffed 00 exactly when i > 0 and bytes i-1, i are FF 00 (an FF
// is always a data byte for JpegBitReader), whichever lane looks at it; a
// position never lies inside a stuffed byte, and a chunk whose first byte is
// one starts a byte later.
//
// Nothing here reads outside [begin, end) of the scan, writes a coefficient
// outside block indices [0, nblk) x 64, or loops longer than the bit length
// it is asked to walk, whatever the bytes are.
#pragma once

#include "jpeg_decode_common.h"

namespace sca {

// Default chunk size; chosen among 32, 64, 128 and 256 from the A/B in
// profiles/jpeg_decode.md (the fastest on smooth 1080p files, level with
// the others on noise).
constexpr u32 kJpegSyncChunkBytes = 128;
// Chunks of one file that synchronise inside one workgroup.
constexpr u32 kJpegSyncGroupChunks = 256;
// Rounds of synchronisation across groups that are run at most. A file of G
// groups is exact after G - 1 rounds; a larger file relies on the sync
// distance being short against a group, and on the verification otherwise.
constexpr u32 kJpegSyncMaxRounds = 3;
// Longer scans are left to the serial decoder: bit positions are 32-bit.
constexpr u32 kJpegSyncMaxScanBytes = 1u << 28;

// why a row failed verification, next to JpegBlockStatus 1..3
enum JpegSyncStatus : u32 {
  kJpegSyncMismatch = 4,  // a writing walk did not end at the recorded exit
  kJpegSyncCount = 5,     // the chunks hold another number of blocks
  kJpegSyncDcRange = 6,   // a running DC value leaves int16
};

struct JpegSyncState {
  u32 bit;  // position in the scan, bits
  u32 blk;  // block inside the MCU
  u32 zz;   // next zig-zag index; 0: a DC code comes next
};
JPEG_HD inline bool jpeg_sync_same(const JpegSyncState& a,
                                   const JpegSyncState& b) {
  return a.bit == b.bit && a.blk == b.blk && a.zz == b.zz;
}

// what is kept per chunk between the passes
struct JpegSyncChunk {
  JpegSyncState entry, exit;
  u32 blocks;  // blocks completed between them
  u32 status;  // kJpegBlockOk, or why the walk gave up
};

struct JpegSyncScan {
  const u8* p;
  u32 begin, end;  // the scan, bytes of p
  u32 blocks_per_mcu;
  u32 ny;  // luma blocks per MCU
  const JpegHuff* dc;  // [3], per component
  const JpegHuff* ac;
};

JPEG_HD inline bool jpeg_sync_valid_chunk_bytes(u32 cb) {
  return cb >= 4 && (cb & (cb - 1)) == 0;
}
JPEG_HD inline u32 jpeg_sync_chunk_count(u32 scan_bytes, u32 cb) {
  u32 n = scan_bytes / cb + (scan_bytes % cb ? 1u : 0u);
  return n ? n : 1u;
}

JPEG_HD inline bool jpeg_sync_is_stuffing(const JpegSyncScan& sc, u32 byte) {
  u32 i = sc.begin + byte;
  return byte > 0 && i < sc.end && sc.p[i] == 0 && sc.p[i - 1] == 0xffu;
}

// First bit of chunk c; chunk `count` starts at the end of the scan.
JPEG_HD inline u32 jpeg_sync_chunk_start(const JpegSyncScan& sc, u32 c,
                                         u32 cb, u32 count) {
  u32 len = sc.end - sc.begin;
  if (c >= count) return len * 8;
  u32 byte = c * cb;
  if (jpeg_sync_is_stuffing(sc, byte)) ++byte;
  return byte * 8;
}

// Position of the next unconsumed bit of a reader opened on the scan: walk
// back from the load position over the data bytes still held.
JPEG_HD inline u32 jpeg_sync_bitpos(const JpegBitReader& br,
                                    const JpegSyncScan& sc) {
  u32 real = br.n - br.phantom;
  u32 i = br.pos;
  for (u32 k = (real + 7) >> 3; k; --k) {
    --i;
    if (i > sc.begin && br.p[i] == 0 && br.p[i - 1] == 0xffu) --i;
  }
  return (i - sc.begin) * 8 + ((8 - (real & 7u)) & 7u);
}

struct JpegSyncWalk {
  JpegSyncState exit;
  u32 blocks;
  u32 status;
  bool by_count;  // the writing walk stopped at the file's block count
};

// Walk the symbols from `entry` to the first symbol boundary at or past
// `end_bit`. kWrite = false is the speculative chunk decode: it stores
// nothing, and on a bad code or index it gives up with exit (end_bit, 0, 0),
// keeping the blocks counted so far. kWrite = true is the writing chunk
// decode from a true entry: `first_block` is the index of the block the
// entry lies in; every coefficient goes to coef[block * 64 + zz2nat[k]] (the
// DC difference to [block * 64]), and the walk stops once the block index
// reaches nblk, so the 1-bits that pad the last byte are never decoded.
template <bool kWrite>
JPEG_HD inline JpegSyncWalk jpeg_sync_walk(const JpegSyncScan& sc,
                                           JpegSyncState entry, u32 end_bit,
                                           u32 first_block, u32 nblk,
                                           const u8* zz2nat, i16* coef) {
  JpegSyncWalk r;
  r.exit = entry;
  r.blocks = 0;
  r.status = kJpegBlockOk;
  r.by_count = false;
  u32 len_bits = (sc.end - sc.begin) * 8;
  if (end_bit > len_bits) end_bit = len_bits;
  if (entry.bit >= end_bit) return r;
  JpegSyncState s = entry;
  u32 status = kJpegBadIndex;
  if (s.blk < sc.blocks_per_mcu && s.zz < 64) {
    JpegBitReader br;
    jpeg_bits_init(br, sc.p, sc.begin + (s.bit >> 3), sc.end);
    jpeg_bits_fill(br);
    jpeg_bits_skip(br, s.bit & 7u);
    // a symbol takes at least one bit
    for (u32 budget = end_bit - s.bit; budget; --budget) {
      u32 b = first_block + r.blocks;
      if (kWrite && b >= nblk) {
        r.by_count = true;
        s.bit = jpeg_sync_bitpos(br, sc);
        r.exit = s;
        return r;
      }
      u32 comp = s.blk < sc.ny ? 0u : s.blk - sc.ny + 1;
      if (comp > 2) comp = 2;
      bool done = false;
      if (s.zz == 0) {
        i32 sym = jpeg_huff_symbol(br, sc.dc[comp]);
        if (sym < 0 || sym > 15) {
          status = br.exhausted ? kJpegExhausted : kJpegBadCode;
          break;
        }
        i32 v = jpeg_receive_extend(br, (u32)sym);
        if (kWrite && !br.exhausted) coef[(size_t)b * 64] = (i16)v;
        s.zz = 1;
      } else {
        i32 rs = jpeg_huff_symbol(br, sc.ac[comp]);
        if (rs < 0) {
          status = br.exhausted ? kJpegExhausted : kJpegBadCode;
          break;
        }
        u32 run = (u32)rs >> 4, sz = (u32)rs & 15u;
        if (sz == 0) {
          if (run == 15) {  // ZRL
            s.zz += 16;
            if (s.zz > 64) {
              status = kJpegBadIndex;
              break;
            }
            done = s.zz == 64;
          } else if (run != 0) {
            status = kJpegBadCode;
            break;
          } else {
            done = true;  // EOB
          }
        } else {
          u32 k = s.zz + run;
          if (k > 63) {
            status = kJpegBadIndex;
            break;
          }
          i32 v = jpeg_receive_extend(br, sz);
          if (kWrite && !br.exhausted)
            coef[(size_t)b * 64 + zz2nat[k]] = (i16)v;
          s.zz = k + 1;
          done = s.zz == 64;
        }
      }
      if (br.exhausted) {
        status = kJpegExhausted;
        break;
      }
      if (done) {
        s.zz = 0;
        s.blk = s.blk + 1 == sc.blocks_per_mcu ? 0u : s.blk + 1;
        ++r.blocks;
      }
      // stuffed bytes only move the true position further back, so this
      // cheap bound decides all but the last few symbols of a chunk
      if ((br.pos - sc.begin) * 8 - (br.n - br.phantom) >= end_bit) {
        u32 pos = jpeg_sync_bitpos(br, sc);
        if (pos >= end_bit) {
          s.bit = pos;
          r.exit = s;
          return r;
        }
      }
    }
  }
  r.exit.bit = end_bit;
  r.exit.blk = 0;
  r.exit.zz = 0;
  r.status = status;
  return r;
}

// One step of the synchronisation, for the chunk whose current record is
// `c`: decode again from `entry` if that is not what the record was decoded
// from. True when the exit changed.
JPEG_HD inline bool jpeg_sync_step(const JpegSyncScan& sc, JpegSyncChunk& c,
                                   const JpegSyncState& entry, u32 end_bit) {
  if (jpeg_sync_same(entry, c.entry)) return false;
  JpegSyncWalk w =
      jpeg_sync_walk<false>(sc, entry, end_bit, 0, 0, nullptr, nullptr);
  bool changed = !jpeg_sync_same(w.exit, c.exit);
  c.entry = entry;
  c.exit = w.exit;
  c.blocks = w.blocks;
  c.status = w.status;
  return changed;
}

// The first decode of a chunk, from the guess (chunk start, 0, 0); for chunk
// 0 the guess is the true state.
JPEG_HD inline void jpeg_sync_first(const JpegSyncScan& sc, JpegSyncChunk& c,
                                    u32 start_bit, u32 end_bit) {
  c.entry.bit = start_bit;
  c.entry.blk = 0;
  c.entry.zz = 0;
  JpegSyncWalk w =
      jpeg_sync_walk<false>(sc, c.entry, end_bit, 0, 0, nullptr, nullptr);
  c.exit = w.exit;
  c.blocks = w.blocks;
  c.status = w.status;
}

// The writing decode of chunk `rec` from the true entry; 0 when it agrees
// with the record, else the status to report for the row.
JPEG_HD inline u32 jpeg_sync_write(const JpegSyncScan& sc,
                                   const JpegSyncChunk& rec,
                                   const JpegSyncState& entry, u32 end_bit,
                                   u32 first_block, u32 nblk,
                                   const u8* zz2nat, i16* coef) {
  if (first_block >= nblk) return kJpegBlockOk;
  JpegSyncWalk w =
      jpeg_sync_walk<true>(sc, entry, end_bit, first_block, nblk, zz2nat, coef);
  if (w.status != kJpegBlockOk) return w.status;
  if (w.by_count) return kJpegBlockOk;  // the block total is checked apart
  if (!jpeg_sync_same(w.exit, rec.exit) || w.blocks != rec.blocks)
    return kJpegSyncMismatch;
  return kJpegBlockOk;
}

// rounds across groups for a file of `groups` groups
JPEG_HD inline u32 jpeg_sync_rounds(u32 groups) {
  u32 r = groups ? groups - 1 : 0;
  return r < kJpegSyncMaxRounds ? r : kJpegSyncMaxRounds;
}

}  // namespace sca
