// Progressive JPEG (SOF2) block decoders shared by the CPU decoder
// (jpeg_decode_cpu.cpp) and the HIP decoder
// (kernels/jpeg_progressive_decode.hip). Written from ITU-T T.81 Annex G;
// the refinement scans follow libjpeg's reading of G.1.2.3. Integer-only, so
// the two decoders store the same coefficients and reach the same verdict by
// construction and differ only in which lane runs which restart segment.
//
// A scan codes a band Ss..Se of the zig-zag sequence at one bit position:
//   DC first       Huffman size + bits of the DC difference, stored << Al
//   DC refinement  one bit per block, OR-ed in at 1 << Al
//   AC first       run/size symbols; EOBn ends the band for 2^n + bits
//                  blocks (this one included); values stored << Al
//   AC refinement  run/size symbols with size 1 place new +-(1 << Al)
//                  coefficients; every coefficient that is already non-zero
//                  and is passed on the way takes one correction bit, which
//                  moves it away from zero by 1 << Al when that bit is not
//                  yet set; EOBn as above, and the blocks of an EOB run take
//                  their correction bits too
// The caller carries `eobrun` (blocks still covered by an EOB run, at most
// 32767) from block to block and resets it with the DC predictor at every
// restart segment.
//
// Nothing here reads outside the [begin, end) byte range of the bit reader
// or writes outside the 64-entry block; every loop ends after at most 64
// symbols, and a run never takes the index past Se.
#pragma once

#include "jpeg_decode_common.h"

namespace sca {

// Largest Al (and Ah) a scan may carry, T.81 Table B.3.
constexpr u32 kJpegProgMaxAl = 13;

JPEG_HD inline u32 jpeg_prog_bits(JpegBitReader& br, u32 k) {
  if (k == 0) return 0;
  jpeg_bits_fill(br);
  u32 v = jpeg_bits_peek(br, k);
  jpeg_bits_skip(br, k);
  return v;
}

JPEG_HD inline u32 jpeg_prog_fail(const JpegBitReader& br, u32 cause) {
  return br.exhausted ? (u32)kJpegExhausted : cause;
}

// G.1.2.1, first scan: `pred` is the predictor of the point-transformed DC.
JPEG_HD inline u32 jpeg_prog_dc_first(JpegBitReader& br, const JpegHuff& dc,
                                      u32 al, i32& pred, i16* blk) {
  i32 s = jpeg_huff_symbol(br, dc);
  if (s < 0 || s > 15) return jpeg_prog_fail(br, kJpegBadCode);
  pred = jpeg_clamp_i16(pred + jpeg_receive_extend(br, (u32)s));
  if (br.exhausted) return kJpegExhausted;
  blk[0] = (i16)jpeg_clamp_i16(pred * (1 << al));
  return kJpegBlockOk;
}

// G.1.2.1, refinement: one bit
JPEG_HD inline u32 jpeg_prog_dc_refine(JpegBitReader& br, u32 al, i16* blk) {
  u32 bit = jpeg_prog_bits(br, 1);
  if (br.exhausted) return kJpegExhausted;
  if (bit) blk[0] = (i16)(blk[0] | (i16)(1 << al));
  return kJpegBlockOk;
}

// G.1.2.2
JPEG_HD inline u32 jpeg_prog_ac_first(JpegBitReader& br, const JpegHuff& ac,
                                      const u8* zz2nat, u32 ss, u32 se, u32 al,
                                      u32& eobrun, i16* blk) {
  if (eobrun > 0) {
    --eobrun;
    return kJpegBlockOk;
  }
  u32 k = ss;
  while (k <= se) {
    i32 rs = jpeg_huff_symbol(br, ac);
    if (rs < 0) return jpeg_prog_fail(br, kJpegBadCode);
    u32 r = (u32)rs >> 4, sz = (u32)rs & 15u;
    if (sz == 0) {
      if (r != 15) {  // EOBr: 2^r + r bits blocks, this one included
        eobrun = (1u << r) + jpeg_prog_bits(br, r) - 1;
        break;
      }
      k += 16;  // ZRL
      if (k > se + 1) return jpeg_prog_fail(br, kJpegBadIndex);
      continue;
    }
    k += r;
    if (k > se) return jpeg_prog_fail(br, kJpegBadIndex);
    i32 v = jpeg_receive_extend(br, sz);
    if (br.exhausted) return kJpegExhausted;
    blk[zz2nat[k]] = (i16)jpeg_clamp_i16(v * (1 << al));
    ++k;
  }
  return br.exhausted ? (u32)kJpegExhausted : (u32)kJpegBlockOk;
}

// one correction bit for a coefficient that is already non-zero
JPEG_HD inline void jpeg_prog_correct(JpegBitReader& br, u32 al, i16* c) {
  if (!jpeg_prog_bits(br, 1)) return;
  i32 v = *c, p1 = 1 << al;
  if ((v & p1) == 0) *c = (i16)jpeg_clamp_i16(v >= 0 ? v + p1 : v - p1);
}

// G.1.2.3
JPEG_HD inline u32 jpeg_prog_ac_refine(JpegBitReader& br, const JpegHuff& ac,
                                       const u8* zz2nat, u32 ss, u32 se,
                                       u32 al, u32& eobrun, i16* blk) {
  u32 k = ss;
  if (eobrun == 0) {
    while (k <= se) {
      i32 rs = jpeg_huff_symbol(br, ac);
      if (rs < 0) return jpeg_prog_fail(br, kJpegBadCode);
      u32 r = (u32)rs >> 4, sz = (u32)rs & 15u;
      i32 nv = 0;
      if (sz != 0) {
        if (sz != 1) return jpeg_prog_fail(br, kJpegBadCode);
        nv = jpeg_prog_bits(br, 1) ? (1 << al) : -(1 << al);
      } else if (r != 15) {
        // EOBr; this block's remaining correction bits are read below
        eobrun = (1u << r) + jpeg_prog_bits(br, r);
        break;
      }
      // pass r coefficients that are still zero (16 for ZRL), correcting
      // the non-zero ones on the way; stop on the zero after them
      u32 zeros = sz ? r : 15u;
      bool placed = false;
      while (k <= se) {
        i16* c = blk + zz2nat[k];
        if (*c != 0) {
          jpeg_prog_correct(br, al, c);
        } else {
          if (zeros == 0) {
            placed = true;
            break;
          }
          --zeros;
        }
        ++k;
      }
      if (!placed) return jpeg_prog_fail(br, kJpegBadIndex);
      if (sz) blk[zz2nat[k]] = (i16)nv;
      ++k;
      if (br.exhausted) return kJpegExhausted;
    }
  }
  if (eobrun > 0) {
    for (; k <= se; ++k) {
      i16* c = blk + zz2nat[k];
      if (*c != 0) jpeg_prog_correct(br, al, c);
    }
    --eobrun;
  }
  return br.exhausted ? (u32)kJpegExhausted : (u32)kJpegBlockOk;
}

// One block of a scan. `tab` is the component's DC table when ss == 0 and
// its AC table otherwise; 0 <= ss <= se <= 63, al <= kJpegProgMaxAl (the
// parser checks, the callers clamp).
JPEG_HD inline u32 jpeg_prog_block(JpegBitReader& br, const JpegHuff& tab,
                                   const u8* zz2nat, u32 ss, u32 se, u32 ah,
                                   u32 al, i32& pred, u32& eobrun, i16* blk) {
  if (ss == 0)
    return ah == 0 ? jpeg_prog_dc_first(br, tab, al, pred, blk)
                   : jpeg_prog_dc_refine(br, al, blk);
  return ah == 0 ? jpeg_prog_ac_first(br, tab, zz2nat, ss, se, al, eobrun, blk)
                 : jpeg_prog_ac_refine(br, tab, zz2nat, ss, se, al, eobrun,
                                       blk);
}

// ---- geometry of a single-component scan ----
// Such a scan walks the blocks of the component's own raster,
// ceil(comp_w / 8) x ceil(comp_h / 8), row by row (T.81 A.2.2), not the
// MCU-padded one.
JPEG_HD inline void jpeg_prog_comp_blocks(const JpegDecGeom& g, u32 comp,
                                          u32& bw, u32& bh) {
  u32 cw = comp == 0 ? (u32)g.w : g.cw, ch = comp == 0 ? (u32)g.h : g.ch;
  bw = (cw + 7) / 8;
  bh = (ch + 7) / 8;
}

// Block (bx, by) of a component's raster -> index of the block in MCU order,
// m * blocks_per_mcu + b with (m, b) as jpeg_block_pos takes them.
JPEG_HD inline u32 jpeg_prog_block_index(const JpegDecGeom& g, u32 comp,
                                         u32 bx, u32 by) {
  if (g.nc == 1) return by * g.mcus_x + bx;
  if (comp == 0) {
    u32 m = (by / g.vs) * g.mcus_x + bx / g.hs;
    return m * g.blocks_per_mcu + (by % g.vs) * g.hs + bx % g.hs;
  }
  return (by * g.mcus_x + bx) * g.blocks_per_mcu + g.hs * g.vs + comp - 1;
}

// component of block b of an MCU
JPEG_HD inline u32 jpeg_prog_block_comp(const JpegDecGeom& g, u32 b) {
  u32 ny = g.hs * g.vs;
  if (g.nc == 1 || b < ny) return 0;
  u32 c = b - ny + 1;
  return c > 2 ? 2u : c;
}

}  // namespace sca
