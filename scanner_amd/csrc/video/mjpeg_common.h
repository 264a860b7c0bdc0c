// The restart-segment index of one Motion-JPEG sample, shared by the host
// reference (mjpeg_index_ref, below) and the HIP kernel
// (kernels/mjpeg_index.hip). HIP-free; format: mjpeg.h.
//
// Given a sample whose first `header_len` bytes equal the item's reference
// header (SOI .. SOS of sample 0), the index finds what jpeg_parse finds in
// the scan that follows: the RSTn markers, in order, and the EOI that ends
// the scan. It does so from a classification of single byte positions that
// does not depend on where a walk started, so every lane can classify its
// own bytes.
//
// The rule: byte i >= header_len starts a marker iff b[i] == FF, b[i+1]
// exists, and b[i+1] is neither 00 nor FF.
//
// Why this equals the serial loop of jpeg_parse. That loop walks the scan
// with a cursor. At a byte that is not FF it steps by one. At an FF it looks
// at the next byte: 00 (a stuffed data byte) steps by two, FF (a fill byte)
// steps by one, anything else is a marker at the cursor, and an RSTn then
// steps by two. So the only positions the cursor never stands on are those
// directly behind an FF whose follower is 00, or is a marker code. Such a
// skipped byte is 00 or a marker code, and no marker code is FF: a skipped
// byte is never FF. Hence the cursor stands on every FF of the scan up to
// the first marker that is not RSTn, where it stops. Standing on an FF, the
// loop calls it a marker exactly when the follower is neither 00 nor FF,
// which is the rule. An FF that is the last byte of the sample has no
// follower: the loop gives up there ("truncated"), and the rule does not
// call it a marker, so no end of scan is found either way.
//
// Acceptance (all of jpeg_parse's checks on the scan, for a header with a
// DRI segment):
//   - a first marker that is not RSTn exists, and it is EOI; what follows
//     it is ignored;
//   - the RSTn before it number exactly nseg - 1, and the k-th carries
//     k mod 8;
//   - the scan holds at least min_scan_bytes bytes.
// A sample that fails is reported by a status word and is decoded by the
// serial path instead. Several causes may hold at once; the status is the
// smallest of their codes, which does not depend on the order in which
// lanes meet them.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MJPEG_HD __host__ __device__
#else
#define MJPEG_HD
#endif

namespace sca {

enum MjpegIndexStatus : uint32_t {
  kMjpegOk = 0,
  kMjpegHeaderDiffers = 1,  // shorter than, or not equal to, the reference
  kMjpegNoEnd = 2,          // no marker other than RSTn: truncated
  kMjpegBadEnd = 3,         // the first such marker is not EOI
  kMjpegRstSequence = 4,    // RST k does not carry k mod 8
  kMjpegRstCount = 5,       // not nseg - 1 restart markers
  kMjpegScanShort = 6,      // fewer entropy bytes than the geometry needs
  kMjpegStatusNone = 0xffffffffu,  // "no failure yet" while an index runs
};

// What the index needs from the reference header.
struct MjpegIndexParams {
  uint32_t header_len;      // offset of the first entropy-coded byte
  uint32_t nseg;            // restart segments of the geometry, >= 1
  uint32_t mcus_per_seg;    // the restart interval
  uint32_t nmcu;
  uint32_t min_scan_bytes;  // ceil(nmcu * blocks_per_mcu * 2 / 8)
};

// One restart segment, the layout of JpegDecSeg and of JpegSegment.
struct MjpegSeg {
  uint32_t begin, end;
  uint32_t first_mcu, mcu_count;
};

// Does byte i of a sample of `size` bytes start a marker? Reads b[i] and,
// only when i + 1 < size, b[i + 1].
MJPEG_HD inline bool mjpeg_is_marker(const uint8_t* b, size_t size, size_t i) {
  if (b[i] != 0xffu || i + 1 >= size) return false;
  uint8_t m = b[i + 1];
  return m != 0x00u && m != 0xffu;
}
// The same from the two bytes; `have_next` is i + 1 < size.
MJPEG_HD inline bool mjpeg_is_marker2(uint32_t b0, uint32_t b1,
                                      bool have_next) {
  return b0 == 0xffu && have_next && b1 != 0x00u && b1 != 0xffu;
}
MJPEG_HD inline bool mjpeg_is_rst(uint32_t code) {
  return code >= 0xd0u && code <= 0xd7u;
}
// Is restart marker number k, carrying `code`, acceptable?
MJPEG_HD inline bool mjpeg_rst_in_sequence(uint32_t k, uint32_t code) {
  return code - 0xd0u == (k & 7u);
}
// MCUs of segment k.
MJPEG_HD inline void mjpeg_seg_mcus(const MjpegIndexParams& p, uint32_t k,
                                    uint32_t& first, uint32_t& count) {
  first = k * p.mcus_per_seg;
  count = k + 1 < p.nseg ? p.mcus_per_seg : p.nmcu - first;
}
// The verdict once the scan has been classified. `end` is the position of
// the first marker that is not RSTn, or `size` when there is none; `nrst`
// counts the RSTn before `end`; `failed` is the smallest failure code met
// while classifying, or kMjpegStatusNone.
MJPEG_HD inline uint32_t mjpeg_verdict(const MjpegIndexParams& p, size_t size,
                                       size_t end, uint32_t end_code,
                                       uint32_t nrst, uint32_t failed) {
  uint32_t st = failed;
  const uint32_t scan_short = kMjpegScanShort, rst_count = kMjpegRstCount,
                 no_end = kMjpegNoEnd, bad_end = kMjpegBadEnd;
  if (end - p.header_len < p.min_scan_bytes) st = st < scan_short ? st : scan_short;
  if (nrst != p.nseg - 1) st = st < rst_count ? st : rst_count;
  if (end >= size) st = st < no_end ? st : no_end;
  else if (end_code != 0xd9u) st = st < bad_end ? st : bad_end;
  return st == kMjpegStatusNone ? (uint32_t)kMjpegOk : st;
}

// Host reference: the index of one sample, serially, from the rule above.
// `segs` has room for p.nseg records; on a status other than kMjpegOk its
// content is unspecified. Offsets are relative to `sample` plus `rebase`.
// Reads only sample[0, size).
inline uint32_t mjpeg_index_ref(const uint8_t* sample, size_t size,
                                const uint8_t* ref_header,
                                const MjpegIndexParams& p, uint32_t rebase,
                                MjpegSeg* segs) {
  if (size < p.header_len) return kMjpegHeaderDiffers;
  for (size_t i = 0; i < p.header_len; ++i)
    if (sample[i] != ref_header[i]) return kMjpegHeaderDiffers;
  uint32_t failed = kMjpegStatusNone;
  size_t end = size;
  uint32_t end_code = 0, nrst = 0;
  for (size_t i = p.header_len; i < size; ++i) {
    if (!mjpeg_is_marker(sample, size, i)) continue;
    uint32_t code = sample[i + 1];
    if (!mjpeg_is_rst(code)) {
      end = i;
      end_code = code;
      break;
    }
    if (nrst + 1 < p.nseg) {
      if (!mjpeg_rst_in_sequence(nrst, code) && kMjpegRstSequence < failed)
        failed = kMjpegRstSequence;
      segs[nrst].end = rebase + (uint32_t)i;
      segs[nrst + 1].begin = rebase + (uint32_t)i + 2;
    }
    ++nrst;
  }
  uint32_t st = mjpeg_verdict(p, size, end, end_code, nrst, failed);
  if (st != kMjpegOk) return st;
  segs[0].begin = rebase + p.header_len;
  segs[p.nseg - 1].end = rebase + (uint32_t)end;
  for (uint32_t k = 0; k < p.nseg; ++k)
    mjpeg_seg_mcus(p, k, segs[k].first_mcu, segs[k].mcu_count);
  return kMjpegOk;
}

}  // namespace sca
