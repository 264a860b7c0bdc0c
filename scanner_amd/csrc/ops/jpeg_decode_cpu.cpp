// JPEG parser and the sequential decoder, baseline and progressive: the
// definition of the pixels the HIP decoders (kernels/jpeg_decode.hip,
// kernels/jpeg_progressive_decode.hip) have to reproduce. Marker syntax from
// ITU-T T.81 Annex B, the scan script rules from G.1.1.1.1; arithmetic:
// jpeg_decode_common.h, jpeg_progressive_common.h. HIP-free.
#include <algorithm>

#include "image_decode.h"
#include "jpeg_progressive_common.h"

namespace sca {

namespace {

// bounds-checked big-endian reader over the file
struct Reader {
  const u8* p;
  size_t n;
  size_t pos = 0;
  u32 u8_at(size_t i, const char* what) const {
    SCA_CHECK(i < n, std::string("truncated JPEG: ") + what);
    return p[i];
  }
  u32 u16_at(size_t i, const char* what) const {
    SCA_CHECK(i + 1 < n, std::string("truncated JPEG: ") + what);
    return (u32)p[i] << 8 | p[i + 1];
  }
};

// T.81 Figure A.6, generated: walk the anti-diagonals
void make_zigzag(u8 (&zz2nat)[64]) {
  int k = 0;
  for (int s = 0; s < 15; ++s) {
    int lo = std::max(0, s - 7), hi = std::min(s, 7);
    for (int i = lo; i <= hi; ++i) {
      // even diagonals run bottom-left to top-right
      int r = (s & 1) ? i : s - i;
      zz2nat[k++] = (u8)(r * 8 + (s - r));
    }
  }
}

const char* sof_name(u32 m) {
  switch (m) {
    case 0xc2: return "progressive JPEG (SOF2) is not supported";
    case 0xc3: return "lossless JPEG (SOF3) is not supported";
    case 0xc9: case 0xca: case 0xcb: case 0xcd: case 0xce: case 0xcf:
      return "arithmetic-coded JPEG is not supported";
    default: return "differential/hierarchical JPEG is not supported";
  }
}

// Splits the entropy-coded data of scan `k` of a progressive file, which
// starts at `start`, at its RSTn markers. Returns the offset of the marker
// that ends the scan. The baseline rules, with the scan in the message.
size_t walk_progressive_scan(const u8* data, size_t size, size_t start,
                             u32 k, JpegScan& sc) {
  std::string in_scan = " in scan " + std::to_string(k);
  u32 ri = sc.restart_interval;
  u32 per_seg = ri ? ri : sc.units;
  u32 nseg = (sc.units + per_seg - 1) / per_seg;
  size_t i = start, seg_begin = start;
  bool ended = false;
  while (i < size) {
    if (data[i] != 0xff) {
      ++i;
      continue;
    }
    if (i + 1 >= size) break;  // a lone FF at the very end: truncated
    u32 m = data[i + 1];
    if (m == 0) {
      i += 2;
    } else if (m == 0xff) {
      ++i;  // fill byte
    } else if (m >= 0xd0 && m <= 0xd7) {
      SCA_CHECK(ri != 0, "restart marker without a DRI segment in force" +
                             in_scan);
      u32 n = (u32)sc.segments.size();
      SCA_CHECK(n + 1 < nseg,
                "more restart markers than restart intervals" + in_scan);
      SCA_CHECK(m - 0xd0 == (n & 7),
                "restart markers out of sequence: RST" +
                    std::to_string(m - 0xd0) + " where RST" +
                    std::to_string(n & 7) + " belongs" + in_scan);
      sc.segments.push_back({(u32)seg_begin, (u32)i, n * per_seg, per_seg});
      i += 2;
      seg_begin = i;
    } else {
      ended = true;
      break;
    }
  }
  SCA_CHECK(ended, "truncated JPEG: no EOI marker after scan " +
                       std::to_string(k));
  u32 n = (u32)sc.segments.size();
  SCA_CHECK(n + 1 == nseg,
            "scan " + std::to_string(k) + " has " + std::to_string(n + 1) +
                " restart segments, its size and restart interval need " +
                std::to_string(nseg));
  sc.segments.push_back(
      {(u32)seg_begin, (u32)i, n * per_seg, sc.units - n * per_seg});
  // every block of a DC-first scan costs at least one bit: a header that
  // promises more blocks than the scan can hold is refused before the
  // coefficient buffer is allocated for it
  if (sc.ss == 0 && sc.ah == 0)
    SCA_CHECK(((u64)i - start) * 8 >= (u64)sc.units * sc.blocks_per_unit,
              "truncated JPEG: the scan is too short for the image size (scan " +
                  std::to_string(k) + ")");
  return i;
}

// The parser. `full` false: stop at the first scan (jpeg_parse_header).
// Returns the offset of the first entropy-coded byte.
size_t parse_markers(const u8* data, size_t size, JpegInfo& info,
                     JpegParseOptions opt, bool full);

}  // namespace

bool jpeg_progressive_option(const std::string& value, const char* who) {
  SCA_CHECK(value == "reject" || value == "decode",
            std::string(who) + " supports progressive=reject|decode, got '" +
                value + "'");
  return value == "decode";
}

bool is_jpeg(const u8* d, size_t n) {
  return n >= 2 && d[0] == 0xff && d[1] == 0xd8;
}

std::string jpeg_entropy_error(u32 status, u32 segment) {
  const char* what = status == kJpegBadCode    ? "invalid Huffman code"
                     : status == kJpegBadIndex ? "coefficient index past 63"
                                               : "segment ends inside a block";
  return std::string("corrupt JPEG entropy data: ") + what +
         " in restart segment " + std::to_string(segment);
}

std::string jpeg_entropy_error(u32 status, u32 segment, u32 scan) {
  return jpeg_entropy_error(status, segment) + " of scan " +
         std::to_string(scan);
}

size_t jpeg_parse_header(const u8* data, size_t size, JpegInfo& info,
                         JpegParseOptions opt) {
  return parse_markers(data, size, info, opt, false);
}

namespace {

size_t parse_markers(const u8* data, size_t size, JpegInfo& info,
                     JpegParseOptions opt, bool full) {
  SCA_CHECK(data != nullptr && is_jpeg(data, size),
            "not a JPEG file (no SOI marker)");
  SCA_CHECK(size < (1ull << 31), "JPEG file of 2 GiB or more");
  Reader r{data, size};
  info = JpegInfo{};
  make_zigzag(info.zz2nat);

  u16 qt[4][64];
  bool have_q[4] = {false, false, false, false};
  JpegHuff huff[2][4];
  bool have_h[2][4] = {};
  bool have_sof = false;
  i32 h = 0, w = 0, nc = 0;
  u32 comp_id[3] = {0, 0, 0}, comp_hv[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
  size_t scan = 0;  // first entropy-coded byte
  // progressive: Al of the last scan over coefficient k of component c, or
  // -1 while none has coded it
  int last_al[3][64];
  for (auto& row : last_al) std::fill(row, row + 64, -1);
  bool ended = false;  // progressive: EOI seen after the last scan

  size_t pos = 2;
  while (!scan || (info.progressive && full && !ended)) {
    SCA_CHECK(r.u8_at(pos, "marker expected") == 0xff,
              "JPEG marker expected at byte " + std::to_string(pos));
    while (r.u8_at(pos + 1, "marker code") == 0xff) ++pos;  // fill bytes
    u32 m = data[pos + 1];
    pos += 2;
    if (m == 0xd9 && !info.scans.empty()) {
      ended = true;
      break;
    }
    SCA_CHECK(m != 0xd9, "JPEG ends (EOI) before any scan");
    SCA_CHECK(m != 0xd8, "second SOI marker");
    SCA_CHECK(m != 0 && !(m >= 0xd0 && m <= 0xd7),
              "restart marker or stuffed byte outside a scan");
    if (m == 0x01) continue;  // TEM: no payload
    u32 len = r.u16_at(pos, "segment length");
    SCA_CHECK(len >= 2 && pos + len <= size,
              "truncated JPEG: segment of marker 0x" +
                  std::string(1, "0123456789abcdef"[m >> 4]) +
                  std::string(1, "0123456789abcdef"[m & 15]) +
                  " runs past the end");
    const u8* s = data + pos + 2;
    u32 n = len - 2;
    pos += len;
    if (m == 0xdb) {  // DQT
      u32 i = 0;
      while (i < n) {
        u32 pq = s[i] >> 4, tq = s[i] & 15;
        SCA_CHECK(pq <= 1 && tq <= 3, "bad DQT precision or table id");
        u32 need = 1 + 64 * (pq + 1);
        SCA_CHECK(i + need <= n, "truncated JPEG: DQT table");
        for (u32 k = 0; k < 64; ++k) {
          u32 v = pq ? (u32)s[i + 1 + 2 * k] << 8 | s[i + 2 + 2 * k]
                     : s[i + 1 + k];
          qt[tq][info.zz2nat[k]] = (u16)v;
        }
        have_q[tq] = true;
        i += need;
      }
    } else if (m == 0xc4) {  // DHT
      u32 i = 0;
      while (i < n) {
        u32 tc = s[i] >> 4, th = s[i] & 15;
        SCA_CHECK(tc <= 1 && th <= 3, "bad DHT class or table id");
        SCA_CHECK(i + 17 <= n, "truncated JPEG: DHT counts");
        u32 total = 0;
        for (u32 k = 0; k < 16; ++k) total += s[i + 1 + k];
        SCA_CHECK(total <= 256 && i + 17 + total <= n,
                  "truncated JPEG: DHT values");
        SCA_CHECK(jpeg_build_huff(s + i + 1, s + i + 17, total, huff[tc][th]),
                  "DHT code lengths do not form a prefix code");
        have_h[tc][th] = true;
        i += 17 + total;
      }
    } else if (m == 0xc0 || m == 0xc1 ||
               (m == 0xc2 && opt.allow_progressive)) {  // SOF0 / SOF1 / SOF2
      info.progressive = m == 0xc2;
      SCA_CHECK(!have_sof, "second frame header");
      SCA_CHECK(n >= 6, "truncated JPEG: SOF");
      SCA_CHECK(s[0] == 8, "only 8-bit JPEG is supported, got " +
                               std::to_string(s[0]) + "-bit precision");
      h = (i32)((u32)s[1] << 8 | s[2]);
      w = (i32)((u32)s[3] << 8 | s[4]);
      nc = s[5];
      SCA_CHECK(h >= 1 && w >= 1, "JPEG with zero rows or columns");
      SCA_CHECK(nc == 1 || nc == 3,
                std::to_string(nc) + "-component JPEG is not supported (CMYK "
                "and other layouts); 1 or 3 components are");
      SCA_CHECK(n == 6 + 3 * (u32)nc, "bad SOF length");
      for (i32 c = 0; c < nc; ++c) {
        comp_id[c] = s[6 + 3 * c];
        comp_hv[c] = s[7 + 3 * c];
        comp_tq[c] = s[8 + 3 * c];
        SCA_CHECK(comp_tq[c] <= 3, "bad quantisation table id in SOF");
      }
      if (nc == 3) {
        SCA_CHECK((comp_hv[0] == 0x11 || comp_hv[0] == 0x21 ||
                   comp_hv[0] == 0x22) &&
                      comp_hv[1] == 0x11 && comp_hv[2] == 0x11,
                  "unsupported sampling factors: luma must be 1x1, 2x1 or "
                  "2x2 and chroma 1x1");
      }
      have_sof = true;
    } else if (m >= 0xc2 && m <= 0xcf && m != 0xc8 && m != 0xcc) {
      SCA_CHECK(false, sof_name(m));
    } else if (m == 0xdd) {  // DRI
      SCA_CHECK(n == 2, "bad DRI length");
      info.restart_interval = (u32)s[0] << 8 | s[1];
    } else if (m == 0xda && info.progressive) {  // SOS of a progressive file
      SCA_CHECK(n >= 1, "truncated JPEG: SOS");
      u32 ns = s[0];
      u32 k = (u32)info.scans.size();
      SCA_CHECK(ns >= 1 && ns <= 4 && n == 4 + 2 * ns, "bad SOS length");
      SCA_CHECK(ns == 1 || ns == (u32)nc,
                "a progressive scan of " + std::to_string(ns) + " of " +
                    std::to_string(nc) + " components is not supported: a "
                    "scan holds one component or all of them");
      JpegScan sc{};
      sc.ncomp = ns;
      sc.ss = s[1 + 2 * ns];
      sc.se = s[2 + 2 * ns];
      sc.ah = s[3 + 2 * ns] >> 4;
      sc.al = s[3 + 2 * ns] & 15;
      const std::string bad = "invalid progressive scan script: scan " +
                              std::to_string(k) + ": ";
      SCA_CHECK(sc.ss <= sc.se && sc.se <= 63,
                bad + "spectral selection " + std::to_string(sc.ss) + ".." +
                    std::to_string(sc.se) + " is not a band of 0..63");
      SCA_CHECK(sc.ss != 0 || sc.se == 0,
                bad + "a scan that starts at the DC coefficient holds "
                      "nothing else, Se must be 0");
      SCA_CHECK(sc.ss == 0 || ns == 1,
                bad + "an AC scan holds one component");
      SCA_CHECK(sc.al <= kJpegProgMaxAl && sc.ah <= kJpegProgMaxAl,
                bad + "successive approximation position above 13");
      SCA_CHECK(sc.ah == 0 || sc.al + 1 == sc.ah,
                bad + "a refinement scan codes one bit, Al must be Ah - 1");
      for (u32 c = 0; c < ns; ++c) {
        u32 fc = c;
        if (ns == 1) {
          fc = 0;
          while (fc < (u32)nc && comp_id[fc] != s[1]) ++fc;
          SCA_CHECK(fc < (u32)nc,
                    "scan names a component the frame does not have");
        } else {
          SCA_CHECK(s[1 + 2 * c] == comp_id[c],
                    "scan components are not in frame order");
        }
        sc.comp[c] = fc;
        u32 td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
        SCA_CHECK(td <= 3 && ta <= 3, "bad Huffman table id in SOS");
        if (sc.ss == 0 && sc.ah == 0) {
          SCA_CHECK(have_h[0][td],
                    "scan uses a Huffman table that was not defined");
          sc.dc[fc] = huff[0][td];
        } else if (sc.ss != 0) {
          SCA_CHECK(have_h[1][ta],
                    "scan uses a Huffman table that was not defined");
          sc.ac[fc] = huff[1][ta];
        }
        SCA_CHECK(sc.ss == 0 || last_al[fc][0] >= 0,
                  bad + "an AC scan of a component comes before its first "
                        "DC scan");
        for (u32 z = sc.ss; z <= sc.se; ++z) {
          int& la = last_al[fc][z];
          if (sc.ah == 0)
            SCA_CHECK(la < 0, bad + "coefficient " + std::to_string(z) +
                                  " is coded a second time with Ah = 0");
          else
            SCA_CHECK(la >= 0 && (u32)la == sc.ah,
                      bad + "Ah = " + std::to_string(sc.ah) + " refines "
                      "coefficient " + std::to_string(z) + ", which " +
                          (la < 0 ? std::string("no scan has coded yet")
                                  : "was last coded with Al = " +
                                        std::to_string(la)));
          la = (int)sc.al;
        }
      }
      sc.restart_interval = info.restart_interval;
      JpegDecGeom g =
          jpeg_dec_geom(h, w, nc, comp_hv[0] >> 4, comp_hv[0] & 15);
      if (ns == 1) {
        u32 bw, bh;
        jpeg_prog_comp_blocks(g, sc.comp[0], bw, bh);
        sc.units = bw * bh;
        sc.blocks_per_unit = 1;
      } else {
        sc.units = g.nmcu;
        sc.blocks_per_unit = g.blocks_per_mcu;
      }
      if (!scan) scan = pos;
      if (!full) break;
      pos = walk_progressive_scan(data, size, pos, k, sc);
      info.scans.push_back(std::move(sc));
    } else if (m == 0xda) {  // SOS
      SCA_CHECK(have_sof, "scan before the frame header");
      SCA_CHECK(n >= 1, "truncated JPEG: SOS");
      u32 ns = s[0];
      SCA_CHECK(ns == (u32)nc,
                "multi-scan JPEG is not supported: the scan holds " +
                    std::to_string(ns) + " of " + std::to_string(nc) +
                    " components");
      SCA_CHECK(n == 4 + 2 * ns, "bad SOS length");
      for (u32 c = 0; c < ns; ++c) {
        SCA_CHECK(s[1 + 2 * c] == comp_id[c],
                  "scan components are not in frame order");
        u32 td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
        SCA_CHECK(td <= 3 && ta <= 3, "bad Huffman table id in SOS");
        SCA_CHECK(have_h[0][td] && have_h[1][ta],
                  "scan uses a Huffman table that was not defined");
        SCA_CHECK(have_q[comp_tq[c]],
                  "frame uses a quantisation table that was not defined");
        info.dc[c] = huff[0][td];
        info.ac[c] = huff[1][ta];
        std::copy(qt[comp_tq[c]], qt[comp_tq[c]] + 64, info.q[c]);
      }
      SCA_CHECK(s[1 + 2 * ns] == 0 && s[2 + 2 * ns] == 63 &&
                    s[3 + 2 * ns] == 0,
                "spectral selection / successive approximation (progressive "
                "scan parameters) are not supported");
      scan = pos;
    }
    // APPn, COM and anything else with a length: skipped
  }
  if (info.progressive) {
    // the quantisation tables as they stand when the frame ends (or, for
    // jpeg_parse_header, at the first scan: what is defined so far)
    for (i32 c = 0; c < nc; ++c) {
      SCA_CHECK(!full || have_q[comp_tq[c]],
                "frame uses a quantisation table that was not defined");
      if (have_q[comp_tq[c]])
        std::copy(qt[comp_tq[c]], qt[comp_tq[c]] + 64, info.q[c]);
    }
  }
  for (i32 c = nc; c < 3; ++c) {  // unused slots stay defined
    info.dc[c] = info.dc[0];
    info.ac[c] = info.ac[0];
    std::copy(info.q[0], info.q[0] + 64, info.q[c]);
  }
  info.g = jpeg_dec_geom(h, w, nc, comp_hv[0] >> 4, comp_hv[0] & 15);
  return scan;
}

}  // namespace

JpegInfo jpeg_parse(const u8* data, size_t size, JpegParseOptions opt) {
  JpegInfo info;
  size_t scan = parse_markers(data, size, info, opt, true);
  if (info.progressive) return info;
  const JpegDecGeom& g = info.g;

  // ---- segment index: split the entropy-coded data at RSTn ----
  u32 ri = info.restart_interval;
  u32 per_seg = ri ? ri : g.nmcu;
  u32 nseg = (g.nmcu + per_seg - 1) / per_seg;
  size_t i = scan, seg_begin = scan;
  bool ended = false;
  while (i < size) {
    if (data[i] != 0xff) {
      ++i;
      continue;
    }
    if (i + 1 >= size) break;  // a lone FF at the very end: truncated
    u32 m = data[i + 1];
    if (m == 0) {
      i += 2;
    } else if (m == 0xff) {
      ++i;  // fill byte
    } else if (m >= 0xd0 && m <= 0xd7) {
      SCA_CHECK(ri != 0, "restart marker in a JPEG without a DRI segment");
      u32 k = (u32)info.segments.size();
      SCA_CHECK(k + 1 < nseg, "more restart markers than restart intervals");
      SCA_CHECK(m - 0xd0 == (k & 7),
                "restart markers out of sequence: RST" +
                    std::to_string(m - 0xd0) + " where RST" +
                    std::to_string(k & 7) + " belongs");
      info.segments.push_back(
          {(u32)seg_begin, (u32)i, k * per_seg, per_seg});
      i += 2;
      seg_begin = i;
    } else {
      SCA_CHECK(m == 0xd9,
                m == 0xda || m == 0xc4 || m == 0xdb
                    ? "multi-scan JPEG is not supported: tables or a second "
                      "scan follow the first"
                    : "unexpected marker inside the scan");
      ended = true;
      break;
    }
  }
  SCA_CHECK(ended, "truncated JPEG: no EOI marker after the scan");
  u32 k = (u32)info.segments.size();
  SCA_CHECK(k + 1 == nseg,
            "JPEG has " + std::to_string(k + 1) + " restart segments, its "
            "size and restart interval need " + std::to_string(nseg));
  info.segments.push_back(
      {(u32)seg_begin, (u32)i, k * per_seg, g.nmcu - k * per_seg});
  // the shortest block is a 1-bit DC code and a 1-bit EOB: a header that
  // promises more blocks than the scan can hold is refused before anything
  // is allocated for it
  SCA_CHECK(((u64)i - scan) * 8 >= (u64)g.nmcu * g.blocks_per_mcu * 2,
            "truncated JPEG: the scan is too short for the image size");
  return info;
}

namespace {

// the scans of a progressive file in file order, each scan's segments in
// order, into the zeroed `coef`
void decode_progressive_scans(const u8* data, const JpegInfo& info,
                              i16* coef) {
  const JpegDecGeom& g = info.g;
  for (size_t k = 0; k < info.scans.size(); ++k) {
    const JpegScan& sc = info.scans[k];
    u32 bw = 1, bh = 1;
    if (sc.ncomp == 1) jpeg_prog_comp_blocks(g, sc.comp[0], bw, bh);
    for (size_t s = 0; s < sc.segments.size(); ++s) {
      const JpegSegment& seg = sc.segments[s];
      JpegBitReader br;
      jpeg_bits_init(br, data, seg.begin, seg.end);
      i32 pred[3] = {0, 0, 0};
      u32 eobrun = 0;
      for (u32 u = seg.first_mcu; u < seg.first_mcu + seg.mcu_count; ++u) {
        for (u32 b = 0; b < sc.blocks_per_unit; ++b) {
          u32 comp, idx;
          if (sc.ncomp == 1) {
            comp = sc.comp[0];
            idx = jpeg_prog_block_index(g, comp, u % bw, u / bw);
          } else {
            comp = jpeg_prog_block_comp(g, b);
            idx = u * g.blocks_per_mcu + b;
          }
          u32 st = jpeg_prog_block(
              br, sc.ss == 0 ? sc.dc[comp] : sc.ac[comp], info.zz2nat, sc.ss,
              sc.se, sc.ah, sc.al, pred[comp], eobrun,
              coef + (size_t)idx * 64);
          SCA_CHECK(st == kJpegBlockOk,
                    jpeg_entropy_error(st, (u32)s, (u32)k));
        }
      }
    }
  }
}

}  // namespace

void jpeg_coefficients_cpu(const u8* data, const JpegInfo& info,
                           std::vector<i16>& coef) {
  const JpegDecGeom& g = info.g;
  coef.assign((size_t)g.nmcu * g.blocks_per_mcu * 64, 0);
  if (info.progressive) {
    decode_progressive_scans(data, info, coef.data());
    return;
  }
  for (size_t s = 0; s < info.segments.size(); ++s) {
    const JpegSegment& seg = info.segments[s];
    JpegBitReader br;
    jpeg_bits_init(br, data, seg.begin, seg.end);
    i32 pred[3] = {0, 0, 0};
    for (u32 m = seg.first_mcu; m < seg.first_mcu + seg.mcu_count; ++m)
      for (u32 b = 0; b < g.blocks_per_mcu; ++b) {
        u32 comp = jpeg_prog_block_comp(g, b);
        u32 st = jpeg_decode_block(
            br, info.dc[comp], info.ac[comp], info.zz2nat, pred[comp],
            coef.data() + ((size_t)m * g.blocks_per_mcu + b) * 64);
        SCA_CHECK(st == kJpegBlockOk, jpeg_entropy_error(st, (u32)s));
      }
  }
}

void jpeg_decode_cpu_into(const u8* data, const JpegInfo& info, u8* out) {
  const JpegDecGeom& g = info.g;
  size_t ysz = (size_t)g.y_stride * g.y_rows;
  size_t csz = (size_t)g.c_stride * g.c_rows;
  std::vector<u8> planes(ysz + 2 * csz);
  u8* plane[3] = {planes.data(), planes.data() + ysz,
                  planes.data() + ysz + csz};
  u32 stride[3] = {g.y_stride, g.c_stride, g.c_stride};

  if (info.progressive) {
    std::vector<i16> coef;
    jpeg_coefficients_cpu(data, info, coef);
    for (u32 m = 0; m < g.nmcu; ++m) {
      for (u32 b = 0; b < g.blocks_per_mcu; ++b) {
        u32 comp, px, py;
        jpeg_block_pos(g, m, b, comp, px, py);
        const i16* blk = coef.data() + ((size_t)m * g.blocks_per_mcu + b) * 64;
        i32 deq[64];
        for (int k = 0; k < 64; ++k)
          deq[k] = jpeg_dequant(blk[k], info.q[comp][k]);
        u8 pix[64];
        jpeg_idct_block(deq, pix);
        u8* dst = plane[comp] + (size_t)py * stride[comp] + px;
        for (int y = 0; y < 8; ++y)
          std::copy(pix + y * 8, pix + y * 8 + 8, dst + (size_t)y * stride[comp]);
      }
    }
  }
  for (size_t s = 0; s < info.segments.size(); ++s) {
    const JpegSegment& seg = info.segments[s];
    JpegBitReader br;
    jpeg_bits_init(br, data, seg.begin, seg.end);
    i32 pred[3] = {0, 0, 0};
    for (u32 m = seg.first_mcu; m < seg.first_mcu + seg.mcu_count; ++m) {
      for (u32 b = 0; b < g.blocks_per_mcu; ++b) {
        u32 comp, px, py;
        jpeg_block_pos(g, m, b, comp, px, py);
        i16 coef[64] = {0};
        u32 st = jpeg_decode_block(br, info.dc[comp], info.ac[comp],
                                   info.zz2nat, pred[comp], coef);
        SCA_CHECK(st == kJpegBlockOk, jpeg_entropy_error(st, (u32)s));
        i32 deq[64];
        for (int k = 0; k < 64; ++k)
          deq[k] = jpeg_dequant(coef[k], info.q[comp][k]);
        u8 pix[64];
        jpeg_idct_block(deq, pix);
        u8* dst = plane[comp] + (size_t)py * stride[comp] + px;
        for (int y = 0; y < 8; ++y)
          std::copy(pix + y * 8, pix + y * 8 + 8, dst + (size_t)y * stride[comp]);
      }
    }
  }
  if (g.nc == 1) {
    for (i32 y = 0; y < g.h; ++y)
      std::copy(plane[0] + (size_t)y * g.y_stride,
                plane[0] + (size_t)y * g.y_stride + g.w,
                out + (size_t)y * g.w);
    return;
  }
  for (i32 y = 0; y < g.h; ++y)
    for (i32 x = 0; x < g.w; ++x)
      jpeg_pixel_rgb(g, plane[0], plane[1], plane[2], (u32)x, (u32)y,
                     out + ((size_t)y * g.w + x) * 3);
}

DecodedImage jpeg_decode_cpu(const u8* data, size_t size,
                             JpegParseOptions opt) {
  JpegInfo info = jpeg_parse(data, size, opt);
  DecodedImage img;
  img.h = info.g.h;
  img.w = info.g.w;
  img.c = info.g.nc;
  img.pixels.resize((size_t)img.h * img.w * img.c);
  jpeg_decode_cpu_into(data, info, img.pixels.data());
  return img;
}

DecodedImage image_decode_cpu(const u8* data, size_t size,
                              JpegParseOptions opt) {
  if (is_jpeg(data, size)) return jpeg_decode_cpu(data, size, opt);
  if (is_png(data, size)) return png_decode(data, size);
  SCA_CHECK(false, "unknown image format: neither a JPEG (FF D8) nor a PNG "
                   "signature");
  return {};
}

}  // namespace sca
