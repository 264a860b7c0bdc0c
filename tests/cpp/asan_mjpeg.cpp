// AddressSanitizer/UBSan-verified mutation fuzz of the Motion-JPEG host
// code: mjpeg_index_ref (csrc/video/mjpeg_common.h, the classification and
// acceptance rule that kernels/mjpeg_index.hip compiles for the GPU) and
// mp4_parse on Motion-JPEG files (csrc/video/mp4.cpp). HIP-free, plain g++.
// Every iteration works on an exact-size heap copy, so a read past the end
// is an ASan report.
//
// The index is also held against jpeg_parse: a mutated sample whose header
// still equals the reference is accepted by the index exactly when
// jpeg_parse accepts it, and then with the same segments.
// tests/test_mjpeg_fuzz.py builds and runs this.
//
// Usage: asan_mjpeg <iters> <jpeg with DRI>... --mp4 <mp4 file>...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../scanner_amd/csrc/ops/image_decode.h"
#include "../../scanner_amd/csrc/video/mjpeg_common.h"
#include "../../scanner_amd/csrc/video/mp4.h"

using sca::u8;

namespace {

uint64_t rng_state = 0x2545f4914f6cdd1dull;
uint64_t xorshift() {
  uint64_t x = rng_state;
  x ^= x << 13;
  x ^= x >> 7;
  x ^= x << 17;
  return rng_state = x;
}

std::vector<u8> read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  return std::vector<u8>(std::istreambuf_iterator<char>(f),
                         std::istreambuf_iterator<char>());
}

void die(const char* name, int iter, const char* what) {
  std::fprintf(stderr, "%s: iteration %d: %s\n", name, iter, what);
  std::abort();
}

// mutations of bytes [lo, size): what an index has to survive
void mutate(std::vector<u8>& d, size_t lo) {
  static const u8 kInteresting[] = {0xff, 0x00, 0xd0, 0xd1, 0xd7, 0xd8,
                                    0xd9, 0xda, 0xc4, 0x01};
  size_t span = d.size() - lo;
  switch (xorshift() % 6) {
    case 0:  // truncation
      d.resize(xorshift() % (d.size() + 1));
      break;
    case 1: {  // bit flips
      int n = 1 + (int)(xorshift() % 6);
      for (int k = 0; k < n && span; ++k)
        d[lo + xorshift() % span] ^= (u8)(1u << (xorshift() % 8));
      break;
    }
    case 2: {  // marker-like bytes
      int n = 1 + (int)(xorshift() % 4);
      for (int k = 0; k < n && span; ++k)
        d[lo + xorshift() % span] = kInteresting[xorshift() % 10];
      break;
    }
    case 3: {  // an FF xx pair
      if (span < 2) break;
      size_t p = lo + xorshift() % (span - 1);
      d[p] = 0xff;
      d[p + 1] = kInteresting[xorshift() % 10];
      break;
    }
    case 4: {  // cut a piece out
      if (!span) break;
      size_t a = lo + xorshift() % span;
      size_t n = 1 + xorshift() % 16;
      d.erase(d.begin() + a, d.begin() + std::min(d.size(), a + n));
      break;
    }
    default: {  // insert a piece
      size_t a = lo + (span ? xorshift() % span : 0);
      size_t n = 1 + xorshift() % 4;
      for (size_t k = 0; k < n; ++k)
        d.insert(d.begin() + a, kInteresting[xorshift() % 10]);
      break;
    }
  }
}

void fuzz_index(const char* name, const std::vector<u8>& base, int iters) {
  sca::JpegInfo hdr;
  size_t scan = sca::jpeg_parse_header(base.data(), base.size(), hdr);
  if (hdr.restart_interval == 0) die(name, -1, "seed has no DRI segment");
  sca::MjpegIndexParams p;
  p.header_len = (uint32_t)scan;
  p.mcus_per_seg = hdr.restart_interval;
  p.nmcu = hdr.g.nmcu;
  p.nseg = (p.nmcu + p.mcus_per_seg - 1) / p.mcus_per_seg;
  p.min_scan_bytes =
      (uint32_t)(((uint64_t)p.nmcu * hdr.g.blocks_per_mcu * 2 + 7) / 8);
  int accepted = 0, refused = 0, other_header = 0;
  for (int i = 0; i < iters; ++i) {
    std::vector<u8> data = base;
    // one mutation in eight may hit the header too
    mutate(data, xorshift() % 8 == 0 ? 2 : scan);
    u8* exact = (u8*)std::malloc(data.size() ? data.size() : 1);
    std::memcpy(exact, data.data(), data.size());
    auto* segs = (sca::MjpegSeg*)std::malloc(sizeof(sca::MjpegSeg) * p.nseg);
    uint32_t st = sca::mjpeg_index_ref(exact, data.size(), base.data(), p, 0,
                                       segs);
    bool parsed = true;
    sca::JpegInfo info;
    try {
      info = sca::jpeg_parse(exact, data.size());
    } catch (const std::exception&) {
      parsed = false;
    }
    if (st == sca::kMjpegHeaderDiffers) {
      ++other_header;
    } else if (st == sca::kMjpegOk) {
      ++accepted;
      if (!parsed) die(name, i, "index accepts what jpeg_parse refuses");
      if (info.segments.size() != p.nseg) die(name, i, "segment count");
      for (uint32_t k = 0; k < p.nseg; ++k) {
        const sca::JpegSegment& a = info.segments[k];
        if (a.begin != segs[k].begin || a.end != segs[k].end ||
            a.first_mcu != segs[k].first_mcu ||
            a.mcu_count != segs[k].mcu_count)
          die(name, i, "segments differ from jpeg_parse");
      }
    } else {
      ++refused;
      if (parsed) die(name, i, "index refuses what jpeg_parse accepts");
    }
    std::free(segs);
    std::free(exact);
  }
  std::printf("%s: %d iters, %d accepted, %d refused, %d other header\n",
              name, iters, accepted, refused, other_header);
}

void fuzz_mp4(const char* name, const std::vector<u8>& base, int iters) {
  int parsed = 0;
  for (int i = 0; i < iters; ++i) {
    std::vector<u8> data = base;
    if (i) mutate(data, 0);
    u8* exact = (u8*)std::malloc(data.size() ? data.size() : 1);
    std::memcpy(exact, data.data(), data.size());
    try {
      sca::Mp4Track t = sca::mp4_parse(exact, data.size());
      ++parsed;
      if (t.sample_offsets.size() != t.sample_sizes.size())
        die(name, i, "offsets and sizes differ in number");
      for (size_t s = 0; s < t.sample_sizes.size(); ++s)
        if (t.sample_offsets[s] > data.size() ||
            t.sample_sizes[s] > data.size() - t.sample_offsets[s])
          die(name, i, "a sample lies outside the file");
      if (i == 0 && t.codec != "mjpeg") die(name, i, "seed is not mjpeg");
    } catch (const std::exception&) {
      if (i == 0) die(name, i, "the seed itself does not parse");
    }
    std::free(exact);
  }
  std::printf("%s: %d iters, %d parsed\n", name, iters, parsed);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <iters> <jpeg>... --mp4 <mp4>...\n",
                 argv[0]);
    return 2;
  }
  int iters = std::atoi(argv[1]);
  bool mp4 = false;
  for (int a = 2; a < argc; ++a) {
    if (std::string(argv[a]) == "--mp4") {
      mp4 = true;
      continue;
    }
    std::vector<u8> base = read_file(argv[a]);
    if (mp4) fuzz_mp4(argv[a], base, iters);
    else fuzz_index(argv[a], base, iters);
  }
  std::printf("asan mjpeg fuzz: OK\n");
  return 0;
}
