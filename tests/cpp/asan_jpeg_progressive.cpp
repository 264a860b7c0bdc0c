// AddressSanitizer/UBSan-verified mutation fuzz of the progressive JPEG
// path of the CPU decoder (csrc/ops/jpeg_decode_cpu.cpp — HIP-free, plain
// g++): the multi-scan parser and, through the decoder, the four block
// decoders and the block index mapping of
// csrc/ops/jpeg_progressive_common.h, which
// kernels/jpeg_progressive_decode.hip compiles for the GPU as they are.
// Every iteration feeds a mutated valid file from an exact-size heap buffer
// with progressive files allowed; the decoder must return or throw — any
// out-of-bounds access is an ASan report, any overflow a UBSan report.
// tests/test_jpeg_progressive_fuzz.py builds and runs this.
//
// Usage: asan_jpeg_progressive <iters> <seed file>... [--exact <file>...]
// Files after --exact are decoded as they are (the corrupt inputs the GPU
// tests later give to the HIP decoder).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../scanner_amd/csrc/ops/image_decode.h"

using sca::u8;

namespace {

uint64_t rng_state = 0x9e3779b9ull;
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

// first byte after the first SOS header of a JPEG (the scans and the
// markers between them follow), 0 if there is none
size_t scan_start(const std::vector<u8>& d) {
  for (size_t i = 2; i + 3 < d.size();) {
    if (d[i] != 0xff) return 0;
    size_t len = (size_t)d[i + 2] << 8 | d[i + 3];
    if (d[i + 1] == 0xda) return i + 2 + len < d.size() ? i + 2 + len : 0;
    i += 2 + len;
  }
  return 0;
}

bool decode(const std::vector<u8>& data) {
  // exact-size heap copy: the redzone starts at the first byte past the end
  u8* exact = (u8*)std::malloc(data.size() ? data.size() : 1);
  std::memcpy(exact, data.data(), data.size());
  bool ok = true;
  try {
    sca::JpegParseOptions opt;
    opt.allow_progressive = true;
    sca::DecodedImage img = sca::jpeg_decode_cpu(exact, data.size(), opt);
    if (img.pixels.size() != (size_t)img.h * img.w * img.c) std::abort();
  } catch (const std::exception&) {
    ok = false;
  }
  std::free(exact);
  return ok;
}

void fuzz(const char* name, const std::vector<u8>& base, int iters) {
  int ok = 0, raised = 0;
  size_t scan = scan_start(base);
  for (int i = 0; i < iters; ++i) {
    std::vector<u8> data = base;
    switch (xorshift() % 5) {
      case 0:  // truncation
        data.resize(xorshift() % (data.size() + 1));
        break;
      case 1: {  // bit flips anywhere
        int n = 1 + (int)(xorshift() % 8);
        for (int k = 0; k < n; ++k)
          data[xorshift() % data.size()] ^= (u8)(1u << (xorshift() % 8));
        break;
      }
      case 2: {  // byte edits in the first 700 bytes: headers, lengths, tables
        int n = 1 + (int)(xorshift() % 4);
        size_t span = data.size() < 700 ? data.size() : 700;
        for (int k = 0; k < n; ++k)
          data[xorshift() % span] = (u8)(xorshift() & 0xff);
        break;
      }
      case 3: {  // bit flips confined to the scans
        size_t lo = scan && scan < data.size() ? scan : data.size() / 2;
        int n = 1 + (int)(xorshift() % 4);
        for (int k = 0; k < n; ++k)
          data[lo + xorshift() % (data.size() - lo)] ^=
              (u8)(1u << (xorshift() % 8));
        break;
      }
      default: {  // a piece of the scans cut out, EOI kept
        size_t lo = scan && scan < data.size() ? scan : data.size() / 2;
        size_t a = lo + xorshift() % (data.size() - lo);
        size_t b = a + xorshift() % (data.size() - a);
        data.erase(data.begin() + (long)a, data.begin() + (long)b);
        break;
      }
    }
    if (decode(data)) ++ok; else ++raised;
  }
  std::printf("%s: %d iters, %d decoded, %d raised\n", name, iters, ok,
              raised);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <iters> <seed>... [--exact <file>...]\n",
                 argv[0]);
    return 2;
  }
  int iters = std::atoi(argv[1]);
  bool exact = false;
  int n_exact_ok = 0, n_exact = 0;
  for (int i = 2; i < argc; ++i) {
    if (std::string(argv[i]) == "--exact") {
      exact = true;
      continue;
    }
    std::vector<u8> base = read_file(argv[i]);
    if (exact) {
      ++n_exact;
      if (decode(base)) ++n_exact_ok;
      continue;
    }
    if (!decode(base)) {
      std::fprintf(stderr, "seed %s does not decode\n", argv[i]);
      return 1;
    }
    fuzz(argv[i], base, iters);
  }
  std::printf("exact: %d files, %d decoded\n", n_exact, n_exact_ok);
  std::printf("asan jpeg progressive fuzz: OK\n");
  return 0;
}
