// AddressSanitizer/UBSan-verified mutation fuzz of the self-synchronising
// JPEG decoder's CPU model (csrc/ops/jpeg_sync_cpu.cpp, HIP-free, plain g++)
// and, through it, of csrc/ops/jpeg_sync_common.h: the chunk walks that
// kernels/jpeg_sync_decode.hip compiles for the GPU are these same
// functions. Every iteration feeds a mutated file without restart markers
// from an exact-size heap buffer to the serial decoder and to the model at
// 4- and 64-byte chunks. The model must return the serial decoder's pixels,
// or report a fallback (and then raise exactly when the serial decoder
// does); any out-of-bounds access is an ASan report, any overflow a UBSan
// report. tests/test_jpeg_sync_fuzz.py builds and runs this.
//
// Usage: asan_jpeg_sync <iters> <seed file>... [--exact <file>...]
// Files after --exact are run as they are.
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

struct Tally {
  int equal = 0, fallback = 0, raised = 0, unparsed = 0;
};

[[noreturn]] void fail(const char* what, unsigned cb) {
  std::fprintf(stderr, "MISMATCH at chunk_bytes %u: %s\n", cb, what);
  std::exit(1);
}

// one file through the serial decoder and the model
void check(const std::vector<u8>& data, Tally& t, bool must_verify) {
  // exact-size heap copy: the redzone starts at the first byte past the end
  u8* exact = (u8*)std::malloc(data.size() ? data.size() : 1);
  std::memcpy(exact, data.data(), data.size());
  sca::JpegInfo info;
  bool parsed = true;
  try {
    info = sca::jpeg_parse(exact, data.size());
  } catch (const std::exception&) {
    parsed = false;
  }
  if (!parsed || info.restart_interval != 0) {
    ++t.unparsed;
    std::free(exact);
    return;
  }
  size_t npix = (size_t)info.g.h * info.g.w * info.g.nc;
  std::vector<u8> want(npix), got(npix);
  bool serial_ok = true;
  try {
    sca::jpeg_decode_cpu_into(exact, info, want.data());
  } catch (const std::exception&) {
    serial_ok = false;
  }
  for (unsigned cb : {4u, 64u}) {
    sca::JpegSyncStats st;
    bool ok = true;
    std::fill(got.begin(), got.end(), 0);
    try {
      sca::jpeg_decode_sync_model(exact, info, cb, got.data(), &st);
    } catch (const std::exception&) {
      ok = false;
    }
    if (!ok) {
      if (st.verified) fail("the model raised on a verified file", cb);
      if (serial_ok) fail("the model raised, the serial decoder did not", cb);
      ++t.raised;
      continue;
    }
    if (!serial_ok) fail("the serial decoder raised, the model did not", cb);
    if (got != want) fail("pixels differ", cb);
    if (must_verify && !st.verified) fail("a seed file fell back", cb);
    if (st.verified) ++t.equal; else ++t.fallback;
  }
  std::free(exact);
}

// first byte after the SOS header, 0 if there is none
size_t scan_start(const std::vector<u8>& d) {
  for (size_t i = 2; i + 3 < d.size();) {
    if (d[i] != 0xff) return 0;
    size_t len = (size_t)d[i + 2] << 8 | d[i + 3];
    if (d[i + 1] == 0xda) return i + 2 + len < d.size() ? i + 2 + len : 0;
    i += 2 + len;
  }
  return 0;
}

void fuzz(const char* name, const std::vector<u8>& base, int iters) {
  Tally t;
  size_t scan = scan_start(base);
  for (int i = 0; i < iters; ++i) {
    std::vector<u8> data = base;
    size_t lo = scan && scan + 2 < data.size() ? scan : data.size() / 2;
    size_t hi = data.size() - 2;  // the EOI marker stays
    switch (xorshift() % 4) {
      case 0: {  // bit flips in the entropy-coded data
        int n = 1 + (int)(xorshift() % 4);
        for (int k = 0; k < n; ++k)
          data[lo + xorshift() % (hi - lo)] ^= (u8)(1u << (xorshift() % 8));
        break;
      }
      case 1: {  // bytes overwritten, FF and 00 among them
        int n = 1 + (int)(xorshift() % 4);
        for (int k = 0; k < n; ++k) {
          uint64_t r = xorshift();
          data[lo + r % (hi - lo)] =
              (r >> 32) % 3 == 0 ? 0xff : (r >> 32) % 3 == 1 ? 0 : (u8)(r >> 40);
        }
        break;
      }
      case 2: {  // a piece cut out
        size_t a = lo + xorshift() % (hi - lo);
        size_t b = a + xorshift() % (hi - a);
        data.erase(data.begin() + (long)a, data.begin() + (long)b);
        break;
      }
      default: {  // Huffman and quantisation tables, sizes: header bytes
        int n = 1 + (int)(xorshift() % 3);
        for (int k = 0; k < n; ++k)
          data[xorshift() % lo] ^= (u8)(1u << (xorshift() % 8));
        break;
      }
    }
    check(data, t, false);
  }
  std::printf("%s: %d iters, %d equal, %d fallback, %d raised, %d unparsed\n",
              name, iters, t.equal, t.fallback, t.raised, t.unparsed);
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
  Tally te;
  int n_exact = 0;
  for (int i = 2; i < argc; ++i) {
    if (std::string(argv[i]) == "--exact") {
      exact = true;
      continue;
    }
    std::vector<u8> base = read_file(argv[i]);
    if (exact) {
      ++n_exact;
      check(base, te, false);
      continue;
    }
    Tally t;
    check(base, t, true);
    if (t.equal != 2) {
      std::fprintf(stderr, "seed %s is not a JPEG without restart markers\n",
                   argv[i]);
      return 1;
    }
    fuzz(argv[i], base, iters);
  }
  std::printf("exact: %d files, %d equal, %d fallback, %d raised\n", n_exact,
              te.equal, te.fallback, te.raised);
  std::printf("asan jpeg sync fuzz: OK\n");
  return 0;
}
