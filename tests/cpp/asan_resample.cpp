// AddressSanitizer/UBSan run of csrc/ops/resample_common.h: the tap-table
// builder, the two-pass CPU resampler, the nearest gather and the fit rule
// are index arithmetic on caller-chosen sizes. Every size from 1 to 70 is
// resampled to every other, along each axis in turn and both at once on a
// coarser grid, with every filter and 1, 3 and 4 channels, from exact-size
// heap buffers: an access outside a frame, the tables or the intermediate is
// an ASan report, an accumulator overflow a UBSan report. The program also
// checks what the tables promise: taps inside the source, rows that sum to
// 2^22, a constant frame that stays constant.
// tests/test_resize_filters_cpu.py builds and runs this with plain g++.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../scanner_amd/csrc/ops/resample_common.h"

using namespace sca;

namespace {

const ResampleFilter kFilters[] = {ResampleFilter::kBox,
                                   ResampleFilter::kTriangle,
                                   ResampleFilter::kCubic,
                                   ResampleFilter::kLanczos3};

void fail(const char* what, int a, int b) {
  std::printf("FAILED: %s (%d -> %d)\n", what, a, b);
  std::exit(1);
}

void check_axis(const ResampleAxis& ax) {
  for (i32 d = 0; d < ax.n_dst; ++d) {
    if (ax.first[d] < 0 || ax.count[d] < 1 ||
        ax.first[d] + ax.count[d] > ax.n_src || ax.count[d] > ax.max_taps)
      fail("tap range", ax.n_src, ax.n_dst);
    if (d && (ax.first[d] < ax.first[d - 1] ||
              ax.first[d] + ax.count[d] < ax.first[d - 1] + ax.count[d - 1]))
      fail("tap ranges not monotone", ax.n_src, ax.n_dst);
    i64 sum = 0;
    for (i32 j = 0; j < ax.count[d]; ++j)
      sum += ax.weights[(size_t)d * ax.max_taps + j];
    if (sum != kWeightOne) fail("row sum", ax.n_src, ax.n_dst);
  }
  if (ax.packed().size() != (size_t)ax.n_dst * (2 + ax.max_taps))
    fail("packed size", ax.n_src, ax.n_dst);
}

u32 rng = 12345;
u8 next_byte() {
  rng = rng * 1664525u + 1013904223u;
  return (u8)(rng >> 24);
}

void resample_once(ResampleFilter f, i32 sh, i32 sw, i32 dh, i32 dw, i32 c,
                   int fill) {
  // exact-size heap buffers
  std::vector<u8> src((size_t)sh * sw * c), dst((size_t)dh * dw * c);
  for (u8& b : src)
    b = fill == 0 ? next_byte() : fill == 1 ? (next_byte() & 1 ? 255 : 0) : 77;
  ResampleAxis ax = resample_build_axis(f, sw, dw);
  ResampleAxis ay = resample_build_axis(f, sh, dh);
  check_axis(ax);
  check_axis(ay);
  std::vector<i16> tmp;
  resample_cpu(src.data(), sh, sw, c, ax, ay, dst.data(), tmp);
  if (fill == 2)
    for (u8 b : dst)
      if (b != 77) fail("constant frame changed", sh * 1000 + sw, dh * 1000 + dw);
  if (fill == 0 && sh == dh && sw == dw && src != dst)
    fail("same-size resize changed the frame", sh, sw);
  std::vector<u8> near((size_t)dh * dw * c);
  resample_nearest_cpu(src.data(), sh, sw, c, near.data(), dh, dw);
}

}  // namespace

int main() {
  long runs = 0;
  for (ResampleFilter f : kFilters) {
    for (i32 a = 1; a <= 70; ++a) {
      for (i32 b = 1; b <= 70; ++b) {
        check_axis(resample_build_axis(f, a, b));
        // along x, then along y, 3 channels, noise that overshoots
        resample_once(f, 2, a, 2, b, 3, 1);
        resample_once(f, a, 2, b, 2, 3, 1);
        runs += 2;
      }
    }
    // both axes at once on a coarser grid, every channel count and content
    for (i32 a = 1; a <= 70; a += 7)
      for (i32 b = 1; b <= 70; b += 9)
        for (i32 c : {1, 3, 4})
          for (int fill = 0; fill < 3; ++fill) {
            resample_once(f, a, 71 - a, b, 71 - b, c, fill);
            resample_once(f, a, a, a, a, c, fill);
            runs += 2;
          }
    // the widest downscales the formats must hold
    check_axis(resample_build_axis(f, 3840, 224));
    check_axis(resample_build_axis(f, 5000, 1));
    check_axis(resample_build_axis(f, 1, 5000));
  }
  for (i32 sh = 1; sh <= 70; ++sh)
    for (i32 sw = 1; sw <= 70; ++sw)
      for (i32 H : {1, 7, 32, 70})
        for (i32 W : {1, 32, 70}) {
          i32 dh = 0, dw = 0;
          resample_fit(sh, sw, H, W, &dh, &dw);
          if (dh < 1 || dw < 1 || dh > H || dw > W || (dh != H && dw != W))
            fail("fit outside its box", sh * 1000 + sw, dh * 1000 + dw);
        }
  bool threw = false;
  try {
    resample_parse_filter("gaussian");
  } catch (const ScannerError&) {
    threw = true;
  }
  if (!threw) fail("unknown filter accepted", 0, 0);
  std::printf("asan resample: OK (%ld frames)\n", runs);
  return 0;
}
