// Filtered resampling for Resize: filter names, the aspect-preserving fit,
// the per-axis tap tables and the CPU two-pass resampler. HIP-free; the CPU
// kernel (stdlib_cpu.cpp), the HIP kernels (kernels/resample.hip) and the
// sanitiser program (tests/cpp/asan_resample.cpp) all compile this file, and
// it is the specification of the fixed-point formats both devices share.
//
// Definition (per axis, separable; Pillow's Image.resize with BOX, BILINEAR,
// BICUBIC, LANCZOS, without Pillow's u8 intermediate). For n_src -> n_dst:
//   scale = n_src / n_dst, fscale = max(1, scale), support = r * fscale
//   r = 0.5 box, 1 triangle, 2 cubic, 3 lanczos3
//   output d: center = (d + 0.5) * scale
//     taps k in [max(0, trunc(center - support + 0.5)),
//                min(n_src, trunc(center + support + 0.5)))
//     weight f((k + 0.5 - center) / fscale), normalised to sum to one
// "nearest" takes source index ((2d+1) * n_src) / (2 * n_dst), no arithmetic
// on pixels.
//
// Formats. Weights are computed in double and quantised to kWeightBits = 22
// fractional bits (i32); the largest weight of a row then absorbs the
// rounding residue, so each row sums to exactly 2^22: a constant frame stays
// constant and a same-size resize returns its input.
//   horizontal pass  acc32 = sum w * u8            Q22
//                    inter = (acc32 + 2^15) >> 16  i16, kInterBits = 6
//   vertical pass    acc64 = sum w * inter         Q28
//                    out   = clamp((acc64 + 2^27) >> 28, 0, 255)
// Ranges. build_axis() refuses a row whose sum |w| reaches 2 (kMaxAbsSum);
// lanczos3, the widest, stays near 1.3. So |acc32| <= 255 * 2 * 2^22 =
// 2 139 095 040 < 2^31, |inter| <= 510 * 64 + 1 = 32 641 < 2^15 (no clip to
// [0, 255]: lanczos3 reaches about -43 .. 319 on noise), and |acc64| <
// 2^23 * 2^15 = 2^38 per row of weights. Right shifts of negative values are
// arithmetic on both devices (round half up).
#pragma once

#include <cmath>
#include <string>
#include <vector>

#include "../common.h"

namespace sca {

enum class ResampleFilter : i32 {
  kBilinear = 0,  // the two-tap sampler Resize always had; no table
  kNearest,
  kBox,
  kTriangle,
  kCubic,
  kLanczos3,
};

constexpr int kWeightBits = 22;
constexpr int kInterBits = 6;
constexpr i32 kWeightOne = 1 << kWeightBits;
constexpr i64 kMaxAbsSum = 2 * (i64)kWeightOne;

inline ResampleFilter resample_parse_filter(const std::string& name) {
  if (name == "bilinear") return ResampleFilter::kBilinear;
  if (name == "nearest") return ResampleFilter::kNearest;
  if (name == "box") return ResampleFilter::kBox;
  if (name == "triangle") return ResampleFilter::kTriangle;
  if (name == "cubic") return ResampleFilter::kCubic;
  if (name == "lanczos3") return ResampleFilter::kLanczos3;
  throw ScannerError(
      "Resize filter must be one of 'bilinear', 'nearest', 'box', "
      "'triangle', 'cubic', 'lanczos3', got '" + name + "'");
}

inline bool resample_is_convolution(ResampleFilter f) {
  return f != ResampleFilter::kBilinear && f != ResampleFilter::kNearest;
}

// Largest dh x dw of the aspect of sh x sw that fits the box H x W, exact
// integers (the rounded side is round-half-up, at least 1, at most the box).
inline void resample_fit(i32 sh, i32 sw, i32 H, i32 W, i32* dh, i32* dw) {
  i64 h = sh, w = sw;
  if ((i64)W * h <= (i64)H * w) {
    *dw = W;
    *dh = (i32)std::min<i64>(H, std::max<i64>(1, (2 * h * W + w) / (2 * w)));
  } else {
    *dh = H;
    *dw = (i32)std::min<i64>(W, std::max<i64>(1, (2 * w * H + h) / (2 * h)));
  }
}

inline i32 resample_nearest_index(i32 d, i32 n_src, i32 n_dst) {
  return (i32)(((2 * (i64)d + 1) * n_src) / (2 * (i64)n_dst));
}

inline f64 resample_filter_radius(ResampleFilter f) {
  switch (f) {
    case ResampleFilter::kBox: return 0.5;
    case ResampleFilter::kTriangle: return 1.0;
    case ResampleFilter::kCubic: return 2.0;
    case ResampleFilter::kLanczos3: return 3.0;
    default: throw ScannerError("resample: filter has no kernel function");
  }
}

inline f64 resample_filter_value(ResampleFilter f, f64 x) {
  const f64 kPi = 3.14159265358979323846;
  switch (f) {
    case ResampleFilter::kBox:
      return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case ResampleFilter::kTriangle: {
      f64 a = std::fabs(x);
      return a < 1.0 ? 1.0 - a : 0.0;
    }
    case ResampleFilter::kCubic: {  // Keys, a = -0.5
      const f64 a = -0.5;
      f64 t = std::fabs(x);
      if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
      if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
      return 0.0;
    }
    case ResampleFilter::kLanczos3: {
      if (x <= -3.0 || x >= 3.0) return 0.0;
      if (x == 0.0) return 1.0;
      f64 px = kPi * x;
      return std::sin(px) / px * (std::sin(px / 3.0) / (px / 3.0));
    }
    default: throw ScannerError("resample: filter has no kernel function");
  }
}

// Taps of one axis. Output d reads source indices first[d] .. first[d] +
// count[d] - 1 with weights weights[d * max_taps + j] (Q22, the unused tail
// of a row is zero). first and first + count never decrease with d.
struct ResampleAxis {
  i32 n_src = 0, n_dst = 0, max_taps = 0;
  std::vector<i32> first, count, weights;

  // The same table as one array, the form the HIP kernels read:
  // [first: n_dst][count: n_dst][weights: n_dst * max_taps]
  std::vector<i32> packed() const {
    std::vector<i32> p;
    p.reserve(2 * (size_t)n_dst + weights.size());
    p.insert(p.end(), first.begin(), first.end());
    p.insert(p.end(), count.begin(), count.end());
    p.insert(p.end(), weights.begin(), weights.end());
    return p;
  }
};

inline ResampleAxis resample_build_axis(ResampleFilter f, i32 n_src,
                                        i32 n_dst) {
  SCA_CHECK(n_src > 0 && n_dst > 0, "resample: sizes must be positive");
  const f64 radius = resample_filter_radius(f);
  const f64 scale = (f64)n_src / (f64)n_dst;
  const f64 fscale = scale < 1.0 ? 1.0 : scale;
  const f64 support = radius * fscale;
  ResampleAxis ax;
  ax.n_src = n_src;
  ax.n_dst = n_dst;
  ax.first.resize(n_dst);
  ax.count.resize(n_dst);
  for (i32 d = 0; d < n_dst; ++d) {
    f64 center = (d + 0.5) * scale;
    i64 lo = (i64)(center - support + 0.5);
    i64 hi = (i64)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > n_src) hi = n_src;
    if (lo > n_src - 1) lo = n_src - 1;
    if (hi <= lo) hi = lo + 1;  // never an empty row
    ax.first[d] = (i32)lo;
    ax.count[d] = (i32)(hi - lo);
    ax.max_taps = std::max(ax.max_taps, ax.count[d]);
  }
  ax.weights.assign((size_t)n_dst * ax.max_taps, 0);
  std::vector<f64> w(ax.max_taps);
  for (i32 d = 0; d < n_dst; ++d) {
    f64 center = (d + 0.5) * scale;
    i32 n = ax.count[d];
    f64 sum = 0.0;
    for (i32 j = 0; j < n; ++j) {
      w[j] = resample_filter_value(f, (ax.first[d] + j + 0.5 - center) / fscale);
      sum += w[j];
    }
    // a row whose taps all fall where f is zero (possible only at a clamped
    // edge) degenerates to its nearest tap
    if (!(sum > 1e-9)) {
      for (i32 j = 0; j < n; ++j) w[j] = 0.0;
      w[n / 2] = 1.0;
      sum = 1.0;
    }
    i32* q = &ax.weights[(size_t)d * ax.max_taps];
    i64 qsum = 0, abs_sum = 0;
    i32 big = 0;
    for (i32 j = 0; j < n; ++j) {
      q[j] = (i32)std::llround(w[j] / sum * (f64)kWeightOne);
      qsum += q[j];
      if (q[j] > q[big]) big = j;
    }
    q[big] += (i32)((i64)kWeightOne - qsum);
    for (i32 j = 0; j < n; ++j) abs_sum += q[j] < 0 ? -(i64)q[j] : (i64)q[j];
    SCA_CHECK(abs_sum < kMaxAbsSum,
              "resample: sum of |weights| of a row reaches 2, the "
              "accumulator formats do not hold it");
  }
  return ax;
}

// Two-pass resampler over tables, the CPU kernel. src and dst are packed HWC
// u8; tmp is scratch that the call resizes to sh * dw * c.
inline void resample_cpu(const u8* src, i32 sh, i32 sw, i32 c,
                         const ResampleAxis& ax, const ResampleAxis& ay,
                         u8* dst, std::vector<i16>& tmp) {
  SCA_CHECK(ax.n_src == sw && ay.n_src == sh, "resample: table/frame mismatch");
  const i32 dw = ax.n_dst, dh = ay.n_dst;
  const size_t row = (size_t)dw * c;
  tmp.resize((size_t)sh * row);
  for (i32 y = 0; y < sh; ++y) {
    const u8* s = src + (size_t)y * sw * c;
    i16* t = tmp.data() + (size_t)y * row;
    for (i32 x = 0; x < dw; ++x) {
      const i32* w = &ax.weights[(size_t)x * ax.max_taps];
      const u8* p = s + (size_t)ax.first[x] * c;
      const i32 n = ax.count[x];
      for (i32 ch = 0; ch < c; ++ch) {
        i32 acc = 0;
        for (i32 j = 0; j < n; ++j) acc += w[j] * (i32)p[(size_t)j * c + ch];
        t[(size_t)x * c + ch] =
            (i16)((acc + (1 << (kWeightBits - kInterBits - 1))) >>
                  (kWeightBits - kInterBits));
      }
    }
  }
  for (i32 y = 0; y < dh; ++y) {
    const i32* w = &ay.weights[(size_t)y * ay.max_taps];
    const i16* t = tmp.data() + (size_t)ay.first[y] * row;
    const i32 n = ay.count[y];
    u8* o = dst + (size_t)y * row;
    for (size_t i = 0; i < row; ++i) {
      i64 acc = 0;
      for (i32 j = 0; j < n; ++j) acc += (i64)w[j] * t[(size_t)j * row + i];
      i64 v = (acc + ((i64)1 << (kWeightBits + kInterBits - 1))) >>
              (kWeightBits + kInterBits);
      o[i] = (u8)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
  }
}

inline void resample_nearest_cpu(const u8* src, i32 sh, i32 sw, i32 c, u8* dst,
                                 i32 dh, i32 dw) {
  for (i32 y = 0; y < dh; ++y) {
    const u8* s = src + (size_t)resample_nearest_index(y, sh, dh) * sw * c;
    u8* o = dst + (size_t)y * dw * c;
    for (i32 x = 0; x < dw; ++x) {
      const u8* p = s + (size_t)resample_nearest_index(x, sw, dw) * c;
      for (i32 ch = 0; ch < c; ++ch) o[(size_t)x * c + ch] = p[ch];
    }
  }
}

}  // namespace sca
