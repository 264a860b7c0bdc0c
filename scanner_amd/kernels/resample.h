// Host interface of kernels/resample.hip: the filtered Resize paths on the
// GPU ("nearest", "box", "triangle", "cubic", "lanczos3"). ResizeKernelGPU
// (image_ops.hip) owns one ResampleGPU per kernel object and hands it every
// batch whose filter is not "bilinear".
#pragma once

#include <memory>
#include <vector>

#include "../csrc/element.h"
#include "../csrc/ops/resample_common.h"

namespace sca {

class ResampleGPU {
 public:
  ResampleGPU(DeviceHandle device, ResampleFilter filter);
  ~ResampleGPU();
  ResampleGPU(const ResampleGPU&) = delete;
  ResampleGPU& operator=(const ResampleGPU&) = delete;

  // Resamples in[i] (u8 HWC frames on the device) to dst_hw[i] = (dh, dw)
  // and appends one frame per input to `out`, in order. Frames are grouped
  // by geometry; each group takes one launch per pass on `stream`.
  void run(const ElementVector& in,
           const std::vector<std::pair<i32, i32>>& dst_hw, ElementVector& out,
           void* stream);

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace sca
