// Filtered Resize on gfx950 (MI355X): "nearest", "box", "triangle", "cubic"
// and "lanczos3". The arithmetic is the integer scheme of
// csrc/ops/resample_common.h (Q22 weights, i16 Q6 intermediate, one rounding
// and clamp at the end), so the bytes equal the CPU kernel's.
//
// Structure. The frames of a batch are grouped by geometry (sh, sw, c, dh,
// dw); a group takes ONE launch per pass, with the frame index in grid.y and
// a device array of {src, dst, tmp} pointers. Tap tables are built on the
// host, uploaded once per (n_src, n_dst) and cached on the kernel object; the
// intermediate and the pointer array live in a grow-only workspace on the
// kernel object, so a steady-state call allocates only its outputs and never
// waits for the device.
//
//  * horizontal pass (resample_h_kernel): a workgroup owns `tx` output
//    columns of `rows` source rows. It stages the source span those outputs
//    read into LDS (8 KiB per workgroup: these passes are bandwidth- and
//    latency-bound, and 8 KiB leaves room for 8+ workgroups per CU), then one
//    lane per output (row, x, channel) loops over its taps. A span longer
//    than a row's share of the stage is consumed in chunks. Source rows start
//    at any byte address (13x17x3 frames carved from one block): the VEC
//    instantiation stages with 16-byte loads and is used only when every
//    frame of the group starts on a 16-byte boundary and the row pitch is a
//    multiple of 16; otherwise bytes.
//  * vertical pass (resample_v_kernel): lanes run along the contiguous x*c
//    dimension of one output row, so every tap reads one coalesced run of the
//    intermediate; first/count/weights of the row are wave-uniform.
//  * nearest (resample_nearest_kernel): a gather.
// Tiles are walked with a grid-stride loop (grid.x is capped), and taps are
// looped, never unrolled to a maximum: 4K -> 224 lanczos3 has ~100 per axis.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <map>

#include "../csrc/memory.h"
#include "resample.h"

namespace sca {

namespace {

#define HIPR_CHECK(expr)                                                  \
  do {                                                                    \
    hipError_t _e = (expr);                                               \
    if (_e != hipSuccess) {                                               \
      throw ScannerError(std::string("HIP error in Resize: ") +           \
                         hipGetErrorString(_e));                          \
    }                                                                     \
  } while (0)

struct FrameDesc {
  const u8* src;
  u8* dst;
  i16* tmp;
};

constexpr int kBlock = 256;
constexpr int kStageBytes = 8192;   // LDS per workgroup of the H pass
constexpr int kMaxRows = 8;         // source rows per workgroup of the H pass
constexpr u32 kMaxBlocks = 2048;    // per launch, over all frames of a group
constexpr u32 kMaxGridY = 32768;
constexpr int kHRound = kWeightBits - kInterBits;   // 16
constexpr int kVRound = kWeightBits + kInterBits;   // 28

// tab = [first: dw][count: dw][weights: dw * max_taps] of the x axis.
// A tile is `tx` outputs x `rows` source rows; cap = bytes of stage per row
// (a multiple of 16), chunk_px = (cap - 32) / c pixels staged at a time.
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
    resample_h_kernel(const FrameDesc* __restrict__ frames,
                      const i32* __restrict__ tab, int sh, int sw, int dw,
                      int c, int max_taps, int tx, int rows, int cap,
                      int chunk_px, u32 tiles_x, u32 total_tiles) {
  __shared__ uint4 stage4[kStageBytes / 16];
  u8* stage = reinterpret_cast<u8*>(stage4);
  const FrameDesc fr = frames[blockIdx.y];
  const i32* first = tab;
  const i32* count = tab + dw;
  const i32* wts = tab + 2 * (size_t)dw;
  const size_t pitch = (size_t)sw * c;
  const int tid = threadIdx.x;
  for (u32 t = blockIdx.x; t < total_tiles; t += gridDim.x) {
    const int x0 = (int)(t % tiles_x) * tx;
    const int y0 = (int)(t / tiles_x) * rows;
    const int xe = min(x0 + tx, dw);
    const int nr = min(rows, sh - y0);
    // first[] and first[] + count[] never decrease with x
    const int span_lo = first[x0];
    const int span_hi = first[xe - 1] + count[xe - 1];
    const int per_row = (xe - x0) * c;
    const int nitems = nr * per_row;
    // one round unless c > 256 (a tile is then one column of one row)
    for (int ib = 0; ib < nitems; ib += kBlock) {
      const int item = ib + tid;
      const bool live = item < nitems;
      int r = 0, x = x0, ch = 0, f = 0, n = 0;
      const i32* w = wts;
      if (live) {
        r = item / per_row;
        int rem = item - r * per_row;
        x = x0 + rem / c;
        ch = rem % c;
        f = first[x];
        n = count[x];
        w = wts + (size_t)x * max_taps;
      }
      i32 acc = 0;
      for (int cb = span_lo; cb < span_hi; cb += chunk_px) {
        const int ce = min(cb + chunk_px, span_hi);
        const int b0 = cb * c, b1 = ce * c;   // bytes of a row, [b0, b1)
        int off = 0;
        if (VEC) {
          // pitch % 16 == 0 and b1 <= pitch, so a1 <= pitch: no load leaves
          // its row. a1 - a0 <= chunk_px * c + 30 <= cap.
          const int a0 = b0 & ~15, a1 = (b1 + 15) & ~15;
          off = b0 - a0;
          const int nv = (a1 - a0) >> 4;
          for (int i = tid; i < nr * nv; i += kBlock) {
            int rr = i / nv, v = i - rr * nv;
            stage4[((rr * cap) >> 4) + v] = *reinterpret_cast<const uint4*>(
                fr.src + (size_t)(y0 + rr) * pitch + a0 + (size_t)v * 16);
          }
        } else {
          const int nb = b1 - b0;   // <= cap - 32
          for (int i = tid; i < nr * nb; i += kBlock) {
            int rr = i / nb, b = i - rr * nb;
            stage[rr * cap + b] =
                fr.src[(size_t)(y0 + rr) * pitch + b0 + b];
          }
        }
        __syncthreads();
        if (live) {
          const int k0 = max(f, cb), k1 = min(f + n, ce);
          const u8* p = stage + r * cap + off + ch;
          for (int k = k0; k < k1; ++k)
            acc += w[k - f] * (i32)p[(k - cb) * c];
        }
        __syncthreads();
      }
      if (live)
        fr.tmp[((size_t)(y0 + r) * dw + x) * c + ch] =
            (i16)((acc + (1 << (kHRound - 1))) >> kHRound);
    }
  }
}

// tab = the y axis table. A tile is 256 consecutive x*c positions of one
// output row; rowlen = dw * c.
__global__ void __launch_bounds__(kBlock)
    resample_v_kernel(const FrameDesc* __restrict__ frames,
                      const i32* __restrict__ tab, int dh, int rowlen,
                      int max_taps, u32 tiles_x, u32 total_tiles) {
  const FrameDesc fr = frames[blockIdx.y];
  for (u32 t = blockIdx.x; t < total_tiles; t += gridDim.x) {
    const int y = (int)(t / tiles_x);
    const int xc = (int)(t % tiles_x) * kBlock + threadIdx.x;
    const int first = tab[y];
    const int n = tab[dh + y];
    const i32* w = tab + 2 * (size_t)dh + (size_t)y * max_taps;
    if (xc < rowlen) {
      const i16* p = fr.tmp + (size_t)first * rowlen + xc;
      i64 acc = 0;
      for (int j = 0; j < n; ++j)
        acc += (i64)w[j] * (i64)p[(size_t)j * rowlen];
      i64 v = (acc + ((i64)1 << (kVRound - 1))) >> kVRound;
      fr.dst[(size_t)y * rowlen + xc] = (u8)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
  }
}

__global__ void __launch_bounds__(kBlock)
    resample_nearest_kernel(const FrameDesc* __restrict__ frames, int sh,
                            int sw, int dh, int dw, int c) {
  const FrameDesc fr = frames[blockIdx.y];
  const u64 total = (u64)dh * dw * c;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    u32 ch = (u32)(i % c);
    u64 pix = i / c;
    u64 x = pix % dw, y = pix / dw;
    u64 sx = ((2 * x + 1) * (u64)sw) / (2 * (u64)dw);   // < sw
    u64 sy = ((2 * y + 1) * (u64)sh) / (2 * (u64)dh);   // < sh
    fr.dst[i] = fr.src[(sy * sw + sx) * c + ch];
  }
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

struct ResampleGPU::Impl {
  struct AxisTable {
    u8* dev = nullptr;
    i32 max_taps = 0;
    std::vector<i32> host;   // the upload's source, kept for its lifetime
    // span[i]: most source pixels that the outputs of one tile of 1 << i
    // columns read
    i32 span[9] = {0};
  };

  DeviceHandle device;
  ResampleFilter filter;
  u64 gen = 0;
  hipStream_t last_stream = nullptr;
  bool issued = false;
  std::map<std::pair<i32, i32>, AxisTable> tables;
  u8* work = nullptr;
  size_t work_size = 0;
  u8* descs = nullptr;
  size_t descs_cap = 0;
  std::vector<FrameDesc> host_descs;

  // Buffers of an older allocator generation are gone with their pool:
  // forget them, never free them into the current one (csrc/memory.h).
  void check_generation() {
    if (gen == memory_generation()) return;
    tables.clear();
    work = descs = nullptr;
    work_size = descs_cap = 0;
    issued = false;
    gen = memory_generation();
  }

  void wait() {
    if (issued) (void)hipStreamSynchronize(last_stream);
    issued = false;
  }

  void drop_tables() {
    for (auto& kv : tables)
      if (kv.second.dev) delete_buffer(device, kv.second.dev);
    tables.clear();
  }

  void release() {
    if (!memory_initialized() || gen != memory_generation()) return;
    wait();   // the kernels that read these buffers have finished
    drop_tables();
    if (work) delete_buffer(device, work);
    if (descs) delete_buffer(device, descs);
    work = descs = nullptr;
    work_size = descs_cap = 0;
  }

  // Grow-only; the rare growth waits for the stream before the old buffer
  // goes back to the shared pool.
  void ensure(u8*& buf, size_t& cap, size_t want) {
    if (want <= cap) return;
    if (buf) {
      wait();
      delete_buffer(device, buf);
      buf = nullptr;
      cap = 0;
    }
    buf = new_buffer(device, want);
    cap = want;
  }

  const AxisTable& table(i32 n_src, i32 n_dst, hipStream_t s) {
    auto key = std::make_pair(n_src, n_dst);
    auto it = tables.find(key);
    if (it != tables.end()) return it->second;
    ResampleAxis ax = resample_build_axis(filter, n_src, n_dst);
    AxisTable t;
    t.max_taps = ax.max_taps;
    for (int i = 0; i < 9; ++i) {
      i32 tx = 1 << i, worst = 0;
      for (i32 x0 = 0; x0 < n_dst; x0 += tx) {
        i32 xe = std::min(x0 + tx, n_dst);
        worst = std::max(worst,
                         ax.first[xe - 1] + ax.count[xe - 1] - ax.first[x0]);
      }
      t.span[i] = worst;
    }
    t.host = ax.packed();
    size_t bytes = t.host.size() * sizeof(i32);
    t.dev = new_buffer(device, bytes);
    AxisTable& slot = tables.emplace(key, std::move(t)).first->second;
    HIPR_CHECK(hipMemcpyAsync(slot.dev, slot.host.data(), bytes,
                              hipMemcpyHostToDevice, s));
    return slot;
  }
};

ResampleGPU::ResampleGPU(DeviceHandle device, ResampleFilter filter)
    : impl_(new Impl) {
  SCA_CHECK(filter != ResampleFilter::kBilinear,
            "ResampleGPU does not run the bilinear sampler");
  impl_->device = device;
  impl_->filter = filter;
  impl_->gen = memory_generation();
}

ResampleGPU::~ResampleGPU() { impl_->release(); }

void ResampleGPU::run(const ElementVector& in,
                      const std::vector<std::pair<i32, i32>>& dst_hw,
                      ElementVector& out, void* stream) {
  Impl& m = *impl_;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = in.size();
  if (n == 0) return;
  SCA_CHECK(dst_hw.size() == n, "Resize: one output size per frame");
  m.check_generation();
  if (m.issued && m.last_stream != s) m.wait();
  m.last_stream = s;
  // a column of ever-changing sizes must not grow the cache without bound
  if (m.tables.size() > 64) {
    m.wait();
    m.drop_tables();
  }
  const bool conv = resample_is_convolution(m.filter);

  // group by geometry, in order of first appearance within a group
  std::map<std::array<i32, 5>, std::vector<size_t>> groups;
  for (size_t i = 0; i < n; ++i) {
    const Element& f = in[i];
    SCA_CHECK(f.is_frame && f.device.is_gpu(), "GPU Resize needs GPU input");
    SCA_CHECK(f.frame_info.type == FrameType::U8,
              "Resize filters other than 'bilinear' need u8 frames");
    i32 h = f.frame_info.shape[0], w = f.frame_info.shape[1],
        c = f.frame_info.shape[2];
    SCA_CHECK(h > 0 && w > 0 && c > 0, "Resize needs a non-empty frame");
    SCA_CHECK(c <= 4096, "Resize filters support at most 4096 channels");
    SCA_CHECK((u64)w * c < (1ull << 31), "Resize: source row too long");
    SCA_CHECK(dst_hw[i].first > 0 && dst_hw[i].second > 0,
              "Resize output size must be positive");
    groups[{h, w, c, dst_hw[i].first, dst_hw[i].second}].push_back(i);
  }

  // outputs, in input order; `out` owns them from here on
  const size_t out_base = out.size();
  size_t tmp_total = 0;
  for (size_t i = 0; i < n; ++i) {
    Element e;
    e.is_frame = true;
    e.frame_info.shape[0] = dst_hw[i].first;
    e.frame_info.shape[1] = dst_hw[i].second;
    e.frame_info.shape[2] = in[i].frame_info.shape[2];
    e.frame_info.type = FrameType::U8;
    e.size = e.frame_info.size();
    e.buffer = new_buffer(m.device, e.size);
    e.device = m.device;
    out.push_back(e);
    if (conv)
      tmp_total += align16((size_t)in[i].frame_info.shape[0] *
                           dst_hw[i].second * in[i].frame_info.shape[2] *
                           sizeof(i16));
  }
  if (conv) m.ensure(m.work, m.work_size, tmp_total);
  m.ensure(m.descs, m.descs_cap, n * sizeof(FrameDesc));

  // descriptors ordered by group, one upload
  m.host_descs.resize(n);
  {
    size_t k = 0, tmp_off = 0;
    for (auto& g : groups) {
      for (size_t i : g.second) {
        FrameDesc& d = m.host_descs[k++];
        d.src = in[i].buffer;
        d.dst = out[out_base + i].buffer;
        d.tmp = conv ? reinterpret_cast<i16*>(m.work + tmp_off) : nullptr;
        if (conv)
          tmp_off += align16((size_t)in[i].frame_info.shape[0] *
                             dst_hw[i].second * in[i].frame_info.shape[2] *
                             sizeof(i16));
      }
    }
  }
  m.issued = true;
  HIPR_CHECK(hipMemcpyAsync(m.descs, m.host_descs.data(),
                            n * sizeof(FrameDesc), hipMemcpyHostToDevice, s));

  size_t base = 0;
  for (auto& g : groups) {
    const i32 sh = g.first[0], sw = g.first[1], c = g.first[2],
              dh = g.first[3], dw = g.first[4];
    const size_t gn = g.second.size();
    const Impl::AxisTable* tx_tab = nullptr;
    const Impl::AxisTable* ty_tab = nullptr;
    int tx = 1, rows = 1, cap = kStageBytes, chunk_px = 1;
    bool vec = false;
    if (conv) {
      tx_tab = &m.table(sw, dw, s);
      ty_tab = &m.table(sh, dh, s);   // std::map: tx_tab stays valid
      // the widest tile (a power of two, tx * c <= 256, not wider than the
      // row needs) whose span fits the stage in one chunk; else one column
      int top = 0;
      while (top < 8 && (2 << top) * c <= kBlock && (1 << top) < dw) ++top;
      auto shape = [&](int i) {
        tx = 1 << i;
        rows = std::max(1, std::min({kMaxRows, kBlock / (tx * c), (int)sh}));
        cap = (kStageBytes / rows) & ~15;
        chunk_px = (cap - 32) / c;
      };
      int pick = top;
      for (; pick >= 0; --pick) {
        shape(pick);
        if (tx_tab->span[pick] <= chunk_px) break;
      }
      if (pick < 0) shape(0);
      SCA_CHECK(chunk_px >= 1 && rows * cap <= kStageBytes,
                "Resize: horizontal tile does not fit its stage");
      vec = ((size_t)sw * c) % 16 == 0;
      for (size_t i : g.second)
        vec = vec && ((uintptr_t)in[i].buffer & 15) == 0;
    }
    for (size_t f0 = 0; f0 < gn; f0 += kMaxGridY) {
      const u32 gy = (u32)std::min<size_t>(kMaxGridY, gn - f0);
      const u32 cap_x = std::max<u32>(1, kMaxBlocks / gy);
      const FrameDesc* d =
          reinterpret_cast<const FrameDesc*>(m.descs) + base + f0;
      if (!conv) {
        u64 total = (u64)dh * dw * c;
        u32 gx = (u32)std::min<u64>(cap_x, (total + kBlock - 1) / kBlock);
        resample_nearest_kernel<<<dim3(gx, gy), kBlock, 0, s>>>(d, sh, sw, dh,
                                                                dw, c);
        HIPR_CHECK(hipGetLastError());
        continue;
      }
      {
        u32 tiles_x = (u32)((dw + tx - 1) / tx);
        u64 tiles = (u64)tiles_x * (u64)((sh + rows - 1) / rows);
        SCA_CHECK(tiles < (1ull << 32), "Resize: frame too large");
        u32 gx = (u32)std::min<u64>(cap_x, tiles);
        const i32* tab = reinterpret_cast<const i32*>(tx_tab->dev);
        if (vec) {
          resample_h_kernel<true><<<dim3(gx, gy), kBlock, 0, s>>>(
              d, tab, sh, sw, dw, c, tx_tab->max_taps, tx, rows, cap, chunk_px,
              tiles_x, (u32)tiles);
        } else {
          resample_h_kernel<false><<<dim3(gx, gy), kBlock, 0, s>>>(
              d, tab, sh, sw, dw, c, tx_tab->max_taps, tx, rows, cap, chunk_px,
              tiles_x, (u32)tiles);
        }
        HIPR_CHECK(hipGetLastError());
      }
      {
        u64 rowlen = (u64)dw * c;
        SCA_CHECK(rowlen < (1ull << 31), "Resize: output row too long");
        u32 tiles_x = (u32)((rowlen + kBlock - 1) / kBlock);
        u64 tiles = (u64)tiles_x * (u64)dh;
        SCA_CHECK(tiles < (1ull << 32), "Resize: frame too large");
        u32 gx = (u32)std::min<u64>(cap_x, tiles);
        resample_v_kernel<<<dim3(gx, gy), kBlock, 0, s>>>(
            d, reinterpret_cast<const i32*>(ty_tab->dev), dh, (int)rowlen,
            ty_tab->max_taps, tiles_x, (u32)tiles);
        HIPR_CHECK(hipGetLastError());
      }
    }
    base += gn;
  }
}

}  // namespace sca
