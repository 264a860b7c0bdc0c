// GPU encoder for the SVC codec (format: csrc/video/svc.h) — the sink-side
// counterpart of svc_codec.hip: device-resident u8 frames are turned into
// SVC packets in HBM and only the compressed bytes cross the host link.
// The output is byte-identical to svc_encode_cpu.
//
// Kernel shape (three launches per chunk of <= 16 frames, independent of
// the frame count; keyframes are a bit in a mask):
//   widths  grid (nsuper, nframes) x 128 lanes, one lane per 32-byte group:
//           zigzag residuals in registers -> max -> bit width. Writes the
//           packet header, width[g] and the supergroup's payload total.
//   scan    one workgroup per frame: exclusive scan of the nsuper totals
//           (any count, 256 per step with a running carry) -> super_off[]
//           and the packet's size.
//   pack    same grid as widths: residuals are recomputed (the raw frame is
//           re-read instead of 32 B/group of residuals being spilled), each
//           lane packs its group's `width` u32 words LSB-first into an LDS
//           image of the supergroup's <= 4 KiB payload, and the workgroup
//           writes that image out contiguously.
// Packets sit in device staging at the worst-case stride svc_packet_bound;
// the host copies only each packet's used prefix.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../csrc/memory.h"
#include "../csrc/video/svc.h"

namespace sca {

namespace {

#define SVC_ENC_CHECK(expr)                                              \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess) {                                              \
      throw ScannerError(std::string("HIP error in svc encode: ") +      \
                         hipGetErrorString(_e));                         \
    }                                                                    \
  } while (0)

constexpr int kEncBatch = 16;  // frames per launch sequence (= kGopBatch)
constexpr u32 kMagic = 0x31435653;  // 'SVC1' LE

// frame load paths, chosen on the host from pointer/size alignment
enum : u32 { kLoad16 = 0, kLoad4 = 1, kLoad1 = 2 };

struct SvcEncArgs {
  const u8* frames[kEncBatch];
  const u8* prev;  // prediction source of frame 0 when it is a delta frame
  u8* staging;     // packets at f * stride
  u32* totals;     // [nframes][nsuper] payload bytes per supergroup
  u32* sizes;      // [nframes] packet sizes
  u64 stride;
  u32 key_mask;    // bit f = frame f is a keyframe
  u32 nframes;
  u32 nbytes, ngroups, nsuper;
  u32 load_mode;
};

// Load the 32 bytes of group `base/32` as 8 little-endian words; bytes at
// or past `nvalid` (tail group) are not read and come back as zero.
__device__ inline void load_group(const u8* __restrict__ p, u64 base,
                                  u32 nvalid, u32 mode, u32 (&v)[8]) {
  if (nvalid == 32 && mode == kLoad16) {
    const uint4* p4 = reinterpret_cast<const uint4*>(p + base);
    uint4 a = p4[0], b = p4[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else if (nvalid == 32 && mode == kLoad4) {
    const u32* p1 = reinterpret_cast<const u32*>(p + base);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p1[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0;
#pragma unroll
    for (u32 k = 0; k < 32; ++k) {
      if (k < nvalid) v[k / 4] |= (u32)p[base + k] << (8 * (k & 3));
    }
  }
}

__device__ inline u32 dev_zigzag(u32 cur, u32 pred) {
  u32 v = (cur - pred) & 0xffu;              // residual as i8 bits
  u32 sign = (v & 0x80u) ? 0xffu : 0u;       // arithmetic v >> 7
  return ((v << 1) & 0xffu) ^ sign;
}

// Zigzag residuals of one group, 4 per word. Key groups predict from the
// previous byte within the group (first byte from 128), delta groups from
// the same byte of the previous frame. Bytes past the frame give 0.
__device__ inline u32 group_residuals(const u32 (&cur)[8], const u32 (&prv)[8],
                                      bool key, u32 nvalid, u32 (&res)[8]) {
  u32 mx = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    u32 pred = prv[k];
    if (key) pred = (cur[k] << 8) | (k == 0 ? 128u : (cur[k - 1] >> 24));
    u32 r = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      u32 z = dev_zigzag((cur[k] >> (8 * b)) & 0xffu,
                         (pred >> (8 * b)) & 0xffu);
      if ((u32)(4 * k + b) >= nvalid) z = 0;
      mx = max(mx, z);
      r |= z << (8 * b);
    }
    res[k] = r;
  }
  return mx;
}

// 0->0, 1->1, 2-3->2, ..., 128-255->8
__device__ inline u32 dev_bits_needed(u32 maxz) {
  return maxz == 0 ? 0u : 32u - (u32)__clz((int)maxz);
}

struct GroupCtx {
  u32 g;       // group index within the frame
  u32 nvalid;  // payload bytes in this group (0 for a lane past ngroups)
};

__device__ inline GroupCtx group_ctx(const SvcEncArgs& a, u32 s, u32 tid) {
  GroupCtx c;
  c.g = s * 128 + tid;
  c.nvalid = 0;
  if (c.g < a.ngroups) {
    u64 base = (u64)c.g * 32;
    u64 left = (u64)a.nbytes - base;
    c.nvalid = left < 32 ? (u32)left : 32u;
  }
  return c;
}

// residuals + width of this lane's group in frame f
__device__ inline u32 lane_residuals(const SvcEncArgs& a, u32 f,
                                     const GroupCtx& c, u32 (&res)[8]) {
  u32 cur[8], prv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { cur[k] = 0; prv[k] = 0; res[k] = 0; }
  if (c.nvalid == 0) return 0;
  bool key = (a.key_mask >> f) & 1u;
  u64 base = (u64)c.g * 32;
  load_group(a.frames[f], base, c.nvalid, a.load_mode, cur);
  if (!key) {
    const u8* pp = f == 0 ? a.prev : a.frames[f - 1];
    load_group(pp, base, c.nvalid, a.load_mode, prv);
  }
  return dev_bits_needed(group_residuals(cur, prv, key, c.nvalid, res));
}

__global__ void __launch_bounds__(128)
    svc_encode_widths_kernel(SvcEncArgs a) {
  __shared__ u32 wave_sum[2];
  u32 s = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  GroupCtx c = group_ctx(a, s, tid);
  u32 res[8];
  u32 w = lane_residuals(a, f, c, res);

  u8* pkt = a.staging + (u64)f * a.stride;
  u8* widths = pkt + 20ull + (u64)a.nsuper * 4;
  if (c.nvalid) {
    widths[c.g] = (u8)w;
    if (c.g == a.ngroups - 1) {
      // zero the pad up to the 4-byte aligned packed region
      for (u32 p = a.ngroups; p < (a.ngroups + 3) / 4 * 4; ++p) widths[p] = 0;
    }
  }
  if (s == 0 && tid == 0) {
    u32* h = reinterpret_cast<u32*>(pkt);
    h[0] = kMagic;
    h[1] = ((a.key_mask >> f) & 1u) ? 0u : 1u;  // type byte + 3 pad bytes
    h[2] = a.nbytes;
    h[3] = a.ngroups;
    h[4] = a.nsuper;
  }

  u32 sum = 4u * w;
#pragma unroll
  for (u32 d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) a.totals[(u64)f * a.nsuper + s] = wave_sum[0] + wave_sum[1];
}

// One workgroup per frame; 256 totals per step, carry kept across steps.
__global__ void __launch_bounds__(256) svc_encode_scan_kernel(SvcEncArgs a) {
  __shared__ u32 wave_sum[4];
  u32 f = blockIdx.x, tid = threadIdx.x;
  u32 lane = tid & 63, wave = tid >> 6;
  u8* pkt = a.staging + (u64)f * a.stride;
  u32* super_off = reinterpret_cast<u32*>(pkt + 20);
  const u32* totals = a.totals + (u64)f * a.nsuper;
  u32 carry = 0;
  for (u32 s0 = 0; s0 < a.nsuper; s0 += 256) {
    u32 s = s0 + tid;
    u32 val = s < a.nsuper ? totals[s] : 0;
    u32 x = val;
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
      u32 y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    u32 before = 0, all = 0;
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
      u32 t = wave_sum[k];
      if (k < wave) before += t;
      all += t;
    }
    if (s < a.nsuper) super_off[s] = carry + before + x - val;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) {
    u64 head = 20ull + (u64)a.nsuper * 4 + (u64)((a.ngroups + 3) / 4 * 4);
    a.sizes[f] = (u32)(head + carry);
  }
}

__global__ void __launch_bounds__(128) svc_encode_pack_kernel(SvcEncArgs a) {
  __shared__ u32 stage[1024];  // 128 groups x <= 8 words
  __shared__ u32 wave_sum[2];
  u32 s = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  u32 lane = tid & 63, wave = tid >> 6;
  GroupCtx c = group_ctx(a, s, tid);
  u32 res[8];
  u32 w = lane_residuals(a, f, c, res);

  // in-block exclusive prefix of the per-group word counts
  u32 x = w;
#pragma unroll
  for (u32 d = 1; d < 64; d <<= 1) {
    u32 y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wave_sum[wave] = x;
  __syncthreads();
  u32 my_word = x - w + (wave == 1 ? wave_sum[0] : 0u);
  u32 total_words = wave_sum[0] + wave_sum[1];

  if (w) {
    // values k = 0..31, w bits each, LSB first; word j = bits [32j, 32j+32)
    u64 acc = 0;
    u32 nacc = 0, qi = my_word;
    u32 mask = (1u << w) - 1;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      u32 r = (res[k / 4] >> (8 * (k & 3))) & mask;
      acc |= (u64)r << nacc;
      nacc += w;
      if (nacc >= 32) {
        stage[qi++] = (u32)acc;
        acc >>= 32;
        nacc -= 32;
      }
    }
  }
  __syncthreads();

  u8* pkt = a.staging + (u64)f * a.stride;
  const u32* super_off = reinterpret_cast<const u32*>(pkt + 20);
  u64 packed_off = 20ull + (u64)a.nsuper * 4 + (u64)((a.ngroups + 3) / 4 * 4);
  u32* dst = reinterpret_cast<u32*>(pkt + (packed_off + (u64)super_off[s]));
  for (u32 i = tid; i < total_words; i += 128) dst[i] = stage[i];
}

}  // namespace

void svc_encode_gpu(const std::vector<const u8*>& frames, const u8* prev,
                    const std::vector<u8>& key, u32 nbytes, DeviceHandle dev,
                    std::vector<u8>& stream, std::vector<u64>& sizes) {
  SCA_CHECK(frames.size() == key.size(), "svc encode: frames/key mismatch");
  SCA_CHECK(nbytes > 0, "svc encode: empty frame");
  SCA_CHECK(dev.is_gpu(), "svc_encode_gpu needs a GPU device");
  if (frames.empty()) return;
  SCA_CHECK(key[0] || prev, "svc encode: delta frame without a predecessor");
  SVC_ENC_CHECK(hipSetDevice(dev.id));
  hipStream_t s = (hipStream_t)per_thread_hip_stream();

  u32 ngroups = (u32)(((u64)nbytes + 31) / 32);
  u32 nsuper = (ngroups + 127) / 128;
  // packets at a 16-byte multiple of the worst case; the totals and sizes
  // arrays follow them in the same slab-pool allocation
  u64 stride = (svc_packet_bound(nbytes) + 15) / 16 * 16;
  size_t chunk_max = std::min<size_t>(frames.size(), kEncBatch);
  u64 totals_off = stride * chunk_max;
  u64 sizes_off = totals_off + (u64)chunk_max * nsuper * 4;
  u64 staging_bytes = sizes_off + (u64)chunk_max * 4;
  u8* staging = new_buffer(dev, staging_bytes);
  u32 host_sizes[kEncBatch];

  try {
    for (size_t c0 = 0; c0 < frames.size(); c0 += kEncBatch) {
      size_t n = std::min<size_t>(kEncBatch, frames.size() - c0);
      SvcEncArgs a{};
      a.staging = staging;
      a.totals = reinterpret_cast<u32*>(staging + totals_off);
      a.sizes = reinterpret_cast<u32*>(staging + sizes_off);
      a.stride = stride;
      a.nframes = (u32)n;
      a.nbytes = nbytes;
      a.ngroups = ngroups;
      a.nsuper = nsuper;
      a.prev = c0 == 0 ? prev : frames[c0 - 1];
      // Frames carved out of a block buffer with an odd frame size are not
      // 16-byte aligned: pick the widest load every pointer allows.
      uintptr_t align = (uintptr_t)nbytes;
      if (!key[c0]) align |= (uintptr_t)a.prev;
      for (size_t i = 0; i < n; ++i) {
        SCA_CHECK(frames[c0 + i], "svc encode: null frame pointer");
        a.frames[i] = frames[c0 + i];
        if (key[c0 + i]) a.key_mask |= 1u << i;
        align |= (uintptr_t)frames[c0 + i];
      }
      a.load_mode = (align & 15) == 0 ? kLoad16 : (align & 3) == 0 ? kLoad4
                                                                   : kLoad1;
      dim3 grid(nsuper, (u32)n);
      svc_encode_widths_kernel<<<grid, 128, 0, s>>>(a);
      SVC_ENC_CHECK(hipGetLastError());
      svc_encode_scan_kernel<<<(u32)n, 256, 0, s>>>(a);
      SVC_ENC_CHECK(hipGetLastError());
      SVC_ENC_CHECK(hipMemcpyAsync(host_sizes, a.sizes, n * 4,
                                   hipMemcpyDeviceToHost, s));
      svc_encode_pack_kernel<<<grid, 128, 0, s>>>(a);
      SVC_ENC_CHECK(hipGetLastError());
      SVC_ENC_CHECK(hipStreamSynchronize(s));

      // only the used prefix of each packet crosses the host link
      size_t pos = stream.size();
      u64 total = 0;
      for (size_t i = 0; i < n; ++i) {
        SCA_CHECK(host_sizes[i] >= 20 && host_sizes[i] <= stride,
                  "svc encode: packet size out of range");
        total += host_sizes[i];
      }
      stream.resize(pos + total);
      for (size_t i = 0; i < n; ++i) {
        SVC_ENC_CHECK(hipMemcpyAsync(stream.data() + pos,
                                     staging + (u64)i * stride, host_sizes[i],
                                     hipMemcpyDeviceToHost, s));
        pos += host_sizes[i];
        sizes.push_back(host_sizes[i]);
      }
      SVC_ENC_CHECK(hipStreamSynchronize(s));
    }
  } catch (...) {
    (void)hipStreamSynchronize(s);
    delete_buffer(dev, staging);
    throw;
  }
  delete_buffer(dev, staging);
}

}  // namespace sca
