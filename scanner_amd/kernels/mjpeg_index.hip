// Device-side restart-segment index for Motion-JPEG on gfx950, and the GPU
// decode of an mjpeg item that is resident in HBM (csrc/video/mjpeg.h).
//
// The video path keeps compressed spans in HBM and must not touch them on
// the host, but the JPEG decode kernels (kernels/jpeg_decode.hip) need to
// know where every restart segment of every file begins and ends. For a
// still image the host finds that out while parsing. Here a kernel does:
// one workgroup per wanted frame classifies the bytes of the frame's scan
// with the position-independent rule of csrc/video/mjpeg_common.h, compacts
// the RSTn positions in order with a block scan, and writes the JpegDecSeg
// records that jpeg_entropy_idct_kernel then consumes, offsets relative to
// the span. The host contributes one header per item: every descriptor is
// built from it, and the kernel refuses a frame whose first bytes differ.
//
// Layout: 256 lanes x 16 bytes = one 4 KiB tile per step. A lane's 16 bytes
// sit at a 16-byte aligned ADDRESS (frames start at any byte, so the first
// and last chunk of a frame are partial): whole chunks are one dwordx4
// load, partial ones are read byte by byte. The lane also needs the byte
// behind its chunk to classify its last position. Bytes outside
// [header_len, size) of the sample are never read; they count as 00, which
// starts no marker and makes no FF a marker. The next tile is loaded before
// the current one is classified, so the barriers of a step overlap a load.
//
// Per step: (1) every lane finds its markers, and the first one that is not
// RSTn goes to an LDS minimum, the end of the scan; barrier; (2) RSTn
// before that end are counted, an exclusive scan over the block (wave
// shuffles, then four wave sums through LDS) numbers them, and marker k
// closes segment k and opens segment k + 1, after the sequence check;
// barrier. The step that found the end is the last.
//
// Bounds: reads are confined to the sample by construction of the load;
// segment writes to k + 1 < nseg; everything else is a status word. A frame
// that fails keeps mcu_count 0 in every record, so the entropy kernel does
// nothing for it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../csrc/memory.h"
#include "../csrc/video/mjpeg.h"
#include "jpeg_decode_dev.h"

namespace sca {

namespace {

#define MJPEG_CHECK(expr)                                                \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess) {                                              \
      throw ScannerError(std::string("HIP error in mjpeg decode: ") +    \
                         hipGetErrorString(_e));                         \
    }                                                                    \
  } while (0)

constexpr u32 kIndexThreads = 256;
constexpr u32 kLaneBytes = 16;
constexpr u32 kTileBytes = kIndexThreads * kLaneBytes;
constexpr u32 kNone = 0xffffffffu;

static_assert(sizeof(MjpegSeg) == sizeof(JpegDecSeg), "one record layout");

struct MjpegIndexArgs {
  const u8* span;          // segment offsets are relative to this
  const u32* sample_off;   // per frame, from `span`
  const u32* sample_size;  // per frame
  const u8* ref_header;    // p.header_len bytes
  MjpegSeg* segs;          // p.nseg per frame, zeroed by the caller
  u32* status;             // per frame
  MjpegIndexParams p;
};

// 16 bytes of a sample at sample-relative position c (which may be negative
// or reach past the end), and the byte behind them, as 17 bytes in five
// words. Positions outside [lo, size) read as 00 and are not touched.
struct Chunk {
  u32 w0, w1, w2, w3;
  u32 next;
};
__device__ inline Chunk load_chunk(const u8* b, i64 c, i64 lo, i64 size) {
  Chunk ch;
  if (c >= lo && c + kLaneBytes <= size) {
    // b + c is 16-byte aligned: the tiles start at an aligned address
    uint4 v = *reinterpret_cast<const uint4*>(b + c);
    ch.w0 = v.x;
    ch.w1 = v.y;
    ch.w2 = v.z;
    ch.w3 = v.w;
  } else {
    ch.w0 = ch.w1 = ch.w2 = ch.w3 = 0;
    if (c + kLaneBytes > lo && c < size) {
      auto at = [&](u32 j) -> u32 {
        i64 pos = c + j;
        return pos >= lo && pos < size ? (u32)b[pos] << (8 * (j & 3)) : 0u;
      };
      ch.w0 = at(0) | at(1) | at(2) | at(3);
      ch.w1 = at(4) | at(5) | at(6) | at(7);
      ch.w2 = at(8) | at(9) | at(10) | at(11);
      ch.w3 = at(12) | at(13) | at(14) | at(15);
    }
  }
  i64 pn = c + kLaneBytes;
  ch.next = pn >= lo && pn < size ? b[pn] : 0u;
  return ch;
}
__device__ inline u32 chunk_byte(const Chunk& ch, u32 j) {
  // selects, not an indexed read: with a run-time j the words stay in
  // registers
  u32 i = j >> 2;
  u32 word = i == 0 ? ch.w0 : i == 1 ? ch.w1 : i == 2 ? ch.w2 : ch.w3;
  return j < kLaneBytes ? (word >> (8 * (j & 3))) & 0xffu : ch.next;
}

__global__ void __launch_bounds__(kIndexThreads) mjpeg_index_kernel(
    MjpegIndexArgs a) {
  __shared__ u32 s_differs, s_end, s_failed, s_status;
  __shared__ u32 s_wave[kIndexThreads / 64];
  const u32 f = blockIdx.x, tid = threadIdx.x;
  const MjpegIndexParams& p = a.p;
  const u32 off = a.sample_off[f];
  const u32 size = a.sample_size[f];
  const u8* b = a.span + off;
  MjpegSeg* segs = a.segs + (u64)f * p.nseg;

  if (tid == 0) {
    s_differs = size < p.header_len ? 1u : 0u;
    s_end = kNone;
    s_failed = kMjpegStatusNone;
  }
  __syncthreads();
  if (size >= p.header_len) {
    bool differs = false;
    for (u32 i = tid; i < p.header_len; i += kIndexThreads)
      differs |= b[i] != a.ref_header[i];
    if (differs) atomicOr(&s_differs, 1u);
  }
  __syncthreads();
  if (s_differs) {
    if (tid == 0) a.status[f] = kMjpegHeaderDiffers;
    return;
  }

  const i64 lo = p.header_len, sz = size;
  // tiles start at the 16-byte aligned address at or below the first
  // entropy byte
  const i64 start =
      lo - (i64)(reinterpret_cast<uintptr_t>(b + lo) & (kLaneBytes - 1));
  u32 nrst = 0;  // RSTn before this tile, the same in every lane
  i64 c = start + (i64)tid * kLaneBytes;
  Chunk cur = load_chunk(b, c, lo, sz);
  for (i64 t = start; t < sz; t += kTileBytes, c += kTileBytes) {
    Chunk nxt = load_chunk(b, c + kTileBytes, lo, sz);
    // (1) markers of this lane; the first that is not RSTn ends the scan
    u32 mask = 0, first_other = kNone;
#pragma unroll
    for (u32 j = 0; j < kLaneBytes; ++j) {
      u32 b0 = chunk_byte(cur, j), b1 = chunk_byte(cur, j + 1);
      if (mjpeg_is_marker2(b0, b1, true)) {
        mask |= 1u << j;
        if (!mjpeg_is_rst(b1) && first_other == kNone)
          first_other = (u32)(c + j);
      }
    }
    if (first_other != kNone) atomicMin(&s_end, first_other);
    __syncthreads();
    const u32 end = s_end;
    // (2) RSTn before the end, numbered in order
    u32 rmask = 0;
#pragma unroll
    for (u32 j = 0; j < kLaneBytes; ++j)
      if ((mask >> j & 1u) && (u64)(c + j) < (u64)end) rmask |= 1u << j;
    u32 cnt = __popc(rmask), incl = cnt;
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
      u32 up = __shfl_up(incl, d, 64);
      if ((tid & 63u) >= d) incl += up;
    }
    if ((tid & 63u) == 63u) s_wave[tid >> 6] = incl;
    __syncthreads();
    u32 k = nrst + incl - cnt, total = 0;
#pragma unroll
    for (u32 wv = 0; wv < kIndexThreads / 64; ++wv) {
      u32 ws = s_wave[wv];
      if (wv < (tid >> 6)) k += ws;
      total += ws;
    }
    while (rmask) {
      u32 j = __ffs(rmask) - 1;
      rmask &= rmask - 1;
      if (k + 1 < p.nseg) {
        u32 pos = (u32)(c + j);
        if (!mjpeg_rst_in_sequence(k, chunk_byte(cur, j + 1)))
          atomicMin(&s_failed, (u32)kMjpegRstSequence);
        segs[k].end = off + pos;
        segs[k + 1].begin = off + pos + 2;
      }
      ++k;
    }
    nrst += total;
    if (end != kNone) break;  // the same in every lane
    cur = nxt;
  }
  __syncthreads();
  if (tid == 0) {
    u32 e = s_end;
    size_t end = e == kNone ? (size_t)size : (size_t)e;
    // a marker has a follower inside the sample, by the rule
    u32 end_code = e == kNone ? 0u : b[e + 1];
    u32 st = mjpeg_verdict(p, size, end, end_code, nrst, s_failed);
    if (st == kMjpegOk) {
      segs[0].begin = off + p.header_len;
      segs[p.nseg - 1].end = off + (u32)end;
    }
    a.status[f] = st;
    s_status = st;
  }
  __syncthreads();
  if (s_status != kMjpegOk) return;
  for (u32 k = tid; k < p.nseg; k += kIndexThreads)
    mjpeg_seg_mcus(p, k, segs[k].first_mcu, segs[k].mcu_count);
}

u64 align_up(u64 x, u64 a) { return (x + a - 1) / a * a; }

Element frame_element(const VideoMetadata& vm, u8* buffer, DeviceHandle dev,
                      i64 index) {
  Element e;
  e.is_frame = true;
  e.frame_info.shape[0] = vm.height;
  e.frame_info.shape[1] = vm.width;
  e.frame_info.shape[2] = vm.channels;
  e.frame_info.type = FrameType::U8;
  e.size = (size_t)vm.height * vm.width * vm.channels;
  e.buffer = buffer;
  e.device = dev;
  e.index = index;
  return e;
}

// Frames the device did not take: their bytes come back from the span and
// go through the still-image path with the serial-scan decoder on.
void decode_fallback(const u8* stream_dev, u64 dev_lo, const VideoMetadata& vm,
                     const std::vector<i64>& frames, DeviceHandle dev,
                     hipStream_t s, std::vector<u8*>& out_buffers) {
  size_t n = frames.size();
  out_buffers.assign(n, nullptr);
  if (n == 0) return;
  u64 total = 0;
  for (i64 f : frames) total += align_up(vm.sample_sizes[f], 16);
  u8* host = new_buffer(CPU_DEVICE, std::max<u64>(total, 1));
  std::vector<DeviceFrame> dframes;
  try {
    std::vector<ImageBlob> blobs(n);
    u64 pos = 0;
    for (size_t i = 0; i < n; ++i) {
      u64 sz = vm.sample_sizes[frames[i]];
      MJPEG_CHECK(hipMemcpyAsync(
          host + pos, stream_dev + (vm.sample_offsets[frames[i]] - dev_lo), sz,
          hipMemcpyDeviceToHost, s));
      blobs[i] = {host + pos, (size_t)sz};
      pos += align_up(sz, 16);
    }
    MJPEG_CHECK(hipStreamSynchronize(s));
    std::vector<JpegInfo> infos(n);
    for (size_t i = 0; i < n; ++i) {
      try {
        infos[i] = jpeg_parse(blobs[i].data, blobs[i].size);
        SCA_CHECK(infos[i].g.h == vm.height && infos[i].g.w == vm.width &&
                      infos[i].g.nc == vm.channels,
                  "its shape " + std::to_string(infos[i].g.h) + "x" +
                      std::to_string(infos[i].g.w) + "x" +
                      std::to_string(infos[i].g.nc) + " is not the item's");
      } catch (const ScannerError& err) {
        throw ScannerError("mjpeg: frame " + std::to_string(frames[i]) + ": " +
                           err.what());
      }
    }
    JpegGpuOptions opt;
    opt.serial_scan_on_device = true;
    // a corrupt scan is the CPU decoder's error; name the frame, one at a
    // time only when the batch as a whole fails
    try {
      jpeg_decode_gpu(blobs, infos, dev, s, dframes, nullptr, opt, nullptr);
    } catch (const ScannerError&) {
      for (size_t i = 0; i < n; ++i) {
        try {
          DecodedImage img = jpeg_decode_cpu(blobs[i].data, blobs[i].size);
        } catch (const ScannerError& err) {
          throw ScannerError("mjpeg: frame " + std::to_string(frames[i]) +
                             ": " + err.what());
        }
      }
      throw;
    }
  } catch (...) {
    delete_buffer(CPU_DEVICE, host);
    throw;
  }
  delete_buffer(CPU_DEVICE, host);
  for (size_t i = 0; i < n; ++i) out_buffers[i] = dframes[i].buffer;
}

// One part of a call: wanted frames whose samples lie within 4 GiB of the
// first one's start.
void decode_part(const u8* stream_dev, u64 dev_lo, const VideoMetadata& vm,
                 const std::vector<i64>& want, DeviceHandle dev,
                 const MjpegRefHeader& ref, hipStream_t s,
                 std::vector<Element>& out, MjpegGpuStats& stats) {
  const size_t n = want.size();
  if (n == 0) return;
  const JpegDecGeom& g = ref.info.g;
  const MjpegIndexParams& p = ref.params;
  // a sample 0 without a DRI segment, or (never from this project's own
  // ingest) of another shape than the item: nothing for the index to find
  const bool use_index = ref.device_ok && g.h == vm.height &&
                         g.w == vm.width && g.nc == vm.channels;
  std::vector<i64> fell_back;
  std::vector<size_t> fell_back_slot;
  std::vector<u8*> buffers(n, nullptr);

  if (!use_index) {
    for (size_t i = 0; i < n; ++i) {
      fell_back.push_back(want[i]);
      fell_back_slot.push_back(i);
    }
  } else {
    const u64 base = vm.sample_offsets[want[0]];
    const u8* span = stream_dev + (base - dev_lo);
    const u64 fbytes = align_up((u64)g.h * g.w * g.nc, 256);
    const u32 groups_per_file = (p.nseg + kJpegDecLanes - 1) / kJpegDecLanes;
    const u64 plane_bytes =
        g.nc == 3 ? align_up((u64)g.y_stride * g.y_rows, 256) +
                        2 * align_up((u64)g.c_stride * g.c_rows, 256)
                  : 0;
    // upload: status (entropy) | files | groups | sample offsets | sample
    // sizes | reference header; device only: index status | segments |
    // planes
    u64 status_off = 0;
    u64 files_off = align_up(status_off + 4 * n, 256);
    u64 groups_off = align_up(files_off + sizeof(JpegDecFile) * n, 256);
    u64 soff_off =
        align_up(groups_off + sizeof(JpegDecGroup) * groups_per_file * n, 256);
    u64 ssize_off = align_up(soff_off + 4 * n, 256);
    u64 hdr_off = align_up(ssize_off + 4 * n, 256);
    u64 upload = align_up(hdr_off + p.header_len, 256);
    u64 istatus_off = upload;
    // room for the entropy status behind the index status (see the gather)
    u64 segs_off = align_up(istatus_off + 8 * n, 256);
    u64 segs_bytes = sizeof(MjpegSeg) * (u64)p.nseg * n;
    u64 planes_off = align_up(segs_off + segs_bytes, 256);
    u64 ws_size = planes_off + plane_bytes * n;
    u64 back_off = upload;  // staging only: both status arrays
    u64 staging_size = back_off + align_up(8 * n, 256);

    u8* out_block = nullptr;
    u8* staging = nullptr;
    u8* ws = nullptr;
    i32 refs_left = (i32)n;
    try {
      out_block = new_block_buffer(dev, fbytes * n, (i32)n);
      staging = new_buffer(CPU_DEVICE, staging_size);
      ws = new_buffer(dev, ws_size);
      u32* status = reinterpret_cast<u32*>(staging + status_off);
      auto* files = reinterpret_cast<JpegDecFile*>(staging + files_off);
      auto* groups = reinterpret_cast<JpegDecGroup*>(staging + groups_off);
      u32* soff = reinterpret_cast<u32*>(staging + soff_off);
      u32* ssize = reinterpret_cast<u32*>(staging + ssize_off);
      std::memcpy(staging + hdr_off, ref.bytes.data(), p.header_len);
      u32 gi = 0;
      for (size_t i = 0; i < n; ++i) {
        i64 fr = want[i];
        buffers[i] = out_block + fbytes * i;
        status[i] = kJpegDecNoError;
        soff[i] = (u32)(vm.sample_offsets[fr] - base);
        ssize[i] = (u32)vm.sample_sizes[fr];
        JpegDecFile& f = files[i];
        std::memset(&f, 0, sizeof(f));
        f.g = g;
        f.status_index = (u32)i;
        f.out = buffers[i];
        if (g.nc == 3) {
          u64 ysz = align_up((u64)g.y_stride * g.y_rows, 256);
          u64 csz = align_up((u64)g.c_stride * g.c_rows, 256);
          f.plane_off[0] = plane_bytes * i;
          f.plane_off[1] = plane_bytes * i + ysz;
          f.plane_off[2] = plane_bytes * i + ysz + csz;
        }
        std::memcpy(f.q, ref.info.q, sizeof(f.q));
        std::memcpy(f.zz2nat, ref.info.zz2nat, sizeof(f.zz2nat));
        for (int c = 0; c < 3; ++c) {
          f.dc[c] = ref.info.dc[c];
          f.ac[c] = ref.info.ac[c];
        }
        for (u32 k = 0; k < p.nseg; k += kJpegDecLanes)
          groups[gi++] = {(u32)i, (u32)(i * p.nseg + k),
                          std::min(kJpegDecLanes, p.nseg - k), k};
      }
      MJPEG_CHECK(
          hipMemcpyAsync(ws, staging, upload, hipMemcpyHostToDevice, s));
      MJPEG_CHECK(hipMemsetAsync(ws + segs_off, 0, segs_bytes, s));
      MjpegIndexArgs ia{};
      ia.span = span;
      ia.sample_off = reinterpret_cast<const u32*>(ws + soff_off);
      ia.sample_size = reinterpret_cast<const u32*>(ws + ssize_off);
      ia.ref_header = ws + hdr_off;
      ia.segs = reinterpret_cast<MjpegSeg*>(ws + segs_off);
      ia.status = reinterpret_cast<u32*>(ws + istatus_off);
      ia.p = p;
      mjpeg_index_kernel<<<(u32)n, kIndexThreads, 0, s>>>(ia);
      MJPEG_CHECK(hipGetLastError());
      JpegDecArgs a{};
      a.files = reinterpret_cast<const JpegDecFile*>(ws + files_off);
      a.groups = reinterpret_cast<const JpegDecGroup*>(ws + groups_off);
      a.segs = reinterpret_cast<const JpegDecSeg*>(ws + segs_off);
      a.entropy = span;
      a.planes = ws + planes_off;
      a.status = reinterpret_cast<u32*>(ws + status_off);
      a.nfiles = (u32)n;
      jpeg_dec_enqueue(a, gi, jpeg_dec_colour_blocks(g), s);
      // the two status arrays come back as one copy: gather them first
      MJPEG_CHECK(hipMemcpyAsync(ws + istatus_off + 4 * n, ws + status_off,
                                 4 * n, hipMemcpyDeviceToDevice, s));
      MJPEG_CHECK(hipMemcpyAsync(staging + back_off, ws + istatus_off, 8 * n,
                                 hipMemcpyDeviceToHost, s));
      MJPEG_CHECK(hipStreamSynchronize(s));
      const u32* ist = reinterpret_cast<const u32*>(staging + back_off);
      const u32* est = ist + n;
      for (size_t i = 0; i < n; ++i) {
        if (ist[i] == kMjpegOk && est[i] == kJpegDecNoError) continue;
        fell_back.push_back(want[i]);
        fell_back_slot.push_back(i);
      }
    } catch (...) {
      (void)hipStreamSynchronize(s);
      if (staging) delete_buffer(CPU_DEVICE, staging);
      if (ws) delete_buffer(dev, ws);
      if (out_block)
        for (i32 k = 0; k < refs_left; ++k) delete_buffer(dev, out_block);
      throw;
    }
    delete_buffer(CPU_DEVICE, staging);
    delete_buffer(dev, ws);
  }

  // release the slots of the frames that fell back, then decode those
  auto release_all = [&]() {
    for (size_t i = 0; i < n; ++i)
      if (buffers[i]) delete_buffer(dev, buffers[i]);
  };
  for (size_t slot : fell_back_slot) {
    if (buffers[slot]) delete_buffer(dev, buffers[slot]);
    buffers[slot] = nullptr;
  }
  if (!fell_back.empty()) {
    std::vector<u8*> fb;
    try {
      decode_fallback(stream_dev, dev_lo, vm, fell_back, dev, s, fb);
    } catch (...) {
      release_all();
      throw;
    }
    for (size_t k = 0; k < fell_back.size(); ++k)
      buffers[fell_back_slot[k]] = fb[k];
  }
  stats.index_frames += (i64)(n - fell_back.size());
  stats.fallback_frames += (i64)fell_back.size();
  for (size_t i = 0; i < n; ++i)
    out.push_back(frame_element(vm, buffers[i], dev, want[i]));
}

}  // namespace

std::vector<Element> mjpeg_decode_gpu_dev(const u8* stream_dev, u64 dev_lo,
                                          const VideoMetadata& vm,
                                          const std::vector<i64>& want,
                                          DeviceHandle dev,
                                          const MjpegRefHeader& ref_header,
                                          MjpegGpuStats* stats) {
  SCA_CHECK(dev.is_gpu(), "mjpeg_decode_gpu_dev needs a GPU device");
  std::vector<Element> out;
  if (want.empty()) return out;
  MJPEG_CHECK(hipSetDevice(dev.id));
  hipStream_t s = (hipStream_t)per_thread_hip_stream();
  for (i64 f : want) {
    SCA_CHECK(f >= 0 && (size_t)f < vm.sample_offsets.size(),
              "mjpeg: frame " + std::to_string(f) + " is not in the item");
    SCA_CHECK(vm.sample_offsets[f] >= dev_lo,
              "mjpeg device stream range does not cover frame " +
                  std::to_string(f));
    SCA_CHECK(vm.sample_sizes[f] < (1ull << 31),
              "mjpeg: sample of 2 GiB or more");
  }
  MjpegGpuStats st;
  try {
    // segment offsets are u32 from the first sample of a part
    size_t i0 = 0;
    while (i0 < want.size()) {
      u64 base = vm.sample_offsets[want[i0]];
      size_t i1 = i0 + 1;
      while (i1 < want.size() &&
             vm.sample_offsets[want[i1]] >= base &&
             vm.sample_offsets[want[i1]] + vm.sample_sizes[want[i1]] - base <
                 (1ull << 32))
        ++i1;
      std::vector<i64> part(want.begin() + i0, want.begin() + i1);
      decode_part(stream_dev, dev_lo, vm, part, dev, ref_header, s, out, st);
      i0 = i1;
    }
  } catch (...) {
    for (Element& e : out)
      if (e.buffer) delete_buffer(dev, e.buffer);
    throw;
  }
  if (stats) *stats = st;
  return out;
}

std::vector<Element> mjpeg_decode_gpu(const u8* stream_host, size_t size,
                                      const VideoMetadata& vm,
                                      const std::vector<i64>& want,
                                      DeviceHandle dev,
                                      const MjpegRefHeader& ref_header,
                                      u64 stream_offset,
                                      MjpegGpuStats* stats) {
  SCA_CHECK(dev.is_gpu(), "mjpeg_decode_gpu needs a GPU device");
  if (want.empty()) return {};
  MJPEG_CHECK(hipSetDevice(dev.id));
  hipStream_t s = (hipStream_t)per_thread_hip_stream();
  u8* d = new_buffer(dev, std::max<size_t>(size, 1));
  std::vector<Element> out;
  try {
    MJPEG_CHECK(hipMemcpyAsync(d, stream_host, size, hipMemcpyHostToDevice, s));
    out = mjpeg_decode_gpu_dev(d, stream_offset, vm, want, dev, ref_header,
                               stats);
  } catch (...) {
    (void)hipStreamSynchronize(s);
    delete_buffer(dev, d);
    throw;
  }
  delete_buffer(dev, d);
  return out;
}

void mjpeg_index_gpu(const u8* stream, size_t stream_size,
                     const std::vector<u64>& offsets,
                     const std::vector<u64>& sizes, const u8* ref_header,
                     const MjpegIndexParams& p, std::vector<MjpegSeg>& segs,
                     std::vector<u32>& status, double* kernel_ms,
                     int repeats) {
  size_t n = offsets.size();
  SCA_CHECK(sizes.size() == n, "one size per offset");
  SCA_CHECK(p.nseg >= 1, "nseg must be at least 1");
  SCA_CHECK(stream_size < (1ull << 32), "mjpeg_index_gpu: 4 GiB or more");
  for (size_t i = 0; i < n; ++i)
    SCA_CHECK(offsets[i] <= stream_size && sizes[i] <= stream_size - offsets[i],
              "sample " + std::to_string(i) + " lies outside the stream");
  segs.assign(n * p.nseg, MjpegSeg{0, 0, 0, 0});
  status.assign(n, 0);
  if (n == 0) return;
  DeviceHandle dev{DeviceType::GPU, 0};
  MJPEG_CHECK(hipSetDevice(dev.id));
  hipStream_t s = (hipStream_t)per_thread_hip_stream();
  u64 soff_off = 0;
  u64 ssize_off = align_up(soff_off + 4 * n, 256);
  u64 hdr_off = align_up(ssize_off + 4 * n, 256);
  u64 status_off = align_up(hdr_off + p.header_len, 256);
  u64 segs_off = align_up(status_off + 4 * n, 256);
  u64 segs_bytes = sizeof(MjpegSeg) * segs.size();
  u64 ws_size = segs_off + segs_bytes;
  std::vector<u8> host(status_off, 0);
  for (size_t i = 0; i < n; ++i) {
    reinterpret_cast<u32*>(host.data() + soff_off)[i] = (u32)offsets[i];
    reinterpret_cast<u32*>(host.data() + ssize_off)[i] = (u32)sizes[i];
  }
  std::memcpy(host.data() + hdr_off, ref_header, p.header_len);
  u8* d_stream = nullptr;
  u8* ws = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  try {
    d_stream = new_buffer(dev, std::max<size_t>(stream_size, 1));
    ws = new_buffer(dev, ws_size);
    MJPEG_CHECK(hipMemcpyAsync(d_stream, stream, stream_size,
                               hipMemcpyHostToDevice, s));
    MJPEG_CHECK(hipMemcpyAsync(ws, host.data(), host.size(),
                               hipMemcpyHostToDevice, s));
    MjpegIndexArgs ia{};
    ia.span = d_stream;
    ia.sample_off = reinterpret_cast<const u32*>(ws + soff_off);
    ia.sample_size = reinterpret_cast<const u32*>(ws + ssize_off);
    ia.ref_header = ws + hdr_off;
    ia.segs = reinterpret_cast<MjpegSeg*>(ws + segs_off);
    ia.status = reinterpret_cast<u32*>(ws + status_off);
    ia.p = p;
    MJPEG_CHECK(hipEventCreate(&e0));
    MJPEG_CHECK(hipEventCreate(&e1));
    for (int r = 0; r < std::max(repeats, 1); ++r) {
      MJPEG_CHECK(hipMemsetAsync(ws + segs_off, 0, segs_bytes, s));
      if (r == std::max(repeats, 1) - 1) MJPEG_CHECK(hipEventRecord(e0, s));
      mjpeg_index_kernel<<<(u32)n, kIndexThreads, 0, s>>>(ia);
      MJPEG_CHECK(hipGetLastError());
    }
    MJPEG_CHECK(hipEventRecord(e1, s));
    MJPEG_CHECK(hipMemcpyAsync(status.data(), ws + status_off, 4 * n,
                               hipMemcpyDeviceToHost, s));
    MJPEG_CHECK(hipMemcpyAsync(segs.data(), ws + segs_off, segs_bytes,
                               hipMemcpyDeviceToHost, s));
    MJPEG_CHECK(hipStreamSynchronize(s));
    if (kernel_ms) {
      float ms = 0;
      MJPEG_CHECK(hipEventElapsedTime(&ms, e0, e1));
      *kernel_ms = ms;
    }
  } catch (...) {
    (void)hipStreamSynchronize(s);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_stream) delete_buffer(dev, d_stream);
    if (ws) delete_buffer(dev, ws);
    throw;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  delete_buffer(dev, d_stream);
  delete_buffer(dev, ws);
  // a failed sample's records are unspecified: report them as zero
  for (size_t i = 0; i < n; ++i)
    if (status[i] != kMjpegOk)
      std::fill(segs.begin() + i * p.nseg, segs.begin() + (i + 1) * p.nseg,
                MjpegSeg{0, 0, 0, 0});
}

}  // namespace sca
