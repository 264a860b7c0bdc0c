// GPU baseline JPEG decoder for gfx950: files in host memory become HWC u8
// frames in HBM, byte-identical to jpeg_decode_cpu, so an image source moves
// only compressed bytes over the host link. Formats and the shared integer
// arithmetic: csrc/ops/image_decode.h, csrc/ops/jpeg_decode_common.h.
//
// A JPEG scan is one serial bit stream except at restart markers, where the
// DC prediction and the bit alignment start afresh; so the unit of
// parallelism is the restart segment. PNG files are decoded by the CPU
// decoder and uploaded; so are files without a DRI segment, unless the
// caller asks for the self-synchronising decoder of
// kernels/jpeg_sync_decode.hip, which this file's host side feeds from the
// same staging buffer and whose rows share the colour kernel and the status
// words (records of both: kernels/jpeg_decode_dev.h). Progressive files go
// the same way to kernels/jpeg_progressive_decode.hip.
//
// Per batch (any mix of shapes, samplings and tables):
//   host     parse every file; pack status words, one descriptor per file
//            (geometry, quantisation and Huffman tables), one record per
//            workgroup, one record per segment and the entropy-coded bytes
//            into one pinned staging buffer -> one hipMemcpyAsync
//   entropy  one lane per restart segment, 64 segments of ONE file per
//            workgroup; the file's descriptor sits in LDS. A lane decodes a
//            block into its private 64 x int16 slot of an LDS tile (the
//            zig-zag scatter needs addressable storage), runs the IDCT on
//            it from registers and stores 8 rows of 8 bytes to the padded
//            component plane (grey: straight to the image). Coefficients
//            never reach HBM. The lanes share no data after the descriptor
//            load, so the loop has no barrier.
//   colour   one lane per 4 output pixels: chroma upsampling and
//            YCbCr -> RGB, 12 bytes stored as three dwords. Grey files skip
//            it.
//   status   one word per file, atomicMin of (segment << 4 | cause), read
//            back with one D2H and the only stream synchronise of the call.
//
// Safety on hostile entropy data: every read is bounded by the segment
// record (JpegBitReader), every coefficient write by the 64-entry slot
// (jpeg_decode_block), every plane write by the MCU count of the geometry,
// and the loops by MCU count x blocks per MCU x 64 symbols. A lane that
// meets an error records it and stops; the host discards the image.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>

#include "../csrc/memory.h"
#include "../csrc/ops/image_decode.h"
#include "../csrc/ops/kernel.h"
#include "jpeg_decode_dev.h"

namespace sca {

namespace {

#define JPEG_DEC_CHECK(expr)                                             \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess) {                                              \
      throw ScannerError(std::string("HIP error in jpeg decode: ") +     \
                         hipGetErrorString(_e));                         \
    }                                                                    \
  } while (0)

constexpr u32 kLanes = 64;        // restart segments per workgroup
constexpr u32 kSlotStride = 66;   // int16 per lane slot: 33 words, so lanes
                                  // reading the same coefficient hit
                                  // different banks
constexpr u32 kColourThreads = 256;
constexpr u32 kNoError = kJpegDecNoError;

__global__ void __launch_bounds__(kLanes) jpeg_entropy_idct_kernel(
    JpegDecArgs a) {
  __shared__ JpegDecFile f;
  __shared__ i16 tile[kLanes * kSlotStride];
  const JpegDecGroup grp = a.groups[blockIdx.x];
  u32 lane = threadIdx.x;
  {
    const u32* src = reinterpret_cast<const u32*>(a.files + grp.file);
    u32* dst = reinterpret_cast<u32*>(&f);
    for (u32 i = lane; i < sizeof(JpegDecFile) / 4; i += kLanes) dst[i] = src[i];
  }
  __syncthreads();
  if (lane >= grp.nseg) return;
  const JpegDecGeom& g = f.g;
  const JpegDecSeg seg = a.segs[grp.seg0 + lane];
  // the host builds the records from the same geometry; the clamp makes
  // every plane write below in range whatever they hold
  u32 m0 = min(seg.first_mcu, g.nmcu);
  u32 m1 = m0 + min(seg.mcu_count, g.nmcu - m0);

  JpegBitReader br;
  jpeg_bits_init(br, a.entropy, seg.begin, seg.end);
  i32 pred[3] = {0, 0, 0};
  i16* slot = tile + lane * kSlotStride;
  u32* slot32 = reinterpret_cast<u32*>(slot);

  for (u32 m = m0; m < m1; ++m) {
    for (u32 b = 0; b < g.blocks_per_mcu; ++b) {
      u32 comp, px, py;
      jpeg_block_pos(g, m, b, comp, px, py);
#pragma unroll
      for (u32 i = 0; i < 32; ++i) slot32[i] = 0;
      i32 p = comp == 0 ? pred[0] : comp == 1 ? pred[1] : pred[2];
      u32 st = jpeg_decode_block(br, f.dc[comp], f.ac[comp], f.zz2nat, p, slot);
      if (comp == 0) pred[0] = p; else if (comp == 1) pred[1] = p; else pred[2] = p;
      if (st != kJpegBlockOk) {
        atomicMin(&a.status[f.status_index], (grp.file_seg0 + lane) << 4 | st);
        return;
      }
      i32 deq[64];
      const u16* q = f.q[comp];
#pragma unroll
      for (int k = 0; k < 64; ++k) deq[k] = jpeg_dequant(slot[k], q[k]);
      u8 pix[64];
      jpeg_idct_block(deq, pix);
      if (g.nc == 1) {
        jpeg_store_block_grey(pix, f.out, (u32)g.h, (u32)g.w, px, py);
      } else {
        u32 stride = comp == 0 ? g.y_stride : g.c_stride;
        jpeg_store_block_plane(
            pix, a.planes + f.plane_off[comp] + (u64)py * stride + px, stride);
      }
    }
  }
}

// grid (pixel groups of the largest file, files); a lane owns pixels
// [4t, 4t + 4) of the flattened image, i.e. bytes [12t, 12t + 12)
__global__ void __launch_bounds__(kColourThreads) jpeg_colour_kernel(
    JpegDecArgs a) {
  const JpegDecFile& f = a.files[blockIdx.y];
  const JpegDecGeom g = f.g;
  if (g.nc != 3) return;
  u64 npix = (u64)g.h * g.w;
  u64 p0 = ((u64)blockIdx.x * kColourThreads + threadIdx.x) * 4;
  if (p0 >= npix) return;
  const u8* yp = a.planes + f.plane_off[0];
  const u8* cbp = a.planes + f.plane_off[1];
  const u8* crp = a.planes + f.plane_off[2];
  u8 rgb[12];
  u32 n = (u32)min((u64)4, npix - p0);
  u32 y = (u32)(p0 / (u32)g.w), x = (u32)(p0 % (u32)g.w);
#pragma unroll
  for (u32 i = 0; i < 4; ++i) {
    if (i < n) {
      jpeg_pixel_rgb(g, yp, cbp, crp, x, y, rgb + 3 * i);
      if (++x == (u32)g.w) {
        x = 0;
        ++y;
      }
    } else {
      rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = 0;
    }
  }
  u8* dst = f.out + p0 * 3;  // out is 256-byte aligned, p0 * 3 = 12 t
  if (n == 4) {
    u32* d4 = reinterpret_cast<u32*>(dst);
#pragma unroll
    for (u32 k = 0; k < 3; ++k)
      d4[k] = rgb[4 * k] | rgb[4 * k + 1] << 8 | rgb[4 * k + 2] << 16 |
              (u32)rgb[4 * k + 3] << 24;
  } else {
    for (u32 k = 0; k < 3 * n; ++k) dst[k] = rgb[k];
  }
}

u64 align_up(u64 x, u64 a) { return (x + a - 1) / a * a; }

thread_local double t_last_sync = 0;

}  // namespace

double jpeg_decode_gpu_last_sync_seconds() { return t_last_sync; }

static_assert(kJpegDecLanes == kLanes, "one lane per restart segment");

u32 jpeg_dec_colour_blocks(const JpegDecGeom& g) {
  if (g.nc != 3) return 0;
  u64 groups4 = ((u64)g.h * g.w + 3) / 4;
  return (u32)((groups4 + kColourThreads - 1) / kColourThreads);
}

void jpeg_dec_enqueue(const JpegDecArgs& a, u32 ngroups, u32 colour_blocks,
                      hipStream_t stream) {
  if (ngroups) {
    jpeg_entropy_idct_kernel<<<ngroups, kLanes, 0, stream>>>(a);
    JPEG_DEC_CHECK(hipGetLastError());
  }
  if (colour_blocks && a.nfiles) {
    jpeg_colour_kernel<<<dim3(colour_blocks, a.nfiles), kColourThreads, 0,
                         stream>>>(a);
    JPEG_DEC_CHECK(hipGetLastError());
  }
}

void jpeg_decode_gpu(const std::vector<ImageBlob>& blobs,
                     const std::vector<JpegInfo>& infos, DeviceHandle dev,
                     void* stream, std::vector<DeviceFrame>& out_frames,
                     i64* host_rows, JpegGpuOptions opt,
                     JpegGpuStats* stats) {
  SCA_CHECK(dev.is_gpu(), "jpeg_decode_gpu needs a GPU device");
  SCA_CHECK(infos.size() == blobs.size(), "one JpegInfo per blob");
  size_t n = blobs.size();
  out_frames.assign(n, DeviceFrame{});
  if (host_rows) *host_rows = 0;
  if (stats) *stats = JpegGpuStats{};
  u32 chunk_bytes = opt.chunk_bytes ? opt.chunk_bytes : kJpegSyncChunkBytes;
  SCA_CHECK(jpeg_sync_valid_chunk_bytes(chunk_bytes),
            "chunk_bytes must be a power of two >= 4, got " +
                std::to_string(chunk_bytes));
  if (n == 0) return;
  JPEG_DEC_CHECK(hipSetDevice(dev.id));
  hipStream_t s = (hipStream_t)stream;

  // ---- classify, decode the host rows, lay out the outputs ----
  // 0 null, 1 device by restart segments, 2 host, 3 device by chunks,
  // 4 device, progressive
  std::vector<int> kind(n, 0);
  auto on_device = [&](size_t i) {
    return kind[i] == 1 || kind[i] == 3 || kind[i] == 4;
  };
  std::vector<DecodedImage> host_img(n);
  std::vector<u64> out_off(n, 0);
  u64 out_total = 0, host_pix_total = 0;
  i32 live = 0;
  size_t ndev = 0, nsync = 0, nprog = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!blobs[i].data) continue;
    DeviceFrame& fr = out_frames[i];
    bool jpeg = is_jpeg(blobs[i].data, blobs[i].size);
    bool prog = jpeg && infos[i].progressive;
    bool prog_dev = false;
    if (prog) {
      SCA_CHECK(opt.progressive,
                "ImageDecoder: row " + std::to_string(i) + " of the batch: "
                "progressive JPEG (SOF2) is not supported");
      // a scan without a restart interval is one lane of the scan kernel:
      // on the device only where the caller asked for serial scans there
      bool all_dri = true;
      for (const JpegScan& sc : infos[i].scans)
        all_dri = all_dri && sc.restart_interval != 0;
      prog_dev = (all_dri || opt.serial_scan_on_device) &&
                 !infos[i].scans.empty() &&
                 infos[i].scans.size() <= kJpegProgMaxDeviceScans;
    }
    bool by_chunks =
        jpeg && !prog && opt.serial_scan_on_device &&
        infos[i].restart_interval == 0 &&
        infos[i].segments.size() == 1 &&
        infos[i].segments[0].end - infos[i].segments[0].begin <
            kJpegSyncMaxScanBytes;
    if ((jpeg && !prog && infos[i].restart_interval != 0) || by_chunks ||
        prog_dev) {
      kind[i] = prog_dev ? 4 : by_chunks ? 3 : 1;
      nsync += by_chunks;
      nprog += prog_dev;
      ++ndev;
      fr.h = infos[i].g.h;
      fr.w = infos[i].g.w;
      fr.c = infos[i].g.nc;
    } else {
      kind[i] = 2;
      try {
        if (is_jpeg(blobs[i].data, blobs[i].size)) {
          host_img[i].h = infos[i].g.h;
          host_img[i].w = infos[i].g.w;
          host_img[i].c = infos[i].g.nc;
          host_img[i].pixels.resize((size_t)infos[i].g.h * infos[i].g.w *
                                    infos[i].g.nc);
          jpeg_decode_cpu_into(blobs[i].data, infos[i],
                               host_img[i].pixels.data());
        } else {
          host_img[i] = image_decode_cpu(blobs[i].data, blobs[i].size);
        }
      } catch (const ScannerError& err) {
        throw ScannerError("ImageDecoder: row " + std::to_string(i) +
                           " of the batch: " + err.what());
      }
      fr.h = host_img[i].h;
      fr.w = host_img[i].w;
      fr.c = host_img[i].c;
      host_pix_total += align_up(host_img[i].pixels.size(), 256);
      if (host_rows) ++*host_rows;
    }
    out_off[i] = out_total;
    out_total += align_up((u64)fr.h * fr.w * fr.c, 256);
    ++live;
  }
  if (live == 0) return;

  // ---- staging layout: status | files | groups | segments | chunked
  // files | their groups | entropy | (host only) pixels of the host rows ----
  size_t ngroups = 0, nsegs = 0, nsgroups = 0, nchunks = 0;
  size_t npdescs = 0, npgroups = 0, npsegs = 0, nlaunch = 0;
  u64 entropy_total = 0, planes_total = 0, coef_total = 0, pcoef_total = 0;
  // [first, last) entropy-coded byte of a device row
  auto entropy_range = [&](size_t i, u32& base, u32& len) {
    const JpegInfo& in = infos[i];
    const auto& first = in.progressive ? in.scans.front().segments : in.segments;
    const auto& last = in.progressive ? in.scans.back().segments : in.segments;
    base = first.front().begin;
    len = last.back().end - base;
  };
  for (size_t i = 0; i < n; ++i) {
    if (!on_device(i)) continue;
    const JpegInfo& in = infos[i];
    if (kind[i] == 4) {
      npdescs += in.scans.size();
      nlaunch = std::max(nlaunch, in.scans.size());
      for (const JpegScan& sc : in.scans) {
        npsegs += sc.segments.size();
        npgroups += (sc.segments.size() + kLanes - 1) / kLanes;
      }
      pcoef_total += (u64)in.g.nmcu * in.g.blocks_per_mcu * 64;
    } else if (kind[i] == 3) {
      u32 nc = jpeg_sync_chunk_count(
          in.segments[0].end - in.segments[0].begin, chunk_bytes);
      nchunks += nc;
      nsgroups += (nc + kJpegSyncGroupChunks - 1) / kJpegSyncGroupChunks;
      coef_total += (u64)in.g.nmcu * in.g.blocks_per_mcu * 64;
    } else {
      nsegs += in.segments.size();
      ngroups += (in.segments.size() + kLanes - 1) / kLanes;
    }
    u32 ebase, elen;
    entropy_range(i, ebase, elen);
    entropy_total += align_up(elen, 16);
    if (in.g.nc == 3)
      planes_total += align_up((u64)in.g.y_stride * in.g.y_rows, 256) +
                      2 * align_up((u64)in.g.c_stride * in.g.c_rows, 256);
  }
  u64 status_off = 0;
  // the second ndev words: the failing scan of a progressive row
  u64 files_off = align_up(status_off + 8 * ndev, 256);
  u64 groups_off = align_up(files_off + sizeof(JpegDecFile) * ndev, 256);
  u64 segs_off = align_up(groups_off + sizeof(JpegDecGroup) * ngroups, 256);
  u64 sfiles_off = align_up(segs_off + sizeof(JpegDecSeg) * nsegs, 256);
  u64 sgroups_off = align_up(sfiles_off + sizeof(JpegSyncFile) * nsync, 256);
  u64 pdescs_off =
      align_up(sgroups_off + sizeof(JpegSyncGroup) * nsgroups, 256);
  u64 pgroups_off =
      align_up(pdescs_off + sizeof(JpegProgScanDesc) * npdescs, 256);
  u64 psegs_off = align_up(pgroups_off + sizeof(JpegProgGroup) * npgroups, 256);
  u64 pfiles_off = align_up(psegs_off + sizeof(JpegDecSeg) * npsegs, 256);
  u64 entropy_off = align_up(pfiles_off + sizeof(JpegProgFile) * nprog, 256);
  u64 upload = align_up(entropy_off + entropy_total, 256);
  // device only, behind the upload: planes | chunk records | first blocks |
  // group exits | coefficients
  u64 chunks_off = align_up(upload + planes_total, 256);
  u64 first_off = align_up(chunks_off + sizeof(JpegSyncChunk) * nchunks, 256);
  u64 gexit_off = align_up(first_off + 4 * nchunks, 256);
  u64 coef_off =
      align_up(gexit_off + 2 * sizeof(JpegSyncState) * nsgroups, 256);
  u64 pcoef_off = align_up(coef_off + coef_total * sizeof(i16), 256);
  u64 ws_size = pcoef_off + pcoef_total * sizeof(i16);
  u64 host_pix_off = upload;
  u64 status_back_off = host_pix_off + host_pix_total;
  u64 staging_size = status_back_off + align_up(8 * ndev, 256) + 256;
  SCA_CHECK(upload < (1ull << 32), "jpeg decode: batch of 4 GiB or more");

  u8* out_block = nullptr;
  u8* staging = nullptr;
  u8* fallback = nullptr;  // pinned: pixels of the rows that fell back
  u8* ws = nullptr;  // device: the uploaded part, then the workspaces
  auto release = [&](bool outputs_too) {
    if (staging) delete_buffer(CPU_DEVICE, staging);
    if (fallback) delete_buffer(CPU_DEVICE, fallback);
    if (ws) delete_buffer(dev, ws);
    staging = fallback = ws = nullptr;
    if (outputs_too && out_block) {
      for (i32 k = 0; k < live; ++k) delete_buffer(dev, out_block);
      out_block = nullptr;
      out_frames.assign(n, DeviceFrame{});
    }
  };
  try {
    out_block = new_block_buffer(dev, out_total, live);
    staging = new_buffer(CPU_DEVICE, staging_size);
    if (ndev) ws = new_buffer(dev, ws_size);
    for (size_t i = 0; i < n; ++i)
      if (kind[i]) out_frames[i].buffer = out_block + out_off[i];

    u32 max_colour_blocks = 0;
    if (ndev) {
      u32* status = reinterpret_cast<u32*>(staging + status_off);
      auto* files = reinterpret_cast<JpegDecFile*>(staging + files_off);
      auto* groups = reinterpret_cast<JpegDecGroup*>(staging + groups_off);
      auto* segs = reinterpret_cast<JpegDecSeg*>(staging + segs_off);
      u8* entropy = staging + entropy_off;
      auto* sfiles = reinterpret_cast<JpegSyncFile*>(staging + sfiles_off);
      auto* sgroups = reinterpret_cast<JpegSyncGroup*>(staging + sgroups_off);
      auto* pdescs = reinterpret_cast<JpegProgScanDesc*>(staging + pdescs_off);
      auto* pgroups = reinterpret_cast<JpegProgGroup*>(staging + pgroups_off);
      auto* psegs = reinterpret_cast<JpegDecSeg*>(staging + psegs_off);
      auto* pfiles = reinterpret_cast<JpegProgFile*>(staging + pfiles_off);
      u32 fi = 0, gi = 0, si = 0, sfi = 0, sgi = 0, ci = 0;
      u32 pdi = 0, psi = 0, pfi = 0;
      u32 max_rounds = 0, max_nblk = 0, max_pnblk = 0;
      u64 epos = 0, ppos = 0, cpos = 0, pcpos = 0;
      // progressive group records are ordered by scan index, then file:
      // one launch per scan index over a contiguous range
      struct PendingGroup {
        u32 scan;
        JpegProgGroup g;
      };
      std::vector<PendingGroup> pending;
      for (size_t i = 0; i < n; ++i) {
        if (!on_device(i)) continue;
        const JpegInfo& in = infos[i];
        status[fi] = kNoError;
        status[ndev + fi] = kNoError;
        JpegDecFile& f = files[fi];
        std::memset(&f, 0, sizeof(f));
        f.g = in.g;
        f.status_index = fi;
        f.out = out_frames[i].buffer;
        if (in.g.nc == 3) {
          u64 ysz = align_up((u64)in.g.y_stride * in.g.y_rows, 256);
          u64 csz = align_up((u64)in.g.c_stride * in.g.c_rows, 256);
          f.plane_off[0] = ppos;
          f.plane_off[1] = ppos + ysz;
          f.plane_off[2] = ppos + ysz + csz;
          ppos += ysz + 2 * csz;
          u64 groups4 = ((u64)in.g.h * in.g.w + 3) / 4;
          max_colour_blocks = std::max<u32>(
              max_colour_blocks,
              (u32)((groups4 + kColourThreads - 1) / kColourThreads));
        }
        std::memcpy(f.q, in.q, sizeof(f.q));
        std::memcpy(f.zz2nat, in.zz2nat, sizeof(f.zz2nat));
        for (int c = 0; c < 3; ++c) {
          f.dc[c] = in.dc[c];
          f.ac[c] = in.ac[c];
        }
        u32 base, len;
        entropy_range(i, base, len);
        std::memcpy(entropy + epos, blobs[i].data + base, len);
        if (kind[i] == 4) {
          JpegProgFile& pf = pfiles[pfi++];
          pf.file = fi;
          pf.nblk = in.g.nmcu * in.g.blocks_per_mcu;
          pf.coef_off = pcpos;
          max_pnblk = std::max(max_pnblk, pf.nblk);
          for (size_t k = 0; k < in.scans.size(); ++k) {
            const JpegScan& sc = in.scans[k];
            JpegProgScanDesc& d = pdescs[pdi];
            std::memset(&d, 0, sizeof(d));
            d.g = in.g;
            d.file = fi;
            d.ncomp = sc.ncomp;
            d.comp = sc.comp[0];
            d.ss = sc.ss;
            d.se = sc.se;
            d.ah = sc.ah;
            d.al = sc.al;
            d.coef_off = pcpos;
            std::memcpy(d.zz2nat, in.zz2nat, sizeof(d.zz2nat));
            if (sc.ss == 0) {
              for (int c = 0; c < 3; ++c) d.tab[c] = sc.dc[c];
            } else {
              d.tab[0] = sc.ac[sc.comp[0]];
            }
            u32 nseg = (u32)sc.segments.size();
            for (u32 j = 0; j < nseg; j += kLanes)
              pending.push_back(
                  {(u32)k, {pdi, psi + j, std::min(kLanes, nseg - j), j}});
            for (const JpegSegment& sg : sc.segments)
              psegs[psi++] = {(u32)(epos + sg.begin - base),
                              (u32)(epos + sg.end - base), sg.first_mcu,
                              sg.mcu_count};
            ++pdi;
          }
          pcpos += (u64)pf.nblk * 64;
        } else if (kind[i] == 3) {
          JpegSyncFile& sf = sfiles[sfi];
          std::memset(&sf, 0, sizeof(sf));
          sf.file = fi;
          sf.begin = (u32)epos;
          sf.end = (u32)(epos + len);
          sf.chunk_bytes = chunk_bytes;
          sf.nchunks = jpeg_sync_chunk_count(len, chunk_bytes);
          sf.chunk0 = ci;
          sf.ngroups =
              (sf.nchunks + kJpegSyncGroupChunks - 1) / kJpegSyncGroupChunks;
          sf.rounds = jpeg_sync_rounds(sf.ngroups);
          sf.nblk = in.g.nmcu * in.g.blocks_per_mcu;
          sf.coef_off = cpos;
          for (u32 k = 0; k < sf.ngroups; ++k) sgroups[sgi++] = {sfi, k};
          ci += sf.nchunks;
          cpos += (u64)sf.nblk * 64;
          max_rounds = std::max(max_rounds, sf.rounds);
          max_nblk = std::max(max_nblk, sf.nblk);
          ++sfi;
        } else {
          u32 nseg = (u32)in.segments.size();
          for (u32 k = 0; k < nseg; k += kLanes)
            groups[gi++] = {fi, si + k, std::min(kLanes, nseg - k), k};
          for (const JpegSegment& sg : in.segments)
            segs[si++] = {(u32)(epos + sg.begin - base),
                          (u32)(epos + sg.end - base), sg.first_mcu,
                          sg.mcu_count};
        }
        epos += align_up(len, 16);
        ++fi;
      }
      std::vector<u32> launch_group0(nlaunch + 1, 0);
      if (nprog) {
        std::stable_sort(pending.begin(), pending.end(),
                         [](const PendingGroup& x, const PendingGroup& y) {
                           return x.scan < y.scan;
                         });
        for (size_t j = 0; j < pending.size(); ++j) {
          pgroups[j] = pending[j].g;
          ++launch_group0[pending[j].scan + 1];
        }
        for (size_t k = 0; k < nlaunch; ++k)
          launch_group0[k + 1] += launch_group0[k];
      }
      JPEG_DEC_CHECK(
          hipMemcpyAsync(ws, staging, upload, hipMemcpyHostToDevice, s));
      JpegDecArgs a{};
      a.status = reinterpret_cast<u32*>(ws + status_off);
      a.files = reinterpret_cast<const JpegDecFile*>(ws + files_off);
      a.groups = reinterpret_cast<const JpegDecGroup*>(ws + groups_off);
      a.segs = reinterpret_cast<const JpegDecSeg*>(ws + segs_off);
      a.entropy = ws + entropy_off;
      a.planes = ws + upload;
      a.nfiles = (u32)ndev;
      if (ngroups) {
        jpeg_entropy_idct_kernel<<<(u32)ngroups, kLanes, 0, s>>>(a);
        JPEG_DEC_CHECK(hipGetLastError());
      }
      if (nsync) {
        JpegSyncArgs sa{};
        sa.dec = a;
        sa.sfiles = reinterpret_cast<const JpegSyncFile*>(ws + sfiles_off);
        sa.sgroups = reinterpret_cast<const JpegSyncGroup*>(ws + sgroups_off);
        sa.chunks = reinterpret_cast<JpegSyncChunk*>(ws + chunks_off);
        sa.first_block = reinterpret_cast<u32*>(ws + first_off);
        sa.gexit = reinterpret_cast<JpegSyncState*>(ws + gexit_off);
        sa.coef = reinterpret_cast<i16*>(ws + coef_off);
        sa.coef_count = coef_total;
        sa.nsfiles = (u32)nsync;
        sa.nsgroups = (u32)nsgroups;
        sa.max_rounds = max_rounds;
        sa.max_nblk = max_nblk;
        jpeg_sync_enqueue(sa, s);
      }
      if (nprog) {
        JpegProgArgs pa{};
        pa.dec = a;
        pa.descs = reinterpret_cast<const JpegProgScanDesc*>(ws + pdescs_off);
        pa.groups = reinterpret_cast<const JpegProgGroup*>(ws + pgroups_off);
        pa.segs = reinterpret_cast<const JpegDecSeg*>(ws + psegs_off);
        pa.pfiles = reinterpret_cast<const JpegProgFile*>(ws + pfiles_off);
        pa.fail_scan = a.status + ndev;
        pa.coef = reinterpret_cast<i16*>(ws + pcoef_off);
        pa.coef_count = pcoef_total;
        pa.npfiles = (u32)nprog;
        pa.max_nblk = max_pnblk;
        jpeg_prog_enqueue(pa, launch_group0.data(), (u32)nlaunch, s);
      }
      if (max_colour_blocks) {
        jpeg_colour_kernel<<<dim3(max_colour_blocks, (u32)ndev),
                             kColourThreads, 0, s>>>(a);
        JPEG_DEC_CHECK(hipGetLastError());
      }
      JPEG_DEC_CHECK(hipMemcpyAsync(staging + status_back_off,
                                    ws + status_off, 8 * ndev,
                                    hipMemcpyDeviceToHost, s));
    }
    // host rows: pixels through the pinned staging
    u64 hpos = host_pix_off;
    for (size_t i = 0; i < n; ++i) {
      if (kind[i] != 2) continue;
      size_t sz = host_img[i].pixels.size();
      std::memcpy(staging + hpos, host_img[i].pixels.data(), sz);
      JPEG_DEC_CHECK(hipMemcpyAsync(out_frames[i].buffer, staging + hpos, sz,
                                    hipMemcpyHostToDevice, s));
      hpos += align_up(sz, 256);
    }
    auto sync0 = std::chrono::steady_clock::now();
    JPEG_DEC_CHECK(hipStreamSynchronize(s));  // the only one
    t_last_sync = std::chrono::duration<double>(
                      std::chrono::steady_clock::now() - sync0)
                      .count();
    if (ndev) {
      const u32* back =
          reinterpret_cast<const u32*>(staging + status_back_off);
      u32 fi = 0;
      std::vector<size_t> fell_back;
      u64 fallback_total = 0;
      for (size_t i = 0; i < n; ++i) {
        if (!on_device(i)) continue;
        u32 st = back[fi];
        u32 failed_scan = back[ndev + fi];
        ++fi;
        if (st == kNoError) continue;
        if (kind[i] == 4)
          throw ScannerError("ImageDecoder: row " + std::to_string(i) +
                             " of the batch: check failed: " +
                             jpeg_entropy_error(st & 15u, st >> 4,
                                                failed_scan));
        if (kind[i] == 1)
          throw ScannerError("ImageDecoder: row " + std::to_string(i) +
                             " of the batch: check failed: " +
                             jpeg_entropy_error(st & 15u, st >> 4));
        // a chunked row that failed verification: the CPU decoder's pixels,
        // or its error
        DecodedImage& img = host_img[i];
        img.pixels.resize((size_t)infos[i].g.h * infos[i].g.w * infos[i].g.nc);
        try {
          jpeg_decode_cpu_into(blobs[i].data, infos[i], img.pixels.data());
        } catch (const ScannerError& err) {
          throw ScannerError("ImageDecoder: row " + std::to_string(i) +
                             " of the batch: " + err.what());
        }
        fell_back.push_back(i);
        fallback_total += align_up(img.pixels.size(), 256);
      }
      if (!fell_back.empty()) {
        fallback = new_buffer(CPU_DEVICE, fallback_total);
        u64 fpos = 0;
        for (size_t i : fell_back) {
          size_t sz = host_img[i].pixels.size();
          std::memcpy(fallback + fpos, host_img[i].pixels.data(), sz);
          JPEG_DEC_CHECK(hipMemcpyAsync(out_frames[i].buffer, fallback + fpos,
                                        sz, hipMemcpyHostToDevice, s));
          fpos += align_up(sz, 256);
        }
        JPEG_DEC_CHECK(hipStreamSynchronize(s));
        if (host_rows) *host_rows += (i64)fell_back.size();
      }
      if (stats) {
        stats->fallback_rows = (i64)fell_back.size();
        stats->sync_rows = (i64)nsync - stats->fallback_rows;
        stats->progressive_rows = (i64)nprog;
      }
    }
  } catch (...) {
    (void)hipStreamSynchronize(s);
    release(true);
    throw;
  }
  release(false);
}

namespace {

// ImageDecoder on the GPU. Registered with host_inputs: the files stay where
// the executor found them; this kernel parses them on the host and uploads
// the entropy-coded bytes of the whole batch at once.
class ImageDecoderKernelGPU : public BatchedKernel {
 public:
  explicit ImageDecoderKernelGPU(const KernelConfig& cfg)
      : BatchedKernel(cfg) {
    opt_.serial_scan_on_device = image_decoder_serial_scan_on_device(cfg.args);
    opt_.progressive = image_decoder_progressive(cfg.args);
    parse_.allow_progressive = opt_.progressive;
  }

  void execute_batch(const BatchedElements& in, BatchedElements& out) override {
    const ElementVector& col = in[0];
    size_t n = col.size();
    out[0].resize(n);
    std::vector<ImageBlob> blobs(n, ImageBlob{nullptr, 0});
    std::vector<JpegInfo> infos(n);
    std::vector<u8*> host_copies;
    std::vector<DeviceFrame> frames;
    i64 host_rows = 0, live = 0;
    JpegGpuStats stats;
    try {
      for (size_t i = 0; i < n; ++i) {
        const Element& b = col[i];
        if (b.is_null) continue;
        SCA_CHECK(!b.is_frame, "ImageDecoder needs a bytes input");
        const u8* p = b.buffer;
        if (b.device.is_gpu()) {
          // e.g. straight from a GPU ImageEncoder: compressed bytes are
          // small, bring them to the host
          u8* h = new_buffer(CPU_DEVICE, std::max<size_t>(b.size, 1));
          host_copies.push_back(h);
          memcpy_buffer(h, CPU_DEVICE, b.buffer, b.device, b.size);
          p = h;
        }
        blobs[i] = {p, b.size};
        ++live;
        if (is_jpeg(p, b.size)) {
          try {
            infos[i] = jpeg_parse(p, b.size, parse_);
          } catch (const ScannerError& err) {
            throw ScannerError("ImageDecoder: row " + std::to_string(i) +
                               " of the batch: " + err.what());
          }
        }
      }
      void* stream =
          config_.hip_stream ? config_.hip_stream : per_thread_hip_stream();
      jpeg_decode_gpu(blobs, infos, config_.device, stream, frames,
                      &host_rows, opt_, &stats);
    } catch (...) {
      for (u8* h : host_copies) delete_buffer(CPU_DEVICE, h);
      throw;
    }
    for (u8* h : host_copies) delete_buffer(CPU_DEVICE, h);
    for (size_t i = 0; i < n; ++i) {
      Element& e = out[0][i];
      if (col[i].is_null) {
        e.is_null = true;
        continue;
      }
      e.is_frame = true;
      e.frame_info.shape[0] = frames[i].h;
      e.frame_info.shape[1] = frames[i].w;
      e.frame_info.shape[2] = frames[i].c;
      e.frame_info.type = FrameType::U8;
      e.size = (size_t)frames[i].h * frames[i].w * frames[i].c;
      e.buffer = frames[i].buffer;
      e.device = config_.device;
    }
    if (config_.profiler) {
      config_.profiler->increment("jpeg_gpu_decode_frames", live - host_rows);
      config_.profiler->increment("image_decode_host_rows", host_rows);
      if (opt_.progressive)
        config_.profiler->increment("jpeg_gpu_progressive_frames",
                                    stats.progressive_rows);
      if (opt_.serial_scan_on_device) {
        config_.profiler->increment("jpeg_gpu_sync_frames", stats.sync_rows);
        config_.profiler->increment("jpeg_sync_fallback_rows",
                                    stats.fallback_rows);
      }
    }
  }

 private:
  JpegGpuOptions opt_;
  JpegParseOptions parse_;
};

}  // namespace

void register_image_decoder_gpu() {
  static bool done = false;
  if (done) return;
  done = true;
  KernelFactory f;
  f.op_name = "ImageDecoder";
  f.device_type = DeviceType::GPU;
  f.preferred_batch = 8;
  f.host_inputs = true;
  f.make = [](const KernelConfig& c) -> std::unique_ptr<BaseKernel> {
    return std::make_unique<ImageDecoderKernelGPU>(c);
  };
  kernel_registry().add(f);
}

}  // namespace sca
