// GPU decode of JPEG scans without restart markers for gfx950: the
// self-synchronising parallel Huffman decoder of csrc/ops/jpeg_sync_common.h
// (which says why it is sound), one lane per chunk of the scan. The host
// side of a batch, the colour kernel and the status words are those of
// kernels/jpeg_decode.hip; csrc/ops/jpeg_sync_cpu.cpp runs the same
// functions in the same order on the CPU.
//
// Per batch, for the files that have no DRI segment:
//   sync     round 0: one lane per chunk, 256 chunks of ONE file per
//            workgroup, the file's descriptor in LDS. Every lane decodes its
//            chunk from the guess (chunk start, 0, 0), then again from its
//            left neighbour's exit (through LDS) until no exit of the
//            workgroup changed. Rounds 1..R, one launch each: the first
//            chunk of a workgroup takes the last exit the workgroup before
//            it had after the round before (double-buffered, so a round
//            reads nothing that it writes) and the same loop repairs
//            forward. A lane whose entry did not change decodes nothing, so
//            a round that has nothing to repair only reads its records.
//            R = min(groups - 1, kJpegSyncMaxRounds) per file, fixed: the
//            host polls nothing and the call keeps its single synchronise.
//   scan     one workgroup per file: exclusive sum of the blocks per chunk
//            -> first block of every chunk; the total must be the file's.
//   write    one lane per chunk: the writing walk from the left neighbour's
//            final exit stores int16 coefficients (DC differences) to HBM
//            and must end exactly at the chunk's recorded exit.
//   dc       one workgroup per file: per-component prefix sum of the DC
//            differences in 64-bit; a value outside int16 fails the row.
//   idct     one lane per block: dequantise, IDCT, the stores of the restart
//            kernel.
// A row that fails any check has its status word set; the host decodes it
// with the CPU decoder after the synchronise.
//
// Bounds: every read of the scan lies in [begin, end) of the file's record,
// every coefficient write in block [0, nblk) x 64 of the file's slice, every
// plane write inside the MCU count of the geometry; the walks loop at most
// once per bit of their chunk, the in-group loop at most 256 times.
#include <hip/hip_runtime.h>

#include "jpeg_decode_dev.h"

namespace sca {

namespace {

constexpr u32 kLanes = kJpegSyncGroupChunks;
constexpr u32 kIdctLanes = 64;

__device__ inline void load_file(JpegDecFile& f, const JpegDecFile* src_file,
                                 u32 lane) {
  const u32* src = reinterpret_cast<const u32*>(src_file);
  u32* dst = reinterpret_cast<u32*>(&f);
  for (u32 i = lane; i < sizeof(JpegDecFile) / 4; i += kLanes) dst[i] = src[i];
}

__device__ inline JpegSyncScan make_scan(const JpegSyncArgs& a,
                                         const JpegSyncFile& sf,
                                         const JpegDecFile& f) {
  JpegSyncScan sc;
  sc.p = a.dec.entropy;
  sc.begin = sf.begin;
  sc.end = sf.end;
  sc.blocks_per_mcu = f.g.blocks_per_mcu;
  sc.ny = f.g.nc == 1 ? 1u : f.g.hs * f.g.vs;
  sc.dc = f.dc;
  sc.ac = f.ac;
  return sc;
}

__global__ void __launch_bounds__(kLanes) jpeg_sync_kernel(JpegSyncArgs a,
                                                           u32 round) {
  __shared__ JpegDecFile f;
  __shared__ JpegSyncState exits[kLanes];
  const JpegSyncGroup grp = a.sgroups[blockIdx.x];
  const JpegSyncFile sf = a.sfiles[grp.sfile];
  if (round > sf.rounds) return;
  u32 lane = threadIdx.x;
  load_file(f, a.dec.files + sf.file, lane);
  __syncthreads();
  const JpegSyncScan sc = make_scan(a, sf, f);
  u32 c = grp.index * kLanes + lane;
  bool active = c < sf.nchunks;
  u32 gc = sf.chunk0 + c;
  u32 end_bit = jpeg_sync_chunk_start(sc, c + 1, sf.chunk_bytes, sf.nchunks);

  JpegSyncChunk my{};
  if (active) {
    if (round == 0) {
      jpeg_sync_first(
          sc, my, jpeg_sync_chunk_start(sc, c, sf.chunk_bytes, sf.nchunks),
          end_bit);
    } else {
      my = a.chunks[gc];
    }
    exits[lane] = my.exit;
  }
  if (round == 0 || grp.index > 0) {
    JpegSyncState e0 = my.entry;
    if (round > 0) e0 = a.gexit[(round & 1u) * a.nsgroups + blockIdx.x - 1];
    __syncthreads();
    u32 it = 0;
    int any;
    do {
      JpegSyncState cand = e0;
      if (active && lane > 0) cand = exits[lane - 1];
      __syncthreads();
      int changed = 0;
      if (active && jpeg_sync_step(sc, my, cand, end_bit)) {
        changed = 1;
        exits[lane] = my.exit;
      }
      any = __syncthreads_or(changed);
      ++it;
    } while (any && it < kLanes);
    if (active) a.chunks[gc] = my;
  }
  u32 last = min(kLanes, sf.nchunks - grp.index * kLanes) - 1;
  if (lane == last)
    a.gexit[((round + 1) & 1u) * a.nsgroups + blockIdx.x] = my.exit;
}

__global__ void __launch_bounds__(kLanes) jpeg_sync_scan_kernel(
    JpegSyncArgs a) {
  __shared__ u32 part[2][kLanes];
  const JpegSyncFile sf = a.sfiles[blockIdx.x];
  u32 lane = threadIdx.x;
  u32 per = (sf.nchunks + kLanes - 1) / kLanes;
  u32 c0 = min(lane * per, sf.nchunks), c1 = min(c0 + per, sf.nchunks);
  u32 sum = 0;
  for (u32 c = c0; c < c1; ++c) sum += a.chunks[sf.chunk0 + c].blocks;
  part[0][lane] = sum;
  __syncthreads();
  u32 cur = 0;
  for (u32 d = 1; d < kLanes; d <<= 1) {
    u32 v = part[cur][lane];
    if (lane >= d) v += part[cur][lane - d];
    part[cur ^ 1][lane] = v;
    cur ^= 1;
    __syncthreads();
  }
  u32 run = part[cur][lane] - sum;
  for (u32 c = c0; c < c1; ++c) {
    a.first_block[sf.chunk0 + c] = run;
    run += a.chunks[sf.chunk0 + c].blocks;
  }
  if (lane == kLanes - 1 && part[cur][lane] != sf.nblk)
    atomicMin(&a.dec.status[sf.file], (u32)kJpegSyncCount);
}

__global__ void __launch_bounds__(kLanes) jpeg_sync_write_kernel(
    JpegSyncArgs a) {
  __shared__ JpegDecFile f;
  const JpegSyncGroup grp = a.sgroups[blockIdx.x];
  const JpegSyncFile sf = a.sfiles[grp.sfile];
  u32 lane = threadIdx.x;
  load_file(f, a.dec.files + sf.file, lane);
  __syncthreads();
  u32 c = grp.index * kLanes + lane;
  if (c >= sf.nchunks) return;
  const JpegSyncScan sc = make_scan(a, sf, f);
  u32 gc = sf.chunk0 + c;
  JpegSyncState entry{0, 0, 0};
  if (c > 0) entry = a.chunks[gc - 1].exit;
  u64 coef_off = min(sf.coef_off, a.coef_count);
  u32 nblk = (u32)min((u64)sf.nblk, (a.coef_count - coef_off) / 64);
  u32 st = jpeg_sync_write(
      sc, a.chunks[gc], entry,
      jpeg_sync_chunk_start(sc, c + 1, sf.chunk_bytes, sf.nchunks),
      a.first_block[gc], nblk, f.zz2nat, a.coef + coef_off);
  if (st != kJpegBlockOk) atomicMin(&a.dec.status[sf.file], st);
}

// component of block b of an MCU
__device__ inline u32 block_comp(u32 bi, u32 ny) {
  return bi < ny ? 0u : min(bi - ny + 1, 2u);
}

__global__ void __launch_bounds__(kLanes) jpeg_sync_dc_kernel(JpegSyncArgs a) {
  __shared__ i64 part[2][3][kLanes];
  const JpegSyncFile sf = a.sfiles[blockIdx.x];
  // set by earlier kernels of the stream only: the same for every lane
  if (a.dec.status[sf.file] != kJpegDecNoError) return;
  const JpegDecGeom g = a.dec.files[sf.file].g;
  u32 lane = threadIdx.x;
  u32 bpm = g.blocks_per_mcu, ny = g.nc == 1 ? 1u : g.hs * g.vs;
  u64 coef_off = min(sf.coef_off, a.coef_count);
  u32 nblk = (u32)min((u64)sf.nblk, (a.coef_count - coef_off) / 64);
  u32 nmcu = nblk / bpm;
  i16* coef = a.coef + coef_off;
  u32 per = (nmcu + kLanes - 1) / kLanes;
  u32 m0 = min(lane * per, nmcu), m1 = min(m0 + per, nmcu);
  i64 sum[3] = {0, 0, 0};
  for (u32 m = m0; m < m1; ++m)
    for (u32 bi = 0; bi < bpm; ++bi) {
      i64 d = coef[((u64)m * bpm + bi) * 64];
      u32 comp = block_comp(bi, ny);
      if (comp == 0) sum[0] += d; else if (comp == 1) sum[1] += d; else sum[2] += d;
    }
  for (u32 k = 0; k < 3; ++k) part[0][k][lane] = sum[k];
  __syncthreads();
  u32 cur = 0;
  for (u32 d = 1; d < kLanes; d <<= 1) {
    for (u32 k = 0; k < 3; ++k) {
      i64 v = part[cur][k][lane];
      if (lane >= d) v += part[cur][k][lane - d];
      part[cur ^ 1][k][lane] = v;
    }
    cur ^= 1;
    __syncthreads();
  }
  i64 pred[3];
  for (u32 k = 0; k < 3; ++k) pred[k] = part[cur][k][lane] - sum[k];
  bool in_range = true;
  for (u32 m = m0; m < m1; ++m)
    for (u32 bi = 0; bi < bpm; ++bi) {
      i16* dcp = coef + ((u64)m * bpm + bi) * 64;
      u32 comp = block_comp(bi, ny);
      i64 p = (comp == 0 ? pred[0] : comp == 1 ? pred[1] : pred[2]) + *dcp;
      if (comp == 0) pred[0] = p; else if (comp == 1) pred[1] = p; else pred[2] = p;
      in_range &= p >= -32768 && p <= 32767;
      *dcp = (i16)(p < -32768 ? -32768 : p > 32767 ? 32767 : p);
    }
  if (!in_range) atomicMin(&a.dec.status[sf.file], (u32)kJpegSyncDcRange);
}

// grid (64-block groups of the largest file, files)
__global__ void __launch_bounds__(kIdctLanes) jpeg_sync_idct_kernel(
    JpegSyncArgs a) {
  const JpegSyncFile sf = a.sfiles[blockIdx.y];
  if (a.dec.status[sf.file] != kJpegDecNoError) return;
  const JpegDecFile& f = a.dec.files[sf.file];
  const JpegDecGeom g = f.g;
  u64 coef_off = min(sf.coef_off, a.coef_count);
  u32 nblk = (u32)min((u64)sf.nblk, (a.coef_count - coef_off) / 64);
  // the host builds nblk from the same geometry; the clamp keeps every
  // plane write in range whatever the record holds
  nblk = min(nblk, g.nmcu * g.blocks_per_mcu);
  u32 b = blockIdx.x * kIdctLanes + threadIdx.x;
  if (b >= nblk) return;
  u32 comp, px, py;
  jpeg_block_pos(g, b / g.blocks_per_mcu, b % g.blocks_per_mcu, comp, px, py);
  const uint4* src =
      reinterpret_cast<const uint4*>(a.coef + coef_off + (u64)b * 64);
  const u16* q = f.q[comp];
  i32 deq[64];
#pragma unroll
  for (u32 i = 0; i < 8; ++i) {
    uint4 v = src[i];
    u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (u32 j = 0; j < 4; ++j) {
      deq[i * 8 + 2 * j] = jpeg_dequant((i16)(w[j] & 0xffffu), q[i * 8 + 2 * j]);
      deq[i * 8 + 2 * j + 1] =
          jpeg_dequant((i16)(w[j] >> 16), q[i * 8 + 2 * j + 1]);
    }
  }
  u8 pix[64];
  jpeg_idct_block(deq, pix);
  if (g.nc == 1) {
    jpeg_store_block_grey(pix, f.out, (u32)g.h, (u32)g.w, px, py);
  } else {
    u32 stride = comp == 0 ? g.y_stride : g.c_stride;
    jpeg_store_block_plane(
        pix, a.dec.planes + f.plane_off[comp] + (u64)py * stride + px, stride);
  }
}

}  // namespace

void jpeg_sync_enqueue(const JpegSyncArgs& a, hipStream_t s) {
  auto check = [](hipError_t e) {
    if (e != hipSuccess)
      throw ScannerError(std::string("HIP error in jpeg sync decode: ") +
                         hipGetErrorString(e));
  };
  if (a.nsfiles == 0) return;
  check(hipMemsetAsync(a.coef, 0, a.coef_count * sizeof(i16), s));
  for (u32 r = 0; r <= a.max_rounds; ++r) {
    jpeg_sync_kernel<<<a.nsgroups, kLanes, 0, s>>>(a, r);
    check(hipGetLastError());
  }
  jpeg_sync_scan_kernel<<<a.nsfiles, kLanes, 0, s>>>(a);
  check(hipGetLastError());
  jpeg_sync_write_kernel<<<a.nsgroups, kLanes, 0, s>>>(a);
  check(hipGetLastError());
  jpeg_sync_dc_kernel<<<a.nsfiles, kLanes, 0, s>>>(a);
  check(hipGetLastError());
  jpeg_sync_idct_kernel<<<dim3((a.max_nblk + kIdctLanes - 1) / kIdctLanes,
                               a.nsfiles),
                          kIdctLanes, 0, s>>>(a);
  check(hipGetLastError());
}

}  // namespace sca
