// GPU decode of progressive JPEG (SOF2) for gfx950: the block decoders of
// csrc/ops/jpeg_progressive_common.h, one lane per restart segment of a
// scan. The host side of a batch, the colour kernel and the status words
// are those of kernels/jpeg_decode.hip; csrc/ops/jpeg_decode_cpu.cpp runs
// the same functions scan by scan on the CPU.
//
// A progressive file codes every coefficient in several scans, so the
// quantised coefficients live in an int16 workspace in HBM (64 per block, in
// the MCU order of jpeg_block_pos, zeroed per call) until the last scan has
// run. Scans of one file depend on each other, scans of different files do
// not: launch k runs scan k of every file of the batch that has one, and
// stream order is the only dependency between launches.
//   scan     one lane per restart segment, 64 segments of ONE scan of ONE
//            file per workgroup, the scan's descriptor (tables, band, bit
//            position, geometry) in LDS. A DC scan touches one coefficient
//            of a block: the lane reads and writes those two bytes in the
//            workspace directly. An AC scan works on a private 64 x int16
//            slot of an LDS tile (the zig-zag scatter and the refinement's
//            read-modify-write need addressable storage): the block is
//            loaded from the workspace as eight 16-byte pieces, decoded and
//            stored back the same way. A block inside an EOB run of an
//            AC-first scan is not touched at all. The lanes share nothing
//            after the descriptor load, so the loop has no barrier. A scan
//            without a restart interval is the degenerate case, one lane.
//   idct     one lane per block: dequantise, IDCT, the stores of the
//            restart kernel (a sibling of the self-synchronising decoder's).
// Status: a lane that meets an error writes the scan to the file's
// fail_scan word (every failing lane of a launch writes the same value) and
// atomicMin(segment << 4 | cause) to its status word, then stops. Launch k
// skips a file whose fail_scan is below k; a value written during launch k
// is k, so the lanes of the failing scan all run and the lowest failing
// segment of the first failing scan wins, which is what the CPU decoder
// reports.
//
// Bounds: every read of the entropy bytes lies in [begin, end) of the
// segment record (JpegBitReader); every workspace access in block
// [0, nblk) x 64 of the file's slice, clamped to the workspace; every slot
// write inside the lane's 64 entries (Se is clamped to 63); every plane
// write inside the MCU count of the geometry. The loops are bounded by the
// unit count of the segment x blocks per unit x 64 symbols.
#include <hip/hip_runtime.h>

#include "../csrc/ops/jpeg_progressive_common.h"
#include "jpeg_decode_dev.h"

namespace sca {

namespace {

constexpr u32 kLanes = 64;       // restart segments per workgroup
constexpr u32 kSlotStride = 66;  // int16 per lane slot: 33 words, so lanes
                                 // reading the same coefficient hit
                                 // different banks
constexpr u32 kIdctLanes = 64;

// a lane's slot is written by the block decoders as int16 and moved to and
// from the workspace as words: the word view has to be allowed to alias
typedef u32 __attribute__((may_alias)) SlotWord;

__global__ void __launch_bounds__(kLanes) jpeg_prog_scan_kernel(
    JpegProgArgs a, u32 group0, u32 k) {
  __shared__ JpegProgScanDesc d;
  __shared__ __attribute__((aligned(4))) i16 tile[kLanes * kSlotStride];
  const JpegProgGroup grp = a.groups[group0 + blockIdx.x];
  u32 lane = threadIdx.x;
  {
    const u32* src = reinterpret_cast<const u32*>(a.descs + grp.desc);
    u32* dst = reinterpret_cast<u32*>(&d);
    for (u32 i = lane; i < sizeof(JpegProgScanDesc) / 4; i += kLanes)
      dst[i] = src[i];
  }
  __syncthreads();
  if (lane >= grp.nseg) return;
  // an earlier scan of this file failed (a word written during this launch
  // holds k and does not count)
  if (a.fail_scan[d.file] < k) return;
  const JpegDecGeom& g = d.g;
  const JpegDecSeg seg = a.segs[grp.seg0 + lane];
  // the host builds the records from the same geometry; the clamps make
  // every access below in range whatever they hold
  const bool single = d.ncomp == 1;
  const u32 comp1 = min(d.comp, 2u);
  u32 bw = 1, bh = 1;
  if (single) jpeg_prog_comp_blocks(g, comp1, bw, bh);
  const u32 units = single ? bw * bh : g.nmcu;
  const u32 per_unit = single ? 1u : g.blocks_per_mcu;
  const u32 u0 = min(seg.first_mcu, units);
  const u32 u1 = u0 + min(seg.mcu_count, units - u0);
  const u64 coef_off = min(d.coef_off, a.coef_count);
  const u32 nblk = (u32)min((u64)g.nmcu * g.blocks_per_mcu,
                            (a.coef_count - coef_off) / 64);
  i16* coef = a.coef + coef_off;
  const u32 se = min(d.se, 63u), ss = min(d.ss, se);
  const u32 al = min(d.al, kJpegProgMaxAl), ah = d.ah;

  JpegBitReader br;
  jpeg_bits_init(br, a.dec.entropy, seg.begin, seg.end);
  i32 pred[3] = {0, 0, 0};
  u32 eobrun = 0;
  i16* slot = tile + lane * kSlotStride;
  u32 st = kJpegBlockOk;

  for (u32 u = u0; u < u1 && st == kJpegBlockOk; ++u) {
    for (u32 b = 0; b < per_unit; ++b) {
      u32 comp = single ? comp1 : jpeg_prog_block_comp(g, b);
      u32 idx = single ? jpeg_prog_block_index(g, comp, u % bw, u / bw)
                       : u * g.blocks_per_mcu + b;
      if (idx >= nblk) continue;
      i16* blk = coef + (u64)idx * 64;
      if (ss == 0) {
        // one coefficient: straight on the workspace
        i16 dcv = ah ? blk[0] : (i16)0;
        i32 p = comp == 0 ? pred[0] : comp == 1 ? pred[1] : pred[2];
        const JpegHuff& t = comp == 0 ? d.tab[0] : comp == 1 ? d.tab[1] : d.tab[2];
        st = jpeg_prog_block(br, t, d.zz2nat, 0, 0, ah, al, p, eobrun, &dcv);
        if (comp == 0) pred[0] = p; else if (comp == 1) pred[1] = p; else pred[2] = p;
        if (st != kJpegBlockOk) break;
        blk[0] = dcv;
        continue;
      }
      if (ah == 0 && eobrun > 0) {  // inside an EOB run: nothing to store
        --eobrun;
        continue;
      }
      uint4* blk4 = reinterpret_cast<uint4*>(blk);
      SlotWord* slot32 = reinterpret_cast<SlotWord*>(slot);
#pragma unroll
      for (u32 i = 0; i < 8; ++i) {
        uint4 v = blk4[i];
        slot32[4 * i] = v.x;
        slot32[4 * i + 1] = v.y;
        slot32[4 * i + 2] = v.z;
        slot32[4 * i + 3] = v.w;
      }
      i32 p = 0;
      st = jpeg_prog_block(br, d.tab[0], d.zz2nat, ss, se, ah, al, p, eobrun,
                           slot);
      if (st != kJpegBlockOk) break;
#pragma unroll
      for (u32 i = 0; i < 8; ++i)
        blk4[i] = make_uint4(slot32[4 * i], slot32[4 * i + 1],
                             slot32[4 * i + 2], slot32[4 * i + 3]);
    }
  }
  if (st != kJpegBlockOk) {
    a.fail_scan[d.file] = k;
    atomicMin(&a.dec.status[d.file], (grp.file_seg0 + lane) << 4 | st);
  }
}

// grid (64-block groups of the largest file, files)
__global__ void __launch_bounds__(kIdctLanes) jpeg_prog_idct_kernel(
    JpegProgArgs a) {
  const JpegProgFile pf = a.pfiles[blockIdx.y];
  if (a.dec.status[pf.file] != kJpegDecNoError) return;
  const JpegDecFile& f = a.dec.files[pf.file];
  const JpegDecGeom g = f.g;
  u64 coef_off = min(pf.coef_off, a.coef_count);
  u32 nblk = (u32)min((u64)pf.nblk, (a.coef_count - coef_off) / 64);
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

void jpeg_prog_enqueue(const JpegProgArgs& a, const u32* group0, u32 nlaunch,
                       hipStream_t s) {
  auto check = [](hipError_t e) {
    if (e != hipSuccess)
      throw ScannerError(std::string("HIP error in jpeg progressive decode: ") +
                         hipGetErrorString(e));
  };
  if (a.npfiles == 0) return;
  check(hipMemsetAsync(a.coef, 0, a.coef_count * sizeof(i16), s));
  for (u32 k = 0; k < nlaunch; ++k) {
    u32 n = group0[k + 1] - group0[k];
    if (n == 0) continue;
    jpeg_prog_scan_kernel<<<n, kLanes, 0, s>>>(a, group0[k], k);
    check(hipGetLastError());
  }
  jpeg_prog_idct_kernel<<<dim3((a.max_nblk + kIdctLanes - 1) / kIdctLanes,
                               a.npfiles),
                          kIdctLanes, 0, s>>>(a);
  check(hipGetLastError());
}

}  // namespace sca
