// Device-side records shared by the two halves of the GPU JPEG decoder:
// kernels/jpeg_decode.hip (restart segments, colour, the host side of a
// batch) and kernels/jpeg_sync_decode.hip (scans without restart markers).
#pragma once

#include <hip/hip_runtime.h>

#include "../csrc/ops/image_decode.h"
#include "../csrc/ops/jpeg_sync_common.h"

namespace sca {

constexpr u32 kJpegDecNoError = 0xffffffffu;

struct JpegDecFile {
  JpegDecGeom g;
  u32 status_index;
  u32 pad;
  u64 plane_off[3];  // into the plane workspace; unused for grey
  u8* out;           // HWC u8
  u16 q[3][64];
  u8 zz2nat[64];
  JpegHuff dc[3], ac[3];
};
static_assert(sizeof(JpegDecFile) % 8 == 0, "descriptors are copied as words");

struct JpegDecGroup {
  u32 file;
  u32 seg0;        // first segment record of the workgroup
  u32 nseg;        // lanes in use
  u32 file_seg0;   // index of that segment inside its file
};
struct JpegDecSeg {
  u32 begin, end;  // into the packed entropy bytes
  u32 first_mcu, mcu_count;
};

struct JpegDecArgs {
  const JpegDecFile* files;
  const JpegDecGroup* groups;
  const JpegDecSeg* segs;
  const u8* entropy;
  u8* planes;
  u32* status;
  u32 nfiles;
};

// Launches of kernels/jpeg_decode.hip for a caller that has built the
// records itself (kernels/mjpeg_index.hip, whose entropy bytes are a
// device-resident span): the restart-segment kernel over `ngroups` group
// records, then, when colour_blocks is not 0, the colour kernel over
// a.nfiles files. Failures go to the status words, which the caller has set
// to kJpegDecNoError.
constexpr u32 kJpegDecLanes = 64;  // restart segments per workgroup
void jpeg_dec_enqueue(const JpegDecArgs& a, u32 ngroups, u32 colour_blocks,
                      hipStream_t stream);
// x extent of the colour grid one file of this geometry needs (0: grey)
u32 jpeg_dec_colour_blocks(const JpegDecGeom& g);

// 8x8 samples of a grey file go straight to the image: only the part of the
// block inside it
__device__ inline void jpeg_store_block_grey(const u8 (&pix)[64], u8* img,
                                             u32 h, u32 w, u32 px, u32 py) {
#pragma unroll
  for (u32 y = 0; y < 8; ++y) {
    if (py + y >= h) break;
#pragma unroll
    for (u32 x = 0; x < 8; ++x) {
      if (px + x < w) img[(u64)(py + y) * w + px + x] = pix[y * 8 + x];
    }
  }
}
// ... of a colour file to the padded component plane, 8 rows of 8 bytes
__device__ inline void jpeg_store_block_plane(const u8 (&pix)[64], u8* dst,
                                              u32 stride) {
#pragma unroll
  for (u32 y = 0; y < 8; ++y) {
    uint2 v;
    v.x = pix[y * 8] | pix[y * 8 + 1] << 8 | pix[y * 8 + 2] << 16 |
          (u32)pix[y * 8 + 3] << 24;
    v.y = pix[y * 8 + 4] | pix[y * 8 + 5] << 8 | pix[y * 8 + 6] << 16 |
          (u32)pix[y * 8 + 7] << 24;
    *reinterpret_cast<uint2*>(dst + (u64)y * stride) = v;
  }
}

// ---- scans without restart markers (jpeg_sync_decode.hip) ----
struct JpegSyncFile {
  u32 file;        // its JpegDecFile, and its status word
  u32 begin, end;  // the scan, in the packed entropy bytes
  u32 chunk_bytes;
  u32 nchunks, chunk0;  // chunk0: its first record in the batch's arrays
  u32 ngroups;
  u32 rounds;  // jpeg_sync_rounds(ngroups)
  u32 nblk;    // nmcu * blocks_per_mcu
  u32 pad;
  u64 coef_off;  // into the coefficient workspace, int16 units
};
struct JpegSyncGroup {
  u32 sfile;  // JpegSyncFile
  u32 index;  // group inside its file; a file's groups are consecutive
};
struct JpegSyncArgs {
  JpegDecArgs dec;
  const JpegSyncFile* sfiles;
  const JpegSyncGroup* sgroups;
  JpegSyncChunk* chunks;   // one per chunk of the batch
  u32* first_block;        // one per chunk
  JpegSyncState* gexit;    // [2][nsgroups]: last exit of a group, two rounds
  i16* coef;               // 64 per block, zeroed by the enqueue
  u64 coef_count;
  u32 nsfiles, nsgroups;
  u32 max_rounds, max_nblk;  // over the files
};
// Enqueues everything between the upload and the colour kernel for the
// batch's files without restart markers; failures go to the status words.
void jpeg_sync_enqueue(const JpegSyncArgs& a, hipStream_t stream);

// ---- progressive files (jpeg_progressive_decode.hip) ----
// One scan of one file: what a workgroup keeps in LDS.
struct JpegProgScanDesc {
  JpegDecGeom g;
  u32 file;         // its JpegDecFile, and its status words
  u32 ncomp, comp;  // comp: the component of a single-component scan
  u32 ss, se, ah, al;
  u32 pad;
  u64 coef_off;     // the file's slice of the coefficient workspace, int16s
  u8 zz2nat[64];
  // ss == 0: the DC tables of components 0..2; else [0] is the AC table
  JpegHuff tab[3];
};
static_assert(sizeof(JpegProgScanDesc) % 8 == 0,
              "descriptors are copied as words");
struct JpegProgGroup {
  u32 desc;
  u32 seg0;       // first segment record of the workgroup
  u32 nseg;       // lanes in use
  u32 file_seg0;  // index of that segment inside its scan
};
struct JpegProgFile {
  u32 file;  // its JpegDecFile
  u32 nblk;  // nmcu * blocks_per_mcu
  u64 coef_off;
};
struct JpegProgArgs {
  JpegDecArgs dec;
  const JpegProgScanDesc* descs;
  const JpegProgGroup* groups;  // ordered by scan index, then file
  const JpegDecSeg* segs;       // first_mcu/mcu_count in the scan's units
  const JpegProgFile* pfiles;
  // one word per JpegDecFile, kJpegDecNoError or the scan that failed; the
  // cause and the segment go to dec.status as for a baseline file
  u32* fail_scan;
  i16* coef;  // 64 per block, zeroed by the enqueue
  u64 coef_count;
  u32 npfiles, max_nblk;
};
// Enqueues everything between the upload and the colour kernel for the
// batch's progressive files: the memset of the workspace, one launch per
// scan index k over groups [group0[k], group0[k + 1]), k < nlaunch, and the
// IDCT. Failures go to the status words.
void jpeg_prog_enqueue(const JpegProgArgs& a, const u32* group0, u32 nlaunch,
                       hipStream_t stream);

}  // namespace sca
