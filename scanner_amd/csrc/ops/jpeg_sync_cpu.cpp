// CPU model of the self-synchronising JPEG decode in
// kernels/jpeg_sync_decode.hip: the functions of jpeg_sync_common.h in the
// order the kernels run them, lane by lane, with the same chunks, the same
// groups of 256 chunks and the same rounds across groups. It yields the
// pixels and the verdict (device row or fallback) of the kernels, runs
// without a GPU and is what the sanitizer build checks. HIP-free.
#include <algorithm>

#include "image_decode.h"
#include "jpeg_sync_common.h"

namespace sca {

void jpeg_decode_sync_model(const u8* data, const JpegInfo& info,
                            u32 chunk_bytes, u8* out, JpegSyncStats* stats) {
  u32 cb = chunk_bytes ? chunk_bytes : kJpegSyncChunkBytes;
  SCA_CHECK(jpeg_sync_valid_chunk_bytes(cb),
            "chunk_bytes must be a power of two >= 4, got " +
                std::to_string(cb));
  SCA_CHECK(info.restart_interval == 0 && info.segments.size() == 1,
            "the sync decoder takes a JPEG without restart markers");
  const JpegDecGeom& g = info.g;
  JpegSyncScan sc{data,   info.segments[0].begin, info.segments[0].end,
                  g.blocks_per_mcu, g.nc == 1 ? 1u : g.hs * g.vs,
                  info.dc, info.ac};
  u32 len = sc.end - sc.begin;
  JpegSyncStats st{};
  u32 status = kJpegBlockOk;
  auto raise = [&](u32 s) {
    if (s != kJpegBlockOk && (status == kJpegBlockOk || s < status)) status = s;
  };
  u32 nblk = g.nmcu * g.blocks_per_mcu;
  std::vector<i16> coef;

  if (len < kJpegSyncMaxScanBytes) {
    const u32 L = kJpegSyncGroupChunks;
    u32 n = jpeg_sync_chunk_count(len, cb);
    u32 groups = (n + L - 1) / L;
    u32 rounds = jpeg_sync_rounds(groups);
    st.chunks = n;
    st.groups = groups;
    auto start = [&](u32 c) { return jpeg_sync_chunk_start(sc, c, cb, n); };
    std::vector<JpegSyncChunk> rec(n);
    for (u32 c = 1; c < n; ++c)
      if (jpeg_sync_is_stuffing(sc, c * cb)) ++st.stuffed_starts;

    // one workgroup: lane i decodes again from lane i - 1's exit of the
    // iteration before, until no exit of the group changed
    auto sync_group = [&](u32 grp, const JpegSyncState& e0) {
      u32 c0 = grp * L, lanes = std::min(L, n - c0);
      std::vector<JpegSyncState> cand(lanes);
      bool any_changed = false;
      u32 it = 0;
      bool any;
      do {
        cand[0] = e0;
        for (u32 l = 1; l < lanes; ++l) cand[l] = rec[c0 + l - 1].exit;
        any = false;
        for (u32 l = 0; l < lanes; ++l)
          any |= jpeg_sync_step(sc, rec[c0 + l], cand[l], start(c0 + l + 1));
        any_changed |= any;
        ++it;
      } while (any && it < L);
      st.group_iterations = std::max(st.group_iterations, it);
      return any_changed;
    };

    std::vector<JpegSyncState> snap(groups), next(groups);
    for (u32 grp = 0; grp < groups; ++grp) {
      u32 c0 = grp * L, lanes = std::min(L, n - c0);
      for (u32 l = 0; l < lanes; ++l)
        jpeg_sync_first(sc, rec[c0 + l], start(c0 + l), start(c0 + l + 1));
      sync_group(grp, rec[c0].entry);
      snap[grp] = rec[c0 + lanes - 1].exit;
    }
    for (u32 r = 1; r <= rounds; ++r) {
      for (u32 grp = 0; grp < groups; ++grp) {
        u32 c0 = grp * L, lanes = std::min(L, n - c0);
        if (grp > 0 && sync_group(grp, snap[grp - 1])) {
          st.cross_rounds = r;
          ++st.cross_repairs;
        }
        next[grp] = rec[c0 + lanes - 1].exit;
      }
      snap.swap(next);
    }

    // scan: first block of every chunk, and the total
    std::vector<u32> first(n);
    u32 total = 0;
    for (u32 c = 0; c < n; ++c) {
      first[c] = total;
      total += rec[c].blocks;
      if (rec[c].entry.bit >= start(c + 1)) ++st.empty_chunks;
    }
    if (total != nblk) raise(kJpegSyncCount);

    // write
    coef.assign((size_t)nblk * 64, 0);
    for (u32 c = 0; c < n; ++c) {
      JpegSyncState entry = c ? rec[c - 1].exit : JpegSyncState{0, 0, 0};
      raise(jpeg_sync_write(sc, rec[c], entry, start(c + 1), first[c], nblk,
                            info.zz2nat, coef.data()));
    }

    // DC: running sums per component; the serial decoder clamps to int16,
    // which a prefix sum cannot reproduce
    if (status == kJpegBlockOk) {
      i64 pred[3] = {0, 0, 0};
      bool in_range = true;
      for (u32 b = 0; b < nblk; ++b) {
        u32 bi = b % g.blocks_per_mcu;
        u32 comp = bi < sc.ny ? 0u : bi - sc.ny + 1;
        pred[comp] += coef[(size_t)b * 64];
        in_range &= pred[comp] >= -32768 && pred[comp] <= 32767;
        coef[(size_t)b * 64] =
            (i16)std::max<i64>(-32768, std::min<i64>(32767, pred[comp]));
      }
      if (!in_range) raise(kJpegSyncDcRange);
    }
  } else {
    raise(kJpegSyncCount);
  }

  st.status = status;
  st.verified = status == kJpegBlockOk;
  if (stats) *stats = st;
  if (!st.verified) {
    // what the kernels' host side does with such a row
    jpeg_decode_cpu_into(data, info, out);
    return;
  }

  // IDCT and colour, as jpeg_decode_cpu_into
  size_t ysz = (size_t)g.y_stride * g.y_rows;
  size_t csz = (size_t)g.c_stride * g.c_rows;
  std::vector<u8> planes(ysz + 2 * csz);
  u8* plane[3] = {planes.data(), planes.data() + ysz,
                  planes.data() + ysz + csz};
  u32 stride[3] = {g.y_stride, g.c_stride, g.c_stride};
  for (u32 b = 0; b < nblk; ++b) {
    u32 comp, px, py;
    jpeg_block_pos(g, b / g.blocks_per_mcu, b % g.blocks_per_mcu, comp, px,
                   py);
    i32 deq[64];
    for (int k = 0; k < 64; ++k)
      deq[k] = jpeg_dequant(coef[(size_t)b * 64 + k], info.q[comp][k]);
    u8 pix[64];
    jpeg_idct_block(deq, pix);
    u8* dst = plane[comp] + (size_t)py * stride[comp] + px;
    for (int y = 0; y < 8; ++y)
      std::copy(pix + y * 8, pix + y * 8 + 8, dst + (size_t)y * stride[comp]);
  }
  if (g.nc == 1) {
    for (i32 y = 0; y < g.h; ++y)
      std::copy(plane[0] + (size_t)y * g.y_stride,
                plane[0] + (size_t)y * g.y_stride + g.w,
                out + (size_t)y * g.w);
    return;
  }
  for (i32 y = 0; y < g.h; ++y)
    for (i32 x = 0; x < g.w; ++x)
      jpeg_pixel_rgb(g, plane[0], plane[1], plane[2], (u32)x, (u32)y,
                     out + ((size_t)y * g.w + x) * 3);
}

}  // namespace sca
