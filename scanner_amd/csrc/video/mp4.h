// Minimal ISO-BMFF (mp4) demuxer and remuxer — pure parsing, no codec or
// container libraries.
//
// Capability parity: the reference demuxes mp4 through FFmpeg AVIO during
// ingest (scanner/engine/ingest.cpp:82-155) and indexes mp4s in place via
// the external hwang parser (ingest.cpp:382); its save_mp4 export
// (python/scannerpy/storage.py:353-374) also rides on FFmpeg. Here the
// sample tables (stsd/avcC, stts, stss, stsc, stsz, stco/co64) are parsed
// directly, giving per-sample absolute byte offsets + keyframes, and the
// writer remuxes an indexed H.264 elementary stream back into a playable
// .mp4 — no transcode, so no codec needed.
//
// Motion-JPEG tracks (video/mjpeg.h) are read and written too. Two sample
// entries carry them: 'jpeg', QuickTime's Photo-JPEG, a plain
// VisualSampleEntry; and 'mp4v' whose 'esds' DecoderConfigDescriptor has
// objectTypeIndication 0x6C (ISO/IEC 14496-1: "Visual ISO/IEC 10918-1",
// JPEG), which is what ffmpeg writes into .mp4. Each sample is one complete
// JPEG file and every sample is a sync sample.
#pragma once

#include <string>
#include <vector>

#include "../common.h"

namespace sca {

struct Mp4Track {
  std::string codec = "h264";       // "h264" or "mjpeg"
  i32 width = 0, height = 0;        // h264: from the SPS (authoritative);
                                    // mjpeg: from the sample entry
  i32 length_size = 4;              // AVCC NAL length prefix bytes
  std::vector<std::vector<u8>> sps; // raw NAL bytes (no start code)
  std::vector<std::vector<u8>> pps;
  std::vector<u64> sample_offsets;  // absolute file offsets
  std::vector<u64> sample_sizes;
  std::vector<i64> keyframe_indices;
  u32 timescale = 0;
  std::vector<u32> sample_deltas;   // per-sample duration (expanded stts)
};

// Parse the first video track of an mp4 or mov in memory: AVC, or
// Motion-JPEG in one of the two sample entries above. Throws ScannerError on
// anything malformed or missing.
Mp4Track mp4_parse(const u8* data, size_t size);

// Remux: wrap H.264 access units (Annex-B byte ranges of `stream` given by
// offsets/sizes) into an mp4. `sps`/`pps` are raw NAL bytes. `fps` sets
// stts. Returns the complete file contents.
std::vector<u8> mp4_write(const u8* stream, size_t stream_size,
                          const std::vector<u64>& sample_offsets,
                          const std::vector<u64>& sample_sizes,
                          const std::vector<i64>& keyframe_indices,
                          const std::vector<u8>& sps,
                          const std::vector<u8>& pps, i32 width, i32 height,
                          double fps = 30.0);

// Wrap Motion-JPEG samples (complete JPEG files, byte ranges of `stream`)
// into an mp4: sample entry 'mp4v' with an 'esds' of ES_Descriptor ->
// DecoderConfigDescriptor (objectTypeIndication 0x6C, streamType visual, no
// DecoderSpecificInfo) -> SLConfigDescriptor (predefined 0x02); no 'stss',
// so every sample is a sync sample.
std::vector<u8> mp4_write_mjpeg(const u8* stream, size_t stream_size,
                                const std::vector<u64>& sample_offsets,
                                const std::vector<u64>& sample_sizes,
                                i32 width, i32 height, double fps = 30.0);

}  // namespace sca
