// Hand-written bf16 GEMM on MFMA for gfx950 — the conv/GEMM engine of the
// DNN-inference op (ResNet-50). Structure follows the CDNA4 canonical GEMM
// anatomy (cdna_hip_programming.md §5): 128-wide tiles, global_load_lds
// 16-byte staging into double-buffered LDS, v_mfma_f32_16x16x32_bf16 inner
// loop accumulating fp32, fused epilogue (per-channel scale+bias = folded
// BN, ReLU, residual add) writing bf16.
//
// C[M,N] = A[M,K] @ B[N,K]^T   (A row-major [M][K]; B stored [N][K] so
// both operands are contiguous in K — weights are laid out at init time).
// K and N must be multiples of 64 (callers pad); M is arbitrary.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>
#include <type_traits>

#include "../csrc/memory.h"
#include "dnn.h"

namespace sca {

namespace {

using bf16 = __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ inline float bf16_to_f32(bf16 v) { return (float)v; }

__device__ inline bf16 f32_to_bf16(float v) { return (bf16)v; }

__device__ inline void glds16(const bf16* src, bf16* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) uint32_t*)src,
      (__attribute__((address_space(3))) uint32_t*)lds_dst, 16, 0, 0);
}

// The wave's FN per-column scale and bias values (folded BN), one register
// each: column n0 + wcol*COLS + j*16 + (lane & 15) = col0 + j*16. Loaded
// once per workgroup, unconditionally behind ONE workgroup-uniform null
// test per pointer. (A `scale ? scale[col] : 1.f` per fragment makes hipcc
// branch around each load and wait vmcnt(0) right after it: 2*FM*FN
// dependent L2 round trips per workgroup.) Callers issue this before their
// first stage(), so the K loop's first vmcnt(0) retires the loads for free.
template <int FN>
__device__ inline void load_scale_bias(float (&sc)[FN], float (&bi)[FN],
                                       const float* __restrict__ scale,
                                       const float* __restrict__ bias,
                                       int col0) {
  if (scale) {
#pragma unroll
    for (int j = 0; j < FN; ++j) sc[j] = scale[col0 + j * 16];
  } else {
#pragma unroll
    for (int j = 0; j < FN; ++j) sc[j] = 1.f;
  }
  if (bias) {
#pragma unroll
    for (int j = 0; j < FN; ++j) bi[j] = bias[col0 + j * 16];
  } else {
#pragma unroll
    for (int j = 0; j < FN; ++j) bi[j] = 0.f;
  }
}

// All of a wave's residual reads for one output tile, issued back to back:
// FM 16-row blocks x CHUNK/8 16-byte loads per lane, in the layout
// epilogue_store consumes (lane -> row lane>>2, CHUNK columns from chunk
// lane&3). Rows past M are clamped to M-1 (never stored), which keeps the
// loads free of branches.
template <int FM, int FN>
__device__ inline void load_residual(bf16x8 (&res)[FM][FN / 2],
                                     const bf16* __restrict__ residual,
                                     int M, int N, int m0, int n0, int wrow,
                                     int wcol, int lane) {
  constexpr int COLS = FN * 16;
  constexpr int CHUNK = COLS / 4;
  int colbase = n0 + wcol * COLS + (lane & 3) * CHUNK;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    int row = m0 + wrow * (FM * 16) + i * 16 + (lane >> 2);
    row = row < M ? row : M - 1;
    const bf16* src = residual + (size_t)row * N + colbase;
#pragma unroll
    for (int c = 0; c < CHUNK / 8; ++c)
      res[i][c] = *reinterpret_cast<const bf16x8*>(src + c * 8);
  }
}

// Coalesced epilogue: the MFMA fragment layout leaves each lane holding
// 4 rows x 1 col, so direct stores are 2-byte scattered (measured 1.4 TB/s
// on store-bound shapes — 1/6 of HBM). Transpose each 16-row block through
// per-wave LDS scratch (write col-major with scale/bias applied, read back
// 16 consecutive cols per lane), then store 32 contiguous bytes per lane —
// full 64-byte-per-4-lane coalescing. Scratch is per-wave, so only
// intra-wave lgkmcnt ordering is needed: no block barrier, which keeps the
// small-K kernel's cross-tile A prefetch in flight. Scale, bias and the
// residual arrive in registers (load_scale_bias / load_residual): no global
// load is issued in here.
template <int FM, int FN, bool RELU, bool RESIDUAL>
__device__ inline void epilogue_store(f32x4 (&acc)[FM][FN], float* scratch,
                                      bf16* __restrict__ C,
                                      const bf16x8 (&res)[FM][FN / 2], int M,
                                      int N, int m0, int n0, int wrow,
                                      int wcol, int lane,
                                      const float (&sc)[FN],
                                      const float (&bi)[FN]) {
  constexpr int COLS = FN * 16;
  constexpr int STRIDE = COLS + 4;  // keeps 16 B row alignment, breaks banks
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    asm volatile("s_waitcnt lgkmcnt(0)");  // WAR: prior reads done
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      int cw = j * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        scratch[((lane >> 4) * 4 + r) * STRIDE + cw] =
            acc[i][j][r] * sc[j] + bi[j];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)");  // writes visible to own reads
    constexpr int CHUNK = COLS / 4;        // contiguous cols per lane (>=8)
    static_assert(CHUNK >= 8 && CHUNK % 8 == 0, "wave tile too narrow");
    int r2 = lane >> 2;                    // 16 rows
    int q = lane & 3;                      // 4 chunks per row
    int row = m0 + wrow * (FM * 16) + i * 16 + r2;
    if (row < M) {
      int colbase = n0 + wcol * COLS + q * CHUNK;
      const float* src = scratch + r2 * STRIDE + q * CHUNK;
      bf16 out[CHUNK];
#pragma unroll
      for (int k = 0; k < CHUNK; ++k) {
        float v = src[k];
        if constexpr (RESIDUAL) v += bf16_to_f32(res[i][k / 8][k % 8]);
        if constexpr (RELU) v = v > 0.f ? v : 0.f;
        out[k] = f32_to_bf16(v);
      }
      // 16-byte stores, contiguous across the 4 q-lanes of each row
#pragma unroll
      for (int c8 = 0; c8 < CHUNK; c8 += 8) {
        *reinterpret_cast<bf16x8*>(C + (size_t)row * N + colbase + c8) =
            *reinterpret_cast<const bf16x8*>(out + c8);
      }
    }
  }
}

// LDS staging of one BM x 64 A tile and one BN x 64 B tile per K step, for
// the tile kernel and the split-K kernel alike. Each wave covers 8 rows x
// 64 k per LDS-DMA instruction (64 lanes x 16 B = 8 bf16 each): BM/32
// instructions per wave for A, BN/32 for B. All divisions happen in
// init(); advance() and issue() do none, and issue() has no branch around
// a DMA: the zero-or-address choice is a select, so the DMAs of a step go
// out back to back.
//
// IMPLICIT: A is the NHWC activation tensor and the staging gathers im2col
// rows on the fly (ConvDesc d gives the geometry; zero points at 16+ zero
// bytes for padding / k-pad lanes). Lane-addressed global_load_lds makes
// the gather free of any HBM im2col round trip.
//  - generic (any c % 8 == 0; conv1's c = 8, c = 24): per lane, the
//    output-pixel part of the gather address is k-independent and
//    (cell, cj, dr, ds) advance by a constant per step; the former is
//    precomputed, the latter stepped incrementally.
//  - FAST (c % 64 == 0, r*s <= 32, K == r*s*c; chosen on the host — every
//    3x3 and strided 1x1 conv of ResNet-50): a 64-wide step never leaves
//    one (r, s) cell, so cell/dr/ds and the step's element offset are
//    workgroup-uniform scalars. Per lane and row only a base pointer (tap
//    (0,0), may lie outside the image — it is dereferenced only when the
//    tap's validity bit is set) and a validity word with one bit per tap
//    are kept. A DMA then costs an add of the uniform offset, a bit test
//    and a select.
template <int BM, int BN, bool IMPLICIT, bool FAST>
struct TileStager {
  static constexpr int BK = 64;
  static constexpr int A_INSTRS = BM / 8 / 4;  // per wave
  static constexpr int B_INSTRS = BN / 8 / 4;
  static_assert(IMPLICIT || !FAST, "FAST is an implicit-conv mode");

  const bf16* b_src[B_INSTRS];    // at the current k
  const bf16* a_src[A_INSTRS];    // direct: at the current k; FAST: tap (0,0)
  uint32_t valid[A_INSTRS];       // FAST: bit (dr*s + ds) = tap inside image
  i64 rowbase[A_INSTRS];          // generic: nn*h*w*c
  int hh0[A_INSTRS];              // generic: p*stride - pad
  int ww0[A_INSTRS];              // generic: q*stride - pad
  int cell, cj, dr, ds;           // generic: per lane; FAST: uniform

  // k0: first k of the first step (a multiple of 64, workgroup-uniform)
  __device__ inline void init(const bf16* __restrict__ A,
                              const bf16* __restrict__ B, int M, int K,
                              int m0, int n0, int wave, int lane, int k0,
                              const ConvDesc& d) {
    const int lrow = lane >> 3;     // 0..7 row within instr block
    const int lk = (lane & 7) * 8;  // k offset (8 bf16 = 16B)
#pragma unroll
    for (int i = 0; i < B_INSTRS; ++i) {
      int row = (wave * B_INSTRS + i) * 8 + lrow;
      b_src[i] = B + (size_t)(n0 + row) * K + k0 + lk;
    }
#pragma unroll
    for (int i = 0; i < A_INSTRS; ++i) {
      int row = (wave * A_INSTRS + i) * 8 + lrow;
      int grow = m0 + row;
      if (grow >= M) grow = M - 1;  // clamp: garbage rows masked at store
      if constexpr (!IMPLICIT) {
        a_src[i] = A + (size_t)grow * K + k0 + lk;
      } else {
        int q = grow % d.ow;
        int t = grow / d.ow;
        int p = t % d.oh;
        int nn = t / d.oh;
        int h0 = p * d.stride - d.pad;
        int w0 = q * d.stride - d.pad;
        if constexpr (FAST) {
          a_src[i] =
              A + ((((i64)nn * d.h + h0) * d.w + w0) * d.c + lk);
          uint32_t cmask = 0;
          for (int x = 0; x < d.s; ++x)
            cmask |= (uint32_t)((unsigned)(w0 + x) < (unsigned)d.w) << x;
          uint32_t v = 0;
          for (int y = 0; y < d.r; ++y)
            v |= ((unsigned)(h0 + y) < (unsigned)d.h) ? cmask << (y * d.s)
                                                     : 0u;
          valid[i] = v;
        } else {
          rowbase[i] = (i64)nn * d.h * d.w * d.c;
          hh0[i] = h0;
          ww0[i] = w0;
        }
      }
    }
    if constexpr (IMPLICIT) {
      int k = FAST ? k0 : k0 + lk;
      cell = k / d.c;
      cj = k - cell * d.c;
      dr = cell / d.s;
      ds = cell - dr * d.s;
    }
  }

  // step to the next 64 k
  __device__ inline void advance(const ConvDesc& d) {
#pragma unroll
    for (int i = 0; i < B_INSTRS; ++i) b_src[i] += BK;
    if constexpr (!IMPLICIT) {
#pragma unroll
      for (int i = 0; i < A_INSTRS; ++i) a_src[i] += BK;
    } else {
      // c >= 8, so the generic wrap loop is short; with FAST (c % 64 == 0)
      // it runs at most once and on scalars
      cj += BK;
      while (cj >= d.c) {
        cj -= d.c;
        ++cell;
        ++ds;
        if (ds == d.s) {
          ds = 0;
          ++dr;
        }
      }
    }
  }

  // issue the current step's DMAs into the buffer at lds_a
  // ([BM rows of A][BN rows of B], 64 k each)
  __device__ inline void issue(bf16* lds_a, int wave,
                               const bf16* __restrict__ A,
                               const ConvDesc& d,
                               const bf16* __restrict__ zero) const {
    bf16* lds_b = lds_a + BM * BK;
    i64 step_off = 0;
    if constexpr (FAST) step_off = ((i64)dr * d.w + ds) * d.c + cj;
#pragma unroll
    for (int i = 0; i < A_INSTRS; ++i) {
      const bf16* src;
      if constexpr (!IMPLICIT) {
        src = a_src[i];
      } else if constexpr (FAST) {
        src = ((valid[i] >> cell) & 1u) ? a_src[i] + step_off : zero;
      } else {
        int hh = hh0[i] + dr;
        int ww = ww0[i] + ds;
        bool ok = cell < d.r * d.s && (unsigned)hh < (unsigned)d.h &&
                  (unsigned)ww < (unsigned)d.w;
        const bf16* in =
            A + (rowbase[i] + ((i64)hh * d.w + ww) * d.c + cj);
        src = ok ? in : zero;
      }
      glds16(src, lds_a + (size_t)(wave * A_INSTRS + i) * 8 * BK);
    }
#pragma unroll
    for (int i = 0; i < B_INSTRS; ++i)
      glds16(b_src[i], lds_b + (size_t)(wave * B_INSTRS + i) * 8 * BK);
  }
};

// One 64-wide K step of MFMAs on the staged tile at lds_a.
template <int BM, int BN, int WM, int WN, int FM, int FN>
__device__ inline void mfma_step(f32x4 (&acc)[FM][FN], const bf16* lds_a,
                                 int wrow, int wcol, int lane) {
  constexpr int BK = 64;
  const bf16* lds_b = lds_a + BM * BK;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {  // two K=32 chunks per BK
    int kbase = kk * 32 + (lane >> 4) * 8;
    bf16x8 afrag[FM], bfrag[FN];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      int row = wrow * (BM / WM) + i * 16 + (lane & 15);
      afrag[i] = *reinterpret_cast<const bf16x8*>(
          lds_a + (size_t)row * BK + kbase);
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      int col = wcol * (BN / WN) + j * 16 + (lane & 15);
      bfrag[j] = *reinterpret_cast<const bf16x8*>(
          lds_b + (size_t)col * BK + kbase);
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag[i], bfrag[j], acc[i][j], 0, 0, 0);
  }
}

// One workgroup = 256 threads = 4 waves in a WM x WN grid; each wave owns
// a (BM/WM) x (BN/WN) output sub-tile as FM x FN fragments of 16x16.
// IMPLICIT / FAST: see TileStager.
template <int BM, int BN, int WM, int WN, bool RELU, bool RESIDUAL,
          bool IMPLICIT, bool FAST>
__global__ void __launch_bounds__(256, 2)
    gemm_bf16_kernel(const bf16* __restrict__ A, const bf16* __restrict__ B,
                     bf16* __restrict__ C, int M, int N, int K,
                     const float* __restrict__ scale,
                     const float* __restrict__ bias,
                     const bf16* __restrict__ residual, ConvDesc d,
                     const bf16* __restrict__ zero) {
  constexpr int BK = 64;
  constexpr int FM = BM / WM / 16;
  constexpr int FN = BN / WN / 16;
  // LDS: [2 buffers][A BM rows + B BN rows][BK]
  __shared__ bf16 lds[2 * (BM + BN) * BK];

  int tid = threadIdx.x;
  int lane = tid & 63;
  int wave = tid >> 6;
  int wrow = wave / WN;
  int wcol = wave % WN;

  // XCD-aware swizzle (T1): consecutive blockIdx.x stay on one XCD's share
  // of the N dimension when the grid allows.
  int nwg = gridDim.x;
  int wgid = blockIdx.x;
  if (nwg % 8 == 0) {
    int q = nwg / 8;
    wgid = (wgid % q) * 8 + wgid / q;
  }
  int ntiles_n = (N + BN - 1) / BN;
  int m0 = (wgid / ntiles_n) * BM;
  int n0 = (wgid % ntiles_n) * BN;

  // epilogue operands first: the K loop's first vmcnt(0) retires them
  float sc[FN], bi[FN];
  load_scale_bias<FN>(sc, bi, scale, bias,
                      n0 + wcol * (FN * 16) + (lane & 15));

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  TileStager<BM, BN, IMPLICIT, FAST> st;
  st.init(A, B, M, K, m0, n0, wave, lane, 0, d);
  bf16x8 res[FM][FN / 2] = {};

  int ksteps = K / BK;
  st.issue(lds, wave, A, d, zero);
  for (int ks = 0; ks + 1 < ksteps; ++ks) {
    int buf = ks & 1;
    // prefetch next while computing current
    __builtin_amdgcn_s_waitcnt(/*vmcnt(0) lgkmcnt(0)*/ 0);
    __syncthreads();
    st.advance(d);
    st.issue(lds + (buf ^ 1) * (BM + BN) * BK, wave, A, d, zero);
    mfma_step<BM, BN, WM, WN>(acc, lds + buf * (BM + BN) * BK, wrow, wcol,
                              lane);
    // No trailing barrier: the next iteration's leading waitcnt+barrier
    // orders everything, and a __syncthreads() here would drain the
    // in-flight LDS-DMA prefetch (vmcnt(0) in its fence).
  }
  // Last step, peeled: no LDS-DMA is outstanding any more, so the tile's
  // residual reads go out here and land under the step's MFMAs. (Inside
  // the loop the loaded registers would be live around the back edge, and
  // hipcc then waits vmcnt(0) for them in every step — draining the
  // prefetch.)
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if constexpr (RESIDUAL)
    load_residual<FM, FN>(res, residual, M, N, m0, n0, wrow, wcol, lane);
  mfma_step<BM, BN, WM, WN>(acc, lds + ((ksteps - 1) & 1) * (BM + BN) * BK,
                            wrow, wcol, lane);

  // epilogue: D = act(acc * scale[col] + bias[col] [+ residual]), stored
  // coalesced via per-wave LDS transpose. The scratch overlays the staging
  // LDS (no extra LDS), so one barrier first: every wave must be done
  // reading its final fragments before any wave overwrites the buffer.
  // No LDS-DMA is in flight here (the last iteration stages no prefetch);
  // the barrier's fence only waits for the residual reads issued above.
  __syncthreads();
  constexpr int EP_STRIDE = BN / WN + 4;
  float* scratch =
      reinterpret_cast<float*>(lds) + (size_t)wave * 16 * EP_STRIDE;
  epilogue_store<FM, FN, RELU, RESIDUAL>(acc, scratch, C, res, M, N, m0, n0,
                                         wrow, wcol, lane, sc, bi);
}

// Small-K variant (K = 64: the DNN ops' 1x1 convolutions out of 64-channel
// activations). A single K-step leaves the main kernel with no prefetch
// overlap — every A tile is a cold HBM read the MFMAs must wait on
// (measured 69 TF/s at M=50176,N=256,K=64). Here a workgroup walks
// MULTIPLE M-tiles of one N-strip, double-buffering the A staging across
// tiles: tile t+1's global_load_lds runs while tile t's MFMAs and stores
// execute. B ([BN][64], 16 KB) is staged once and reused for the whole
// walk. K=64 keeps the 128-byte LDS row layout the lane-contiguous
// LDS-DMA scatter requires.
template <int BM, int BN, int WM, int WN, bool RELU, bool RESIDUAL>
__global__ void __launch_bounds__(256, 2)
    gemm_bf16_smallk_kernel(const bf16* __restrict__ A,
                            const bf16* __restrict__ B, bf16* __restrict__ C,
                            int M, int N, const float* __restrict__ scale,
                            const float* __restrict__ bias,
                            const bf16* __restrict__ residual,
                            int tiles_per_wg) {
  constexpr int K = 64;
  constexpr int FM = BM / WM / 16;
  constexpr int FN = BN / WN / 16;
  // ONE __shared__ array for B, the two A buffers and the epilogue
  // scratch: with several LDS objects next to an LDS-DMA target hipcc puts
  // s_waitcnt vmcnt(0) in front of the first ds_read of every tile, which
  // drains the A prefetch issued just before it.
  constexpr int EP_FLOATS = 4 * 16 * (BN / WN + 4);
  __shared__ bf16 lds[BN * K + 2 * BM * K + EP_FLOATS * 2];
  bf16* lds_b = lds;
  bf16* lds_a = lds + BN * K;
  float* lds_ep = reinterpret_cast<float*>(lds + BN * K + 2 * BM * K);

  int tid = threadIdx.x;
  int lane = tid & 63;
  int wave = tid >> 6;
  int wrow = wave / WN;
  int wcol = wave % WN;

  int ntiles_n = (N + BN - 1) / BN;
  int ntiles_m = (M + BM - 1) / BM;
  int strip = blockIdx.x / ntiles_n;
  int n0 = (blockIdx.x % ntiles_n) * BN;
  int mt0 = strip * tiles_per_wg;
  int mt_end = min(mt0 + tiles_per_wg, ntiles_m);
  if (mt0 >= ntiles_m) return;

  // the strip's scale/bias: once, before the M walk (retired by the first
  // tile's vmcnt(0))
  float sc[FN], bi[FN];
  load_scale_bias<FN>(sc, bi, scale, bias,
                      n0 + wcol * (FN * 16) + (lane & 15));

  const int lrow = lane >> 3;
  const int lk = (lane & 7) * 8;
  constexpr int B_INSTRS = BN / 8 / 4;
  constexpr int A_INSTRS = BM / 8 / 4;

#pragma unroll
  for (int i = 0; i < B_INSTRS; ++i) {
    int row = (wave * B_INSTRS + i) * 8 + lrow;
    glds16(B + (size_t)(n0 + row) * K + lk,
           lds_b + (size_t)(wave * B_INSTRS + i) * 8 * K);
  }

  auto stage_a = [&](int buf, int mt) {
    int m0 = mt * BM;
    bf16* dst = lds_a + buf * BM * K;
#pragma unroll
    for (int i = 0; i < A_INSTRS; ++i) {
      int row = (wave * A_INSTRS + i) * 8 + lrow;
      int grow = m0 + row;
      if (grow >= M) grow = M - 1;
      glds16(A + (size_t)grow * K + lk,
             dst + (size_t)(wave * A_INSTRS + i) * 8 * K);
    }
  };

  stage_a(0, mt0);
  for (int mt = mt0; mt < mt_end; ++mt) {
    int buf = (mt - mt0) & 1;
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (mt + 1 < mt_end) stage_a(buf ^ 1, mt + 1);

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const bf16* la = lds_a + buf * BM * K;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      int kbase = kk * 32 + (lane >> 4) * 8;
      bf16x8 afrag[FM], bfrag[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        int row = wrow * (BM / WM) + i * 16 + (lane & 15);
        afrag[i] =
            *reinterpret_cast<const bf16x8*>(la + (size_t)row * K + kbase);
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        int col = wcol * (BN / WN) + j * 16 + (lane & 15);
        bfrag[j] = *reinterpret_cast<const bf16x8*>(lds_b +
                                                    (size_t)col * K + kbase);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[i], bfrag[j], acc[i][j], 0, 0, 0);
    }

    // Coalesced store through dedicated per-wave scratch (lds_a/lds_b stay
    // live — the next tile's A prefetch is in flight right now, and the
    // wave-local lgkmcnt waits inside don't drain it). The residual reads
    // go out here, all at once, and not before the MFMAs: vmcnt retires in
    // order, so waiting for them also waits for the A prefetch issued
    // above, and that wait belongs after the MFMAs.
    bf16x8 res[FM][FN / 2] = {};
    if constexpr (RESIDUAL)
      load_residual<FM, FN>(res, residual, M, N, mt * BM, n0, wrow, wcol,
                            lane);
    epilogue_store<FM, FN, RELU, RESIDUAL>(
        acc, lds_ep + (size_t)wave * 16 * (BN / WN + 4), C, res, M, N,
        mt * BM, n0, wrow, wcol, lane, sc, bi);
    // No trailing barrier (see main kernel note): next iteration's leading
    // waitcnt+barrier is the only ordering needed, and keeping the A
    // prefetch un-drained across the epilogue is the whole point.
  }
}

// ---- split-K path ----
// For launch-bound shapes (few output tiles, deep K — e.g. ResNet stage-4
// conv2: M-tiles x N-tiles = 52 workgroups on a 256-CU chip, measured
// ~59 TF/s), S workgroup groups each compute a K-slice partial into f32
// scratch and a reduce kernel applies the epilogue. An OPT-IN fused
// variant (SCANNER_SPLITK_FUSED=1) instead has the LAST workgroup to
// finish a tile (tile-completion counter) reduce the partials in-kernel —
// G16-safe since no workgroup ever WAITS on another (each increments its
// tile's counter exactly once and exits; only the one observing
// count == splits-1 does the extra work) — but it measured 2.2x SLOWER on
// the flagship (see the kFused comment in try_splitk), so the separate
// reduce launch stays the default.
struct SplitkEp {
  unsigned int* counters = nullptr;  // null => unfused (write partials only)
  int splits = 0;
  const float* scale = nullptr;
  const float* bias = nullptr;
  const bf16* residual = nullptr;
  bf16* C = nullptr;
  int relu = 0;
};

// One float4 quad of each split's partial ([split][M][N], quad at element
// offset off). S > 0: the split count is a template argument and load()
// issues all S loads back to back (independent loads, one wait); a runtime
// loop of load-then-add is a chain of `splits` dependent HBM round trips.
// S == 0 keeps that runtime loop for split counts above 6
// (SCANNER_SPLITK_MAX). sum() adds in the fixed order every reduce variant
// shares, split 0 first, so they agree bit for bit.
template <int S>
struct SplitPartials {
  float4 p[S > 0 ? S : 1];
  const float* base;
  size_t stride;

  __device__ inline void load(const float* __restrict__ partials,
                              size_t split_stride, size_t off) {
    base = partials + off;
    stride = split_stride;
#pragma unroll
    for (int sp = 0; sp < S; ++sp)
      p[sp] = *reinterpret_cast<const float4*>(base + sp * stride);
  }

  __device__ inline float4 sum(int splits) const {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (S > 0) {
#pragma unroll
      for (int sp = 0; sp < S; ++sp) {
        acc.x += p[sp].x;
        acc.y += p[sp].y;
        acc.z += p[sp].z;
        acc.w += p[sp].w;
      }
    } else {
      for (int sp = 0; sp < splits; ++sp) {
        float4 v = *reinterpret_cast<const float4*>(base + sp * stride);
        acc.x += v.x;
        acc.y += v.y;
        acc.z += v.z;
        acc.w += v.w;
      }
    }
    return acc;
  }
};

// Epilogue operands of one output quad (4 consecutive columns of one row;
// N % 64 == 0, so a quad never straddles a row): one 16-byte load each for
// scale and bias, one 8-byte load for the residual, each behind a uniform
// test (has_res is a compile-time constant in the reduce kernels) and
// independent of everything else the thread loads. Callers issue their
// partial loads first, so one wait covers all of a quad's reads.
struct QuadOperands {
  float4 sc, bi;
  uint2 res;
};

__device__ inline QuadOperands load_quad_operands(
    const float* __restrict__ scale, const float* __restrict__ bias,
    const bf16* __restrict__ residual, bool has_res, int col, size_t off) {
  QuadOperands o;
  o.sc = make_float4(1.f, 1.f, 1.f, 1.f);
  o.bi = make_float4(0.f, 0.f, 0.f, 0.f);
  o.res = make_uint2(0u, 0u);
  if (scale) o.sc = *reinterpret_cast<const float4*>(scale + col);
  if (bias) o.bi = *reinterpret_cast<const float4*>(bias + col);
  if (has_res) o.res = *reinterpret_cast<const uint2*>(residual + off);
  return o;
}

// v * scale, + bias, + residual, ReLU, bf16 — as separate roundings (no
// fused multiply-add), which is what the split-K paths have always
// computed; one 8-byte store.
__device__ inline void store_quad(float4 a, const QuadOperands& o,
                                  bool has_scale, bool has_bias,
                                  bool has_res, bool relu,
                                  bf16* __restrict__ dst) {
#pragma clang fp contract(off)
  float v4[4] = {a.x, a.y, a.z, a.w};
  float s4[4] = {o.sc.x, o.sc.y, o.sc.z, o.sc.w};
  float b4[4] = {o.bi.x, o.bi.y, o.bi.z, o.bi.w};
  bf16 r4[4];
  *reinterpret_cast<uint2*>(r4) = o.res;
  bf16 o4[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v = v4[k];
    if (has_scale) v *= s4[k];
    if (has_bias) v += b4[k];
    if (has_res) v += bf16_to_f32(r4[k]);
    if (relu) v = v > 0.f ? v : 0.f;
    o4[k] = f32_to_bf16(v);
  }
  *reinterpret_cast<uint64_t*>(dst) = *reinterpret_cast<const uint64_t*>(o4);
}

template <int BM, int BN, int WM, int WN, bool IMPLICIT, bool FAST,
          bool ATOMIC>
__global__ void __launch_bounds__(256, 2)
    gemm_bf16_splitk_kernel(const bf16* __restrict__ A,
                            const bf16* __restrict__ B, int M, int N, int K,
                            int ksteps_per_split,
                            float* __restrict__ partials, ConvDesc d,
                            const bf16* __restrict__ zero, SplitkEp ep) {
  constexpr int BK = 64;
  constexpr int FM = BM / WM / 16;
  constexpr int FN = BN / WN / 16;
  __shared__ bf16 lds[2 * (BM + BN) * BK];

  int tid = threadIdx.x;
  int lane = tid & 63;
  int wave = tid >> 6;
  int wrow = wave / WN;
  int wcol = wave % WN;

  int ntiles_n = (N + BN - 1) / BN;
  int ntiles_m = (M + BM - 1) / BM;
  int tiles = ntiles_m * ntiles_n;
  int split = blockIdx.x / tiles;
  int tile = blockIdx.x % tiles;
  int m0 = (tile / ntiles_n) * BM;
  int n0 = (tile % ntiles_n) * BN;
  int ks_begin = split * ksteps_per_split;
  int ks_end = min(ks_begin + ksteps_per_split, K / BK);
  if (ks_begin >= ks_end) return;

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the same staging as the tile kernel, started at this split's first k
  TileStager<BM, BN, IMPLICIT, FAST> st;
  st.init(A, B, M, K, m0, n0, wave, lane, ks_begin * BK, d);

  st.issue(lds, wave, A, d, zero);
  for (int ks = ks_begin; ks < ks_end; ++ks) {
    int buf = (ks - ks_begin) & 1;
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (ks + 1 < ks_end) {
      st.advance(d);
      st.issue(lds + (buf ^ 1) * (BM + BN) * BK, wave, A, d, zero);
    }
    mfma_step<BM, BN, WM, WN>(acc, lds + buf * (BM + BN) * BK, wrow, wcol,
                              lane);
    // No trailing barrier, as in the tile kernel: the next iteration's
    // leading waitcnt+barrier comes before anything is staged into the
    // buffer read here, and a __syncthreads() at this point would drain
    // the in-flight LDS-DMA prefetch (vmcnt(0) in its fence) and cost a
    // second barrier per step. Nothing after the loop reuses the LDS
    // without a barrier of its own.
  }

  if constexpr (ATOMIC) {
    // Atomic split-K: all splits add into ONE pre-zeroed f32 [M][N]
    // buffer (f32 atomic adds are commutative — no inter-WG ordering,
    // G16-safe); a finalize kernel applies the epilogue. Vs the
    // partials+reduce pair this removes the S x M x N reduce read
    // (measured ~12% of all flagship GPU time).
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        int col = n0 + wcol * (BN / WN) + j * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = m0 + wrow * (BM / WM) + i * 16 + (lane >> 4) * 4 + r;
          if (row < M)
            atomicAdd(&partials[(size_t)row * N + col], acc[i][j][r]);
        }
      }
    }
  } else {
    // f32 partials: [split][M][N]; lanes 0-15 write 64-byte runs
    float* out = partials + (size_t)split * M * N;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        int col = n0 + wcol * (BN / WN) + j * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = m0 + wrow * (BM / WM) + i * 16 + (lane >> 4) * 4 + r;
          if (row < M) out[(size_t)row * N + col] = acc[i][j][r];
        }
      }
    }
    if (ep.counters) {
      // Fused reduce: release this split's partial (per-thread fence,
      // then a block barrier so tid 0's atomic is ordered after EVERY
      // thread's stores), count the tile's completions, and if this
      // workgroup is the last one, sum the partials in fixed split order
      // (bitwise identical to splitk_reduce_kernel) + epilogue + bf16
      // store. The counter is restored to 0 for the next launch that
      // reuses this scratch (launches on the stream are ordered, and
      // hipGraph replays see the same all-zero state).
      // The "last arriver" flag overlays the staging LDS (every wave is
      // past its last fragment read at the barrier below): a second
      // __shared__ object beside the LDS-DMA target makes hipcc wait
      // vmcnt(0) before the first ds_read of every K step, which drains
      // the prefetch just issued.
      __threadfence();
      __syncthreads();
      unsigned int& s_old = *reinterpret_cast<unsigned int*>(lds);
      if (tid == 0) s_old = atomicAdd(ep.counters + tile, 1u);
      __syncthreads();
      if (s_old != (unsigned int)ep.splits - 1) return;
      __threadfence();  // acquire: other splits' partials now visible
      int rows = min(BM, M - m0);
      constexpr int Q = BN / 4;  // float4 quads per tile row
      const size_t mn = (size_t)M * N;
      for (int idx = tid; idx < rows * Q; idx += 256) {
        int r = idx / Q, q = idx - r * Q;
        size_t base = (size_t)(m0 + r) * N + n0 + q * 4;
        auto finish = [&](auto nsplit) {
          SplitPartials<decltype(nsplit)::value> sp;
          sp.load(partials, mn, base);
          QuadOperands o =
              load_quad_operands(ep.scale, ep.bias, ep.residual,
                                 ep.residual != nullptr, n0 + q * 4, base);
          store_quad(sp.sum(ep.splits), o, ep.scale != nullptr,
                     ep.bias != nullptr, ep.residual != nullptr,
                     ep.relu != 0, ep.C + base);
        };
        switch (ep.splits) {
          case 2: finish(std::integral_constant<int, 2>{}); break;
          case 3: finish(std::integral_constant<int, 3>{}); break;
          case 4: finish(std::integral_constant<int, 4>{}); break;
          case 5: finish(std::integral_constant<int, 5>{}); break;
          case 6: finish(std::integral_constant<int, 6>{}); break;
          default: finish(std::integral_constant<int, 0>{});
        }
      }
      if (tid == 0) ep.counters[tile] = 0;
    }
  }
}

// Quad index -> column without 64-bit division: one 32-bit modulo for the
// thread's first quad (the grid is at most 4096 x 256 threads, so it fits
// 32 bits whatever mn is), then an add and a conditional subtract per
// grid stride.
struct QuadColumn {
  unsigned nq, cq, cstep;
  __device__ inline QuadColumn(int N) {
    nq = (unsigned)N / 4;
    unsigned gs = gridDim.x * blockDim.x;
    cq = (blockIdx.x * blockDim.x + threadIdx.x) % nq;
    cstep = gs % nq;
  }
  __device__ inline int col() const { return (int)(cq * 4); }
  __device__ inline void next() {
    cq += cstep;
    if (cq >= nq) cq -= nq;
  }
};

template <bool RELU, bool RESIDUAL>
__global__ void __launch_bounds__(256)
    splitk_finalize_kernel(const float* __restrict__ acc, i64 mn, int N,
                           const float* __restrict__ scale,
                           const float* __restrict__ bias,
                           const bf16* __restrict__ residual,
                           bf16* __restrict__ C) {
  i64 quads = mn / 4;
  i64 gs = (i64)gridDim.x * blockDim.x;
  QuadColumn qc(N);
  for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < quads;
       q += gs, qc.next()) {
    i64 i = q * 4;
    float4 a4 = reinterpret_cast<const float4*>(acc)[q];
    QuadOperands o = load_quad_operands(scale, bias, residual, RESIDUAL,
                                        qc.col(), (size_t)i);
    store_quad(a4, o, scale != nullptr, bias != nullptr, RESIDUAL, RELU,
               C + i);
  }
}

// S: the split count when it is 2..6 (all partial loads independent), 0
// for a runtime count (see SplitPartials). The grid covers every quad of a
// split shape in one pass (tiles < 256 bounds mn below 4096 x 256 x 4),
// so the grid-stride loop runs once; it stays for safety.
template <bool RELU, bool RESIDUAL, int S>
__global__ void __launch_bounds__(256)
    splitk_reduce_kernel(const float* __restrict__ partials, int splits,
                         i64 mn, int N, const float* __restrict__ scale,
                         const float* __restrict__ bias,
                         const bf16* __restrict__ residual,
                         bf16* __restrict__ C) {
  // 4 elements per thread via float4 (N is a multiple of 64, so mn % 4 ==
  // 0 and every row stays 16-byte aligned): the scalar version measured
  // only ~2.2 TB/s on S x M x N partial streams.
  i64 quads = mn / 4;
  i64 gs = (i64)gridDim.x * blockDim.x;
  QuadColumn qc(N);
  for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < quads;
       q += gs, qc.next()) {
    i64 i = q * 4;
    SplitPartials<S> sp;
    sp.load(partials, (size_t)mn, (size_t)i);
    QuadOperands o = load_quad_operands(scale, bias, residual, RESIDUAL,
                                        qc.col(), (size_t)i);
    store_quad(sp.sum(splits), o, scale != nullptr, bias != nullptr,
               RESIDUAL, RELU, C + i);
  }
}

const bf16* device_zero_chunk();

// TileStager's FAST mode: every 64-wide K step lies inside one (r, s)
// cell, one validity bit per tap fits a 32-bit word, and K has no padded
// tail.
bool conv_fast_path(const ConvDesc& d, int K) {
  return d.c % 64 == 0 && d.r * d.s <= 32 && K == d.r * d.s * d.c;
}

constexpr size_t kSplitkCtrBytes = 4096;  // tile counters at the scratch tail

// Split-K decision (the launch below follows it verbatim). Returns false
// when the shape should not split.
bool plan_splitk(int M, int N, int K, size_t scratch_bytes, GemmPlan& p) {
  constexpr int BM = 128, BN = 128;
  // SCANNER_SPLITK_OFF=1: skip split-K entirely (A/B: with multiple
  // pipeline instances co-running, their kernels may fill the chip
  // without paying the partial+reduce HBM traffic).
  static const bool kOff = []() {
    const char* e = std::getenv("SCANNER_SPLITK_OFF");
    return e && e[0] == '1';
  }();
  if (kOff) return false;
  if (!scratch_bytes || N % BN != 0 || K < 1024) return false;
  int ntiles_m = (M + BM - 1) / BM;
  int tiles = ntiles_m * (N / BN);
  if (tiles >= 256) return false;  // already fills the chip
  static const int kMaxSplits = []() {
    const char* e = std::getenv("SCANNER_SPLITK_MAX");
    // A/B on the flagship: 6 > 8 > 16 (18.0k / 17.95k / 15.4k f/s) —
    // fewer splits cut the partial+reduce HBM traffic and the chip stays
    // fed by the co-running pipeline instances.
    return e ? std::max(2, atoi(e)) : 6;
  }();
  int ksteps = K / 64;
  int want = std::min({kMaxSplits, ksteps / 4, (2048 + tiles - 1) / tiles});
  size_t per_split = (size_t)M * N * 4;
  // The scratch tail holds the fused-reduce tile counters (tiles < 256 so
  // 4 KB is ample); the owner zeroes it once at allocation
  // (splitk_scratch_init) and the kernel self-restores it after each use.
  size_t avail = scratch_bytes > kSplitkCtrBytes
                     ? scratch_bytes - kSplitkCtrBytes
                     : 0;
  int fit = (int)(avail / per_split);
  int splits = std::min(want, fit);
  if (splits < 2) return false;
  int ksteps_per_split = (ksteps + splits - 1) / splits;
  splits = (ksteps + ksteps_per_split - 1) / ksteps_per_split;
  // Atomic accumulation (opt-in, SCANNER_SPLITK_ATOMIC=1): one pre-zeroed
  // f32 [M][N] buffer, no S x M x N reduce read — but f32 atomic-add
  // ORDER is nondeterministic, so results vary at the last bf16 ulp
  // between runs. The default stays the deterministic partials+reduce
  // pair (run-to-run reproducibility is a framework property our own
  // regression tests rely on).
  static const bool kAtomic = []() {
    const char* e = std::getenv("SCANNER_SPLITK_ATOMIC");
    return e && e[0] == '1';
  }();
  // Fused reduce (opt-in, SCANNER_SPLITK_FUSED=1; default OFF). Measured
  // NEGATIVE on MI355X: flagship 7.6k vs 16.6k f/s, resnet 7.9k vs 18.0k
  // (same box, 3-step A/B, profiles/r02_results.md update 12). Numerics
  // are correct (tests/test_dnn_kernels_gpu.py holds it bit-equal to the
  // default path), but the device-scope release fence every workgroup
  // needs before bumping its tile counter
  // forces an L2 writeback per WG — on 8 per-XCD L2s that evicts the
  // B-operand and co-running instances' working sets — and the tail
  // reduce runs with one 256-thread WG per tile vs the standalone
  // kernel's chip-wide parallelism. Kept as a documented experiment; the
  // separate splitk_reduce_kernel launch is the default.
  static const bool kFused = []() {
    const char* e = std::getenv("SCANNER_SPLITK_FUSED");
    return e && e[0] == '1';
  }();
  p.kernel = GemmKernel::SplitK;
  p.splits = splits;
  p.ksteps_per_split = ksteps_per_split;
  p.grid = tiles * splits;
  p.atomic = kAtomic;
  p.fused = kFused && !kAtomic;
  return true;
}

void launch_splitk(const GemmArgs& g, hipStream_t s, const GemmPlan& p,
                   const ConvDesc* dd = nullptr) {
  constexpr int BM = 128, BN = 128;
  const int splits = p.splits;
  const int ksteps_per_split = p.ksteps_per_split;
  const int grid_main = p.grid;
  const bool kAtomic = p.atomic;
  const bool fused = p.fused;
  i64 mn = (i64)g.M * g.N;
  SplitkEp ep{};
  if (fused) {
    ep.counters = reinterpret_cast<unsigned int*>(
        (u8*)g.splitk_scratch + g.splitk_scratch_bytes - kSplitkCtrBytes);
    ep.splits = splits;
    ep.scale = g.scale;
    ep.bias = g.bias;
    ep.residual = (const bf16*)g.residual;
    ep.C = (bf16*)g.C;
    ep.relu = g.relu ? 1 : 0;
  }
  hipError_t e;
  if (kAtomic) {
    e = hipMemsetAsync(g.splitk_scratch, 0, (size_t)mn * 4, s);
    if (e != hipSuccess) {
      throw ScannerError(std::string("splitk memset failed: ") +
                         hipGetErrorString(e));
    }
  }
  auto main_kernel = [&](auto implicit, auto fast, auto atomic) {
    constexpr bool kImplicit = decltype(implicit)::value;
    gemm_bf16_splitk_kernel<BM, BN, 2, 2, kImplicit, decltype(fast)::value,
                            decltype(atomic)::value>
        <<<grid_main, 256, 0, s>>>(
            (const bf16*)g.A, (const bf16*)g.B, g.M, g.N, g.K,
            ksteps_per_split, (float*)g.splitk_scratch,
            kImplicit ? *dd : ConvDesc{},
            kImplicit ? device_zero_chunk() : nullptr,
            decltype(atomic)::value ? SplitkEp{} : ep);
  };
  auto by_atomic = [&](auto implicit, auto fast) {
    if (kAtomic)
      main_kernel(implicit, fast, std::true_type{});
    else
      main_kernel(implicit, fast, std::false_type{});
  };
  if (!dd)
    by_atomic(std::false_type{}, std::false_type{});
  else if (conv_fast_path(*dd, g.K))
    by_atomic(std::true_type{}, std::true_type{});
  else
    by_atomic(std::true_type{}, std::false_type{});
  e = hipGetLastError();
  if (e != hipSuccess) {
    throw ScannerError(std::string("splitk launch failed: ") +
                       hipGetErrorString(e));
  }
  if (fused) return;  // epilogue ran in-kernel; no reduce launch
  // 4x more threads than quads: the extra waves are pure memory-level
  // parallelism for this latency-bound pass (measured 18.2 us avg vs a
  // ~1.3 us bandwidth bound)
  int grid = (int)std::min<i64>(4096, (mn + 255) / 256);
  auto disp = [&](auto relu, auto res) {
    if (kAtomic) {
      splitk_finalize_kernel<decltype(relu)::value, decltype(res)::value>
          <<<grid, 256, 0, s>>>((const float*)g.splitk_scratch, mn, g.N,
                                g.scale, g.bias, (const bf16*)g.residual,
                                (bf16*)g.C);
    } else {
      auto reduce = [&](auto nsplit) {
        splitk_reduce_kernel<decltype(relu)::value, decltype(res)::value,
                             decltype(nsplit)::value>
            <<<grid, 256, 0, s>>>((const float*)g.splitk_scratch, splits, mn,
                                  g.N, g.scale, g.bias,
                                  (const bf16*)g.residual, (bf16*)g.C);
      };
      switch (splits) {
        case 2: reduce(std::integral_constant<int, 2>{}); break;
        case 3: reduce(std::integral_constant<int, 3>{}); break;
        case 4: reduce(std::integral_constant<int, 4>{}); break;
        case 5: reduce(std::integral_constant<int, 5>{}); break;
        case 6: reduce(std::integral_constant<int, 6>{}); break;
        default: reduce(std::integral_constant<int, 0>{});  // runtime count
      }
    }
  };
  if (g.relu && g.residual)
    disp(std::true_type{}, std::true_type{});
  else if (g.relu)
    disp(std::true_type{}, std::false_type{});
  else if (g.residual)
    disp(std::false_type{}, std::true_type{});
  else
    disp(std::false_type{}, std::false_type{});
  e = hipGetLastError();
  if (e != hipSuccess) {
    throw ScannerError(std::string("splitk reduce launch failed: ") +
                       hipGetErrorString(e));
  }
}

void plan_smallk(int M, int N, GemmPlan& p) {
  constexpr int BM = 128, BN = 128;
  int ntiles_m = (M + BM - 1) / BM;
  int ntiles_n = (N + BN - 1) / BN;
  // Enough strips to fill the chip (>=2048 workgroups when the shape
  // allows), each walking a run of consecutive M-tiles.
  static const int target_wgs = []() {
    const char* e = std::getenv("SCANNER_SMALLK_WGS");
    return e ? std::max(256, atoi(e)) : 2048;
  }();
  int strips = std::max(1, std::min(ntiles_m, target_wgs / ntiles_n));
  int tiles_per_wg = (ntiles_m + strips - 1) / strips;
  strips = (ntiles_m + tiles_per_wg - 1) / tiles_per_wg;
  p.kernel = GemmKernel::SmallK;
  p.tiles_per_wg = tiles_per_wg;
  p.grid = strips * ntiles_n;
}

void launch_smallk(const GemmArgs& g, hipStream_t s, const GemmPlan& p) {
  constexpr int BM = 128, BN = 128;
  const int grid = p.grid;
  const int tiles_per_wg = p.tiles_per_wg;
  auto disp = [&](auto relu, auto res) {
    gemm_bf16_smallk_kernel<BM, BN, 2, 2, decltype(relu)::value,
                            decltype(res)::value><<<grid, 256, 0, s>>>(
        (const bf16*)g.A, (const bf16*)g.B, (bf16*)g.C, g.M, g.N, g.scale,
        g.bias, (const bf16*)g.residual, tiles_per_wg);
  };
  if (g.relu && g.residual)
    disp(std::true_type{}, std::true_type{});
  else if (g.relu)
    disp(std::true_type{}, std::false_type{});
  else if (g.residual)
    disp(std::false_type{}, std::true_type{});
  else
    disp(std::false_type{}, std::false_type{});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    throw ScannerError(std::string("gemm smallk launch failed: ") +
                       hipGetErrorString(e));
  }
}

template <int BM, int BN, int WM, int WN>
void launch_variant(const GemmArgs& g, hipStream_t s, const GemmPlan& p) {
  const int grid = p.grid;
  auto disp = [&](auto relu, auto res) {
    gemm_bf16_kernel<BM, BN, WM, WN, decltype(relu)::value,
                     decltype(res)::value, false, false>
        <<<grid, 256, 0, s>>>(
        (const bf16*)g.A, (const bf16*)g.B, (bf16*)g.C, g.M, g.N, g.K,
        g.scale, g.bias, (const bf16*)g.residual, ConvDesc{}, nullptr);
  };
  if (g.relu && g.residual)
    disp(std::true_type{}, std::true_type{});
  else if (g.relu)
    disp(std::true_type{}, std::false_type{});
  else if (g.residual)
    disp(std::false_type{}, std::true_type{});
  else
    disp(std::false_type{}, std::false_type{});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    throw ScannerError(std::string("gemm launch failed: ") +
                       hipGetErrorString(e));
  }
}

// 16+ zero bytes in device memory for implicit-conv padding lanes; one
// per device, allocated outside the pool so memory teardown cycles never
// invalidate it.
const bf16* device_zero_chunk() {
  static std::mutex mu;
  static std::map<int, bf16*> per_dev;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> l(mu);
  auto it = per_dev.find(dev);
  if (it != per_dev.end()) return it->second;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, 256);
  if (e != hipSuccess || hipMemset(p, 0, 256) != hipSuccess) {
    throw ScannerError("failed to allocate implicit-conv zero chunk");
  }
  per_dev[dev] = (bf16*)p;
  return (bf16*)p;
}

template <int BM, int BN, int WM, int WN>
void launch_conv_variant(const GemmArgs& g, const ConvDesc& d,
                         hipStream_t s, const GemmPlan& p) {
  const int grid = p.grid;
  const bf16* zero = device_zero_chunk();
  const bool fast = conv_fast_path(d, g.K);
  auto launch = [&](auto relu, auto res, auto fast_t) {
    gemm_bf16_kernel<BM, BN, WM, WN, decltype(relu)::value,
                     decltype(res)::value, true, decltype(fast_t)::value>
        <<<grid, 256, 0, s>>>(
            (const bf16*)g.A, (const bf16*)g.B, (bf16*)g.C, g.M, g.N, g.K,
            g.scale, g.bias, (const bf16*)g.residual, d, zero);
  };
  auto disp = [&](auto relu, auto res) {
    if (fast)
      launch(relu, res, std::true_type{});
    else
      launch(relu, res, std::false_type{});
  };
  if (g.relu && g.residual)
    disp(std::true_type{}, std::true_type{});
  else if (g.relu)
    disp(std::true_type{}, std::false_type{});
  else if (g.residual)
    disp(std::false_type{}, std::true_type{});
  else
    disp(std::false_type{}, std::false_type{});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    throw ScannerError(std::string("conv gemm launch failed: ") +
                       hipGetErrorString(e));
  }
}

}  // namespace

GemmPlan gemm_plan(int M, int N, int K, size_t scratch_bytes, bool is_conv) {
  SCA_CHECK(K % 64 == 0 && N % 64 == 0, "gemm K/N must be x64");
  GemmPlan p;
  p.ksteps_per_split = K / 64;
  if (!is_conv && K == 64 && N % 128 == 0 && M >= 1024) {
    plan_smallk(M, N, p);
    return p;
  }
  if (plan_splitk(M, N, K, scratch_bytes, p)) return p;
  // the implicit-conv path has no M > 64 condition
  bool big = N % 128 == 0 && (is_conv || M > 64);
  int bt = big ? 128 : 64;
  p.kernel = big ? GemmKernel::Tile128 : GemmKernel::Tile64;
  p.grid = ((M + bt - 1) / bt) * (N / bt);
  p.swizzle = p.grid % 8 == 0;
  return p;
}

void conv_gemm_bf16(const GemmArgs& g, const ConvDesc& d, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  SCA_CHECK(g.K % 64 == 0 && g.N % 64 == 0, "conv gemm K/N must be x64");
  SCA_CHECK(d.c % 8 == 0, "implicit conv needs c % 8 == 0");
  SCA_CHECK(g.M == d.n * d.oh * d.ow, "conv gemm M mismatch");
  GemmPlan p = gemm_plan(g.M, g.N, g.K,
                         g.splitk_scratch ? g.splitk_scratch_bytes : 0, true);
  switch (p.kernel) {
    case GemmKernel::SplitK:
      launch_splitk(g, s, p, &d);
      break;
    case GemmKernel::Tile128:
      launch_conv_variant<128, 128, 2, 2>(g, d, s, p);
      break;
    case GemmKernel::Tile64:
      launch_conv_variant<64, 64, 2, 2>(g, d, s, p);
      break;
    case GemmKernel::SmallK:
      SCA_CHECK(false, "conv gemm has no small-K path");
  }
}

void splitk_scratch_init(void* scratch, size_t bytes, void* stream) {
  if (!scratch || bytes < 4096) return;
  u8* tail = (u8*)scratch + bytes - 4096;
  hipError_t e = stream
                     ? hipMemsetAsync(tail, 0, 4096, (hipStream_t)stream)
                     : hipMemset(tail, 0, 4096);
  SCA_CHECK(e == hipSuccess, "splitk_scratch_init memset failed");
}

void gemm_bf16(const GemmArgs& g, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  SCA_CHECK(g.K % 64 == 0, "gemm K must be a multiple of 64");
  SCA_CHECK(g.N % 64 == 0, "gemm N must be a multiple of 64");
  GemmPlan p = gemm_plan(g.M, g.N, g.K,
                         g.splitk_scratch ? g.splitk_scratch_bytes : 0, false);
  switch (p.kernel) {
    case GemmKernel::SmallK:
      launch_smallk(g, s, p);
      break;
    case GemmKernel::SplitK:
      launch_splitk(g, s, p);
      break;
    case GemmKernel::Tile128:
      launch_variant<128, 128, 2, 2>(g, s, p);
      break;
    case GemmKernel::Tile64:
      launch_variant<64, 64, 2, 2>(g, s, p);
      break;
  }
}

}  // namespace sca
