// What the LDS-DMA implicit GEMMs share between their two numerics: conv_igemm2.hip (bf16 / f16 storage, one MFMA per product) and
// conv_igemm_x3.hip (float32 storage, f16x3 matrix math).  The pipeline around the MFMA loop is one design (conv_igemm2.hip's header
// describes it); the MFMA loop bodies, the epilogues, the ticketed split-K finish and the fused bin head differ and stay in their files.
// So do the operand loaders (row bookkeeping, im2col position, issue()): shared as a struct they compiled to other schedules -- issue() as a
// method to more registers, the set-up alone to slower launches (profiles/igemm_shared_core_ab.txt, sections 2b and 4b).
// What lives here, once:
//   * IGEMM_VARIANTS            the variant ids of both kernels (tile, stages, K groups, wave layouts, the f16x3-only flags)
//   * igemm_lds_bytes, igemm_tiles, igemm_launch     the host side of a launch
//   * IgemmTile / igemm_tile    blockIdx -> (row tile, first channel, row range, split, K-step range, per-image weight offset)
//   * kg_exchange, store_slab   the accumulator exchange of the two K groups, the float32 slab store of the split-K form
// (wait_stage, the counted wait in front of a stage, is in lds_dma.h: the halo kernels use it too.)
#pragma once
#include "igemm_core.h"
#include "lds_dma.h"

// ---- variants -------------------------------------------------------------------------------------------------------------------------
// X(id, BM, BN, STAGES, KG, 16-bit WM, WN, f16x3 WM, WN, AD, OCC).  Ids 0-21 exist in both kernels (the plan function is shared); the wave
// layouts differ where the f16x3 kernel wants a wave's A rows private (4 x 1: every A element is split once).  KG = 2: eight waves, two K
// groups.  AD: A-direct loop.  OCC > 0: compiled for that many waves per SIMD (conv_igemm_x3.hip).
#define IGEMM_VARIANTS(X)                                                                                                              \
  X(0, 128, 128, 3, 1, 2, 2, 2, 2, false, 0)                                                                                           \
  X(1, 128, 128, 2, 1, 2, 2, 2, 2, false, 0)                                                                                           \
  X(2, 128, 64, 3, 1, 2, 2, 4, 1, false, 0)                                                                                            \
  X(3, 128, 64, 4, 1, 2, 2, 4, 1, false, 0)                                                                                            \
  X(4, 64, 64, 3, 1, 2, 2, 4, 1, false, 0)                                                                                             \
  X(5, 64, 64, 4, 1, 2, 2, 4, 1, false, 0)                                                                                             \
  X(6, 256, 32, 3, 1, 4, 1, 4, 1, false, 0)                                                                                            \
  X(7, 256, 32, 2, 1, 4, 1, 4, 1, false, 0)                                                                                            \
  X(8, 128, 32, 3, 1, 4, 1, 4, 1, false, 0)                                                                                            \
  X(9, 128, 32, 4, 1, 4, 1, 4, 1, false, 0)                                                                                            \
  X(10, 256, 16, 2, 1, 4, 1, 4, 1, false, 0)                                                                                           \
  X(11, 128, 16, 4, 1, 4, 1, 4, 1, false, 0)                                                                                           \
  X(12, 64, 128, 3, 1, 2, 2, 2, 2, false, 0)                                                                                           \
  X(13, 64, 64, 2, 1, 2, 2, 4, 1, false, 0)                                                                                            \
  X(14, 128, 64, 2, 1, 2, 2, 4, 1, false, 0)                                                                                           \
  X(15, 64, 128, 2, 1, 2, 2, 2, 2, false, 0)                                                                                           \
  X(16, 128, 32, 2, 1, 4, 1, 4, 1, false, 0)                                                                                           \
  /* 17, 18: few-row / long-K problems with per-image weights (the squeeze-excite project GEMMs at 1/32: 300 rows per image): twice */ \
  /* the workgroups of the 64-row tiles, so that 8 images x 232 channels fill the chip */                                              \
  X(17, 32, 64, 3, 1, 1, 4, 1, 4, false, 0)                                                                                            \
  X(18, 32, 128, 3, 1, 1, 4, 1, 4, false, 0)                                                                                           \
  /* 19-21: two K groups (eight waves): long-K launches of a few hundred tiles */                                                      \
  X(19, 64, 64, 2, 2, 2, 2, 4, 1, false, 0)                                                                                            \
  X(20, 64, 64, 3, 2, 2, 2, 4, 1, false, 0)                                                                                            \
  X(21, 64, 128, 2, 2, 2, 2, 2, 2, false, 0)
// f16x3 only (no 16-bit wave layout).  22-27: larger row tiles (fewer L2 -> LDS bytes per MFMA) and the other wave layouts of the common
// shapes.  28-33: A-direct, 4 x 1 waves, the A values go global -> registers and only the W tile through LDS.  34-36: ids 13 / 16 / 15
// compiled for 4 / 4 / 3 waves per SIMD (in-flight plans; the same arithmetic in the same order).
#define IGEMM_VARIANTS_X3_ONLY(X)                                                                                                      \
  X(22, 256, 128, 2, 1, 0, 0, 2, 2, false, 0)                                                                                          \
  X(23, 256, 64, 2, 1, 0, 0, 4, 1, false, 0)                                                                                           \
  X(24, 64, 64, 2, 1, 0, 0, 2, 2, false, 0)                                                                                            \
  X(25, 128, 64, 2, 1, 0, 0, 2, 2, false, 0)                                                                                           \
  X(26, 128, 128, 2, 1, 0, 0, 4, 1, false, 0)                                                                                          \
  X(27, 64, 128, 2, 1, 0, 0, 4, 1, false, 0)                                                                                           \
  X(28, 128, 128, 2, 1, 0, 0, 4, 1, true, 0)                                                                                           \
  X(29, 128, 64, 2, 1, 0, 0, 4, 1, true, 0)                                                                                            \
  X(30, 64, 64, 2, 1, 0, 0, 4, 1, true, 0)                                                                                             \
  X(31, 256, 64, 2, 1, 0, 0, 4, 1, true, 0)                                                                                            \
  X(32, 128, 32, 2, 1, 0, 0, 4, 1, true, 0)                                                                                            \
  X(33, 256, 128, 2, 1, 0, 0, 4, 1, true, 0)                                                                                           \
  X(34, 64, 64, 2, 1, 0, 0, 4, 1, false, 4)                                                                                            \
  X(35, 128, 32, 2, 1, 0, 0, 4, 1, false, 4)                                                                                           \
  X(36, 64, 128, 2, 1, 0, 0, 2, 2, false, 3)

struct IgemmCfg { int bm, bn, stages; };
#define IGEMM_CFG_ROW(id, BM, BN, STAGES, ...) {BM, BN, STAGES},
constexpr IgemmCfg kIgemmCfg[] = {IGEMM_VARIANTS(IGEMM_CFG_ROW) IGEMM_VARIANTS_X3_ONLY(IGEMM_CFG_ROW)};
#undef IGEMM_CFG_ROW
#define IGEMM_COUNT_ROW(...) +1
constexpr int kNumIgemmCfg16 = 0 IGEMM_VARIANTS(IGEMM_COUNT_ROW);      // the ids both kernels have come first
constexpr int kNumIgemmCfgX3 = kNumIgemmCfg16 IGEMM_VARIANTS_X3_ONLY(IGEMM_COUNT_ROW);
#undef IGEMM_COUNT_ROW
static_assert(kNumIgemmCfgX3 == sizeof(kIgemmCfg) / sizeof(kIgemmCfg[0]) && kNumIgemmCfg16 == 22 && kNumIgemmCfgX3 == 37, "variant ids are public (cfp_debug_set, plans)");

// ---- host side ------------------------------------------------------------------------------------------------------------------------
constexpr size_t kIgemmLdsMax = 160 * 1024;
// LDS bytes of a workgroup: KG groups x STAGES stages of 128-byte rows, BM of A (none in the A-direct loop) and BN of W
constexpr size_t igemm_lds_bytes(int bm, int bn, int stages, int kg, bool ad) { return (size_t)kg * stages * ((ad ? 0 : bm) + bn) * 128; }
inline long long igemm_tiles(const ConvP& p, int bm, int bn) {
  const long long tiles_m = p.rows_per_batch > 0 ? (long long)p.B * cdiv(p.rows_per_batch, bm) : cdiv(p.M, bm);
  return tiles_m * cdiv(p.Cout, bn);
}
// Launch KERNEL(args...) on `wgs` workgroups with `lds` bytes of dynamic LDS; the attribute that lifts the 64 KB limit is set once per
// instantiation.  0, or -2 = the attribute call failed.
template <auto KERNEL, typename... Args> int igemm_launch(long long wgs, int threads, size_t lds, hipStream_t s, Args... args) {
  static bool attr = false;
  if (!attr) { if (hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kIgemmLdsMax) != hipSuccess) return -2; attr = true; }
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)wgs), dim3(threads), lds, s, args...);
  return 0;
}

// ---- device side ----------------------------------------------------------------------------------------------------------------------
struct IgemmTile {
  int tile, tile_m, n0;      // output tile (the split index taken off), its row tile, its first output channel
  int m0, m_end;             // rows [m0, min(m0 + BM, m_end)): `rows_per_batch > 0` keeps a tile inside one image
  int sp, k0, k1;            // split index and its K-steps [k0, k1) of the nk_all
  long long w_off;           // elements from p.w to this image's weights (p.w_bstride per image)
};
template <int BM, int BN, bool SPLITK> __device__ __forceinline__ IgemmTile igemm_tile(const ConvP& p, int splits, int nk_all) {
  IgemmTile t;
  const int tiles_n = (p.Cout + BN - 1) / BN;
  int bid = xcd_remap(blockIdx.x, gridDim.x);   // an XCD's L2 sees a contiguous run of tiles (shared A rows / halos / weights)
  t.sp = 0;
  if constexpr (SPLITK) { t.sp = bid % splits; bid /= splits; }
  t.tile = bid;
  t.n0 = (bid % tiles_n) * BN;
  t.tile_m = bid / tiles_n;
  if (p.rows_per_batch > 0) {
    const int tpb = (p.rows_per_batch + BM - 1) / BM;
    const int b = t.tile_m / tpb;
    t.m0 = b * p.rows_per_batch + (t.tile_m % tpb) * BM;
    t.m_end = (b + 1) * p.rows_per_batch;
    t.w_off = (long long)b * p.w_bstride;
  } else {
    t.m0 = t.tile_m * BM;
    t.m_end = p.M;
    t.w_off = 0;
  }
  t.k0 = 0; t.k1 = nk_all;
  if constexpr (SPLITK) {
    const int per = (nk_all + splits - 1) / splits;
    t.k0 = t.sp * per;
    t.k1 = min(nk_all, t.k0 + per);
  }
  return t;
}

// KG == 2: the second group's accumulators travel through LDS (float32, lane-contiguous 16-byte pieces) and are added by the first.  Every
// wave must be done with the operand stages (a barrier before the call); the exchange area is not free again before the caller's next barrier.
template <int TM, int TN> __device__ __forceinline__ void kg_exchange(f32x4 (&acc)[TM][TN], unsigned char* smem, int kg, int wave, int lane) {
  f32x4* xch = reinterpret_cast<f32x4*>(smem) + wave * (TM * TN * 64) + lane;
  if (kg == 1) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) xch[(i * TN + j) * 64] = acc[i][j];
  }
  __syncthreads();
  if (kg == 0) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const f32x4 o = xch[(i * TN + j) * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] += o[r];
      }
  }
}

// The split-K form's float32 slab store: the accumulators are held transposed (weights as the MFMA's row operand), so a lane owns four
// consecutive output channels n_base + j * 16 + 4 fq .. of pixel row m_base + i * 16 + fr: 16-byte stores (Cout % 4 == 0).
template <int TM, int TN>
__device__ __forceinline__ void store_slab(const f32x4 (&acc)[TM][TN], float* __restrict__ slab, int Cout, int m_base, int m_end, int n_base, int fr, int fq) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int m = m_base + i * 16 + fr;
      const int n = n_base + j * 16 + fq * 4;
      if (m < m_end && n < Cout) *reinterpret_cast<f32x4*>(slab + (long long)m * Cout + n) = acc[i][j];
    }
}
