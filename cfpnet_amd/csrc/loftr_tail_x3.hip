// Fused tail of a LoFTR encoder layer (transformer.py:45-71, attention.py:48-49) in the DEFAULT numerics of the drop-in boundary: float32
// tensors, every GEMM of the chain as A_hi W_hi + A_hi W_lo + A_lo W_hi on v_mfma_f32_16x16x32_f16 (conv_igemm_x3.hip has the arithmetic).
//
//   q   = x @ Wq^T                                        q projection of this wave's own rows (transformer.py:45)
//   msg = (elu1(q) KV[g]) / (elu1(q) . Ksum[g] + eps) * S linear-attention apply, per head (float32 VALU)
//   y1  = LayerNorm1(msg @ Wm^T)                          merge + norm1
//   h   = relu([x | y1] @ W0^T)                           mlp.0
//   out = LayerNorm2(h @ W2^T) + x                        mlp.2 + norm2 + residual
//
// Unfused (the float32 mode's path, and this mode's until round 4) this is six launches per layer -- q GEMM, apply, merge GEMM + LayerNorm,
// mlp.0 GEMM, mlp.2 GEMM + LayerNorm -- 18 layers per forward: 72 of the 154 small f16x3 GEMM launches and the 24 attention-apply launches,
// 1.5 ms of the 5.1 ms step with four batches in flight (tools/ablate_time.py --x3).  Structure = loftr_tail.hip's (the 16-bit kernel): a wave
// owns 16 token rows from the projection to the final store, its tiles live in a private LDS region, only the weights are shared (LDS-DMA,
// 128-byte swizzled rows [hi(32) | lo(32)] of cfp_pack_w_x3's operand, double buffered, one barrier per 32-channel K-step).  Differences:
//   * the tiles are FLOAT32 (row pitch D + 8 floats = 2 (mod 4) sixteen-byte slots: the A-fragment reads of 16 rows are conflict-free);
//     a lane reads its two channel quads (4 fq .., 16 + 4 fq ..) of the K-step and splits them in registers -- one fragment per K-step
//     and wave (16 rows), ~20 VALU instructions beside 3 x NT MFMAs;
//   * mlp.0 / mlp.2 run in two halves of the hidden width: half of h (D channels) is produced, then consumed as a K range of mlp.2 into
//     accumulators that stay in registers -- the hidden tile is D wide instead of 2 D, so that four waves' tiles and the weight stages
//     fit the LDS at D = 128 (152 KB with the three weight stages);
//   * nothing is rounded on the way: msg, y1, h stay float32 (the unfused float32 path stores them in float32 as well).
#include "tail_core.h"

namespace {

// One GEMM of the chain for this wave's 16 rows: acc[j] += A[16 x 32 nks] * W[N x ..]^T over the K-steps [ks0, ks0 + nks) of the weight rows
// (N = NT * 16 rows starting at W, `wrow` halves per row).  `arow(ks)` returns the wave-private float32 row pointer (lane's row fr) of the
// A operand's 32 channels of K-step ks.  All four waves of the workgroup must call it together (they share the weight stages).
// Weight stages per kernel: three (two K-steps of DMA in flight) unless one fewer lets ANOTHER WORKGROUP share the CU -- these kernels run
// their phases (projection, attention apply, GEMM chain, LayerNorms) behind barriers, so a co-resident workgroup is what fills the gaps (the
// lesson of DESIGN.md 4.5): the LoFTR tail at D = 32 is 43 KB with three stages (three per CU) and 39 KB with two (four per CU; its GEMMs
// are one or two K-steps long anyway); the LKPM tail at D = 64 is 61 KB -> 53 KB (two -> three per CU).
template <int D> constexpr int tail_nst_loftr() { return D == 32 ? 2 : 3; }
template <int D> constexpr int tail_nst_lkpm() { return D == 64 ? 2 : 3; }
template <int NT, int BSTAGE, bool ZERO, int NST, int WAVES, typename AF>
__device__ __forceinline__ void tail_gemm_x3(f32x4 (&acc)[NT], const f16_t* __restrict__ W, int wrow, int ks0, int nks, AF arow, unsigned char* sB,
                                             int wave, int lane) {
  constexpr int N = NT * 16;
  constexpr int NBG = N / 8;                  // 8-row DMA groups of a weight stage
  constexpr int NBW = (NBG + WAVES - 1) / WAVES;      // LDS-DMA instructions per wave and stage
  static_assert(N * 128 <= BSTAGE, "weight stage");
  const int fr = lane & 15, fq = lane >> 4;
  const int rsub = lane >> 3;
  const int lc = (lane & 7) ^ rsub;
  if (ZERO) {
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int pc0 = ((fq) ^ (fr & 7)) * 16, pc1 = ((4 + fq) ^ (fr & 7)) * 16;
  auto issue = [&](int i, int st) {
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      const int g = (j * WAVES + wave) % NBG;
      const int n = g * 8 + rsub;
      glds16(W + (long long)n * wrow + ((ks0 + i) * 8 + lc) * 8, sB + st * BSTAGE + g * 1024);      // rows are zero-padded to whole K-steps
    }
  };
  tail_ring_begin<NST, NBW>(nks, issue);
  for (int i = 0; i < nks; ++i) {
    const unsigned char* cB = sB + tail_ring_step<NST, NBW>(i, nks, issue) * BSTAGE;
    const float* ar = arow(ks0 + i);
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(ar + 4 * fq);
    const f32x4 x1 = *reinterpret_cast<const f32x4*>(ar + 16 + 4 * fq);
    f16x8 ahi, alo;
    split8(x0, x1, ahi, alo);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const f16x8 bh = *reinterpret_cast<const f16x8*>(cB + (j * 16 + fr) * 128 + pc0);
      const f16x8 bl = *reinterpret_cast<const f16x8*>(cB + (j * 16 + fr) * 128 + pc1);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bh, acc[j], 0, 0, 0);      // acc[r] = row fq * 4 + r, column j * 16 + fr
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bl, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bh, acc[j], 0, 0, 0);
    }
  }
}

// WAVES (1, 2 or 4) waves of 16 token rows per workgroup.  Every wave reads the WHOLE weight tile of a K-step from LDS (16 KB at D = 128), so four
// waves share one LDS pipe for four times the bytes: the GEMM phases of the four-wave kernel are LDS-read bound (64 KB per step at 128 B / clk
// against 24 MFMAs per wave).  Few token rows (a single image: 19 four-wave workgroups at D = 128 on 256 CUs) therefore run as MORE, NARROWER
// workgroups -- each streams all the weights from L2 itself, which is cheap while the chip is mostly idle -- and many rows keep four waves
// (the weight stream is then shared by 64 rows).  Same arithmetic per row in every layout.
template <int D, int HEADS, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void loftr_tail_x3_kernel(TailP<float, f16_t> p) {
  constexpr int NT = D / 16;
  constexpr int PA = D + 8;                                // row pitch in floats: (D + 8) / 4 = 2 (mod 4) sixteen-byte slots
  constexpr int TILE = 16 * PA;                            // floats per tile
  constexpr int WAVE_LDS = 3 * TILE * 4;                   // msg / y1 | x | q / h-half tiles of one wave
  constexpr int BSTAGE = D * 128;                          // weight stage: [D rows][hi(32) | lo(32)]
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  constexpr int NST = tail_nst_loftr<D>();
  unsigned char* sB = smem;
  float* tMsg = reinterpret_cast<float*>(smem + NST * BSTAGE + wave * WAVE_LDS);
  float* tX = tMsg + TILE;
  float* tH = tX + TILE;
  const long long row0 = (long long)blockIdx.x * (16 * WAVES) + wave * 16;
  constexpr int wrow1 = (D / 32) * 64, wrow2 = (2 * D / 32) * 64;      // halves per packed weight row for K = D and K = 2 D

  // ---- x tile -> LDS (16-byte vectors) ------------------------------------------------------------------------------------------
  tail_tile_load<float, D, PA>(tX, p.x, p.x_ld, row0, p.rows, lane);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- optional q projection for this wave's rows -----------------------------------------------------------------------------------
  const bool own_q = p.wq != nullptr;
  if (own_q) {
    f32x4 acc[NT];
    tail_gemm_x3<NT, BSTAGE, true, NST, WAVES>(acc, p.wq, wrow1, 0, D / 32, [&](int ks) { return tX + fr * PA + ks * 32; }, sB, wave, lane);
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) tH[(fq * 4 + r) * PA + j * 16 + fr] = acc[j][r];      // the hidden tile is free until mlp.0
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }

  // ---- linear-attention apply: lane = (row, head slot) ------------------------------------------------------------------------------
  tail_attn_apply<float, D, HEADS, PA, PA>(p, row0, tH, tMsg, fr, fq);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- merge + norm1 -----------------------------------------------------------------------------------------------------------------
  {
    f32x4 acc[NT];
    tail_gemm_x3<NT, BSTAGE, true, NST, WAVES>(acc, p.wm, wrow1, 0, D / 32, [&](int ks) { return tMsg + fr * PA + ks * 32; }, sB, wave, lane);
    tail_layernorm<NT, float>(acc, p.g1, p.b1, p.ln_eps, fr);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // this wave's reads of msg are complete
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) tMsg[(fq * 4 + r) * PA + j * 16 + fr] = acc[j][r];      // y1 replaces msg
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- mlp.0 ([x | y1], K = 2 D -> 2 D, ReLU) and mlp.2 (K = 2 D -> D) in two halves of the hidden width -------------------------------
  f32x4 acc2[NT];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    f32x4 acc[NT];
    tail_gemm_x3<NT, BSTAGE, true, NST, WAVES>(acc, p.w0 + (long long)half * D * wrow2, wrow2, 0, 2 * D / 32,
                                   [&](int ks) { return ks * 32 < D ? tX + fr * PA + ks * 32 : tMsg + fr * PA + (ks * 32 - D); }, sB, wave, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // (second half) this wave's mlp.2 reads of the previous half are complete
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) tH[(fq * 4 + r) * PA + j * 16 + fr] = fmaxf(acc[j][r], 0.f);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (half == 0)
      tail_gemm_x3<NT, BSTAGE, true, NST, WAVES>(acc2, p.w2, wrow2, 0, D / 32, [&](int ks) { return tH + fr * PA + ks * 32; }, sB, wave, lane);
    else
      tail_gemm_x3<NT, BSTAGE, false, NST, WAVES>(acc2, p.w2, wrow2, D / 32, D / 32, [&](int ks) { return tH + fr * PA + (ks * 32 - D); }, sB, wave, lane);
  }
  tail_layernorm<NT, float>(acc2, p.g2, p.b2, p.ln_eps, fr);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = fq * 4 + r, col = j * 16 + fr;
      tMsg[row * PA + col] = acc2[j][r] + tX[row * PA + col];      // stage the output tile
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  tail_tile_store<float, D, PA>(p.out, p.out_ld, tMsg, row0, p.rows, lane);
}

// ---- LKPM tail (Block14.forward after the depthwise conv, convnext.py:48-58): LayerNorm(1e-6) -> pwconv1 (D -> 4 D) -> GELU -> pwconv2
// (4 D -> D) -> + input, for the 16 token rows of a wave, in the default numerics.  The hidden width runs in FOUR quarters of D channels:
// a quarter of h is produced (bias + exact erf GELU), then consumed as a K range of pwconv2 into accumulators that stay in registers.
template <int D, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void lkpm_tail_x3_kernel(LkpmP<float, f16_t> p) {
  constexpr int NT = D / 16;
  constexpr int PA = D + 8;
  constexpr int TILE = 16 * PA;
  constexpr int WAVE_LDS = 2 * TILE * 4;                   // normalised input / output tile | hidden quarter
  constexpr int BSTAGE = D * 128;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  unsigned char* sB = smem;
  constexpr int NST = tail_nst_lkpm<D>();
  float* tA = reinterpret_cast<float*>(smem + NST * BSTAGE + wave * WAVE_LDS);
  float* tH = tA + TILE;
  const long long row0 = (long long)blockIdx.x * (16 * WAVES) + wave * 16;
  constexpr int XCH = D / 4;
  constexpr int wrow1 = (D / 32) * 64, wrow2 = (4 * D / 32) * 64;

  tail_tile_load<float, D, PA>(tA, p.t, p.t_ld, row0, p.rows, lane);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  tail_row_layernorm<float, D, PA>(tA, p.lg, p.lb, p.ln_eps, fr, fq);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  f32x4 acc2[NT];
#pragma unroll
  for (int part = 0; part < 4; ++part) {
    f32x4 acc[NT];
    tail_gemm_x3<NT, BSTAGE, true, NST, WAVES>(acc, p.w1 + (long long)part * D * wrow1, wrow1, 0, D / 32, [&](int ks) { return tA + fr * PA + ks * 32; }, sB, wave, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // this wave's pwconv2 reads of the previous quarter are complete
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float bj = p.b1[part * D + j * 16 + fr];
#pragma unroll
      for (int r = 0; r < 4; ++r) tH[(fq * 4 + r) * PA + j * 16 + fr] = act_c<CFP_ACT_GELU>(acc[j][r] + bj);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (part == 0)
      tail_gemm_x3<NT, BSTAGE, true, NST, WAVES>(acc2, p.w2, wrow2, 0, D / 32, [&](int ks) { return tH + fr * PA + ks * 32; }, sB, wave, lane);
    else
      tail_gemm_x3<NT, BSTAGE, false, NST, WAVES>(acc2, p.w2, wrow2, part * (D / 32), D / 32, [&](int ks) { return tH + fr * PA + (ks * 32 - part * D); }, sB, wave, lane);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const float bj = p.b2[j * 16 + fr];
#pragma unroll
    for (int r = 0; r < 4; ++r) tA[(fq * 4 + r) * PA + j * 16 + fr] = acc2[j][r] + bj;      // the normalised input is consumed: stage the output tile
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  for (int i = lane; i < 16 * XCH; i += 64) {
    const int r = i / XCH, ch = i - r * XCH;
    const long long m = row0 + r;
    if (m < p.rows) {
      f32x4 a = *reinterpret_cast<const f32x4*>(tA + r * PA + ch * 4);
      const f32x4 b = *reinterpret_cast<const f32x4*>(p.xin + m * p.x_ld + ch * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += b[e];
      *reinterpret_cast<f32x4*>(p.out + m * p.out_ld + ch * 4) = a;
    }
  }
}

int g_tail_waves = 0;      // cfp_debug_set key 35: 0 = by the row count, else 1 / 2 / 4 waves per workgroup (A/B)

}  // namespace

void cfp_tail_x3_debug_set(int value) { g_tail_waves = value; }

int loftr_tail_x3_launch(const TailP<float, f16_t>& p, int heads, int D, hipStream_t s) {
  return tail_pick<32, 64, 128>(D, [&](auto d) { return tail_pick<4, 8>(heads, [&](auto h) {
    return tail_pick<1, 2, 4>(tail_waves(p.rows, g_tail_waves), [&](auto w) {
      constexpr int D_ = d, W_ = w;
      constexpr size_t lds = tail_nst_loftr<D_>() * (D_ * 128) + W_ * (3 * 16 * (D_ + 8) * 4);      // weight stages + the waves' tiles
      return tail_launch<loftr_tail_x3_kernel<D_, h, W_>, lds>(p, W_, s);
    }); }); });
}

int lkpm_tail_x3_launch(const LkpmP<float, f16_t>& p, int D, hipStream_t s) {
  return tail_pick<32, 64, 128>(D, [&](auto d) { return tail_pick<1, 2, 4>(tail_waves(p.rows, g_tail_waves), [&](auto w) {
    constexpr int D_ = d, W_ = w;
    constexpr size_t lds = tail_nst_lkpm<D_>() * (D_ * 128) + W_ * (2 * 16 * (D_ + 8) * 4);
    return tail_launch<lkpm_tail_x3_kernel<D_, W_>, lds>(p, W_, s);
  }); });
}
