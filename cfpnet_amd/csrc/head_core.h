// What the two one-kernel adaptive-bins heads share: head_fused.hip (depth_head.conv3x3 from `unet` in HBM, 128 pixels and four waves per
// workgroup) and head_conv0.hip (decoder.conv0 computed on chip in front of it, a 16 x 16 pixel tile and eight waves).  How the operands of
// GEMM1 reach a wave differs and stays in the files, with the LDS maps, the placement of the Wout halves, the probe exits, the copy-out
// loops and every global address.  From the accumulators of GEMM1 on, a wave does the same work in both -- acc1[i][j][r] = ram(channel
// 16 i + 4 fq + r, pixel 16 j + fr of the wave's 32) -- and that work lives here, once; tests/test_head_conv0_gpu.py holds the two kernels
// to the same bits:
//   * HEAD_K_*            the float32 constants block in LDS
//   * head_handover       the stage hand-over of the LDS-DMA pipelines
//   * head_issue_wout     one half of conv_out's weights -> 32 KB of LDS by DMA
//   * head_ram_fragments  ram = acc1 * scale3 + shift3, packed into GEMM2's B fragments (head_fused.hip's header: why they ARE the fragments)
//   * head_acc2_init, head_gemm2_half     GEMM2 from the conv_out bias, one Wout half at a time
//   * head_softmax_column the softmax over the 256 bins of a pixel, its expectation, the prob staging and the uncertainty sums
// Nothing here touches global memory except through the callables the kernels pass in.
#pragma once
#include "common.h"
#include "head_stats.h"

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int HEAD_C = 128;               // channels of unet and of ram
constexpr int HEAD_NB = 256;              // bins

// The constants block, 4 KB of float32, filled at kernel entry (loading the vectors where they are used cost an exposed global round trip
// each).  The first 768 floats are the same in both kernels; the last 256 are the kernel's own.
constexpr int HEAD_K_BIAS = 0;            // [256] conv_out bias
constexpr int HEAD_K_SCALE3 = 256;        // [128] depth_head.conv3x3 scale
constexpr int HEAD_K_SHIFT3 = 384;        // [128] ... and shift
constexpr int HEAD_K_CEN = 512;           // [256] bin centres of the tile's (first) image
constexpr int HEAD_K_CEN1 = 768;          // [256] head_fused.hip: centres of the image the tile ends in
constexpr int HEAD_K_SCALE0 = 768;        // [128] head_conv0.hip: decoder.conv0 scale
constexpr int HEAD_K_SHIFT0 = 896;        // [128] ... and shift
constexpr int HEAD_K_BYTES = 1024 * 4;

// Stage hand-over: this wave's LDS-DMA loads have landed (vmcnt) AND its LDS-side operations have drained (lgkmcnt), then the
// workgroup barrier.  With `s_waitcnt vmcnt(0)` + a raw s_barrier alone head_fused.hip produced a wrong 32-pixel group (one wave's
// pixels) about once per 640 forwards when three captured forwards ran concurrently -- never alone, never with same-input repeats
// (tools/probes/inflight_race*.py, profiles/r2_inflight_race.txt: 5 / 3200 wrong results vs 0 / 3200 with this form): the zero words the
// hardware writes for out-of-range lanes of a `buffer_load ... lds` are apparently not covered by vmcnt.
__device__ __forceinline__ void head_handover() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  asm volatile("" ::: "memory");
}

// One half (64 permuted channels) of a Wout plane -> 32 KB at `dst`: 256 rows of 128 bytes in 32 DMA groups of 8 rows, 32 / WAVES per wave.
// `src` is the byte offset of the half (and plane) inside the descriptor; rsub = lane >> 3, lc = (lane & 7) ^ rsub as in the K loops.
template <int WAVES>
__device__ __forceinline__ void head_issue_wout(__amdgpu_buffer_rsrc_t rs_o, unsigned char* dst, int src, int wave, int rsub, int lc) {
#pragma unroll
  for (int q = 0; q < 32 / WAVES; ++q) {
    const int g = q * WAVES + wave;                        // 8-row group
    const unsigned v = (unsigned)(g * 8 + rsub) * (unsigned)(HEAD_C * 2) + (unsigned)lc * 16u;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_o, (lds_ptr_t)(dst + g * 1024), 16, (int)v, src, 0, 0);
  }
}

// The B fragments of GEMM2: K-block kb, pixel group j.  lo (RAMLO, head_fused.hip's exactness island) holds what the rounding of hi dropped.
template <bool RAMLO>
struct HeadFrags {
  s16x8 hi[4][2];
  s16x8 lo[RAMLO ? 4 : 1][2];
};

// ram = scale * acc + shift (depth_head.conv3x3 has a bias and no activation) -> B fragments of GEMM2.  ram_hook(kb, j, hi) sees the four
// packed words of (K-block, pixel group): channels (2 kb + u) * 16 + 4 fq + {0..3} in hi[2 u], hi[2 u + 1].
template <typename H, bool RAMLO, typename HOOK>
__device__ __forceinline__ void head_ram_fragments(const f32x4 (&acc1)[8][2], const float* sK, int fq, HeadFrags<RAMLO>& b, HOOK ram_hook) {
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    float sc[2][4], sh[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int ch = (2 * kb + u) * 16 + fq * 4;
      Vec<float>::load(sK + HEAD_K_SCALE3 + ch, sc[u]);
      Vec<float>::load(sK + HEAD_K_SHIFT3 + ch, sh[u]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[u * 4 + r] = acc1[2 * kb + u][j][r] * sc[u][r] + sh[u][r];
      uint32_t hi[4], lo[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const H h0 = from_f32<H>(v[2 * e]), h1 = from_f32<H>(v[2 * e + 1]);
        hi[e] = (uint32_t)to_bits<H>(h0) | ((uint32_t)to_bits<H>(h1) << 16);
        if constexpr (RAMLO) lo[e] = pack2<H>(v[2 * e] - to_f32<H>(h0), v[2 * e + 1] - to_f32<H>(h1));
      }
      b.hi[kb][j] = __builtin_bit_cast(s16x8, u32x4{hi[0], hi[1], hi[2], hi[3]});
      if constexpr (RAMLO) b.lo[kb][j] = __builtin_bit_cast(s16x8, u32x4{lo[0], lo[1], lo[2], lo[3]});
      ram_hook(kb, j, hi);
    }
  }
}

// GEMM2: logit^T[bin][px], accumulators start at the conv_out bias
__device__ __forceinline__ void head_acc2_init(f32x4 (&acc2)[16][2], const float* sK, int fq) {
#pragma unroll
  for (int ti = 0; ti < 16; ++ti) {
    float b4[4];
    Vec<float>::load(sK + HEAD_K_BIAS + ti * 16 + fq * 4, b4);
#pragma unroll
    for (int j = 0; j < 2; ++j) acc2[ti][j] = f32x4{b4[0], b4[1], b4[2], b4[3]};
  }
}

// ... and one half of its K axis: the Wout half at `base` (256 XOR-swizzled rows of 128 bytes) against K-blocks 2 half, 2 half + 1
template <typename H, bool RAMLO>
__device__ __forceinline__ void head_gemm2_half(f32x4 (&acc2)[16][2], const HeadFrags<RAMLO>& b, int half, const unsigned char* base,
                                                bool use_lo_b, int fr, int fq) {
#pragma unroll
  for (int kl = 0; kl < 2; ++kl) {
    const int kb = half * 2 + kl;
    const int pc = ((kl * 4 + fq) ^ (fr & 7)) * 16;
#pragma unroll
    for (int ti = 0; ti < 16; ++ti) {
      const s16x8 af = *reinterpret_cast<const s16x8*>(base + (ti * 16 + fr) * 128 + pc);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc2[ti][j] = mfma16<H>(af, b.hi[kb][j], acc2[ti][j]);
        if constexpr (RAMLO) { if (use_lo_b) acc2[ti][j] = mfma16<H>(af, b.lo[kb][j], acc2[ti][j]); }
      }
    }
  }
}

// What head_softmax_column returns with STATS (zeros without): the arguments of unc_plane (head_stats.h)
struct HeadMoments { float var, ent, inv; };

// Softmax over the 256 bins of pixel group j's pixel fr, and its expectation against `cen` (the 256 centres of the pixel's image, in LDS):
// a register reduction + two lane-group shuffles each.  Leaves the exponentials in acc2[.][j].  `stage` is the pixel's column of the prob
// staging tile [256 bins][PITCH], written where `staged` (the kernel has a prob output) holds.  The flag travels beside the pointer so that
// a caller can hand over a wave-uniform test: with a null column pointer as the only signal the test is per lane, and a launch of the
// conv0 kernel without prob walked all 64 stores of a pixel group with an empty exec mask (4 - 7 us per call, profiles/head_core_ab.txt).
// pred_out(dot) gets the expectation (every lane quarter holds it) before the variance walk.
template <typename H, bool STATS, int PITCH, typename PRED>
__device__ __forceinline__ HeadMoments head_softmax_column(f32x4 (&acc2)[16][2], int j, const float* cen, bool staged, H* stage, int fq, PRED pred_out) {
  float mx = -3.0e38f;
#pragma unroll
  for (int ti = 0; ti < 16; ++ti)
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, acc2[ti][j][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float s = 0.f, t = 0.f;
#pragma unroll
  for (int ti = 0; ti < 16; ++ti)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float d = acc2[ti][j][r] - mx;
      const float e = __expf(d);
      acc2[ti][j][r] = e;
      s += e;
      if constexpr (STATS) t = fmaf(e, d, t);
    }
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  if constexpr (STATS) {
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
  }
  const float inv = 1.f / s;
  float ent = 0.f;
  if constexpr (STATS) ent = unc_entropy(s, t, inv);
  float dot = 0.f;
#pragma unroll
  for (int ti = 0; ti < 16; ++ti) {
    float c4[4];
    Vec<float>::load(cen + ti * 16 + fq * 4, c4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pr = acc2[ti][j][r] * inv;
      dot = fmaf(pr, c4[r], dot);
      if constexpr (!STATS) { if (staged) stage[(ti * 16 + fq * 4 + r) * PITCH] = from_f32<H>(pr); }
    }
  }
  dot += __shfl_xor(dot, 16, 64);
  dot += __shfl_xor(dot, 32, 64);
  pred_out(dot);
  float var = 0.f;        // sum e (c - mu)^2: the accumulators hold the exponentials, 1 / s is applied once at the end
  if constexpr (STATS) {
#pragma unroll
    for (int ti = 0; ti < 16; ++ti) {
      float c4[4];
      Vec<float>::load(cen + ti * 16 + fq * 4, c4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dc = c4[r] - dot;
        var = fmaf(acc2[ti][j][r] * dc, dc, var);
        // the staging store waits for this walk, where the accumulators die one by one as they do in the plain kernel's expectation
        // loop: with it up there all 128 stay live across both loops and the allocator spills
        if (staged) stage[(ti * 16 + fq * 4 + r) * PITCH] = from_f32<H>(acc2[ti][j][r] * inv);
      }
    }
    var += __shfl_xor(var, 16, 64);
    var += __shfl_xor(var, 32, 64);
  }
  return {var * inv, ent, inv};
}

}  // namespace
