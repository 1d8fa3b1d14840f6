// 16-bit 3x3 stride-1 convolution for FEW input channels (Cin <= 64): the whole-depth input halo of a pixel tile stays in LDS.
//
// Reference ops: the EfficientNetV2 stem-side blocks of the RGB encoder (timm ConvBnAct / EdgeResidual: conv 3x3 -> BatchNorm -> SiLU
// [+ skip], oracle/cfpnet_oracle.py encoder()) and the decoder's 3x3 convolutions on 32 / 64 channels (decoder.py:51-58 UpSampleBN).
// They are this network's many-pixel, short-K problems (6 x 10^5 ... 4 x 10^4 pixels, K = 144 ... 576): by FLOPs they are nothing,
// by HBM bytes they should take 5-15 us each at batch 8, and as implicit GEMMs they take 16-54 us (profiles/r3_conv_sweep: 2.7x
// their ideal over the family) because the im2col A operand is fetched from L2 nine times -- once per tap -- and once more per
// N-tile: 442 MB of L2->LDS traffic for a 49 MB input.  conv3x3_direct.hip removed the nine but re-staged the halo per 64-channel
// chunk and per 32-cout tile behind three coarse pipeline steps, and lost to the implicit GEMM on every one of these shapes.
//
// This kernel:
//   * a workgroup owns TH x 16 output pixels (TH = 16 or 8) and all output channels, or one of 2-3 blocks of them; the (TH + 2) x 18 input halo with all Cin
//     channels is loaded ONCE (16-byte pieces, register-staged, pixel pitch an odd number of 16-byte slots so that the 16 lanes of
//     an MFMA operand read -- 16 consecutive pixels of a row -- fall on 16 different slots of the 256-byte bank row);
//   * K runs over (tap, 8-channel chunk) in the weight tensor's own order [Cout][kh][kw][Cin]: the B fragment of k-chunk c is the
//     halo pixel shifted by tap c / (Cin / 8), so the nine taps are address arithmetic on the resident tile (per lane, two
//     compare-and-subtract updates per 32-deep MFMA step);
//   * the weights are the only streamed operand: 64-deep K-steps of [Cout][64] rows, `global_load_lds_dwordx4` into XOR-swizzled
//     128-byte rows exactly as conv_igemm2.hip stages its W tile, 2-3 stages, counted `s_waitcnt vmcnt`, one raw barrier per K-step;
//   * a wave computes 4 pixel rows x NT 16-channel tiles; accumulators transposed (weights as the MFMA row operand): a lane owns 4
//     consecutive channels of one pixel and the epilogue (folded BatchNorm, activation, optional skip) stores 8 bytes from registers.
//
// Same products, float32 accumulation in a different order than the implicit GEMM: results agree to float32 re-association
// (tests: <= 1 ulp of the storage type against cfp_conv2d_nhwc's other kernels, bit-exact on small integers).
//
// The tile constants, the workgroup decode, the bilinear taps of the UP loader and the host side
// (variant table, pitch rule, LDS sizes, launch) are shared with the float32 kernels of conv3x3_halo_x3.hip: halo_core.h.
#include "halo_core.h"

namespace {

struct HaloP : HaloGeo {      // PP: Cin * 2 rounded up by halo16_pitch; PPX = 16-byte pieces of a pixel the loader fetches = Cin / 8 (8-channel chunks)
  // --- PW = true only (cfp_conv3x3_pw_fused): the 1x1 convolution that consumes this one's output in the same launch ---
  const void* w2;          // [16 ceil(Cout2 / 16)][Kp] 16-bit, zero padded (ops.pad_pw_w)
  const float* scale2;     // folded BatchNorm / bias of the 1x1 convolution [Cout2] (null = 1 / 0)
  const float* shift2;
  int Cout2, Kp;           // Kp = mid channels rounded up to 32
  float slope2;            // the 1x1's activation as y > 0 ? y : slope2 * y: 1 = none, 0.01 = LeakyReLU
  int w2_kb;               // size of w2 in KB (a whole number: 16 rows x 32 K-values are 1 KB)
  int koff;                // byte offset of the epilogue constants in LDS: behind the stages + halo and behind the `mid` tile of the tail
};

// UP = true (cfp_upsample_cat_conv3x3, decoder.py:51-58 UpSampleBN): the 16-byte pieces of the halo that belong to channels below p.up_C
// are not fetched but BLENDED from four taps of the low-resolution map (resize_kernel's own float32 arithmetic, rounded to the storage
// type as the stored upsampled tensor would have been); the other channels come from the skip tensor.
// STRIDE = 2 (the stem and the first block of an encoder stage, TF-"same" padding): the halo is (2 TH + 1) x 33 input pixels, an output pixel's
// tap (dy, dx) is input pixel (2 y + dy, 2 x + dx) of it.
// PW = true (cfp_conv3x3_pw_fused: timm EdgeResidual conv_exp -> bn1 -> SiLU -> conv_pwl -> bn2 [+ shortcut], and any other 3x3 whose only
// reader is a 1x1): the workgroup owns ALL mid channels of its pixels (n_blocks == 1) and `mid` never leaves the chip.  After the K loop
// the accumulators get this convolution's epilogue, are rounded to the storage type exactly as the stored tensor would have been and go to
// LDS as the workgroup's [pixels][mid] tile (the stage the last K-step read and the halo are free by then).  The second GEMM
// out^T[Cout2][px] = W2 * mid^T then runs per wave over ALL mid channels of two (WN = 2) or four pixel rows: its B fragments are plain
// 16-byte reads of that tile, its K blocks run in the channel order into ONE accumulator -- the summation order of the 1x1 launch this
// replaces (conv_igemm.hip, conv_igemm2.hip), so the result is that launch's bit for bit, not merely to re-association.  (Feeding the packed
// accumulators to the MFMA directly, as head_fused.hip does, needs no LDS round trip but permutes K inside a block and, with the mid
// channels split over two waves, adds two partial sums: 0.01-0.07 % of the outputs then differ by an ulp, and this network spreads such
// flips into a different forward.)  W2 [16 ceil(Cout2 / 16)][Kp], zero padded, comes by LDS-DMA into stage 0 during the last K-step (the
// stages rotate by nk & 1 so that this step reads stage 1).  p.out / out_ld / res / res_ld describe the 1x1 convolution's output,
// p.Cout / scale / shift / act the 3x3 one's.  The tail runs once per workgroup, so its cost is latency and code size: the per-channel
// vectors of both epilogues wait in LDS from the start, and the tail is ONE straight path with the 1x1's activation as a slope -- with
// a copy of the epilogue per wave half and a runtime activation switch per element an earlier form measured 4-6 us slower per launch for
// identical arithmetic.
template <typename H, int NT, int WN, int STAGES, bool UP = false, int STRIDE = 1, bool PW = false>
__global__ __launch_bounds__(256, 2) void conv3x3_halo_kernel(ConvP p, HaloP hp) {
  using T = HaloTile<NT, WN>;
  constexpr int TH = T::TH, NPAD = T::NPAD, NB = T::NB, WSTAGE = T::WSTAGE;
  constexpr int HC = 15 * STRIDE + 3;        // halo columns
  constexpr int HPIX = ((TH - 1) * STRIDE + 3) * HC;
  static_assert(!(UP && STRIDE != 1), "the upsampling loader is stride 1");
  constexpr int LB = UP ? 4 : 6;             // halo pieces per thread and loader pass (UP: four taps each)
  static_assert((STAGES - 2) * NB <= 63, "vmcnt field");
  static_assert(!PW || (STAGES == 2 && !UP && WN <= 2), "the fused 1x1 takes stage 0 of two weight stages");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sW = smem;                              // STAGES weight stages
  unsigned char* sX = smem + STAGES * WSTAGE;            // the halo tile

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int fr = lane & 15, fq = lane >> 4;

  const HaloWg wg = halo_wg<NT, WN>(hp);
  const int n_base = wg.n_base, x0 = wg.x0, y0 = wg.y0, b = wg.b;

  const H* __restrict__ in = reinterpret_cast<const H*>(p.in) + (long long)b * p.H * p.W * p.in_ld;
  const int nk = (p.K + 63) >> 6;

  // ---- weight stages: lane (row rsub of an 8-row group, logical chunk lc); 64-deep K-steps of the [Cout][K] rows, the K tail masked ------------------------------------------------------
  const int rsub = lane >> 3;
  const int lc = (lane & 7) ^ rsub;
  const H* __restrict__ wt = reinterpret_cast<const H*>(p.w);
  const void* zsrc = reinterpret_cast<const void*>(g_zero16);
  const H* b_ptr[NB];
  unsigned b_okmask = 0;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int n = n_base + ((j * 4 + wave) % T::NBG) * 8 + rsub;
    const bool ok = n < p.Cout;
    if (ok) b_okmask |= 1u << j;
    b_ptr[j] = wt + (long long)(ok ? n : 0) * p.K;
  }
  auto issue = [&](int ks, int buf) {
    unsigned char* s = sW + buf * WSTAGE;
    const int kk = (ks * 8 + lc) * 8;
    const bool kok = kk < p.K;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const bool ok = kok && ((b_okmask >> j) & 1u);
      glds16(ok ? (const void*)(b_ptr[j] + kk) : zsrc, s + ((j * 4 + wave) % T::NBG) * 1024);
    }
  };
  const int sb = PW ? (nk & 1) : 0;      // PW: the stages rotate so that the LAST K-step reads stage 1 and W2 lands in stage 0
  auto issue_w2 = [&](int buf) {      // PW: the whole permuted 1x1 weight, 1 KB per instruction, linear
    const unsigned char* g = reinterpret_cast<const unsigned char*>(hp.w2) + lane * 16;
    for (int i = wave; i < hp.w2_kb; i += 4) glds16(g + i * 1024, sW + buf * WSTAGE + i * 1024);
  };
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nk) issue(s, (s + sb) % STAGES);

  // PW: the per-channel vectors of both epilogues go to LDS -- fetched now, stored behind the halo (their global latency hides behind its
  // loads), where loading them at their use costs one exposed round trip each per workgroup (head_fused.hip found the same).
  // [NPAD] scale | [NPAD] shift | [64] scale2 | [64] shift2
  float* sK = reinterpret_cast<float*>(smem + hp.koff);
  float k_sc = 1.f, k_sh = 0.f, k_sc2 = 1.f, k_sh2 = 0.f;
  static_assert(!PW || NPAD <= 256, "one channel per thread");
  if constexpr (PW) {
    if (tid < p.Cout && p.scale) k_sc = p.scale[tid];
    if (tid < p.Cout && p.shift) k_sh = p.shift[tid];
    if (tid < hp.Cout2 && hp.scale2) k_sc2 = hp.scale2[tid];
    if (tid < hp.Cout2 && hp.shift2) k_sh2 = hp.shift2[tid];
  }

  // ---- the halo: all pieces of the thread in flight, then the LDS stores (the compiler drains the DMA queue before them; both are
  //      needed before the first MFMA anyway) ---------------------------------------------------------------------------------------
  {
    const int nitems = HPIX * hp.PPX;
    const H* __restrict__ low = nullptr;
    int upc = 0;
    if constexpr (UP) { low = reinterpret_cast<const H*>(p.up_src) + (long long)b * p.up_H * p.up_W * p.up_ld; upc = p.up_C >> 3; }
    for (int base = 0; base < nitems; base += 256 * LB) {
      u32x4 v[LB][UP ? 4 : 1];
      int dst[LB];
      float lyx[LB][UP ? 2 : 1];
      bool blend[LB];
#pragma unroll
      for (int n = 0; n < LB; ++n) {
        const int i = base + tid + n * 256;
        unsigned upx, uch;
        fd_rowcol((unsigned)i, hp.dpx, upx, uch);
        const int px = (int)upx, ch = (int)uch;
        const int hy = px / HC, hx = px - hy * HC;
        const int y = y0 * STRIDE - p.pad_t + hy, x = x0 * STRIDE - p.pad_l + hx;
        const bool ok = i < nitems && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
        dst[n] = i < nitems ? px * hp.PP + ch * 16 : -1;
        blend[n] = false;
#pragma unroll
        for (int t = 0; t < (UP ? 4 : 1); ++t) v[n][t] = u32x4{0u, 0u, 0u, 0u};
        if constexpr (UP) {
          if (ch < upc) {
            blend[n] = ok;
            const BilinTap bt = bilin_tap(p, y, x);
            lyx[n][0] = bt.ly; lyx[n][1] = bt.lx;
            if (ok) {
              const H* s00 = low + bt.off + ch * 8;
              v[n][0] = *reinterpret_cast<const u32x4*>(s00); v[n][1] = *reinterpret_cast<const u32x4*>(s00 + bt.dxo);
              v[n][2] = *reinterpret_cast<const u32x4*>(s00 + bt.dyo); v[n][3] = *reinterpret_cast<const u32x4*>(s00 + bt.dyo + bt.dxo);
            }
            continue;
          }
        }
        if (ok) v[n][0] = *reinterpret_cast<const u32x4*>(in + (y * p.W + x) * p.in_ld + ch * 8);      // one image < 2^31 elements (host check)
      }
#pragma unroll
      for (int n = 0; n < LB; ++n) {
        if (dst[n] < 0) continue;
        if constexpr (UP) {
          if (blend[n]) {
            float t[4][8], o[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) Vec<H>::load(reinterpret_cast<const H*>(&v[n][q]), t[q]);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = bilin_blend(lyx[n][0], lyx[n][1], t[0][e], t[1][e], t[2][e], t[3][e]);
            Vec<H>::store(reinterpret_cast<H*>(sX + dst[n]), o);
            continue;
          }
        }
        *reinterpret_cast<u32x4*>(sX + dst[n]) = v[n][0];
      }
    }
  }

  if constexpr (PW) {
    if (tid < NPAD) { sK[tid] = k_sc; sK[NPAD + tid] = k_sh; }
    if (tid < 64) { sK[2 * NPAD + tid] = k_sc2; sK[2 * NPAD + 64 + tid] = k_sh2; }
  }

  f32x4 acc[4][NT];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[g][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // im2col position of this lane's k-chunk (c = 4 * step + fq): tap offset inside the halo and chunk inside the pixel
  const int ntap_chunks = 9 * hp.PPX;
  int c_cc, c_dx = 0, c_off = 0, c_idx = fq;
  {
    const int tap = fq / hp.PPX;
    c_cc = fq - tap * hp.PPX;
    c_dx = tap;                                  // fq <= 3 and PPX >= 1: tap <= 3; normalised below
    while (c_dx >= 3) { c_dx -= 3; c_off += HC * hp.PP; }
    c_off += c_dx * hp.PP;
  }
  const unsigned char* xrow = sX + ((wm * 4 * STRIDE) * HC + fr * STRIDE) * hp.PP;      // tap (0, 0) of output pixel (row wm * 4, column fr)
  const int growb = STRIDE * HC * hp.PP;                                                 // one output row further

  for (int ks = 0; ks < nk; ++ks) {
    const int buf = (ks + sb) % STAGES;
    wait_stage<STAGES, NB>(min(nk - 1 - ks, STAGES - 2));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's halo stores (first time round) and fragment reads of the previous step
    __builtin_amdgcn_s_barrier();          // stage `buf` (and the halo) landed for every wave; stage buf-1 fully consumed.  Raw: a __syncthreads() would drain the DMA queue
    asm volatile("" ::: "memory");
    if (ks + STAGES - 1 < nk) issue(ks + STAGES - 1, (ks + STAGES - 1 + sb) % STAGES);
    else if constexpr (PW) issue_w2(0);      // the last K-step: stage 0 is free
    const unsigned char* cW = sW + buf * WSTAGE + (wn * NT * 16) * 128;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      s16x8 wf[NT], xf[4];
      const int pc = ((s * 4 + fq) ^ (fr & 7)) * 16;
#pragma unroll
      for (int j = 0; j < NT; ++j) wf[j] = *reinterpret_cast<const s16x8*>(cW + (j * 16 + fr) * 128 + pc);
      // chunks past the ninth tap meet zero weights: read any finite data -- the tile's first piece, the SAME address in every such lane
      // (identical addresses broadcast; per-lane addresses there collided with the live lanes of their read group)
      const bool live = c_idx < ntap_chunks;
      const int xo = c_off + c_cc * 16;
#pragma unroll
      for (int g = 0; g < 4; ++g) xf[g] = *reinterpret_cast<const s16x8*>(live ? xrow + g * growb + xo : sX);
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[g][j] = mfma16<H>(wf[j], xf[g], acc[g][j]);   // acc[r] = channel 4 fq + r of tile j, pixel fr
      // next 32-deep step: four chunks further
      c_idx += 4;
      c_cc += 4;
      while (c_cc >= hp.PPX) {
        c_cc -= hp.PPX;
        c_off += hp.PP;
        if (++c_dx == 3) { c_dx = 0; c_off += (HC - 3) * hp.PP; }
      }
    }
  }

  if constexpr (PW) {
    H* __restrict__ out = reinterpret_cast<H*>(p.out) + (long long)b * p.Ho * p.Wo * p.out_ld;
    const H* __restrict__ res = p.res ? reinterpret_cast<const H*>(p.res) + (long long)b * p.Ho * p.Wo * p.res_ld : nullptr;
    const int x = x0 + fr;
    constexpr int NG = WN == 2 ? 2 : 4;          // pixel rows a wave finishes: [g0, g0 + NG)
    const int g0 = WN == 2 ? 2 * wn : 0;
    // ---- this convolution's epilogue on the accumulators, rounded as the stored tensor would be: pk[g][j] = channels 16 j + 4 fq + {0..3} ----
    uint2 pk[4][NT];
    {
      f32x4 sc[NT], sh[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = (wn * NT + j) * 16 + fq * 4;
        sc[j] = *reinterpret_cast<const f32x4*>(sK + n);
        sh[j] = *reinterpret_cast<const f32x4*>(sK + NPAD + n);
      }
      with_act(p.act, [&](auto A) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            float yv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) yv[r] = act_c16<decltype(A)::value>(acc[g][j][r] * sc[j][r] + sh[j][r]);
            pk[g][j].x = pack2<H>(yv[0], yv[1]);
            pk[g][j].y = pack2<H>(yv[2], yv[3]);
          }
      });
    }
    // ---- the workgroup's `mid` tile [TH * 16 pixels][Kp channels] in LDS, behind W2 (stage 0): stage 1 and the halo are free once every
    //      wave has left the last K-step.  Pixel pitch Kp * 2 + 16 bytes: the 16 pixels of a fragment read fall on 16 different slots ----
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int mpitch = hp.Kp * 2 + 16;
    unsigned char* sM = smem + hp.w2_kb * 1024;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = (wn * NT + j) * 16 + fq * 4;
        if (n < hp.Kp) *reinterpret_cast<uint2*>(sM + ((wm * 4 + g) * 16 + fr) * mpitch + n * 2) = pk[g][j];
      }
    wait_vmcnt<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();          // W2 landed and `mid` written for every wave
    asm volatile("" ::: "memory");
    // the skip values of the pixel rows this wave finishes: in flight across the second GEMM (issued behind the wait for W2, which would
    // otherwise wait for them too)
    uint2 rres[NG][4];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi)
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        const int y = y0 + wm * 4 + g0 + gi, n = ti * 16 + fq * 4;
        rres[gi][ti] = (res && y < p.Ho && x < p.Wo && n < hp.Cout2) ? *reinterpret_cast<const uint2*>(res + ((long long)y * p.Wo + x) * p.res_ld + n) : uint2{0u, 0u};
      }
    const int t2n = (hp.Cout2 + 15) >> 4;
    const int rowb = hp.Kp * 2;

    // ---- GEMM2: out^T[Cout2][px] for this wave's NG pixel rows over ALL mid channels, K blocks in order into one accumulator ----
    f32x4 fin[NG][4];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi)
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) fin[gi][ti] = f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned char* mrow = sM + ((wm * 4 + g0) * 16 + fr) * mpitch + fq * 16;
    const unsigned char* wrow = smem + fr * rowb + fq * 16;
#pragma unroll
    for (int kb = 0; kb < NPAD / 32; ++kb) {
      if (kb * 32 >= hp.Kp) continue;
      s16x8 bfr[NG];
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) bfr[gi] = *reinterpret_cast<const s16x8*>(mrow + gi * 16 * mpitch + kb * 64);
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        if (ti >= t2n) continue;
        const s16x8 af = *reinterpret_cast<const s16x8*>(wrow + ti * 16 * rowb + kb * 64);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) fin[gi][ti] = mfma16<H>(af, bfr[gi], fin[gi][ti]);
      }
    }

    // ---- the 1x1 convolution's epilogue: scale / shift, none / LeakyReLU as a slope, the skip added to the ROUNDED value as every
    //      conv kernel here does, 8-byte stores ----
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
      const int n = ti * 16 + fq * 4;
      if (n >= hp.Cout2) continue;
      const f32x4 sc2 = *reinterpret_cast<const f32x4*>(sK + 2 * NPAD + n);
      const f32x4 sh2 = *reinterpret_cast<const f32x4*>(sK + 2 * NPAD + 64 + n);
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        const int y = y0 + wm * 4 + g0 + gi;
        if (!(y < p.Ho && x < p.Wo)) continue;
        const long long pix = (long long)y * p.Wo + x;
        float yv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = fin[gi][ti][r] * sc2[r] + sh2[r];
          yv[r] = v > 0.f ? v : v * hp.slope2;
        }
        uint2 o2;
        o2.x = pack2<H>(yv[0], yv[1]);
        o2.y = pack2<H>(yv[2], yv[3]);
        if (res) {
          const H* ph = reinterpret_cast<const H*>(&o2);
          const H* rh = reinterpret_cast<const H*>(&rres[gi][ti]);
          H oh[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) oh[r] = from_f32<H>(to_f32<H>(ph[r]) + to_f32<H>(rh[r]));
          o2 = *reinterpret_cast<const uint2*>(oh);
        }
        *reinterpret_cast<uint2*>(out + pix * p.out_ld + n) = o2;
      }
    }
    return;
  }

  // ---- epilogue: folded BatchNorm / bias, activation, optional skip; 8-byte stores from the accumulators -------------------------------
  H* __restrict__ out = reinterpret_cast<H*>(p.out) + (long long)b * p.Ho * p.Wo * p.out_ld;
  const H* __restrict__ res = p.res ? reinterpret_cast<const H*>(p.res) + (long long)b * p.Ho * p.Wo * p.res_ld : nullptr;
  const int x = x0 + fr;
  f32x4 sc[NT], sh[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n_base + (wn * NT + j) * 16 + fq * 4;
    const bool ok = n < p.Cout;
    sc[j] = (ok && p.scale) ? *reinterpret_cast<const f32x4*>(p.scale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
    sh[j] = (ok && p.shift) ? *reinterpret_cast<const f32x4*>(p.shift + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  with_act(p.act, [&](auto A) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int y = y0 + wm * 4 + g;
      const bool pix_ok = y < p.Ho && x < p.Wo;
      const long long pix = (long long)y * p.Wo + x;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = n_base + (wn * NT + j) * 16 + fq * 4;
        float yv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) yv[r] = act_c16<decltype(A)::value>(acc[g][j][r] * sc[j][r] + sh[j][r]);
        uint2 pk;
        pk.x = pack2<H>(yv[0], yv[1]);
        pk.y = pack2<H>(yv[2], yv[3]);
        if (!(pix_ok && n < p.Cout)) continue;
        if (res) {
          // the skip is added to the ROUNDED activation, as the other conv kernels do (they round into their LDS C tile first)
          const uint2 rr = *reinterpret_cast<const uint2*>(res + pix * p.res_ld + n);
          const H* ph = reinterpret_cast<const H*>(&pk);
          const H* rh = reinterpret_cast<const H*>(&rr);
          float o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = to_f32<H>(ph[r]) + to_f32<H>(rh[r]);
          H oh[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) oh[r] = from_f32<H>(o[r]);
          pk = *reinterpret_cast<const uint2*>(oh);
        }
        *reinterpret_cast<uint2*>(out + pix * p.out_ld + n) = pk;
      }
    }
  });
}

int g_halo_odd_pitch = 0;    // cfp_debug_set key 27: 1 = the round-3 odd pixel pitch
int g_halo_stages = 0;      // cfp_debug_set key 13: force the number of weight stages (2-4), 0 = automatic

template <typename H, int NT, int WN, bool UP = false, int STRIDE = 1, bool PW = false>
int launch_h(const ConvP& p, hipStream_t s, const ConvPwP* pw = nullptr) {
  constexpr HaloTileV t = halo_tile(NT, WN);
  HaloP hp{};
  if (!halo_geo<NT, WN>(hp, p, p.Cin / 8, halo16_pitch(p.Cin, STRIDE, g_halo_odd_pitch != 0))) return -1;
  // weight stages: two.  More would hide more of the DMA latency behind MFMAs, but measured (tools/conv_bench.py --halo, us with
  // 2 / 3 / 4 stages: 614400 px x 128 ch 82 / 93 / 96, 153600 x 160 36 / 38 / 52, 614400 x 16 23 / 25 / 25, 38400 x 224 19 / 24 / 32)
  // the LDS they take costs more in resident workgroups than it gains -- the same finding as for the implicit GEMM's tiles
  const int stages = g_halo_stages && !PW ? g_halo_stages : 2;
  size_t lds = halo16_lds(t, stages, STRIDE, hp.PP);
  if constexpr (PW) {
    if (!pw || hp.n_blocks != 1 || pw->Cout2 > 64 || pw->Cout2 % 8 != 0) return -1;
    hp.w2 = pw->w2; hp.scale2 = pw->scale2; hp.shift2 = pw->shift2; hp.Cout2 = pw->Cout2; hp.slope2 = pw->act2 == CFP_ACT_LRELU ? 0.01f : 1.f;
    hp.Kp = cdiv(p.Cout, 32) * 32;
    hp.w2_kb = (int)(halo16_pw_w2_bytes(p.Cout, pw->Cout2) / 1024);
    if (halo16_pw_w2_bytes(p.Cout, pw->Cout2) > (size_t)t.wstage) return -1;      // W2 must fit one weight stage
    hp.koff = (int)halo16_pw_body(t, STRIDE, hp.PP, p.Cout, pw->Cout2);
    lds = halo16_pw_lds(t, STRIDE, hp.PP, p.Cout, pw->Cout2);
  }
  if constexpr (UP || STRIDE != 1 || PW) return halo_launch<conv3x3_halo_kernel<H, NT, WN, 2, UP, STRIDE, PW>>(p, hp, lds, s);
  else return stages == 4 ? halo_launch<conv3x3_halo_kernel<H, NT, WN, 4>>(p, hp, lds, s)
            : stages == 3 ? halo_launch<conv3x3_halo_kernel<H, NT, WN, 3>>(p, hp, lds, s) : halo_launch<conv3x3_halo_kernel<H, NT, WN, 2>>(p, hp, lds, s);
}

}  // namespace

int conv3x3_halo_num_variants() { return kNumHCfg16; }
void conv3x3_halo_debug_stages(int v) { g_halo_stages = v; }
void conv3x3_halo_debug_odd_pitch(int v) { g_halo_odd_pitch = v; }

// The problems this kernel takes: 3x3, stride 1 or 2, undilated, 16-bit, Cin a multiple of 8 and <= 128 (the plan uses it up to 64), no
// LayerNorm epilogue / per-image weights.
bool conv3x3_halo_takes(const ConvP& p) {
  return p.KH == 3 && p.KW == 3 && (p.stride == 1 || (p.stride == 2 && p.up_src == nullptr)) && p.dil <= 1 && p.Cin % 8 == 0 && p.Cin >= 8 && p.Cin <= 128 && p.Cout % 8 == 0 &&
         p.Cout <= 512 && p.ln_gamma == nullptr && p.rows_per_batch == 0 && p.k2 == 0 && p.K == 9 * p.Cin &&
         p.pad_t >= 0 && p.pad_l >= 0 && p.pad_t <= 2 && p.pad_l <= 2;
}

// variant < 0: chosen from Cout and the number of tiles.  Returns 0, or a negative value if the variant cannot run this problem.
int conv3x3_halo_launch(int v, const ConvP& p, hipStream_t s) {
  if (v < 0) {
    const long long t16 = (long long)p.B * cdiv(p.Wo, 16) * cdiv(p.Ho, 16);
    if (p.up_src != nullptr && p.Cout > 64) return -3;
    if (p.up_src != nullptr) v = p.Cout <= 32 ? 7 : 3;       // 8 x 16 pixel tiles: the blended halo is large, four workgroups per CU matter more (up4: 85 us, 16 x 16 tiles 104, direct kernel 112)
    else if (p.Cout <= 16) v = 0;
    else if (p.Cout <= 32) v = t16 >= 1024 ? 1 : 7;
    else if (p.Cout <= 64) v = t16 >= 1024 ? 2 : 3;
    else if (p.Cout <= 128) v = 4;
    else if (p.Cout <= 160) v = 5;
    else v = 4;                      // two or more 128-channel blocks
  }
  if (v >= kNumHCfg16) return -3;
  if (p.up_src != nullptr) {      // upsample + concatenation in the loader: the thin-output tiles only (the decoder's first conv of a stage)
#define HU(NT, WN) (p.f16 ? launch_h<f16_t, NT, WN, true>(p, s) : launch_h<bf16_t, NT, WN, true>(p, s))
    switch (v) {
      case 0: return HU(1, 1);
      case 1: return HU(2, 1);
      case 2: return HU(4, 1);
      case 3: return HU(2, 2);
      case 7: return HU(1, 2);
      default: return -3;
    }
#undef HU
  }
  if (p.stride == 2) {
#define HS(NT, WN) (p.f16 ? launch_h<f16_t, NT, WN, false, 2>(p, s) : launch_h<bf16_t, NT, WN, false, 2>(p, s))
    switch (v) {
      case 0: return HS(1, 1);
      case 1: return HS(2, 1);
      case 2: return HS(4, 1);
      case 3: return HS(2, 2);
      case 4: return HS(4, 2);
      case 5: return HS(5, 2);
      case 7: return HS(1, 2);
      default: return -3;
    }
#undef HS
  }
#define HV(NT, WN) (p.f16 ? launch_h<f16_t, NT, WN>(p, s) : launch_h<bf16_t, NT, WN>(p, s))
  switch (v) {
    case 0: return HV(1, 1);
    case 1: return HV(2, 1);
    case 2: return HV(4, 1);
    case 3: return HV(2, 2);
    case 4: return HV(4, 2);
    case 5: return HV(5, 2);
    case 6: return HV(7, 2);
    case 7: return HV(1, 2);
    default: return -3;
  }
#undef HV
}

// ---- cfp_conv3x3_pw_fused: 3x3 -> 1x1 in one launch (the kernel above with PW = true) ----
// The single-block variant for `mid` channels, or -1 when the problem is not taken: W2 must fit one weight stage and the workgroup's LDS
// the 160 KB of a CU.  (Cin, stride) decide the halo size, nothing else about the problem does.
int conv3x3_pw_variant(int Cin, int mid, int Cout2, int stride) {
  if (Cin < 8 || Cin > 128 || Cin % 8 != 0 || mid < 8 || mid % 8 != 0 || Cout2 < 8 || Cout2 > 64 || Cout2 % 8 != 0 || (stride != 1 && stride != 2)) return -1;
  const int v = mid <= 64 ? 2 : mid <= 160 ? 5 : mid <= 224 ? 6 : -1;
  if (v < 0 || (stride == 2 && v == 6)) return -1;
  const HaloTileV t = halo_tile(kHCfg[v].nt, kHCfg[v].wn);
  if (halo16_pw_w2_bytes(mid, Cout2) > (size_t)t.wstage) return -1;
  return halo16_pw_lds(t, stride, halo16_pitch(Cin, stride, false), mid, Cout2) <= kHaloLdsMax ? v : -1;
}

int conv3x3_pw_launch(const ConvP& p, const ConvPwP& pw, hipStream_t s) {
  const int v = conv3x3_pw_variant(p.Cin, p.Cout, pw.Cout2, p.stride);
  if (v < 0 || !conv3x3_halo_takes(p) || p.up_src != nullptr) return -3;
#define HP(NT, WN, ST) (p.f16 ? launch_h<f16_t, NT, WN, false, ST, true>(p, s, &pw) : launch_h<bf16_t, NT, WN, false, ST, true>(p, s, &pw))
  if (p.stride == 2) return v == 2 ? HP(4, 1, 2) : HP(5, 2, 2);
  return v == 2 ? HP(4, 1, 1) : v == 5 ? HP(5, 2, 1) : HP(7, 2, 1);
#undef HP
}

extern "C" int cfp_conv3x3_pw_fused_variant(int Cin, int Cmid, int Cout, int stride, int dtype) {
  return is16(dtype) ? conv3x3_pw_variant(Cin, Cmid, Cout, stride) : -1;
}

extern "C" int cfp_conv3x3_pw_fused(const void* in, int in_ld, const void* w1, const float* scale1, const float* shift1, int act1,
                                    const void* w2_pad, const float* scale2, const float* shift2, int act2, const void* residual, int res_ld,
                                    void* out, int out_ld, int B, int H, int W, int Cin, int Cmid, int Cout, int stride, int pad_t, int pad_l,
                                    int Ho, int Wo, int dtype, cfp_stream_t stream) {
  CFP_REQUIRE(in && w1 && w2_pad && out, CFP_EINVAL, "cfp_conv3x3_pw_fused: null pointer");
  CFP_REQUIRE(is16(dtype), CFP_EINVAL, "cfp_conv3x3_pw_fused: bf16 / f16 storage only");
  CFP_REQUIRE(act1 >= CFP_ACT_NONE && act1 <= CFP_ACT_SIGMOID && (act2 == CFP_ACT_NONE || act2 == CFP_ACT_LRELU), CFP_EINVAL,
              "cfp_conv3x3_pw_fused: bad activation (the 1x1 takes CFP_ACT_NONE or CFP_ACT_LRELU)");
  CFP_REQUIRE(B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && Cin > 0 && Cmid > 0 && Cout > 0, CFP_ESHAPE, "cfp_conv3x3_pw_fused: non-positive dimension");
  CFP_REQUIRE(cfp_conv3x3_pw_fused_variant(Cin, Cmid, Cout, stride, dtype) >= 0, CFP_ESHAPE,
              "cfp_conv3x3_pw_fused: shape not taken (cfp_conv3x3_pw_fused_variant: Cin % 8 == 0 and <= 128, Cmid % 8 == 0 and <= 224 (160 at stride 2), "
              "Cout % 8 == 0 and <= 64, stride 1 or 2, the 1x1 weights within one weight stage)");
  CFP_REQUIRE(in_ld % 8 == 0 && in_ld >= Cin && out_ld % 8 == 0 && out_ld >= Cout && (!residual || (res_ld % 8 == 0 && res_ld >= Cout)), CFP_ESHAPE,
              "cfp_conv3x3_pw_fused: row pitches must be multiples of the 16-byte vector and cover the channels");
  CFP_REQUIRE(pad_t >= 0 && pad_l >= 0 && pad_t <= 2 && pad_l <= 2 && (Ho - 1) * stride - pad_t + 2 < H + 3 && (Wo - 1) * stride - pad_l + 2 < W + 3, CFP_ESHAPE,
              "cfp_conv3x3_pw_fused: output size inconsistent with input size");
  CFP_REQUIRE((long long)B * Ho * Wo < (1ll << 31) && (long long)H * W * in_ld < (1ll << 31), CFP_ESHAPE, "cfp_conv3x3_pw_fused: problem too large");
  CFP_REQUIRE(aligned16(in) && aligned16(w1) && aligned16(w2_pad) && aligned16(out) && aligned16(residual) && aligned16(scale1) && aligned16(shift1) &&
                  aligned16(scale2) && aligned16(shift2), CFP_EINVAL, "cfp_conv3x3_pw_fused: pointers must be 16-byte aligned");
  ConvP p{};
  p.in = in; p.w = w1; p.out = out; p.res = residual; p.scale = scale1; p.shift = shift1;
  p.in_ld = in_ld; p.out_ld = out_ld; p.res_ld = res_ld;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.Cout = Cmid;
  p.KH = 3; p.KW = 3; p.stride = stride; p.pad_t = pad_t; p.pad_l = pad_l;
  p.M = B * Ho * Wo; p.K = 9 * Cin; p.act = act1; p.f16 = dtype == CFP_F16; p.dil = 1;
  ConvPwP pw{w2_pad, scale2, shift2, Cout, act2};
  const int rc = conv3x3_pw_launch(p, pw, reinterpret_cast<hipStream_t>(stream));
  CFP_REQUIRE(rc == 0, CFP_EHIP, "cfp_conv3x3_pw_fused: kernel launch failed");
  return cfp_check_launch("cfp_conv3x3_pw_fused");
}
