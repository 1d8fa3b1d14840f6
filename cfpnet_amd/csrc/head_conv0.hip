// decoder.conv0 (3x3, 32 -> 128, bias only) + the adaptive-bins head of head_fused.hip in ONE kernel: `unet` never reaches HBM.
// Reference: src/models/decoder.py conv0 (`x_d0 = self.conv0(...)`), decoder.py:22-27, deltar.py:18-19,51-61.
//
// Before: the halo kernel wrote unet = conv0(t) (157 MB at batch 8, 240 x 320) and depth_head_fused_kernel read it back nine times, once
// per tap, by LDS-DMA.  Here a workgroup of eight waves owns a 16 x 16 pixel tile of one image and computes the 18 x 18 halo of `unet` that
// its 3x3 needs from the 20 x 20 halo of the 32-channel `t` (1.27 x conv0's work), keeps it in LDS and runs GEMM1's nine taps as address
// arithmetic on that tile.  Only weights stream.
//
//   phase 0  t halo (20 x 20 pixels x 32 channels, 80-byte pixel pitch; pixels outside the image are out-of-range lanes of the buffer
//            descriptor = zeros) -> conv0 on 324 halo pixels = 21 groups of 16 (wave w: groups w, w + 8, w + 16) x 8 channel tiles, K in
//            conv3x3_halo.hip's order: tap-major, ONE 32-deep MFMA step per tap into one accumulator, so the float32 sums are that
//            kernel's bit for bit -> its epilogue (acc * scale + shift, no activation), rounded to the storage type, and FORCED TO ZERO
//            where the halo pixel lies outside the image (the head pads unet, not t) -> the [324][128] tile, pixel pitch 288 bytes
//            (18 slots = 2 mod 4, halo_core.h's rule for several chunks per pixel: the two lane sets of a ds_read_b128 group fall on the
//            even and the odd slots; 17 slots leave one two-way conflict per read).  conv0's weights [128][288] come in five
//            64-deep K-steps through the weight stages.
//   phase 1  GEMM1 = depth_head.conv3x3, transposed as in head_fused.hip (acc1[i][j][r] = ram(ch 16 i + 4 fq + r, px 16 j + fr)); a wave
//            owns two pixel rows of the tile; the B fragment of tap (dy, dx) is a 16-byte read of pixel (y + dy, fr + dx) of the tile.
//            w3 streams in 18 K-steps of 64: LDS-DMA, XOR-swizzled 128-byte rows, two 16 KB stages, head_core.h's stage hand-over
//            (vmcnt AND lgkmcnt(0) before the barrier: the zero words of out-of-range DMA lanes).
//   phase 2  GEMM2 (conv_out from the packed accumulators: ops.permute_wout's K order), softmax, expectation, prob transposed through
//            LDS: head_core.h, the code head_fused.hip runs, on 256 pixels.  Wout half 0 lands in the dead t halo during GEMM1, half 1
//            in the two stages after it; the prob staging tile overlays stages, t halo and the unet tile.
//
// LDS map (162 944 bytes: one workgroup = two waves per SIMD per CU):
//   [      0,  32768)  two weight stages (conv0's K-steps, w3's K-steps, later Wout half 1)
//   [  32768,  65536)  t halo, 400 x 80 bytes (later Wout half 0)
//   [  65536, 158848)  unet halo, 324 x 288 bytes
//   [ 158848, 162944)  f32: conv_out bias [256] | scale3, shift3 [128 each] | bin centres of the image [256] | conv0 scale, shift [128 each]
//   [      0, 135168)  prob staging [256 bins][264] once GEMM2 is done
// Every LDS-DMA destination lies below 64 KB.
#include "head_core.h"

namespace {

constexpr int HC_C = HEAD_C;              // unet / ram channels
constexpr int HC_NB = HEAD_NB;            // bins
constexpr int HC_CIN = 32;                // channels of t
constexpr int HC_K0 = 9 * HC_CIN;         // 288
constexpr int HC_K3 = 9 * HC_C;           // 1152
constexpr int HC_STEPS = HC_K3 / 64;      // 18
constexpr int HC_WSTAGE = HC_C * 128;     // 16 KB: 128 weight rows of one 64-deep K-step
constexpr int HC_TW = 20, HC_TPIX = HC_TW * HC_TW, HC_TP = 80;       // t halo: width, pixels, pixel pitch (5 slots)
constexpr int HC_UW = 18, HC_UPIX = HC_UW * HC_UW, HC_UP = 288;      // unet halo: width, pixels, pixel pitch (18 slots)
constexpr int HC_UGROUPS = (HC_UPIX + 15) / 16;                      // 21 groups of 16 halo pixels
constexpr int HC_OFF_T = 2 * HC_WSTAGE;
constexpr int HC_OFF_U = 65536;
constexpr int HC_OFF_K = HC_OFF_U + HC_UPIX * HC_UP;
constexpr int HC_LDS = HC_OFF_K + HEAD_K_BYTES;
constexpr int HC_BM = 256;                // pixels of a tile
constexpr int HC_PPITCH = HC_BM + 8;      // prob staging pitch (elements)
constexpr unsigned HC_OOB = 0x80000000u;
static_assert(HC_OFF_T + HC_TPIX * HC_TP <= HC_OFF_U, "t halo");
static_assert(HC_NB * HC_PPITCH * 2 <= HC_OFF_K, "prob staging must end before the constants");
static_assert(HC_LDS <= 160 * 1024, "LDS of a CU");

struct HeadC0P {
  const void* t; const void* w0; const float* scale0; const float* shift0;
  const void* w3; const float* scale3; const float* shift3;
  const void* wout; const float* bias_out; const float* centers;
  void* prob; float* pred;
  int t_ld, B, H, W, HW, tiles_x, tiles_y;
  int probe;        // timing probes (tools/head_bench.py): 1 = descriptors with zero records (no fetch), 2 = stop after GEMM1, 4 = stop after GEMM2, 8 = stop after phase 0
};

template <typename H>
__global__ __launch_bounds__(512, 1) void depth_head_conv0_kernel(HeadC0P p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sT = smem + HC_OFF_T;
  unsigned char* sU = smem + HC_OFF_U;
  float* sK = reinterpret_cast<float*>(smem + HC_OFF_K);   // head_core.h's constants block; its last quarter: conv0's scale and shift
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int rsub = lane >> 3;
  const int lc = (lane & 7) ^ rsub;                        // logical 16-byte chunk of the 128-byte K-step row this lane fetches
  int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int x0 = (bid % p.tiles_x) * 16; bid /= p.tiles_x;
  const int y0 = (bid % p.tiles_y) * 16;
  const int b = bid / p.tiles_y;

  const int live = (p.probe & 1) ? 0 : 1;                  // probe: zero records = every load is dropped by the range check
  const auto rs_t = __builtin_amdgcn_make_buffer_rsrc((void*)p.t, 0, (int)((unsigned)p.B * (unsigned)p.HW * (unsigned)p.t_ld * 2u) * live, 0x00020000);
  const auto rs_w0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.w0, 0, HC_C * HC_K0 * 2 * live, 0x00020000);
  const auto rs_w3 = __builtin_amdgcn_make_buffer_rsrc((void*)p.w3, 0, HC_C * HC_K3 * 2 * live, 0x00020000);
  const auto rs_o = __builtin_amdgcn_make_buffer_rsrc((void*)p.wout, 0, HC_NB * HC_C * 2 * live, 0x00020000);

  // ---- weight loaders: a stage is 128 rows x 128 bytes = 16 DMA groups of 8 rows, two per wave ------------------------------------------
  auto issue_w0 = [&](int ks, int buf) {                   // conv0: rows of 576 bytes, the last K-step holds one tap (its second half is masked)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int g = i * 8 + wave;
      const unsigned v = (ks * 8 + lc) * 8 < HC_K0 ? (unsigned)(g * 8 + rsub) * (unsigned)(HC_K0 * 2) + (unsigned)lc * 16u : HC_OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w0, (lds_ptr_t)(smem + buf * HC_WSTAGE + g * 1024), 16, (int)v, ks * 128, 0, 0);
    }
  };
  auto issue_w3 = [&](int ks, int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int g = i * 8 + wave;
      const unsigned v = (unsigned)(g * 8 + rsub) * (unsigned)(HC_K3 * 2) + (unsigned)lc * 16u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w3, (lds_ptr_t)(smem + buf * HC_WSTAGE + g * 1024), 16, (int)v, ks * 128, 0, 0);
    }
  };
  // one half (64 permuted channels) of Wout -> 32 KB at `off`
  auto issue_wout = [&](int half, int off) { head_issue_wout<8>(rs_o, smem + off, half * 128, wave, rsub, lc); };

  issue_w0(0, 0);

  // ---- the t halo: pixels (y0 - 2 .. y0 + 17, x0 - 2 .. x0 + 17), four 16-byte pieces each; all loads in flight, then the LDS stores ----
  {
    u32x4 v[4];
    int dst[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int i = tid + n * 512;
      const int px = i >> 2, ch = i & 3;
      const int hy = px / HC_TW, hx = px - hy * HC_TW;
      const int y = y0 - 2 + hy, x = x0 - 2 + hx;
      const bool ok = px < HC_TPIX && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
      const unsigned off = ok ? (unsigned)((b * p.H + y) * p.W + x) * (unsigned)p.t_ld * 2u + (unsigned)ch * 16u : HC_OOB;
      v[n] = __builtin_amdgcn_raw_buffer_load_b128(rs_t, (int)off, 0, 0);
      dst[n] = px < HC_TPIX ? px * HC_TP + ch * 16 : -1;
    }
    // the per-channel / per-bin vectors of the epilogues wait in LDS from the start (head_fused.hip: loading them at their use costs an
    // exposed global round trip each)
    if (tid < 256) {
      sK[HEAD_K_BIAS + tid] = p.bias_out[tid];
      sK[HEAD_K_CEN + tid] = p.centers[(long long)b * HC_NB + tid];
    } else if (tid < 384) {
      const int u = tid - 256;
      sK[HEAD_K_SCALE3 + u] = p.scale3 ? p.scale3[u] : 1.f;
      sK[HEAD_K_SCALE0 + u] = p.scale0 ? p.scale0[u] : 1.f;
    } else {
      const int u = tid - 384;
      sK[HEAD_K_SHIFT3 + u] = p.shift3 ? p.shift3[u] : 0.f;
      sK[HEAD_K_SHIFT0 + u] = p.shift0 ? p.shift0[u] : 0.f;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
      if (dst[n] >= 0) *reinterpret_cast<u32x4*>(sT + dst[n]) = v[n];
  }

  // ---- phase 0: conv0 on the 18 x 18 halo of unet ----------------------------------------------------------------------------------------
  {
    const int ng = wave + 16 < HC_UGROUPS ? 3 : 2;         // pixel groups of this wave: wave, wave + 8 (, wave + 16)
    int tb[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int q = min((wave + 8 * g) * 16 + fr, HC_UPIX - 1);      // lanes past the last halo pixel repeat it (never stored)
      const int hy = q / HC_UW, hx = q - hy * HC_UW;
      tb[g] = (hy * HC_TW + hx) * HC_TP + fq * 16;                   // tap (0, 0) of unet halo pixel (hy, hx) = t halo pixel (hy, hx)
    }
    f32x4 acc0[3][8];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc0[g][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
      head_handover();                                     // stage ks & 1 (and, first time round, the t halo) landed; the other stage is consumed
      if (ks < 4) issue_w0(ks + 1, (ks + 1) & 1);
      else issue_w3(0, 1);                                 // GEMM1's K-step k reads stage (k + 1) & 1
      const unsigned char* cW = smem + (ks & 1) * HC_WSTAGE;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int tap = 2 * ks + s;
        if (tap >= 9) break;
        const int pc = ((s * 4 + fq) ^ (fr & 7)) * 16;
        const int toff = ((tap / 3) * HC_TW + tap % 3) * HC_TP;
        s16x8 wf[8], xf[3];
#pragma unroll
        for (int i = 0; i < 8; ++i) wf[i] = *reinterpret_cast<const s16x8*>(cW + (i * 16 + fr) * 128 + pc);
#pragma unroll
        for (int g = 0; g < 3; ++g)
          if (g < ng) xf[g] = *reinterpret_cast<const s16x8*>(sT + tb[g] + toff);
#pragma unroll
        for (int g = 0; g < 3; ++g)
          if (g < ng) {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc0[g][i] = mfma16<H>(wf[i], xf[g], acc0[g][i]);      // acc[r] = channel 16 i + 4 fq + r, halo pixel fr of the group
          }
      }
    }
    // conv0's epilogue as conv3x3_halo.hip stores it (acc * scale + shift, rounded to the storage type), zero outside the image
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      if (g >= ng) continue;
      const int q = (wave + 8 * g) * 16 + fr;
      const int hy = q / HC_UW, hx = q - hy * HC_UW;
      const int y = y0 - 1 + hy, x = x0 - 1 + hx;
      const bool inside = (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int ch = i * 16 + fq * 4;
        float sc[4], sh[4], yv[4];
        Vec<float>::load(sK + HEAD_K_SCALE0 + ch, sc);
        Vec<float>::load(sK + HEAD_K_SHIFT0 + ch, sh);
#pragma unroll
        for (int r = 0; r < 4; ++r) yv[r] = acc0[g][i][r] * sc[r] + sh[r];
        uint2 pk;
        pk.x = inside ? pack2<H>(yv[0], yv[1]) : 0u;
        pk.y = inside ? pack2<H>(yv[2], yv[3]) : 0u;
        if (q < HC_UPIX) *reinterpret_cast<uint2*>(sU + q * HC_UP + ch * 2) = pk;
      }
    }
  }
  if (p.probe & 8) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    return;
  }

  // ---- phase 1: GEMM1 from the resident tile; this wave's pixels are rows 2 wave, 2 wave + 1 of the tile, column fr ---------------------
  f32x4 acc1[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const unsigned char* urow = sU + ((2 * wave) * HC_UW + fr) * HC_UP + fq * 16;      // tap (0, 0) of pixel (2 wave, fr)
  for (int ks = 0; ks < HC_STEPS; ++ks) {
    head_handover();                                       // stage (ks + 1) & 1 landed; the other consumed; ks == 0: the unet tile is written, t is dead
    if (ks == 0) issue_wout(0, HC_OFF_T);
    if (ks + 1 < HC_STEPS) issue_w3(ks + 1, ks & 1);
    const int tap = ks >> 1;                               // 128 channels = two K-steps per tap
    const int dy = tap / 3, dx = tap - dy * 3;
    const unsigned char* cP = urow + (dy * HC_UW + dx) * HC_UP + (ks & 1) * 128;
    const unsigned char* cW = smem + ((ks + 1) & 1) * HC_WSTAGE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int pc = ((s * 4 + fq) ^ (fr & 7)) * 16;
      s16x8 wf[8], pf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) pf[j] = *reinterpret_cast<const s16x8*>(cP + j * (HC_UW * HC_UP) + s * 64);
#pragma unroll
      for (int i = 0; i < 8; ++i) wf[i] = *reinterpret_cast<const s16x8*>(cW + (i * 16 + fr) * 128 + pc);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc1[i][j] = mfma16<H>(wf[i], pf[j], acc1[i][j]);
    }
  }
  head_handover();                                         // both stages consumed by every wave (Wout half 0 landed long ago)
  issue_wout(1, 0);                                        // lands while GEMM2 runs on half 0
  if (p.probe & 2) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0 && acc1[0][0][0] == 123.456f) p.pred[0] = acc1[7][1][3];
    return;
  }

  // ---- ram -> B fragments of GEMM2 ------------------------------------------------------------------------------------------------------
  HeadFrags<false> bf;
  head_ram_fragments<H, false>(acc1, sK, fq, bf, [](int, int, const uint32_t (&)[4]) {});

  __builtin_amdgcn_sched_barrier(0);      // acc1 is dead from here: keep the 128 registers of acc2 from being set up above this line

  // ---- GEMM2 -----------------------------------------------------------------------------------------------------------------------------
  f32x4 acc2[16][2];
  head_acc2_init(acc2, sK, fq);
  head_gemm2_half<H, false>(acc2, bf, 0, smem + HC_OFF_T, false, fr, fq);
  head_handover();                                         // Wout half 1 landed
  head_gemm2_half<H, false>(acc2, bf, 1, smem, false, fr, fq);
  if (p.probe & 4) {
    if (tid == 0 && acc2[0][0][0] == 123.456f) p.pred[0] = acc2[15][1][3];
    return;
  }
  __syncthreads();                                         // LDS becomes the prob staging tile

  // ---- softmax over the 256 bins of each pixel + expectation -----------------------------------------------------------------------------
  H* sP = reinterpret_cast<H*>(smem);                      // [256 bins][HC_PPITCH]
  H* prob = reinterpret_cast<H*>(p.prob);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int pl = wave * 32 + j * 16 + fr;                // pixel within the tile: row 2 wave + j, column fr
    // no STATS here: the moments it returns are zeros and go unused
    head_softmax_column<H, false, HC_PPITCH>(acc2, j, sK + HEAD_K_CEN, prob != nullptr, sP + pl, fq, [&](float dot) {
      if (fq == 0) p.pred[(long long)b * p.HW + (y0 + 2 * wave + j) * p.W + x0 + fr] = dot;
    });
  }
  if (!prob) return;
  __syncthreads();
  // NCHW copy-out: 256 bin rows x 16 tile rows x 2 chunks of 8 pixels
#pragma unroll 4
  for (int q = tid; q < HC_NB * 32; q += 512) {
    const int n = q >> 5, c = q & 31;
    const int row = c >> 1, half = c & 1;
    *reinterpret_cast<u32x4*>(prob + ((long long)b * HC_NB + n) * p.HW + (y0 + row) * p.W + x0 + half * 8) =
        *reinterpret_cast<const u32x4*>(sP + n * HC_PPITCH + row * 16 + half * 8);
  }
}

}  // namespace

extern "C" int cfp_depth_head_conv0_fused(const void* t, int t_ld, const void* w0, const float* scale0, const float* shift0, const void* w3,
                                          const float* scale3, const float* shift3, const void* wout_perm, const float* bias_out,
                                          const float* centers, void* prob, float* pred, int B, int H, int W, int flags, int dtype,
                                          cfp_stream_t stream) {
  CFP_REQUIRE(is16(dtype), CFP_EINVAL, "cfp_depth_head_conv0_fused: bf16/f16 only");
  CFP_REQUIRE(t && w0 && w3 && wout_perm && bias_out && centers && pred, CFP_EINVAL, "cfp_depth_head_conv0_fused: null pointer");
  CFP_REQUIRE(B > 0 && H > 0 && W > 0 && t_ld >= HC_CIN && t_ld % 8 == 0, CFP_ESHAPE, "cfp_depth_head_conv0_fused: bad shape (32 input channels, t_ld % 8 == 0)");
  CFP_REQUIRE(H % 16 == 0 && W % 16 == 0, CFP_ESHAPE, "cfp_depth_head_conv0_fused: H and W must be multiples of the 16 x 16 tile");
  const long long M = (long long)B * H * W;
  CFP_REQUIRE(M * t_ld * 2 < (1ll << 31) - 4096 && M / 256 < (1ll << 31), CFP_ESHAPE, "cfp_depth_head_conv0_fused: input larger than 2 GB");
  CFP_REQUIRE(aligned16(t) && aligned16(w0) && aligned16(w3) && aligned16(wout_perm) && aligned16(prob) && aligned16(bias_out) && aligned16(centers) &&
                  aligned16(scale0) && aligned16(shift0) && aligned16(scale3) && aligned16(shift3), CFP_EINVAL,
              "cfp_depth_head_conv0_fused: pointers must be 16-byte aligned");
  CFP_REQUIRE((flags & ~(15 << 8)) == 0, CFP_EINVAL, "cfp_depth_head_conv0_fused: unknown flags");
  static int lds_max = -1;
  if (lds_max < 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
      cfp_set_error("cfp_depth_head_conv0_fused: cannot query the LDS size");
      return CFP_EHIP;
    }
    lds_max = v;
  }
  CFP_REQUIRE(lds_max >= HC_LDS, CFP_ESHAPE, "cfp_depth_head_conv0_fused: the device does not grant 162944 bytes of LDS to a workgroup");
  HeadC0P p;
  p.t = t; p.w0 = w0; p.scale0 = scale0; p.shift0 = shift0; p.w3 = w3; p.scale3 = scale3; p.shift3 = shift3;
  p.wout = wout_perm; p.bias_out = bias_out; p.centers = centers; p.prob = prob; p.pred = pred;
  p.t_ld = t_ld; p.B = B; p.H = H; p.W = W; p.HW = H * W; p.tiles_x = W / 16; p.tiles_y = H / 16;
  p.probe = (flags >> 8) & 15;
  const int grid = (int)(M / HC_BM);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define HC_LAUNCH(T)                                                                                                                       \
  do {                                                                                                                                     \
    static bool attr = false;                                                                                                              \
    if (!attr) {                                                                                                                           \
      if (hipFuncSetAttribute((const void*)depth_head_conv0_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, HC_LDS) != hipSuccess) { \
        cfp_set_error("cfp_depth_head_conv0_fused: cannot set the LDS size");                                                              \
        return CFP_EHIP;                                                                                                                   \
      }                                                                                                                                    \
      attr = true;                                                                                                                         \
    }                                                                                                                                      \
    hipLaunchKernelGGL((depth_head_conv0_kernel<T>), dim3(grid), dim3(512), HC_LDS, s, p);                                                 \
  } while (0)
  if (dtype == CFP_F16) HC_LAUNCH(f16_t);
  else HC_LAUNCH(bf16_t);
#undef HC_LAUNCH
  return cfp_check_launch("cfp_depth_head_conv0_fused");
}
