// Fused tail of a LoFTR encoder layer (transformer.py:48-71, attention.py:48-49), bf16:
//
//   msg = (Q' KV[g]) / (Q' . Ksum[g] + eps) * S          linear-attention apply, per head
//   y1  = LayerNorm1(msg @ Wm^T)                          merge + norm1
//   h   = relu([x | y1] @ W0^T)                           mlp.0 (the concat is a split K range)
//   out = LayerNorm2(h @ W2^T) + x                        mlp.2 + norm2 + residual
//
// Unfused this is 4-5 launches per layer (apply, merge+LN, mlp0, mlp2+LN) over tensors of a few MB,
// 18 layers per forward.  Here a wave owns 16 token rows from the apply to the final store: its
// msg / y1 / x / h tiles live in a private LDS region (row pitch padded by 16 bytes, so the MFMA
// A-operand read of 16 rows is conflict-free), and only the weights are shared: each GEMM streams
// its [N][64] weight slabs global -> LDS with `global_load_lds_dwordx4` (XOR-swizzled 128-byte rows,
// double buffered, one barrier per 64-wide K step).  Rows never leave their wave, so both
// LayerNorms are a 16-lane shuffle reduction over the accumulator registers.
// Rounding points match the unfused path (msg, the GEMM outputs before each LayerNorm and h are
// rounded to bf16), so the two paths agree to accumulation order.
#include "tail_core.h"

namespace {

// One GEMM of the chain for this wave's 16 rows: acc[j] += A[16 x K] * W[N x K]^T, N = NT * 16.
// `afrag(k)` returns the lane's A fragment for columns [k, k + 32) of the wave-private operand.
// All four waves of the workgroup must call it together (they share the weight slabs).
template <typename H, int NT, int BSTAGE, int WAVES, typename AF>
__device__ __forceinline__ void tail_gemm(f32x4 (&acc)[NT], const H* __restrict__ W, int K, AF afrag, unsigned char* sB,
                                          int wave, int lane) {
  constexpr int N = NT * 16;
  constexpr int NBG = N / 8;                  // 8-row DMA groups of a weight slab
  constexpr int NBW = (NBG + WAVES - 1) / WAVES;      // LDS-DMA instructions per wave and slab
  // weight slabs of THIS GEMM are N * 128 bytes; the region holds 2 * BSTAGE bytes (two slabs of the widest GEMM, N = 2 D): the N = D GEMMs
  // fit three of theirs in it and keep two K-steps of DMA in flight (tail_ring_step)
  constexpr int SST = N * 128;
  constexpr int STG = (3 * SST <= 2 * BSTAGE) ? 3 : 2;
  const int fr = lane & 15, fq = lane >> 4;
  const int rsub = lane >> 3;
  const int lc = (lane & 7) ^ rsub;
  const H* zsrc = reinterpret_cast<const H*>(g_zero16);
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = (K + 63) >> 6;
  auto issue = [&](int ks, int st) {
    const int kk = ks * 64 + lc * 8;
    const bool kok = kk < K;
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      const int g = (j * WAVES + wave) % NBG;
      const int n = g * 8 + rsub;
      glds16(kok ? W + (long long)n * K + kk : zsrc, sB + st * SST + g * 1024);
    }
  };
  tail_ring_begin<STG, NBW>(nk, issue);
  for (int ks = 0; ks < nk; ++ks) {
    const unsigned char* cB = sB + tail_ring_step<STG, NBW>(ks, nk, issue) * SST;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int k = ks * 64 + sub * 32;
      if (k < K) {                            // uniform
        const s16x8 a = afrag(k);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const s16x8 b = *reinterpret_cast<const s16x8*>(cB + (j * 16 + fr) * 128 + (((sub * 4 + fq) ^ (fr & 7)) * 16));
          acc[j] = mfma16<H>(a, b, acc[j]);
        }
      }
    }
  }
}

// WAVES waves of 16 token rows per workgroup: 4, or 1 / 2 for few token rows (tail_waves).
// MAP (cfp_loftr_tail_x2i): the rows are a zone grid laid 1:1 over a rectangle of the token map -- x is read from the map and the output is
// pasted into it (tail_core.h); everything between the first load and the final store is the plain kernel's code.
template <typename H, int D, int HEADS, int WAVES, bool MAP = false>
__global__ __launch_bounds__(64 * WAVES) void loftr_tail_kernel(TailP<H, H> p) {
  constexpr int PA = D + 8, PH = 2 * D + 8;               // row pitches (elements): +16 bytes
  constexpr int WAVE_LDS = (2 * PA + PH) * 16 * 2;         // msg/y1 | x | h tiles of one wave
  constexpr int BSTAGE = 2 * D * 128;                      // largest weight slab: [2D rows][64 k]
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  unsigned char* sB = smem;
  H* tMsg = reinterpret_cast<H*>(smem + 2 * BSTAGE + wave * WAVE_LDS);
  H* tX = tMsg + 16 * PA;
  H* tH = tX + 16 * PA;
  const long long row0 = (long long)blockIdx.x * (16 * WAVES) + wave * 16;

  // ---- x tile -> LDS (16-byte vectors) -----------------------------------------------------------
  if constexpr (MAP) tail_tile_load_mapped<H, D, PA>(tX, p, row0, lane);
  else tail_tile_load<H, D, PA>(tX, p.x, p.x_ld, row0, p.rows, lane);

  // ---- optional q projection for this wave's rows (transformer.py:45: q = q_proj(x)): one more GEMM of the chain instead of a separate
  // launch that writes [rows, D] and is read back here; q is rounded to the storage type like the unfused GEMM's output ----------------
  const bool own_q = p.wq != nullptr;
  if (own_q) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    f32x4 acc[D / 16];
    tail_gemm<H, D / 16, BSTAGE, WAVES>(acc, p.wq, D, [&](int k) { return *reinterpret_cast<const s16x8*>(tX + fr * PA + k + fq * 8); }, sB, wave, lane);
#pragma unroll
    for (int j = 0; j < D / 16; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) tH[(fq * 4 + r) * PH + j * 16 + fr] = from_f32<H>(acc[j][r]);     // the hidden tile is free until mlp.0
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }

  // ---- linear-attention apply: lane = (row, head slot) --------------------------------------------
  tail_attn_apply<H, D, HEADS, PA, PH>(p, row0, tH, tMsg, fr, fq);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- merge + norm1 -------------------------------------------------------------------------------
  {
    f32x4 acc[D / 16];
    tail_gemm<H, D / 16, BSTAGE, WAVES>(acc, p.wm, D, [&](int k) { return *reinterpret_cast<const s16x8*>(tMsg + fr * PA + k + fq * 8); }, sB, wave, lane);
    tail_layernorm<D / 16, H>(acc, p.g1, p.b1, p.ln_eps, fr);
#pragma unroll
    for (int j = 0; j < D / 16; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) tMsg[(fq * 4 + r) * PA + j * 16 + fr] = from_f32<H>(acc[j][r]);   // y1 replaces msg
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- mlp.0: [x | y1] (K = 2D) -> 2D, ReLU ---------------------------------------------------------
  {
    f32x4 acc[2 * D / 16];
    tail_gemm<H, 2 * D / 16, BSTAGE, WAVES>(acc, p.w0, 2 * D, [&](int k) {
      const H* src = k < D ? tX + fr * PA + k : tMsg + fr * PA + (k - D);
      return *reinterpret_cast<const s16x8*>(src + fq * 8);
    }, sB, wave, lane);
#pragma unroll
    for (int j = 0; j < 2 * D / 16; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) tH[(fq * 4 + r) * PH + j * 16 + fr] = from_f32<H>(fmaxf(acc[j][r], 0.f));
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- mlp.2 (K = 2D) -> D, norm2, + x ---------------------------------------------------------------
  {
    f32x4 acc[D / 16];
    tail_gemm<H, D / 16, BSTAGE, WAVES>(acc, p.w2, 2 * D, [&](int k) { return *reinterpret_cast<const s16x8*>(tH + fr * PH + k + fq * 8); }, sB, wave, lane);
    tail_layernorm<D / 16, H>(acc, p.g2, p.b2, p.ln_eps, fr);
#pragma unroll
    for (int j = 0; j < D / 16; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = fq * 4 + r, col = j * 16 + fr;
        tMsg[row * PA + col] = from_f32<H>(acc[j][r] + to_f32<H>(tX[row * PA + col]));     // stage the output tile
      }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if constexpr (MAP) tail_tile_store_mapped<H, D, PA>(p, tMsg, row0, lane);
  else tail_tile_store<H, D, PA>(p.out, p.out_ld, tMsg, row0, p.rows, lane);
}

// ---- LKPM tail (Block14.forward after the depthwise conv, convnext.py:48-58): LayerNorm(1e-6) -> pwconv1 (D -> 4D) -> GELU ->
// pwconv2 (4D -> D) -> + input, for the 16 token rows of a wave, with the same machinery as the LoFTR tail: the 4D-wide hidden tile
// lives in the wave's LDS region and never reaches HBM (unfused: a LayerNorm launch, two GEMM launches and 2 x 4D x 2 bytes per
// token of traffic -- 79 MB at the 1/4 scale of a batch of 8).  pwconv1 runs in two halves of 2D output channels so that its weight
// slabs ([2D][64], double buffered) and the four waves' tiles fit the LDS at D = 128.
template <typename H, int D>
__global__ __launch_bounds__(256) void lkpm_tail_kernel(LkpmP<H, H> p) {
  constexpr int PA = D + 8, PH = 4 * D + 8;               // row pitches (elements): +16 bytes
  constexpr int WAVE_LDS = (PA + PH) * 16 * 2;            // normalised-input / output tile | hidden tile of one wave
  constexpr int BSTAGE = 2 * D * 128;                     // largest weight slab: [2D rows][64 k]
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  unsigned char* sB = smem;
  H* tA = reinterpret_cast<H*>(smem + 2 * BSTAGE + wave * WAVE_LDS);
  H* tH = tA + 16 * PA;
  const long long row0 = (long long)blockIdx.x * 64 + wave * 16;
  constexpr int XCH = D / 8;                               // 16-byte chunks per row

  // ---- t tile -> LDS, LayerNorm over the D channels of each row ------------------------------------------------------------------------
  tail_tile_load<H, D, PA>(tA, p.t, p.t_ld, row0, p.rows, lane);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  tail_row_layernorm<H, D, PA>(tA, p.lg, p.lb, p.ln_eps, fr, fq);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- pwconv1 + GELU: two halves of 2D hidden channels ------------------------------------------------------------------------------
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    f32x4 acc[2 * D / 16];
    tail_gemm<H, 2 * D / 16, BSTAGE, 4>(acc, p.w1 + (long long)half * 2 * D * D, D,
                                     [&](int k) { return *reinterpret_cast<const s16x8*>(tA + fr * PA + k + fq * 8); }, sB, wave, lane);
#pragma unroll
    for (int j = 0; j < 2 * D / 16; ++j) {
      const float bj = p.b1[half * 2 * D + j * 16 + fr];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        tH[(fq * 4 + r) * PH + half * 2 * D + j * 16 + fr] = from_f32<H>(act_c16<CFP_ACT_GELU>(acc[j][r] + bj));
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- pwconv2 (K = 4D) + bias, staged in FLOAT32 over the (consumed) hidden tile; the residual is added on the way out, so the
  // output is rounded once, like the unfused GEMM epilogue does -----------------------------------------------------------------------
  constexpr int PF = D + 4;                                // floats per staged row (16 x PF x 4 <= 16 x PH x 2)
  float* tF = reinterpret_cast<float*>(tH);
  {
    f32x4 acc[D / 16];
    tail_gemm<H, D / 16, BSTAGE, 4>(acc, p.w2, 4 * D, [&](int k) { return *reinterpret_cast<const s16x8*>(tH + fr * PH + k + fq * 8); }, sB, wave, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's reads of tH are complete (tail_gemm consumed them)
#pragma unroll
    for (int j = 0; j < D / 16; ++j) {
      const float bj = p.b2[j * 16 + fr];
#pragma unroll
      for (int r = 0; r < 4; ++r) tF[(fq * 4 + r) * PF + j * 16 + fr] = acc[j][r] + bj;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  for (int i = lane; i < 16 * XCH; i += 64) {
    const int r = i / XCH, ch = i - r * XCH;
    const long long m = row0 + r;
    if (m < p.rows) {
      float a[8], b[8];
      Vec<float>::load(tF + r * PF + ch * 8, a);
      Vec<float>::load(tF + r * PF + ch * 8 + 4, a + 4);
      Vec<H>::load(p.xin + m * p.x_ld + ch * 8, b);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += b[e];
      Vec<H>::store(p.out + m * p.out_ld + ch * 8, a);
    }
  }
}

int g_tail16_waves = 0;      // cfp_debug_set key 39: 0 = by the row count, else 1 / 2 / 4 waves per workgroup of the LoFTR tail (A/B)

}  // namespace

void cfp_tail16_debug_set(int value) { g_tail16_waves = value; }

// dtype: bf16 / f16 storage (the kernels above) or CFP_F32X3: float32 tensors, f16x3 matrix math, weights = cfp_pack_w_x3 operands
// (loftr_tail_x3.hip).  The checks are the same up to the elements per 16-byte vector.
// `map` == nullptr: cfp_loftr_tail; otherwise cfp_loftr_tail_x2i (16-bit only, checked there)
static int loftr_tail_impl(const void* q, int q_ld, const float* kv, const float* ksum, const void* x, int x_ld,
                           void* out, int out_ld, const void* w_q, const void* w_merge, const void* w_mlp0, const void* w_mlp2,
                           const float* ln1_g, const float* ln1_b, const float* ln2_g, const float* ln2_b, float ln_eps,
                           int NB, int Hq, int Wq, int qth, int qtw, float v_length, float eps, int heads, int D,
                           int dtype, cfp_stream_t stream, const TailMap* map) {
  const bool x3 = dtype == CFP_F32X3;
  const int vec = x3 ? 4 : 8;                 // pitch multiple = 16 / sizeof(storage element)
  // rows < 2^31 (FastDiv, int row indices).  The float32 side has always reported it with the grid and the 16-bit side after the alignment:
  // kept, so that an input that fails several checks gets the code it always got.
  const bool rows_ok = (long long)NB * Hq * Wq < (1ll << 31);
  CFP_REQUIRE(x3 || is16(dtype), CFP_EINVAL, "cfp_loftr_tail: bf16 / f16 or CFP_F32X3 (the plain f32 parity mode uses the unfused kernels)");
  CFP_REQUIRE((q || w_q) && kv && ksum && x && out && w_merge && w_mlp0 && w_mlp2 && ln1_g && ln1_b && ln2_g && ln2_b, CFP_EINVAL,
              "cfp_loftr_tail: null pointer (q or w_q must be given)");
  CFP_REQUIRE(NB > 0 && Hq > 0 && Wq > 0 && qth > 0 && qtw > 0 && v_length > 0.f && (rows_ok || !x3), CFP_ESHAPE, "cfp_loftr_tail: bad grid");
  CFP_REQUIRE((D == 32 || D == 64 || D == 128) && (heads == 4 || heads == 8), CFP_ESHAPE, "cfp_loftr_tail: D must be 32/64/128 and heads 4/8");
  CFP_REQUIRE((w_q || (q_ld >= D && q_ld % vec == 0)) && x_ld >= D && out_ld >= D && x_ld % vec == 0 && out_ld % vec == 0, CFP_ESHAPE,
              "cfp_loftr_tail: pitches must be >= D and multiples of " + std::to_string(vec));
  CFP_REQUIRE(aligned16(q) && aligned16(w_q) && aligned16(x) && aligned16(out) && aligned16(w_merge) && aligned16(w_mlp0) && aligned16(w_mlp2) &&
                  aligned16(kv), CFP_EINVAL, "cfp_loftr_tail: pointers must be 16-byte aligned");
  CFP_REQUIRE(rows_ok, CFP_ESHAPE, "cfp_loftr_tail: too many rows");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto params = [&](auto t, auto w) {
    return tail_params<decltype(t), decltype(w)>(q, q_ld, kv, ksum, x, x_ld, out, out_ld, w_q, w_merge, w_mlp0, w_mlp2, ln1_g, ln1_b, ln2_g, ln2_b,
                                                 ln_eps, NB, Hq, Wq, qth, qtw, v_length, eps);
  };
  auto run = [&](auto tag) {
    using H = decltype(tag);
    TailP<H, H> p = params(tag, tag);
    if (map) p.map = *map;
    return tail_pick<32, 64, 128>(D, [&](auto d) { return tail_pick<4, 8>(heads, [&](auto h) {
      return tail_pick<1, 2, 4>(tail_waves(p.rows, g_tail16_waves), [&](auto w) {
        constexpr int D_ = d, W_ = w;
        constexpr size_t lds = 2 * (2 * D_ * 128) + W_ * ((2 * (D_ + 8) + 2 * D_ + 8) * 16 * 2);      // weight region + the waves' tiles
        if (map) return tail_launch<loftr_tail_kernel<H, D_, h, W_, true>, lds>(p, W_, s);
        return tail_launch<loftr_tail_kernel<H, D_, h, W_>, lds>(p, W_, s);
      }); }); });
  };
  const int rc = x3 ? loftr_tail_x3_launch(params(float{}, f16_t{}), heads, D, s) : dtype == CFP_F16 ? run(f16_t{}) : run(bf16_t{});
  CFP_REQUIRE(rc == 0, CFP_EHIP, x3 ? "cfp_loftr_tail: f16x3 launch failed" : "cfp_loftr_tail: launch failed");
  return cfp_check_launch("cfp_loftr_tail");
}

extern "C" int cfp_loftr_tail(const void* q, int q_ld, const float* kv, const float* ksum, const void* x, int x_ld,
                              void* out, int out_ld, const void* w_q, const void* w_merge, const void* w_mlp0, const void* w_mlp2,
                              const float* ln1_g, const float* ln1_b, const float* ln2_g, const float* ln2_b, float ln_eps,
                              int NB, int Hq, int Wq, int qth, int qtw, float v_length, float eps, int heads, int D,
                              int dtype, cfp_stream_t stream) {
  return loftr_tail_impl(q, q_ld, kv, ksum, x, x_ld, out, out_ld, w_q, w_merge, w_mlp0, w_mlp2, ln1_g, ln1_b, ln2_g, ln2_b, ln_eps, NB, Hq, Wq, qth, qtw,
                         v_length, eps, heads, D, dtype, stream, nullptr);
}

extern "C" int cfp_loftr_tail_x2i(const float* kv, const float* ksum, void* tok, int tok_ld, int H, int W, int sy, int sx,
                                  const void* w_q, const void* w_merge, const void* w_mlp0, const void* w_mlp2,
                                  const float* ln1_g, const float* ln1_b, const float* ln2_g, const float* ln2_b, float ln_eps,
                                  int NB, int gh, int gw, int p1, int p2, const uint8_t* zone_valid, int zn, int accumulate,
                                  float v_length, float eps, int heads, int D, int dtype, cfp_stream_t stream) {
  CFP_REQUIRE(is16(dtype), CFP_EINVAL, "cfp_loftr_tail_x2i: bf16 / f16 only");
  CFP_REQUIRE(tok && w_q, CFP_EINVAL, "cfp_loftr_tail_x2i: null pointer (the kernel projects q itself: w_q must be given)");
  CFP_REQUIRE(H > 0 && W > 0 && p1 > 0 && p2 > 0 && (long long)NB * H * W < (1ll << 31), CFP_ESHAPE, "cfp_loftr_tail_x2i: bad token map");
  CFP_REQUIRE(!zone_valid || (zn > 0 && gh <= zn * p1 && gw <= zn * p2), CFP_ESHAPE, "cfp_loftr_tail_x2i: zone grid smaller than the query grid");
  TailMap map;
  map.zone_valid = zone_valid; map.H = H; map.W = W; map.sy = sy; map.sx = sx; map.zn = zn; map.p1 = p1; map.p2 = p2; map.accumulate = accumulate;
  return loftr_tail_impl(nullptr, 0, kv, ksum, tok, tok_ld, tok, tok_ld, w_q, w_merge, w_mlp0, w_mlp2, ln1_g, ln1_b, ln2_g, ln2_b, ln_eps, NB, gh, gw,
                         p1, p2, v_length, eps, heads, D, dtype, stream, &map);
}

extern "C" int cfp_lkpm_tail(const void* t, int t_ld, const void* xin, int x_ld, void* out, int out_ld, const void* w1, const float* b1,
                             const void* w2, const float* b2, const float* ln_g, const float* ln_b, float ln_eps, int rows, int D, int dtype,
                             cfp_stream_t stream) {
  const bool x3 = dtype == CFP_F32X3;
  const int vec = x3 ? 4 : 8;                 // pitch multiple = 16 / sizeof(storage element)
  CFP_REQUIRE(x3 || is16(dtype), CFP_EINVAL, "cfp_lkpm_tail: bf16 / f16 or CFP_F32X3 (the plain f32 parity mode uses the unfused kernels)");
  CFP_REQUIRE(t && xin && out && w1 && b1 && w2 && b2 && ln_g && ln_b, CFP_EINVAL, "cfp_lkpm_tail: null pointer");
  CFP_REQUIRE(rows > 0 && (D == 32 || D == 64 || D == 128), CFP_ESHAPE, "cfp_lkpm_tail: D must be 32/64/128");
  CFP_REQUIRE(t_ld >= D && x_ld >= D && out_ld >= D && t_ld % vec == 0 && x_ld % vec == 0 && out_ld % vec == 0, CFP_ESHAPE,
              "cfp_lkpm_tail: pitches must be >= D and multiples of " + std::to_string(vec));
  CFP_REQUIRE(aligned16(t) && aligned16(xin) && aligned16(out) && aligned16(w1) && aligned16(w2), CFP_EINVAL, "cfp_lkpm_tail: pointers must be 16-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto params = [&](auto tt, auto w) {
    return lkpm_params<decltype(tt), decltype(w)>(t, t_ld, xin, x_ld, out, out_ld, w1, b1, w2, b2, ln_g, ln_b, ln_eps, rows);
  };
  auto run = [&](auto tag) {
    using H = decltype(tag);
    const LkpmP<H, H> p = params(tag, tag);
    return tail_pick<32, 64, 128>(D, [&](auto d) {
      constexpr int D_ = d;
      constexpr size_t lds = 2 * (2 * D_ * 128) + 4 * (((D_ + 8) + (4 * D_ + 8)) * 16 * 2);      // weight region + four waves' tiles
      return tail_launch<lkpm_tail_kernel<H, D_>, lds>(p, 4, s);
    });
  };
  const int rc = x3 ? lkpm_tail_x3_launch(params(float{}, f16_t{}), D, s) : dtype == CFP_F16 ? run(f16_t{}) : run(bf16_t{});
  CFP_REQUIRE(rc == 0, CFP_EHIP, x3 ? "cfp_lkpm_tail: f16x3 launch failed" : "cfp_lkpm_tail: launch failed");
  return cfp_check_launch("cfp_lkpm_tail");
}
