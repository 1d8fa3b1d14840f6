// Implicit-GEMM convolution / linear layer on the CDNA4 matrix cores.
//
//   C[m, n] = sum_k A[m, k] * Wt[n, k]        m = (b, ho, wo)   k = (kh, kw, ci)   n = cout
//
// A is never materialised: each 16-byte chunk of a row of A (8 bf16 / 4 f32 consecutive input
// channels of one filter tap) is one global load from the NHWC activation, or zeros at the
// image border.  Weights are pre-packed [Cout][KH*KW*Cin], so both operands are K-contiguous.
//
// Workgroup = 256 threads = 4 waves laid out WM x WN over a BM x BN output tile; every wave
// owns (BM/WM) x (BN/WN) outputs as 16x16 MFMA accumulators.
//   bf16 : v_mfma_f32_16x16x32_bf16, BK = 32 (64-byte tile rows)
//   f32  : v_mfma_f32_16x16x4_f32 (exact f32 FMA chain), BK = 16 -- the parity mode
// Tiles are staged global -> registers -> LDS with the next K-step's loads in flight during the
// MFMAs (double-buffered LDS, one barrier per K-step; igemm_core.h).  LDS rows are 64 bytes with
// a 16-byte chunk XOR swizzle chosen so every ds_read_b128 lane group of the 16x16x32 operand
// pattern hits 64 distinct banks.
// Epilogue: per-channel scale/shift (folded BatchNorm or bias), activation, optional residual;
// bf16 results go through LDS so global stores are full 16-byte vectors along the channel axis.
//
// Split-K: layers with few output tiles but a long K (the GSA "sr" convs: M = 240..1040,
// K = 4608..5184; the 1/32-scale pointwise convs) would run a handful of workgroups through
// 100+ serial K-steps.  They are cut into `splits` K-ranges writing f32 partial slabs
// [split][M][Cout] to a caller-provided workspace; a second kernel sums the slabs in split order
// (deterministic) and applies the epilogue.
#include "igemm_core.h"

namespace {

template <typename T, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvP p) {
  constexpr int VE = Vec<T>::N;
  constexpr int BK = 4 * VE;
  constexpr int TM = BM / WM / 16;
  constexpr int TN = BN / WN / 16;
  constexpr bool kBf16 = sizeof(T) == 2;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (BM + BN) * 64];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int fr = lane & 15, fq = lane >> 4;
  const int tiles_n = (p.Cout + BN - 1) / BN;
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = lbid / tiles_n;
  const int tile_n = lbid % tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  f32x4 acc[TM][TN];
  igemm_mainloop<T, BM, BN, WM, WN>(p, m0, n0, 0, (p.K + BK - 1) / BK, smem, acc);

  // accumulator layout (16x16): col = lane & 15, row = (lane >> 4) * 4 + reg
  T* __restrict__ out = reinterpret_cast<T*>(p.out);
  const T* __restrict__ res = reinterpret_cast<const T*>(p.res);
  float sc[TN], sh[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    int n = n0 + wn * (BN / WN) + j * 16 + fr;
    bool ok = n < p.Cout;
    sc[j] = (ok && p.scale) ? p.scale[n] : 1.f;
    sh[j] = (ok && p.shift) ? p.shift[n] : 0.f;
  }

  if constexpr (kBf16) {
    // C-tile pitch (elements): padded by one 16-byte chunk when the operand LDS has room
    constexpr int CP = (BM * (BN + 8) * 2 <= 2 * (BM + BN) * 64) ? BN + 8 : BN;
    static_assert(BM * CP * 2 <= 2 * (BM + BN) * 64, "C tile must fit in the operand LDS");
    T* sC = reinterpret_cast<T*>(smem);
    with_act(p.act, [&](auto A) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int row = wm * (BM / WM) + i * 16 + fq * 4 + r;
            int col = wn * (BN / WN) + j * 16 + fr;
            sC[row * CP + col] = from_f32<T>(act_c16<decltype(A)::value>(acc[i][j][r] * sc[j] + sh[j]));
          }
    });
    __syncthreads();
    if (p.mom != nullptr) tile_moments<T, BN, 256>(sC, CP, min(BM, p.M - m0), n0, p.Cout, p.mom + (long long)tile_m * 2 * p.Cout, tid);
    constexpr int CH = BN / 8;   // 16-byte chunks per tile row
    for (int q = tid; q < BM * CH; q += 256) {
      int row = q / CH, ch = q % CH;
      int m = m0 + row, n = n0 + ch * 8;
      if (m >= p.M || n >= p.Cout) continue;
      u32x4 v = *reinterpret_cast<const u32x4*>(sC + row * CP + ch * 8);
      if (res) {
        float a[8], b[8];
        Vec<T>::load(reinterpret_cast<const T*>(&v), a);
        Vec<T>::load(res + (long long)m * p.res_ld + n, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += b[e];
        Vec<T>::store(reinterpret_cast<T*>(&v), a);
      }
      *reinterpret_cast<u32x4*>(out + (long long)m * p.out_ld + n) = v;
    }
  } else {
    with_act(p.act, [&](auto A) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][j][r] = act_c<decltype(A)::value>(acc[i][j][r] * sc[j] + sh[j]);
    });
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int m = m0 + wm * (BM / WM) + i * 16 + fq * 4 + r;
          int n = n0 + wn * (BN / WN) + j * 16 + fr;
          if (m < p.M && n < p.Cout) {
            float v = acc[i][j][r];
            if (res) v += to_f32<T>(res[(long long)m * p.res_ld + n]);
            out[(long long)m * p.out_ld + n] = from_f32<T>(v);
          }
        }
  }
}

// Split-K: grid = tiles x splits; raw f32 accumulators to slab[split][m][n].
template <typename T, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void conv_igemm_splitk_kernel(ConvP p, float* __restrict__ slabs, int splits) {
  constexpr int VE = Vec<T>::N;
  constexpr int BK = 4 * VE;
  constexpr int TM = BM / WM / 16;
  constexpr int TN = BN / WN / 16;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (BM + BN) * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN, fr = lane & 15, fq = lane >> 4;
  const int tiles_n = (p.Cout + BN - 1) / BN;
  const int tile = blockIdx.x / splits, sp = blockIdx.x % splits;
  const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
  const int nk = (p.K + BK - 1) / BK;
  const int per = (nk + splits - 1) / splits;
  const int k0 = sp * per, k1 = min(nk, k0 + per);
  f32x4 acc[TM][TN];
  if (k0 < k1) {   // uniform over the workgroup
    igemm_mainloop<T, BM, BN, WM, WN>(p, m0, n0, k0, k1, smem, acc);
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float* slab = slabs + (long long)sp * p.M * p.Cout;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int m = m0 + wm * (BM / WM) + i * 16 + fq * 4 + r;
        int n = n0 + wn * (BN / WN) + j * 16 + fr;
        if (m < p.M && n < p.Cout) slab[(long long)m * p.Cout + n] = acc[i][j][r];
      }
}

template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ slabs, int splits, ConvP p) {
  constexpr int VE = Vec<T>::N;
  const int CV = p.Cout / VE;
  const long long total = (long long)p.M * CV;
  T* __restrict__ out = reinterpret_cast<T*>(p.out);
  const T* __restrict__ res = reinterpret_cast<const T*>(p.res);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int cv = (int)(i % CV);
    const long long m = i / CV;
    const int n = cv * VE;
    float v[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) v[e] = 0.f;
    for (int s = 0; s < splits; ++s) {
      const float* sp = slabs + ((long long)s * p.M + m) * p.Cout + n;
#pragma unroll
      for (int e = 0; e < VE; e += 4) {
        f32x4 x = *reinterpret_cast<const f32x4*>(sp + e);
        v[e] += x[0]; v[e + 1] += x[1]; v[e + 2] += x[2]; v[e + 3] += x[3];
      }
    }
    with_act(p.act, [&](auto A) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        float sc = p.scale ? p.scale[n + e] : 1.f, sh = p.shift ? p.shift[n + e] : 0.f;
        if constexpr (sizeof(T) == 2) v[e] = act_c16<decltype(A)::value>(v[e] * sc + sh);      // like the gen-2 epilogue: same results whether K was split or not
        else v[e] = act_c<decltype(A)::value>(v[e] * sc + sh);
      }
    });
    if constexpr (sizeof(T) == 4) {
      if (p.ln_gamma != nullptr) {
        // LayerNorm over the Cout channels of the row, fused into the finishing sum (round 5: the global attention's patch conv is a split-K
        // GEMM followed by nn.LayerNorm -- twins.py sr + norm).  A row is CV = Cout / 4 consecutive lanes (host: a power of two <= 64 and
        // Cout a multiple of 4), all in one wave and all in this iteration together; two-pass statistics as cfp_layernorm.
        float sum = (v[0] + v[1]) + (v[2] + v[3]);
        for (int o = 1; o < CV; o <<= 1) sum += __shfl_xor(sum, o, 64);
        const float mean = sum / (float)p.Cout;
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < VE; ++e) { v[e] -= mean; q = fmaf(v[e], v[e], q); }
        for (int o = 1; o < CV; o <<= 1) q += __shfl_xor(q, o, 64);
        const float rstd = rsqrtf(q / (float)p.Cout + p.ln_eps);
#pragma unroll
        for (int e = 0; e < VE; ++e) v[e] = v[e] * rstd * p.ln_gamma[n + e] + p.ln_beta[n + e];
      }
    }
    if (res) {
      float r[VE];
      Vec<T>::load(res + m * p.res_ld + n, r);
#pragma unroll
      for (int e = 0; e < VE; ++e) v[e] += r[e];
    }
    Vec<T>::store(out + m * p.out_ld + n, v);
  }
}


// Few-row f32 GEMM: out[m, n] = act(scale[n] * sum_k x[m, k] w[n, k] + shift[n]) (+ res) for M <= 64 rows -- the squeeze-excite
// FCs of the training step on [B, C] vectors and their data gradients, where a 128x64 tile leaves one or two workgroups walking
// K alone (31 us per call).  WPC waves per output column split K in 16-byte pieces (the weight row is read once, the <= 16
// input rows come from L2; all 17 loads of a step are issued before the first FMA), partial sums meet in a wave reduction and,
// for WPC = 4 (long K, few columns), in LDS in wave order.  256 threads = 4 / WPC columns per workgroup.
template <int WPC>
__global__ __launch_bounds__(256) void rowgemm_f32_kernel(ConvP p) {
  __shared__ float red[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = WPC == 4 ? blockIdx.x : blockIdx.x * 4 + wave;
  const bool n_ok = n < p.Cout;
  const int nn = n_ok ? n : 0;
  const float* __restrict__ x = reinterpret_cast<const float*>(p.in);
  const float* __restrict__ w = reinterpret_cast<const float*>(p.w) + (long long)nn * p.K;
  const float* __restrict__ res = reinterpret_cast<const float*>(p.res);
  float* __restrict__ out = reinterpret_cast<float*>(p.out);
  const float sc = p.scale ? p.scale[nn] : 1.f, sh = p.shift ? p.shift[nn] : 0.f;
  const int kstart = (WPC == 4 ? threadIdx.x : lane) * 4, kstep = WPC == 4 ? 1024 : 256;
  for (int m0 = 0; m0 < p.M; m0 += 16) {
    const int mc = min(16, p.M - m0);
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k = kstart; k < p.K; k += kstep) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(w + k);
      f32x4 xv[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) xv[i] = *reinterpret_cast<const f32x4*>(x + (long long)(m0 + min(i, mc - 1)) * p.in_ld + k);
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = fmaf(xv[i][0], wv[0], fmaf(xv[i][1], wv[1], fmaf(xv[i][2], wv[2], fmaf(xv[i][3], wv[3], acc[i]))));
    }
    float mine = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float t = wave_sum(acc[i]);
      if (lane == i) mine = t;
    }
    if (WPC == 4) {
      if (m0 > 0) __syncthreads();
      if (lane < 16) red[wave][lane] = mine;
      __syncthreads();
      mine = lane < 16 ? ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane] : 0.f;
    }
    if (lane < mc && n_ok && (WPC == 1 || wave == 0)) {
      float v = 0.f;
      with_act(p.act, [&](auto A) { v = act_c<decltype(A)::value>(mine * sc + sh); });
      const long long m = m0 + lane;
      if (res) v += res[m * p.res_ld + n];
      out[m * p.out_ld + n] = v;
    }
  }
}

// The finishing sum of a split-K launch (gen-1, gen-2 and f16x3 GEMMs alike): slabs summed in split order + the epilogue.
template <typename T>
void splitk_reduce(const ConvP& p, const float* slabs, int splits, hipStream_t s) {
  long long total = (long long)p.M * (p.Cout / Vec<T>::N);
  int blocks = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
  hipLaunchKernelGGL(splitk_reduce_kernel<T>, dim3(blocks), dim3(256), 0, s, slabs, splits, p);
}

template <typename T, int BM, int BN, int WM, int WN>
void launch(const ConvP& p, float* slabs, int splits, hipStream_t s) {
  int tiles = cdiv(p.M, BM) * cdiv(p.Cout, BN);
  if (splits <= 1) {
    hipLaunchKernelGGL((conv_igemm_kernel<T, BM, BN, WM, WN>), dim3(tiles), dim3(256), 0, s, p);
  } else {
    hipLaunchKernelGGL((conv_igemm_splitk_kernel<T, BM, BN, WM, WN>), dim3(tiles * splits), dim3(256), 0, s, p, slabs, splits);
    splitk_reduce<T>(p, slabs, splits, s);
  }
}

template <typename T>
void dispatch(int variant, const ConvP& p, float* slabs, int splits, hipStream_t s) {
  switch (variant) {
    case 0: return launch<T, 256, 16, 4, 1>(p, slabs, splits, s);
    case 1: return launch<T, 256, 32, 4, 1>(p, slabs, splits, s);
    case 2: return launch<T, 128, 64, 2, 2>(p, slabs, splits, s);
    default: return launch<T, 128, 128, 2, 2>(p, slabs, splits, s);
  }
}

}  // namespace

void splitk_reduce_launch(int dtype, const ConvP& p, const float* slabs, int splits, hipStream_t s) {
  if (dtype == CFP_BF16) splitk_reduce<bf16_t>(p, slabs, splits, s); else if (dtype == CFP_F16) splitk_reduce<f16_t>(p, slabs, splits, s); else splitk_reduce<float>(p, slabs, splits, s);
}

void igemm1_launch(int variant, int dtype, const ConvP& p, float* slabs, int splits, hipStream_t s) {
  if (dtype == CFP_BF16) dispatch<bf16_t>(variant, p, slabs, splits, s); else if (dtype == CFP_F16) dispatch<f16_t>(variant, p, slabs, splits, s); else dispatch<float>(variant, p, slabs, splits, s);
}

void rowgemm_f32_launch(const ConvP& p, hipStream_t s) {
  if (p.K >= 512 && p.Cout <= 1024) hipLaunchKernelGGL(rowgemm_f32_kernel<4>, dim3(p.Cout), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(rowgemm_f32_kernel<1>, dim3(cdiv(p.Cout, 4)), dim3(256), 0, s, p);
}
