// Short-K pointwise GEMM (bf16 / f16 storage): out[m, n] = act(scale[n] * sum_k in[m, k] * w[n, k] + shift[n]), K <= 256.
//
// The expand convolutions of the inverted-residual blocks (1x1, Cin -> 4 or 6 Cin, BatchNorm, SiLU) are 1 to 4 K-steps of the general
// implicit GEMM (conv_igemm2.hip): every one of its 450 ... 1950 tiles pays a cold first stage and an epilogue around those few steps, and
// the same input rows are fetched again by every column tile.  Here K is short enough for a wave's 16 input rows to live in registers
// as whole MFMA fragments (at K = 256: eight 16x16x32 fragments, 32 VGPRs), so a workgroup of four waves
//   * loads its 64 rows ONCE, global -> registers (rows past M and chunks past K are zeros),
//   * and streams only weights: its group of output columns in chunks of 32 weight rows through a ring of three LDS stages
//     (tail_ring_begin / tail_ring_step of tail_core.h own the hand-over; LDS-DMA loads as conv_igemm2.hip, 128-byte rows with the 16-byte
//     chunk XOR-swizzled on the source side), one continuous pipeline from the first chunk to the last.
// From 8 192 rows up a wave owns 32 rows (TM = 2, 128-row workgroups): every weight fragment read from LDS then feeds two MFMAs and a
// workgroup walks half the steps.  With four copies side by side that is the faster form (9600 x 136 x 816: 6.2 against 7.0 us per
// launch, and 9.0 for the implicit GEMM); alone it is 5 % behind TM = 1 (12.6 against 12.0, implicit GEMM 13.4 -- profiles/pw_rows_ab.txt).
// Results leave from registers as 16-byte vectors along the channel axis: LDS row r of a chunk holds weight row
// 8 (r % 16 / 4) + 4 (r / 16) + r % 4, so the two accumulator fragments of a lane are eight CONSECUTIVE output channels of one pixel.
// The stores of chunk i are issued at the start of step i + 1, IN FRONT of the LDS-DMA of chunk i + 3 (inside the ring's issue functor):
// the counted wait of tail_ring_step leaves a wave's NBW youngest vector-memory operations in flight, and those are then the weight loads
// of the newest stage alone, as the ring's protocol assumes.  (Stored right behind the MFMAs, a chunk's stores are the youngest operations
// at the next wait, which then also waits for the first loads of the newest stage: still correct, and measured the same -- 11.8 against
// 11.9 us at 9600 x 136 x 816; what bounds a launch is the life of a workgroup and how many fit a CU, not the depth of the ring.)
//
// Bit for bit the launch it replaces: the same matrix instruction with the weights as its row operand, one accumulator per output that
// takes the 32-wide K blocks in ascending order -- as many of them as igemm2_kernel walks, 2 ceil(K / 64), the last ones zeros -- with
// k = 32 b + 8 q + e at element e of lane group q, and conv_igemm2.hip's epilogue expressions (which row of the instruction an output
// channel sits in does not enter its sum).
#include "tail_core.h"

namespace {

constexpr int PW_NB = 32;                   // weight rows per LDS stage
constexpr int PW_NST = 3;                   // stages of the ring
constexpr int PW_MAX_CPG = 64;              // chunks per workgroup: the scale / shift of its columns (16 KB) sit in LDS behind the stages
constexpr int PW_TARGET_WGS = 512;          // two workgroups per CU
int g_pw_tm = 0;                            // cfp_debug_set key 41: 1 / 2 forces the 16-row fragments per wave, 0 = by the shape

struct PwRowsP {
  const void* in; const void* w; void* out;
  const float* scale; const float* shift;
  int in_ld, out_ld, M, K, N;
  int groups, cpg;                          // column groups, chunks of PW_NB columns per group
};

// TM: 16-row fragments per wave (a workgroup owns 64 TM rows).  TM = 2 reads every weight fragment once for two MFMAs: half the LDS
// reads and half the steps for the same output, at twice the A registers.
template <typename H, int NKS, int TM, int ACT>
__global__ __launch_bounds__(256) void pw_rows_kernel(PwRowsP p) {
  constexpr int NB = PW_NB, NST = PW_NST;
  constexpr int NKB = 2 * NKS;                      // 32-wide K blocks
  constexpr int TN = NB / 16;                       // accumulator fragments per chunk and row fragment
  constexpr int SUB_BYTES = NB * 128;               // one K-step of a chunk: NB rows of 64 elements
  constexpr int STAGE_BYTES = NKS * SUB_BYTES;
  constexpr int NBW = NKS * NB / 32;                // LDS-DMA instructions per wave and stage
  static_assert(TN == 2, "a lane's two fragments are one 16-byte vector");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sSc = reinterpret_cast<float*>(smem + NST * STAGE_BYTES);      // [cpg * NB] scale, then [cpg * NB] shift
  float* sSh = sSc + p.cpg * NB;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int rsub = lane >> 3;
  const int lc = (lane & 7) ^ rsub;                 // logical K chunk this lane fetches (the swizzle, applied to the source)

  const int bid = xcd_remap(blockIdx.x, gridDim.x);  // the groups of a row tile share its rows: neighbours in one L2
  const int g = bid % p.groups;
  const int tile_m = bid / p.groups;
  const int chunks = (p.N + NB - 1) / NB;
  const int c0 = g * p.cpg;
  const int nch = min(p.cpg, chunks - c0);          // this group's chunks (uniform)
  const int n_first = c0 * NB;

  const H* __restrict__ in = reinterpret_cast<const H*>(p.in);
  const H* __restrict__ wt = reinterpret_cast<const H*>(p.w);
  H* __restrict__ out = reinterpret_cast<H*>(p.out);
  const H* zsrc = reinterpret_cast<const H*>(g_zero16);

  // ---- this wave's 16 TM rows as A fragments: lane (fr, fq) holds row 16 t + fr, k = 32 b + 8 fq .. + 7 of block b
  bool m_ok[TM];
  H* dst[TM];
  s16x8 a[TM][NKB];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const long long m = (long long)tile_m * (64 * TM) + (wave * TM + t) * 16 + fr;
    m_ok[t] = m < p.M;
    dst[t] = out + (m_ok[t] ? m : 0) * p.out_ld;
#pragma unroll
    for (int b = 0; b < NKB; ++b) {
      const int k = 32 * b + 8 * fq;
      const H* src = (m_ok[t] && k < p.K) ? in + m * p.in_ld + k : zsrc;
      a[t][b] = *reinterpret_cast<const s16x8*>(src);
    }
  }

  // the finished chunk waits here for the start of the next step
  u32x4 pend[TM] = {};
  int pend_n = p.N;                                 // first channel of pend; p.N = nothing pending
  auto flush = [&]() {
#pragma unroll
    for (int t = 0; t < TM; ++t)
      if (m_ok[t] && pend_n < p.N) *reinterpret_cast<u32x4*>(dst[t] + pend_n) = pend[t];
    pend_n = p.N;
  };
  // chunk i of the group into stage st: 1 KB units (8 rows x 8 chunks of one K-step), unit u = t * 4 + wave
  auto issue = [&](int i, int st) {
    flush();
    const int nc = n_first + i * NB;
    unsigned char* sW = smem + st * STAGE_BYTES;
#pragma unroll
    for (int t = 0; t < NBW; ++t) {
      const int u = t * 4 + wave;
      const int ks = u / (NB / 8), rg = u % (NB / 8);
      const int r = rg * 8 + rsub;                  // LDS row of the chunk
      const int j = r >> 4, ii = r & 15;            // MFMA fragment and row
      const int n = nc + (ii >> 2) * 8 + j * 4 + (ii & 3);
      const int k = ks * 64 + lc * 8;
      const bool ok = n < p.N && k < p.K;
      glds16(ok ? wt + (long long)n * p.K + k : zsrc, sW + u * 1024);
    }
  };

  tail_ring_begin<NST, NBW>(nch, issue);
  // ---- scale / shift of the group's columns (1 / 0 where there is none), BEHIND the first weight loads: one memory round trip for the
  // rows, the first two stages and these (the barrier of the first step publishes them)
  for (int c = tid; c < nch * NB; c += 256) {
    const int n = n_first + c;
    sSc[c] = (p.scale && n < p.N) ? p.scale[n] : 1.f;
    sSh[c] = (p.shift && n < p.N) ? p.shift[n] : 0.f;
  }
  // The wait for the A rows belongs HERE, once, beside the first two stages' DMA: left to the compiler it lands in front of the first MFMA
  // inside the loop as `s_waitcnt vmcnt(0)` (the loads are still pending on the loop's entry edge), which drains the ring in every step.
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int b = 0; b < NKB; ++b) asm volatile("" : "+v"(a[t][b]));
  for (int i = 0; i < nch; ++i) {
    const int st = tail_ring_step<NST, NBW>(i, nch, issue);
    if (i + NST - 1 >= nch) flush();                // the last steps issue nothing
    const unsigned char* cW = smem + st * STAGE_BYTES;
    f32x4 acc[TM][TN];
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < NKB; ++b) {
      const int pc = (((b & 1) * 4 + fq) ^ (fr & 7)) * 16;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const s16x8 bfr = *reinterpret_cast<const s16x8*>(cW + (b >> 1) * SUB_BYTES + (j * 16 + fr) * 128 + pc);
#pragma unroll
        for (int t = 0; t < TM; ++t)      // transposed, as igemm2_kernel: acc[t][j][r] = weight row 4 fq + r of fragment j, pixel row 16 t + fr
          acc[t][j] = mfma16<H>(bfr, a[t][b], acc[t][j]);
      }
    }
    // ---- epilogue: the two fragments of a lane are the channels nc + 8 fq .. + 7 of its pixel
    const int c = i * NB + fq * 8;
    const f32x4 sc0 = *reinterpret_cast<const f32x4*>(sSc + c), sc1 = *reinterpret_cast<const f32x4*>(sSc + c + 4);
    const f32x4 sh0 = *reinterpret_cast<const f32x4*>(sSh + c), sh1 = *reinterpret_cast<const f32x4*>(sSh + c + 4);
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      float y[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        y[r] = act_c16<ACT>(acc[t][0][r] * sc0[r] + sh0[r]);
        y[4 + r] = act_c16<ACT>(acc[t][1][r] * sc1[r] + sh1[r]);
      }
      pend[t][0] = pack2<H>(y[0], y[1]); pend[t][1] = pack2<H>(y[2], y[3]);
      pend[t][2] = pack2<H>(y[4], y[5]); pend[t][3] = pack2<H>(y[6], y[7]);
    }
    pend_n = n_first + c;
  }
  flush();
}

constexpr size_t pw_rows_lds(int nks, int cpg) { return (size_t)PW_NST * nks * PW_NB * 128 + (size_t)cpg * PW_NB * 8; }
static_assert(pw_rows_lds(4, PW_MAX_CPG) <= 64 * 1024, "LDS of the widest launch");

bool pw_rows_fits(long long M, int K, int N, int in_ld, int out_ld, int dtype) {
  return is16(dtype) && M > 0 && M < (1ll << 31) && K > 0 && K <= 256 && K % 8 == 0 && N > 0 && N % 8 == 0 && in_ld >= K && in_ld % 8 == 0 &&
         out_ld >= N && out_ld % 8 == 0;
}

// 16-row fragments per wave.
int pw_rows_tm(long long M) {
  if (g_pw_tm == 1 || g_pw_tm == 2) return g_pw_tm;
  return M >= 8192 ? 2 : 1;      // 2400 rows are 19 tiles of 128: 4.5 against 4.3 us in flight, 8.1 against 7.7 alone
}

// Column groups of a launch: enough for about two workgroups per CU (at batch 8 the 1/32 scale has 38 row tiles), never more than there
// are chunks, never so few that a group's scale / shift would not fit behind the stages.  *max_groups = the chunk count.
int pw_rows_groups(long long M, int N, int tm, int forced, int* max_groups, int* cpg_out) {
  const int chunks = cdiv(N, PW_NB);
  const int tiles_m = cdiv(M, 64 * tm);
  const int lo = cdiv(chunks, PW_MAX_CPG);
  int g = forced > 0 ? forced : cdiv(PW_TARGET_WGS, tiles_m);
  g = g < lo ? lo : g > chunks ? chunks : g;
  const int cpg = cdiv(chunks, g);
  if (max_groups) *max_groups = chunks;
  if (cpg_out) *cpg_out = cpg;
  return cdiv(chunks, cpg);                         // no empty group
}

template <typename H, int NKS>
void pw_rows_launch(const PwRowsP& p, int tm, int act, long long wgs, hipStream_t s) {
  const size_t lds = pw_rows_lds(NKS, p.cpg);
  const dim3 grid((unsigned)wgs), block(256);
  if (tm == 2) {
    if (act == CFP_ACT_SILU) hipLaunchKernelGGL((pw_rows_kernel<H, NKS, 2, CFP_ACT_SILU>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((pw_rows_kernel<H, NKS, 2, CFP_ACT_NONE>), grid, block, lds, s, p);
  } else {
    if (act == CFP_ACT_SILU) hipLaunchKernelGGL((pw_rows_kernel<H, NKS, 1, CFP_ACT_SILU>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((pw_rows_kernel<H, NKS, 1, CFP_ACT_NONE>), grid, block, lds, s, p);
  }
}

}  // namespace

void cfp_pw_rows_debug_set(int value) { g_pw_tm = value; }

extern "C" int cfp_pw_rows_fits(long long M, int K, int N, int in_ld, int out_ld, int dtype) { return pw_rows_fits(M, K, N, in_ld, out_ld, dtype) ? 1 : 0; }

extern "C" int cfp_pw_rows_groups(long long M, int K, int N, int* max_groups) {
  if (M <= 0 || K <= 0 || N <= 0) { if (max_groups) *max_groups = 0; return 0; }
  return pw_rows_groups(M, N, pw_rows_tm(M), 0, max_groups, nullptr);
}

extern "C" int cfp_pw_rows(const void* in, int in_ld, const void* w, const float* scale, const float* shift, int act, void* out, int out_ld,
                           long long M, int K, int N, int groups, int dtype, cfp_stream_t stream) {
  CFP_REQUIRE(in && w && out, CFP_EINVAL, "cfp_pw_rows: null pointer");
  CFP_REQUIRE(is16(dtype), CFP_EINVAL, "cfp_pw_rows: bf16 / f16 storage only");
  CFP_REQUIRE(act == CFP_ACT_NONE || act == CFP_ACT_SILU, CFP_EINVAL, "cfp_pw_rows: bad activation (CFP_ACT_NONE or CFP_ACT_SILU)");
  CFP_REQUIRE(groups >= 0, CFP_EINVAL, "cfp_pw_rows: negative column-group count");
  CFP_REQUIRE(pw_rows_fits(M, K, N, in_ld, out_ld, dtype), CFP_ESHAPE,
              "cfp_pw_rows: shape not taken (cfp_pw_rows_fits: K % 8 == 0 and <= 256, N % 8 == 0, row pitches multiples of 8 that cover the channels, M < 2^31)");
  CFP_REQUIRE(aligned16(in) && aligned16(w) && aligned16(out) && aligned16(scale) && aligned16(shift), CFP_EINVAL,
              "cfp_pw_rows: pointers must be 16-byte aligned");
  PwRowsP p{};
  p.in = in; p.w = w; p.out = out; p.scale = scale; p.shift = shift;
  p.in_ld = in_ld; p.out_ld = out_ld; p.M = (int)M; p.K = K; p.N = N;
  const int tm = pw_rows_tm(M);
  p.groups = pw_rows_groups(M, N, tm, groups, nullptr, &p.cpg);
  const long long wgs = (long long)cdiv(M, 64 * tm) * p.groups;
  CFP_REQUIRE(wgs < (1ll << 31), CFP_ESHAPE, "cfp_pw_rows: problem too large");
  hipStream_t s = (hipStream_t)stream;
  const bool f16 = dtype == CFP_F16;
  switch (cdiv(K, 64)) {
    case 1: f16 ? pw_rows_launch<f16_t, 1>(p, tm, act, wgs, s) : pw_rows_launch<bf16_t, 1>(p, tm, act, wgs, s); break;
    case 2: f16 ? pw_rows_launch<f16_t, 2>(p, tm, act, wgs, s) : pw_rows_launch<bf16_t, 2>(p, tm, act, wgs, s); break;
    case 3: f16 ? pw_rows_launch<f16_t, 3>(p, tm, act, wgs, s) : pw_rows_launch<bf16_t, 3>(p, tm, act, wgs, s); break;
    default: f16 ? pw_rows_launch<f16_t, 4>(p, tm, act, wgs, s) : pw_rows_launch<bf16_t, 4>(p, tm, act, wgs, s); break;
  }
  return cfp_check_launch("cfp_pw_rows");
}
