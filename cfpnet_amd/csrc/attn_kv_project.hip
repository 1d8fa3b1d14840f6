// Key/value state of the linear attention straight from the key TOKENS: k|v projection + reduction in one kernel.
//
// Unfused, every LoFTR layer writes K|V = X Wkv^T ([keys][2 D], as large as the tokens times two) to HBM with a GEMM launch and
// cfp_attn_kv_reduce reads it straight back to reduce it to a few KB of state.  Here one workgroup owns a (group, split) of keys -- the
// same partition as cfp_attn_kv_reduce, same split count -- with one wave per head:
//   A  the split's key rows of X are gathered into LDS (row pitch + 16 bytes), K|V = X Wkv^T is computed on the matrix cores (16 x 16 x 32
//      MFMAs, one accumulator per output, K blocks of 32 channels in ascending order: the order of the GEMM kernels), rounded to the storage
//      type like the GEMM epilogue does (scale 1, shift 0, no activation) and left in LDS as a [keys][2 D] tile;
//   B  after one barrier wave h runs the reduction of head h (kv_reduce_core.h: the body cfp_attn_kv_reduce runs) on the LDS tile.
// The projected tensor never exists in memory; the sums are the unfused pair's bit for bit.  The weights ([2 D][D], at most 64 KB, L2
// resident) are fetched as MFMA fragments from global memory once per wave: a wave owns whole 16-column blocks of the output.
#include "kv_reduce_core.h"

namespace {

struct KvProjP {
  KvP r;               // the reduction's parameters; r.k / r.v are unused
  const void* x;       // key tokens [rows][D], pitch x_ld
  const void* w;       // [2 D][D]: rows 0 .. D-1 project K, D .. 2D-1 project V
  int x_ld;
  int rows16;          // 16-row tiles of LDS a workgroup holds: ceil(ceil(Smax / nsplit) / 16)
};

template <typename H, int DM, int HEADS, bool DEV>
__global__ __launch_bounds__(64 * HEADS) void kv_project_reduce_kernel(KvProjP pp) {
  constexpr int d = DM / HEADS;
  constexpr int PX = DM + 8, PKV = 2 * DM + 8;            // row pitches (elements): +16 bytes
  constexpr int XCH = DM / 8;                              // 16-byte chunks per token row
  constexpr int NT = 2 * DM / 16;                          // 16-column blocks of K|V
  constexpr int CW = NT < HEADS ? NT : HEADS;              // waves across the column blocks ...
  constexpr int RW = HEADS / CW;                           // ... and across the 16-row tiles
  constexpr int NJ = NT / CW;                              // column blocks per wave
  constexpr int NKB = DM / 32;                             // K blocks
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const KvP& p = pp.r;
  H* tX = reinterpret_cast<H*>(smem);
  H* tKV = tX + pp.rows16 * 16 * PX;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int g = blockIdx.x, sp = blockIdx.y;
  const KvGeom q = kv_group_geom<DEV>(p, g, sp);
  const int n = max(q.s_end - q.s_begin, 0);               // keys of this split (uniform)
  const int nt16 = (n + 15) >> 4;                          // <= pp.rows16: the host sizes the LDS by the unclipped group

  if (n > 0) {
    // ---- A: weight fragments of this wave's column blocks (B operand: output column fr of the block, channels kb * 32 + fq * 8 ...)
    const int cg = wave % CW, rg = wave / CW;
    const H* __restrict__ W = reinterpret_cast<const H*>(pp.w);
    s16x8 bw[NJ][NKB];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
        bw[j][kb] = *reinterpret_cast<const s16x8*>(W + (long long)((cg + j * CW) * 16 + fr) * DM + kb * 32 + fq * 8);
    // the split's key rows of X -> LDS; the rows that pad the last 16-row tile are zeros
    const H* __restrict__ X = reinterpret_cast<const H*>(pp.x);
    const int rwd = max(q.rw, 1);
    for (int i = tid; i < nt16 * 16 * XCH; i += 64 * HEADS) {
      const int r = i / XCH, ch = i - r * XCH;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (r < n) {
        const int s = q.s_begin + r;
        const int sy = s / rwd, sx = s - sy * rwd;
        const long long row = ((long long)q.b * p.Hk + q.y0 + sy) * p.Wk + q.x0 + sx;
        v = *reinterpret_cast<const u32x4*>(X + row * pp.x_ld + ch * 8);
      }
      *reinterpret_cast<u32x4*>(tX + r * PX + ch * 8) = v;
    }
    __syncthreads();
    for (int rt = rg; rt < nt16; rt += RW) {
      f32x4 acc[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const s16x8 a = *reinterpret_cast<const s16x8*>(tX + (rt * 16 + fr) * PX + kb * 32 + fq * 8);
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = mfma16<H>(a, bw[j][kb], acc[j]);
      }
      // the GEMM epilogue of a linear layer without scale, shift or activation: acc * 1 + 0, rounded to the storage type
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) tKV[(rt * 16 + fq * 4 + r) * PKV + (cg + j * CW) * 16 + fr] = from_f32<H>(acc[j][r] * 1.f + 0.f);
    }
  }
  __syncthreads();

  // ---- B: wave h reduces head h from the tile
  constexpr int TPK = d / KvCfg<d>::IC;
  KvTileKeys<H> keys(tKV, PKV, DM, q, lane / TPK, 64 / TPK);
  kv_reduce_body<H, d>(p, q, g, wave, sp, lane, keys);
}

// LDS of a workgroup: the X tile and the K|V tile of `rows16` 16-row tiles
size_t proj_lds_bytes(int rows16, int DM) { return (size_t)rows16 * 16 * ((DM + 8) + (2 * DM + 8)) * 2; }
// at least three workgroups per CU (160 KB of LDS)
constexpr size_t kProjLdsBudget = 52 * 1024;

int proj_rows16(int NB, int Hk, int Wk, int th, int tw, int heads) {
  const long long groups = (long long)NB * cdiv(Hk, th) * cdiv(Wk, tw);
  const int S = (th < Hk ? th : Hk) * (tw < Wk ? tw : Wk);
  const int ns = kv_pick_nsplit(S, groups * heads);
  return cdiv(cdiv(S, ns), 16);
}

bool proj_fits(int NB, int Hk, int Wk, int th, int tw, int heads, int d, int dtype) {
  if (!is16(dtype) || NB <= 0 || Hk <= 0 || Wk <= 0 || th <= 0 || tw <= 0 || (heads != 4 && heads != 8)) return false;
  const int DM = heads * d;
  if (DM != 32 && DM != 64 && DM != 128) return false;
  return proj_lds_bytes(proj_rows16(NB, Hk, Wk, th, tw, heads), DM) <= kProjLdsBudget;
}

int project_reduce_impl(const void* x, int x_ld, const void* w_kv, float* kv, float* ksum, float* ws, int NB, int Hk, int Wk, int th, int tw,
                        int cy0, int cy1, int cx0, int cx1, int count_pad, float v_length, const int* rec, int heads, int d, int dtype,
                        cfp_stream_t stream, const char* who) {
  CFP_REQUIRE(is16(dtype), CFP_EINVAL, std::string(who) + ": bf16 / f16 storage only");
  CFP_REQUIRE(x && w_kv && kv && ksum, CFP_EINVAL, std::string(who) + ": null pointer");
  CFP_REQUIRE(aligned16(x) && aligned16(w_kv), CFP_EINVAL, std::string(who) + ": x and the weights must be 16-byte aligned");
  CFP_REQUIRE(proj_fits(NB, Hk, Wk, th, tw, heads, d, dtype), CFP_ESHAPE,
              std::string(who) + ": the problem does not fit (cfp_attn_kv_project_fits): D = heads * d in 32 / 64 / 128, heads 4 / 8, a split's rows within the LDS budget");
  const int DM = heads * d;
  CFP_REQUIRE(x_ld >= DM && x_ld % 8 == 0, CFP_ESHAPE, std::string(who) + ": the token pitch must be >= D and a multiple of 8");
  KvProjP pp;
  const int rc = kv_fill_params(pp.r, kv, ksum, ws, NB, Hk, Wk, th, tw, cy0, cy1, cx0, cx1, count_pad, v_length, rec, heads, d, who);
  if (rc != CFP_OK) return rc;
  pp.x = x; pp.w = w_kv; pp.x_ld = x_ld;
  pp.rows16 = proj_rows16(NB, Hk, Wk, th, tw, heads);
  CFP_REQUIRE(pp.r.nsplit <= 65535, CFP_ESHAPE, std::string(who) + ": grid too large");
  const size_t lds = proj_lds_bytes(pp.rows16, DM);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((long long)NB * pp.r.gy * pp.r.gx), pp.r.nsplit);
#define KVP_LAUNCH(T, DM_, HD) do { if (rec) hipLaunchKernelGGL((kv_project_reduce_kernel<T, DM_, HD, true>), grid, dim3(64 * HD), lds, s, pp); \
                                    else hipLaunchKernelGGL((kv_project_reduce_kernel<T, DM_, HD, false>), grid, dim3(64 * HD), lds, s, pp); } while (0)
#define KVP_HEADS(T, DM_) do { if (heads == 4) KVP_LAUNCH(T, DM_, 4); else KVP_LAUNCH(T, DM_, 8); } while (0)
#define KVP_SWITCH(T) switch (DM) { case 32: KVP_HEADS(T, 32); break; case 64: KVP_HEADS(T, 64); break; default: KVP_HEADS(T, 128); break; }
  if (dtype == CFP_BF16) { KVP_SWITCH(bf16_t) } else { KVP_SWITCH(f16_t) }
#undef KVP_SWITCH
#undef KVP_HEADS
#undef KVP_LAUNCH
  if (pp.r.nsplit > 1) kv_finalize_launch(pp.r, s);
  return cfp_check_launch(who);
}

}  // namespace

extern "C" int cfp_attn_kv_project_fits(int NB, int Hk, int Wk, int th, int tw, int heads, int d, int dtype) {
  return proj_fits(NB, Hk, Wk, th, tw, heads, d, dtype) ? 1 : 0;
}

extern "C" int cfp_attn_kv_project_reduce(const void* x, int x_ld, const void* w_kv, float* kv, float* ksum, float* ws,
                                          int NB, int Hk, int Wk, int th, int tw, int cy0, int cy1, int cx0, int cx1,
                                          int count_pad, float v_length, int heads, int d, int dtype, cfp_stream_t stream) {
  return project_reduce_impl(x, x_ld, w_kv, kv, ksum, ws, NB, Hk, Wk, th, tw, cy0, cy1, cx0, cx1, count_pad, v_length, nullptr, heads, d, dtype,
                             stream, "cfp_attn_kv_project_reduce");
}

extern "C" int cfp_attn_kv_project_reduce_dev(const void* x, int x_ld, const void* w_kv, float* kv, float* ksum, float* ws,
                                              int NB, int Hk, int Wk, int th, int tw, const int* rec, int count_pad, int heads, int d, int dtype,
                                              cfp_stream_t stream) {
  CFP_REQUIRE(rec && (reinterpret_cast<uintptr_t>(rec) & 3) == 0, CFP_EINVAL, "cfp_attn_kv_project_reduce_dev: bad record pointer");
  return project_reduce_impl(x, x_ld, w_kv, kv, ksum, ws, NB, Hk, Wk, th, tw, 0, 0, 0, 0, count_pad, 1.f, rec, heads, d, dtype, stream,
                             "cfp_attn_kv_project_reduce_dev");
}
