// What the fused LoFTR / LKPM tails share between their two storage widths: loftr_tail.hip (bf16 / f16 storage, one MFMA per product) and
// loftr_tail_x3.hip (float32 storage, f16x3 matrix math).  A wave owns 16 token rows from the first load to the final store, its tiles
// live in a private LDS region, and only the weights are shared: every GEMM of the chain streams them through a ring of LDS stages.
// The kernels differ in structure and stay in their files; the pieces that are the same design twice live here, once:
//   * tail_ring_begin/_step  the hand-over of the shared weight stages between consecutive GEMMs and the counted wait of the K loop
//   * tail_layernorm         LayerNorm over the accumulator registers
//   * tail_attn_apply        the linear-attention apply
//   * tail_tile_load/_store  the 16-row tile copies in 16-byte chunks (and their forms through a row map: hist2image in place)
//   * tail_row_layernorm     the LKPM input LayerNorm on the tile
//   * host side: the parameter blocks and their fill, the waves-per-workgroup rule, the D x heads x waves dispatch and the launch helper
// T is the storage type of the tensors and tiles (float, bf16_t, f16_t), W the element type of the weights (T, or f16_t for the packed
// operands of cfp_pack_w_x3).
#pragma once
#include <type_traits>

#include "lds_dma.h"

// ---- the ring of shared weight stages ---------------------------------------------------------------------------------------------
// One GEMM of the chain, `n` K-steps, is
//     tail_ring_begin<NST, NBW>(n, issue);
//     for (int i = 0; i < n; ++i) { const int st = tail_ring_step<NST, NBW>(i, n, issue);  ... compute step i from stage st ... }
// issue(i, st) starts this wave's NBW LDS-DMA loads of step i into stage st.  NST = 3 keeps two K-steps of DMA in flight, NST = 2 one.
// All waves of the workgroup must run it together.  The two functions own the whole synchronisation protocol; the loop and its body stay
// in the caller (passed in as a functor the body was compiled on its own first and came out scheduled differently: the 16-bit LoFTR tail
// at D = 64, 16 channels per head, was 4 % slower).
template <int NST, int NBW, typename ISSUE>
__device__ __forceinline__ void tail_ring_begin(int n, ISSUE issue) {
  static_assert(NST == 2 || NST == 3, "wait ladder in tail_ring_step");
  // Hand-over of the shared weight stages.  `s_barrier` has no memory semantics for the compiler and LDS reads are asynchronous: without the
  // wait + clobber IN FRONT of the barrier the previous GEMM's last fragment reads (one K-step GEMMs at D = 32 are straight-line code once
  // inlined) may be scheduled -- or still be in flight -- behind it, while a faster wave already streams the next weights into the stage they
  // read.  Found in the float32 kernels as a timing-dependent mismatch of a few 16-row tiles at D = 32 (tools/probes/x3_tail_stability.py:
  // 109 of 76 800 rows in one of 20 runs); D = 64 / 128 and the 16-bit kernels never showed it.
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();               // every wave is done with the previous GEMM's stages
  asm volatile("" ::: "memory");
  issue(0, 0);
  if (NST > 2 && n > 1) issue(1, 1);
}
// Start of step i: waits for its stage, hands the stage of step i - 1 to the DMA of step i + NST - 1, returns the stage to compute from.
template <int NST, int NBW, typename ISSUE>
__device__ __forceinline__ int tail_ring_step(int i, int n, ISSUE issue) {
  constexpr int AHEAD = NST - 1;              // K-steps of DMA in flight beside the one being computed
  // THREE weight stages, two K-steps of DMA in flight (round 4, late): a K-step here is a few MFMAs (~0.1-0.2 us) against a ~0.7-1 us round
  // trip of its weight tile from L2 -- with two stages every step of the chain (32 of them at D = 128) waited out that round trip
  // (batch-1 forward 3.50 -> 3.41 ms).  Counted wait: the loads of a stage are this wave's NBW youngest vector-memory operations when the
  // next stage has been issued behind it, and they complete in order; the last step waits for everything.  Issuing the first stages of the
  // NEXT GEMM of the chain right after a K loop (under the LayerNorm / attention / GELU work between the GEMMs) was built too and measured
  // no gain (3.42 ms; it costs a barrier per GEMM) -- not kept.
  if (AHEAD > 1 && i + 1 < n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NBW) : "memory");      // stage i landed, the loads of step i + 1 may still fly
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (i + AHEAD < n) issue(i + AHEAD, (i + AHEAD) % NST);      // the stage of step i - 1: everybody has read it (barrier above)
  return i % NST;
}

// ---- LayerNorm over the N = NT * 16 columns of each of this lane's 4 accumulator rows (row = fq * 4 + r, col = j * 16 + fr): two-pass
// statistics over the 16 lanes of a DPP row, as cfp_layernorm.  ROUND_T != float first rounds the values to that type (the unfused 16-bit
// path stores the GEMM output in the storage type before its LayerNorm).
template <int NT, typename ROUND_T>
__device__ __forceinline__ void tail_layernorm(f32x4 (&acc)[NT], const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int fr) {
  constexpr float inv_n = 1.f / (float)(NT * 16);
  float g[NT], bt[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) { g[j] = gamma[j * 16 + fr]; bt[j] = beta[j * 16 + fr]; }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      if constexpr (!std::is_same<ROUND_T, float>::value) acc[j][r] = to_f32<ROUND_T>(from_f32<ROUND_T>(acc[j][r]));
      s += acc[j][r];
    }
    s = row16_sum(s);
    const float mean = s * inv_n;
    float qq = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) { const float dlt = acc[j][r] - mean; qq = fmaf(dlt, dlt, qq); }
    qq = row16_sum(qq);
    const float rstd = rsqrtf(qq * inv_n + eps);
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j][r] = (acc[j][r] - mean) * rstd * g[j] + bt[j];
  }
}

// ---- 16-row tile copies in 16-byte chunks: global rows [row0, row0 + 16) x D <-> the wave's LDS tile (row pitch PA elements); rows past
// `rows` load as zeros and are not stored.
template <typename T, int D, int PA>
__device__ __forceinline__ void tail_tile_load(T* tile, const T* src, int ld, long long row0, int rows, int lane) {
  constexpr int E = 16 / sizeof(T), XCH = D / E;           // elements per chunk, chunks per row
  for (int i = lane; i < 16 * XCH; i += 64) {
    const int r = i / XCH, ch = i - r * XCH;
    const long long m = row0 + r;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (m < rows) v = *reinterpret_cast<const u32x4*>(src + m * ld + ch * E);
    *reinterpret_cast<u32x4*>(tile + r * PA + ch * E) = v;
  }
}
template <typename T, int D, int PA>
__device__ __forceinline__ void tail_tile_store(T* dst, int ld, const T* tile, long long row0, int rows, int lane) {
  constexpr int E = 16 / sizeof(T), XCH = D / E;
  for (int i = lane; i < 16 * XCH; i += 64) {
    const int r = i / XCH, ch = i - r * XCH;
    const long long m = row0 + r;
    if (m < rows) *reinterpret_cast<u32x4*>(dst + m * ld + ch * E) = *reinterpret_cast<const u32x4*>(tile + r * PA + ch * E);
  }
}

// ---- LayerNorm over the D channels of each row of the tile, in place: lane = (row fr, quarter fq of the channels) ---------------------
template <typename T, int D, int PA>
__device__ __forceinline__ void tail_row_layernorm(T* tile, const float* gamma, const float* beta, float eps, int fr, int fq) {
  constexpr int Q = D / 4, E = Vec<T>::N;                  // channels per lane, elements per 16-byte vector
  T* row = tile + fr * PA + fq * Q;
  float v[Q];
#pragma unroll
  for (int c = 0; c < Q; c += E) Vec<T>::load(row + c, v + c);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < Q; ++c) s += v[c];
  s += __shfl_xor(s, 16, 64); s += __shfl_xor(s, 32, 64);
  const float mean = s * (1.f / (float)D);
  float qq = 0.f;
#pragma unroll
  for (int c = 0; c < Q; ++c) { const float dl = v[c] - mean; qq = fmaf(dl, dl, qq); }
  qq += __shfl_xor(qq, 16, 64); qq += __shfl_xor(qq, 32, 64);
  const float rstd = rsqrtf(qq * (1.f / (float)D) + eps);
#pragma unroll
  for (int c = 0; c < Q; c += E) {
    float o[E];
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = (v[c + e] - mean) * rstd * gamma[fq * Q + c + e] + beta[fq * Q + c + e];
    Vec<T>::store(row + c, o);
  }
}

// ---- parameter blocks ---------------------------------------------------------------------------------------------------------------
// Optional row map of the LoFTR tail (hist2image at 1:1, cfp_loftr_tail_x2i): the Hq x Wq query grid of image b is the rectangle with origin
// (sy, sx) of an H x W token map, x and out are that map, and the final store is the paste of the zone grid -- see tail_tile_store_mapped.
struct TailMap {
  const uint8_t* zone_valid;     // [B][zn][zn] or null: the zone of grid position (gy, gx) is (gy / p1, gx / p2)
  int H, W, sy, sx, zn, p1, p2, accumulate;
};
template <typename T, typename W> struct TailP {
  const T* q; const float* kv; const float* ksum; const T* x; T* out;
  const W* wq;                   // optional: q_proj weights [D][D]; the kernel then computes q = x @ wq^T for its own rows and `q` is unused
  const W* wm; const W* w0; const W* w2;      // [D][D], [2D][2D], [D][2D]
  const float* g1; const float* b1; const float* g2; const float* b2;
  int q_ld, x_ld, out_ld;
  int rows, Hq, Wq, qth, qtw, ggy, ggx;
  FastDiv fwq, fhq, fqth, fqtw;  // rows < 2^31: the token -> (image, y, x) -> key-group split without 64-bit divisions (four of them per lane and
                                 // row tile were ~600 VALU instructions: about a third of the kernel at D = 32)
  float v_length, eps, ln_eps;
  TailMap map;                   // read by the mapped instantiations only (last: the plain kernels' argument offsets stay)
};
template <typename T, typename W> struct LkpmP {
  const T* t; const T* xin; T* out;
  const W* w1; const W* w2;      // [4D][D], [D][4D]
  const float* lg; const float* lb; const float* b1; const float* b2;
  int t_ld, x_ld, out_ld, rows;
  float ln_eps;
};

// N consecutive elements of T as float32, in 16-byte vectors where N allows.  LDS = true: `src` points into LDS and is read as such.  (Through
// a generic pointer the optimiser folds the tile read and the global read of the attention apply's two q sources into ONE flat load behind
// a pointer select: slower than a ds_read, and it counts on both wait counters.)
template <typename T, int N, bool LDS>
__device__ __forceinline__ void tail_load_f32(const T* src, float* v) {
  constexpr int E = Vec<T>::N;
  if constexpr (N >= E) {
#pragma unroll
    for (int c = 0; c < N; c += E) {
      if constexpr (LDS) {
        const u32x4 raw = *(const __attribute__((address_space(3))) u32x4*)(src + c);
        Vec<T>::load(reinterpret_cast<const T*>(&raw), v + c);
      } else {
        Vec<T>::load(src + c, v + c);
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = to_f32<T>(LDS ? *(const __attribute__((address_space(3))) T*)(src + c) : src[c]);
  }
}

// ---- linear-attention apply for the wave's 16 rows: lane = (row fr, head slot fq); msg = (elu1(q) KV[g]) / (elu1(q) . Ksum[g] + eps) * S
// into the msg tile (row pitch PA).  q comes from the wave's own tile `tq` (row pitch PQ) when the kernel projected it itself (p.wq given),
// else from p.q.
template <typename T, int D, int HEADS, int PA, int PQ, typename W>
__device__ __forceinline__ void tail_attn_apply(const TailP<T, W>& p, long long row0, const T* tq, T* tMsg, int fr, int fq) {
  constexpr int d = D / HEADS;
  const bool own_q = p.wq != nullptr;
  const int r = fr;
  const long long m = row0 + r;
  const bool ok = m < p.rows;
  const long long mm = ok ? m : 0;
  const unsigned t = fd_div((unsigned)mm, p.fwq), xq = (unsigned)mm - t * (unsigned)p.Wq;
  const unsigned b = fd_div(t, p.fhq), yq = t - b * (unsigned)p.Hq;
  const long long g = ((long long)b * p.ggy + fd_div(yq, p.fqth)) * p.ggx + fd_div(xq, p.fqtw);
#pragma unroll
  for (int hs = 0; hs < HEADS / 4; ++hs) {
    const int h = fq + 4 * hs;
    const float* __restrict__ kv = p.kv + (g * HEADS + h) * d * d;
    const float* __restrict__ ks = p.ksum + (g * HEADS + h) * d;
    float qv[d];
    if (own_q) tail_load_f32<T, d, true>(tq + r * PQ + h * d, qv);      // uniform
    else tail_load_f32<T, d, false>(p.q + mm * p.q_ld + h * d, qv);
    float o[d];
#pragma unroll
    for (int j = 0; j < d; ++j) o[j] = 0.f;
    float z = 0.f;
#pragma unroll
    for (int i = 0; i < d; ++i) {
      const float qe = elu1(qv[i]);
      z = fmaf(qe, ks[i], z);
#pragma unroll
      for (int j = 0; j < d; j += 4) {
        const f32x4 kk = *reinterpret_cast<const f32x4*>(kv + i * d + j);
        o[j] = fmaf(qe, kk[0], o[j]); o[j + 1] = fmaf(qe, kk[1], o[j + 1]);
        o[j + 2] = fmaf(qe, kk[2], o[j + 2]); o[j + 3] = fmaf(qe, kk[3], o[j + 3]);
      }
    }
    const float zi = 1.f / (z + p.eps);                    // (o * 1/(z+eps)) * S, as attention.py:48-49
#pragma unroll
    for (int j = 0; j < d; ++j) {
      // the value first, then a plain select on the row guard: written as `ok ? from_f32(..) : 0` the compiler sinks the whole FMA chain into
      // per-element `ok` branches, keeps every kv load of the head alive up to them and spills (2.4 KB of scratch per lane at d = 32)
      const T v = from_f32<T>(o[j] * zi * p.v_length);
      tMsg[r * PA + h * d + j] = ok ? v : T(0);
    }
  }
}

// ---- the same tile copies through the row map: tile row m = (b, gy, gx) of the grid <-> token row (b * H + sy + gy) * W + sx + gx ------------
// The token row of tile row m, or -1 when the grid position lies outside the image.
template <typename T, typename W>
__device__ __forceinline__ long long tail_map_row(const TailP<T, W>& p, long long m, int& b, int& gy, int& gx) {
  const unsigned t = fd_div((unsigned)m, p.fwq);
  gx = (int)((unsigned)m - t * (unsigned)p.Wq);
  const unsigned bu = fd_div(t, p.fhq);
  gy = (int)(t - bu * (unsigned)p.Hq);
  b = (int)bu;
  const int y = p.map.sy + gy, x = p.map.sx + gx;
  if (y < 0 || y >= p.map.H || x < 0 || x >= p.map.W) return -1;
  return ((long long)b * p.map.H + y) * p.map.W + x;
}
// What the 1:1 crop of the rectangle gives: the token row, zeros outside the image (the crop applies no zone mask).
template <typename T, int D, int PA, typename W>
__device__ __forceinline__ void tail_tile_load_mapped(T* tile, const TailP<T, W>& p, long long row0, int lane) {
  constexpr int E = 16 / sizeof(T), XCH = D / E;
  for (int i = lane; i < 16 * XCH; i += 64) {
    const int r = i / XCH, ch = i - r * XCH;
    const long long m = row0 + r;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (m < p.rows) {
      int b, gy, gx;
      const long long tr = tail_map_row(p, m, b, gy, gx);
      if (tr >= 0) v = *reinterpret_cast<const u32x4*>(p.x + tr * p.x_ld + ch * E);
    }
    *reinterpret_cast<u32x4*>(tile + r * PA + ch * E) = v;
  }
}
// What the 1:1 paste of the zone grid does with the tail's output (already rounded to the storage type in the tile, as the grid tensor
// was), line by line as cfp_resize_bilinear at scale 1: o = zone kept ? out : 0, o += token when accumulating, stored unconditionally and
// rounded once (a dropped zone stores token + 0); grid positions outside the image are skipped.  The token is read from the map, not from
// the x tile, and each token row is read and written by the one wave that owns it: in place is safe.
template <typename T, int D, int PA, typename W>
__device__ __forceinline__ void tail_tile_store_mapped(const TailP<T, W>& p, const T* tile, long long row0, int lane) {
  constexpr int E = Vec<T>::N, XCH = D / E;
  for (int i = lane; i < 16 * XCH; i += 64) {
    const int r = i / XCH, ch = i - r * XCH;
    const long long m = row0 + r;
    if (m >= p.rows) continue;
    int b, gy, gx;
    const long long tr = tail_map_row(p, m, b, gy, gx);
    if (tr < 0) continue;
    bool keep = true;
    if (p.map.zone_valid)
      keep = p.map.zone_valid[(long long)b * p.map.zn * p.map.zn + min(max(gy / p.map.p1, 0), p.map.zn - 1) * p.map.zn +
                              min(max(gx / p.map.p2, 0), p.map.zn - 1)] != 0;
    float o[E];
    Vec<T>::load(tile + r * PA + ch * E, o);
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = keep ? o[e] : 0.f;
    T* dp = p.out + tr * p.out_ld + ch * E;
    if (p.map.accumulate) {
      float d[E];
      Vec<T>::load(dp, d);
#pragma unroll
      for (int e = 0; e < E; ++e) o[e] += d[e];
    }
    Vec<T>::store(dp, o);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
template <typename T, typename W>
TailP<T, W> tail_params(const void* q, int q_ld, const float* kv, const float* ksum, const void* x, int x_ld, void* out, int out_ld, const void* w_q,
                        const void* w_merge, const void* w_mlp0, const void* w_mlp2, const float* ln1_g, const float* ln1_b, const float* ln2_g,
                        const float* ln2_b, float ln_eps, int NB, int Hq, int Wq, int qth, int qtw, float v_length, float eps) {
  TailP<T, W> p;
  p.q = (const T*)q; p.kv = kv; p.ksum = ksum; p.x = (const T*)x; p.out = (T*)out;
  p.wq = (const W*)w_q; p.wm = (const W*)w_merge; p.w0 = (const W*)w_mlp0; p.w2 = (const W*)w_mlp2;
  p.g1 = ln1_g; p.b1 = ln1_b; p.g2 = ln2_g; p.b2 = ln2_b;
  p.q_ld = q_ld; p.x_ld = x_ld; p.out_ld = out_ld;
  p.rows = NB * Hq * Wq; p.Hq = Hq; p.Wq = Wq; p.qth = qth; p.qtw = qtw; p.ggy = cdiv(Hq, qth); p.ggx = cdiv(Wq, qtw);
  p.fwq = make_fastdiv((unsigned)Wq); p.fhq = make_fastdiv((unsigned)Hq); p.fqth = make_fastdiv((unsigned)qth); p.fqtw = make_fastdiv((unsigned)qtw);
  p.v_length = v_length; p.eps = eps; p.ln_eps = ln_eps;
  p.map = TailMap{};
  return p;
}
template <typename T, typename W>
LkpmP<T, W> lkpm_params(const void* t, int t_ld, const void* xin, int x_ld, void* out, int out_ld, const void* w1, const float* b1, const void* w2,
                        const float* b2, const float* ln_g, const float* ln_b, float ln_eps, int rows) {
  LkpmP<T, W> p;
  p.t = (const T*)t; p.xin = (const T*)xin; p.out = (T*)out; p.w1 = (const W*)w1; p.w2 = (const W*)w2;
  p.lg = ln_g; p.lb = ln_b; p.b1 = b1; p.b2 = b2; p.t_ld = t_ld; p.x_ld = x_ld; p.out_ld = out_ld; p.rows = rows; p.ln_eps = ln_eps;
  return p;
}

// Waves of 16 token rows per workgroup: few rows (a single image) run as MORE, NARROWER workgroups -- they fill more of an otherwise idle
// chip and shorten each one's chain -- and many rows keep four waves, which share one weight stream.  Same arithmetic per row in every
// layout.  (A batch of 8 at D = 128, 9 600 rows, measured slower with two waves: 6.50 vs 6.32 ms per forward.)  `forced` = 1 / 2 / 4 is
// the A/B switch of cfp_debug_set (key 35: float32 kernels, key 39: 16-bit LoFTR tail), anything else = by the row count.
inline int tail_waves(long long rows, int forced) {
  if (forced == 1 || forced == 2 || forced == 4) return forced;
  return rows <= 4800 ? 1 : rows < 8192 ? 2 : 4;
}

// Run-time value -> template argument: f(std::integral_constant<int, V>{}) for the V equal to v, -2 if there is none.  The D x heads x waves
// dispatch of a kernel is a nest of these, one generic lambda per level.
template <int... V, typename F>
int tail_pick(int v, F f) {
  int rc = -2;
  ((v == V ? (void)(rc = f(std::integral_constant<int, V>{})) : (void)0), ...);
  return rc;
}

// Launch KERNEL with `waves` waves of 16 rows per workgroup and LDS bytes of dynamic LDS; the attribute that lifts the 64 KB limit is set
// once per instantiation.
template <auto KERNEL, size_t LDS, typename P>
int tail_launch(const P& p, int waves, hipStream_t s) {
  static_assert(LDS <= 160 * 1024, "LDS budget");
  static bool attr = false;
  if (!attr) { if (hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return -1; attr = true; }
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)cdiv(p.rows, 16 * waves)), dim3(64 * waves), LDS, s, p);
  return 0;
}

// the CFP_F32X3 side of cfp_loftr_tail / cfp_lkpm_tail (loftr_tail_x3.hip); 0, -1 = the attribute call failed, -2 = no such instantiation
int loftr_tail_x3_launch(const TailP<float, f16_t>& p, int heads, int D, hipStream_t s);
int lkpm_tail_x3_launch(const LkpmP<float, f16_t>& p, int D, hipStream_t s);
