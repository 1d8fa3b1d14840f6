// Linear attention (feature map elu(x)+1) -- there is no QK^T matrix and no softmax here:
//   reduce:  KV[g,h] = sum_s K'_s^T (V_s / S),  Ksum[g,h] = sum_s K'_s      (d x d and d per head)
//   apply :  out_q   = (Q'_q KV) / (Q'_q . Ksum + eps) * S
// d = D / heads is 4..32, so the d x d accumulator of one (group, head) lives in the registers of
// one wave: lane = (key lane, row chunk); the cross-lane sum over key lanes is a butterfly of
// wavefront shuffles.  Which keys form a group (a ToF zone's 16 samples, a ws x ws window with
// its zero padding, the sub-sampled global keys, the inside-zone rectangle) is pure addressing.
#include "kv_reduce_core.h"

namespace {

// One wave per (group, head, split): the keys' projected K / V rows come from global memory (kv_reduce_core.h has the arithmetic).
template <typename T, int D, bool DEV>
__global__ __launch_bounds__(64) void kv_reduce_kernel(KvP p) {
  const int g = blockIdx.x, h = blockIdx.y, sp = blockIdx.z;
  const int lane = threadIdx.x;
  const KvGeom q = kv_group_geom<DEV>(p, g, sp);
  constexpr int TPK = D / KvCfg<D>::IC;
  KvGlobalKeys<T> keys(p, q, lane / TPK, 64 / TPK);
  kv_reduce_body<T, D>(p, q, g, h, sp, lane, keys);
}

__global__ __launch_bounds__(256) void kv_finalize_kernel(const float* __restrict__ ws, float* __restrict__ kv,
                                                          float* __restrict__ ksum, int nsplit, int d, long long items) {
  // one thread per element of [group*head][d*d + d]; the split partials are summed in split order, eight
  // independent loads in flight at a time (the serial chain of up to 64 dependent loads was the whole kernel)
  const int per = d * d + d;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items * per; i += (long long)gridDim.x * 256) {
    const long long gh = (long long)((unsigned long long)i / (unsigned)per);      // one division; the remainder by multiply-subtract
    const int e = (int)(i - gh * per);
    const float* base = ws + gh * nsplit * per + e;
    float s = 0.f;
    int j = 0;
    for (; j + 7 < nsplit; j += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = base[(long long)(j + u) * per];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; j < nsplit; ++j) s += base[(long long)j * per];
    if (e < d * d) kv[gh * d * d + e] = s; else ksum[gh * d + (e - d * d)] = s;
  }
}

struct ApP {
  const void* q; const float* kv; const float* ksum; void* out;
  int q_ld, out_ld, NB, Hq, Wq, qth, qtw, ggy, ggx;
  int ey0, ey1, ex0, ex1, heads;
  float v_length, eps;
  FastDiv fheads, fwq, fhq, fqth, fqtw;      // (token, head) index arithmetic without 64-bit divisions (five per element in the first version)
  const int* rec;      // DEV only (last, as in KvP): the zone record, see cfp_attn_apply_dev
};

// JS lanes share one (token, head): lane js computes the D / JS outputs js * D / JS ... (and the normaliser, redundantly).  With one lane per
// (token, head) a d = 32 head is a chain of 1 024 dependent-latency FMAs fed by 256 sixteen-byte loads, and a single image has 4 800 such lanes --
// 19 workgroups, 24 us; eight lanes each shorten the chain eightfold and fill eight times the CUs.  Every output is the same sum in the same order.
// DEV: exclusion rectangle and v_length from the zone record, as in kv_reduce_kernel.
template <typename T, int D, int JS, bool DEV>
__global__ __launch_bounds__(256) void attn_apply_kernel(ApP p) {
  constexpr int DJ = D / JS;
  const T* __restrict__ Q = reinterpret_cast<const T*>(p.q);
  T* __restrict__ O = reinterpret_cast<T*>(p.out);
  int ey0 = p.ey0, ey1 = p.ey1, ex0 = p.ex0, ex1 = p.ex1;
  float v_length = p.v_length;
  if constexpr (DEV) {
    const int* __restrict__ rec = p.rec;
    ey0 = rec[4]; ey1 = rec[5]; ex0 = rec[6]; ex1 = rec[7];
    v_length = (float)max(rec[8], 1);
  }
  const unsigned total = (unsigned)p.NB * p.Hq * p.Wq * p.heads * JS;      // < 2^31: host check
  for (unsigned i0 = blockIdx.x * 256u + threadIdx.x; i0 < total; i0 += gridDim.x * 256u) {
    const unsigned i = i0 / JS;
    const int js = (int)(i0 - i * JS);
    unsigned toku, hu, tu, xu, bu, yu;
    fd_rowcol(i, p.fheads, toku, hu);
    fd_rowcol(toku, p.fwq, tu, xu);
    fd_rowcol(tu, p.fhq, bu, yu);
    const int h = (int)hu, x = (int)xu, y = (int)yu, b = (int)bu;
    const long long tok = toku;
    T* op = O + tok * p.out_ld + h * D + js * DJ;
    float o[DJ];
    if (y >= ey0 && y < ey1 && x >= ex0 && x < ex1) {
#pragma unroll
      for (int j = 0; j < DJ; ++j) o[j] = 0.f;
    } else {
      const long long g = ((long long)b * p.ggy + fd_div((unsigned)y, p.fqth)) * p.ggx + fd_div((unsigned)x, p.fqtw);
      const float* kv = p.kv + (g * p.heads + h) * D * D + js * DJ;
      const float* ks = p.ksum + (g * p.heads + h) * D;
      const T* qp = Q + tok * p.q_ld + h * D;
      float z = 0.f;
#pragma unroll
      for (int j = 0; j < DJ; ++j) o[j] = 0.f;
#pragma unroll
      for (int ii = 0; ii < D; ++ii) {
        const float qv = elu1(to_f32<T>(qp[ii]));
        z = fmaf(qv, ks[ii], z);
#pragma unroll
        for (int j = 0; j < DJ; ++j) o[j] = fmaf(qv, kv[ii * D + j], o[j]);
      }
      const float zi = 1.f / (z + p.eps);
#pragma unroll
      for (int j = 0; j < DJ; ++j) o[j] = o[j] * zi * v_length;
    }
#pragma unroll
    for (int j = 0; j < DJ; ++j) op[j] = from_f32<T>(o[j]);
  }
}

int g_ap_split_below = 65536;      // cfp_debug_set key 38: (token, head) pairs below which the outputs of a pair are split over several lanes
int g_kv_target_waves = 2048;      // cfp_debug_set key 19 (A/B)
int pick_nsplit(int S, long long groups_heads) {
  // enough waves to cover the chip, at least ~64 keys per wave
  long long want = (g_kv_target_waves + groups_heads - 1) / groups_heads;
  int by_keys = (S + 63) / 64;
  long long n = want < by_keys ? want : by_keys;
  if (n < 1) n = 1;
  if (n > 64) n = 64;
  return (int)n;
}

}  // namespace

void cfp_attn_debug_set(int value) { g_kv_target_waves = value; }
int kv_pick_nsplit(int S, long long groups_heads) { return pick_nsplit(S, groups_heads); }
void cfp_attn_apply_debug_set(int value) { g_ap_split_below = value; }

extern "C" size_t cfp_attn_kv_ws_floats(int NB, int Hk, int Wk, int th, int tw, int heads, int d) {
  if (NB <= 0 || Hk <= 0 || Wk <= 0 || th <= 0 || tw <= 0 || heads <= 0 || d <= 0) return 0;
  long long groups = (long long)NB * cdiv(Hk, th) * cdiv(Wk, tw);
  int S = (th < Hk ? th : Hk) * (tw < Wk ? tw : Wk);
  int ns = pick_nsplit(S, groups * heads);
  return (size_t)(groups * heads * ns * (d * d + d));
}

// What cfp_attn_kv_reduce[_dev] and cfp_attn_kv_project_reduce[_dev] share on the host: the checks of the geometry, the parameter block
// and the split count.  `k` / `v` and their pitches are the caller's.
int kv_fill_params(KvP& p, float* kv, float* ksum, float* ws, int NB, int Hk, int Wk, int th, int tw, int cy0, int cy1, int cx0, int cx1,
                   int count_pad, float v_length, const int* rec, int heads, int d, const char* who) {
  CFP_REQUIRE(kv && ksum, CFP_EINVAL, std::string(who) + ": null pointer");
  CFP_REQUIRE(NB > 0 && Hk > 0 && Wk > 0 && th > 0 && tw > 0 && heads > 0 && (d == 4 || d == 8 || d == 16 || d == 32) && v_length > 0.f,
              CFP_ESHAPE, std::string(who) + ": bad shape (head dim must be 4, 8, 16 or 32)");
  p.rec = rec;
  p.k = nullptr; p.v = nullptr; p.k_ld = 0; p.v_ld = 0;
  p.kv = kv; p.ksum = ksum; p.ws = ws;
  p.NB = NB; p.Hk = Hk; p.Wk = Wk; p.th = th; p.tw = tw; p.gy = cdiv(Hk, th); p.gx = cdiv(Wk, tw);
  p.cy0 = cy0; p.cy1 = cy1; p.cx0 = cx0; p.cx1 = cx1; p.count_pad = count_pad; p.heads = heads; p.d = d;
  p.inv_len = 1.0f / v_length;
  long long groups = (long long)NB * p.gy * p.gx;
  int S = (th < Hk ? th : Hk) * (tw < Wk ? tw : Wk);
  p.nsplit = pick_nsplit(S, groups * heads);
  CFP_REQUIRE(p.nsplit == 1 || ws, CFP_EINVAL, std::string(who) + ": workspace required");
  CFP_REQUIRE(groups < (1ll << 31) && heads <= 65535, CFP_ESHAPE, std::string(who) + ": grid too large");
  return CFP_OK;
}

// the split slabs of `ws` summed in split order into kv / ksum (p.nsplit > 1)
void kv_finalize_launch(const KvP& p, hipStream_t s) {
  long long items = (long long)p.NB * p.gy * p.gx * p.heads;
  long long total = items * (p.d * p.d + p.d);
  int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(kv_finalize_kernel, dim3(blocks), dim3(256), 0, s, p.ws, p.kv, p.ksum, p.nsplit, p.d, items);
}

// `rec` == nullptr: the scalar entry point (clip rectangle and v_length from the arguments); otherwise the record-reading one
static int kv_reduce_impl(const void* k, int k_ld, const void* v, int v_ld, float* kv, float* ksum, float* ws,
                          int NB, int Hk, int Wk, int th, int tw, int cy0, int cy1, int cx0, int cx1,
                          int count_pad, float v_length, const int* rec, int heads, int d, int dtype, cfp_stream_t stream, const char* who) {
  CFP_REQUIRE(dtype_ok(dtype), CFP_EINVAL, std::string(who) + ": bad dtype");
  CFP_REQUIRE(k && v && kv && ksum, CFP_EINVAL, std::string(who) + ": null pointer");
  CFP_REQUIRE(heads > 0 && d > 0 && k_ld >= heads * d && v_ld >= heads * d, CFP_ESHAPE, std::string(who) + ": bad shape (head dim must be 4, 8, 16 or 32)");
  KvP p;
  const int rc = kv_fill_params(p, kv, ksum, ws, NB, Hk, Wk, th, tw, cy0, cy1, cx0, cx1, count_pad, v_length, rec, heads, d, who);
  if (rc != CFP_OK) return rc;
  p.k = k; p.v = v; p.k_ld = k_ld; p.v_ld = v_ld;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)((long long)NB * p.gy * p.gx), heads, p.nsplit);
#define KV_LAUNCH(T, D) do { if (rec) hipLaunchKernelGGL((kv_reduce_kernel<T, D, true>), grid, dim3(64), 0, s, p); \
                             else hipLaunchKernelGGL((kv_reduce_kernel<T, D, false>), grid, dim3(64), 0, s, p); } while (0)
#define KV_SWITCH(T) switch (d) { case 4: KV_LAUNCH(T, 4); break; case 8: KV_LAUNCH(T, 8); break; \
                                  case 16: KV_LAUNCH(T, 16); break; default: KV_LAUNCH(T, 32); break; }
  if (dtype == CFP_BF16) { KV_SWITCH(bf16_t) } else if (dtype == CFP_F16) { KV_SWITCH(f16_t) } else { KV_SWITCH(float) }
#undef KV_SWITCH
#undef KV_LAUNCH
  if (p.nsplit > 1) kv_finalize_launch(p, s);
  return cfp_check_launch(who);
}

extern "C" int cfp_attn_kv_reduce(const void* k, int k_ld, const void* v, int v_ld, float* kv, float* ksum, float* ws,
                                  int NB, int Hk, int Wk, int th, int tw, int cy0, int cy1, int cx0, int cx1,
                                  int count_pad, float v_length, int heads, int d, int dtype, cfp_stream_t stream) {
  return kv_reduce_impl(k, k_ld, v, v_ld, kv, ksum, ws, NB, Hk, Wk, th, tw, cy0, cy1, cx0, cx1, count_pad, v_length, nullptr, heads, d, dtype,
                        stream, "cfp_attn_kv_reduce");
}

extern "C" int cfp_attn_kv_reduce_dev(const void* k, int k_ld, const void* v, int v_ld, float* kv, float* ksum, float* ws,
                                      int NB, int Hk, int Wk, int th, int tw, const int* rec, int count_pad, int heads, int d, int dtype,
                                      cfp_stream_t stream) {
  CFP_REQUIRE(rec && (reinterpret_cast<uintptr_t>(rec) & 3) == 0, CFP_EINVAL, "cfp_attn_kv_reduce_dev: bad record pointer");
  return kv_reduce_impl(k, k_ld, v, v_ld, kv, ksum, ws, NB, Hk, Wk, th, tw, 0, 0, 0, 0, count_pad, 1.f, rec, heads, d, dtype, stream,
                        "cfp_attn_kv_reduce_dev");
}

static int attn_apply_impl(const void* q, int q_ld, const float* kv, const float* ksum, void* out, int out_ld,
                           int NB, int Hq, int Wq, int qth, int qtw, int ey0, int ey1, int ex0, int ex1,
                           float v_length, const int* rec, float eps, int heads, int d, int dtype, cfp_stream_t stream, const char* who) {
  CFP_REQUIRE(dtype_ok(dtype), CFP_EINVAL, std::string(who) + ": bad dtype");
  CFP_REQUIRE(q && kv && ksum && out, CFP_EINVAL, std::string(who) + ": null pointer");
  CFP_REQUIRE(NB > 0 && Hq > 0 && Wq > 0 && qth > 0 && qtw > 0 && heads > 0 && (d == 4 || d == 8 || d == 16 || d == 32) &&
                  q_ld >= heads * d && out_ld >= heads * d, CFP_ESHAPE, std::string(who) + ": bad shape");
  ApP p;
  p.rec = rec;
  p.q = q; p.kv = kv; p.ksum = ksum; p.out = out; p.q_ld = q_ld; p.out_ld = out_ld;
  p.NB = NB; p.Hq = Hq; p.Wq = Wq; p.qth = qth; p.qtw = qtw; p.ggy = cdiv(Hq, qth); p.ggx = cdiv(Wq, qtw);
  p.ey0 = ey0; p.ey1 = ey1; p.ex0 = ex0; p.ex1 = ex1; p.heads = heads; p.v_length = v_length; p.eps = eps;
  long long total = (long long)NB * Hq * Wq * heads;
  CFP_REQUIRE(total < (1ll << 31), CFP_ESHAPE, std::string(who) + ": too many (token, head) pairs");
  p.fheads = make_fastdiv((unsigned)heads); p.fwq = make_fastdiv((unsigned)Wq); p.fhq = make_fastdiv((unsigned)Hq);
  p.fqth = make_fastdiv((unsigned)qth); p.fqtw = make_fastdiv((unsigned)qtw);
  const int js = total < g_ap_split_below ? (d >= 32 ? 8 : d >= 16 ? 4 : d >= 8 ? 2 : 1) : 1;
  CFP_REQUIRE(total * js < (1ll << 31), CFP_ESHAPE, std::string(who) + ": too many lanes");
  const long long lanes = total * js;
  int blocks = (int)((lanes + 255) / 256 > 8192 ? 8192 : (lanes + 255) / 256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define AP_LAUNCH(T, D, JS) do { if (rec) hipLaunchKernelGGL((attn_apply_kernel<T, D, JS, true>), dim3(blocks), dim3(256), 0, s, p); \
                                 else hipLaunchKernelGGL((attn_apply_kernel<T, D, JS, false>), dim3(blocks), dim3(256), 0, s, p); } while (0)
#define AP_SWITCH(T) switch (d) { case 4: AP_LAUNCH(T, 4, 1); break; \
                                  case 8: if (js > 1) AP_LAUNCH(T, 8, 2); else AP_LAUNCH(T, 8, 1); break; \
                                  case 16: if (js > 1) AP_LAUNCH(T, 16, 4); else AP_LAUNCH(T, 16, 1); break; \
                                  default: if (js > 1) AP_LAUNCH(T, 32, 8); else AP_LAUNCH(T, 32, 1); break; }
  if (dtype == CFP_BF16) { AP_SWITCH(bf16_t) } else if (dtype == CFP_F16) { AP_SWITCH(f16_t) } else { AP_SWITCH(float) }
#undef AP_SWITCH
#undef AP_LAUNCH
  return cfp_check_launch(who);
}

extern "C" int cfp_attn_apply(const void* q, int q_ld, const float* kv, const float* ksum, void* out, int out_ld,
                              int NB, int Hq, int Wq, int qth, int qtw, int ey0, int ey1, int ex0, int ex1,
                              float v_length, float eps, int heads, int d, int dtype, cfp_stream_t stream) {
  return attn_apply_impl(q, q_ld, kv, ksum, out, out_ld, NB, Hq, Wq, qth, qtw, ey0, ey1, ex0, ex1, v_length, nullptr, eps, heads, d, dtype,
                         stream, "cfp_attn_apply");
}

extern "C" int cfp_attn_apply_dev(const void* q, int q_ld, const float* kv, const float* ksum, void* out, int out_ld,
                                  int NB, int Hq, int Wq, int qth, int qtw, const int* rec, float eps, int heads, int d, int dtype,
                                  cfp_stream_t stream) {
  CFP_REQUIRE(rec && (reinterpret_cast<uintptr_t>(rec) & 3) == 0, CFP_EINVAL, "cfp_attn_apply_dev: bad record pointer");
  return attn_apply_impl(q, q_ld, kv, ksum, out, out_ld, NB, Hq, Wq, qth, qtw, 0, 0, 0, 0, 1.f, rec, eps, heads, d, dtype, stream,
                         "cfp_attn_apply_dev");
}
