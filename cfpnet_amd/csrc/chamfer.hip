// Bin-centre chamfer loss of the training step (`--w_chamfer`), value and gradient in one pass over the pixels, f32 in / f64 inside.
//
//   c_p = 0.5 (e_p + e_{p+1})                      centres of image b, strictly increasing
//   T_b = { target[b,y,x] : mask != 0 }            (mask NULL: target >= 1e-3),  N_b = |T_b|
//   L_b = (1/P) sum_p min_t (c_p - t)^2 + (1/N_b) sum_t min_p (c_p - t)^2,       L = (1/B) sum_b L_b        (N_b = 0: L_b = 0)
//
// The centres are sorted, so nothing is compared all-to-all.  A pixel finds its interval k (c_{k-1} <= t < c_k, k = 0..P) by a binary
// search over the centres in LDS; its nearest centre nn is one of the interval's two ends (tie: the lower index).  The pixel pass keeps
//   per centre    sum of d = t - c_nn           LDS int64 atomics in fixed point, quantum 2^-40 (see kQuantBits)
//   per interval  min and max target            LDS uint atomics on an order-preserving key of the float
//   per thread    sum of d^2 and the count      f64 registers, a fixed-order tree at the end
// (the per-centre count and sum of d^2 of a textbook statement are only ever used summed over the centres, so they are kept as that
// sum, in f64, and lose nothing to a quantum).  Integer atomics commute: the LDS contents do not depend on the order of arrival.
// Every kSub pixels each thread moves "its" centres' fixed-point sums into f64 registers and clears them, so no image size can
// overflow them.  One workgroup writes one slab of partials; the finaliser (one workgroup per image) combines the slabs in index
// order, turns the interval extrema into "nearest target below / above each centre" by a prefix-max and a suffix-min scan (an empty
// interval holds the scans' identities, so runs of empty intervals are stepped over by construction), and forms L_b and
//   dL_b / dc_p = 2 (c_p - near_p) / P - 2 (sum d)_p / N_b                       (tie: the lower target)
// A third one-wave launch averages L_b over B.  No float atomics, no host sync, no allocation: bit-identical from run to run.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxP = 1024;             // centres per image: 4 per thread, 20.5 KB of LDS
constexpr int kSub = 4096;              // pixels of a workgroup between two flushes of the fixed-point sums
constexpr int kMaxGroups = 64;          // workgroups (slabs of partials) per image
// fixed point of sum d: |d| is clamped to kDClamp = 2^11 - 1 and a flush comes after at most 2^12 pixels, so |sum| < 2^23 * 2^40 = 2^63.
// d = t - c is exact in f64 and has 24 significant bits, so the quantum 2^-40 rounds it only where |d| < 2^-16 (by <= 2^-41).
constexpr int kQuantBits = 40;
constexpr double kDClamp = 2047.0;
constexpr unsigned kNoMin = 0xffffffffu, kNoMax = 0u;      // keys no float but a NaN has: "no target in this interval"

// order-preserving key of a float (unsigned compare == float compare) and back
__device__ __forceinline__ unsigned fkey(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fval(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

struct ChamferP {
  const float* edges; const float* target; const unsigned char* mask;
  double* dsum;          // [B][G][P]   sum d per centre, in quanta
  double* d2n;           // [B][G][2]   sum d^2, count
  double* lb;            // [B]         L_b
  unsigned* kmin;        // [B][G][P+1] key of the smallest target per interval
  unsigned* kmax;        // [B][G][P+1] key of the largest
  long long HW, chunk;
  int B, P, G;
};

__global__ __launch_bounds__(kThreads) void chamfer_pixels_kernel(ChamferP p) {
  __shared__ float c[kMaxP];
  __shared__ unsigned long long sd[kMaxP];
  __shared__ unsigned smin[kMaxP + 1], smax[kMaxP + 1];
  __shared__ double red[2][kThreads];
  const int tid = threadIdx.x, P = p.P;
  const int b = blockIdx.x / p.G, g = blockIdx.x - b * p.G;
  const float* __restrict__ e = p.edges + (long long)b * (P + 1);
  for (int i = tid; i < P; i += kThreads) { c[i] = 0.5f * (e[i] + e[i + 1]); sd[i] = 0ull; }
  for (int i = tid; i <= P; i += kThreads) { smin[i] = kNoMin; smax[i] = kNoMax; }
  __syncthreads();
  double acc[kMaxP / kThreads] = {0.0, 0.0, 0.0, 0.0};
  double s2 = 0.0, n = 0.0;
  const long long base = (long long)b * p.HW;
  const long long lo = (long long)g * p.chunk, hi = min(p.HW, lo + p.chunk);
  const float* __restrict__ tg = p.target + base;
  const unsigned char* __restrict__ mk = p.mask ? p.mask + base : nullptr;
  for (long long s = lo; s < hi; s += kSub) {              // uniform over the workgroup
    const long long se = min(hi, s + (long long)kSub);
    for (long long i = s + tid; i < se; i += kThreads) {
      const float t = tg[i];
      if (mk ? mk[i] != 0 : t >= 1e-3f) {
        int k = 0, len = P;                                // k = number of centres <= t
        while (len > 0) {
          const int half = len >> 1;
          if (c[k + half] <= t) { k += half + 1; len -= half + 1; } else len = half;
        }
        int nn = k == 0 ? 0 : k - 1;
        if (k > 0 && k < P && (double)t - (double)c[k - 1] > (double)c[k] - (double)t) nn = k;
        const double d = (double)t - (double)c[nn];
        s2 += d * d; n += 1.0;
        const long long q = __double2ll_rn(fmin(fmax(d, -kDClamp), kDClamp) * (double)(1ll << kQuantBits));
        atomicAdd(&sd[nn], (unsigned long long)q);
        const unsigned key = fkey(t);
        atomicMin(&smin[k], key);
        atomicMax(&smax[k], key);
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kMaxP / kThreads; ++j) {
      const int idx = tid + j * kThreads;
      if (idx < P) { acc[j] += (double)(long long)sd[idx]; sd[idx] = 0ull; }
    }
    __syncthreads();
  }
  const long long slab = (long long)b * p.G + g;
#pragma unroll
  for (int j = 0; j < kMaxP / kThreads; ++j) {
    const int idx = tid + j * kThreads;
    if (idx < P) p.dsum[slab * P + idx] = acc[j];
  }
  for (int i = tid; i <= P; i += kThreads) { p.kmin[slab * (P + 1) + i] = smin[i]; p.kmax[slab * (P + 1) + i] = smax[i]; }
  red[0][tid] = s2; red[1][tid] = n;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { p.d2n[slab * 2] = red[0][0]; p.d2n[slab * 2 + 1] = red[1][0]; }
}

__global__ __launch_bounds__(kThreads) void chamfer_final_kernel(ChamferP p, float grad_scale, float* __restrict__ loss, float* __restrict__ grad) {
  __shared__ unsigned below[kMaxP + 1], above[kMaxP + 1];      // interval maxima -> prefix max; interval minima -> suffix min
  __shared__ unsigned tot[2][kThreads];
  __shared__ double red[kThreads];
  __shared__ double sn[2];
  const int tid = threadIdx.x, P = p.P, G = p.G, b = blockIdx.x;
  const long long slab0 = (long long)b * G;
  for (int i = tid; i <= P; i += kThreads) {
    unsigned mn = kNoMin, mx = kNoMax;
    for (int g = 0; g < G; ++g) {
      mn = min(mn, p.kmin[(slab0 + g) * (P + 1) + i]);
      mx = max(mx, p.kmax[(slab0 + g) * (P + 1) + i]);
    }
    below[i] = mx; above[i] = mn;
  }
  if (tid == 0) {
    double s2 = 0.0, n = 0.0;
    for (int g = 0; g < G; ++g) { s2 += p.d2n[(slab0 + g) * 2]; n += p.d2n[(slab0 + g) * 2 + 1]; }
    sn[0] = s2; sn[1] = n;
  }
  __syncthreads();
  const double N = sn[1];
  if (N == 0.0) {                                              // uniform: no valid pixel, the image contributes nothing
    if (grad) for (int i = tid; i < P; i += kThreads) grad[(long long)b * P + i] = 0.f;
    if (tid == 0) { p.lb[b] = 0.0; loss[1 + b] = 0.f; }
    return;
  }
  // the two scans over the P + 1 intervals: each thread owns E consecutive entries, the thread totals are scanned through LDS
  const int E = (P + kThreads) / kThreads;                     // ceil((P + 1) / kThreads)
  const int i0 = min(tid * E, P + 1), i1 = min(i0 + E, P + 1);
  unsigned mx = kNoMax, mn = kNoMin;
  for (int i = i0; i < i1; ++i) { mx = max(mx, below[i]); mn = min(mn, above[i]); }
  tot[0][tid] = mx; tot[1][tid] = mn;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {
    const unsigned a = tid >= o ? tot[0][tid - o] : kNoMax;
    const unsigned m = tid + o < kThreads ? tot[1][tid + o] : kNoMin;
    __syncthreads();
    tot[0][tid] = max(tot[0][tid], a); tot[1][tid] = min(tot[1][tid], m);
    __syncthreads();
  }
  mx = tid > 0 ? tot[0][tid - 1] : kNoMax;
  mn = tid + 1 < kThreads ? tot[1][tid + 1] : kNoMin;
  for (int i = i0; i < i1; ++i) { mx = max(mx, below[i]); below[i] = mx; }
  for (int i = i1 - 1; i >= i0; --i) { mn = min(mn, above[i]); above[i] = mn; }
  __syncthreads();
  // below[p]: largest target < c_p (intervals 0..p); above[p + 1]: smallest target >= c_p (intervals p+1..P)
  const float* __restrict__ e = p.edges + (long long)b * (P + 1);
  const double gs = (double)grad_scale / (double)p.B;
  double term = 0.0;
  for (int i = tid; i < P; i += kThreads) {
    const double cp = (double)(0.5f * (e[i] + e[i + 1]));
    const unsigned kl = below[i], kh = above[i + 1];
    const double dl = cp - (double)fval(kl), dh = (double)fval(kh) - cp;
    const bool use_lo = kl != kNoMax && (kh == kNoMin || dl <= dh);
    const double diff = use_lo ? dl : -dh;                     // c_p - near_p
    term += diff * diff;
    if (grad) {
      double sd = 0.0;
      for (int g = 0; g < G; ++g) sd += p.dsum[(slab0 + g) * P + i];
      sd *= 1.0 / (double)(1ll << kQuantBits);
      grad[(long long)b * P + i] = (float)(gs * (2.0 * diff / (double)P - 2.0 * sd / N));
    }
  }
  red[tid] = term;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double L = red[0] / (double)P + sn[0] / N;
    p.lb[b] = L; loss[1 + b] = (float)L;
  }
}

__global__ void chamfer_mean_kernel(const double* __restrict__ lb, int B, float* __restrict__ loss) {
  __shared__ double red[64];
  double s = 0.0;
  for (int i = threadIdx.x; i < B; i += 64) s += lb[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 32; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)B);
}

inline int chamfer_groups(long long hw) {
  const long long g = (hw + kSub - 1) / kSub;
  return (int)(g < 1 ? 1 : (g > kMaxGroups ? kMaxGroups : g));
}

inline bool chamfer_shape_ok(int B, int Ht, int Wt, int P) {
  return B > 0 && Ht > 0 && Wt > 0 && P >= 1 && P <= kMaxP && (long long)B * Ht * Wt < (1ll << 31);
}

}  // namespace

// ws layout: dsum [B][G][P] f64 | d2n [B][G][2] f64 | lb [B] f64 | kmin [B][G][P+1] u32 | kmax [B][G][P+1] u32
extern "C" size_t cfp_bins_chamfer_ws_bytes(int B, int Ht, int Wt, int P) {
  if (!chamfer_shape_ok(B, Ht, Wt, P)) return 0;
  const size_t slabs = (size_t)B * chamfer_groups((long long)Ht * Wt);
  return (slabs * P + slabs * 2 + (size_t)B) * sizeof(double) + 2 * slabs * (P + 1) * sizeof(unsigned);
}

extern "C" int cfp_bins_chamfer(const float* edges, const float* target, const unsigned char* mask, int B, int Ht, int Wt, int P,
                                float grad_scale, void* ws, size_t ws_bytes, float* loss, float* grad_centers, cfp_stream_t stream) {
  CFP_REQUIRE(edges && target && ws && loss, CFP_EINVAL, "cfp_bins_chamfer: null pointer");
  CFP_REQUIRE(B > 0 && Ht > 0 && Wt > 0, CFP_ESHAPE, "cfp_bins_chamfer: non-positive dimension");
  CFP_REQUIRE(P >= 1 && P <= kMaxP, CFP_ESHAPE, "cfp_bins_chamfer: the number of bins must be in 1..1024");
  CFP_REQUIRE((long long)B * Ht * Wt < (1ll << 31), CFP_ESHAPE, "cfp_bins_chamfer: B*Ht*Wt must be below 2^31");
  CFP_REQUIRE(aligned16(ws), CFP_EINVAL, "cfp_bins_chamfer: workspace must be 16-byte aligned");
  CFP_REQUIRE(ws_bytes >= cfp_bins_chamfer_ws_bytes(B, Ht, Wt, P), CFP_EINVAL, "cfp_bins_chamfer: workspace too small");
  ChamferP p;
  p.edges = edges; p.target = target; p.mask = mask;
  p.HW = (long long)Ht * Wt; p.B = B; p.P = P; p.G = chamfer_groups(p.HW);
  p.chunk = (p.HW + p.G - 1) / p.G;
  const size_t slabs = (size_t)B * p.G;
  p.dsum = reinterpret_cast<double*>(ws);
  p.d2n = p.dsum + slabs * P;
  p.lb = p.d2n + slabs * 2;
  p.kmin = reinterpret_cast<unsigned*>(p.lb + B);
  p.kmax = p.kmin + slabs * (P + 1);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(chamfer_pixels_kernel, dim3((unsigned)slabs), dim3(kThreads), 0, s, p);
  hipLaunchKernelGGL(chamfer_final_kernel, dim3(B), dim3(kThreads), 0, s, p, grad_scale, loss, grad_centers);
  hipLaunchKernelGGL(chamfer_mean_kernel, dim3(1), dim3(64), 0, s, p.lb, B, loss);
  return cfp_check_launch("cfp_bins_chamfer");
}
