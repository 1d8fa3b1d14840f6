// Sparsification curves, AUSE and AURG of the uncertainty planes on the device (include/cfpnet_hip.h, cfp_unc_sparsification).
//
// Per image and ranking (three uncertainty scores, two oracle scores): remove the valid pixels in order of decreasing score and
// report RMSE / abs-rel of the rest at K removal fractions.  No sort: the K boundaries are order statistics of one score, found
// together by a most-significant-digit radix select on an order-preserving uint32 image of the float32 score.
//
//   spars_keys_kernel     one pass over gt, pred and the three planes: the five keys of every pixel -> workspace
//                         (key 0 = pixel outside lo < gt < hi).  Keys 3 and 4 are the images of the terms t0 = d*d and
//                         t1 = |d|/g themselves, so the later passes read 8-12 B per pixel and never touch the inputs again.
//   spars_hist_kernel     radix select, four levels of 8 bits, S slices per (ranking, image): per level one 256-bin count histogram
//                         per still-distinct boundary prefix (<= K of them) in LDS with integer LDS atomics, then one integer
//                         global atomic per non-empty bin.
//   spars_select_kernel   after each level, one workgroup per (ranking, image), one wave per boundary: walks its histogram to fix 8
//                         more bits of its key, the count of keys below it and, at the end, the size of its tie group.
//   spars_sum_kernel      same slices: sums t0 / t1 per segment between two boundaries and per boundary tie group, one slab per slice.
//   spars_curve_kernel    slabs added, the prefix over segments, the tie share t/c, the curve.
//                         One image on one workgroup needs no global counts at all and was the first version: it took 1.2-1.4 ms at
//                         8 x 480x640 whatever the scores, bound by instruction issue on 40 CUs; the slices made it 0.3 ms.
//   spars_summary_kernel  AUSE / AURG per image from the five curves; NaN rows for an image without valid pixels or e0 == 0.
//
// Sums: the per-pixel terms are float32.  Each bucket adds them EXACTLY, as integers: a float32 is m * 2^(e-150) with a 24-bit m,
// and m << (e-1 & 31) is split over two 32-bit digits of a 9-digit base-2^32 number whose digits sit in int64 words (room for
// 2^31 carries).  Integer adds commute, so neither the LDS atomics nor the order of the slices can change a bit; the prefix over
// buckets is integer too, and one conversion to float64 per curve point (nine terms, most significant first) rounds it.  The
// result is the correctly accumulated sum to ~1e-15 relative: inside the float64-sum contract (any order of 3e5 float64 adds is
// within ~3e-11 of it) and bit-identical from run to run and between rankings that keep the same pixels.
#include "common.h"
#include "metrics_pred.h"

namespace {

constexpr int kSpMaxSteps = 100;
constexpr int kSpRank = 5;           // CFP_SPARS_*
constexpr int kSpThreads = 1024;     // histogram / summation kernels: 16 waves per slice
constexpr int kSpMaxSlices = 6;      // workgroups per (ranking, image): 8 images x 5 rankings x 6 fill the chip once
constexpr int kSpUnroll = 8;         // keys per lane and trip: that many independent loads in flight
constexpr int kSpLimbs = 9;          // base-2^32 digits of the exact float32 sum: bit positions 0..253+55
constexpr unsigned kSpNanKey = 0xFFFFFFFFu;

// float32 -> uint32 with the same order: -0 == +0, every NaN is one value above +inf; 0 stays free (the image of a negative NaN,
// which is never produced) and marks an invalid pixel
__device__ __forceinline__ unsigned spars_key(float s) {
  if (s != s) return kSpNanKey;
  unsigned u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float spars_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);      // kSpNanKey -> 0x7FFFFFFF, a NaN
}

struct SpKeyP {
  MetP m;                  // pred, gt, sizes, protocol (partial / out unused)
  const float* unc;        // [B,3,Hp,Wp]
  unsigned* keys;          // [B,5,H*W]
};

__global__ __launch_bounds__(256) void spars_keys_kernel(SpKeyP q) {
  const MetP& p = q.m;
  const int b = blockIdx.y, hwp = p.Hp * p.Wp;
  const size_t hw = (size_t)p.H * p.W;
  const float* pb = p.pred + (long long)b * hwp;
  const float* ub = q.unc + (long long)b * 3 * hwp;
  const float* gb = p.gt + (long long)b * hw;
  unsigned* kb = q.keys + (long long)b * kSpRank * hw;
  for (size_t i0 = blockIdx.x * 256 + threadIdx.x; i0 < hw; i0 += gridDim.x * 256) {
    const int i = (int)i0;
    const float g = gb[i];
    unsigned k0 = 0u, k1 = 0u, k2 = 0u, k3 = 0u, k4 = 0u;
    if (g > p.lo && g < p.hi) {
      const float v = met_pred(p, pb, i);
      const float d = g - v;
      k0 = spars_key(met_plane(p, ub, i));
      k1 = spars_key(met_plane(p, ub + hwp, i));
      k2 = spars_key(1.f - met_plane(p, ub + 2 * hwp, i));
      k3 = spars_key(d * d);
      k4 = spars_key(fabsf(d) / g);
    }
    kb[i] = k0; kb[hw + i] = k1; kb[2 * hw + i] = k2; kb[3 * hw + i] = k3; kb[4 * hw + i] = k4;
  }
}

// what the select knows about the K boundaries of one (image, ranking), carried from level to level in the workspace
struct SpState {
  unsigned pref[kSpMaxSteps];       // boundary k: the key bits fixed so far
  unsigned rem[kSpMaxSteps];        //   1-based rank still to find among the keys that share them (after level 3: t, the kept ties)
  unsigned below[kSpMaxSteps];      //   keys below every key that shares them
  unsigned cnt[kSpMaxSteps];        //   keys that share them (after level 3: c, the tie group of the boundary key)
  int slot[kSpMaxSteps];            //   its histogram (after level 3: its index among the distinct boundary keys)
  unsigned slotpref[kSpMaxSteps];   // distinct prefixes, descending (boundary keys fall as k grows)
  int nslot;
  unsigned n;                       // valid pixels
};
static_assert(sizeof(SpState) % 8 == 0, "workspace sections stay 8-byte aligned");

struct SpRankP {
  const unsigned* keys;             // [B,5,HW]
  SpState* state;                   // [B,5]
  unsigned* ghist;                  // [B,5,K,256] counts of the level in flight, zero between levels
  unsigned long long* slabs;        // [B,5,S,2K,2,kSpLimbs] exact partial sums per slice
  unsigned* slab_flags;             // [B,5,S,2K,2]
  double* curves;                   // [B,5,2,K]
  double* n_valid;                  // [B]
  int HW, K, S, chunk;              // slice s of an image = pixels [s*chunk, min(HW, (s+1)*chunk))
};

// index of `x` in the descending list a[0..n): the number of entries greater than x (== n if x is below all of them)
__device__ __forceinline__ int spars_rank_desc(const unsigned* a, int n, unsigned x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] > x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// exact add of one float32 term into a 9-digit accumulator; non-finite terms only leave a flag (1 +inf, 2 NaN, 4 -inf)
__device__ __forceinline__ void spars_add(unsigned long long* acc, unsigned* flag, float t) {
  const unsigned u = __float_as_uint(t);
  unsigned e = (u >> 23) & 255u, m = u & 0x7FFFFFu;
  if (e == 255u) { atomicOr(flag, m ? 2u : ((u >> 31) ? 4u : 1u)); return; }
  if (e) m |= 0x800000u; else e = 1u;                 // subnormal: same scale as e = 1, no hidden bit
  if (!m) return;
  const unsigned pos = e - 1u;                         // value = m * 2^(pos - 149)
  const unsigned long long v = (unsigned long long)m << (pos & 31u);
  unsigned long long lo = v & 0xFFFFFFFFull, hi = v >> 32;
  if (u >> 31) { lo = 0ull - lo; hi = 0ull - hi; }     // two's complement: the int64 digits may go negative
  unsigned long long* a = acc + (pos >> 5);
  if (lo) atomicAdd(a, lo);
  if (hi) atomicAdd(a + 1, hi);
}

__device__ __forceinline__ double spars_value(const long long (&d)[kSpLimbs], unsigned flag) {
  if ((flag & 2u) || ((flag & 1u) && (flag & 4u))) return __longlong_as_double(0x7FF8000000000000ll);
  if (flag & 1u) return __longlong_as_double(0x7FF0000000000000ll);
  if (flag & 4u) return __longlong_as_double(0xFFF0000000000000ll);
  double s = 0.0;
#pragma unroll
  for (int i = kSpLimbs - 1; i >= 0; --i) s += ldexp((double)d[i], 32 * i - 149);
  return s;
}

// one level of the select, one slice: counts of the next 8 key bits per still-distinct prefix in LDS (integer LDS atomics), then one integer
// global atomic per non-empty bin
__global__ __launch_bounds__(kSpThreads) void spars_hist_kernel(SpRankP p, int level) {
  extern __shared__ __align__(16) unsigned char sp_smem[];
  unsigned* hist = reinterpret_cast<unsigned*>(sp_smem);               // [slots][256]
  __shared__ unsigned s_slotpref[kSpMaxSteps];
  const int s = blockIdx.x, r = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const SpState* st = p.state + b * kSpRank + r;
  if (level && st->n == 0u) return;
  const int nslot = level ? st->nslot : 1;
  if (tid < nslot) s_slotpref[tid] = st->slotpref[tid];
  for (int i = tid; i < nslot * 256; i += kSpThreads) hist[i] = 0u;
  __syncthreads();
  const unsigned* key = p.keys + ((long long)b * kSpRank + r) * p.HW;
  const int end = min(p.HW, (s + 1) * p.chunk), sh = 24 - 8 * level;
  for (int i0 = s * p.chunk + tid; i0 < end; i0 += kSpThreads * kSpUnroll) {       // kSpUnroll independent loads in flight per lane
    unsigned xs[kSpUnroll];
#pragma unroll
    for (int u = 0; u < kSpUnroll; ++u) xs[u] = i0 + u * kSpThreads < end ? key[i0 + u * kSpThreads] : 0u;
#pragma unroll
    for (int u = 0; u < kSpUnroll; ++u) {
      const unsigned x = xs[u];
      if (!x) continue;
      int slot = 0;
      if (level) {
        const unsigned pre = x >> (sh + 8);
        slot = spars_rank_desc(s_slotpref, nslot, pre);
        if (slot >= nslot || s_slotpref[slot] != pre) continue;
      }
      atomicAdd(&hist[slot * 256 + ((x >> sh) & 255u)], 1u);
    }
  }
  __syncthreads();
  unsigned* gh = p.ghist + (long long)(b * kSpRank + r) * p.K * 256;
  for (int i = tid; i < nslot * 256; i += kSpThreads) {
    const unsigned c = hist[i];
    if (c) atomicAdd(&gh[i], c);
  }
}

// after a level: every boundary walks its histogram to fix 8 more bits of its key; the distinct prefixes become the next level's slots
__global__ __launch_bounds__(kSpThreads) void spars_select_kernel(SpRankP p, int level) {
  extern __shared__ __align__(16) unsigned char sp_smem[];
  unsigned* hist = reinterpret_cast<unsigned*>(sp_smem);
  __shared__ unsigned s_pref[kSpMaxSteps];
  const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, K = p.K;
  SpState* st = p.state + b * kSpRank + r;
  if (level && st->n == 0u) return;
  const int nslot = level ? st->nslot : 1;
  unsigned* gh = p.ghist + (long long)(b * kSpRank + r) * K * 256;
  for (int i = tid; i < nslot * 256; i += kSpThreads) { hist[i] = gh[i]; gh[i] = 0u; }      // and leave the counts zero for the next level / call
  __syncthreads();
  // one wave per boundary: lane l holds bins 4l..4l+3, a wave scan gives the counts before them, the first lane whose running count
  // reaches the wanted rank holds the digit
  const int lane = tid & 63;
  for (int k = tid >> 6; k < K; k += kSpThreads / 64) {
    unsigned rem = 0u, below = 0u, pref = 0u;
    int slot = 0;
    if (level) { rem = st->rem[k]; below = st->below[k]; pref = st->pref[k]; slot = st->slot[k]; }
    const uint4 h4 = reinterpret_cast<const uint4*>(hist + slot * 256)[lane];
    const unsigned loc = h4.x + h4.y + h4.z + h4.w;
    unsigned inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_up(inc, o);
      if (lane >= o) inc += v;
    }
    if (level == 0) {
      const unsigned n = __shfl(inc, 63);
      if (k == 0 && lane == 0) st->n = n;
      rem = n - (unsigned)(((unsigned long long)k * n) / (unsigned)K);      // n_k
    }
    const unsigned long long reach = __ballot(inc >= rem);
    const int hit = reach ? __ffsll((long long)reach) - 1 : 63;
    if (lane == hit) {
      const unsigned h[4] = {h4.x, h4.y, h4.z, h4.w};
      unsigned cum = inc - loc, c = h[3];
      int i = 3;
#pragma unroll
      for (int q = 2; q >= 0; --q) {                 // the first of the four bins that reaches the rank (the last one otherwise)
        unsigned before = inc - loc;
#pragma unroll
        for (int w = 0; w < q; ++w) before += h[w];
        if (before + h[q] >= rem) { i = q; cum = before; c = h[q]; }
      }
      if (i == 3) cum = inc - h[3];
      pref = (pref << 8) | (unsigned)(4 * lane + i);
      st->rem[k] = rem - cum; st->below[k] = below + cum; st->pref[k] = pref; st->cnt[k] = c;
      s_pref[k] = pref;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int ns = 0;
    for (int k = 0; k < K; ++k) {
      if (k == 0 || s_pref[k] != s_pref[k - 1]) st->slotpref[ns++] = s_pref[k];
      st->slot[k] = ns - 1;
    }
    st->nslot = ns;
  }
}

// summation pass, one slice.  M distinct boundary keys u_0 > u_1 > ... ; bucket 2j = the tie group of u_j, bucket 2j+1 = the keys strictly
// between u_{j+1} and u_j (everything below u_{M-1} for j = M-1).  u_0 is the largest key (n_0 = N keeps all).
__global__ __launch_bounds__(kSpThreads) void spars_sum_kernel(SpRankP p) {
  extern __shared__ __align__(16) unsigned char sp_smem[];
  __shared__ unsigned s_slotpref[kSpMaxSteps];
  const int s = blockIdx.x, r = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, hw = p.HW;
  const SpState* st = p.state + b * kSpRank + r;
  if (st->n == 0u) return;
  const int M = st->nslot;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(sp_smem);       // [2M][2][kSpLimbs]
  unsigned* flags = reinterpret_cast<unsigned*>(acc + 2 * M * 2 * kSpLimbs);      // [2M][2]
  if (tid < M) s_slotpref[tid] = st->slotpref[tid];
  for (int i = tid; i < 2 * M * 2 * kSpLimbs; i += kSpThreads) acc[i] = 0ull;
  for (int i = tid; i < 2 * M * 2; i += kSpThreads) flags[i] = 0u;
  __syncthreads();
  const unsigned* key = p.keys + ((long long)b * kSpRank + r) * hw;
  const unsigned* key0 = p.keys + ((long long)b * kSpRank + 3) * hw;
  const unsigned* key1 = key0 + hw;
  const int end = min(hw, (s + 1) * p.chunk);
  for (int i0 = s * p.chunk + tid; i0 < end; i0 += kSpThreads * kSpUnroll) {
    unsigned xs[kSpUnroll], a0[kSpUnroll], a1[kSpUnroll];
#pragma unroll
    for (int u = 0; u < kSpUnroll; ++u) {
      const int i = min(i0 + u * kSpThreads, end - 1);
      xs[u] = i0 + u * kSpThreads < end ? key[i] : 0u;
      a0[u] = key0[i]; a1[u] = key1[i];
    }
#pragma unroll
    for (int u = 0; u < kSpUnroll; ++u) {
      const unsigned x = xs[u];
      if (!x) continue;
      const float t0 = spars_unkey(a0[u]), t1 = spars_unkey(a1[u]);
      const int j = spars_rank_desc(s_slotpref, M, x);          // j >= 1 unless x == u_0
      const int bucket = (j < M && s_slotpref[j] == x) ? 2 * j : 2 * (j - 1) + 1;
      if (bucket < 0) continue;                                  // cannot happen (u_0 is the largest key); never index below the array
      spars_add(acc + (bucket * 2 + 0) * kSpLimbs, flags + bucket * 2 + 0, t0);
      spars_add(acc + (bucket * 2 + 1) * kSpLimbs, flags + bucket * 2 + 1, t1);
    }
  }
  __syncthreads();
  const long long slab = (long long)(b * kSpRank + r) * p.S + s;
  unsigned long long* ga = p.slabs + slab * (2 * p.K * 2 * kSpLimbs);
  unsigned* gf = p.slab_flags + slab * (2 * p.K * 2);
  for (int i = tid; i < 2 * M * 2 * kSpLimbs; i += kSpThreads) ga[i] = acc[i];
  for (int i = tid; i < 2 * M * 2; i += kSpThreads) gf[i] = flags[i];
}

// the slices' exact sums added up (integers: any order gives the same bits), the prefix over buckets, the tie share t/c, the curve
__global__ __launch_bounds__(256) void spars_curve_kernel(SpRankP p) {
  extern __shared__ __align__(16) unsigned char sp_smem[];
  const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, K = p.K;
  const SpState* st = p.state + b * kSpRank + r;
  double* cv = p.curves + ((long long)b * kSpRank + r) * 2 * K;
  const unsigned n = st->n;
  if (r == 0 && tid == 0) p.n_valid[b] = (double)n;
  if (n == 0u) {
    for (int i = tid; i < 2 * K; i += 256) cv[i] = __longlong_as_double(0x7FF8000000000000ll);
    return;
  }
  const int M = st->nslot;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(sp_smem);       // [2M][2][kSpLimbs]
  unsigned* flags = reinterpret_cast<unsigned*>(acc + 2 * M * 2 * kSpLimbs);      // [2M][2]
  const long long slab0 = (long long)(b * kSpRank + r) * p.S;
  for (int i = tid; i < 2 * M * 2 * kSpLimbs; i += 256) {
    unsigned long long a = 0ull;
    for (int s = 0; s < p.S; ++s) a += p.slabs[(slab0 + s) * (2 * K * 2 * kSpLimbs) + i];
    acc[i] = a;
  }
  for (int i = tid; i < 2 * M * 2; i += 256) {
    unsigned f = 0u;
    for (int s = 0; s < p.S; ++s) f |= p.slab_flags[(slab0 + s) * (2 * K * 2) + i];
    flags[i] = f;
  }
  __syncthreads();
  if (tid < K) {
    const int j = st->slot[tid];
    const unsigned t = st->rem[tid], c = st->cnt[tid];      // t of the c tied keys are kept
    const unsigned nk = st->below[tid] + t;
    const bool whole = t == c;
    const int first = whole ? 2 * j : 2 * j + 1;        // every bucket from here on is kept entirely
    double S[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      long long d[kSpLimbs];
#pragma unroll
      for (int l = 0; l < kSpLimbs; ++l) d[l] = 0ll;
      unsigned fl = 0u;
      for (int q = first; q < 2 * M; ++q) {
        const unsigned long long* a = acc + (q * 2 + m) * kSpLimbs;
#pragma unroll
        for (int l = 0; l < kSpLimbs; ++l) d[l] += (long long)a[l];
        fl |= flags[q * 2 + m];
      }
      S[m] = spars_value(d, fl);
      if (!whole) {
        const unsigned long long* a = acc + (2 * j * 2 + m) * kSpLimbs;
#pragma unroll
        for (int l = 0; l < kSpLimbs; ++l) d[l] = (long long)a[l];
        S[m] += ((double)t / (double)c) * spars_value(d, flags[2 * j * 2 + m]);
      }
    }
    cv[tid] = sqrt(S[0] / (double)nk);
    cv[K + tid] = S[1] / (double)nk;
  }
}

__global__ __launch_bounds__(64) void spars_summary_kernel(double* __restrict__ curves, double* __restrict__ summary,
                                                           const double* __restrict__ n_valid, int K) {
  const int b = blockIdx.x, tid = threadIdx.x;
  double* cv = curves + (long long)b * kSpRank * 2 * K;
  double* sm = summary + (long long)b * 12;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const double e0r = cv[3 * 2 * K], e0a = cv[(3 * 2 + 1) * K];     // k = 0 keeps every pixel: the same exact sum in all rankings
  if (n_valid[b] == 0.0 || e0r == 0.0 || e0a == 0.0) {
    __syncthreads();                                                // every lane has read e0 before the row is overwritten
    for (int i = tid; i < kSpRank * 2 * K; i += 64) cv[i] = nan;
    if (tid < 12) sm[tid] = nan;
    return;
  }
  if (tid < 6) {
    const int u = tid >> 1, m = tid & 1;
    const double e0 = m ? e0a : e0r;
    const double* cu = cv + (u * 2 + m) * K;
    const double* co = cv + ((3 + m) * 2 + m) * K;
    double a = 0.0, g = 0.0;
    for (int k = 0; k < K; ++k) { a += cu[k] - co[k]; g += e0 - cu[k]; }
    sm[(u * 2 + m) * 2 + 0] = a / (double)K / e0;
    sm[(u * 2 + m) * 2 + 1] = g / (double)K / e0;
  }
}

int spars_slices(long long hw) { return (int)std::min<long long>(kSpMaxSlices, (hw + 16383) / 16384); }
size_t spars_lds_bytes(int K) { return (size_t)K * 256 * sizeof(unsigned); }    // >= the 2K buckets of the summation pass (304 B per step)

// workspace sections, each a multiple of 8 bytes
struct SpLayout { size_t keys, state, ghist, slabs, flags, total; };
SpLayout spars_layout(int B, int H, int W, int K) {
  const size_t hw = (size_t)H * W, S = (size_t)spars_slices((long long)hw), img = (size_t)B * kSpRank;
  SpLayout l;
  l.keys = 0;
  l.state = (img * hw * sizeof(unsigned) + 7) & ~(size_t)7;
  l.ghist = l.state + img * sizeof(SpState);
  l.slabs = l.ghist + img * K * 256 * sizeof(unsigned);
  l.flags = l.slabs + img * S * 2 * K * 2 * kSpLimbs * sizeof(unsigned long long);
  l.total = l.flags + img * S * 2 * K * 2 * sizeof(unsigned);
  return l;
}

}  // namespace

extern "C" size_t cfp_unc_sparsification_ws_bytes(int B, int H, int W, int steps) {
  if (B <= 0 || H <= 0 || W <= 0 || steps <= 0) return 0;
  return spars_layout(B, H, W, steps).total;
}

extern "C" int cfp_unc_sparsification(const float* pred, const float* unc, int Hp, int Wp, const float* gt, int H, int W, int B,
                                      int interpolate, int mode, float lo, float hi, int steps, void* ws, size_t ws_bytes,
                                      double* curves, double* summary, double* n_valid, cfp_stream_t stream) {
  CFP_REQUIRE(pred && unc && gt && ws && curves && summary && n_valid, CFP_EINVAL, "cfp_unc_sparsification: null pointer");
  CFP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0, CFP_ESHAPE, "cfp_unc_sparsification: non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) && B <= 65535, CFP_ESHAPE, "cfp_unc_sparsification: image or batch too large");
  CFP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, "cfp_unc_sparsification: sizes differ and interpolate is off");
  CFP_REQUIRE(mode == 0 || mode == 1, CFP_EINVAL, "cfp_unc_sparsification: mode must be 0 (evaluate_all) or 1 (validate)");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, "cfp_unc_sparsification: empty depth range");
  CFP_REQUIRE(steps >= 1 && steps <= kSpMaxSteps, CFP_EINVAL, "cfp_unc_sparsification: steps must be 1..100");
  CFP_REQUIRE(ws_bytes >= cfp_unc_sparsification_ws_bytes(B, H, W, steps), CFP_EINVAL, "cfp_unc_sparsification: workspace too small");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, CFP_EINVAL, "cfp_unc_sparsification: workspace must be 8-byte aligned");
  static bool attr = false;
  if (!attr) {
    CFP_REQUIRE(hipFuncSetAttribute((const void*)spars_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)spars_lds_bytes(kSpMaxSteps)) == hipSuccess &&
                hipFuncSetAttribute((const void*)spars_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)spars_lds_bytes(kSpMaxSteps)) == hipSuccess,
                CFP_EHIP, "cfp_unc_sparsification: cannot reserve LDS for the select kernels");
    attr = true;
  }
  SpKeyP q;
  q.m = met_params(pred, gt, Hp, Wp, H, W, B, interpolate, mode, lo, hi);
  q.unc = unc; q.keys = reinterpret_cast<unsigned*>(ws);
  const SpLayout l = spars_layout(B, H, W, steps);
  unsigned char* base = reinterpret_cast<unsigned char*>(ws);
  SpRankP p;
  p.keys = q.keys; p.state = reinterpret_cast<SpState*>(base + l.state); p.ghist = reinterpret_cast<unsigned*>(base + l.ghist);
  p.slabs = reinterpret_cast<unsigned long long*>(base + l.slabs); p.slab_flags = reinterpret_cast<unsigned*>(base + l.flags);
  p.curves = curves; p.n_valid = n_valid; p.HW = H * W; p.K = steps;
  p.S = spars_slices((long long)H * W);
  p.chunk = (p.HW + p.S - 1) / p.S;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int kblocks = (int)std::min<long long>(((long long)H * W + 255) / 256, 256);
  CFP_REQUIRE(hipMemsetAsync(p.ghist, 0, l.slabs - l.ghist, s) == hipSuccess, CFP_EHIP, "cfp_unc_sparsification: cannot clear the histograms");
  hipLaunchKernelGGL(spars_keys_kernel, dim3(kblocks, B), dim3(256), 0, s, q);
  for (int level = 0; level < 4; ++level) {
    hipLaunchKernelGGL(spars_hist_kernel, dim3(p.S, kSpRank, B), dim3(kSpThreads), spars_lds_bytes(steps), s, p, level);
    hipLaunchKernelGGL(spars_select_kernel, dim3(kSpRank, B), dim3(kSpThreads), spars_lds_bytes(steps), s, p, level);
  }
  const size_t bucket_lds = (size_t)steps * (2 * 2 * kSpLimbs * 8 + 2 * 2 * 4);
  hipLaunchKernelGGL(spars_sum_kernel, dim3(p.S, kSpRank, B), dim3(kSpThreads), bucket_lds, s, p);
  hipLaunchKernelGGL(spars_curve_kernel, dim3(kSpRank, B), dim3(256), bucket_lds, s, p);
  hipLaunchKernelGGL(spars_summary_kernel, dim3(B), dim3(64), 0, s, curves, summary, n_valid, steps);
  return cfp_check_launch("cfp_unc_sparsification");
}
