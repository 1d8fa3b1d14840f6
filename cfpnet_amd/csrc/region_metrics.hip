// Region- and range-resolved depth metrics on the device: the nine metrics of metrics.hip, per image, split by where a pixel lies
// relative to the ToF zones and by how far away it is.  One pass over prediction and ground truth.
//
//   reference hooks: `my_mask`, the rectangle spanned by the first and the last zone (src/dataloader/nyu.py:182-187, zjuL5.py:137-144),
//   the flags --zone_area_only / --outside_zone_area_only (src/config.py:90-91) and the commented-out depth-range mask of
//   evaluate_all.py:81-82.  The protocols (mode 0 / 1, clip / bilinear order, valid = lo < gt < hi) are those of metrics.hip: the
//   prediction at a pixel is met_pred of metrics_pred.h, bit for bit.
//
// Every valid pixel falls into exactly one CELL = zone class (outside the FoV rectangle / inside a zone whose mask is set / inside the
// FoV rectangle otherwise) x depth range (number of edges e with gt >= e).  All ten accumulated terms are additive, so the kernel sums
// per cell and the finalise kernel forms the unions (all, fov_in, "all depths") from the cell sums.
//
// Shape: a wave walks steps of 256 contiguous pixels (4 per lane).  Regions and depth are spatially coherent, so a step holds few
// distinct cells (usually 1-3); for each one present -- picked wave-uniformly -- the lanes add the float32 terms of their matching
// pixels in float64, a fixed xor butterfly reduces the six real-valued terms, the four counts (a1 a2 a3 n) are popcounts of ballots,
// and lanes 0..9 add the ten values into a wave-private LDS table.  Tables leave as per-workgroup partials; the finalise kernel adds
// them in index order.  No floating-point atomics anywhere: the order is a function of the inputs alone, repeated launches are
// bit-identical.  Up to 24 cells x 10 doubles live in LDS (7.5 KB per workgroup), not in registers; the kernel uses no scratch.
#include "common.h"
#include "metrics_pred.h"

namespace {

constexpr int kRegBlocks = 96;                        // workgroups per image
constexpr int kRegTerms = 10;                         // a1 a2 a3 abs_rel se log10 le2 le sq_rel n  (the order of metrics.hip)
constexpr int kRegMaxEdges = 7;
constexpr int kRegMaxCells = 3 * (kRegMaxEdges + 1);
constexpr int kRegU = 4;                              // pixels per lane and step
constexpr int kRegStep = 64 * kRegU;

struct RegP {
  MetP m;
  const float* rect; const unsigned char* mask;
  int Z, n_edges;
  float edges[kRegMaxEdges];                          // unused entries are +inf: no valid gt reaches them
};

// The zone grid of one image when it is what the simulation lays down (src/utils/dataloader.py:121-123): Z = n*n <= 64 rectangles,
// row-major, integer-valued, one size, constant pitch >= size.  Then membership is integer arithmetic on the pixel; any other set of
// rectangles takes the loop over the rectangles, which is the definition.
struct ZoneGrid {
  int n, sy0, sx0, ph, pw, h, w;
  float iph, ipw;
  unsigned long long bits;                            // mask[z] != 0 at bit z
};

__device__ __forceinline__ bool reg_isint(float v) { return fabsf(v) < 1048576.f && v == truncf(v); }

// floor(r / p) for 0 <= r < 2^24, p > 0: the float quotient is off by at most one
__device__ __forceinline__ int reg_div(int r, int p, float ip) {
  int q = (int)((float)r * ip);
  if (q * p > r) --q;
  else if ((q + 1) * p <= r) ++q;
  return q;
}

__global__ __launch_bounds__(256) void region_metrics_kernel(RegP p) {
  __shared__ double tab[4][kRegMaxCells * kRegTerms];
  __shared__ unsigned long long s_bits;
  const MetP& m = p.m;
  const int b = blockIdx.y;
  const int hw = m.H * m.W;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* pb = m.pred + (long long)b * m.Hp * m.Wp;
  const float* gb = m.gt + (long long)b * hw;
  const float* rb = p.rect + (long long)b * p.Z * 4;
  const unsigned char* mb = p.mask + (long long)b * p.Z;
  const int R = p.n_edges + 1;

  for (int k = lane; k < kRegMaxCells * kRegTerms; k += 64) tab[wave][k] = 0.0;

  // the FoV rectangle (`my_mask`): first zone's start, last zone's end, truncated and clamped to the image
  const float f_aa = rb[0], f_bb = rb[1], f_cc = rb[(p.Z - 1) * 4 + 2], f_dd = rb[(p.Z - 1) * 4 + 3];
  const int aa = max(0, (int)f_aa), bb = max(0, (int)f_bb), cc = min(m.H, (int)f_cc), dd = min(m.W, (int)f_dd);

  // is this image's zone set the regular grid?  (uniform part first, then one rectangle per thread)
  ZoneGrid zg;
  bool cand = p.Z <= 64;
  zg.n = 0;
  if (cand) {
    int n = (int)sqrtf((float)p.Z);
    while (n * n > p.Z) --n;
    while ((n + 1) * (n + 1) <= p.Z) ++n;
    zg.n = n;
    cand = n * n == p.Z;
  }
  cand = cand && reg_isint(f_aa) && reg_isint(f_bb) && reg_isint(rb[2]) && reg_isint(rb[3]);
  zg.sy0 = cand ? (int)f_aa : 0; zg.sx0 = cand ? (int)f_bb : 0;
  zg.h = cand ? (int)rb[2] - zg.sy0 : 1; zg.w = cand ? (int)rb[3] - zg.sx0 : 1;
  zg.ph = zg.h; zg.pw = zg.w;
  if (cand && zg.n > 1) {
    const float ny = rb[zg.n * 4], nx = rb[4 + 1];
    cand = reg_isint(ny) && reg_isint(nx);
    if (cand) { zg.ph = (int)ny - zg.sy0; zg.pw = (int)nx - zg.sx0; }
  }
  cand = cand && zg.h > 0 && zg.w > 0 && zg.ph >= zg.h && zg.pw >= zg.w;
  bool mine_ok = true;
  if (cand && (int)threadIdx.x < p.Z) {
    const int z = threadIdx.x, zy = z / zg.n, zx = z - zy * zg.n;
    const float r0 = rb[z * 4], r1 = rb[z * 4 + 1], r2 = rb[z * 4 + 2], r3 = rb[z * 4 + 3];
    const int sy = zg.sy0 + zy * zg.ph, sx = zg.sx0 + zx * zg.pw;
    mine_ok = reg_isint(r0) && reg_isint(r1) && reg_isint(r2) && reg_isint(r3) && r0 == (float)sy && r1 == (float)sx &&
              r2 == (float)(sy + zg.h) && r3 == (float)(sx + zg.w);
  }
  if (wave == 0) {
    const unsigned long long bits = __ballot(lane < p.Z && mb[min(lane, p.Z - 1)] != 0);
    if (lane == 0) s_bits = bits;
  }
  const bool is_grid = __syncthreads_and(cand && mine_ok) != 0;     // also orders the zeroed tables and s_bits
  zg.bits = s_bits;
  zg.iph = 1.f / (float)zg.ph; zg.ipw = 1.f / (float)zg.pw;

  const int nsteps = (hw + kRegStep - 1) / kRegStep;
  for (int step = blockIdx.x * 4 + wave; step < nsteps; step += kRegBlocks * 4) {
    const int base = step * kRegStep;
    float g[kRegU], v[kRegU];
#pragma unroll
    for (int u = 0; u < kRegU; ++u) g[u] = gb[min(base + u * 64 + lane, hw - 1)];
#pragma unroll
    for (int u = 0; u < kRegU; ++u) v[u] = met_pred(m, pb, min(base + u * 64 + lane, hw - 1));

    // zone class per pixel: 0 outside the FoV rectangle, 1 in a zone whose mask is set, 2 in the FoV rectangle otherwise
    int zc[kRegU], py[kRegU], px[kRegU];
#pragma unroll
    for (int u = 0; u < kRegU; ++u) {
      const int i = min(base + u * 64 + lane, hw - 1);
      py[u] = i / m.W; px[u] = i - py[u] * m.W;
      zc[u] = (py[u] >= aa && py[u] < cc && px[u] >= bb && px[u] < dd) ? 2 : 0;
    }
    if (is_grid) {
#pragma unroll
      for (int u = 0; u < kRegU; ++u) {
        if (zc[u] == 0) continue;
        const int ry = py[u] - zg.sy0, rx = px[u] - zg.sx0;          // >= 0 inside the FoV rectangle, below n * pitch
        const int zy = reg_div(ry, zg.ph, zg.iph), zx = reg_div(rx, zg.pw, zg.ipw);
        const bool in = ry - zy * zg.ph < zg.h && rx - zx * zg.pw < zg.w;
        if (in && ((zg.bits >> (zy * zg.n + zx)) & 1ull)) zc[u] = 1;
      }
    } else {
      // the definition: sy <= y < ey && sx <= x < ex in float, over the zones whose mask is set; zones whose rows miss the
      // step's rows are skipped for the whole wave
      const float ylo = (float)(base / m.W), yhi = (float)(min(base + kRegStep - 1, hw - 1) / m.W);
      float fy[kRegU], fx[kRegU];
#pragma unroll
      for (int u = 0; u < kRegU; ++u) { fy[u] = (float)py[u]; fx[u] = (float)px[u]; }
      for (int z = 0; z < p.Z; ++z) {
        if (mb[z] == 0) continue;
        const float sy = rb[z * 4], sx = rb[z * 4 + 1], ey = rb[z * 4 + 2], ex = rb[z * 4 + 3];
        if (!(sy <= yhi && ey > ylo)) continue;
#pragma unroll
        for (int u = 0; u < kRegU; ++u)
          if (zc[u] == 2 && sy <= fy[u] && fy[u] < ey && sx <= fx[u] && fx[u] < ex) zc[u] = 1;
      }
    }

    // per-pixel terms (float32, as metrics.hip) and the cell id; -1 = not a valid pixel
    int cell[kRegU];
    float t[kRegU][6];
    unsigned long long b1[kRegU], b2[kRegU], b3[kRegU];
#pragma unroll
    for (int u = 0; u < kRegU; ++u) {
      const bool valid = base + u * 64 + lane < hw && g[u] > m.lo && g[u] < m.hi;
      int r = 0;
#pragma unroll
      for (int e = 0; e < kRegMaxEdges; ++e) r += g[u] >= p.edges[e] ? 1 : 0;
      cell[u] = valid ? zc[u] * R + r : -1;
      const float th = fmaxf(g[u] / v[u], v[u] / g[u]);
      const float d = g[u] - v[u];
      const float le = logf(g[u]) - logf(v[u]);
      b1[u] = __ballot(th < 1.25f);
      b2[u] = __ballot(th < 1.5625f);
      b3[u] = __ballot(th < 1.953125f);
      t[u][0] = fabsf(d) / g[u];
      t[u][1] = d * d;
      t[u][2] = fabsf(log10f(g[u]) - log10f(v[u]));
      t[u][3] = le * le;
      t[u][4] = -le;                            // err = log pred - log gt
      t[u][5] = (d * d) / g[u];
    }

    // one round per cell present in the step, smallest pending id of the first lane that has one
    for (;;) {
      int pend = 0x7fffffff;
#pragma unroll
      for (int u = 0; u < kRegU; ++u) pend = cell[u] >= 0 ? min(pend, cell[u]) : pend;
      const unsigned long long any = __ballot(pend != 0x7fffffff);
      if (any == 0) break;
      const int c = __builtin_amdgcn_readlane(pend, __ffsll((long long)any) - 1);
      double s[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) s[k] = 0.0;
      int n = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
      for (int u = 0; u < kRegU; ++u) {
        const bool hit = cell[u] == c;
        const unsigned long long hb = __ballot(hit);
        n += __popcll(hb); a1 += __popcll(hb & b1[u]); a2 += __popcll(hb & b2[u]); a3 += __popcll(hb & b3[u]);
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += hit ? (double)t[u][k] : 0.0;
        if (hit) cell[u] = -1;
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
      }
      const double val = lane == 0 ? (double)a1 : lane == 1 ? (double)a2 : lane == 2 ? (double)a3 : lane == 3 ? s[0] : lane == 4 ? s[1]
                       : lane == 5 ? s[2] : lane == 6 ? s[3] : lane == 7 ? s[4] : lane == 8 ? s[5] : (double)n;
      if (lane < kRegTerms) tab[wave][c * kRegTerms + lane] += val;
    }
  }
  __syncthreads();
  const int nc = 3 * R * kRegTerms;
  if ((int)threadIdx.x < nc)
    m.partial[((long long)b * kRegBlocks + blockIdx.x) * nc + threadIdx.x] =
        ((tab[0][threadIdx.x] + tab[1][threadIdx.x]) + tab[2][threadIdx.x]) + tab[3][threadIdx.x];
}

// out[b][region][q][10]: region CFP_REGION_*, q = 0 "all depths" / 1 + r range r, the ten values of cfp_eval_metrics
__global__ __launch_bounds__(256) void region_metrics_finalize_kernel(const double* __restrict__ partial, double* __restrict__ out, int R, int Q) {
  __shared__ double cs[kRegMaxCells * kRegTerms];
  const int b = blockIdx.x, t = threadIdx.x;
  const int nc = 3 * R * kRegTerms;
  static_assert(kRegBlocks % 4 == 0, "four chains over the partials");
  if (t < nc) {
    const double* pp = partial + (long long)b * kRegBlocks * nc + t;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < kRegBlocks; j += 4) {        // four independent chains, combined in a fixed order
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] += pp[(long long)(j + q) * nc];
    }
    cs[t] = (a[0] + a[1]) + (a[2] + a[3]);
  }
  __syncthreads();
  if (t >= 5 * Q) return;
  const int region = t / Q, q = t - region * Q;
  const int classes = region == 0 ? 7 : region == 1 ? 6 : region == 2 ? 1 : region == 3 ? 2 : 4;    // bit zc: outside, zone_valid, zone_invalid
  const int r0 = q == 0 ? 0 : q - 1, r1 = q == 0 ? R : q;
  double s[kRegTerms];
#pragma unroll
  for (int k = 0; k < kRegTerms; ++k) s[k] = 0.0;
  for (int zc = 0; zc < 3; ++zc) {
    if (!((classes >> zc) & 1)) continue;
    for (int r = r0; r < r1; ++r) {
#pragma unroll
      for (int k = 0; k < kRegTerms; ++k) s[k] += cs[(zc * R + r) * kRegTerms + k];
    }
  }
  const double n = s[9];
  double* o = out + (((long long)b * 5 + region) * Q + q) * kRegTerms;
  const double mle = s[7] / n;
  o[0] = s[0] / n; o[1] = s[1] / n; o[2] = s[2] / n;
  o[3] = s[3] / n;
  o[4] = sqrt(s[4] / n);
  o[5] = s[5] / n;
  o[6] = sqrt(s[6] / n);
  o[7] = sqrt(s[6] / n - mle * mle) * 100.0;
  o[8] = s[8] / n;
  o[9] = n;
}

}  // namespace

extern "C" size_t cfp_eval_metrics_regions_ws_bytes(int B) {
  return B > 0 ? (size_t)B * kRegBlocks * kRegMaxCells * kRegTerms * sizeof(double) : 0;
}

extern "C" int cfp_eval_metrics_regions(const float* pred, int Hp, int Wp, const float* gt, int H, int W, int B, int interpolate, int mode,
                                        float lo, float hi, const float* rect, const unsigned char* mask, int Z, const float* edges,
                                        int n_edges, void* ws, size_t ws_bytes, double* out, cfp_stream_t stream) {
  CFP_REQUIRE(pred && gt && rect && mask && ws && out, CFP_EINVAL, "cfp_eval_metrics_regions: null pointer");
  CFP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0, CFP_ESHAPE, "cfp_eval_metrics_regions: non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) - 2 * kRegStep && B <= 65535, CFP_ESHAPE, "cfp_eval_metrics_regions: image or batch too large");
  CFP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, "cfp_eval_metrics_regions: sizes differ and interpolate is off");
  CFP_REQUIRE(Z > 0, CFP_ESHAPE, "cfp_eval_metrics_regions: Z must be positive");
  CFP_REQUIRE(n_edges >= 0 && n_edges <= kRegMaxEdges, CFP_EINVAL, "cfp_eval_metrics_regions: n_edges must be 0..7");
  CFP_REQUIRE(n_edges == 0 || edges, CFP_EINVAL, "cfp_eval_metrics_regions: null pointer (edges)");
  CFP_REQUIRE(mode == 0 || mode == 1, CFP_EINVAL, "cfp_eval_metrics_regions: mode must be 0 (evaluate_all) or 1 (validate)");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, "cfp_eval_metrics_regions: empty depth range");
  CFP_REQUIRE(ws_bytes >= cfp_eval_metrics_regions_ws_bytes(B), CFP_EINVAL, "cfp_eval_metrics_regions: workspace too small");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, CFP_EINVAL, "cfp_eval_metrics_regions: workspace must be 8-byte aligned");
  RegP p;
  for (int e = 0; e < kRegMaxEdges; ++e) p.edges[e] = INFINITY;
  for (int e = 0; e < n_edges; ++e) {                     // edges is the one host pointer of the call
    const float v = edges[e];
    CFP_REQUIRE(std::isfinite(v) && (e == 0 || v > edges[e - 1]), CFP_EINVAL,
                "cfp_eval_metrics_regions: edges must be finite and strictly increasing");
    p.edges[e] = v;
  }
  MetP& m = p.m;
  m = met_params(pred, gt, Hp, Wp, H, W, B, interpolate, mode, lo, hi);
  m.partial = reinterpret_cast<double*>(ws); m.out = out;
  p.rect = rect; p.mask = mask; p.Z = Z; p.n_edges = n_edges;
  const int R = n_edges + 1, Q = n_edges == 0 ? 1 : n_edges + 2;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(region_metrics_kernel, dim3(kRegBlocks, B), dim3(256), 0, s, p);
  hipLaunchKernelGGL(region_metrics_finalize_kernel, dim3(B), dim3(256), 0, s, m.partial, out, R, Q);
  return cfp_check_launch("cfp_eval_metrics_regions");
}
