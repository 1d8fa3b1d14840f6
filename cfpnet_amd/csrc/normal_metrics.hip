// Surface-normal error of the predicted geometry against the ground truth's, per image, on the device (cfp_normal_metrics): the angle
// between the normal of the prediction and the normal of the ground-truth depth at every pixel, its mean / median / RMSE and the share
// of pixels below 11.25, 22.5 and 30 degrees -- the standard set of the normal-estimation literature.  The definition is in
// include/cfpnet_hip.h.
//
//   The depth of the prediction at a pixel is met_pred of metrics_pred.h in mode 0, the value cfp_eval_metrics evaluates, bit for bit.
//   The normal is the `Normal` of cfp_depth_unproject (pointcloud.hip), restated here in the same order of float32 operations so that
//   the same five depths and intrinsics give the same three floats; tests/test_normal_metrics_gpu.py holds the two together.
//
// Main kernel.  A workgroup of 256 lanes owns tiles of 16 x 64 pixels of one image (grid.y), strided over at most kNmGroups workgroups
// per image.  It stages the met_pred depths and the ground truth of the tile and a 1-pixel halo in LDS (two 18 x 66 float tiles; a halo
// cell outside the image holds the value at the clamped coordinate, which is the clamped neighbour of the definition, so the edge needs
// no branch), then each wave takes four rows, one pixel per lane and row: both normals, the angle, the optional angle map.  Counts are
// integers and order-independent: the histogram and the four counters (N and the three thresholds) are LDS atomics per workgroup, added
// to the image's cells in the workspace with global integer atomics when the workgroup is done (the non-zero cells only).  The two
// float64 sums never see an atomic: per lane in tile order, a butterfly inside the wave, the four waves in order, one partial per
// workgroup.
// Finalize kernel.  One workgroup per image adds the partials in a fixed order, scans the histogram for the median and writes `out`
// (and `hist`).
#include "common.h"
#include "metrics_pred.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kTileH = 16, kTileW = 64;
constexpr int kHaloH = kTileH + 2, kHaloW = kTileW + 2;
constexpr int kRowsPerWave = kTileH / 4;
constexpr int kNmBins = 1800;                         // 0.1 degree each
constexpr int kNmCells = kNmBins + 4;                 // + N, a < 11.25, a < 22.5, a < 30
constexpr int kNmGroups = 512;                        // workgroups per image at most: two partials per lane of the finalize kernel
constexpr int kNmOut = 7;

struct NormP {
  MetP m;                                             // pred, gt, Hp, Wp, H, W, interpolate, mode 0, lo, hi, sy, sx
  const float* K;
  double* partial;                                    // [B][groups][2]: sum a, sum a*a
  int* cells;                                         // [B][kNmCells]: the histogram, then the four counters; zero before the launch
  float* angle_map;
  int tiles_x, tiles, groups;                         // tiles and workgroups per image
};

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }      // false for NaN

// `Normal` of cfp_depth_unproject from the five depths around c (a staged tile with pitch kHaloW); false and (0, 0, 0) for the zero normal
__device__ __forceinline__ bool normal_at(const float* c, int x, int y, int W, int H, float fx, float fy, float cx, float cy, float rx,
                                          float ry, float& ox, float& oy, float& oz) {
  const float d = c[0], d0 = c[-1], d1 = c[1], e0 = c[-kHaloW], e1 = c[kHaloW];
  const int x0 = max(x - 1, 0), x1 = min(x + 1, W - 1), y0 = max(y - 1, 0), y1 = min(y + 1, H - 1);
  const float kx = (float)(x1 - x0), ky = (float)(y1 - y0);
  const float xm = 0.5f * (float)(x0 + x1), ym = 0.5f * (float)(y0 + y1);
  const float dd = d1 - d0, ds = d1 + d0, ed = e1 - e0, es = e1 + e0;
  const float txx = dd * ((xm - cx) / fx) + ds * (0.5f * kx / fx), txy = dd * ry, txz = dd;
  const float tyx = ed * rx, tyy = ed * ((ym - cy) / fy) + es * (0.5f * ky / fy), tyz = ed;
  const float nx = tyy * txz - tyz * txy, ny = tyz * txx - tyx * txz, nz = tyx * txy - tyy * txx;      // T_y x T_x
  const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
  const bool ok = finitef(d) && finitef(d0) && finitef(d1) && finitef(e0) && finitef(e1) && len > 0.f && finitef(len);
  ox = ok ? nx / len : 0.f; oy = ok ? ny / len : 0.f; oz = ok ? nz / len : 0.f;
  return ok;
}

template <bool MAP>
__global__ __launch_bounds__(256) void normal_metrics_kernel(NormP p) {
  __shared__ float sD[kHaloH * kHaloW];
  __shared__ float sG[kHaloH * kHaloW];
  __shared__ int sCells[kNmCells];
  __shared__ double sRed[4][2];
  const MetP& m = p.m;
  const int H = m.H, W = m.W;
  const int b = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* pb = m.pred + (long long)b * m.Hp * m.Wp;
  const float* gb = m.gt + (long long)b * H * W;
  const float fx = p.K[b * 4 + 0], fy = p.K[b * 4 + 1], cx = p.K[b * 4 + 2], cy = p.K[b * 4 + 3];
  const float lo = m.lo, hi = m.hi;

  for (int c = threadIdx.x; c < kNmCells; c += 256) sCells[c] = 0;
  double sum_a = 0.0, sum_aa = 0.0;
  int n = 0, n11 = 0, n22 = 0, n30 = 0;               // wave-uniform

  for (int t = blockIdx.x; t < p.tiles; t += p.groups) {
    const int tyi = t / p.tiles_x, txi = t - tyi * p.tiles_x;
    const int ty0 = tyi * kTileH, tx0 = txi * kTileW;

    __syncthreads();                                  // the tile before is read; the first time: sCells is zero
    for (int c = threadIdx.x; c < kHaloH * kHaloW; c += 256) {
      const int hy = c / kHaloW, hx = c - hy * kHaloW;
      const int gy = min(max(ty0 + hy - 1, 0), H - 1), gx = min(max(tx0 + hx - 1, 0), W - 1);
      sD[c] = met_pred(m, pb, gy * W + gx);
      sG[c] = gb[gy * W + gx];
    }
    __syncthreads();

    const int x = tx0 + lane;
    const float rx = ((float)x - cx) / fx;
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
      const int ly = wave * kRowsPerWave + r, y = ty0 + ly;
      const int ci = (ly + 1) * kHaloW + lane + 1;
      const float ry = ((float)y - cy) / fy;
      float px, py, pz, qx, qy, qz;
      const bool okp = normal_at(sD + ci, x, y, W, H, fx, fy, cx, cy, rx, ry, px, py, pz);
      const bool okg = normal_at(sG + ci, x, y, W, H, fx, fy, cx, cy, rx, ry, qx, qy, qz);
      const float* g = sG + ci;
      const float g0 = g[0], g1 = g[-1], g2 = g[1], g3 = g[-kHaloW], g4 = g[kHaloW];
      const bool in = x < W && y < H;
      const bool valid = in && okp && okg && g0 > lo && g0 < hi && g1 > lo && g1 < hi && g2 > lo && g2 < hi && g3 > lo && g3 < hi &&
                         g4 > lo && g4 < hi;
      const float dot = (px * qx + py * qy) + pz * qz;
      const float ux = py * qz - pz * qy, uy = pz * qx - px * qz, uz = px * qy - py * qx;
      const float a = atan2f(sqrtf((ux * ux + uy * uy) + uz * uz), dot) * 57.29577951308232f;
      if (valid) {
        sum_a += (double)a;
        sum_aa += (double)(a * a);
        atomicAdd(&sCells[min((int)(a * 10.0f), kNmBins - 1)], 1);
      }
      n += __popcll(__ballot(valid));
      n11 += __popcll(__ballot(valid && a < 11.25f));
      n22 += __popcll(__ballot(valid && a < 22.5f));
      n30 += __popcll(__ballot(valid && a < 30.0f));
      if constexpr (MAP) {
        if (in) p.angle_map[((long long)b * H + y) * W + x] = valid ? a : __builtin_nanf("");
      }
    }
  }

  // the float64 sums: butterfly inside the wave, then the four waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sum_a += __shfl_xor(sum_a, o); sum_aa += __shfl_xor(sum_aa, o); }
  if (lane == 0) {
    sRed[wave][0] = sum_a; sRed[wave][1] = sum_aa;
    atomicAdd(&sCells[kNmBins + 0], n); atomicAdd(&sCells[kNmBins + 1], n11);
    atomicAdd(&sCells[kNmBins + 2], n22); atomicAdd(&sCells[kNmBins + 3], n30);
  }
  __syncthreads();
  if (threadIdx.x < 2)
    p.partial[((long long)b * p.groups + blockIdx.x) * 2 + threadIdx.x] =
        ((sRed[0][threadIdx.x] + sRed[1][threadIdx.x]) + sRed[2][threadIdx.x]) + sRed[3][threadIdx.x];
  int* cells = p.cells + (long long)b * kNmCells;
  for (int c = threadIdx.x; c < kNmCells; c += 256) {
    const int v = sCells[c];
    if (v) atomicAdd(&cells[c], v);
  }
}

// out[b] = {mean_deg, median_deg, rmse_deg, frac_11_25, frac_22_5, frac_30, n_valid}
constexpr int kBinsPerLane = 8;
static_assert(256 * kBinsPerLane >= kNmBins, "a lane of the finalize kernel owns 8 consecutive bins");

__global__ __launch_bounds__(256) void normal_metrics_finalize_kernel(const double* __restrict__ partial, const int* __restrict__ cells_all,
                                                                      int groups, double* __restrict__ out, int* __restrict__ hist) {
  __shared__ int sScan[2][256];
  __shared__ double sRed[4][2];
  __shared__ int sBin;
  const int b = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int* cells = cells_all + (long long)b * kNmCells;

  // the partials: lane t takes t and t + 256, butterfly, the four waves in order
  double s0 = 0.0, s1 = 0.0;
  const double* pb = partial + (long long)b * groups * 2;
  if (t < groups) { s0 = pb[t * 2]; s1 = pb[t * 2 + 1]; }
  if (t + 256 < groups) { s0 += pb[(t + 256) * 2]; s1 += pb[(t + 256) * 2 + 1]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
  if (lane == 0) { sRed[wave][0] = s0; sRed[wave][1] = s1; }

  // the histogram: 8 consecutive bins per lane, an inclusive scan of the run sums, then the run that holds the median's rank
  int h[kBinsPerLane], run = 0;
#pragma unroll
  for (int j = 0; j < kBinsPerLane; ++j) {
    const int k = t * kBinsPerLane + j;
    h[j] = k < kNmBins ? cells[k] : 0;
    run += h[j];
    if (hist && k < kNmBins) hist[(long long)b * kNmBins + k] = h[j];
  }
  sScan[0][t] = run;
  if (t == 0) sBin = 0;
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < 256; o <<= 1) {                             // Hillis-Steele
    sScan[cur ^ 1][t] = sScan[cur][t] + (t >= o ? sScan[cur][t - o] : 0);
    cur ^= 1;
    __syncthreads();
  }
  const int N = cells[kNmBins];
  const int rank = (N + 1) / 2;
  const int incl = sScan[cur][t];
  int below = incl - run;                                         // the count in the bins before this lane's run
  if (N > 0 && below < rank && rank <= incl) {                    // exactly one lane
    int k = t * kBinsPerLane;
#pragma unroll
    for (int j = 0; j < kBinsPerLane; ++j) {
      if (below + h[j] >= rank) break;
      below += h[j]; ++k;
    }
    sBin = k;
  }
  __syncthreads();
  if (t == 0) {
    double* o = out + (long long)b * kNmOut;
    const double n = (double)N;
    const double sa = ((sRed[0][0] + sRed[1][0]) + sRed[2][0]) + sRed[3][0];
    const double saa = ((sRed[0][1] + sRed[1][1]) + sRed[2][1]) + sRed[3][1];
    const double nan = __builtin_nan("");
    o[0] = N > 0 ? sa / n : nan;
    o[1] = N > 0 ? ((double)sBin + 0.5) * 0.1 : nan;
    o[2] = N > 0 ? sqrt(saa / n) : nan;
    o[3] = N > 0 ? (double)cells[kNmBins + 1] / n : nan;
    o[4] = N > 0 ? (double)cells[kNmBins + 2] / n : nan;
    o[5] = N > 0 ? (double)cells[kNmBins + 3] / n : nan;
    o[6] = n;
  }
}

// workgroups per image, 0 if the arguments make no sense
int nm_groups(int H, int W) {
  if (H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31)) return 0;
  return (int)std::min<long long>((long long)cdiv(H, kTileH) * cdiv(W, kTileW), kNmGroups);
}

size_t nm_partial_bytes(int B, int H, int W) { return (size_t)B * nm_groups(H, W) * 2 * sizeof(double); }

}  // namespace

extern "C" size_t cfp_normal_metrics_ws_bytes(int B, int H, int W) {
  if (B <= 0 || B > 65535 || nm_groups(H, W) == 0) return 0;
  static_assert(kNmCells * sizeof(int) % 8 == 0, "the cells of an image are a whole number of 8-byte words");
  return nm_partial_bytes(B, H, W) + (size_t)B * kNmCells * sizeof(int);
}

extern "C" int cfp_normal_metrics(const float* pred, int Hp, int Wp, const float* gt, int H, int W, int B, int interpolate, float lo,
                                  float hi, const float* K, void* ws, size_t ws_bytes, double* out, int* hist, float* angle_map,
                                  cfp_stream_t stream) {
  CFP_REQUIRE(pred && gt && K && ws && out, CFP_EINVAL, "cfp_normal_metrics: null pointer");
  CFP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0, CFP_ESHAPE, "cfp_normal_metrics: non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) && (long long)Hp * Wp < (1ll << 31) && B <= 65535, CFP_ESHAPE,
              "cfp_normal_metrics: image or batch too large");
  CFP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, "cfp_normal_metrics: sizes differ and interpolate is off");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, "cfp_normal_metrics: empty depth range");
  CFP_REQUIRE(ws_bytes >= cfp_normal_metrics_ws_bytes(B, H, W), CFP_EINVAL, "cfp_normal_metrics: workspace too small");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, CFP_EINVAL, "cfp_normal_metrics: workspace must be 8-byte aligned");
  NormP p;
  p.m = met_params(pred, gt, Hp, Wp, H, W, B, interpolate, 0, lo, hi);
  p.K = K;
  p.partial = reinterpret_cast<double*>(ws);
  p.cells = reinterpret_cast<int*>(static_cast<char*>(ws) + nm_partial_bytes(B, H, W));
  p.angle_map = angle_map;
  p.tiles_x = cdiv(W, kTileW);
  p.tiles = p.tiles_x * cdiv(H, kTileH);
  p.groups = nm_groups(H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  CFP_REQUIRE(hipMemsetAsync(p.cells, 0, (size_t)B * kNmCells * sizeof(int), s) == hipSuccess, CFP_EHIP,
              "cfp_normal_metrics: cannot clear the histograms");
  if (angle_map) hipLaunchKernelGGL(normal_metrics_kernel<true>, dim3(p.groups, B), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(normal_metrics_kernel<false>, dim3(p.groups, B), dim3(256), 0, s, p);
  hipLaunchKernelGGL(normal_metrics_finalize_kernel, dim3(B), dim3(256), 0, s, p.partial, p.cells, p.groups, out, hist);
  return cfp_check_launch("cfp_normal_metrics");
}
