// Zone consistency (cfp_tof_zone_consistency): the ToF zones re-simulated from the PREDICTION and compared with what the sensor measured,
// per image, on the device.  The one quality number that needs no ground truth: on a rig the measurement is the sensor itself -- per
// zone a rectangle, a validity bit and the (mu, sigma) of its strongest return (the reference's `raw_data`, src/dataloader/zjuL5.py:106,148).
// The definition is in include/cfpnet_hip.h.
//
//   The depth at a pixel is met_pred of metrics_pred.h in mode 0, the value cfp_eval_metrics evaluates, bit for bit.
//   The sensor model -- the bin of histc, the ambient floor, the strongest run, its float64 moments -- is tof_cluster.h, the code
//   cfp_tof_hist_sim runs: a ground-truth map is perfectly consistent with its own simulation (tests/test_zone_consistency_gpu.py).
//
// Zone kernel.  One workgroup of 256 lanes per (image, zone).  The rectangle is cut to the image once (integer bounds that select the
// pixels of the float rule); the lanes then walk its pixels in passes of 256 x 8: the eight depths of a lane are formed before the first
// bin is computed, equal bins of a wave are merged with a ballot before the LDS atomic (a smooth prediction puts a whole zone into two
// or three bins), and the pixels inside the measured window are counted in the same pass (a ballot per wave, one LDS integer add).
// Summary kernel.  One workgroup per image reads the zone table: lane t takes zones t, t + 256, ... in ascending order, a butterfly
// inside the wave, the four waves in order.
// Map kernel (optional).  One lane per pixel of an 8 x 32 tile; the image's rectangles go through LDS in chunks of 256, so Z is not bounded
// by LDS, and only the measured zones that can touch the tile are staged.
// No workspace, no global atomics, no floating-point atomics: two calls on the same tensors give identical bits.
#include "common.h"
#include "metrics_pred.h"
#include "tof_cluster.h"

#include <algorithm>

namespace {

constexpr int kZcBatch = 8;                           // pixels per lane in flight
constexpr int kZcZone = 6, kZcSum = 10;
constexpr int kZcChunk = 256;                         // rectangles looked at per pass of the map kernel
constexpr int kZcTileH = 8, kZcTileW = 32;           // its tile: one pixel per lane, a wave writes two 128-byte row segments
static_assert(kZcTileH * kZcTileW == kZcChunk && kZcChunk == 256, "one lane per pixel of the tile and per zone of the chunk, four waves");

struct ZoneP {
  MetP m;                                             // pred, Hp, Wp, H, W, interpolate, mode 0, lo, hi, sy, sx
  const float* rect; const unsigned char* mask; const double* raw; int Z;
  float max_d; int bins; double bin_width; int floor_count;
  double* zone; double* summary; float* dev_map;
};

__global__ __launch_bounds__(kTofThreads) void zone_consistency_kernel(ZoneP p) {
  __shared__ int cnt[kTofMaxBins];
  __shared__ unsigned long long best;
  __shared__ int sWindow;
  const MetP& m = p.m;
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.x / p.Z, z = blockIdx.x - b * p.Z;
  const long long o = (long long)b * p.Z + z;
  const float* pb = m.pred + (long long)b * m.Hp * m.Wp;

  for (int i = tid; i < p.bins; i += kTofThreads) cnt[i] = 0;
  if (tid == 0) { best = 0ull; sWindow = 0; }
  __syncthreads();

  int y0, y1, x0, x1;
  zc_span(p.rect[o * 4 + 0], p.rect[o * 4 + 2], m.H, y0, y1);
  zc_span(p.rect[o * 4 + 1], p.rect[o * 4 + 3], m.W, x0, x1);
  const int rw = x1 - x0;
  const int npx = (y1 - y0) * rw;                     // the in-image pixels of the zone; < 2^31 with H * W
  const bool measured = p.mask[o] != 0;
  // the measured window in float64: mu_m -+ max(3 sigma_m, bin_width); a NaN sigma_m leaves bin_width, a NaN mu_m an empty window
  const double mu_m = p.raw[o * 2], s3 = 3.0 * p.raw[o * 2 + 1];
  const double w = s3 > p.bin_width ? s3 : p.bin_width;
  const double wlo = mu_m - w, whi = mu_m + w;

  int n_window = 0;                                   // wave-uniform
  for (int c0 = 0; c0 < npx; c0 += kTofThreads * kZcBatch) {
    // the depths of the batch are formed before the first bin is computed: their loads are in flight together
    float v[kZcBatch];
#pragma unroll
    for (int u = 0; u < kZcBatch; ++u) {
      const int i = min(c0 + u * kTofThreads + tid, npx - 1);
      const int y = i / rw, x = i - y * rw;
      v[u] = met_pred(m, pb, (y0 + y) * m.W + (x0 + x));
    }
#pragma unroll
    for (int u = 0; u < kZcBatch; ++u) {
      const bool in = c0 + u * kTofThreads + tid < npx;
      tof_hist_add(cnt, in ? tof_bin(v[u], p.max_d, p.bins) : -1, lane);
      const double d = (double)v[u];
      n_window += (int)__popcll(__ballot(in && measured && wlo <= d && d <= whi));
    }
  }
  if (lane == 0 && n_window) atomicAdd(&sWindow, n_window);
  __syncthreads();

  const TofRun run = tof_cluster(cnt, &best, p.bins, p.floor_count, tid);
  if (tid == 0) {
    double mu, sigma;
    tof_moments(cnt, run, p.bin_width, mu, sigma);
    double* zo = p.zone + o * kZcZone;
    zo[0] = mu; zo[1] = sigma; zo[2] = (double)run.n; zo[3] = (double)npx; zo[4] = (double)sWindow;
    zo[5] = measured ? (run.n > 0 ? 0.0 : 1.0) : (run.n > 0 ? 2.0 : 3.0);
  }
}

// summary[b] = {n_compared, mae_mu, rmse_mu, rel_mu, mae_sigma, frac_1bin, frac_window, n_lost, n_unmeasured, n_measured}
__global__ __launch_bounds__(256) void zone_summary_kernel(const double* __restrict__ zone, const double* __restrict__ raw, int Z,
                                                           double bin_width, double* __restrict__ summary) {
  __shared__ double sF[4][4];
  __shared__ long long sI[4][7];
  const int b = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  double f[4] = {0.0, 0.0, 0.0, 0.0};                 // sum |dmu|, dmu^2, |dmu| / mu_m, |dsigma| over the compared zones
  long long c[7] = {0, 0, 0, 0, 0, 0, 0};             // compared, within one bin, lost, unmeasured, measured, sum n_window, sum n_pix
  for (int z = t; z < Z; z += 256) {
    const long long o = (long long)b * Z + z;
    const double* zo = zone + o * kZcZone;
    const int state = (int)zo[5];
    if (state == 0) {
      const double mu_m = raw[o * 2], dmu = fabs(zo[0] - mu_m);
      f[0] += dmu; f[1] += dmu * dmu; f[2] += dmu / mu_m; f[3] += fabs(zo[1] - raw[o * 2 + 1]);
      c[0] += 1; c[1] += dmu <= bin_width ? 1 : 0;
    }
    c[2] += state == 1; c[3] += state == 2;
    if (state <= 1) { c[4] += 1; c[5] += (long long)zo[4]; c[6] += (long long)zo[3]; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] += __shfl_xor(f[k], o);
#pragma unroll
    for (int k = 0; k < 7; ++k) c[k] += __shfl_xor(c[k], o);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) sF[wave][k] = f[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) sI[wave][k] = c[k];
  }
  __syncthreads();
  if (t == 0) {
    double F[4]; long long C[7];
    for (int k = 0; k < 4; ++k) F[k] = ((sF[0][k] + sF[1][k]) + sF[2][k]) + sF[3][k];
    for (int k = 0; k < 7; ++k) C[k] = ((sI[0][k] + sI[1][k]) + sI[2][k]) + sI[3][k];
    double* s = summary + (long long)b * kZcSum;
    const double nan = __builtin_nan(""), n = (double)C[0];
    const bool any = C[0] > 0;
    s[0] = n;
    s[1] = any ? F[0] / n : nan;
    s[2] = any ? sqrt(F[1] / n) : nan;
    s[3] = any ? F[2] / n : nan;
    s[4] = any ? F[3] / n : nan;
    s[5] = any ? (double)C[1] / n : nan;
    s[6] = C[6] > 0 ? (double)C[5] / (double)C[6] : nan;
    s[7] = (double)C[2]; s[8] = (double)C[3]; s[9] = (double)C[4];
  }
}

// dev_map[b][y][x] = d - (float)mu_m of the lowest-index measured zone that contains the pixel, NaN where there is none.
// A workgroup owns a tile of 8 x 32 pixels.  Per chunk of 256 zones each lane looks at one zone and keeps it if it is measured and can
// hold a pixel of the tile; the kept ones are compacted into LDS in index order (a ballot per wave, the four wave counts through LDS),
// so the per-pixel loop runs over the few zones that touch the tile and the first hit is still the lowest index.
__global__ __launch_bounds__(kZcChunk) void zone_dev_map_kernel(ZoneP p, int tiles_x) {
  __shared__ float sRect[kZcChunk][4];
  __shared__ float sMu[kZcChunk];
  __shared__ int sKept[kZcChunk / 64];
  const MetP& m = p.m;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
  const int ty0 = tyi * kZcTileH, tx0 = txi * kZcTileW;
  const int y = ty0 + t / kZcTileW, x = tx0 + t % kZcTileW;
  const float fy = (float)y, fx = (float)x;
  // the first and the last pixel of the tile inside the image
  const float ylo = (float)ty0, yhi = (float)(min(ty0 + kZcTileH, m.H) - 1), xlo = (float)tx0, xhi = (float)(min(tx0 + kZcTileW, m.W) - 1);
  for (int b = blockIdx.y; b < m.B; b += gridDim.y) {
    bool found = false;
    float mu = 0.f;
    for (int z0 = 0; z0 < p.Z; z0 += kZcChunk) {
      const int z = z0 + t;
      bool keep = false;
      float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f, zm = 0.f;
      if (z < p.Z) {
        const long long o = (long long)b * p.Z + z;
        r0 = p.rect[o * 4 + 0]; r1 = p.rect[o * 4 + 1]; r2 = p.rect[o * 4 + 2]; r3 = p.rect[o * 4 + 3];
        zm = (float)p.raw[o * 2];
        keep = p.mask[o] != 0 && r0 <= yhi && ylo < r2 && r1 <= xhi && xlo < r3;      // a NaN coordinate: never kept
      }
      const unsigned long long kept = __ballot(keep);
      __syncthreads();                                // the chunk before is read
      if (lane == 0) sKept[wave] = (int)__popcll(kept);
      __syncthreads();
      int pos = (int)__popcll(kept & ((1ull << lane) - 1ull));
      for (int k = 0; k < wave; ++k) pos += sKept[k];
      const int nz = (sKept[0] + sKept[1]) + (sKept[2] + sKept[3]);
      if (keep) { sRect[pos][0] = r0; sRect[pos][1] = r1; sRect[pos][2] = r2; sRect[pos][3] = r3; sMu[pos] = zm; }
      __syncthreads();
      for (int k = 0; k < nz && !found; ++k) {
        if (sRect[k][0] <= fy && fy < sRect[k][2] && sRect[k][1] <= fx && fx < sRect[k][3]) { found = true; mu = sMu[k]; }
      }
    }
    if (y < m.H && x < m.W) {
      const int i = y * m.W + x;
      const float d = met_pred(m, m.pred + (long long)b * m.Hp * m.Wp, i);
      p.dev_map[((long long)b * m.H + y) * m.W + x] = found ? d - mu : __builtin_nanf("");
    }
  }
}

}  // namespace

extern "C" int cfp_tof_zone_consistency(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                                        const float* rect, const unsigned char* mask, const double* raw, int Z, float max_distance,
                                        int bins, double bin_width, int floor_count, double* zone, double* summary, float* dev_map,
                                        cfp_stream_t stream) {
  CFP_REQUIRE(pred && rect && mask && raw && zone && summary, CFP_EINVAL, "cfp_tof_zone_consistency: null pointer");
  CFP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0 && Z > 0, CFP_ESHAPE, "cfp_tof_zone_consistency: non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) && (long long)Hp * Wp < (1ll << 31) && H <= (1 << 24) && W <= (1 << 24), CFP_ESHAPE,
              "cfp_tof_zone_consistency: image too large");
  CFP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, "cfp_tof_zone_consistency: sizes differ and interpolate is off");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, "cfp_tof_zone_consistency: empty depth range");
  CFP_REQUIRE(bins > 0 && bins <= kTofMaxBins, CFP_ESHAPE, "cfp_tof_zone_consistency: bins must be in 1..1024");
  CFP_REQUIRE(max_distance > 0.f && bin_width > 0.0 && floor_count >= 0, CFP_EINVAL, "cfp_tof_zone_consistency: bad histogram parameters");
  CFP_REQUIRE((long long)B * Z < (1ll << 31), CFP_ESHAPE, "cfp_tof_zone_consistency: too many zones");
  ZoneP p;
  MetP& m = p.m;
  m.pred = pred; m.gt = nullptr; m.partial = nullptr; m.out = nullptr;
  m.B = B; m.Hp = Hp; m.Wp = Wp; m.H = H; m.W = W; m.interpolate = interpolate; m.mode = 0; m.lo = lo; m.hi = hi;
  m.sy = H > 1 ? (float)(Hp - 1) / (float)(H - 1) : 0.f;
  m.sx = W > 1 ? (float)(Wp - 1) / (float)(W - 1) : 0.f;
  p.rect = rect; p.mask = mask; p.raw = raw; p.Z = Z;
  p.max_d = max_distance; p.bins = bins; p.bin_width = bin_width; p.floor_count = floor_count;
  p.zone = zone; p.summary = summary; p.dev_map = dev_map;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(zone_consistency_kernel, dim3(B * Z), dim3(kTofThreads), 0, s, p);
  hipLaunchKernelGGL(zone_summary_kernel, dim3(B), dim3(256), 0, s, zone, raw, Z, bin_width, summary);
  if (dev_map) {
    const int tiles_x = cdiv(W, kZcTileW);
    hipLaunchKernelGGL(zone_dev_map_kernel, dim3(tiles_x * cdiv(H, kZcTileH), std::min(B, 65535)), dim3(kZcChunk), 0, s, p, tiles_x);
  }
  return cfp_check_launch("cfp_tof_zone_consistency");
}
