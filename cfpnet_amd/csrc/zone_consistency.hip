// Zone consistency (cfp_tof_zone_consistency): the ToF zones re-simulated from the PREDICTION and compared with what the sensor measured,
// per image, on the device.  The one quality number that needs no ground truth: on a rig the measurement is the sensor itself -- per
// zone a rectangle, a validity bit and the (mu, sigma) of its strongest return (the reference's `raw_data`, src/dataloader/zjuL5.py:106,148).
// The definition is in include/cfpnet_hip.h.
//
//   The depth at a pixel is met_pred of metrics_pred.h in mode 0, the value cfp_eval_metrics evaluates, bit for bit.
//   The sensor model -- the bin of histc, the ambient floor, the strongest run, its float64 moments -- is tof_cluster.h, the code
//   cfp_tof_hist_sim runs: a ground-truth map is perfectly consistent with its own simulation (tests/test_zone_consistency_gpu.py).
//   The argument checks, the walk over a zone's pixels and the zone staging of a tile are zone_core.h, shared with the loss (zone_loss.hip).
//
// Zone kernel.  One workgroup of 256 lanes per (image, zone) walks the zone's pixels (ZoneSweep): equal bins of a wave are merged with a
// ballot before the LDS atomic (a smooth prediction puts a whole zone into two or three bins), and the pixels inside the measured window
// are counted in the same pass (a ballot per wave, one LDS integer add).
// Summary kernel.  One workgroup per image reads the zone table: lane t takes zones t, t + 256, ... in ascending order, a butterfly
// inside the wave, the four waves in order.
// Map kernel (optional).  One lane per pixel of an 8 x 32 tile; only the measured zones that can touch the tile are staged (ZoneStage).
// No workspace, no global atomics, no floating-point atomics: two calls on the same tensors give identical bits.
#include "zone_core.h"

#include <algorithm>

namespace {

constexpr int kZcZone = 6, kZcSum = 10;

struct ZoneP : ZoneArgs { double* zone; double* summary; float* dev_map; };

__global__ __launch_bounds__(kTofThreads) void zone_consistency_kernel(ZoneP p) {
  __shared__ int cnt[kTofMaxBins];
  __shared__ unsigned long long best;
  __shared__ int sWindow;
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.x / p.Z, z = blockIdx.x - b * p.Z;
  const long long o = (long long)b * p.Z + z;

  for (int i = tid; i < p.bins; i += kTofThreads) cnt[i] = 0;
  if (tid == 0) { best = 0ull; sWindow = 0; }
  __syncthreads();

  const ZoneSweep sweep(p, b, z);
  const bool measured = p.mask[o] != 0;
  // the measured window in float64: mu_m -+ max(3 sigma_m, bin_width); a NaN sigma_m leaves bin_width, a NaN mu_m an empty window
  const double mu_m = p.raw[o * 2], s3 = 3.0 * p.raw[o * 2 + 1];
  const double w = s3 > p.bin_width ? s3 : p.bin_width;
  const double wlo = mu_m - w, whi = mu_m + w;

  int n_window = 0;                                   // wave-uniform
  // the window test's operands are captured by value: behind references hipcc keeps the && chain as eight more branches per pass
  sweep.walk(p.m, [&, measured, wlo, whi](float v, bool in) {
    tof_hist_add(cnt, in ? tof_bin(v, p.max_d, p.bins) : -1, lane);
    const double d = (double)v;
    n_window += (int)__popcll(__ballot(in && measured && wlo <= d && d <= whi));
  });
  if (lane == 0 && n_window) atomicAdd(&sWindow, n_window);
  __syncthreads();

  const TofRun run = tof_cluster(cnt, &best, p.bins, p.floor_count, tid);
  if (tid == 0) {
    double mu, sigma;
    tof_moments(cnt, run, p.bin_width, mu, sigma);
    double* zo = p.zone + o * kZcZone;
    zo[0] = mu; zo[1] = sigma; zo[2] = (double)run.n; zo[3] = (double)sweep.npx; zo[4] = (double)sWindow;
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
// A workgroup owns a tile of 8 x 32 pixels and stages the measured zones that can hold a pixel of it (ZoneStage, zone_core.h).
__global__ __launch_bounds__(kZoneChunk) void zone_dev_map_kernel(ZoneP p, int tiles_x) {
  __shared__ ZoneStage st;
  __shared__ float sMu[kZoneChunk];
  const MetP& m = p.m;
  const int t = threadIdx.x;
  const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
  const int ty0 = tyi * kZoneTileH, tx0 = txi * kZoneTileW;
  const int y = ty0 + t / kZoneTileW, x = tx0 + t % kZoneTileW;
  const float fy = (float)y, fx = (float)x;
  // the first and the last pixel of the tile inside the image
  const ZoneTile tile = {(float)ty0, (float)(min(ty0 + kZoneTileH, m.H) - 1), (float)tx0, (float)(min(tx0 + kZoneTileW, m.W) - 1)};
  for (int b = blockIdx.y; b < m.B; b += gridDim.y) {
    bool found = false;
    float mu = 0.f;
    for (int z0 = 0; z0 < p.Z; z0 += kZoneChunk) {
      const int z = z0 + t;
      bool keep = false;
      float r[4] = {0.f, 0.f, 0.f, 0.f}, zm = 0.f;
      if (z < p.Z) {
        const long long o = (long long)b * p.Z + z;
        r[0] = p.rect[o * 4 + 0]; r[1] = p.rect[o * 4 + 1]; r[2] = p.rect[o * 4 + 2]; r[3] = p.rect[o * 4 + 3];
        zm = (float)p.raw[o * 2];
        keep = p.mask[o] != 0 && tile.touches(r);
      }
      int pos;
      const int nz = st.stage(r, keep, pos);
      if (keep) sMu[pos] = zm;
      __syncthreads();
      for (int k = 0; k < nz && !found; ++k) {
        if (st.holds(k, fy, fx)) { found = true; mu = sMu[k]; }
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
  ZoneP p;
  if (const int rc = zone_args(p, "cfp_tof_zone_consistency", pred, Hp, Wp, H, W, B, interpolate, lo, hi, rect, mask, raw, Z, max_distance,
                               bins, bin_width, floor_count)) return rc;
  CFP_REQUIRE((long long)B * Z < (1ll << 31), CFP_ESHAPE, "cfp_tof_zone_consistency: too many zones");
  p.zone = zone; p.summary = summary; p.dev_map = dev_map;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(zone_consistency_kernel, dim3(B * Z), dim3(kTofThreads), 0, s, p);
  hipLaunchKernelGGL(zone_summary_kernel, dim3(B), dim3(256), 0, s, zone, raw, Z, bin_width, summary);
  if (dev_map) {
    const int tiles_x = cdiv(W, kZoneTileW);
    hipLaunchKernelGGL(zone_dev_map_kernel, dim3(tiles_x * cdiv(H, kZoneTileH), std::min(B, 65535)), dim3(kZoneChunk), 0, s, p, tiles_x);
  }
  return cfp_check_launch("cfp_tof_zone_consistency");
}
