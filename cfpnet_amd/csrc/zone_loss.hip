// Zone-consistency loss (cfp_tof_zone_loss): the ToF zones re-simulated from the PREDICTION, their mean depth compared with the measured
// mu, as a training objective with a gradient on the prediction -- the term that needs no ground truth.  The definition is in
// include/cfpnet_hip.h.
//
//   Everything up to the strongest run is the metric's (zone_consistency.hip), bit for bit, because it is the same code: the argument
//   checks, the walk over a zone's pixels (met_pred of metrics_pred.h in mode 0 on the pixels of zc_span) and the zone staging of a tile
//   are zone_core.h; the histogram, the floor and the run are tof_cluster.h.
//
// Zone kernel.  One workgroup of 256 lanes per (image, zone).  First sweep: the histogram, as the metric builds it.  The raw counts are
// copied beside it in LDS before tof_cluster floors them, so that omega_j = c'_j / cnt_j exists for the bins of the run.  Second sweep over the
// same pixels (the depths are formed again: the same float32 bits): sum omega_bin(d) * d in float64 -- per lane in pixel order, a butterfly
// inside the wave, the four waves in order.  It writes m_z, n_z, the run and the state to the zone table and omega_j / n_z for every bin
// (0 outside the run) to the workspace.
// Image kernel.  ONE workgroup; wave w takes images w, w + 4, ...: lane t takes zones t, t + 64, ... in ascending order, a butterfly, then
// lane 0 has n_b and L_b.  A second pass writes r_z, rho_z and coef_z = s * min(e_z / delta, 1) * sgn(r_z) / (B * n_b).  After a barrier
// thread 0 sums the L_b in index order: L needs no atomic and no further launch.
// Backward kernel (skipped when grad_pred is null).  A gather over the pred grid, one lane per pixel of an 8 x 32 tile.  Only the zones
// with coef != 0 that can touch the tile's footprint are staged (ZoneStage).  A lane walks the pixels of the H x W grid whose bilinear
// footprint holds its pred pixel (as silog_bwd_kernel does), forms each one's depth and bin once it lies in a kept zone, and adds
// w_y * w_x * coef_z * omega_bin / n_z  in float64; one rounding to float32 at the end, times the derivative of the clip.
// No global atomics, no floating-point atomics (integer LDS atomics only): two calls on the same tensors give identical bits.
#include "zone_core.h"

#include <algorithm>

namespace {

constexpr int kZlZone = 8;                            // {m_z, n_z, r_z, rho_z, run_start, run_stop, state, coef}

struct ZoneLossP : ZoneArgs {
  double delta; float grad_scale; int accumulate;
  double* table;                                      // workspace [B][Z][bins]: omega_j / n_z
  double* zone; float* out; float* grad_pred;
};

__global__ __launch_bounds__(kTofThreads) void zone_loss_zone_kernel(ZoneLossP p) {
  __shared__ int cnt[kTofMaxBins];
  __shared__ int rawc[kTofMaxBins];
  __shared__ unsigned long long best;
  __shared__ double sAcc[kTofThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / p.Z, z = blockIdx.x - b * p.Z;
  const long long o = (long long)b * p.Z + z;

  for (int i = tid; i < p.bins; i += kTofThreads) cnt[i] = 0;
  if (tid == 0) best = 0ull;
  __syncthreads();

  const ZoneSweep sweep(p, b, z);
  sweep.walk(p.m, [&](float v, bool in) { tof_hist_add(cnt, in ? tof_bin(v, p.max_d, p.bins) : -1, lane); });
  __syncthreads();
  for (int i = tid; i < p.bins; i += kTofThreads) rawc[i] = cnt[i];       // the bins this lane reads first in tof_cluster

  const TofRun run = tof_cluster(cnt, &best, p.bins, p.floor_count, tid);  // cnt: the counts after the floor, visible to every lane

  // second sweep: sum omega_bin(d) * d over the pixels whose bin lies in the run
  double acc = 0.0;
  if (run.n > 0) {
    sweep.walk(p.m, [&](float v, bool in) {
      const int bin = in ? tof_bin(v, p.max_d, p.bins) : -1;
      if (bin >= run.start && bin < run.stop) acc += ((double)cnt[bin] / (double)rawc[bin]) * (double)v;
    });
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
  if (lane == 0) sAcc[wave] = acc;

  // omega_j / n_z for every bin of the zone: the backward reads it at the bin of a pixel
  double* tab = p.table + o * (long long)p.bins;
  const double nz = (double)run.n;
  for (int j = tid; j < p.bins; j += kTofThreads)
    tab[j] = (j >= run.start && j < run.stop) ? ((double)cnt[j] / (double)rawc[j]) / nz : 0.0;
  __syncthreads();

  if (tid == 0) {
    const double sum = ((sAcc[0] + sAcc[1]) + sAcc[2]) + sAcc[3];
    const bool measured = p.mask[o] != 0;
    double* zo = p.zone + o * kZlZone;
    zo[0] = run.n > 0 ? sum / nz : 0.0;
    zo[1] = nz;
    zo[4] = (double)run.start; zo[5] = (double)run.stop;
    zo[6] = measured ? (run.n > 0 ? 0.0 : 1.0) : (run.n > 0 ? 2.0 : 3.0);
    // r_z, rho_z and coef (zo[2], zo[3], zo[7]) are the image kernel's
  }
}

// compared: measured, a return in the prediction, and a finite measured mu
__device__ __forceinline__ bool zl_compared(const double* zo, double mu_m) {
  return zo[6] == 0.0 && mu_m - mu_m == 0.0;
}

__global__ __launch_bounds__(256) void zone_loss_image_kernel(ZoneLossP p) {
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int B = p.m.B, Z = p.Z;
  const double half = p.bin_width / 2.0, delta = p.delta;
  for (int b = wave; b < B; b += 4) {
    double sum = 0.0;
    int n = 0;
    for (int z = lane; z < Z; z += 64) {
      const long long o = (long long)b * Z + z;
      const double* zo = p.zone + o * kZlZone;
      const double mu_m = p.raw[o * 2];
      if (zl_compared(zo, mu_m)) {
        const double e = fmax(fabs(zo[0] - mu_m) - half, 0.0);
        sum += e <= delta ? e * e / (2.0 * delta) : e - delta / 2.0;
        n += 1;
      }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { sum += __shfl_xor(sum, s); n += __shfl_xor(n, s); }
    const double Lb = n > 0 ? sum / (double)n : 0.0;
    if (lane == 0) p.out[1 + b] = (float)Lb;
    const double k = n > 0 ? (double)p.grad_scale / ((double)B * (double)n) : 0.0;
    for (int z = lane; z < Z; z += 64) {
      const long long o = (long long)b * Z + z;
      double* zo = p.zone + o * kZlZone;
      const double mu_m = p.raw[o * 2];
      double r = __builtin_nan(""), rho = 0.0, coef = 0.0;
      if (zl_compared(zo, mu_m)) {
        r = zo[0] - mu_m;
        const double e = fmax(fabs(r) - half, 0.0);
        rho = e <= delta ? e * e / (2.0 * delta) : e - delta / 2.0;
        coef = k * fmin(e / delta, 1.0) * (r > 0.0 ? 1.0 : -1.0);
        if (e == 0.0) coef = 0.0;
      }
      zo[2] = r; zo[3] = rho; zo[7] = coef;
    }
  }
  __syncthreads();                                     // the L_b this workgroup wrote are visible to it
  if (t == 0) {
    double L = 0.0;                                    // the float32 L_b the caller sees, summed in index order in float64
    for (int b = 0; b < B; ++b) L += (double)p.out[1 + b];
    p.out[0] = (float)(L / (double)B);
  }
}

// The rows Y of the H grid whose source coordinate s * Y lies within one row of [a, b] on the pred grid: a superset, as silog_bwd_kernel's.
__device__ __forceinline__ void zl_footprint(float s, int a, int b, int n, int& lo, int& hi) {
  lo = s > 0.f ? max(0, (int)ceilf(((float)a - 1.f) / s) - 1) : 0;
  hi = s > 0.f ? min(n - 1, (int)floorf(((float)b + 1.f) / s) + 1) : n - 1;
}

__global__ __launch_bounds__(kZoneChunk) void zone_loss_bwd_kernel(ZoneLossP p, int tiles_x) {
  __shared__ ZoneStage st;
  __shared__ double sCoef[kZoneChunk];
  __shared__ int sIdx[kZoneChunk];
  const MetP& m = p.m;
  const int t = threadIdx.x;
  const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
  const int ty0 = tyi * kZoneTileH, tx0 = txi * kZoneTileW;
  const int ty1 = min(ty0 + kZoneTileH, m.Hp) - 1, tx1 = min(tx0 + kZoneTileW, m.Wp) - 1;  // the last pixel of the tile inside pred
  const int y = ty0 + t / kZoneTileW, x = tx0 + t % kZoneTileW;
  const bool live = y < m.Hp && x < m.Wp;
  // the pixels of the H x W grid that can hold a pixel of the tile / this lane's pixel in their footprint
  int TY0 = ty0, TY1 = ty1, TX0 = tx0, TX1 = tx1, Y0 = y, Y1 = y, X0 = x, X1 = x;
  if (m.interpolate) {
    zl_footprint(m.sy, ty0, ty1, m.H, TY0, TY1); zl_footprint(m.sx, tx0, tx1, m.W, TX0, TX1);
    zl_footprint(m.sy, y, y, m.H, Y0, Y1); zl_footprint(m.sx, x, x, m.W, X0, X1);
  }
  const ZoneTile tile = {(float)TY0, (float)TY1, (float)TX0, (float)TX1};
  for (int b = blockIdx.y; b < m.B; b += gridDim.y) {
    const float* pb = m.pred + (long long)b * m.Hp * m.Wp;
    double acc = 0.0;
    for (int z0 = 0; z0 < p.Z; z0 += kZoneChunk) {
      const int z = z0 + t;
      bool keep = false;
      float r[4] = {0.f, 0.f, 0.f, 0.f};
      double coef = 0.0;
      if (z < p.Z) {
        const long long o = (long long)b * p.Z + z;
        r[0] = p.rect[o * 4 + 0]; r[1] = p.rect[o * 4 + 1]; r[2] = p.rect[o * 4 + 2]; r[3] = p.rect[o * 4 + 3];
        coef = p.zone[o * kZlZone + 7];
        keep = coef != 0.0 && tile.touches(r);
      }
      int pos;
      const int nz = st.stage(r, keep, pos);
      if (keep) { sCoef[pos] = coef; sIdx[pos] = z; }
      __syncthreads();
      if (!live || nz == 0) continue;                 // nz is the same in every lane; a lane off the image takes part in the barriers only
      for (int Y = Y0; Y <= Y1; ++Y) {
        float wy = 1.f;
        if (m.interpolate) {
          const float fy = m.sy * (float)Y;
          const int s0 = min((int)fy, m.Hp - 1), s1 = m.Hp == m.H ? s0 : min(s0 + 1, m.Hp - 1);
          const float ly = fy - (float)s0;
          wy = 0.f;                                   // both taps can land on the same row
          if (y == s0) wy += 1.f - ly;
          if (y == s1) wy += ly;
          if (wy == 0.f) continue;
        }
        const float fY = (float)Y;
        for (int X = X0; X <= X1; ++X) {
          float wx = 1.f;
          if (m.interpolate) {
            const float fx = m.sx * (float)X;
            const int s0 = min((int)fx, m.Wp - 1), s1 = m.Wp == m.W ? s0 : min(s0 + 1, m.Wp - 1);
            const float lx = fx - (float)s0;
            wx = 0.f;
            if (x == s0) wx += 1.f - lx;
            if (x == s1) wx += lx;
            if (wx == 0.f) continue;
          }
          const float fX = (float)X;
          int bin = -2;                               // -2: the depth of (Y, X) is not formed yet
          double g = 0.0;
          for (int k = 0; k < nz; ++k) {
            if (st.holds(k, fY, fX)) {
              if (bin == -2) bin = tof_bin(met_pred(m, pb, Y * m.W + X), p.max_d, p.bins);
              if (bin < 0) break;                     // a NaN or out-of-range depth has no bin and no gradient
              g += sCoef[k] * p.table[((long long)b * p.Z + sIdx[k]) * p.bins + bin];
            }
          }
          acc += ((double)wy * (double)wx) * g;
        }
      }
    }
    if (live) {
      const long long i = ((long long)b * m.Hp + y) * m.Wp + x;
      const float pv = pb[y * m.Wp + x];
      const float g = (pv >= m.lo && pv <= m.hi) ? (float)acc : 0.f;      // the derivative of the clip, closed interval; NaN and Inf: 0
      p.grad_pred[i] = p.accumulate ? p.grad_pred[i] + g : g;
    }
  }
}

}  // namespace

extern "C" size_t cfp_tof_zone_loss_ws_bytes(int B, int Z, int bins) {
  if (B <= 0 || Z <= 0 || bins <= 0 || bins > kTofMaxBins || (long long)B * Z >= (1ll << 31)) return 0;
  return (size_t)B * Z * bins * sizeof(double);
}

extern "C" int cfp_tof_zone_loss(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                                 const float* rect, const unsigned char* mask, const double* raw, int Z, float max_distance, int bins,
                                 double bin_width, int floor_count, double delta, float grad_scale, int accumulate, void* ws,
                                 size_t ws_bytes, double* zone, float* out, float* grad_pred, cfp_stream_t stream) {
  CFP_REQUIRE(pred && rect && mask && raw && ws && zone && out, CFP_EINVAL, "cfp_tof_zone_loss: null pointer");
  ZoneLossP p;
  if (const int rc = zone_args(p, "cfp_tof_zone_loss", pred, Hp, Wp, H, W, B, interpolate, lo, hi, rect, mask, raw, Z, max_distance, bins,
                               bin_width, floor_count)) return rc;
  CFP_REQUIRE(delta > 0.0 && delta - delta == 0.0, CFP_EINVAL, "cfp_tof_zone_loss: delta must be positive and finite");
  CFP_REQUIRE(accumulate == 0 || accumulate == 1, CFP_EINVAL, "cfp_tof_zone_loss: accumulate must be 0 or 1");
  CFP_REQUIRE((long long)B * Z < (1ll << 31), CFP_ESHAPE, "cfp_tof_zone_loss: too many zones");
  CFP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, CFP_EINVAL, "cfp_tof_zone_loss: workspace must be 16-byte aligned");
  CFP_REQUIRE(ws_bytes >= cfp_tof_zone_loss_ws_bytes(B, Z, bins), CFP_EINVAL, "cfp_tof_zone_loss: workspace too small");
  p.delta = delta; p.grad_scale = grad_scale; p.accumulate = accumulate;
  p.table = reinterpret_cast<double*>(ws); p.zone = zone; p.out = out; p.grad_pred = grad_pred;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(zone_loss_zone_kernel, dim3(B * Z), dim3(kTofThreads), 0, s, p);
  hipLaunchKernelGGL(zone_loss_image_kernel, dim3(1), dim3(256), 0, s, p);
  if (grad_pred) {
    const int tiles_x = cdiv(Wp, kZoneTileW);
    hipLaunchKernelGGL(zone_loss_bwd_kernel, dim3(tiles_x * cdiv(Hp, kZoneTileH), std::min(B, 65535)), dim3(kZoneChunk), 0, s, p, tiles_x);
  }
  return cfp_check_launch("cfp_tof_zone_loss");
}
