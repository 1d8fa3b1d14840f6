// The prediction a depth-evaluation kernel sees at a ground-truth pixel: the clip / bilinear order of the two reference protocols
// (metrics.hip header).  Shared by metrics.hip (the nine depth metrics) and unc_metrics.hip (sparsification curves), so both evaluate the
// same float32 value bit for bit.
#pragma once
#include "common.h"

namespace {

struct MetP {
  const float* pred; const float* gt; double* partial; double* out;
  int B, Hp, Wp, H, W, interpolate, mode;
  float lo, hi, sy, sx;
};

// The block of a B x Hp x Wp prediction seen on the H x W grid, with the align-corners scales every kernel here uses; `partial` and `out`
// are null: the caller that uses them sets them afterwards.
inline MetP met_params(const float* pred, const float* gt, int Hp, int Wp, int H, int W, int B, int interpolate, int mode, float lo,
                       float hi) {
  MetP p;
  p.pred = pred; p.gt = gt; p.partial = nullptr; p.out = nullptr;
  p.B = B; p.Hp = Hp; p.Wp = Wp; p.H = H; p.W = W; p.interpolate = interpolate; p.mode = mode; p.lo = lo; p.hi = hi;
  p.sy = H > 1 ? (float)(Hp - 1) / (float)(H - 1) : 0.f;
  p.sx = W > 1 ? (float)(Wp - 1) / (float)(W - 1) : 0.f;
  return p;
}

__device__ __forceinline__ float clipf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // NaN passes, like np.clip

__device__ __forceinline__ float met_pred(const MetP& p, const float* __restrict__ pb, int i) {
  float v;
  if (p.interpolate) {
    const int y = i / p.W, x = i - y * p.W;
    const float fy = p.sy * (float)y, fx = p.sx * (float)x;
    const int y0 = min((int)fy, p.Hp - 1), x0 = min((int)fx, p.Wp - 1);
    // ATen (UpSample.h compute_source_index_and_lambda): a dimension whose size does not change reads the SAME
    // pixel twice with weights (1, 0), so a non-finite value turns into NaN there and does not touch its neighbours
    const int y1 = p.Hp == p.H ? y0 : min(y0 + 1, p.Hp - 1), x1 = p.Wp == p.W ? x0 : min(x0 + 1, p.Wp - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    float t00 = pb[y0 * p.Wp + x0], t01 = pb[y0 * p.Wp + x1], t10 = pb[y1 * p.Wp + x0], t11 = pb[y1 * p.Wp + x1];
    if (p.mode == 0) { t00 = clipf(t00, p.lo, p.hi); t01 = clipf(t01, p.lo, p.hi); t10 = clipf(t10, p.lo, p.hi); t11 = clipf(t11, p.lo, p.hi); }
    v = hy * (hx * t00 + lx * t01) + ly * (hx * t10 + lx * t11);
  } else {
    v = pb[i];
    if (p.mode == 0) v = clipf(v, p.lo, p.hi);
  }
  if (p.mode == 1) {
    v = clipf(v, p.lo, p.hi);
    if (v != v) v = p.lo;
  }
  return v;
}

// A map that travels with the prediction (an uncertainty plane), brought to the ground-truth grid with the same align-corners taps and
// float32 blend as met_pred, without clip or nan handling; read directly when nothing is interpolated.
__device__ __forceinline__ float met_plane(const MetP& p, const float* __restrict__ pb, int i) {
  if (!p.interpolate) return pb[i];
  const int y = i / p.W, x = i - y * p.W;
  const float fy = p.sy * (float)y, fx = p.sx * (float)x;
  const int y0 = min((int)fy, p.Hp - 1), x0 = min((int)fx, p.Wp - 1);
  const int y1 = p.Hp == p.H ? y0 : min(y0 + 1, p.Hp - 1), x1 = p.Wp == p.W ? x0 : min(x0 + 1, p.Wp - 1);
  const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
  const float t00 = pb[y0 * p.Wp + x0], t01 = pb[y0 * p.Wp + x1], t10 = pb[y1 * p.Wp + x0], t11 = pb[y1 * p.Wp + x1];
  return hy * (hx * t00 + lx * t01) + ly * (hx * t10 + lx * t11);
}

}  // namespace
