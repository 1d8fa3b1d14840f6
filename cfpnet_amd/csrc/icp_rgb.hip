// Colour in camera tracking: one Gauss-Newton iteration of the joint point-to-plane and photometric ICP (cfp_icp_rgb_step), and the
// luminance planes it reads (cfp_luma).  The definition is in include/cfpnet_hip.h.
//
// Accumulate.  The loop of icp.hip, one thread per pixel of the stride grid; the pair is icp_pair of icp_core.h, bit for bit the one of
// cfp_icp_step.  A pixel that has a geometric pair blends the model's luminance at its UNROUNDED projection (four taps, issued without a
// branch like the other gathers, at the map's first pixel where the cell leaves it), compares it with the frame's own luminance and adds
// 30 more products: the second half of a row of 60 doubles.  Sixty double accumulators are 120 VGPRs of a thread; with 256 threads per
// workgroup the register file leaves each thread 512, and the kernel holds no scratch (DESIGN 4.33 has the numbers).
//
// Finalize.  One 64-lane workgroup per image sums the rows, the geometric 30 and the photometric 30 one after the other (icp_sum_rows);
// lane 0 adds the two systems in double and takes the step of icp.hip on the sum (icp_update_pose).  No atomics anywhere.
#include "common.h"
#include "icp_core.h"
#include "metrics_pred.h"

namespace {

using namespace icp_core;

constexpr int kRgbTerms = 2 * kIcpTerms;              // a workspace row: the 30 of the geometric pairs, then the 30 of the photometric

struct IcpRgbP {
  IcpP g;
  const float* src_luma; const float* mdl_luma;
  float photo_weight, photo_max;
  float* residual;
};

template <int PI, int SI>
__global__ __launch_bounds__(256) void icp_rgb_accumulate_kernel(IcpRgbP pp) {
  __shared__ double red[4][kRgbTerms];
  const IcpP& p = pp.g;
  MetP m = p.m, su = p.u;
  m.interpolate = PI; m.mode = 0; su.interpolate = SI == 2 ? 1 : 0;
  su.H = m.H; su.W = m.W;
  const int b = blockIdx.y;
  const IcpImg g = icp_image<SI>(p, m, b);
  int* ib = p.index ? p.index + (long long)b * m.H * m.W : nullptr;
  float* rb = pp.residual ? pp.residual + (long long)b * m.H * m.W : nullptr;
  const float* sl = pp.src_luma + (long long)b * m.H * m.W;
  const float* ml = pp.mdl_luma + (long long)b * p.Hm * p.Wm;
  const float wI = pp.photo_weight, photo_max = pp.photo_max;
  __shared__ float cam[24];
  IcpCam c;
  icp_load_cam(p, b, cam, c);
  double acc[kRgbTerms];
#pragma unroll
  for (int k = 0; k < kRgbTerms; ++k) acc[k] = 0.0;
  const unsigned n = (unsigned)p.ws * (unsigned)p.hs;              // < 2^31
  for (long long i64 = (long long)blockIdx.x * 256 + threadIdx.x; i64 < n; i64 += (long long)gridDim.x * 256) {
    IcpPair q;
    icp_pair(p, m, su, c, g, (unsigned)i64, q);
    // the photometric pair: the cell of the unrounded projection, tested on the float values (NaN fails); where it fails all four taps
    // read the map's first pixel, so no load leaves the map whatever its size
    const float x0 = floorf(q.u), y0 = floorf(q.v);
    const float ax = q.u - x0, ay = q.v - y0;
    bool pok = q.mi >= 0 && x0 >= 0.f && x0 + 1.f <= (float)(p.Wm - 1) && y0 >= 0.f && y0 + 1.f <= (float)(p.Hm - 1);
    const int t0 = pok ? (int)y0 * p.Wm + (int)x0 : 0, dx = pok ? 1 : 0, dy = pok ? p.Wm : 0;
    const float I00 = ml[t0], I10 = ml[t0 + dx], I01 = ml[t0 + dy], I11 = ml[t0 + dy + dx];
    const float Is = sl[q.pix];
    pok = pok && finitef(I00) && finitef(I10) && finitef(I01) && finitef(I11) && finitef(Is);
    const float top = I00 + ax * (I10 - I00);
    const float bot = I01 + ax * (I11 - I01);
    const float Im = top + ay * (bot - top);
    const float gx = (I10 - I00) + ay * ((I11 - I01) - (I10 - I00));
    const float gy = bot - top;
    const float rI = Im - Is;
    pok = pok && fabsf(rI) <= photo_max;                            // false for NaN
    if (ib) icp_write_cell(ib, p, m, q, q.mi, -1);
    if (rb) icp_write_cell(rb, p, m, q, pok ? rI : NAN, NAN);
    if (q.mi < 0) continue;
    icp_add_terms(acc, q.w, q.J, q.r);
    if (!pok) continue;
    const float gfx = gx * c.fxm, gfy = gy * c.fym;
    const float a0 = gfx / q.Zp, a1 = gfy / q.Zp;
    const float a2 = -((gfx * (q.Xp / q.Zp) + gfy * (q.Yp / q.Zp)) / q.Zp);
    const float JI[6] = {q.Yp * a2 - q.Zp * a1, q.Zp * a0 - q.Xp * a2, q.Xp * a1 - q.Yp * a0, a0, a1, a2};
    icp_add_terms(acc + kIcpTerms, wI, JI, rI);
  }
  icp_block_reduce<kRgbTerms>(acc, red, p.partial + ((long long)b * gridDim.x + blockIdx.x) * kRgbTerms);
}

__global__ __launch_bounds__(64) void icp_rgb_finalize_kernel(IcpF p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int r0 = min(lane, p.nblocks - 1), r1 = min(lane + 64, p.nblocks - 1);
  const double* q0 = p.partial + ((long long)b * p.nblocks + r0) * kRgbTerms;
  const double* q1 = p.partial + ((long long)b * p.nblocks + r1) * kRgbTerms;
  double s[kRgbTerms];
  icp_sum_rows(q0, q1, lane, p.nblocks, s);
  icp_sum_rows(q0 + kIcpTerms, q1 + kIcpTerms, lane, p.nblocks, s + kIcpTerms);
  if (lane != 0) return;
  if (p.sums) {
#pragma unroll
    for (int k = 0; k < kRgbTerms; ++k) p.sums[b * 64 + k] = s[k];
#pragma unroll
    for (int k = kRgbTerms; k < 64; ++k) p.sums[b * 64 + k] = 0.0;
  }
  double sys[27];                                     // A = A_geo + A_photo, g = g_geo + g_photo
#pragma unroll
  for (int k = 0; k < 27; ++k) sys[k] = s[k] + s[kIcpTerms + k];
  double wn, vn;
  const bool accepted = icp_update_pose(sys, s[29] >= (double)p.min_pairs, p.min_pivot, p.T + b * 12, p.T_ref ? p.T_ref + b * 12 : nullptr,
                                        p.T_world ? p.T_world + b * 12 : nullptr, wn, vn);
  float* st = p.stats + b * 8;
  icp_write_stats(st, s, wn, vn, accepted);
  st[6] = (float)s[59];
  st[7] = s[59] > 0.0 ? sqrtf((float)(s[57] / s[58])) : NAN;
}

struct LumaP {
  const float* rgb; float* out;
  long long hw, n;                                    // pixels of an image, of the batch
  float mean[3], cstd[3];
};

struct Rgb3 { float r, g, b; };                       // 12 bytes, 4-byte aligned: one three-dword load

// LAYOUT 0: planar [B,3,H,W], c = rgb * std + mean; 1: interleaved [B,H,W,3], c = rgb.  One pixel per lane.
template <int LAYOUT>
__global__ __launch_bounds__(256) void luma_kernel(LumaP p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  float R, G, B;
  if (LAYOUT == 0) {
    const long long b = i / p.hw, o = i - b * p.hw;
    const float* q = p.rgb + b * 3 * p.hw + o;
    R = q[0] * p.cstd[0] + p.mean[0]; G = q[p.hw] * p.cstd[1] + p.mean[1]; B = q[2 * p.hw] * p.cstd[2] + p.mean[2];
  } else {
    const Rgb3 v = reinterpret_cast<const Rgb3*>(p.rgb)[i];
    R = v.r; G = v.g; B = v.b;
  }
  const float Y = (0.299f * R + 0.587f * G) + 0.114f * B;
  p.out[i] = finitef(R) && finitef(G) && finitef(B) ? Y : NAN;
}

}  // namespace

extern "C" int cfp_luma(const float* rgb, int layout, const float* mean, const float* cstd, int H, int W, int B, float* luma,
                        cfp_stream_t stream) {
  CFP_REQUIRE(rgb && luma, CFP_EINVAL, "cfp_luma: null pointer");
  CFP_REQUIRE(layout == 0 || layout == 1, CFP_EINVAL, "cfp_luma: layout must be 0 (planar, normalised) or 1 (interleaved, 0..1)");
  CFP_REQUIRE(layout == 1 || (mean && cstd), CFP_EINVAL, "cfp_luma: the planar layout needs mean and std");
  CFP_REQUIRE(B > 0 && H > 0 && W > 0, CFP_ESHAPE, "cfp_luma: non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) && B <= 65535, CFP_ESHAPE, "cfp_luma: image or batch too large");
  LumaP p;
  p.rgb = rgb; p.out = luma;
  p.hw = (long long)H * W; p.n = p.hw * B;
  for (int k = 0; k < 3; ++k) {
    p.mean[k] = layout == 0 ? mean[k] : 0.f; p.cstd[k] = layout == 0 ? cstd[k] : 1.f;
    CFP_REQUIRE(std::isfinite(p.mean[k]) && std::isfinite(p.cstd[k]), CFP_EINVAL, "cfp_luma: mean and std must be finite");
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((p.n + 255) / 256));     // < 2^31 * 65535 / 256 < 2^39: checked against the grid limit below
  CFP_REQUIRE((p.n + 255) / 256 < (1ll << 31), CFP_ESHAPE, "cfp_luma: image or batch too large");
  if (layout == 0) hipLaunchKernelGGL(luma_kernel<0>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(luma_kernel<1>, grid, dim3(256), 0, s, p);
  return cfp_check_launch("cfp_luma");
}

extern "C" size_t cfp_icp_rgb_ws_bytes(int B, int H, int W, int stride) {
  if (B <= 0 || H <= 0 || W <= 0 || stride < 1) return 0;
  return (size_t)B * icp_blocks(H, W, stride) * kRgbTerms * sizeof(double);
}

extern "C" int cfp_icp_rgb_step(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                                const float* std, int Hu, int Wu, long long std_stride, float std_floor, const float* src_normals,
                                float cos_min, const float* K_src, const float* mdl_depth, const float* mdl_normals, const float* mdl_std,
                                int Hm, int Wm, const float* K_mdl, int stride, float z_near, float dist_max, int min_pairs,
                                float min_pivot, float* T, const float* T_ref, float* T_world, int* index, double* sums, float* stats,
                                void* ws, size_t ws_bytes, const float* src_luma, const float* mdl_luma, float photo_weight,
                                float photo_max, float* residual, cfp_stream_t stream) {
  const int rc = icp_check("cfp_icp_rgb_step", pred, Hp, Wp, H, W, B, interpolate, lo, hi, std, Hu, Wu, std_stride, std_floor, cos_min,
                           K_src, mdl_depth, mdl_normals, Hm, Wm, K_mdl, stride, z_near, dist_max, min_pairs, min_pivot, T, T_ref, T_world,
                           sums, stats, ws, ws_bytes, kRgbTerms);
  if (rc != CFP_OK) return rc;
  CFP_REQUIRE((src_luma != nullptr) == (mdl_luma != nullptr), CFP_EINVAL,
              "cfp_icp_rgb_step: src_luma and mdl_luma are given together or not at all");
  CFP_REQUIRE(src_luma, CFP_EINVAL, "cfp_icp_rgb_step: no luminance planes: cfp_icp_step is the entry that tracks without an image");
  CFP_REQUIRE(pos_finite(photo_weight), CFP_EINVAL, "cfp_icp_rgb_step: photo_weight must be positive and finite");
  CFP_REQUIRE(photo_max > 0.f, CFP_EINVAL, "cfp_icp_rgb_step: photo_max must be positive (it may be infinite)");
  IcpRgbP p;
  IcpF f;
  icp_fill(p.g, f, pred, Hp, Wp, H, W, B, interpolate, lo, hi, std, Hu, Wu, std_stride, std_floor, src_normals, cos_min, K_src, mdl_depth,
           mdl_normals, mdl_std, Hm, Wm, K_mdl, stride, z_near, dist_max, min_pairs, min_pivot, T, T_ref, T_world, index, sums, stats, ws);
  p.src_luma = src_luma; p.mdl_luma = mdl_luma;
  p.photo_weight = photo_weight; p.photo_max = photo_max;
  p.residual = residual;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)f.nblocks, B);
  const int si = !std ? 0 : (p.g.u.interpolate ? 2 : 1);
#define CFP_ICP_LAUNCH(PI, SI) hipLaunchKernelGGL((icp_rgb_accumulate_kernel<PI, SI>), grid, dim3(256), 0, s, p)
  if (interpolate) {
    if (si == 0) CFP_ICP_LAUNCH(1, 0); else if (si == 1) CFP_ICP_LAUNCH(1, 1); else CFP_ICP_LAUNCH(1, 2);
  } else {
    if (si == 0) CFP_ICP_LAUNCH(0, 0); else if (si == 1) CFP_ICP_LAUNCH(0, 1); else CFP_ICP_LAUNCH(0, 2);
  }
#undef CFP_ICP_LAUNCH
  hipLaunchKernelGGL(icp_rgb_finalize_kernel, dim3(B), dim3(64), 0, s, f);
  return cfp_check_launch("cfp_icp_rgb_step");
}
