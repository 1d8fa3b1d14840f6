// A world-anchored map on the device: a truncated signed distance field whose per-voxel weight is the inverse-variance sum that
// cfp_depth_fuse keeps per pixel (cfp_tsdf_integrate), and the raycast that turns the volume back into depth, normals and std in any
// view (cfp_tsdf_raycast).  The definitions are in include/cfpnet_hip.h; the depth at a pixel is met_pred of metrics_pred.h in mode 0,
// the value cfp_depth_unproject back-projects, bit for bit, and the std that travels with it is met_plane.
//
// Integrate.  One thread per voxel, x along the lanes, so the (F, Wt) pairs of a wave are 512 contiguous bytes read and written once as
// float2.  A voxel projects into the image and reads one depth (and one std): neighbouring voxels read neighbouring pixels, the taps
// are gathers that stay in L2.  The grid is capped and strided; the three counts are summed per thread over its voxels, per workgroup
// through LDS in a fixed tree, and leave as one INTEGER atomic add per workgroup and count onto a word a first launch has zeroed -- an
// integer sum does not depend on the order of arrival, so two launches give identical bits.
//
// Integrate with colour (cfp_tsdf_integrate_rgb) is the same kernel with COLOR = true: a voxel the geometry step has updated and that lies
// within trunc of the surface reads the three planes of the image at the pixel its depth came from and folds them into its (R, G, B, Wc)
// entry of the colour volume -- one 16-byte load and one 16-byte store, 1 KB contiguous per wave -- and a fourth count joins the three.
// The COLOR = false instance is the kernel cfp_tsdf_integrate has always launched.
//
// Raycast.  A workgroup owns a 16 x 16 pixel tile (a wave four rows of 16), so that neighbouring rays walk through the same cells and
// their 8-corner gathers hit the same lines.  Every sample reads its corners as float2 (F, Wt).  The march may skip the part of the ray
// that cannot touch the volume's box; the skipped samples are ones the per-sample test would call invalid anyway.
#include "common.h"
#include "metrics_pred.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kMaxBlocks = 2048;                      // workgroups per image of the integrate kernel; the voxels beyond are grid-strided
constexpr long long kMaxDim = 1ll << 24;              // a row, column, voxel or step index is used as a float: exact below 2^24
constexpr int kTile = 16;                             // the raycast's pixel tile

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }      // false for NaN

struct IntegrateP {
  MetP m;                                             // the depth: pred, Hp, Wp, H, W, interpolate, mode 0, lo, hi
  MetP u;                                             // the std plane as met_plane reads it (pred = null: every observation weighs 1)
  long long std_stride;
  const float* K; const float* T;
  float2* volume;
  int Dx, Dy, Dz;
  FastDiv div_x, div_xy;
  float ox, oy, oz, voxel, trunc, z_near, w_max, std_floor;
  int* counts;
  const float* rgb; float4* color;                    // COLOR only: the image [B][3][H][W], the colour volume, c = x * cstd + mean
  float mean[3], cstd[3];
};

// counts are zeroed by a launch of the library's own: a captured hipMemsetAsync of these B * 12 bytes (not a multiple of 8) came back from
// a graph replay on the MI355X with its first 32 bytes holding something else than zeros and only the 4-byte tail cleared
__global__ __launch_bounds__(256) void tsdf_zero_counts_kernel(int* __restrict__ counts, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) counts[i] = 0;
}

template <bool COLOR>
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(IntegrateP p) {
  constexpr int kCounts = COLOR ? 4 : 3;
  __shared__ int s[kCounts][256];
  const MetP& m = p.m;
  const int b = blockIdx.y;
  const unsigned nvox = (unsigned)p.Dx * p.Dy * p.Dz;            // < 2^31
  const float* pb = m.pred + (long long)b * m.Hp * m.Wp;
  const float* sb = p.u.pred ? p.u.pred + (long long)b * p.std_stride : nullptr;
  const float* K = p.K + b * 4;
  const float* T = p.T + b * 12;
  float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  float2* vol = p.volume + (long long)b * nvox;
  int seen = 0, updated = 0, behind = 0, coloured = 0;
  // The plain kernel fills the scalar register file to the brim, and the colour step's extra branches and pointers made the compiler
  // spill scalars.  The COLOR instance therefore holds its launch constants -- camera, pose, volume frame, image and colour volume -- in
  // vector registers (the empty asm's "+v"), of which it has plenty: 72 of 512 / 7 waves.  The plain instance compiles as before.
  float cm[3] = {0.f, 0.f, 0.f}, cs[3] = {1.f, 1.f, 1.f};
  const float* rgb = nullptr; float4* cvol = nullptr;
  int plane = 0;
  float ox = p.ox, oy = p.oy, oz = p.oz, voxel = p.voxel, trunc = p.trunc, w_max = p.w_max;
  float tv[12] = {};
  auto Tat = [&](int e) { if constexpr (COLOR) return tv[e]; else return T[e]; };
  if constexpr (COLOR) {
    asm volatile("" : "+v"(fx), "+v"(fy), "+v"(cx), "+v"(cy));
    asm volatile("" : "+v"(ox), "+v"(oy), "+v"(oz), "+v"(voxel), "+v"(trunc), "+v"(w_max));
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      tv[e] = T[e];
      asm volatile("" : "+v"(tv[e]));
    }
    plane = m.H * m.W;                                // < 2^31 - 256
    rgb = p.rgb + (long long)b * 3 * plane;
    cvol = p.color + (long long)b * nvox;
    asm volatile("" : "+v"(rgb), "+v"(cvol), "+v"(plane));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      cm[c] = p.mean[c]; cs[c] = p.cstd[c];
      asm volatile("" : "+v"(cm[c]), "+v"(cs[c]));
    }
  }
  for (long long n64 = (long long)blockIdx.x * 256 + threadIdx.x; n64 < nvox; n64 += (long long)gridDim.x * 256) {
    const unsigned n = (unsigned)n64;
    const unsigned k = fd_div(n, p.div_xy), r = n - k * p.div_xy.d;
    const unsigned j = fd_div(r, p.div_x), i = r - j * p.div_x.d;
    const float Xw = ox + voxel * (float)i, Yw = oy + voxel * (float)j, Zw = oz + voxel * (float)k;
    const float Xc = (Tat(0) * Xw + Tat(1) * Yw) + Tat(2) * Zw + Tat(3);
    const float Yc = (Tat(4) * Xw + Tat(5) * Yw) + Tat(6) * Zw + Tat(7);
    const float Zc = (Tat(8) * Xw + Tat(9) * Yw) + Tat(10) * Zw + Tat(11);
    if (!(finitef(Zc) && Zc >= p.z_near)) continue;
    const float uu = fx * (Xc / Zc) + cx, vv = fy * (Yc / Zc) + cy;
    const float col = floorf(uu + 0.5f), row = floorf(vv + 0.5f);
    if (!(col >= 0.f && col < (float)m.W && row >= 0.f && row < (float)m.H)) continue;      // NaN fails
    const int pix = (int)row * m.W + (int)col;
    const float d = met_pred(m, pb, pix);
    if (!(finitef(d) && d > 0.f)) continue;
    seen += 1;
    const float sdf = d - Zc;
    if (sdf < -trunc) { behind += 1; continue; }
    const float f = fminf(1.f, sdf / trunc);
    float w = 1.f;
    if (sb) {
      const float sd = met_plane(p.u, sb, pix);
      const float sf = sd > p.std_floor ? sd : p.std_floor;      // a NaN std takes the floor
      w = 1.f / (sf * sf);
    }
    if (!(w > 0.f && w < INFINITY)) continue;                    // an infinite std observes nothing
    const float2 fw = vol[n];
    const float tot = fw.y + w;
    vol[n] = make_float2((fw.x * fw.y + f * w) / tot, fminf(tot, w_max));
    updated += 1;
    if constexpr (COLOR) {
      if (sdf > trunc) continue;                                 // free space in front of the surface takes no colour
      const float* cb = rgb + pix;
      const float c0 = cb[0] * cs[0] + cm[0], c1 = cb[plane] * cs[1] + cm[1], c2 = cb[2ll * plane] * cs[2] + cm[2];
      if (!(finitef(c0) && finitef(c1) && finitef(c2))) continue;
      const float4 cw = cvol[n];
      const float ctot = cw.w + w;
      cvol[n] = make_float4((cw.x * cw.w + c0 * w) / ctot, (cw.y * cw.w + c1 * w) / ctot, (cw.z * cw.w + c2 * w) / ctot, fminf(ctot, w_max));
      coloured += 1;
    }
  }
  s[0][threadIdx.x] = seen; s[1][threadIdx.x] = updated; s[2][threadIdx.x] = behind;
  if constexpr (COLOR) s[3][threadIdx.x] = coloured;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s[0][threadIdx.x] += s[0][threadIdx.x + o]; s[1][threadIdx.x] += s[1][threadIdx.x + o]; s[2][threadIdx.x] += s[2][threadIdx.x + o];
      if constexpr (COLOR) s[3][threadIdx.x] += s[3][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < kCounts && s[threadIdx.x][0] != 0) atomicAdd(p.counts + b * kCounts + threadIdx.x, s[threadIdx.x][0]);
}

struct RaycastP {
  const float2* volume;
  int Dx, Dy, Dz;
  float ox, oy, oz, voxel;
  const float* K; const float* T;
  int Hd, Wd, tiles_x, kmax;
  float t_min, step;
  float* depth; float* normal; float* std;
};

struct Ray {                                          // per pixel: R, t of the pose, the ray's two slopes
  float T[12];
  float rx, ry;
};

// the grid coordinates of the ray's point at depth t
__device__ __forceinline__ void ray_point(const RaycastP& p, const Ray& r, float t, float& gx, float& gy, float& gz) {
  const float qx = r.rx * t - r.T[3], qy = r.ry * t - r.T[7], qz = t - r.T[11];
  const float Xw = (r.T[0] * qx + r.T[4] * qy) + r.T[8] * qz;
  const float Yw = (r.T[1] * qx + r.T[5] * qy) + r.T[9] * qz;
  const float Zw = (r.T[2] * qx + r.T[6] * qy) + r.T[10] * qz;
  gx = (Xw - p.ox) / p.voxel; gy = (Yw - p.oy) / p.voxel; gz = (Zw - p.oz) / p.voxel;
}

// trilinear (F, Wt) at grid coordinates g: false unless the 8 corners lie in the grid and all have Wt > 0
__device__ __forceinline__ bool tsdf_sample(const RaycastP& p, const float2* __restrict__ vol, float gx, float gy, float gz, float& F,
                                            float& Wt) {
  const float x0 = floorf(gx), y0 = floorf(gy), z0 = floorf(gz);
  if (!(x0 >= 0.f && x0 <= (float)(p.Dx - 2) && y0 >= 0.f && y0 <= (float)(p.Dy - 2) && z0 >= 0.f && z0 <= (float)(p.Dz - 2)))
    return false;                                     // on the float values; NaN fails
  const float a = gx - x0, bb = gy - y0, c = gz - z0, ha = 1.f - a, hb = 1.f - bb, hc = 1.f - c;
  const long long sy = p.Dx, sz = (long long)p.Dx * p.Dy;
  const float2* q = vol + ((long long)(int)z0 * sz + (long long)(int)y0 * sy + (int)x0);
  const float2 v000 = q[0], v100 = q[1], v010 = q[sy], v110 = q[sy + 1];
  const float2 v001 = q[sz], v101 = q[sz + 1], v011 = q[sz + sy], v111 = q[sz + sy + 1];
  if (!(v000.y > 0.f && v100.y > 0.f && v010.y > 0.f && v110.y > 0.f && v001.y > 0.f && v101.y > 0.f && v011.y > 0.f && v111.y > 0.f))
    return false;
  F = hc * (hb * (ha * v000.x + a * v100.x) + bb * (ha * v010.x + a * v110.x)) +
      c * (hb * (ha * v001.x + a * v101.x) + bb * (ha * v011.x + a * v111.x));
  Wt = hc * (hb * (ha * v000.y + a * v100.y) + bb * (ha * v010.y + a * v110.y)) +
       c * (hb * (ha * v001.y + a * v101.y) + bb * (ha * v011.y + a * v111.y));
  return true;
}

// The steps k0 .. k1 outside which the ray cannot have a valid sample: the slab test against the box -1 .. D of the grid coordinates (a
// voxel wider than the cells a valid sample needs), one more step either side.  Speed only: whatever it leaves in is still tested.
__device__ __forceinline__ void ray_clip(const RaycastP& p, const Ray& r, int& k0, int& k1) {
  float g0[3], g1[3];
  const float t_end = p.t_min + (float)p.kmax * p.step;
  ray_point(p, r, p.t_min, g0[0], g0[1], g0[2]);
  ray_point(p, r, t_end, g1[0], g1[1], g1[2]);
  const float hi[3] = {(float)p.Dx, (float)p.Dy, (float)p.Dz};
  float ka = 0.f, kb = (float)p.kmax;                 // in steps: g(k) = g0 + (g1 - g0) * k / kmax
  const float km = (float)max(p.kmax, 1);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if ((g0[a] < -2.f && g1[a] < -2.f) || (g0[a] > hi[a] + 1.f && g1[a] > hi[a] + 1.f)) kb = -1.f;      // both ends on one side of the slab
    const float gd = (g1[a] - g0[a]) / km;            // per step
    if (fabsf(gd) > 1e-6f) {
      float e0 = (-1.f - g0[a]) / gd, e1 = (hi[a] - g0[a]) / gd;
      if (e0 > e1) { const float t = e0; e0 = e1; e1 = t; }
      ka = fmaxf(ka, e0 - (2.f + 1e-5f * fabsf(e0)));            // fmaxf / fminf drop a NaN
      kb = fminf(kb, e1 + (2.f + 1e-5f * fabsf(e1)));
    }
  }
  k0 = (int)fminf(fmaxf(floorf(ka), 0.f), (float)p.kmax + 1.f);
  k1 = kb < 0.f ? -1 : (int)fminf(ceilf(kb), (float)p.kmax);
}

template <bool NORMALS>
__global__ __launch_bounds__(kTile * kTile) void tsdf_raycast_kernel(RaycastP p) {
  const int b = blockIdx.y;
  const int tyi = blockIdx.x / p.tiles_x, txi = blockIdx.x - tyi * p.tiles_x;
  const int x = txi * kTile + (threadIdx.x & (kTile - 1)), y = tyi * kTile + (threadIdx.x >> 4);
  if (x >= p.Wd || y >= p.Hd) return;
  const float* K = p.K + b * 4;
  Ray r;
#pragma unroll
  for (int e = 0; e < 12; ++e) r.T[e] = p.T[b * 12 + e];
  r.rx = ((float)x - K[2]) / K[0];
  r.ry = ((float)y - K[3]) / K[1];
  const float2* vol = p.volume + (long long)b * p.Dx * p.Dy * p.Dz;
  int k0, k1;
  ray_clip(p, r, k0, k1);
  bool prev = false;
  float F_prev = 0.f, depth = NAN;
  for (int k = k0; k <= k1; ++k) {
    const float t = p.t_min + (float)k * p.step;
    float gx, gy, gz, F = 0.f, Wt = 0.f;
    ray_point(p, r, t, gx, gy, gz);
    const bool ok = tsdf_sample(p, vol, gx, gy, gz, F, Wt);
    if (ok && prev) {
      if (F_prev > 0.f && F <= 0.f) {
        const float t_prev = p.t_min + (float)(k - 1) * p.step;
        depth = t_prev + p.step * (F_prev / (F_prev - F));
        break;
      }
      if (F_prev < 0.f && F > 0.f) break;             // a back face ends the ray
    }
    prev = ok; F_prev = F;
  }
  const long long o = ((long long)b * p.Hd + y) * p.Wd + x;
  p.depth[o] = depth;
  if (!p.std && !NORMALS) return;
  float sd = NAN, nx = NAN, ny = NAN, nz = NAN;
  if (depth == depth) {
    float gx, gy, gz, F, Wt;
    ray_point(p, r, depth, gx, gy, gz);
    if (tsdf_sample(p, vol, gx, gy, gz, F, Wt)) sd = 1.f / sqrtf(Wt);
    if constexpr (NORMALS) {
      float f0 = 0.f, f1 = 0.f, w = 0.f;
      bool ok = tsdf_sample(p, vol, gx - 1.f, gy, gz, f0, w) && tsdf_sample(p, vol, gx + 1.f, gy, gz, f1, w);
      const float dx = f1 - f0;
      ok = ok && tsdf_sample(p, vol, gx, gy - 1.f, gz, f0, w) && tsdf_sample(p, vol, gx, gy + 1.f, gz, f1, w);
      const float dy = f1 - f0;
      ok = ok && tsdf_sample(p, vol, gx, gy, gz - 1.f, f0, w) && tsdf_sample(p, vol, gx, gy, gz + 1.f, f1, w);
      const float dz = f1 - f0;
      const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
      if (ok && len > 0.f && finitef(len)) {
        const float wx = dx / len, wy = dy / len, wz = dz / len;
        nx = (r.T[0] * wx + r.T[1] * wy) + r.T[2] * wz;
        ny = (r.T[4] * wx + r.T[5] * wy) + r.T[6] * wz;
        nz = (r.T[8] * wx + r.T[9] * wy) + r.T[10] * wz;
      }
    }
  }
  if (p.std) p.std[o] = sd;
  if constexpr (NORMALS) { p.normal[o * 3] = nx; p.normal[o * 3 + 1] = ny; p.normal[o * 3 + 2] = nz; }
}

bool pos_finite(float v) { return v > 0.f && v < INFINITY; }      // false for NaN

// cfp_tsdf_integrate and cfp_tsdf_integrate_rgb: one set of checks (`who` names the caller in the message) and one launch; rgb != null
// selects the COLOR instance, whose mean, cstd and color the caller has checked
int integrate_launch(const char* who_, const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                     const float* std, int Hu, int Wu, long long std_stride, float std_floor, const float* K, const float* T, float* volume,
                     int Dx, int Dy, int Dz, float ox, float oy, float oz, float voxel, float trunc, float z_near, float w_max,
                     const float* rgb, const float* mean, const float* cstd, float* color, int* counts, cfp_stream_t stream) {
  const std::string who(who_);
  CFP_REQUIRE(pred && K && T && volume && counts, CFP_EINVAL, who + ": null pointer");
  CFP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0 && Dx > 0 && Dy > 0 && Dz > 0, CFP_ESHAPE, who + ": non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) - 256 && (long long)Hp * Wp < (1ll << 31) && H <= kMaxDim && W <= kMaxDim && B <= 65535,
              CFP_ESHAPE, who + ": image or batch too large");
  CFP_REQUIRE(Dx <= kMaxDim && Dy <= kMaxDim && Dz <= kMaxDim && (long long)Dx * Dy < (1ll << 31) &&
                  (long long)Dx * Dy * Dz < (1ll << 31) - 256, CFP_ESHAPE, who + ": volume too large");
  CFP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, who + ": sizes differ and interpolate is off");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, who + ": empty depth range");
  if (std) {
    CFP_REQUIRE(Hu > 0 && Wu > 0, CFP_ESHAPE, who + ": non-positive dimension (std)");
    CFP_REQUIRE((long long)Hu * Wu < (1ll << 31), CFP_ESHAPE, who + ": std plane too large");
    CFP_REQUIRE(std_stride >= 0, CFP_EINVAL, who + ": negative std image stride");
  }
  CFP_REQUIRE(pos_finite(std_floor), CFP_EINVAL, who + ": std_floor must be positive and finite");
  CFP_REQUIRE(pos_finite(voxel), CFP_EINVAL, who + ": voxel must be positive and finite");
  CFP_REQUIRE(pos_finite(trunc), CFP_EINVAL, who + ": trunc must be positive and finite");
  CFP_REQUIRE(pos_finite(z_near), CFP_EINVAL, who + ": z_near must be positive and finite");
  CFP_REQUIRE(pos_finite(w_max), CFP_EINVAL, who + ": w_max must be positive and finite");
  CFP_REQUIRE(std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz), CFP_EINVAL, who + ": origin must be finite");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(volume) & 7) == 0, CFP_EINVAL, who + ": volume must be 8-byte aligned");
  IntegrateP p;
  p.m = met_params(pred, nullptr, Hp, Wp, H, W, B, interpolate, 0, lo, hi);
  p.u = met_params(std, nullptr, std ? Hu : H, std ? Wu : W, H, W, B, std && (Hu != H || Wu != W) ? 1 : 0, 0, 0.f, 0.f);
  p.std_stride = std_stride;
  p.K = K; p.T = T;
  p.volume = reinterpret_cast<float2*>(volume);
  p.Dx = Dx; p.Dy = Dy; p.Dz = Dz;
  p.div_x = make_fastdiv((unsigned)Dx); p.div_xy = make_fastdiv((unsigned)Dx * (unsigned)Dy);
  p.ox = ox; p.oy = oy; p.oz = oz; p.voxel = voxel; p.trunc = trunc; p.z_near = z_near; p.w_max = w_max; p.std_floor = std_floor;
  p.counts = counts;
  p.rgb = rgb; p.color = reinterpret_cast<float4*>(color);
  for (int c = 0; c < 3; ++c) { p.mean[c] = rgb ? mean[c] : 0.f; p.cstd[c] = rgb ? cstd[c] : 1.f; }      // the host pointers of the call
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long nvox = (long long)Dx * Dy * Dz;
  const int ncounts = B * (rgb ? 4 : 3);
  const dim3 grid((unsigned)std::min<long long>((nvox + 255) / 256, kMaxBlocks), B);
  hipLaunchKernelGGL(tsdf_zero_counts_kernel, dim3(cdiv(ncounts, 256)), dim3(256), 0, s, counts, ncounts);
  if (rgb) hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, dim3(256), 0, s, p);
  return cfp_check_launch(who_);
}

}  // namespace

extern "C" int cfp_tsdf_integrate(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                                  const float* std, int Hu, int Wu, long long std_stride, float std_floor, const float* K, const float* T,
                                  float* volume, int Dx, int Dy, int Dz, float ox, float oy, float oz, float voxel, float trunc,
                                  float z_near, float w_max, int* counts, cfp_stream_t stream) {
  return integrate_launch("cfp_tsdf_integrate", pred, Hp, Wp, H, W, B, interpolate, lo, hi, std, Hu, Wu, std_stride, std_floor, K, T, volume,
                          Dx, Dy, Dz, ox, oy, oz, voxel, trunc, z_near, w_max, nullptr, nullptr, nullptr, nullptr, counts, stream);
}

extern "C" int cfp_tsdf_integrate_rgb(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                                      const float* std, int Hu, int Wu, long long std_stride, float std_floor, const float* K,
                                      const float* T, float* volume, int Dx, int Dy, int Dz, float ox, float oy, float oz, float voxel,
                                      float trunc, float z_near, float w_max, const float* rgb, const float* mean, const float* cstd,
                                      float* color, int* counts, cfp_stream_t stream) {
  CFP_REQUIRE(rgb && mean && cstd && color, CFP_EINVAL, "cfp_tsdf_integrate_rgb: null pointer");
  for (int c = 0; c < 3; ++c)
    CFP_REQUIRE(std::isfinite(mean[c]) && std::isfinite(cstd[c]), CFP_EINVAL, "cfp_tsdf_integrate_rgb: mean and cstd must be finite");
  CFP_REQUIRE(aligned16(color), CFP_EINVAL, "cfp_tsdf_integrate_rgb: color must be 16-byte aligned");
  return integrate_launch("cfp_tsdf_integrate_rgb", pred, Hp, Wp, H, W, B, interpolate, lo, hi, std, Hu, Wu, std_stride, std_floor, K, T,
                          volume, Dx, Dy, Dz, ox, oy, oz, voxel, trunc, z_near, w_max, rgb, mean, cstd, color, counts, stream);
}

extern "C" int cfp_tsdf_raycast(const float* volume, int Dx, int Dy, int Dz, int B, float ox, float oy, float oz, float voxel,
                                const float* K, const float* T, int Hd, int Wd, float t_min, float t_max, float step, float* depth,
                                float* normal, float* std, cfp_stream_t stream) {
  CFP_REQUIRE(volume && K && T && depth, CFP_EINVAL, "cfp_tsdf_raycast: null pointer");
  CFP_REQUIRE(B > 0 && Dx > 0 && Dy > 0 && Dz > 0 && Hd > 0 && Wd > 0, CFP_ESHAPE, "cfp_tsdf_raycast: non-positive dimension");
  CFP_REQUIRE(Dx <= kMaxDim && Dy <= kMaxDim && Dz <= kMaxDim && (long long)Dx * Dy < (1ll << 31) &&
                  (long long)Dx * Dy * Dz < (1ll << 31) - 256, CFP_ESHAPE, "cfp_tsdf_raycast: volume too large");
  CFP_REQUIRE((long long)Hd * Wd < (1ll << 31) - 256 && Hd <= kMaxDim && Wd <= kMaxDim && B <= 65535, CFP_ESHAPE,
              "cfp_tsdf_raycast: image or batch too large");
  CFP_REQUIRE(pos_finite(voxel), CFP_EINVAL, "cfp_tsdf_raycast: voxel must be positive and finite");
  CFP_REQUIRE(pos_finite(step), CFP_EINVAL, "cfp_tsdf_raycast: step must be positive and finite");
  CFP_REQUIRE(t_min < t_max && std::isfinite(t_min) && std::isfinite(t_max), CFP_EINVAL,
              "cfp_tsdf_raycast: t_min < t_max, both finite, is required");
  CFP_REQUIRE(std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz), CFP_EINVAL, "cfp_tsdf_raycast: origin must be finite");
  const float steps = floorf((t_max - t_min) / step);
  CFP_REQUIRE(steps < (float)kMaxDim, CFP_ESHAPE, "cfp_tsdf_raycast: too large a number of steps");      // false for NaN / inf
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(volume) & 7) == 0, CFP_EINVAL, "cfp_tsdf_raycast: volume must be 8-byte aligned");
  RaycastP p;
  p.volume = reinterpret_cast<const float2*>(volume);
  p.Dx = Dx; p.Dy = Dy; p.Dz = Dz;
  p.ox = ox; p.oy = oy; p.oz = oz; p.voxel = voxel;
  p.K = K; p.T = T;
  p.Hd = Hd; p.Wd = Wd; p.tiles_x = cdiv(Wd, kTile); p.kmax = (int)steps;
  p.t_min = t_min; p.step = step;
  p.depth = depth; p.normal = normal; p.std = std;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(p.tiles_x * cdiv(Hd, kTile)), B);
  if (normal) hipLaunchKernelGGL(tsdf_raycast_kernel<true>, grid, dim3(kTile * kTile), 0, s, p);
  else hipLaunchKernelGGL(tsdf_raycast_kernel<false>, grid, dim3(kTile * kTile), 0, s, p);
  return cfp_check_launch("cfp_tsdf_raycast");
}
