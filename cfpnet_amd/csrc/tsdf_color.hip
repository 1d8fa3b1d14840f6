// Reading the colour volume cfp_tsdf_integrate_rgb keeps next to the TSDF (float4 (R, G, B, Wc) per voxel; the definitions are in
// include/cfpnet_hip.h): the colour of the map at the points a depth map names (cfp_tsdf_shade) and at the lattice edges
// cfp_tsdf_surface has extracted (cfp_tsdf_surface_rgb).  Both only read the volumes, have no workspace and no atomics.
//
// Shade.  One thread per pixel in the raycast's 16 x 16 tiles, so neighbouring pixels gather the corners of the same cells; a corner is
// one 16-byte load.  The ray and its point are the raycast's expressions, restated here: sharing them through a header would put the
// raycast kernel's code generation at the mercy of this file's needs.  The blend is renormalised over the corners that have a colour.
//
// Surface colours.  One thread per row of the index list.  The index is device data: an edge that is not one of the lattice's reads
// nothing and gives NaN.
#include "common.h"

#include <cmath>

namespace {

constexpr long long kMaxDim = 1ll << 24;              // a row, column or voxel index is used as a float: exact below 2^24
constexpr int kTile = 16;                             // the raycast's pixel tile

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }      // false for NaN

struct ShadeP {
  const float4* color;
  int Dx, Dy, Dz;
  float ox, oy, oz, voxel;
  const float* K; const float* T;
  int Hd, Wd, tiles_x;
  const float* depth; float* out;
};

__global__ __launch_bounds__(kTile * kTile) void tsdf_shade_kernel(ShadeP p) {
  const int b = blockIdx.y;
  const int tyi = blockIdx.x / p.tiles_x, txi = blockIdx.x - tyi * p.tiles_x;
  const int x = txi * kTile + (threadIdx.x & (kTile - 1)), y = tyi * kTile + (threadIdx.x >> 4);
  if (x >= p.Wd || y >= p.Hd) return;
  const float* K = p.K + b * 4;
  const float* T = p.T + b * 12;
  const long long o = ((long long)b * p.Hd + y) * p.Wd + x;
  const float t = p.depth[o];
  float r0 = NAN, r1 = NAN, r2 = NAN;
  if (finitef(t)) {
    const float rx = ((float)x - K[2]) / K[0], ry = ((float)y - K[3]) / K[1];
    const float qx = rx * t - T[3], qy = ry * t - T[7], qz = t - T[11];
    const float Xw = (T[0] * qx + T[4] * qy) + T[8] * qz;
    const float Yw = (T[1] * qx + T[5] * qy) + T[9] * qz;
    const float Zw = (T[2] * qx + T[6] * qy) + T[10] * qz;
    const float gx = (Xw - p.ox) / p.voxel, gy = (Yw - p.oy) / p.voxel, gz = (Zw - p.oz) / p.voxel;
    const float x0 = floorf(gx), y0 = floorf(gy), z0 = floorf(gz);
    if (x0 >= 0.f && x0 <= (float)(p.Dx - 2) && y0 >= 0.f && y0 <= (float)(p.Dy - 2) && z0 >= 0.f && z0 <= (float)(p.Dz - 2)) {      // NaN fails
      const float a = gx - x0, bb = gy - y0, c = gz - z0;
      const float wx[2] = {1.f - a, a}, wy[2] = {1.f - bb, bb}, wz[2] = {1.f - c, c};
      const long long sy = p.Dx, sz = (long long)p.Dx * p.Dy;
      const float4* q = p.color + (long long)b * sz * p.Dz + ((long long)(int)z0 * sz + (long long)(int)y0 * sy + (int)x0);
      float4 v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = q[(e >> 2) * sz + ((e >> 1) & 1) * sy + (e & 1)];      // x fastest, then y, then z
      float den = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
      bool any = false;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float tw = (wx[e & 1] * wy[(e >> 1) & 1]) * wz[e >> 2];
        if (v[e].w > 0.f) {
          any = true;
          den += tw; n0 += tw * v[e].x; n1 += tw * v[e].y; n2 += tw * v[e].z;
        }
      }
      if (any) { r0 = n0 / den; r1 = n1 / den; r2 = n2 / den; }
    }
  }
  p.out[o * 3] = r0; p.out[o * 3 + 1] = r1; p.out[o * 3 + 2] = r2;
}

struct SurfRgbP {
  const float2* volume; const float4* color;
  int Dx, Dy, Dz, nvox, cap;
  FastDiv div_x, div_xy;
  const int* index; const int* counts;
  float* colors;
};

__global__ __launch_bounds__(256) void tsdf_surface_rgb_kernel(SurfRgbP p) {
  const int b = blockIdx.y;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= p.cap || r >= p.counts[b]) return;
  const long long row = (long long)b * p.cap + r;
  const int e = p.index[row];
  float c0 = NAN, c1 = NAN, c2 = NAN;
  if (e >= 0 && e < 3 * p.nvox) {                                 // 3 * nvox < 2^31
    const unsigned n = (unsigned)e / 3u, a = (unsigned)e - 3u * n;
    const unsigned k = fd_div(n, p.div_xy), rr = n - k * p.div_xy.d;
    const unsigned j = fd_div(rr, p.div_x), i = rr - j * p.div_x.d;
    const bool in = a == 0 ? (int)i + 1 < p.Dx : (a == 1 ? (int)j + 1 < p.Dy : (int)k + 1 < p.Dz);
    if (in) {                                                     // q = n + dn is a voxel of the grid
      const unsigned dn = a == 0 ? 1u : (a == 1 ? (unsigned)p.Dx : p.div_xy.d);
      const float2* vol = p.volume + (long long)b * p.nvox;
      const float4* col = p.color + (long long)b * p.nvox;
      const float fp = vol[n].x, fq = vol[n + dn].x;
      const float4 cp = col[n], cq = col[n + dn];
      const float t = fp / (fp - fq), h = 1.f - t;
      if (cp.w > 0.f && cq.w > 0.f) { c0 = h * cp.x + t * cq.x; c1 = h * cp.y + t * cq.y; c2 = h * cp.z + t * cq.z; }
      else if (cp.w > 0.f) { c0 = cp.x; c1 = cp.y; c2 = cp.z; }
      else if (cq.w > 0.f) { c0 = cq.x; c1 = cq.y; c2 = cq.z; }
    }
  }
  p.colors[row * 3] = c0; p.colors[row * 3 + 1] = c1; p.colors[row * 3 + 2] = c2;
}

}  // namespace

extern "C" int cfp_tsdf_shade(const float* color, int Dx, int Dy, int Dz, int B, float ox, float oy, float oz, float voxel, const float* K,
                              const float* T, int Hd, int Wd, const float* depth, float* rgb_out, cfp_stream_t stream) {
  CFP_REQUIRE(color && K && T && depth && rgb_out, CFP_EINVAL, "cfp_tsdf_shade: null pointer");
  CFP_REQUIRE(B > 0 && Dx > 0 && Dy > 0 && Dz > 0 && Hd > 0 && Wd > 0, CFP_ESHAPE, "cfp_tsdf_shade: non-positive dimension");
  CFP_REQUIRE(Dx <= kMaxDim && Dy <= kMaxDim && Dz <= kMaxDim && (long long)Dx * Dy < (1ll << 31) &&
                  (long long)Dx * Dy * Dz < (1ll << 31) - 256, CFP_ESHAPE, "cfp_tsdf_shade: volume too large");
  CFP_REQUIRE((long long)Hd * Wd < (1ll << 31) - 256 && Hd <= kMaxDim && Wd <= kMaxDim && B <= 65535, CFP_ESHAPE,
              "cfp_tsdf_shade: image or batch too large");
  CFP_REQUIRE(voxel > 0.f && voxel < INFINITY, CFP_EINVAL, "cfp_tsdf_shade: voxel must be positive and finite");
  CFP_REQUIRE(std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz), CFP_EINVAL, "cfp_tsdf_shade: origin must be finite");
  CFP_REQUIRE(aligned16(color), CFP_EINVAL, "cfp_tsdf_shade: color must be 16-byte aligned");
  ShadeP p;
  p.color = reinterpret_cast<const float4*>(color);
  p.Dx = Dx; p.Dy = Dy; p.Dz = Dz;
  p.ox = ox; p.oy = oy; p.oz = oz; p.voxel = voxel;
  p.K = K; p.T = T;
  p.Hd = Hd; p.Wd = Wd; p.tiles_x = cdiv(Wd, kTile);
  p.depth = depth; p.out = rgb_out;
  hipLaunchKernelGGL(tsdf_shade_kernel, dim3((unsigned)(p.tiles_x * cdiv(Hd, kTile)), B), dim3(kTile * kTile), 0,
                     reinterpret_cast<hipStream_t>(stream), p);
  return cfp_check_launch("cfp_tsdf_shade");
}

extern "C" int cfp_tsdf_surface_rgb(const float* volume, const float* color, int Dx, int Dy, int Dz, int B, const int* index,
                                    const int* counts, int cap, float* colors, cfp_stream_t stream) {
  CFP_REQUIRE(volume && color && index && counts && colors, CFP_EINVAL, "cfp_tsdf_surface_rgb: null pointer");
  CFP_REQUIRE(B > 0 && Dx > 0 && Dy > 0 && Dz > 0, CFP_ESHAPE, "cfp_tsdf_surface_rgb: non-positive dimension");
  CFP_REQUIRE((long long)Dx * Dy < (1ll << 31) && 3 * ((long long)Dx * Dy * Dz) < (1ll << 31) && B <= 65535, CFP_ESHAPE,
              "cfp_tsdf_surface_rgb: volume or batch too large (an edge index 3 * Dx * Dy * Dz must fit an int32)");
  CFP_REQUIRE(cap >= 1, CFP_EINVAL, "cfp_tsdf_surface_rgb: cap must be at least 1");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(volume) & 7) == 0, CFP_EINVAL, "cfp_tsdf_surface_rgb: volume must be 8-byte aligned");
  CFP_REQUIRE(aligned16(color), CFP_EINVAL, "cfp_tsdf_surface_rgb: color must be 16-byte aligned");
  SurfRgbP p;
  p.volume = reinterpret_cast<const float2*>(volume);
  p.color = reinterpret_cast<const float4*>(color);
  p.Dx = Dx; p.Dy = Dy; p.Dz = Dz; p.nvox = Dx * Dy * Dz; p.cap = cap;
  p.div_x = make_fastdiv((unsigned)Dx); p.div_xy = make_fastdiv((unsigned)Dx * (unsigned)Dy);
  p.index = index; p.counts = counts; p.colors = colors;
  hipLaunchKernelGGL(tsdf_surface_rgb_kernel, dim3(cdiv(cap, 256), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
  return cfp_check_launch("cfp_tsdf_surface_rgb");
}
