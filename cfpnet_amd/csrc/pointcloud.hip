// The last mile after the depth map, on the device: back-projection of the prediction to an organised point map with surface normals
// (cfp_depth_unproject) and an order-preserving compaction of that map to the points a consumer wants (cfp_points_compact).
//
//   reference hooks: the clip / bilinear protocol of evaluate_all.py:40-41 -- the depth at a full-resolution pixel is met_pred of
//   metrics_pred.h in mode 0, the value cfp_eval_metrics evaluates, bit for bit -- and the pinhole intrinsics (fx, fy, cx, cy) the
//   ZJU-L5 loader carries and never uses (src/dataloader/zjuL5.py:66-71).  The definition is in include/cfpnet_hip.h.
//
// Unproject.  A workgroup owns tiles of 16 x 64 pixels.  It interpolates every depth of the tile and of a 1-pixel halo once into LDS
// (1188 evaluations per 1024 pixels; a halo cell outside the image holds the depth of the clamped coordinate, which is exactly the clamped
// neighbour of the definition), then each wave takes four rows, one pixel per lane and row, and stages the xyz triples in LDS so that
// they leave as contiguous runs: 16-byte stores when the row pitch allows it, dword stores of 256 contiguous bytes per wave otherwise.
// Both outputs are write-once streams of 12 bytes per pixel; measured against a same-bytes copy in DESIGN.md section 4.15.
//
// Compact.  Candidates are the pixels on the stride grid, numbered row-major -- the same order as their pixel indices.  A wave owns a
// chunk of 256 consecutive candidates (4 per lane, step by step 64 contiguous ones).  Three launches and no atomics, so the order and
// every bit of the result are a function of the inputs alone:
//   1. count    per (image, chunk): popcount of the predicate's ballots -> workspace
//   2. scan     one workgroup per image: exclusive scan of the chunk counts in place, the total -> counts[b] (chunk_scan.h)
//   3. scatter  the predicate again; rank = chunk offset + kept lanes of the earlier steps + popcount(ballot & lanes below)
// Rows at or beyond `cap` are dropped, counts[b] stays the true total.
#include "common.h"
#include "chunk_scan.h"
#include "metrics_pred.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kTileH = 16, kTileW = 64;
constexpr int kHaloH = kTileH + 2, kHaloW = kTileW + 2;
constexpr int kRowsPerWave = kTileH / 4;
constexpr int kMaxBlocks = 2048;                      // grid cap of a memory-bound kernel; the tiles beyond it are grid-strided

struct UnprojP {
  MetP m;                                             // pred, Hp, Wp, H, W, interpolate, mode 0, lo, hi, sy, sx
  const float* K;
  float* points; float* normals;
  int tiles_x, tiles_y;
  long long tiles;
};

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }      // false for NaN

// V4: rows leave as 16-byte stores (W % 4 == 0 and 16-byte aligned outputs, so a vector never straddles the end of a row)
template <bool NORMALS, bool V4>
__global__ __launch_bounds__(256) void unproject_kernel(UnprojP p) {
  __shared__ float sD[kHaloH * kHaloW];
  __shared__ __attribute__((aligned(16))) float sP[4][kRowsPerWave * kTileW * 3];
  __shared__ __attribute__((aligned(16))) float sN[NORMALS ? 4 : 1][NORMALS ? kRowsPerWave * kTileW * 3 : 4];
  const MetP& m = p.m;
  const int H = m.H, W = m.W;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int per_image = p.tiles_x * p.tiles_y;

  for (long long tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int b = (int)(tile / per_image);
    const int t = (int)(tile - (long long)b * per_image);
    const int tyi = t / p.tiles_x, txi = t - tyi * p.tiles_x;
    const int ty0 = tyi * kTileH, tx0 = txi * kTileW;
    const float* pb = m.pred + (long long)b * m.Hp * m.Wp;

    // every depth of the tile and its halo once; coordinates clamped to the image
    for (int c = threadIdx.x; c < kHaloH * kHaloW; c += 256) {
      const int hy = c / kHaloW, hx = c - hy * kHaloW;
      const int gy = min(max(ty0 + hy - 1, 0), H - 1), gx = min(max(tx0 + hx - 1, 0), W - 1);
      sD[c] = met_pred(m, pb, gy * W + gx);
    }
    __syncthreads();

    const float fx = p.K[b * 4 + 0], fy = p.K[b * 4 + 1], cx = p.K[b * 4 + 2], cy = p.K[b * 4 + 3];
    const int x = tx0 + lane;
    const float rx = ((float)x - cx) / fx;
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
      const int ly = wave * kRowsPerWave + r, y = ty0 + ly;
      const float* c = sD + (ly + 1) * kHaloW + lane + 1;
      const float d = c[0];
      const float ry = ((float)y - cy) / fy;
      float* o = &sP[wave][(r * kTileW + lane) * 3];
      o[0] = rx * d; o[1] = ry * d; o[2] = d;
      if constexpr (NORMALS) {
        const float d0 = c[-1], d1 = c[1], e0 = c[-kHaloW], e1 = c[kHaloW];
        const int x0 = max(x - 1, 0), x1 = min(x + 1, W - 1), y0 = max(y - 1, 0), y1 = min(y + 1, H - 1);
        const float kx = (float)(x1 - x0), ky = (float)(y1 - y0);
        const float xm = 0.5f * (float)(x0 + x1), ym = 0.5f * (float)(y0 + y1);
        const float dd = d1 - d0, ds = d1 + d0, ed = e1 - e0, es = e1 + e0;
        // T_x = P(x1, y) - P(x0, y) and T_y = P(x, y1) - P(x, y0) without the cancellation of the point differences
        const float txx = dd * ((xm - cx) / fx) + ds * (0.5f * kx / fx), txy = dd * ry, txz = dd;
        const float tyx = ed * rx, tyy = ed * ((ym - cy) / fy) + es * (0.5f * ky / fy), tyz = ed;
        const float nx = tyy * txz - tyz * txy, ny = tyz * txx - tyx * txz, nz = tyx * txy - tyy * txx;      // T_y x T_x
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        const bool ok = finitef(d) && finitef(d0) && finitef(d1) && finitef(e0) && finitef(e1) && len > 0.f && finitef(len);
        float* q = &sN[wave][(r * kTileW + lane) * 3];
        q[0] = ok ? nx / len : 0.f; q[1] = ok ? ny / len : 0.f; q[2] = ok ? nz / len : 0.f;
      }
    }
    __syncthreads();

    // the staged rows leave as contiguous runs of min(64, W - tx0) * 3 floats
    const int run = min(kTileW, W - tx0) * 3;
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
      const int y = ty0 + wave * kRowsPerWave + r;
      if (y >= H) break;
      const long long g = (((long long)b * H + y) * W + tx0) * 3;
      const float* sp = &sP[wave][r * kTileW * 3];
      const float* sn = &sN[NORMALS ? wave : 0][NORMALS ? r * kTileW * 3 : 0];
      if constexpr (V4) {
        const int j = lane * 4;                                   // 48 vectors cover a full row; run % 4 == 0
        if (lane < kTileW * 3 / 4 && j < run) {
          *reinterpret_cast<f32x4*>(p.points + g + j) = *reinterpret_cast<const f32x4*>(sp + j);
          if constexpr (NORMALS) *reinterpret_cast<f32x4*>(p.normals + g + j) = *reinterpret_cast<const f32x4*>(sn + j);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int j = k * 64 + lane;
          if (j < run) {
            p.points[g + j] = sp[j];
            if constexpr (NORMALS) p.normals[g + j] = sn[j];
          }
        }
      }
    }
    __syncthreads();                                              // the next tile overwrites sD / sP / sN
  }
}

// ---- compaction --------------------------------------------------------------------------------------------------------------------------

constexpr int kCompU = 4;                             // steps of 64 candidates per wave
constexpr int kChunk = 64 * kCompU;                   // candidates per chunk (one wave)

struct CompP {
  MetP u;                                             // the uncertainty plane as met_plane reads it: pred = plane base, Hp x Wp = Hu x Wu
  const float* points; const float* normals;
  long long unc_stride;
  int Wc, N, nchunks, stride, cap, has_unc;
  float z_near, z_far, unc_lo, unc_hi;
  float* out_points; float* out_normals; int* out_index; int* counts; int* ws;
};

// candidate j of image b -> its pixel index y * W + x, or -1 past the last candidate
__device__ __forceinline__ int comp_pixel(const CompP& p, int j) {
  if (j >= p.N) return -1;
  const int yc = j / p.Wc, xc = j - yc * p.Wc;
  return yc * p.stride * p.u.W + xc * p.stride;
}

__device__ __forceinline__ bool comp_keep(const CompP& p, int b, int pix) {
  if (pix < 0) return false;
  const float z = p.points[((long long)b * p.u.H * p.u.W + pix) * 3 + 2];
  bool keep = finitef(z) && z > p.z_near && z < p.z_far;
  if (keep && p.has_unc) {
    const float u = met_plane(p.u, p.u.pred + (long long)b * p.unc_stride, pix);
    keep = u >= p.unc_lo && u <= p.unc_hi;                        // NaN fails
  }
  return keep;
}

__global__ __launch_bounds__(256) void compact_count_kernel(CompP p) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= p.nchunks) return;                                 // wave-uniform
  int n = 0;
#pragma unroll
  for (int s = 0; s < kCompU; ++s) n += __popcll(__ballot(comp_keep(p, b, comp_pixel(p, chunk * kChunk + s * 64 + lane))));
  if (lane == 0) p.ws[(long long)b * p.nchunks + chunk] = n;
}

template <bool NORMALS>
__global__ __launch_bounds__(256) void compact_scatter_kernel(CompP p) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= p.nchunks) return;                                 // wave-uniform
  int base = p.ws[(long long)b * p.nchunks + chunk];
  if (base >= p.cap) return;                                      // everything from here on is beyond the capacity
  const unsigned long long below = (1ull << lane) - 1ull;
  const long long img = (long long)b * p.u.H * p.u.W;
#pragma unroll
  for (int s = 0; s < kCompU; ++s) {
    const int pix = comp_pixel(p, chunk * kChunk + s * 64 + lane);
    const bool keep = comp_keep(p, b, pix);
    const unsigned long long bal = __ballot(keep);
    const int row = base + __popcll(bal & below);
    if (keep && row < p.cap) {
      const long long src = (img + pix) * 3, dst = ((long long)b * p.cap + row) * 3;
      p.out_points[dst] = p.points[src]; p.out_points[dst + 1] = p.points[src + 1]; p.out_points[dst + 2] = p.points[src + 2];
      if constexpr (NORMALS) {
        p.out_normals[dst] = p.normals[src]; p.out_normals[dst + 1] = p.normals[src + 1]; p.out_normals[dst + 2] = p.normals[src + 2];
      }
      p.out_index[(long long)b * p.cap + row] = pix;
    }
    base += __popcll(bal);
  }
}

// candidates per image on the stride grid (at most H * W), 0 if the arguments make no sense
long long comp_candidates(int H, int W, int stride) {
  if (H <= 0 || W <= 0 || stride < 1) return 0;
  return (long long)((H + stride - 1) / stride) * ((W + stride - 1) / stride);
}

}  // namespace

extern "C" int cfp_depth_unproject(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                                   const float* K, float* points, float* normals, cfp_stream_t stream) {
  CFP_REQUIRE(pred && K && points, CFP_EINVAL, "cfp_depth_unproject: null pointer");
  CFP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0, CFP_ESHAPE, "cfp_depth_unproject: non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) - 2 * kChunk && (long long)Hp * Wp < (1ll << 31), CFP_ESHAPE,
              "cfp_depth_unproject: image too large");
  CFP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, "cfp_depth_unproject: sizes differ and interpolate is off");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, "cfp_depth_unproject: empty depth range");
  UnprojP p;
  p.m = met_params(pred, nullptr, Hp, Wp, H, W, B, interpolate, 0, lo, hi);
  p.K = K; p.points = points; p.normals = normals;
  p.tiles_x = cdiv(W, kTileW); p.tiles_y = cdiv(H, kTileH);
  p.tiles = (long long)B * p.tiles_x * p.tiles_y;
  const int grid = (int)std::min<long long>(p.tiles, kMaxBlocks);
  const bool v4 = W % 4 == 0 && aligned16(points) && (!normals || aligned16(normals));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (normals) {
    if (v4) hipLaunchKernelGGL((unproject_kernel<true, true>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((unproject_kernel<true, false>), dim3(grid), dim3(256), 0, s, p);
  } else {
    if (v4) hipLaunchKernelGGL((unproject_kernel<false, true>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((unproject_kernel<false, false>), dim3(grid), dim3(256), 0, s, p);
  }
  return cfp_check_launch("cfp_depth_unproject");
}

extern "C" size_t cfp_points_compact_ws_bytes(int B, int H, int W, int stride) {
  const long long n = comp_candidates(H, W, stride);
  if (B <= 0 || n <= 0) return 0;
  const size_t ints = (size_t)B * (size_t)((n + kChunk - 1) / kChunk);
  return ((ints + 1) / 2) * 8;
}

extern "C" int cfp_points_compact(const float* points, const float* normals, int H, int W, int B, int stride, float z_near, float z_far,
                                  const float* unc, int Hu, int Wu, long long unc_stride, float unc_lo, float unc_hi, int cap,
                                  float* out_points, float* out_normals, int* out_index, int* counts, void* ws, size_t ws_bytes,
                                  cfp_stream_t stream) {
  CFP_REQUIRE(points && out_points && out_index && counts && ws, CFP_EINVAL, "cfp_points_compact: null pointer");
  CFP_REQUIRE(B > 0 && H > 0 && W > 0, CFP_ESHAPE, "cfp_points_compact: non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) - 2 * kChunk && B <= 65535, CFP_ESHAPE, "cfp_points_compact: image or batch too large");
  CFP_REQUIRE(stride >= 1, CFP_EINVAL, "cfp_points_compact: stride must be at least 1");
  CFP_REQUIRE(cap >= 1, CFP_EINVAL, "cfp_points_compact: cap must be at least 1");
  CFP_REQUIRE(z_near < z_far, CFP_EINVAL, "cfp_points_compact: empty depth range");
  CFP_REQUIRE((normals != nullptr) == (out_normals != nullptr), CFP_EINVAL,
              "cfp_points_compact: normals and out_normals must be given together");
  if (unc) {
    CFP_REQUIRE(Hu > 0 && Wu > 0 && (long long)Hu * Wu < (1ll << 31), CFP_ESHAPE, "cfp_points_compact: non-positive dimension (uncertainty plane)");
    CFP_REQUIRE(unc_stride >= 0, CFP_EINVAL, "cfp_points_compact: negative uncertainty image stride");
    CFP_REQUIRE(unc_lo <= unc_hi, CFP_EINVAL, "cfp_points_compact: empty uncertainty interval");      // false for NaN too
  }
  CFP_REQUIRE(ws_bytes >= cfp_points_compact_ws_bytes(B, H, W, stride), CFP_EINVAL, "cfp_points_compact: workspace too small");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, CFP_EINVAL, "cfp_points_compact: workspace must be 8-byte aligned");
  CompP p;
  p.u = met_params(unc, nullptr, unc ? Hu : H, unc ? Wu : W, H, W, B, unc && (Hu != H || Wu != W) ? 1 : 0, 0, 0.f, 0.f);
  p.points = points; p.normals = normals; p.unc_stride = unc_stride; p.has_unc = unc ? 1 : 0;
  p.Wc = (W + stride - 1) / stride;
  p.N = (int)comp_candidates(H, W, stride);
  p.nchunks = (p.N + kChunk - 1) / kChunk;
  p.stride = stride; p.cap = cap;
  p.z_near = z_near; p.z_far = z_far; p.unc_lo = unc_lo; p.unc_hi = unc_hi;
  p.out_points = out_points; p.out_normals = out_normals; p.out_index = out_index; p.counts = counts; p.ws = reinterpret_cast<int*>(ws);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(cdiv(p.nchunks, 4), B);
  hipLaunchKernelGGL(compact_count_kernel, grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL(chunk_scan_kernel, dim3(B), dim3(256), 0, s, p.ws, counts, p.nchunks);
  if (normals) hipLaunchKernelGGL(compact_scatter_kernel<true>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(compact_scatter_kernel<false>, grid, dim3(256), 0, s, p);
  return cfp_check_launch("cfp_points_compact");
}
