// The map out of the volume: the zero crossings of F along the edges of the voxel lattice, each a world-frame point with a normal, a std
// and the index of its edge (cfp_tsdf_surface; the definition is in include/cfpnet_hip.h next to cfp_tsdf_raycast).
//
// Candidates are the edges e = 3 * n + a in ascending order: voxel-major like the volume itself, then the axis.  The scheme is that of
// cfp_points_compact (pointcloud.hip): a wave owns a chunk of 256 consecutive voxels, 64 contiguous ones per step; no atomics, so the
// order and every bit of the result are a function of the volume alone:
//   1. count    per (image, chunk): popcounts of the three per-axis ballots -> workspace.  This pass IS a stream of the volume: x along
//               the lanes, (F, Wt) as one float2 per lane, 512 contiguous bytes per wave.  The +x neighbour is the next lane's value
//               (one more load for the last lane), the +y and +z neighbours are coalesced loads of rows that are centres a little later.
//   2. scan     in two levels, because a 256^3 volume has 65 536 chunks and one workgroup walking over them all took longer than the
//               count pass: a workgroup per tile of 256 chunks scans its tile in place and leaves the tile's total; chunk_scan.h then
//               scans the tile totals per image, the grand total -> counts[b]
//   3. scatter  a chunk whose count is 0 -- nearly all of a real map -- returns after three words; the others evaluate the predicate
//               again.  rank = tile offset + chunk offset + kept edges of the earlier steps + kept edges of the lanes below over the
//               three masks + the lane's own lower axes.  The 12 neighbour reads of a normal happen only at a kept edge.
// Every word of the workspace is written before it is read, so nothing is zeroed.
#include "common.h"
#include "chunk_scan.h"

#include <cmath>

namespace {

constexpr int kSteps = 4;                             // steps of 64 voxels per wave
constexpr int kChunk = 64 * kSteps;                   // voxels per chunk (one wave)
constexpr int kTile = 256;                            // chunks per tile of the scan's first level (one workgroup, a chunk per thread)

struct SurfP {
  const float2* volume;
  int Dx, Dy, Dz, nvox, nchunks, ntiles, cap;
  FastDiv div_x, div_xy;
  float ox, oy, oz, voxel, w_min, max_jump;
  float* points; float* normals; float* std; int* index; int* counts;
  int* ws; int* tiles;                                // [B][nchunks] chunk counts / offsets within the tile, [B][ntiles] tile totals / offsets
};

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }      // false for NaN

// the edge from a voxel holding a to its neighbour holding q: both observed, F changes sign (-0 is non-negative, NaN never crosses).
// Bitwise on purpose: short-circuit tests become a chain of branches, and every branch between two loads keeps the second from being issued
__device__ __forceinline__ bool surf_kept(const SurfP& p, const float2 a, const float2 q) {
  return (a.y > 0.f) & (q.y > 0.f) & (a.y >= p.w_min) & (q.y >= p.w_min) & (((a.x < 0.f) & (q.x >= 0.f)) | ((a.x >= 0.f) & (q.x < 0.f))) &
         (fabsf(a.x - q.x) <= p.max_jump);
}

struct SurfStep {                                     // one voxel per lane: its index, (F, Wt) of it and of its +x, +y, +z neighbours
  int n, i, j, k;
  float2 c, qx, qy, qz;
  bool hx, hy, hz;                                    // the neighbour is in the grid
  bool kx, ky, kz;                                    // the edge is kept
};

// The loads of a step, all issued before anything waits for one: no branch but the last lane's.  A voxel or neighbour outside the grid
// reads the last voxel instead (h* say so); qx is filled in by surf_eval.
__device__ __forceinline__ void surf_load(const SurfP& p, const float2* __restrict__ vol, int n, int lane, SurfStep& s) {
  const bool in = n < p.nvox;
  const int nc = min(n, p.nvox - 1);
  const unsigned k = fd_div((unsigned)nc, p.div_xy), r = (unsigned)nc - k * p.div_xy.d;
  const unsigned j = fd_div(r, p.div_x), i = r - j * p.div_x.d;
  s.n = n; s.i = (int)i; s.j = (int)j; s.k = (int)k;
  s.hx = in & (s.i + 1 < p.Dx); s.hy = in & (s.j + 1 < p.Dy); s.hz = in & (s.k + 1 < p.Dz);      // hx: n + 1 is in this row, so in the grid
  s.c = vol[nc];
  s.qy = vol[s.hy ? nc + p.Dx : nc];
  s.qz = vol[s.hz ? nc + (int)p.div_xy.d : nc];
  s.qx = make_float2(1.f, 0.f);                       // not s.c: a copy would wait for that load before the next step's are issued
  if (lane == 63) s.qx = vol[s.hx ? nc + 1 : nc];
}

// call with the whole wave: the +x neighbour travels between lanes
__device__ __forceinline__ void surf_eval(const SurfP& p, int lane, SurfStep& s) {
  const float nx = __shfl_down(s.c.x, 1), ny = __shfl_down(s.c.y, 1);
  if (lane != 63) s.qx = make_float2(nx, ny);
  s.kx = s.hx & surf_kept(p, s.c, s.qx);
  s.ky = s.hy & surf_kept(p, s.c, s.qy);
  s.kz = s.hz & surf_kept(p, s.c, s.qz);
}

__global__ __launch_bounds__(256) void surface_count_kernel(SurfP p) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= p.nchunks) return;                                 // wave-uniform
  const float2* vol = p.volume + (long long)b * p.nvox;
  SurfStep s[kSteps];
#pragma unroll
  for (int st = 0; st < kSteps; ++st) surf_load(p, vol, chunk * kChunk + st * 64 + lane, lane, s[st]);      // 13 loads in flight per lane
  int cnt = 0;
#pragma unroll
  for (int st = 0; st < kSteps; ++st) {
    surf_eval(p, lane, s[st]);
    cnt += __popcll(__ballot(s[st].kx)) + __popcll(__ballot(s[st].ky)) + __popcll(__ballot(s[st].kz));
  }
  if (lane == 0) p.ws[(long long)b * p.nchunks + chunk] = cnt;
}

// first level of the scan: exclusive scan of one tile's chunk counts in place, the tile's total -> tiles
__global__ __launch_bounds__(kTile) void surface_tile_scan_kernel(SurfP p) {
  __shared__ int s[2][kTile];
  const int b = blockIdx.y, t = threadIdx.x, c = blockIdx.x * kTile + t;
  int* w = p.ws + (long long)b * p.nchunks;
  const int v = c < p.nchunks ? w[c] : 0;
  s[0][t] = v;
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < kTile; o <<= 1) {                           // inclusive Hillis-Steele scan
    s[cur ^ 1][t] = s[cur][t] + (t >= o ? s[cur][t - o] : 0);
    cur ^= 1;
    __syncthreads();
  }
  if (c < p.nchunks) w[c] = s[cur][t] - v;
  if (t == kTile - 1) p.tiles[(long long)b * p.ntiles + blockIdx.x] = s[cur][kTile - 1];
}

// the central differences of F at voxel n = (i, j, k): false unless the six neighbours are in the grid with Wt > 0
__device__ __forceinline__ bool surf_gradient(const SurfP& p, const float2* __restrict__ vol, int n, int i, int j, int k, float* g) {
  const bool in = i >= 1 && i + 1 < p.Dx && j >= 1 && j + 1 < p.Dy && k >= 1 && k + 1 < p.Dz;
  g[0] = g[1] = g[2] = 0.f;
  if (!in) return false;
  const int sy = p.Dx, sz = (int)p.div_xy.d;
  const float2 x0 = vol[n - 1], x1 = vol[n + 1], y0 = vol[n - sy], y1 = vol[n + sy], z0 = vol[n - sz], z1 = vol[n + sz];
  g[0] = x1.x - x0.x; g[1] = y1.x - y0.x; g[2] = z1.x - z0.x;
  return x0.y > 0.f && x1.y > 0.f && y0.y > 0.f && y1.y > 0.f && z0.y > 0.f && z1.y > 0.f;
}

template <bool NORMALS>
__global__ __launch_bounds__(256) void surface_scatter_kernel(SurfP p) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= p.nchunks) return;                                 // wave-uniform
  const int* w = p.ws + (long long)b * p.nchunks;
  const int* tiles = p.tiles + (long long)b * p.ntiles;
  const int tile = chunk / kTile, off = tiles[tile];
  int base = off + w[chunk];
  const int next = (chunk + 1) % kTile != 0 && chunk + 1 < p.nchunks ? off + w[chunk + 1] : (tile + 1 < p.ntiles ? tiles[tile + 1] : p.counts[b]);
  if (next == base || base >= p.cap) return;                      // no crossing in this chunk, or everything from here on is beyond the capacity
  const float2* vol = p.volume + (long long)b * p.nvox;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 1
  for (int st = 0; st < kSteps; ++st) {
    SurfStep s;
    surf_load(p, vol, chunk * kChunk + st * 64 + lane, lane, s);
    surf_eval(p, lane, s);
    const unsigned long long b0 = __ballot(s.kx), b1 = __ballot(s.ky), b2 = __ballot(s.kz);
    int row = base + __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below);
    base += __popcll(b0) + __popcll(b1) + __popcll(b2);
    const int mask = (int)s.kx | ((int)s.ky << 1) | ((int)s.kz << 2);
#pragma unroll 1
    for (int a = 0; a < 3; ++a) {
      if (!((mask >> a) & 1)) continue;
      if (row < p.cap) {
        const float2 q = a == 0 ? s.qx : (a == 1 ? s.qy : s.qz);
        const float t = s.c.x / (s.c.x - q.x);
        const float X = p.ox + p.voxel * (a == 0 ? (float)s.i + t : (float)s.i);
        const float Y = p.oy + p.voxel * (a == 1 ? (float)s.j + t : (float)s.j);
        const float Z = p.oz + p.voxel * (a == 2 ? (float)s.k + t : (float)s.k);
        const long long dst = (long long)b * p.cap + row;
        p.points[dst * 3] = X; p.points[dst * 3 + 1] = Y; p.points[dst * 3 + 2] = Z;
        p.index[dst] = 3 * s.n + a;
        const float h = 1.f - t;
        if (p.std) p.std[dst] = 1.f / sqrtf(h * s.c.y + t * q.y);
        if constexpr (NORMALS) {
          float gp[3], gq[3];
          const int dn = a == 0 ? 1 : (a == 1 ? p.Dx : (int)p.div_xy.d);
          bool ok = surf_gradient(p, vol, s.n, s.i, s.j, s.k, gp);
          ok = surf_gradient(p, vol, s.n + dn, s.i + (a == 0), s.j + (a == 1), s.k + (a == 2), gq) && ok;
          const float gx = h * gp[0] + t * gq[0], gy = h * gp[1] + t * gq[1], gz = h * gp[2] + t * gq[2];
          const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
          ok = ok && len > 0.f && finitef(len);
          p.normals[dst * 3] = ok ? gx / len : NAN; p.normals[dst * 3 + 1] = ok ? gy / len : NAN; p.normals[dst * 3 + 2] = ok ? gz / len : NAN;
        }
      }
      ++row;
    }
  }
}

// voxels per image, 0 if the arguments make no sense or an edge index 3 * n + a would not fit an int32
long long surf_voxels(int Dx, int Dy, int Dz) {
  if (Dx <= 0 || Dy <= 0 || Dz <= 0) return 0;
  if ((long long)Dx * Dy >= (1ll << 31)) return 0;
  const long long n = (long long)Dx * Dy * Dz;                    // < 2^62
  return 3 * n < (1ll << 31) ? n : 0;
}

}  // namespace

extern "C" size_t cfp_tsdf_surface_ws_bytes(int B, int Dx, int Dy, int Dz) {
  const long long n = surf_voxels(Dx, Dy, Dz);
  if (B <= 0 || B > 65535 || n <= 0) return 0;
  const size_t nchunks = (size_t)((n + kChunk - 1) / kChunk);
  const size_t ints = (size_t)B * (nchunks + (nchunks + kTile - 1) / kTile);                // a count per chunk, a total per tile of chunks
  return ((ints + 1) / 2) * 8;
}

extern "C" int cfp_tsdf_surface(const float* volume, int Dx, int Dy, int Dz, int B, float ox, float oy, float oz, float voxel, float w_min,
                                float max_jump, int cap, float* points, float* normals, float* std, int* index, int* counts, void* ws,
                                size_t ws_bytes, cfp_stream_t stream) {
  CFP_REQUIRE(volume && counts && ws, CFP_EINVAL, "cfp_tsdf_surface: null pointer");
  CFP_REQUIRE((points != nullptr) == (index != nullptr), CFP_EINVAL, "cfp_tsdf_surface: points and index must be given together");
  CFP_REQUIRE(points || (!normals && !std), CFP_EINVAL, "cfp_tsdf_surface: normals and std need points");
  CFP_REQUIRE(B > 0 && Dx > 0 && Dy > 0 && Dz > 0, CFP_ESHAPE, "cfp_tsdf_surface: non-positive dimension");
  CFP_REQUIRE(surf_voxels(Dx, Dy, Dz) > 0 && B <= 65535, CFP_ESHAPE,
              "cfp_tsdf_surface: volume or batch too large (an edge index 3 * Dx * Dy * Dz must fit an int32)");
  CFP_REQUIRE(std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz), CFP_EINVAL, "cfp_tsdf_surface: origin must be finite");
  CFP_REQUIRE(voxel > 0.f && voxel < INFINITY, CFP_EINVAL, "cfp_tsdf_surface: voxel must be positive and finite");
  CFP_REQUIRE(w_min >= 0.f, CFP_EINVAL, "cfp_tsdf_surface: w_min must not be negative");              // false for NaN
  CFP_REQUIRE(max_jump >= 0.f, CFP_EINVAL, "cfp_tsdf_surface: max_jump must not be negative");        // false for NaN; +inf: no filter
  CFP_REQUIRE(!points || cap >= 1, CFP_EINVAL, "cfp_tsdf_surface: cap must be at least 1");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(volume) & 7) == 0, CFP_EINVAL, "cfp_tsdf_surface: volume must be 8-byte aligned");
  CFP_REQUIRE(ws_bytes >= cfp_tsdf_surface_ws_bytes(B, Dx, Dy, Dz), CFP_EINVAL, "cfp_tsdf_surface: workspace too small");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, CFP_EINVAL, "cfp_tsdf_surface: workspace must be 8-byte aligned");
  SurfP p;
  p.volume = reinterpret_cast<const float2*>(volume);
  p.Dx = Dx; p.Dy = Dy; p.Dz = Dz;
  p.nvox = (int)surf_voxels(Dx, Dy, Dz);
  p.nchunks = (p.nvox + kChunk - 1) / kChunk;
  p.ntiles = (p.nchunks + kTile - 1) / kTile;
  p.cap = cap;
  p.div_x = make_fastdiv((unsigned)Dx); p.div_xy = make_fastdiv((unsigned)Dx * (unsigned)Dy);
  p.ox = ox; p.oy = oy; p.oz = oz; p.voxel = voxel; p.w_min = w_min; p.max_jump = max_jump;
  p.points = points; p.normals = normals; p.std = std; p.index = index; p.counts = counts;
  p.ws = reinterpret_cast<int*>(ws); p.tiles = p.ws + (long long)B * p.nchunks;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(cdiv(p.nchunks, 4), B);
  hipLaunchKernelGGL(surface_count_kernel, grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL(surface_tile_scan_kernel, dim3(p.ntiles, B), dim3(kTile), 0, s, p);
  hipLaunchKernelGGL(chunk_scan_kernel, dim3(B), dim3(256), 0, s, p.tiles, counts, p.ntiles);
  if (points) {
    if (normals) hipLaunchKernelGGL(surface_scatter_kernel<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(surface_scatter_kernel<false>, grid, dim3(256), 0, s, p);
  }
  return cfp_check_launch("cfp_tsdf_surface");
}
