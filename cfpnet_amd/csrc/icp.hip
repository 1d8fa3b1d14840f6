// Camera tracking on the device: one Gauss-Newton iteration of dense point-to-plane ICP of a frame (the prediction and its std) against a
// model map (depth, normals and std in the model camera: a cfp_tsdf_raycast, or the previous frame's cfp_depth_unproject), per image
// (cfp_icp_step).  The definition is in include/cfpnet_hip.h; the depth at a source pixel is met_pred of metrics_pred.h in mode 0, the
// value cfp_depth_unproject back-projects, bit for bit, and the std that travels with it is met_plane.
//
// Accumulate.  One thread per pixel of the stride grid, x along the lanes, grid-striding over the image: neighbouring lanes project to
// neighbouring model pixels, so the depth / normal / std gathers of a wave hit the same lines.  The pose and the two cameras are uniform
// per workgroup (scalar loads).  A pair's 30 terms are float32 products; each is added to a double accumulator of the thread, the
// threads are summed by a butterfly inside the wave and the four waves in order through LDS, and a workgroup leaves ONE row of 30
// doubles in the workspace.  The number of workgroups per image is a function of the shape alone, capped at kIcpBlocks.
//
// Finalize.  One 64-lane workgroup per image sums the rows in a fixed order (two rows per lane, then the butterfly); lane 0 solves the
// 6 x 6 system by LDL^T in double, refuses a step that is not constrained, composes exp(xi) with the pose, re-orthonormalises and
// writes the pose back as float32.  No atomics anywhere: two calls on the same inputs give identical bits.
#include "common.h"
#include "metrics_pred.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kIcpBlocks = 128;                       // workgroups per image at most: the finalize reads two rows per lane (256 and four measured slower)
constexpr int kIcpTerms = 30;                         // 21 of A (upper triangle, by rows), 6 of g, sum w r r, sum w, pairs
constexpr long long kMaxDim = 1ll << 24;              // a row or column index is used as a float: exact below 2^24

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }      // false for NaN

struct IcpP {
  MetP m;                                             // the depth: pred, Hp, Wp, H, W, interpolate, mode 0, lo, hi
  MetP u;                                             // the std plane as met_plane reads it (pred = null: none)
  long long std_stride;
  float std_floor;
  const float* src_normals; float cos_min;
  const float* K_src; const float* K_mdl;
  const float* mdl_depth; const float* mdl_normals; const float* mdl_std;
  int Hm, Wm;
  int stride, ws, hs;                                 // the stride grid is hs x ws
  FastDiv div_ws;
  float z_near, dist2;
  const float* T;
  int* index;
  double* partial;
};

__device__ __forceinline__ bool normal_ok(float x, float y, float z) {
  return finitef(x) && finitef(y) && finitef(z) && (x * x + y * y) + z * z > 0.25f;
}

// PI: the prediction is blended to the grid (met_pred's interpolate); SI: 0 no std plane, 1 read directly, 2 blended (met_plane's).  As
// template arguments they leave each instance the uniform state of its own path only, which is what keeps the scalar file from spilling.
template <int PI, int SI>
__global__ __launch_bounds__(256) void icp_accumulate_kernel(IcpP p) {
  __shared__ double red[4][kIcpTerms];
  MetP m = p.m, su = p.u;
  m.interpolate = PI; m.mode = 0; su.interpolate = SI == 2 ? 1 : 0;
  su.H = m.H; su.W = m.W;                             // the same grid: one row / column split serves both blends
  const int b = blockIdx.y;
  const float* pb = m.pred + (long long)b * m.Hp * m.Wp;
  const float* sb = SI ? p.u.pred + (long long)b * p.std_stride : nullptr;
  const float* nb = p.src_normals ? p.src_normals + (long long)b * m.H * m.W * 3 : nullptr;
  const long long mhw = (long long)p.Hm * p.Wm;
  const float* md = p.mdl_depth + (long long)b * mhw;
  const float* mn = p.mdl_normals + (long long)b * mhw * 3;
  const float* ms = p.mdl_std ? p.mdl_std + (long long)b * mhw : nullptr;
  int* ib = p.index ? p.index + (long long)b * m.H * m.W : nullptr;
  // the pose and the two cameras go through LDS into vector registers: as scalars they, the pointers and the sizes of the two blends
  // are more uniform state than the scalar file holds
  __shared__ float cam[24];
  if (threadIdx.x < 12) cam[threadIdx.x] = p.T[b * 12 + threadIdx.x];
  else if (threadIdx.x < 16) cam[threadIdx.x] = p.K_src[b * 4 + (threadIdx.x - 12)];
  else if (threadIdx.x < 20) cam[threadIdx.x] = p.K_mdl[b * 4 + (threadIdx.x - 16)];
  else if (threadIdx.x == 20) { cam[20] = p.z_near; cam[21] = p.dist2; cam[22] = p.std_floor; cam[23] = p.cos_min; }
  __syncthreads();
  float T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = cam[e];
  const float fx = cam[12], fy = cam[13], cx = cam[14], cy = cam[15];
  const float fxm = cam[16], fym = cam[17], cxm = cam[18], cym = cam[19];
  const float z_near = cam[20], dist2 = cam[21], std_floor = cam[22], cos_min = cam[23];
  double acc[kIcpTerms];
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) acc[k] = 0.0;
  const unsigned n = (unsigned)p.ws * (unsigned)p.hs;              // < 2^31
  for (long long i64 = (long long)blockIdx.x * 256 + threadIdx.x; i64 < n; i64 += (long long)gridDim.x * 256) {
    const unsigned i = (unsigned)i64;
    const unsigned ys = fd_div(i, p.div_ws), xs = i - ys * p.div_ws.d;
    const int x = (int)xs * p.stride, y = (int)ys * p.stride;
    const int pix = y * m.W + x;
    // No branch up to the sums: every test narrows `ok`, every gather is issued (at pixel 0 of the model map where there is no pair), so
    // the loads of a pixel are independent of each other and in flight together.
    const float d = met_pred(m, pb, pix);
    bool ok = finitef(d) && d > 0.f;
    const float rx = ((float)x - cx) / fx, ry = ((float)y - cy) / fy;
    const float X = rx * d, Y = ry * d, Z = d;
    const float Xp = (T[0] * X + T[1] * Y) + T[2] * Z + T[3];
    const float Yp = (T[4] * X + T[5] * Y) + T[6] * Z + T[7];
    const float Zp = (T[8] * X + T[9] * Y) + T[10] * Z + T[11];
    ok = ok && finitef(Zp) && Zp >= z_near;
    const float uu = fxm * (Xp / Zp) + cxm, vv = fym * (Yp / Zp) + cym;
    float col = floorf(uu + 0.5f), row = floorf(vv + 0.5f);
    ok = ok && col >= 0.f && col < (float)p.Wm && row >= 0.f && row < (float)p.Hm;      // on the float values; NaN fails
    col = ok ? col : 0.f; row = ok ? row : 0.f;
    const int mi = (int)row * p.Wm + (int)col;
    const float dm = md[mi];
    const float nx = mn[(long long)mi * 3], ny = mn[(long long)mi * 3 + 1], nz = mn[(long long)mi * 3 + 2];
    ok = ok && finitef(dm) && dm > 0.f && normal_ok(nx, ny, nz);
    const float Qx = (col - cxm) / fxm * dm, Qy = (row - cym) / fym * dm;
    const float Dx = Xp - Qx, Dy = Yp - Qy, Dz = Zp - dm;
    ok = ok && (Dx * Dx + Dy * Dy) + Dz * Dz <= dist2;
    if (nb) {
      const float sx = nb[(long long)pix * 3], sy = nb[(long long)pix * 3 + 1], sz = nb[(long long)pix * 3 + 2];
      const float qx = (T[0] * sx + T[1] * sy) + T[2] * sz;
      const float qy = (T[4] * sx + T[5] * sy) + T[6] * sz;
      const float qz = (T[8] * sx + T[9] * sy) + T[10] * sz;
      ok = ok && normal_ok(sx, sy, sz) && (qx * nx + qy * ny) + qz * nz >= cos_min;
    }
    float w = 1.f;
    if (sb || ms) {
      float sf = std_floor, sm = 0.f;
      if (sb) {
        const float sd = met_plane(su, sb, pix);
        sf = sd > std_floor ? sd : std_floor;                  // a NaN std takes the floor
      }
      if (ms) {
        const float v = ms[mi];
        sm = finitef(v) ? v : 0.f;
      }
      w = 1.f / (sf * sf + sm * sm);
      ok = ok && w > 0.f && w < INFINITY;                          // an infinite std observes nothing
    }
    const float r = (nx * Dx + ny * Dy) + nz * Dz;
    const float J[6] = {Yp * nz - Zp * ny, Zp * nx - Xp * nz, Xp * ny - Yp * nx, nx, ny, nz};
    const int pair = ok ? mi : -1;
    if (ib) {
      if (p.stride == 1) {
        ib[pix] = pair;
      } else {                                                      // the thread owns the stride x stride cell below and right of its pixel
        const int x1 = min(x + p.stride, m.W), y1 = min(y + p.stride, m.H);
        for (int yy = y; yy < y1; ++yy)
          for (int xx = x; xx < x1; ++xx) ib[yy * m.W + xx] = (yy == y && xx == x) ? pair : -1;
      }
    }
    if (pair < 0) continue;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const float wj = w * J[a];
#pragma unroll
      for (int c = a; c < 6; ++c) acc[k++] += (double)(wj * J[c]);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] += (double)((w * J[a]) * r);
    acc[27] += (double)((w * r) * r);
    acc[28] += (double)w;
    acc[29] += 1.0;
  }
  // fixed-order reduction: butterfly inside the wave, then the four waves in order
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) {
    double a = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = a;
  }
  __syncthreads();
  if (threadIdx.x < kIcpTerms)
    p.partial[((long long)b * gridDim.x + blockIdx.x) * kIcpTerms + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

struct IcpF {
  const double* partial; int nblocks;
  int min_pairs; double min_pivot;
  float* T; const float* T_ref; float* T_world;
  double* sums; float* stats;
};

// A xi = -g by LDL^T; false when a pivot is not above min_pivot * (largest diagonal entry of A)
__device__ bool icp_solve(const double* s, double min_pivot, double* xi) {
  double A[6][6], L[6][6], D[6];
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = a; c < 6; ++c) { A[a][c] = s[k]; A[c][a] = s[k]; ++k; }
  double top = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) top = fmax(top, A[a][a]);
  const double thresh = min_pivot * top;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double dj = A[j][j];
#pragma unroll
    for (int q = 0; q < j; ++q) dj -= L[j][q] * L[j][q] * D[q];
    if (!(dj > thresh) || !(dj > 0.0)) ok = false;
    D[j] = dj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int q = 0; q < j; ++q) v -= L[i][q] * L[j][q] * D[q];
      L[i][j] = v / dj;
    }
  }
  if (!ok) return false;
  double z[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = -s[21 + i];
#pragma unroll
    for (int q = 0; q < i; ++q) v -= L[i][q] * z[q];
    z[i] = v;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = z[i] / D[i];
#pragma unroll
    for (int q = i + 1; q < 6; ++q) v -= L[q][i] * xi[q];
    xi[i] = v;
  }
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) fin = fin && (fabs(xi[i]) < (double)INFINITY);
  return fin;
}

__global__ __launch_bounds__(64) void icp_finalize_kernel(IcpF p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  static_assert(kIcpBlocks <= 128, "two partial rows per lane");
  // every load is issued, at a clamped row, and the select comes after it: behind a branch per row the 60 loads of a lane went out one
  // after the other, each waiting for the last
  const int r0 = min(lane, p.nblocks - 1), r1 = min(lane + 64, p.nblocks - 1);
  const double* q0 = p.partial + ((long long)b * p.nblocks + r0) * kIcpTerms;
  const double* q1 = p.partial + ((long long)b * p.nblocks + r1) * kIcpTerms;
  double s[kIcpTerms], v0[kIcpTerms], v1[kIcpTerms];
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) { v0[k] = q0[k]; v1[k] = q1[k]; }
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) {               // the order of the additions is fixed
    double a = lane < p.nblocks ? v0[k] : 0.0;
    if (lane + 64 < p.nblocks) a += v1[k];
    s[k] = a;
  }
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
  }
  if (lane != 0) return;
  if (p.sums) {
#pragma unroll
    for (int k = 0; k < kIcpTerms; ++k) p.sums[b * 32 + k] = s[k];
    p.sums[b * 32 + 30] = 0.0; p.sums[b * 32 + 31] = 0.0;
  }
  float* T = p.T + b * 12;
  double xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const bool accepted = s[29] >= (double)p.min_pairs && icp_solve(s, p.min_pivot, xi);
  double wn = 0.0, vn = 0.0;
  if (accepted) {
    const double ox = xi[0], oy = xi[1], oz = xi[2];
    const double th2 = (ox * ox + oy * oy) + oz * oz;
    double ca = 1.0, cb = 0.5, cc = 1.0 / 6.0;
    if (!(th2 < 1e-12)) {
      const double th = sqrt(th2);
      ca = sin(th) / th; cb = (1.0 - cos(th)) / th2; cc = (th - sin(th)) / (th2 * th);
    }
    const double Kx[3][3] = {{0.0, -oz, oy}, {oz, 0.0, -ox}, {-oy, ox, 0.0}};
    double K2[3][3], Re[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        K2[i][j] = (Kx[i][0] * Kx[0][j] + Kx[i][1] * Kx[1][j]) + Kx[i][2] * Kx[2][j];
        const double e = i == j ? 1.0 : 0.0;
        Re[i][j] = e + ca * Kx[i][j] + cb * K2[i][j];
        V[i][j] = e + cb * Kx[i][j] + cc * K2[i][j];
      }
    double te[3], M[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i) te[i] = (V[i][0] * xi[3] + V[i][1] * xi[4]) + V[i][2] * xi[5];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        M[i][j] = (Re[i][0] * (double)T[j] + Re[i][1] * (double)T[4 + j]) + Re[i][2] * (double)T[8 + j];
      M[i][3] += te[i];
    }
    // Gram-Schmidt on the rows: row 0, row 1, row 2 = row 0 x row 1
    const double l0 = sqrt((M[0][0] * M[0][0] + M[0][1] * M[0][1]) + M[0][2] * M[0][2]);
    const double a0 = M[0][0] / l0, a1 = M[0][1] / l0, a2 = M[0][2] / l0;
    const double dp = (a0 * M[1][0] + a1 * M[1][1]) + a2 * M[1][2];
    const double e0 = M[1][0] - dp * a0, e1 = M[1][1] - dp * a1, e2 = M[1][2] - dp * a2;
    const double l1 = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    const double b0 = e0 / l1, b1 = e1 / l1, b2 = e2 / l1;
    T[0] = (float)a0; T[1] = (float)a1; T[2] = (float)a2; T[3] = (float)M[0][3];
    T[4] = (float)b0; T[5] = (float)b1; T[6] = (float)b2; T[7] = (float)M[1][3];
    T[8] = (float)(a1 * b2 - a2 * b1); T[9] = (float)(a2 * b0 - a0 * b2); T[10] = (float)(a0 * b1 - a1 * b0); T[11] = (float)M[2][3];
    wn = sqrt(th2);
    vn = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
  }
  if (p.T_world) {                                    // camera-from-world of the current frame: R^T R_ref, R^T (t_ref - t)
    const float* Tr = p.T_ref + b * 12;
    float* Tw = p.T_world + b * 12;
    const double dx = (double)Tr[3] - (double)T[3], dy = (double)Tr[7] - (double)T[7], dz = (double)Tr[11] - (double)T[11];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        Tw[i * 4 + j] = (float)(((double)T[i] * (double)Tr[j] + (double)T[4 + i] * (double)Tr[4 + j]) + (double)T[8 + i] * (double)Tr[8 + j]);
      Tw[i * 4 + 3] = (float)(((double)T[i] * dx + (double)T[4 + i] * dy) + (double)T[8 + i] * dz);
    }
  }
  float* st = p.stats + b * 6;
  st[0] = (float)s[29]; st[1] = (float)s[28];
  st[2] = s[29] > 0.0 ? sqrtf((float)(s[27] / s[28])) : NAN;
  st[3] = (float)wn; st[4] = (float)vn; st[5] = accepted ? 1.f : 0.f;
}

bool pos_finite(float v) { return v > 0.f && v < INFINITY; }      // false for NaN

int icp_blocks(int H, int W, int stride) {
  const long long n = (long long)cdiv(H, stride) * cdiv(W, stride);
  return (int)std::min<long long>((n + 255) / 256, kIcpBlocks);
}

}  // namespace

extern "C" size_t cfp_icp_ws_bytes(int B, int H, int W, int stride) {
  if (B <= 0 || H <= 0 || W <= 0 || stride < 1) return 0;
  return (size_t)B * icp_blocks(H, W, stride) * kIcpTerms * sizeof(double);
}

extern "C" int cfp_icp_step(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi, const float* std,
                            int Hu, int Wu, long long std_stride, float std_floor, const float* src_normals, float cos_min,
                            const float* K_src, const float* mdl_depth, const float* mdl_normals, const float* mdl_std, int Hm, int Wm,
                            const float* K_mdl, int stride, float z_near, float dist_max, int min_pairs, float min_pivot, float* T,
                            const float* T_ref, float* T_world, int* index, double* sums, float* stats, void* ws, size_t ws_bytes,
                            cfp_stream_t stream) {
  CFP_REQUIRE(pred && K_src && mdl_depth && mdl_normals && K_mdl && T && stats && ws, CFP_EINVAL, "cfp_icp_step: null pointer");
  CFP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0 && Hm > 0 && Wm > 0, CFP_ESHAPE, "cfp_icp_step: non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) - 256 && (long long)Hp * Wp < (1ll << 31) && H <= kMaxDim && W <= kMaxDim && B <= 65535,
              CFP_ESHAPE, "cfp_icp_step: image or batch too large");
  CFP_REQUIRE((long long)Hm * Wm < (1ll << 31) - 256 && Hm <= kMaxDim && Wm <= kMaxDim, CFP_ESHAPE, "cfp_icp_step: model map too large");
  CFP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, "cfp_icp_step: sizes differ and interpolate is off");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, "cfp_icp_step: empty depth range");
  if (std) {
    CFP_REQUIRE(Hu > 0 && Wu > 0, CFP_ESHAPE, "cfp_icp_step: non-positive dimension (std)");
    CFP_REQUIRE((long long)Hu * Wu < (1ll << 31), CFP_ESHAPE, "cfp_icp_step: std plane too large");
    CFP_REQUIRE(std_stride >= 0, CFP_EINVAL, "cfp_icp_step: negative std image stride");
  }
  CFP_REQUIRE(stride >= 1, CFP_EINVAL, "cfp_icp_step: stride must be at least 1");
  CFP_REQUIRE(pos_finite(std_floor), CFP_EINVAL, "cfp_icp_step: std_floor must be positive and finite");
  CFP_REQUIRE(pos_finite(z_near), CFP_EINVAL, "cfp_icp_step: z_near must be positive and finite");
  CFP_REQUIRE(pos_finite(dist_max) && pos_finite(dist_max * dist_max), CFP_EINVAL, "cfp_icp_step: dist_max must be positive and finite");
  CFP_REQUIRE(min_pivot >= 0.f && min_pivot < 1.f, CFP_EINVAL, "cfp_icp_step: min_pivot must lie in [0, 1)");
  CFP_REQUIRE(min_pairs >= 6, CFP_EINVAL, "cfp_icp_step: min_pairs must be at least 6");
  CFP_REQUIRE(cos_min >= -1.f && cos_min <= 1.f, CFP_EINVAL, "cfp_icp_step: cos_min must lie in [-1, 1]");
  CFP_REQUIRE((T_ref != nullptr) == (T_world != nullptr), CFP_EINVAL, "cfp_icp_step: T_ref and T_world are given together or not at all");
  CFP_REQUIRE(ws_bytes >= cfp_icp_ws_bytes(B, H, W, stride), CFP_EINVAL, "cfp_icp_step: workspace too small");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, CFP_EINVAL, "cfp_icp_step: workspace must be 8-byte aligned");
  CFP_REQUIRE(!sums || (reinterpret_cast<uintptr_t>(sums) & 7) == 0, CFP_EINVAL, "cfp_icp_step: sums must be 8-byte aligned");
  IcpP p;
  p.m = met_params(pred, nullptr, Hp, Wp, H, W, B, interpolate, 0, lo, hi);
  p.u = met_params(std, nullptr, std ? Hu : H, std ? Wu : W, H, W, B, std && (Hu != H || Wu != W) ? 1 : 0, 0, 0.f, 0.f);
  p.std_stride = std_stride; p.std_floor = std_floor;
  p.src_normals = src_normals; p.cos_min = cos_min;
  p.K_src = K_src; p.K_mdl = K_mdl;
  p.mdl_depth = mdl_depth; p.mdl_normals = mdl_normals; p.mdl_std = mdl_std;
  p.Hm = Hm; p.Wm = Wm;
  p.stride = stride; p.ws = cdiv(W, stride); p.hs = cdiv(H, stride);
  p.div_ws = make_fastdiv((unsigned)p.ws);
  p.z_near = z_near; p.dist2 = dist_max * dist_max;
  p.T = T;
  p.index = index;
  p.partial = reinterpret_cast<double*>(ws);
  IcpF f;
  f.partial = p.partial; f.nblocks = icp_blocks(H, W, stride);
  f.min_pairs = min_pairs; f.min_pivot = (double)min_pivot;
  f.T = T; f.T_ref = T_ref; f.T_world = T_world;
  f.sums = sums; f.stats = stats;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)f.nblocks, B);
  const int si = !std ? 0 : (p.u.interpolate ? 2 : 1);
#define CFP_ICP_LAUNCH(PI, SI) hipLaunchKernelGGL((icp_accumulate_kernel<PI, SI>), grid, dim3(256), 0, s, p)
  if (interpolate) {
    if (si == 0) CFP_ICP_LAUNCH(1, 0); else if (si == 1) CFP_ICP_LAUNCH(1, 1); else CFP_ICP_LAUNCH(1, 2);
  } else {
    if (si == 0) CFP_ICP_LAUNCH(0, 0); else if (si == 1) CFP_ICP_LAUNCH(0, 1); else CFP_ICP_LAUNCH(0, 2);
  }
#undef CFP_ICP_LAUNCH
  hipLaunchKernelGGL(icp_finalize_kernel, dim3(B), dim3(64), 0, s, f);
  return cfp_check_launch("cfp_icp_step");
}
