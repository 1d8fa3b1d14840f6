// What the two camera-tracking kernels share (icp.hip: point-to-plane; icp_rgb.hip: point-to-plane and photometric): the geometry of one
// pair, bit for bit the `Pair` of cfp_icp_step in include/cfpnet_hip.h, the fixed-order reduction of a workgroup's sums, the sum of the
// workgroups' rows, the LDL^T solve and the pose update of the finalize, and the host's argument checks.  Everything is forced inline, so
// each kernel compiles the same sequence of float32 operations it would hold on its own (the library is built without fused multiply-adds).
#pragma once
#include "common.h"
#include "metrics_pred.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace icp_core {

constexpr int kIcpBlocks = 128;                       // workgroups per image at most: the finalize reads two rows per lane (256 and four measured slower)
constexpr int kIcpTerms = 30;                         // 21 of A (upper triangle, by rows), 6 of g, sum w r r, sum w, pairs
constexpr long long kMaxDim = 1ll << 24;              // a row or column index is used as a float: exact below 2^24

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

struct IcpF {
  const double* partial; int nblocks;
  int min_pairs; double min_pivot;
  float* T; const float* T_ref; float* T_world;
  double* sums; float* stats;
};

#ifdef __HIPCC__
__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }      // false for NaN

__device__ __forceinline__ bool normal_ok(float x, float y, float z) {
  return finitef(x) && finitef(y) && finitef(z) && (x * x + y * y) + z * z > 0.25f;
}

// the pose, the two cameras and the four thresholds of image b, per thread
struct IcpCam {
  float T[12];
  float fx, fy, cx, cy, fxm, fym, cxm, cym;
  float z_near, dist2, std_floor, cos_min;
};

// The pose and the two cameras go through LDS (cam: 24 floats of the workgroup) into vector registers: as scalars they, the pointers and
// the sizes of the two blends are more uniform state than the scalar file holds.  Holds a barrier: every thread of the workgroup calls it.
__device__ __forceinline__ void icp_load_cam(const IcpP& p, int b, float* cam, IcpCam& c) {
  if (threadIdx.x < 12) cam[threadIdx.x] = p.T[b * 12 + threadIdx.x];
  else if (threadIdx.x < 16) cam[threadIdx.x] = p.K_src[b * 4 + (threadIdx.x - 12)];
  else if (threadIdx.x < 20) cam[threadIdx.x] = p.K_mdl[b * 4 + (threadIdx.x - 16)];
  else if (threadIdx.x == 20) { cam[20] = p.z_near; cam[21] = p.dist2; cam[22] = p.std_floor; cam[23] = p.cos_min; }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 12; ++e) c.T[e] = cam[e];
  c.fx = cam[12]; c.fy = cam[13]; c.cx = cam[14]; c.cy = cam[15];
  c.fxm = cam[16]; c.fym = cam[17]; c.cxm = cam[18]; c.cym = cam[19];
  c.z_near = cam[20]; c.dist2 = cam[21]; c.std_floor = cam[22]; c.cos_min = cam[23];
}

// the pointers of image b
struct IcpImg {
  const float* pb; const float* sb; const float* nb;
  const float* md; const float* mn; const float* ms;
};

template <int SI>
__device__ __forceinline__ IcpImg icp_image(const IcpP& p, const MetP& m, int b) {
  IcpImg g;
  g.pb = m.pred + (long long)b * m.Hp * m.Wp;
  g.sb = SI ? p.u.pred + (long long)b * p.std_stride : nullptr;
  g.nb = p.src_normals ? p.src_normals + (long long)b * m.H * m.W * 3 : nullptr;
  const long long mhw = (long long)p.Hm * p.Wm;
  g.md = p.mdl_depth + (long long)b * mhw;
  g.mn = p.mdl_normals + (long long)b * mhw * 3;
  g.ms = p.mdl_std ? p.mdl_std + (long long)b * mhw : nullptr;
  return g;
}

// one source pixel of the stride grid and what it is paired with
struct IcpPair {
  int x, y, pix;
  int mi;                                             // ym * Wm + xm, -1: no pair
  float u, v, Xp, Yp, Zp;                             // the projection and the moved point, unrounded
  float w, r, J[6];
};

// Pixel i of the stride grid.  No branch: every test narrows `ok`, every gather is issued (at pixel 0 of the model map where there is no
// pair), so the loads of a pixel are independent of each other and in flight together.
__device__ __forceinline__ void icp_pair(const IcpP& p, const MetP& m, const MetP& su, const IcpCam& c, const IcpImg& g, unsigned i,
                                         IcpPair& q) {
  const float* T = c.T;
  const unsigned ys = fd_div(i, p.div_ws), xs = i - ys * p.div_ws.d;
  const int x = (int)xs * p.stride, y = (int)ys * p.stride;
  const int pix = y * m.W + x;
  const float d = met_pred(m, g.pb, pix);
  bool ok = finitef(d) && d > 0.f;
  const float rx = ((float)x - c.cx) / c.fx, ry = ((float)y - c.cy) / c.fy;
  const float X = rx * d, Y = ry * d, Z = d;
  const float Xp = (T[0] * X + T[1] * Y) + T[2] * Z + T[3];
  const float Yp = (T[4] * X + T[5] * Y) + T[6] * Z + T[7];
  const float Zp = (T[8] * X + T[9] * Y) + T[10] * Z + T[11];
  ok = ok && finitef(Zp) && Zp >= c.z_near;
  const float uu = c.fxm * (Xp / Zp) + c.cxm, vv = c.fym * (Yp / Zp) + c.cym;
  float col = floorf(uu + 0.5f), row = floorf(vv + 0.5f);
  ok = ok && col >= 0.f && col < (float)p.Wm && row >= 0.f && row < (float)p.Hm;      // on the float values; NaN fails
  col = ok ? col : 0.f; row = ok ? row : 0.f;
  const int mi = (int)row * p.Wm + (int)col;
  const float dm = g.md[mi];
  const float nx = g.mn[(long long)mi * 3], ny = g.mn[(long long)mi * 3 + 1], nz = g.mn[(long long)mi * 3 + 2];
  ok = ok && finitef(dm) && dm > 0.f && normal_ok(nx, ny, nz);
  const float Qx = (col - c.cxm) / c.fxm * dm, Qy = (row - c.cym) / c.fym * dm;
  const float Dx = Xp - Qx, Dy = Yp - Qy, Dz = Zp - dm;
  ok = ok && (Dx * Dx + Dy * Dy) + Dz * Dz <= c.dist2;
  if (g.nb) {
    const float sx = g.nb[(long long)pix * 3], sy = g.nb[(long long)pix * 3 + 1], sz = g.nb[(long long)pix * 3 + 2];
    const float qx = (T[0] * sx + T[1] * sy) + T[2] * sz;
    const float qy = (T[4] * sx + T[5] * sy) + T[6] * sz;
    const float qz = (T[8] * sx + T[9] * sy) + T[10] * sz;
    ok = ok && normal_ok(sx, sy, sz) && (qx * nx + qy * ny) + qz * nz >= c.cos_min;
  }
  float w = 1.f;
  if (g.sb || g.ms) {
    float sf = c.std_floor, sm = 0.f;
    if (g.sb) {
      const float sd = met_plane(su, g.sb, pix);
      sf = sd > c.std_floor ? sd : c.std_floor;                    // a NaN std takes the floor
    }
    if (g.ms) {
      const float v = g.ms[mi];
      sm = finitef(v) ? v : 0.f;
    }
    w = 1.f / (sf * sf + sm * sm);
    ok = ok && w > 0.f && w < INFINITY;                              // an infinite std observes nothing
  }
  q.x = x; q.y = y; q.pix = pix;
  q.mi = ok ? mi : -1;
  q.u = uu; q.v = vv; q.Xp = Xp; q.Yp = Yp; q.Zp = Zp;
  q.w = w;
  q.r = (nx * Dx + ny * Dy) + nz * Dz;
  q.J[0] = Yp * nz - Zp * ny; q.J[1] = Zp * nx - Xp * nz; q.J[2] = Xp * ny - Yp * nx; q.J[3] = nx; q.J[4] = ny; q.J[5] = nz;
}

// A per-pixel output map [H,W] of image b: the thread owns the stride x stride cell below and right of its pixel, writes `value` at the
// pixel and `none` at the rest of the cell, so the map is fully written.
template <typename V>
__device__ __forceinline__ void icp_write_cell(V* ob, const IcpP& p, const MetP& m, const IcpPair& q, V value, V none) {
  if (p.stride == 1) {
    ob[q.pix] = value;
  } else {
    const int x1 = min(q.x + p.stride, m.W), y1 = min(q.y + p.stride, m.H);
    for (int yy = q.y; yy < y1; ++yy)
      for (int xx = q.x; xx < x1; ++xx) ob[yy * m.W + xx] = (yy == q.y && xx == q.x) ? value : none;
  }
}

// the 30 terms of one pair onto the thread's accumulators: float32 products, double sums
__device__ __forceinline__ void icp_add_terms(double* acc, float w, const float* J, float r) {
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

// fixed-order reduction of N accumulators over a workgroup of 256: butterfly inside the wave, then the four waves in order; `row` is the
// workgroup's row of N doubles in the workspace.  Holds a barrier.
template <int N>
__device__ __forceinline__ void icp_block_reduce(const double* acc, double (*red)[N], double* row) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double a = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = a;
  }
  __syncthreads();
  if (threadIdx.x < N) row[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// The finalize's sum of the workgroups' rows, 30 terms at a time, by one wave: lane l holds rows l and l + 64 (q0, q1 point at their
// terms; the rows are clamped by the caller), then the butterfly.  Every load is issued, at a clamped row, and the select comes after it:
// behind a branch per row the 60 loads of a lane went out one after the other, each waiting for the last.
__device__ __forceinline__ void icp_sum_rows(const double* q0, const double* q1, int lane, int nblocks, double* s) {
  static_assert(kIcpBlocks <= 128, "two partial rows per lane");
  double v0[kIcpTerms], v1[kIcpTerms];
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) { v0[k] = q0[k]; v1[k] = q1[k]; }
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) {               // the order of the additions is fixed
    double a = lane < nblocks ? v0[k] : 0.0;
    if (lane + 64 < nblocks) a += v1[k];
    s[k] = a;
  }
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
  }
}

// A xi = -g by LDL^T (s: the 21 of A, the 6 of g); false when a pivot is not above min_pivot * (largest diagonal entry of A)
__device__ inline bool icp_solve(const double* s, double min_pivot, double* xi) {
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

// The step of one image by one thread: solves the system s (the 21 of A, the 6 of g) when `enough`, composes exp(xi) with T,
// re-orthonormalises and writes T back as float32; a refused step leaves T as it is.  T_world is written either way.  wn, vn: |omega| and
// |v| of the step, 0 when refused.  Returns whether the step was accepted.
__device__ __forceinline__ bool icp_update_pose(const double* s, bool enough, double min_pivot, float* T, const float* Tr, float* Tw,
                                                double& wn, double& vn) {
  double xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const bool accepted = enough && icp_solve(s, min_pivot, xi);
  wn = 0.0; vn = 0.0;
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
  if (Tw) {                                           // camera-from-world of the current frame: R^T R_ref, R^T (t_ref - t)
    const double dx = (double)Tr[3] - (double)T[3], dy = (double)Tr[7] - (double)T[7], dz = (double)Tr[11] - (double)T[11];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        Tw[i * 4 + j] = (float)(((double)T[i] * (double)Tr[j] + (double)T[4 + i] * (double)Tr[4 + j]) + (double)T[8 + i] * (double)Tr[8 + j]);
      Tw[i * 4 + 3] = (float)(((double)T[i] * dx + (double)T[4 + i] * dy) + (double)T[8 + i] * dz);
    }
  }
  return accepted;
}

// the six columns of `stats` both entries write: s = the 30 geometric sums
__device__ __forceinline__ void icp_write_stats(float* st, const double* s, double wn, double vn, bool accepted) {
  st[0] = (float)s[29]; st[1] = (float)s[28];
  st[2] = s[29] > 0.0 ? sqrtf((float)(s[27] / s[28])) : NAN;
  st[3] = (float)wn; st[4] = (float)vn; st[5] = accepted ? 1.f : 0.f;
}
#endif  // __HIPCC__

// ---- host side ---------------------------------------------------------------------------------------------------------------------------

inline bool pos_finite(float v) { return v > 0.f && v < INFINITY; }      // false for NaN

inline int icp_blocks(int H, int W, int stride) {
  const long long n = (long long)cdiv(H, stride) * cdiv(W, stride);
  return (int)std::min<long long>((n + 255) / 256, kIcpBlocks);
}

#define CFP_ICP_REQUIRE(cond, code, msg) CFP_REQUIRE(cond, code, std::string(who) + ": " + msg)

// the checks of cfp_icp_step, for the entry `who`; terms: the doubles of a workspace row
inline int icp_check(const char* who, const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                     const float* std, int Hu, int Wu, long long std_stride, float std_floor, float cos_min, const float* K_src,
                     const float* mdl_depth, const float* mdl_normals, int Hm, int Wm, const float* K_mdl, int stride, float z_near,
                     float dist_max, int min_pairs, float min_pivot, const float* T, const float* T_ref, const float* T_world,
                     const double* sums, const float* stats, const void* ws, size_t ws_bytes, int terms) {
  CFP_ICP_REQUIRE(pred && K_src && mdl_depth && mdl_normals && K_mdl && T && stats && ws, CFP_EINVAL, "null pointer");
  CFP_ICP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0 && Hm > 0 && Wm > 0, CFP_ESHAPE, "non-positive dimension");
  CFP_ICP_REQUIRE((long long)H * W < (1ll << 31) - 256 && (long long)Hp * Wp < (1ll << 31) && H <= kMaxDim && W <= kMaxDim && B <= 65535,
                  CFP_ESHAPE, "image or batch too large");
  CFP_ICP_REQUIRE((long long)Hm * Wm < (1ll << 31) - 256 && Hm <= kMaxDim && Wm <= kMaxDim, CFP_ESHAPE, "model map too large");
  CFP_ICP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, "sizes differ and interpolate is off");
  CFP_ICP_REQUIRE(lo < hi, CFP_EINVAL, "empty depth range");
  if (std) {
    CFP_ICP_REQUIRE(Hu > 0 && Wu > 0, CFP_ESHAPE, "non-positive dimension (std)");
    CFP_ICP_REQUIRE((long long)Hu * Wu < (1ll << 31), CFP_ESHAPE, "std plane too large");
    CFP_ICP_REQUIRE(std_stride >= 0, CFP_EINVAL, "negative std image stride");
  }
  CFP_ICP_REQUIRE(stride >= 1, CFP_EINVAL, "stride must be at least 1");
  CFP_ICP_REQUIRE(pos_finite(std_floor), CFP_EINVAL, "std_floor must be positive and finite");
  CFP_ICP_REQUIRE(pos_finite(z_near), CFP_EINVAL, "z_near must be positive and finite");
  CFP_ICP_REQUIRE(pos_finite(dist_max) && pos_finite(dist_max * dist_max), CFP_EINVAL, "dist_max must be positive and finite");
  CFP_ICP_REQUIRE(min_pivot >= 0.f && min_pivot < 1.f, CFP_EINVAL, "min_pivot must lie in [0, 1)");
  CFP_ICP_REQUIRE(min_pairs >= 6, CFP_EINVAL, "min_pairs must be at least 6");
  CFP_ICP_REQUIRE(cos_min >= -1.f && cos_min <= 1.f, CFP_EINVAL, "cos_min must lie in [-1, 1]");
  CFP_ICP_REQUIRE((T_ref != nullptr) == (T_world != nullptr), CFP_EINVAL, "T_ref and T_world are given together or not at all");
  CFP_ICP_REQUIRE(ws_bytes >= (size_t)B * icp_blocks(H, W, stride) * terms * sizeof(double), CFP_EINVAL, "workspace too small");
  CFP_ICP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, CFP_EINVAL, "workspace must be 8-byte aligned");
  CFP_ICP_REQUIRE(!sums || (reinterpret_cast<uintptr_t>(sums) & 7) == 0, CFP_EINVAL, "sums must be 8-byte aligned");
  return CFP_OK;
}

inline void icp_fill(IcpP& p, IcpF& f, const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                     const float* std, int Hu, int Wu, long long std_stride, float std_floor, const float* src_normals, float cos_min,
                     const float* K_src, const float* mdl_depth, const float* mdl_normals, const float* mdl_std, int Hm, int Wm,
                     const float* K_mdl, int stride, float z_near, float dist_max, int min_pairs, float min_pivot, float* T,
                     const float* T_ref, float* T_world, int* index, double* sums, float* stats, void* ws) {
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
  f.partial = p.partial; f.nblocks = icp_blocks(H, W, stride);
  f.min_pairs = min_pairs; f.min_pivot = (double)min_pivot;
  f.T = T; f.T_ref = T_ref; f.T_world = T_world;
  f.sums = sums; f.stats = stats;
}

}  // namespace icp_core
