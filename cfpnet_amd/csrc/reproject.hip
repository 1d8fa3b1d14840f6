// Depth across views and across time, on the device: the forward warp of the prediction into another camera with a z-buffer
// (cfp_depth_reproject) and the per-pixel fusion of the current prediction with such a warped prior by their variances (cfp_depth_fuse).
// The definitions are in include/cfpnet_hip.h; the depth at a source pixel is met_pred of metrics_pred.h in mode 0, the value
// cfp_depth_unproject back-projects, bit for bit, and a map that travels with it is met_plane.
//
// Reproject.  A forward warp is a scatter: several sources can land on one target pixel and the nearest must win.  The workspace holds one
// 64-bit key per target pixel, (bits(Z') << 32) | source index; three launches:
//   1. fill     every key all ones
//   2. splat    one thread per source pixel: depth, point, pose, projection, then one 64-bit unsigned atomicMin per target pixel hit
//               (1 or 4).  Positive floats order like their bits; an integer minimum is independent of the order of arrival.
//   3. resolve  one thread per target pixel: the key's two halves, and the plane at the winning source pixel
// The atomics are scattered 8-byte ones, a lane per address; measured against a same-bytes copy in DESIGN.md section 4.27.
//
// Fuse.  Elementwise, with four counts and two float64 sums per image: a workgroup strides over its image's pixels, reduces its threads'
// partials through LDS in a fixed tree and stores them; a second launch adds each image's workgroup partials in the same fixed tree.
#include "common.h"
#include "metrics_pred.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kMaxBlocks = 2048;                      // grid cap of the fill / resolve kernels; the pixels beyond it are grid-strided
constexpr int kFuseMaxBlocks = 128;                   // workgroups per image of the fuse kernel = partials the finish kernel adds
constexpr int kFusePixPerBlock = 2048;                // pixels a fuse workgroup takes before another one is worth starting
constexpr long long kMaxDim = 1ll << 24;              // a target row / column index is compared as a float: exact below 2^24
constexpr unsigned long long kEmpty = ~0ull;

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }      // false for NaN

struct ReprojP {
  MetP m;                                             // the source depth: pred, Hp, Wp, H, W, interpolate, mode 0, lo, hi
  MetP u;                                             // the plane as met_plane reads it: pred = plane base, Hp x Wp = Hu x Wu
  const float* K_src; const float* T; const float* K_dst;
  long long plane_stride, n_dst;                      // n_dst = B * Hd * Wd
  int Hd, Wd, splat;
  float z_near;
  float* depth_out; int* index_out; float* plane_out;
  unsigned long long* ws;
};

__global__ __launch_bounds__(256) void reproject_fill_kernel(unsigned long long* __restrict__ ws, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) ws[i] = kEmpty;
}

// one target pixel of image b's z-buffer, if (col, row) -- still floats -- lies inside the Hd x Wd grid
__device__ __forceinline__ void reproject_hit(const ReprojP& p, unsigned long long* zb, float col, float row, unsigned long long key) {
  if (!(col >= 0.f && col < (float)p.Wd && row >= 0.f && row < (float)p.Hd)) return;      // NaN fails
  atomicMin(zb + (long long)(int)row * p.Wd + (int)col, key);
}

__global__ __launch_bounds__(256) void reproject_splat_kernel(ReprojP p) {
  const MetP& m = p.m;
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;       // H * W < 2^31 - 256
  if (i >= m.H * m.W) return;
  const float d = met_pred(m, m.pred + (long long)b * m.Hp * m.Wp, i);
  if (!(finitef(d) && d > 0.f)) return;
  const int y = i / m.W, x = i - y * m.W;
  const float* K = p.K_src + b * 4;
  const float* T = p.T + b * 12;
  const float* Kd = p.K_dst + b * 4;
  const float X = ((float)x - K[2]) / K[0] * d, Y = ((float)y - K[3]) / K[1] * d, Z = d;
  const float Xp = (T[0] * X + T[1] * Y) + T[2] * Z + T[3];
  const float Yp = (T[4] * X + T[5] * Y) + T[6] * Z + T[7];
  const float Zp = (T[8] * X + T[9] * Y) + T[10] * Z + T[11];
  if (!(finitef(Zp) && Zp >= p.z_near)) return;
  const float u = Kd[0] * (Xp / Zp) + Kd[2], v = Kd[1] * (Yp / Zp) + Kd[3];
  const unsigned long long key = ((unsigned long long)__float_as_uint(Zp) << 32) | (unsigned)i;
  unsigned long long* zb = p.ws + (long long)b * p.Hd * p.Wd;
  if (p.splat == 1) {
    reproject_hit(p, zb, floorf(u + 0.5f), floorf(v + 0.5f), key);
  } else {
    const float u0 = floorf(u), v0 = floorf(v);
    reproject_hit(p, zb, u0, v0, key);
    reproject_hit(p, zb, u0 + 1.f, v0, key);
    reproject_hit(p, zb, u0, v0 + 1.f, key);
    reproject_hit(p, zb, u0 + 1.f, v0 + 1.f, key);
  }
}

template <bool PLANE>
__global__ __launch_bounds__(256) void reproject_resolve_kernel(ReprojP p) {
  const long long per_image = (long long)p.Hd * p.Wd;
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < p.n_dst; j += (long long)gridDim.x * 256) {
    const unsigned long long key = p.ws[j];
    const bool hit = key != kEmpty;
    const int src = hit ? (int)(unsigned)(key & 0xffffffffull) : -1;
    p.depth_out[j] = hit ? __uint_as_float((unsigned)(key >> 32)) : NAN;
    p.index_out[j] = src;
    if constexpr (PLANE) {
      const int b = (int)(j / per_image);
      p.plane_out[j] = hit ? met_plane(p.u, p.u.pred + (long long)b * p.plane_stride, src) : NAN;
    }
  }
}

// ---- fusion --------------------------------------------------------------------------------------------------------------------------------

struct FuseP {
  MetP m;                                             // the current prediction
  MetP u;                                             // its std plane
  long long std_stride;
  const float* prior_depth; const float* prior_var;
  float std_floor, process_var, gate_k, gate_abs;
  float* out_depth; float* out_var;
  int* counts; double* stats;
  double* ws;                                         // [B][nblk][4]: {sum |p - c|, sum (p - c)^2, two doubles' room for the four counts}
  int nblk;
};

struct FuseAcc {
  double s_abs, s_sq;
  int n[4];
};

__device__ __forceinline__ void fuse_add(FuseAcc& a, const FuseAcc& o) {
  a.s_abs += o.s_abs; a.s_sq += o.s_sq;
#pragma unroll
  for (int k = 0; k < 4; ++k) a.n[k] += o.n[k];
}

// the sum over a workgroup's threads in a fixed tree, valid in thread 0; N threads, a power of two
template <int N>
__device__ __forceinline__ FuseAcc fuse_block_sum(FuseAcc a, FuseAcc* s) {
  s[threadIdx.x] = a;
  __syncthreads();
#pragma unroll
  for (int o = N / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) fuse_add(s[threadIdx.x], s[threadIdx.x + o]);
    __syncthreads();
  }
  return s[0];
}

__global__ __launch_bounds__(256) void fuse_kernel(FuseP p) {
  __shared__ FuseAcc s[256];
  const MetP& m = p.m;
  const int b = blockIdx.y, HW = m.H * m.W;
  const float* cb = m.pred + (long long)b * m.Hp * m.Wp;
  const float* sb = p.u.pred + (long long)b * p.std_stride;
  const long long img = (long long)b * HW;
  FuseAcc a = {0.0, 0.0, {0, 0, 0, 0}};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256) {
    const float c = met_pred(m, cb, (int)i);
    const float sd = met_plane(p.u, sb, (int)i);
    const float sf = sd > p.std_floor ? sd : p.std_floor;
    const float vc = sf * sf;
    const float pd = p.prior_depth[img + i], vp0 = p.prior_var[img + i];
    const bool present = finitef(pd) && finitef(vp0), cf = finitef(c);
    const float vp = vp0 + p.process_var;
    float od, ov;
    if (!present) {
      od = cf ? c : NAN; ov = cf ? vc : INFINITY;
    } else {
      a.n[CFP_FUSE_PRIOR] += 1;
      if (!cf) {
        od = pd; ov = vp;
        a.n[CFP_FUSE_FILLED] += 1;
      } else {
        const float diff = pd - c, ad = fabsf(diff), sum = vc + vp;
        a.s_abs += (double)ad;
        a.s_sq += (double)(diff * diff);
        if (ad > p.gate_k * sqrtf(sum) + p.gate_abs) {
          od = c; ov = vc;
          a.n[CFP_FUSE_REJECTED] += 1;
        } else {
          const float w = vc / sum;
          od = c + w * diff; ov = (vc * vp) / sum;
          a.n[CFP_FUSE_FUSED] += 1;
        }
      }
    }
    p.out_depth[img + i] = od;
    p.out_var[img + i] = ov;
  }
  a = fuse_block_sum<256>(a, s);
  if (threadIdx.x == 0) {
    double* w = p.ws + ((long long)b * p.nblk + blockIdx.x) * 4;
    w[0] = a.s_abs; w[1] = a.s_sq;
    int* wn = reinterpret_cast<int*>(w + 2);
    wn[0] = a.n[0]; wn[1] = a.n[1]; wn[2] = a.n[2]; wn[3] = a.n[3];
  }
}

// one workgroup per image: thread t takes workgroup t's partial (nblk <= kFuseMaxBlocks), the same tree
__global__ __launch_bounds__(kFuseMaxBlocks) void fuse_finish_kernel(FuseP p) {
  __shared__ FuseAcc s[kFuseMaxBlocks];
  const int b = blockIdx.x, t = threadIdx.x;
  FuseAcc a = {0.0, 0.0, {0, 0, 0, 0}};
  if (t < p.nblk) {
    const double* w = p.ws + ((long long)b * p.nblk + t) * 4;
    const int* wn = reinterpret_cast<const int*>(w + 2);
    a.s_abs = w[0]; a.s_sq = w[1];
    a.n[0] = wn[0]; a.n[1] = wn[1]; a.n[2] = wn[2]; a.n[3] = wn[3];
  }
  a = fuse_block_sum<kFuseMaxBlocks>(a, s);
  if (t == 0) {
    p.stats[b * 2] = a.s_abs; p.stats[b * 2 + 1] = a.s_sq;
    p.counts[b * 4] = a.n[0]; p.counts[b * 4 + 1] = a.n[1]; p.counts[b * 4 + 2] = a.n[2]; p.counts[b * 4 + 3] = a.n[3];
  }
}

int fuse_blocks(int H, int W) {
  return (int)std::min<long long>(kFuseMaxBlocks, ((long long)H * W + kFusePixPerBlock - 1) / kFusePixPerBlock);
}

}  // namespace

extern "C" size_t cfp_depth_reproject_ws_bytes(int B, int Hd, int Wd) {
  if (B <= 0 || Hd <= 0 || Wd <= 0) return 0;
  return (size_t)B * (size_t)Hd * (size_t)Wd * 8;
}

extern "C" int cfp_depth_reproject(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                                   const float* K_src, const float* T, const float* K_dst, int Hd, int Wd, int splat, float z_near,
                                   const float* plane, int Hu, int Wu, long long plane_stride, float* depth_out, int* index_out,
                                   float* plane_out, void* ws, size_t ws_bytes, cfp_stream_t stream) {
  CFP_REQUIRE(pred && K_src && T && K_dst && depth_out && index_out && ws, CFP_EINVAL, "cfp_depth_reproject: null pointer");
  CFP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0 && Hd > 0 && Wd > 0, CFP_ESHAPE, "cfp_depth_reproject: non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) - 256 && (long long)Hp * Wp < (1ll << 31) && (long long)Hd * Wd < (1ll << 31) &&
                  Hd <= kMaxDim && Wd <= kMaxDim && B <= 65535, CFP_ESHAPE, "cfp_depth_reproject: image or batch too large");
  CFP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, "cfp_depth_reproject: sizes differ and interpolate is off");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, "cfp_depth_reproject: empty depth range");
  CFP_REQUIRE(splat == 1 || splat == 2, CFP_EINVAL, "cfp_depth_reproject: splat must be 1 or 2");
  CFP_REQUIRE(z_near > 0.f, CFP_EINVAL, "cfp_depth_reproject: z_near must be positive");      // false for NaN too
  CFP_REQUIRE((plane != nullptr) == (plane_out != nullptr), CFP_EINVAL,
              "cfp_depth_reproject: plane and plane_out must be given together");
  if (plane) {
    CFP_REQUIRE(Hu > 0 && Wu > 0 && (long long)Hu * Wu < (1ll << 31), CFP_ESHAPE, "cfp_depth_reproject: non-positive dimension (plane)");
    CFP_REQUIRE(plane_stride >= 0, CFP_EINVAL, "cfp_depth_reproject: negative plane image stride");
  }
  CFP_REQUIRE(ws_bytes >= cfp_depth_reproject_ws_bytes(B, Hd, Wd), CFP_EINVAL, "cfp_depth_reproject: workspace too small");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, CFP_EINVAL, "cfp_depth_reproject: workspace must be 8-byte aligned");
  ReprojP p;
  p.m = met_params(pred, nullptr, Hp, Wp, H, W, B, interpolate, 0, lo, hi);
  p.u = met_params(plane, nullptr, plane ? Hu : H, plane ? Wu : W, H, W, B, plane && (Hu != H || Wu != W) ? 1 : 0, 0, 0.f, 0.f);
  p.K_src = K_src; p.T = T; p.K_dst = K_dst;
  p.plane_stride = plane_stride; p.n_dst = (long long)B * Hd * Wd;
  p.Hd = Hd; p.Wd = Wd; p.splat = splat; p.z_near = z_near;
  p.depth_out = depth_out; p.index_out = index_out; p.plane_out = plane_out;
  p.ws = reinterpret_cast<unsigned long long*>(ws);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int grid = (int)std::min<long long>((p.n_dst + 255) / 256, kMaxBlocks);
  hipLaunchKernelGGL(reproject_fill_kernel, dim3(grid), dim3(256), 0, s, p.ws, p.n_dst);
  hipLaunchKernelGGL(reproject_splat_kernel, dim3(cdiv((long long)H * W, 256), B), dim3(256), 0, s, p);
  if (plane) hipLaunchKernelGGL(reproject_resolve_kernel<true>, dim3(grid), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(reproject_resolve_kernel<false>, dim3(grid), dim3(256), 0, s, p);
  return cfp_check_launch("cfp_depth_reproject");
}

extern "C" size_t cfp_depth_fuse_ws_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * (size_t)fuse_blocks(H, W) * 4 * sizeof(double);
}

extern "C" int cfp_depth_fuse(const float* cur, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi,
                              const float* cur_std, int Hu, int Wu, long long std_stride, float std_floor, const float* prior_depth,
                              const float* prior_var, float process_var, float gate_k, float gate_abs, float* out_depth, float* out_var,
                              int* counts, double* stats, void* ws, size_t ws_bytes, cfp_stream_t stream) {
  CFP_REQUIRE(cur && cur_std && prior_depth && prior_var && out_depth && out_var && counts && stats && ws, CFP_EINVAL,
              "cfp_depth_fuse: null pointer");
  CFP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0 && Hu > 0 && Wu > 0, CFP_ESHAPE, "cfp_depth_fuse: non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) - 256 && (long long)Hp * Wp < (1ll << 31) && (long long)Hu * Wu < (1ll << 31) && B <= 65535,
              CFP_ESHAPE, "cfp_depth_fuse: image or batch too large");
  CFP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, "cfp_depth_fuse: sizes differ and interpolate is off");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, "cfp_depth_fuse: empty depth range");
  CFP_REQUIRE(std_stride >= 0, CFP_EINVAL, "cfp_depth_fuse: negative std image stride");
  CFP_REQUIRE(std_floor > 0.f && std_floor < INFINITY, CFP_EINVAL, "cfp_depth_fuse: std_floor must be positive and finite");
  CFP_REQUIRE(process_var >= 0.f && process_var < INFINITY, CFP_EINVAL, "cfp_depth_fuse: process_var must be non-negative and finite");
  CFP_REQUIRE(gate_k >= 0.f && gate_abs >= 0.f, CFP_EINVAL, "cfp_depth_fuse: gate_k and gate_abs must be non-negative");      // false for NaN
  CFP_REQUIRE(ws_bytes >= cfp_depth_fuse_ws_bytes(B, H, W), CFP_EINVAL, "cfp_depth_fuse: workspace too small");
  CFP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, CFP_EINVAL, "cfp_depth_fuse: workspace must be 8-byte aligned");
  FuseP p;
  p.m = met_params(cur, nullptr, Hp, Wp, H, W, B, interpolate, 0, lo, hi);
  p.u = met_params(cur_std, nullptr, Hu, Wu, H, W, B, (Hu != H || Wu != W) ? 1 : 0, 0, 0.f, 0.f);
  p.std_stride = std_stride;
  p.prior_depth = prior_depth; p.prior_var = prior_var;
  p.std_floor = std_floor; p.process_var = process_var; p.gate_k = gate_k; p.gate_abs = gate_abs;
  p.out_depth = out_depth; p.out_var = out_var; p.counts = counts; p.stats = stats;
  p.ws = reinterpret_cast<double*>(ws);
  p.nblk = fuse_blocks(H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(fuse_kernel, dim3(p.nblk, B), dim3(256), 0, s, p);
  hipLaunchKernelGGL(fuse_finish_kernel, dim3(B), dim3(kFuseMaxBlocks), 0, s, p);
  return cfp_check_launch("cfp_depth_fuse");
}
