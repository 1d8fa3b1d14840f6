// Pictures of what the pipeline produces, on the device: the prediction, the ground truth or their error through a colour table
// (cfp_render_depth, with an optional 16-bit millimetre plane), the ToF zones drawn over a picture (cfp_render_zones) and the
// de-normalised colour image (cfp_render_rgb).
//
//   reference hooks: `colorize` (src/utils/utils.py:44-64: normalise, colour table, invalid pixels white) and the clip / bilinear
//   protocol of evaluate_all.py:40-41 -- the depth at a pixel is met_pred of metrics_pred.h in mode 0, the value cfp_eval_metrics and
//   cfp_depth_unproject see, bit for bit.  The definitions are in include/cfpnet_hip.h.
//
// Shape, the same for the three kernels: blockIdx.y is the image, a lane owns a QUAD of 4 consecutive pixels of a row, consecutive
// lanes consecutive quads in row-major order (grid-strided).  A quad's 12 bytes of RGB leave as three dword stores and its four 16-bit
// values as two when the destination allows it (base, image stride and row pitch keep every quad on a dword boundary); otherwise,
// and for the W % 4 tail of a row, they leave as bytes / halfwords of the same values.  The colour table sits in LDS as one packed
// dword per entry; cfp_render_zones also keeps the image's rectangles and the colour inside every zone there (Z <= 256).  No
// workspace, no atomics, no host synchronisation.
#include "common.h"
#include "metrics_pred.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kMaxBlocksX = 256;                      // workgroups per image; the quads beyond are grid-strided
constexpr int kMaxZones = 256;
constexpr uint32_t kWhite = 0x00ffffffu;              // colours travel as r | g << 8 | b << 16

struct RenderOut {
  unsigned char* out; long long image_stride; int pitch, vec;         // vec: every full quad starts on a dword boundary
};

__device__ __forceinline__ void load_lut(uint32_t* sLut, const unsigned char* lut) {
  const int t = threadIdx.x;                          // 256 threads, 256 entries
  sLut[t] = (uint32_t)lut[3 * t] | ((uint32_t)lut[3 * t + 1] << 8) | ((uint32_t)lut[3 * t + 2] << 16);
}

// matplotlib's rule for float input with bytes=True
__device__ __forceinline__ uint32_t lut_colour(float v, float vmin, float vmax, const uint32_t* sLut) {
  const float t = (v - vmin) / (vmax - vmin) * 256.f;
  if (t != t) return 0u;
  if (t < 0.f) return sLut[0];
  if (t >= 256.f) return sLut[255];
  return sLut[(int)t];
}

__device__ __forceinline__ unsigned char* quad_ptr(const RenderOut& o, int b, int y, int x4) {
  return o.out + (long long)b * o.image_stride + ((long long)y * o.pitch + x4) * 3;
}

// the pixels x4 .. x4 + 3 of row y that lie inside the image
__device__ __forceinline__ void store_quad(const RenderOut& o, int b, int y, int x4, int W, const uint32_t* c) {
  unsigned char* q = quad_ptr(o, b, y, x4);
  if (o.vec && x4 + 3 < W) {
    uint32_t* d = reinterpret_cast<uint32_t*>(q);
    d[0] = c[0] | (c[1] << 24);
    d[1] = (c[1] >> 8) | (c[2] << 16);
    d[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (x4 + k < W) {
        q[3 * k] = (unsigned char)(c[k] & 255u); q[3 * k + 1] = (unsigned char)((c[k] >> 8) & 255u); q[3 * k + 2] = (unsigned char)(c[k] >> 16);
      }
    }
  }
}

// ---- depth / ground truth / error ------------------------------------------------------------------------------------------------------

struct DepthP {
  MetP m;                                             // pred, gt, Hp, Wp, H, W, interpolate, mode 0, lo, hi, sy, sx
  int what, Q, u16_vec;
  float vmin, vmax, u16_scale;
  const unsigned char* lut;
  RenderOut o;
  unsigned short* u16;
};

__device__ __forceinline__ unsigned short to_u16(float v, float scale) {
  const float mm = v * scale;
  if (!(mm > 0.f)) return 0;                          // NaN too
  if (mm >= 65535.f) return 65535;
  return (unsigned short)rintf(mm);
}

__global__ __launch_bounds__(256) void render_depth_kernel(DepthP p) {
  __shared__ uint32_t sLut[256];
  const MetP& m = p.m;
  if (p.o.out) load_lut(sLut, p.lut);
  __syncthreads();
  const int b = blockIdx.y, W = m.W;
  const float* pb = m.pred ? m.pred + (long long)b * m.Hp * m.Wp : nullptr;
  const float* gb = m.gt ? m.gt + (long long)b * m.H * W : nullptr;
  const bool use_pred = p.what != CFP_RENDER_GT, use_gt = p.what != CFP_RENDER_DEPTH;
  const int n = m.H * p.Q;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int y = i / p.Q, x4 = (i - y * p.Q) * 4;
    uint32_t c[4];
    unsigned short u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int pix = y * W + min(x4 + k, W - 1);     // a quad past the end of the row repeats the last pixel and does not store it
      const float d = use_pred ? met_pred(m, pb, pix) : 0.f;
      const float g = use_gt ? gb[pix] : 0.f;
      const bool painted = !use_gt || (g > m.lo && g < m.hi);
      const float v = p.what == CFP_RENDER_DEPTH ? d : p.what == CFP_RENDER_GT ? g : p.what == CFP_RENDER_ABS_ERR ? fabsf(d - g) : fabsf(d - g) / g;
      c[k] = !p.o.out ? 0u : painted ? lut_colour(v, p.vmin, p.vmax, sLut) : kWhite;
      u[k] = painted ? to_u16(v, p.u16_scale) : (unsigned short)0;
    }
    if (p.o.out) store_quad(p.o, b, y, x4, W, c);
    if (p.u16) {
      unsigned short* q = p.u16 + ((long long)b * m.H + y) * W + x4;
      if (p.u16_vec && x4 + 3 < W) {
        uint32_t* d = reinterpret_cast<uint32_t*>(q);
        d[0] = (uint32_t)u[0] | ((uint32_t)u[1] << 16);
        d[1] = (uint32_t)u[2] | ((uint32_t)u[3] << 16);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x4 + k < W) q[k] = u[k];
      }
    }
  }
}

// ---- the ToF zones over a picture ------------------------------------------------------------------------------------------------------

struct ZonesP {
  const float* hist; const float* rect; const unsigned char* mask; const unsigned char* lut;
  int Z, S, H, W, Q, alpha;
  float vmin, vmax;
  RenderOut o;
};

__device__ __forceinline__ uint32_t blend(uint32_t c, uint32_t old, uint32_t alpha) {
  uint32_t r = 0u;
#pragma unroll
  for (int s = 0; s < 24; s += 8) r |= ((((c >> s) & 255u) * alpha + ((old >> s) & 255u) * (256u - alpha) + 128u) >> 8) << s;
  return r;
}

__global__ __launch_bounds__(256) void render_zones_kernel(ZonesP p) {
  __shared__ uint32_t sLut[256];
  __shared__ float sRect[kMaxZones * 4];
  __shared__ uint32_t sCol[kMaxZones];                // the colour inside the border
  const int b = blockIdx.y, W = p.W, t = threadIdx.x;
  load_lut(sLut, p.lut);
  __syncthreads();
  if (t < p.Z) {
    const float* r = p.rect + ((long long)b * p.Z + t) * 4;
    sRect[t * 4] = r[0]; sRect[t * 4 + 1] = r[1]; sRect[t * 4 + 2] = r[2]; sRect[t * 4 + 3] = r[3];
    uint32_t col = 0x00808080u;
    if (p.mask[(long long)b * p.Z + t] != 0) {
      const float* h = p.hist + ((long long)b * p.Z + t) * p.S;
      float sum = h[0];
      for (int s = 1; s < p.S; ++s) sum += h[s];
      col = lut_colour(sum / (float)p.S, p.vmin, p.vmax, sLut);
    }
    sCol[t] = col;
  }
  __syncthreads();
  // A wave walks steps of 64 consecutive quads, which span few rows: lane l first tests zone l (l + 64, ...) against the step's rows, and
  // only the zones of that ballot -- in index order, so that the first zone wins -- are tested per pixel.
  const int n = p.H * p.Q, lane = t & 63;
  for (int i0 = blockIdx.x * 256 + (t & ~63); i0 < n; i0 += gridDim.x * 256) {          // wave-uniform
    const bool active = i0 + lane < n;
    const int i = min(i0 + lane, n - 1);
    const int y = i / p.Q, x4 = (i - y * p.Q) * 4;
    const float fy = (float)y;
    const float fy_first = (float)(i0 / p.Q), fy_last = (float)(min(i0 + 63, n - 1) / p.Q);
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    unsigned hit = 0u;                                // bit k: pixel x4 + k lies in a zone
    const unsigned inside = !active ? 0u : x4 + 3 < W ? 15u : (1u << (W - x4)) - 1u;
    for (int z0 = 0; z0 < p.Z; z0 += 64) {
      const int zl = min(z0 + lane, p.Z - 1);
      unsigned long long cand = __ballot(z0 + lane < p.Z && sRect[zl * 4] <= fy_last && sRect[zl * 4 + 2] > fy_first);
      while (cand) {
        const int z = z0 + __ffsll((long long)cand) - 1;
        cand &= cand - 1ull;
        const float sy = sRect[z * 4], sx = sRect[z * 4 + 1], ey = sRect[z * 4 + 2], ex = sRect[z * 4 + 3];
        if (!(sy <= fy && fy < ey)) continue;
        const bool yb = fy < sy + 1.f || fy >= ey - 1.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float fx = (float)(x4 + k);
          if (((inside & ~hit) >> k & 1u) && sx <= fx && fx < ex) {
            hit |= 1u << k;
            c[k] = (yb || fx < sx + 1.f || fx >= ex - 1.f) ? 0u : sCol[z];
          }
        }
      }
    }
    if (hit == 0u) continue;                          // no pixel of the quad is in a zone: nothing is read or written
    unsigned char* q = quad_ptr(p.o, b, y, x4);
    if (p.o.vec && x4 + 3 < W) {
      uint32_t* d = reinterpret_cast<uint32_t*>(q);
      const uint32_t w0 = d[0], w1 = d[1], w2 = d[2];
      uint32_t old[4] = {w0 & kWhite, (w0 >> 24) | ((w1 & 0xffffu) << 8), (w1 >> 16) | ((w2 & 255u) << 16), w2 >> 8};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (hit >> k & 1u) old[k] = blend(c[k], old[k], (uint32_t)p.alpha);
      d[0] = old[0] | (old[1] << 24);
      d[1] = (old[1] >> 8) | (old[2] << 16);
      d[2] = (old[2] >> 16) | (old[3] << 8);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (hit >> k & 1u) {
          const uint32_t old = (uint32_t)q[3 * k] | ((uint32_t)q[3 * k + 1] << 8) | ((uint32_t)q[3 * k + 2] << 16);
          const uint32_t r = blend(c[k], old, (uint32_t)p.alpha);
          q[3 * k] = (unsigned char)(r & 255u); q[3 * k + 1] = (unsigned char)((r >> 8) & 255u); q[3 * k + 2] = (unsigned char)(r >> 16);
        }
      }
    }
  }
}

// ---- the colour image ------------------------------------------------------------------------------------------------------------------

struct RgbP {
  const float* rgb;
  float mean[3], std[3];
  int H, W, Q, v4;                                    // v4: a quad's four floats of a channel are one aligned 16-byte load
  RenderOut o;
};

__device__ __forceinline__ uint32_t to_u8(float x, float std, float mean) {
  const float v = x * std + mean;
  if (!(v > 0.f)) return 0u;                          // NaN too
  if (v >= 1.f) return 255u;
  return (uint32_t)(unsigned char)rintf(v * 255.f);
}

__global__ __launch_bounds__(256) void render_rgb_kernel(RgbP p) {
  const int b = blockIdx.y, W = p.W;
  const long long plane = (long long)p.H * W;
  const float* ib = p.rgb + (long long)b * 3 * plane;
  const int n = p.H * p.Q;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int y = i / p.Q, x4 = (i - y * p.Q) * 4;
    uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float* row = ib + ch * plane + (long long)y * W;
      float x[4];
      if (p.v4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + x4);
        x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = row[min(x4 + k, W - 1)];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) c[k] |= to_u8(x[k], p.std[ch], p.mean[ch]) << (8 * ch);
    }
    store_quad(p.o, b, y, x4, W, c);
  }
}

// the checks on a destination the three entry points share; 0 or the error code
int check_out(const char* who, int H, int W, long long image_stride, int pitch) {
  CFP_REQUIRE(pitch >= W, CFP_ESHAPE, std::string(who) + ": pitch is smaller than W");
  CFP_REQUIRE(image_stride >= (long long)H * pitch * 3, CFP_ESHAPE, std::string(who) + ": image_stride is smaller than H * pitch * 3");
  return CFP_OK;
}

RenderOut make_out(unsigned char* out, long long image_stride, int pitch) {
  RenderOut o;
  o.out = out; o.image_stride = image_stride; o.pitch = pitch;
  o.vec = (reinterpret_cast<uintptr_t>(out) & 3) == 0 && image_stride % 4 == 0 && pitch % 4 == 0;
  return o;
}

dim3 quad_grid(int H, int Q, int B) { return dim3(std::min(cdiv((long long)H * Q, 256), kMaxBlocksX), B); }

constexpr long long kMaxPixels = (1ll << 31) - (1ll << 20);         // the grid-strided quad index stays an int

}  // namespace

extern "C" int cfp_render_depth(const float* pred, int Hp, int Wp, const float* gt, int H, int W, int B, int interpolate, float lo, float hi,
                                int what, float vmin, float vmax, const unsigned char* lut, unsigned char* out, long long image_stride,
                                int pitch, unsigned short* u16_out, float u16_scale, cfp_stream_t stream) {
  CFP_REQUIRE(what == CFP_RENDER_DEPTH || what == CFP_RENDER_GT || what == CFP_RENDER_ABS_ERR || what == CFP_RENDER_REL_ERR, CFP_EINVAL,
              "cfp_render_depth: unknown what");
  const bool use_pred = what != CFP_RENDER_GT, use_gt = what != CFP_RENDER_DEPTH;
  CFP_REQUIRE(B > 0 && H > 0 && W > 0 && (!use_pred || (Hp > 0 && Wp > 0)), CFP_ESHAPE, "cfp_render_depth: non-positive dimension");
  CFP_REQUIRE((long long)H * W < kMaxPixels && (!use_pred || (long long)Hp * Wp < (1ll << 31)) && B <= 65535, CFP_ESHAPE,
              "cfp_render_depth: image or batch too large");
  CFP_REQUIRE(!use_pred || interpolate || (Hp == H && Wp == W), CFP_ESHAPE, "cfp_render_depth: sizes differ and interpolate is off");
  CFP_REQUIRE((!use_pred || pred) && (!use_gt || gt), CFP_EINVAL, "cfp_render_depth: null pointer");
  CFP_REQUIRE(out || u16_out, CFP_EINVAL, "cfp_render_depth: out and u16_out are both null");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, "cfp_render_depth: empty depth range");
  if (out) {
    CFP_REQUIRE(lut, CFP_EINVAL, "cfp_render_depth: null pointer (lut)");
    CFP_REQUIRE(std::isfinite(vmin) && std::isfinite(vmax) && vmin < vmax, CFP_EINVAL, "cfp_render_depth: vmin < vmax must be finite");
    if (const int rc = check_out("cfp_render_depth", H, W, image_stride, pitch)) return rc;
  }
  if (u16_out) {
    CFP_REQUIRE(what == CFP_RENDER_DEPTH || what == CFP_RENDER_GT, CFP_EINVAL, "cfp_render_depth: u16_out goes with DEPTH and GT only");
    CFP_REQUIRE(std::isfinite(u16_scale) && u16_scale > 0.f, CFP_EINVAL, "cfp_render_depth: u16_scale must be finite and positive");
  }
  DepthP p;
  p.m = met_params(use_pred ? pred : nullptr, use_gt ? gt : nullptr, use_pred ? Hp : H, use_pred ? Wp : W, H, W, B,
                   use_pred ? interpolate : 0, 0, lo, hi);
  p.what = what; p.Q = cdiv(W, 4);
  p.vmin = vmin; p.vmax = vmax; p.u16_scale = u16_scale; p.lut = lut;
  p.o = make_out(out, image_stride, pitch);
  p.u16 = u16_out;
  p.u16_vec = (reinterpret_cast<uintptr_t>(u16_out) & 3) == 0 && W % 2 == 0;
  hipLaunchKernelGGL(render_depth_kernel, quad_grid(H, p.Q, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
  return cfp_check_launch("cfp_render_depth");
}

extern "C" int cfp_render_zones(const float* hist, const float* rect, const unsigned char* mask, int Z, int S, int H, int W, int B, float vmin,
                                float vmax, const unsigned char* lut, int alpha, unsigned char* out, long long image_stride, int pitch,
                                cfp_stream_t stream) {
  CFP_REQUIRE(B > 0 && H > 0 && W > 0, CFP_ESHAPE, "cfp_render_zones: non-positive dimension");
  CFP_REQUIRE((long long)H * W < kMaxPixels && B <= 65535, CFP_ESHAPE, "cfp_render_zones: image or batch too large");
  CFP_REQUIRE(Z >= 1 && Z <= kMaxZones && S >= 1, CFP_ESHAPE, "cfp_render_zones: Z must be 1..256 and S positive");
  CFP_REQUIRE(hist && rect && mask && lut && out, CFP_EINVAL, "cfp_render_zones: null pointer");
  CFP_REQUIRE(std::isfinite(vmin) && std::isfinite(vmax) && vmin < vmax, CFP_EINVAL, "cfp_render_zones: vmin < vmax must be finite");
  CFP_REQUIRE(alpha >= 0 && alpha <= 256, CFP_EINVAL, "cfp_render_zones: alpha must be 0..256");
  if (const int rc = check_out("cfp_render_zones", H, W, image_stride, pitch)) return rc;
  ZonesP p;
  p.hist = hist; p.rect = rect; p.mask = mask; p.lut = lut;
  p.Z = Z; p.S = S; p.H = H; p.W = W; p.Q = cdiv(W, 4); p.alpha = alpha;
  p.vmin = vmin; p.vmax = vmax;
  p.o = make_out(out, image_stride, pitch);
  hipLaunchKernelGGL(render_zones_kernel, quad_grid(H, p.Q, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
  return cfp_check_launch("cfp_render_zones");
}

extern "C" int cfp_render_rgb(const float* rgb, const float* mean, const float* std_, int H, int W, int B, unsigned char* out,
                              long long image_stride, int pitch, cfp_stream_t stream) {
  CFP_REQUIRE(B > 0 && H > 0 && W > 0, CFP_ESHAPE, "cfp_render_rgb: non-positive dimension");
  CFP_REQUIRE((long long)H * W < kMaxPixels && B <= 65535, CFP_ESHAPE, "cfp_render_rgb: image or batch too large");
  CFP_REQUIRE(rgb && mean && std_ && out, CFP_EINVAL, "cfp_render_rgb: null pointer");
  if (const int rc = check_out("cfp_render_rgb", H, W, image_stride, pitch)) return rc;
  RgbP p;
  p.rgb = rgb;
  for (int c = 0; c < 3; ++c) {                       // mean and std are the host pointers of the call
    CFP_REQUIRE(std::isfinite(mean[c]) && std::isfinite(std_[c]), CFP_EINVAL, "cfp_render_rgb: mean and std must be finite");
    p.mean[c] = mean[c]; p.std[c] = std_[c];
  }
  p.H = H; p.W = W; p.Q = cdiv(W, 4);
  p.v4 = W % 4 == 0 && aligned16(rgb);
  p.o = make_out(out, image_stride, pitch);
  hipLaunchKernelGGL(render_rgb_kernel, quad_grid(H, p.Q, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
  return cfp_check_launch("cfp_render_rgb");
}
