// Dynamic zone geometry of the training step: the fusion layers' zone rectangle read from a DEVICE record, so one captured
// step serves every per-sample grid offset (`--train_zone_random_offset`).
//
//   record (int32[9], geometry.zone_record): sy, sx, tzh, tzw   -- the batch rectangle in token coordinates (may overhang),
//                                            y0, y1, x0, x1     -- its part inside the H x W token map (fusion.py:104),
//                                            n_in               -- (y1 - y0) * (x1 - x0)
//   grid: Gh x Gw = zn*p1 x zn*p2, the zone-token grid hist2image attends on; zone layout [(b, zy, zx), (i, j)].
//
//   crop   (fusion.py:129-133): zone[b, zy, zx, i, j] = bilinear(align_corners) of the zero-extended map's [sy:sy+tzh, sx:sx+tzw]
//          at grid point (zy*p1 + i, zx*p2 + j); when (tzh, tzw) == (Gh, Gw) the weights are 1 / 0 and the kernel copies the
//          element (bit-identical to the cfp_index_rows crop + regroup of the static path).
//   paste  (fusion.py:136-157): out = tok + resize(zone grid -> tzh x tzw) on the clipped rectangle, tok elsewhere.
//   rect rows (transformer.py:215-234): zero the inside rows / gather them into a [B * cap] buffer (rows >= n_in zero) / the
//          adjoint of that gather.
// Every backward is in gather form: each output element sums its contributions in a fixed order, no atomics (a captured step
// is bit-identical to the eager one).  One thread per 16-byte channel vector of one row, wave64.
#include "common.h"

namespace {

struct Rec { int sy, sx, tzh, tzw, y0, y1, x0, x1, n_in; };

__device__ __forceinline__ Rec load_rec(const int* __restrict__ r) {
  Rec g;
  g.sy = r[0]; g.sx = r[1]; g.tzh = r[2]; g.tzw = r[3]; g.y0 = r[4]; g.y1 = r[5]; g.x0 = r[6]; g.x1 = r[7]; g.n_in = r[8];
  return g;
}

// align_corners source coordinate of destination index d for a resize n_src -> n_dst: cfp_resize_bilinear's own arithmetic
// (scale = (n_src - 1) / (n_dst - 1) in float32, src = scale * d, truncation, second tap clamped at the border)
struct Tap { int i0, i1; float l0, l1; };
__device__ __forceinline__ Tap tap(int d, int n_src, int n_dst) {
  const float sc = n_dst > 1 ? (float)(n_src - 1) / (float)(n_dst - 1) : 0.f;
  const float f = sc * (float)d;
  Tap t;
  t.i0 = min((int)f, n_src - 1);
  t.i1 = t.i0 + (t.i0 < n_src - 1 ? 1 : 0);
  t.l1 = f - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// destination indices whose taps can reach source index s (a superset; the caller re-evaluates `tap`)
__device__ __forceinline__ void tap_range(int s, int n_src, int n_dst, int lo_clamp, int hi_clamp, int* lo, int* hi) {
  if (n_src > 1 && n_dst > 1) {
    const float inv = (float)(n_dst - 1) / (float)(n_src - 1);
    *lo = max((int)floorf((float)(s - 1) * inv) - 1, lo_clamp);
    *hi = min((int)ceilf((float)(s + 1) * inv) + 1, hi_clamp);
  } else {
    *lo = lo_clamp; *hi = hi_clamp;
  }
}

__device__ __forceinline__ float tap_weight(const Tap& t, int s) { return (t.i0 == s ? t.l0 : 0.f) + (t.i1 == s ? t.l1 : 0.f); }

template <typename T>
__device__ __forceinline__ void vzero(T* p) {
  float z[Vec<T>::N];
#pragma unroll
  for (int e = 0; e < Vec<T>::N; ++e) z[e] = 0.f;
  Vec<T>::store(p, z);
}

template <typename T>
__device__ __forceinline__ void vcopy(const T* __restrict__ s, T* __restrict__ d) {
  *reinterpret_cast<u32x4*>(d) = *reinterpret_cast<const u32x4*>(s);
}

template <typename T>
__device__ __forceinline__ void vaxpy(float w, const T* __restrict__ p, float* acc) {
  float v[Vec<T>::N];
  Vec<T>::load(p, v);
#pragma unroll
  for (int e = 0; e < Vec<T>::N; ++e) acc[e] = fmaf(w, v[e], acc[e]);
}

// zone-layout row of grid point (gy, gx)
__device__ __forceinline__ long long zrow(int b, int gy, int gx, int zn, int p1, int p2) {
  const int zy = gy / p1, i = gy - zy * p1, zx = gx / p2, j = gx - zx * p2;
  return ((long long)(b * zn + zy) * zn + zx) * (p1 * p2) + i * p2 + j;
}

template <typename T>
__global__ __launch_bounds__(256) void zone_crop_kernel(const T* __restrict__ tok, int tok_ld, const int* __restrict__ rec, T* __restrict__ out,
                                                        int out_ld, int B, int H, int W, int C, int zn, int p1, int p2) {
  constexpr int VE = Vec<T>::N;
  const Rec g = load_rec(rec);
  const int CV = C / VE, Gh = zn * p1, Gw = zn * p2;
  const long long total = (long long)B * Gh * Gw * CV;
  const bool ident = g.tzh == Gh && g.tzw == Gw;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int cv = (int)(e % CV);
    long long r = e / CV;
    const int j = (int)(r % p2); r /= p2;
    const int i = (int)(r % p1); r /= p1;
    const int zx = (int)(r % zn); r /= zn;
    const int zy = (int)(r % zn);
    const int b = (int)(r / zn);
    const int gy = zy * p1 + i, gx = zx * p2 + j;
    T* o = out + (e / CV) * out_ld + cv * VE;
    if (g.tzh <= 0 || g.tzw <= 0) { vzero(o); continue; }
    auto src = [&](int cy, int cx) -> const T* {
      const int py = g.sy + cy, px = g.sx + cx;
      return (py >= 0 && py < H && px >= 0 && px < W) ? tok + ((long long)(b * H + py) * W + px) * tok_ld + cv * VE : nullptr;
    };
    if (ident) {
      const T* s = src(gy, gx);
      if (s) vcopy(s, o); else vzero(o);
      continue;
    }
    const Tap ty = tap(gy, g.tzh, Gh), tx = tap(gx, g.tzw, Gw);
    float a0[VE], a1[VE], acc[VE];
#pragma unroll
    for (int q = 0; q < VE; ++q) { a0[q] = 0.f; a1[q] = 0.f; }
    const T* s;
    if ((s = src(ty.i0, tx.i0))) vaxpy(tx.l0, s, a0);
    if ((s = src(ty.i0, tx.i1))) vaxpy(tx.l1, s, a0);
    if ((s = src(ty.i1, tx.i0))) vaxpy(tx.l0, s, a1);
    if ((s = src(ty.i1, tx.i1))) vaxpy(tx.l1, s, a1);
#pragma unroll
    for (int q = 0; q < VE; ++q) acc[q] = ty.l0 * a0[q] + ty.l1 * a1[q];
    Vec<T>::store(o, acc);
  }
}

// adjoint of zone_crop: every map pixel gathers the zone-grid gradients that read it (zero outside the rectangle)
template <typename T>
__global__ __launch_bounds__(256) void zone_crop_bwd_kernel(const T* __restrict__ dz, int dz_ld, const int* __restrict__ rec, T* __restrict__ dtok,
                                                            int dtok_ld, int B, int H, int W, int C, int zn, int p1, int p2) {
  constexpr int VE = Vec<T>::N;
  const Rec g = load_rec(rec);
  const int CV = C / VE, Gh = zn * p1, Gw = zn * p2;
  const long long total = (long long)B * H * W * CV;
  const bool ident = g.tzh == Gh && g.tzw == Gw;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int cv = (int)(e % CV);
    long long r = e / CV;
    const int px = (int)(r % W); r /= W;
    const int py = (int)(r % H);
    const int b = (int)(r / H);
    const int cy = py - g.sy, cx = px - g.sx;
    T* o = dtok + (e / CV) * dtok_ld + cv * VE;
    if (cy < 0 || cy >= g.tzh || cx < 0 || cx >= g.tzw) { vzero(o); continue; }
    if (ident) { vcopy(dz + zrow(b, cy, cx, zn, p1, p2) * dz_ld + cv * VE, o); continue; }
    int gy0, gy1, gx0, gx1;
    tap_range(cy, g.tzh, Gh, 0, Gh - 1, &gy0, &gy1);
    tap_range(cx, g.tzw, Gw, 0, Gw - 1, &gx0, &gx1);
    float acc[VE];
#pragma unroll
    for (int q = 0; q < VE; ++q) acc[q] = 0.f;
    for (int gy = gy0; gy <= gy1; ++gy) {
      const Tap t = tap(gy, g.tzh, Gh);
      if (t.i0 != cy && t.i1 != cy) continue;
      const float wy = tap_weight(t, cy);
      for (int gx = gx0; gx <= gx1; ++gx) {
        const Tap u = tap(gx, g.tzw, Gw);
        if (u.i0 != cx && u.i1 != cx) continue;
        vaxpy(wy * tap_weight(u, cx), dz + zrow(b, gy, gx, zn, p1, p2) * dz_ld + cv * VE, acc);
      }
    }
    Vec<T>::store(o, acc);
  }
}

// out = tok + resize(zone grid -> tzh x tzw) on the clipped rectangle; tok elsewhere
template <typename T>
__global__ __launch_bounds__(256) void zone_paste_kernel(const T* __restrict__ tok, int tok_ld, const T* __restrict__ z, int z_ld,
                                                         const int* __restrict__ rec, T* __restrict__ out, int out_ld, int B, int H, int W, int C,
                                                         int zn, int p1, int p2) {
  constexpr int VE = Vec<T>::N;
  const Rec g = load_rec(rec);
  const int CV = C / VE, Gh = zn * p1, Gw = zn * p2;
  const long long total = (long long)B * H * W * CV;
  const bool ident = g.tzh == Gh && g.tzw == Gw;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int cv = (int)(e % CV);
    long long r = e / CV;
    const int px = (int)(r % W); r /= W;
    const int py = (int)(r % H);
    const int b = (int)(r / H);
    const T* t = tok + (e / CV) * tok_ld + cv * VE;
    T* o = out + (e / CV) * out_ld + cv * VE;
    const int ry = py - g.sy, rx = px - g.sx;
    const bool in = py >= g.y0 && py < g.y1 && px >= g.x0 && px < g.x1 && ry >= 0 && ry < g.tzh && rx >= 0 && rx < g.tzw;
    if (!in) { vcopy(t, o); continue; }
    float acc[VE];
    Vec<T>::load(t, acc);
    if (ident) {
      vaxpy(1.f, z + zrow(b, ry, rx, zn, p1, p2) * z_ld + cv * VE, acc);
    } else {
      const Tap ty = tap(ry, Gh, g.tzh), tx = tap(rx, Gw, g.tzw);
      float a0[VE], a1[VE];
#pragma unroll
      for (int q = 0; q < VE; ++q) { a0[q] = 0.f; a1[q] = 0.f; }
      vaxpy(tx.l0, z + zrow(b, ty.i0, tx.i0, zn, p1, p2) * z_ld + cv * VE, a0);
      vaxpy(tx.l1, z + zrow(b, ty.i0, tx.i1, zn, p1, p2) * z_ld + cv * VE, a0);
      vaxpy(tx.l0, z + zrow(b, ty.i1, tx.i0, zn, p1, p2) * z_ld + cv * VE, a1);
      vaxpy(tx.l1, z + zrow(b, ty.i1, tx.i1, zn, p1, p2) * z_ld + cv * VE, a1);
#pragma unroll
      for (int q = 0; q < VE; ++q) acc[q] += ty.l0 * a0[q] + ty.l1 * a1[q];
    }
    Vec<T>::store(o, acc);
  }
}

// adjoint of the pasted term: every zone-grid point gathers the map gradients of the rectangle pixels (inside the map) that read it
template <typename T>
__global__ __launch_bounds__(256) void zone_paste_bwd_kernel(const T* __restrict__ dy, int dy_ld, const int* __restrict__ rec, T* __restrict__ dz,
                                                             int dz_ld, int B, int H, int W, int C, int zn, int p1, int p2) {
  constexpr int VE = Vec<T>::N;
  Rec g = load_rec(rec);
  g.y0 = max(g.y0, 0); g.y1 = min(g.y1, H); g.x0 = max(g.x0, 0); g.x1 = min(g.x1, W);      // never read outside the map
  const int CV = C / VE, Gh = zn * p1, Gw = zn * p2;
  const long long total = (long long)B * Gh * Gw * CV;
  const bool ident = g.tzh == Gh && g.tzw == Gw;
  // rectangle pixels inside the map (clipped rectangle, in rectangle coordinates)
  const int ry_lo = max(g.y0 - g.sy, 0), ry_hi = min(g.y1 - g.sy, g.tzh) - 1;
  const int rx_lo = max(g.x0 - g.sx, 0), rx_hi = min(g.x1 - g.sx, g.tzw) - 1;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int cv = (int)(e % CV);
    long long r = e / CV;
    const int j = (int)(r % p2); r /= p2;
    const int i = (int)(r % p1); r /= p1;
    const int zx = (int)(r % zn); r /= zn;
    const int zy = (int)(r % zn);
    const int b = (int)(r / zn);
    const int gy = zy * p1 + i, gx = zx * p2 + j;
    T* o = dz + (e / CV) * dz_ld + cv * VE;
    if (ident) {
      if (gy >= ry_lo && gy <= ry_hi && gx >= rx_lo && gx <= rx_hi)
        vcopy(dy + ((long long)(b * H + g.sy + gy) * W + g.sx + gx) * dy_ld + cv * VE, o);
      else
        vzero(o);
      continue;
    }
    int y_lo, y_hi, x_lo, x_hi;
    tap_range(gy, Gh, g.tzh, ry_lo, ry_hi, &y_lo, &y_hi);
    tap_range(gx, Gw, g.tzw, rx_lo, rx_hi, &x_lo, &x_hi);
    float acc[VE];
#pragma unroll
    for (int q = 0; q < VE; ++q) acc[q] = 0.f;
    for (int ry = y_lo; ry <= y_hi; ++ry) {
      const Tap t = tap(ry, Gh, g.tzh);
      if (t.i0 != gy && t.i1 != gy) continue;
      const float wy = tap_weight(t, gy);
      for (int rx = x_lo; rx <= x_hi; ++rx) {
        const Tap u = tap(rx, Gw, g.tzw);
        if (u.i0 != gx && u.i1 != gx) continue;
        vaxpy(wy * tap_weight(u, gx), dy + ((long long)(b * H + g.sy + ry) * W + g.sx + rx) * dy_ld + cv * VE, acc);
      }
    }
    Vec<T>::store(o, acc);
  }
}

// mode 0: out [B*H*W] = x with the rectangle's rows zeroed; 1: out [B*cap] = the rectangle's rows of x (row-major inside the
// rectangle, rows >= n_in zero); 2: out [B*H*W] = the adjoint of mode 1 (x [B*cap] back into the rectangle, zero elsewhere)
template <typename T>
__global__ __launch_bounds__(256) void zone_rect_rows_kernel(const T* __restrict__ x, int x_ld, const int* __restrict__ rec, T* __restrict__ out,
                                                             int out_ld, int B, int H, int W, int C, int cap, int mode) {
  constexpr int VE = Vec<T>::N;
  Rec g = load_rec(rec);
  g.y0 = max(g.y0, 0); g.y1 = min(g.y1, H); g.x0 = max(g.x0, 0); g.x1 = min(g.x1, W);      // never touch rows outside the map
  const int CV = C / VE, w = g.x1 - g.x0;
  const int n_in = min(max(g.n_in, 0), cap);
  const long long rows = mode == 1 ? (long long)B * cap : (long long)B * H * W;
  const long long total = rows * CV;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int cv = (int)(e % CV);
    const long long r = e / CV;
    T* o = out + r * out_ld + cv * VE;
    if (mode == 1) {
      const int b = (int)(r / cap), k = (int)(r - (long long)b * cap);
      if (k >= n_in || w <= 0) { vzero(o); continue; }
      const int py = g.y0 + k / w, px = g.x0 + k % w;
      if (py >= H || px >= W) { vzero(o); continue; }
      vcopy(x + ((long long)(b * H + py) * W + px) * x_ld + cv * VE, o);
      continue;
    }
    const int px = (int)(r % W), py = (int)((r / W) % H), b = (int)(r / ((long long)H * W));
    const bool in = py >= g.y0 && py < g.y1 && px >= g.x0 && px < g.x1;
    if (mode == 0) {
      if (in) vzero(o); else vcopy(x + r * x_ld + cv * VE, o);
    } else {
      const int k = in ? (py - g.y0) * w + (px - g.x0) : -1;
      if (k >= 0 && k < n_in) vcopy(x + ((long long)b * cap + k) * x_ld + cv * VE, o); else vzero(o);
    }
  }
}

}  // namespace

static inline unsigned zw_blocks(long long total) { return (unsigned)std::max(1ll, std::min((total + 255) / 256, 8192ll)); }

#define ZW_CHECK(name, a, b)                                                                                                        \
  CFP_REQUIRE(dtype_ok(dtype), CFP_EINVAL, name ": bad dtype");                                                                    \
  CFP_REQUIRE(a && b && rec && aligned16(a) && aligned16(b), CFP_EINVAL, name ": bad pointer");                                     \
  const int ve = vec_elems(dtype);                                                                                                  \
  CFP_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % ve == 0, CFP_ESHAPE, name ": bad shape");                                     \
  hipStream_t s = reinterpret_cast<hipStream_t>(stream)
#define ZW_LD(name, a, b) CFP_REQUIRE(a >= C && b >= C && a % ve == 0 && b % ve == 0, CFP_ESHAPE, name ": bad pitch")
#define ZW_ZONES(name) CFP_REQUIRE(zn > 0 && p1 > 0 && p2 > 0 && zn * p1 > 1 && zn * p2 > 1, CFP_ESHAPE, name ": bad zone grid")
#define ZW_DISPATCH(L) do { if (dtype == CFP_BF16) L(bf16_t); else if (dtype == CFP_F16) L(f16_t); else L(float); } while (0)

extern "C" int cfp_zone_crop(const void* tok, int tok_ld, const int* rec, void* out, int out_ld, int B, int H, int W, int C, int zn, int p1,
                             int p2, int dtype, cfp_stream_t stream) {
  ZW_CHECK("cfp_zone_crop", tok, out);
  ZW_ZONES("cfp_zone_crop");
  ZW_LD("cfp_zone_crop", tok_ld, out_ld);
  const unsigned nb = zw_blocks((long long)B * zn * zn * p1 * p2 * (C / ve));
#define L(T) hipLaunchKernelGGL(zone_crop_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)tok, tok_ld, rec, (T*)out, out_ld, B, H, W, C, zn, p1, p2)
  ZW_DISPATCH(L);
#undef L
  return cfp_check_launch("cfp_zone_crop");
}

extern "C" int cfp_zone_crop_bwd(const void* dz, int dz_ld, const int* rec, void* dtok, int dtok_ld, int B, int H, int W, int C, int zn, int p1,
                                 int p2, int dtype, cfp_stream_t stream) {
  ZW_CHECK("cfp_zone_crop_bwd", dz, dtok);
  ZW_ZONES("cfp_zone_crop_bwd");
  ZW_LD("cfp_zone_crop_bwd", dz_ld, dtok_ld);
  const unsigned nb = zw_blocks((long long)B * H * W * (C / ve));
#define L(T) hipLaunchKernelGGL(zone_crop_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)dz, dz_ld, rec, (T*)dtok, dtok_ld, B, H, W, C, zn, p1, p2)
  ZW_DISPATCH(L);
#undef L
  return cfp_check_launch("cfp_zone_crop_bwd");
}

extern "C" int cfp_zone_paste(const void* tok, int tok_ld, const void* z, int z_ld, const int* rec, void* out, int out_ld, int B, int H, int W,
                              int C, int zn, int p1, int p2, int dtype, cfp_stream_t stream) {
  ZW_CHECK("cfp_zone_paste", tok, out);
  ZW_ZONES("cfp_zone_paste");
  CFP_REQUIRE(z && aligned16(z), CFP_EINVAL, "cfp_zone_paste: bad pointer");
  ZW_LD("cfp_zone_paste", tok_ld, out_ld);
  ZW_LD("cfp_zone_paste", z_ld, z_ld);
  const unsigned nb = zw_blocks((long long)B * H * W * (C / ve));
#define L(T) hipLaunchKernelGGL(zone_paste_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)tok, tok_ld, (const T*)z, z_ld, rec, (T*)out, out_ld, \
                                B, H, W, C, zn, p1, p2)
  ZW_DISPATCH(L);
#undef L
  return cfp_check_launch("cfp_zone_paste");
}

extern "C" int cfp_zone_paste_bwd(const void* dy, int dy_ld, const int* rec, void* dz, int dz_ld, int B, int H, int W, int C, int zn, int p1,
                                  int p2, int dtype, cfp_stream_t stream) {
  ZW_CHECK("cfp_zone_paste_bwd", dy, dz);
  ZW_ZONES("cfp_zone_paste_bwd");
  ZW_LD("cfp_zone_paste_bwd", dy_ld, dz_ld);
  const unsigned nb = zw_blocks((long long)B * zn * zn * p1 * p2 * (C / ve));
#define L(T) hipLaunchKernelGGL(zone_paste_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)dy, dy_ld, rec, (T*)dz, dz_ld, B, H, W, C, zn, p1, p2)
  ZW_DISPATCH(L);
#undef L
  return cfp_check_launch("cfp_zone_paste_bwd");
}

extern "C" int cfp_zone_rect_rows(const void* x, int x_ld, const int* rec, void* out, int out_ld, int B, int H, int W, int C, int cap, int mode,
                                  int dtype, cfp_stream_t stream) {
  ZW_CHECK("cfp_zone_rect_rows", x, out);
  ZW_LD("cfp_zone_rect_rows", x_ld, out_ld);
  CFP_REQUIRE(mode >= 0 && mode <= 2 && (mode == 0 || cap > 0), CFP_EINVAL, "cfp_zone_rect_rows: bad mode / capacity");
  const unsigned nb = zw_blocks((mode == 1 ? (long long)B * cap : (long long)B * H * W) * (C / ve));
#define L(T) hipLaunchKernelGGL(zone_rect_rows_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)x, x_ld, rec, (T*)out, out_ld, B, H, W, C, cap, mode)
  ZW_DISPATCH(L);
#undef L
  return cfp_check_launch("cfp_zone_rect_rows");
}
