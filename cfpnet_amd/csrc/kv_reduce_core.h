// The key/value reduction of the linear attention, shared by its two kernels: kv_reduce_kernel (attention.hip) reads projected K / V rows
// from global memory, kv_project_reduce_kernel (attn_kv_project.hip) projects them itself and reads them from its LDS tile.  Which keys
// form a (group, split) and the whole arithmetic on them -- lane mapping, key order per lane, inv_len scaling, elu1, the fmaf chain, the
// butterfly, the padding term and the destination -- is this one body; the kernels differ only in where a key's K and V rows are found
// (the KEYS argument), so their sums are the same code on the same values.
#pragma once
#include "common.h"

struct KvP {
  const void* k; const void* v;
  float* kv; float* ksum; float* ws;
  int k_ld, v_ld;
  int NB, Hk, Wk, th, tw, gy, gx;
  int cy0, cy1, cx0, cx1;
  int count_pad, heads, d, nsplit;
  float inv_len;
  const int* rec;      // DEV only (last: the scalar instantiation's argument offsets stay): the zone record, see cfp_attn_kv_reduce_dev
};

// IC rows of the d x d accumulator per lane; TPK = d / IC lanes per key; KL = 64 / TPK key lanes.
template <int D> struct KvCfg;
// The cross-lane sum over the KL key lanes is a butterfly of log2(KL) steps x (IC * d + IC) `ds_bpermute`s: with a lane holding all d
// rows (IC = d at d = 8) that was 432 of the kernel's 946 vector instructions.  Two rows per lane (TPK = d / 2 lanes share a key and
// load its V row together) leave 16 / 8 key lanes: 72 / 102 permutes at d = 8 / 16, the same two to four load rounds per lane.
template <> struct KvCfg<4>  { static constexpr int IC = 1; };
template <> struct KvCfg<8>  { static constexpr int IC = 2; };
template <> struct KvCfg<16> { static constexpr int IC = 2; };
template <> struct KvCfg<32> { static constexpr int IC = 2; };

// The keys of (group g, split sp): key s of the group's rectangle sits at (y0 + s / rw, x0 + s % rw) of image b, the split owns
// s_begin <= s < s_end.
struct KvGeom { int b, y0, x0, rw, S, s_begin, s_end; float inv_len; };

// DEV: the clip rectangle and v_length come from the int32[9] zone record in device memory (y0, y1, x0, x1, n_inside: uniform loads)
// instead of the host's integers; everything after that is the scalar instantiation's own code.
template <bool DEV>
__device__ __forceinline__ KvGeom kv_group_geom(const KvP& p, int g, int sp) {
  KvGeom q;
  const int gpb = p.gy * p.gx;
  const int gi = g % gpb;
  q.b = g / gpb;
  const int ty = gi / p.gx, tx = gi % p.gx;
  int cy0 = p.cy0, cy1 = p.cy1, cx0 = p.cx0, cx1 = p.cx1;
  q.inv_len = p.inv_len;
  if constexpr (DEV) {
    const int* __restrict__ rec = p.rec;
    cy0 = rec[4]; cy1 = rec[5]; cx0 = rec[6]; cx1 = rec[7];
    q.inv_len = 1.0f / (float)max(rec[8], 1);      // the host's expression: 1 / v_length, v_length = max(n_inside, 1)
  }
  // key rectangle of this group: tile, clipped to the grid and to the clip rectangle
  q.y0 = max(max(ty * p.th, cy0), 0);
  q.x0 = max(max(tx * p.tw, cx0), 0);
  const int y1 = min(min((ty + 1) * p.th, cy1), p.Hk);
  const int x1 = min(min((tx + 1) * p.tw, cx1), p.Wk);
  const int rh = max(y1 - q.y0, 0);
  q.rw = max(x1 - q.x0, 0);
  q.S = rh * q.rw;
  const int per = (q.S + p.nsplit - 1) / p.nsplit;
  q.s_begin = sp * per;
  q.s_end = min(q.S, q.s_begin + per);
  return q;
}

// Keys in global memory.  key s of the rectangle sits at (y0 + s / rw, x0 + s % rw): the lane's position advances by KL keys per load, so
// the division happens once (the quotient / remainder of the step and of the first and last key) and every step after that is an add and
// one wrap -- the per-key signed division was ~35 VALU instructions against 2 D = 8 .. 64 FMAs
template <typename T>
struct KvGlobalKeys {
  const T* K; const T* V;
  long long k_ld, v_ld;
  int b, Hk, Wk, y0, x0, rwd, step_q, step_r, cy, cx, ly, lx;
  __device__ __forceinline__ KvGlobalKeys(const KvP& p, const KvGeom& q, int kl, int KL)
      : K(reinterpret_cast<const T*>(p.k)), V(reinterpret_cast<const T*>(p.v)), k_ld(p.k_ld), v_ld(p.v_ld), b(q.b), Hk(p.Hk), Wk(p.Wk),
        y0(q.y0), x0(q.x0) {
    rwd = max(q.rw, 1);
    step_q = KL / rwd; step_r = KL - step_q * rwd;
    const int s_first = min(q.s_begin + kl, max(q.s_end - 1, 0));
    cy = s_first / rwd; cx = s_first - cy * rwd;                      // (row, column) of key s0 + u * KL, before clamping
    ly = max(q.s_end - 1, 0) / rwd; lx = max(q.s_end - 1, 0) - ly * rwd;      // of the last key (what the clamped tail loads read)
  }
  // the next key of this lane (`in`: it exists, else the split's last key is read and not used); K and V row pointers
  __device__ __forceinline__ void next(bool in, const T*& kp, const T*& vp) {
    const int yy = y0 + (in ? cy : ly), xx = x0 + (in ? cx : lx);
    cx += step_r; cy += step_q;
    if (cx >= rwd) { cx -= rwd; ++cy; }
    const long long row = ((long long)b * Hk + yy) * Wk + xx;
    kp = K + row * k_ld;
    vp = V + row * v_ld;
  }
};

// Keys in an LDS tile of the split's projected rows: row s - s_begin holds [K (DM) | V (DM)] of key s, pitch `ld` elements.
template <typename T>
struct KvTileKeys {
  const T* tile;
  int ld, dm, cur, step, last;
  __device__ __forceinline__ KvTileKeys(const T* tile_, int ld_, int dm_, const KvGeom& q, int kl, int KL)
      : tile(tile_), ld(ld_), dm(dm_), cur(kl), step(KL), last(max(q.s_end - 1 - q.s_begin, 0)) {}
  __device__ __forceinline__ void next(bool in, const T*& kp, const T*& vp) {
    const int r = in ? cur : last;
    cur += step;
    kp = tile + r * ld;
    vp = kp + dm;
  }
};

// One wave: the d x d state of (group g, head h, split sp).  D = the head dimension d.
template <typename T, int D, typename KEYS>
__device__ __forceinline__ void kv_reduce_body(const KvP& p, const KvGeom& q, int g, int h, int sp, int lane, KEYS& keys) {
  constexpr int IC = KvCfg<D>::IC;
  constexpr int TPK = D / IC;
  constexpr int KL = 64 / TPK;
  const int ip = lane % TPK, kl = lane / TPK;
  const int s_begin = q.s_begin, s_end = q.s_end;
  const float inv_len = q.inv_len;

  float acc[IC][D];
  float ks[IC];
#pragma unroll
  for (int i = 0; i < IC; ++i) {
    ks[i] = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) acc[i][j] = 0.f;
  }
  // KU keys per iteration, their loads issued together: the loop is a chain of memory round trips (one per key before), not FMAs
  constexpr int KU = 4;
  for (int s0 = s_begin + kl; s0 < s_end; s0 += KL * KU) {
    float kf[KU][IC], vf[KU][D];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const bool in = s0 + u * KL < s_end;
      const T* kr; const T* vr;
      keys.next(in, kr, vr);
      const T* kp = kr + h * D + ip * IC;
      const T* vp = vr + h * D;
#pragma unroll
      for (int i = 0; i < IC; ++i) kf[u][i] = to_f32<T>(kp[i]);
#pragma unroll
      for (int j = 0; j < D; ++j) vf[u][j] = to_f32<T>(vp[j]);
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      if (s0 + u * KL >= s_end) continue;              // same order of accumulation per lane as the one-key loop
#pragma unroll
      for (int j = 0; j < D; ++j) vf[u][j] *= inv_len;
#pragma unroll
      for (int i = 0; i < IC; ++i) {
        const float kk = elu1(kf[u][i]);
        ks[i] += kk;
#pragma unroll
        for (int j = 0; j < D; ++j) acc[i][j] = fmaf(kk, vf[u][j], acc[i][j]);
      }
    }
  }
  // butterfly over the key lanes (lanes with equal ip)
#pragma unroll
  for (int o = TPK; o < 64; o <<= 1) {
#pragma unroll
    for (int i = 0; i < IC; ++i) {
      ks[i] += __shfl_xor(ks[i], o, 64);
#pragma unroll
      for (int j = 0; j < D; ++j) acc[i][j] += __shfl_xor(acc[i][j], o, 64);
    }
  }
  if (kl == 0) {
    // zero-padded window positions: K' = elu(0)+1 = 1, V = 0 (only the first split adds them)
    float padk = 0.f;
    if (p.count_pad && sp == 0) padk = (float)(p.th * p.tw - q.S);
    float* dkv; float* dks;
    if (p.nsplit == 1) {
      dkv = p.kv + ((long long)g * p.heads + h) * D * D;
      dks = p.ksum + ((long long)g * p.heads + h) * D;
    } else {
      float* base = p.ws + (((long long)g * p.heads + h) * p.nsplit + sp) * (D * D + D);
      dkv = base; dks = base + D * D;
    }
#pragma unroll
    for (int i = 0; i < IC; ++i) {
      dks[ip * IC + i] = ks[i] + padk;
#pragma unroll
      for (int j = 0; j < D; ++j) dkv[(ip * IC + i) * D + j] = acc[i][j];
    }
  }
}

// attention.hip: the split count of a launch, the finishing sum of the split slabs and the parameter fill with its checks
int kv_pick_nsplit(int S, long long groups_heads);
int kv_fill_params(KvP& p, float* kv, float* ksum, float* ws, int NB, int Hk, int Wk, int th, int tw, int cy0, int cy1, int cx0, int cx1,
                   int count_pad, float v_length, const int* rec, int heads, int d, const char* who);
void kv_finalize_launch(const KvP& p, hipStream_t s);
