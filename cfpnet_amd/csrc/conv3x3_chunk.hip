// 16-bit 3x3 stride-1 convolution for DEEP inputs (Cin > 64): the input halo of a pixel tile goes through LDS one 64-channel chunk at a
// time, the weights one (tap, chunk) at a time, and two or three workgroups share a CU.
//
// Reference ops: the decoder's UpSampleBN convolutions on the concatenation [upsampled | skip] and on their own output (decoder.py:51-58,
// 168 / 312 / 392 -> 64 / 128 / 256 channels) and the DAPM's conv1 / conv2 on [x | msg] (128 / 256 input channels).  As implicit GEMMs
// (conv_igemm2.hip) they fetch every input pixel from L2 into LDS nine times, once per tap.  conv3x3_direct.hip has the right K order for
// them -- the halo of a chunk staged once, the nine taps as shifted views of it -- but its 128-channel tile holds 2 x 24 KB of halo and
// 2 x 48 KB of three-tap weight slabs: one workgroup per CU, a drained DMA queue and a barrier three times per chunk, the halo staged
// again per channel tile and an LDS C tile at the end.  This kernel keeps that K order and lays the work out as conv3x3_halo.hip does:
//
//   * a workgroup (four waves, 2 x 2) owns 8 x 16 output pixels and 64 output channels (tile 1) or 128 (tile 0); wider outputs take
//     several channel blocks, neighbours in the grid so that they meet the same halo in L2;
//   * K order: 64-channel chunk (outer) -> kh -> kw -> two 32-deep MFMA blocks in channel order, ONE accumulator per output --
//     conv3x3_direct_kernel's order, so the results are that kernel's bit for bit.  The channel tail of the last chunk reads the zero
//     word on both operands; its second 32-deep block is skipped when it holds no channel at all (as the direct kernel's `nsub`);
//   * one K-step = one (chunk, tap): its weights [channel block][64] are 128-byte rows of the standard [Cout][kh][kw][Cin] tensor,
//     LDS-DMA'd into XOR-swizzled rows, three stages of 8 KB (16 KB): the weights of two steps are in flight while one computes, and the
//     wait in front of a step's barrier is counted -- it leaves the next step's weights (and the halo registers) in flight;
//   * the chunk's halo, 10 x 18 pixels x 128 bytes, has ONE 24 KB buffer.  The next chunk's is fetched into registers in tap 5 (six
//     16-byte pieces per thread) and stored after tap 8 behind a barrier of its own, when nobody reads the old chunk any more;
//   * 3 x 8 + 24 = 48 KB for tile 1: THREE workgroups per CU (168 VGPRs); 3 x 16 + 24 = 72 KB for tile 0: two.  What decided the layout
//     was measured (profiles/conv3x3_chunk_ab.txt): with two DMA halo buffers the 64-channel tile takes 64 KB (two weight stages) or
//     72 KB (three) -- two per CU -- and runs 153600 px x 168 -> 64 in 50 us alone / 42 in flight either way; with one buffer and three
//     per CU 43 / 39.  The stage count alone changed nothing, the third workgroup did;
//   * accumulators transposed (weights as the MFMA row operand): a lane owns four consecutive channels of one pixel, and the epilogue
//     (scale / shift, activation, optional residual) stores 8 bytes from registers.  No LDS C tile;
//   * one raw barrier per K-step (+ one per chunk in front of the halo stores).
//
// Hand-over schedule (tools/probes/chunk16_schedule.cpp replays it on the host): step s = 9 chunk + tap reads weight stage s % 3 and the
// halo buffer.  Behind the barrier that opens step s every wave has left step s - 1, whose stage (s + 2) % 3 the weights of step s + 2
// may then overwrite.  The halo buffer is overwritten behind the extra barrier after tap 8, which every wave reaches with its last
// fragment read of the chunk done, and read again behind the barrier that opens tap 0, in front of which every wave has waited for its
// own stores.
#include "halo_core.h"

namespace {

// all but this wave's n youngest vector-memory operations have landed (n is wave-uniform and, the taps being unrolled, mostly a constant)
__device__ __forceinline__ void wait_vmcnt_dyn(int n) {
  switch (n) {
    case 0: wait_vmcnt<0>(); break;   case 1: wait_vmcnt<1>(); break;   case 2: wait_vmcnt<2>(); break;   case 3: wait_vmcnt<3>(); break;
    case 4: wait_vmcnt<4>(); break;   case 5: wait_vmcnt<5>(); break;   case 6: wait_vmcnt<6>(); break;   case 7: wait_vmcnt<7>(); break;
    case 8: wait_vmcnt<8>(); break;   case 9: wait_vmcnt<9>(); break;   case 10: wait_vmcnt<10>(); break;
    default: wait_vmcnt<0>(); break;      // (never more than NB + LB = 10: waiting for everything is always correct)
  }
}

template <typename H, int NT, int WN>
__global__ __launch_bounds__(256, NT <= 2 ? 3 : 2) void conv3x3_chunk_kernel(ConvP p, HaloGeo hp) {
  using T = HaloTile<NT, WN>;
  constexpr int TH = T::TH, NB = T::NB, WSTAGE = T::WSTAGE;
  constexpr int ST = kChunk16Stages;           // weight stages
  constexpr int HC = 18;                       // halo columns
  constexpr int HPIX = (TH + 2) * HC;
  constexpr int LB = (HPIX + 31) / 32;         // 16-byte halo pieces per thread: a pass of the workgroup is 32 pixels x 8 pieces
  constexpr int kTapLoad = 5;                  // the tap whose step fetches the next chunk's halo into registers
  static_assert(ST == 3 && kTapLoad + ST - 1 <= 8, "the halo registers are waited for by the counted waits of taps 6 and 7");
  static_assert(NB + LB <= 10, "wait_vmcnt_dyn");
  static_assert(T::NBG % 4 == 0, "every wave stages the same number of weight groups");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sW = smem;                    // ST weight stages
  unsigned char* sX = smem + ST * WSTAGE;      // the halo buffer: LB * 32 pixel rows of 128 bytes (chunk16_halo_buf)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int fr = lane & 15, fq = lane >> 4;
  const int rsub = lane >> 3;                  // row of an 8-row DMA group
  const int lc = (lane & 7) ^ rsub;            // logical 16-byte chunk this lane fetches into physical chunk lane & 7

  const HaloWg wg = halo_wg<NT, WN>(hp);
  const int n_base = wg.n_base, x0 = wg.x0, y0 = wg.y0, b = wg.b;

  const H* __restrict__ in = reinterpret_cast<const H*>(p.in) + (long long)b * p.H * p.W * p.in_ld;
  const H* __restrict__ wt = reinterpret_cast<const H*>(p.w);
  const H* zsrc = reinterpret_cast<const H*>(g_zero16);

  // ---- per-thread bookkeeping of the loaders: element offsets, -1 = the zero word ----
  int a_off[LB];        // halo pixel i * 32 + tid / 8, chunk tid & 7, inside the image (one image < 2^31 elements: host check)
#pragma unroll
  for (int i = 0; i < LB; ++i) {
    const int hpx = i * 32 + (tid >> 3);
    const int hy = hpx / HC, hx = hpx - hy * HC;
    const int y = y0 - p.pad_t + hy, x = x0 - p.pad_l + hx;
    const bool ok = hpx < HPIX && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
    a_off[i] = ok ? (y * p.W + x) * p.in_ld + (tid & 7) * 8 : -1;
  }
  int b_off[NB];        // weight row (+ this lane's chunk) of tap 0, chunk 0 (Cout * K < 2^31: host check)
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int n = n_base + (j * 4 + wave) * 8 + rsub;
    b_off[j] = n < p.Cout ? n * p.K + lc * 8 : -1;
  }
  const int nchunks = (p.Cin + 63) >> 6;
  const int nsteps = nchunks * 9;

  u32x4 hv[LB];
  auto load_h = [&](int chunk) {      // this thread's pieces of a chunk's halo, all in flight together.  Unconditional loads: what lies outside
    const int c0 = chunk * 64;        // the image or past Cin reads the zero word
    const bool cok = c0 + (tid & 7) * 8 < p.Cin;
#pragma unroll
    for (int i = 0; i < LB; ++i) hv[i] = *reinterpret_cast<const u32x4*>((cok && a_off[i] >= 0) ? in + a_off[i] + c0 : zsrc);
  };
  auto store_h = [&]() {              // pixel rows of 128 bytes, chunk ^ (pixel & 7): the 16 lanes of an MFMA operand read (16 consecutive
#pragma unroll                        // pixels, one chunk) fall on 16 different 16-byte slots
    for (int i = 0; i < LB; ++i) {
      const int hpx = i * 32 + (tid >> 3);
      *reinterpret_cast<u32x4*>(sX + hpx * 128 + (((tid & 7) ^ (hpx & 7)) * 16)) = hv[i];
    }
  };
  auto issue_w = [&](int chunk, int tap, int buf) {
    const int c0 = chunk * 64;
    const bool cok = c0 + lc * 8 < p.Cin;
    const int koff = tap * p.Cin + c0;
#pragma unroll
    for (int j = 0; j < NB; ++j) glds16((cok && b_off[j] >= 0) ? wt + b_off[j] + koff : zsrc, sW + buf * WSTAGE + (j * 4 + wave) * 1024);
  };

  f32x4 acc[4][NT];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[g][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: the halo of chunk 0 and the weights of the first ST - 1 steps (a chunk has nine: they exist) ----
  load_h(0);
#pragma unroll
  for (int s = 0; s < ST - 1; ++s) issue_w(0, s, s);
  store_h();

  const int px0 = (wm * 4) * HC + fr;          // halo pixel of tap (0, 0) of this lane's output pixel in row wm * 4
  const int wrow = (wn * NT * 16 + fr) * 128;  // this lane's weight row of channel tile 0
  const int wsw = fr & 7;

  int stage = 0;                               // s % ST
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    const bool more = chunk + 1 < nchunks;
    const int nsub = (p.Cin - chunk * 64) > 32 ? 2 : 1;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int s = chunk * 9 + tap;
      // This wave's weights of step s, and everything older, have landed.  Younger and left in flight: the weights of step s + 1 and, in
      // tap 6, the halo registers (issued in tap 5 in front of the weights of step s + 1; the wait of tap 7 retires them)
      wait_vmcnt_dyn(min(nsteps - 1 - s, ST - 2) * NB + ((tap == kTapLoad + 1 && more) ? LB : 0));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // fragment reads of the previous step; at tap 0 this wave's halo stores
      __builtin_amdgcn_s_barrier();          // ... for every wave, and every wave has left the previous step.  Raw: a __syncthreads() would drain the DMA queue
      asm volatile("" ::: "memory");
      if (tap == kTapLoad && more) load_h(chunk + 1);
      {                                        // the weights of step s + ST - 1 into the stage that step s - 1 read
        const int t2 = tap + ST - 1;
        const int nstage = stage == 0 ? ST - 1 : stage - 1;
        if (t2 < 9) issue_w(chunk, t2, nstage);
        else if (more) issue_w(chunk + 1, t2 - 9, nstage);
      }

      const unsigned char* cW = sW + stage * WSTAGE + wrow;
      const int kh = tap / 3, kw = tap - 3 * (tap / 3);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        if (sub < nsub) {      // wave-uniform
          s16x8 wf[NT], xf[4];
#pragma unroll
          for (int j = 0; j < NT; ++j) wf[j] = *reinterpret_cast<const s16x8*>(cW + j * 16 * 128 + (((sub * 4 + fq) ^ wsw) * 16));
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int hpx = px0 + (g + kh) * HC + kw;
            xf[g] = *reinterpret_cast<const s16x8*>(sX + hpx * 128 + (((sub * 4 + fq) ^ (hpx & 7)) * 16));
          }
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[g][j] = mfma16<H>(wf[j], xf[g], acc[g][j]);      // acc[r] = channel 4 fq + r of tile j, pixel fr
        }
      }
      stage = stage == ST - 1 ? 0 : stage + 1;
    }
    if (more) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();          // every wave has read its last fragment of this chunk's halo
      asm volatile("" ::: "memory");
      store_h();                             // (read behind the barrier that opens tap 0)
    }
  }

  // ---- epilogue: folded BatchNorm / bias, activation, optional skip; 8-byte stores from the accumulators ----
  H* __restrict__ out = reinterpret_cast<H*>(p.out) + (long long)b * p.Ho * p.Wo * p.out_ld;
  const H* __restrict__ res = p.res ? reinterpret_cast<const H*>(p.res) + (long long)b * p.Ho * p.Wo * p.res_ld : nullptr;
  const int x = x0 + fr;
  f32x4 sc[NT], sh[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n_base + (wn * NT + j) * 16 + fq * 4;
    const bool ok = n < p.Cout;
    sc[j] = (ok && p.scale) ? *reinterpret_cast<const f32x4*>(p.scale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
    sh[j] = (ok && p.shift) ? *reinterpret_cast<const f32x4*>(p.shift + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  with_act(p.act, [&](auto A) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int y = y0 + wm * 4 + g;
      const bool pix_ok = y < p.Ho && x < p.Wo;
      const long long pix = (long long)y * p.Wo + x;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = n_base + (wn * NT + j) * 16 + fq * 4;
        float yv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) yv[r] = act_c16<decltype(A)::value>(acc[g][j][r] * sc[j][r] + sh[j][r]);
        uint2 pk;
        pk.x = pack2<H>(yv[0], yv[1]);
        pk.y = pack2<H>(yv[2], yv[3]);
        if (!(pix_ok && n < p.Cout)) continue;
        if (res) {
          // the skip is added to the ROUNDED activation, as the other conv kernels do (they round into their LDS C tile first)
          const uint2 rr = *reinterpret_cast<const uint2*>(res + pix * p.res_ld + n);
          const H* ph = reinterpret_cast<const H*>(&pk);
          const H* rh = reinterpret_cast<const H*>(&rr);
          H oh[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) oh[r] = from_f32<H>(to_f32<H>(ph[r]) + to_f32<H>(rh[r]));
          pk = *reinterpret_cast<const uint2*>(oh);
        }
        *reinterpret_cast<uint2*>(out + pix * p.out_ld + n) = pk;
      }
    }
  });
}

// tiles: {NT, WN} of HaloTile -- 0: 128 channels x 8 x 16 pixels (72 KB), 1: 64 channels x 8 x 16 pixels (48 KB)
constexpr HCfg kChunkCfg[] = {{4, 2}, {2, 2}};
constexpr int kNumChunkCfg = sizeof(kChunkCfg) / sizeof(kChunkCfg[0]);

template <typename H, int NT, int WN>
int launch_c(const ConvP& p, hipStream_t s) {
  constexpr HaloTileV t = halo_tile(NT, WN);
  HaloGeo hp{};
  if (!halo_geo<NT, WN>(hp, p, 8, 128)) return -1;
  return halo_launch<conv3x3_chunk_kernel<H, NT, WN>>(p, hp, chunk16_lds(t), s);
}

}  // namespace

int conv3x3_chunk_num_variants() { return kNumChunkCfg; }
size_t conv3x3_chunk_lds(int v) { return v >= 0 && v < kNumChunkCfg ? chunk16_lds(halo_tile(kChunkCfg[v].nt, kChunkCfg[v].wn)) : 0; }

// The problems this kernel takes: 3x3, stride 1, undilated, 16-bit, more than 64 input channels in 16-byte vectors, shared weights, no
// LayerNorm epilogue, no moments, no two-term weights, one source; 32-bit element offsets inside an image and inside the weights.
bool conv3x3_chunk_takes(const ConvP& p) {
  return p.KH == 3 && p.KW == 3 && p.stride == 1 && p.dil <= 1 && p.Cin > 64 && p.Cin % 8 == 0 && p.Cout % 8 == 0 && p.K == 9 * p.Cin &&
         p.ln_gamma == nullptr && p.rows_per_batch == 0 && p.k2 == 0 && p.mom == nullptr && p.up_src == nullptr &&
         p.pad_t >= 0 && p.pad_l >= 0 && p.pad_t <= 2 && p.pad_l <= 2 &&
         (long long)p.H * p.W * p.in_ld < (1ll << 31) && (long long)p.Cout * p.K < (1ll << 31);
}

// Returns 0, or a negative value if the variant does not exist or the launch does not fit.
int conv3x3_chunk_launch(int v, const ConvP& p, hipStream_t s) {
  if (!conv3x3_chunk_takes(p)) return -3;
#define HC_(NT, WN) (p.f16 ? launch_c<f16_t, NT, WN>(p, s) : launch_c<bf16_t, NT, WN>(p, s))
  switch (v) {
    case 0: return HC_(4, 2);
    case 1: return HC_(2, 2);
    default: return -3;
  }
#undef HC_
}
