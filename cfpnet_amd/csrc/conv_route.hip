// The routing policy of the dense convolutions / linear layers: which of the eight kernel families (gen-1 and few-row GEMMs of
// conv_igemm.hip, conv_igemm2.hip, conv3x3_direct.hip, conv3x3_halo.hip, conv3x3_chunk.hip, conv_igemm_x3.hip, the halo and chunk tiles of
// conv3x3_halo_x3.hip) runs a problem, with which tile and how many K splits.  conv_route() is the ONLY place that decides: conv2d_impl
// (conv_entry.hip) launches what it returns, cfp_conv2d_plan / cfp_conv2d_ws_bytes report what it returns for the canonical problem of
// their arguments.  The rule functions carry the measurements each threshold was fitted on; cfp_debug_set lives here because most of its
// keys are planning switches.
#include "conv_route.h"

namespace {

int tile_count(int variant, int M, int Cout) {
  static const int bm[4] = {256, 256, 128, 128}, bn[4] = {16, 32, 64, 128};
  return cdiv(M, bm[variant]) * cdiv(Cout, bn[variant]);
}

// K-splits for a problem on gen-1 tile `variant`: only when the grid would leave most CUs idle and K is long.
int pick_splits(int variant, int M, int Cout, int K, int dtype) {
  const int bk = is16(dtype) ? 32 : 16;
  const int nk = cdiv(K, bk);
  const int tiles = tile_count(variant, M, Cout);
  if (tiles >= 128 || nk < 16) return 1;
  int s = cdiv(256, tiles);
  if (s > nk / 6) s = nk / 6;
  if (s > 32) s = 32;
  return s < 2 ? 1 : s;
}

}  // namespace

// ---- debug knobs (tools/conv_bench.py): key 0 = force gen-2 variant (-1 auto), key 1 = force K-splits
// (-1 auto), key 2 = 1 routes bf16 through the first-generation kernel.  Not thread-safe; test use only.
static int g_force_variant = -1, g_force_splits = -1;
int g_use_v1 = 0;
int g_tput = 0;                 // cfp_debug_set key 17 (tools): 1 = every call plans for several batches in flight; callers say it per call with the
                                // CFP_CONV_IN_FLIGHT bit of cfp_conv2d_nhwc_ex's flags (Engine does while it captures in-flight slots).
                                // Side by side, what a launch costs is the resources it holds, not its own latency, and the sweep with four
                                // copies running together (tools/conv_bench.py --sweep --inflight 4, three runs, profiles/r3_conv_sweep_inflight4.json)
                                // prefers larger tiles than the isolated sweep the default plan is fitted on
int g_probe = 0;                // cfp_debug_set key 16: ConvP.probe
int g_x3_ad = 0;                // cfp_debug_set key 29: f16x3 implicit GEMMs with four row waves take their A-direct form (A values global -> registers)
int g_x3_small_m = 4800, g_x3_small_k = 1 << 30;      // cfp_debug_set keys 33 / 34: single-image plans take the 32 x 64 tile up to this many rows / this K
int g_x3_occ = 1;            // cfp_debug_set key 32: 0 = in-flight plans keep the unconstrained instantiations of the 64 x 64 / 128 x 32 / 64 x 128 tiles
static int x3_occ_of(int v) { return v == 13 ? 34 : v == 16 ? 35 : v == 15 ? 36 : v; }
static int x3_ad_of(int v) { return v == 26 ? 28 : v == 14 ? 29 : v == 13 ? 30 : v == 23 ? 31 : v == 16 ? 32 : v; }
int g_small_s2 = 1;             // cfp_debug_set key 15: 0 = three-stage 64x64 tiles for the small GEMMs (the round-2 plan)
int g_up_halo = 1;              // cfp_debug_set key 14: cfp_upsample_cat_conv3x3 through the halo kernel: 0 never, 1 where planned, 2 wherever it can run
int g_halo_s2 = 1;              // cfp_debug_set key 18: 0 = stride-2 convs never take the halo kernel
int g_halo = 1;                 // cfp_debug_set key 12: 0 = never take the whole-depth halo kernel, 2 = wherever it can run
// Where conv3x3_halo.hip beats the implicit GEMMs (tools/conv_bench.py --halo at batch 8, us halo / without: 614400 px x 16 ch, K = 360:
// 28 / 43; K = 144: 24 / 31; x 32 ch: 28 / 40; 153600 px x 160 ch: 38 / 50; 614400 x 128: 81 / 84) and where it does not (153600 px
// x 32 / 64 ch: 18-25 / 16-24, 38400 px: 13-23 / 11-23): the thin-output layers at full resolution and the wide expand convs.
// stride 2 (tools/conv_bench.py --halo, us with / without): stem 614400 x 40 x 72 25.5-27 / 29, 153600 x 64 x 144 23.4 / 26, 38400 x 160 x 360 20.8 / 23.4
extern int g_bin_head_x3_rows;  // conv_igemm_x3.hip
int g_x3_ln_fused = 1;          // cfp_debug_set key 26: 0 = the f16x3 GEMMs run a following LayerNorm as a second kernel
int g_halo_x3 = 1;              // cfp_debug_set key 24: 0 = the f16x3 3x3 convolutions never take the halo kernel
// where conv3x3_halo_x3.hip replaces the f16x3 implicit GEMM: many pixels (the halo and the weights of a channel block are fetched once
// per workgroup instead of nine times / once per 128 rows) and an input depth whose halo fits LDS
// (tools/conv_bench_x3.py --halo, us halo / implicit GEMM, alone and with four copies side by side; profiles/r4_conv_bench_x3_halo_*.txt):
// it wins where the input is SHALLOW -- 614400 px: 32 -> 128 ch 152 / 188 in flight (167 / 207 alone), 40 -> 16 63 / 83, 32 -> 32 60 / 73,
// 16 -> 16 23 / 41; 153600 px 40 -> 160 62 / 97; 38400 px 56 -> 224 33 / 41 -- and loses from 64 input channels up (the head's 128 -> 128:
// 692 / 573, 153600 px 168 -> 64: 182 / 136, 38400 px 128 -> 64: 39 / 23): a deep halo leaves one workgroup per CU, whose load phase
// (95-124 KB through registers) nothing overlaps, where the implicit GEMM pipelines its operand stream over K.
// alone (one graph at a time) the halo kernel already wins at half the pixels (batch 1: 19200 px x 160 x 360 19.3 vs 24.2 us, profiles/r4_conv_bench_x3_b1_alone.txt)
static bool halo_x3_wins(long long M, int Cin, int Cout, bool tput) { return M >= (tput ? 30000 : 15000) && Cin <= 56; }
// Deep inputs (Cin % 32 == 0, >= 64): which tile of the chunk-pipelined kernel, or -1 = the implicit GEMM.  Round 5: the single-chunk-buffer tiles
// (36: 128 channels x 8 x 16 pixels, 61 KB; 38: 64 channels x 16 x 16 pixels, 68 KB) hold TWO workgroups per CU, whose load / split / MFMA / store
// phases cover each other -- tools/probes/chunk_x3_inflight.py, us per call with four copies side by side (alone):
//   614400 px 128 -> 128 (head conv)  464 (490) against 529 (577) for the 256-pixel double-buffered tile 22;  76800 px (batch 1): 62 (84) vs 79 (95)
//   153600 px  64 -> 64   35 (54) vs 44 (54) for tile 24;   64 -> 32: 30 (46) vs 40 (51);   64 -> 128: 68 (74) vs 88 (96, implicit GEMM)
//    38400 px 128 -> 128  32 (59) vs 47 (80, implicit GEMM); 256 -> 128: 61 (92) vs 88 (143); 128 -> 64: 16 (42) vs 21 (38): in flight only
//     9600 px 256 -> 256  35 (72) vs 45 (73, implicit GEMM); 128 / 256 -> 128: the implicit GEMM stays ahead (12.4 / 22.4 vs 13.7 / 23.7)
// Round 5, late (tools/conv_bench_x3.py --halo with the single-buffer tiles in the sweep, batch 1 alone and batch 8 with four copies in flight):
//   * ONE input chunk (Cin = 32) is a problem for these tiles too: 32 -> 32 through tile 45 beats the whole-depth halo kernel (614400 px 50.5 vs 56.7 us in
//     flight, 76800 px alone 14.0 vs 14.6), and a single image's 32 -> 128 (the head's conv0, 76800 px) runs 28.4 us through tile 44 against 34.1;
//   * a single graph's 65 ... 128 output channels below 200 000 pixels: tile 44 (64 channels x 8 x 16 pixels, two channel blocks) instead of 36 --
//     the head conv of one image is 600 workgroups of tile 36 on 512 slots (two rounds for 1.17 rounds of work); 1 200 half-size ones: 74.7 vs 82.5 us;
//   * 32 output channels alone: tile 45 from 15 000 pixels (19200 px 64 -> 32: 14.5 vs 16.1 us through the implicit GEMM).
static int chunk_x3_variant(long long M, int Cin, int Cout, bool tput) {
  if (Cin % 32 != 0) return -1;
  if (Cin == 32) {
    if (Cout <= 32) return M >= 30000 ? 45 : -1;
    if (Cout > 64 && Cout <= 128 && !tput) return (M >= 30000 && M < 200000) ? 44 : -1;
    return -1;
  }
  if (Cout > 128) return (tput && M >= 9000) ? 36 : -1;
  if (Cout > 64) return M >= 30000 ? ((!tput && M < 200000) ? 44 : 36) : -1;
  if (Cout <= 32) return M >= (tput ? 30000 : 15000) ? 45 : -1;      // 32 channels x 8 x 16 pixels, 37 KB (four per CU): 614400 px 96 -> 32 (up4's first conv on the padded
                                                    // concatenation) 127 (136) vs 174 (187) for the 64-channel tile 38; 153600 px 64 -> 32: 20 (35) vs 30 (45)
  if (M >= 100000) return 38;
  if (M >= 30000) return tput ? 38 : 24;
  return -1;
}
int g_chunk16 = 1;              // cfp_debug_set key 40: the 16-bit 3x3 convolutions on deep inputs take the chunk kernel (conv3x3_chunk.hip) 0 = never, 1 = where planned,
                                // 2 = wherever it can run (the 128-channel tile above 64 output channels, the 64-channel tile below)
// Deep inputs (Cin > 64, Cin % 8 == 0) in the 16-bit modes: which tile of conv3x3_chunk.hip, or -1 = today's plan (implicit GEMM / direct kernel).
// Fitted on tools/conv_bench.py --chunk at batch 8, alone and with four copies side by side (profiles/conv3x3_chunk_ab.txt; us per call, today's
// plan three times -> tile 1, the 64-channel tile with three workgroups per CU; tile 0 ties it in flight at 128 output channels and loses alone):
//                                    alone                          four in flight
//   153600 px  168 ->  64   58.8 / 59.9 / 60.7 -> 43.1      50.5 / 50.7 / 51.1 -> 38.8
//    38400 px  312 -> 128   48.1 / 48.5 / 49.0 -> 38.1      38.0 / 38.0 / 38.1 -> 30.4
//    38400 px  128 -> 128   21.5 / 21.6 / 21.9 -> 18.3      15.1 / 15.1 / 15.2 -> 12.5
//    38400 px  128 ->  64   15.7 / 15.8 / 16.1 -> 13.9       7.9 /  7.9 /  8.0 ->  6.6
//     9600 px  392 -> 256   41.9 / 42.5 / 43.2 -> 37.1      21.6 / 22.1 / 22.2 -> 22.7  (stays: the 128 x 128 implicit GEMM)
//     9600 px  256 -> 256   29.1 / 29.1 / 29.3 -> 23.7      12.4 / 12.4 / 12.4 -> 13.3  (stays)
//     9600 px  256 -> 128   16.2 / 16.3 / 16.3 -> 18.8  (stays: direct tile 4)     10.4 / 10.6 / 10.6 ->  7.3
//     9600 px  128 -> 128   10.8 / 10.9 / 10.9 -> 13.4  (stays)                      6.8 /  6.8 /  6.8 ->  5.0
// Only what was measured moves: 30 000 ... 200 000 pixels, and around 9 600 pixels the wide outputs alone and the narrow ones in flight.
static int chunk16_variant(long long M, int Cin, int Cout, bool tput) {
  if (Cin <= 64 || Cin % 8 != 0 || Cout <= 0 || Cout % 8 != 0 || M <= 0 || g_chunk16 == 0) return -1;
  if (g_chunk16 == 2) return Cout > 64 ? 0 : 1;
  if (M >= 30000 && M < 200000) return 1;
  if (M >= 8000 && M < 12000) return (Cout > 128) != tput ? 1 : -1;
  return -1;
}
extern "C" int cfp_conv3x3_chunk_variant(int M, int Cin, int Cout, int in_flight) { return chunk16_variant(M, Cin, Cout, in_flight > 1); }
static bool halo_wins_s2(long long M, int Cout) { return g_halo == 2 || (g_halo == 1 && g_halo_s2 && M >= 30000 && Cout <= 160); }
static bool halo_wins(long long M, int Cout, bool tput) {
  if (g_halo == 2) return true;
  if (g_halo == 1 && tput && M >= 100000 && Cout <= 64) return true;      // 153600 px x 32 / 64 ch: 8 x 16 pixel tiles, 10.6 -> 7.6 / 12.9 -> 10.8 / 20.8 -> 16.7 us per call in flight
  return g_halo == 1 && ((M >= 300000 && (Cout <= 32 || Cout == 128)) || (M >= 100000 && Cout > 128 && Cout <= 160) ||
                         (M >= 30000 && Cout > 160 && Cout <= 256));          // 38400 px x 224 ch (two 128-channel blocks): 19.8 / 22.9
}
void cfp_tail_x3_debug_set(int value);      // loftr_tail_x3.hip: key 35 = waves per workgroup of the fused tails (0 = by the row count)
void cfp_fold_debug_set(int v);
void cfp_tail16_debug_set(int value);
void cfp_pw_rows_debug_set(int value);      // pw_rows.hip: key 41 = 16-row fragments per wave of the short-K pointwise GEMM (1 / 2, 0 = by the shape)
void cfp_attn_apply_debug_set(int value);
void cfp_dwl3_debug_set(int value);          // dwlarge_x3.hip: key 30 = 1: the 32 x 32 pixel tile for k = 31 (two workgroups per CU)
void cfp_dwl_wgrad_debug_set(int value);     // train_misc2.hip: key 23 = 1 keeps the VALU kernels for the large depthwise weight gradient
void cfp_wgrad_debug_set(int value);         // conv_bwd.hip: key 22 = workgroups a small weight-gradient launch aims for (sets the slab count)
void cfp_bn_debug_set(int key, int value);   // bn_train.hip: 20 / 21 = workgroup targets of the column reductions / elementwise sweeps
void cfp_attn_debug_set(int value);          // attention.hip: key 19 = waves the key / value reduction aims for when it splits a group's keys
int cfp_dw_debug_set(int key, int value);    // dwconv.hip: depthwise 3x3 keys 3-6 and 9-11 (CFP_EINVAL for a value it does not take)
extern "C" int cfp_debug_set(int key, int value) {
  switch (key) {
    case 3: case 4: case 5: case 6: case 9: case 10: case 11: return cfp_dw_debug_set(key, value);
    case 30: cfp_dwl3_debug_set(value); return CFP_OK;
    case 32: g_x3_occ = value; return CFP_OK;
    case 33: g_x3_small_m = value; return CFP_OK;
    case 34: g_x3_small_k = value; return CFP_OK;
    case 35: cfp_tail_x3_debug_set(value); return CFP_OK;
    case 37: cfp_fold_debug_set(value); return CFP_OK;
    case 38: cfp_attn_apply_debug_set(value); return CFP_OK;
    case 39: cfp_tail16_debug_set(value); return CFP_OK;
    case 40: g_chunk16 = value; return CFP_OK;
    case 41: cfp_pw_rows_debug_set(value); return CFP_OK;
    case 17: g_tput = value; return CFP_OK;
    case 16: g_probe = (g_probe & 16) | value; return CFP_OK;
    case 29: g_x3_ad = value; return CFP_OK;
    case 28: g_probe = (g_probe & ~16) | (value ? 16 : 0); return CFP_OK;      // f16x3 GEMM: 1 = the plain (not fragment-pipelined) K loop
    case 15: g_small_s2 = value; return CFP_OK;
    case 14: g_up_halo = value; return CFP_OK;
    case 19: cfp_attn_debug_set(value); return CFP_OK;
    case 20: case 21: cfp_bn_debug_set(key, value); return CFP_OK;
    case 22: cfp_wgrad_debug_set(value); return CFP_OK;
    case 23: cfp_dwl_wgrad_debug_set(value); return CFP_OK;
    case 18: g_halo_s2 = value; return CFP_OK;
    case 12: g_halo = value; return CFP_OK;
    case 24: g_halo_x3 = value; return CFP_OK;
    case 25: g_bin_head_x3_rows = value; return CFP_OK;
    case 26: g_x3_ln_fused = value; return CFP_OK;
    case 27: conv3x3_halo_debug_odd_pitch(value); return CFP_OK;
    case 13: conv3x3_halo_debug_stages(value); return CFP_OK;
    case 0: g_force_variant = value; return CFP_OK;
    case 1: g_force_splits = value; return CFP_OK;
    case 2: g_use_v1 = value; return CFP_OK;
    default: cfp_set_error("cfp_debug_set: unknown key"); return CFP_EINVAL;
  }
}

// Which tile configuration the first-generation (f32) kernel picks: 0 = 256x16, 1 = 256x32,
// 2 = 128x64, 3 = 128x128.
extern "C" int cfp_conv2d_variant(int M, int Cout) {
  if (Cout <= 16) return 0;
  if (Cout <= 32) return 1;
  if (Cout <= 64) return 2;
  long long t128 = (long long)cdiv(M, 128) * cdiv(Cout, 128);
  bool waste = (Cout % 128) != 0 && (Cout % 128) <= 64;   // e.g. Cout = 136, 160, 448
  return (t128 < 192 || waste) ? 2 : 3;
}

namespace {

// Plan for a bf16 problem: kernel generation, tile variant, K-splits.  The rules are fitted on the
// per-shape sweep of tools/conv_bench.py over this network's 80 distinct conv/linear problems at
// batch 8 (profiles/r1_conv_sweep.json: every variant x 1..16 splits, timed inside a replayed HIP
// graph).  What the sweep says:
//   * what decides is workgroups resident per CU, not prefetch depth: 2-stage 64x64 / 128x64 /
//     64x128 tiles (32-48 KB LDS, 3-5 workgroups per CU) beat the 3-stage ones almost everywhere;
//   * 128x128 (2 stages, 2 workgroups/CU) pays only for >= 10^7 outputs with K >= 512 or a long K;
//   * short-K, many-row problems are bandwidth-bound: the first-generation kernel (K-step 32,
//     12-24 KB LDS, up to 6 workgroups/CU) wins or ties there;
//   * the direct 3x3 kernel (LDS halo tile) wins with its smallest tile (8x16 pixels x 32 couts,
//     2 workgroups/CU) on the Cout <= 32 layers with K >= 576 and on the 1/16-scale DAPM convs;
//   * few-row / long-K problems (GSA sr convs) want 8 K-splits.
struct Plan2 { int variant, splits; bool gen1; int direct; };   // direct >= 0: conv3x3_direct variant

Plan2 plan2(long long M, int N, int K, int rpb, int B, bool allow_split, bool conv3x3s1 = false, bool tput = false) {
  Plan2 pl{4, 1, false, -1};
  const int nv = igemm2_num_variants();
  const bool big = M >= 100000, mid = M >= 30000;
  if (N <= 16) {
    if (big && K <= 144) pl.gen1 = true; else pl.variant = 16;
  } else if (N <= 32) {
    if (conv3x3s1 && K >= 576 && mid) pl.direct = 4;
    else if ((big && K <= 128) || (mid && K <= 64)) pl.gen1 = true;
    else pl.variant = mid ? 16 : 9;
  } else if (N <= 64) {
    if ((big && K <= 160) || (mid && K <= 64)) pl.gen1 = true;
    else pl.variant = big ? 14 : mid ? 13 : 4;
  } else {
    if ((big && K <= 288) || (mid && K <= 64)) pl.gen1 = true;
    else if ((M * N >= 614400ll * 128 && K >= 512) || (mid && K >= 2048)) pl.variant = 1;
    else if (mid) pl.variant = (N % 128 != 0 && N % 128 <= 64) ? 14 : 15;
    else if ((N >= 256 && K >= 2048) || N >= 1024) pl.variant = 12;
    else if (conv3x3s1 && N <= 128 && K >= 1152 && M >= 8000) pl.direct = 4;
    else pl.variant = 4;
  }
  if (rpb > 0) { pl.gen1 = false; pl.direct = -1; if (pl.variant != 12) pl.variant = 4; }
  // long K on fewer 64x64 tiles than CUs (the 1/32-scale project GEMMs: 160 tiles x 22 K-steps): two K groups per workgroup
  // (tools/conv_bench.py --kgroups: 12.8 -> 9.3 us at 2400 x 232 x 1392, 8.7 -> 7.1 at K = 816; no gain once two workgroups share a CU)
  if (pl.variant == 4 && !pl.gen1 && pl.direct < 0 && K >= 768) {
    const long long tm = rpb > 0 ? (long long)B * ((rpb + 63) / 64) : (M + 63) / 64;
    if (tm * ((N + 63) / 64) <= 256) pl.variant = 19;
  }
  if (allow_split && K >= 2048 && (M <= 1100 || ((M + 63) / 64) * ((N + 63) / 64) <= 48)) { pl.variant = 4; pl.splits = 8; pl.gen1 = false; pl.direct = -1; }
  // the 64x64 tile with two stages instead of three wherever K is not split: alone it is 3 % faster over the network's small GEMMs
  // (tools/conv_bench.py --kgroups, k13 vs k4), and at 32 KB instead of 48 KB of LDS five of them share a CU with the other batches'
  // kernels instead of three
  if (pl.variant == 4 && pl.splits == 1 && !pl.gen1 && pl.direct < 0 && g_small_s2) pl.variant = 13;
  // ... and the 64x128 tile with two stages instead of three (2400 x 1392 x 232: 9.3 vs 9.7 us alone, 4.7 vs 5.5 per call in flight); wide
  // pointwise layers at the 1/16 scale on 128x64 tiles (9600 x 816 x 136: equal alone, 8.4 vs 9.6 in flight)
  if (pl.variant == 12 && pl.splits == 1 && !pl.gen1 && pl.direct < 0 && g_small_s2) pl.variant = 15;
  if (pl.variant == 13 && !pl.gen1 && pl.direct < 0 && rpb == 0 && M >= 9000 && M < 30000 && N >= 512 && K <= 256 && g_small_s2) pl.variant = 14;
  // single images: the deep decoder convs on a few row tiles (1200 x 256 x 3528 / x 2304) run 21.4 / 14.6 us through the direct kernel's 8 x 16 pixel tiles
  // against 37.8 / 25.8 us on 64 x 128 GEMM tiles (tools/conv_bench.py --sweep --batch 1, profiles/r4_conv_bench_bf16_b1_alone.txt)
  if (!tput && !g_tput && conv3x3s1 && rpb == 0 && !pl.gen1 && pl.splits == 1 && pl.direct < 0 && M <= 2400 && N >= 256 && K >= 2048) pl.direct = 4;
  if ((tput || g_tput) && !pl.gen1 && pl.splits == 1) {
    if (pl.direct < 0 && M <= 20000 && N >= 256 && K >= 2048) pl.variant = 1;                    // 9600 x 256 x 3528: 20.6 vs 31.0 us per call in flight (alone: 51 vs 42)
    if (pl.direct < 0 && pl.variant == 13 && rpb == 0 && M >= 30000 && M < 100000 && N <= 64 && K >= 512) pl.variant = 14;      // 38400 x 64 x 1152: 7.8 vs 10.1
  }
  if (g_force_variant >= 200 && conv3x3s1 && g_force_variant - 200 < conv3x3_num_variants()) { pl.direct = g_force_variant - 200; pl.gen1 = false; pl.splits = 1; }
  else if (g_force_variant >= 0) pl.direct = -1;
  if (g_force_variant >= 0 && g_force_variant < nv) { pl.variant = g_force_variant; pl.gen1 = false; }
  if (g_force_splits >= 1) pl.splits = g_force_splits;
  if (pl.splits > 1 && pl.variant >= 19 && pl.variant <= 21 && g_force_variant < 0) pl.variant = 4;      // K groups and split-K exclude each other
  if (pl.direct >= 0) { pl.gen1 = false; pl.splits = 1; }
  return pl;
}

int pick_ln_variant(int Cout, long long M) {   // the tile must span exactly Cout channels
  switch (Cout) {
    case 128: return M <= 20000 ? 12 : 1;
    case 64: return 2;
    case 32: return 8;
    case 16: return 11;
    default: return -1;
  }
}

}  // namespace

// Plan of the f16x3 kernels (float32 storage, conv_igemm_x3.hip): the gen-2 rules on the equivalent 16-bit problem.  A K-step of 32
// channels moves the bytes and takes the LDS reads of a 64-channel 16-bit step, so the rules see twice the K.
static Plan2 plan_x3(long long M, int N, int K, int rpb, int B, bool allow_split, bool tput, bool piw_split = true) {
  Plan2 pl = plan2(M, N, 2 * (cdiv(K, 32) * 32), rpb, B, allow_split, false, tput);
  // short-K, many-row problems (the rules' "first-generation" answer) and the direct 3x3 kernel have no f16x3 form: row-heavy tiles
  if (pl.gen1 || pl.direct >= 0) pl.variant = N <= 16 ? 10 : N <= 32 ? 16 : N <= 64 ? 14 : K <= 64 ? 16 : 1;
  pl.gen1 = false; pl.direct = -1;
  // tools/conv_bench_x3.py (alone and four copies side by side, profiles/r4_conv_bench_x3_*.txt): the 128 x 128 tile as four row waves
  // (every A fragment converted once) beats the 2 x 2 layout everywhere (head conv 562 vs 614 us alone, 537 vs 569 in flight), and in
  // flight it also beats the 64 x 128 tile on the long-K decoder convs (9600 x 256 x 3528: 53 vs 58 us, 38400 x 224 x 504: 36 vs 43)
  if (pl.variant == 0 || pl.variant == 1) pl.variant = 26;
  if (tput && pl.variant == 15 && M >= 9000 && N >= 128 && N <= 256 && K >= 500) pl.variant = 26;
  if (pl.variant < 0 || pl.variant >= igemm_x3_num_variants()) pl.variant = 13;
  // single images (tools/conv_bench_x3.py --batch 1, profiles/r4_conv_bench_x3_b1_alone.txt): few row tiles and a long K -> the two-K-group
  // tile halves the serial chain (1200 x 256 x 3528: 43.7 vs 77.5 us, x 2304: 30.4 vs 49.7); a few hundred rows x many channels -> 32-row tiles
  // (300 x 1392 x 232: 7.7 vs 10.5 us)
  if (!tput && rpb == 0 && pl.splits <= 1 && M <= 2400 && K >= 2000 && N >= 128 && (pl.variant == 15 || pl.variant == 13)) pl.variant = 19;
  // round 5, late: REAL K splits measured against the two K groups (tools/probes/splitk_b1_probe.py -- the sweep tool's forced splits had silently
  // run un-split for want of a workspace): 1200 x 256 x 3528 22.3 us (eight splits + the reduce launch) vs 42.2, 1200 x 256 x 2304 20.4 (four) vs 27.5,
  // 4800 x 128 x 2808 29.5 (four) vs 32.8; from 1 152 deep down the K groups stay ahead (4800 x 128 x 1152: 17.1 vs 20.0)
  if (!tput && rpb == 0 && allow_split && pl.splits <= 1 && K >= 2000 && (M <= 1200 || (M <= 4800 && K >= 2500))) {
    pl.variant = 13; pl.splits = (M <= 1200 && K >= 3000) ? 8 : 4;
  }
  if (!tput && rpb == 0 && pl.splits <= 1 && M <= 512 && N >= 512 && K <= 512) pl.variant = 17;
  // round 5, late (full sweep of a single image's launches, tools/conv_bench_x3.py --batch 1): up to 4 800 rows the 32 x 64 tile (twice the workgroups,
  // four column waves) is ahead of 64 x 64 on every short-K layer (4800 x 56 x 224: 7.3 vs 8.6 us, 1200 x 512 x 128: 7.8 vs 9.4, 4800 x 256 x 64: 8.0 vs
  // 9.4; whole forward, same box: 3.03 vs 3.15 ms -- far more than the isolated launches predict); at 19 200 rows it is level or behind.  The 12 x 12 / 9 x 9 / 6 x 6 patch convolutions of the global attention (30 ... 130 rows, K ~ 5 000,
  // eight K splits): 16.8 / 17.9 / 16.8 us against 17.9 / 19.8 / 18.0 through 64-row tiles that are mostly padding
  if (!tput && pl.splits <= 1 && pl.variant == 13 && M <= g_x3_small_m && K <= g_x3_small_k) pl.variant = 17;
  if (!tput && rpb == 0 && pl.splits >= 4 && M <= 160 && (pl.variant == 4 || pl.variant == 13)) pl.variant = 17;
  // per-image weights (the squeeze-excite-folded project GEMMs) on a handful of row tiles with a long K -- single images: 300 x 232 x 1392 is
  // 20 tiles of 44 serial K-steps at ~0.8 us each (18.2 us, profiles/r4_conv_bench_x3_b1_alone.txt) on 20 of 256 CUs.  K splits instead of the
  // two K groups (round 5; the caller passes the slab workspace, cfp_conv2d_plan with rows_per_batch > 0 tells it the split count)
  if (rpb > 0 && !tput && piw_split && pl.splits <= 1) {
    const long long tiles = (long long)B * cdiv(rpb, 64) * cdiv(N, 64);
    const int nks = cdiv(K, 32);
    if (tiles <= 64 && nks >= 20) { pl.variant = 4; pl.splits = nks >= 40 ? 8 : 4; }
  }
  if (g_x3_ad && pl.splits <= 1) pl.variant = x3_ad_of(pl.variant);
  if (tput && g_x3_occ && pl.splits <= 1) pl.variant = x3_occ_of(pl.variant);      // one more resident workgroup per CU (conv_igemm_x3.hip, OCC)
  return pl;
}

// The f16x3 route (float32 storage, CFP_CONV_X3).
static ConvRoute route_x3(const ConvP& p, const ConvArgs& a) {
  ConvRoute r{};
  const bool tput = a.in_flight || g_tput != 0;
  const int rpb = a.per_image ? p.Ho * p.Wo : 0;
  // 3x3 stride-1 layers with the whole-depth halo in LDS (conv3x3_halo_x3.hip): cfp_debug_set(0, 500 + v) forces its tile v, 500 + 99 its
  // automatic tile, 400 + v keeps the implicit GEMM
  // deep inputs (Cin % 32 == 0, >= 64): the chunk-pipelined form where it measured ahead of the implicit GEMM with four copies side by side
  // (tools/conv_bench_x3.py --halo --inflight 4: 153600 px 64 -> 64 ch 43.6 vs 49.4 us, 38400 px 128 -> 64 20.4 vs 22.0, head conv 556 vs 565)
  // (batch 1: the head conv, 76800 px, 84 us through chunk tile 24 against 118 us through the 128 x 128 implicit GEMM)
  const int chunk_v = g_halo_x3 ? chunk_x3_variant(p.M, p.Cin, p.Cout, tput) : -1;
  const bool halo = !a.per_image && !a.ln && conv3x3_halo_x3_takes(p) &&
                    (g_force_variant >= 500 || (g_force_variant < 0 && g_halo_x3 && (chunk_v >= 0 || halo_x3_wins(p.M, p.Cin, p.Cout, tput))));
  auto plan = [&](bool piw_split) { return plan_x3(p.M, p.Cout, p.K, rpb, p.B, rpb == 0, tput, piw_split); };
  Plan2 pl = plan(true);
  if (g_force_variant >= 400 && g_force_variant - 400 < igemm_x3_num_variants()) pl.variant = g_force_variant - 400;
  if (g_force_splits >= 1) pl.splits = g_force_splits;
  if (pl.splits > 1 && pl.variant >= 19) pl.variant = 4;
  if (pl.splits > 1 && a.ws_bytes < (size_t)pl.splits * p.M * p.Cout * sizeof(float) + (a.want_tickets ? CFP_CONV_TICKET_BYTES : 0)) {
    if (rpb > 0) pl = plan(false);      // no workspace: the un-split plan of this problem (K groups)
    pl.splits = 1;
  }
  // LayerNorm over Cout in the epilogue when a four-row-wave tile spans exactly Cout channels; otherwise as a second kernel
  int ln_v = -1;
  if (a.ln && rpb == 0 && g_x3_ln_fused) ln_v = p.Cout == 128 ? (p.M >= 30000 ? 26 : 27) : p.Cout == 64 ? (p.M >= 100000 ? 14 : 13) : p.Cout == 32 ? 16 : p.Cout == 16 ? 11 : -1;
  // ... or, when K is split, inside the finishing sum (splitk_reduce_kernel): a row must be a power-of-two group of lanes of one wave
  const int cv4 = p.Cout / 4;
  if (a.ln && pl.splits > 1 && p.Cout % 4 == 0 && cv4 <= 64 && (cv4 & (cv4 - 1)) == 0 && g_x3_ln_fused) {
    r.ln = ConvLn::Reduce;      // (the split GEMM ignores the LayerNorm parameters: it only writes slabs)
  } else if (ln_v >= 0) {
    pl.variant = g_x3_ad ? x3_ad_of(ln_v) : ln_v; pl.splits = 1; r.ln = ConvLn::Tile;
  } else if (a.ln) {
    r.ln = ConvLn::After;
  }
  // CFP_CONV_WS_TICKETS: the last workgroup to reach an output tile finishes it (sum in split order + epilogue), no second launch
  // (a LayerNorm that rides in the finishing sum keeps the reduce launch: the ticketed finish has no row-wide statistics)
  if (a.want_tickets && pl.splits > 1 && r.ln != ConvLn::Reduce) {
    int bm, bn, st;
    igemm_x3_variant_shape(pl.variant, &bm, &bn, &st);
    const long long tiles = (rpb > 0 ? (long long)p.B * cdiv(rpb, bm) : cdiv(p.M, bm)) * cdiv(p.Cout, bn);
    r.tickets = tiles <= CFP_TICKET_SLOTS && (long long)pl.splits * p.M * p.Cout * 4 < (1ll << 31) - 16;      // (slabs behind one buffer descriptor)
  }
  r.fallback = {ConvFamily::X3, pl.variant};
  r.splits = pl.splits;
  r.first = r.fallback;
  if (halo) {
    r.first = {ConvFamily::HaloX3, g_force_variant >= 500 && g_force_variant < 599 ? g_force_variant - 500 : chunk_v};
    r.must_run = g_force_variant >= 500;
  }
  return r;
}

ConvRoute conv_route(const ConvP& p, const ConvArgs& a) {
  if (a.x3) return route_x3(p, a);
  ConvRoute r{};
  const bool tput = a.in_flight || g_tput != 0;
  // channel moments of the output for the BatchNorm that follows (training): only the kernels that end with the output tile in LDS
  // produce them (gen-2 without split-K, gen-1 16-bit); every other route reports 0 row tiles and the caller runs its statistics pass
  auto mom_rows = [&](int bm) { return a.want_mom && (size_t)cdiv(p.M, bm) * 2 * p.Cout <= a.mom_floats ? bm : 0; };
  bool tried = false, gen1 = true;
  if (a.gen2_fits && !g_use_v1) {
    const int rpb = a.per_image ? p.Ho * p.Wo : 0;
    const int ln_variant = a.ln ? pick_ln_variant(p.Cout, p.M) : -1;
    const bool c33 = p.KH == 3 && p.KW == 3 && p.stride == 1 && !a.ln && rpb == 0 && (long long)p.Cout * p.K < (1ll << 31);
    Plan2 pl = plan2(p.M, p.Cout, a.w2 ? 2 * cdiv(p.K, 64) * 64 : p.K, rpb, p.B, rpb == 0 && ln_variant < 0, c33, tput);
    if (a.w2) { pl.gen1 = false; pl.direct = -1; }
    // few input channels, many pixels: the whole-depth halo kernel (conv3x3_halo.hip); cfp_debug_set(0, 300 + v) forces its variant v,
    // any other forced variant / the gen-1 switch keeps the implicit GEMMs (A/B, tests)
    // deep inputs: the chunk kernel (conv3x3_chunk.hip) where chunk16_variant measured it ahead; cfp_debug_set(0, 600 + v) forces its tile v
    // and is an error for a problem the kernel does not take, cfp_debug_set(40, 0) keeps every problem on its earlier kernel
    {
      const bool forced = g_force_variant >= 600 && g_force_variant < 700;
      const bool takes = !a.w2 && c33 && !a.want_mom && conv3x3_chunk_takes(p);
      if (forced && !(takes && g_force_variant - 600 < conv3x3_chunk_num_variants())) {
        r.error = "cfp_conv2d_nhwc: the forced chunk variant cannot run this problem";
      } else {
        const int cv = forced ? g_force_variant - 600 : (takes && g_force_variant < 0) ? chunk16_variant(p.M, p.Cin, p.Cout, tput) : -1;
        if (cv >= 0) { r.first = {ConvFamily::Chunk, cv}; tried = true; }
      }
    }
    const bool c33s2 = p.KH == 3 && p.KW == 3 && p.stride == 2 && !a.ln && rpb == 0;
    if (!tried && !a.w2 && (c33 || c33s2) && !a.want_mom && conv3x3_halo_takes(p) &&
        (g_force_variant < 0 ? (p.Cin <= 64 && (p.stride == 1 ? halo_wins(p.M, p.Cout, tput) : halo_wins_s2(p.M, p.Cout))) : g_force_variant >= 300)) {
      int hv = g_force_variant >= 300 ? g_force_variant - 300 : -1;
      if (hv < 0 && p.stride == 2 && p.Cout > 64) hv = 3;
      if (hv < 0 && tput) hv = (p.M < 300000 && p.Cout <= 32) ? 7 : (p.M < 300000 && p.Cout <= 64) ? 3 : (p.Cout > 160 && p.Cout <= 224) ? 6 : -1;
      r.first = {ConvFamily::Halo, hv};
      r.must_run = g_force_variant >= 0;
      tried = true;
    }
    if (pl.direct >= 0 && !a.want_mom) {
      r.fallback = {ConvFamily::Direct, pl.direct};
      r.splits = 1;
      gen1 = false;
    } else {
      if (pl.direct >= 0) { pl.direct = -1; pl.variant = 14; pl.splits = 1; }      // statistics wanted: the implicit GEMM (it ends with the tile in LDS)
      gen1 = pl.gen1 && !a.ln;
      if (!gen1) {
        if (ln_variant >= 0 && g_force_variant < 0) pl.variant = ln_variant;
        if (ln_variant >= 0) { r.ln = ConvLn::Tile; pl.splits = 1; }
        if (pl.splits > 1 && a.ws_bytes < (size_t)pl.splits * p.M * p.Cout * sizeof(float)) pl.splits = 1;
        if (a.ln && ln_variant < 0) r.ln = ConvLn::After;      // Cout has no exact-width tile: LayerNorm as a second kernel
        if (pl.splits == 1) { int bm, bn, st; igemm2_variant_shape(pl.variant, &bm, &bn, &st); r.mom_rows = mom_rows(bm); }
        r.fallback = {ConvFamily::Gen2, pl.variant};
        r.splits = pl.splits;      // (per-image weights: only a forced count can be above 1 here, and the gen-2 launch runs them un-split)
      }
    }
  }
  if (gen1) {
    // first-generation kernels (f32 parity mode, short-K bf16): per-image weights run image by image, LayerNorm as a second kernel
    const int m1 = a.per_image ? p.Ho * p.Wo : p.M;      // rows of one launch
    const int v1 = cfp_conv2d_variant(m1, p.Cout);
    int splits = pick_splits(v1, m1, p.Cout, p.K, a.dtype);
    if (splits > 1 && a.ws_bytes < (size_t)splits * m1 * p.Cout * sizeof(float)) splits = 1;
    const bool rows = a.dtype == CFP_F32 && p.pointwise && p.M <= 64 && !a.per_image && !a.ln && !g_use_v1;
    r.fallback = {rows ? ConvFamily::RowGemm : ConvFamily::Gen1, v1};
    r.splits = splits;
    if (!rows && a.ln) r.ln = ConvLn::After;
    if (!rows && splits == 1 && is16(a.dtype) && !a.per_image) r.mom_rows = mom_rows(v1 <= 1 ? 256 : 128);
  }
  if (!tried) r.first = r.fallback;
  return r;
}

// cfp_upsample_cat_conv3x3, 16-bit: few concatenated channels and a thin output at many pixels (up4: 64 + 24 -> 32 at 240 x 320): the
// whole-depth halo kernel blends into its resident tile once per workgroup; the 64-channel-chunk direct kernel otherwise.
// cfp_debug_set(14, 0) keeps the direct kernel.
int up_cat_halo_variant(const ConvP& p) {
  if (!(g_up_halo && conv3x3_halo_takes(p) && p.Cout <= 64 && (g_up_halo == 2 || (long long)p.B * p.H * p.W >= 300000))) return -2;
  return g_force_variant >= 300 ? g_force_variant - 300 : -1;
}
int up_cat_direct_variant(int Cout) { return Cout <= 16 ? 5 : (Cout <= 32 ? 4 : (Cout <= 64 ? 1 : 0)); }
int up_cat_x3_variant(int Cout) { return g_force_variant >= 540 && g_force_variant <= 542 ? g_force_variant - 500 : (Cout <= 32 ? 40 : Cout <= 64 ? 41 : 42); }

// The route of the CANONICAL problem of the eight arguments: KW = KH, padding 1 for a 3x3 filter and 0 otherwise, channel strides equal to
// the channel counts, B images of M / B output pixels, no LayerNorm, no residual, no moments, a sufficient workspace, in flight only when
// cfp_debug_set(17, 1) says so, and (16-bit) a problem within the gen-2 kernel's K <= 16384 and 32-bit-offset limits.
extern "C" int cfp_conv2d_plan(int M, int Cout, int K, int KH, int stride, int dtype, int rows_per_batch, int B, int* variant,
                               int* splits) {
  if (KH <= 0 || K % (KH * KH) != 0) KH = 1;      // not a KH x KH filter over whole channels: planned as the plain GEMM of its K
  const int rows = rows_per_batch > 0 ? rows_per_batch : cdiv(M > 0 ? M : 1, B > 0 ? B : 1);      // output pixels of one image, as one row
  ConvP p{};
  p.B = B; p.Ho = 1; p.Wo = rows; p.H = stride; p.W = rows * stride;
  p.KH = p.KW = KH; p.stride = stride; p.pad_t = p.pad_l = KH == 3 ? 1 : 0; p.dil = 1;
  p.Cin = K / (KH * KH); p.Cout = Cout; p.M = M; p.K = K;
  p.in_ld = p.Cin; p.out_ld = Cout;
  p.pointwise = KH == 1 && stride == 1;
  p.f16 = dtype == CFP_F16;
  ConvArgs a{};
  a.dtype = dtype == CFP_F32X3 ? CFP_F32 : dtype;
  a.x3 = dtype == CFP_F32X3;
  a.per_image = rows_per_batch > 0;
  a.ws_bytes = ~(size_t)0;
  a.gen2_fits = is16(dtype);
  ConvRoute r = conv_route(p, a);
  // per-image weights through the first-generation kernels run image by image; the query keeps answering with the plan of the whole
  // batch (callers size the workspace of the batch from it)
  if (a.per_image && (r.first.family == ConvFamily::Gen1 || r.first.family == ConvFamily::RowGemm)) { a.per_image = false; r = conv_route(p, a); }
  static const int base[] = {0, 0, 100, 200, 300, 600, 400, 500};      // by ConvFamily; the halo kernels choose their tile at launch
  const ConvFamily f = r.first.family;
  if (variant) *variant = base[(int)f] + (f == ConvFamily::Halo || f == ConvFamily::HaloX3 ? 0 : r.first.variant);
  if (splits) *splits = f == r.fallback.family ? r.splits : 1;
  return CFP_OK;
}

extern "C" size_t cfp_conv2d_ws_bytes(int M, int Cout, int K, int dtype) {
  if (M <= 0 || Cout <= 0 || K <= 0) return 0;
  int v, s;
  cfp_conv2d_plan(M, Cout, K, 1, 1, dtype, 0, 1, &v, &s);
  return s <= 1 ? 0 : (size_t)s * M * Cout * sizeof(float);
}
