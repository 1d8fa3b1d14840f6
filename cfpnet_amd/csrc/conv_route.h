// Which kernel a dense convolution / linear layer runs (conv_route.hip): ONE decision, taken by the launch (conv2d_impl, conv_entry.hip)
// and by the queries (cfp_conv2d_plan, cfp_conv2d_ws_bytes) through the same function.
#pragma once
#include "igemm_core.h"

enum class ConvFamily {
  Gen1,      // conv_igemm.hip: first-generation implicit GEMM (float32 parity mode, short-K 16-bit), variant 0..3
  RowGemm,   // conv_igemm.hip: few-row float32 GEMM; it has no plan code of its own: variant / splits are the gen-1 plan of the problem
  Gen2,      // conv_igemm2.hip
  Direct,    // conv3x3_direct.hip
  Halo,      // conv3x3_halo.hip, variant < 0 = the launcher picks the tile
  Chunk,     // conv3x3_chunk.hip
  X3,        // conv_igemm_x3.hip
  HaloX3,    // conv3x3_halo_x3.hip (whole-depth and chunk-pipelined tiles), variant < 0 = the launcher picks the tile
};

enum class ConvLn {
  None,
  Tile,      // in the epilogue of a tile that spans exactly Cout channels
  Reduce,    // in the finishing sum of a split-K launch (splitk_reduce_kernel)
  After,     // cfp_layernorm as a second kernel; the residual is added there
};

struct ConvKernel { ConvFamily family; int variant; };

struct ConvRoute {
  ConvKernel first;     // the kernel to launch
  bool must_run;        // first is Halo / HaloX3: its launcher may decline (LDS does not fit, 2^31 workgroups).  true = that is an error (a
                        // forced variant), false = `fallback` runs instead.  Every other family's launcher failing is an error
  ConvKernel fallback;  // what runs when `first` declines: Gen1 / RowGemm / Gen2 / Direct / X3 (== first when that is already one of them)
  // the plan of `fallback` (the 3x3 kernels run un-split, without LayerNorm, tickets or moments)
  int splits;
  ConvLn ln;
  bool tickets;         // the split-K launch finishes its tiles itself (CFP_CONV_WS_TICKETS), no reduce launch
  int mom_rows;         // rows per tile of the channel moments `fallback` writes, 0 = it writes none
  const char* error;    // non-null: cfp_debug_set(0, ..) forces a variant that cannot run this problem; the launch returns CFP_EHIP and
                        // launches nothing (the queries report the rest of the route as it stands)
};

// What the caller passed beside the problem itself.
struct ConvArgs {
  int dtype;                                           // CFP_F32 / CFP_BF16 / CFP_F16 (storage)
  bool per_image, w2, x3, in_flight, want_tickets;     // the bits of cfp_conv2d_nhwc_ex's flags
  bool ln;
  bool want_mom; size_t mom_floats;                    // channel moments wanted (and the call is one that can have them) / room for them
  size_t ws_bytes;                                     // 0 when there is no workspace
  bool gen2_fits;                                      // 16-bit, undilated, K <= 16384 and every operand within the gen-2 kernel's 32-bit byte offsets
};

// `p` as conv2d_impl fills it before any route-dependent field (ln_gamma, rows_per_batch, w_bstride, k2, mom) is set.  Reads the
// debug state of cfp_debug_set.
ConvRoute conv_route(const ConvP& p, const ConvArgs& a);

// cfp_upsample_cat_conv3x3: the 16-bit call's whole-depth halo variant (-1 = its launcher picks) when that kernel is to be tried first,
// -2 when not; the direct kernel's tile; the f16x3 kernel's tile
int up_cat_halo_variant(const ConvP& p);
int up_cat_direct_variant(int Cout);
int up_cat_x3_variant(int Cout);

extern int g_use_v1;      // cfp_debug_set key 2
extern int g_probe;       // cfp_debug_set keys 16 / 28: ConvP.probe
