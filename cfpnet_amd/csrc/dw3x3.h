// Depthwise 3x3: the plans and launches of the kernel files beside dwconv.hip.  dw3x3_choose (dwconv.hip) is the only caller of the
// *_plan functions, so the partial-sum slot queries and the launches see the same choice.
#pragma once
#include "common.h"

// dw3x3_rows.hip (float32 storage): runs of R output rows; nps workgroups = partial-sum slots per image, ncb channel blocks.
// force_R = cfp_debug_set key 11 (0 = automatic).
struct DwrPlan { int R, nruns, npx, nps, ncb; };
bool dwr_plan(int B, int H, int W, int Ho, int Wo, int C, int stride, int in_ld, int out_ld, int force_R, DwrPlan& d);
int dwr_launch(const DwrPlan& d, const void* in, int in_ld, const void* w, const float* scale, const float* shift, void* out, int out_ld,
               float* partial, const float* w_red, int RD, float* hpart, int B, int H, int W, int C, int stride, int pad_t, int pad_l,
               int Ho, int Wo, int act, cfp_stream_t stream, const char* who);

// dw3x3_slide.hip (16-bit storage, C % 16 == 0): nyr y-runs x nxs x-segments = partial-sum slots per image, 64-channel blocks.
// force_xs = cfp_debug_set key 9 (0 = automatic).
struct DwlPlan { int XS, nxs, nyr, colsA, rowpitch; size_t lds; };
bool dwl_plan(int B, int Ho, int Wo, int C, int stride, int force_xs, DwlPlan& d);
int dwl_launch(const DwlPlan& d, const void* in, int in_ld, const void* w, const float* scale, const float* shift, void* out, int out_ld,
               float* partial, const float* w_red, int RD, float* hpart, int B, int H, int W, int C, int stride, int pad_t, int pad_l,
               int Ho, int Wo, int act, int dtype, cfp_stream_t stream, const char* who);
