// Per-pixel uncertainty planes of the bin heads (cfpnet_hip.h: CFP_UNC_STD / CFP_UNC_ENTROPY / CFP_UNC_PMAX), shared by the four kernels
// that take a softmax over the bins: bin_softmax_kernel, bin_head_fused_kernel (head.hip), depth_head_fused_kernel (head_fused.hip) and
// bin_head_x3_kernel (conv_igemm_x3.hip).
#pragma once
#include "common.h"

// The value of plane k for one pixel from its reduced sums over the bins: var = sum p (c - mu)^2, ent = unc_entropy(s, t, inv) with
// s = sum e^d and t = sum e^d d over the shifted logits d = l - max, inv = 1 / s.  The maximal logit's exponential is exactly 1, so
// pmax = inv; entropy = ln s - t / s needs no log of a probability (taken as soon as inv exists: s and t need not stay in registers).
// The clamps only catch rounding at the two ends of the range.
__device__ __forceinline__ float unc_entropy(float s, float t, float inv) { return fmaxf(logf(s) - t * inv, 0.f); }
__device__ __forceinline__ float unc_plane(int k, float var, float ent, float inv) {
  return k == CFP_UNC_STD ? sqrtf(fmaxf(var, 0.f)) : k == CFP_UNC_ENTROPY ? ent : inv;
}
