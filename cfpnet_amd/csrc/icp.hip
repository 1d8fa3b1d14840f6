// Camera tracking on the device: one Gauss-Newton iteration of dense point-to-plane ICP of a frame (the prediction and its std) against a
// model map (depth, normals and std in the model camera: a cfp_tsdf_raycast, or the previous frame's cfp_depth_unproject), per image
// (cfp_icp_step).  The definition is in include/cfpnet_hip.h; the depth at a source pixel is met_pred of metrics_pred.h in mode 0, the
// value cfp_depth_unproject back-projects, bit for bit, and the std that travels with it is met_plane.
//
// Accumulate.  One thread per pixel of the stride grid, x along the lanes, grid-striding over the image: neighbouring lanes project to
// neighbouring model pixels, so the depth / normal / std gathers of a wave hit the same lines.  The pose and the two cameras are uniform
// per workgroup (scalar loads).  A pair's 30 terms are float32 products; each is added to a double accumulator of the thread, the
// threads are summed by a butterfly inside the wave and the four waves in order through LDS, and a workgroup leaves ONE row of 30
// doubles in the workspace.  The number of workgroups per image is a function of the shape alone, capped at kIcpBlocks.
//
// Finalize.  One 64-lane workgroup per image sums the rows in a fixed order (two rows per lane, then the butterfly); lane 0 solves the
// 6 x 6 system by LDL^T in double, refuses a step that is not constrained, composes exp(xi) with the pose, re-orthonormalises and
// writes the pose back as float32.  No atomics anywhere: two calls on the same inputs give identical bits.
//
// The pieces live in icp_core.h, which icp_rgb.hip (the step that also looks at the image) shares: icp_pair is the pixel -- its depth is
// met_pred(m, pb, pix), its std met_plane(su, sb, pix) --, icp_add_terms the 30 products, icp_block_reduce the __shfl_xor butterfly and the
// four waves, icp_sum_rows / icp_solve / icp_update_pose the finalize.  The kernels below are what is left: the loop and the launch.
#include "common.h"
#include "icp_core.h"
#include "metrics_pred.h"

namespace {

using namespace icp_core;                             // the pair, the reductions, the solve and the pose update: shared with icp_rgb.hip

// PI: the prediction is blended to the grid (met_pred's interpolate); SI: 0 no std plane, 1 read directly, 2 blended (met_plane's).  As
// template arguments they leave each instance the uniform state of its own path only, which is what keeps the scalar file from spilling.
template <int PI, int SI>
__global__ __launch_bounds__(256) void icp_accumulate_kernel(IcpP p) {
  __shared__ double red[4][kIcpTerms];
  MetP m = p.m, su = p.u;
  m.interpolate = PI; m.mode = 0; su.interpolate = SI == 2 ? 1 : 0;
  su.H = m.H; su.W = m.W;                             // the same grid: one row / column split serves both blends
  const int b = blockIdx.y;
  const IcpImg g = icp_image<SI>(p, m, b);
  int* ib = p.index ? p.index + (long long)b * m.H * m.W : nullptr;
  __shared__ float cam[24];
  IcpCam c;
  icp_load_cam(p, b, cam, c);
  double acc[kIcpTerms];
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) acc[k] = 0.0;
  const unsigned n = (unsigned)p.ws * (unsigned)p.hs;              // < 2^31
  for (long long i64 = (long long)blockIdx.x * 256 + threadIdx.x; i64 < n; i64 += (long long)gridDim.x * 256) {
    IcpPair q;
    icp_pair(p, m, su, c, g, (unsigned)i64, q);
    if (ib) icp_write_cell(ib, p, m, q, q.mi, -1);
    if (q.mi < 0) continue;
    icp_add_terms(acc, q.w, q.J, q.r);
  }
  icp_block_reduce<kIcpTerms>(acc, red, p.partial + ((long long)b * gridDim.x + blockIdx.x) * kIcpTerms);
}

__global__ __launch_bounds__(64) void icp_finalize_kernel(IcpF p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int r0 = min(lane, p.nblocks - 1), r1 = min(lane + 64, p.nblocks - 1);
  double s[kIcpTerms];
  icp_sum_rows(p.partial + ((long long)b * p.nblocks + r0) * kIcpTerms, p.partial + ((long long)b * p.nblocks + r1) * kIcpTerms, lane,
               p.nblocks, s);
  if (lane != 0) return;
  if (p.sums) {
#pragma unroll
    for (int k = 0; k < kIcpTerms; ++k) p.sums[b * 32 + k] = s[k];
    p.sums[b * 32 + 30] = 0.0; p.sums[b * 32 + 31] = 0.0;
  }
  double wn, vn;
  const bool accepted = icp_update_pose(s, s[29] >= (double)p.min_pairs, p.min_pivot, p.T + b * 12, p.T_ref ? p.T_ref + b * 12 : nullptr,
                                        p.T_world ? p.T_world + b * 12 : nullptr, wn, vn);
  icp_write_stats(p.stats + b * 6, s, wn, vn, accepted);
}

}  // namespace

extern "C" size_t cfp_icp_ws_bytes(int B, int H, int W, int stride) {
  if (B <= 0 || H <= 0 || W <= 0 || stride < 1) return 0;
  return (size_t)B * icp_blocks(H, W, stride) * kIcpTerms * sizeof(double);
}

extern "C" int cfp_icp_step(const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo, float hi, const float* std,
                            int Hu, int Wu, long long std_stride, float std_floor, const float* src_normals, float cos_min,
                            const float* K_src, const float* mdl_depth, const float* mdl_normals, const float* mdl_std, int Hm, int Wm,
                            const float* K_mdl, int stride, float z_near, float dist_max, int min_pairs, float min_pivot, float* T,
                            const float* T_ref, float* T_world, int* index, double* sums, float* stats, void* ws, size_t ws_bytes,
                            cfp_stream_t stream) {
  const int rc = icp_check("cfp_icp_step", pred, Hp, Wp, H, W, B, interpolate, lo, hi, std, Hu, Wu, std_stride, std_floor, cos_min, K_src,
                           mdl_depth, mdl_normals, Hm, Wm, K_mdl, stride, z_near, dist_max, min_pairs, min_pivot, T, T_ref, T_world, sums,
                           stats, ws, ws_bytes, kIcpTerms);
  if (rc != CFP_OK) return rc;
  IcpP p;
  IcpF f;
  icp_fill(p, f, pred, Hp, Wp, H, W, B, interpolate, lo, hi, std, Hu, Wu, std_stride, std_floor, src_normals, cos_min, K_src, mdl_depth,
           mdl_normals, mdl_std, Hm, Wm, K_mdl, stride, z_near, dist_max, min_pairs, min_pivot, T, T_ref, T_world, index, sums, stats, ws);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)f.nblocks, B);
  const int si = !std ? 0 : (p.u.interpolate ? 2 : 1);
#define CFP_ICP_LAUNCH(PI, SI) hipLaunchKernelGGL((icp_accumulate_kernel<PI, SI>), grid, dim3(256), 0, s, p)
  if (interpolate) {
    if (si == 0) CFP_ICP_LAUNCH(1, 0); else if (si == 1) CFP_ICP_LAUNCH(1, 1); else CFP_ICP_LAUNCH(1, 2);
  } else {
    if (si == 0) CFP_ICP_LAUNCH(0, 0); else if (si == 1) CFP_ICP_LAUNCH(0, 1); else CFP_ICP_LAUNCH(0, 2);
  }
#undef CFP_ICP_LAUNCH
  hipLaunchKernelGGL(icp_finalize_kernel, dim3(B), dim3(64), 0, s, f);
  return cfp_check_launch("cfp_icp_step");
}
