// The middle launch of the project's order-preserving compactions (cfp_points_compact, cfp_tsdf_surface): count per chunk -> exclusive
// scan per image -> scatter.  No atomics, so the order and every bit of a result are a function of the inputs alone.
#pragma once
#include "common.h"

namespace {

// exclusive scan of one image's chunk counts in place, the total -> counts[b]; thread t owns a run of consecutive chunks
__global__ __launch_bounds__(256) void chunk_scan_kernel(int* __restrict__ ws, int* __restrict__ counts, int nchunks) {
  __shared__ int s[2][256];
  const int b = blockIdx.x, t = threadIdx.x;
  int* w = ws + (long long)b * nchunks;
  const int L = (nchunks + 255) / 256;
  const int j0 = min((long long)t * L, (long long)nchunks), j1 = min((long long)(t + 1) * L, (long long)nchunks);
  int sum = 0;
  for (int j = j0; j < j1; ++j) sum += w[j];
  s[0][t] = sum;
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < 256; o <<= 1) {                             // inclusive Hillis-Steele scan of the 256 run sums
    s[cur ^ 1][t] = s[cur][t] + (t >= o ? s[cur][t - o] : 0);
    cur ^= 1;
    __syncthreads();
  }
  int run = s[cur][t] - sum;                                      // exclusive prefix of this thread's run
  for (int j = j0; j < j1; ++j) { const int c = w[j]; w[j] = run; run += c; }
  if (t == 255) counts[b] = s[cur][255];
}

}  // namespace
