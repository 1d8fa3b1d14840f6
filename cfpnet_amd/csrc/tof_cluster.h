// The L5 sensor model on one zone's histogram, shared by the simulation from ground-truth depth (tof_sim.hip) and the re-simulation from
// the prediction (zone_consistency.hip), so that both turn the same depths into the same (n, mu, sigma), bit for bit.
//
//   reference: src/utils/dataloader.py:104-130 (get_hist_parallel after the unfold).
//
//   tof_bin       the float32 bin of torch.histc(bins, min=0, max=max_d) as ATen's CPU kernel evaluates it
//   tof_hist_add  one pixel per lane into the LDS counters, equal bins of a wave merged with a ballot
//   tof_cluster   ambient floor, then the strongest run of consecutive non-zero bins
//   tof_moments   n, mu, sigma of that run over the bin centres in float64
//
// A workgroup of kTofThreads lanes owns one zone: `cnt` (kTofMaxBins LDS counters, the first `bins` in use) and `best` (one LDS word).
#pragma once
#include "common.h"

namespace {

constexpr int kTofThreads = 256;
constexpr int kTofMaxBins = 1024;

// bin = int(((v - 0) * bins) / (max_d - 0)); v == max_d folds into the last bin; values outside [0, max_d] and NaN: -1 (ignored)
__device__ __forceinline__ int tof_bin(float v, float max_d, int bins) {
  int bin = -1;
  if (v >= 0.f && v <= max_d) {
    bin = (int)(((v - 0.f) * (float)bins) / (max_d - 0.f));
    if (bin == bins) bin = bins - 1;
  }
  return bin;
}

// The pixels of a zone along one axis: the integers i of [0, n) with a <= (float)i < b are [lo, hi).  n <= 2^24, so (float)i is exact and
// the float rule is a rule on ceil().  A NaN bound gives the empty range.  (The membership rule of the zone consistency and the zone loss.)
__device__ __forceinline__ void zc_span(float a, float b, int n, int& lo, int& hi) {
  lo = hi = 0;
  if (a != a || b != b) return;
  lo = !(a > 0.f) ? 0 : (a >= (float)n ? n : (int)ceilf(a));
  hi = !(b > 0.f) ? 0 : (b >= (float)n ? n : (int)ceilf(b));
  if (hi < lo) hi = lo;
}

// Every lane of the wave calls this with its pixel's bin (-1: nothing to add).  Lanes that hit the same bin are merged with a ballot so
// a flat zone (every pixel in two or three bins) does not serialise 64-way on one LDS counter.
__device__ __forceinline__ void tof_hist_add(int* cnt, int bin, int lane) {
  unsigned long long todo = __ballot(bin >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lb = __builtin_amdgcn_readlane(bin, leader);
    const unsigned long long same = __ballot(bin == lb);
    if (lane == leader) atomicAdd(&cnt[lb], (int)__popcll(same));
    todo &= ~same;
  }
}

// The surviving run, the same in every lane: bins [start, stop) of `cnt` with `n` counts in all; n == 0: start == stop == bins.
struct TofRun { long long n; int start, stop; };

// Steps 2 and 3.  On entry the histogram in `cnt` is complete and *best == 0, both visible to the workgroup (a barrier after the last
// add).  On return `cnt` holds the counts after the floor -- bin 0 cleared, `floor_count` subtracted and clamped at 0 -- and every lane
// holds the run: the one with the largest sum, the lowest start on ties.
__device__ __forceinline__ TofRun tof_cluster(int* cnt, unsigned long long* best, int bins, int floor_count, int tid) {
  // 2. ambient floor
  int hloc[kTofMaxBins / kTofThreads];
#pragma unroll
  for (int k = 0; k < kTofMaxBins / kTofThreads; ++k) {
    const int i = tid + k * kTofThreads;
    hloc[k] = (i < bins && i > 0) ? max(cnt[i] - floor_count, 0) : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kTofMaxBins / kTofThreads; ++k) {
    const int i = tid + k * kTofThreads;
    if (i < bins) cnt[i] = hloc[k];
  }
  __syncthreads();

  // 3. every run start walks its run; key = (sum << 32) | ~start so the largest sum wins and, on ties, the lowest start
#pragma unroll
  for (int k = 0; k < kTofMaxBins / kTofThreads; ++k) {
    const int i = tid + k * kTofThreads;
    if (i < bins && hloc[k] > 0 && (i == 0 || cnt[i - 1] == 0)) {
      unsigned long long s = 0;
      for (int j = i; j < bins && cnt[j] > 0; ++j) s += (unsigned long long)cnt[j];
      atomicMax(best, (s << 32) | (unsigned long long)(0xffffffffu - (unsigned)i));
    }
  }
  __syncthreads();
  const unsigned long long key = *best;
  TofRun r;
  r.n = (long long)(key >> 32);
  r.start = key ? (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)) : bins;
  r.stop = r.start;
  while (r.stop < bins && cnt[r.stop] > 0) ++r.stop;        // every thread: <= run length LDS reads
  return r;
}

// Step 4, for one lane: moments over the bin centres ((double)(float)((j+1)*bin_width) + j*bin_width)/2 in ascending bin order, float64,
// no FMA contraction.  n == 0 gives mu = 0 and sigma = 1e-9.
__device__ __forceinline__ void tof_moments(const int* cnt, const TofRun& r, double bin_width, double& mu, double& sigma) {
  const double nf = (double)((float)r.n + 1e-9f);           // the reference's `n + 1e-9` stays float32
  double acc = 0.0;
  for (int j = r.start; j < r.stop; ++j) {
    const double c = ((double)(float)((double)(j + 1) * bin_width) + (double)j * bin_width) / 2.0;
    acc += c * (double)cnt[j];
  }
  mu = acc / nf;
  double var = 0.0;
  for (int j = r.start; j < r.stop; ++j) {
    const double c = ((double)(float)((double)(j + 1) * bin_width) + (double)j * bin_width) / 2.0;
    const double d = c - mu;
    var += (double)cnt[j] * (d * d);
  }
  sigma = sqrt(var / nf) + 1e-9;
}

}  // namespace
