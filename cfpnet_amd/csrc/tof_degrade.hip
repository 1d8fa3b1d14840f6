// ToF degradation between the simulation and the model: random zone dropout and Gaussian range noise, one workgroup per image.
//
//   reference: src/dataloader/nyu.py:155-158 (drop_hist: int(len * drop) of the valid zones, drawn WITH replacement, lose their
//   validity) and :159-163 (noise on mu; the reference writes it into a copy, so there it has no effect -- here it is what those
//   lines intended), then :179 (sample_point_from_hist_parallel on the result).  The reference does this per sample on the CPU in
//   the data-loader workers; here a batch is one launch and nothing returns to the host.
//
// Random numbers: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (i, b, step, stream): b the image, stream 0 the
// dropout (i = draw index), stream 1 the noise (i = zone index).  An image's result depends on (seed, step, b) and its own
// inputs only, never on B or on the launch geometry.
//
// Per image (thread t owns zone t, Z <= 256 = kDegThreads):
//   1. compaction  V = valid zones ascending, in LDS: ballot + popcount below the lane inside a wave, plus the popcounts of the waves
//                  before it (Z = 256 spans four waves); n = |V|
//   2. dropout     k = (int)((double)n * drop); draw j < k (lanes in parallel) clears the flag of V[(word0(j) * n) >> 32].  Two draws
//                  clearing one flag is a same-value LDS store.
//   3. noise       on zones still valid: words w of counter (z, b, step, 1); hit when w0 * 2^-32 < noise_prob; then
//                  mu += noise_mean + noise_sigma * sqrt(-2 ln((w1 + 1) * 2^-32)) * cos(2 pi * w2 * 2^-32) in float64
//   4. samples     tof_sample() of tof_sample.h on the resulting (mu, sigma); zero rows for zones that are not valid any more
// No atomics on global memory, plain vector stores; counts are popcounts of ballots.
//
// The launch is latency bound like tof_hist_kernel: B workgroups, ~0.6 KB read and ~2.9 KB written per image at Z = 36, S = 16, three
// barriers and at most ceil(k / 256) + 1 Philox blocks per lane.  A roofline says nothing about it; the measured launch time is in
// DESIGN.md 4.25.
#include "common.h"
#include "tof_sample.h"

namespace {

constexpr int kDegThreads = 256;      // one lane per zone: the largest grid of the project is 16 x 16
constexpr int kDegWaves = kDegThreads / 64;

struct Philox4 { unsigned int w[4]; };

// Philox4x32-10 (Salmon et al., SC'11), the constants of Random123
__device__ __forceinline__ Philox4 philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3, unsigned int k0,
                                                 unsigned int k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned int)p1; c3 = (unsigned int)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

struct DegP {
  const double* fh; const unsigned char* mask; int Z;
  double drop, noise_prob, noise_mean, noise_sigma;
  unsigned int key0, key1, step;
  const float* w0; const float* w1; int nsamp; int sample_mode;
  unsigned char* mask_out; double* fh_out; float* pts; int* counts;
};

__global__ __launch_bounds__(kDegThreads) void tof_degrade_kernel(DegP p) {
  __shared__ int wave_n[kDegWaves], wave_dropped[kDegWaves], wave_noised[kDegWaves];
  __shared__ unsigned short list[kDegThreads];
  __shared__ unsigned char keep[kDegThreads];
  __shared__ double smu[kDegThreads], ssg[kDegThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned int b = blockIdx.x;
  const long long base = (long long)b * p.Z;
  const unsigned long long below = (1ull << lane) - 1ull;

  // 1. the valid zones, compacted in ascending order
  const bool in = tid < p.Z;
  const bool valid = in && p.mask[base + tid] != 0;
  double mu = 0.0, sg = 0.0;
  if (in) { mu = p.fh[(base + tid) * 2]; sg = p.fh[(base + tid) * 2 + 1]; }
  const unsigned long long bal = __ballot(valid);
  if (lane == 0) wave_n[wave] = (int)__popcll(bal);
  keep[tid] = valid ? 1 : 0;
  __syncthreads();
  int first = 0, n = 0;
#pragma unroll
  for (int w = 0; w < kDegWaves; ++w) {
    const int c = wave_n[w];
    first += w < wave ? c : 0;
    n += c;
  }
  if (valid) list[first + (int)__popcll(bal & below)] = (unsigned short)tid;
  __syncthreads();

  // 2. dropout: k draws with replacement from the n valid zones.  (word * n) >> 32 maps a uniform 32-bit word to 0..n-1 with a bias
  // below n / 2^32 (some indices get one more of the 2^32 words than others): < 6e-8 at n <= 256
  const int k = (int)((double)n * p.drop);
  for (int j = tid; j < k; j += kDegThreads) {
    const Philox4 r = philox4x32_10((unsigned int)j, b, p.step, 0u, p.key0, p.key1);
    const int pick = (int)(((unsigned long long)r.w[0] * (unsigned long long)n) >> 32);     // < n: list[pick] was written above
    keep[list[pick]] = 0;
  }
  __syncthreads();
  const bool kept = keep[tid] != 0;

  // 3. noise on the zones that are still valid
  bool hit = false;
  if (kept && p.noise_prob > 0.0) {
    const Philox4 r = philox4x32_10((unsigned int)tid, b, p.step, 1u, p.key0, p.key1);
    hit = (double)r.w[0] * 0x1p-32 < p.noise_prob;
    if (hit) {
      const double rad = sqrt(-2.0 * log(((double)r.w[1] + 1.0) * 0x1p-32));
      const double ang = 6.283185307179586 * ((double)r.w[2] * 0x1p-32);
      mu += p.noise_mean + p.noise_sigma * rad * cos(ang);
    }
  }
  const unsigned long long bal_dropped = __ballot(valid && !kept), bal_noised = __ballot(hit);
  if (lane == 0) { wave_dropped[wave] = (int)__popcll(bal_dropped); wave_noised[wave] = (int)__popcll(bal_noised); }
  smu[tid] = mu; ssg[tid] = sg;
  if (in) {
    p.mask_out[base + tid] = kept ? 1 : 0;
    if (p.fh_out) { p.fh_out[(base + tid) * 2] = mu; p.fh_out[(base + tid) * 2 + 1] = sg; }
  }
  __syncthreads();
  if (tid == 0 && p.counts) {
    int d = 0, h = 0;
#pragma unroll
    for (int w = 0; w < kDegWaves; ++w) { d += wave_dropped[w]; h += wave_noised[w]; }
    p.counts[(long long)b * 3 + 0] = n; p.counts[(long long)b * 3 + 1] = d; p.counts[(long long)b * 3 + 2] = h;
  }

  // 4. samples, consecutive lanes on consecutive floats of the image's [Z, nsamp] block
  const int total = p.Z * p.nsamp;
  float* out = p.pts + base * p.nsamp;
  for (int i = tid; i < total; i += kDegThreads) {
    const int z = i / p.nsamp, t = i - z * p.nsamp;
    float v = 0.f;
    if (keep[z]) v = tof_sample(smu[z], ssg[z], p.w0[t], p.w1 ? p.w1[t] : 0.f, p.sample_mode);
    out[i] = v;
  }
}

}  // namespace

extern "C" int cfp_tof_degrade(const double* fh, const unsigned char* mask, int B, int Z, double drop, double noise_prob, double noise_mean,
                               double noise_sigma, unsigned long long seed, unsigned int step, const float* w0, const float* w1, int nsamp,
                               int sample_mode, unsigned char* mask_out, double* fh_out, float* pts, int* counts, cfp_stream_t stream) {
  CFP_REQUIRE(fh && mask && w0 && mask_out && pts && (w1 || sample_mode == CFP_TOF_SAMPLE_ICDF), CFP_EINVAL, "cfp_tof_degrade: null pointer");
  CFP_REQUIRE(sample_mode == CFP_TOF_SAMPLE_UNIFORM || sample_mode == CFP_TOF_SAMPLE_ICDF, CFP_EINVAL, "cfp_tof_degrade: bad sample_mode");
  CFP_REQUIRE(B > 0 && nsamp > 0, CFP_ESHAPE, "cfp_tof_degrade: non-positive dimension");
  CFP_REQUIRE(Z >= 1 && Z <= kDegThreads, CFP_ESHAPE, "cfp_tof_degrade: zones per image must be in 1..256");
  CFP_REQUIRE((long long)B * Z < (1ll << 31) && (long long)Z * nsamp < (1ll << 31), CFP_ESHAPE, "cfp_tof_degrade: too many zones (B*Z must stay below 2^31)");
  CFP_REQUIRE(drop >= 0.0 && drop <= 1.0, CFP_EINVAL, "cfp_tof_degrade: drop must be in [0, 1]");
  CFP_REQUIRE(noise_prob >= 0.0 && noise_prob <= 1.0, CFP_EINVAL, "cfp_tof_degrade: noise_prob must be in [0, 1]");
  CFP_REQUIRE(noise_sigma >= 0.0 && noise_sigma <= 1.7e308 && noise_mean >= -1.7e308 && noise_mean <= 1.7e308, CFP_EINVAL,
              "cfp_tof_degrade: noise_sigma must be non-negative and finite, noise_mean finite");
  CFP_REQUIRE(fh_out || noise_prob == 0.0, CFP_EINVAL, "cfp_tof_degrade: null pointer (fh_out may be NULL only with noise_prob == 0)");
  DegP p;
  p.fh = fh; p.mask = mask; p.Z = Z;
  p.drop = drop; p.noise_prob = noise_prob; p.noise_mean = noise_mean; p.noise_sigma = noise_sigma;
  p.key0 = (unsigned int)(seed & 0xffffffffull); p.key1 = (unsigned int)(seed >> 32); p.step = step;
  p.w0 = w0; p.w1 = w1; p.nsamp = nsamp; p.sample_mode = sample_mode;
  p.mask_out = mask_out; p.fh_out = fh_out; p.pts = pts; p.counts = counts;
  hipLaunchKernelGGL(tof_degrade_kernel, dim3((unsigned)B), dim3(kDegThreads), 0, reinterpret_cast<hipStream_t>(stream), p);
  return cfp_check_launch("cfp_tof_degrade");
}
