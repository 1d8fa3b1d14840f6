// The sample points of one ToF zone from its (mu, sigma): step 5 of the simulation (tof_sim.hip) and the last stage of the degradation
// (tof_degrade.hip), one implementation so that both give the same bits.
#pragma once
#include "common.h"

// One (zone, sample): both branches of sample_point_from_hist_parallel (dataloader.py:65-80) in float64, rounded to
// float32.  UNIFORM: tensor_linspace(mu-3s, mu+3s) = w0*lo + w1*hi with the host's float32 linspace tables.  ICDF (the argparse
// default, `--sample_uniform` absent): torch.distributions.Normal(mu, s).icdf(ppf) = mu + s * erfinv(2 ppf - 1) * sqrt(2), where
// erfinv is evaluated in FLOAT32 on the 16 ppf points (the ppf tensor is float32, only the product is promoted) -- so that
// table (`w0` here) is an input evaluated on the host like the linspace tables; product order as in Normal.icdf.
__device__ __forceinline__ float tof_sample(double mu, double sg, float a, float b, int mode) {
  if (mode == CFP_TOF_SAMPLE_ICDF) return (float)(mu + (sg * (double)a) * 1.4142135623730951);
  const double lo = mu - 3.0 * sg, hi = mu + 3.0 * sg;
  return (float)((double)a * lo + (double)b * hi);
}
