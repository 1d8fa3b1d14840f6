// What the zone consistency (zone_consistency.hip) and the zone-consistency loss (zone_loss.hip) share, so that up to the strongest run
// the loss is the metric bit for bit by construction:
//   ZoneArgs / zone_args   the head of both argument blocks and the host checks that fill it
//   ZoneSweep              the pixels of one zone, walked by a workgroup of kTofThreads lanes: what is done with a depth is the caller's
//   ZoneStage              the zones that can touch a tile of 8 x 32 pixels, staged through LDS in chunks of 256 in index order
// The depth at a pixel is met_pred of metrics_pred.h in mode 0; the pixel set, the bin and the histogram are tof_cluster.h's.
#pragma once
#include "metrics_pred.h"
#include "tof_cluster.h"

namespace {

constexpr int kZoneBatch = 8;                         // pixels per lane in flight in the sweep
constexpr int kZoneChunk = 256;                       // rectangles looked at per staging pass
constexpr int kZoneTileH = 8, kZoneTileW = 32;       // the tile: one pixel per lane, a wave covers two 128-byte row segments
static_assert(kZoneTileH * kZoneTileW == kZoneChunk && kZoneChunk == 256, "one lane per pixel of the tile and per zone of the chunk, four waves");

struct ZoneArgs {
  MetP m;                                             // pred, Hp, Wp, H, W, interpolate, mode 0, lo, hi, sy, sx
  const float* rect; const unsigned char* mask; const double* raw; int Z;
  float max_d; int bins; double bin_width; int floor_count;
};

// The refusals both entries state, in their order, under the entry's `name`, then the block.  Null pointers come before (the pointer sets
// differ) and B * Z after: the loss has checks of its own in front of that one.
inline int zone_args(ZoneArgs& a, const char* name, const float* pred, int Hp, int Wp, int H, int W, int B, int interpolate, float lo,
                     float hi, const float* rect, const unsigned char* mask, const double* raw, int Z, float max_distance, int bins,
                     double bin_width, int floor_count) {
  CFP_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && H > 0 && W > 0 && Z > 0, CFP_ESHAPE, std::string(name) + ": non-positive dimension");
  CFP_REQUIRE((long long)H * W < (1ll << 31) && (long long)Hp * Wp < (1ll << 31) && H <= (1 << 24) && W <= (1 << 24), CFP_ESHAPE,
              std::string(name) + ": image too large");
  CFP_REQUIRE(interpolate || (Hp == H && Wp == W), CFP_ESHAPE, std::string(name) + ": sizes differ and interpolate is off");
  CFP_REQUIRE(lo < hi, CFP_EINVAL, std::string(name) + ": empty depth range");
  CFP_REQUIRE(bins > 0 && bins <= kTofMaxBins, CFP_ESHAPE, std::string(name) + ": bins must be in 1..1024");
  CFP_REQUIRE(max_distance > 0.f && bin_width > 0.0 && floor_count >= 0, CFP_EINVAL, std::string(name) + ": bad histogram parameters");
  a.m = met_params(pred, nullptr, Hp, Wp, H, W, B, interpolate, 0, lo, hi);
  a.rect = rect; a.mask = mask; a.raw = raw; a.Z = Z;
  a.max_d = max_distance; a.bins = bins; a.bin_width = bin_width; a.floor_count = floor_count;
  return CFP_OK;
}

// The pixels of zone z of image b, walked by the whole workgroup.  The rectangle is cut to the image once (integer bounds that select the
// pixels of the float rule; the loss walks the cut twice).  A walk goes in passes of 256 x 8: the eight depths of a lane are formed before
// the first f, so their loads are in flight together.  EVERY lane calls f(v, in) for every slot of every pass -- f may hold a ballot --
// with `in` false past the last pixel (v is then the last pixel's depth).  A lane sees its pixels in ascending order.
struct ZoneSweep {
  const float* pb; int y0, x0, rw, npx;               // npx: the in-image pixels of the zone; < 2^31 with H * W
  __device__ __forceinline__ ZoneSweep(const ZoneArgs& p, int b, int z) {
    const long long o = (long long)b * p.Z + z;
    int y1, x1;
    zc_span(p.rect[o * 4 + 0], p.rect[o * 4 + 2], p.m.H, y0, y1);
    zc_span(p.rect[o * 4 + 1], p.rect[o * 4 + 3], p.m.W, x0, x1);
    pb = p.m.pred + (long long)b * p.m.Hp * p.m.Wp;
    rw = x1 - x0; npx = (y1 - y0) * rw;
  }
  template <typename F>
  __device__ __forceinline__ void walk(const MetP& m, F f) const {
    const int tid = threadIdx.x;
    for (int c0 = 0; c0 < npx; c0 += kTofThreads * kZoneBatch) {
      float v[kZoneBatch];
#pragma unroll
      for (int u = 0; u < kZoneBatch; ++u) {
        const int i = min(c0 + u * kTofThreads + tid, npx - 1);
        const int y = i / rw, x = i - y * rw;
        v[u] = met_pred(m, pb, (y0 + y) * m.W + (x0 + x));
      }
#pragma unroll
      for (int u = 0; u < kZoneBatch; ++u) f(v[u], c0 + u * kTofThreads + tid < npx);
    }
  }
};

// The first and the last row and column of a tile, and whether rectangle r can hold a pixel of it: a NaN coordinate never does.
struct ZoneTile {
  float ylo, yhi, xlo, xhi;
  __device__ __forceinline__ bool touches(const float (&r)[4]) const { return r[0] <= yhi && ylo < r[2] && r[1] <= xhi && xlo < r[3]; }
};

// The rectangles of one chunk that can touch the tile, compacted in index order: the loop over them is short and its first hit is still
// the lowest index.  Z is not bounded by LDS.  A workgroup of kZoneChunk lanes, all of which make every call.
struct ZoneStage {
  alignas(16) float rect[kZoneChunk][4];              // one 16-byte LDS access per rectangle, and per read of the four counts
  alignas(16) int kept[kZoneChunk / 64];
  // Lane t brings rectangle r of zone z0 + t and whether to keep it: its own condition on the zone and ZoneTile::touches, formed where
  // the zone is loaded so that the loads are in flight together; false past Z.  A kept rectangle is written at `pos`, where the caller
  // writes what it keeps beside it; a barrier of the caller's closes the chunk.  Returns the number of kept zones, the same in every lane.
  __device__ __forceinline__ int stage(const float (&r)[4], bool keep, int& pos) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long k = __ballot(keep);
    __syncthreads();                                  // the chunk before is read
    if (lane == 0) kept[wave] = (int)__popcll(k);
    __syncthreads();
    pos = (int)__popcll(k & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += kept[w];
    const int nz = (kept[0] + kept[1]) + (kept[2] + kept[3]);
    if (keep) { rect[pos][0] = r[0]; rect[pos][1] = r[1]; rect[pos][2] = r[2]; rect[pos][3] = r[3]; }
    return nz;
  }
  __device__ __forceinline__ bool holds(int k, float fy, float fx) const {      // the membership rule of zc_span on staged rectangle k
    return rect[k][0] <= fy && fy < rect[k][2] && rect[k][1] <= fx && fx < rect[k][3];
  }
};

}  // namespace
