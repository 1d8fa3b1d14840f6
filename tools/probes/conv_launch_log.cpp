// Host-only log of every kernel launch the dense-convolution entry points make (no GPU is touched): the program defines hipLaunchKernel,
// the call-configuration pair, hipGetLastError, hipFuncSetAttribute, cfp_layernorm and cfp_grad_scale itself, so the library's objects,
// linked into it, print kernel symbol, grid, workgroup, LDS bytes, every ConvP field and the slab / split / ticket arguments instead of
// launching.  N random calls (seeded) of cfp_conv2d_nhwc_ex / _moments / _dgrad / _dgrad_x3 / cfp_upsample_cat_conv3x3 over debug states.
// A one-off probe, run by no test and by no tool: it leans on --allow-multiple-definition to put its own definitions first, finds kernel
// names with `nm` on itself and knows the reduce kernel by the fake workspace address it passes.
// Two builds of the library (before / after a change to csrc/conv_route.hip or csrc/conv_entry.hip) must print the same log:
//   C=cfpnet_amd/csrc; make -C $C
//   hipcc -O1 -std=c++17 --offload-arch=gfx950 -I$C -Iinclude -x hip -c tools/probes/conv_launch_log.cpp -o cll.o
//   hipcc --offload-arch=gfx950 -Wl,--allow-multiple-definition -o cll cll.o $C/*.o && ./cll 200000 > log.txt
#include "igemm_core.h"
#include <cstdio>
#include <cstdint>
#include <random>
#include <unistd.h>
#include <map>
#include <string>
extern char __executable_start;
static void dumpP(const ConvP& p) {
  printf(" P[in=%p w=%p out=%p res=%p sc=%p sh=%p ld=%d,%d,%d B=%d H=%d W=%d Cin=%d Ho=%d Wo=%d Cout=%d K=%dx%d s=%d pad=%d,%d M=%d K=%d act=%d pw=%d ln=%p,%p eps=%g rpb=%d wbs=%lld f16=%d k2=%d up=%p,%d,%d,%d,%d,%g,%g probe=%d mom=%p dil=%d]",
         p.in, p.w, p.out, p.res, (const void*)p.scale, (const void*)p.shift, p.in_ld, p.out_ld, p.res_ld, p.B, p.H, p.W, p.Cin, p.Ho, p.Wo, p.Cout, p.KH, p.KW, p.stride,
         p.pad_t, p.pad_l, p.M, p.K, p.act, p.pointwise, (const void*)p.ln_gamma, (const void*)p.ln_beta, p.ln_eps, p.rows_per_batch, p.w_bstride, p.f16, p.k2,
         p.up_src, p.up_ld, p.up_C, p.up_H, p.up_W, p.up_sy, p.up_sx, p.probe, (void*)p.mom, p.dil);
}
static int g_nlaunch = 0;
static std::map<uintptr_t, std::string> g_sym;
static uintptr_t g_sym_base = 0;
static void load_syms() {
  char self[1024] = {0}; if (readlink("/proc/self/exe", self, sizeof self - 1) <= 0) return;
  FILE* f = popen((std::string("nm --defined-only ") + self).c_str(), "r");
  char line[4096]; unsigned long a; char t; char name[4000];
  while (fgets(line, sizeof line, f)) if (sscanf(line, "%lx %c %3999s", &a, &t, name) == 3) g_sym.emplace(a, name);
  pclose(f);
  for (auto& kv : g_sym) if (kv.second == "__executable_start") g_sym_base = kv.first;
}
extern "C" hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void** args, size_t shmem, hipStream_t s) {
  ++g_nlaunch;
  printf("  launch grid=%u,%u,%u block=%u shmem=%zu", g.x, g.y, g.z, b.x, shmem);
  // ConvP is args[0] of every conv kernel; the reduce kernel (slabs, splits, ConvP) is recognised by its 3 arguments: print both candidates' sanity
  const uintptr_t a0 = *(const uintptr_t*)args[0];
  if (a0 == 0x700000000000ull || a0 == 0x700000001000ull) { printf(" slabs=%p splits=%d", (void*)a0, *(int*)args[1]); dumpP(*(const ConvP*)args[2]); }
  else dumpP(*(const ConvP*)args[0]);
  {
    auto itn = g_sym.find((uintptr_t)((const char*)f - &__executable_start) + g_sym_base);
    const std::string nm = itn == g_sym.end() ? "?" : itn->second;
    if (nm.find("igemm_x3_kernel") != std::string::npos) printf(" x3: slabs=%p splits=%d tickets=%p", *(void**)args[1], *(int*)args[2], *(void**)args[3]);
    else if (nm.find("igemm2_kernel") != std::string::npos || nm.find("conv_igemm_splitk") != std::string::npos) printf(" g: slabs=%p splits=%d", *(void**)args[1], *(int*)args[2]);
    printf(" %s", nm.c_str());
  }
  printf("\n");
  return hipSuccess;
}
static dim3 c_g, c_b; static size_t c_sh; static hipStream_t c_s;
extern "C" hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, hipStream_t s) { c_g = g; c_b = b; c_sh = sh; c_s = s; return hipSuccess; }
extern "C" hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, hipStream_t* s) { *g = c_g; *b = c_b; *sh = c_sh; *s = c_s; return hipSuccess; }
extern "C" hipError_t hipGetLastError() { return hipSuccess; }
extern "C" hipError_t hipPeekAtLastError() { return hipSuccess; }
extern "C" hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
extern "C" int cfp_layernorm(const void* in, int in_ld, const float* gamma, const float* beta, float eps, const void* residual, int res_ld, void* out, int out_ld, int rows, int C, int dtype, cfp_stream_t) {
  printf("  layernorm in=%p %d g=%p b=%p eps=%g res=%p %d out=%p %d rows=%d C=%d dt=%d\n", in, in_ld, (const void*)gamma, (const void*)beta, eps, residual, res_ld, out, out_ld, rows, C, dtype);
  return 0;
}
extern "C" int cfp_grad_scale(const float* dy, int dy_ld, int B, int Ho, int Wo, int Cout, int stride, const int* sc, float* dys, float* inv, int Cin, cfp_stream_t) {
  printf("  grad_scale dy=%p %d %d %d %d %d s=%d sc=%p dys=%p inv=%p Cin=%d\n", (const void*)dy, dy_ld, B, Ho, Wo, Cout, stride, (const void*)sc, (void*)dys, (void*)inv, Cin);
  return 0;
}
#define PTR(x) ((void*)(uintptr_t)(x))
int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  load_syms();
  std::mt19937 rng(12345);
  auto pick = [&](std::initializer_list<int> l) { auto it = l.begin(); std::advance(it, rng() % l.size()); return *it; };
  const int N = argc > 1 ? atoi(argv[1]) : 20000;
  const int reset[][2] = {{0, -1}, {1, -1}, {2, 0}, {12, 1}, {14, 1}, {15, 1}, {17, 0}, {18, 1}, {24, 1}, {26, 1}, {29, 0}, {32, 1}, {33, 4800}, {40, 1}, {16, 0}};
  for (int it = 0; it < N; ++it) {
    for (auto& r : reset) cfp_debug_set(r[0], r[1]);
    // debug state: mostly default
    const int nkeys = pick({0, 0, 0, 1, 1, 2});
    for (int k = 0; k < nkeys; ++k) {
      switch (rng() % 14) {
        case 0: cfp_debug_set(17, 1); break;  case 1: cfp_debug_set(2, 1); break;  case 2: cfp_debug_set(12, pick({0, 2})); break;
        case 3: cfp_debug_set(18, 0); break;  case 4: cfp_debug_set(24, 0); break; case 5: cfp_debug_set(40, pick({0, 2})); break;
        case 6: cfp_debug_set(15, 0); break;  case 7: cfp_debug_set(29, 1); break; case 8: cfp_debug_set(32, 0); break;
        case 9: cfp_debug_set(33, 0); break;  case 10: cfp_debug_set(1, pick({1, 2, 4, 8})); break;
        case 11: cfp_debug_set(0, pick({4, 13, 14, 19, 1, 204, 201, 300, 303, 307, 308, 413, 404, 419, 426, 500, 503, 524, 536, 599, 600, 601, 602, 540})); break;
        case 12: cfp_debug_set(26, 0); break; case 13: cfp_debug_set(14, pick({0, 2})); break;
      }
    }
    const int mode = rng() % 10;      // 0-5 conv_ex, 6 moments, 7 dgrad, 8 dgrad_x3, 9 upsample
    const int kh = pick({1, 1, 3, 3, 3, 6}), stride = kh == 6 ? 6 : pick({1, 1, 1, 2});
    const int pad = kh == 3 ? pick({1, 1, 0}) : 0;
    const int B = pick({1, 1, 2, 8, 16});
    const int Ho = pick({1, 3, 8, 15, 30, 60, 120, 240}), Wo = pick({1, 4, 20, 40, 80, 160, 320});
    const int H = (Ho - 1) * stride + kh - 2 * pad > 0 ? (Ho - 1) * stride + kh - 2 * pad + (stride == 2 ? (int)(rng() % 2) : 0) : 1, W = (Wo - 1) * stride + kh - 2 * pad > 0 ? (Wo - 1) * stride + kh - 2 * pad : 1;
    const int Cin = pick({8, 16, 24, 32, 40, 56, 64, 72, 96, 128, 168, 256, 312, 392, 512, 1392}), Cout = pick({8, 16, 24, 32, 40, 64, 72, 128, 136, 160, 224, 232, 256, 304, 512, 1024, 1392});
    const int dtype = pick({0, 1, 1, 2});
    const bool x3 = dtype == 0 && rng() % 3 != 0;
    int flags = (rng() % 5 == 0 ? 1 : 0) | (rng() % 4 == 0 ? 4 : 0) | (x3 ? 8 : 0) | (x3 && rng() % 3 == 0 ? 16 : 0);
    if (kh == 1 && stride == 1 && dtype != 0 && rng() % 8 == 0) flags |= 2;
    const bool ln = rng() % 5 == 0, res = rng() % 3 == 0;
    const int wsk = rng() % 4;      // 0 none, 1 plenty, 2 small, 3 medium
    const long long M = (long long)B * Ho * Wo;
    const size_t wsb = wsk == 0 ? 0 : wsk == 1 ? (size_t)1 << 40 : wsk == 2 ? (size_t)M * Cout * 4 * 3 : (size_t)M * Cout * 4 * 5 + 4096;
    void* ws = wsk ? PTR(0x700000000000) : nullptr;
    const int act = pick({0, 0, 1, 3});
    int rc = -99, ns = -1, rps = -1;
    printf("#%d mode=%d k=%d s=%d pad=%d B=%d %dx%d->%dx%d Cin=%d Cout=%d dt=%d flags=%d ln=%d res=%d ws=%d act=%d\n", it, mode, kh, stride, pad, B, H, W, Ho, Wo, Cin, Cout, dtype, flags, ln, res, wsk, act);
    if (mode <= 5) {
      rc = cfp_conv2d_nhwc_ex(PTR(0x100000000000), Cin + (rng() % 2) * 16, PTR(0x200000000000), rng() % 4 ? (float*)PTR(0x300000000000) : nullptr, (float*)PTR(0x310000000000), res ? PTR(0x400000000000) : nullptr, Cout,
                              PTR(0x500000000000), Cout + (rng() % 2) * 24, B, H, W, Cin, Cout, kh, kh, stride, pad, pad, Ho, Wo, act, dtype,
                              ln ? (float*)PTR(0x600000000000) : nullptr, ln ? (float*)PTR(0x610000000000) : nullptr, 1e-5f, flags, ws, wsb, nullptr);
    } else if (mode == 6) {
      const size_t mf = pick({0, 64, 100000, 100000000});
      rc = cfp_conv2d_nhwc_moments(PTR(0x100000000000), Cin, PTR(0x200000000000), (float*)PTR(0x310000000000), PTR(0x500000000000), Cout, B, H, W, Cin, Cout, kh, kh, stride, pad, pad, Ho, Wo,
                                   dtype, ws, wsb, (float*)PTR(0x800000000000), mf, &ns, &rps, nullptr);
    } else if (mode == 7) {
      rc = cfp_conv2d_dgrad(PTR(0x100000000000), Cout, PTR(0x200000000000), PTR(0x500000000000), Cin, B, H, W, Cin, Cout, kh, kh, stride, pad, pad, Ho, Wo, rng() % 2, x3 ? 3 : dtype, ws, wsb, nullptr);
    } else if (mode == 8) {
      rc = cfp_conv2d_dgrad_x3((float*)PTR(0x100000000000), Cout, PTR(0x200000000000), res ? (float*)PTR(0x400000000000) : nullptr, Cin, (float*)PTR(0x500000000000), Cin, B, H, W, Cin, Cout, kh, kh, stride, pad, pad,
                               Ho, Wo, rng() % 2 ? (int*)PTR(0x900000000000) : nullptr, ws, wsb, nullptr);
    } else {
      const int Cup = pick({32, 64, 128, 256}), Cskip = pick({8, 16, 24, 40, 56, 64});
      rc = cfp_upsample_cat_conv3x3(PTR(0x100000000000), Cup, pick({15, 30, 60, 120}), pick({20, 40, 80, 160}), Cup, PTR(0x110000000000), Cskip, Cskip, PTR(0x200000000000), (float*)PTR(0x300000000000),
                                    (float*)PTR(0x310000000000), PTR(0x500000000000), Cout, B, Ho + 1, Wo + 1, Cout, act, x3 ? 3 : dtype, nullptr);
    }
    printf("  rc=%d ns=%d rps=%d\n", rc, ns, rps);
  }
  fprintf(stderr, "%d calls, %d launches\n", N, g_nlaunch);
  return 0;
}
