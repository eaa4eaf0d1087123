// Stand-alone timing and bit-equality check of the fused GRU recurrence
// kernels (msrflute_amd/csrc/gru_seq*.hip): the program behind
// profiles/r07_gru_bf16_stats.md and the kernel times in PERF.md.
//
//   bench_gru_seq [B [T]]        (default 64 25, the nlg_gru shape)
//
// Event-times the four launchers (5 warm-up calls, then 3 x 50 calls,
// lowest and highest average printed in us) on random inputs whose weights
// are already bf16-rounded, so the fp32 and bf16 kernels must agree bit for
// bit; h_seq, gates, ghn, dgi, dgh are compared with memcmp and a mismatch
// is exit status 4.  Run it under rocprofv3 --kernel-trace --stats for the
// profiler's figures.
//
// Build (C = msrflute_amd/csrc, F = -O3 -std=c++17 --offload-arch=gfx950
// -fno-gpu-rdc; the objects as setup.py builds them):
//   hipcc $F -c $C/gru_seq.hip -o gru_seq.o
//   hipcc $F -Xclang -target-feature -Xclang -packed-fp32-ops \
//         [-DGRU_WREG_BF16_FWD=.. -DGRU_UNROLL_BF16_FWD=..
//          -DGRU_WREG_BF16_BWD=.. -DGRU_UNROLL_BF16_BWD=..] \
//         -c $C/gru_seq_bf16.hip -o gru_seq_bf16.o
//   hipcc $F -I$C -x hip tools/bench_gru_seq.cpp -x none \
//         gru_seq.o gru_seq_bf16.o -o bench_gru_seq
// An older revision's fp32 kernels: link its gru_seq.o alone and add
// -DNO_BF16.
#include <hip/hip_runtime.h>

#include "launchers.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { \
  printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(3); } } while (0)

static unsigned short bf16_rne(float f) {
  unsigned u; memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
static float bf16_f(unsigned short b) { unsigned u = (unsigned)b << 16; float f; memcpy(&f, &u, 4); return f; }

template <typename F>
static void timeit(const char* name, F f) {
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  for (int i = 0; i < 5; ++i) f();
  CK(hipDeviceSynchronize());
  float lo = 1e30f, hi = 0.f;
  for (int r = 0; r < 3; ++r) {
    CK(hipEventRecord(a, 0));
    for (int i = 0; i < 50; ++i) f();
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b));
    float us = ms * 1000.f / 50.f;
    lo = us < lo ? us : lo; hi = us > hi ? us : hi;
  }
  printf("%s us %.1f %.1f\n", name, lo, hi);
}

int main(int argc, char** argv) {
  const int H = 512, B = argc > 1 ? atoi(argv[1]) : 64, T = argc > 2 ? atoi(argv[2]) : 25;
  std::mt19937 rng(5);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<float> W((size_t)3 * H * H), gi((size_t)B * T * 3 * H), bh(3 * H), dh((size_t)B * T * H);
  for (auto& v : W) v = bf16_f(bf16_rne(nd(rng) * 0.0442f));   // rounded masters
  for (auto& v : gi) v = nd(rng);
  for (auto& v : bh) v = nd(rng) * 0.05f;
  for (auto& v : dh) v = nd(rng);
  // packs
  std::vector<float> pf((size_t)3 * H * H), pb((size_t)3 * H * H);
  std::vector<unsigned short> qf((size_t)3 * H * H), qb((size_t)3 * H * H);
  for (int j = 0; j < 3 * H; ++j)
    for (int k = 0; k < H; ++k) {
      float w = W[(size_t)j * H + k];
      pf[((size_t)(k / 4) * 3 * H + j) * 4 + k % 4] = w;
      pb[((size_t)(j / 4) * H + k) * 4 + j % 4] = w;
      qf[((size_t)(k / 8) * 3 * H + j) * 8 + k % 8] = bf16_rne(w);
      qb[((size_t)(j / 8) * H + k) * 8 + j % 8] = bf16_rne(w);
    }
  size_t n3 = (size_t)B * T * 3 * H, n1 = (size_t)B * T * H;
  float *d_gi, *d_bh, *d_dh, *d_pf, *d_pb, *hs[2], *gt[2], *gn[2], *dgi[2], *dgh[2];
  unsigned short *d_qf, *d_qb;
  CK(hipMalloc(&d_gi, n3 * 4)); CK(hipMalloc(&d_bh, 3 * H * 4)); CK(hipMalloc(&d_dh, n1 * 4));
  CK(hipMalloc(&d_pf, pf.size() * 4)); CK(hipMalloc(&d_pb, pb.size() * 4));
  CK(hipMalloc(&d_qf, qf.size() * 2)); CK(hipMalloc(&d_qb, qb.size() * 2));
  for (int i = 0; i < 2; ++i) {
    CK(hipMalloc(&hs[i], n1 * 4)); CK(hipMalloc(&gt[i], n3 * 4)); CK(hipMalloc(&gn[i], n1 * 4));
    CK(hipMalloc(&dgi[i], n3 * 4)); CK(hipMalloc(&dgh[i], n3 * 4));
  }
  CK(hipMemcpy(d_gi, gi.data(), n3 * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_bh, bh.data(), 3 * H * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_dh, dh.data(), n1 * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_pf, pf.data(), pf.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_pb, pb.data(), pb.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_qf, qf.data(), qf.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_qb, qb.data(), qb.size() * 2, hipMemcpyHostToDevice));

  timeit("fwd_fp32", [&] { launch_gru_seq_fwd(d_gi, d_pf, d_bh, hs[0], gt[0], gn[0], B, T, 0); });
  timeit("bwd_fp32", [&] { launch_gru_seq_bwd(gt[0], gn[0], hs[0], d_pb, d_dh, dgi[0], dgh[0], B, T, 0); });
  CK(hipDeviceSynchronize());
#ifndef NO_BF16
  timeit("fwd_bf16", [&] { launch_gru_seq_fwd_bf16(d_gi, d_qf, d_bh, hs[1], gt[1], gn[1], B, T, 0); });
  timeit("bwd_bf16", [&] { launch_gru_seq_bwd_bf16(gt[1], gn[1], hs[1], d_qb, d_dh, dgi[1], dgh[1], B, T, 0); });
  CK(hipDeviceSynchronize());
  std::vector<float> a(n3), b(n3);
  int bad = 0;
  auto cmp = [&](const char* nm, float* x, float* y, size_t n) {
    CK(hipMemcpy(a.data(), x, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(b.data(), y, n * 4, hipMemcpyDeviceToHost));
    int eq = memcmp(a.data(), b.data(), n * 4) == 0;
    double s = 0; for (size_t i = 0; i < n; ++i) s += (double)a[i] * a[i];
    printf("%s bit-equal %d sumsq %.6e\n", nm, eq, s);
    bad += !eq;
  };
  cmp("h_seq", hs[0], hs[1], n1); cmp("gates", gt[0], gt[1], n3); cmp("ghn", gn[0], gn[1], n1);
  cmp("dgi", dgi[0], dgi[1], n3); cmp("dgh", dgh[0], dgh[1], n3);
  return bad ? 4 : 0;
#else
  return 0;
#endif
}
