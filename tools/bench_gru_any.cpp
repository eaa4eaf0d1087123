// Stand-alone timing of the any-H fused GRU recurrence
// (msrflute_amd/csrc/gru_seq_any.hip) over its resident-group / unroll
// variants: the program behind the variant table in docs/kernels.md,
// "Any-H GRU".
//
//   bench_gru_any [H [B [T]]]        (default 400 16 20, the fednewsrec shape)
//
// Event-times every variant below (5 warm-up calls, then 3 x 50 calls,
// lowest and highest average printed in us) on the same random inputs.
// Chain order does not depend on the variant, so every variant's outputs
// must equal the first's bit for bit; a mismatch is exit status 4.
//
// Build (the flags setup.py gives gru_seq_any.hip):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc \
//         -Xclang -target-feature -Xclang -packed-fp32-ops \
//         -Imsrflute_amd/csrc -x hip tools/bench_gru_any.cpp -o bench_gru_any
#include "gru_seq_any.hip"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { \
  printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(3); } } while (0)

static int H = 400, B = 16, T = 20, bad = 0;
static float *d_gi, *d_bh, *d_dh, *d_pf, *d_pb;
static float *hs[2], *gt[2], *gn[2], *dgi[2], *dgh[2];

template <typename F>
static void timeit(const char* name, int reg, int unroll, F f) {
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
  printf("H %d B %d T %d %s reg %d unroll %d us %.1f %.1f\n", H, B, T, name,
         reg, unroll, lo, hi);
}

static void same(const char* nm, const float* x, const float* y, size_t n) {
  std::vector<float> a(n), b(n);
  CK(hipMemcpy(a.data(), x, n * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(b.data(), y, n * 4, hipMemcpyDeviceToHost));
  if (memcmp(a.data(), b.data(), n * 4)) { printf("%s differs\n", nm); ++bad; }
}

// slot 0 holds the first variant's outputs, slot 1 every later one's
template <int REG, int UNROLL>
static void fwd(int slot) {
  dim3 blk(64 * ((H + 63) / 64));
  timeit("fwd", REG, UNROLL, [&] {
    hipLaunchKernelGGL((k_gru_seq_any_fwd<REG, UNROLL>), dim3(B), blk, 0, 0,
                       d_gi, d_pf, d_bh, hs[slot], gt[slot], gn[slot], H, B, T);
  });
  if (slot) {
    same("h_seq", hs[0], hs[1], (size_t)B * T * H);
    same("gates", gt[0], gt[1], (size_t)B * T * 3 * H);
    same("ghn", gn[0], gn[1], (size_t)B * T * H);
  }
}

template <int REG, int UNROLL>
static void bwd(int slot) {
  dim3 blk(64 * ((H + 63) / 64));
  timeit("bwd", REG, UNROLL, [&] {
    hipLaunchKernelGGL((k_gru_seq_any_bwd<REG, UNROLL>), dim3(B), blk, 0, 0,
                       gt[0], gn[0], hs[0], d_pb, d_dh, dgi[slot], dgh[slot],
                       H, B, T);
  });
  if (slot) {
    same("dgi", dgi[0], dgi[1], (size_t)B * T * 3 * H);
    same("dgh", dgh[0], dgh[1], (size_t)B * T * 3 * H);
  }
}

int main(int argc, char** argv) {
  if (argc > 1) H = atoi(argv[1]);
  if (argc > 2) B = atoi(argv[2]);
  if (argc > 3) T = atoi(argv[3]);
  if (H % 4 || H < 4 || H > GRU_ANY_MAX_H || B < 1 || T < 1) return 2;
  std::mt19937 rng(5);
  std::normal_distribution<float> nd(0.f, 1.f);
  size_t nw = (size_t)3 * H * H, n3 = (size_t)B * T * 3 * H, n1 = (size_t)B * T * H;
  std::vector<float> pf(nw), pb(nw), gi(n3), bh(3 * H), dh(n1);
  float sc = 1.f / sqrtf((float)H);
  for (int j = 0; j < 3 * H; ++j)
    for (int k = 0; k < H; ++k) {
      float w = nd(rng) * sc;
      pf[((size_t)(k / 4) * 3 * H + j) * 4 + k % 4] = w;
      pb[((size_t)(j / 4) * H + k) * 4 + j % 4] = w;
    }
  for (auto& v : gi) v = nd(rng);
  for (auto& v : bh) v = nd(rng) * 0.05f;
  for (auto& v : dh) v = nd(rng);
  CK(hipMalloc(&d_gi, n3 * 4)); CK(hipMalloc(&d_bh, 3 * H * 4));
  CK(hipMalloc(&d_dh, n1 * 4));
  CK(hipMalloc(&d_pf, nw * 4)); CK(hipMalloc(&d_pb, nw * 4));
  for (int i = 0; i < 2; ++i) {
    CK(hipMalloc(&hs[i], n1 * 4)); CK(hipMalloc(&gt[i], n3 * 4));
    CK(hipMalloc(&gn[i], n1 * 4));
    CK(hipMalloc(&dgi[i], n3 * 4)); CK(hipMalloc(&dgh[i], n3 * 4));
  }
  CK(hipMemcpy(d_gi, gi.data(), n3 * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_bh, bh.data(), 3 * H * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_dh, dh.data(), n1 * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_pf, pf.data(), nw * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_pb, pb.data(), nw * 4, hipMemcpyHostToDevice));

  fwd<8, 8>(0);  fwd<0, 8>(1);  fwd<8, 4>(1);  fwd<12, 8>(1);
  fwd<16, 4>(1); fwd<16, 8>(1); fwd<8, 2>(1);  fwd<8, 6>(1);
  fwd<4, 4>(1);  fwd<12, 4>(1); fwd<8, 1>(1);  fwd<8, 3>(1);
  fwd<4, 2>(1);  fwd<12, 2>(1); fwd<16, 2>(1);
  bwd<0, 8>(0);  bwd<0, 4>(1);  bwd<8, 4>(1);  bwd<16, 4>(1);
  bwd<24, 8>(1); bwd<24, 4>(1); bwd<48, 8>(1); bwd<48, 4>(1);
  bwd<8, 2>(1);  bwd<8, 6>(1);  bwd<0, 6>(1);  bwd<8, 3>(1);
  bwd<8, 5>(1);  bwd<0, 3>(1);  bwd<0, 5>(1);  bwd<16, 6>(1); bwd<4, 4>(1);
  CK(hipDeviceSynchronize());
  return bad ? 4 : 0;
}
