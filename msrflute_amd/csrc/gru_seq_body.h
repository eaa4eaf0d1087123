// Fused GRU sequence recurrence for gfx950 (nlg_gru task).
//
// Same design as lstm_seq.hip: one 512-thread workgroup per batch row
// runs the whole T-step recurrence; h_{t-1} is wave-broadcast from LDS;
// the forward reads W_hh transposed for coalesced lanes.  Cell math
// follows the reference GRU2 (experiments/nlg_gru/model.py:20-28):
//   gh = W_hh h + b_hh            (three blocks r, i/z, n)
//   r = sig(gi_r + gh_r); z = sig(gi_z + gh_z)
//   n = tanh(gi_n + r*gh_n);  h' = n + z*(h - n)
// gi = W_ih x + b_ih is precomputed for ALL steps by one caller GEMM.
//
// Saved for backward: r, z, n (activated, [B,T,3H]) and gh_n [B,T,H].
//
// Each kernel is ONE templated body instantiated for two weight storage
// formats (GWF32 / GWBF16 below), as in lstm_seq.hip.  bf16 is a STORAGE
// format only: a packed word widens to two exact fp32 values (u << 16,
// u & 0xffff0000), h, gi, b_hh, the gates, ghn, dgh, dh_rec and every
// accumulator stay fp32, and every product lands in the same accumulator
// chain in the same order as in the fp32 kernel.  So the bf16 pair
// computes the fp32 pair on bf16-rounded W_hh bit for bit, at half the
// bytes of the per-step L2 stream.
//
// This header holds the bodies; gru_seq.hip instantiates <GWF32> under the
// extension's flags (the code generation the fp32 pair has always had) and
// gru_seq_bf16.hip instantiates <GWBF16>, compiled without gfx950's packed
// fp32 VALU ops (setup.py; measured in profiles/r07_gru_bf16_stats.md).
#pragma once

#include <hip/hip_runtime.h>

#include "launchers.h"

#define GRU_H 512
// float4 weight groups per gate column the fp32 forward keeps in registers
// across all T steps (the fp32 backward keeps none)
#define GWREG 8
// The bf16 kernels' 8-k groups kept in registers (forward: per gate
// column, 12 VGPRs a group; backward: 4 VGPRs a group) and the unroll of
// their streamed loops (loads issued back to back).  A 512-thread block is
// 2 waves per SIMD, so a lane has up to 256 VGPRs.  The shipped counts are
// the fastest zero-scratch variants measured at B = 64, T = 25
// (profiles/r07_gru_bf16_stats.md); -D overrides on gru_seq_bf16.hip,
// timed by tools/bench_gru_seq.cpp, reproduce that table.
#ifndef GRU_WREG_BF16_FWD
#define GRU_WREG_BF16_FWD 12
#endif
#ifndef GRU_UNROLL_BF16_FWD
#define GRU_UNROLL_BF16_FWD 26
#endif
#ifndef GRU_WREG_BF16_BWD
#define GRU_WREG_BF16_BWD 12
#endif
#ifndef GRU_UNROLL_BF16_BWD
#define GRU_UNROLL_BF16_BWD 4
#endif

__device__ inline float gsig(float x) { return 1.f / (1.f + __expf(-x)); }

// Weight storage formats.  A GROUP is one 16-byte load: KPG consecutive
// k's of one column.  hvec is the KPG fp32 values of the LDS vector
// (h_prev or dgh) a group multiplies.  dot() is the forward's single
// chain per gate, consuming a float4's elements .w, .z, .y, .x; fma4() is
// the backward's four chains, element d into chain d & 3.  pin() is called
// on a register-resident group at its use inside the t loop.
struct GWF32 {
  using elem = float;
  using vec = float4;
  using hvec = float4;
  static constexpr int KPG = 4;
  static constexpr int REG_FWD = GWREG, UNROLL_FWD = 8;
  static constexpr int REG_BWD = 0, UNROLL_BWD = 8;
  // the block is always 512 threads; 1024 is the bound the fp32 backward
  // has always been compiled for (128 VGPRs)
  static constexpr int BWD_BOUND = 1024;
  static __device__ inline void pin(vec&) {}
  static __device__ inline hvec lds(const float4* v, int kk) { return v[kk]; }
  static __device__ inline float dot(const vec& w, const hvec& hv, float s) {
    return fmaf(w.x, hv.x, fmaf(w.y, hv.y,
           fmaf(w.z, hv.z, fmaf(w.w, hv.w, s))));
  }
  static __device__ inline void fma4(const vec& wv, const hvec& dv, float& s0,
                                     float& s1, float& s2, float& s3) {
    s0 = fmaf(wv.x, dv.x, s0);
    s1 = fmaf(wv.y, dv.y, s1);
    s2 = fmaf(wv.z, dv.z, s2);
    s3 = fmaf(wv.w, dv.w, s3);
  }
};

struct GWBF16 {
  using elem = unsigned short;  // raw bf16 bits
  using vec = uint4;            // 8 of them; element d even = low half of word
  struct hvec { float4 a, b; };
  static constexpr int KPG = 8;
  static constexpr int REG_FWD = GRU_WREG_BF16_FWD;
  static constexpr int UNROLL_FWD = GRU_UNROLL_BF16_FWD;
  static constexpr int REG_BWD = GRU_WREG_BF16_BWD;
  static constexpr int UNROLL_BWD = GRU_UNROLL_BF16_BWD;
  static constexpr int BWD_BOUND = GRU_H;   // 2 waves/SIMD: 256 VGPRs
  static __device__ inline float lo(unsigned u) {
    return __uint_as_float(u << 16);
  }
  static __device__ inline float hi(unsigned u) {
    return __uint_as_float(u & 0xffff0000u);
  }
  // The resident packed words are loop-invariant, so the compiler hoists
  // their widening out of the t loop and keeps the fp32 values instead
  // (twice the registers).  An empty statement that claims to rewrite the
  // words pins the widening to where the group is used (lstm_seq.hip).
  static __device__ inline void pin(vec& w) {
    asm volatile("" : "+v"(w.x), "+v"(w.y), "+v"(w.z), "+v"(w.w));
  }
  static __device__ inline hvec lds(const float4* v, int kk) {
    return {v[2 * kk], v[2 * kk + 1]};
  }
  // d = 3, 2, 1, 0, then 7, 6, 5, 4: two fp32 groups, in the fp32 order
  static __device__ inline float dot(const vec& w, const hvec& hv, float s) {
    s = fmaf(lo(w.x), hv.a.x, fmaf(hi(w.x), hv.a.y,
        fmaf(lo(w.y), hv.a.z, fmaf(hi(w.y), hv.a.w, s))));
    return fmaf(lo(w.z), hv.b.x, fmaf(hi(w.z), hv.b.y,
           fmaf(lo(w.w), hv.b.z, fmaf(hi(w.w), hv.b.w, s))));
  }
  static __device__ inline void fma4(const vec& wv, const hvec& dv, float& s0,
                                     float& s1, float& s2, float& s3) {
    s0 = fmaf(lo(wv.x), dv.a.x, s0);
    s1 = fmaf(hi(wv.x), dv.a.y, s1);
    s2 = fmaf(lo(wv.y), dv.a.z, s2);
    s3 = fmaf(hi(wv.y), dv.a.w, s3);
    s0 = fmaf(lo(wv.z), dv.b.x, s0);
    s1 = fmaf(hi(wv.z), dv.b.y, s1);
    s2 = fmaf(lo(wv.w), dv.b.z, s2);
    s3 = fmaf(hi(wv.w), dv.b.w, s3);
  }
};

// gi:     [B, T, 3H]
// whh_t:  [H/KPG, 3H, KPG]  packed transposed W_hh: element (kk, j, d) =
//         W_hh[j, KPG*kk + d] (fp32: ops/lstm._gru_pack_fwd, bf16:
//         _gru_pack_fwd_bf16) — one 16-byte load per KPG hidden units
// b_hh:   [3H]
// h_seq:  [B, T, H] out
// gates:  [B, T, 3H] out (activated r, z, n)
// ghn:    [B, T, H] out (pre-activation hidden contribution of the n gate)
template <typename W>
__global__ __launch_bounds__(GRU_H)
void k_gru_seq_fwd(const float* __restrict__ gi,
                   const typename W::elem* __restrict__ whh_t,
                   const float* __restrict__ b_hh,
                   float* __restrict__ h_seq,
                   float* __restrict__ gates,
                   float* __restrict__ ghn, int B, int T) {
  __shared__ float h_prev[GRU_H];
  int h = threadIdx.x;
  int b = blockIdx.x;
  h_prev[h] = 0.f;
  using wvec = typename W::vec;
  constexpr int NG = GRU_H / W::KPG;      // weight groups per gate column
  // packed weights cut the latency-bound per-step loads KPG-fold, and the
  // first REG_FWD groups of each gate column stay register-resident
  // across ALL T steps (W_hh is time-invariant) — the lstm_seq.hip
  // recipe, measured +34% there
  const wvec* wp = reinterpret_cast<const wvec*>(whh_t);
  const float4* hp4 = reinterpret_cast<const float4*>(h_prev);
  constexpr int NR = W::REG_FWD > 0 ? W::REG_FWD : 1;
  wvec wrr[NR], wzr[NR], wnr[NR];
  #pragma unroll
  for (int kk = 0; kk < W::REG_FWD; ++kk) {
    wrr[kk] = wp[(long long)kk * 3 * GRU_H + h];
    wzr[kk] = wp[(long long)kk * 3 * GRU_H + GRU_H + h];
    wnr[kk] = wp[(long long)kk * 3 * GRU_H + 2 * GRU_H + h];
  }
  __syncthreads();
  float br = b_hh[h], bz = b_hh[GRU_H + h], bn = b_hh[2 * GRU_H + h];
  for (int t = 0; t < T; ++t) {
    const float* gr = gi + ((long long)b * T + t) * 3 * GRU_H;
    float sr = br, sz = bz, sn = bn;
    #pragma unroll
    for (int kk = 0; kk < W::REG_FWD; ++kk) {
      typename W::hvec hv = W::lds(hp4, kk);
      W::pin(wrr[kk]); W::pin(wzr[kk]); W::pin(wnr[kk]);
      sr = W::dot(wrr[kk], hv, sr);
      sz = W::dot(wzr[kk], hv, sz);
      sn = W::dot(wnr[kk], hv, sn);
    }
    #pragma unroll W::UNROLL_FWD
    for (int kk = W::REG_FWD; kk < NG; ++kk) {
      typename W::hvec hv = W::lds(hp4, kk);
      wvec w0 = wp[(long long)kk * 3 * GRU_H + h];
      wvec w1 = wp[(long long)kk * 3 * GRU_H + GRU_H + h];
      wvec w2 = wp[(long long)kk * 3 * GRU_H + 2 * GRU_H + h];
      sr = W::dot(w0, hv, sr);
      sz = W::dot(w1, hv, sz);
      sn = W::dot(w2, hv, sn);
    }
    float hp = h_prev[h];
    float r = gsig(gr[h] + sr);
    float z = gsig(gr[GRU_H + h] + sz);
    float n = tanhf(gr[2 * GRU_H + h] + r * sn);
    float hn = n + z * (hp - n);
    long long base = ((long long)b * T + t) * 3 * GRU_H;
    gates[base + h] = r;
    gates[base + GRU_H + h] = z;
    gates[base + 2 * GRU_H + h] = n;
    ghn[((long long)b * T + t) * GRU_H + h] = sn;
    h_seq[((long long)b * T + t) * GRU_H + h] = hn;
    __syncthreads();
    h_prev[h] = hn;
    __syncthreads();
  }
}

// Backward: produces dgh [B,T,3H] (grads wrt the PRE-activation hidden
// contributions — caller turns them into dW_hh/db_hh/dh via GEMMs) and
// dgi [B,T,3H] (grads of the input projection).
// w_hh: [3H/KPG, H, KPG] packed W_hh: element (jg, h, d) =
// W_hh[KPG*jg + d, h] (fp32: ops/lstm._gru_pack_bwd, bf16:
// _gru_pack_bwd_bf16).  The first REG_BWD groups of thread h's column stay
// in registers across the BPTT loop (bf16 only; the fp32 kernel has none).
template <typename W>
__global__ __launch_bounds__(W::BWD_BOUND)
void k_gru_seq_bwd(const float* __restrict__ gates,
                   const float* __restrict__ ghn,
                   const float* __restrict__ h_seq,
                   const typename W::elem* __restrict__ w_hh,
                   const float* __restrict__ dh_out,
                   float* __restrict__ dgi,
                   float* __restrict__ dgh, int B, int T) {
  __shared__ float dgh_l[3 * GRU_H];
  int h = threadIdx.x;
  int b = blockIdx.x;
  using wvec = typename W::vec;
  constexpr int NG = 3 * GRU_H / W::KPG;  // weight groups per column
  wvec wregB[W::REG_BWD > 0 ? W::REG_BWD : 1];
  #pragma unroll
  for (int jg = 0; jg < W::REG_BWD; ++jg)
    wregB[jg] = reinterpret_cast<const wvec*>(w_hh)[(long long)jg * GRU_H + h];
  float dh_rec = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    long long base = ((long long)b * T + t) * 3 * GRU_H;
    long long hbase = ((long long)b * T + t) * GRU_H;
    float r = gates[base + h];
    float z = gates[base + GRU_H + h];
    float n = gates[base + 2 * GRU_H + h];
    float sn = ghn[hbase + h];
    float hp = (t > 0) ? h_seq[hbase - GRU_H + h] : 0.f;
    float dh = dh_out[hbase + h] + dh_rec;
    float dn = dh * (1.f - z);
    float dz = dh * (hp - n);
    float dhp_direct = dh * z;
    float dan = dn * (1.f - n * n);        // pre-tanh n grad
    float dr = dan * sn;
    float dghn = dan * r;
    float daz = dz * z * (1.f - z);
    float dar = dr * r * (1.f - r);
    // input-projection grads (gate order r, z, n)
    dgi[base + h] = dar;
    dgi[base + GRU_H + h] = daz;
    dgi[base + 2 * GRU_H + h] = dan;
    dgh[base + h] = dar;
    dgh[base + GRU_H + h] = daz;
    dgh[base + 2 * GRU_H + h] = dghn;
    __syncthreads();
    dgh_l[h] = dar;
    dgh_l[GRU_H + h] = daz;
    dgh_l[2 * GRU_H + h] = dghn;
    __syncthreads();
    {
      const wvec* wpB = reinterpret_cast<const wvec*>(w_hh);
      const float4* dg4 = reinterpret_cast<const float4*>(dgh_l);
      float s0 = dhp_direct, s1 = 0.f, s2 = 0.f, s3 = 0.f;
      #pragma unroll
      for (int jg = 0; jg < W::REG_BWD; ++jg) {
        W::pin(wregB[jg]);
        W::fma4(wregB[jg], W::lds(dg4, jg), s0, s1, s2, s3);
      }
      #pragma unroll W::UNROLL_BWD
      for (int jg = W::REG_BWD; jg < NG; ++jg) {
        wvec wv = wpB[(long long)jg * GRU_H + h];
        W::fma4(wv, W::lds(dg4, jg), s0, s1, s2, s3);
      }
      dh_rec = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
  }
}

template <typename W>
static void gru_fwd(const float* gi, const typename W::elem* whh_t,
                    const float* b_hh, float* h_seq, float* gates,
                    float* ghn, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL(k_gru_seq_fwd<W>, dim3(B), dim3(GRU_H), 0, s,
                     gi, whh_t, b_hh, h_seq, gates, ghn, B, T);
}

template <typename W>
static void gru_bwd(const float* gates, const float* ghn, const float* h_seq,
                    const typename W::elem* w_hh, const float* dh_out,
                    float* dgi, float* dgh, int B, int T, hipStream_t s) {
  hipLaunchKernelGGL(k_gru_seq_bwd<W>, dim3(B), dim3(GRU_H), 0, s,
                     gates, ghn, h_seq, w_hh, dh_out, dgi, dgh, B, T);
}

