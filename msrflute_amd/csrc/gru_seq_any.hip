// Fused GRU sequence recurrence for any hidden size H with H % 4 == 0 and
// 4 <= H <= 512 (fednewsrec's H = 400 user encoder, nlg_gru at hidden sizes
// other than 512).  fp32 only.
//
// Cell math, outputs, saved tensors and weight layouts are those of
// k_gru_seq_fwd/_bwd<GWF32> (gru_seq_body.h), whose gsig, GWF32::dot and
// GWF32::fma4 are used here, with H a kernel argument and a leading client
// dimension on the weights (the LSTM's K-stacked contract): the grid is all
// K clients' rows, one block per row, row r belongs to client
// r / rows_per_client, and a row's arithmetic does not depend on K.
//
//   whh_t_stack [K, H/4, 3H, 4]   (kk, j, d) = W_hh[j, 4kk+d]
//   w_hh_stack  [K, 3H/4, H, 4]   (jg, h, d) = W_hh[4jg+d, h]
//   b_hh_stack  [K, 3H]
//
// Block: 64 * ceil(H / 64) threads; thread h owns hidden unit h and its
// three gate columns.  Lanes with h >= H (the tail of the last wave) run
// the whole step on a clamped index, arrive at every barrier and store
// nothing: they sit behind no branch around a load (docs/kernels.md,
// k_fc1_bwd_x_mfma_mb).
//
// Residency: the first REG groups of a thread's columns are held in fully
// unrolled register arrays across all T steps, each slot under the
// block-uniform guard `kk < NG`; the remaining NG - REG groups are streamed
// from L2 every step by a loop with a run-time trip count.  When NG <= REG
// the t loop has no weight load at all.  Which of the two a group is does
// not change the chain its products land in, or when: forward one chain per
// gate from the bias, kk ascending, a group consumed .w, .z, .y, .x;
// backward four chains, element d into chain d, s0 from dhp_direct, jg
// ascending, (s0+s1)+(s2+s3).  That is the order of the H = 512 pair, so at
// H = 512 the two pairs agree bit for bit (tests/test_gru_any_gpu.py).

#include "gru_seq_body.h"

// Resident groups (forward: per gate column, 12 VGPRs a group; backward: 4
// VGPRs a group) and the unroll of the streamed loops.  A block of up to 512
// threads is at most 2 waves per SIMD, so a lane has up to 256 VGPRs; the
// shipped counts are the fastest zero-scratch variants measured
// (docs/kernels.md, "Any-H GRU"; tools/bench_gru_any.cpp times the others).
#ifndef GRU_ANY_REG_FWD
#define GRU_ANY_REG_FWD 16
#endif
#ifndef GRU_ANY_UNROLL_FWD
#define GRU_ANY_UNROLL_FWD 2
#endif
#ifndef GRU_ANY_REG_BWD
#define GRU_ANY_REG_BWD 8
#endif
#ifndef GRU_ANY_UNROLL_BWD
#define GRU_ANY_UNROLL_BWD 5
#endif
#define GRU_ANY_MAX_H 512

// gi [R, T, 3H]; out: h_seq [R, T, H], activated gates [R, T, 3H] (r, z, n),
// ghn [R, T, H] (pre-activation hidden contribution of the n gate)
template <int REG, int UNROLL>
__global__ __launch_bounds__(GRU_ANY_MAX_H)
void k_gru_seq_any_fwd(const float* __restrict__ gi,
                       const float* __restrict__ whh_t_stack,
                       const float* __restrict__ b_hh_stack,
                       float* __restrict__ h_seq,
                       float* __restrict__ gates,
                       float* __restrict__ ghn, int H, int rows_per_client,
                       int T) {
  __shared__ float h_prev[GRU_ANY_MAX_H];
  const int H3 = 3 * H, NG = H >> 2;
  const bool live = (int)threadIdx.x < H;
  const int h = live ? (int)threadIdx.x : H - 1;   // idle lanes: clamped
  const int b = blockIdx.x;
  const int client = b / rows_per_client;
  const float4* wp = reinterpret_cast<const float4*>(
      whh_t_stack + (long long)client * H3 * H) + h;
  const float* bp = b_hh_stack + (long long)client * H3;
  const float4* hp4 = reinterpret_cast<const float4*>(h_prev);
  h_prev[threadIdx.x] = 0.f;
  constexpr int NR = REG > 0 ? REG : 1;
  float4 wrr[NR], wzr[NR], wnr[NR];
  #pragma unroll
  for (int kk = 0; kk < REG; ++kk) {
    wrr[kk] = wzr[kk] = wnr[kk] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kk < NG) {
      wrr[kk] = wp[(long long)kk * H3];
      wzr[kk] = wp[(long long)kk * H3 + H];
      wnr[kk] = wp[(long long)kk * H3 + 2 * H];
    }
  }
  __syncthreads();
  const float br = bp[h], bz = bp[H + h], bn = bp[2 * H + h];
  for (int t = 0; t < T; ++t) {
    const float* gr = gi + ((long long)b * T + t) * H3;
    float sr = br, sz = bz, sn = bn;
    #pragma unroll
    for (int kk = 0; kk < REG; ++kk) {
      if (kk < NG) {
        float4 hv = hp4[kk];
        sr = GWF32::dot(wrr[kk], hv, sr);
        sz = GWF32::dot(wzr[kk], hv, sz);
        sn = GWF32::dot(wnr[kk], hv, sn);
      }
    }
    #pragma unroll UNROLL
    for (int kk = REG; kk < NG; ++kk) {
      float4 hv = hp4[kk];
      float4 w0 = wp[(long long)kk * H3];
      float4 w1 = wp[(long long)kk * H3 + H];
      float4 w2 = wp[(long long)kk * H3 + 2 * H];
      sr = GWF32::dot(w0, hv, sr);
      sz = GWF32::dot(w1, hv, sz);
      sn = GWF32::dot(w2, hv, sn);
    }
    float hp = h_prev[h];
    float r = gsig(gr[h] + sr);
    float z = gsig(gr[H + h] + sz);
    float n = tanhf(gr[2 * H + h] + r * sn);
    float hn = n + z * (hp - n);
    if (live) {
      long long base = ((long long)b * T + t) * H3;
      gates[base + h] = r;
      gates[base + H + h] = z;
      gates[base + 2 * H + h] = n;
      ghn[((long long)b * T + t) * H + h] = sn;
      h_seq[((long long)b * T + t) * H + h] = hn;
    }
    __syncthreads();
    if (live) h_prev[h] = hn;
    __syncthreads();
  }
}

// out: dgi [R, T, 3H] (grads of the input projection) and dgh [R, T, 3H]
// (grads of the pre-activation hidden contributions; the caller's GEMM and
// sum turn them into dW_hh and db_hh)
template <int REG, int UNROLL>
__global__ __launch_bounds__(GRU_ANY_MAX_H)
void k_gru_seq_any_bwd(const float* __restrict__ gates,
                       const float* __restrict__ ghn,
                       const float* __restrict__ h_seq,
                       const float* __restrict__ w_hh_stack,
                       const float* __restrict__ dh_out,
                       float* __restrict__ dgi,
                       float* __restrict__ dgh, int H, int rows_per_client,
                       int T) {
  __shared__ float dgh_l[3 * GRU_ANY_MAX_H];
  const int H3 = 3 * H, NG = H3 >> 2;
  const bool live = (int)threadIdx.x < H;
  const int h = live ? (int)threadIdx.x : H - 1;
  const int b = blockIdx.x;
  const int client = b / rows_per_client;
  const float4* wpB = reinterpret_cast<const float4*>(
      w_hh_stack + (long long)client * H3 * H) + h;
  const float4* dg4 = reinterpret_cast<const float4*>(dgh_l);
  float4 wregB[REG > 0 ? REG : 1];
  #pragma unroll
  for (int jg = 0; jg < REG; ++jg) {
    wregB[jg] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (jg < NG) wregB[jg] = wpB[(long long)jg * H];
  }
  float dh_rec = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    long long base = ((long long)b * T + t) * H3;
    long long hbase = ((long long)b * T + t) * H;
    float r = gates[base + h];
    float z = gates[base + H + h];
    float n = gates[base + 2 * H + h];
    float sn = ghn[hbase + h];
    float hp = (t > 0) ? h_seq[hbase - H + h] : 0.f;
    float dh = dh_out[hbase + h] + dh_rec;
    float dn = dh * (1.f - z);
    float dz = dh * (hp - n);
    float dhp_direct = dh * z;
    float dan = dn * (1.f - n * n);        // pre-tanh n grad
    float dr = dan * sn;
    float dghn = dan * r;
    float daz = dz * z * (1.f - z);
    float dar = dr * r * (1.f - r);
    if (live) {
      dgi[base + h] = dar;
      dgi[base + H + h] = daz;
      dgi[base + 2 * H + h] = dan;
      dgh[base + h] = dar;
      dgh[base + H + h] = daz;
      dgh[base + 2 * H + h] = dghn;
    }
    __syncthreads();
    if (live) {
      dgh_l[h] = dar;
      dgh_l[H + h] = daz;
      dgh_l[2 * H + h] = dghn;
    }
    __syncthreads();
    float s0 = dhp_direct, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    #pragma unroll
    for (int jg = 0; jg < REG; ++jg)
      if (jg < NG) GWF32::fma4(wregB[jg], dg4[jg], s0, s1, s2, s3);
    #pragma unroll UNROLL
    for (int jg = REG; jg < NG; ++jg) {
      float4 wv = wpB[(long long)jg * H];
      GWF32::fma4(wv, dg4[jg], s0, s1, s2, s3);
    }
    dh_rec = (s0 + s1) + (s2 + s3);
    __syncthreads();
  }
}

extern "C" {

void launch_gru_seq_any_fwd(const float* gi, const float* whh_t_stack,
                            const float* b_hh_stack, float* h_seq,
                            float* gates, float* ghn, int R,
                            int rows_per_client, int T, int H,
                            hipStream_t s) {
  hipLaunchKernelGGL(
      (k_gru_seq_any_fwd<GRU_ANY_REG_FWD, GRU_ANY_UNROLL_FWD>), dim3(R),
      dim3(64 * ((H + 63) / 64)), 0, s, gi, whh_t_stack, b_hh_stack, h_seq,
      gates, ghn, H, rows_per_client, T);
}

void launch_gru_seq_any_bwd(const float* gates, const float* ghn,
                            const float* h_seq, const float* w_hh_stack,
                            const float* dh_out, float* dgi, float* dgh,
                            int R, int rows_per_client, int T, int H,
                            hipStream_t s) {
  hipLaunchKernelGGL(
      (k_gru_seq_any_bwd<GRU_ANY_REG_BWD, GRU_ANY_UNROLL_BWD>), dim3(R),
      dim3(64 * ((H + 63) / 64)), 0, s, gates, ghn, h_seq, w_hh_stack,
      dh_out, dgi, dgh, H, rows_per_client, T);
}

}  // extern "C"
