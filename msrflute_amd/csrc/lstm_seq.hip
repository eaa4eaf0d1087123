// Fused LSTM sequence recurrence for gfx950 (nlp_rnn_fedshakespeare /
// BASELINE benchmark task 4).
//
// MIOpen's RNN path is both slow at FL batch sizes (~9 ms per batch-4
// step sequence) and segfaults under hipGraph capture, so the eager
// Shakespeare client ran at reference speed.  These two kernels run the
// ENTIRE T-step recurrence of one layer in one launch each:
//
//   fwd: given X_proj = x@W_ih^T + b_ih + b_hh (one hipBLASLt GEMM for
//        all steps, done by the caller), loop t: gates = X_proj[t] +
//        W_hh @ h_{t-1}; i,f,g,o activations; c_t, h_t.  Saves activated
//        gates + c for backward.
//   bwd: reverse BPTT loop producing the PRE-activation gate grads
//        (= grads of X_proj, from which the caller gets dW_ih, db and dx
//        with GEMMs) and dh via W_hh^T inside the loop.
//
// Parallel shape: the recurrence is serial in t but independent across
// rows — one 1024-thread workgroup (16 waves on one CU) per row, so rows
// run on separate CUs.  h_{t-1} lives in LDS and is wave-broadcast in
// the k-loop; weights stream from L2 (W_hh for H=256 is 1 MB) with 4
// waves per SIMD hiding the latency.  Gate order follows torch: i, f, g, o.
//
// Weights are K-STACKED: the grid is all clients' rows, row r belongs to
// client r / rows_per_client and each block indexes its client's
// float4-packed W_hh (ops/lstm._pack_fwd / _pack_bwd).  One launch covers
// a whole cohort's recurrence (Shakespeare mega round); the per-client
// FusedLSTM is the same launch at K = 1, rows_per_client = B.
//
// Each kernel is ONE templated body instantiated for two weight storage
// formats (WF32 / WBF16 below).  bf16 is a STORAGE format only: a packed
// word widens to two exact fp32 values in the k-loop (u << 16,
// u & 0xffff0000) and every product and sum stays fp32, so the bf16
// instantiation computes the fp32 kernel on bf16-rounded W_hh — k by k
// in the same four accumulator chains, so bit for bit.  Half the bytes
// per k halves the per-step L2 stream that bounds the fp32 kernels.

#include <hip/hip_runtime.h>

#include "launchers.h"

#define LSTM_H 256           // hidden size of the benchmark model
// float4 weight groups each thread keeps in registers across all T steps
// (16 is the 128-VGPR/16-wave occupancy limit, 24 spills)
#define LSTM_WREG 16
// The same for the bf16 kernels' 8-k groups, with the unroll of the
// streamed loop (loads issued back to back).  With half the bytes per k
// the stream no longer bounds the kernel and the widening costs one VALU
// op per k wherever the word lives, so MORE resident groups do not help:
// measured at K = 10 x 4 rows, T = 80 (profiles/r04_shakespeare_bf16_stats.md),
// forward 4 resident + 28 streamed in one batch beat 16 + 16 by 10 %, and
// backward 8 + 24 (unroll 16) beat 16 + 16 (unroll 8) by 13 %.  Both
// compile to zero scratch at 4 waves/SIMD; the table there lists the
// combinations that spill.  -D overrides reproduce that table.
#ifndef LSTM_WREG_BF16_FWD
#define LSTM_WREG_BF16_FWD 4
#endif
#ifndef LSTM_UNROLL_BF16_FWD
#define LSTM_UNROLL_BF16_FWD 28
#endif
#ifndef LSTM_WREG_BF16_BWD
#define LSTM_WREG_BF16_BWD 8
#endif
#ifndef LSTM_UNROLL_BF16_BWD
#define LSTM_UNROLL_BF16_BWD 16
#endif

__device__ inline float sigf(float x) { return 1.f / (1.f + __expf(-x)); }

// Weight storage formats.  A GROUP is one 16-byte load: KPG consecutive
// k's of one column.  fma() adds group kk's products with the fp32
// vector v (h_prev or dg, read from LDS as float4) into four independent
// accumulator chains; pin() is called on a register-resident group at
// its use inside the t loop.
struct WF32 {
  using elem = float;
  using vec = float4;
  static constexpr int KPG = 4;
  static constexpr int REG_FWD = LSTM_WREG, REG_BWD = LSTM_WREG;
  // loads of the streamed loop issued back to back
  static constexpr int UNROLL_FWD = 16, UNROLL_BWD = 16;
  static __device__ inline void pin(vec&) {}
  static __device__ inline void fma(const vec& w, const float4* v, int kk,
                                    float& s0, float& s1, float& s2,
                                    float& s3) {
    float4 hv = v[kk];
    s0 = fmaf(w.x, hv.x, s0);
    s1 = fmaf(w.y, hv.y, s1);
    s2 = fmaf(w.z, hv.z, s2);
    s3 = fmaf(w.w, hv.w, s3);
  }
};

struct WBF16 {
  using elem = unsigned short; // raw bf16 bits
  using vec = uint4;           // 8 of them; element d even = low half of word
  static constexpr int KPG = 8;
  static constexpr int REG_FWD = LSTM_WREG_BF16_FWD;
  static constexpr int REG_BWD = LSTM_WREG_BF16_BWD;
  static constexpr int UNROLL_FWD = LSTM_UNROLL_BF16_FWD;
  static constexpr int UNROLL_BWD = LSTM_UNROLL_BF16_BWD;
  static __device__ inline float lo(unsigned u) {
    return __uint_as_float(u << 16);
  }
  static __device__ inline float hi(unsigned u) {
    return __uint_as_float(u & 0xffff0000u);
  }
  // The packed words are loop-invariant, so the compiler hoists their
  // widening out of the t loop and keeps the fp32 values instead: 8
  // VGPRs per group where 4 were planned (11 resident groups spill).
  // An empty statement that claims to rewrite the words pins the
  // widening to where the group is used.
  static __device__ inline void pin(vec& w) {
    asm volatile("" : "+v"(w.x), "+v"(w.y), "+v"(w.z), "+v"(w.w));
  }
  static __device__ inline void fma(const vec& w, const float4* v, int kk,
                                    float& s0, float& s1, float& s2,
                                    float& s3) {
    float4 ha = v[2 * kk], hb = v[2 * kk + 1];
    s0 = fmaf(lo(w.x), ha.x, s0);
    s1 = fmaf(hi(w.x), ha.y, s1);
    s2 = fmaf(lo(w.y), ha.z, s2);
    s3 = fmaf(hi(w.y), ha.w, s3);
    s0 = fmaf(lo(w.z), hb.x, s0);
    s1 = fmaf(hi(w.z), hb.y, s1);
    s2 = fmaf(lo(w.w), hb.z, s2);
    s3 = fmaf(hi(w.w), hb.w, s3);
  }
};

// xp:           [R, T, 4H]  pre-activation input projection (order ifgo)
// w_hh_t_stack: [K, H/KPG, 4H, KPG]  packed transposed W_hh per client
//               (fp32: ops/lstm._pack_fwd, bf16: _pack_fwd_bf16)
// h_seq:        [R, T, H]   out
// gates:        [R, T, 4H]  out (ACTIVATED i,f,g,o — saved for backward)
// c_seq:        [R, T, H]   out (cell states)
// thread = gate column j = g*H + h, so the per-step GEMV reads its weight
// column fully coalesced.
template <typename W>
__global__ __launch_bounds__(1024)
void k_lstm_seq_fwd(const float* __restrict__ xp,
                    const typename W::elem* __restrict__ w_hh_t_stack,
                    float* __restrict__ h_seq,
                    float* __restrict__ gates,
                    float* __restrict__ c_seq, int rows_per_client,
                    int T) {
  __shared__ float h_prev[LSTM_H];
  __shared__ float act_l[4 * LSTM_H];
  int tid = threadIdx.x;
  int g = tid >> 8;
  int b = blockIdx.x;
  using wvec = typename W::vec;
  constexpr int NG = LSTM_H / W::KPG;     // weight groups per column
  const typename W::elem* w_hh_t = w_hh_t_stack
      + (long long)(b / rows_per_client) * LSTM_H * 4 * LSTM_H;
  const wvec* wp = reinterpret_cast<const wvec*>(w_hh_t);
  const float4* hp4 = reinterpret_cast<const float4*>(h_prev);
  if (tid < LSTM_H) h_prev[tid] = 0.f;
  float c = 0.f;
  // weights are time-invariant: keep the first REG_FWD groups of this
  // thread's column resident in registers across ALL T steps (fp32: 64
  // k's, removes 1/4 of the latency-bound per-step loads; bf16: 32 k's)
  wvec wreg[W::REG_FWD];
  #pragma unroll
  for (int kk = 0; kk < W::REG_FWD; ++kk)
    wreg[kk] = wp[(long long)kk * 4 * LSTM_H + tid];
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const float* xr = xp + ((long long)b * T + t) * 4 * LSTM_H;
    // float4-packed weights ([H/4, 4H, 4]: one b128 load covers 4 k's)
    // + 4 independent accumulator chains: the b32 form was bound by
    // exposed L2 latency x load count (256 loads/step/thread -> 64)
    float s0 = xr[tid], s1 = 0.f, s2 = 0.f, s3 = 0.f;
    #pragma unroll
    for (int kk = 0; kk < W::REG_FWD; ++kk) {
      W::pin(wreg[kk]);
      W::fma(wreg[kk], hp4, kk, s0, s1, s2, s3);
    }
    #pragma unroll W::UNROLL_FWD
    for (int kk = W::REG_FWD; kk < NG; ++kk) {
      wvec wv = wp[(long long)kk * 4 * LSTM_H + tid];
      W::fma(wv, hp4, kk, s0, s1, s2, s3);
    }
    float s = (s0 + s1) + (s2 + s3);
    float act = (g == 2) ? tanhf(s) : sigf(s);
    long long base = ((long long)b * T + t) * 4 * LSTM_H;
    gates[base + tid] = act;
    act_l[tid] = act;
    __syncthreads();
    if (tid < LSTM_H) {
      float i = act_l[tid], f = act_l[LSTM_H + tid];
      float gg = act_l[2 * LSTM_H + tid], o = act_l[3 * LSTM_H + tid];
      c = f * c + i * gg;
      float hn = o * tanhf(c);
      c_seq[((long long)b * T + t) * LSTM_H + tid] = c;
      h_seq[((long long)b * T + t) * LSTM_H + tid] = hn;
      h_prev[tid] = hn;
    }
    __syncthreads();
  }
}

// Backward: dh_out [R, T, H] upstream grads of h_seq; produces
// dg_pre [R, T, 4H] (pre-activation gate grads == grads of xp).
// w_hh_stack: [K, 4H/KPG, H, KPG] packed W_hh per client (fp32:
// ops/lstm._pack_bwd, bf16: _pack_bwd_bf16); thread (q, h) sums its
// 256-row quarter of W_hh^T dg with lane-coalesced reads.
template <typename W>
__global__ __launch_bounds__(1024)
void k_lstm_seq_bwd(const float* __restrict__ gates,
                    const float* __restrict__ c_seq,
                    const typename W::elem* __restrict__ w_hh_stack,
                    const float* __restrict__ dh_out,
                    float* __restrict__ dg_pre, int rows_per_client,
                    int T) {
  __shared__ float dg_l[4 * LSTM_H];
  __shared__ float part[4 * LSTM_H];
  __shared__ float dh_rec_l[LSTM_H];
  int tid = threadIdx.x;
  int h = tid & (LSTM_H - 1), q = tid >> 8;
  int b = blockIdx.x;
  using wvec = typename W::vec;
  constexpr int NG = LSTM_H / W::KPG;     // weight groups per quarter
  const typename W::elem* w_hh = w_hh_stack
      + (long long)(b / rows_per_client) * 4 * LSTM_H * LSTM_H;
  const wvec* wpB = reinterpret_cast<const wvec*>(w_hh) + h;
  const float4* dgp4 = reinterpret_cast<const float4*>(dg_l);
  float dc = 0.f;
  if (tid < LSTM_H) dh_rec_l[tid] = 0.f;
  // register-resident first REG_BWD weight groups of this thread's
  // quarter (time-invariant across the BPTT loop)
  wvec wregB[W::REG_BWD];
  #pragma unroll
  for (int jj = 0; jj < W::REG_BWD; ++jj)
    wregB[jj] = wpB[(long long)(q * NG + jj) * LSTM_H];
  __syncthreads();
  for (int t = T - 1; t >= 0; --t) {
    long long base = ((long long)b * T + t) * 4 * LSTM_H;
    long long cbase = ((long long)b * T + t) * LSTM_H;
    if (tid < LSTM_H) {
      float i = gates[base + tid];
      float f = gates[base + LSTM_H + tid];
      float g = gates[base + 2 * LSTM_H + tid];
      float o = gates[base + 3 * LSTM_H + tid];
      float ct = c_seq[cbase + tid];
      float cprev = (t > 0) ? c_seq[cbase - LSTM_H + tid] : 0.f;
      float tc = tanhf(ct);
      float dh = dh_out[cbase + tid] + dh_rec_l[tid];
      float do_ = dh * tc * o * (1.f - o);
      dc = dc + dh * o * (1.f - tc * tc);
      float di = dc * g * i * (1.f - i);
      float df = dc * cprev * f * (1.f - f);
      float dg = dc * i * (1.f - g * g);
      dc = dc * f;
      dg_l[tid] = di;
      dg_l[LSTM_H + tid] = df;
      dg_l[2 * LSTM_H + tid] = dg;
      dg_l[3 * LSTM_H + tid] = do_;
      dg_pre[base + tid] = di;
      dg_pre[base + LSTM_H + tid] = df;
      dg_pre[base + 2 * LSTM_H + tid] = dg;
      dg_pre[base + 3 * LSTM_H + tid] = do_;
    }
    __syncthreads();
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    #pragma unroll
    for (int jj = 0; jj < W::REG_BWD; ++jj) {
      W::pin(wregB[jj]);
      W::fma(wregB[jj], dgp4, q * NG + jj, s0, s1, s2, s3);
    }
    #pragma unroll W::UNROLL_BWD
    for (int jj = W::REG_BWD; jj < NG; ++jj) {
      int jg = q * NG + jj;              // group of KPG j's
      wvec wv = wpB[(long long)jg * LSTM_H];
      W::fma(wv, dgp4, jg, s0, s1, s2, s3);
    }
    float s = (s0 + s1) + (s2 + s3);
    part[tid] = s;
    __syncthreads();
    if (tid < LSTM_H)
      dh_rec_l[tid] = part[tid] + part[LSTM_H + tid]
                      + part[2 * LSTM_H + tid] + part[3 * LSTM_H + tid];
    __syncthreads();
  }
}

extern "C" {

void launch_lstm_seq_fwd(const float* xp, const float* w_hh_t_stack,
                         float* h_seq, float* gates, float* c_seq, int R,
                         int rows_per_client, int T, hipStream_t s) {
  hipLaunchKernelGGL(k_lstm_seq_fwd<WF32>, dim3(R), dim3(4 * LSTM_H), 0, s,
                     xp, w_hh_t_stack, h_seq, gates, c_seq,
                     rows_per_client, T);
}

void launch_lstm_seq_bwd(const float* gates, const float* c_seq,
                         const float* w_hh_stack, const float* dh_out,
                         float* dg_pre, int R, int rows_per_client, int T,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_lstm_seq_bwd<WF32>, dim3(R), dim3(4 * LSTM_H), 0, s,
                     gates, c_seq, w_hh_stack, dh_out, dg_pre,
                     rows_per_client, T);
}

// bf16-stored weights (raw 16-bit words; 16-byte aligned stacks)
void launch_lstm_seq_fwd_bf16(const float* xp,
                              const unsigned short* w_hh_t_stack,
                              float* h_seq, float* gates, float* c_seq,
                              int R, int rows_per_client, int T,
                              hipStream_t s) {
  hipLaunchKernelGGL(k_lstm_seq_fwd<WBF16>, dim3(R), dim3(4 * LSTM_H), 0, s,
                     xp, w_hh_t_stack, h_seq, gates, c_seq,
                     rows_per_client, T);
}

void launch_lstm_seq_bwd_bf16(const float* gates, const float* c_seq,
                              const unsigned short* w_hh_stack,
                              const float* dh_out, float* dg_pre, int R,
                              int rows_per_client, int T, hipStream_t s) {
  hipLaunchKernelGGL(k_lstm_seq_bwd<WBF16>, dim3(R), dim3(4 * LSTM_H), 0, s,
                     gates, c_seq, w_hh_stack, dh_out, dg_pre,
                     rows_per_client, T);
}

}  // extern "C"
