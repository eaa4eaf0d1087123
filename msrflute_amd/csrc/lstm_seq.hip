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

#include <hip/hip_runtime.h>

#include "launchers.h"

#define LSTM_H 256           // hidden size of the benchmark model
// float4 weight groups each thread keeps in registers across all T steps
// (16 is the 128-VGPR/16-wave occupancy limit, 24 spills)
#define LSTM_WREG 16

__device__ inline float sigf(float x) { return 1.f / (1.f + __expf(-x)); }

// xp:           [R, T, 4H]  pre-activation input projection (order ifgo)
// w_hh_t_stack: [K, H/4, 4H, 4]  packed transposed W_hh per client
// h_seq:        [R, T, H]   out
// gates:        [R, T, 4H]  out (ACTIVATED i,f,g,o — saved for backward)
// c_seq:        [R, T, H]   out (cell states)
// thread = gate column j = g*H + h, so the per-step GEMV reads its weight
// column fully coalesced.
__global__ __launch_bounds__(1024)
void k_lstm_seq_fwd(const float* __restrict__ xp,
                    const float* __restrict__ w_hh_t_stack,
                    float* __restrict__ h_seq,
                    float* __restrict__ gates,
                    float* __restrict__ c_seq, int rows_per_client,
                    int T) {
  __shared__ float h_prev[LSTM_H];
  __shared__ float act_l[4 * LSTM_H];
  int tid = threadIdx.x;
  int g = tid >> 8;
  int b = blockIdx.x;
  const float* w_hh_t = w_hh_t_stack
      + (long long)(b / rows_per_client) * LSTM_H * 4 * LSTM_H;
  const float4* wp = reinterpret_cast<const float4*>(w_hh_t);
  const float4* hp4 = reinterpret_cast<const float4*>(h_prev);
  if (tid < LSTM_H) h_prev[tid] = 0.f;
  float c = 0.f;
  // weights are time-invariant: keep the first LSTM_WREG float4 groups of
  // this thread's column resident in registers across ALL T steps
  // (removes 1/4 of the latency-bound per-step loads)
  float4 wreg[LSTM_WREG];
  #pragma unroll
  for (int kk = 0; kk < LSTM_WREG; ++kk)
    wreg[kk] = wp[(long long)kk * 4 * LSTM_H + tid];
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const float* xr = xp + ((long long)b * T + t) * 4 * LSTM_H;
    // float4-packed weights ([H/4, 4H, 4]: one b128 load covers 4 k's)
    // + 4 independent accumulator chains: the b32 form was bound by
    // exposed L2 latency x load count (256 loads/step/thread -> 64)
    float s0 = xr[tid], s1 = 0.f, s2 = 0.f, s3 = 0.f;
    #pragma unroll
    for (int kk = 0; kk < LSTM_WREG; ++kk) {
      float4 hv = hp4[kk];
      s0 = fmaf(wreg[kk].x, hv.x, s0);
      s1 = fmaf(wreg[kk].y, hv.y, s1);
      s2 = fmaf(wreg[kk].z, hv.z, s2);
      s3 = fmaf(wreg[kk].w, hv.w, s3);
    }
    #pragma unroll 16
    for (int kk = LSTM_WREG; kk < LSTM_H / 4; ++kk) {
      float4 wv = wp[(long long)kk * 4 * LSTM_H + tid];
      float4 hv = hp4[kk];
      s0 = fmaf(wv.x, hv.x, s0);
      s1 = fmaf(wv.y, hv.y, s1);
      s2 = fmaf(wv.z, hv.z, s2);
      s3 = fmaf(wv.w, hv.w, s3);
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
// w_hh_stack: [K, 4H/4, H, 4] packed W_hh per client; thread (q, h) sums
// its 256-row quarter of W_hh^T dg with lane-coalesced reads.
__global__ __launch_bounds__(1024)
void k_lstm_seq_bwd(const float* __restrict__ gates,
                    const float* __restrict__ c_seq,
                    const float* __restrict__ w_hh_stack,
                    const float* __restrict__ dh_out,
                    float* __restrict__ dg_pre, int rows_per_client,
                    int T) {
  __shared__ float dg_l[4 * LSTM_H];
  __shared__ float part[4 * LSTM_H];
  __shared__ float dh_rec_l[LSTM_H];
  int tid = threadIdx.x;
  int h = tid & (LSTM_H - 1), q = tid >> 8;
  int b = blockIdx.x;
  const float* w_hh = w_hh_stack
      + (long long)(b / rows_per_client) * 4 * LSTM_H * LSTM_H;
  const float4* wpB = reinterpret_cast<const float4*>(w_hh);
  const float4* dgp4 = reinterpret_cast<const float4*>(dg_l);
  float dc = 0.f;
  if (tid < LSTM_H) dh_rec_l[tid] = 0.f;
  // register-resident first LSTM_WREG weight groups of this thread's
  // quarter (time-invariant across the BPTT loop)
  float4 wregB[LSTM_WREG];
  #pragma unroll
  for (int jj = 0; jj < LSTM_WREG; ++jj)
    wregB[jj] = wpB[(long long)(q * (LSTM_H / 4) + jj) * LSTM_H + h];
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
    for (int jj = 0; jj < LSTM_WREG; ++jj) {
      float4 dv = dgp4[q * (LSTM_H / 4) + jj];
      s0 = fmaf(wregB[jj].x, dv.x, s0);
      s1 = fmaf(wregB[jj].y, dv.y, s1);
      s2 = fmaf(wregB[jj].z, dv.z, s2);
      s3 = fmaf(wregB[jj].w, dv.w, s3);
    }
    #pragma unroll 16
    for (int jj = LSTM_WREG; jj < LSTM_H / 4; ++jj) {
      int jg = q * (LSTM_H / 4) + jj;    // float4 group of 4 j's
      float4 wv = wpB[(long long)jg * LSTM_H + h];
      float4 dv = dgp4[jg];
      s0 = fmaf(wv.x, dv.x, s0);
      s1 = fmaf(wv.y, dv.y, s1);
      s2 = fmaf(wv.z, dv.z, s2);
      s3 = fmaf(wv.w, dv.w, s3);
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
  hipLaunchKernelGGL(k_lstm_seq_fwd, dim3(R), dim3(4 * LSTM_H), 0, s,
                     xp, w_hh_t_stack, h_seq, gates, c_seq,
                     rows_per_client, T);
}

void launch_lstm_seq_bwd(const float* gates, const float* c_seq,
                         const float* w_hh_stack, const float* dh_out,
                         float* dg_pre, int R, int rows_per_client, int T,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_lstm_seq_bwd, dim3(R), dim3(4 * LSTM_H), 0, s,
                     gates, c_seq, w_hh_stack, dh_out, dg_pre,
                     rows_per_client, T);
}

}  // extern "C"
