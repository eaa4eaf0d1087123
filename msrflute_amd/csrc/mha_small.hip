// Fused scaled-dot-product attention for short sequences, forward and
// backward: fp32, 1 <= L <= 64, head dimension d % 4 == 0 with 4 <= d <= 32,
// any number of heads, no mask, no dropout, not causal, scale 1/sqrt(d)
// (fednewsrec: 20 heads of d = 20, L = 28 in the DocEncoder and L = 50 in
// the UserEncoder, thousands of tiny problems).
//
// q, k, v are read in the projections' own layout [N, L, heads*d]: head hd
// of row (n, i) is the d floats at (n*L + i)*S + hd*d, with the row stride S
// (in floats, S % 4 == 0, bases 16-byte aligned) an argument, so the three
// may be contiguous tensors or slices of one [N, L, 3*heads*d] GEMM output.
// o, dq, dk, dv are written contiguous [N, L, heads*d]; lse is
// [N, heads, L] = max_j s_ij + log(sum_j exp(s_ij - max)).  No
// [N, heads, L, d] copy and no score matrix exists anywhere, in global
// memory or LDS.
//
// Work split.  A lane owns one row of one (sequence, head) problem; a wave
// serves one problem, or two when L <= 32 (lanes 0-31 and 32-63).  A block
// takes HB consecutive heads of one sequence (HB chosen by the launcher
// from MHA_WAVES and the 64 KB of LDS a block may ask for), so a global row
// contributes one contiguous run of HB*d floats, which the block moves with
// cooperative float4 accesses: lanes map to (row, float4 of the run), not
// to "my own row".  Results go back the same way: after a barrier a lane
// puts its finished row over a staged row that is no longer needed, and the
// block stores the runs.  Lanes beyond L (and the waves of a last block with
// fewer heads) compute on a clamped row, arrive at every barrier and store
// nothing; a tail lane of a staging loop repeats the last item.  No load
// sits behind a lane-divergent branch.
//
// LDS rows are RS floats apart with RS/4 odd (RS = d, or d + 4 when d/4 is
// even): every LDS access here is 16 bytes wide, and the lanes of a wave
// that read their own rows then fall into distinct groups of four banks.
// K_j, V_j (and Q_i, dO_i in the column pass) are read as wave broadcasts.
//
// Registers.  A lane's q row, accumulators and (backward) k, v rows are
// float4[CAP] arrays in fully unrolled loops, slot c under the
// block-uniform guard c < d/4 (docs/kernels.md rule 2).  Two
// instantiations: CAP = 5 serves d <= 20, CAP = 8 serves 24 <= d <= 32.
//
// Arithmetic order, the same for every problem whatever N, heads or HB:
// every dot product is mha_dot (four chains, element e of each float4 into
// chain e, slots ascending, (s0+s1)+(s2+s3)); sums over j or i run
// ascending.  The scale is folded in once, where Q is staged: LDS holds
// scale*q, both backward passes use it, and dQ is scaled once at the end.
//   forward:  m_i = max_j s_ij, then p = exp(s_ij - m_i), l += p,
//             acc += p V_j; o_i = acc / l, lse_i = m_i + log(l)  (max pass
//             then sum pass: s is computed twice, nothing is ever rescaled)
//   backward: D_i = mha_dot(dO_i, O_i)
//     row pass (lane i owns dQ_i), j ascending:
//             p = exp(s_ij - lse_i), dp = mha_dot(dO_i, V_j),
//             ds = p (dp - D_i), dQ_i += ds K_j
//     column pass (lane j holds K_j, V_j, owns dK_j, dV_j), i ascending:
//             s, p, dp, ds as above from broadcast scale*Q_i, dO_i, lse_i,
//             D_i; dV_j += p dO_i, dK_j += ds (scale*Q_i)
//   One launch, no atomics.  At L = 1, p = 1, O_0 = V_0, so dp and D_0 are
//   the same mha_dot of the same operands and ds is exactly zero.
//
// Built without gfx950's packed fp32 VALU ops (setup.py), like
// gru_seq_any.hip: the chains are scalar fmaf by design.

#include <hip/hip_runtime.h>

#include <cmath>

#include "launchers.h"

// waves per block (fewer when the heads or the LDS limit say so)
#ifndef MHA_WAVES
#define MHA_WAVES 2
#endif
#define MHA_LDS_LIMIT 65536

namespace {

__device__ __forceinline__ float4 mha_ld4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ void mha_st4(float* p, float4 v) {
  *reinterpret_cast<float4*>(p) = v;
}

// a: a row in registers; b: a row in LDS
template <int CAP>
__device__ __forceinline__ float mha_dot(const float4 (&a)[CAP],
                                         const float4* b, int d4) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  #pragma unroll
  for (int c = 0; c < CAP; ++c) {
    if (c < d4) {
      float4 x = b[c];
      s0 = __builtin_fmaf(a[c].x, x.x, s0);
      s1 = __builtin_fmaf(a[c].y, x.y, s1);
      s2 = __builtin_fmaf(a[c].z, x.z, s2);
      s3 = __builtin_fmaf(a[c].w, x.w, s3);
    }
  }
  return (s0 + s1) + (s2 + s3);
}

template <int CAP>
__device__ __forceinline__ void mha_load_row(float4 (&r)[CAP],
                                             const float4* row, int d4) {
  #pragma unroll
  for (int c = 0; c < CAP; ++c) {
    r[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < d4) r[c] = row[c];
  }
}

// r += a * x
template <int CAP>
__device__ __forceinline__ void mha_axpy_row(float4 (&r)[CAP], float a,
                                             const float4* row, int d4) {
  #pragma unroll
  for (int c = 0; c < CAP; ++c) {
    if (c < d4) {
      float4 x = row[c];
      r[c].x = __builtin_fmaf(a, x.x, r[c].x);
      r[c].y = __builtin_fmaf(a, x.y, r[c].y);
      r[c].z = __builtin_fmaf(a, x.z, r[c].z);
      r[c].w = __builtin_fmaf(a, x.w, r[c].w);
    }
  }
}

// Which (sequence, heads) a block serves and which (head, row) a lane owns.
struct MhaWho {
  int n, h0, nh;     // sequence, first head, heads in this block (<= HB)
  int hl, i;         // the lane's head within the block and row, clamped
  bool live;         // false: a clamped duplicate that stores nothing
};

__device__ __forceinline__ MhaWho mha_who(int L, int heads, int HB) {
  MhaWho w;
  const int nb = (heads + HB - 1) / HB;
  w.n = blockIdx.x / nb;
  w.h0 = (blockIdx.x - w.n * nb) * HB;
  w.nh = min(HB, heads - w.h0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = L <= 32 ? 2 * wave + (lane >> 5) : wave;
  const int row = L <= 32 ? (lane & 31) : lane;
  w.live = p < w.nh && row < L;
  w.hl = min(p, w.nh - 1);
  w.i = min(row, L - 1);
  return w;
}

// Item idx of a block's staging loops: float4 c of the contiguous run of
// nh*d floats that global row `row` contributes; it lives at LDS float
// offset `lds` of a staged tensor.
struct MhaItem { int row, c, lds; };

__device__ __forceinline__ MhaItem mha_item(int idx, int L, int nh, int d4,
                                            int RS) {
  MhaItem it;
  const int run = nh * d4;
  it.row = idx / run;
  it.c = idx - it.row * run;
  const int hl = it.c / d4, part = it.c - hl * d4;
  it.lds = (hl * L + it.row) * RS + 4 * part;
  return it;
}

// LDS rows of a staged tensor -> contiguous [N, L, E] rows at `out`
__device__ __forceinline__ void mha_store_runs(const float* lds_t,
                                               float* __restrict__ out,
                                               int E, int L, int nh, int d4,
                                               int RS) {
  const int total = L * nh * d4;
  for (int base = 0; base < total; base += blockDim.x) {
    const int idx = base + (int)threadIdx.x;
    MhaItem it = mha_item(min(idx, total - 1), L, nh, d4, RS);
    float4 x = mha_ld4(lds_t + it.lds);
    if (idx < total) mha_st4(out + (long long)it.row * E + 4 * it.c, x);
  }
}

template <int CAP>
__global__ __launch_bounds__(64 * MHA_WAVES)
void k_mha_small_fwd(const float* __restrict__ q, const float* __restrict__ k,
                     const float* __restrict__ v, float* __restrict__ o,
                     float* __restrict__ lse, int L, int heads, int d4,
                     long long S, int HB, int RS, float scale) {
  extern __shared__ float4 mha_lds4[];
  float* sm = reinterpret_cast<float*>(mha_lds4);
  const MhaWho w = mha_who(L, heads, HB);
  const int d = 4 * d4, E = heads * d, RS4 = RS >> 2;
  const int tsz = HB * L * RS;               // floats per staged tensor
  float* Qs = sm;
  float* Ks = sm + tsz;
  float* Vs = sm + 2 * tsz;

  const long long in0 = (long long)w.n * L * S + w.h0 * d;
  const int total = L * w.nh * d4;
  for (int base = 0; base < total; base += blockDim.x) {
    MhaItem it = mha_item(min(base + (int)threadIdx.x, total - 1), L, w.nh,
                          d4, RS);
    const long long g = in0 + (long long)it.row * S + 4 * it.c;
    float4 xq = mha_ld4(q + g), xk = mha_ld4(k + g), xv = mha_ld4(v + g);
    xq.x *= scale; xq.y *= scale; xq.z *= scale; xq.w *= scale;
    mha_st4(Qs + it.lds, xq);
    mha_st4(Ks + it.lds, xk);
    mha_st4(Vs + it.lds, xv);
  }
  __syncthreads();

  float* q_own = Qs + (w.hl * L + w.i) * RS;
  const float4* Kh = reinterpret_cast<const float4*>(Ks + w.hl * L * RS);
  const float4* Vh = reinterpret_cast<const float4*>(Vs + w.hl * L * RS);
  float4 qr[CAP], acc[CAP];
  mha_load_row<CAP>(qr, reinterpret_cast<const float4*>(q_own), d4);
  float m = -__builtin_huge_valf();
  for (int j = 0; j < L; ++j)
    m = __builtin_fmaxf(m, mha_dot<CAP>(qr, Kh + j * RS4, d4));
  #pragma unroll
  for (int c = 0; c < CAP; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  float l = 0.f;
  for (int j = 0; j < L; ++j) {
    float p = expf(mha_dot<CAP>(qr, Kh + j * RS4, d4) - m);
    l += p;
    mha_axpy_row<CAP>(acc, p, Vh + j * RS4, d4);
  }
  // o_i goes into the lane's Q row (all reads of Q are over), then out in runs
  __syncthreads();
  if (w.live) {
    #pragma unroll
    for (int c = 0; c < CAP; ++c)
      if (c < d4)
        mha_st4(q_own + 4 * c, make_float4(acc[c].x / l, acc[c].y / l,
                                           acc[c].z / l, acc[c].w / l));
    lse[((long long)w.n * heads + w.h0 + w.hl) * L + w.i] = m + logf(l);
  }
  __syncthreads();
  mha_store_runs(Qs, o + (long long)w.n * L * E + w.h0 * d, E, L, w.nh, d4,
                 RS);
}

template <int CAP>
__global__ __launch_bounds__(64 * MHA_WAVES)
void k_mha_small_bwd(const float* __restrict__ q, const float* __restrict__ k,
                     const float* __restrict__ v, const float* __restrict__ o,
                     const float* __restrict__ lse,
                     const float* __restrict__ d_o, float* __restrict__ dq,
                     float* __restrict__ dk, float* __restrict__ dv, int L,
                     int heads, int d4, long long S, int HB, int RS,
                     float scale) {
  extern __shared__ float4 mha_lds4[];
  float* sm = reinterpret_cast<float*>(mha_lds4);
  const MhaWho w = mha_who(L, heads, HB);
  const int d = 4 * d4, E = heads * d, RS4 = RS >> 2;
  const int tsz = HB * L * RS;
  float* Qs = sm;                 // scale*q
  float* Ks = sm + tsz;           // k, then dk
  float* Vs = sm + 2 * tsz;       // v, then dv
  float* Gs = sm + 3 * tsz;       // dO
  float* Os = sm + 4 * tsz;       // o, then dq
  float* lse_s = sm + 5 * tsz;    // [HB, L]
  float* D_s = lse_s + HB * L;    // [HB, L]

  const long long in0 = (long long)w.n * L * S + w.h0 * d;
  const long long out0 = (long long)w.n * L * E + w.h0 * d;
  const int total = L * w.nh * d4;
  for (int base = 0; base < total; base += blockDim.x) {
    MhaItem it = mha_item(min(base + (int)threadIdx.x, total - 1), L, w.nh,
                          d4, RS);
    const long long g = in0 + (long long)it.row * S + 4 * it.c;
    const long long gc = out0 + (long long)it.row * E + 4 * it.c;
    float4 xq = mha_ld4(q + g), xk = mha_ld4(k + g), xv = mha_ld4(v + g);
    float4 xg = mha_ld4(d_o + gc), xo = mha_ld4(o + gc);
    xq.x *= scale; xq.y *= scale; xq.z *= scale; xq.w *= scale;
    mha_st4(Qs + it.lds, xq);
    mha_st4(Ks + it.lds, xk);
    mha_st4(Vs + it.lds, xv);
    mha_st4(Gs + it.lds, xg);
    mha_st4(Os + it.lds, xo);
  }
  const int nlse = w.nh * L;      // heads h0 .. h0+nh-1 are contiguous in lse
  for (int base = 0; base < nlse; base += blockDim.x) {
    const int idx = min(base + (int)threadIdx.x, nlse - 1);
    lse_s[idx] = lse[((long long)w.n * heads + w.h0) * L + idx];
  }
  __syncthreads();

  const int own = (w.hl * L + w.i) * RS;
  const float4* Qh = reinterpret_cast<const float4*>(Qs + w.hl * L * RS);
  const float4* Kh = reinterpret_cast<const float4*>(Ks + w.hl * L * RS);
  const float4* Vh = reinterpret_cast<const float4*>(Vs + w.hl * L * RS);
  const float4* Gh = reinterpret_cast<const float4*>(Gs + w.hl * L * RS);
  const float* lse_h = lse_s + w.hl * L;
  float* D_h = D_s + w.hl * L;

  // a: this lane's row of the pass's first operand pair (row pass scale*Q_i
  // and dO_i, column pass K_j and V_j); r: the gradients it owns
  float4 a0[CAP], a1[CAP], r0[CAP], r1[CAP];

  // row pass
  mha_load_row<CAP>(a0, reinterpret_cast<const float4*>(Qs + own), d4);
  mha_load_row<CAP>(a1, reinterpret_cast<const float4*>(Gs + own), d4);
  const float Di =
      mha_dot<CAP>(a1, reinterpret_cast<const float4*>(Os + own), d4);
  const float lse_i = lse_h[w.i];
  #pragma unroll
  for (int c = 0; c < CAP; ++c) r0[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = 0; j < L; ++j) {
    float p = expf(mha_dot<CAP>(a0, Kh + j * RS4, d4) - lse_i);
    float dp = mha_dot<CAP>(a1, Vh + j * RS4, d4);
    mha_axpy_row<CAP>(r0, p * (dp - Di), Kh + j * RS4, d4);
  }
  // dQ_i goes into the lane's O row (all reads of O are over)
  __syncthreads();
  if (w.live) {
    #pragma unroll
    for (int c = 0; c < CAP; ++c)
      if (c < d4)
        mha_st4(Os + own + 4 * c,
                make_float4(r0[c].x * scale, r0[c].y * scale,
                            r0[c].z * scale, r0[c].w * scale));
    D_h[w.i] = Di;
  }
  __syncthreads();

  // column pass
  mha_load_row<CAP>(a0, reinterpret_cast<const float4*>(Ks + own), d4);
  mha_load_row<CAP>(a1, reinterpret_cast<const float4*>(Vs + own), d4);
  #pragma unroll
  for (int c = 0; c < CAP; ++c)
    r0[c] = r1[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = 0; i < L; ++i) {
    float p = expf(mha_dot<CAP>(a0, Qh + i * RS4, d4) - lse_h[i]);
    float dp = mha_dot<CAP>(a1, Gh + i * RS4, d4);
    mha_axpy_row<CAP>(r1, p, Gh + i * RS4, d4);                 // dV_j
    mha_axpy_row<CAP>(r0, p * (dp - D_h[i]), Qh + i * RS4, d4);   // dK_j
  }
  // dK_j, dV_j go into the lane's K and V rows (all reads of them are over)
  __syncthreads();
  if (w.live) {
    #pragma unroll
    for (int c = 0; c < CAP; ++c)
      if (c < d4) {
        mha_st4(Ks + own + 4 * c, r0[c]);
        mha_st4(Vs + own + 4 * c, r1[c]);
      }
  }
  __syncthreads();
  mha_store_runs(Os, dq + out0, E, L, w.nh, d4, RS);
  mha_store_runs(Ks, dk + out0, E, L, w.nh, d4, RS);
  mha_store_runs(Vs, dv + out0, E, L, w.nh, d4, RS);
}

// Heads per block, LDS row stride, block size and LDS bytes for a launch.
// `tensors` staged tensors of HB*L*RS floats and `vectors` of HB*L floats.
struct MhaPlan { int HB, RS, threads; size_t lds; };

MhaPlan mha_plan(int L, int heads, int d, int tensors, int vectors) {
  MhaPlan p;
  const int ppw = L <= 32 ? 2 : 1;          // problems per wave
  p.RS = (d / 4) % 2 ? d : d + 4;
  p.HB = MHA_WAVES * ppw < heads ? MHA_WAVES * ppw : heads;
  for (;; --p.HB) {
    p.lds = sizeof(float) * p.HB * L * ((size_t)tensors * p.RS + vectors);
    if (p.lds <= MHA_LDS_LIMIT || p.HB == 1) break;
  }
  p.threads = 64 * ((p.HB + ppw - 1) / ppw);
  return p;
}

}  // namespace

extern "C" {

void launch_mha_small_fwd(const float* q, const float* k, const float* v,
                          float* o, float* lse, int N, int L, int heads,
                          int d, long long S, hipStream_t s) {
  const MhaPlan p = mha_plan(L, heads, d, 3, 0);
  const dim3 grid(N * ((heads + p.HB - 1) / p.HB)), block(p.threads);
  const float scale = (float)(1.0 / sqrt((double)d));
  if (d <= 20)
    hipLaunchKernelGGL((k_mha_small_fwd<5>), grid, block, p.lds, s, q, k, v,
                       o, lse, L, heads, d / 4, S, p.HB, p.RS, scale);
  else
    hipLaunchKernelGGL((k_mha_small_fwd<8>), grid, block, p.lds, s, q, k, v,
                       o, lse, L, heads, d / 4, S, p.HB, p.RS, scale);
}

void launch_mha_small_bwd(const float* q, const float* k, const float* v,
                          const float* o, const float* lse, const float* d_o,
                          float* dq, float* dk, float* dv, int N, int L,
                          int heads, int d, long long S, hipStream_t s) {
  const MhaPlan p = mha_plan(L, heads, d, 5, 2);
  const dim3 grid(N * ((heads + p.HB - 1) / p.HB)), block(p.threads);
  const float scale = (float)(1.0 / sqrt((double)d));
  if (d <= 20)
    hipLaunchKernelGGL((k_mha_small_bwd<5>), grid, block, p.lds, s, q, k, v,
                       o, lse, d_o, dq, dk, dv, L, heads, d / 4, S, p.HB,
                       p.RS, scale);
  else
    hipLaunchKernelGGL((k_mha_small_bwd<8>), grid, block, p.lds, s, q, k, v,
                       o, lse, d_o, dq, dk, dv, L, heads, d / 4, S, p.HB,
                       p.RS, scale);
}

}  // extern "C"
