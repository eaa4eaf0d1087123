// Short-sequence attention on the fp32 MFMA, forward and backward: the
// range of mha_small.hip (fp32, 1 <= L <= 64, head dimension d % 4 == 0 with
// 4 <= d <= 32, any number of heads, no mask, no dropout, not causal, scale
// 1/sqrt(d)) and its memory contract: q, k, v are read in the projections'
// own layout, head hd of row (n, i) at (n*L + i)*S + hd*d floats, S % 4 == 0,
// bases 16-byte aligned; d_o is contiguous; o, dq, dk, dv are written
// contiguous [N, L, heads*d].  No lse: the backward reads q, k, v, d_o only.
//
// Work split.  A wave owns one (sequence, head) problem and computes it on
// v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered fmaf chain per output
// element); a block of up to 4 waves takes 4 consecutive heads of one
// sequence, so a global row contributes one run of nh*d floats that the
// block moves with cooperative float4 accesses.  Q (times the scale), K, V
// and, in the backward, dO of the block's heads are staged in LDS once, as
// [head][R = 16 MT rows][RS floats], MT = ceil(L / 16); the rows L .. R-1
// are staged as zeros.  The waves of a last block with fewer heads compute
// on the last head again, reach every barrier and store nothing.  MT and
// D4 = d / 4 are template parameters: every loop below is fully unrolled
// and no branch sits between MFMAs.
//
// LDS rows are RS floats apart with RS / 4 odd (RS = d, or d + 4).  A
// fragment read is one float per lane.  Lane l = (lo = l & 15, kq = l >> 4):
//   row fragments  X[16 x + lo][4 ks + kq]: float lo*RS + kq + const; RS / 4
//     odd makes lo*RS sixteen distinct multiples of 4 mod 64, plus kq = 0..3:
//     64 distinct banks;
//   column fragments  Z[16 x + 4 kq + r][16 ct + lo]: float 4*kq*RS + lo +
//     const, and 4*RS is an odd multiple of 16: 64 distinct banks.  A column
//     beyond d - 1 is clamped to d - 1 (a duplicate column, never stored).
//
// P stays in registers.  For a query tile `it` the scores are computed
// transposed, S^T = K (scale Q)^T with A = K and B = Q: in the 16x16x4
// result layout lane (lo, kq) then holds S[16 it + lo][16 jt + 4 kq + r],
// r = 0..3, for every key tile jt: values of ONE query row.  Row max and row
// sum are an in-lane pass (jt, then r, ascending) and two cross-lane steps
// (l ^ 16, then l ^ 32); columns j >= L are -inf for the max and 0 for the
// sum.  The same registers are the A operand of O = P V: MFMA r of key tile
// jt takes component r as A and V[16 jt + 4 kq + r][c] as B, so A and B
// agree on k = 4 kq + r and the chain over j is jt ascending, r ascending,
// kq ascending inside the instruction.  O comes out as
// O[16 it + 4 kq + r][16 ct + lo]; the row's sum is fetched from lane
// 4 kq + r and divided in.
//
// Backward, one launch, no atomics.  Row pass (per query tile): S^T and the
// row's max m and sum l exactly as in the forward (the same helper), P =
// p * (1/l); dP^T = V dO^T in the same layout; D_i = sum_j P_ij dP_ij as an
// in-lane fmaf chain (jt, r ascending) plus the two cross-lane steps;
// dS = P (dP - D); dQ = scale * (dS K), with dS as the A operand like P
// above.  Column pass (per key tile): S and dP are computed a second time
// untransposed (the same fragments with A and B exchanged, so the same
// chains and the same bits): lane (lo, kq) holds S[16 it + 4 kq + r][16 jt +
// lo], values of one key column; the three row scalars m, 1/l, D of row
// 4 kq + r come from lane 4 kq + r of the row pass by ds_bpermute, no LDS.
// dV = P^T dO and dK = dS^T (scale Q) take these registers as A, the chain
// over i being it, r, kq ascending.  At L = 1: P = 1, D = fmaf(1, dP, 0) +
// 0 + 0 = dP, dS = 0 and dQ = dK = 0 exactly.
//
// Results go into the wave's own Q / K / V rows after a barrier and leave
// as float4 runs.  A problem's arithmetic depends on L and d only, never on
// N, heads or the wave it lands in.
//
// Built without gfx950's packed fp32 VALU ops (setup.py): MFMA chains and
// scalar epilogues in a fixed order; exp_s is scalar_math.h's.

#include <hip/hip_runtime.h>

#include <cmath>

#include "launchers.h"
#include "scalar_math.h"

#define MM_HB 4
#define MM_LDS_DEFAULT 65536

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ float4 mm_ld4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ void mm_st4(float* p, float4 v) {
  *reinterpret_cast<float4*>(p) = v;
}

template <int D4>
struct MmDim {
  static constexpr int d = 4 * D4;
  static constexpr int RS = D4 % 2 ? d : d + 4;
  static constexpr int CT = (d + 15) / 16;
};

// t[x] += sum_k X[16 x + lo][k] Y[16 y + lo][k], x = 0 .. MT-1: lane
// (lo, kq) gets rows 4 kq + r of the X tile and column lo of the Y tile.
template <int MT, int D4>
__device__ __forceinline__ void mm_nt(f32x4 (&t)[MT], const float* X,
                                      const float* Y, int y, int lane) {
  constexpr int RS = MmDim<D4>::RS;
  const float* xa = X + (lane & 15) * RS + (lane >> 4);
  const float* yb = Y + (16 * y + (lane & 15)) * RS + (lane >> 4);
  #pragma unroll
  for (int ks = 0; ks < D4; ++ks) {
    const float b = yb[4 * ks];
    #pragma unroll
    for (int x = 0; x < MT; ++x)
      t[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[16 * x * RS + 4 * ks],
                                                  b, t[x], 0, 0, 0);
  }
}

// acc[ct] += sum_x sum_r p[x][r] (as A, k = 4 kq + r) Z[16 x + 4 kq + r][c]
template <int MT, int D4>
__device__ __forceinline__ void mm_pz(f32x4 (&acc)[MmDim<D4>::CT],
                                      const f32x4 (&p)[MT], const float* Z,
                                      int lane) {
  constexpr int RS = MmDim<D4>::RS, CT = MmDim<D4>::CT, d = MmDim<D4>::d;
  const float* zr = Z + 4 * (lane >> 4) * RS;
  int col[CT];
  #pragma unroll
  for (int ct = 0; ct < CT; ++ct) col[ct] = min(16 * ct + (lane & 15), d - 1);
  #pragma unroll
  for (int x = 0; x < MT; ++x) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      #pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            p[x][r], zr[(16 * x + r) * RS + col[ct]], acc[ct], 0, 0, 0);
    }
  }
}

// t holds one query row's scores, column 16 x + 4 kq + r in t[x][r]; on
// return it holds exp(s - m), 0 in the columns beyond L; l is their sum.
template <int MT>
__device__ __forceinline__ void mm_softmax(f32x4 (&t)[MT], int L, int lane,
                                           float& m, float& l) {
  const int j0 = 4 * (lane >> 4);
  m = -__builtin_huge_valf();
  #pragma unroll
  for (int x = 0; x < MT; ++x) {
    #pragma unroll
    for (int r = 0; r < 4; ++r)
      m = __builtin_fmaxf(
          m, 16 * x + j0 + r < L ? t[x][r] : -__builtin_huge_valf());
  }
  m = __builtin_fmaxf(m, __shfl_xor(m, 16));
  m = __builtin_fmaxf(m, __shfl_xor(m, 32));
  l = 0.f;
  #pragma unroll
  for (int x = 0; x < MT; ++x) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = exp_s(t[x][r] - m);
      t[x][r] = 16 * x + j0 + r < L ? e : 0.f;
      l += t[x][r];
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
}

// Which (sequence, heads) a block serves, and the wave's head.
struct MmWho {
  int n, h0, nh, hl;
  bool live;                 // false: a duplicate wave that stores nothing
};

__device__ __forceinline__ MmWho mm_who(int heads) {
  MmWho w;
  const int nb = (heads + MM_HB - 1) / MM_HB;
  w.n = blockIdx.x / nb;
  w.h0 = (blockIdx.x - w.n * nb) * MM_HB;
  w.nh = min(MM_HB, heads - w.h0);
  const int wave = (int)threadIdx.x >> 6;
  w.live = wave < w.nh;
  w.hl = min(wave, w.nh - 1);
  return w;
}

// Item idx of a staging loop: float4 c of the run of nh*d floats that row
// `row` contributes, at LDS float offset `lds` of a staged tensor.
struct MmItem { int row, c, lds; };

template <int MT, int D4>
__device__ __forceinline__ MmItem mm_item(int idx, int nh) {
  MmItem it;
  const int run = nh * D4;
  it.row = idx / run;
  it.c = idx - it.row * run;
  const int hl = it.c / D4, part = it.c - hl * D4;
  it.lds = (hl * 16 * MT + it.row) * MmDim<D4>::RS + 4 * part;
  return it;
}

// rows 0 .. L-1 of `src` (row stride S floats), times a, and zeros in rows
// L .. 16 MT - 1.  Tail lanes repeat the last item; a row beyond L loads
// row L - 1 and keeps nothing of it.
template <int MT, int D4>
__device__ __forceinline__ void mm_stage(float* dst,
                                         const float* __restrict__ src,
                                         long long S, int L, int nh,
                                         float a) {
  const int total = 16 * MT * nh * D4;
  for (int base = 0; base < total; base += blockDim.x) {
    const MmItem it =
        mm_item<MT, D4>(min(base + (int)threadIdx.x, total - 1), nh);
    float4 x = mm_ld4(src + (long long)min(it.row, L - 1) * S + 4 * it.c);
    x.x *= a; x.y *= a; x.z *= a; x.w *= a;
    mm_st4(dst + it.lds,
           it.row < L ? x : make_float4(0.f, 0.f, 0.f, 0.f));
  }
}

// LDS rows 0 .. L-1 of a staged tensor -> contiguous rows at `out`
template <int MT, int D4>
__device__ __forceinline__ void mm_store_runs(const float* lds_t,
                                              float* __restrict__ out, int E,
                                              int L, int nh) {
  const int total = L * nh * D4;
  for (int base = 0; base < total; base += blockDim.x) {
    const int idx = base + (int)threadIdx.x;
    const MmItem it = mm_item<MT, D4>(min(idx, total - 1), nh);
    const float4 x = mm_ld4(lds_t + it.lds);
    if (idx < total) mm_st4(out + (long long)it.row * E + 4 * it.c, x);
  }
}

// acc (rows 16 y + 4 kq + r, columns 16 ct + lo) times a -> the wave's rows
template <int D4>
__device__ __forceinline__ void mm_put(float* Th, int y,
                                       const f32x4 (&acc)[MmDim<D4>::CT],
                                       float a, int lane) {
  constexpr int RS = MmDim<D4>::RS, CT = MmDim<D4>::CT, d = MmDim<D4>::d;
  #pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int col = 16 * ct + (lane & 15);
    #pragma unroll
    for (int r = 0; r < 4; ++r)
      if (col < d)
        Th[(16 * y + 4 * (lane >> 4) + r) * RS + col] = acc[ct][r] * a;
  }
}

template <int MT, int D4>
__global__ __launch_bounds__(64 * MM_HB)
void k_mha_mfma_fwd(const float* __restrict__ q, const float* __restrict__ k,
                    const float* __restrict__ v, float* __restrict__ o, int L,
                    int heads, long long S, float scale) {
  constexpr int RS = MmDim<D4>::RS, CT = MmDim<D4>::CT, d = MmDim<D4>::d;
  constexpr int HS = 16 * MT * RS;            // floats per staged head
  extern __shared__ float4 mm_lds4[];
  float* sm = reinterpret_cast<float*>(mm_lds4);
  const int tsz = ((int)blockDim.x >> 6) * HS;
  float* Qs = sm;                             // scale*q, then o
  float* Ks = sm + tsz;
  float* Vs = sm + 2 * tsz;
  const MmWho w = mm_who(heads);
  const int lane = (int)threadIdx.x & 63, E = heads * d;

  const long long in0 = (long long)w.n * L * S + w.h0 * d;
  mm_stage<MT, D4>(Qs, q + in0, S, L, w.nh, scale);
  mm_stage<MT, D4>(Ks, k + in0, S, L, w.nh, 1.f);
  mm_stage<MT, D4>(Vs, v + in0, S, L, w.nh, 1.f);
  __syncthreads();

  float* Qh = Qs + w.hl * HS;
  const float* Kh = Ks + w.hl * HS;
  const float* Vh = Vs + w.hl * HS;
  f32x4 acc[MT][CT];
  float rl[MT][4];                            // row sums of rows 4 kq + r
  #pragma unroll
  for (int it = 0; it < MT; ++it) {
    f32x4 t[MT];
    #pragma unroll
    for (int x = 0; x < MT; ++x) t[x] = f32x4{0.f, 0.f, 0.f, 0.f};
    mm_nt<MT, D4>(t, Kh, Qh, it, lane);
    float m, l;
    mm_softmax<MT>(t, L, lane, m, l);
    #pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[it][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    mm_pz<MT, D4>(acc[it], t, Vh, lane);
    #pragma unroll
    for (int r = 0; r < 4; ++r) rl[it][r] = __shfl(l, 4 * (lane >> 4) + r);
  }
  // o goes into the wave's Q rows (all reads of Q are over), then out in runs
  __syncthreads();
  if (w.live) {
    #pragma unroll
    for (int it = 0; it < MT; ++it) {
      #pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int col = 16 * ct + (lane & 15);
        #pragma unroll
        for (int r = 0; r < 4; ++r)
          if (col < d)
            Qh[(16 * it + 4 * (lane >> 4) + r) * RS + col] =
                acc[it][ct][r] / rl[it][r];
      }
    }
  }
  __syncthreads();
  mm_store_runs<MT, D4>(Qs, o + (long long)w.n * L * E + w.h0 * d, E, L,
                        w.nh);
}

template <int MT, int D4>
__global__ __launch_bounds__(64 * MM_HB)
void k_mha_mfma_bwd(const float* __restrict__ q, const float* __restrict__ k,
                    const float* __restrict__ v,
                    const float* __restrict__ d_o, float* __restrict__ dq,
                    float* __restrict__ dk, float* __restrict__ dv, int L,
                    int heads, long long S, float scale) {
  constexpr int RS = MmDim<D4>::RS, CT = MmDim<D4>::CT, d = MmDim<D4>::d;
  constexpr int HS = 16 * MT * RS;
  extern __shared__ float4 mm_lds4[];
  float* sm = reinterpret_cast<float*>(mm_lds4);
  const int tsz = ((int)blockDim.x >> 6) * HS;
  float* Qs = sm;                             // scale*q, then dq
  float* Ks = sm + tsz;                       // k, then dk
  float* Vs = sm + 2 * tsz;                   // v, then dv
  float* Gs = sm + 3 * tsz;                   // dO
  const MmWho w = mm_who(heads);
  const int lane = (int)threadIdx.x & 63, E = heads * d;

  const long long in0 = (long long)w.n * L * S + w.h0 * d;
  const long long out0 = (long long)w.n * L * E + w.h0 * d;
  mm_stage<MT, D4>(Qs, q + in0, S, L, w.nh, scale);
  mm_stage<MT, D4>(Ks, k + in0, S, L, w.nh, 1.f);
  mm_stage<MT, D4>(Vs, v + in0, S, L, w.nh, 1.f);
  mm_stage<MT, D4>(Gs, d_o + out0, E, L, w.nh, 1.f);
  __syncthreads();

  float* Qh = Qs + w.hl * HS;
  float* Kh = Ks + w.hl * HS;
  float* Vh = Vs + w.hl * HS;
  const float* Gh = Gs + w.hl * HS;

  // row pass: lane (lo, kq) holds row 16 it + lo, columns 16 jt + 4 kq + r
  f32x4 gq[MT][CT];
  float rm[MT], ri[MT], rd[MT];               // the row's max, 1 / sum, D
  #pragma unroll
  for (int it = 0; it < MT; ++it) {
    f32x4 t[MT], u[MT];
    #pragma unroll
    for (int x = 0; x < MT; ++x)
      t[x] = u[x] = f32x4{0.f, 0.f, 0.f, 0.f};
    mm_nt<MT, D4>(t, Kh, Qh, it, lane);
    mm_nt<MT, D4>(u, Vh, Gh, it, lane);
    float l;
    mm_softmax<MT>(t, L, lane, rm[it], l);
    ri[it] = 1.f / l;
    float D = 0.f;
    #pragma unroll
    for (int x = 0; x < MT; ++x) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        t[x][r] *= ri[it];
        D = __builtin_fmaf(t[x][r], u[x][r], D);
      }
    }
    D += __shfl_xor(D, 16);
    D += __shfl_xor(D, 32);
    rd[it] = D;
    #pragma unroll
    for (int x = 0; x < MT; ++x) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) t[x][r] *= u[x][r] - D;
    }
    #pragma unroll
    for (int ct = 0; ct < CT; ++ct) gq[it][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    mm_pz<MT, D4>(gq[it], t, Kh, lane);
  }

  // column pass: lane (lo, kq) holds column 16 jt + lo, rows 16 it + 4 kq + r
  f32x4 gk[MT][CT], gv[MT][CT];
  #pragma unroll
  for (int jt = 0; jt < MT; ++jt) {
    f32x4 t[MT], u[MT];
    #pragma unroll
    for (int x = 0; x < MT; ++x)
      t[x] = u[x] = f32x4{0.f, 0.f, 0.f, 0.f};
    mm_nt<MT, D4>(t, Qh, Kh, jt, lane);
    mm_nt<MT, D4>(u, Gh, Vh, jt, lane);
    const bool jok = 16 * jt + (lane & 15) < L;
    #pragma unroll
    for (int x = 0; x < MT; ++x) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int src = 4 * (lane >> 4) + r;
        const float mi = __shfl(rm[x], src), ii = __shfl(ri[x], src);
        const float Di = __shfl(rd[x], src);
        const float e = exp_s(t[x][r] - mi);
        t[x][r] = (jok ? e : 0.f) * ii;
        u[x][r] = t[x][r] * (u[x][r] - Di);
      }
    }
    #pragma unroll
    for (int ct = 0; ct < CT; ++ct)
      gv[jt][ct] = gk[jt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    mm_pz<MT, D4>(gv[jt], t, Gh, lane);
    mm_pz<MT, D4>(gk[jt], u, Qh, lane);
  }

  // the gradients go into the wave's Q, K, V rows (all reads are over)
  __syncthreads();
  if (w.live) {
    #pragma unroll
    for (int y = 0; y < MT; ++y) {
      mm_put<D4>(Qh, y, gq[y], scale, lane);
      mm_put<D4>(Kh, y, gk[y], 1.f, lane);
      mm_put<D4>(Vh, y, gv[y], 1.f, lane);
    }
  }
  __syncthreads();
  mm_store_runs<MT, D4>(Qs, dq + out0, E, L, w.nh);
  mm_store_runs<MT, D4>(Ks, dk + out0, E, L, w.nh);
  mm_store_runs<MT, D4>(Vs, dv + out0, E, L, w.nh);
}

// Launch kern<MT, D4> with `tensors` staged tensors of HB heads.
template <class Kern, class... Args>
void mm_launch(Kern kern, int N, int L, int heads, int d, int tensors,
               hipStream_t s, Args... args) {
  const int HB = heads < MM_HB ? heads : MM_HB;
  const int RS = (d / 4) % 2 ? d : d + 4;
  const size_t lds =
      sizeof(float) * tensors * HB * (16 * ((L + 15) / 16)) * RS;
  if (lds > MM_LDS_DEFAULT)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  hipLaunchKernelGGL(kern, dim3(N * ((heads + MM_HB - 1) / MM_HB)),
                     dim3(64 * HB), lds, s, args...);
}

#define MM_D4_CASES(NAME, MT, ...)                                         \
  switch (d / 4) {                                                         \
    case 1: mm_launch(NAME<MT, 1>, __VA_ARGS__); break;                    \
    case 2: mm_launch(NAME<MT, 2>, __VA_ARGS__); break;                    \
    case 3: mm_launch(NAME<MT, 3>, __VA_ARGS__); break;                    \
    case 4: mm_launch(NAME<MT, 4>, __VA_ARGS__); break;                    \
    case 5: mm_launch(NAME<MT, 5>, __VA_ARGS__); break;                    \
    case 6: mm_launch(NAME<MT, 6>, __VA_ARGS__); break;                    \
    case 7: mm_launch(NAME<MT, 7>, __VA_ARGS__); break;                    \
    default: mm_launch(NAME<MT, 8>, __VA_ARGS__); break;                   \
  }

#define MM_DISPATCH(NAME, ...)                                             \
  switch ((L + 15) / 16) {                                                 \
    case 1: MM_D4_CASES(NAME, 1, __VA_ARGS__) break;                       \
    case 2: MM_D4_CASES(NAME, 2, __VA_ARGS__) break;                       \
    case 3: MM_D4_CASES(NAME, 3, __VA_ARGS__) break;                       \
    default: MM_D4_CASES(NAME, 4, __VA_ARGS__) break;                      \
  }

}  // namespace

extern "C" {

void launch_mha_mfma_fwd(const float* q, const float* k, const float* v,
                         float* o, int N, int L, int heads, int d,
                         long long S, hipStream_t s) {
  const float scale = (float)(1.0 / sqrt((double)d));
  MM_DISPATCH(k_mha_mfma_fwd, N, L, heads, d, 3, s, q, k, v, o, L, heads, S,
              scale)
}

void launch_mha_mfma_bwd(const float* q, const float* k, const float* v,
                         const float* d_o, float* dq, float* dk, float* dv,
                         int N, int L, int heads, int d, long long S,
                         hipStream_t s) {
  const float scale = (float)(1.0 / sqrt((double)d));
  MM_DISPATCH(k_mha_mfma_bwd, N, L, heads, d, 4, s, q, k, v, d_o, dq, dk, dv,
              L, heads, S, scale)
}

}  // extern "C"
