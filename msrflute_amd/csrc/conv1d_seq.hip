// Fused Conv1d + bias + ReLU over [N, T, C] rows, forward and backward-data:
// fp32, stride 1, no padding, dilation 1, groups 1; 1 <= KW <= 5,
// KW <= T <= 64, Cin % 4 == 0 with 4 <= Cin <= 512, Cout % 4 == 0 with
// 4 <= Cout <= 512 (fednewsrec titles: T = 30, Cin = 300, Cout = 400, KW = 3).
//
//   y[n, t, c]  = relu(b[c] + sum_{k < KW} sum_e x[n, t + k, e] W[c, e, k])
//   dz          = dy (y > 0)
//   dx[n, t, e] = sum_{k < KW} sum_c dz[n, t - k, c] W[c, e, k]
//
// x, dx [N, T, Cin]; y, dy [N, Lout, Cout] with Lout = T - KW + 1;
// dz_pad [N, T, Cout]; Wp [KW, Cout, Cin] with Wp[k][c][e] = W[c, e, k];
// b [Cout]; all contiguous, 16-byte aligned bases.  Nothing else is written:
// no transposed copy of x or y, no im2col, no pre-activation.  One pack
// serves both kernels: the forward reads Wp[k] as B^T (one float4 per lane
// along e), the backward reads it as B (four floats per lane, 64 contiguous
// bytes per 16 lanes), attn_pool.hip's two patterns on its row-major W1.
//
// Flat rows.  Index the rows of x by r = n T + t.  Then
//   z[r] = sum_k x_flat[r + k] Wp[k]^T
// is the convolution for every row with t <= T - KW; the other KW - 1 rows
// of each sequence mix two sequences.  They are garbage, computed on real
// data; they reach every barrier and are never stored.  So tap k's A
// fragment is the SAME LDS tile read k rows further down: no im2col, no
// staging per tap, no mask per row inside the k loop.  A block stages its
// rows and KW - 1 more; a row past the end of x is staged from the last row
// of x (it feeds garbage rows only).
// The backward is the mirror image.  dz_pad has T rows per sequence, the
// rows t >= Lout written as exact zeros, and
//   dx[r] = sum_k dz_pad_flat[r - k] Wp[k]:
// for t < k the row r - k is one of the previous sequence's zero rows, and
// the KW - 1 rows before the block's first sequence are staged as zeros.
//
// Work split (attn_pool.hip's).  A block of 4 waves owns SEQ = max(1, 64 / T)
// whole consecutive sequences, rows = nseq T <= 64 flat rows, MT =
// ceil(rows / 16) m-tiles of v_mfma_f32_16x16x4_f32.  Wave w owns n-tiles
// w, w + 4, w + 8, w + 12 of a pass of 16 and every m-tile of them: up to 16
// output tiles (two accumulators each, below), each B fragment loaded once
// per block.  ceil(Cout / 256) passes forward, ceil(Cin / 256) backward.
//
// K loop: tap-major, and within a tap the inner index (e forward, c
// backward) ascending 16 at a time.  Lane (i or j = l & 15, kq = l >> 4)
// holds a float4 at k0 + 4 kq; MFMA s = 0..3 consumes component s.  An inner
// index past its end is a clamped load with both operands zeroed.  The next
// step (of the next tap, at a tap's end) is loaded before the current
// step's MFMAs and first touched after them.
//
// LDS.  (rows + KW - 1) rows RS floats apart, RS / 4 odd (attn_pool.hip's
// rule: the 16 rows of a fragment read hit 16 distinct groups of four
// banks, whichever tap shifts them).  Forward 66 x 300 floats = 79200 B at
// the title shape, 68 x 516 = 140352 B at (KW, Cin) = (5, 512); backward
// 66 x 404 = 106656 B at Cout = 400, 140352 B at 512.  One block per CU.
// NEED_DX = false stages nothing and uses no LDS.
//
// Rows past the block's sequences and columns of a partial n-tile compute on
// a clamped row / column and store nothing; tail lanes of the staging loops
// repeat the last item.  Guards around loads are block- or wave-uniform.
//
// Arithmetic order, a function of the output element only, never of N, the
// block or the tile position.  The steps of 16 run tap ascending, then the
// inner index ascending (within 16: 4 kq + s, s-major); an element has two
// MFMA chains, one over the even steps of that sequence and one over the
// odd ones, added once, even + odd (one chain over all KW K terms measured
// 4.7 x the float32 noise floor at KW K = 2560, above the project's bound
// of 4; docs/kernels.md).  The bias is added after that, then max(., 0).
// dz is dy or +0, a select.  No atomics.  Built without gfx950's packed
// fp32 VALU ops (setup.py).

#include <hip/hip_runtime.h>

#include "launchers.h"

#define CV_THREADS 256
#define CV_ROWS 64

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ f32x4 cv_ld4(const float* p) {
  return *reinterpret_cast<const f32x4*>(p);
}
__device__ __forceinline__ void cv_st4(float* p, f32x4 v) {
  *reinterpret_cast<f32x4*>(p) = v;
}

// A and B fragments of one 16-k step: float4 per m-tile and per n-tile
struct CvFrag { f32x4 a[4], b[4]; };

// LDS float offsets of the lane's row in each m-tile (tap 0) and its
// (clamped) B column in each n-tile
struct CvLane { int aoff[4], col[4]; };

// One step of the K loop: tap and first inner index
struct CvStep { int tap, k0; };

__device__ __forceinline__ CvStep cv_next(CvStep s, int KW, int K) {
  CvStep n = s;
  if (s.k0 + 16 < K) n.k0 = s.k0 + 16;
  else if (s.tap + 1 < KW) { n.tap = s.tap + 1; n.k0 = 0; }
  return n;                    // the last step is its own successor
}

// BT: tap's B^T is row-major (forward: Wp[tap] [Cout, Cin], K = Cin, lane
// column = c); else B is (backward: K = Cout, lane column = e).  atap:
// floats between the A rows of consecutive taps (+RS forward, -RS backward).
template <bool BT>
__device__ __forceinline__ void cv_load(CvFrag& f, const float* As,
                                        const CvLane& ln, int MT, int NT,
                                        const float* __restrict__ wp, int Cin,
                                        int Cout, int atap, int K,
                                        CvStep st) {
  const int kk = st.k0 + 4 * (((int)threadIdx.x & 63) >> 4);
  const int kc = kk < K ? kk : K - 4;
  const float* a = As + st.tap * atap + kc;
  const float* w = wp + (long long)st.tap * Cout * Cin;
  #pragma unroll
  for (int mt = 0; mt < 4; ++mt)
    if (mt < MT) f.a[mt] = cv_ld4(a + ln.aoff[mt]);
  #pragma unroll
  for (int t = 0; t < 4; ++t)
    if (t < NT) {
      if (BT) {
        f.b[t] = cv_ld4(w + ln.col[t] * Cin + kc);
      } else {
        const float* q = w + kc * Cin + ln.col[t];
        f.b[t][0] = q[0];
        f.b[t][1] = q[Cin];
        f.b[t][2] = q[2 * Cin];
        f.b[t][3] = q[3 * Cin];
      }
    }
}

// cur = the loaded step nxt, the inner indices beyond K of a partial step
// set to zero in both operands; after the MFMAs of the step before.
__device__ __forceinline__ void cv_take(CvFrag& cur, const CvFrag& nxt,
                                        int MT, int NT, int K, int k0) {
  const bool ok = k0 + 4 * (((int)threadIdx.x & 63) >> 4) < K;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < MT) cur.a[i] = ok ? nxt.a[i] : zero;
    if (i < NT) cur.b[i] = ok ? nxt.b[i] : zero;
  }
}

// One step: load the step after `st` into nxt, run cur's MFMAs into acc,
// then take nxt as cur.
template <bool BT>
__device__ __forceinline__ void cv_step(f32x4 (&acc)[4][4], CvFrag& cur,
                                        CvFrag& nxt, CvStep& st,
                                        const float* As, const CvLane& ln,
                                        int MT, int NT,
                                        const float* __restrict__ wp, int Cin,
                                        int Cout, int atap, int KW, int K) {
  st = cv_next(st, KW, K);
  cv_load<BT>(nxt, As, ln, MT, NT, wp, Cin, Cout, atap, K, st);
  #pragma unroll
  for (int s = 0; s < 4; ++s) {
    #pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < NT) {
        #pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          if (mt < MT)
            acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                cur.a[mt][s], cur.b[t][s], acc[mt][t], 0, 0, 0);
      }
  }
  cv_take(cur, nxt, MT, NT, K, st.k0);
}

// acc[mt][t] = sum over taps and the inner index of A(m-tile mt, shifted by
// the tap) B(tap, n-tile slot t), as two chains: the even steps of the
// tap-major sequence and the odd ones, added once at the end.
template <bool BT>
__device__ __forceinline__ void cv_gemm(f32x4 (&acc)[4][4], const float* As,
                                        const CvLane& ln, int MT, int NT,
                                        const float* __restrict__ wp, int Cin,
                                        int Cout, int atap, int KW, int K) {
  f32x4 odd[4][4];
  #pragma unroll
  for (int mt = 0; mt < 4; ++mt)
    #pragma unroll
    for (int t = 0; t < 4; ++t)
      acc[mt][t] = odd[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  CvFrag cur, nxt;
  CvStep st = {0, 0};
  cv_load<BT>(nxt, As, ln, MT, NT, wp, Cin, Cout, atap, K, st);
  cv_take(cur, nxt, MT, NT, K, 0);
  const int steps = KW * ((K + 15) >> 4);
  for (int i = 0; i < steps; i += 2) {
    cv_step<BT>(acc, cur, nxt, st, As, ln, MT, NT, wp, Cin, Cout, atap, KW,
                K);
    if (i + 1 < steps)
      cv_step<BT>(odd, cur, nxt, st, As, ln, MT, NT, wp, Cin, Cout, atap, KW,
                  K);
  }
  #pragma unroll
  for (int mt = 0; mt < 4; ++mt)
    #pragma unroll
    for (int t = 0; t < 4; ++t) acc[mt][t] += odd[mt][t];
}

// Which sequences and flat rows a block owns.
struct CvWho { int n0, nseq, rows, MT; };

__device__ __forceinline__ CvWho cv_who(int N, int T, int SEQ) {
  CvWho w;
  w.n0 = blockIdx.x * SEQ;
  w.nseq = min(SEQ, N - w.n0);
  w.rows = w.nseq * T;
  w.MT = (w.rows + 15) >> 4;
  return w;
}

// n-tiles first + 4 t < tiles owned by a wave, and the lane's fragment
// addresses: rows clamped to rows - 1 and moved down by `lead` staged rows,
// columns clamped to ncols - 1
__device__ __forceinline__ int cv_lane(CvLane& ln, int rows, int lead, int RS,
                                       int first, int tiles, int ncols) {
  const int ij = (int)threadIdx.x & 15;
  #pragma unroll
  for (int t = 0; t < 4; ++t) {
    ln.aoff[t] = (min(16 * t + ij, rows - 1) + lead) * RS;
    ln.col[t] = min(16 * (first + 4 * t) + ij, ncols - 1);
  }
  return first < tiles ? min(4, (tiles - first + 3) >> 2) : 0;
}

__global__ __launch_bounds__(CV_THREADS)
void k_conv1d_relu_fwd(const float* __restrict__ x,
                       const float* __restrict__ wp,
                       const float* __restrict__ bias, float* __restrict__ y,
                       int N, int T, int Cin, int Cout, int KW, int SEQ,
                       int RS) {
  extern __shared__ float4 cv_lds4[];
  float* xs = reinterpret_cast<float*>(cv_lds4);   // [rows + KW - 1][RS]
  const CvWho who = cv_who(N, T, SEQ);
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int C4 = Cin >> 2, Lout = T - KW + 1;
  const long long row0 = (long long)who.n0 * T, last = (long long)N * T - 1;

  const int total = (who.rows + KW - 1) * C4;
  for (int base = 0; base < total; base += CV_THREADS) {
    const int idx = min(base + tid, total - 1);
    const int r = idx / C4, c = idx - r * C4;
    const long long gr = min(row0 + r, last);
    cv_st4(xs + r * RS + 4 * c, cv_ld4(x + gr * Cin + 4 * c));
  }
  __syncthreads();

  // row 16 mt + 4 kq + r of the tile -> row of the block's y, or -1 where
  // nothing is stored (t >= Lout, or past the block's sequences)
  int orow[4][4];
  #pragma unroll
  for (int mt = 0; mt < 4; ++mt)
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * mt + 4 * (lane >> 4) + r;
      const int s = row / T, t = row - s * T;
      orow[mt][r] = row < who.rows && t < Lout ? s * Lout + t : -1;
    }
  float* yb = y + (long long)who.n0 * Lout * Cout;

  const int tiles = (Cout + 15) >> 4;
  for (int pass = 0; pass < tiles; pass += 16) {
    CvLane ln;
    const int NT = cv_lane(ln, who.rows, 0, RS, pass + wave, tiles, Cout);
    f32x4 acc[4][4];
    cv_gemm<true>(acc, xs, ln, who.MT, NT, wp, Cin, Cout, RS, KW, Cin);
    #pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < NT) {
        const int col = 16 * (pass + wave + 4 * t) + (lane & 15);
        const float bv = bias[ln.col[t]];
        #pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          if (mt < who.MT) {
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float o = __builtin_fmaxf(acc[mt][t][r] + bv, 0.f);
              if (orow[mt][r] >= 0 && col < Cout)
                yb[orow[mt][r] * Cout + col] = o;
            }
          }
      }
  }
}

template <bool NEED_DX>
__global__ __launch_bounds__(CV_THREADS)
void k_conv1d_relu_bwd(const float* __restrict__ y,
                       const float* __restrict__ wp,
                       const float* __restrict__ dy, float* __restrict__ dx,
                       float* __restrict__ dz_pad, int N, int T, int Cin,
                       int Cout, int KW, int SEQ, int RS) {
  extern __shared__ float4 cv_lds4[];
  float* zs = reinterpret_cast<float*>(cv_lds4);   // [KW - 1 + rows][RS]
  const CvWho who = cv_who(N, T, SEQ);
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int C4 = Cout >> 2, Lout = T - KW + 1;
  const long long row0 = (long long)who.n0 * T;

  // dz = dy (y > 0), zero rows at t >= Lout: to dz_pad and, behind KW - 1
  // zero rows, to LDS as the A operand
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (NEED_DX) {
    const int lead = (KW - 1) * C4;
    for (int idx = tid; idx < lead; idx += CV_THREADS) {
      const int r = idx / C4, c = idx - r * C4;
      cv_st4(zs + r * RS + 4 * c, zero);
    }
  }
  const int total = who.rows * C4;
  for (int base = 0; base < total; base += CV_THREADS) {
    const int idx = min(base + tid, total - 1);
    const int r = idx / C4, c = idx - r * C4;
    const int s = r / T, t = r - s * T;
    const long long src =
        (((long long)(who.n0 + s) * Lout + min(t, Lout - 1)) * C4 + c) * 4;
    const f32x4 yv = cv_ld4(y + src), gv = cv_ld4(dy + src);
    f32x4 z;
    #pragma unroll
    for (int q = 0; q < 4; ++q)
      z[q] = t < Lout && yv[q] > 0.f ? gv[q] : 0.f;
    if (NEED_DX) cv_st4(zs + (KW - 1 + r) * RS + 4 * c, z);
    if (base + tid < total) cv_st4(dz_pad + row0 * Cout + 4LL * idx, z);
  }
  if (!NEED_DX) return;
  __syncthreads();

  // dx = sum_k dz_pad_flat[r - k] Wp[k], 16 n-tiles of Cin per pass
  float* db = dx + row0 * Cin;
  const int tiles = (Cin + 15) >> 4;
  for (int pass = 0; pass < tiles; pass += 16) {
    CvLane ln;
    const int NT = cv_lane(ln, who.rows, KW - 1, RS, pass + wave, tiles, Cin);
    f32x4 acc[4][4];
    cv_gemm<false>(acc, zs, ln, who.MT, NT, wp, Cin, Cout, -RS, KW, Cout);
    #pragma unroll
    for (int mt = 0; mt < 4; ++mt)
      if (mt < who.MT) {
        #pragma unroll
        for (int t = 0; t < 4; ++t)
          if (t < NT) {
            const int col = 16 * (pass + wave + 4 * t) + (lane & 15);
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = 16 * mt + 4 * (lane >> 4) + r;
              if (row < who.rows && col < Cin)
                db[row * Cin + col] = acc[mt][t][r];
            }
          }
      }
  }
}

// Sequences per block, LDS row stride of the A operand (K floats wide) and
// LDS bytes for the 64 block rows and KW - 1 more.
struct CvPlan { int SEQ, RS, blocks; size_t lds; };

CvPlan cv_plan(int N, int T, int K, int KW) {
  CvPlan p;
  p.SEQ = CV_ROWS / T > 1 ? CV_ROWS / T : 1;
  p.RS = (K / 4) % 2 ? K : K + 4;
  p.blocks = (N + p.SEQ - 1) / p.SEQ;
  p.lds = sizeof(float) * (size_t)(p.SEQ * T + KW - 1) * p.RS;
  return p;
}

// a block may ask for more than 64 KB of dynamic LDS only after this
template <class Kern>
void cv_allow_lds(Kern kern) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024);
}

}  // namespace

extern "C" {

void launch_conv1d_relu_fwd(const float* x, const float* wp,
                            const float* bias, float* y, int N, int T,
                            int Cin, int Cout, int KW, hipStream_t s) {
  static const bool once = (cv_allow_lds(k_conv1d_relu_fwd), true);
  (void)once;
  const CvPlan pl = cv_plan(N, T, Cin, KW);
  hipLaunchKernelGGL(k_conv1d_relu_fwd, dim3(pl.blocks), dim3(CV_THREADS),
                     pl.lds, s, x, wp, bias, y, N, T, Cin, Cout, KW, pl.SEQ,
                     pl.RS);
}

void launch_conv1d_relu_bwd(const float* y, const float* wp, const float* dy,
                            float* dx, float* dz_pad, int N, int T, int Cin,
                            int Cout, int KW, int need_dx, hipStream_t s) {
  static const bool once = (cv_allow_lds(k_conv1d_relu_bwd<true>), true);
  (void)once;
  const CvPlan pl = cv_plan(N, T, Cout, KW);
  if (need_dx)
    hipLaunchKernelGGL((k_conv1d_relu_bwd<true>), dim3(pl.blocks),
                       dim3(CV_THREADS), pl.lds, s, y, wp, dy, dx, dz_pad, N,
                       T, Cin, Cout, KW, pl.SEQ, pl.RS);
  else
    hipLaunchKernelGGL((k_conv1d_relu_bwd<false>), dim3(pl.blocks),
                       dim3(CV_THREADS), 0, s, y, wp, dy, dx, dz_pad, N, T,
                       Cin, Cout, KW, pl.SEQ, pl.RS);
}

}  // extern "C"
