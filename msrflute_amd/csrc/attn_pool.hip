// Fused attentive pooling, forward and backward: fp32, 1 <= L <= 64,
// D % 4 == 0 with 4 <= D <= 512, Hd % 4 == 0 with 4 <= Hd <= 256
// (fednewsrec: D = 400, Hd = 200, L = 28 / 50 / 2).
//
//   e = tanh(x W1^T + b1)   [N, L, Hd]     dp_l = dy . x_l
//   a = e . w2 + b2         [N, L]         da_l = p_l (dp_l - sum_l' p_l' dp_l')
//   p = softmax_L(a)        [N, L]         dz   = da_l w2 (1 - e^2)
//   y = sum_l p_l x_l       [N, D]         dx   = p_l dy + dz W1
//
// x [N, L, D], W1 [Hd, D], e, dz [N, L, Hd], p, da [N, L], y, dy [N, D], all
// contiguous, 16-byte aligned bases.  Nothing but e, p, y (forward) and dx,
// dz, da (backward) is written; the [N*L, Hd] pre-activation, the scores
// and the exponentials never leave the block.
//
// Work split.  A block of 4 waves owns SEQ = max(1, 64 / L) whole
// consecutive sequences (a function of L alone), that is rows = nseq * L
// <= 64 rows of the [N*L, .] matrices, MT = ceil(rows / 16) m-tiles of the
// fp32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32, a k-ordered fmaf chain
// per output element).  Wave w owns the n-tiles w, w + 4, w + 8, w + 12 of
// a pass of 16 n-tiles and all MT m-tiles of them: up to 16 independent
// accumulators, so no MFMA waits for the one before it, and the B fragment
// of an n-tile is loaded once, by its wave, for every m-tile of the block.
// The forward GEMM (K = D, N = Hd <= 256) is one pass; the backward GEMM
// (K = Hd, N = D <= 512) is up to two.
//
// Fragments, 16 k at a time.  Lane l = (i or j = l & 15, kq = l >> 4) loads
// ONE float4: A row i at k0 + 4 kq .. + 3 from LDS, and (forward) W1 row j
// at the same four k from global, W1 [Hd, D] row-major being B^T.  MFMA
// s = 0..3 of the step takes component s of both, so it sums
// k = k0 + 4 kq + s over kq: within 16 the order is s-major, not ascending,
// but it is one fixed chain per output element, the same wherever the row
// lands.  In the backward W1 row-major is B itself and a lane loads the
// four floats W1[k0 + 4 kq + s][16 nt + j] (64 contiguous bytes per 16
// lanes).  A k beyond K (K % 16 != 0) is a clamped load with both operands
// set to zero.  The next step's fragments are loaded before the MFMAs of
// the current one and first touched after them.  No packed W1 layout is
// needed for 16-byte loads.
//
// LDS.  The A operand is staged as raw rows, RS floats apart with RS / 4
// odd (RS = K when K / 4 is odd, else K + 4).  A fragment read is 16 bytes
// per lane; the 16 lanes of one kq read rows i = 0..15 at float4 index
// i * RS/4 + const, which are 16 distinct residues mod 16: 16 distinct
// groups of four banks, conflict-free.  Forward: x [rows][RS(D)] (at most
// 64 * 516 * 4 = 132096 B, 103424 B at D = 400) + 448 floats; x is read
// from global once and the staged rows serve both the GEMM and y, no
// k-chunking.  Backward: dz [rows][RS(Hd)] (at most 66560 B, 52224 B at
// Hd = 200) + 192 floats; x is needed only for dp and is read once, from
// global.  gfx950 gives a block up to 160 KB.
//
// Padding.  Rows beyond the block's sequences (up to 16 MT) and columns of
// a partial n-tile (Hd = 200 is 12.5 tiles) compute on a clamped row /
// column, arrive at every barrier and store nothing; tail lanes of the
// staging loops repeat the last item.  Guards around loads are block- or
// wave-uniform (mt < MT, t < NT); no load sits behind a lane-divergent
// branch.
//
// Arithmetic order, a function of (l, column) only, never of N, the block
// or the tile position:
//   z    one MFMA chain over k as above, + b1; e = tanh_s(z)
//   a    per lane the <= 4 n-tiles of its wave ascending (fmaf), xor
//        butterfly over the 16 column lanes (1, 2, 4, 8), the four waves as
//        (w0 + w1) + (w2 + w3), + b2
//   p    max over l ascending, exp_s(a - max), sum over l ascending, divide
//   y    fmaf chain over l ascending
//   dp   per lane float4s lane, lane + 64 of the row in four chains
//        (s0 + s1) + (s2 + s3), xor butterfly over 64 lanes (1 .. 32)
//   da   sum_l p_l dp_l as an fmaf chain over l ascending
//   dx   fmaf(p_l, dy, chain)
// No atomics.  At L = 1: p = 1, y = x, da = 1 * (dp - fmaf(1, dp, 0)) = 0
// and dx = dy, bit for bit.
//
// tanh_s / exp_s are the LSTM kernels' (scalar_math.h).  Built without
// gfx950's packed fp32 VALU ops (setup.py): the epilogues are scalar fmaf
// chains in a fixed order and the matrix work is on the MFMA pipe.

#include <hip/hip_runtime.h>

#include "launchers.h"
#include "scalar_math.h"

#define AP_THREADS 256
#define AP_ROWS 64

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ f32x4 ap_ld4(const float* p) {
  return *reinterpret_cast<const f32x4*>(p);
}
__device__ __forceinline__ void ap_st4(float* p, f32x4 v) {
  *reinterpret_cast<f32x4*>(p) = v;
}

// A and B fragments of one 16-k step: float4 per m-tile and per n-tile
struct ApFrag { f32x4 a[4], b[4]; };

// What a lane needs to address its fragments: LDS float offsets of its row
// in each m-tile and its (clamped) B column in each n-tile.
struct ApLane { int aoff[4], col[4]; };

// BT: B^T is row-major in global (forward, w = W1 [N, K]); else B is
// (backward, w = W1 [K, N]).  ldb: floats between rows of w.
template <bool BT>
__device__ __forceinline__ void ap_load(ApFrag& f, const float* As,
                                        const ApLane& ln, int MT, int NT,
                                        const float* __restrict__ w, int ldb,
                                        int K, int k0) {
  const int kk = k0 + 4 * (((int)threadIdx.x & 63) >> 4);
  const int kc = kk < K ? kk : K - 4;
  #pragma unroll
  for (int mt = 0; mt < 4; ++mt)
    if (mt < MT) f.a[mt] = ap_ld4(As + ln.aoff[mt] + kc);
  #pragma unroll
  for (int t = 0; t < 4; ++t)
    if (t < NT) {
      if (BT) {
        f.b[t] = ap_ld4(w + (long long)ln.col[t] * ldb + kc);
      } else {
        const float* q = w + (long long)kc * ldb + ln.col[t];
        f.b[t][0] = q[0];
        f.b[t][1] = q[ldb];
        f.b[t][2] = q[2 * ldb];
        f.b[t][3] = q[3 * ldb];
      }
    }
}

// cur = the loaded step nxt, with the k beyond K of a last partial step set
// to zero in both operands.  Done here, after the MFMAs of the step before,
// so that nothing waits for nxt's loads until they have had that time.
__device__ __forceinline__ void ap_take(ApFrag& cur, const ApFrag& nxt,
                                        int MT, int NT, int K, int k0) {
  const bool ok = k0 + 4 * (((int)threadIdx.x & 63) >> 4) < K;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < MT) cur.a[i] = ok ? nxt.a[i] : zero;
    if (i < NT) cur.b[i] = ok ? nxt.b[i] : zero;
  }
}

// acc[mt][t] += A(m-tile mt) B(n-tile slot t) over k = 0 .. K-1, A in LDS
template <bool BT>
__device__ __forceinline__ void ap_gemm(f32x4 (&acc)[4][4], const float* As,
                                        const ApLane& ln, int MT, int NT,
                                        const float* __restrict__ w, int ldb,
                                        int K) {
  ApFrag cur, nxt;
  ap_load<BT>(nxt, As, ln, MT, NT, w, ldb, K, 0);
  ap_take(cur, nxt, MT, NT, K, 0);
  for (int k0 = 0; k0 < K; k0 += 16) {
    // the last step loads itself again: no branch around a load
    const int kn = k0 + 16 < K ? k0 + 16 : k0;
    ap_load<BT>(nxt, As, ln, MT, NT, w, ldb, K, kn);
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
    ap_take(cur, nxt, MT, NT, K, kn);
  }
}

// Which sequences and rows a block owns.
struct ApWho {
  int n0, nseq, rows, MT;
  long long row0;              // first row of the flat [N*L, .] matrices
};

__device__ __forceinline__ ApWho ap_who(int N, int L, int SEQ) {
  ApWho w;
  w.n0 = blockIdx.x * SEQ;
  w.nseq = min(SEQ, N - w.n0);
  w.rows = w.nseq * L;
  w.MT = (w.rows + 15) >> 4;
  w.row0 = (long long)w.n0 * L;
  return w;
}

// n-tiles first + 4 t < tiles owned by a wave, and the lane's fragment
// addresses: rows clamped to rows - 1, columns to ncols - 1
__device__ __forceinline__ int ap_lane(ApLane& ln, int rows, int RS,
                                       int first, int tiles, int ncols) {
  const int ij = (int)threadIdx.x & 15;
  #pragma unroll
  for (int t = 0; t < 4; ++t) {
    ln.aoff[t] = min(16 * t + ij, rows - 1) * RS;
    ln.col[t] = min(16 * (first + 4 * t) + ij, ncols - 1);
  }
  return first < tiles ? min(4, (tiles - first + 3) >> 2) : 0;
}

template <bool SAVE_E>
__global__ __launch_bounds__(AP_THREADS)
void k_attn_pool_fwd(const float* __restrict__ x, const float* __restrict__ w1,
                     const float* __restrict__ b1,
                     const float* __restrict__ w2,
                     const float* __restrict__ b2, float* __restrict__ y,
                     float* __restrict__ p, float* __restrict__ e, int N,
                     int L, int D, int Hd, int SEQ, int RS) {
  extern __shared__ float4 ap_lds4[];
  float* xs = reinterpret_cast<float*>(ap_lds4);   // [SEQ*L][RS]
  float* part_s = xs + SEQ * L * RS;               // [4 waves][64 rows]
  float* a_s = part_s + 4 * AP_ROWS;               // [64] scores
  float* ex_s = a_s + AP_ROWS;                     // [64] exp(a - max)
  float* p_s = ex_s + AP_ROWS;                     // [64]
  const ApWho who = ap_who(N, L, SEQ);
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int D4 = D >> 2;

  // the block's rows are one contiguous run of rows * D floats
  const int total = who.rows * D4;
  for (int base = 0; base < total; base += AP_THREADS) {
    const int idx = min(base + tid, total - 1);
    const int r = idx / D4, c = idx - r * D4;
    ap_st4(xs + r * RS + 4 * c, ap_ld4(x + who.row0 * D + 4LL * idx));
  }
  __syncthreads();

  ApLane ln;
  const int NT = ap_lane(ln, who.rows, RS, wave, (Hd + 15) >> 4, Hd);
  f32x4 acc[4][4];
  #pragma unroll
  for (int mt = 0; mt < 4; ++mt)
    #pragma unroll
    for (int t = 0; t < 4; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  ap_gemm<true>(acc, xs, ln, who.MT, NT, w1, D, D);

  // bias, tanh, e, and this wave's share of e . w2 for rows 4 kq + r of
  // each m-tile; D fragment: row = 4 (l >> 4) + r, column = l & 15
  float b1v[4], w2v[4];
  #pragma unroll
  for (int t = 0; t < 4; ++t)
    if (t < NT) { b1v[t] = b1[ln.col[t]]; w2v[t] = w2[ln.col[t]]; }
  #pragma unroll
  for (int mt = 0; mt < 4; ++mt)
    if (mt < who.MT) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * mt + 4 * (lane >> 4) + r;
        float sum = 0.f;
        #pragma unroll
        for (int t = 0; t < 4; ++t)
          if (t < NT) {
            const int col = 16 * (wave + 4 * t) + (lane & 15);
            const float ev = tanh_s(acc[mt][t][r] + b1v[t]);
            if (col < Hd) sum = __builtin_fmaf(ev, w2v[t], sum);
            if (SAVE_E && col < Hd && row < who.rows)
              e[(who.row0 + row) * Hd + col] = ev;
          }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        sum += __shfl_xor(sum, 4);
        sum += __shfl_xor(sum, 8);
        if ((lane & 15) == 0) part_s[wave * AP_ROWS + row] = sum;
      }
    }
  __syncthreads();

  // thread r < 64 serves row r (clamped); every thread of a sequence runs
  // the same max and the same sum in the same order
  const int rc = min(tid, who.rows - 1), l0 = (rc / L) * L;
  if (tid < AP_ROWS)
    a_s[tid] = ((part_s[rc] + part_s[AP_ROWS + rc]) +
                (part_s[2 * AP_ROWS + rc] + part_s[3 * AP_ROWS + rc])) +
               b2[0];
  __syncthreads();
  if (tid < AP_ROWS) {
    float m = a_s[l0];
    for (int l = 1; l < L; ++l) m = __builtin_fmaxf(m, a_s[l0 + l]);
    ex_s[tid] = exp_s(a_s[rc] - m);
  }
  __syncthreads();
  if (tid < AP_ROWS) {
    float sum = 0.f;
    for (int l = 0; l < L; ++l) sum += ex_s[l0 + l];
    const float pv = ex_s[rc] / sum;
    p_s[tid] = pv;
    if (tid < who.rows) p[who.row0 + tid] = pv;
  }
  __syncthreads();

  const int items = who.nseq * D4;
  for (int base = 0; base < items; base += AP_THREADS) {
    const int idx = min(base + tid, items - 1);
    const int s = idx / D4, c = idx - s * D4;
    const float* xr = xs + s * L * RS + 4 * c;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < L; ++l) {
      const float pv = p_s[s * L + l];
      const f32x4 xv = ap_ld4(xr + l * RS);
      o[0] = __builtin_fmaf(pv, xv[0], o[0]);
      o[1] = __builtin_fmaf(pv, xv[1], o[1]);
      o[2] = __builtin_fmaf(pv, xv[2], o[2]);
      o[3] = __builtin_fmaf(pv, xv[3], o[3]);
    }
    if (base + tid < items) ap_st4(y + (long long)who.n0 * D + 4LL * idx, o);
  }
}

__global__ __launch_bounds__(AP_THREADS)
void k_attn_pool_bwd(const float* __restrict__ x, const float* __restrict__ e,
                     const float* __restrict__ p, const float* __restrict__ w1,
                     const float* __restrict__ w2,
                     const float* __restrict__ dy, float* __restrict__ dx,
                     float* __restrict__ dz, float* __restrict__ da, int N,
                     int L, int D, int Hd, int SEQ, int RS) {
  extern __shared__ float4 ap_lds4[];
  float* zs = reinterpret_cast<float*>(ap_lds4);   // dz [SEQ*L][RS]
  float* dp_s = zs + SEQ * L * RS;                 // [64]
  float* da_s = dp_s + AP_ROWS;                    // [64]
  float* p_s = da_s + AP_ROWS;                     // [64]
  const ApWho who = ap_who(N, L, SEQ);
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int D4 = D >> 2, H4 = Hd >> 2;

  // dp_l = dy . x_l: wave w takes rows w, w + 4, ...
  for (int r = wave; r < who.rows; r += 4) {
    const float* xr = x + (who.row0 + r) * D;
    const float* gr = dy + (long long)(who.n0 + r / L) * D;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    #pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int c = lane + 64 * it;
      const int cc = min(c, D4 - 1);
      f32x4 xv = ap_ld4(xr + 4 * cc);
      const f32x4 gv = ap_ld4(gr + 4 * cc);
      if (c >= D4) xv = f32x4{0.f, 0.f, 0.f, 0.f};
      s0 = __builtin_fmaf(xv[0], gv[0], s0);
      s1 = __builtin_fmaf(xv[1], gv[1], s1);
      s2 = __builtin_fmaf(xv[2], gv[2], s2);
      s3 = __builtin_fmaf(xv[3], gv[3], s3);
    }
    float sum = (s0 + s1) + (s2 + s3);
    #pragma unroll
    for (int m = 1; m < 64; m <<= 1) sum += __shfl_xor(sum, m);
    if (lane == 0) dp_s[r] = sum;
  }
  const int rc = min(tid, who.rows - 1), l0 = (rc / L) * L;
  if (tid < AP_ROWS) p_s[tid] = p[who.row0 + rc];
  __syncthreads();

  if (tid < AP_ROWS) {
    float sum = 0.f;
    for (int l = 0; l < L; ++l)
      sum = __builtin_fmaf(p_s[l0 + l], dp_s[l0 + l], sum);
    const float dav = p_s[rc] * (dp_s[rc] - sum);
    da_s[tid] = dav;
    if (tid < who.rows) da[who.row0 + tid] = dav;
  }
  __syncthreads();

  // dz = da w2 (1 - e^2): to global and, as the A operand, to LDS
  const int total = who.rows * H4;
  for (int base = 0; base < total; base += AP_THREADS) {
    const int idx = min(base + tid, total - 1);
    const int r = idx / H4, c = idx - r * H4;
    const f32x4 ev = ap_ld4(e + who.row0 * Hd + 4LL * idx);
    const f32x4 wv = ap_ld4(w2 + 4 * c);
    const float dav = da_s[r];
    f32x4 z;
    #pragma unroll
    for (int q = 0; q < 4; ++q) z[q] = (dav * wv[q]) * (1.f - ev[q] * ev[q]);
    ap_st4(zs + r * RS + 4 * c, z);
    if (base + tid < total) ap_st4(dz + who.row0 * Hd + 4LL * idx, z);
  }
  __syncthreads();

  // dx = p_l dy + dz W1, 16 n-tiles of D per pass
  const int tiles = (D + 15) >> 4;
  int seq[4][4];                 // sequence of row 16 mt + 4 kq + r, clamped
  float pv[4][4];
  #pragma unroll
  for (int mt = 0; mt < 4; ++mt)
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = min(16 * mt + 4 * (lane >> 4) + r, who.rows - 1);
      seq[mt][r] = who.n0 + row / L;
      pv[mt][r] = p_s[row];
    }
  for (int pass = 0; pass < tiles; pass += 16) {
    ApLane ln;
    const int NT = ap_lane(ln, who.rows, RS, pass + wave, tiles, D);
    f32x4 acc[4][4];
    #pragma unroll
    for (int mt = 0; mt < 4; ++mt)
      #pragma unroll
      for (int t = 0; t < 4; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    ap_gemm<false>(acc, zs, ln, who.MT, NT, w1, D, Hd);
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
              const float g = dy[(long long)seq[mt][r] * D + ln.col[t]];
              const float o = __builtin_fmaf(pv[mt][r], g, acc[mt][t][r]);
              if (row < who.rows && col < D)
                dx[(who.row0 + row) * D + col] = o;
            }
          }
      }
  }
}

// Sequences per block, LDS row stride of the A operand (K floats wide) and
// LDS bytes with `extra` more floats.
struct ApPlan { int SEQ, RS, blocks; size_t lds; };

ApPlan ap_plan(int N, int L, int K, int extra) {
  ApPlan p;
  p.SEQ = AP_ROWS / L > 1 ? AP_ROWS / L : 1;
  p.RS = (K / 4) % 2 ? K : K + 4;
  p.blocks = (N + p.SEQ - 1) / p.SEQ;
  p.lds = sizeof(float) * ((size_t)p.SEQ * L * p.RS + extra);
  return p;
}

// a block may ask for more than 64 KB of dynamic LDS only after this
template <class Kern>
void ap_allow_lds(Kern kern) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024);
}

}  // namespace

extern "C" {

void launch_attn_pool_fwd(const float* x, const float* w1, const float* b1,
                          const float* w2, const float* b2, float* y,
                          float* p, float* e, int N, int L, int D, int Hd,
                          int save_e, hipStream_t s) {
  static const bool once = (ap_allow_lds(k_attn_pool_fwd<true>),
                            ap_allow_lds(k_attn_pool_fwd<false>), true);
  (void)once;
  const ApPlan pl = ap_plan(N, L, D, 7 * AP_ROWS);
  if (save_e)
    hipLaunchKernelGGL((k_attn_pool_fwd<true>), dim3(pl.blocks),
                       dim3(AP_THREADS), pl.lds, s, x, w1, b1, w2, b2, y, p,
                       e, N, L, D, Hd, pl.SEQ, pl.RS);
  else
    hipLaunchKernelGGL((k_attn_pool_fwd<false>), dim3(pl.blocks),
                       dim3(AP_THREADS), pl.lds, s, x, w1, b1, w2, b2, y, p,
                       e, N, L, D, Hd, pl.SEQ, pl.RS);
}

void launch_attn_pool_bwd(const float* x, const float* e, const float* p,
                          const float* w1, const float* w2, const float* dy,
                          float* dx, float* dz, float* da, int N, int L,
                          int D, int Hd, hipStream_t s) {
  static const bool once = (ap_allow_lds(k_attn_pool_bwd), true);
  (void)once;
  const ApPlan pl = ap_plan(N, L, Hd, 3 * AP_ROWS);
  hipLaunchKernelGGL(k_attn_pool_bwd, dim3(pl.blocks), dim3(AP_THREADS),
                     pl.lds, s, x, e, p, w1, w2, dy, dx, dz, da, N, L, D, Hd,
                     pl.SEQ, pl.RS);
}

}  // extern "C"
