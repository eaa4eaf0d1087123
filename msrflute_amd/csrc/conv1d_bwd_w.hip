// Conv1d + ReLU backward-weights over [N, T, C] rows: dW and db of the
// convolution conv1d_seq.hip computes, in its ranges (fp32, stride 1, no
// padding; 1 <= KW <= 5, KW <= T <= 64, Cin % 4 == 0 with 4 <= Cin <= 512,
// Cout % 4 == 0 with 4 <= Cout <= 512).
//
// On the flat rows r = n T + t, R = N T, Lout = T - KW + 1:
//   dz[r, c]    = dy[n, t, c] (y[n, t, c] > 0)   for t < Lout, else exactly 0
//   dW[c, e, k] = sum_r dz[r, c] x_flat[r + k, e]
//   db[c]       = sum_r dz[r, c]
// The zero rows at t >= Lout remove every cross-sequence term, and every
// r + k >= R pairs with a zero row, so a row past the end of x is staged
// from its last row (the forward's rule).  x [N, T, Cin]; y, dy
// [N, Lout, Cout]; dW [Cout, Cin, KW] (nn.Conv1d's own layout); db [Cout];
// all contiguous, 16-byte aligned bases.  The kernel reads x, y and dy as
// they are: the mask and the zero rows are applied while staging, there is
// no dz_pad and no packed weight.
//
// k_conv1d_bwd_w<KW> is a transposed-A GEMM on v_mfma_f32_16x16x4_f32:
// M = Cout, N = Cin, the reduction runs over flat rows, 4 per MFMA.  Both
// operands are read from LDS with lanes along the contiguous channels: lane
// (i = l & 15, kq = l >> 4) takes dz[r0 + kq][c0 + i] as A and
// x[r0 + kq + k][e0 + i] as B of tap k, one dword each.  Tap k's B fragment
// is the same staged x tile read k rows further down, and one A fragment
// feeds every tap and every n-tile of the wave.  So a wave owns MTW x NTW
// output tiles x KW taps, all of them in accumulators for the whole
// reduction: 4 x 4 at KW <= 3, 4 x 3 at KW = 4, 3 x 3 at KW = 5 (48, 48, 45
// accumulator tiles, one wave per SIMD).  Per 4-row step a wave issues MTW
// A reads and NTW KW B reads for MTW NTW KW MFMAs of 32 cycles each.
//
// Split of the output.  The TM = ceil(Cout / 16) m-tiles are cut into
// CM = ceil(TM / MTW) wave tiles, wave tile i owning m-tiles
// [i TM / CM, (i + 1) TM / CM) (integer division: sizes differ by at most
// one and never exceed MTW); the n-tiles likewise.  A block of 4 waves is
// WM x WN wave tiles, 2 x 2, 4 x 1 or 1 x 4: the arrangement with the
// fewest blocks, which is the fewest idle waves, and among equals the first
// of that list (2 x 2 stages the fewest columns).  At (Cout, Cin, KW) =
// (400, 300, 3): 25 x 19 tiles, 7 x 5 wave tiles, 4 x 1, 2 x 5 = 10 blocks,
// 35 of 40 waves busy.  At a row-chunk the block stages the dz columns and
// the x columns of its wave tiles once for all four waves.  A wave whose
// tile is full runs without a branch; any other wave skips its missing
// tiles by wave-uniform guards.  Columns of a partial tile compute on a
// clamped column and store nothing; tail lanes of the staging loops repeat
// the last item; guards around loads are block- or wave-uniform.
//
// Split-K.  The R rows are cut into S = ceil(R / SLAB) slabs of
// SLAB = CONV1D_BWD_W_SLAB rows (launchers.h), a compile-time constant: S
// and the order of every sum depend on the shapes only.  The grid is
// (output blocks) x S.  A slab boundary may fall inside a sequence; rows at
// or past the slab's end are staged as zero rows of dz, and x rows past it
// are read as they are (they belong to the taps of the slab's last rows).
// Within a slab the block walks chunks of 16 rows: the next chunk's global
// loads (y, dy, x) are issued before the current chunk's MFMAs and
// committed, masked, to the other LDS buffer after them; one barrier per
// chunk.  Each block writes its tile to part[S, KW, Cout, Cin]; the blocks
// of the first Cin block also sum their staged dz chunk down the rows, one
// thread per channel, into dbpart[S, Cout].  No atomics.
// k_conv1d_bwd_w_fold sums the S partials of each element and writes dW in
// [Cout, Cin, KW] and db.
//
// LDS.  Two buffers of 16 rows of dz RSA floats apart and 16 + KW - 1 rows
// of x RSB floats apart.  RS is the staged width rounded up to 16 mod 32:
// the 4 rows x 16 floats of one fragment read then start 0, 16, 32, 48 (or
// 0, 48, 32, 16) banks apart and fall on 64 distinct banks, whichever tap
// shifts them.  4 x 1 at KW = 3: 2 x (16 x 272 + 18 x 80) floats = 46 336 B;
// never above 48 KB, so no attribute is asked for.
//
// Order of every sum, a function of (element, R, SLAB) alone.  An element's
// chain runs over the slab's rows ascending, 4 per MFMA (row 4 j + kq is
// the MFMA's k index kq), from a zero accumulator; the fold adds the slabs
// ascending from the first.  db: rows ascending within the slab, slabs
// ascending.  Two calls on the same inputs are bit-equal.  dz is dy or +0, a
// select.  Built without gfx950's packed fp32 VALU ops (setup.py).

#include <hip/hip_runtime.h>

#include "launchers.h"

#define CW_THREADS 256
#define CW_CH 16
#define CW_SLAB CONV1D_BWD_W_SLAB

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ f32x4 cw_ld4(const float* p) {
  return *reinterpret_cast<const f32x4*>(p);
}
__device__ __forceinline__ void cw_st4(float* p, f32x4 v) {
  *reinterpret_cast<f32x4*>(p) = v;
}

// Register tile of a wave and the float4 items a thread stages per chunk
// at the widest arrangement (4 wave tiles across).
template <int KW>
struct CwCfg {
  static constexpr int MTW = KW <= 4 ? 4 : 3;
  static constexpr int NTW = KW <= 3 ? 4 : 3;
  static constexpr int ITA =
      (CW_CH * 16 * MTW + CW_THREADS - 1) / CW_THREADS;
  static constexpr int ITB =
      ((CW_CH + KW - 1) * 16 * NTW + CW_THREADS - 1) / CW_THREADS;
};

// Wave arrangement WM x WN, wave tiles CM x CN, blocks BM x BN, LDS strides
struct CwGeo { int WM, WN, CM, CN, BM, BN, RSA, RSB; };

// A thread's items of a chunk: LDS float offset and first global column of
// each, the (sequence, t) of the dz row and the flat row of the x row.
template <int KW>
struct CwItems {
  int alds[CwCfg<KW>::ITA], acol[CwCfg<KW>::ITA];
  int an[CwCfg<KW>::ITA], at[CwCfg<KW>::ITA];
  int blds[CwCfg<KW>::ITB], bcol[CwCfg<KW>::ITB], brow[CwCfg<KW>::ITB];
};

// One chunk in flight: y, dy and x as loaded, and which dz items are real
// rows (t < Lout, before the slab's end).
template <int KW>
struct CwStage {
  f32x4 y[CwCfg<KW>::ITA], g[CwCfg<KW>::ITA], x[CwCfg<KW>::ITB];
  unsigned ok;
};

struct CwShape { int N, T, Cin, Cout, Lout, R; };

// Issue the global loads of the items' chunk and move the items one chunk
// on (dN = CW_CH / T sequences and dT = CW_CH % T rows).
template <int KW>
__device__ __forceinline__ void cw_load(CwStage<KW>& st, CwItems<KW>& im,
                                        const float* __restrict__ x,
                                        const float* __restrict__ y,
                                        const float* __restrict__ dy,
                                        const CwShape& sh, int totA, int totB,
                                        int rend, int dN, int dT) {
  st.ok = 0;
  #pragma unroll
  for (int it = 0; it < CwCfg<KW>::ITA; ++it)
    if (it * CW_THREADS < totA) {
      const int n = im.an[it], t = im.at[it];
      if (t < sh.Lout && n * sh.T + t < rend) st.ok |= 1u << it;
      const int srow = min(n * sh.Lout + min(t, sh.Lout - 1),
                           sh.N * sh.Lout - 1);
      const long long off = (long long)srow * sh.Cout + im.acol[it];
      st.y[it] = cw_ld4(y + off);
      st.g[it] = cw_ld4(dy + off);
      const bool wrap = t + dT >= sh.T;
      im.at[it] = wrap ? t + dT - sh.T : t + dT;
      im.an[it] = n + dN + (wrap ? 1 : 0);
    }
  #pragma unroll
  for (int it = 0; it < CwCfg<KW>::ITB; ++it)
    if (it * CW_THREADS < totB) {
      const long long r = min(im.brow[it], sh.R - 1);
      st.x[it] = cw_ld4(x + r * sh.Cin + im.bcol[it]);
      im.brow[it] += CW_CH;
    }
}

// dz = dy (y > 0) on real rows, +0 elsewhere, and x, to the LDS buffer
template <int KW>
__device__ __forceinline__ void cw_commit(const CwStage<KW>& st,
                                          const CwItems<KW>& im, float* As,
                                          float* Bs, int totA, int totB) {
  #pragma unroll
  for (int it = 0; it < CwCfg<KW>::ITA; ++it)
    if (it * CW_THREADS < totA) {
      const bool ok = (st.ok >> it) & 1u;
      f32x4 z;
      #pragma unroll
      for (int q = 0; q < 4; ++q)
        z[q] = ok && st.y[it][q] > 0.f ? st.g[it][q] : 0.f;
      cw_st4(As + im.alds[it], z);
    }
  #pragma unroll
  for (int it = 0; it < CwCfg<KW>::ITB; ++it)
    if (it * CW_THREADS < totB) cw_st4(Bs + im.blds[it], st.x[it]);
}

// The CW_CH / 4 steps of one staged chunk.  ac / bc: the lane's column in
// the staged dz / x tile per m-tile / n-tile.  FULL: the wave tile has all
// MTW x NTW tiles and nothing is guarded.
template <int KW, bool FULL>
__device__ __forceinline__ void cw_chunk(
    f32x4 (&acc)[CwCfg<KW>::MTW][CwCfg<KW>::NTW][KW], const float* As,
    const float* Bs, const int (&ac)[CwCfg<KW>::MTW],
    const int (&bc)[CwCfg<KW>::NTW], int mcnt, int ncnt, int RSA, int RSB,
    int kq) {
  constexpr int MTW = CwCfg<KW>::MTW, NTW = CwCfg<KW>::NTW;
  #pragma unroll
  for (int j = 0; j < CW_CH / 4; ++j) {
    const float* a = As + (4 * j + kq) * RSA;
    const float* b = Bs + (4 * j + kq) * RSB;
    float av[MTW], bv[NTW][KW];
    #pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
      av[mt] = 0.f;
      if (FULL || mt < mcnt) av[mt] = a[ac[mt]];
    }
    #pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      #pragma unroll
      for (int k = 0; k < KW; ++k) {
        bv[nt][k] = 0.f;
        if (FULL || nt < ncnt) bv[nt][k] = b[k * RSB + bc[nt]];
      }
    }
    #pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
      if (FULL || nt < ncnt) {
        #pragma unroll
        for (int mt = 0; mt < MTW; ++mt)
          if (FULL || mt < mcnt) {
            #pragma unroll
            for (int k = 0; k < KW; ++k)
              acc[mt][nt][k] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  av[mt], bv[nt][k], acc[mt][nt][k], 0, 0, 0);
          }
      }
  }
}

// What a wave needs of its block and its tile in the slab loop: slab s,
// rows up to rend in nch chunks, the items' step (dN, dT) and counts, the
// block's first dz column and dz float4 width, and the wave's m-tiles
// [tm0, tm0 + mcnt) and n-tiles [tn0, tn0 + ncnt) (none for an idle wave).
struct CwBlk {
  int s, bn, rend, nch, dN, dT, totA, totB, cA0, wA4;
  int tm0, tn0, mcnt, ncnt;
};

// The slab loop and the store of the wave's partial tile.  FULL and the
// guarded version are two whole instantiations, so the accumulators never
// meet at a join inside the loop.
template <int KW, bool FULL>
__device__ __forceinline__ void cw_slab(
    const float* __restrict__ x, const float* __restrict__ y,
    const float* __restrict__ dy, float* __restrict__ part,
    float* __restrict__ dbpart, const CwShape& sh, const CwGeo& g,
    const CwBlk& b, CwItems<KW>& im, float* lds,
    const int (&ac)[CwCfg<KW>::MTW], const int (&bc)[CwCfg<KW>::NTW]) {
  constexpr int MTW = CwCfg<KW>::MTW, NTW = CwCfg<KW>::NTW;
  const int szA = CW_CH * g.RSA, szBuf = szA + (CW_CH + KW - 1) * g.RSB;
  const int tid = (int)threadIdx.x, i = tid & 15, kq = (tid & 63) >> 4;
  f32x4 acc[MTW][NTW][KW];
  #pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
    #pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
      #pragma unroll
      for (int k = 0; k < KW; ++k)
        acc[mt][nt][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int dbcol = min(tid, 4 * b.wA4 - 1);
  float dbacc = 0.f;

  CwStage<KW> st;
  cw_load<KW>(st, im, x, y, dy, sh, b.totA, b.totB, b.rend, b.dN, b.dT);
  cw_commit<KW>(st, im, lds, lds + szA, b.totA, b.totB);
  __syncthreads();
  for (int ch = 0; ch < b.nch; ++ch) {
    const float* As = lds + (ch & 1) * szBuf;
    float* An = lds + ((ch + 1) & 1) * szBuf;
    const bool more = ch + 1 < b.nch;
    if (more)
      cw_load<KW>(st, im, x, y, dy, sh, b.totA, b.totB, b.rend, b.dN, b.dT);
    cw_chunk<KW, FULL>(acc, As, As + szA, ac, bc, b.mcnt, b.ncnt, g.RSA,
                       g.RSB, kq);
    if (b.bn == 0) {
      #pragma unroll
      for (int r = 0; r < CW_CH; ++r) dbacc += As[r * g.RSA + dbcol];
    }
    if (more) cw_commit<KW>(st, im, An, An + szA, b.totA, b.totB);
    __syncthreads();
  }

  if (b.bn == 0 && tid < 4 * b.wA4)
    dbpart[(long long)b.s * sh.Cout + b.cA0 + tid] = dbacc;
  const long long CE = (long long)sh.Cout * sh.Cin;
  #pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
    if (FULL || mt < b.mcnt) {
      #pragma unroll
      for (int nt = 0; nt < NTW; ++nt)
        if (FULL || nt < b.ncnt) {
          const int e = 16 * (b.tn0 + nt) + i;
          #pragma unroll
          for (int k = 0; k < KW; ++k) {
            float* p = part + ((long long)b.s * KW + k) * CE + e;
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = 16 * (b.tm0 + mt) + 4 * kq + r;
              if (c < sh.Cout && e < sh.Cin)
                p[(long long)c * sh.Cin] = acc[mt][nt][k][r];
            }
          }
        }
    }
}

template <int KW>
__global__ __launch_bounds__(CW_THREADS)
void k_conv1d_bwd_w(const float* __restrict__ x, const float* __restrict__ y,
                    const float* __restrict__ dy, float* __restrict__ part,
                    float* __restrict__ dbpart, CwShape sh, CwGeo g) {
  constexpr int MTW = CwCfg<KW>::MTW, NTW = CwCfg<KW>::NTW;
  extern __shared__ float4 cw_lds4[];
  float* lds = reinterpret_cast<float*>(cw_lds4);

  const int tid = (int)threadIdx.x, i = tid & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bm = (int)blockIdx.x / g.BN;
  const int TM = (sh.Cout + 15) >> 4, TN = (sh.Cin + 15) >> 4;
  CwBlk b;
  b.bn = (int)blockIdx.x - bm * g.BN;
  b.s = (int)blockIdx.y;
  const int row0 = b.s * CW_SLAB;
  b.rend = min(sh.R, row0 + CW_SLAB);
  b.nch = (b.rend - row0 + CW_CH - 1) / CW_CH;

  // the block's staged columns: those of its wave tiles, cut at the end
  const int im0 = bm * g.WM, in0 = b.bn * g.WN;
  b.cA0 = 16 * (im0 * TM / g.CM);
  const int cA1 = min(sh.Cout, 16 * (min(g.CM, im0 + g.WM) * TM / g.CM));
  const int cB0 = 16 * (in0 * TN / g.CN);
  const int cB1 = min(sh.Cin, 16 * (min(g.CN, in0 + g.WN) * TN / g.CN));
  const int wB4 = (cB1 - cB0) >> 2;
  b.wA4 = (cA1 - b.cA0) >> 2;
  b.totA = CW_CH * b.wA4;
  b.totB = (CW_CH + KW - 1) * wB4;

  const int wm = im0 + wave / g.WN, wn = in0 + wave % g.WN;
  const bool busy = wm < g.CM && wn < g.CN;
  b.tm0 = busy ? wm * TM / g.CM : 0;
  b.tn0 = busy ? wn * TN / g.CN : 0;
  b.mcnt = busy ? (wm + 1) * TM / g.CM - b.tm0 : 0;
  b.ncnt = busy ? (wn + 1) * TN / g.CN - b.tn0 : 0;
  // the lane's column in the staged tiles, clamped into them
  int ac[MTW], bc[NTW];
  #pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
    ac[mt] = max(min(16 * (b.tm0 + mt) + i, cA1 - 1) - b.cA0, 0);
  #pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
    bc[nt] = max(min(16 * (b.tn0 + nt) + i, cB1 - 1) - cB0, 0);

  CwItems<KW> im;
  #pragma unroll
  for (int it = 0; it < CwCfg<KW>::ITA; ++it) {
    const int idx = min(it * CW_THREADS + tid, b.totA - 1);
    const int r = idx / b.wA4, c4 = idx - r * b.wA4;
    im.alds[it] = r * g.RSA + 4 * c4;
    im.acol[it] = b.cA0 + 4 * c4;
    im.an[it] = (row0 + r) / sh.T;
    im.at[it] = row0 + r - im.an[it] * sh.T;
  }
  #pragma unroll
  for (int it = 0; it < CwCfg<KW>::ITB; ++it) {
    const int idx = min(it * CW_THREADS + tid, b.totB - 1);
    const int r = idx / wB4, c4 = idx - r * wB4;
    im.blds[it] = r * g.RSB + 4 * c4;
    im.bcol[it] = cB0 + 4 * c4;
    im.brow[it] = row0 + r;
  }
  b.dN = CW_CH / sh.T;
  b.dT = CW_CH - b.dN * sh.T;

  if (b.mcnt == MTW && b.ncnt == NTW)
    cw_slab<KW, true>(x, y, dy, part, dbpart, sh, g, b, im, lds, ac, bc);
  else
    cw_slab<KW, false>(x, y, dy, part, dbpart, sh, g, b, im, lds, ac, bc);
}

// dW[c, e, k] = sum_s part[s, k, c, e] and db[c] = sum_s dbpart[s, c], s
// ascending.  One thread per (c, e), which writes its KW taps side by side;
// the blocks after those, one thread per c.
__global__ __launch_bounds__(CW_THREADS)
void k_conv1d_bwd_w_fold(const float* __restrict__ part,
                         const float* __restrict__ dbpart,
                         float* __restrict__ dW, float* __restrict__ db,
                         int S, int KW, int Cout, int Cin, int wblocks) {
  const int CE = Cout * Cin;
  if ((int)blockIdx.x < wblocks) {
    const int idx = (int)blockIdx.x * CW_THREADS + (int)threadIdx.x;
    if (idx >= CE) return;
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const float* p = part + idx;
    #pragma unroll 4
    for (int s = 0; s < S; ++s) {
      #pragma unroll
      for (int k = 0; k < 5; ++k)
        if (k < KW) acc[k] += p[((long long)s * KW + k) * CE];
    }
    #pragma unroll
    for (int k = 0; k < 5; ++k)
      if (k < KW) dW[(long long)idx * KW + k] = acc[k];
  } else {
    const int c = ((int)blockIdx.x - wblocks) * CW_THREADS + (int)threadIdx.x;
    if (c >= Cout) return;
    float acc = 0.f;
    #pragma unroll 4
    for (int s = 0; s < S; ++s) acc += dbpart[(long long)s * Cout + c];
    db[c] = acc;
  }
}

// smallest stride >= w (a multiple of 16) that is 16 mod 32
int cw_rs(int w) { return (w + 15) / 32 * 32 + 16; }

CwGeo cw_geo(int Cin, int Cout, int MTW, int NTW) {
  static const int arr[3][2] = {{2, 2}, {4, 1}, {1, 4}};
  const int TM = (Cout + 15) / 16, TN = (Cin + 15) / 16;
  CwGeo g;
  g.CM = (TM + MTW - 1) / MTW;
  g.CN = (TN + NTW - 1) / NTW;
  int best = -1;
  for (const auto& a : arr) {
    const int BM = (g.CM + a[0] - 1) / a[0], BN = (g.CN + a[1] - 1) / a[1];
    if (best < 0 || BM * BN < best) {
      best = BM * BN;
      g.WM = a[0]; g.WN = a[1]; g.BM = BM; g.BN = BN;
    }
  }
  g.RSA = cw_rs(16 * MTW * g.WM);
  g.RSB = cw_rs(16 * NTW * g.WN);
  return g;
}

template <int KW>
void cw_launch(const float* x, const float* y, const float* dy, float* part,
               float* dbpart, const CwShape& sh, int S, hipStream_t s) {
  const CwGeo g = cw_geo(sh.Cin, sh.Cout, CwCfg<KW>::MTW, CwCfg<KW>::NTW);
  const size_t lds = sizeof(float) * 2 *
      (size_t)(CW_CH * g.RSA + (CW_CH + KW - 1) * g.RSB);
  hipLaunchKernelGGL((k_conv1d_bwd_w<KW>), dim3(g.BM * g.BN, S),
                     dim3(CW_THREADS), lds, s, x, y, dy, part, dbpart, sh, g);
}

}  // namespace

extern "C" {

void launch_conv1d_bwd_w(const float* x, const float* y, const float* dy,
                         float* part, float* dbpart, float* dW, float* db,
                         int N, int T, int Cin, int Cout, int KW,
                         hipStream_t s) {
  const CwShape sh = {N, T, Cin, Cout, T - KW + 1, N * T};
  const int S = (int)conv1d_bwd_w_slabs(N, T);
  switch (KW) {
    case 1: cw_launch<1>(x, y, dy, part, dbpart, sh, S, s); break;
    case 2: cw_launch<2>(x, y, dy, part, dbpart, sh, S, s); break;
    case 3: cw_launch<3>(x, y, dy, part, dbpart, sh, S, s); break;
    case 4: cw_launch<4>(x, y, dy, part, dbpart, sh, S, s); break;
    default: cw_launch<5>(x, y, dy, part, dbpart, sh, S, s); break;
  }
  const int wblocks = (Cout * Cin + CW_THREADS - 1) / CW_THREADS;
  const int bblocks = (Cout + CW_THREADS - 1) / CW_THREADS;
  hipLaunchKernelGGL(k_conv1d_bwd_w_fold, dim3(wblocks + bblocks),
                     dim3(CW_THREADS), 0, s, part, dbpart, dW, db, S, KW,
                     Cout, Cin, wblocks);
}

}  // extern "C"
