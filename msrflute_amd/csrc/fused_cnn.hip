// Fully-fused CNN-FEMNIST client step for gfx950.  The flagship
// benchmark model (experiments/cv_cnn_femnist/model.py: conv1 1->32 3x3,
// relu, conv2 32->64 3x3, relu, maxpool2, dropout .25, fc1 9216->128,
// relu, dropout .5, fc2 128->C, CE) trained WITHOUT torch autograd:
// forward, backward, clip+stats and the SGD step are ~20 kernel launches
// per batch driven by one host call.  Gradients are written (not
// accumulated) straight into the flat arena at the parameters' fixed
// offsets, so no zero_grad is needed either.  Shapes are the task's
// (28x28 in, spatial 26/24/12 fixed); batch size and class count C are
// runtime args.
//
// ONE kernel set serves both drivers.  Every kernel is written for the
// cross-client mega round (launch_cnn_round_mega): ONE launch set per
// batch-step trains ALL K sampled clients, the super-batch dimension is
// G = K*bs rows (row g belongs to client k = g/bs), every kernel takes
// per-client parameter/gradient stacks (params_stack[k*P ..]), and grids
// scale by K — conv2 fwd is K*bs*6 = 1200 blocks at the benchmark shape,
// where a per-client grid (120 blocks) underfills the 256-CU chip.  The
// per-client epoch (launch_cnn_epoch) launches the same kernels at K = 1
// with bs := the batch's actual row count and the client's own arena as
// the stack.  Both drivers issue a batch-step through ONE host function,
// cnn_step.  The ops that read per-client metadata (gather, the conv2
// forward's pool/dropout epilogue, the bf16 path's pool dropout, fc1
// reduce, loss) are templates over a by-value step-metadata argument:
// StepMetaDev (mega round) points at the seeds[k]/counts[k] device arrays,
// StepMetaOne (K = 1) carries the same facts as launch scalars, so that
// path uploads nothing.
//
// Ragged handling is free of masks in the backward chain: the gather
// zero-fills inactive rows (b >= B_k(t)) and writes yb = -1, the loss
// kernel zeroes those rows' dlogits, and every weight gradient is then
// exactly the per-client value (zero rows contribute nothing).  Clients
// whose epochs ended (t >= ceil(count/bs)) naturally produce zero
// gradients and their SGD step no-ops.  Dropout Philox streams use
// CLIENT-LOCAL indices keyed by (seed, batch index), so masks are
// bit-identical between the two drivers and deterministic per client
// epoch.

#include <hip/hip_runtime.h>
#include <hiprand/hiprand_kernel.h>

#include <cstdio>
#include <cstdlib>

#include "launchers.h"

#define FBLK 256

// gfx950's f32-input MFMA (v_mfma_f32_16x16x4_f32) is EXACT f32 — a
// k-ordered fmaf chain at the full f32 rate — so the f32 GEMM kernels
// keep fp32 numerics while moving the matrix work onto the matrix pipe.
// Fragment maps: A[i=l&15][k=l>>4], B[k=l>>4][j=l&15] one f32 VGPR each;
// D[row=(l>>4)*4+r][col=l&15], 4 f32 per lane.
typedef __attribute__((ext_vector_type(4))) float f32x4;

// per-row helpers: g in [0, K*bs), k = g / bs, b = g % bs
__device__ __forceinline__ int mega_Bk(const long long* counts, int k,
                                       int t, int bs) {
  long long rem = counts[k] - (long long)t * bs;
  return rem <= 0 ? 0 : (rem < bs ? (int)rem : bs);
}

// Who is in this batch-step, passed by value to the kernels that read
// per-client metadata (they are templates over the form).  Two forms with
// the same accessors: the mega round's points at the [K] device arrays and
// carries the step index t; the per-client epoch's (K = 1) carries the same
// facts as launch scalars, so that path uploads nothing.  The form is a
// type, so no accessor costs a select at run time.
struct StepMetaDev {
  const long long* row_bases;
  const long long* order_offs;
  const long long* counts;
  const long long* seeds;
  int t;
  static constexpr bool DEV = true;
  static constexpr unsigned long long seed = 0;  // unused in this form
  // rows of client k at this step
  __device__ __forceinline__ int rows(int k, int bs) const {
    return mega_Bk(counts, k, t, bs);
  }
  __device__ __forceinline__ unsigned long long seed_of(int k) const {
    return (unsigned long long)seeds[k];
  }
  // shard row that batch row b of client k gathers
  __device__ __forceinline__ long long src_row(
      const long long* __restrict__ orders, int k, int b, int bs) const {
    return row_bases[k] + orders[order_offs[k] + (long long)t * bs + b];
  }
};
struct StepMetaOne {
  long long row_base, start;  // shard row offset; batch start in `orders`
  int B;                      // rows of this batch
  unsigned long long seed;
  static constexpr bool DEV = false;
  static constexpr const long long* seeds = nullptr;  // unused in this form
  __device__ __forceinline__ int rows(int, int) const { return B; }
  __device__ __forceinline__ unsigned long long seed_of(int) const {
    return seed;
  }
  __device__ __forceinline__ long long src_row(
      const long long* __restrict__ orders, int, int b, int) const {
    return row_base + orders[start + b];
  }
};

__global__ void k_copy_stack(float* __restrict__ dst,
                             const float* __restrict__ src, long long P,
                             int K) {
  long long total = (long long)K * P;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x)
    dst[i] = src[i % P];
}

// per-client round plumbing (launch_cnn_round): copy-in, weighted
// pseudo-gradient grad = (w_server - w_trained) * weight, accumulate
__global__ void k_copy(float* __restrict__ dst, const float* __restrict__ src,
                       long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    dst[i] = src[i];
}

__global__ void k_cnn_pseudo_grad(float* __restrict__ g,
                                  const float* __restrict__ ws,
                                  const float* __restrict__ wt, float weight,
                                  long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    g[i] = (ws[i] - wt[i]) * weight;
}

__global__ void k_cnn_axpy(float* __restrict__ y, const float* __restrict__ x,
                           long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    y[i] += x[i];
}

// ---------------------------------------------------------------------------
// gather a shuffled batch from the device-resident shard: element j of
// batch row g comes from shard row src
// ---------------------------------------------------------------------------
template <typename Meta>
__global__ void k_gather_mb(const float* __restrict__ shard_x,
                            const long long* __restrict__ shard_y,
                            const long long* __restrict__ orders,
                            Meta meta, int bs, int K,
                            float* __restrict__ xb, int* __restrict__ yb,
                            double* __restrict__ acc2k, int n_acc) {
  int G = K * bs;
  // first kernel of a batch-step: zero the clip's sum / sumsq slots (2 per
  // client; 3 under FedProx) — their last reader, the previous step's clip
  // kernel, precedes this kernel in stream order
  if (blockIdx.x == 0)
    for (int q = threadIdx.x; q < n_acc; q += blockDim.x) acc2k[q] = 0.0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < (long long)G * 784; i += (long long)gridDim.x * blockDim.x) {
    int g = (int)(i / 784), j = (int)(i % 784);
    int k = g / bs, b = g % bs;
    if (b < meta.rows(k, bs)) {
      long long src = meta.src_row(orders, k, b, bs);
      xb[i] = shard_x[src * 784 + j];
      if (j == 0) yb[g] = (int)shard_y[src];
    } else {
      xb[i] = 0.f;
      if (j == 0) yb[g] = -1;
    }
  }
}

__global__ void k_conv1_fwd_mb(const float* __restrict__ x,
                               const float* __restrict__ params, long long P,
                               long long ow1, long long ob1, int bs, int K,
                               float* __restrict__ a1) {
  long long total = (long long)K * bs * 21632;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    int xx = (int)(i % 26), yy = (int)((i / 26) % 26);
    int co = (int)((i / 676) % 32);
    long long g = i / 21632;
    int k = (int)(g / bs);
    const float* w1 = params + (long long)k * P + ow1;
    const float* b1 = params + (long long)k * P + ob1;
    const float* xp = x + g * 784 + yy * 28 + xx;
    const float* wp = w1 + co * 9;
    float acc = b1[co];
    #pragma unroll
    for (int kh = 0; kh < 3; ++kh)
      #pragma unroll
      for (int kw = 0; kw < 3; ++kw)
        acc = fmaf(wp[kh * 3 + kw], xp[kh * 28 + kw], acc);
    a1[i] = acc > 0.f ? acc : 0.f;
  }
}

__global__ void k_w2_layouts_mb(const float* __restrict__ params,
                                long long P, long long ow2, int K,
                                float* __restrict__ w2t_stack,
                                float* __restrict__ w2rot_stack) {
  long long total = (long long)K * 18432;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    int k = (int)(i / 18432), r = (int)(i % 18432);
    int co = r / 288, kk = r % 288;
    float v = params[(long long)k * P + ow2 + r];
    w2t_stack[(long long)k * 18432 + kk * 64 + co] = v;
    int rem = kk % 9;
    w2rot_stack[(long long)k * 18432 + ((long long)co * 9 + rem) * 32
                + kk / 9] = v;
  }
}

// Lane constants of the (channel, kh, kw) k-decomposition shared by the
// conv2 forward and backward-data implicit GEMMs.  The k index of lane
// group kc in MFMA step s is 4s + kc and decomposes with period 9, so
// over 36 k (9 steps, 4 channels) step j touches channel (4j+kc)/9 and
// tap (4j+kc)%9: nine loop-invariant LDS offsets per lane, and the
// k-loop only adds a 4-channel stride.  cs = staged channel stride,
// tap = signed (kh, kw) step of the staged image (row stride rs).
__device__ __forceinline__ void conv2_tap_offsets(int kc, int cs, int rs,
                                                  int sgn, int off[9]) {
  #pragma unroll
  for (int j = 0; j < 9; ++j) {
    int q = 4 * j + kc, c = q / 9, rem = q % 9;
    off[j] = c * cs + sgn * ((rem / 3) * rs + rem % 3);
  }
}

// conv2 forward (f32 MFMA), implicit GEMM straight from raw activations.
// grid = G * C2F_SLABS; a block owns a slab of CONV2_FWD_SLAB_ROWS output
// rows (96 positions x 64 co) of one image and stages only the rows+2
// input rows of each ci it needs (19.5 KB, one 624 B run per plane), so
// an image's a1 is filled ~1.5x instead of 9x.  Wave w owns a 3 x 2 block
// of 16x16 accumulators (m-tiles 3*(w>>1).., co half w&1): each W2
// fragment (one global load per k-step from w2t) feeds 3 MFMAs, each a1
// fragment 2, and consecutive MFMAs are independent.  Every output's k
// order is (ci,kh,kw) ascending from 0, bias and ReLU after, as before.
#define C2F_ROWS CONV2_FWD_SLAB_ROWS
#define C2F_SLABS (24 / C2F_ROWS)
#define C2F_CS ((C2F_ROWS + 2) * 26)  /* staged floats per ci plane */
static_assert(24 % C2F_ROWS == 0 && (C2F_ROWS * 24) % 96 == 0 &&
              C2F_CS % 4 == 0 && C2F_CS / 4 <= 64,
              "conv2 fwd slab: 6 m-tiles per block, float4 plane copies");
// POOL = false stores r2 (bias + ReLU).  POOL = true never writes r2: it
// finishes with maxpool 2x2 + dropout(p1) and writes a2 / pidx / m2.  The
// mapping of an MFMA row to an output position only enters through
// base[i] (no output's k-chain depends on it), so POOL maps row
// il = 4q + e of m-tile i to window element e of pool cell px = 4i + q of
// the wave's pool row: wave mh = w >> 1 owns slab rows 2mh, 2mh + 1, and
// the D fragment of lane (il, kc) is then acc[i][n][0..3] = the 2x2 window
// of cell px = 4i + kc of channel co = il.. in pool_drop_cell's order
// (base[0], base[1], base[24], base[25]): bias, ReLU and the strict->
// argmax are in-register.  The cells then go through the (dead) staging
// LDS so that the Philox draw runs in a rolled loop behind the
// accumulators and consecutive lanes store consecutive cells.
static_assert(C2F_ROWS == 4 && 2 * 64 * 24 <= 32 * C2F_CS,
              "POOL epilogue: waves 2mh, 2mh+1 own pool row mh of the slab; "
              "the cell image fits the staging LDS");
template <bool POOL>
__device__ __forceinline__ void conv2_fwd_body(
    const float* __restrict__ a1, const float* __restrict__ w2t_stack,
    const float* __restrict__ params, long long P, long long ob2, int bs,
    float* __restrict__ r2, float p1, unsigned long long seed,
    unsigned long long offset, float* __restrict__ a2,
    unsigned char* __restrict__ pidx, unsigned char* __restrict__ m2) {
  __shared__ __attribute__((aligned(16))) float lds[32 * C2F_CS];
  long long g = blockIdx.x / C2F_SLABS;
  int sl = blockIdx.x % C2F_SLABS;
  int k = (int)(g / bs);
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // wave w copies planes w, w+4, ..: lanes 0..38 move one float4 each
  const float4* src = reinterpret_cast<const float4*>(
      a1 + g * 21632 + sl * (C2F_ROWS * 26));
  if (lane < C2F_CS / 4)
    for (int ci = w; ci < 32; ci += 4)
      reinterpret_cast<float4*>(lds)[ci * (C2F_CS / 4) + lane] =
          src[ci * 169 + lane];
  __syncthreads();
  int il = lane & 15, kc = lane >> 4;
  int nh = w & 1, mh = w >> 1;
  int off[9], base[3];
  conv2_tap_offsets(kc, C2F_CS, 26, 1, off);
  #pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (POOL) {
      int q = il >> 2, e = il & 3;
      base[i] = (2 * mh + (e >> 1)) * 26 + 2 * (4 * i + q) + (e & 1);
    } else {
      int m = (mh * 3 + i) * 16 + il;
      base[i] = (m / 24) * 26 + m % 24;
    }
  }
  const float* wp = w2t_stack + (long long)k * 18432 + kc * 64 + nh * 32 + il;
  f32x4 acc[3][2];
  #pragma unroll
  for (int i = 0; i < 3; ++i)
    acc[i][0] = acc[i][1] = f32x4{0, 0, 0, 0};
  for (int t = 0; t < 8; ++t) {
    const float* lt = lds + t * 4 * C2F_CS;
    const float* wt = wp + t * 36 * 64;
    #pragma unroll
    for (int j = 0; j < 9; ++j) {
      float b0 = wt[j * 256], b1 = wt[j * 256 + 16];
      #pragma unroll
      for (int i = 0; i < 3; ++i) {
        float a = lt[base[i] + off[j]];
        acc[i][0] =
            __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[i][0], 0, 0, 0);
        acc[i][1] =
            __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[i][1], 0, 0, 0);
      }
    }
  }
  const float* b2 = params + (long long)k * P + ob2;
  if (!POOL) {
    #pragma unroll
    for (int n = 0; n < 2; ++n) {
      int co = nh * 32 + n * 16 + il;
      float bias = b2[co];
      #pragma unroll
      for (int i = 0; i < 3; ++i) {
        int om = sl * (C2F_ROWS * 24) + (mh * 3 + i) * 16 + kc * 4;
        float4 v;
        v.x = acc[i][n][0] + bias; v.y = acc[i][n][1] + bias;
        v.z = acc[i][n][2] + bias; v.w = acc[i][n][3] + bias;
        v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f;
        v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
        *reinterpret_cast<float4*>(r2 + (g * 64 + co) * 576 + om) = v;
      }
    }
    return;
  }
  // phase 1: the block's 64 co x 24 cells (2 pool rows x 12) as max and
  // argmax | gate << 2, in [co][24] order, over the staged a1
  float* cmax = lds;
  int* cidx = reinterpret_cast<int*>(lds + 64 * 24);
  __syncthreads();
  #pragma unroll
  for (int n = 0; n < 2; ++n) {
    int co = nh * 32 + n * 16 + il;
    float bias = b2[co];
    #pragma unroll
    for (int i = 0; i < 3; ++i) {
      float v0 = acc[i][n][0] + bias, v1 = acc[i][n][1] + bias;
      float v2 = acc[i][n][2] + bias, v3 = acc[i][n][3] + bias;
      v0 = v0 > 0.f ? v0 : 0.f; v1 = v1 > 0.f ? v1 : 0.f;
      v2 = v2 > 0.f ? v2 : 0.f; v3 = v3 > 0.f ? v3 : 0.f;
      float m = v0; int idx = 0;
      if (v1 > m) { m = v1; idx = 1; }
      if (v2 > m) { m = v2; idx = 2; }
      if (v3 > m) { m = v3; idx = 3; }
      int c = co * 24 + mh * 12 + 4 * i + kc;
      cmax[c] = m;
      cidx[c] = idx | (m > 0.f ? 4 : 0);
    }
  }
  __syncthreads();
  // phase 2: thread j takes cells j, j + 256, ..; the 24 cells of a co are
  // one 96 B run of a2 (24 B of pidx / m2) at cell sl * 24 of its plane
  float inv_keep = (p1 < 1.f) ? 1.f / (1.f - p1) : 0.f;
  int b = (int)(g % bs);
  #pragma unroll 1
  for (int c = threadIdx.x; c < 64 * 24; c += 256) {
    int co = c / 24, rem = c % 24;
    int lc = co * 144 + sl * 24 + rem;   // cell within the image
    long long i = g * 9216 + lc;
    int li = b * 9216 + lc;              // client-local: the Philox key
    float m = cmax[c];
    unsigned char keep = 1;
    if (p1 > 0.f) {
      hiprandStatePhilox4_32_10_t st;
      hiprand_init(seed, (unsigned long long)(li >> 2), offset, &st);
      float4 u = hiprand_uniform4(&st);
      float uu = (li & 3) == 0 ? u.x : (li & 3) == 1 ? u.y
                 : (li & 3) == 2 ? u.z : u.w;
      keep = uu >= p1;
    }
    pidx[i] = (unsigned char)cidx[c];
    m2[i] = keep;
    a2[i] = keep ? m * inv_keep : 0.f;
  }
}

__global__ __launch_bounds__(256)
void k_conv2_fwd_mfma_mb(const float* __restrict__ a1,
                         const float* __restrict__ w2t_stack,
                         const float* __restrict__ params, long long P,
                         long long ob2, int bs, int K,
                         float* __restrict__ r2) {
  conv2_fwd_body<false>(a1, w2t_stack, params, P, ob2, bs, r2, 0.f, 0ull,
                        0ull, nullptr, nullptr, nullptr);
}

// the POOL form: client k draws from meta's seed
template <typename Meta>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(5, 5)))
void k_conv2_fwd_pool_mfma_mb(const float* __restrict__ a1,
                              const float* __restrict__ w2t_stack,
                              const float* __restrict__ params, long long P,
                              long long ob2, int bs, int K, float p1,
                              Meta meta, unsigned long long offset,
                              float* __restrict__ a2,
                              unsigned char* __restrict__ pidx,
                              unsigned char* __restrict__ m2) {
  int k = (int)(blockIdx.x / C2F_SLABS / bs);
  conv2_fwd_body<true>(a1, w2t_stack, params, P, ob2, bs, nullptr, p1,
                       meta.seed_of(k), offset, a2, pidx, m2);
}

// maxpool 2x2 + dropout(p1) of pool cell i, whose 2x2 window starts at
// `base`: a2 = keep ? max/(1-p1) : 0; save argmax (bits 0-1 of pidx), the
// ReLU gate max > 0 (bit 2: all the backward needs of r2) + mask.  The Philox
// key is (seed, li >> 2, batch offset) with li the CLIENT-LOCAL cell
// index, so a client's masks do not depend on which driver or which
// stack slot trains it.
__device__ __forceinline__ void pool_drop_cell(
    const float* __restrict__ base, long long i, long long li, float p1,
    float inv_keep, unsigned long long seed, unsigned long long offset,
    float* __restrict__ a2, unsigned char* __restrict__ pidx,
    unsigned char* __restrict__ m2) {
  float v0 = base[0], v1 = base[1], v2 = base[24], v3 = base[25];
  float m = v0; int idx = 0;
  if (v1 > m) { m = v1; idx = 1; }
  if (v2 > m) { m = v2; idx = 2; }
  if (v3 > m) { m = v3; idx = 3; }
  unsigned char keep = 1;
  if (p1 > 0.f) {
    // one Philox draw covers 4 cells (init is ~10 rounds — the cost)
    hiprandStatePhilox4_32_10_t st;
    hiprand_init(seed, (unsigned long long)(li >> 2), offset, &st);
    float4 u = hiprand_uniform4(&st);
    float uu = (li & 3) == 0 ? u.x : (li & 3) == 1 ? u.y
               : (li & 3) == 2 ? u.z : u.w;
    keep = uu >= p1;
  }
  pidx[i] = (unsigned char)(idx | (m > 0.f ? 4 : 0));
  m2[i] = keep;
  a2[i] = keep ? m * inv_keep : 0.f;
}

template <typename Meta>
__global__ void k_pool_drop_fwd_mb(const float* __restrict__ r2, int bs,
                                   int K, float p1, Meta meta,
                                   unsigned long long offset,
                                   float* __restrict__ a2,
                                   unsigned char* __restrict__ pidx,
                                   unsigned char* __restrict__ m2) {
  long long total = (long long)K * bs * 9216;
  float inv_keep = (p1 < 1.f) ? 1.f / (1.f - p1) : 0.f;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    int px = (int)(i % 12), py = (int)((i / 12) % 12);
    int c = (int)((i / 144) % 64);
    long long g = i / 9216;
    int k = (int)(g / bs), b = (int)(g % bs);
    const float* base = r2 + ((g * 64 + c) * 24 + 2 * py) * 24 + 2 * px;
    long long li = (long long)b * 9216 + (i % 9216);
    pool_drop_cell(base, i, li, p1, inv_keep, meta.seed_of(k), offset, a2,
                   pidx, m2);
  }
}

// widest vector (in floats) that an access at byte address `a` and at any
// multiple of 16 B past it may use.  The per-client stacks put client k at
// k*P floats, and P need not be a multiple of 4 (P*4 mod 16 = 8 at C = 62),
// so the fc1 kernels pick their global access width per block from the
// actual addresses: 16 B, two 8 B halves, or dwords.
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ int addr_vec(unsigned long long a) {
  return (a & 15) == 0 ? 4 : ((a & 7) == 0 ? 2 : 1);
}
template <int VEC>
__device__ __forceinline__ void ld_vec(const float* __restrict__ p,
                                       float* v) {
  if (VEC == 4) {
    f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else if (VEC == 2) {
    f32x2 t = *reinterpret_cast<const f32x2*>(p);
    v[0] = t[0]; v[1] = t[1];
  } else {
    v[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void st_vec(float* __restrict__ p,
                                       const float* v) {
  if (VEC == 4)
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  else if (VEC == 2)
    *reinterpret_cast<f32x2*>(p) = f32x2{v[0], v[1]};
  else
    p[0] = v[0];
}

// fc1 forward as split-K MFMA GEMM: z3^T[j,b] = sum_k W3[j,k]*a2[b,k],
// M=128 (j), N=32 (b, masked to bs), K=9216 split into FC1_SPLIT chunks;
// per-chunk partials land in the slab and k_fc1_fwd_reduce* folds them.
// grid = K * FC1_SPLIT blocks.  A block walks its 144-k chunk in three
// 48-k sub-chunks: the next sub-chunk's global loads (VEC floats each)
// are issued into registers before the current sub-chunk's MFMAs, and
// the 31.25 KB LDS image lets five blocks share a CU, so all K * 64
// blocks are co-resident and one block's fill overlaps another's math.
// Every partial is still one k-ordered MFMA chain over its 144 k.
#define FC1_SPLIT 64
#define FC1_CH (9216 / FC1_SPLIT)  /* 144 k per chunk */
#define FC1_SUB 48                 /* k per LDS sub-chunk */
#define FC1_LD (FC1_SUB + 2)       /* LDS row stride 50 = 18 mod 32: the 32
                                      lanes of a ds_read_b32 group (16 rows x
                                      2 k) hit 32 distinct banks */
template <int VEC>
__device__ __forceinline__ void fc1_fwd_body(
    const float* __restrict__ w3, const float* __restrict__ a2k, int bs,
    int k_base, float* lw, float* la, f32x4 (&acc)[2][2]) {
  constexpr int PER_ROW = FC1_SUB / VEC;          // items per row
  constexpr int NW = 128 * PER_ROW / 256;         // W items per thread
  constexpr int A_ITEMS = 32 * PER_ROW;
  constexpr int NA = (A_ITEMS + 255) / 256;       // a2 items per thread
  float rw[NW][VEC], ra[NA][VEC];
  auto fetch = [&](int sub) {
    int kb = k_base + sub * FC1_SUB;
    #pragma unroll
    for (int n = 0; n < NW; ++n) {
      int i = threadIdx.x + n * 256;
      int row = i / PER_ROW, c = i % PER_ROW;
      ld_vec<VEC>(w3 + (row * 9216 + kb + c * VEC), rw[n]);
    }
    #pragma unroll
    for (int n = 0; n < NA; ++n) {
      int i = threadIdx.x + n * 256;
      int bu = i / PER_ROW, c = i % PER_ROW;
      #pragma unroll
      for (int e = 0; e < VEC; ++e) ra[n][e] = 0.f;
      if (i < A_ITEMS && bu < bs)
        ld_vec<VEC>(a2k + (bu * 9216 + kb + c * VEC), ra[n]);
    }
  };
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int kc = lane >> 4, il = lane & 15;
  fetch(0);
  #pragma unroll 1
  for (int sub = 0; sub < FC1_CH / FC1_SUB; ++sub) {
    #pragma unroll
    for (int n = 0; n < NW; ++n) {
      int i = threadIdx.x + n * 256;
      int row = i / PER_ROW, c = i % PER_ROW;
      #pragma unroll
      for (int e = 0; e < VEC; ++e)
        lw[row * FC1_LD + c * VEC + e] = rw[n][e];
    }
    #pragma unroll
    for (int n = 0; n < NA; ++n) {
      int i = threadIdx.x + n * 256;
      int bu = i / PER_ROW, c = i % PER_ROW;
      if (i < A_ITEMS) {
        #pragma unroll
        for (int e = 0; e < VEC; ++e)
          la[bu * FC1_LD + c * VEC + e] = ra[n][e];
      }
    }
    __syncthreads();
    if (sub + 1 < FC1_CH / FC1_SUB) fetch(sub + 1);
    #pragma unroll 6
    for (int k0 = 0; k0 < FC1_SUB; k0 += 4) {
      int kk = k0 + kc;
      float a0 = lw[(w * 32 + il) * FC1_LD + kk];
      float a1v = lw[(w * 32 + 16 + il) * FC1_LD + kk];
      #pragma unroll
      for (int u = 0; u < 2; ++u) {
        float bv = la[(u * 16 + il) * FC1_LD + kk];
        acc[0][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][u], 0, 0, 0);
        acc[1][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v, bv, acc[1][u], 0, 0, 0);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256, 3)  // 3 blocks/CU: K*64 = 640 co-resident
void k_fc1_fwd_mfma_mb(const float* __restrict__ a2,
                       const float* __restrict__ params, long long P,
                       long long ow3, int bs, int K,
                       float* __restrict__ slab) {
  __shared__ float lw[128 * FC1_LD];
  __shared__ float la[32 * FC1_LD];
  int k = blockIdx.x / FC1_SPLIT;
  int s = blockIdx.x % FC1_SPLIT;
  int k_base = s * FC1_CH;
  const float* w3 = params + (long long)k * P + ow3;
  const float* a2k = a2 + (long long)k * bs * 9216;
  f32x4 acc[2][2] = {{f32x4{0,0,0,0}, f32x4{0,0,0,0}},
                     {f32x4{0,0,0,0}, f32x4{0,0,0,0}}};
  int vec = addr_vec((unsigned long long)w3 | (unsigned long long)a2k);
  if (vec == 4) fc1_fwd_body<4>(w3, a2k, bs, k_base, lw, la, acc);
  else if (vec == 2) fc1_fwd_body<2>(w3, a2k, bs, k_base, lw, la, acc);
  else fc1_fwd_body<1>(w3, a2k, bs, k_base, lw, la, acc);
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int il = lane & 15;
  float* slk = slab + (long long)k * FC1_SPLIT * bs * 128;
  #pragma unroll
  for (int tt = 0; tt < 2; ++tt)
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      int bu = u * 16 + il;
      if (bu >= bs) continue;
      int j = w * 32 + tt * 16 + (lane >> 4) * 4;
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        slk[((long long)s * bs + bu) * 128 + j + r] = acc[tt][u][r];
    }
}

// fold one client's SPLIT split-K partials for (row b, unit j) in fixed
// order (deterministic — no atomics) + bias + relu + dropout(p2) into
// element i of z3/a3/m3.  Philox key: (seed ^ golden ratio, li, batch
// offset) with li = b*128 + j the CLIENT-LOCAL element index.
// The fold wrappers launch FC1R_BLK-thread blocks.  Measured at the
// benchmark shape (25,600 outputs): 256-thread blocks 11 us, 128 17 us,
// 64 18 us — spreading the fold over more CUs is slower, so the block
// stays at 256; the launch bound keeps the Philox state's LDS image small.
#define FC1R_BLK 256
#define FC1R_BATCH 64
template <int SPLIT>
__device__ __forceinline__ void fc1_reduce_elem(
    const float* __restrict__ slk, float bias, int bs, int b, int j,
    long long i, long long li, float p2, unsigned long long seed,
    unsigned long long offset, float* __restrict__ z3,
    float* __restrict__ a3, unsigned char* __restrict__ m3) {
  // the loads of a batch of FC1R_BATCH partials are issued before its
  // first add (one round trip per batch, not one per partial); the adds
  // run in the fixed order s = 0, 1, …
  float t = bias;
  #pragma unroll
  for (int s0 = 0; s0 < SPLIT; s0 += FC1R_BATCH) {
    float v[FC1R_BATCH];
    #pragma unroll
    for (int n = 0; n < FC1R_BATCH; ++n)
      if (s0 + n < SPLIT)
        v[n] = slk[((long long)(s0 + n) * bs + b) * 128 + j];
    #pragma unroll
    for (int n = 0; n < FC1R_BATCH; ++n)
      if (s0 + n < SPLIT) t += v[n];
  }
  z3[i] = t;
  float r = t > 0.f ? t : 0.f;
  unsigned char keep = 1;
  if (p2 > 0.f) {
    hiprandStatePhilox4_32_10_t st;
    hiprand_init(seed ^ 0x9e3779b97f4a7c15ull, (unsigned long long)li,
                 offset, &st);
    keep = hiprand_uniform(&st) >= p2;
  }
  m3[i] = keep;
  a3[i] = keep ? r / (1.f - p2) : 0.f;
}

// DEV = StepMetaDev's form: seeds[k]; else the one `seed`.  The two fold
// kernels take the pair as plain arguments, not as a metadata struct: the
// fold's register budget is tight, and with the seeds pointer inside a
// by-value struct (no longer a restrict kernel argument) the fp32 fold went
// from 96 to 97 VGPRs and lost a wave, the bf16 fold from 58 to 105.
template <int SPLIT, bool DEV>
__device__ __forceinline__ void fc1_reduce_stack(
    const float* __restrict__ slab, const float* __restrict__ params,
    long long P, long long ob3, int bs, int K, float p2,
    const long long* __restrict__ seeds, unsigned long long seed,
    unsigned long long offset, float* __restrict__ z3,
    float* __restrict__ a3, unsigned char* __restrict__ m3) {
  long long total = (long long)K * bs * 128;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    long long g = i / 128;
    int j = (int)(i % 128);
    int k = (int)(g / bs), b = (int)(g % bs);
    fc1_reduce_elem<SPLIT>(slab + (long long)k * SPLIT * bs * 128,
                           params[(long long)k * P + ob3 + j], bs, b, j, i,
                           (long long)b * 128 + j, p2,
                           DEV ? (unsigned long long)seeds[k] : seed, offset,
                           z3, a3, m3);
  }
}

template <bool DEV>
__global__ __launch_bounds__(FC1R_BLK)
void k_fc1_fwd_reduce_mb(const float* __restrict__ slab,
                         const float* __restrict__ params, long long P,
                         long long ob3, int bs, int K, float p2,
                         const long long* __restrict__ seeds,
                         unsigned long long seed, unsigned long long offset,
                         float* __restrict__ z3, float* __restrict__ a3,
                         unsigned char* __restrict__ m3) {
  fc1_reduce_stack<FC1_SPLIT, DEV>(slab, params, P, ob3, bs, K, p2, seeds,
                                   seed, offset, z3, a3, m3);
}

// fc2 + softmax + CE for one sample row (one block): logits = W4 @ a3 +
// b4 ; softmax ; *loss += -log p[target]/Bk ; dlogit = (p - onehot)/Bk,
// Bk the row count of the client's batch.  sm holds C floats of LDS.
// The row's dlogits also stay in sm, and the block then does the row's
// fc2 backward-data: dz3[kk] = sum_j dlogit[j] * W4[j][kk] (j ascending),
// gated by the fc1 dropout mask and z3 > 0.  z3r / m3r / dz3r point at the
// row's 128 elements.
__device__ __forceinline__ void fc2_loss_row(
    const float* __restrict__ ap, const float* __restrict__ w4,
    const float* __restrict__ b4, int target, int Bk, int C,
    float* __restrict__ dl, float* __restrict__ loss, float* sm,
    const float* __restrict__ z3r, const unsigned char* __restrict__ m3r,
    float p2, float* __restrict__ dz3r) {
  for (int j = threadIdx.x; j < C; j += blockDim.x) {
    const float* wp = w4 + (long long)j * 128;
    float s = b4[j];
    #pragma unroll 4
    for (int kk = 0; kk < 128; ++kk) s = fmaf(wp[kk], ap[kk], s);
    sm[j] = s;
  }
  __syncthreads();
  // one thread does the softmax: C is small
  if (threadIdx.x == 0) {
    float mx = sm[0];
    for (int j = 1; j < C; ++j) mx = fmaxf(mx, sm[j]);
    float z = 0.f;
    for (int j = 0; j < C; ++j) { sm[j] = __expf(sm[j] - mx); z += sm[j]; }
    float inv = 1.f / z;
    float pt = sm[target] * inv;
    for (int j = 0; j < C; ++j) {
      float p = sm[j] * inv;
      float d = (p - (j == target ? 1.f : 0.f)) / (float)Bk;
      dl[j] = d;
      sm[j] = d;
    }
    atomicAdd(loss, -__logf(fmaxf(pt, 1e-30f)) / (float)Bk);
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    int kk = threadIdx.x;
    float zv = z3r[kk];
    unsigned char mk = m3r[kk];
    float s = 0.f;
    for (int j = 0; j < C; ++j)
      s = fmaf(sm[j], w4[(long long)j * 128 + kk], s);
    float gg = (p2 > 0.f) ? (mk ? s * (1.f / (1.f - p2)) : 0.f) : s;
    dz3r[kk] = zv > 0.f ? gg : 0.f;
  }
}

// one block per super-row g; yb<0 (inactive) rows zero their dlogits and
// their dz3 (what backward-data gives from zero dlogits)
template <typename Meta>
__global__ void k_fc2_loss_fwd_mb(const float* __restrict__ a3,
                                  const float* __restrict__ params,
                                  long long P, long long ow4, long long ob4,
                                  Meta meta, int bs, int K, int C,
                                  const int* __restrict__ yb,
                                  float* __restrict__ dlogits,
                                  float* __restrict__ loss_out,
                                  const float* __restrict__ z3,
                                  const unsigned char* __restrict__ m3,
                                  float p2, float* __restrict__ dz3) {
  extern __shared__ float sm[];
  long long g = blockIdx.x;
  int k = (int)(g / bs);
  int target = yb[g];
  if (target < 0) {
    for (int j = threadIdx.x; j < C; j += blockDim.x)
      dlogits[g * C + j] = 0.f;
    if (threadIdx.x < 128) dz3[g * 128 + threadIdx.x] = 0.f;
    return;
  }
  fc2_loss_row(a3 + g * 128, params + (long long)k * P + ow4,
               params + (long long)k * P + ob4, target,
               meta.rows(k, bs), C, dlogits + g * C, loss_out + k,
               sm, z3 + g * 128, m3 + g * 128, p2, dz3 + g * 128);
}

// fc2 backward (weights): grid = K * ceil(C*128/256)
__global__ void k_fc2_bwd_w_mb(const float* __restrict__ dlogits,
                               const float* __restrict__ a3,
                               float* __restrict__ grads, long long P,
                               long long ow4, long long ob4, int bs, int K,
                               int C) {
  int per_k = (C * 128 + FBLK - 1) / FBLK;
  int k = blockIdx.x / per_k;
  int i0 = (blockIdx.x % per_k) * FBLK + threadIdx.x;
  if (i0 >= C * 128) return;
  int kk = i0 % 128, j = i0 / 128;
  const float* dlk = dlogits + (long long)k * bs * C;
  const float* a3k = a3 + (long long)k * bs * 128;
  float s = 0.f, sb = 0.f;
  for (int b = 0; b < bs; ++b) {
    float d = dlk[(long long)b * C + j];
    s = fmaf(d, a3k[(long long)b * 128 + kk], s);
    if (kk == 0) sb += d;
  }
  grads[(long long)k * P + ow4 + i0] = s;
  if (kk == 0) grads[(long long)k * P + ob4 + j] = sb;
}

// Column map of the two fc1 backward kernels.  n = 9216 is an OUTPUT
// dimension in both, so which lane owns which column is free and changes
// no element's summation chain.  A wave's 64 columns are owned so that a
// lane reads and writes VEC adjacent columns at once: n-tile nt of lane
// il is column (nt / VEC) * 16 * VEC + VEC * il + nt % VEC.  VEC = 4: one
// 16 B access of columns 4*il .. 4*il+3, a wave instruction covers 256
// contiguous bytes per row; VEC = 2: two 8 B halves 32 columns apart;
// VEC = 1: the dword map nt * 16 + il.
#define FC1B_COL(VEC, g, il) ((g) * 16 * (VEC) + (VEC) * (il))

// fc1 backward weights (f32 MFMA): grid = K * 144.  Block 0 of every
// client also writes the 128 bias sums db3[j] = sum_b dz3[b][j].
template <int VEC>
__device__ __forceinline__ void fc1_bwd_w_body(
    const float* __restrict__ dz, const float* __restrict__ a2k,
    float* __restrict__ dw3, int bs, int nblk) {
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int kc = lane >> 4, il = lane & 15;
  f32x4 acc[2][4] = {{f32x4{0,0,0,0}, f32x4{0,0,0,0}, f32x4{0,0,0,0}, f32x4{0,0,0,0}},
                     {f32x4{0,0,0,0}, f32x4{0,0,0,0}, f32x4{0,0,0,0}, f32x4{0,0,0,0}}};
  for (int k0 = 0; k0 < ((bs + 3) & ~3); k0 += 4) {
    int b = k0 + kc;
    bool kv = b < bs;
    // rows >= bs read the last valid row and are zeroed by selects, so no
    // load sits behind a branch (and a full wait)
    int bl = kv ? b : bs - 1;
    float a0 = dz[bl * 128 + w * 32 + il];
    float a1v = dz[bl * 128 + w * 32 + 16 + il];
    float bv[4];
    #pragma unroll
    for (int g = 0; g < 4 / VEC; ++g)
      ld_vec<VEC>(a2k + (bl * 9216 + nblk * 64 + FC1B_COL(VEC, g, il)),
                  bv + g * VEC);
    if (!kv) {
      a0 = 0.f; a1v = 0.f;
      #pragma unroll
      for (int nt = 0; nt < 4; ++nt) bv[nt] = 0.f;
    }
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv[nt], acc[0][nt], 0, 0, 0);
      acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v, bv[nt], acc[1][nt], 0, 0, 0);
    }
  }
  #pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    int j = w * 32 + tt * 16 + (lane >> 4) * 4;
    #pragma unroll
    for (int r = 0; r < 4; ++r)
      #pragma unroll
      for (int g = 0; g < 4 / VEC; ++g) {
        float v[VEC];
        #pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = acc[tt][g * VEC + e][r];
        st_vec<VEC>(dw3 + ((j + r) * 9216 + nblk * 64 +
                           FC1B_COL(VEC, g, il)), v);
      }
  }
}

// dw3 rows live at gw + k*Pw + ow3, the bias sums at gb + k*Pb + ob3 (the
// round passes the gradient stack twice; the debug launcher two buffers)
__global__ __launch_bounds__(256)
void k_fc1_bwd_w_mfma_mb(const float* __restrict__ dz3,
                         const float* __restrict__ a2,
                         float* gw, long long Pw, long long ow3,
                         float* gb, long long Pb, long long ob3,
                         int bs, int K) {
  int k = blockIdx.x / 144;
  int nblk = blockIdx.x % 144;
  const float* dz = dz3 + (long long)k * bs * 128;
  const float* a2k = a2 + (long long)k * bs * 9216;
  float* dw3 = gw + (long long)k * Pw + ow3;
  int vec = addr_vec((unsigned long long)a2k | (unsigned long long)dw3);
  if (vec == 4) fc1_bwd_w_body<4>(dz, a2k, dw3, bs, nblk);
  else if (vec == 2) fc1_bwd_w_body<2>(dz, a2k, dw3, bs, nblk);
  else fc1_bwd_w_body<1>(dz, a2k, dw3, bs, nblk);
  if (nblk == 0 && threadIdx.x < 128) {
    int j = threadIdx.x;
    float s = 0.f;
    for (int b = 0; b < bs; ++b) s += dz[(long long)b * 128 + j];
    gb[(long long)k * Pb + ob3 + j] = s;
  }
}

// fc1 backward data (f32 MFMA): grid = K * FC1X_BLKS blocks of FC1X_WAVES
// waves; a wave owns 64 columns (2 x 4 accumulators) and walks j = 0..127
// in order, FC1X_GRP k-steps of loads in flight at a time.
#define FC1X_WAVES 2
#define FC1X_GRP 8
#define FC1X_BLKS (9216 / (64 * FC1X_WAVES))
template <int VEC>
__device__ __forceinline__ void fc1_bwd_x_body(
    const float* __restrict__ dz, const float* __restrict__ w3,
    float* __restrict__ da, int bs, int col0) {
  int lane = threadIdx.x & 63;
  int kc = lane >> 4, il = lane & 15;
  f32x4 acc[2][4] = {{f32x4{0,0,0,0}, f32x4{0,0,0,0}, f32x4{0,0,0,0}, f32x4{0,0,0,0}},
                     {f32x4{0,0,0,0}, f32x4{0,0,0,0}, f32x4{0,0,0,0}, f32x4{0,0,0,0}}};
  // FC1X_GRP k-steps at a time: all of the group's loads are issued into
  // registers, then its MFMAs run in k order.  Rows >= bs read a clamped
  // (valid) dz row and are zeroed by a select: a branch around a load
  // would put a full wait behind it.
  int r0 = (il < bs ? il : bs - 1) * 128 + kc;
  int r1 = (16 + il < bs ? 16 + il : bs - 1) * 128 + kc;
  #pragma unroll 1
  for (int k0 = 0; k0 < 128; k0 += 4 * FC1X_GRP) {
    float bv[FC1X_GRP][4], av[FC1X_GRP][2];
    #pragma unroll
    for (int u = 0; u < FC1X_GRP; ++u) {
      int j = k0 + 4 * u + kc;
      #pragma unroll
      for (int g = 0; g < 4 / VEC; ++g)
        ld_vec<VEC>(w3 + (j * 9216 + col0 + FC1B_COL(VEC, g, il)),
                    bv[u] + g * VEC);
      av[u][0] = dz[r0 + k0 + 4 * u];
      av[u][1] = dz[r1 + k0 + 4 * u];
    }
    #pragma unroll
    for (int u = 0; u < FC1X_GRP; ++u)
      #pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        float a = tt * 16 + il < bs ? av[u][tt] : 0.f;
        #pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          acc[tt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[u][nt], acc[tt][nt], 0, 0, 0);
      }
  }
  #pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    int bu = tt * 16 + (lane >> 4) * 4;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (bu + r >= bs) continue;
      #pragma unroll
      for (int g = 0; g < 4 / VEC; ++g) {
        float v[VEC];
        #pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = acc[tt][g * VEC + e][r];
        st_vec<VEC>(da + ((bu + r) * 9216 + col0 + FC1B_COL(VEC, g, il)),
                    v);
      }
    }
  }
}

__global__ __launch_bounds__(64 * FC1X_WAVES)
void k_fc1_bwd_x_mfma_mb(const float* __restrict__ dz3,
                         const float* __restrict__ params, long long P,
                         long long ow3, int bs, int K,
                         float* __restrict__ da2) {
  int k = blockIdx.x / FC1X_BLKS;
  int nblk = blockIdx.x % FC1X_BLKS;
  const float* dz = dz3 + (long long)k * bs * 128;
  const float* w3 = params + (long long)k * P + ow3;
  float* da = da2 + (long long)k * bs * 9216;
  int col0 = (nblk * FC1X_WAVES + (int)(threadIdx.x >> 6)) * 64;
  int vec = addr_vec((unsigned long long)w3 | (unsigned long long)da);
  if (vec == 4) fc1_bwd_x_body<4>(dz, w3, da, bs, col0);
  else if (vec == 2) fc1_bwd_x_body<2>(dz, w3, da, bs, col0);
  else fc1_bwd_x_body<1>(dz, w3, da, bs, col0);
}

// the conv2 bias sum of one (client, channel) block: every thread's
// partial s through the 64-lane shuffle-down tree, then the wave sums in
// wave order
__device__ __forceinline__ void conv2_bias_block_sum(float s,
                                                     float* __restrict__ out) {
  for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
  __shared__ float lds[4];
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tt = 0.f;
    for (int q = 0; q < (int)blockDim.x / 64; ++q) tt += lds[q];
    *out = tt;
  }
}

// dropout(p1) + maxpool 2x2 + ReLU backward, and the conv2 bias gradient
// of the dz2 it writes.  grid = K * 64, FBLK threads, one block per
// (client, co).  Thread t walks the client's bs * 576 elements of that
// channel e = t, t + 256, .. (b = e / 576, o = e % 576): the element is
// its cell's gradient gg iff pidx names it AND carries the gate bit
// (pidx == d | 4, the forward's max > 0), else 0.  It reads no r2.  Each
// element is stored to dz2 (coalesced dwords) and added to the thread's
// partial in e order, exactly the chain k_conv2_bwd_b_mb runs over a
// stored dz2.  PDB_U elements are loaded before the first add; past the
// end a clamped (valid) element is loaded and dropped by selects, so no
// load sits behind a branch.
#define PDB_U 9  /* 45 strides at bs = 20: five groups of 27 loads */
__global__ __launch_bounds__(FBLK)
void k_pool_drop_bwd_bias_mb(const float* __restrict__ da2,
                             const unsigned char* __restrict__ pidx,
                             const unsigned char* __restrict__ m2, int bs,
                             int K, float p1, float* __restrict__ dz2,
                             float* __restrict__ grads, long long P,
                             long long ob2) {
  int k = blockIdx.x / 64;
  int co = blockIdx.x % 64;
  int n = bs * 576;
  bool drop = p1 > 0.f;
  float inv_keep = (p1 < 1.f) ? 1.f / (1.f - p1) : 0.f;
  float sc = drop ? inv_keep : 1.f;
  const long long row0 = (long long)k * bs * 64 + co;  // plane of b = 0
  float s = 0.f;
  for (int e0 = threadIdx.x; e0 < n; e0 += PDB_U * FBLK) {
    float da[PDB_U];
    unsigned char pi[PDB_U], mk[PDB_U];
    #pragma unroll
    for (int u = 0; u < PDB_U; ++u) {
      int e = e0 + u * FBLK;
      e = e < n ? e : n - 1;
      int b = e / 576, o = e % 576;
      int y = o / 24, x = o % 24;
      long long cell = (row0 + (long long)b * 64) * 144 + (y >> 1) * 12
                       + (x >> 1);
      da[u] = da2[cell];
      pi[u] = pidx[cell];
      mk[u] = m2[cell];
    }
    #pragma unroll
    for (int u = 0; u < PDB_U; ++u) {
      int e = e0 + u * FBLK;
      int ec = e < n ? e : n - 1;
      int b = ec / 576, o = ec % 576;
      int d = ((o / 24) & 1) * 2 + (o & 1);  // 24 is even: x & 1 == o & 1
      // = drop ? (mk ? da * inv_keep : 0) : da, as selects (da * 1.f == da)
      float gg = (drop && !mk[u]) ? 0.f : da[u] * sc;
      float v = pi[u] == (d | 4) ? gg : 0.f;
      if (e < n) {
        dz2[(row0 + (long long)b * 64) * 576 + o] = v;
        s += v;
      }
    }
  }
  conv2_bias_block_sum(s, grads + (long long)k * P + ob2 + co);
}

// conv2 backward weights (f32 MFMA): per image, dw[co][n] = sum over the
// 576 output positions o of dz2[co][o] * a1[ci(n)][(y+kh)*26 + x+kw].
// grid = G * 9, 128 threads; a block owns all 64 co x 32 n columns and
// walks o in chunks of C2W_ROWS output rows.  Per chunk it stages the
// dz2 rows in their native [co][o] layout (8 lanes x float4 = one 128 B
// line per row piece) and the raw rows+2 a1 rows of the <= 5 ci planes
// its 32 columns touch; no im2col tile and no transposed copy of dz2.
// The B address is o + 2*(o/24) plus a per-lane (ci,kh,kw) constant: the
// k-loop is unrolled by one 24-wide output row, so every offset is an
// immediate.  Wave w owns a 2 x 2 block of accumulators (co 32w..32w+31),
// each dz2 / a1 fragment feeds 2 MFMAs.  Each image's partial runs over o
// ascending from 0; k_conv2_bwd_w_fold_mb then sums rows b ascending.
#define C2W_ROWS 4                      /* output rows per staged chunk */
#define C2W_OC (C2W_ROWS * 24)          /* k (= o) values per chunk */
#define C2W_LD (C2W_OC + 2)             /* 98 %% 32 = 2: the 16 co x 2 kc of
                                           a 32-lane group hit 32 banks */
#define C2W_PS ((C2W_ROWS + 2) * 26)    /* staged floats per a1 plane */
static_assert(24 % C2W_ROWS == 0 && C2W_OC % 32 == 0 && C2W_PS <= 256,
              "conv2 bwd_w chunk: whole rows, whole 128 B row pieces, an a1 "
              "plane in two passes of the 128 threads");
__global__ __launch_bounds__(128)
void k_conv2_bwd_w_mfma_mb(const float* __restrict__ dz2,
                           const float* __restrict__ a1, int bs, int K,
                           float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) float dzl[64 * C2W_LD];
  __shared__ float apl[5 * C2W_PS];
  int nb = blockIdx.x % 9;
  long long g = blockIdx.x / 9;
  const float* dzb = dz2 + g * 36864;
  const float* a1b = a1 + g * 21632;
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int il = lane & 15, kc = lane >> 4;
  int ci0 = nb * 32 / 9;
  int npl = 32 - ci0 < 5 ? 32 - ci0 : 5;
  int aoff[2], boff[2];
  #pragma unroll
  for (int q = 0; q < 2; ++q) {
    aoff[q] = (w * 32 + q * 16 + il) * C2W_LD + kc;
    int n = nb * 32 + q * 16 + il;
    int ci = n / 9, rem = n % 9;
    boff[q] = (ci - ci0) * C2W_PS + (rem / 3) * 26 + rem % 3 + kc;
  }
  f32x4 acc[2][2];
  acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = f32x4{0, 0, 0, 0};
  int sub = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  // The next chunk's global loads are issued before the current chunk's
  // MFMAs and held in registers, so their latency hides behind the
  // matrix work; only the register -> LDS copy sits between barriers.
  float4 pdz[4][C2W_OC / 32];
  float pa[5][2];
  auto fetch = [&](int c) {
    #pragma unroll
    for (int it = 0; it < 4; ++it) {
      const float4* sp = reinterpret_cast<const float4*>(
          dzb + (r0 + 16 * it) * 576 + c * C2W_OC);
      #pragma unroll
      for (int u = 0; u < C2W_OC / 32; ++u) pdz[it][u] = sp[sub + 8 * u];
    }
    #pragma unroll
    for (int p = 0; p < 5; ++p) {
      const float* sp = a1b + (ci0 + p) * 676 + c * (C2W_ROWS * 26);
      #pragma unroll
      for (int h = 0; h < 2; ++h) {
        int j = threadIdx.x + 128 * h;
        pa[p][h] = (p < npl && j < C2W_PS) ? sp[j] : 0.f;
      }
    }
  };
  fetch(0);
  for (int c = 0; c < 24 / C2W_ROWS; ++c) {
    __syncthreads();
    #pragma unroll
    for (int it = 0; it < 4; ++it) {
      float* dp = dzl + (r0 + 16 * it) * C2W_LD;
      #pragma unroll
      for (int u = 0; u < C2W_OC / 32; ++u) {
        float4 v = pdz[it][u];
        float2* d2 = reinterpret_cast<float2*>(dp + 4 * (sub + 8 * u));
        d2[0] = float2{v.x, v.y};
        d2[1] = float2{v.z, v.w};
      }
    }
    #pragma unroll
    for (int p = 0; p < 5; ++p)
      #pragma unroll
      for (int h = 0; h < 2; ++h) {
        int j = threadIdx.x + 128 * h;
        if (j < C2W_PS) apl[p * C2W_PS + j] = pa[p][h];
      }
    __syncthreads();
    if (c + 1 < 24 / C2W_ROWS) fetch(c + 1);
    #pragma unroll
    for (int y = 0; y < C2W_ROWS; ++y)
      #pragma unroll
      for (int s = 0; s < 6; ++s) {
        float a0 = dzl[aoff[0] + y * 24 + 4 * s];
        float a1v = dzl[aoff[1] + y * 24 + 4 * s];
        float b0 = apl[boff[0] + y * 26 + 4 * s];
        float b1 = apl[boff[1] + y * 26 + 4 * s];
        acc[0][0] =
            __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] =
            __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] =
            __builtin_amdgcn_mfma_f32_16x16x4f32(a1v, b0, acc[1][0], 0, 0, 0);
        acc[1][1] =
            __builtin_amdgcn_mfma_f32_16x16x4f32(a1v, b1, acc[1][1], 0, 0, 0);
      }
  }
  float* out = slab + g * 18432;
  #pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    int orow = w * 32 + mt * 16 + kc * 4;
    #pragma unroll
    for (int nt = 0; nt < 2; ++nt)
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(orow + r) * 288 + nb * 32 + nt * 16 + il] = acc[mt][nt][r];
  }
}

__global__ void k_conv2_bwd_w_fold_mb(const float* __restrict__ slab,
                                      float* __restrict__ grads, long long P,
                                      long long ow2, int bs, int K) {
  int per_k = (18432 + FBLK - 1) / FBLK;
  int k = blockIdx.x / per_k;
  int i = (blockIdx.x % per_k) * FBLK + threadIdx.x;
  if (i >= 18432) return;
  const float* slk = slab + (long long)k * bs * 18432;
  float s = 0.f;
  for (int b = 0; b < bs; ++b) s += slk[(long long)b * 18432 + i];
  grads[(long long)k * P + ow2 + i] = s;
}

// bias sum over a dz2 that is already in memory: the per-kernel debug
// launchers only (they take dz2 as an input).  The drivers get the same
// chain from k_pool_drop_bwd_bias_mb, which writes dz2.
__global__ void k_conv2_bwd_b_mb(const float* __restrict__ dz2,
                                 float* __restrict__ grads, long long P,
                                 long long ob2, int bs, int K) {
  int k = blockIdx.x / 64;
  int co = blockIdx.x % 64;
  const float* dzk = dz2 + (long long)k * bs * 36864;
  float s = 0.f;
  for (int t = threadIdx.x; t < bs * 576; t += blockDim.x) {
    int o = t % 576, b = t / 576;
    s += dzk[((long long)b * 64 + co) * 576 + o];
  }
  conv2_bias_block_sum(s, grads + (long long)k * P + ob2 + co);
}

// conv2 backward data (f32 MFMA), implicit GEMM from a zero-padded dz2.
// grid = G * C2X_BLKS; a block owns 128 consecutive output positions
// (m = p*26 + q) x all 32 ci of one image.  It stages, once and with no
// per-element index arithmetic, the <= 8 padded dz2 rows those positions
// read for all 64 co: each (co, row) task loads one 96 B row as float4s
// and writes it as a 28-float row with a 2-column zero halo; rows outside
// the image are zero rows, so the k-loop has no bounds test.  56 KB ->
// 2 blocks/CU.  Wave w owns a 2 x 2 block of accumulators (positions
// 32w..32w+31, both ci tiles); each W2 fragment (one global load per
// k-step from w2rot) and each dz2 fragment feeds 2 MFMAs.  Every output's
// k order is (co,kh,kw) ascending from 0; the a1 > 0 mask is applied at
// the store.  Positions past 675 in the last block are clamped for the
// reads and never stored.
#define C2X_MT 128                      /* output positions per block */
#define C2X_BLKS ((676 + C2X_MT - 1) / C2X_MT)
#define C2X_ROWS 8                      /* staged padded rows per co */
#define C2X_CS (C2X_ROWS * 28)          /* staged floats per co plane */
static_assert((25 + C2X_MT + 25) / 26 + 2 <= C2X_ROWS,
              "conv2 bwd_x: a block's positions span at most ROWS-2 rows");
__global__ __launch_bounds__(256)
void k_conv2_bwd_x_mfma_mb(const float* __restrict__ dz2,
                           const float* __restrict__ w2rot_stack,
                           const float* __restrict__ a1, int bs, int K,
                           float* __restrict__ dz1) {
  __shared__ __attribute__((aligned(16))) float lds[64 * C2X_CS];
  long long g = blockIdx.x / C2X_BLKS;
  int mb = blockIdx.x % C2X_BLKS;
  int k = (int)(g / bs);
  int m0 = mb * C2X_MT, p0 = m0 / 26;
  const float* dzb = dz2 + g * 36864;
  // staged row lr of plane co holds dz2 row p0 + lr - 2 at columns 2..25
  for (int task = threadIdx.x; task < 64 * C2X_ROWS; task += 256) {
    int co = task / C2X_ROWS, lr = task % C2X_ROWS;
    int y = p0 + lr - 2;
    float4 s[6];
    if (y >= 0 && y < 24) {
      const float4* sp =
          reinterpret_cast<const float4*>(dzb + co * 576 + y * 24);
      #pragma unroll
      for (int u = 0; u < 6; ++u) s[u] = sp[u];
    } else {
      #pragma unroll
      for (int u = 0; u < 6; ++u) s[u] = float4{0.f, 0.f, 0.f, 0.f};
    }
    float4* dp = reinterpret_cast<float4*>(lds + co * C2X_CS + lr * 28);
    dp[0] = float4{0.f, 0.f, s[0].x, s[0].y};
    #pragma unroll
    for (int u = 1; u < 6; ++u)
      dp[u] = float4{s[u - 1].z, s[u - 1].w, s[u].x, s[u].y};
    dp[6] = float4{s[5].z, s[5].w, 0.f, 0.f};
  }
  __syncthreads();
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int il = lane & 15, kc = lane >> 4;
  int mw = m0 + w * 32;
  if (mw >= 676) return;
  int off[9], base[2];
  conv2_tap_offsets(kc, C2X_CS, 28, -1, off);
  #pragma unroll
  for (int i = 0; i < 2; ++i) {
    int m = mw + i * 16 + il;
    m = m < 676 ? m : 675;
    base[i] = (m / 26 - p0 + 2) * 28 + m % 26 + 2;
  }
  const float* wp = w2rot_stack + (long long)k * 18432 + kc * 32 + il;
  f32x4 acc[2][2];
  acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = f32x4{0, 0, 0, 0};
  for (int t = 0; t < 16; ++t) {
    const float* lt = lds + t * 4 * C2X_CS;
    const float* wt = wp + t * 36 * 32;
    #pragma unroll
    for (int j = 0; j < 9; ++j) {
      float b0 = wt[j * 128], b1 = wt[j * 128 + 16];
      #pragma unroll
      for (int i = 0; i < 2; ++i) {
        float a = lt[base[i] + off[j]];
        acc[i][0] =
            __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[i][0], 0, 0, 0);
        acc[i][1] =
            __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[i][1], 0, 0, 0);
      }
    }
  }
  #pragma unroll
  for (int i = 0; i < 2; ++i) {
    int om = mw + i * 16 + kc * 4;  // 4 | 676: a quad is all in or all out
    if (om >= 676) continue;
    #pragma unroll
    for (int n = 0; n < 2; ++n) {
      long long o = (g * 32 + n * 16 + il) * 676 + om;
      float4 av = *reinterpret_cast<const float4*>(a1 + o);
      float4 v;
      v.x = av.x > 0.f ? acc[i][n][0] : 0.f;
      v.y = av.y > 0.f ? acc[i][n][1] : 0.f;
      v.z = av.z > 0.f ? acc[i][n][2] : 0.f;
      v.w = av.w > 0.f ? acc[i][n][3] : 0.f;
      *reinterpret_cast<float4*>(dz1 + o) = v;
    }
  }
}

__global__ void k_conv1_bwd_w_mb(const float* __restrict__ x,
                                 const float* __restrict__ dz1,
                                 float* __restrict__ grads, long long P,
                                 long long ow1, long long ob1, int bs,
                                 int K) {
  int k = blockIdx.x / 32;
  int co = blockIdx.x % 32;
  const float* xk = x + (long long)k * bs * 784;
  const float* dzk = dz1 + (long long)k * bs * 21632;
  float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  float accb = 0.f;
  for (int t = threadIdx.x; t < bs * 676; t += blockDim.x) {
    int o = t % 676, b = t / 676;
    int xx = o % 26, yy = o / 26;
    float d = dzk[((long long)b * 32 + co) * 676 + o];
    const float* xp = xk + b * 784 + yy * 28 + xx;
    #pragma unroll
    for (int kh = 0; kh < 3; ++kh)
      #pragma unroll
      for (int kw = 0; kw < 3; ++kw)
        acc[kh * 3 + kw] = fmaf(xp[kh * 28 + kw], d, acc[kh * 3 + kw]);
    accb += d;
  }
  __shared__ float lds[16 * 10];
  int n_waves = blockDim.x / 64;
  int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  #pragma unroll
  for (int kk = 0; kk < 9; ++kk) {
    float s = acc[kk];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if (lane == 0) lds[wave * 10 + kk] = s;
  }
  float sb = accb;
  for (int d = 32; d > 0; d >>= 1) sb += __shfl_down(sb, d, 64);
  if (lane == 0) lds[wave * 10 + 9] = sb;
  __syncthreads();
  if (threadIdx.x < 9) {
    float s = 0.f;
    for (int w = 0; w < n_waves; ++w) s += lds[w * 10 + threadIdx.x];
    grads[(long long)k * P + ow1 + co * 9 + threadIdx.x] = s;
  }
  if (threadIdx.x == 9) {
    float s = 0.f;
    for (int w = 0; w < n_waves; ++w) s += lds[w * 10 + 9];
    grads[(long long)k * P + ob1 + co] = s;
  }
}

// per-client clip + sufficient stats + SGD over the gradient stacks.
// Stage 1: per-(k, chunk) partial sum/sumsq -> f64 atomics into acc[2k]
// (few hundred atomics per client per step).  Stage 2 (k_clip_sgd_mb):
// per-client scale + SGD in one elementwise pass, whose block 0 also
// accumulates the K clients' clipped stats.
//
// FedProx (the ProxArgs instantiations of both kernels; NoProx, an empty
// argument, instantiates the FedAvg code unchanged): the
// gradient both passes see is gp = g + mu * (w - w_g), formed in registers
// by prox_grad() and never stored unless STORE_G; a third f64 slot per
// client, acc[2K + k], collects sum (w - w_g)^2 for the reported loss.
// The term exists only for a client that is ACTIVE at this step: an idle
// client (epoch finished / masked) has g == 0 exactly and must not move,
// although its w != w_g.  Idleness is a select on mu, not a branch around
// the loads: mu_eff = 0 makes gp = fma(0, w - w_g, g) = g bit for bit.
struct NoProx { static constexpr bool PROX = false; };
struct ProxArgs {
  static constexpr bool PROX = true;
  const float* params;       // [K * P] weights before the step (sumsq pass)
  int K;
  const float* server;       // [P] server weights w_g, shared by all K
  float mu;
  // active predicate, first non-null wins; neither = every client active
  const long long* counts;   // mega driver: active iff t * bs < counts[k]
  int t, bs;
  const unsigned char* active;  // stand-alone entry: per-client mask [K]
  float* loss_out;           // [K] += 0.5 * mu * sum (w - w_g)^2, or null
};

__device__ __forceinline__ bool prox_active(const NoProx&, int) {
  return true;
}
__device__ __forceinline__ bool prox_active(const ProxArgs& a, int k) {
  if (a.counts) return mega_Bk(a.counts, k, a.t, a.bs) > 0;
  if (a.active) return a.active[k] != 0;
  return true;
}

// the ONE place gp is formed: explicit single roundings, so the value
// whose square k_sumsq sums is bit for bit the value k_clip_sgd applies
__device__ __forceinline__ float prox_grad(float g, float w, float wg,
                                           float mu_eff) {
  return fmaf(mu_eff, __fsub_rn(w, wg), g);
}

// one block per (client, contiguous chunk): block-local tree reduce,
// ONE f64 atomicAdd pair (PROX: triple) per block
// (~K * ceil(P/32768) atomics per step)
#define SUMSQ_CHUNK 32768
template <typename PX>
__global__ void k_sumsq_mb(const float* __restrict__ grads, long long P,
                           int blocks_per_k, double* __restrict__ acc,
                           PX px) {
  constexpr bool PROX = PX::PROX;
  int k = blockIdx.x / blocks_per_k;
  int c = blockIdx.x % blocks_per_k;
  long long lo = (long long)c * SUMSQ_CHUNK;
  long long hi = lo + SUMSQ_CHUNK;
  if (hi > P) hi = P;
  const float* g = grads + (long long)k * P;
  const float* w = nullptr;
  float mu_eff = 0.f;
  if constexpr (PROX) {
    w = px.params + (long long)k * P;
    mu_eff = prox_active(px, k) ? px.mu : 0.f;
  }
  // float4 loads + independent accumulator pairs break the dependent
  // f64-add chain (was ~74 us per step at 190 underfilled blocks)
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;  // PROX: (w - w_g)^2
  // scalar loads (the k*P segment bases are not 16 B aligned); the win
  // is the 4 independent f64 accumulator chains
  long long i = lo + (long long)threadIdx.x * 4;
  for (; i + 3 < hi; i += (long long)blockDim.x * 4) {
    double a, b, cc, d;
    if constexpr (PROX) {
      float d0 = __fsub_rn(w[i], px.server[i]);
      float d1 = __fsub_rn(w[i + 1], px.server[i + 1]);
      float d2 = __fsub_rn(w[i + 2], px.server[i + 2]);
      float d3 = __fsub_rn(w[i + 3], px.server[i + 3]);
      a = prox_grad(g[i], w[i], px.server[i], mu_eff);
      b = prox_grad(g[i + 1], w[i + 1], px.server[i + 1], mu_eff);
      cc = prox_grad(g[i + 2], w[i + 2], px.server[i + 2], mu_eff);
      d = prox_grad(g[i + 3], w[i + 3], px.server[i + 3], mu_eff);
      r0 += (double)d0 * d0; r1 += (double)d1 * d1;
      r2 += (double)d2 * d2; r3 += (double)d3 * d3;
    } else {
      a = g[i]; b = g[i + 1]; cc = g[i + 2]; d = g[i + 3];
    }
    s0 += a; q0 += a * a;
    s1 += b; q1 += b * b;
    s2 += cc; q2 += cc * cc;
    s3 += d; q3 += d * d;
  }
  for (long long j = i; j < hi; ++j) {  // ragged tail (P % 4)
    double v;
    if constexpr (PROX) {
      float dj = __fsub_rn(w[j], px.server[j]);
      v = (double)prox_grad(g[j], w[j], px.server[j], mu_eff);
      r0 += (double)dj * dj;
    } else {
      v = (double)g[j];
    }
    s0 += v; q0 += v * v;
  }
  double fs = (s0 + s1) + (s2 + s3);
  double fq = (q0 + q1) + (q2 + q3);
  double fr = (r0 + r1) + (r2 + r3);
  for (int d = 32; d > 0; d >>= 1) {
    fs += __shfl_down(fs, d, 64);
    fq += __shfl_down(fq, d, 64);
    if constexpr (PROX) fr += __shfl_down(fr, d, 64);
  }
  __shared__ double lds[(PROX ? 3 : 2) * 4];
  constexpr int NS = PROX ? 3 : 2;
  int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    lds[NS * wave] = fs; lds[NS * wave + 1] = fq;
    if constexpr (PROX) lds[NS * wave + 2] = fr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ts = 0.0, tq = 0.0, tr = 0.0;
    for (int wv = 0; wv < (int)blockDim.x / 64; ++wv) {
      ts += lds[NS * wv]; tq += lds[NS * wv + 1];
      if constexpr (PROX) tr += lds[NS * wv + 2];
    }
    atomicAdd(acc + 2 * k, ts);
    atomicAdd(acc + 2 * k + 1, tq);
    if constexpr (PROX) atomicAdd(acc + 2 * px.K + k, tr);
  }
}

__device__ __forceinline__ float clip_scale(const double* __restrict__ acc,
                                            int k, float max_norm,
                                            float eps) {
  float norm = (float)sqrt(acc[2 * k + 1]);
  return (max_norm > 0.f && norm > max_norm) ? max_norm / (norm + eps) : 1.f;
}

// STORE_G: also write the clipped gradient back.  The CNN mega round
// never reads it (the next batch-step's backward kernels and
// k_pseudo_grad_mb overwrite the whole stack), so it runs the variant
// without that store; the stand-alone entry keeps it.  i only grows, so
// a thread re-derives its client and the scale when it crosses a segment
// end, not per element.
template <bool STORE_G, typename PX>
__global__ void k_clip_sgd_mb(float* __restrict__ params,
                              float* __restrict__ grads, long long P, int K,
                              const double* __restrict__ acc, float max_norm,
                              float eps, const float* __restrict__ lr_t,
                              float* __restrict__ stats_out, PX px) {
  constexpr bool PROX = PX::PROX;
  long long total = (long long)K * P;
  float lr = lr_t[0];
  // block 0 also accumulates the per-client clipped stats:
  // stats_out[2k] += scale * sum, stats_out[2k+1] += scale^2 * sumsq
  if (blockIdx.x == 0)
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
      float scale = clip_scale(acc, k, max_norm, eps);
      stats_out[2 * k] += scale * (float)acc[2 * k];
      stats_out[2 * k + 1] += scale * scale * (float)acc[2 * k + 1];
      if constexpr (PROX)
        // the regulariser of an ACTIVE client's step, next to its CE
        if (px.loss_out && prox_active(px, k))
          px.loss_out[k] += (float)(0.5 * (double)px.mu * acc[2 * K + k]);
    }
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  int k = (int)(i / P);
  long long seg_end = (long long)(k + 1) * P;
  float scale = clip_scale(acc, k, max_norm, eps);
  float mu_eff = 0.f;
  if constexpr (PROX) mu_eff = prox_active(px, k) ? px.mu : 0.f;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    if (i >= seg_end) {
      k = (int)(i / P);
      seg_end = (long long)(k + 1) * P;
      scale = clip_scale(acc, k, max_norm, eps);
      if constexpr (PROX) mu_eff = prox_active(px, k) ? px.mu : 0.f;
    }
    if constexpr (PROX) {
      float w = params[i];
      float gv = prox_grad(grads[i], w, px.server[i - (long long)k * P],
                           mu_eff) * scale;
      if constexpr (STORE_G) grads[i] = gv;
      params[i] = w - lr * gv;
    } else {
      float gv = grads[i] * scale;
      if constexpr (STORE_G) grads[i] = gv;
      params[i] -= lr * gv;
    }
  }
}

// weighted pseudo-gradients + deterministic accumulate into round_accum
__global__ void k_pseudo_grad_mb(float* __restrict__ grads,
                                 const float* __restrict__ server,
                                 const float* __restrict__ params,
                                 const float* __restrict__ weights,
                                 long long P, int K) {
  long long total = (long long)K * P;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    int k = (int)(i / P);
    grads[i] = (server[i % P] - params[i]) * weights[k];
  }
}

__global__ void k_accum_mb(float* __restrict__ round_accum,
                           const float* __restrict__ grads, long long P,
                           int K) {
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       p < P; p += (long long)gridDim.x * blockDim.x) {
    float s = round_accum[p];
    for (int k = 0; k < K; ++k) s += grads[(long long)k * P + p];
    round_accum[p] = s;
  }
}

// ---------------------------------------------------------------------------
// DGA tail: the end of a round under dynamic gradient aggregation
// (strategies/dga.py generate_client_payload, clip-only local DP), with
// the aggregation weight formed on the device and no K*P pseudo-gradient
// stack.  Two kernels:
//   k_dga_normsq_mb (clip only): normsq[k] = sum_p (w_g[p] - w_k[p])^2 in
//     f64, k_sumsq_mb's reduction (4 chains per thread, shuffle, LDS, one
//     atomicAdd per (client, chunk) block);
//   k_dga_accum_mb: every block recomputes the K <= 32 coefficients
//     c_k = (float)(weight_k * dp_k) into LDS (one thread per client, all
//     f64), then round_accum[p] += sum_k c_k * (w_g[p] - w_k[p]) with k
//     ascending: one __fsub_rn, one __fmul_rn and one __fadd_rn per
//     (k, p), the roundings of k_pseudo_grad_mb + k_accum_mb.  A client
//     with c_k == 0 is skipped, so it leaves round_accum's bits alone (the
//     host does not accumulate a zero-weight client either).
// ---------------------------------------------------------------------------
#define DGA_MIN_WEIGHT 1e-7  // strategies/dga.py MIN_WEIGHT

__global__ void k_dga_normsq_mb(const float* __restrict__ params,
                                const float* __restrict__ server,
                                long long P, int blocks_per_k,
                                double* __restrict__ normsq) {
  int k = blockIdx.x / blocks_per_k;
  int c = blockIdx.x % blocks_per_k;
  long long lo = (long long)c * SUMSQ_CHUNK;
  long long hi = lo + SUMSQ_CHUNK;
  if (hi > P) hi = P;
  const float* w = params + (long long)k * P;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  long long i = lo + (long long)threadIdx.x * 4;
  for (; i + 3 < hi; i += (long long)blockDim.x * 4) {
    float d0 = __fsub_rn(server[i], w[i]);
    float d1 = __fsub_rn(server[i + 1], w[i + 1]);
    float d2 = __fsub_rn(server[i + 2], w[i + 2]);
    float d3 = __fsub_rn(server[i + 3], w[i + 3]);
    r0 += (double)d0 * d0; r1 += (double)d1 * d1;
    r2 += (double)d2 * d2; r3 += (double)d3 * d3;
  }
  for (long long j = i; j < hi; ++j) {  // ragged tail (P % 4)
    float dj = __fsub_rn(server[j], w[j]);
    r0 += (double)dj * dj;
  }
  double fr = (r0 + r1) + (r2 + r3);
  for (int d = 32; d > 0; d >>= 1) fr += __shfl_down(fr, d, 64);
  __shared__ double lds[4];
  int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) lds[wave] = fr;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tr = 0.0;
    for (int wv = 0; wv < (int)blockDim.x / 64; ++wv) tr += lds[wv];
    atomicAdd(normsq + k, tr);
  }
}

// weight_k of generate_client_payload, all in f64 as on the host
__device__ __forceinline__ double dga_weight(const DgaArgs& a, double loss,
                                             double s, double q,
                                             long long count, long long n) {
  if (a.mode == DGA_MEAN) return 1.0;
  double nd = (double)(n > 1 ? n : 1);
  double tw;
  if (a.mode == DGA_TRAIN_LOSS) {
    tw = loss / (double)(count > 1 ? count : 1);
  } else if (a.mode == DGA_MAG_VAR) {
    double mean = s / nd;
    tw = fmax(__dsub_rn(q / nd, __dmul_rn(mean, mean)), 0.0);
  } else if (a.mode == DGA_MAG_MEAN) {
    tw = s / nd;
  } else {
    tw = sqrt(fmax(q / nd, 0.0));
  }
  double arg = __dmul_rn(-a.beta, tw);
  double w = exp(arg);
  // math.exp raises OverflowError (-> MIN_WEIGHT) for a finite argument
  // only; exp(+inf) returns inf and filter_weight zeroes it
  if (isinf(w) && !isinf(arg)) w = DGA_MIN_WEIGHT;
  if (isnan(w) || isinf(w)) w = 0.0;   // filter_weight
  else if (w > 100.0) w = 100.0;
  return w;
}

__global__ void k_dga_accum_mb(float* __restrict__ round_accum,
                               const float* __restrict__ server,
                               const float* __restrict__ params, long long P,
                               int K, const float* __restrict__ loss_out,
                               const float* __restrict__ stats_out,
                               const long long* __restrict__ counts, int bs,
                               DgaArgs a, const double* __restrict__ normsq,
                               double* __restrict__ dga_out) {
  __shared__ float coef[DGA_MAX_K];
  if ((int)threadIdx.x < K) {
    int k = threadIdx.x;
    long long cnt = counts[k];
    long long n = ((cnt + bs - 1) / bs) * P;
    double w = dga_weight(a, (double)loss_out[k], (double)stats_out[2 * k],
                          (double)stats_out[2 * k + 1], cnt, n);
    double norm = 0.0, dp = 1.0;
    if (a.clip) {
      norm = sqrt(normsq[k]);
      if (norm > a.max_grad) dp = a.max_grad / norm;
    }
    double c = __dmul_rn(w, dp);
    coef[k] = (float)c;
    if (blockIdx.x == 0) {
      dga_out[k] = w;
      dga_out[K + k] = norm;
      dga_out[2 * K + k] = (double)coef[k];  // as applied: f32-rounded
    }
  }
  __syncthreads();
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       p < P; p += (long long)gridDim.x * blockDim.x) {
    float wg = server[p];
    float s = round_accum[p];
    for (int k = 0; k < K; ++k) {
      float c = coef[k];
      if (c != 0.f) {  // block-uniform: coef is per client
        float d = __fsub_rn(wg, params[(long long)k * P + p]);
        s = __fadd_rn(s, __fmul_rn(c, d));
      }
    }
    round_accum[p] = s;
  }
}

static void dga_tail(const float* params_stack, const float* server,
                     long long P, int K, const float* loss_out,
                     const float* stats_out, const long long* counts_dev,
                     int bs, const DgaArgs& dga, float* round_accum,
                     double* dga_out, hipStream_t s) {
  double* normsq = dga_out + 3 * K;
  if (dga.clip) {
    int blocks_per_k = (int)((P + SUMSQ_CHUNK - 1) / SUMSQ_CHUNK);
    hipMemsetAsync(normsq, 0, K * sizeof(double), s);
    hipLaunchKernelGGL(k_dga_normsq_mb, dim3(K * blocks_per_k), dim3(FBLK),
                       0, s, params_stack, server, P, blocks_per_k, normsq);
  }
  int gp = (int)((P + FBLK - 1) / FBLK); if (gp > 2048) gp = 2048;
  hipLaunchKernelGGL(k_dga_accum_mb, dim3(gp), dim3(FBLK), 0, s, round_accum,
                     server, params_stack, P, K, loss_out, stats_out,
                     counts_dev, bs, dga, normsq, dga_out);
}

// ---------------------------------------------------------------------------
// bf16 GEMM kernels (mixed precision: bf16 MFMA inputs at ~13-16x the
// f32 MFMA rate, fp32 accumulators, fp32 master weights/outputs — the
// SGD step, clip/stats, DP/quant hooks all stay fp32).  The GEMM
// operands are materialized in LDS as bf16 with k-contiguous rows so
// each lane's 8-element fragment is ONE 16 B ds_read; row strides are
// padded so 16-lane fragment groups hit distinct banks.  Conversion
// f32->bf16 happens during LDS staging (round-to-nearest via __bf16
// cast); the inner loops read ONLY LDS, so the L2-latency bound of the
// f32 variants does not apply.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

__device__ __forceinline__ bf16x8 ld_bf16x8(const __bf16* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}

// [k][ci][k'=(co,kh,kw)] bf16 layout for the bwd-data B operand (built
// once per batch into the w2rot_stack buffer reinterpreted as bf16)
__global__ void k_w2rotbf_mb(const float* __restrict__ params, long long P,
                             long long ow2, int K,
                             __bf16* __restrict__ w2rotbf) {
  long long total = (long long)K * 18432;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    int k = (int)(i / 18432), r = (int)(i % 18432);
    int co = r / 288, rem9 = r % 288;
    int ci = rem9 / 9, rem = rem9 % 9;
    w2rotbf[(long long)k * 18432 + (long long)ci * 576 + co * 9 + rem] =
        (__bf16)params[(long long)k * P + ow2 + r];
  }
}

#define MC2_LD 296
__global__ __launch_bounds__(256)
void k_conv2_fwd_mfma_mb_bf16(const float* __restrict__ a1,
                              const float* __restrict__ params, long long P,
                              long long ow2, long long ob2, int bs, int K,
                              float* __restrict__ r2) {
  __shared__ __bf16 imc[64 * MC2_LD];
  __shared__ __bf16 wb[64 * MC2_LD];
  long long g = blockIdx.x / 9;
  int mt = blockIdx.x % 9;
  int k = (int)(g / bs);
  const float* a1b = a1 + g * 21632;
  const float* w2 = params + (long long)k * P + ow2;
  const float* b2 = params + (long long)k * P + ob2;
  for (int i = threadIdx.x; i < 64 * 288; i += 256) {
    int mr = i / 288, kk = i % 288;
    int m = mt * 64 + mr, yy = m / 24, xx = m % 24;
    int ci = kk / 9, rem = kk % 9, kh = rem / 3, kw = rem % 3;
    imc[mr * MC2_LD + kk] = (__bf16)a1b[ci * 676 + (yy + kh) * 26 + xx + kw];
    wb[mr * MC2_LD + kk] = (__bf16)w2[i];  // mr doubles as co
  }
  __syncthreads();
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int il = lane & 15, kc8 = (lane >> 4) * 8;
  f32x4 acc[4] = {f32x4{0,0,0,0}, f32x4{0,0,0,0},
                  f32x4{0,0,0,0}, f32x4{0,0,0,0}};
  for (int k0 = 0; k0 < 288; k0 += 32) {
    bf16x8 a = ld_bf16x8(&imc[(w * 16 + il) * MC2_LD + k0 + kc8]);
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      bf16x8 bv = ld_bf16x8(&wb[(nt * 16 + il) * MC2_LD + k0 + kc8]);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bv, acc[nt], 0, 0, 0);
    }
  }
  int om = mt * 64 + w * 16 + (lane >> 4) * 4;
  #pragma unroll
  for (int r = 0; r < 4; ++r)
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      int co = nt * 16 + il;
      float v = acc[nt][r] + b2[co];
      r2[(g * 64 + co) * 576 + om + r] = v > 0.f ? v : 0.f;
    }
}

#define MC2B_LD 584
// 32-row m-tiles (imc 37.4 KB -> 4 blocks/CU of 4 waves hide the staging
// latency that bound the 64-row form to ~340 us); the B operand streams
// from the pre-built global w2rotbf (18 16-B reads per lane, unrolled).
// Wave w: m-subtile (w & 1), ci-tile (w >> 1).
__global__ __launch_bounds__(256)
void k_conv2_bwd_x_mfma_mb_bf16(const float* __restrict__ dz2,
                                const __bf16* __restrict__ w2rotbf,
                                int bs, int K,
                                const float* __restrict__ a1,
                                float* __restrict__ dz1) {
  __shared__ __bf16 imc[32 * MC2B_LD];
  long long g = blockIdx.x / 22;
  int mt = blockIdx.x % 22;
  int k = (int)(g / bs);
  const float* dzb = dz2 + g * 36864;
  const __bf16* wtk = w2rotbf + (long long)k * 18432;
  for (int i = threadIdx.x; i < 32 * 576; i += 256) {
    int mr = i / 576, kk = i % 576;
    int m = mt * 32 + mr, p = m / 26, q = m % 26;
    int co = kk / 9, rem = kk % 9, kh = rem / 3, kw = rem % 3;
    int y = p - kh, x = q - kw;
    imc[mr * MC2B_LD + kk] =
        (__bf16)((m < 676 && y >= 0 && y < 24 && x >= 0 && x < 24)
                     ? dzb[co * 576 + y * 24 + x] : 0.f);
  }
  __syncthreads();
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int il = lane & 15, kc8 = (lane >> 4) * 8;
  int msub = w & 1, nt = w >> 1;
  f32x4 acc = {0, 0, 0, 0};
  #pragma unroll 3
  for (int k0 = 0; k0 < 576; k0 += 32) {
    bf16x8 a = ld_bf16x8(&imc[(msub * 16 + il) * MC2B_LD + k0 + kc8]);
    bf16x8 bv = ld_bf16x8(&wtk[(long long)(nt * 16 + il) * 576
                                 + k0 + kc8]);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bv, acc, 0, 0, 0);
  }
  int om = mt * 32 + msub * 16 + (lane >> 4) * 4;
  int ci = nt * 16 + il;
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (om + r >= 676) continue;
    long long o = (g * 32 + ci) * 676 + om + r;
    dz1[o] = a1[o] > 0.f ? acc[r] : 0.f;
  }
}

// block = 32 co-rows x 32 n-cols over K=576 (dzb16 37.4 KB + imt
// 37.4 KB -> 2 blocks/CU); grid = G * 2(co) * 9(n).  Wave w: co-subtile
// (w & 1), n-subtile (w >> 1).
__global__ __launch_bounds__(256)
void k_conv2_bwd_w_mfma_mb_bf16(const float* __restrict__ dz2,
                                const float* __restrict__ a1, int bs, int K,
                                float* __restrict__ slab) {
  __shared__ __bf16 dzb16[32 * MC2B_LD];
  __shared__ __bf16 imt[32 * MC2B_LD];
  int blk = blockIdx.x % 18;
  int ch = blk / 9;         // co half (0: rows 0-31, 1: rows 32-63)
  int nb = blk % 9;         // 32-col n-block
  long long g = blockIdx.x / 18;
  const float* dzb = dz2 + g * 36864 + (long long)ch * 32 * 576;
  const float* a1b = a1 + g * 21632;
  for (int i = threadIdx.x; i < 32 * 576; i += 256) {
    int co = i / 576;
    dzb16[co * MC2B_LD + (i % 576)] = (__bf16)dzb[i];
  }
  for (int i = threadIdx.x; i < 32 * 576; i += 256) {
    int nr = i / 576, o = i % 576;
    int n = nb * 32 + nr;
    int ci = n / 9, rem = n % 9, kh = rem / 3, kw = rem % 3;
    int yy = o / 24, xx = o % 24;
    imt[nr * MC2B_LD + o] = (__bf16)a1b[ci * 676 + (yy + kh) * 26 + xx + kw];
  }
  __syncthreads();
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int il = lane & 15, kc8 = (lane >> 4) * 8;
  int csub = w & 1, nt = w >> 1;
  f32x4 acc = {0, 0, 0, 0};
  #pragma unroll 3
  for (int k0 = 0; k0 < 576; k0 += 32) {
    bf16x8 a = ld_bf16x8(&dzb16[(csub * 16 + il) * MC2B_LD + k0 + kc8]);
    bf16x8 bv = ld_bf16x8(&imt[(nt * 16 + il) * MC2B_LD + k0 + kc8]);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bv, acc, 0, 0, 0);
  }
  float* out = slab + g * 18432;
  int orow = ch * 32 + csub * 16 + (lane >> 4) * 4;
  #pragma unroll
  for (int r = 0; r < 4; ++r)
    out[(orow + r) * 288 + nb * 32 + nt * 16 + il] = acc[r];
}

#define FC1B_SPLIT 36
#define FC1B_CH 256
#define FC1B_LD 264
__global__ __launch_bounds__(256)
void k_fc1_fwd_mfma_mb_bf16(const float* __restrict__ a2,
                            const float* __restrict__ params, long long P,
                            long long ow3, int bs, int K,
                            float* __restrict__ slab) {
  __shared__ __bf16 lw[128 * FC1B_LD];
  __shared__ __bf16 la[32 * FC1B_LD];
  int k = blockIdx.x / FC1B_SPLIT;
  int s = blockIdx.x % FC1B_SPLIT;
  int k_base = s * FC1B_CH;
  const float* w3 = params + (long long)k * P + ow3;
  const float* a2k = a2 + (long long)k * bs * 9216;
  for (int i = threadIdx.x; i < 128 * FC1B_CH; i += 256) {
    int row = i / FC1B_CH, kk = i % FC1B_CH;
    lw[row * FC1B_LD + kk] = (__bf16)w3[(long long)row * 9216 + k_base + kk];
  }
  for (int i = threadIdx.x; i < 32 * FC1B_CH; i += 256) {
    int bu = i / FC1B_CH, kk = i % FC1B_CH;
    la[bu * FC1B_LD + kk] =
        (__bf16)(bu < bs ? a2k[(long long)bu * 9216 + k_base + kk] : 0.f);
  }
  __syncthreads();
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int il = lane & 15, kc8 = (lane >> 4) * 8;
  f32x4 acc[2][2] = {{f32x4{0,0,0,0}, f32x4{0,0,0,0}},
                     {f32x4{0,0,0,0}, f32x4{0,0,0,0}}};
  for (int k0 = 0; k0 < FC1B_CH; k0 += 32) {
    bf16x8 a0 = ld_bf16x8(&lw[(w * 32 + il) * FC1B_LD + k0 + kc8]);
    bf16x8 a1v = ld_bf16x8(&lw[(w * 32 + 16 + il) * FC1B_LD + k0 + kc8]);
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      bf16x8 bv = ld_bf16x8(&la[(u * 16 + il) * FC1B_LD + k0 + kc8]);
      acc[0][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bv, acc[0][u], 0, 0, 0);
      acc[1][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1v, bv, acc[1][u], 0, 0, 0);
    }
  }
  float* slk = slab + (long long)k * FC1B_SPLIT * bs * 128;
  #pragma unroll
  for (int tt = 0; tt < 2; ++tt)
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      int bu = u * 16 + il;
      if (bu >= bs) continue;
      int j = w * 32 + tt * 16 + (lane >> 4) * 4;
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        slk[((long long)s * bs + bu) * 128 + j + r] = acc[tt][u][r];
    }
}

template <bool DEV>
__global__ __launch_bounds__(FC1R_BLK)
void k_fc1_fwd_reduce_mb_bf16(const float* __restrict__ slab,
                              const float* __restrict__ params, long long P,
                              long long ob3, int bs, int K, float p2,
                              const long long* __restrict__ seeds,
                              unsigned long long seed,
                              unsigned long long offset,
                              float* __restrict__ z3, float* __restrict__ a3,
                              unsigned char* __restrict__ m3) {
  fc1_reduce_stack<FC1B_SPLIT, DEV>(slab, params, P, ob3, bs, K, p2, seeds,
                                    seed, offset, z3, a3, m3);
}

// bf16 MFMA probe: one v_mfma_f32_16x16x32_bf16 with the documented
// fragment maps (A[i=l&15][k=(l>>4)*8+e], B[k=(l>>4)*8+e][j=l&15],
// D[row=(l>>4)*4+r][col=l&15]) — the numerics test pins the layout the
// bf16 kernels build on.
__global__ void k_mfma_bf16_probe(const __bf16* __restrict__ A,   // [16][32]
                                  const __bf16* __restrict__ B,   // [32][16]
                                  float* __restrict__ D) {        // [16][16]
  int l = threadIdx.x;
  bf16x8 a, b;
  #pragma unroll
  for (int e = 0; e < 8; ++e) {
    int k = (l >> 4) * 8 + e;
    a[e] = A[(l & 15) * 32 + k];
    b[e] = B[k * 16 + (l & 15)];
  }
  f32x4 acc = {0, 0, 0, 0};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  #pragma unroll
  for (int r = 0; r < 4; ++r)
    D[((l >> 4) * 4 + r) * 16 + (l & 15)] = acc[r];
}


// ---------------------------------------------------------------------------
// ONE batch-step, shared by both drivers: the launches from the gather
// through conv1's backward, for K clients of bs rows each (G = K*bs).  The
// per-client epoch calls it with K = 1, bs := this batch's row count and
// its arena as the stack; the mega round with (K, bs, t).  `meta` says who
// is in the step (StepMetaDev / StepMetaOne), t keys the dropout streams,
// and the gather zeroes the n_acc doubles at `acc` for the caller's clip
// tail.
// ---------------------------------------------------------------------------

// CNN_EPOCH_DEBUG=1: synchronize + check after every launch so a device
// fault names the kernel that raised it (diagnostics only — the hot path
// never syncs)
static bool epoch_dbg() {
  static const bool on = getenv("CNN_EPOCH_DEBUG") != nullptr;
  return on;
}
#define EPOCH_CHK(name, t, bs)                                             \
  do {                                                                     \
    if (epoch_dbg()) {                                                     \
      hipError_t e_ = hipStreamSynchronize(s);                             \
      hipError_t e2_ = hipGetLastError();                                  \
      if (e_ != hipSuccess || e2_ != hipSuccess) {                         \
        fprintf(stderr, "cnn_step fault after %s (t=%d bs=%d): %s / %s\n", \
                name, t, bs, hipGetErrorString(e_),                        \
                hipGetErrorString(e2_));                                   \
        fflush(stderr);                                                    \
        abort();                                                           \
      }                                                                    \
    }                                                                      \
  } while (0)

template <typename Meta>
static void cnn_step(const float* shard_x, const long long* shard_y,
                     const long long* orders, const Meta& meta, int t,
                     int K, int bs, int C, float* params, float* grads,
                     const CnnWorkspace& ws, double* acc, int n_acc,
                     float p1, float p2, float* loss_out, int use_bf16,
                     hipStream_t s) {
  CnnOffsets o = cnn_offsets(C);
  long long P = o.total;
  int G = K * bs;
  // grid of `blk`-thread blocks covering per_row elements of each of G rows
  auto blocks = [G](long long per_row, int blk) {
    return dim3((int)((G * per_row + blk - 1) / blk));
  };
  static_assert(18432 % FBLK == 0, "w2_grid: whole blocks per client");
  dim3 w2_grid(K * (18432 / FBLK));  // one thread per W2 element
  unsigned long long off = (unsigned long long)t;  // Philox batch offset
#define STEP(kernel, grid, block, shmem, ...)                              \
  hipLaunchKernelGGL(kernel, grid, block, shmem, s, __VA_ARGS__);          \
  EPOCH_CHK(#kernel, t, bs)
  STEP(k_gather_mb<Meta>, blocks(784, FBLK), dim3(FBLK), 0, shard_x, shard_y,
       orders, meta, bs, K, ws.xb, ws.yb, acc, n_acc);
  STEP(k_conv1_fwd_mb, blocks(21632, FBLK), dim3(FBLK), 0, ws.xb, params,
       P, o.w1, o.b1, bs, K, ws.a1);
  if (use_bf16) {
    // bf16 kernels read w2 directly (LDS staging converts); bwd-data
    // wants its own [ci][k'] bf16 layout, which fits in ws.w2rot
    STEP(k_w2rotbf_mb, w2_grid, dim3(FBLK), 0, params, P, o.w2, K,
         reinterpret_cast<__bf16*>(ws.w2rot));
    STEP(k_conv2_fwd_mfma_mb_bf16, dim3(G * 9), dim3(FBLK), 0, ws.a1, params,
         P, o.w2, o.b2, bs, K, ws.r2);
    STEP(k_pool_drop_fwd_mb<Meta>, blocks(9216, FBLK), dim3(FBLK), 0, ws.r2,
         bs, K, p1, meta, off, ws.a2, ws.pidx, ws.m2);
    STEP(k_fc1_fwd_mfma_mb_bf16, dim3(K * FC1B_SPLIT), dim3(FBLK), 0, ws.a2,
         params, P, o.w3, bs, K, ws.wsl);
    STEP(k_fc1_fwd_reduce_mb_bf16<Meta::DEV>, blocks(128, FC1R_BLK),
         dim3(FC1R_BLK), 0, ws.wsl, params, P, o.b3, bs, K, p2, meta.seeds,
         meta.seed, off, ws.z3, ws.a3, ws.m3);
  } else {
    STEP(k_w2_layouts_mb, w2_grid, dim3(FBLK), 0, params, P, o.w2, K, ws.w2t,
         ws.w2rot);
    // conv2 + pool + dropout in one kernel: no r2 on the fp32 path
    STEP(k_conv2_fwd_pool_mfma_mb<Meta>, dim3(G * C2F_SLABS), dim3(FBLK), 0,
         ws.a1, ws.w2t, params, P, o.b2, bs, K, p1, meta, off, ws.a2,
         ws.pidx, ws.m2);
    STEP(k_fc1_fwd_mfma_mb, dim3(K * FC1_SPLIT), dim3(FBLK), 0, ws.a2,
         params, P, o.w3, bs, K, ws.wsl);
    STEP(k_fc1_fwd_reduce_mb<Meta::DEV>, blocks(128, FC1R_BLK),
         dim3(FC1R_BLK), 0, ws.wsl, params, P, o.b3, bs, K, p2, meta.seeds,
         meta.seed, off, ws.z3, ws.a3, ws.m3);
  }
  STEP(k_fc2_loss_fwd_mb<Meta>, dim3(G), dim3(FBLK), C * (int)sizeof(float),
       ws.a3, params, P, o.w4, o.b4, meta, bs, K, C, ws.yb, ws.dlogits,
       loss_out, ws.z3, ws.m3, p2, ws.dz3);
  STEP(k_fc2_bwd_w_mb, dim3(K * ((C * 128 + FBLK - 1) / FBLK)), dim3(FBLK), 0,
       ws.dlogits, ws.a3, grads, P, o.w4, o.b4, bs, K, C);
  STEP(k_fc1_bwd_w_mfma_mb, dim3(K * 144), dim3(FBLK), 0, ws.dz3, ws.a2,
       grads, P, o.w3, grads, P, o.b3, bs, K);
  STEP(k_fc1_bwd_x_mfma_mb, dim3(K * FC1X_BLKS), dim3(64 * FC1X_WAVES), 0,
       ws.dz3, params, P, o.w3, bs, K, ws.da2);
  STEP(k_pool_drop_bwd_bias_mb, dim3(K * 64), dim3(FBLK), 0, ws.da2, ws.pidx,
       ws.m2, bs, K, p1, ws.dz2, grads, P, o.b2);
  if (use_bf16) {
    STEP(k_conv2_bwd_w_mfma_mb_bf16, dim3(18 * G), dim3(FBLK), 0, ws.dz2,
         ws.a1, bs, K, ws.wsl);
  } else {
    STEP(k_conv2_bwd_w_mfma_mb, dim3(9 * G), dim3(128), 0, ws.dz2, ws.a1, bs,
         K, ws.wsl);
  }
  STEP(k_conv2_bwd_w_fold_mb, w2_grid, dim3(FBLK), 0, ws.wsl, grads, P, o.w2,
       bs, K);
  if (use_bf16) {
    STEP(k_conv2_bwd_x_mfma_mb_bf16, dim3(G * 22), dim3(FBLK), 0, ws.dz2,
         reinterpret_cast<const __bf16*>(ws.w2rot), bs, K, ws.a1, ws.dz1);
  } else {
    STEP(k_conv2_bwd_x_mfma_mb, dim3(G * C2X_BLKS), dim3(FBLK), 0, ws.dz2,
         ws.w2rot, ws.a1, bs, K, ws.dz1);
  }
  STEP(k_conv1_bwd_w_mb, dim3(K * 32), dim3(1024), 0, ws.xb, ws.dz1, grads,
       P, o.w1, o.b1, bs, K);
#undef STEP
}

// ---------------------------------------------------------------------------
// per-client epoch driver: loops every batch of ONE client's local epoch:
// cnn_step at K = 1 (bs := this batch's row count, the client's arena as
// the stack) + clip-stats + SGD via flat_ops.hip.
// ---------------------------------------------------------------------------
extern "C" void launch_cnn_epoch(
    const float* shard_x, const long long* shard_y, const long long* order,
    long long n, int bs, int C, float* params, float* grads,
    CnnWorkspace ws, const float* lr_t, float max_norm, float p1, float p2,
    float* stats_acc, float* loss_acc, unsigned long long seed,
    hipStream_t s, long long row_base, int use_bf16,
    const float* server_params, float mu) {
  long long P = cnn_offsets(C).total;
  const int K = 1;
  const bool prox = mu > 0.f;
  int n_batches = (int)((n + bs - 1) / bs);
  for (int it = 0; it < n_batches; ++it) {
    long long start = (long long)it * bs;
    int B = (int)((start + bs <= n) ? bs : (n - start));
    // the gather zeroes what this step's clip tail accumulates into
    cnn_step(shard_x, shard_y, order, StepMetaOne{row_base, start, B, seed},
             it, K, B, C, params, grads, ws,
             prox ? ws.red_partials : ws.red_acc, prox ? 3 : 2, p1, p2,
             loss_acc, use_bf16, s);
    if (prox) {
      // FedProx: the PROX pair at K = 1, every step active; forms
      // g + mu (w - w_g) in registers and adds the regulariser to loss_acc
      ProxArgs px{params, K, server_params, mu, nullptr, 0, 0, nullptr,
                  loss_acc};
      int blocks_per_k = (int)((P + SUMSQ_CHUNK - 1) / SUMSQ_CHUNK);
      hipLaunchKernelGGL(k_sumsq_mb<ProxArgs>, dim3(blocks_per_k),
                         dim3(FBLK), 0, s, grads, P, blocks_per_k,
                         ws.red_partials, px);
      EPOCH_CHK("k_sumsq_mb<ProxArgs>", it, B);
      int gkp = (int)((P + FBLK - 1) / FBLK); if (gkp > 4096) gkp = 4096;
      hipLaunchKernelGGL((k_clip_sgd_mb<false, ProxArgs>), dim3(gkp),
                         dim3(FBLK), 0, s, params, grads, P, K,
                         ws.red_partials, max_norm, 1e-6f, lr_t, stats_acc,
                         px);
      EPOCH_CHK("k_clip_sgd_mb<ProxArgs>", it, B);
      continue;
    }
    // fused clip + sufficient stats + SGD on the whole arena
    launch_sum_sumsq2(grads, P, ws.red_partials, ws.red_acc, s);
    EPOCH_CHK("launch_sum_sumsq2", it, B);
    launch_clip_apply_stats(grads, P, ws.red_acc, max_norm, 1e-6f,
                            stats_acc, s);
    EPOCH_CHK("launch_clip_apply_stats", it, B);
    launch_sgd_step(params, grads, nullptr, 0.f, lr_t, 0.f, 0.f, 0.f, 0, 0,
                    P, s);
    EPOCH_CHK("launch_sgd_step", it, B);
  }
}

// ---------------------------------------------------------------------------
// per-client WHOLE-ROUND driver: trains K clients back-to-back in one
// host call — per client: copy-in server weights, run the fused epoch,
// write the weighted pseudo-gradient, accumulate into the round buffer.
// Per-client losses/stats land in slots of loss_out[K] / stats_out[K*2].
// ---------------------------------------------------------------------------
extern "C" void launch_cnn_round(
    const float* shard_x, const long long* shard_y, const long long* orders,
    const long long* row_bases, const long long* order_offs,
    const long long* counts, const float* weights,
    const unsigned long long* seeds, int K, int bs, int C,
    const float* server_params, float* params, float* grads,
    float* round_accum, CnnWorkspace ws, const float* lr_t, float max_norm,
    float p1, float p2, float* stats_out, float* loss_out,
    hipStream_t s, int use_bf16, float mu) {
  CnnOffsets o = cnn_offsets(C);
  int gp = (int)((o.total + FBLK - 1) / FBLK);
  if (gp > 2048) gp = 2048;
  for (int k = 0; k < K; ++k) {
    hipLaunchKernelGGL(k_copy, dim3(gp), dim3(FBLK), 0, s,
                       params, server_params, o.total);
    launch_cnn_epoch(shard_x, shard_y, orders + order_offs[k], counts[k],
                     bs, C, params, grads, ws, lr_t, max_norm, p1, p2,
                     stats_out + 2 * k, loss_out + k, seeds[k], s,
                     row_bases[k], use_bf16, server_params, mu);
    hipLaunchKernelGGL(k_cnn_pseudo_grad, dim3(gp), dim3(FBLK), 0, s,
                       grads, server_params, params, weights[k], o.total);
    hipLaunchKernelGGL(k_cnn_axpy, dim3(gp), dim3(FBLK), 0, s,
                       round_accum, grads, o.total);
  }
}

// ---------------------------------------------------------------------------
// mega driver: one launch set per batch-step for ALL K clients
// ---------------------------------------------------------------------------
extern "C" void launch_cnn_round_mega(
    const float* shard_x, const long long* shard_y,
    const long long* orders_dev,
    const long long* row_bases_dev, const long long* order_offs_dev,
    const long long* counts_dev, const long long* counts_host,
    const float* weights_dev, const long long* seeds_dev,
    int K, int bs, int C,
    const float* server_params, float* params_stack, float* grads_stack,
    float* round_accum, CnnWorkspace ws, double* acc2k,
    const float* lr_t, float max_norm, float p1, float p2,
    float* stats_out, float* loss_out, hipStream_t s, int use_bf16,
    float mu, const DgaArgs* dga, double* dga_out) {
  long long P = cnn_offsets(C).total;
  const bool prox = mu > 0.f;  // FedProx: acc2k holds 3K doubles
  int max_batches = 0;
  for (int k = 0; k < K; ++k) {
    int nb = (int)((counts_host[k] + bs - 1) / bs);
    if (nb > max_batches) max_batches = nb;
  }
  long long kp = (long long)K * P;
  int gkp = (int)((kp + FBLK - 1) / FBLK); if (gkp > 4096) gkp = 4096;
  int gp = (int)((P + FBLK - 1) / FBLK); if (gp > 2048) gp = 2048;
  hipLaunchKernelGGL(k_copy_stack, dim3(gkp), dim3(FBLK), 0, s,
                     params_stack, server_params, P, K);
  for (int t = 0; t < max_batches; ++t) {
    cnn_step(shard_x, shard_y, orders_dev,
             StepMetaDev{row_bases_dev, order_offs_dev, counts_dev, seeds_dev,
                         t},
             t, K, bs, C, params_stack, grads_stack, ws, acc2k,
             prox ? 3 * K : 2 * K, p1, p2, loss_out, use_bf16, s);
    // acc2k was zeroed by this step's k_gather_mb
    int blocks_per_k = (int)((P + SUMSQ_CHUNK - 1) / SUMSQ_CHUNK);
    if (prox) {
      // same two dispatches; idle clients (t * bs >= counts[k]) get no
      // proximal term and no regulariser
      ProxArgs px{params_stack, K, server_params, mu, counts_dev, t, bs,
                  nullptr, loss_out};
      hipLaunchKernelGGL(k_sumsq_mb<ProxArgs>, dim3(K * blocks_per_k),
                         dim3(FBLK), 0, s, grads_stack, P, blocks_per_k,
                         acc2k, px);
      hipLaunchKernelGGL((k_clip_sgd_mb<false, ProxArgs>), dim3(gkp),
                         dim3(FBLK), 0, s, params_stack, grads_stack, P, K,
                         acc2k, max_norm, 1e-6f, lr_t, stats_out, px);
      continue;
    }
    hipLaunchKernelGGL(k_sumsq_mb<NoProx>, dim3(K * blocks_per_k),
                       dim3(FBLK), 0, s, grads_stack, P, blocks_per_k, acc2k,
                       NoProx{});
    hipLaunchKernelGGL((k_clip_sgd_mb<false, NoProx>), dim3(gkp), dim3(FBLK),
                       0, s, params_stack, grads_stack, P, K, acc2k, max_norm,
                       1e-6f, lr_t, stats_out, NoProx{});
  }
  if (dga) {
    dga_tail(params_stack, server_params, P, K, loss_out, stats_out,
             counts_dev, bs, *dga, round_accum, dga_out, s);
    return;
  }
  hipLaunchKernelGGL(k_pseudo_grad_mb, dim3(gkp), dim3(FBLK), 0, s,
                     grads_stack, server_params, params_stack, weights_dev,
                     P, K);
  hipLaunchKernelGGL(k_accum_mb, dim3(gp), dim3(FBLK), 0, s,
                     round_accum, grads_stack, P, K);
}


// ---------------------------------------------------------------------------
// standalone entries for K-stacked flat arenas (reused by the
// Shakespeare mega round's graph-captured epoch): per-client clip +
// stats + SGD, and weighted pseudo-grad + deterministic accumulate.
// ---------------------------------------------------------------------------
extern "C" void launch_mega_clip_sgd(float* params_stack, float* grads_stack,
                                     long long P, int K, double* acc2k,
                                     float max_norm, const float* lr_t,
                                     float* stats_out, hipStream_t s,
                                     const float* server, float mu,
                                     const unsigned char* active,
                                     float* loss_out) {
  int blocks_per_k = (int)((P + SUMSQ_CHUNK - 1) / SUMSQ_CHUNK);
  long long kp = (long long)K * P;
  int gkp = (int)((kp + FBLK - 1) / FBLK); if (gkp > 4096) gkp = 4096;
  if (mu > 0.f) {
    // FedProx: acc2k holds 3K doubles; the stored gradient is scale * gp
    ProxArgs px{params_stack, K, server, mu, nullptr, 0, 0, active,
                loss_out};
    hipMemsetAsync(acc2k, 0, 3 * K * sizeof(double), s);
    hipLaunchKernelGGL(k_sumsq_mb<ProxArgs>, dim3(K * blocks_per_k),
                       dim3(FBLK), 0, s, grads_stack, P, blocks_per_k, acc2k,
                       px);
    hipLaunchKernelGGL((k_clip_sgd_mb<true, ProxArgs>), dim3(gkp),
                       dim3(FBLK), 0, s, params_stack, grads_stack, P, K,
                       acc2k, max_norm, 1e-6f, lr_t, stats_out, px);
    return;
  }
  hipMemsetAsync(acc2k, 0, 2 * K * sizeof(double), s);
  hipLaunchKernelGGL(k_sumsq_mb<NoProx>, dim3(K * blocks_per_k), dim3(FBLK),
                     0, s, grads_stack, P, blocks_per_k, acc2k, NoProx{});
  hipLaunchKernelGGL((k_clip_sgd_mb<true, NoProx>), dim3(gkp), dim3(FBLK), 0,
                     s, params_stack, grads_stack, P, K, acc2k, max_norm,
                     1e-6f, lr_t, stats_out, NoProx{});
}

extern "C" void launch_mega_pseudo_accum(float* grads_stack,
                                         const float* server,
                                         const float* params_stack,
                                         const float* weights_dev,
                                         float* round_accum, long long P,
                                         int K, hipStream_t s) {
  long long kp = (long long)K * P;
  int gkp = (int)((kp + FBLK - 1) / FBLK); if (gkp > 4096) gkp = 4096;
  int gp = (int)((P + FBLK - 1) / FBLK); if (gp > 2048) gp = 2048;
  hipLaunchKernelGGL(k_pseudo_grad_mb, dim3(gkp), dim3(FBLK), 0, s,
                     grads_stack, server, params_stack, weights_dev, P, K);
  hipLaunchKernelGGL(k_accum_mb, dim3(gp), dim3(FBLK), 0, s,
                     round_accum, grads_stack, P, K);
}

extern "C" void launch_mega_dga_accum(const float* params_stack,
                                      const float* server, long long P, int K,
                                      const float* loss_out,
                                      const float* stats_out,
                                      const long long* counts_dev, int bs,
                                      DgaArgs dga, float* round_accum,
                                      double* dga_out, hipStream_t s) {
  dga_tail(params_stack, server, P, K, loss_out, stats_out, counts_dev, bs,
           dga, round_accum, dga_out, s);
}

// ---------------------------------------------------------------------------
// debug/test launchers for the MFMA kernels (numerics tests call these
// one-by-one against torch references — tests/test_mfma_gpu.py,
// tests/test_bf16_gpu.py).  An operand that arrives as its own K-stack
// is passed as the parameter stack with its own length as the stride P
// and offset 0.
// ---------------------------------------------------------------------------
#define W2N 18432LL
#define W3N 1179648LL

extern "C" {
void launch_w2_layouts(const float* w2, int K, float* w2t, float* w2rot,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_w2_layouts_mb, dim3((K * 18432 + FBLK - 1) / FBLK),
                     dim3(FBLK), 0, s, w2, W2N, 0LL, K, w2t, w2rot);
}
void launch_conv2_fwd_mfma(const float* a1, const float* w2t, const float* b2,
                           int bs, int K, float* r2, hipStream_t s) {
  hipLaunchKernelGGL(k_conv2_fwd_mfma_mb, dim3(K * bs * C2F_SLABS),
                     dim3(FBLK), 0, s, a1, w2t, b2, 64LL, 0LL, bs, K, r2);
}
void launch_conv2_fwd_pool_mfma(const float* a1, const float* w2t,
                                const float* b2, int bs, int K, float p1,
                                const long long* seeds_dev,
                                unsigned long long offset, float* a2,
                                unsigned char* pidx, unsigned char* m2,
                                hipStream_t s) {
  hipLaunchKernelGGL(k_conv2_fwd_pool_mfma_mb<StepMetaDev>,
                     dim3(K * bs * C2F_SLABS), dim3(FBLK), 0, s, a1, w2t, b2,
                     64LL, 0LL, bs, K, p1,
                     StepMetaDev{nullptr, nullptr, nullptr, seeds_dev, 0},
                     offset, a2, pidx, m2);
}
void launch_pool_drop_bwd_bias(const float* da2, const unsigned char* pidx,
                               const unsigned char* m2, int bs, int K,
                               float p1, float* dz2, float* db2,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_pool_drop_bwd_bias_mb, dim3(K * 64), dim3(FBLK), 0, s,
                     da2, pidx, m2, bs, K, p1, dz2, db2, 64LL, 0LL);
}
void launch_conv2_bwd_x_mfma(const float* dz2, const float* w2rot,
                             const float* a1, int bs, int K, float* dz1,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_conv2_bwd_x_mfma_mb, dim3(K * bs * C2X_BLKS),
                     dim3(FBLK), 0, s, dz2, w2rot, a1, bs, K, dz1);
}
static void conv2_bwd_w_tail(const float* dz2, const float* slab, int bs,
                             int K, float* dw2, float* db2, hipStream_t s) {
  hipLaunchKernelGGL(k_conv2_bwd_w_fold_mb,
                     dim3(K * ((18432 + FBLK - 1) / FBLK)), dim3(FBLK), 0, s,
                     slab, dw2, W2N, 0LL, bs, K);
  hipLaunchKernelGGL(k_conv2_bwd_b_mb, dim3(K * 64), dim3(FBLK), 0, s,
                     dz2, db2, 64LL, 0LL, bs, K);
}
void launch_conv2_bwd_w_mfma(const float* dz2, const float* a1, int bs, int K,
                             float* slab, float* dw2, float* db2,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_conv2_bwd_w_mfma_mb, dim3(9 * K * bs), dim3(128), 0,
                     s, dz2, a1, bs, K, slab);
  conv2_bwd_w_tail(dz2, slab, bs, K, dw2, db2, s);
}
// the seed arrives by value (the fold's DEV = false form): every client
// draws from the same seed
void launch_fc1_fwd_mfma(const float* a2, const float* w3, const float* b3,
                         int bs, int K, float p2, unsigned long long seed,
                         unsigned long long offset, float* slab, float* z3,
                         float* a3, unsigned char* m3, hipStream_t s) {
  hipLaunchKernelGGL(k_fc1_fwd_mfma_mb, dim3(K * FC1_SPLIT), dim3(FBLK), 0, s,
                     a2, w3, W3N, 0LL, bs, K, slab);
  hipLaunchKernelGGL(k_fc1_fwd_reduce_mb<false>,
                     dim3((K * bs * 128 + FC1R_BLK - 1) / FC1R_BLK),
                     dim3(FC1R_BLK), 0, s, slab, b3, 128LL, 0LL, bs, K, p2,
                     nullptr, seed, offset, z3, a3, m3);
}
void launch_fc1_bwd_w_mfma(const float* dz3, const float* a2, int bs, int K,
                           float* dw3, float* db3, hipStream_t s) {
  hipLaunchKernelGGL(k_fc1_bwd_w_mfma_mb, dim3(K * 144), dim3(FBLK), 0, s,
                     dz3, a2, dw3, W3N, 0LL, db3, 128LL, 0LL, bs, K);
}
void launch_fc1_bwd_x_mfma(const float* dz3, const float* w3, int bs, int K,
                           float* da2, hipStream_t s) {
  hipLaunchKernelGGL(k_fc1_bwd_x_mfma_mb, dim3(K * FC1X_BLKS),
                     dim3(64 * FC1X_WAVES), 0, s,
                     dz3, w3, W3N, 0LL, bs, K, da2);
}
void launch_mfma_bf16_probe(const void* A, const void* B, float* D,
                            hipStream_t s) {
  hipLaunchKernelGGL(k_mfma_bf16_probe, dim3(1), dim3(64), 0, s,
                     (const __bf16*)A, (const __bf16*)B, D);
}
void launch_fc1_fwd_mfma_bf16(const float* a2, const float* w3,
                              const float* b3, int bs, int K, float p2,
                              unsigned long long seed,
                              unsigned long long offset, float* slab,
                              float* z3, float* a3, unsigned char* m3,
                              hipStream_t s) {
  hipLaunchKernelGGL(k_fc1_fwd_mfma_mb_bf16, dim3(K * FC1B_SPLIT), dim3(FBLK),
                     0, s, a2, w3, W3N, 0LL, bs, K, slab);
  hipLaunchKernelGGL(k_fc1_fwd_reduce_mb_bf16<false>,
                     dim3((K * bs * 128 + FC1R_BLK - 1) / FC1R_BLK),
                     dim3(FC1R_BLK), 0, s, slab, b3, 128LL, 0LL, bs, K, p2,
                     nullptr, seed, offset, z3, a3, m3);
}
// this kernel reads w2 and b2 through ONE stack pointer: w2b2 is K blocks
// of [w2 (18432) | b2 (64)]
void launch_conv2_fwd_mfma_bf16(const float* a1, const float* w2b2, int bs,
                                int K, float* r2, hipStream_t s) {
  hipLaunchKernelGGL(k_conv2_fwd_mfma_mb_bf16, dim3(K * bs * 9), dim3(FBLK),
                     0, s, a1, w2b2, W2N + 64, 0LL, W2N, bs, K, r2);
}
void launch_conv2_bwd_x_mfma_bf16(const float* dz2, const float* w2,
                                  const float* a1, int bs, int K,
                                  float* w2rotbf, float* dz1, hipStream_t s) {
  hipLaunchKernelGGL(k_w2rotbf_mb, dim3((K * 18432 + FBLK - 1) / FBLK),
                     dim3(FBLK), 0, s, w2, W2N, 0LL, K,
                     reinterpret_cast<__bf16*>(w2rotbf));
  hipLaunchKernelGGL(k_conv2_bwd_x_mfma_mb_bf16, dim3(K * bs * 22),
                     dim3(FBLK), 0, s, dz2,
                     reinterpret_cast<const __bf16*>(w2rotbf), bs, K, a1,
                     dz1);
}
void launch_conv2_bwd_w_mfma_bf16(const float* dz2, const float* a1, int bs,
                                  int K, float* slab, float* dw2, float* db2,
                                  hipStream_t s) {
  hipLaunchKernelGGL(k_conv2_bwd_w_mfma_mb_bf16, dim3(18 * K * bs),
                     dim3(FBLK), 0, s, dz2, a1, bs, K, slab);
  conv2_bwd_w_tail(dz2, slab, bs, K, dw2, db2, s);
}
}  // extern "C"
