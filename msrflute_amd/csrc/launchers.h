// Host-side declarations shared by bindings.cpp and every .hip file that
// defines or calls a launcher: the CNN workspace struct, the flat-arena
// offsets of the CNN and the prototype of every extern "C" launcher.
// Each definition includes this header, so a signature that disagrees
// with its declaration fails to compile instead of corrupting a call.
#pragma once

#include <hip/hip_runtime.h>

// arena offsets (fp32 indices) of the CNN-FEMNIST parameters for C classes
struct CnnOffsets {
  long long w1, b1, w2, b2, w3, b3, w4, b4, total;
};

inline CnnOffsets cnn_offsets(int C) {
  CnnOffsets o;
  o.w1 = 0;               // [32,1,3,3]
  o.b1 = o.w1 + 288;      // [32]
  o.w2 = o.b1 + 32;       // [64,32,3,3]
  o.b2 = o.w2 + 18432;    // [64]
  o.w3 = o.b2 + 64;       // [128,9216]
  o.b3 = o.w3 + 1179648;  // [128]
  o.w4 = o.b3 + 128;      // [C,128]
  o.b4 = o.w4 + (long long)C * 128;  // [C]
  o.total = o.b4 + C;
  return o;
}

// Output rows per block of the f32 conv2 forward kernel: slab s of an
// image covers output rows [s*ROWS, (s+1)*ROWS), so rows ROWS, 2*ROWS, ..
// are the seams between blocks.  Exported as _C.CONV2_FWD_SLAB_ROWS.
#define CONV2_FWD_SLAB_ROWS 4

// CNN workspace of G = K * bs rows over K clients (K = 1: the per-client
// drivers), laid out inside the caller's buffers by the one slicer in
// bindings.cpp
struct CnnWorkspace {
  float *xb, *a1, *r2, *a2, *z3, *a3, *dlogits, *dz3, *da2, *dz2, *dz1;
  float *wsl;  // split-K partial slab (G*18432 floats), shared fwd/bwd
  float *w2t, *w2rot;  // per-step W2 fragment layouts (K*18432 floats each)
  int *yb;             // G labels, -1 = inactive row
  unsigned char *pidx, *m2, *m3;
  // K = 1 drivers only (their bindings set these): the two-stage
  // launch_sum_sumsq2 partials and its 2-double result
  double *red_partials, *red_acc;
};

// element counts of that workspace: what the slicer checks and what the
// Python drivers allocate (_C.cnn_workspace_sizes)
struct CnnWorkspaceSizes {
  long long n_float, n_int, n_byte;
};

inline CnnWorkspaceSizes cnn_workspace_sizes(long long G, long long K,
                                             long long C) {
  CnnWorkspaceSizes z;
  z.n_float = G * (784 + 2 * 21632 + 2 * 36864 + 2 * 9216 + 3 * 128 + 18432
                   + C) + K * 2 * 18432;
  z.n_int = G;
  z.n_byte = G * (2 * 9216 + 128);
  return z;
}

// DGA end-of-round tail (k_dga_normsq_mb / k_dga_accum_mb): how client
// k's aggregation weight is formed on the device.  ``mode`` selects
// server_config.weight_train_loss; DGA_MEAN is aggregate_median: mean
// (weight 1).  ``clip`` is local DP in clip-only mode (eps < 0).
enum DgaMode { DGA_MEAN = 0, DGA_TRAIN_LOSS = 1, DGA_MAG_VAR = 2,
               DGA_MAG_MEAN = 3, DGA_MAG = 4 };
#define DGA_MAX_K 32
struct DgaArgs {
  int mode;
  int clip;
  double beta;      // softmax_beta
  double max_grad;  // dp_config.max_grad (clip only)
};

extern "C" {

// flat_ops.hip
void launch_pseudo_grad(float* out, const float* ws, const float* wt,
                        float weight, long long n, hipStream_t s);
void launch_axpy(float* y, const float* x, float alpha, long long n,
                 hipStream_t s);
void launch_scale(float* x, float alpha, long long n, hipStream_t s);
void launch_sum_sumsq(const float* x, long long n, double* out2,
                      hipStream_t s);
void launch_sum_sumsq2(const float* x, long long n, double* partials,
                       double* out2, hipStream_t s);
int sum_sumsq2_partials(long long n);
void launch_clip_apply(float* x, long long n, const double* out2,
                       float max_norm, float eps, float* norm_out,
                       hipStream_t s);
void launch_add_gaussian_noise(float* x, long long n, float sigma,
                               unsigned long long seed,
                               unsigned long long offset, hipStream_t s);
void launch_sgd_step(float* p, const float* g, float* buf, float lr,
                     const float* lr_ptr, float momentum, float dampening,
                     float weight_decay, int nesterov, int first_step,
                     long long n, hipStream_t s);
void launch_clip_apply_stats(float* x, long long n, const double* out2,
                             float max_norm, float eps, float* stats_acc,
                             hipStream_t s);
void launch_adam_step(float* p, const float* g, float* m, float* v,
                      float* vmax, float lr, float beta1, float beta2,
                      float eps, float weight_decay, float bc1, float bc2,
                      int amsgrad, int adamw, long long n, hipStream_t s);
void launch_adamax_step(float* p, const float* g, float* m, float* u,
                        float lr, float beta1, float beta2, float eps,
                        float weight_decay, float bc1, long long n,
                        hipStream_t s);
void launch_segmented_sqnorm(const float* x, const long long* offs,
                             int n_segs, double* out, hipStream_t s);
void launch_quant_bin_mask(float* x, long long n, const float* min_t,
                           const float* max_t, const float* thresh_t,
                           int n_bins, hipStream_t s);
void launch_gru_gates(const float* g_i, const float* g_h, const float* h,
                      float* out, int B, int H, hipStream_t s);

// lstm_seq.hip — K-stacked packed W_hh; row r of the R rows belongs to
// client r / rows_per_client (K = 1, rows_per_client = R: one model)
void launch_lstm_seq_fwd(const float* xp, const float* w_hh_t_stack,
                         float* h_seq, float* gates, float* c_seq, int R,
                         int rows_per_client, int T, hipStream_t s);
void launch_lstm_seq_bwd(const float* gates, const float* c_seq,
                         const float* w_hh_stack, const float* dh_out,
                         float* dg_pre, int R, int rows_per_client, int T,
                         hipStream_t s);
// the same kernels on bf16-stored W_hh (8 k's per 16-byte group,
// ops/lstm._pack_fwd_bf16 / _pack_bwd_bf16); all arithmetic stays fp32
void launch_lstm_seq_fwd_bf16(const float* xp,
                              const unsigned short* w_hh_t_stack,
                              float* h_seq, float* gates, float* c_seq,
                              int R, int rows_per_client, int T,
                              hipStream_t s);
void launch_lstm_seq_bwd_bf16(const float* gates, const float* c_seq,
                              const unsigned short* w_hh_stack,
                              const float* dh_out, float* dg_pre, int R,
                              int rows_per_client, int T, hipStream_t s);

// gru_seq.hip
void launch_gru_seq_fwd(const float* gi, const float* whh_t,
                        const float* b_hh, float* h_seq, float* gates,
                        float* ghn, int B, int T, hipStream_t s);
void launch_gru_seq_bwd(const float* gates, const float* ghn,
                        const float* h_seq, const float* w_hh,
                        const float* dh_out, float* dgi, float* dgh,
                        int B, int T, hipStream_t s);

// fused_cnn.hip — drivers.  mu > 0 (FedProx) makes the clip/SGD tail of
// every step use g + mu (w - server) and adds 0.5 mu ||w - server||^2 to
// the step's loss, for the clients active at that step; mu == 0 launches
// exactly the FedAvg kernels.
void launch_cnn_epoch(
    const float* shard_x, const long long* shard_y, const long long* order,
    long long n, int bs, int C, float* params, float* grads,
    CnnWorkspace ws, const float* lr_t, float max_norm, float p1, float p2,
    float* stats_acc, float* loss_acc, unsigned long long seed,
    hipStream_t s, long long row_base, int use_bf16,
    const float* server_params, float mu);
void launch_cnn_round(
    const float* shard_x, const long long* shard_y,
    const long long* orders,            // concatenated per-client shuffles
    const long long* row_bases,         // HOST: K shard row offsets
    const long long* order_offs,        // HOST: K offsets into `orders`
    const long long* counts,            // HOST: K sample counts
    const float* weights,               // HOST: K aggregation weights
    const unsigned long long* seeds,    // HOST: K dropout seeds
    int K, int bs, int C,
    const float* server_params, float* params, float* grads,
    float* round_accum, CnnWorkspace ws, const float* lr_t, float max_norm,
    float p1, float p2, float* stats_out, float* loss_out,
    hipStream_t s, int use_bf16, float mu);
void launch_cnn_round_mega(
    const float* shard_x, const long long* shard_y,
    const long long* orders_dev,
    const long long* row_bases_dev, const long long* order_offs_dev,
    const long long* counts_dev, const long long* counts_host,
    const float* weights_dev, const long long* seeds_dev,
    int K, int bs, int C,
    const float* server_params, float* params_stack, float* grads_stack,
    float* round_accum, CnnWorkspace ws,
    double* acc2k,                      // 2K doubles; 3K when mu > 0
    const float* lr_t, float max_norm, float p1, float p2,
    float* stats_out, float* loss_out, hipStream_t s, int use_bf16,
    float mu,
    // null: end in k_pseudo_grad_mb + k_accum_mb with weights_dev (the
    // FedAvg / FedProx launches); else end in the DGA tail, which ignores
    // weights_dev and writes dga_out (4K doubles, see launch_mega_dga_accum)
    const DgaArgs* dga, double* dga_out);
void launch_mega_clip_sgd(float* params_stack, float* grads_stack,
                          long long P, int K, double* acc2k, float max_norm,
                          const float* lr_t, float* stats_out, hipStream_t s,
                          const float* server, float mu,
                          const unsigned char* active,  // [K] or null = all
                          float* loss_out);             // [K] or null
void launch_mega_pseudo_accum(float* grads_stack, const float* server,
                              const float* params_stack,
                              const float* weights_dev, float* round_accum,
                              long long P, int K, hipStream_t s);

// DGA tail over a K-stacked flat arena, K <= DGA_MAX_K:
// round_accum[p] += sum_k c_k (server[p] - params[k*P + p]) with c_k formed
// on the device from loss_out[K], stats_out[2K] and counts_dev[K].
// dga_out holds 4K doubles: weight_k, norm_k (0 without clip), c_k, and K
// doubles of scratch (the clip pass's sum of squares).  No host sync, no
// allocation: graph-capturable.
void launch_mega_dga_accum(const float* params_stack, const float* server,
                           long long P, int K, const float* loss_out,
                           const float* stats_out,
                           const long long* counts_dev, int bs, DgaArgs dga,
                           float* round_accum, double* dga_out,
                           hipStream_t s);

// fused_cnn.hip — per-kernel debug launchers.  Every operand is a
// K-stack (client k's rows are [k*bs, (k+1)*bs), its weights / biases /
// gradients the k-th contiguous block); K = 1 is the per-client case.
void launch_w2_layouts(const float* w2, int K, float* w2t, float* w2rot,
                       hipStream_t s);
void launch_conv2_fwd_mfma(const float* a1, const float* w2t,
                           const float* b2, int bs, int K, float* r2,
                           hipStream_t s);
// the same GEMM with the maxpool + dropout(p1) epilogue: writes a2, pidx
// (argmax | gate << 2) and m2 instead of r2; client k draws from
// seeds_dev[k] (device array)
void launch_conv2_fwd_pool_mfma(const float* a1, const float* w2t,
                                const float* b2, int bs, int K, float p1,
                                const long long* seeds_dev,
                                unsigned long long offset, float* a2,
                                unsigned char* pidx, unsigned char* m2,
                                hipStream_t s);
// dropout + maxpool + ReLU backward: dz2 and the conv2 bias sums db2[K*64]
void launch_pool_drop_bwd_bias(const float* da2, const unsigned char* pidx,
                               const unsigned char* m2, int bs, int K,
                               float p1, float* dz2, float* db2,
                               hipStream_t s);
void launch_conv2_bwd_x_mfma(const float* dz2, const float* w2rot,
                             const float* a1, int bs, int K, float* dz1,
                             hipStream_t s);
void launch_conv2_bwd_w_mfma(const float* dz2, const float* a1, int bs,
                             int K, float* slab, float* dw2, float* db2,
                             hipStream_t s);
void launch_fc1_fwd_mfma(const float* a2, const float* w3, const float* b3,
                         int bs, int K, float p2, unsigned long long seed,
                         unsigned long long offset, float* slab, float* z3,
                         float* a3, unsigned char* m3, hipStream_t s);
void launch_fc1_bwd_w_mfma(const float* dz3, const float* a2, int bs, int K,
                           float* dw3, float* db3, hipStream_t s);
void launch_fc1_bwd_x_mfma(const float* dz3, const float* w3, int bs, int K,
                           float* da2, hipStream_t s);
void launch_mfma_bf16_probe(const void* A, const void* B, float* D,
                            hipStream_t s);
void launch_fc1_fwd_mfma_bf16(const float* a2, const float* w3,
                              const float* b3, int bs, int K, float p2,
                              unsigned long long seed,
                              unsigned long long offset, float* slab,
                              float* z3, float* a3, unsigned char* m3,
                              hipStream_t s);
void launch_conv2_fwd_mfma_bf16(const float* a1, const float* w2b2, int bs,
                                int K, float* r2, hipStream_t s);
void launch_conv2_bwd_x_mfma_bf16(const float* dz2, const float* w2,
                                  const float* a1, int bs, int K,
                                  float* w2rotbf, float* dz1, hipStream_t s);
void launch_conv2_bwd_w_mfma_bf16(const float* dz2, const float* a1, int bs,
                                  int K, float* slab, float* dw2, float* db2,
                                  hipStream_t s);

}  // extern "C"
