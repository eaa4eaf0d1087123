// Python bindings for the gfx950 flat-arena kernels (flat_ops.hip).
//
// Host side is written against the native ROCm/HIP ATen surface of
// PyTorch-ROCm (c10::hip) — no CUDA compatibility layer.  All launches go
// onto the current torch stream; no host synchronization anywhere.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "launchers.h"

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_flat(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
}

void pseudo_grad(torch::Tensor out, torch::Tensor ws, torch::Tensor wt,
                 double weight) {
  check_flat(out, "out"); check_flat(ws, "ws"); check_flat(wt, "wt");
  TORCH_CHECK(out.numel() == ws.numel() && ws.numel() == wt.numel());
  launch_pseudo_grad(out.data_ptr<float>(), ws.data_ptr<float>(),
                     wt.data_ptr<float>(), (float)weight, out.numel(),
                     cur_stream());
}

void axpy(torch::Tensor y, torch::Tensor x, double alpha) {
  check_flat(y, "y"); check_flat(x, "x");
  TORCH_CHECK(y.numel() == x.numel());
  launch_axpy(y.data_ptr<float>(), x.data_ptr<float>(), (float)alpha,
              y.numel(), cur_stream());
}

void scale(torch::Tensor x, double alpha) {
  check_flat(x, "x");
  launch_scale(x.data_ptr<float>(), (float)alpha, x.numel(), cur_stream());
}

// two-stage reduction helper: no f64 atomics on the hot path
static torch::Tensor sum_sumsq_acc(const torch::Tensor& x) {
  auto acc = torch::zeros({2}, x.options().dtype(torch::kFloat64));
  int nparts = sum_sumsq2_partials(x.numel());
  auto partials = torch::empty({2 * (long long)nparts},
                               x.options().dtype(torch::kFloat64));
  launch_sum_sumsq2(x.data_ptr<float>(), x.numel(),
                    partials.data_ptr<double>(), acc.data_ptr<double>(),
                    cur_stream());
  return acc;
}

torch::Tensor sum_sumsq(torch::Tensor x) {
  check_flat(x, "x");
  return sum_sumsq_acc(x).to(torch::kFloat32);
}

torch::Tensor clip_by_norm(torch::Tensor x, double max_norm, double eps) {
  check_flat(x, "x");
  auto acc = sum_sumsq_acc(x);
  auto norm = torch::empty({}, x.options());
  launch_clip_apply(x.data_ptr<float>(), x.numel(), acc.data_ptr<double>(),
                    (float)max_norm, (float)eps, norm.data_ptr<float>(),
                    cur_stream());
  return norm;
}

void add_gaussian_noise(torch::Tensor x, double sigma, int64_t seed,
                        int64_t offset) {
  check_flat(x, "x");
  launch_add_gaussian_noise(x.data_ptr<float>(), x.numel(), (float)sigma,
                            (unsigned long long)seed,
                            (unsigned long long)offset, cur_stream());
}

void sgd_step(torch::Tensor p, torch::Tensor g, torch::Tensor buf, double lr,
              double momentum, double dampening, double weight_decay,
              bool nesterov, bool first_step) {
  check_flat(p, "p"); check_flat(g, "g");
  if (momentum != 0.0) {
    check_flat(buf, "buf");
    TORCH_CHECK(buf.numel() == p.numel(), "momentum buffer size mismatch");
  }
  launch_sgd_step(p.data_ptr<float>(), g.data_ptr<float>(),
                  buf.numel() ? buf.data_ptr<float>() : nullptr, (float)lr,
                  nullptr, (float)momentum, (float)dampening,
                  (float)weight_decay, nesterov ? 1 : 0, first_step ? 1 : 0,
                  p.numel(), cur_stream());
}

// graph-replayable SGD: lr read from a 1-element device tensor
void sgd_step_devlr(torch::Tensor p, torch::Tensor g, torch::Tensor buf,
                    torch::Tensor lr_t, double momentum, double dampening,
                    double weight_decay, bool nesterov, bool first_step) {
  check_flat(p, "p"); check_flat(g, "g"); check_flat(lr_t, "lr_t");
  if (momentum != 0.0) {
    check_flat(buf, "buf");
    TORCH_CHECK(buf.numel() == p.numel(), "momentum buffer size mismatch");
  }
  launch_sgd_step(p.data_ptr<float>(), g.data_ptr<float>(),
                  buf.numel() ? buf.data_ptr<float>() : nullptr, 0.f,
                  lr_t.data_ptr<float>(), (float)momentum, (float)dampening,
                  (float)weight_decay, nesterov ? 1 : 0, first_step ? 1 : 0,
                  p.numel(), cur_stream());
}

// fused per-batch clip + sufficient-stats accumulate (one reduction pass):
// clips x to max_norm and adds post-clip {Σx, Σx²} into stats_acc[0..1]
void clip_stats_accumulate(torch::Tensor x, double max_norm, double eps,
                           torch::Tensor stats_acc) {
  check_flat(x, "x"); check_flat(stats_acc, "stats_acc");
  TORCH_CHECK(stats_acc.numel() >= 2, "stats_acc must have 2 elements");
  auto acc = sum_sumsq_acc(x);
  launch_clip_apply_stats(x.data_ptr<float>(), x.numel(),
                          acc.data_ptr<double>(), (float)max_norm, (float)eps,
                          stats_acc.data_ptr<float>(), cur_stream());
}

void adam_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
               torch::Tensor v, torch::Tensor vmax, int64_t step, double lr,
               double beta1, double beta2, double eps, double weight_decay,
               bool amsgrad, bool adamw) {
  check_flat(p, "p"); check_flat(g, "g"); check_flat(m, "m"); check_flat(v, "v");
  if (amsgrad) check_flat(vmax, "vmax");
  float bc1 = 1.0f - (float)std::pow(beta1, (double)step);
  float bc2 = 1.0f - (float)std::pow(beta2, (double)step);
  launch_adam_step(p.data_ptr<float>(), g.data_ptr<float>(),
                   m.data_ptr<float>(), v.data_ptr<float>(),
                   vmax.numel() ? vmax.data_ptr<float>() : nullptr, (float)lr,
                   (float)beta1, (float)beta2, (float)eps, (float)weight_decay,
                   bc1, bc2, amsgrad ? 1 : 0, adamw ? 1 : 0, p.numel(),
                   cur_stream());
}

void adamax_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                 torch::Tensor u, int64_t step, double lr, double beta1,
                 double beta2, double eps, double weight_decay) {
  check_flat(p, "p"); check_flat(g, "g"); check_flat(m, "m"); check_flat(u, "u");
  float bc1 = 1.0f - (float)std::pow(beta1, (double)step);
  launch_adamax_step(p.data_ptr<float>(), g.data_ptr<float>(),
                     m.data_ptr<float>(), u.data_ptr<float>(), (float)lr,
                     (float)beta1, (float)beta2, (float)eps,
                     (float)weight_decay, bc1, p.numel(), cur_stream());
}

torch::Tensor segmented_sqnorm(torch::Tensor x, torch::Tensor seg_offsets) {
  check_flat(x, "x");
  TORCH_CHECK(seg_offsets.is_cuda() && seg_offsets.is_contiguous() &&
              seg_offsets.scalar_type() == torch::kInt64,
              "seg_offsets must be contiguous int64 on GPU");
  int n_segs = (int)seg_offsets.numel() - 1;
  auto out = torch::zeros({n_segs}, x.options().dtype(torch::kFloat64));
  launch_segmented_sqnorm(
      x.data_ptr<float>(),
      reinterpret_cast<const long long*>(seg_offsets.data_ptr<int64_t>()),
      n_segs, out.data_ptr<double>(), cur_stream());
  return out.to(torch::kFloat32);
}

void quant_bin_mask(torch::Tensor x, torch::Tensor min_t, torch::Tensor max_t,
                    torch::Tensor thresh_t, int64_t n_bins) {
  check_flat(x, "x");
  check_flat(min_t, "min_t"); check_flat(max_t, "max_t");
  check_flat(thresh_t, "thresh_t");
  launch_quant_bin_mask(x.data_ptr<float>(), x.numel(),
                        min_t.data_ptr<float>(), max_t.data_ptr<float>(),
                        thresh_t.data_ptr<float>(), (int)n_bins, cur_stream());
}

// the ONE slicer of the CNN workspace (G = K * bs rows over K clients;
// K = 1 for cnn_epoch / cnn_round).  Byte layout: pidx at 0, m2 at G*9216,
// m3 at 2*G*9216.  The float layout may be reordered on two conditions:
// dlogits stays last (G*C need not be a multiple of 4 floats), and every
// region before it stays a multiple of 4 floats, so that the buffers the
// kernels move as float4 keep their 16 B alignment.
static CnnWorkspace slice_ws(torch::Tensor& work_f, torch::Tensor& work_i,
                             torch::Tensor& work_b, long long G, long long K,
                             long long C) {
  CnnWorkspaceSizes z = cnn_workspace_sizes(G, K, C);
  TORCH_CHECK(work_f.numel() >= z.n_float, "float workspace too small");
  TORCH_CHECK(work_i.numel() >= z.n_int, "int workspace too small");
  TORCH_CHECK(work_b.numel() >= z.n_byte, "byte workspace too small");
  float* f = work_f.data_ptr<float>();
  auto take = [&](long long n) { float* p = f; f += n; return p; };
  CnnWorkspace ws;
  ws.xb = take(G * 784);
  ws.a1 = take(G * 21632);
  ws.r2 = take(G * 36864);
  ws.a2 = take(G * 9216);
  ws.z3 = take(G * 128);
  ws.a3 = take(G * 128);
  ws.dz3 = take(G * 128);
  ws.da2 = take(G * 9216);
  ws.dz2 = take(G * 36864);
  ws.dz1 = take(G * 21632);
  ws.w2t = take(K * 18432);
  ws.w2rot = take(K * 18432);
  ws.wsl = take(G * 18432);
  ws.dlogits = take(G * C);
  TORCH_CHECK(f - work_f.data_ptr<float>() == z.n_float,
              "cnn_workspace_sizes disagrees with the slicer");
  ws.yb = work_i.data_ptr<int>();
  unsigned char* u = work_b.data_ptr<unsigned char>();
  ws.pidx = u;
  ws.m2 = u + G * 9216;
  ws.m3 = u + 2 * G * 9216;
  ws.red_partials = ws.red_acc = nullptr;
  return ws;
}

// the K = 1 drivers' double workspace: launch_sum_sumsq2's partials and,
// in the last two slots, its result
static void slice_red(CnnWorkspace& ws, torch::Tensor& work_d) {
  TORCH_CHECK(work_d.numel() >= 2 * 2048 + 2, "double workspace too small");
  ws.red_partials = work_d.data_ptr<double>();
  ws.red_acc = work_d.data_ptr<double>() + work_d.numel() - 2;
}

static std::tuple<int64_t, int64_t, int64_t> cnn_workspace_sizes_py(
    int64_t G, int64_t K, int64_t C) {
  TORCH_CHECK(G >= K && K >= 1 && C >= 1);
  CnnWorkspaceSizes z = cnn_workspace_sizes(G, K, C);
  return {z.n_float, z.n_int, z.n_byte};
}

// bound every per-client (row_base, order_off, count) against the shard /
// order tensors so inconsistent host metadata raises instead of launching
// out-of-bounds device reads.  The three are host int64 tensors of K.
static void check_client_meta(const torch::Tensor& shard_x,
                              const torch::Tensor& shard_y,
                              const torch::Tensor& orders_dev,
                              const torch::Tensor& row_bases,
                              const torch::Tensor& order_offs,
                              const torch::Tensor& counts,
                              bool allow_empty) {
  long long n_rows = shard_y.numel();
  TORCH_CHECK(shard_x.numel() == n_rows * 784,
              "shard_x rows must match shard_y (784 features each)");
  long long n_orders = orders_dev.numel();
  auto rb = row_bases.accessor<int64_t, 1>();
  auto oo = order_offs.accessor<int64_t, 1>();
  auto ct = counts.accessor<int64_t, 1>();
  for (int k = 0; k < (int)counts.numel(); ++k) {
    TORCH_CHECK(ct[k] >= (allow_empty ? 0 : 1) && rb[k] >= 0 && oo[k] >= 0,
                "negative per-client metadata",
                allow_empty ? "" : " or empty client", " at k=", k);
    TORCH_CHECK(rb[k] + ct[k] <= n_rows,
                "client ", k, ": row_base+count ", rb[k] + ct[k],
                " exceeds shard rows ", n_rows);
    TORCH_CHECK(oo[k] + ct[k] <= n_orders,
                "client ", k, ": order_off+count ", oo[k] + ct[k],
                " exceeds orders length ", n_orders);
  }
}

// FedProx arguments shared by the CNN / clip entries: mu == 0 is plain
// SGD and needs no server vector; mu > 0 needs the [P] server weights
static const float* prox_server(const c10::optional<torch::Tensor>& server,
                                double mu, long long P) {
  TORCH_CHECK(mu >= 0.0, "mu must be >= 0");
  if (mu == 0.0) return nullptr;
  TORCH_CHECK(server.has_value(), "mu > 0 needs the server weights");
  check_flat(*server, "server");
  TORCH_CHECK(server->numel() == P, "server must hold P floats");
  return server->data_ptr<float>();
}

// fully-fused CNN-FEMNIST client epoch (fused_cnn.hip): one host call
// trains a whole local epoch — fwd, bwd, clip+stats, SGD per batch —
// bypassing autograd and hip graphs entirely.
void cnn_epoch(torch::Tensor shard_x, torch::Tensor shard_y,
               torch::Tensor order, int64_t bs, int64_t C,
               torch::Tensor params, torch::Tensor grads,
               torch::Tensor work_f, torch::Tensor work_i,
               torch::Tensor work_b, torch::Tensor work_d,
               torch::Tensor lr_t, double max_norm, double p1, double p2,
               torch::Tensor stats_acc, torch::Tensor loss_acc,
               int64_t seed, bool use_bf16,
               c10::optional<torch::Tensor> server, double mu) {
  check_flat(params, "params"); check_flat(grads, "grads");
  const float* server_p = prox_server(server, mu, params.numel());
  check_flat(lr_t, "lr_t"); check_flat(stats_acc, "stats_acc");
  check_flat(loss_acc, "loss_acc"); check_flat(work_f, "work_f");
  TORCH_CHECK(shard_x.is_cuda() && shard_x.is_contiguous() &&
              shard_x.scalar_type() == torch::kFloat32, "shard_x");
  TORCH_CHECK(shard_y.is_cuda() && shard_y.is_contiguous() &&
              shard_y.scalar_type() == torch::kInt64, "shard_y");
  TORCH_CHECK(order.is_cuda() && order.scalar_type() == torch::kInt64,
              "order must be int64 on device");
  long long n = shard_y.numel();
  TORCH_CHECK(shard_x.numel() == n * 784, "shard_x must be [n,784]");
  TORCH_CHECK(bs >= 1 && bs <= 32, "fused CNN epoch supports batch <= 32");
  int B = (int)bs;
  CnnWorkspace ws = slice_ws(work_f, work_i, work_b, B, 1, C);
  slice_red(ws, work_d);
  launch_cnn_epoch(shard_x.data_ptr<float>(),
                   reinterpret_cast<const long long*>(
                       shard_y.data_ptr<int64_t>()),
                   reinterpret_cast<const long long*>(
                       order.data_ptr<int64_t>()),
                   n, B, (int)C,
                   params.data_ptr<float>(), grads.data_ptr<float>(), ws,
                   lr_t.data_ptr<float>(), (float)max_norm, (float)p1,
                   (float)p2, stats_acc.data_ptr<float>(),
                   loss_acc.data_ptr<float>(), (unsigned long long)seed,
                   cur_stream(), 0, use_bf16 ? 1 : 0, server_p, (float)mu);
}

// whole-round driver: K clients in ONE host call (copy-in, fused epoch,
// weighted pseudo-gradient, accumulate) — per-client loss/stats in slots
void cnn_round(torch::Tensor shard_x, torch::Tensor shard_y,
               torch::Tensor orders_dev, torch::Tensor row_bases,
               torch::Tensor order_offs, torch::Tensor counts,
               torch::Tensor weights, torch::Tensor seeds, int64_t bs,
               int64_t C, torch::Tensor server_params, torch::Tensor params,
               torch::Tensor grads, torch::Tensor round_accum,
               torch::Tensor work_f, torch::Tensor work_i,
               torch::Tensor work_b, torch::Tensor work_d,
               torch::Tensor lr_t, double max_norm, double p1, double p2,
               torch::Tensor stats_out, torch::Tensor loss_out,
               bool use_bf16, double mu) {
  TORCH_CHECK(mu >= 0.0, "mu must be >= 0");
  check_flat(server_params, "server_params"); check_flat(params, "params");
  check_flat(grads, "grads"); check_flat(round_accum, "round_accum");
  TORCH_CHECK(orders_dev.is_cuda() && orders_dev.scalar_type() == torch::kInt64);
  TORCH_CHECK(!row_bases.is_cuda() && !order_offs.is_cuda() &&
              !counts.is_cuda() && !weights.is_cuda() && !seeds.is_cuda(),
              "per-client metadata must be host tensors");
  TORCH_CHECK(row_bases.scalar_type() == torch::kInt64 &&
              order_offs.scalar_type() == torch::kInt64 &&
              counts.scalar_type() == torch::kInt64 &&
              seeds.scalar_type() == torch::kInt64 &&
              weights.scalar_type() == torch::kFloat32,
              "metadata dtypes: int64 (weights fp32)");
  TORCH_CHECK(row_bases.is_contiguous() && order_offs.is_contiguous() &&
              counts.is_contiguous() && weights.is_contiguous() &&
              seeds.is_contiguous());
  int K = (int)counts.numel();
  TORCH_CHECK(stats_out.numel() >= 2 * K && loss_out.numel() >= K);
  TORCH_CHECK(bs >= 1 && bs <= 32);
  TORCH_CHECK(row_bases.numel() == K && order_offs.numel() == K &&
              weights.numel() == K && seeds.numel() == K,
              "per-client metadata lengths must all equal K");
  check_client_meta(shard_x, shard_y, orders_dev, row_bases, order_offs,
                    counts, /*allow_empty=*/true);
  CnnWorkspace ws = slice_ws(work_f, work_i, work_b, bs, 1, C);
  slice_red(ws, work_d);
  launch_cnn_round(
      shard_x.data_ptr<float>(),
      reinterpret_cast<const long long*>(shard_y.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(orders_dev.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(row_bases.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(order_offs.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(counts.data_ptr<int64_t>()),
      weights.data_ptr<float>(),
      reinterpret_cast<const unsigned long long*>(seeds.data_ptr<int64_t>()),
      K, (int)bs, (int)C, server_params.data_ptr<float>(),
      params.data_ptr<float>(), grads.data_ptr<float>(),
      round_accum.data_ptr<float>(), ws, lr_t.data_ptr<float>(),
      (float)max_norm, (float)p1, (float)p2, stats_out.data_ptr<float>(),
      loss_out.data_ptr<float>(), cur_stream(), use_bf16 ? 1 : 0,
      (float)mu);
}

// fused LSTM sequence recurrence (lstm_seq.hip): all T steps in one
// launch over xp [R, T, 4H] and K-stacked float4-packed hidden weights
// (ops/lstm._pack_fwd / _pack_bwd); row r belongs to client
// r / rows_per_client.  Forward returns (h_seq, activated gates, cell
// states).  Both dispatch on w_packed_stack's dtype: float32 as above,
// bfloat16 = the bf16-stored layouts of ops/lstm._pack_fwd_bf16 /
// _pack_bwd_bf16 (same element count; everything else stays fp32).
static bool lstm_w_is_bf16(const torch::Tensor& w, const char* layout) {
  if (w.scalar_type() == torch::kFloat32) {
    check_flat(w, "w_packed_stack");
    return false;
  }
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16,
              "w_packed_stack must be float32 or bfloat16");
  TORCH_CHECK(w.is_cuda(), "w_packed_stack must be a GPU tensor");
  TORCH_CHECK(w.is_contiguous(), "w_packed_stack must be contiguous ",
              layout);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "w_packed_stack must be 16-byte aligned");
  return true;
}

std::vector<torch::Tensor> lstm_seq_fwd(torch::Tensor xp,
                                        torch::Tensor w_packed_stack,
                                        int64_t rows_per_client) {
  check_flat(xp, "xp");
  bool bf16 = lstm_w_is_bf16(w_packed_stack,
                             "[K, 256/8, 4*256, 8] (ops/lstm._pack_fwd_bf16)");
  TORCH_CHECK(xp.dim() == 3 && xp.size(2) == 4 * 256,
              "fused LSTM supports hidden size 256: xp must be "
              "[R, T, 4*256]");
  long long R = xp.size(0), T = xp.size(1);
  TORCH_CHECK(rows_per_client > 0 && R % rows_per_client == 0);
  long long K = R / rows_per_client;
  TORCH_CHECK(w_packed_stack.numel() == K * 256 * 4 * 256,
              "w_packed_stack must be [K, 256/4, 4*256, 4] "
              "(ops/lstm._pack_fwd)");
  auto h_seq = torch::empty({R, T, 256}, xp.options());
  auto gates = torch::empty({R, T, 4 * 256}, xp.options());
  auto c_seq = torch::empty({R, T, 256}, xp.options());
  if (bf16)
    launch_lstm_seq_fwd_bf16(
        xp.data_ptr<float>(),
        static_cast<const unsigned short*>(w_packed_stack.data_ptr()),
        h_seq.data_ptr<float>(), gates.data_ptr<float>(),
        c_seq.data_ptr<float>(), (int)R, (int)rows_per_client, (int)T,
        cur_stream());
  else
    launch_lstm_seq_fwd(xp.data_ptr<float>(),
                        w_packed_stack.data_ptr<float>(),
                        h_seq.data_ptr<float>(), gates.data_ptr<float>(),
                        c_seq.data_ptr<float>(), (int)R,
                        (int)rows_per_client, (int)T, cur_stream());
  return {h_seq, gates, c_seq};
}

torch::Tensor lstm_seq_bwd(torch::Tensor gates, torch::Tensor c_seq,
                           torch::Tensor w_packed_stack,
                           torch::Tensor dh_out, int64_t rows_per_client) {
  check_flat(gates, "gates"); check_flat(c_seq, "c_seq");
  bool bf16 = lstm_w_is_bf16(w_packed_stack,
                             "[K, 4*256/8, 256, 8] (ops/lstm._pack_bwd_bf16)");
  check_flat(dh_out, "dh_out");
  long long R = gates.size(0), T = gates.size(1);
  TORCH_CHECK(rows_per_client > 0 && R % rows_per_client == 0);
  long long K = R / rows_per_client;
  TORCH_CHECK(w_packed_stack.numel() == K * 4 * 256 * 256,
              "w_packed_stack must be [K, 4*256/4, 256, 4] "
              "(ops/lstm._pack_bwd)");
  auto dg = torch::empty_like(gates);
  if (bf16)
    launch_lstm_seq_bwd_bf16(
        gates.data_ptr<float>(), c_seq.data_ptr<float>(),
        static_cast<const unsigned short*>(w_packed_stack.data_ptr()),
        dh_out.data_ptr<float>(), dg.data_ptr<float>(), (int)R,
        (int)rows_per_client, (int)T, cur_stream());
  else
    launch_lstm_seq_bwd(gates.data_ptr<float>(), c_seq.data_ptr<float>(),
                        w_packed_stack.data_ptr<float>(),
                        dh_out.data_ptr<float>(), dg.data_ptr<float>(),
                        (int)R, (int)rows_per_client, (int)T, cur_stream());
  return dg;
}

// fused GRU sequence recurrence (gru_seq.hip)
std::vector<torch::Tensor> gru_seq_fwd(torch::Tensor gi, torch::Tensor whh_t,
                                       torch::Tensor b_hh) {
  check_flat(gi, "gi"); check_flat(whh_t, "whh_t"); check_flat(b_hh, "b_hh");
  TORCH_CHECK(gi.dim() == 3 && gi.size(2) == 3 * 512 &&
              whh_t.numel() == 512 * 3 * 512,
              "fused GRU supports hidden size 512; pass W_hh "
              "float4-packed [H/4, 3H, 4] (ops/lstm._GRUSeq)");
  long long B = gi.size(0), T = gi.size(1);
  auto h_seq = torch::empty({B, T, 512}, gi.options());
  auto gates = torch::empty({B, T, 3 * 512}, gi.options());
  auto ghn = torch::empty({B, T, 512}, gi.options());
  launch_gru_seq_fwd(gi.data_ptr<float>(), whh_t.data_ptr<float>(),
                     b_hh.data_ptr<float>(), h_seq.data_ptr<float>(),
                     gates.data_ptr<float>(), ghn.data_ptr<float>(),
                     (int)B, (int)T, cur_stream());
  return {h_seq, gates, ghn};
}

std::vector<torch::Tensor> gru_seq_bwd(torch::Tensor gates, torch::Tensor ghn,
                                       torch::Tensor h_seq,
                                       torch::Tensor w_hh,
                                       torch::Tensor dh_out) {
  check_flat(gates, "gates"); check_flat(ghn, "ghn");
  check_flat(h_seq, "h_seq"); check_flat(w_hh, "w_hh");
  check_flat(dh_out, "dh_out");
  TORCH_CHECK(w_hh.numel() == 3 * 512 * 512,
              "gru_seq_bwd wants W_hh float4-packed [3H/4, H, 4]");
  long long B = gates.size(0), T = gates.size(1);
  auto dgi = torch::empty_like(gates);
  auto dgh = torch::empty_like(gates);
  launch_gru_seq_bwd(gates.data_ptr<float>(), ghn.data_ptr<float>(),
                     h_seq.data_ptr<float>(), w_hh.data_ptr<float>(),
                     dh_out.data_ptr<float>(), dgi.data_ptr<float>(),
                     dgh.data_ptr<float>(), (int)B, (int)T, cur_stream());
  return {dgi, dgh};
}

// fused GRU gate math (no-grad eval path of the nlg_gru recurrence)
torch::Tensor gru_gates(torch::Tensor g_i, torch::Tensor g_h,
                        torch::Tensor h) {
  check_flat(g_i, "g_i"); check_flat(g_h, "g_h"); check_flat(h, "h");
  int B = (int)h.size(0), H = (int)h.size(1);
  TORCH_CHECK(g_i.numel() == 3LL * B * H && g_h.numel() == 3LL * B * H,
              "g_i/g_h must be [B, 3H]");
  auto out = torch::empty_like(h);
  launch_gru_gates(g_i.data_ptr<float>(), g_h.data_ptr<float>(),
                   h.data_ptr<float>(), out.data_ptr<float>(), B, H,
                   cur_stream());
  return out;
}

}  // namespace

// ---------------------------------------------------------------------------
// per-kernel MFMA debug entries (numerics tests vs torch references; the
// drivers launch the same kernels).  Operands may be K-stacked: B is the
// total row count, client k owns rows [k*B/K, (k+1)*B/K) and the k-th
// block of every weight / bias / gradient tensor.  K is inferred from the
// weight length where a weight is passed and given explicitly where only
// gradients come out.
// ---------------------------------------------------------------------------
static int rows_per_client(int64_t B, int64_t K) {
  TORCH_CHECK(K >= 1 && B >= K && B % K == 0, "B rows must split over K");
  return (int)(B / K);
}

// the fc1 GEMMs mask ONE 32-row tile per client
static int fc1_rows_per_client(int64_t B, int64_t K) {
  int bs = rows_per_client(B, K);
  TORCH_CHECK(bs <= 32, "fc1 kernels take at most 32 rows per client");
  return bs;
}

static int stack_len(const torch::Tensor& w, int64_t per, const char* name) {
  TORCH_CHECK(w.numel() > 0 && w.numel() % per == 0, name,
              " must hold K blocks of ", per);
  return (int)(w.numel() / per);
}

torch::Tensor dbg_conv2_fwd_mfma(torch::Tensor a1, torch::Tensor w2,
                                 torch::Tensor b2, int64_t B) {
  check_flat(a1, "a1"); check_flat(w2, "w2"); check_flat(b2, "b2");
  int K = stack_len(w2, 18432, "w2");
  int bs = rows_per_client(B, K);
  TORCH_CHECK(a1.numel() >= B * 21632 && b2.numel() == K * 64);
  auto r2 = torch::empty({B * 36864}, a1.options());
  auto w2t = torch::empty_like(w2);
  auto w2rot = torch::empty_like(w2);
  launch_w2_layouts(w2.data_ptr<float>(), K, w2t.data_ptr<float>(),
                    w2rot.data_ptr<float>(), cur_stream());
  launch_conv2_fwd_mfma(a1.data_ptr<float>(), w2t.data_ptr<float>(),
                        b2.data_ptr<float>(), bs, K, r2.data_ptr<float>(),
                        cur_stream());
  return r2;
}

// conv2 forward with the pool + dropout epilogue: (a2, pidx, m2) of
// K clients x bs rows; seeds is an int64 tensor of K dropout seeds
std::vector<torch::Tensor> dbg_conv2_fwd_pool_mfma(
    torch::Tensor a1, torch::Tensor w2, torch::Tensor b2, int64_t bs,
    int64_t K, double p1, torch::Tensor seeds, int64_t offset) {
  check_flat(a1, "a1"); check_flat(w2, "w2"); check_flat(b2, "b2");
  TORCH_CHECK(K >= 1 && bs >= 1 && bs <= 32);
  long long B = K * bs;
  TORCH_CHECK(w2.numel() == K * 18432 && b2.numel() == K * 64 &&
              a1.numel() >= B * 21632);
  TORCH_CHECK(seeds.scalar_type() == torch::kInt64 && seeds.numel() == K,
              "seeds must be K int64 values");
  auto seeds_dev = seeds.to(a1.device()).contiguous();
  auto w2t = torch::empty_like(w2);
  auto w2rot = torch::empty_like(w2);
  auto a2 = torch::empty({B * 9216}, a1.options());
  auto pidx = torch::empty({B * 9216}, a1.options().dtype(torch::kUInt8));
  auto m2 = torch::empty({B * 9216}, a1.options().dtype(torch::kUInt8));
  launch_w2_layouts(w2.data_ptr<float>(), (int)K, w2t.data_ptr<float>(),
                    w2rot.data_ptr<float>(), cur_stream());
  launch_conv2_fwd_pool_mfma(
      a1.data_ptr<float>(), w2t.data_ptr<float>(), b2.data_ptr<float>(),
      (int)bs, (int)K, (float)p1,
      reinterpret_cast<const long long*>(seeds_dev.data_ptr<int64_t>()),
      (unsigned long long)offset, a2.data_ptr<float>(),
      pidx.data_ptr<unsigned char>(), m2.data_ptr<unsigned char>(),
      cur_stream());
  return {a2, pidx, m2};
}

// pool/dropout backward with the conv2 bias sums: (dz2, db2)
std::vector<torch::Tensor> dbg_pool_drop_bwd_bias(
    torch::Tensor da2, torch::Tensor pidx, torch::Tensor m2, int64_t bs,
    int64_t K, double p1) {
  check_flat(da2, "da2");
  TORCH_CHECK(K >= 1 && bs >= 1);
  long long B = K * bs;
  TORCH_CHECK(da2.numel() == B * 9216);
  for (const torch::Tensor* t : {&pidx, &m2})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                t->scalar_type() == torch::kUInt8 &&
                t->numel() == B * 9216, "pidx / m2 must be uint8 [B*9216]");
  auto dz2 = torch::empty({B * 36864}, da2.options());
  auto db2 = torch::empty({K * 64}, da2.options());
  launch_pool_drop_bwd_bias(da2.data_ptr<float>(),
                            pidx.data_ptr<unsigned char>(),
                            m2.data_ptr<unsigned char>(), (int)bs, (int)K,
                            (float)p1, dz2.data_ptr<float>(),
                            db2.data_ptr<float>(), cur_stream());
  return {dz2, db2};
}

torch::Tensor dbg_conv2_fwd_mfma_bf16(torch::Tensor a1, torch::Tensor w2,
                                      torch::Tensor b2, int64_t B) {
  check_flat(a1, "a1"); check_flat(w2, "w2"); check_flat(b2, "b2");
  int K = stack_len(w2, 18432, "w2");
  int bs = rows_per_client(B, K);
  TORCH_CHECK(a1.numel() >= B * 21632 && b2.numel() == K * 64);
  // the kernel reads w2 and b2 through one stack pointer
  auto w2b2 = torch::cat({w2.view({K, 18432}), b2.view({K, 64})}, 1)
                  .contiguous();
  auto r2 = torch::empty({B * 36864}, a1.options());
  launch_conv2_fwd_mfma_bf16(a1.data_ptr<float>(), w2b2.data_ptr<float>(),
                             bs, K, r2.data_ptr<float>(), cur_stream());
  return r2;
}

torch::Tensor dbg_conv2_bwd_x_mfma_bf16(torch::Tensor dz2, torch::Tensor w2,
                                        torch::Tensor a1, int64_t B) {
  check_flat(dz2, "dz2"); check_flat(w2, "w2"); check_flat(a1, "a1");
  int K = stack_len(w2, 18432, "w2");
  int bs = rows_per_client(B, K);
  TORCH_CHECK(dz2.numel() >= B * 36864 && a1.numel() >= B * 21632);
  auto dz1 = torch::empty({B * 21632}, dz2.options());
  auto w2rotbf = torch::empty_like(w2);  // holds K*18432 bf16
  launch_conv2_bwd_x_mfma_bf16(dz2.data_ptr<float>(), w2.data_ptr<float>(),
                               a1.data_ptr<float>(), bs, K,
                               w2rotbf.data_ptr<float>(),
                               dz1.data_ptr<float>(), cur_stream());
  return dz1;
}

std::vector<torch::Tensor> dbg_conv2_bwd_w_mfma_bf16(torch::Tensor dz2,
                                                     torch::Tensor a1,
                                                     int64_t B, int64_t K) {
  check_flat(dz2, "dz2"); check_flat(a1, "a1");
  int bs = rows_per_client(B, K);
  TORCH_CHECK(dz2.numel() >= B * 36864 && a1.numel() >= B * 21632);
  auto slab = torch::empty({B * 18432}, dz2.options());
  auto dw2 = torch::empty({K * 18432}, dz2.options());
  auto db2 = torch::empty({K * 64}, dz2.options());
  launch_conv2_bwd_w_mfma_bf16(dz2.data_ptr<float>(), a1.data_ptr<float>(),
                               bs, (int)K, slab.data_ptr<float>(),
                               dw2.data_ptr<float>(), db2.data_ptr<float>(),
                               cur_stream());
  return {dw2, db2};
}

std::vector<torch::Tensor> dbg_fc1_fwd_mfma_bf16(torch::Tensor a2,
                                                 torch::Tensor w3,
                                                 torch::Tensor b3, int64_t B,
                                                 double p2, int64_t seed,
                                                 int64_t offset) {
  check_flat(a2, "a2"); check_flat(w3, "w3"); check_flat(b3, "b3");
  int K = stack_len(w3, 128 * 9216, "w3");
  int bs = fc1_rows_per_client(B, K);
  TORCH_CHECK(a2.numel() >= B * 9216 && b3.numel() == K * 128);
  auto slab = torch::empty({36 * B * 128}, a2.options());
  auto z3 = torch::empty({B * 128}, a2.options());
  auto a3 = torch::empty({B * 128}, a2.options());
  auto m3 = torch::empty({B * 128}, a2.options().dtype(torch::kUInt8));
  launch_fc1_fwd_mfma_bf16(a2.data_ptr<float>(), w3.data_ptr<float>(),
                           b3.data_ptr<float>(), bs, K, (float)p2,
                           (unsigned long long)seed,
                           (unsigned long long)offset,
                           slab.data_ptr<float>(), z3.data_ptr<float>(),
                           a3.data_ptr<float>(), m3.data_ptr<unsigned char>(),
                           cur_stream());
  return {z3, a3, m3};
}

torch::Tensor dbg_conv2_bwd_x_mfma(torch::Tensor dz2, torch::Tensor w2,
                                   torch::Tensor a1, int64_t B) {
  check_flat(dz2, "dz2"); check_flat(w2, "w2"); check_flat(a1, "a1");
  int K = stack_len(w2, 18432, "w2");
  int bs = rows_per_client(B, K);
  TORCH_CHECK(dz2.numel() >= B * 36864 && a1.numel() >= B * 21632);
  auto dz1 = torch::empty({B * 21632}, dz2.options());
  auto w2t = torch::empty_like(w2);
  auto w2rot = torch::empty_like(w2);
  launch_w2_layouts(w2.data_ptr<float>(), K, w2t.data_ptr<float>(),
                    w2rot.data_ptr<float>(), cur_stream());
  launch_conv2_bwd_x_mfma(dz2.data_ptr<float>(), w2rot.data_ptr<float>(),
                          a1.data_ptr<float>(), bs, K,
                          dz1.data_ptr<float>(), cur_stream());
  return dz1;
}

std::vector<torch::Tensor> dbg_conv2_bwd_w_mfma(torch::Tensor dz2,
                                                torch::Tensor a1, int64_t B,
                                                int64_t K) {
  check_flat(dz2, "dz2"); check_flat(a1, "a1");
  int bs = rows_per_client(B, K);
  TORCH_CHECK(dz2.numel() >= B * 36864 && a1.numel() >= B * 21632);
  auto slab = torch::empty({B * 18432}, dz2.options());
  auto dw2 = torch::empty({K * 18432}, dz2.options());
  auto db2 = torch::empty({K * 64}, dz2.options());
  launch_conv2_bwd_w_mfma(dz2.data_ptr<float>(), a1.data_ptr<float>(),
                          bs, (int)K, slab.data_ptr<float>(),
                          dw2.data_ptr<float>(), db2.data_ptr<float>(),
                          cur_stream());
  return {dw2, db2};
}

std::vector<torch::Tensor> dbg_fc1_fwd_mfma(torch::Tensor a2,
                                            torch::Tensor w3,
                                            torch::Tensor b3, int64_t B,
                                            double p2, int64_t seed,
                                            int64_t offset) {
  check_flat(a2, "a2"); check_flat(w3, "w3"); check_flat(b3, "b3");
  int K = stack_len(w3, 128 * 9216, "w3");
  int bs = fc1_rows_per_client(B, K);
  TORCH_CHECK(a2.numel() >= B * 9216 && b3.numel() == K * 128);
  auto slab = torch::empty({64 * B * 128}, a2.options());
  auto z3 = torch::empty({B * 128}, a2.options());
  auto a3 = torch::empty({B * 128}, a2.options());
  auto m3 = torch::empty({B * 128}, a2.options().dtype(torch::kUInt8));
  launch_fc1_fwd_mfma(a2.data_ptr<float>(), w3.data_ptr<float>(),
                      b3.data_ptr<float>(), bs, K, (float)p2,
                      (unsigned long long)seed, (unsigned long long)offset,
                      slab.data_ptr<float>(), z3.data_ptr<float>(),
                      a3.data_ptr<float>(), m3.data_ptr<unsigned char>(),
                      cur_stream());
  return {z3, a3, m3};
}

std::vector<torch::Tensor> dbg_fc1_bwd_w_mfma(torch::Tensor dz3,
                                              torch::Tensor a2, int64_t B,
                                              int64_t K) {
  check_flat(dz3, "dz3"); check_flat(a2, "a2");
  int bs = fc1_rows_per_client(B, K);
  TORCH_CHECK(dz3.numel() >= B * 128 && a2.numel() >= B * 9216);
  auto dw3 = torch::empty({K * 128 * 9216}, dz3.options());
  auto db3 = torch::empty({K * 128}, dz3.options());
  launch_fc1_bwd_w_mfma(dz3.data_ptr<float>(), a2.data_ptr<float>(), bs,
                        (int)K, dw3.data_ptr<float>(), db3.data_ptr<float>(),
                        cur_stream());
  return {dw3, db3};
}

torch::Tensor dbg_fc1_bwd_x_mfma(torch::Tensor dz3, torch::Tensor w3,
                                 int64_t B) {
  check_flat(dz3, "dz3"); check_flat(w3, "w3");
  int K = stack_len(w3, 128 * 9216, "w3");
  int bs = fc1_rows_per_client(B, K);
  TORCH_CHECK(dz3.numel() >= B * 128);
  auto da2 = torch::empty({B * 9216}, dz3.options());
  launch_fc1_bwd_x_mfma(dz3.data_ptr<float>(), w3.data_ptr<float>(), bs, K,
                        da2.data_ptr<float>(), cur_stream());
  return da2;
}

torch::Tensor dbg_mfma_bf16_probe(torch::Tensor A, torch::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == torch::kBFloat16 &&
              A.is_contiguous() && A.numel() == 16 * 32);
  TORCH_CHECK(B.is_cuda() && B.scalar_type() == torch::kBFloat16 &&
              B.is_contiguous() && B.numel() == 32 * 16);
  auto D = torch::empty({16, 16},
                        A.options().dtype(torch::kFloat32));
  launch_mfma_bf16_probe(A.data_ptr(), B.data_ptr(), D.data_ptr<float>(),
                         cur_stream());
  return D;
}

// MEGA round: every sampled client of the round in ONE launch set per
// batch-step (fused_cnn.hip).  Caller provides the per-client
// metadata both on device (kernel use) and host (max_batches), the
// K*P parameter/gradient stacks and a float workspace sliced here.
// validates the DGA argument group shared by cnn_round_mega and
// mega_dga_accum; returns dga_out's pointer (4K doubles)
static double* dga_check(int64_t mode, double beta, bool clip,
                         double max_grad,
                         const c10::optional<torch::Tensor>& dga_out,
                         int64_t K, DgaArgs* out) {
  TORCH_CHECK(mode >= DGA_MEAN && mode <= DGA_MAG, "dga_mode out of range");
  TORCH_CHECK(K > 0 && K <= DGA_MAX_K, "the DGA tail takes K <= ", DGA_MAX_K);
  TORCH_CHECK(!clip || max_grad > 0.0, "dga clip needs max_grad > 0");
  TORCH_CHECK(dga_out.has_value() && dga_out->is_cuda() &&
              dga_out->is_contiguous() &&
              dga_out->scalar_type() == torch::kFloat64 &&
              dga_out->numel() >= 4 * K,
              "dga_out must hold 4K float64 on the device");
  out->mode = (int)mode;
  out->clip = clip ? 1 : 0;
  out->beta = beta;
  out->max_grad = max_grad;
  return dga_out->data_ptr<double>();
}

void cnn_round_mega(torch::Tensor shard_x, torch::Tensor shard_y,
                    torch::Tensor orders_dev, torch::Tensor row_bases_dev,
                    torch::Tensor order_offs_dev, torch::Tensor counts_dev,
                    torch::Tensor counts_host, torch::Tensor weights_dev,
                    torch::Tensor seeds_dev, int64_t bs, int64_t C,
                    torch::Tensor server_params, torch::Tensor params_stack,
                    torch::Tensor grads_stack, torch::Tensor round_accum,
                    torch::Tensor work_f, torch::Tensor work_i,
                    torch::Tensor work_b, torch::Tensor work_d,
                    torch::Tensor lr_t, double max_norm, double p1,
                    double p2, torch::Tensor stats_out,
                    torch::Tensor loss_out, bool use_bf16, double mu,
                    int64_t dga_mode, double dga_beta, bool dga_clip,
                    double dga_max_grad,
                    c10::optional<torch::Tensor> dga_out) {
  TORCH_CHECK(mu >= 0.0, "mu must be >= 0");
  // DGA group (dga_mode >= 0): the round ends in the DGA tail
  DgaArgs dga_args;
  double* dga_out_p = nullptr;
  const bool has_dga = dga_mode >= 0;
  if (has_dga)
    dga_out_p = dga_check(dga_mode, dga_beta, dga_clip, dga_max_grad,
                          dga_out, counts_host.numel(), &dga_args);
  check_flat(server_params, "server_params");
  check_flat(params_stack, "params_stack");
  check_flat(grads_stack, "grads_stack");
  check_flat(round_accum, "round_accum");
  check_flat(work_f, "work_f");
  TORCH_CHECK(orders_dev.is_cuda() && row_bases_dev.is_cuda() &&
              order_offs_dev.is_cuda() && counts_dev.is_cuda() &&
              weights_dev.is_cuda() && seeds_dev.is_cuda(),
              "mega metadata must be device tensors");
  TORCH_CHECK(!counts_host.is_cuda() &&
              counts_host.scalar_type() == torch::kInt64);
  int K = (int)counts_host.numel();
  TORCH_CHECK(row_bases_dev.numel() == K && order_offs_dev.numel() == K &&
              counts_dev.numel() == K && weights_dev.numel() == K &&
              seeds_dev.numel() == K, "metadata lengths must equal K");
  TORCH_CHECK(bs >= 1 && bs <= 32);
  long long P = server_params.numel();
  TORCH_CHECK(params_stack.numel() >= (long long)K * P &&
              grads_stack.numel() >= (long long)K * P,
              "parameter stacks too small");
  TORCH_CHECK(stats_out.numel() >= 2 * K && loss_out.numel() >= K);
  TORCH_CHECK(row_bases_dev.scalar_type() == torch::kInt64 &&
              order_offs_dev.scalar_type() == torch::kInt64 &&
              counts_host.is_contiguous() && counts_host.dim() == 1);
  // the mega driver rejects empty clients
  check_client_meta(shard_x, shard_y, orders_dev, row_bases_dev.cpu(),
                    order_offs_dev.cpu(), counts_host, /*allow_empty=*/false);
  CnnWorkspace ws = slice_ws(work_f, work_i, work_b, (long long)K * bs, K, C);
  TORCH_CHECK(work_d.numel() >= (mu > 0.0 ? 3 : 2) * K,
              "mega double workspace too small");
  launch_cnn_round_mega(
      shard_x.data_ptr<float>(),
      reinterpret_cast<const long long*>(shard_y.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(orders_dev.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(row_bases_dev.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(order_offs_dev.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(counts_dev.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(counts_host.data_ptr<int64_t>()),
      weights_dev.data_ptr<float>(),
      reinterpret_cast<const long long*>(seeds_dev.data_ptr<int64_t>()),
      K, (int)bs, (int)C, server_params.data_ptr<float>(),
      params_stack.data_ptr<float>(), grads_stack.data_ptr<float>(),
      round_accum.data_ptr<float>(), ws, work_d.data_ptr<double>(),
      lr_t.data_ptr<float>(), (float)max_norm, (float)p1, (float)p2,
      stats_out.data_ptr<float>(), loss_out.data_ptr<float>(),
      cur_stream(), use_bf16 ? 1 : 0, (float)mu,
      has_dga ? &dga_args : nullptr, dga_out_p);
}

// per-client clip + sufficient stats + SGD over a K-stacked flat arena
// (graph-capture safe; stats_out[2k] accumulates clipped Σg / Σg²)
void mega_clip_sgd(torch::Tensor params_stack, torch::Tensor grads_stack,
                   int64_t K, torch::Tensor acc2k, double max_norm,
                   torch::Tensor lr_t, torch::Tensor stats_out,
                   c10::optional<torch::Tensor> server, double mu,
                   c10::optional<torch::Tensor> active,
                   c10::optional<torch::Tensor> loss_out) {
  check_flat(params_stack, "params_stack");
  check_flat(grads_stack, "grads_stack");
  check_flat(lr_t, "lr_t"); check_flat(stats_out, "stats_out");
  TORCH_CHECK(K > 0 && params_stack.numel() % K == 0 &&
              params_stack.numel() == grads_stack.numel());
  TORCH_CHECK(acc2k.is_cuda() && acc2k.scalar_type() == torch::kFloat64 &&
              acc2k.numel() >= (mu > 0.0 ? 3 : 2) * K);
  TORCH_CHECK(stats_out.numel() >= 2 * K);
  long long P = params_stack.numel() / K;
  // FedProx (mu > 0): gp = g + mu (w - server) for the clients whose
  // `active` byte is set (absent = all); loss_out[k] += 0.5 mu ||w - server||^2
  const float* server_p = prox_server(server, mu, P);
  const unsigned char* active_p = nullptr;
  float* loss_p = nullptr;
  if (mu > 0.0 && active.has_value()) {
    TORCH_CHECK(active->is_cuda() && active->is_contiguous() &&
                (active->scalar_type() == torch::kBool ||
                 active->scalar_type() == torch::kUInt8) &&
                active->numel() == K, "active must be K bool/uint8 on device");
    active_p = static_cast<const unsigned char*>(active->data_ptr());
  }
  if (mu > 0.0 && loss_out.has_value()) {
    check_flat(*loss_out, "loss_out");
    TORCH_CHECK(loss_out->numel() >= K);
    loss_p = loss_out->data_ptr<float>();
  }
  launch_mega_clip_sgd(params_stack.data_ptr<float>(),
                       grads_stack.data_ptr<float>(), P, (int)K,
                       acc2k.data_ptr<double>(), (float)max_norm,
                       lr_t.data_ptr<float>(), stats_out.data_ptr<float>(),
                       cur_stream(), server_p, (float)mu, active_p, loss_p);
}

void mega_pseudo_accum(torch::Tensor grads_stack, torch::Tensor server,
                       torch::Tensor params_stack, torch::Tensor weights_dev,
                       torch::Tensor round_accum) {
  check_flat(grads_stack, "grads_stack"); check_flat(server, "server");
  check_flat(params_stack, "params_stack");
  check_flat(weights_dev, "weights_dev");
  check_flat(round_accum, "round_accum");
  long long P = server.numel();
  TORCH_CHECK(P > 0 && params_stack.numel() % P == 0);
  int K = (int)(params_stack.numel() / P);
  TORCH_CHECK(weights_dev.numel() >= K && round_accum.numel() == P &&
              grads_stack.numel() == params_stack.numel());
  launch_mega_pseudo_accum(grads_stack.data_ptr<float>(),
                           server.data_ptr<float>(),
                           params_stack.data_ptr<float>(),
                           weights_dev.data_ptr<float>(),
                           round_accum.data_ptr<float>(), P, K,
                           cur_stream());
}

// DGA end-of-round tail over a K-stacked flat arena (graph-capture safe:
// no host sync, no allocation): softmax weight and clip-only local DP
// formed on the device, accumulated into ``accum``; dga_out[4K] f64 =
// weight_k, norm_k, c_k, scratch
void mega_dga_accum(torch::Tensor params_stack, torch::Tensor server,
                    int64_t K, torch::Tensor loss, torch::Tensor stats,
                    torch::Tensor counts, int64_t bs, int64_t dga_mode,
                    double dga_beta, bool dga_clip, double dga_max_grad,
                    torch::Tensor accum, torch::Tensor dga_out) {
  check_flat(params_stack, "params_stack"); check_flat(server, "server");
  check_flat(loss, "loss"); check_flat(stats, "stats");
  check_flat(accum, "accum");
  long long P = server.numel();
  TORCH_CHECK(P > 0 && K > 0 && params_stack.numel() == K * P &&
              accum.numel() == P, "stack / server / accum sizes disagree");
  TORCH_CHECK(loss.numel() >= K && stats.numel() >= 2 * K);
  TORCH_CHECK(counts.is_cuda() && counts.is_contiguous() &&
              counts.scalar_type() == torch::kInt64 && counts.numel() >= K,
              "counts must be K int64 on the device");
  TORCH_CHECK(bs >= 1);
  DgaArgs a;
  double* out = dga_check(dga_mode, dga_beta, dga_clip, dga_max_grad,
                          dga_out, K, &a);
  launch_mega_dga_accum(
      params_stack.data_ptr<float>(), server.data_ptr<float>(), P, (int)K,
      loss.data_ptr<float>(), stats.data_ptr<float>(),
      reinterpret_cast<const long long*>(counts.data_ptr<int64_t>()),
      (int)bs, a, accum.data_ptr<float>(), out, cur_stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  // output rows per block of the f32 conv2 forward (its slab seams)
  m.attr("CONV2_FWD_SLAB_ROWS") = CONV2_FWD_SLAB_ROWS;
  // FedProx arguments trail with defaults: the FedAvg positional calls
  // stay as they were
  m.def("cnn_round_mega", &cnn_round_mega,
        py::arg("shard_x"), py::arg("shard_y"), py::arg("orders_dev"),
        py::arg("row_bases_dev"), py::arg("order_offs_dev"), py::arg("counts_dev"), py::arg("counts_host"), py::arg("weights_dev"), py::arg("seeds_dev"), py::arg("bs"), py::arg("C"), py::arg("server_params"), py::arg("params_stack"), py::arg("grads_stack"), py::arg("round_accum"), py::arg("work_f"), py::arg("work_i"), py::arg("work_b"), py::arg("work_d"), py::arg("lr_t"), py::arg("max_norm"), py::arg("p1"), py::arg("p2"), py::arg("stats_out"), py::arg("loss_out"), py::arg("use_bf16"),
        py::arg("mu") = 0.0,
        // DGA group: dga_mode < 0 = absent (the FedAvg / FedProx tail)
        py::arg("dga_mode") = -1, py::arg("dga_beta") = 0.0,
        py::arg("dga_clip") = false, py::arg("dga_max_grad") = 0.0,
        py::arg("dga_out") = py::none());
  m.def("mega_dga_accum", &mega_dga_accum,
        py::arg("params_stack"), py::arg("server"), py::arg("K"),
        py::arg("loss"), py::arg("stats"), py::arg("counts"), py::arg("bs"),
        py::arg("dga_mode"), py::arg("dga_beta"), py::arg("dga_clip"),
        py::arg("dga_max_grad"), py::arg("accum"), py::arg("dga_out"));
  m.attr("DGA_MODES") = py::dict(
      py::arg("mean") = (int)DGA_MEAN,
      py::arg("train_loss") = (int)DGA_TRAIN_LOSS,
      py::arg("mag_var_loss") = (int)DGA_MAG_VAR,
      py::arg("mag_mean_loss") = (int)DGA_MAG_MEAN,
      py::arg("mag") = (int)DGA_MAG);
  m.def("mega_clip_sgd", &mega_clip_sgd,
        py::arg("params_stack"), py::arg("grads_stack"), py::arg("K"), py::arg("acc2k"), py::arg("max_norm"), py::arg("lr_t"), py::arg("stats_out"),
        py::arg("server") = py::none(), py::arg("mu") = 0.0,
        py::arg("active") = py::none(), py::arg("loss_out") = py::none());
  m.def("mega_pseudo_accum", &mega_pseudo_accum);
  m.def("dbg_mfma_bf16_probe", &dbg_mfma_bf16_probe);
  m.def("dbg_conv2_fwd_mfma_bf16", &dbg_conv2_fwd_mfma_bf16);
  m.def("dbg_conv2_bwd_x_mfma_bf16", &dbg_conv2_bwd_x_mfma_bf16);
  m.def("dbg_conv2_bwd_w_mfma_bf16", &dbg_conv2_bwd_w_mfma_bf16,
        py::arg("dz2"), py::arg("a1"), py::arg("B"), py::arg("K") = 1);
  m.def("dbg_fc1_fwd_mfma_bf16", &dbg_fc1_fwd_mfma_bf16);
  m.def("dbg_conv2_fwd_mfma", &dbg_conv2_fwd_mfma);
  m.def("dbg_conv2_fwd_pool_mfma", &dbg_conv2_fwd_pool_mfma);
  m.def("dbg_pool_drop_bwd_bias", &dbg_pool_drop_bwd_bias);
  m.def("dbg_conv2_bwd_x_mfma", &dbg_conv2_bwd_x_mfma);
  m.def("dbg_conv2_bwd_w_mfma", &dbg_conv2_bwd_w_mfma,
        py::arg("dz2"), py::arg("a1"), py::arg("B"), py::arg("K") = 1);
  m.def("dbg_fc1_fwd_mfma", &dbg_fc1_fwd_mfma);
  m.def("dbg_fc1_bwd_w_mfma", &dbg_fc1_bwd_w_mfma,
        py::arg("dz3"), py::arg("a2"), py::arg("B"), py::arg("K") = 1);
  m.def("dbg_fc1_bwd_x_mfma", &dbg_fc1_bwd_x_mfma);
  m.doc() = "msrflute_amd gfx950 flat-arena kernels";
  m.def("pseudo_grad", &pseudo_grad);
  m.def("axpy", &axpy);
  m.def("scale", &scale);
  m.def("sum_sumsq", &sum_sumsq);
  m.def("clip_by_norm", &clip_by_norm);
  m.def("add_gaussian_noise", &add_gaussian_noise);
  m.def("sgd_step", &sgd_step);
  m.def("sgd_step_devlr", &sgd_step_devlr);
  m.def("clip_stats_accumulate", &clip_stats_accumulate);
  m.def("adam_step", &adam_step);
  m.def("adamax_step", &adamax_step);
  m.def("segmented_sqnorm", &segmented_sqnorm);
  m.def("quant_bin_mask", &quant_bin_mask);
  m.def("gru_gates", &gru_gates);
  m.def("cnn_workspace_sizes", &cnn_workspace_sizes_py,
        "(n_float, n_int, n_byte) of the CNN workspace of G rows over K "
        "clients with C classes");
  m.def("cnn_epoch", &cnn_epoch,
        py::arg("shard_x"), py::arg("shard_y"), py::arg("order"), py::arg("bs"), py::arg("C"), py::arg("params"), py::arg("grads"), py::arg("work_f"), py::arg("work_i"), py::arg("work_b"), py::arg("work_d"), py::arg("lr_t"), py::arg("max_norm"), py::arg("p1"), py::arg("p2"), py::arg("stats_acc"), py::arg("loss_acc"), py::arg("seed"), py::arg("use_bf16"),
        py::arg("server") = py::none(), py::arg("mu") = 0.0);
  m.def("cnn_round", &cnn_round,
        py::arg("shard_x"), py::arg("shard_y"), py::arg("orders_dev"), py::arg("row_bases"), py::arg("order_offs"), py::arg("counts"), py::arg("weights"), py::arg("seeds"), py::arg("bs"), py::arg("C"), py::arg("server_params"), py::arg("params"), py::arg("grads"), py::arg("round_accum"), py::arg("work_f"), py::arg("work_i"), py::arg("work_b"), py::arg("work_d"), py::arg("lr_t"), py::arg("max_norm"), py::arg("p1"), py::arg("p2"), py::arg("stats_out"), py::arg("loss_out"), py::arg("use_bf16"),
        py::arg("mu") = 0.0);
  m.def("lstm_seq_fwd", &lstm_seq_fwd);
  m.def("gru_seq_fwd", &gru_seq_fwd);
  m.def("gru_seq_bwd", &gru_seq_bwd);
  m.def("lstm_seq_bwd", &lstm_seq_bwd);
}
