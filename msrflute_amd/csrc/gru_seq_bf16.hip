// Fused GRU sequence recurrence for gfx950 (nlg_gru task): the
// instantiation of the kernels in gru_seq_body.h for bf16-stored W_hh (raw
// 16-bit words; 16-byte aligned packs).
//
// This file alone is compiled with -Xclang -target-feature -Xclang
// -packed-fp32-ops (setup.py).  Left to itself the vectoriser pairs parts
// of the fmaf chains into v_pk_fma_f32 and pays in v_mov_b32 for the
// aligned register pairs; measured at B = 64, T = 25 with the shipped
// resident / unroll counts, the scalar form runs the forward in 313 us
// against 342 us and the backward in 341 us against 333 us
// (profiles/r07_gru_bf16_stats.md), and the counts were tuned under it.

#include "gru_seq_body.h"

extern "C" {

void launch_gru_seq_fwd_bf16(const float* gi, const unsigned short* whh_t,
                             const float* b_hh, float* h_seq, float* gates,
                             float* ghn, int B, int T, hipStream_t s) {
  gru_fwd<GWBF16>(gi, whh_t, b_hh, h_seq, gates, ghn, B, T, s);
}

void launch_gru_seq_bwd_bf16(const float* gates, const float* ghn,
                             const float* h_seq, const unsigned short* w_hh,
                             const float* dh_out, float* dgi, float* dgh,
                             int B, int T, hipStream_t s) {
  gru_bwd<GWBF16>(gates, ghn, h_seq, w_hh, dh_out, dgi, dgh, B, T, s);
}

}  // extern "C"
