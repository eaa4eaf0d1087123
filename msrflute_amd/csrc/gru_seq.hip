// Fused GRU sequence recurrence for gfx950 (nlg_gru task): the fp32
// instantiation of the kernels in gru_seq_body.h.

#include "gru_seq_body.h"

extern "C" {

void launch_gru_seq_fwd(const float* gi, const float* whh_t,
                        const float* b_hh, float* h_seq, float* gates,
                        float* ghn, int B, int T, hipStream_t s) {
  gru_fwd<GWF32>(gi, whh_t, b_hh, h_seq, gates, ghn, B, T, s);
}

void launch_gru_seq_bwd(const float* gates, const float* ghn,
                        const float* h_seq, const float* w_hh,
                        const float* dh_out, float* dgi, float* dgh,
                        int B, int T, hipStream_t s) {
  gru_bwd<GWF32>(gates, ghn, h_seq, w_hh, dh_out, dgi, dgh, B, T, s);
}

}  // extern "C"
