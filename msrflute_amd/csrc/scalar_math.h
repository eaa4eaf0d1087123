// exp and tanh on builtins, for kernels compiled without gfx950's packed
// fp32 VALU ops: lstm_seq.hip (small-H recurrence) and attn_pool.hip.
//
// SCALAR_F32 takes the packed ops away from one function (device pass only;
// the host pass does not know the feature).  A function with its own target
// features cannot inline the device library or the HIP headers, so the
// transcendentals are written here on builtins, always inlined.
#pragma once

#if defined(__HIP_DEVICE_COMPILE__)
#define SCALAR_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define SCALAR_F32
#endif
#define SCALAR_INL __device__ __forceinline__ SCALAR_F32

// e^x for |x| <= 87 (clamped: every result stays a finite normal):
// v_exp_f32 (1 ulp) on x * log2(e), with the rounding error of that
// product, which |x| would amplify, put back to first order.  The clamp
// is two compare-and-selects, not fmin / fmax: v_min_f32 / v_max_f32
// return the operand that is not a NaN, and a NaN pre-activation (a
// client that diverged upstream) has to come out of sig_s and tanh_s as
// NaN, as it does out of nn.LSTM and the H = 256 kernels.
SCALAR_INL float exp_s(float x) {
  x = x < -87.f ? -87.f : x;
  x = x > 87.f ? 87.f : x;
  const float l2e_hi = 1.44269502e+0f, l2e_lo = 1.92596299e-8f;
  float t = x * l2e_hi;
  float r = __builtin_fmaf(x, l2e_lo, __builtin_fmaf(x, l2e_hi, -t));
  float e = __builtin_amdgcn_exp2f(t);
  return __builtin_fmaf(e, r * 0.693147181f, e);
}

// tanh: below 0.625 an odd polynomial x + x^3 p(x^2); above it
// 1 - 2/(e^2x + 1), where the subtraction no longer cancels (it
// saturates to 1 through the clamp of exp_s).  p is the degree-4
// least-squares fit of (tanh(x)/x - 1)/x^2 in t = x^2 at 400 Chebyshev
// nodes of [0, 0.625^2], computed in float64 (numpy
// Chebyshev.fit -> power basis) and rounded to float32; evaluated as
// below in float32 its largest relative error over the interval is
// 1.42 * 2^-24.  tests/test_lstm_small_gpu.py walks the gate inputs
// across the branch point and into saturation against float64.
SCALAR_INL float tanh_s(float y) {
  float x = __builtin_fabsf(y);
  float t = x * x;
  float p = -0x1.9017fep-8f;
  p = __builtin_fmaf(p, t, 0x1.581fa6p-6f);
  p = __builtin_fmaf(p, t, -0x1.b928e0p-5f);
  p = __builtin_fmaf(p, t, 0x1.110e2ep-3f);
  p = __builtin_fmaf(p, t, -0x1.555552p-2f);
  float small = __builtin_fmaf(t, x * p, x);
  float big = 1.f - 2.f / (exp_s(2.f * x) + 1.f);
  return __builtin_copysignf(x < 0.625f ? small : big, y);
}
