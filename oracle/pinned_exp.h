// pinned_exp.h — the project's pinned fp32 exp, shared by the CPU oracle (oracle.cpp) and by the execution model that
// runs the reference's own kernels on the host (ref_shim/).  TEST INFRASTRUCTURE ONLY.
//
// `exp` is the one libm call on a decision path of the rasteriser; CUDA's expf bits are unobtainable here, so every side
// of every parity test resolves `exp(power)` to this fully specified routine (Cephes-style, <= 1 ulp typical), which the
// HIP kernels restate operation for operation.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

// float -> int conversion with the GPU's saturating semantics (cvt.rzi.s32.f32 on the
// reference's hardware, v_cvt_i32_f32 on gfx950): truncate toward zero, clamp, NaN -> 0.
static inline int f2i_sat(float v) {
  if (v != v) return 0;
  if (v >= 2147483648.0f) return 2147483647;
  if (v <= -2147483648.0f) return (int)0x80000000;
  return (int)v;
}

static inline float bits2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline uint32_t f2bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// Valid for x <= 88; x is clamped below at -87 (the result, ~1.6e-38, times any opacity <= 1 is far under the 1/255
// alpha floor).
static inline float pinned_expf(float x) {
  x = (x < -87.0f) ? -87.0f : x;
  x = (x > 88.0f) ? 88.0f : x;
  float n = std::nearbyintf(x * 1.44269504088896341f);  // round-half-even
  float r = __builtin_fmaf(n, -0.693359375f, x);
  r = __builtin_fmaf(n, 2.12194440e-4f, r);
  float p = 1.9875691500e-4f;
  p = __builtin_fmaf(p, r, 1.3981999507e-3f);
  p = __builtin_fmaf(p, r, 8.3334519073e-3f);
  p = __builtin_fmaf(p, r, 4.1665795894e-2f);
  p = __builtin_fmaf(p, r, 1.6666665459e-1f);
  p = __builtin_fmaf(p, r, 5.0000001201e-1f);
  float e = __builtin_fmaf(p, r * r, r) + 1.0f;
  // (n is NaN for a NaN argument: `(int)n` would be undefined.  f2i_sat is the device's v_cvt_i32_f32, 0 for a NaN, and
  //  e * 2^0 is still NaN; for every other argument n is an integer in [-126, 127] and the conversion is exact)
  int ni = f2i_sat(n);
  return e * bits2f((uint32_t)(ni + 127) << 23);
}
