// pt_postprocess_reference.hpp — the post-process tone map in the REFERENCE arithmetic
// (pt_present_set_arithmetic(h, PT_ARITH_REFERENCE)); included by pt_integrate_reference.hip only.
//   OpenTK-PathTracer/res/shaders/PostProcessing/fragment.glsl:17-44 (ACESFilm, LinearToInverseGamma), run by ScreenEffect.Render
// restated with llvmpipe's arithmetic choices (oracle base variant 951; the primitives: pt_math_reference.hpp), per channel:
//   num = x (2.51 x + 0.03), den = x (2.43 x + 0.59) + 0.14      two roundings per multiply-add (the unit is built with -ffp-contract=off)
//   v   = clamp(num / den, 0, 1)                                  a true, correctly rounded division; IEEE minNum / maxNum
//   hi  = pow(v, 1 / 2.4) 1.055 - 0.055                           gallivm's pow = exp2(log2(v) y); the exponent is the float 0.41666666f
//                                                                 (folded or divided at run time: the same float); unfused
//   lo  = v 12.92
//   out = v < 0.0031308 ? lo : hi
// The last line is a SELECT.  The shader writes mix(hi, lo, vec3(lessThan(..))), and elsewhere r_mix restates mix(x, y, a) as
// x + a (y - x); with a = 1 that form gives hi + (lo - hi), which is not lo: it reproduces only 90.5 % of the values of
// tests/golden/post_aces_gamma.npz, the select all 18,432 of them bit for bit (negative and 1e6 inputs included).
//
// Shared with the contract (pt_math.hpp), because the fixture holds the shader's FLOAT colour and llvmpipe's framebuffer conversion is
// not pinned by it: float -> unorm8 is round-half-up of clamp(v, 0, 1) 255, and alpha is 255.  A NaN colour is clamped by minNum /
// maxNum, so a NaN quotient (NaN and +-inf inputs: inf / inf) becomes 0; the reference's data holds no such value.
//
// Everything is __host__ __device__ so that a CPU test compiles this header for the host (with PT_REFERENCE_PRIMITIVES_ONLY) and compares
// it with the fixture bit for bit; the GPU tests then compare the kernel with that host build.
#pragma once
#include "pt_math_reference.hpp"

namespace pt {
namespace ref {

// fragment.glsl:36-44 ACESFilm, per channel
PT_HD float aces_film_ref(float x)
{
    const float num = x * (2.51f * x + 0.03f);
    const float den = x * (2.43f * x + 0.59f) + 0.14f;
    return __builtin_fminf(__builtin_fmaxf(r_div(num, den), 0.0f), 1.0f);
}

// fragment.glsl:28-32 LinearToInverseGamma(v, 2.4), per channel
PT_HD float linear_to_inverse_gamma_ref(float v)
{
    const float hi = ll_pow(v, 0.41666666f) * 1.055f - 0.055f;
    const float lo = v * 12.92f;
    return v < 0.0031308f ? lo : hi;
}

// the float stage: what the fragment shader writes for one channel
PT_HD float postprocess_channel_ref(float x) { return linear_to_inverse_gamma_ref(aces_film_ref(x)); }

// float -> unorm8, the contract's conversion: a copy of pt_math.hpp's to_unorm8 (that one is __device__ only, this header is also compiled
// for the host) that must stay the same function — tests/test_gpu_reference_postprocess.py compares the two kernels' conversions of
// equal float colours through the oracle on the reference's fixture
PT_HD unsigned char to_unorm8_ref(float v) { return (unsigned char)(int)(__builtin_fminf(__builtin_fmaxf(v, 0.0f), 1.0f) * 255.0f + 0.5f); }

// one pixel of the pass: RGBA32F accumulation -> RGBA8, alpha = 255
PT_HD uchar4 postprocess_pixel_ref(float4 c)
{
    uchar4 o;
    o.x = to_unorm8_ref(postprocess_channel_ref(c.x));
    o.y = to_unorm8_ref(postprocess_channel_ref(c.y));
    o.z = to_unorm8_ref(postprocess_channel_ref(c.z));
    o.w = 255;
    return o;
}

} // namespace ref
} // namespace pt
