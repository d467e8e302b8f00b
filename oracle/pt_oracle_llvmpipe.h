/*
 * pt_oracle_llvmpipe.h — llvmpipe's sin, cos, exp, pow, exp2, log2 restated: THE ORACLE OF THE SHIPPED REFERENCE-ARITHMETIC MODES
 * (pt_set_arithmetic, pt_atmosphere_set_arithmetic, pt_present_set_arithmetic are checked against the witness library at
 * pt_oracle.LLVMPIPE = base variant 951, whose bit 128 selects these).  TEST INFRASTRUCTURE ONLY; included by
 * oracle/study/pt_oracle_witness.c after the contract (it uses the contract's f_bits / f_unbits).
 *
 * base variant bit 128: sin, cos, exp, pow the way llvmpipe's gallivm evaluates them (Mesa, src/gallium/auxiliary/gallivm/lp_bld_arit.c —
 * a third-party dependency of the REFERENCE'S TEST RIG, absent from /root/reference; restated from its published algorithm and pinned by
 * black-box probing: tests/test_arithmetic_choices.py runs the GLSL built-ins on the live llvmpipe through oracle/_ref/glsl_runner and
 * finds these functions BIT-IDENTICAL on 65,536 arguments each).  sin / cos: the Cephes-derived SSE routine (reduction by pi/4 in three
 * steps, j = (int(|x| 4/pi) + 1) & ~1, two minimax polynomials, multiply-adds fused).  exp2: floor / fraction split, degree-5 polynomial of
 * the fraction evaluated as even and odd halves with fused multiply-adds, scaled by 2^floor.  log2: exponent + y P(y^2) with
 * y = (m - 1) / (m + 1), degree-4 P, same evaluation.  exp(x) = exp2(x log2 e), pow(x, y) = exp2(log2(x) y): negative base NaN, zero 0.
 */
#ifndef PT_ORACLE_LLVMPIPE_H
#define PT_ORACLE_LLVMPIPE_H
static inline float ll_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
static float ll_poly(float x, const float *co, int n) /* lp_build_polynomial: even and odd powers separately, then odd * x + even */
{
    const float x2 = x * x;
    float even = 0.0f, odd = 0.0f;
    int haveEven = 0, haveOdd = 0;
    for (int i = n; i--;) {
        if ((i & 1) == 0) { even = haveEven ? ll_fma(x2, even, co[i]) : co[i]; haveEven = 1; }
        else { odd = haveOdd ? ll_fma(x2, odd, co[i]) : co[i]; haveOdd = 1; }
    }
    return haveOdd ? ll_fma(odd, x, even) : even;
}
static float ll_exp2(float x)
{
    static const float co[6] = { 1.000000000000000000000f, 0.693153073200168932794f, 0.240153617044375388211f, 0.0558263180532956664775f,
                                 0.00898934009049466391101f, 0.00187757667519147912699f };
    if (x != x) return x;
    if (x > 128.0f) x = 128.0f;
    if (x < -126.99999f) x = -126.99999f;
    const float ip = floorf(x), fp = x - ip;
    return f_unbits((uint32_t)((int)ip + 127) << 23) * ll_poly(fp, co, 6);
}
static float ll_log2(float x)
{
    static const float co[5] = { 2.88539009343309178325f, 0.961791550404184197881f, 0.577440339438736392009f, 0.403343858251329912514f,
                                 0.406718052498846252698f };
    if (x != x || x < 0.0f) return NAN;
    if (x == 0.0f) return -INFINITY;
    if (isinf(x)) return x;
    const uint32_t i = f_bits(x);
    const float e = (float)((int)((i >> 23) & 0xffu) - 127);
    const float m = f_unbits((i & 0x007fffffu) | 0x3f800000u);
    const float y = (m - 1.0f) / (m + 1.0f);
    return ll_fma(y, ll_poly(y * y, co, 5), e);
}
static float ll_exp(float x) { return ll_exp2(x * 1.44269504088896340735992f); }
static float ll_pow(float x, float y)
{
    if (x != x) return 0.0f; /* (measured: pow(NaN, 5.0) = 0 on llvmpipe) */
    if (x == 0.0f) return 0.0f;
    return ll_exp2(ll_log2(x) * y);
}
static float ll_sin_or_cos(float a, int want_cos)
{
    const float x_abs = fabsf(a);
    int j = (int)(x_abs * 1.27323954473516f);
    j = (j + 1) & ~1;
    const float y = (float)j;
    const int j2 = want_cos ? j - 2 : j;
    const uint32_t sign = want_cos ? ((~(uint32_t)j2 & 4u) << 29) : ((((uint32_t)j2 & 4u) << 29) ^ (f_bits(a) & 0x80000000u));
    float x = ll_fma(y, -0.78515625f, x_abs);
    x = ll_fma(y, -2.4187564849853515625e-4f, x);
    x = ll_fma(y, -3.77489497744594108e-8f, x);
    const float z = x * x;
    float c = ll_fma(z, 2.443315711809948E-005f, -1.388731625493765E-003f);
    c = ll_fma(c, z, 4.166664568298827E-002f);
    c = c * z; c = c * z;
    c = ll_fma(z, -0.5f, c); c = c + 1.0f;
    float sv = ll_fma(z, -1.9515295891E-4f, 8.3321608736E-3f);
    sv = ll_fma(sv, z, -1.6666654611E-1f);
    sv = sv * z;
    sv = ll_fma(sv, x, x);
    return f_unbits(f_bits((j2 & 2) == 0 ? sv : c) ^ sign);
}
#endif
