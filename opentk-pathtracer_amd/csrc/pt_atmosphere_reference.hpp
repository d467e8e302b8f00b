// pt_atmosphere_reference.hpp — the atmosphere environment precompute in the REFERENCE arithmetic
// (pt_atmosphere_set_arithmetic(h, PT_ARITH_REFERENCE)); included by pt_integrate_reference.hip only.
//   OpenTK-PathTracer/res/shaders/AtmosphericScattering/compute.glsl:30-171
//
// Specification: oracle/pt_oracle.c's atmosphere() / atmo_rsi() / atmo_worker() built with -DPT_ORACLE_PERTURB after
// pto_set_base_variant(951), operation for operation, over the primitives of pt_math_reference.hpp:
//   - every a * b + c has two roundings (-ffp-contract=off keeps a written a * b + c as v_mul + v_add);
//   - sqrt, 1 / x and a / b are correctly rounded; normalize = v * (1 / sqrt(dot));
//   - dot sums ax bx + (az bz + ay by), mat4 * vec4 sums cy y + (cz z + (cx x + cw w));
//   - every exp is llvmpipe's (ll_exp).
// The oracle's EXPRESSION FORMS are kept even where they are the contract's and not the shader's, because they are what the
// cubes were measured with: sy * (1 / jSteps) with an IEEE reciprocal, one 1 / (2 a) shared by both roots of
// atmo_rsi, exp(h * (-1 / sh)).  sqrt(base) and the uniform constants are plain IEEE in both arithmetics.
//
// Everything here is __host__ __device__ and free of device-side types, so that a CPU test compiles it for the host
// (-DPT_REFERENCE_PRIMITIVES_ONLY) and compares whole cubes with the oracle bit for bit.
#pragma once
#include "pt_math_reference.hpp"

namespace pt {
namespace ref {

PT_HD float r_min(float a, float b) { return __builtin_fminf(a, b); }

PT_HD void atmo_rsi_ref(v3 r0, v3 rd, float sr, float &x, float &y) // :58-71
{
    const float a = r_dot(rd, rd);
    const float b = 2.0f * r_dot(rd, r0);
    const float c = -sr * sr + r_dot(r0, r0);
    const float d = b * b + -(4.0f * a * c);
    if (d < 0.0f) { x = 1e5f; y = -1e5f; return; }
    const float sq = r_sqrt(d), rden = r_rcp(2.0f * a);
    x = (-b - sq) * rden;
    y = (-b + sq) * rden;
}

PT_HD v3 atmosphere_ref(v3 r, v3 r0, v3 pSun, float iSun, float rPlanet, float rAtmos, v3 kRlh, float kMie, float shRlh,
                        float shMie, float g, int iSteps, int jSteps) // :73-159
{
    pSun = r_normalize(pSun);
    r = r_normalize(r);
    float px, py, qx, qy;
    atmo_rsi_ref(r0, r, rAtmos, px, py);
    if (px > py) return r_V(0.0f, 0.0f, 0.0f);
    atmo_rsi_ref(r0, r, rPlanet, qx, qy);
    py = r_min(py, qx);
    const float iStepSize = (py - px) / (float)iSteps;
    float iTime = 0.0f;
    v3 totalRlh = r_V(0.0f, 0.0f, 0.0f), totalMie = r_V(0.0f, 0.0f, 0.0f);
    float iOdRlh = 0.0f, iOdMie = 0.0f;
    const float mu = r_dot(r, pSun), mumu = mu * mu, gg = g * g;
    const float pRlh = 3.0f / (16.0f * PI) * (1.0f + mumu);
    const float base = 1.0f + gg - 2.0f * mu * g;
    const float pMie = 3.0f / (8.0f * PI) * ((1.0f - gg) * (mumu + 1.0f)) / ((base * r_sqrt(base)) * (2.0f + gg));
    const float invShRlh = -1.0f / shRlh, invShMie = -1.0f / shMie;
    const float invJSteps = 1.0f / (float)jSteps; // uniform
    for (int i = 0; i < iSteps; i++) {
        const v3 iPos = r_madd(r, iStepSize * 0.5f + iTime, r0);
        const float iHeight = r_sqrt(r_dot(iPos, iPos)) - rPlanet;
        const float odStepRlh = ll_exp(iHeight * invShRlh) * iStepSize;
        const float odStepMie = ll_exp(iHeight * invShMie) * iStepSize;
        iOdRlh += odStepRlh;
        iOdMie += odStepMie;
        float sx, sy;
        atmo_rsi_ref(iPos, pSun, rAtmos, sx, sy);
        const float jStepSize = sy * invJSteps;
        float jTime = 0.0f, jOdRlh = 0.0f, jOdMie = 0.0f;
        for (int j = 0; j < jSteps; j++) {
            const v3 jPos = r_madd(pSun, jStepSize * 0.5f + jTime, iPos);
            const float jHeight = r_sqrt(r_dot(jPos, jPos)) - rPlanet;
            jOdRlh = ll_exp(jHeight * invShRlh) * jStepSize + jOdRlh;
            jOdMie = ll_exp(jHeight * invShMie) * jStepSize + jOdMie;
            jTime += jStepSize;
        }
        const float mieTerm = kMie * (iOdMie + jOdMie), rl = iOdRlh + jOdRlh;
        const v3 attn = r_V(ll_exp(-(kRlh.x * rl + mieTerm)), ll_exp(-(kRlh.y * rl + mieTerm)), ll_exp(-(kRlh.z * rl + mieTerm)));
        totalRlh = r_madd(attn, odStepRlh, totalRlh);
        totalMie = r_madd(attn, odStepMie, totalMie);
        iTime += iStepSize;
    }
    const float pm = pMie * kMie;
    return r_V(iSun * (pRlh * kRlh.x * totalRlh.x + pm * totalMie.x), iSun * (pRlh * kRlh.y * totalRlh.y + pm * totalMie.y),
               iSun * (pRlh * kRlh.z * totalRlh.z + pm * totalMie.z));
}

// main :30-56 — ndc from the texel's integer coordinate (no half-texel offset); invView = the face's matrix (16 floats)
PT_HD v3 atmo_texel_direction_ref(const float *invProj, const float *invView, int S, int x, int y)
{
    const float ndcx = (float)x / (float)S * 2.0f + -1.0f, ndcy = (float)y / (float)S * 2.0f + -1.0f;
    float eye[4], wd[4];
    r_mat_vec(invProj, ndcx, ndcy, -1.0f, 0.0f, eye);
    r_mat_vec(invView, eye[0], eye[1], -1.0f, 0.0f, wd);
    return r_normalize(r_V(wd[0], wd[1], wd[2]));
}

// the colour of one texel; invView6 = the six face matrices (96 floats), lightPos = 3 floats
PT_HD v3 atmo_texel_ref(const float *invProj, const float *invView6, const float *lightPos, float lightIntensity, int S, int iSteps,
                        int jSteps, int face, int x, int y)
{
    const v3 dir = atmo_texel_direction_ref(invProj, invView6 + 16 * face, S, x, y);
    return atmosphere_ref(dir, r_V(0.0f, 6376e3f, 0.0f), r_V(lightPos[0], lightPos[1], lightPos[2]), lightIntensity, 6371e3f, 6471e3f,
                          r_V(5.5e-6f, 13.0e-6f, 22.4e-6f), 21e-6f, 8e3f, 1.2e3f, 0.758f, iSteps, jSteps);
}

// The x-mirror shortcut of the contract kernel (pt_helper_kernels.hip) in this arithmetic.  A lane owns the LOWER texel of a pair that
// is mirrored under x -> -x (faces +X / -X with each other, the other faces with themselves, x <-> S - x) or a texel without partner.
// When pSun.x == 0 and the partner's direction is the exact mirror image (-dx, dy, dz), the partner's colour is the texel's, bit for
// bit, in the reference's summation orders too: with r0.x = pSun.x = 0 the direction's x enters atmosphere_ref only
//   - as the term ax bx of r_dot, which is added LAST (ax bx + (az bz + ay by)): squared it is the same number, against r0.x or pSun.x
//     it is a zero whose sign cannot change a sum with the non-zero (az bz + ay by) — and where that is itself zero the result feeds only
//     b b, mu mu or 2 mu g subtracted from 1 + g g, which do not see a zero's sign;
//   - as the x component of iPos = r t + r0 and jPos = pSun s + iPos, which mirrors exactly (adding a zero is exact) and is only squared.
// What does NOT carry over is how often the directions are exact mirrors: ndc = x / S * 2 + -1 rounds after the subtraction here, so
// for sizes that are not powers of two many pairs fail the test below; they are then computed on their own, as the oracle does.
struct AtmoLaneRef {
    int n;       // texels this lane produced (1 or 2)
    int texel[2]; // index into [6][S][S]
    v3 col[2];
};
// canonical texels per cube row: all S of face +X, column 0 of face -X, and columns 0 .. S / 2 of the four other faces
PT_HD int atmo_half_columns_ref(int S) { return S / 2 + 1; }
PT_HD int atmo_row_lanes_ref(int S) { return S + 1 + 4 * atmo_half_columns_ref(S); }

PT_HD AtmoLaneRef atmo_lane_ref(const float *invProj, const float *invView6, const float *lightPos, float lightIntensity, int S,
                                int iSteps, int jSteps, size_t lane) // lane < S * atmo_row_lanes_ref(S)
{
    const int C = atmo_half_columns_ref(S), T = atmo_row_lanes_ref(S);
    const int y = (int)(lane / (size_t)T);
    int r = (int)(lane % (size_t)T), face, x;
    if (r < S) { face = 0; x = r; }
    else if (r == S) { face = 1; x = 0; }
    else { r -= S + 1; face = 2 + r / C; x = r % C; }
    const v3 r0 = r_V(0.0f, 6376e3f, 0.0f), sun = r_V(lightPos[0], lightPos[1], lightPos[2]), kRlh = r_V(5.5e-6f, 13.0e-6f, 22.4e-6f);
    AtmoLaneRef o;
    const v3 dir = atmo_texel_direction_ref(invProj, invView6 + 16 * face, S, x, y);
    o.n = 1;
    o.texel[0] = (face * S + y) * S + x;
    o.col[0] = atmosphere_ref(dir, r0, sun, lightIntensity, 6371e3f, 6471e3f, kRlh, 21e-6f, 8e3f, 1.2e3f, 0.758f, iSteps, jSteps);
    // the texel's mirror image under x -> -x, if it has one that is not itself
    const int mface = face < 2 ? 1 - face : face, mx = S - x;
    o.texel[1] = o.texel[0];
    o.col[1] = o.col[0];
    if (x < 1 || (mface == face && mx == x)) return o;
    const v3 pdir = atmo_texel_direction_ref(invProj, invView6 + 16 * mface, S, mx, y);
    if (!(lightPos[0] == 0.0f && pdir.x == -dir.x && pdir.y == dir.y && pdir.z == dir.z)) // not an exact mirror image: computed on its own
        o.col[1] = atmosphere_ref(pdir, r0, sun, lightIntensity, 6371e3f, 6471e3f, kRlh, 21e-6f, 8e3f, 1.2e3f, 0.758f, iSteps, jSteps);
    o.n = 2;
    o.texel[1] = (mface * S + y) * S + mx;
    return o;
}

} // namespace ref
} // namespace pt
