// pt_math_reference.hpp — the REFERENCE arithmetic (pt_set_arithmetic(h, PT_ARITH_REFERENCE)): the integrator of
//   OpenTK-PathTracer/res/shaders/PathTracing/compute.glsl:101-369
// restated with the arithmetic choices the reference's own GL implementation (Mesa llvmpipe) makes, instead of the "pt-f32"
// contract of pt_math.hpp.  Used by pt_integrate_reference.hip only; nothing of the default path includes it.
//
// Specification: oracle/pt_oracle.c built with -DPT_ORACLE_PERTURB after pto_set_base_variant(951) (ensemble, targeted sites, signature
// alpha and the NaN-environment override off).  951 = never fused | exact divide / sqrt | literal divisions | llvmpipe's mat4 * vec4
// order | dot as x + (z + y) | llvmpipe's sin, cos, exp, pow | mix as x + a (y - x) | the cube filter's nested lerps.  Choice by choice:
//   - every shader-level a * b + c has two roundings (the vector helpers, the integrator, mat_vec, dot, the sampler's corner weights);
//     the translation unit is compiled with -ffp-contract=off, so a written a * b + c stays v_mul + v_add.  __builtin_fmaf appears only
//     where llvmpipe's own code fuses: the built-ins' polynomials and the cube filter's lerps;
//   - 1 / x, a / b and sqrt are correctly rounded (hipcc's v_div_scale / v_div_fmas / v_div_fixup and corrected v_sqrt sequences);
//     inversesqrt(x) = 1 / sqrt(x) with two roundings;
//   - the reference's literal divisions stay divisions: NDC / width, / height (:114), sphere normal / r (:318), Fresnel (:361), the
//     throughput's / prob and / p (:164, :170), the cuboid slabs (min - o) / d (:283-284);
//   - mat4 * vec4 sums cy y + (cz z + (cx x + cw w)); dot sums ax bx + (az bz + ay by); mix(x, y, a) = x + a (y - x);
//   - sin, cos, exp, pow follow gallivm's algorithms (Mesa lp_bld_arit.c, restated from its published algorithm).
// With these choices the restatement equals the reference's own output bit for bit in ~98.6 % of the first-frame pixels of the
// fixtures (the contract: 38.8 %).  Cost: several IEEE divisions per cuboid test (43 issue cycles each on gfx950) — see DESIGN.md.
// The atmosphere precompute in this arithmetic: pt_atmosphere_reference.hpp (a switch of its own, pt_atmosphere_set_arithmetic).
// The post-process tone map in this arithmetic: pt_postprocess_reference.hpp (a switch of its own, pt_present_set_arithmetic).
//
// The scalar primitives and vector helpers are __host__ __device__ so that a CPU test can compare them with the oracle bit for bit
// (that test defines PT_REFERENCE_PRIMITIVES_ONLY: the integrator below needs the device-side scene and environment types).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_math.hpp"
#ifndef PT_REFERENCE_PRIMITIVES_ONLY
#include "pt_device.hpp"
#endif

namespace pt {
namespace ref {

#define PT_HD __host__ __device__ inline

PT_HD uint32_t bits_of(float f) { return __builtin_bit_cast(uint32_t, f); }
PT_HD float from_bits(uint32_t u) { return __builtin_bit_cast(float, u); }

// ---------------------------------------------------------------------------------------------- correctly rounded primitives
PT_HD float r_div(float a, float b) { return a / b; }
PT_HD float r_rcp(float x) { return 1.0f / x; }
PT_HD float r_sqrt(float x) { return __builtin_sqrtf(x); }
PT_HD float r_rsqrt(float x) { return 1.0f / __builtin_sqrtf(x); } // inversesqrt: two roundings

// ---------------------------------------------------------------------------------------------- llvmpipe's built-ins (gallivm)
// lp_build_polynomial: even and odd powers separately (fused steps in x^2), then odd * x + even (fused)
PT_HD float ll_poly(float x, const float *co, int n)
{
    const float x2 = x * x;
    float even = 0.0f, odd = 0.0f;
    bool haveEven = false, haveOdd = false;
    for (int i = n; i--;) {
        if ((i & 1) == 0) { even = haveEven ? __builtin_fmaf(x2, even, co[i]) : co[i]; haveEven = true; }
        else { odd = haveOdd ? __builtin_fmaf(x2, odd, co[i]) : co[i]; haveOdd = true; }
    }
    return haveOdd ? __builtin_fmaf(odd, x, even) : even;
}
// exp2: clamp, floor / fraction split, degree-5 polynomial of the fraction, scaled by 2^floor
PT_HD float ll_exp2(float x)
{
    const float co[6] = {1.000000000000000000000f, 0.693153073200168932794f, 0.240153617044375388211f, 0.0558263180532956664775f,
                         0.00898934009049466391101f, 0.00187757667519147912699f};
    if (x != x) return x;
    if (x > 128.0f) x = 128.0f;
    if (x < -126.99999f) x = -126.99999f;
    const float ip = __builtin_floorf(x), fp = x - ip;
    return from_bits((uint32_t)((int)ip + 127) << 23) * ll_poly(fp, co, 6);
}
// log2: exponent + y P(y^2), y = (m - 1) / (m + 1); negative or NaN -> NaN, 0 -> -inf, inf -> inf
PT_HD float ll_log2(float x)
{
    const float co[5] = {2.88539009343309178325f, 0.961791550404184197881f, 0.577440339438736392009f, 0.403343858251329912514f,
                         0.406718052498846252698f};
    if (x != x || x < 0.0f) return __builtin_nanf("");
    if (x == 0.0f) return -__builtin_inff();
    if (__builtin_isinf(x)) return x;
    const uint32_t i = bits_of(x);
    const float e = (float)((int)((i >> 23) & 0xffu) - 127);
    const float m = from_bits((i & 0x007fffffu) | 0x3f800000u);
    const float y = (m - 1.0f) / (m + 1.0f);
    return __builtin_fmaf(y, ll_poly(y * y, co, 5), e);
}
PT_HD float ll_exp(float x) { return ll_exp2(x * 1.44269504088896340735992f); }
// pow(x, y) = exp2(log2(x) y); a NaN or zero base gives 0 (measured on llvmpipe), a negative base NaN
PT_HD float ll_pow(float x, float y)
{
    if (x != x) return 0.0f;
    if (x == 0.0f) return 0.0f;
    return ll_exp2(ll_log2(x) * y);
}
// sin / cos: the Cephes-derived routine — j = (int(|a| 4/pi) + 1) & ~1, reduction by pi/4 in three fused steps, two minimax polynomials
PT_HD float ll_sin_or_cos(float a, bool wantCos)
{
    const float xAbs = __builtin_fabsf(a);
    int j = (int)(xAbs * 1.27323954473516f);
    j = (j + 1) & ~1;
    const float y = (float)j;
    const int j2 = wantCos ? j - 2 : j;
    const uint32_t sign = wantCos ? ((~(uint32_t)j2 & 4u) << 29) : ((((uint32_t)j2 & 4u) << 29) ^ (bits_of(a) & 0x80000000u));
    float x = __builtin_fmaf(y, -0.78515625f, xAbs);
    x = __builtin_fmaf(y, -2.4187564849853515625e-4f, x);
    x = __builtin_fmaf(y, -3.77489497744594108e-8f, x);
    const float z = x * x;
    float c = __builtin_fmaf(z, 2.443315711809948E-005f, -1.388731625493765E-003f);
    c = __builtin_fmaf(c, z, 4.166664568298827E-002f);
    c = c * z;
    c = c * z;
    c = __builtin_fmaf(z, -0.5f, c);
    c = c + 1.0f;
    float sv = __builtin_fmaf(z, -1.9515295891E-4f, 8.3321608736E-3f);
    sv = __builtin_fmaf(sv, z, -1.6666654611E-1f);
    sv = sv * z;
    sv = __builtin_fmaf(sv, x, x);
    return from_bits(bits_of((j2 & 2) == 0 ? sv : c) ^ sign);
}
PT_HD float ll_sin(float a) { return ll_sin_or_cos(a, false); }
PT_HD float ll_cos(float a) { return ll_sin_or_cos(a, true); }
PT_HD float r_pow5(float x) { return ll_pow(x, 5.0f); } // compute.glsl:363 pow(1 - cosTheta, 5.0)

// ---------------------------------------------------------------------------------------------- vector helpers (never fused)
PT_HD v3 r_V(float x, float y, float z) { return v3{x, y, z}; }
PT_HD v3 r_add(v3 a, v3 b) { return r_V(a.x + b.x, a.y + b.y, a.z + b.z); }
PT_HD v3 r_sub(v3 a, v3 b) { return r_V(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_HD v3 r_mul(v3 a, v3 b) { return r_V(a.x * b.x, a.y * b.y, a.z * b.z); }
PT_HD v3 r_scale(v3 a, float s) { return r_V(a.x * s, a.y * s, a.z * s); }
PT_HD v3 r_neg(v3 a) { return r_V(-a.x, -a.y, -a.z); }
PT_HD v3 r_madd(v3 b, float s, v3 a) { return r_V(b.x * s + a.x, b.y * s + a.y, b.z * s + a.z); } // a + b s, two roundings
PT_HD float r_dot(v3 a, v3 b) { return a.x * b.x + (a.z * b.z + a.y * b.y); }
PT_HD v3 r_normalize(v3 a) { return r_scale(a, r_rsqrt(r_dot(a, a))); }
PT_HD float r_mix(float x, float y, float a) { return x + a * (y - x); }
PT_HD v3 r_vmix(v3 x, v3 y, float a) { return r_V(r_mix(x.x, y.x, a), r_mix(x.y, y.y, a), r_mix(x.z, y.z, a)); }
// GLSL mat4 * vec4 on the column-major view of the UBO bytes (m[4c + r]), summed the way llvmpipe does: cy y + (cz z + (cx x + cw w))
PT_HD void r_mat_vec(const float *m, float x, float y, float z, float w, float *out)
{
    for (int r = 0; r < 4; r++) out[r] = m[4 + r] * y + (m[8 + r] * z + (m[r] * x + m[12 + r] * w));
}

#ifndef PT_REFERENCE_PRIMITIVES_ONLY
// ---------------------------------------------------------------------------------------------- environment (compute.glsl:177)
// texel (ix,iy), possibly outside `face` -> the texel itself or the one across the seam: pt_device.hpp's, the neighbour is integer arithmetic
// and has no arithmetic choice in it
PT_DEV v3 env_texel_wrapped_ref(const EnvRef &e, int face, int ix, int iy) { return env_texel_wrapped(e, face, ix, iy); }
// texture(samplerCube, dir): LOD 0, LINEAR, seamless.  Without a cube-corner tap: two nested fused lerps, x first (llvmpipe's filter);
// at a cube corner the missing tap's weight is shared by the other three, and the four weighted taps are summed unfused
PT_DEV v3 sample_env_ref(const EnvRef &e, v3 d)
{
    const int S = e.size;
    int face;
    float sc, tc, ma;
    dir_to_face(d.x, d.y, d.z, face, sc, tc, ma);
    const float ima = 0.5f * r_rcp(ma);
    const float fs = (float)S;
    float u = (sc * ima + 0.5f) * fs - 0.5f;
    float v = (tc * ima + 0.5f) * fs - 0.5f;
    u = f_min(f_max(u, -1.0f), fs); // NaN / inf directions: the contract's clamp, shared by both arithmetics
    v = f_min(f_max(v, -1.0f), fs);
    const float fu = __builtin_floorf(u), fv = __builtin_floorf(v);
    const float wu = u - fu, wv = v - fv;
    const int x0 = (int)fu, y0 = (int)fv, x1 = x0 + 1, y1 = y0 + 1;
    const bool offx0 = x0 < 0, offx1 = x1 >= S, offy0 = y0 < 0, offy1 = y1 >= S;
    const bool miss00 = offx0 && offy0, miss10 = offx1 && offy0, miss01 = offx0 && offy1, miss11 = offx1 && offy1;
    const v3 zero = V(0.0f, 0.0f, 0.0f);
    const v3 t00 = miss00 ? zero : env_texel_wrapped_ref(e, face, x0, y0);
    const v3 t10 = miss10 ? zero : env_texel_wrapped_ref(e, face, x1, y0);
    const v3 t01 = miss01 ? zero : env_texel_wrapped_ref(e, face, x0, y1);
    const v3 t11 = miss11 ? zero : env_texel_wrapped_ref(e, face, x1, y1);
    if (!(miss00 || miss10 || miss01 || miss11)) {
        auto lerp = [](float a, float b, float w) { return __builtin_fmaf(w, b - a, a); }; // (lp_build_lerp: fused)
        return V(lerp(lerp(t00.x, t10.x, wu), lerp(t01.x, t11.x, wu), wv), lerp(lerp(t00.y, t10.y, wu), lerp(t01.y, t11.y, wu), wv),
                 lerp(lerp(t00.z, t10.z, wu), lerp(t01.z, t11.z, wu), wv));
    }
    float w00 = (1.0f - wu) * (1.0f - wv), w10 = wu * (1.0f - wv), w01 = (1.0f - wu) * wv, w11 = wu * wv;
    const float a = (miss00 ? w00 : miss10 ? w10 : miss01 ? w01 : w11) * 0.333333343f;
    w00 = miss00 ? 0.0f : w00 + a;
    w10 = miss10 ? 0.0f : w10 + a;
    w01 = miss01 ? 0.0f : w01 + a;
    w11 = miss11 ? 0.0f : w11 + a;
    return V(t11.x * w11 + (t01.x * w01 + (t10.x * w10 + t00.x * w00)), t11.y * w11 + (t01.y * w01 + (t10.y * w10 + t00.y * w00)),
             t11.z * w11 + (t01.z * w01 + (t10.z * w10 + t00.z * w00)));
}

// ---------------------------------------------------------------------------------------------- traversal
// compute.glsl:261-277 RaySphereIntersect
PT_DEV bool ray_sphere_ref(v3 o, v3 d, float4 s, float &t1, float &t2)
{
    const v3 oc = r_sub(o, V(s.x, s.y, s.z));
    const float b = r_dot(d, oc);
    const float c = -s.w * s.w + r_dot(oc, oc);
    const float disc = b * b + -c;
    if (disc < 0.0f) return false;
    const float q = r_sqrt(disc);
    t1 = -b - q;
    t2 = -b + q;
    return t1 <= t2;
}
// compute.glsl:280-294 RayCuboidIntersect, the slabs divided literally
PT_DEV bool ray_cuboid_ref(v3 o, v3 d, float4 mn, float4 mx, float &t1, float &t2)
{
    const v3 t0s = V((mn.x - o.x) / d.x, (mn.y - o.y) / d.y, (mn.z - o.z) / d.z);
    const v3 t1s = V((mx.x - o.x) / d.x, (mx.y - o.y) / d.y, (mx.z - o.z) / d.z);
    const v3 sm = V(f_min(t0s.x, t1s.x), f_min(t0s.y, t1s.y), f_min(t0s.z, t1s.z));
    const v3 bg = V(f_max(t0s.x, t1s.x), f_max(t0s.y, t1s.y), f_max(t0s.z, t1s.z));
    t1 = f_max(FLOAT_MIN, f_max(sm.x, f_max(sm.y, sm.z)));
    t2 = f_min(FLOAT_MAX, f_min(bg.x, f_min(bg.y, bg.z)));
    return t1 <= t2;
}
// compute.glsl:322-332 GetNormal(Cuboid)
PT_DEV v3 cuboid_normal_ref(v3 mn, v3 mx, v3 p)
{
    const v3 half = r_scale(r_sub(mx, mn), 0.5f);
    const v3 cs = r_sub(p, r_scale(r_add(mx, mn), 0.5f));
    v3 n;
    n.x = f_sign(cs.x) * f_step(f_abs(f_abs(cs.x) - half.x), EPSILON);
    n.y = f_sign(cs.y) * f_step(f_abs(f_abs(cs.y) - half.y), EPSILON);
    n.z = f_sign(cs.z) * f_step(f_abs(f_abs(cs.z) - half.z), EPSILON);
    return r_normalize(n);
}
// compute.glsl:226-258 RayTrace: every sphere, then every cuboid, in the reference's order.  Acceptance uses the entry distance t1
// against the stored GetSmallestPositive (:234,247,347-350); material and normal are evaluated once for the surviving candidate.
PT_DEV bool ray_trace_ref(const SceneLds &sc, int ns, int nc, v3 o, v3 d, Hit &h)
{
    float T = FLOAT_MAX, wt2 = 0.0f, t1, t2;
    int winner = -1;
    for (int i = 0; i < ns; i++) {
        if (ray_sphere_ref(o, d, sc.sph[i], t1, t2) && t2 > 0.0f && t1 < T) {
            T = t1 < 0.0f ? t2 : t1;
            wt2 = t2;
            winner = i;
        }
    }
    for (int i = 0; i < nc; i++) {
        if (ray_cuboid_ref(o, d, sc.cmin[i], sc.cmax[i], t1, t2) && t2 > 0.0f && t1 < T) {
            T = t1 < 0.0f ? t2 : t1;
            wt2 = t2;
            winner = 256 + i;
        }
    }
    if (winner < 0 || !(T != FLOAT_MAX)) return false; // compute.glsl:257
    h.T = T;
    h.fromInside = (T == wt2);
    h.nearHitPos = r_madd(d, T, o);
    if (winner < 256) {
        const float4 s = sc.sph[winner];
        h.m = load_material(sc.mat + 4 * winner);
        const v3 pc = r_sub(h.nearHitPos, V(s.x, s.y, s.z));
        h.normal = V(pc.x / s.w, pc.y / s.w, pc.z / s.w); // compute.glsl:318
    } else {
        const int ci = winner - 256;
        const float4 mn = sc.cmin[ci], mx = sc.cmax[ci];
        h.m = load_material(sc.mat + 4 * (ns + ci));
        h.normal = cuboid_normal_ref(V(mn.x, mn.y, mn.z), V(mx.x, mx.y, mx.z), h.nearHitPos);
    }
    return true;
}

// ---------------------------------------------------------------------------------------------- sampling / BSDF
// compute.glsl:297-307
PT_DEV v3 cosine_sample_hemisphere_ref(v3 n, uint32_t &seed)
{
    const float z = rand01(seed) * 2.0f + -1.0f;
    const float a = rand01(seed) * 2.0f * PI;
    const float r = r_sqrt(-z * z + 1.0f);
    const float sn = ll_sin(a), cs = ll_cos(a);
    return r_normalize(r_add(n, V(r * cs, r * sn, z)));
}
// compute.glsl:359-364
PT_DEV float fresnel_schlick_ref(float cosTheta, float n1, float n2)
{
    float r0 = (n1 - n2) / (n1 + n2);
    r0 *= r0;
    return (1.0f - r0) * r_pow5(1.0f - cosTheta) + r0;
}
PT_DEV v3 reflect_ref(v3 i, v3 n) { return r_madd(n, -(2.0f * r_dot(n, i)), i); }
PT_DEV v3 refract_ref(v3 i, v3 n, float eta)
{
    const float ni = r_dot(n, i);
    const float k = -(eta * eta) * (-ni * ni + 1.0f) + 1.0f;
    if (k < 0.0f) return V(0.0f, 0.0f, 0.0f);
    const float f = eta * ni + r_sqrt(k);
    return V(eta * i.x + -(f * n.x), eta * i.y + -(f * n.y), eta * i.z + -(f * n.z));
}
// compute.glsl:184-224 BSDF: picks the next ray, returns its probability
PT_DEV float bsdf_ref(v3 &ro, v3 &rd, const Hit &h, bool &isRefractive, uint32_t &seed)
{
    isRefractive = false;
    float spec = h.m.specularChance, refr = h.m.refractionChance;
    if (spec > 0.0f) {
        const float n1 = h.fromInside ? h.m.ior : 1.0f, n2 = !h.fromInside ? h.m.ior : 1.0f;
        spec = r_mix(spec, 1.0f, fresnel_schlick_ref(r_dot(r_neg(rd), h.normal), n1, n2));
        const float diffuse = 1.0f - spec - refr;
        refr = 1.0f - spec - diffuse;
    }
    const v3 diffuseRay = cosine_sample_hemisphere_ref(h.normal, seed);
    float prob;
    const float roll = rand01(seed);
    if (spec > roll) {
        const v3 refl = reflect_ref(rd, h.normal);
        rd = r_normalize(r_vmix(refl, diffuseRay, h.m.specularRoughness * h.m.specularRoughness));
        prob = spec;
    } else if (spec + refr > roll) {
        const v3 rf = refract_ref(rd, h.normal, h.fromInside ? h.m.ior : r_rcp(h.m.ior));
        const v3 rough = cosine_sample_hemisphere_ref(r_neg(h.normal), seed);
        rd = r_normalize(r_vmix(rf, rough, h.m.refractionRoughness * h.m.refractionRoughness));
        prob = refr;
        isRefractive = true;
    } else {
        rd = diffuseRay;
        prob = 1.0f - spec - refr;
    }
    ro = r_madd(rd, EPSILON, h.nearHitPos);
    return f_max(prob, EPSILON);
}

// compute.glsl:132-182 Radiance
PT_DEV v3 radiance_ref(const FrameArgs &a, const SceneLds &sc, const EnvRef &env, v3 ro, v3 rd, uint32_t &seed)
{
    v3 throughput = V(1.0f, 1.0f, 1.0f), rad = V(0.0f, 0.0f, 0.0f);
    for (int i = 0; i < a.rayDepth; i++) {
        Hit h;
        if (!ray_trace_ref(sc, a.numSpheres, a.numCuboids, ro, rd, h)) {
            const v3 e = sample_env_ref(env, rd); // :177
            rad = r_add(r_mul(e, throughput), rad);
            break;
        }
        if (h.fromInside) { // Beer's law, :145-149
            h.normal = r_neg(h.normal);
            throughput.x *= ll_exp(-h.m.absorbance.x * h.T);
            throughput.y *= ll_exp(-h.m.absorbance.y * h.T);
            throughput.z *= ll_exp(-h.m.absorbance.z * h.T);
        }
        bool isRefractive;
        const float prob = bsdf_ref(ro, rd, h, isRefractive, seed);
        rad = r_add(r_mul(h.m.emissiv, throughput), rad);
        if (!isRefractive) throughput = r_mul(throughput, h.m.albedo);
        throughput = V(throughput.x / prob, throughput.y / prob, throughput.z / prob); // :164
        const float p = f_max(throughput.x, f_max(throughput.y, throughput.z)); // Russian roulette, :167-173
        if (rand01(seed) > p) break;
        throughput = V(throughput.x / p, throughput.y / p, throughput.z / p);
    }
    return rad;
}

// compute.glsl:113-121: sub-pixel jitter, GetWorldSpaceRay (:352-357), thin lens (UniformSampleUnitCircle :309-314); 4 RNG draws
PT_DEV void primary_ray_ref(const FrameArgs &a, int px, int py, uint32_t &seed, v3 &ro, v3 &rd)
{
    const float u0 = rand01(seed), u1 = rand01(seed); // :113
    const float ndcx = ((float)px + u0) / (float)a.width * 2.0f + -1.0f; // :114, literal / imgResultSize
    const float ndcy = ((float)py + u1) / (float)a.height * 2.0f + -1.0f;
    float eye[4], wd[4], org[4];
    r_mat_vec(a.invProj, ndcx, ndcy, -1.0f, 0.0f, eye);
    r_mat_vec(a.invView, eye[0], eye[1], -1.0f, 0.0f, wd);
    const v3 dir = r_normalize(V(wd[0], wd[1], wd[2]));
    const v3 focal = r_madd(dir, a.focalLength, V(a.viewPos[0], a.viewPos[1], a.viewPos[2])); // :117
    const float angle = rand01(seed) * 2.0f * PI;
    const float rr = r_sqrt(rand01(seed));
    const float sn = ll_sin(angle), cs = ll_cos(angle);
    const float halfAp = a.apertureDiameter * 0.5f;
    const float ox = halfAp * (cs * rr), oy = halfAp * (sn * rr);
    r_mat_vec(a.invView, ox, oy, 0.0f, 1.0f, org); // :120
    ro = V(org[0], org[1], org[2]);
    rd = r_normalize(r_sub(focal, ro));
}

// compute.glsl:101-130 main for one pixel: returns the new accumulation value (irradiance / SPP, running mean, alpha = 1)
PT_DEV float4 shade_pixel_ref(const FrameArgs &a, const SceneLds &sc, const EnvRef &env, int px, int py, float4 last)
{
    uint32_t seed = pixel_seed(px, py, a.frame); // :106
    v3 irr = V(0.0f, 0.0f, 0.0f);
    for (int s = 0; s < a.spp; s++) {
        v3 ro, rd;
        primary_ray_ref(a, px, py, seed, ro, rd);
        irr = r_add(irr, radiance_ref(a, sc, env, ro, rd, seed));
    }
    irr = r_scale(irr, 1.0f / (float)a.spp); // :125 (uniform reciprocal, as the oracle's)
    const float w = 1.0f / (float)(a.frame + 1); // :128
    return make_float4(r_mix(last.x, irr.x, w), r_mix(last.y, irr.y, w), r_mix(last.z, irr.z, w), 1.0f);
}

#endif // PT_REFERENCE_PRIMITIVES_ONLY

} // namespace ref
} // namespace pt
