/*
 * pt_oracle_witness.c — the WITNESS build of the CPU oracle (_build/libpt_oracle_perturb.so, Oracle(perturb=True)).  TEST INFRASTRUCTURE ONLY.
 *
 * The contract (../pt_oracle.c) turned into its conforming NEIGHBOURS: one primitive some ulps off, single calls and comparisons
 * targeted, whole ensemble members, the path signature, the close-decision record, the base variants (llvmpipe's arithmetic choices,
 * pt_oracle.LLVMPIPE: the oracle of the shipped reference-arithmetic modes) and the per-pixel witness search.  This unit defines the
 * hooks of ../pt_oracle_hooks.h, #includes the contract and then implements the witness entry points of the C ABI.  With every knob
 * at its default the library computes the contract bit for bit (tests/test_oracle_digests.py).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* ---- the witness build (_build/libpt_oracle_perturb.so; tests/test_decision_margins.py).  GLSL leaves the precision of
 * 1/x, inversesqrt, sqrt, sin, cos, exp implementation-defined: an implementation whose primitive P returns results ONE ULP LARGER (or
 * smaller) in magnitude than this contract's is as conforming as the contract.  pto_set_perturbation(P, ulps) turns this library into
 * that implementation (every call of P, every pixel); the margin test uses the family as constructive witnesses: a pixel of the
 * reference that the contract misses must be HIT by one of its neighbours.  P: 0 rcp, 1 rsqrt, 2 sqrt, 3 sin, 4 cos, 5 exp, 6 pow5. */
static int g_perturb_prim = -1, g_perturb_ulps = 0;
/* TARGETED witnesses (round 6).  A global shift of a primitive moves every value of the path; what separates the contract from the
 * reference in an out-of-band pixel is usually ONE comparison that came out the other way.  Two single-site variants, both conforming
 * (GLSL fixes neither the last bits of a primitive at one particular argument nor, therefore, the outcome of a comparison whose operands
 * are closer than those bits):
 *   - g_flip_at[]: the pixel's k-th data-dependent comparison (DECIDE sites: compute.glsl:169,201,208,234,247,269,293,322-332,347-350,
 *     refract's k < 0) is inverted, everything else evaluated by the contract;
 *   - g_tprim / g_tcall / g_tulps [g_tn]: the n-th call of primitive P in this pixel returns a result `ulps` off, every other call the
 *     contract's (up to WIT_MAX_SITES such calls at once: pixels whose paths AMPLIFY — a few bounces on curved surfaces turn one ulp
 *     into 1e-3 of the colour — are reached by a handful of calls a few ulps off, not by one).
 * pto_witness_search tries them for one pixel (single-threaded; the counters are per thread, the targets are globals). */
#define WIT_MAX_CLOSE 2048
#define WIT_MAX_FLIPS 3
static int g_flip_at[WIT_MAX_FLIPS] = { -1, -1, -1 };
#define WIT_MAX_SITES 32
static int g_tn = 0, g_tprim[WIT_MAX_SITES], g_tcall[WIT_MAX_SITES], g_tulps[WIT_MAX_SITES]; /* targeted primitive calls */
static float g_record_gap = 0.0f; /* > 0: record the decisions whose operands are closer than this (relative to their scale) */
static __thread int tl_dec_n, tl_call_n[10], tl_close_n, tl_nan_env;
static __thread struct { int idx; float gap; int line; float diff; } tl_close[WIT_MAX_CLOSE];
static inline float ulp_shift(float y, int ulps)
{
    if (!(fabsf(y) > 1.17549435e-38f) || isinf(y)) return y;
    uint32_t u; memcpy(&u, &y, 4);
    u = (uint32_t)((int32_t)u + ulps); /* (sign-magnitude: + = away from zero) */
    memcpy(&y, &u, 4);
    return y;
}
/* ENSEMBLE members (round 6, pto_set_ensemble; tests/test_ensemble_stability.py).  A member is ONE conforming implementation that differs
 * from the contract everywhere at once, the way a real driver does: its primitive P'(x) = P(x) shifted by s ulps, s a fixed pseudo-random
 * function of (member seed, primitive, the bits of P(x)) in [-a_P, +a_P] with a_P = min(amplitude, GLSL's / the search's allowance for P);
 * each a * b + c is fused or not, each division literal or by reciprocal, as a fixed function of the member and the operands' bits.  The
 * shift depends on the value only, so P' is a function (the same argument gives the same result in every pixel and frame).  A pixel
 * whose value does not move under any member of an ensemble is insensitive to what conforming implementations differ by — the
 * statement the first-order margins can only bound from one side. */
static int g_sig_alpha = 0;            /* pto_set_signature_alpha: the alpha channel carries the pixel's PATH SIGNATURE instead of 1 */
static __thread int tl_ub;            /* the pixel touched something GLSL / GL leave undefined (pow of a base that is negative or within four ulps of zero, a comparison on a NaN, texture(env, NaN)) */
static __thread uint32_t tl_sig;       /* hash of the path's discrete events: object hit, lobe taken, how it ended — per bounce, sample, frame */
static inline void sig_note(uint32_t ev) { tl_sig = (tl_sig ^ ev) * 0x01000193u + 0x9E3779B9u; tl_sig ^= tl_sig >> 15; }
#define SIG_NOTE(ev) sig_note((uint32_t)(ev))
static uint32_t g_ens_seed = 0; /* 0 = off */
static int g_ens_amp = 0;
static const int ens_allow[7] = { 2, 2, 2, 4, 4, 4, 16 }; /* (= wit_ulps below: rcp, rsqrt, sqrt, sin, cos, exp, pow5) */
static inline uint32_t ens_hash(uint32_t a, uint32_t b)
{
    uint32_t h = (g_ens_seed ^ (a * 0x9E3779B9u)) + b * 0x85EBCA6Bu;
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return h;
}
static inline float perturbed(int prim, float y)
{
    const int n = tl_call_n[prim]++;
    for (int t = 0; t < g_tn; t++)
        if (prim == g_tprim[t] && n == g_tcall[t]) return ulp_shift(y, g_tulps[t]);
    if (g_ens_seed != 0 && prim < 7) {
        uint32_t u; memcpy(&u, &y, 4);
        const int a = g_ens_amp < ens_allow[prim] ? g_ens_amp : ens_allow[prim];
        return ulp_shift(y, (int)(ens_hash((uint32_t)prim, u) % (uint32_t)(2 * a + 1)) - a);
    }
    if (prim != g_perturb_prim || g_perturb_ulps == 0) return y;
    return ulp_shift(y, g_perturb_ulps);
}
static inline int decide_at(int cond, float diff, float scale, int line)
{
    const int k = tl_dec_n++;
    if (g_record_gap > 0.0f) {
        const float gap = fabsf(diff) / fmaxf(fabsf(scale), 1e-30f);
        if (gap < g_record_gap && tl_close_n < WIT_MAX_CLOSE) { tl_close[tl_close_n].idx = k; tl_close[tl_close_n].gap = gap; tl_close[tl_close_n].line = line; tl_close[tl_close_n].diff = diff; tl_close_n++; }
    }
    /* an ensemble member decides comparisons ON A NaN for itself (GLSL 4.60 section 4.7.1: "operations and built-in functions that operate on
       a NaN are not required to return a NaN", min / max of a NaN are undefined: after refract() = 0 -> normalize(0) the ray is NaN and
       whether it "hits" a slab is the implementation's choice; llvmpipe's misses everything and looks the environment up at NaN) */
    if (diff != diff) tl_ub = 1;
    if (g_ens_seed != 0 && diff != diff) return (int)(ens_hash(200u + (uint32_t)(k & 15), 0u) >> 31);
    return (k == g_flip_at[0] || k == g_flip_at[1] || k == g_flip_at[2]) ? !cond : cond;
}
#define DECIDE(cond, diff, scale) decide_at((cond), (diff), (scale), __LINE__)
/* "primitive" 7: a * b + c.  GLSL lets an implementation fuse it or not; the contract fuses where this file says fmaf, llvmpipe never
 * does.  A targeted site (any non-zero shift) evaluates that ONE multiply-add the other way; pto_set_unfused(1) all of them (outside
 * the primitives above, whose own Newton steps are part of their definition). */
static int g_unfuse_all = 0, g_pow_neg_nan = 0, g_nan_env_set = 0;
/* base variants (pto_set_base_variant): the searches above run AROUND a conforming implementation, by default the contract; llvmpipe's
 * arithmetic differs from it everywhere at once (correctly rounded 1/x, sqrt, 1/sqrt; the literal a / b; never fused), and a pixel that
 * amplifies is closer to the reference's value from a base that shares those than from the contract */
static int g_base_exact = 0, g_base_truediv = 0;
static int g_base_sampler_lerp = 0; /* (base variant bit 512) */
static int g_base_mix_lerp = 0; /* (base variant bit 256: mix(x, y, a) = x + a (y - x), llvmpipe's form — probed: 100 % bit-identical) */
static int g_base_matvec = 0, g_base_dot = 0; /* (base variants, bits 8 / 16 and 32 / 64: the order in which matrix-vector and dot products sum their terms) */
static float g_nan_env[3]; /* what texture(env, NaN direction) returns instead of the contract's clamped lookup (pto_set_nan_env) */
static inline float wit_fma(float a, float b, float c)
{
    const int n = tl_call_n[7]++;
    int unfused = g_unfuse_all;
    if (g_ens_seed != 0) { /* this member fuses about half of the multiply-adds: a fixed function of the operands */
        uint32_t ua, ub, uc; memcpy(&ua, &a, 4); memcpy(&ub, &b, 4); memcpy(&uc, &c, 4);
        unfused = (int)(ens_hash(7u + ua, ub ^ (uc * 0xC2B2AE35u)) >> 31);
    }
    for (int t = 0; t < g_tn; t++)
        if (g_tprim[t] == 7 && n == g_tcall[t] && g_tulps[t] != 0) unfused = !unfused;
    if (unfused) { const float m = a * b; return m + c; } /* (-ffp-contract=off: two roundings) */
    return __builtin_fmaf(a, b, c);
}
/* "primitive" 8: a / b where the contract multiplies by a reciprocal it has already (sphere normal (p - c) / r, throughput /= prob,
 * throughput /= p: compute.glsl:318,164,170); a targeted site divides.  "primitive" 9: mix(x, y, a) as x + a (y - x) instead of
 * x (1 - a) + y a (GLSL: "the linear blend"; both forms are in use). */
static inline int wit_targeted(int prim)
{
    const int n = tl_call_n[prim]++;
    for (int t = 0; t < g_tn; t++)
        if (g_tprim[t] == prim && n == g_tcall[t] && g_tulps[t] != 0) return 1;
    return 0;
}
static inline float wit_quot(float a, float b, float rb)
{
    int literal = (wit_targeted(8) != 0) != (g_base_truediv != 0);
    if (g_ens_seed != 0) { uint32_t ua, ub; memcpy(&ua, &a, 4); memcpy(&ub, &b, 4); literal = (int)(ens_hash(8u + ua, ub) >> 31); }
    return literal ? a / b : a * rb;
}
#define QUOT(a, b, rb) wit_quot((a), (b), (rb))
#define MIX_OTHER_FORM() ((wit_targeted(9) != 0) != (g_base_mix_lerp != 0))
static int g_base_llvm_math = 0; /* (base variant bit 128: sin, cos, exp, pow as llvmpipe evaluates them, ../pt_oracle_llvmpipe.h) */

/* ---- the remaining hooks (../pt_oracle_hooks.h says where each one sits in the contract) */
#define perturbed(prim, y) perturbed((prim), (y))
#define c_fma(a, b, c) wit_fma((a), (b), (c)) /* (the vector helpers and the integrator; not the primitives) */
#define FLIPPED_NONNEG(x) do { if ((x) < 0.0f) (x) = 0.0f; } while (0) /* (the inverted decision: an implementation whose discriminant came out >= 0 grazes the sphere) */
typedef struct v3 v3;
static int wit_alt_primitive(int prim, float x, float *r);
static int wit_alt_sincos(float a, float *sn, float *cs);
static int wit_alt_dot(v3 a, v3 b, float *r);
static int wit_alt_mat_vec(const float *m, float x, float y, float z, float w, float *out);
static void wit_pixel_begin(const float *last);
static void wit_pixel_end(float *out);
#define ALT_PRIMITIVE(prim, x) do { float r_ = 0.0f; if (wit_alt_primitive((prim), (x), &r_)) return r_; } while (0)
#define ALT_SINCOS(a, sn, cs) do { if (wit_alt_sincos((a), (sn), (cs))) return; } while (0)
#define ALT_DOT(a, b) do { float r_ = 0.0f; if (wit_alt_dot((a), (b), &r_)) return r_; } while (0)
#define ALT_MAT_VEC(m, x, y, z, w, out) do { if (wit_alt_mat_vec((m), (x), (y), (z), (w), (out))) return; } while (0)
/* texture(env, NaN): undefined in GL (see pto_witness_search) */
#define ALT_NAN_ENV(d) do { if ((d).x != (d).x || (d).y != (d).y || (d).z != (d).z) { \
        tl_nan_env = 1; \
        if (g_nan_env_set) { rgb o_ = { g_nan_env[0], g_nan_env[1], g_nan_env[2] }; return o_; } } } while (0)
/* base variant bit 512: two nested lerps a + w (b - a), x first (llvmpipe's filter; lp_build_lerp: a multiply-add of the sampler's own
   code, fused like the built-ins' polynomials) */
#define WIT_LERP_(a_, b_, w_) __builtin_fmaf((w_), (b_) - (a_), (a_))
#define ENV_FILTER(corner, t00, t10, t01, t11, wu, wv, contract) \
    (g_base_sampler_lerp && !(corner) ? WIT_LERP_(WIT_LERP_((t00), (t10), (wu)), WIT_LERP_((t01), (t11), (wu)), (wv)) : (contract))
#define ALT_SLABS(t0s, t1s, mn, mx, o, d) do { if (g_base_truediv) { \
        t0s = V((mn.x - o.x) / d.x, (mn.y - o.y) / d.y, (mn.z - o.z) / d.z); \
        t1s = V((mx.x - o.x) / d.x, (mx.y - o.y) / d.y, (mx.z - o.z) / d.z); } } while (0)
/* (base variant: the literal / imgResultSize of compute.glsl:114 — llvmpipe divides) */
#define ALT_NDC(ndcx, ndcy, px, u0, py, u1, c) do { if (g_base_truediv) { \
        ndcx = c_fma(((float)px + u0) / (float)c->width, 2.0f, -1.0f); \
        ndcy = c_fma(((float)py + u1) / (float)c->height, 2.0f, -1.0f); } } while (0)
#define PIXEL_BEGIN(last) wit_pixel_begin(last)
#define PIXEL_END(out) wit_pixel_end(out)
#define PTO_HAVE_WITNESS_ENTRY_POINTS

#include "../pt_oracle.c"
#include "../pt_oracle_llvmpipe.h"

/* ---- the alternative bodies: correctly rounded 1/x, 1/sqrt, sqrt (base variant bit 2), llvmpipe's exp and pow (bit 128), and what an
 * implementation may make of pow(x, 5) where GLSL leaves it undefined */
static int wit_alt_primitive(int prim, float x, float *r)
{
    switch (prim) {
    case 0: if (!g_base_exact) return 0; *r = perturbed(0, 1.0f / x); return 1;
    case 1: if (!g_base_exact) return 0; *r = perturbed(1, 1.0f / sqrtf(x)); return 1;
    case 2: if (!g_base_exact) return 0; *r = perturbed(2, sqrtf(x)); return 1;
    case 5: if (!g_base_llvm_math) return 0; *r = perturbed(5, ll_exp(x)); return 1;
    case 6:
        /* pow(x, y) is undefined for x < 0 (GLSL 4.60 section 8.2); llvmpipe's exp2(y log2 x) is NaN.  Mode 2: also for a base within four
           ulps of 1 - cos = 0 — whether 1 - dot(-d, n) of two unit vectors comes out as +-1e-7 or 0 is the last bit of the dot product */
        if (g_base_llvm_math && g_ens_seed == 0) { if (x < 0.0f) tl_ub = 1; *r = perturbed(6, ll_pow(x, 5.0f)); return 1; }
        if (x < 4.8e-7f) tl_ub = 1;
        if (g_ens_seed != 0) { /* an ensemble member: a negative base is NaN for two members in three; a base within four ulps of zero is one
                                  whose sign the member's own last bits decide — NaN for about half of such calls (by call, not by value:
                                  the same 1 - cos comes out of different dot products) */
            if (x < 0.0f ? g_pow_neg_nan != 0 : (x < 4.8e-7f && (ens_hash(60u, (uint32_t)tl_call_n[6]) >> 31))) { tl_call_n[6]++; *r = NAN; return 1; }
        } else
        if (g_pow_neg_nan && (x < 0.0f || (g_pow_neg_nan == 2 && x < 4.8e-7f))) { *r = NAN; return 1; }
        return 0;
    default: return 0;
    }
}
static int wit_alt_sincos(float a, float *sn, float *cs)
{
    if (!g_base_llvm_math) return 0;
    *sn = perturbed(3, ll_sin_or_cos(a, 0));
    *cs = perturbed(4, ll_sin_or_cos(a, 1));
    return 1;
}
/* an ensemble member also sums the three products of a dot product in an order of its own (GLSL does not fix one): a fixed function of
   the member and the operands */
static int wit_alt_dot(v3 a, v3 b, float *r)
{
    if (g_ens_seed != 0 || g_base_dot != 0) {
        uint32_t ua, ub; memcpy(&ua, &a.x, 4); memcpy(&ub, &b.y, 4);
        switch (g_ens_seed != 0 ? ens_hash(11u + ua, ub) % 3u : (uint32_t)g_base_dot) {
        case 1: *r = c_fma(a.x, b.x, c_fma(a.z, b.z, a.y * b.y)); return 1;
        case 2: *r = c_fma(a.y, b.y, c_fma(a.x, b.x, a.z * b.z)); return 1;
        default: break;
        }
    }
    return 0;
}
static int wit_alt_mat_vec(const float *m, float x, float y, float z, float w, float *out)
{
    if (g_ens_seed != 0 || g_base_matvec != 0) { /* (an ensemble member's own order of the four column terms, per product) */
        uint32_t ux, uy; memcpy(&ux, &x, 4); memcpy(&uy, &y, 4);
        const uint32_t order = g_ens_seed != 0 ? ens_hash(12u + ux, uy) % 4u : (uint32_t)g_base_matvec;
        for (int r = 0; r < 4; r++) {
            const float cx = m[r], cy = m[4 + r], cz = m[8 + r], cw = m[12 + r];
            out[r] = order == 1 ? c_fma(cx, x, c_fma(cy, y, c_fma(cz, z, cw * w)))        /* w first */
                   : order == 2 ? c_fma(cy, y, c_fma(cz, z, c_fma(cx, x, cw * w)))        /* ((w + x) + z) + y: llvmpipe's, found by matching its primary rays bit for bit */
                   : order == 3 ? c_fma(cz, z, c_fma(cw, w, c_fma(cy, y, cx * x)))
                   : c_fma(cw, w, c_fma(cz, z, c_fma(cy, y, cx * x)));
        }
        return 1;
    }
    return 0;
}
static void wit_pixel_begin(const float *last)
{
    tl_dec_n = 0; tl_close_n = 0; tl_nan_env = 0;
    tl_sig = g_sig_alpha ? (f_bits(last[3]) & 0x7FFFFFu) : 0u; /* (chained over the frames of an accumulation) */
    tl_ub = 0;
    memset(tl_call_n, 0, sizeof tl_call_n);
}
static void wit_pixel_end(float *out)
{
    if (tl_ub || tl_nan_env) sig_note(0xDEAD0000u ^ g_ens_seed ^ 0x5bd1e995u); /* undefined behaviour on the way: no two implementations "follow the same path" */
    if (g_sig_alpha) out[3] = f_unbits(0x3F800000u | (tl_sig & 0x7FFFFFu)); /* a float in [1, 2): 23 bits of the signature, survives copies */
}

/* ------------------------------------------------------------------ the witness entry points of the C ABI */
/* witness build only: primitive `prim` returns results `ulps` units in the last place further from zero (negative: nearer); -1 / 0 = off.
 * (Other builds: the stub at the end of pt_oracle.c returns -1.)  Set while nothing renders. */
PTO_API int pto_set_perturbation(int prim, int ulps)
{
    g_perturb_prim = prim;
    g_perturb_ulps = ulps;
    return 0;
}

/* witness build: 1 = every multiply-add outside the primitives is evaluated with two roundings (what llvmpipe does); 0 = the contract. */
PTO_API int pto_set_unfused(int on)
{
    g_unfuse_all = on != 0;
    return 0;
}

/* witness build: the implementation the searches and replays run around.  bits: 1 = never fuse a * b + c (outside the primitives), 2 =
 * correctly rounded 1/x, 1/sqrt, sqrt, 4 = the literal a / b where the contract multiplies by a reciprocal (cuboid slabs, sphere normal,
 * throughput).  7 = all three, what llvmpipe does; 0 = the contract. */
PTO_API int pto_set_base_variant(int bits)
{
    g_unfuse_all = (bits & 1) != 0;
    g_base_exact = (bits & 2) != 0;
    g_base_truediv = (bits & 4) != 0;
    g_base_matvec = (bits >> 3) & 3; /* 0 = the contract's x, y, z, w chain; 1 = w, z, y, x; 2 = ((w + x) + z) + y, llvmpipe's; 3 = x, y, w, z */
    g_base_dot = (bits >> 5) & 3;    /* 0 = the contract's x, y, z chain; 1 = y, z, x; 2 = z, x, y */
    g_base_sampler_lerp = (bits >> 9) & 1;
    g_base_mix_lerp = (bits >> 8) & 1;
    g_base_llvm_math = (bits >> 7) & 1; /* 128 = sin, cos, exp, pow as llvmpipe's gallivm evaluates them (bit-identical on the probe) */
    return 0;
}

/* witness build: llvmpipe's built-ins as restated above, on arrays (which: 0 sin, 1 cos, 2 exp, 3 pow(x, y), 4 exp2, 5 log2) — for the
 * probe test that compares them bit for bit with the live llvmpipe.  (-1 in other builds.) */
PTO_API int pto_llvmpipe_like(int which, const float *x, const float *y, int n, float *out)
{
    for (int i = 0; i < n; i++)
        out[i] = which == 0 ? ll_sin_or_cos(x[i], 0) : which == 1 ? ll_sin_or_cos(x[i], 1) : which == 2 ? ll_exp(x[i])
               : which == 3 ? ll_pow(x[i], y[i]) : which == 4 ? ll_exp2(x[i]) : ll_log2(x[i]);
    return 0;
}

/* witness build: 1 = the alpha channel of every rendered pixel carries 23 bits of its PATH SIGNATURE (a hash of which object each bounce
 * hit and from which side, which lobe it took and how the path ended, over the samples of the pixel and — through the previous alpha —
 * the frames accumulated so far) instead of 1.0; 0 = the reference's alpha again.  Two implementations whose pixel has the same
 * signature followed the same path through the scene, whatever their colours are. */
PTO_API int pto_set_signature_alpha(int on)
{
    g_sig_alpha = on != 0;
    return 0;
}

/* witness build, diagnostic: the comparisons of pixel (x, y) whose operands are closer than closeGap (relative to their scale), in path
 * order: out4[4 k] = decision index, [4 k + 1] = source line of the DECIDE site in this file, [4 k + 2] = relative gap, [4 k + 3] = a - b.
 * Returns how many (at most cap) (-1 in other builds). */
PTO_API int pto_list_close_decisions(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                                     int x, int y, int frame, const float *last4, float closeGap, int cap, float *out4)
{
    Ctx c;
    float v[4];
    make_ctx(&c, p, basic144, objects26624, env);
    g_record_gap = closeGap;
    shade_pixel(&c, x, y, frame, last4, v, NULL);
    g_record_gap = 0.0f;
    const int n = tl_close_n < cap ? tl_close_n : cap;
    for (int k = 0; k < n; k++) {
        out4[4 * k] = (float)tl_close[k].idx; out4[4 * k + 1] = (float)tl_close[k].line;
        out4[4 * k + 2] = tl_close[k].gap; out4[4 * k + 3] = tl_close[k].diff;
    }
    return n;
}

/* witness build: the library becomes ensemble member `seed` (0: the contract / the base variant again): every primitive call up to
 * min(amplitude, its allowance) ulps off, every multiply-add fused or not, every division literal or by reciprocal — each a fixed
 * pseudo-random function of the member and the operands (see ens_hash).  Thread-safe to render with; set while nothing renders. */
PTO_API int pto_set_ensemble(unsigned seed, int amplitude)
{
    g_ens_seed = seed;
    g_ens_amp = amplitude < 0 ? 0 : amplitude;
    /* what GLSL / GL leave UNDEFINED a member also chooses for itself: pow(x, 5) of a negative base (and, every third member, of a base
       within four ulps of zero: the last bit of 1 - dot(-d, n)) is NaN or the product; texture(env, NaN direction) is some colour */
    g_pow_neg_nan = seed == 0 ? 0 : (int)(seed % 3u);
    g_nan_env_set = seed != 0;
    for (int ch = 0; ch < 3; ch++) g_nan_env[ch] = (float)(ens_hash(100u + (uint32_t)ch, 0u) >> 8) * (1.0f / 16777216.0f);
    return 0;
}

/* witness build: texture(env, NaN direction) returns rgb3 (NULL: the contract's clamped lookup again).  The pixel is linear in this value,
 * so two replays (0 and 1) tell which value of the undefined lookup would reproduce a given pixel of the reference. */
PTO_API int pto_set_nan_env(const float *rgb3)
{
    g_nan_env_set = rgb3 != NULL;
    if (rgb3) memcpy(g_nan_env, rgb3, sizeof g_nan_env);
    return 0;
}

/* witness build: evaluate ONE pixel with up to three of its comparisons inverted (flips3[k] = decision index, -1 = none) and nsites
 * primitive calls shifted (sites[3 t] = primitive, [3 t + 1] = call index within the pixel, [3 t + 2] = ulps); powNegNan 1 / 2: pow() of a
 * negative (or within four ulps of zero) base is NaN.  Returns the number of
 * DECIDE sites the evaluation passed (-1 in other builds). */
PTO_API int pto_render_pixel_variant(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                                     int x, int y, int frame, const float *last4, const int *flips3, int nsites, const int *sites, int powNegNan,
                                     float *out4)
{
    Ctx c;
    make_ctx(&c, p, basic144, objects26624, env);
    if (nsites > WIT_MAX_SITES) return -2;
    g_pow_neg_nan = powNegNan;
    for (int k = 0; k < WIT_MAX_FLIPS; k++) g_flip_at[k] = flips3 ? flips3[k] : -1;
    for (int t = 0; t < nsites; t++) { g_tprim[t] = sites[3 * t]; g_tcall[t] = sites[3 * t + 1]; g_tulps[t] = sites[3 * t + 2]; }
    g_tn = nsites;
    shade_pixel(&c, x, y, frame, last4, out4, NULL);
    for (int k = 0; k < WIT_MAX_FLIPS; k++) g_flip_at[k] = -1;
    g_tn = 0;
    g_pow_neg_nan = 0;
    return tl_dec_n;
}

/* distance from the reference in units of the band: <= 1 is inside (tests/tolerances.py within(); NaN == NaN agrees: the reference has
 * NaN pixels by design) */
static double wit_distance(const float *ref3, const float *got, double band)
{
    int refNan = 0, gotNan = 0;
    double worst = 0.0;
    for (int ch = 0; ch < 3; ch++) { refNan |= ref3[ch] != ref3[ch]; gotNan |= got[ch] != got[ch]; }
    if (refNan || gotNan) return refNan && gotNan ? 0.0 : INFINITY;
    for (int ch = 0; ch < 3; ch++) {
        const double r = ref3[ch], tolc = band * (fabs(r) > 1.0 ? fabs(r) : 1.0), d = fabs(r - (double)got[ch]) / tolc;
        if (!(d <= worst)) worst = d; /* (inf / NaN stay) */
    }
    return worst;
}
static int wit_cmp_gap(const void *a, const void *b)
{
    const float ga = ((const float *)a)[1], gb = ((const float *)b)[1];
    return ga < gb ? -1 : ga > gb;
}
typedef struct { int prim, call; double move; } WitSite;
static int wit_cmp_move(const void *a, const void *b)
{
    const double ma = ((const WitSite *)a)->move, mb = ((const WitSite *)b)->move;
    return ma > mb ? -1 : ma < mb;
}
/* what implementations may differ by, in ulps, per primitive (0 rcp, 1 rsqrt, 2 sqrt, 3 sin, 4 cos, 5 exp, 6 pow5): GLSL 4.60 section 4.7.1
 * allows 2.5 ulp for a / b, 2 for inversesqrt, leaves sin / cos / exp to the implementation and derives pow from exp2 / log2 (llvmpipe's
 * pow(x, 5) is ~22 ulps from the product, its exp ~16); the search stays well inside */
static const int wit_ulps[10] = { 2, 2, 2, 4, 4, 4, 16, 1, 1, 1 }; /* (7 = a multiply-add unfused, 8 = a true division, 9 = the other form of mix: on or off) */

/* witness build: search a conforming neighbour of the contract that puts pixel (x, y) of frame `frame` inside band * max(1, |ref|) of
 * the reference's value ref3.  Order: (0) pow() of a negative base returns NaN (undefined in GLSL; llvmpipe does); (1) each comparison whose operands are closer than closeGap (relative to their scale), nearest
 * first, inverted alone; (2) each call of each primitive alone, +-1 .. its allowance; (3) pairs: a close comparison inverted + one LATER
 * close comparison of the changed path inverted; (4) several calls at once: the calls that move the pixel at all, most sensitive first,
 * each set to the shift (within its allowance) that brings the pixel nearest, two sweeps (coordinate descent).
 * (5) every combination of -2 .. +2 ulps on the six most sensitive calls.
 * Returns 0 = none, 1 = single flip, 2 = single call, 3 = pair of flips, 4 / 5 = several calls, 9 = pow(x < 0, 5) = NaN, 7 / 8 = no neighbour inside but the path
 * (with one comparison inverted / as it is) ends in the environment lookup of a NaN direction, undefined in GL; flips3 / sites (capacity 3 * 32) / *nsites
 * describe the witness for pto_render_pixel_variant; stats4 = { variants evaluated, calls that move the pixel by more than the band
 * when one ulp off, the largest such move in units of the band x 1000 (saturated), the remaining distance in units of the band x 1000 }.
 * out4 = the witness's (or the nearest variant's) pixel.  Single-threaded. */
PTO_API int pto_witness_search(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                               int x, int y, int frame, const float *last4, const float *ref3, double band,
                               float closeGap, int maxFlips, int *flips3, int *sites, int *nsites, int *stats4, float *out4)
{
    Ctx c;
    make_ctx(&c, p, basic144, objects26624, env);
    int tried = 0, found = 0;
    float base[4], v[4];
    flips3[0] = flips3[1] = flips3[2] = -1;
    *nsites = 0;
    /* dry pass: the decisions worth inverting and the primitives' call counts */
    static float close1[WIT_MAX_CLOSE][2], close2[WIT_MAX_CLOSE][2];
    static WitSite moved[65536];
    int calls[10], nmoved = 0, unstable = 0;
    double largest = 0.0;
    g_record_gap = closeGap;
    shade_pixel(&c, x, y, frame, last4, base, NULL);
    memcpy(out4, base, sizeof base);
    const int baseNanEnv = tl_nan_env;
    int flipToNanEnv = -1;
    const int n1 = tl_close_n;
    for (int k = 0; k < n1; k++) { close1[k][0] = (float)tl_close[k].idx; close1[k][1] = tl_close[k].gap; }
    memcpy(calls, tl_call_n, sizeof calls);
    qsort(close1, (size_t)n1, sizeof close1[0], wit_cmp_gap);
    const int nf = n1 < maxFlips ? n1 : maxFlips;
    g_record_gap = 0.0f;
    for (int mode = 1; mode <= 2 && !found; mode++) { /* (0) pow(x < 0, 5) = NaN: 1 - cos(theta) an ulp below zero in the Fresnel term (a camera at the centre of a glass sphere) */
        g_pow_neg_nan = mode;
        shade_pixel(&c, x, y, frame, last4, v, NULL);
        g_pow_neg_nan = 0;
        tried++;
        if (wit_distance(ref3, v, band) <= 1.0) { found = 9; flips3[2] = mode; memcpy(out4, v, sizeof v); } /* (flips3[2]: the mode, for the replay) */
        else if (tl_nan_env && !baseNanEnv && flipToNanEnv == -1) { flipToNanEnv = -2; flips3[2] = mode; }
    }
    for (int k = 0; k < nf && !found; k++) { /* (1) */
        g_flip_at[0] = (int)close1[k][0];
        shade_pixel(&c, x, y, frame, last4, v, NULL);
        tried++;
        if (wit_distance(ref3, v, band) <= 1.0) { found = 1; flips3[0] = g_flip_at[0]; memcpy(out4, v, sizeof v); }
        else if (tl_nan_env && flipToNanEnv < 0) flipToNanEnv = g_flip_at[0];
    }
    g_flip_at[0] = -1;
    g_tn = 1;
    for (int prim = 0; prim < 10 && !found; prim++) /* (2) */
        for (int n = 0; n < calls[prim] && !found; n++)
            for (int u = 1; u <= wit_ulps[prim] && !found; u++)
                for (int sgn = 1; sgn >= (prim >= 7 ? 1 : -1) && !found; sgn -= 2) {
                    g_tprim[0] = prim; g_tcall[0] = n; g_tulps[0] = sgn * u;
                    shade_pixel(&c, x, y, frame, last4, v, NULL);
                    tried++;
                    if (wit_distance(ref3, v, band) <= 1.0) {
                        found = 2; sites[0] = prim; sites[1] = n; sites[2] = sgn * u; *nsites = 1; memcpy(out4, v, sizeof v);
                    }
                    if (u == 1 && sgn == 1) { /* how far ONE ulp at this call moves the pixel, in units of the band around the contract's value */
                        const double mv = wit_distance(base, v, band);
                        if (mv > 1.0) unstable++;
                        if (mv > largest) largest = mv;
                        if (mv > 0.0 && nmoved < 65536) { moved[nmoved].prim = prim; moved[nmoved].call = n; moved[nmoved].move = mv; nmoved++; }
                    }
                }
    g_tn = 0;
    const int npair = nf < 24 ? nf : 24;
    for (int k = 0; k < npair && !found; k++) { /* (3) */
        const int first = (int)close1[k][0];
        g_flip_at[0] = first;
        g_record_gap = closeGap;
        shade_pixel(&c, x, y, frame, last4, v, NULL);
        g_record_gap = 0.0f;
        int n2 = 0;
        for (int q = 0; q < tl_close_n; q++)
            if (tl_close[q].idx > first) { close2[n2][0] = (float)tl_close[q].idx; close2[n2][1] = tl_close[q].gap; n2++; }
        qsort(close2, (size_t)n2, sizeof close2[0], wit_cmp_gap);
        if (n2 > 24) n2 = 24;
        for (int q = 0; q < n2 && !found; q++) {
            g_flip_at[1] = (int)close2[q][0];
            shade_pixel(&c, x, y, frame, last4, v, NULL);
            tried++;
            if (wit_distance(ref3, v, band) <= 1.0) { found = 3; flips3[0] = first; flips3[1] = g_flip_at[1]; memcpy(out4, v, sizeof v); }
        }
        g_flip_at[1] = -1;
    }
    g_flip_at[0] = g_flip_at[1] = -1;
    double best = wit_distance(ref3, base, band);
    if (!found && nmoved > 0 && best < INFINITY) { /* (4) */
        qsort(moved, (size_t)nmoved, sizeof moved[0], wit_cmp_move);
        const int ns = nmoved < WIT_MAX_SITES ? nmoved : WIT_MAX_SITES;
        for (int t = 0; t < ns; t++) { g_tprim[t] = moved[t].prim; g_tcall[t] = moved[t].call; g_tulps[t] = 0; }
        g_tn = ns;
        for (int sweep = 0; sweep < 2 && !found; sweep++)
            for (int t = 0; t < ns && !found; t++) {
                const int U = wit_ulps[g_tprim[t]];
                int keep = g_tulps[t];
                for (int u = (g_tprim[t] >= 7 ? 0 : -U); u <= U && !found; u++) {
                    if (u == keep) continue;
                    g_tulps[t] = u;
                    shade_pixel(&c, x, y, frame, last4, v, NULL);
                    tried++;
                    const double dist = wit_distance(ref3, v, band);
                    if (dist < best) { best = dist; keep = u; memcpy(out4, v, sizeof v); }
                    if (dist <= 1.0) found = 4;
                }
                g_tulps[t] = keep;
            }
        /* (5) the paths that amplify answer a shifted call CHAOTICALLY (the roundings downstream change too: +1 ulp at one normalisation
           moved a pixel by -0.3 bands, -1 by -1.2, +2 by +2.8), so shifts do not add up and descent is a poor guide: enumerate every
           combination of -2 .. +2 ulps on the six calls the pixel is most sensitive to (15,625 neighbours of the contract) */
        if (!found) {
            const int K = ns < 6 ? ns : 6;
            int odo[6], lo[6], hi[6];
            for (int t = 0; t < K; t++) { lo[t] = g_tprim[t] >= 7 ? 0 : -2; hi[t] = g_tprim[t] >= 7 ? 1 : 2; odo[t] = lo[t]; }
            for (int t = 0; t < ns; t++) g_tulps[t] = 0;
            g_tn = K;
            for (;;) {
                for (int t = 0; t < K; t++) g_tulps[t] = odo[t];
                shade_pixel(&c, x, y, frame, last4, v, NULL);
                tried++;
                const double dist = wit_distance(ref3, v, band);
                if (dist < best) { best = dist; memcpy(out4, v, sizeof v); }
                if (dist <= 1.0) { found = 5; break; }
                int t = 0;
                while (t < K && ++odo[t] > hi[t]) { odo[t] = lo[t]; t++; }
                if (t == K) break;
            }
            if (!found) for (int t = 0; t < K; t++) g_tulps[t] = 0;
        }
        if (found) {
            int m = 0;
            for (int t = 0; t < ns; t++)
                if (g_tulps[t] != 0) { sites[3 * m] = g_tprim[t]; sites[3 * m + 1] = g_tcall[t]; sites[3 * m + 2] = g_tulps[t]; m++; }
            *nsites = m;
        }
        g_tn = 0;
    }
    /* no neighbour lands inside, but the pixel's path — the contract's (8), or the contract's with one close comparison inverted (7, e.g.
       refract's k < 0: total internal reflection -> refract() = 0 -> normalize(0) = NaN) — ends in texture(env, NaN direction), which GL
       leaves undefined: llvmpipe returns one deterministic texel average, the contract another (docs/parity.md) */
    if (!found && baseNanEnv) found = 8;
    if (!found && flipToNanEnv != -1) { found = 7; flips3[0] = flipToNanEnv; /* (-2: through pow(x < 0) = NaN) */ }
    stats4[0] = tried;
    stats4[1] = unstable;
    stats4[2] = largest * 1000.0 < 2e9 ? (int)(largest * 1000.0) : 2000000000;
    stats4[3] = found ? 0 : (best * 1000.0 < 2e9 ? (int)(best * 1000.0) : 2000000000);
    return found;
}
