/*
 * pt_oracle.c — CPU restatement of the reference's path-tracing integrator.  TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may build, load or call this file.
 * The product (opentk-pathtracer_amd/csrc, libmi355pt.so) never includes, links or falls back to it.
 *
 * What it restates, function by function (all paths relative to /root/reference/OpenTK-PathTracer/):
 *   res/shaders/PathTracing/compute.glsl:101-369          the integrator (cited per function below)
 *   res/shaders/AtmosphericScattering/compute.glsl:30-171 the atmosphere env-map precompute
 *   res/shaders/PostProcessing/fragment.glsl:17-44        ACES tone map + gamma -> RGBA8 (the step after the path)
 *   src/Render/PathTracer.cs:114-129                      frame counter / dispatch semantics
 *
 * PINNING: the reference has no tests or golden vectors of its own.  This oracle is
 * pinned against outputs of the reference ITSELF run in the build container: the unmodified GLSL executed
 * by Mesa llvmpipe through oracle/glsl_ref/glsl_runner.c; the resulting fixtures are committed under
 * tests/golden/ (generator: tests/golden/make_golden.py) and checked by tests/test_oracle_vs_reference.py.
 *
 * ARITHMETIC CONTRACT ("pt-f32", shared with the HIP kernel so that HIP == oracle BIT-FOR-BIT):
 *   - every value is IEEE-754 binary32; +,-,* are correctly rounded; denormals are kept;
 *   - a*b+c is fused ONLY where this file writes fmaf() (inside the primitives) or c_fma() (everywhere else: the same fmaf, spelled
 *     differently so that a study build can tell the two apart) — compile with -ffp-contract=off;
 *   - dot(a,b)      = fma(a.z,b.z, fma(a.y,b.y, a.x*b.x))
 *   - 1/x           = f_rcp(x): bit-trick seed 0x7EF311C7 - bits(x), three Newton steps y += y*fma(-x,y,1)
 *                     (measured <= 0.51 ulp over 6e6 samples); |x| < FLT_MIN -> +-inf.  a/b is evaluated as a * f_rcp(b)
 *                     everywhere on the per-bounce path (GLSL 4.50 section 4.7.1 allows 2.5 ulp for a/b), and a
 *                     vector divided by a scalar uses ONE reciprocal.  Per-frame uniform reciprocals (1/W, 1/H, 1/SPP,
 *                     1/(frame+1)) and 1/radius (computed once per sphere) use the correctly rounded IEEE quotient.
 *   - inversesqrt(x)= f_rsqrt(x): seed 0x5F3759DF - (bits(x)>>1), three Newton steps (<= 1.7 ulp; GLSL allows 2);
 *                     x < FLT_MIN -> +inf (x >= 0) or NaN (x < 0), so normalize(vec3(0)) is still NaN
 *   - normalize(v)  = v * f_rsqrt(dot(v,v))
 *   - sqrt(x)       = pt_sqrt(x) on the per-bounce path (sphere roots, hemisphere / lens sampling, refract): the same
 *                     seed, TWO Newton steps, then s = x*y; s += fma(-s,s,x) * (y/2)  (<= 0.501 ulp; GLSL inherits
 *                     sqrt's precision from 1/inversesqrt = 2 ulp).  The atmosphere precompute uses it for its per-step
 *                     roots and heights too (round 5; the once-per-texel terms keep IEEE sqrtf and `/`).
 *   - mix(x,y,a)    = fma(y, a, x*(1-a))                       (GLSL 4.50 section 8.3 definition)
 *   - min/max       = IEEE minNum/maxNum (fminf/fmaxf); GLSL leaves NaN handling undefined
 *   - sin/cos/exp   = the fixed polynomial algorithms below (<= ~1.5 ulp), pow(x,5) = x*(x^2)^2,
 *                     pow(x,1.5) = x*sqrt(x)
 *   - cuboid slabs  : (Min-O)/D is evaluated as (Min-O) * f_rcp(D) (one reciprocal per ray component instead of six
 *                     divisions per cuboid).  Define PT_SLAB_TRUE_DIVISION to get the literal IEEE a/b form (kept for
 *                     the fidelity study in DESIGN.md; the HIP kernel implements the reciprocal form).
 *   Why software reciprocals: the correctly rounded IEEE divide / sqrt expand to 43 / 52 issue cycles on gfx950
 *   (tools/ubench.hip) and were 22 % of the integrator's vector work; hardware v_rcp/v_rsq cannot be reproduced on a
 *   CPU, these sequences can — so the GPU result stays bit-identical to this file.
 *   GLSL itself leaves precision of all of these implementation-defined; llvmpipe is one realisation, this
 *   contract is another.  The stated tolerance against llvmpipe lives in tests/test_oracle_vs_reference.py.
 *
 * STUDY BUILDS live in translation units of their own that #include this file: oracle/study/pt_oracle_witness.c (perturbation, targeted
 * sites, ensemble, path signature, base variants, witness search; llvmpipe's built-ins in oracle/pt_oracle_llvmpipe.h) and
 * oracle/study/pt_oracle_margins.c (decision margins).  They can enter this file ONLY through the hooks of pt_oracle_hooks.h, each
 * of which has its identity default there: compiled on its own, this file is the contract and nothing else.
 *
 * Build: gcc -O2 -ffp-contract=off -mfma -shared -fPIC pt_oracle.c -o _build/libpt_oracle.so -lm -lpthread   (oracle/Makefile)
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "pt_oracle_hooks.h"

#define PTO_API __attribute__((visibility("default")))

#define FLOAT_MAX 3.4028235e+38f /* compute.glsl:2 */
#define FLOAT_MIN -3.4028235e+38f /* compute.glsl:3 */
#define EPSILON 0.001f            /* compute.glsl:4 */
#define PI 3.14159265f            /* compute.glsl:5 */

typedef struct v3 { float x, y, z; } v3;

/* ------------------------------------------------------------------ pt-f32 primitives */
static inline float f_min(float a, float b) { return fminf(a, b); }
static inline float f_max(float a, float b) { return fmaxf(a, b); }
static inline uint32_t f_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float f_unbits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
/* pt-f32 reciprocal: seed by exponent negation, three Newton steps; zero and denormals give +-inf */
static inline float f_rcp(float x)
{
#ifdef PT_EXACT_DIVSQRT /* fidelity study only (oracle/Makefile): correctly rounded 1/x, 1/sqrt(x), sqrt(x) as llvmpipe's / and sqrt are */
    return 1.0f / x;
#endif
    ALT_PRIMITIVE(0, x);
    float y = f_unbits(0x7EF311C7u - f_bits(x));
    float e = fmaf(-x, y, 1.0f); y = fmaf(y, e, y);
    e = fmaf(-x, y, 1.0f); y = fmaf(y, e, y);
    e = fmaf(-x, y, 1.0f); y = fmaf(y, e, y);
    if (fabsf(x) < 1.17549435e-38f) y = copysignf(INFINITY, x);
    return perturbed(0, y);
}
/* pt-f32 inverse square root: classic seed, three Newton steps; zero/denormal -> +inf, negative -> NaN */
static inline float f_rsqrt(float x)
{
#ifdef PT_EXACT_DIVSQRT
    return 1.0f / sqrtf(x);
#endif
    ALT_PRIMITIVE(1, x);
    float y = f_unbits(0x5F3759DFu - (f_bits(x) >> 1));
    float h = 0.5f * x, t;
    t = y * y; t = fmaf(-h, t, 1.5f); y = y * t;
    t = y * y; t = fmaf(-h, t, 1.5f); y = y * t;
    t = y * y; t = fmaf(-h, t, 1.5f); y = y * t;
    if (x < 1.17549435e-38f) y = x < 0.0f ? NAN : INFINITY;
    return perturbed(1, y);
}
/* pt-f32 square root: two Newton steps y *= 1.5 - (x/2*y)*y on the same seed (4.7e-6), then one residual correction
 * s += (x - s*s) * y/2  (<= 0.501 ulp); sqrt(0) = 0 exactly; negative, infinite and NaN inputs give a non-finite value
 * (every call site guards its argument: discriminant >= 0, 1 - z*z >= 0, k >= 0, rand in [0,1]) */
static inline float pt_sqrt(float x)
{
#ifdef PT_EXACT_DIVSQRT
    return sqrtf(x);
#endif
    ALT_PRIMITIVE(2, x);
    float y = f_unbits(0x5F3759DFu - (f_bits(x) >> 1));
    float h = 0.5f * x, t;
    t = h * y; t = fmaf(-t, y, 1.5f); y = y * t;
    t = h * y; t = fmaf(-t, y, 1.5f); y = y * t;
    float s = x * y;
    float r = fmaf(-s, s, x);
    return perturbed(2, fmaf(r, 0.5f * y, s));
}
static inline float f_mix(float x, float y, float a)
{
    if (MIX_OTHER_FORM()) return x + a * (y - x);
    return c_fma(y, a, x * (1.0f - a));
}

static inline v3 V(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static inline v3 v_add(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline v3 v_sub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 v_mul(v3 a, v3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline v3 v_scale(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
static inline v3 v_neg(v3 a) { return V(-a.x, -a.y, -a.z); }
/* a + b*s, fused */
static inline v3 v_fma(v3 b, float s, v3 a) { return V(c_fma(b.x, s, a.x), c_fma(b.y, s, a.y), c_fma(b.z, s, a.z)); }
static inline float v_dot(v3 a, v3 b)
{
    ALT_DOT(a, b);
    return c_fma(a.z, b.z, c_fma(a.y, b.y, a.x * b.x));
}
static inline v3 v_normalize(v3 a) { return v_scale(a, f_rsqrt(v_dot(a, a))); }
static inline v3 v_mix(v3 x, v3 y, float a)
{
    float ia = 1.0f - a;
    if (MIX_OTHER_FORM()) return V(x.x + a * (y.x - x.x), x.y + a * (y.y - x.y), x.z + a * (y.z - x.z));
    return V(c_fma(y.x, a, x.x * ia), c_fma(y.y, a, x.y * ia), c_fma(y.z, a, x.z * ia));
}

static inline float f_from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

/* sin and cos of a (radians), |a| small (the integrator only passes [0, 2*pi]).  Cody-Waite reduction by pi/2
 * with two fused steps, then the classic single-precision minimax polynomials on [-pi/4, pi/4]. */
static void f_sincos(float a, float *sn, float *cs)
{
    ALT_SINCOS(a, sn, cs);
    float k = rintf(a * 0.636619772f);
    float r = fmaf(k, -1.57079637050628662109375f, a);
    r = fmaf(k, 4.37113900018624283e-8f, r);
    float z = r * r;
    float ps = fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
    float s = fmaf(ps * z, r, r);
    float pc = fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
    float c = fmaf(pc * z, z, fmaf(-0.5f, z, 1.0f));
    int q = (int)k & 3;
    float s_out = (q & 1) ? c : s;
    float c_out = (q & 1) ? s : c;
    if (q == 1 || q == 2) c_out = -c_out;
    if (q >= 2) s_out = -s_out;
    *sn = perturbed(3, s_out);
    *cs = perturbed(4, c_out);
}

/* e^x.  n = rint(x*log2 e), r = x - n*ln2 (two fused steps), degree-6 polynomial, 2^n applied as two exact
 * power-of-two factors so that denormal results are rounded once. */
static float f_exp(float x)
{
    ALT_PRIMITIVE(5, x);
    if (x != x) return x;
    if (x > 88.72283935546875f) return INFINITY;
    if (x < -104.0f) return 0.0f;
    float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(n, -0.693145751953125f, x);
    r = fmaf(n, -1.428606765330187045e-06f, r);
    float p = fmaf(1.9875691500e-4f, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    float y = fmaf(p, r * r, r) + 1.0f;
    int ni = (int)n;
    int n1 = ni >> 1, n2 = ni - n1;
    y = y * f_from_bits((uint32_t)(n1 + 127) << 23);
    return perturbed(5, y * f_from_bits((uint32_t)(n2 + 127) << 23));
}

static inline float f_pow5(float x) /* (GLSL: pow(x, 5.0) — llvmpipe's is ~22 ulp off) */
{
    ALT_PRIMITIVE(6, x);
    float x2 = x * x;
    return perturbed(6, x * (x2 * x2));
}

/* ------------------------------------------------------------------ scene blob accessors (std140, compute.glsl:13-42,66-70) */
#define SPHERE_STRIDE 20  /* floats: 80 B  */
#define CUBOID_STRIDE 24  /* floats: 96 B  */
#define CUBOIDS_OFFSET 5120 /* floats: 20480 B = 256 * 80 */

typedef struct {
    v3 albedo;   float specularChance;
    v3 emissiv;  float specularRoughness;
    v3 absorbance; float refractionChance;
    float refractionRoughness, ior;
} Material;

static Material load_material(const float *m)
{
    Material r;
    r.albedo = V(m[0], m[1], m[2]);      r.specularChance = m[3];
    r.emissiv = V(m[4], m[5], m[6]);     r.specularRoughness = m[7];
    r.absorbance = V(m[8], m[9], m[10]); r.refractionChance = m[11];
    r.refractionRoughness = m[12];       r.ior = m[13];
    return r;
}

typedef struct Ctx {
    /* BasicDataUBO, compute.glsl:59-64: float[4c+r] = element (row r, col c) of the GLSL matrix */
    float invProj[16], invView[16];
    v3 viewPos;
    const float *objects; /* 6656 floats */
    int numSpheres, numCuboids; /* loops are `int i < float n` (compute.glsl:231,244): i < n  <=>  i < ceil(n) */
    int rayDepth, spp;
    float focalLength, apertureDiameter;
    int width, height;
    int envSize, envFormat; /* 0 = RGBA32F (float[6][S][S][4]), 1 = SRGB8_A8 (uint8[6][S][S][4]) */
    const void *env;
    float srgbLut[256];
} Ctx;

typedef struct { uint64_t samples, bounces, sphereTests, cuboidTests, envLookups, rngDraws; } Stats;

/* ------------------------------------------------------------------ RNG (compute.glsl:334-344) */
static inline uint32_t pcg_hash(uint32_t *seed)
{
    *seed = *seed * 747796405u + 2891336453u;
    uint32_t word = ((*seed >> ((*seed >> 28u) + 4u)) ^ *seed) * 277803737u;
    return (word >> 22u) ^ word;
}
static inline float rand01(uint32_t *seed) { return (float)pcg_hash(seed) * 2.3283064365386962890625e-10f; /* / 2^32, exact */ }

/* ------------------------------------------------------------------ environment lookup (compute.glsl:177)
 * texture(samplerCube, dir) from a compute stage: no derivatives -> LOD 0 -> MAG filter = LINEAR
 * (MainWindow.cs:178, AtmosphericScatterer.cs:68), GL_TEXTURE_CUBE_MAP_SEAMLESS on (MainWindow.cs:168).
 * Face selection / (s,t) mapping: OpenGL 4.5 core spec, table 8.19; ties go Z, then X, then Y (llvmpipe).
 * Seamless filtering: taps that fall off a face edge are fetched from the adjacent face; at a cube corner the
 * tap that falls off two edges has no texel and is replaced by the average of the other three.
 * SRGB8_A8 texels are linearised before filtering (GL 4.5 section 8.24). */
typedef struct rgb { float r, g, b; } rgb;

static rgb env_texel(const Ctx *c, int face, int x, int y)
{
    size_t idx = (((size_t)face * c->envSize + (size_t)y) * c->envSize + (size_t)x) * 4;
    rgb o;
    if (c->envFormat == 0) {
        const float *p = (const float *)c->env + idx;
        o.r = p[0]; o.g = p[1]; o.b = p[2];
    } else {
        const uint8_t *p = (const uint8_t *)c->env + idx;
        o.r = c->srgbLut[p[0]]; o.g = c->srgbLut[p[1]]; o.b = c->srgbLut[p[2]];
    }
    return o;
}

static void dir_to_face(float x, float y, float z, int *face, float *sc, float *tc, float *ma)
{
    float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    if (az >= f_max(ax, ay)) { *face = z < 0.0f ? 5 : 4; *ma = az; *sc = z < 0.0f ? -x : x; *tc = -y; }
    else if (ax >= ay)       { *face = x < 0.0f ? 1 : 0; *ma = ax; *sc = x < 0.0f ? z : -z; *tc = -y; }
    else                     { *face = y < 0.0f ? 3 : 2; *ma = ay; *sc = x; *tc = y < 0.0f ? -z : z; }
}

/* Texel (ix,iy) one step outside `face` -> (face, x, y) of the texel across the seam, in integers, exact for every size.
 * Lattice: the centre of texel (x,y) of a face sits at in-face coordinates (2x+1-S, 2y+1-S) on the cube of half-width S, the face's
 * own axis at +-S (inverse of table 8.19).  A tap one step off the face has one in-face coordinate at +-(S+1); its neighbour is the
 * border texel of the face that coordinate points to: that axis becomes the new major axis, the old major axis drops to the outermost
 * texel centre +-(S-1), the coordinate along the edge is kept.  So the tap is written with S-1 on its own axis, the overflowing
 * +-(S+1) is the unique largest component, and table 8.19 in integers returns the neighbour's lattice point; (c+S-1)/2 is its texel.
 * (The earlier rule re-projected the tap's centre through 3D in binary32 and took floor: one texel off along the edge next to a
 * face corner at some sizes from 3352 upwards, the same texel as this rule at every border tap of every size below.)
 * Taps further out (both coordinates off, or two steps off: only NaN / inf / subnormal directions reach them through the clamp in
 * sample_env) get a defined texel inside the cube through the same ties (Z, X, Y) and the final clamp. */
static void env_wrapped_index(int S, int face, int ix, int iy, int *nface, int *nx, int *ny)
{
    const int a = 2 * ix + 1 - S, b = 2 * iy + 1 - S, m = S - 1;
    int x, y, z, sc, tc;
    switch (face) {
    case 0: x = m;   y = -b;  z = -a;  break;
    case 1: x = -m;  y = -b;  z = a;   break;
    case 2: x = a;   y = m;   z = b;   break;
    case 3: x = a;   y = -m;  z = -b;  break;
    case 4: x = a;   y = -b;  z = m;   break;
    default: x = -a; y = -b;  z = -m;  break;
    }
    const int ax = x < 0 ? -x : x, ay = y < 0 ? -y : y, az = z < 0 ? -z : z;
    if (az >= (ax > ay ? ax : ay)) { *nface = z < 0 ? 5 : 4; sc = z < 0 ? -x : x; tc = -y; }
    else if (ax >= ay)             { *nface = x < 0 ? 1 : 0; sc = x < 0 ? z : -z; tc = -y; }
    else                           { *nface = y < 0 ? 3 : 2; sc = x; tc = y < 0 ? -z : z; }
    int u = (sc + m) >> 1, v = (tc + m) >> 1; /* sc + m is even for a texel centre; >> floors the off-lattice cases */
    if (u < 0) u = 0; if (u > m) u = m;
    if (v < 0) v = 0; if (v > m) v = m;
    *nx = u; *ny = v;
}

/* integer texel (ix,iy), possibly outside `face` -> the texel itself or the one across the seam */
static rgb env_texel_wrapped(const Ctx *c, int face, int ix, int iy)
{
    int S = c->envSize, nface, nx, ny;
    if (ix >= 0 && ix < S && iy >= 0 && iy < S) return env_texel(c, face, ix, iy);
    env_wrapped_index(S, face, ix, iy, &nface, &nx, &ny);
    return env_texel(c, nface, nx, ny);
}

static rgb sample_env(const Ctx *c, v3 d)
{
#ifdef PT_ORACLE_MARK_NAN_ENV /* diagnostic build only (oracle/Makefile): flag the paths that end in texture(env, NaN direction) */
    if (d.x != d.x || d.y != d.y || d.z != d.z) { rgb mark = { 1000.0f, 1000.0f, 1000.0f }; return mark; }
#endif
    ALT_NAN_ENV(d);
    int S = c->envSize, face;
    float sc, tc, ma;
    dir_to_face(d.x, d.y, d.z, &face, &sc, &tc, &ma);
    float ima = 0.5f * f_rcp(ma);
    float fs = (float)S;
    float u = c_fma(sc, ima, 0.5f) * fs - 0.5f;
    float v = c_fma(tc, ima, 0.5f) * fs - 0.5f;
    /* NaN / inf coordinates (NaN ray directions, compute.glsl:211 with total internal reflection):
       clamp so that the integer conversion below is defined identically on CPU and GPU */
    u = f_min(f_max(u, -1.0f), fs);
    v = f_min(f_max(v, -1.0f), fs);
    float fu = floorf(u), fv = floorf(v);
    float wu = u - fu, wv = v - fv;
    int x0 = (int)fu, y0 = (int)fv, x1 = x0 + 1, y1 = y0 + 1;
    int offx0 = x0 < 0, offx1 = x1 >= S, offy0 = y0 < 0, offy1 = y1 >= S;
    float w00 = (1.0f - wu) * (1.0f - wv), w10 = wu * (1.0f - wv), w01 = (1.0f - wu) * wv, w11 = wu * wv;
    int miss00 = offx0 && offy0, miss10 = offx1 && offy0, miss01 = offx0 && offy1, miss11 = offx1 && offy1;
    rgb t00 = { 0, 0, 0 }, t10 = t00, t01 = t00, t11 = t00;
    if (!miss00) t00 = env_texel_wrapped(c, face, x0, y0);
    if (!miss10) t10 = env_texel_wrapped(c, face, x1, y0);
    if (!miss01) t01 = env_texel_wrapped(c, face, x0, y1);
    if (!miss11) t11 = env_texel_wrapped(c, face, x1, y1);
    if (miss00 || miss10 || miss01 || miss11) {
        /* cube corner: the tap that fell off two edges has no texel; it is replaced by the average of the other
           three, i.e. its bilinear weight is shared equally among them (llvmpipe behaviour — pinned by the
           tiny-cube fixtures in tests/golden; GL 4.5 section 8.14.2 recommends exactly this average) */
        float a = (miss00 ? w00 : miss10 ? w10 : miss01 ? w01 : w11) * 0.333333343f;
        w00 = miss00 ? 0.0f : w00 + a; w10 = miss10 ? 0.0f : w10 + a;
        w01 = miss01 ? 0.0f : w01 + a; w11 = miss11 ? 0.0f : w11 + a;
    }
    const int corner = miss00 || miss10 || miss01 || miss11;
    rgb o;
    o.r = ENV_FILTER(corner, t00.r, t10.r, t01.r, t11.r, wu, wv, c_fma(t11.r, w11, c_fma(t01.r, w01, c_fma(t10.r, w10, t00.r * w00))));
    o.g = ENV_FILTER(corner, t00.g, t10.g, t01.g, t11.g, wu, wv, c_fma(t11.g, w11, c_fma(t01.g, w01, c_fma(t10.g, w10, t00.g * w00))));
    o.b = ENV_FILTER(corner, t00.b, t10.b, t01.b, t11.b, wu, wv, c_fma(t11.b, w11, c_fma(t01.b, w01, c_fma(t10.b, w10, t00.b * w00))));
    return o;
}

/* ------------------------------------------------------------------ intersections */
/* compute.glsl:261-277 RaySphereIntersect */
static int ray_sphere(v3 o, v3 d, v3 pos, float radius, float *t1, float *t2)
{
    *t1 = *t2 = FLOAT_MAX;
    v3 oc = v_sub(o, pos);
    float b = v_dot(d, oc);
    float c = c_fma(-radius, radius, v_dot(oc, oc));
    float disc = c_fma(b, b, -c);
    if (DECIDE(disc < 0.0f, disc, f_max(b * b, fabsf(c)))) return 0;
    FLIPPED_NONNEG(disc);
    float s = pt_sqrt(disc);
    *t1 = -b - s;
    *t2 = -b + s;
    return *t1 <= *t2;
}

/* compute.glsl:280-294 RayCuboidIntersect */
static int ray_cuboid(v3 o, v3 d, v3 invd, v3 mn, v3 mx, float *t1, float *t2)
{
#ifdef PT_SLAB_TRUE_DIVISION
    (void)invd;
    v3 t0s = V((mn.x - o.x) / d.x, (mn.y - o.y) / d.y, (mn.z - o.z) / d.z);
    v3 t1s = V((mx.x - o.x) / d.x, (mx.y - o.y) / d.y, (mx.z - o.z) / d.z);
#else
    v3 t0s = v_mul(v_sub(mn, o), invd);
    v3 t1s = v_mul(v_sub(mx, o), invd);
    ALT_SLABS(t0s, t1s, mn, mx, o, d);
#endif
    v3 sm = V(f_min(t0s.x, t1s.x), f_min(t0s.y, t1s.y), f_min(t0s.z, t1s.z));
    v3 bg = V(f_max(t0s.x, t1s.x), f_max(t0s.y, t1s.y), f_max(t0s.z, t1s.z));
    *t1 = f_max(FLOAT_MIN, f_max(sm.x, f_max(sm.y, sm.z)));
    *t2 = f_min(FLOAT_MAX, f_min(bg.x, f_min(bg.y, bg.z)));
    return DECIDE(*t1 <= *t2, *t2 - *t1, f_max(fabsf(*t1), fabsf(*t2)));
}

static inline float f_sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

/* compute.glsl:322-332 GetNormal(Cuboid) */
static v3 cuboid_normal(v3 mn, v3 mx, v3 p)
{
    v3 half = v_scale(v_sub(mx, mn), 0.5f);
    v3 cs = v_sub(p, v_scale(v_add(mx, mn), 0.5f));
    v3 n;
    /* step(edge, x) = x < edge ? 0 : 1 with x = EPSILON, spelled as the comparison it is (three DECIDE sites) */
#define STEP_EPS(c_, h_) (DECIDE(EPSILON < fabsf(fabsf(c_) - (h_)), fabsf(fabsf(c_) - (h_)) - EPSILON, f_max(f_max(fabsf(c_), (h_)), 1.0f)) ? 0.0f : 1.0f)
    n.x = f_sign(cs.x) * STEP_EPS(cs.x, half.x);
    n.y = f_sign(cs.y) * STEP_EPS(cs.y, half.y);
    n.z = f_sign(cs.z) * STEP_EPS(cs.z, half.z);
#undef STEP_EPS
    MARGIN_CUBOID_NORMAL(mn, mx, p, cs, half);
    return v_normalize(n);
}

typedef struct HitInfo {
    float T; int fromInside; v3 nearHitPos, normal; Material m;
} HitInfo;


/* compute.glsl:226-258 RayTrace.  The acceptance test uses the ENTRY distance t1 against the stored
 * GetSmallestPositive(t1,t2) (compute.glsl:234,247,347-350): an object that contains the origin (t1<0) always
 * replaces the current hit.  Objects are visited in reference order.  Material/normal are evaluated once for
 * the surviving candidate (the reference evaluates them per accepted candidate and overwrites). */
static int ray_trace(const Ctx *c, v3 o, v3 d, HitInfo *h, Stats *st)
{
    float T = FLOAT_MAX, t1, t2, wt2 = 0.0f;
    int winner = -1;
    const float *ob = c->objects;
    MARGIN_TRACE_LOCALS;
    for (int i = 0; i < c->numSpheres; i++) {
        const float *s = ob + (size_t)i * SPHERE_STRIDE;
        if (ray_sphere(o, d, V(s[0], s[1], s[2]), s[3], &t1, &t2) && DECIDE(t2 > 0.0f, t2, f_max(fabsf(t1), fabsf(t2))) && DECIDE(t1 < T, t1 - T, f_max(fabsf(t1), fabsf(T)))) {
            MARGIN_NOTE_ACCEPT(T, winner, t1);
            T = DECIDE(t1 < 0.0f, t1, f_max(fabsf(t1), fabsf(t2))) ? t2 : t1;
            wt2 = t2;
            winner = i;
        }
    }
    v3 invd = V(f_rcp(d.x), f_rcp(d.y), f_rcp(d.z));
    for (int i = 0; i < c->numCuboids; i++) {
        const float *q = ob + CUBOIDS_OFFSET + (size_t)i * CUBOID_STRIDE;
        if (ray_cuboid(o, d, invd, V(q[0], q[1], q[2]), V(q[4], q[5], q[6]), &t1, &t2) && DECIDE(t2 > 0.0f, t2, f_max(fabsf(t1), fabsf(t2))) && DECIDE(t1 < T, t1 - T, f_max(fabsf(t1), fabsf(T)))) {
            MARGIN_NOTE_ACCEPT(T, winner, t1);
            T = DECIDE(t1 < 0.0f, t1, f_max(fabsf(t1), fabsf(t2))) ? t2 : t1;
            wt2 = t2;
            winner = 256 + i;
        }
    }
    MARGIN_TRACE(c, o, d, invd, winner, T);
    if (st) { st->sphereTests += (uint64_t)c->numSpheres; st->cuboidTests += (uint64_t)c->numCuboids; }
    if (winner < 0 || !(T != FLOAT_MAX)) return 0; /* compute.glsl:257 */
    h->T = T;
    h->fromInside = (T == wt2);
    SIG_NOTE(0x1000 + winner * 2 + h->fromInside);
    h->nearHitPos = v_fma(d, T, o);
    if (winner < 256) {
        const float *s = ob + (size_t)winner * SPHERE_STRIDE;
        h->m = load_material(s + 4);
        v3 pc = v_sub(h->nearHitPos, V(s[0], s[1], s[2])); /* compute.glsl:316-319 GetNormal(Sphere) */
        const float ir = 1.0f / s[3]; /* 1/radius: IEEE quotient, computed once per sphere */
        h->normal = V(QUOT(pc.x, s[3], ir), QUOT(pc.y, s[3], ir), QUOT(pc.z, s[3], ir));
    } else {
        const float *q = ob + CUBOIDS_OFFSET + (size_t)(winner - 256) * CUBOID_STRIDE;
        h->m = load_material(q + 8);
        h->normal = cuboid_normal(V(q[0], q[1], q[2]), V(q[4], q[5], q[6]), h->nearHitPos);
    }
    return 1;
}

/* ------------------------------------------------------------------ sampling */
/* compute.glsl:297-307 */
static v3 cosine_sample_hemisphere(v3 n, uint32_t *seed)
{
    float z = c_fma(rand01(seed), 2.0f, -1.0f);
    float a = rand01(seed) * 2.0f * PI;
    float r = pt_sqrt(c_fma(-z, z, 1.0f));
    float sn, cs;
    f_sincos(a, &sn, &cs);
    return v_normalize(v_add(n, V(r * cs, r * sn, z)));
}

/* compute.glsl:359-364 */
static float fresnel_schlick(float cosTheta, float n1, float n2)
{
    float r0 = QUOT(n1 - n2, n1 + n2, f_rcp(n1 + n2)); /* (compute.glsl:361 divides; the contract multiplies by the reciprocal) */
    r0 *= r0;
    return c_fma(1.0f - r0, f_pow5(1.0f - cosTheta), r0);
}

static v3 f_reflect(v3 i, v3 n) { return v_fma(n, -(2.0f * v_dot(n, i)), i); }

static v3 f_refract(v3 i, v3 n, float eta)
{
    float ni = v_dot(n, i);
    float k = c_fma(-(eta * eta), c_fma(-ni, ni, 1.0f), 1.0f);
    MARGIN_REFRACT(k, eta, ni);
    if (DECIDE(k < 0.0f, k, f_max(1.0f, eta * eta))) return V(0.0f, 0.0f, 0.0f);
    FLIPPED_NONNEG(k);
    float f = c_fma(eta, ni, pt_sqrt(k));
    return V(c_fma(eta, i.x, -(f * n.x)), c_fma(eta, i.y, -(f * n.y)), c_fma(eta, i.z, -(f * n.z)));
}

/* compute.glsl:184-224 BSDF */
static float bsdf(v3 *ro, v3 *rd, const HitInfo *h, int *isRefractive, uint32_t *seed)
{
    *isRefractive = 0;
    float spec = h->m.specularChance, refr = h->m.refractionChance;
    if (spec > 0.0f) {
        float n1 = h->fromInside ? h->m.ior : 1.0f, n2 = !h->fromInside ? h->m.ior : 1.0f;
        spec = f_mix(spec, 1.0f, fresnel_schlick(v_dot(v_neg(*rd), h->normal), n1, n2));
        float diffuse = 1.0f - spec - refr;
        refr = 1.0f - spec - diffuse;
    }
    v3 diffuseRay = cosine_sample_hemisphere(h->normal, seed);
    float prob;
    float roll = rand01(seed);
    MARGIN_LOBE(h, spec, refr, roll);
    const int lobeSpec = DECIDE(spec > roll, spec - roll, 1.0f);
    if (lobeSpec) {
        v3 refl = f_reflect(*rd, h->normal);
        *rd = v_normalize(v_mix(refl, diffuseRay, h->m.specularRoughness * h->m.specularRoughness));
        prob = spec;
        SIG_NOTE(0x2001);
    } else if (DECIDE(spec + refr > roll, spec + refr - roll, 1.0f)) {
        v3 rf = f_refract(*rd, h->normal, h->fromInside ? h->m.ior : f_rcp(h->m.ior));
        v3 rough = cosine_sample_hemisphere(v_neg(h->normal), seed);
        *rd = v_normalize(v_mix(rf, rough, h->m.refractionRoughness * h->m.refractionRoughness));
        prob = refr;
        *isRefractive = 1;
        SIG_NOTE(0x2002);
    } else {
        *rd = diffuseRay;
        prob = 1.0f - spec - refr;
        SIG_NOTE(0x2000);
    }
    *ro = v_fma(*rd, EPSILON, h->nearHitPos);
    return f_max(prob, EPSILON);
}

/* compute.glsl:132-182 Radiance */
static v3 radiance(const Ctx *c, v3 ro, v3 rd, uint32_t *seed, Stats *st)
{
    v3 throughput = V(1.0f, 1.0f, 1.0f), rad = V(0.0f, 0.0f, 0.0f);
    HitInfo h;
    for (int i = 0; i < c->rayDepth; i++) {
        if (st) st->bounces++;
        if (ray_trace(c, ro, rd, &h, st)) {
            if (h.fromInside) {
                h.normal = v_neg(h.normal);
                throughput.x *= f_exp(-h.m.absorbance.x * h.T);
                throughput.y *= f_exp(-h.m.absorbance.y * h.T);
                throughput.z *= f_exp(-h.m.absorbance.z * h.T);
            }
            MARGIN_HIT(&h);
            int isRefractive;
            float prob = bsdf(&ro, &rd, &h, &isRefractive, seed);
            MARGIN_BOUNCE(&h, ro, throughput);
            rad = V(c_fma(h.m.emissiv.x, throughput.x, rad.x), c_fma(h.m.emissiv.y, throughput.y, rad.y),
                    c_fma(h.m.emissiv.z, throughput.z, rad.z));
            if (!isRefractive) throughput = v_mul(throughput, h.m.albedo);
            {
                const float rprob = f_rcp(prob);
                throughput = V(QUOT(throughput.x, prob, rprob), QUOT(throughput.y, prob, rprob), QUOT(throughput.z, prob, rprob));
            }
            float p = f_max(throughput.x, f_max(throughput.y, throughput.z));
            MARGIN_ROULETTE(c, i, seed, p);
            const float rr_ = rand01(seed);
            if (DECIDE(rr_ > p, rr_ - p, f_max(p, 1.0f))) { SIG_NOTE(0x3001); break; }
            {
                const float rp = f_rcp(p);
                throughput = V(QUOT(throughput.x, p, rp), QUOT(throughput.y, p, rp), QUOT(throughput.z, p, rp));
            }
        } else {
            rgb e = sample_env(c, rd);
            SIG_NOTE(0x3002);
            if (st) st->envLookups++;
            MARGIN_ENV(c, rd, e, throughput);
            rad = V(c_fma(e.r, throughput.x, rad.x), c_fma(e.g, throughput.y, rad.y), c_fma(e.b, throughput.z, rad.z));
            break;
        }
    }
    return rad;
}

/* GLSL mat4 * vec4 with the column-major view of the UBO bytes */
static void mat_vec(const float *m, float x, float y, float z, float w, float *out)
{
    ALT_MAT_VEC(m, x, y, z, w, out);
    for (int r = 0; r < 4; r++)
        out[r] = c_fma(m[12 + r], w, c_fma(m[8 + r], z, c_fma(m[4 + r], y, m[r] * x)));
}

/* compute.glsl:101-130 main, for one pixel; `last` is the pixel's current accumulation value */
static void shade_pixel(const Ctx *c, int px, int py, int frame, const float *last, float *out, Stats *st)
{
    uint32_t seed = ((uint32_t)px * 1973u + (uint32_t)py * 9277u + (uint32_t)frame * 2699u) | 1u; /* :106 */
    v3 irr = V(0.0f, 0.0f, 0.0f);
    PIXEL_BEGIN(last);
    for (int s = 0; s < c->spp; s++) {
        float u0 = rand01(&seed), u1 = rand01(&seed); /* :113, x first */
        float ndcx = c_fma(((float)px + u0) * (1.0f / (float)c->width), 2.0f, -1.0f);  /* uniform 1/W, 1/H */
        float ndcy = c_fma(((float)py + u1) * (1.0f / (float)c->height), 2.0f, -1.0f);
        ALT_NDC(ndcx, ndcy, px, u0, py, u1, c);
        /* GetWorldSpaceRay :352-357 */
        float eye[4], wd[4];
        mat_vec(c->invProj, ndcx, ndcy, -1.0f, 0.0f, eye);
        mat_vec(c->invView, eye[0], eye[1], -1.0f, 0.0f, wd);
        v3 dir = v_normalize(V(wd[0], wd[1], wd[2]));
        v3 focal = v_fma(dir, c->focalLength, c->viewPos); /* :117 */
        /* UniformSampleUnitCircle :309-314 */
        float angle = rand01(&seed) * 2.0f * PI;
        float rr = pt_sqrt(rand01(&seed));
        float sn, cs;
        f_sincos(angle, &sn, &cs);
        float half_ap = c->apertureDiameter * 0.5f;
        float ox = half_ap * (cs * rr), oy = half_ap * (sn * rr);
        float org[4];
        mat_vec(c->invView, ox, oy, 0.0f, 1.0f, org); /* :120 */
        v3 ro = V(org[0], org[1], org[2]);
        v3 rd = v_normalize(v_sub(focal, ro));
        MARGIN_PRIMARY_RAY(ro);
        if (st) st->samples++;
        irr = v_add(irr, radiance(c, ro, rd, &seed, st));
    }
    irr = v_scale(irr, 1.0f / (float)c->spp); /* :125, uniform reciprocal */
    float w = 1.0f / (float)(frame + 1);                  /* :128 */
    out[0] = f_mix(last[0], irr.x, w);
    out[1] = f_mix(last[1], irr.y, w);
    out[2] = f_mix(last[2], irr.z, w);
    out[3] = 1.0f; /* :129 */
    PIXEL_END(out);
}

/* ------------------------------------------------------------------ public C API (ctypes) */
typedef struct {
    int width, height;         /* FULL image size (NDC and seeds use global coordinates) */
    int numSpheres, numCuboids;
    int rayDepth, spp;
    float focalLength, apertureDiameter;
    int envSize, envFormat;
} PtoParams;

static float srgb_to_linear(int v)
{
    /* GL 4.5 section 8.24, evaluated in double and rounded once: a fixed 256-entry table */
    double cs = v / 255.0;
    double cl = cs <= 0.04045 ? cs / 12.92 : pow((cs + 0.055) / 1.055, 2.4);
    return (float)cl;
}

/* Test-only knob: replace the exact GL sRGB decode table, e.g. with llvmpipe's cubic approximation, so that the
 * llvmpipe pinning test can isolate everything else (tests/test_oracle_vs_reference.py). NULL restores exact. */
static float g_lut_override[256];
static int g_lut_overridden = 0;
PTO_API void pto_set_srgb_lut(const float *lut256)
{
    g_lut_overridden = lut256 != NULL;
    if (lut256) memcpy(g_lut_override, lut256, sizeof g_lut_override);
}
static void fill_lut(float *lut)
{
    for (int i = 0; i < 256; i++) lut[i] = g_lut_overridden ? g_lut_override[i] : srgb_to_linear(i);
}

static void make_ctx(Ctx *c, const PtoParams *p, const float *basic, const float *objects, const void *env)
{
    memcpy(c->invProj, basic, 64);
    memcpy(c->invView, basic + 16, 64);
    c->viewPos = V(basic[32], basic[33], basic[34]);
    c->objects = objects;
    c->numSpheres = p->numSpheres; c->numCuboids = p->numCuboids;
    c->rayDepth = p->rayDepth; c->spp = p->spp;
    c->focalLength = p->focalLength; c->apertureDiameter = p->apertureDiameter;
    c->width = p->width; c->height = p->height;
    c->envSize = p->envSize; c->envFormat = p->envFormat; c->env = env;
    fill_lut(c->srgbLut);
}

/* ---- host threading of one frame (bench.py's cpu_baseline leg and the tests).  A persistent pool of worker threads (created on
 * first use, grown on demand, never more than PTO_MAX_THREADS) renders the frame's rows in DYNAMIC chunks of PTO_CHUNK_ROWS rows
 * taken from one atomic counter: rows near the floor cost ~2x sky rows, so a static split leaves most threads idle behind the
 * slowest one, and creating 256 threads per frame costs milliseconds of a sub-second frame.  Which thread renders which row never
 * changes a pixel (every pixel owns its RNG stream, compute.glsl:106): the image is the same for any thread count (tested). */
#define PTO_MAX_THREADS 256
#define PTO_CHUNK_ROWS 4

typedef struct {
    const Ctx *c; float *image; int y0, rows, frame, wantStats;
    float *margins;              /* optional (the margins build): rows x width x 2: the frame's smallest decision margin per pixel (the
                                    eps that flips a comparison), and its flip-free colour error per unit eps */
    int nextChunk;               /* atomic: next chunk of PTO_CHUNK_ROWS rows to hand out */
    Stats st[PTO_MAX_THREADS];   /* per participant (slot 0 = the calling thread) */
} FrameJob;

static void render_chunks(FrameJob *j, int slot)
{
    const Ctx *c = j->c;
    const int chunks = (j->rows + PTO_CHUNK_ROWS - 1) / PTO_CHUNK_ROWS;
    for (;;) {
        const int k = __atomic_fetch_add(&j->nextChunk, 1, __ATOMIC_RELAXED);
        if (k >= chunks) break;
        const int r1 = (k + 1) * PTO_CHUNK_ROWS < j->rows ? (k + 1) * PTO_CHUNK_ROWS : j->rows;
        for (int r = k * PTO_CHUNK_ROWS; r < r1; r++) {
            const int y = j->y0 + r;
            float *row = j->image + (size_t)r * c->width * 4;
            for (int x = 0; x < c->width; x++) {
                float out[4];
                MARGIN_PIXEL_BEGIN();
                shade_pixel(c, x, y, j->frame, row + 4 * x, out, j->wantStats ? &j->st[slot] : NULL);
                memcpy(row + 4 * x, out, 16);
                if (j->margins) MARGIN_PIXEL_READ(j->margins + 2 * ((size_t)r * c->width + x), c->spp);
            }
        }
    }
}

static struct {
    pthread_mutex_t mu;
    pthread_cond_t wake, done;
    pthread_t th[PTO_MAX_THREADS];
    int created;        /* workers that exist (worker w has slot w + 1) */
    unsigned long gen;  /* job generation: a worker runs each generation at most once */
    int wanted;         /* workers with slot <= wanted take part in the current generation */
    int running;        /* participants of the current generation that have not finished yet */
    FrameJob *job;
} g_pool = { PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, PTHREAD_COND_INITIALIZER, { 0 }, 0, 0, 0, 0, NULL };

static void *pool_worker(void *arg)
{
    const int slot = (int)(intptr_t)arg;
    unsigned long seen = 0;
    pthread_mutex_lock(&g_pool.mu);
    for (;;) {
        while (g_pool.gen == seen || slot > g_pool.wanted) {
            if (g_pool.gen != seen && slot > g_pool.wanted) seen = g_pool.gen; /* not invited to this one */
            pthread_cond_wait(&g_pool.wake, &g_pool.mu);
        }
        seen = g_pool.gen;
        FrameJob *j = g_pool.job;
        pthread_mutex_unlock(&g_pool.mu);
        render_chunks(j, slot);
        pthread_mutex_lock(&g_pool.mu);
        if (--g_pool.running == 0) pthread_cond_signal(&g_pool.done);
    }
    return NULL;
}

/* Render one frame into `image` (rows [y0, y0+rows) of the full image, tightly packed RGBA32F, row 0 = y0),
 * accumulating onto its current contents exactly like one PathTracer.Render() call (PathTracer.cs:114-123).
 * stats (optional, 6 x uint64): samples, bounces, sphereTests, cuboidTests, envLookups, reserved.
 * Not re-entrant (one frame at a time per process: the pool is shared); the callers are single-threaded test / bench code. */
static float *g_next_margins = NULL; /* handed to the next pto_render_frame by pto_render_frame_margins (single-threaded callers) */
PTO_API int pto_render_frame(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                             float *image, int y0, int rows, int frame, int nthreads, uint64_t *stats)
{
    static pthread_mutex_t serial = PTHREAD_MUTEX_INITIALIZER;
    Ctx c;
    make_ctx(&c, p, basic144, objects26624, env);
    if (nthreads < 1) nthreads = 1;
    if (nthreads > PTO_MAX_THREADS) nthreads = PTO_MAX_THREADS;
    const int chunks = (rows + PTO_CHUNK_ROWS - 1) / PTO_CHUNK_ROWS;
    if (nthreads > chunks) nthreads = chunks > 0 ? chunks : 1; /* more threads than chunks would idle */
    static FrameJob job; /* (16 KB of per-thread statistics: not on the stack) */
    pthread_mutex_lock(&serial);
    memset(&job, 0, sizeof job);
    job.c = &c; job.image = image; job.y0 = y0; job.rows = rows; job.frame = frame; job.wantStats = stats != NULL;
    job.margins = g_next_margins;
    g_next_margins = NULL;
    int helpers = nthreads - 1;
    pthread_mutex_lock(&g_pool.mu);
    while (g_pool.created < helpers) { /* grow the pool; a thread that cannot be created (EAGAIN) just means fewer helpers */
        if (pthread_create(&g_pool.th[g_pool.created], NULL, pool_worker, (void *)(intptr_t)(g_pool.created + 1)) != 0) break;
        pthread_detach(g_pool.th[g_pool.created]);
        g_pool.created++;
    }
    if (helpers > g_pool.created) helpers = g_pool.created;
    g_pool.job = &job;
    g_pool.wanted = helpers;
    g_pool.running = helpers;
    g_pool.gen++;
    if (helpers > 0) pthread_cond_broadcast(&g_pool.wake);
    pthread_mutex_unlock(&g_pool.mu);
    render_chunks(&job, 0); /* the calling thread takes chunks too (and all of them when it has no helpers) */
    pthread_mutex_lock(&g_pool.mu);
    while (g_pool.running > 0) pthread_cond_wait(&g_pool.done, &g_pool.mu);
    pthread_mutex_unlock(&g_pool.mu);
    if (stats) {
        memset(stats, 0, 6 * sizeof(uint64_t));
        for (int t = 0; t <= helpers; t++) {
            stats[0] += job.st[t].samples; stats[1] += job.st[t].bounces; stats[2] += job.st[t].sphereTests;
            stats[3] += job.st[t].cuboidTests; stats[4] += job.st[t].envLookups;
        }
    }
    pthread_mutex_unlock(&serial);
    return 0;
}

/* Evaluate `n` listed pixels of frame `frame` starting from `last` (n x 4 floats; pass zeros for frame 0).  margins (optional;
 * the margins build, oracle/study/pt_oracle_margins.c; other builds write +inf, 0): n x 2 floats, each pixel's (smallest decision margin, flip-free colour error per unit eps) of this frame. */
PTO_API int pto_render_pixels_margins(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                                      const int *xy, int n, int frame, const float *last, float *out, float *margins)
{
    Ctx c;
    make_ctx(&c, p, basic144, objects26624, env);
    for (int i = 0; i < n; i++) {
        MARGIN_PIXEL_BEGIN();
        shade_pixel(&c, xy[2 * i], xy[2 * i + 1], frame, last + 4 * i, out + 4 * i, NULL);
        if (margins) MARGIN_PIXEL_READ(margins + 2 * i, c.spp);
    }
    return 0;
}
PTO_API int pto_render_pixels(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                              const int *xy, int n, int frame, const float *last, float *out)
{
    return pto_render_pixels_margins(p, basic144, objects26624, env, xy, n, frame, last, out, NULL);
}

/* Per-pixel bounce counts of one frame (diagnostics for the divergence study in DESIGN.md): counts[y*W+x] = number
 * of RayTrace calls the pixel's samples made. */
PTO_API int pto_bounce_counts(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                              int frame, int *counts)
{
    Ctx c;
    make_ctx(&c, p, basic144, objects26624, env);
    float last[4] = { 0, 0, 0, 0 }, out[4];
    for (int y = 0; y < c.height; y++)
        for (int x = 0; x < c.width; x++) {
            Stats st = { 0, 0, 0, 0, 0, 0 };
            shade_pixel(&c, x, y, frame, last, out, &st);
            counts[(size_t)y * c.width + x] = (int)st.bounces;
        }
    return 0;
}

/* ---- micro entry points for unit tests ---- */
PTO_API uint32_t pto_pcg_hash(uint32_t *seed) { return pcg_hash(seed); }
PTO_API float pto_rand01(uint32_t *seed) { return rand01(seed); }
PTO_API uint32_t pto_pixel_seed(int x, int y, int frame)
{ return ((uint32_t)x * 1973u + (uint32_t)y * 9277u + (uint32_t)frame * 2699u) | 1u; }
PTO_API void pto_sincos(float a, float *s, float *c) { f_sincos(a, s, c); }
PTO_API float pto_exp(float x) { return f_exp(x); }
PTO_API int pto_ray_sphere(const float *o, const float *d, const float *pos_r, float *t12)
{ return ray_sphere(V(o[0], o[1], o[2]), V(d[0], d[1], d[2]), V(pos_r[0], pos_r[1], pos_r[2]), pos_r[3], t12, t12 + 1); }
PTO_API int pto_ray_cuboid(const float *o, const float *d, const float *mn, const float *mx, float *t12)
{
    v3 dd = V(d[0], d[1], d[2]);
    return ray_cuboid(V(o[0], o[1], o[2]), dd, V(f_rcp(dd.x), f_rcp(dd.y), f_rcp(dd.z)), V(mn[0], mn[1], mn[2]),
                      V(mx[0], mx[1], mx[2]), t12, t12 + 1);
}
PTO_API void pto_cuboid_normal(const float *mn, const float *mx, const float *p, float *n)
{ v3 r = cuboid_normal(V(mn[0], mn[1], mn[2]), V(mx[0], mx[1], mx[2]), V(p[0], p[1], p[2])); n[0] = r.x; n[1] = r.y; n[2] = r.z; }
PTO_API void pto_sample_env(const void *env, int size, int format, const float *dir, float *rgb_out)
{
    Ctx c;
    memset(&c, 0, sizeof c);
    c.env = env; c.envSize = size; c.envFormat = format;
    fill_lut(c.srgbLut);
    rgb o = sample_env(&c, V(dir[0], dir[1], dir[2]));
    rgb_out[0] = o.r; rgb_out[1] = o.g; rgb_out[2] = o.b;
}
/* n directions (3 floats each) -> n rgb triples: pto_sample_env over an array, the sRGB table built once */
PTO_API void pto_sample_env_n(const void *env, int size, int format, const float *dirs, int n, float *rgb_out)
{
    Ctx c;
    memset(&c, 0, sizeof c);
    c.env = env; c.envSize = size; c.envFormat = format;
    fill_lut(c.srgbLut);
    for (int i = 0; i < n; i++) {
        rgb o = sample_env(&c, V(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
        rgb_out[3 * i] = o.r; rgb_out[3 * i + 1] = o.g; rgb_out[3 * i + 2] = o.b;
    }
}
/* The seam rule alone: (face, x, y) of all 24*S off-face border taps of one size through the code env_texel_wrapped runs.
 * out[((face * 4 + edge) * S + p) * 3 + {0,1,2}]; edge 0: tap (-1, p), 1: (S, p), 2: (p, -1), 3: (p, S). */
PTO_API void pto_env_wrapped_index(int size, int *out)
{
    for (int face = 0; face < 6; face++)
        for (int edge = 0; edge < 4; edge++)
            for (int p = 0; p < size; p++) {
                int *o = out + (((size_t)face * 4 + edge) * size + p) * 3;
                env_wrapped_index(size, face, edge == 0 ? -1 : edge == 1 ? size : p, edge == 2 ? -1 : edge == 3 ? size : p, o, o + 1, o + 2);
            }
}
PTO_API float pto_srgb_to_linear(int v) { return srgb_to_linear(v); }
PTO_API float pto_pow5(float x) { return f_pow5(x); }
PTO_API float pto_fresnel_schlick(float cosTheta, float n1, float n2) { return fresnel_schlick(cosTheta, n1, n2); }
PTO_API void pto_refract(const float *i, const float *n, float eta, float *out)
{ v3 r = f_refract(V(i[0], i[1], i[2]), V(n[0], n[1], n[2]), eta); out[0] = r.x; out[1] = r.y; out[2] = r.z; }
PTO_API void pto_reflect(const float *i, const float *n, float *out)
{ v3 r = f_reflect(V(i[0], i[1], i[2]), V(n[0], n[1], n[2])); out[0] = r.x; out[1] = r.y; out[2] = r.z; }
PTO_API void pto_cosine_sample_hemisphere(const float *n, uint32_t *seed, float *out)
{ v3 r = cosine_sample_hemisphere(V(n[0], n[1], n[2]), seed); out[0] = r.x; out[1] = r.y; out[2] = r.z; }
PTO_API void pto_normalize(const float *v, float *out)
{ v3 r = v_normalize(V(v[0], v[1], v[2])); out[0] = r.x; out[1] = r.y; out[2] = r.z; }

/* ------------------------------------------------------------------ post-process ("next" row 1)
 * res/shaders/PostProcessing/fragment.glsl:17-44, run by src/Render/ScreenEffect.cs:29-37 into an RGBA8 target:
 *   color = texture(Sampler0, uv).rgb (+ an unbound sampler = 0); ACESFilm; LinearToInverseGamma(color, 2.4); alpha 1.
 * pt-f32 contract additions: log(x) = the cephes-style degree-9 polynomial below (~1 ulp), pow(x,y) = exp(y*log(x)),
 * a/b = a * f_rcp(b); float -> unorm8 = round-half-up of clamp(x,0,1)*255 (GL 4.5 section 2.3.5.1 leaves ties open). */
static float f_log(float x)
{
    uint32_t u = f_bits(x);
    int e = (int)(u >> 23) - 127;
    float m = f_unbits((u & 0x007fffffu) | 0x3f800000u); /* [1,2) */
    if (m > 1.41421356237f) { m *= 0.5f; e += 1; }
    float t = m - 1.0f, z = t * t;
    float y = c_fma(7.0376836292e-2f, t, -1.1514610310e-1f);
    y = c_fma(y, t, 1.1676998740e-1f);
    y = c_fma(y, t, -1.2420140846e-1f);
    y = c_fma(y, t, 1.4249322787e-1f);
    y = c_fma(y, t, -1.6668057665e-1f);
    y = c_fma(y, t, 2.0000714765e-1f);
    y = c_fma(y, t, -2.4999993993e-1f);
    y = c_fma(y, t, 3.3333331174e-1f);
    y = y * t * z;
    float fe = (float)e;
    y = c_fma(-2.12194440e-4f, fe, y);
    y = c_fma(-0.5f, z, y);
    return c_fma(0.693359375f, fe, t + y);
}

static inline float f_clamp01(float x) { return f_min(f_max(x, 0.0f), 1.0f); }

static float aces_film(float x) /* fragment.glsl:35-43 */
{
    const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
    float num = x * c_fma(a, x, b), den = c_fma(x, c_fma(c, x, d), e);
    return f_clamp01(num * f_rcp(den));
}

static float linear_to_inverse_gamma(float v, float gamma) /* fragment.glsl:28-32 */
{
    if (v < 0.0031308f) return v * 12.92f;
    return c_fma(f_exp(f_rcp(gamma) * f_log(v)), 1.055f, -0.055f);
}

static inline uint8_t to_unorm8(float v)
{
    float c = f_clamp01(v) * 255.0f + 0.5f;
    return (uint8_t)(int)c;
}

/* out_f (optional): the shader's float colour per pixel (n x 3); out_u8 (optional): the RGBA8 target (n x 4) */
PTO_API int pto_postprocess(const float *rgba, int n, float *out_f, uint8_t *out_u8)
{
    for (int i = 0; i < n; i++) {
        float c[3];
        for (int k = 0; k < 3; k++) c[k] = linear_to_inverse_gamma(aces_film(rgba[4 * i + k]), 2.4f);
        if (out_f) { out_f[3 * i] = c[0]; out_f[3 * i + 1] = c[1]; out_f[3 * i + 2] = c[2]; }
        if (out_u8) {
            out_u8[4 * i] = to_unorm8(c[0]); out_u8[4 * i + 1] = to_unorm8(c[1]); out_u8[4 * i + 2] = to_unorm8(c[2]);
            out_u8[4 * i + 3] = 255;
        }
    }
    return 0;
}
PTO_API float pto_log(float x) { return f_log(x); }
/* the contract's software reciprocal / inverse square root / square root, array form (accuracy property tests) */
PTO_API void pto_rcp_array(const float *x, float *y, int n) { for (int i = 0; i < n; i++) y[i] = f_rcp(x[i]); }
PTO_API void pto_rsqrt_array(const float *x, float *y, int n) { for (int i = 0; i < n; i++) y[i] = f_rsqrt(x[i]); }
PTO_API void pto_sqrt_array(const float *x, float *y, int n) { for (int i = 0; i < n; i++) y[i] = pt_sqrt(x[i]); }
/* array forms of the other primitives and leaf functions (tests/test_math_probe_cpu.py, tests/test_gpu_math_probe.py): every row goes
 * through memory as it is, so a signalling NaN reaches the function unquieted, which an argument passed as a double would not */
PTO_API void pto_mix_array(const float *x, const float *y, const float *a, float *out, int n) { for (int i = 0; i < n; i++) out[i] = f_mix(x[i], y[i], a[i]); }
PTO_API void pto_sincos_array(const float *a, float *s, float *c, int n) { for (int i = 0; i < n; i++) f_sincos(a[i], s + i, c + i); }
PTO_API void pto_exp_array(const float *x, float *y, int n) { for (int i = 0; i < n; i++) y[i] = f_exp(x[i]); }
PTO_API void pto_log_array(const float *x, float *y, int n) { for (int i = 0; i < n; i++) y[i] = f_log(x[i]); }
PTO_API void pto_pow5_array(const float *x, float *y, int n) { for (int i = 0; i < n; i++) y[i] = f_pow5(x[i]); }
PTO_API void pto_aces_film_array(const float *x, float *y, int n) { for (int i = 0; i < n; i++) y[i] = aces_film(x[i]); }
PTO_API void pto_linear_to_inverse_gamma_array(const float *v, float gamma, float *y, int n) { for (int i = 0; i < n; i++) y[i] = linear_to_inverse_gamma(v[i], gamma); }
PTO_API void pto_to_unorm8_array(const float *v, uint8_t *y, int n) { for (int i = 0; i < n; i++) y[i] = to_unorm8(v[i]); }
PTO_API void pto_pcg_hash_array(const uint32_t *seed, uint32_t *word, uint32_t *seed_out, int n)
{ for (int i = 0; i < n; i++) { uint32_t s = seed[i]; word[i] = pcg_hash(&s); seed_out[i] = s; } }
PTO_API void pto_rand01_array(const uint32_t *seed, float *value, uint32_t *seed_out, int n)
{ for (int i = 0; i < n; i++) { uint32_t s = seed[i]; value[i] = rand01(&s); seed_out[i] = s; } }
PTO_API void pto_pixel_seed_array(const int *xyf, uint32_t *seed, int n) { for (int i = 0; i < n; i++) seed[i] = pto_pixel_seed(xyf[3 * i], xyf[3 * i + 1], xyf[3 * i + 2]); }
#define ROW3(p_, i_) V((p_)[3 * (i_)], (p_)[3 * (i_) + 1], (p_)[3 * (i_) + 2])
#define PUT3(p_, i_, v_) do { v3 r_ = (v_); (p_)[3 * (i_)] = r_.x; (p_)[3 * (i_) + 1] = r_.y; (p_)[3 * (i_) + 2] = r_.z; } while (0)
PTO_API void pto_normalize_array(const float *v, float *out, int n) { for (int i = 0; i < n; i++) PUT3(out, i, v_normalize(ROW3(v, i))); }
PTO_API void pto_reflect_array(const float *in, const float *nr, float *out, int n) { for (int i = 0; i < n; i++) PUT3(out, i, f_reflect(ROW3(in, i), ROW3(nr, i))); }
PTO_API void pto_refract_array(const float *in, const float *nr, const float *eta, float *out, int n)
{ for (int i = 0; i < n; i++) PUT3(out, i, f_refract(ROW3(in, i), ROW3(nr, i), eta[i])); }
PTO_API void pto_fresnel_schlick_array(const float *cosTheta, const float *n1, const float *n2, float *out, int n)
{ for (int i = 0; i < n; i++) out[i] = fresnel_schlick(cosTheta[i], n1[i], n2[i]); }
PTO_API void pto_cosine_sample_hemisphere_array(const float *nr, const uint32_t *seed, float *out, uint32_t *seed_out, int n)
{ for (int i = 0; i < n; i++) { uint32_t s = seed[i]; PUT3(out, i, cosine_sample_hemisphere(ROW3(nr, i), &s)); seed_out[i] = s; } }
PTO_API void pto_cuboid_normal_array(const float *mn, const float *mx, const float *p, float *out, int n)
{ for (int i = 0; i < n; i++) PUT3(out, i, cuboid_normal(ROW3(mn, i), ROW3(mx, i), ROW3(p, i))); }
#undef ROW3
#undef PUT3

/* ------------------------------------------------------------------ atmosphere precompute
 * res/shaders/AtmosphericScattering/compute.glsl:30-171 (algorithm credited there to
 * github.com/wwwtyro/glsl-atmosphere).  Same pt-f32 contract. */
static void atmo_rsi(v3 r0, v3 rd, float sr, float *x, float *y) /* :58-71 */
{
    float a = v_dot(rd, rd);
    float b = 2.0f * v_dot(rd, r0);
    float c = c_fma(-sr, sr, v_dot(r0, r0));
    float d = c_fma(b, b, -(4.0f * a * c));
    if (d < 0.0f) { *x = 1e5f; *y = -1e5f; return; }
    /* (round 5: the per-step roots use the contract's pt_sqrt and ONE pt-f32 reciprocal instead of sqrtf and two IEEE divisions —
       the correctly rounded forms are 52 / 43 issue cycles each on gfx950, and this function runs 53 times per texel) */
    float sq = pt_sqrt(d), rden = f_rcp(2.0f * a);
    *x = (-b - sq) * rden;
    *y = (-b + sq) * rden;
}

static v3 atmosphere(v3 r, v3 r0, v3 pSun, float iSun, float rPlanet, float rAtmos, v3 kRlh, float kMie,
                     float shRlh, float shMie, float g, int iSteps, int jSteps) /* :73-159 */
{
    pSun = v_normalize(pSun);
    r = v_normalize(r);
    float px, py, qx, qy;
    atmo_rsi(r0, r, rAtmos, &px, &py);
    if (px > py) return V(0.0f, 0.0f, 0.0f);
    atmo_rsi(r0, r, rPlanet, &qx, &qy);
    py = f_min(py, qx);
    float iStepSize = (py - px) / (float)iSteps;
    float iTime = 0.0f;
    v3 totalRlh = V(0, 0, 0), totalMie = V(0, 0, 0);
    float iOdRlh = 0.0f, iOdMie = 0.0f;
    float mu = v_dot(r, pSun), mumu = mu * mu, gg = g * g;
    float pRlh = 3.0f / (16.0f * PI) * (1.0f + mumu);
    float base = 1.0f + gg - 2.0f * mu * g;
    float pMie = 3.0f / (8.0f * PI) * ((1.0f - gg) * (mumu + 1.0f)) / ((base * sqrtf(base)) * (2.0f + gg));
    float invShRlh = -1.0f / shRlh, invShMie = -1.0f / shMie; /* exp(-h/sh) evaluated as exp(h * (-1/sh)) */
    const float invJSteps = 1.0f / (float)jSteps;               /* uniform IEEE reciprocal: sy / jSteps is evaluated as sy * (1 / jSteps) */
    for (int i = 0; i < iSteps; i++) {
        v3 iPos = v_fma(r, c_fma(iStepSize, 0.5f, iTime), r0);
        float iHeight = pt_sqrt(v_dot(iPos, iPos)) - rPlanet;
        float odStepRlh = f_exp(iHeight * invShRlh) * iStepSize;
        float odStepMie = f_exp(iHeight * invShMie) * iStepSize;
        iOdRlh += odStepRlh;
        iOdMie += odStepMie;
        float sx, sy;
        atmo_rsi(iPos, pSun, rAtmos, &sx, &sy);
        float jStepSize = sy * invJSteps;
        float jTime = 0.0f, jOdRlh = 0.0f, jOdMie = 0.0f;
        for (int j = 0; j < jSteps; j++) {
            v3 jPos = v_fma(pSun, c_fma(jStepSize, 0.5f, jTime), iPos);
            float jHeight = pt_sqrt(v_dot(jPos, jPos)) - rPlanet;
            jOdRlh = c_fma(f_exp(jHeight * invShRlh), jStepSize, jOdRlh);
            jOdMie = c_fma(f_exp(jHeight * invShMie), jStepSize, jOdMie);
            jTime += jStepSize;
        }
        float mieTerm = kMie * (iOdMie + jOdMie), rl = iOdRlh + jOdRlh;
        v3 attn = V(f_exp(-c_fma(kRlh.x, rl, mieTerm)), f_exp(-c_fma(kRlh.y, rl, mieTerm)), f_exp(-c_fma(kRlh.z, rl, mieTerm)));
        totalRlh = v_fma(attn, odStepRlh, totalRlh);
        totalMie = v_fma(attn, odStepMie, totalMie);
        iTime += iStepSize;
    }
    float pm = pMie * kMie;
    return V(iSun * c_fma(pRlh * kRlh.x, totalRlh.x, pm * totalMie.x),
             iSun * c_fma(pRlh * kRlh.y, totalRlh.y, pm * totalMie.y),
             iSun * c_fma(pRlh * kRlh.z, totalRlh.z, pm * totalMie.z));
}

typedef struct { const float *ubo; const float *lightPos; float intensity; int size, iSteps, jSteps; float *out; int tid, nthreads; } AtmoJob;

static void *atmo_worker(void *arg)
{
    AtmoJob *j = (AtmoJob *)arg;
    int S = j->size;
    for (int idx = j->tid; idx < 6 * S; idx += j->nthreads) {
        int face = idx / S, y = idx % S;
        const float *invView = j->ubo + 16 + 16 * face;
        for (int x = 0; x < S; x++) {
            /* main :30-56 : ndc = vec2(imgCoord.xy) / size * 2 - 1 (texel corner, no +0.5) */
            float ndcx = c_fma((float)x / (float)S, 2.0f, -1.0f), ndcy = c_fma((float)y / (float)S, 2.0f, -1.0f);
            float eye[4], wd[4];
            mat_vec(j->ubo, ndcx, ndcy, -1.0f, 0.0f, eye);
            mat_vec(invView, eye[0], eye[1], -1.0f, 0.0f, wd);
            v3 dir = v_normalize(V(wd[0], wd[1], wd[2]));
            v3 col = atmosphere(dir, V(0.0f, 6376e3f, 0.0f), V(j->lightPos[0], j->lightPos[1], j->lightPos[2]), j->intensity,
                                6371e3f, 6471e3f, V(5.5e-6f, 13.0e-6f, 22.4e-6f), 21e-6f, 8e3f, 1.2e3f, 0.758f,
                                j->iSteps, j->jSteps);
            float *o = j->out + (((size_t)face * S + y) * S + x) * 4;
            o[0] = col.x; o[1] = col.y; o[2] = col.z; o[3] = 1.0f;
        }
    }
    return NULL;
}

/* out: float[6][size][size][4]; ubo464: InvProjection + 6 InvView (AtmosphericScatterer.cs:72-89) */
PTO_API int pto_atmosphere(const float *ubo464, const float *lightPos, float lightIntensity, int size, int iSteps,
                           int jSteps, float *out, int nthreads)
{
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 256) nthreads = 256;
    pthread_t th[256];
    AtmoJob jobs[256];
    for (int t = 0; t < nthreads; t++) {
        AtmoJob j = { ubo464, lightPos, lightIntensity, size, iSteps, jSteps, out, t, nthreads };
        jobs[t] = j;
        if (nthreads > 1) pthread_create(&th[t], NULL, atmo_worker, &jobs[t]);
    }
    if (nthreads == 1) atmo_worker(&jobs[0]);
    else for (int t = 0; t < nthreads; t++) pthread_join(th[t], NULL);
    return 0;
}

/* ------------------------------------------------------------------ study entry points this build does not implement
 * Every library exports the full pto_* set (oracle/pt_oracle.py binds all of it on each); what no unit of the build implements
 * returns -1.  The implementations and their documentation: oracle/study/pt_oracle_witness.c, oracle/study/pt_oracle_margins.c. */
#ifndef PTO_HAVE_WITNESS_ENTRY_POINTS
PTO_API int pto_set_perturbation(int prim, int ulps) { (void)prim; (void)ulps; return -1; }
PTO_API int pto_set_unfused(int on) { (void)on; return -1; }
PTO_API int pto_set_base_variant(int bits) { (void)bits; return -1; }
PTO_API int pto_llvmpipe_like(int which, const float *x, const float *y, int n, float *out) { (void)which; (void)x; (void)y; (void)n; (void)out; return -1; }
PTO_API int pto_set_signature_alpha(int on) { (void)on; return -1; }
PTO_API int pto_set_ensemble(unsigned seed, int amplitude) { (void)seed; (void)amplitude; return -1; }
PTO_API int pto_set_nan_env(const float *rgb3) { (void)rgb3; return -1; }
PTO_API int pto_list_close_decisions(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                                     int x, int y, int frame, const float *last4, float closeGap, int cap, float *out4)
{
    (void)p; (void)basic144; (void)objects26624; (void)env; (void)x; (void)y; (void)frame; (void)last4; (void)closeGap; (void)cap; (void)out4;
    return -1;
}
PTO_API int pto_render_pixel_variant(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                                     int x, int y, int frame, const float *last4, const int *flips3, int nsites, const int *sites, int powNegNan,
                                     float *out4)
{
    (void)p; (void)basic144; (void)objects26624; (void)env; (void)x; (void)y; (void)frame; (void)last4; (void)flips3; (void)nsites; (void)sites; (void)powNegNan; (void)out4;
    return -1;
}
PTO_API int pto_witness_search(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                               int x, int y, int frame, const float *last4, const float *ref3, double band,
                               float closeGap, int maxFlips, int *flips3, int *sites, int *nsites, int *stats4, float *out4)
{
    (void)p; (void)basic144; (void)objects26624; (void)env; (void)x; (void)y; (void)frame; (void)last4; (void)ref3; (void)band;
    (void)closeGap; (void)maxFlips; (void)flips3; (void)sites; (void)nsites; (void)stats4; (void)out4;
    return -1;
}
#endif
#ifndef PTO_HAVE_MARGINS_ENTRY_POINTS
PTO_API int pto_render_frame_margins(const PtoParams *p, const float *basic144, const float *objects26624, const void *env,
                                     float *image, int y0, int rows, int frame, int nthreads, float *margins)
{
    (void)p; (void)basic144; (void)objects26624; (void)env; (void)image; (void)y0; (void)rows; (void)frame; (void)nthreads; (void)margins;
    return -1;
}
#endif
