// pt_device_probe.hip — TEST AID, never linked into the product: runs the "pt-f32" primitives of csrc/pt_math.hpp and the leaf functions
// of csrc/pt_device.hpp one call per lane, on words handed in by the caller (pt_probe_eval), or on words generated on the device from the
// word index (pt_probe_sweep: exhaustive sweeps whose reference is computed on the device too).  The functions are INCLUDED from the
// product's headers, never restated, and the library is built with the product's own flags (native.build_probe), so what runs here is
// the code object hipcc produces for those sequences: denormal mode, conversions, min / max, the division and square-root expansions.
//
// With -DPT_PROBE_HOST (hipcc --cuda-host-only, tests/test_math_probe_cpu.py) the same rows and sweeps run in a plain loop on the CPU:
// both headers compile for the host once PT_DEV is __host__ __device__ (what they hold of wave intrinsics and inline assembly sits in
// inline functions no row calls, which the host pass never emits).
//
// Both entry points take HOST pointers, allocate, copy and synchronise on their own, check every HIP call and return the first
// error code (0 = hipSuccess).  The kernels are element-wise and bounds-checked: no LDS, no waiting between lanes or workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef PT_PROBE_HOST
// host overloads of the two bit casts the header uses (HIP declares them for the device only)
__host__ static inline float __uint_as_float(unsigned int x) { float f; __builtin_memcpy(&f, &x, 4); return f; }
__host__ static inline unsigned int __float_as_uint(float x) { unsigned int u; __builtin_memcpy(&u, &x, 4); return u; }
#define PT_DEV __host__ __device__ inline
#define PROBE_FN __host__ __device__ inline
#else
#define PROBE_FN __device__ inline
#endif
#include "pt_device.hpp"

using namespace pt;

#define PT_PROBE_API extern "C" __attribute__((visibility("default")))
#define PT_PROBE_E_BAD_ARGUMENT (-2)

// which (pt_probe_eval): words in -> words out per row.  tests/math_probe_cases.py holds the same table.
enum {
    F_RCP = 0,       // x -> f_rcp
    F_RSQRT,         // x -> f_rsqrt
    F_PT_SQRT,       // x -> pt_sqrt
    F_SQRT,          // x -> f_sqrt
    F_DIV_IEEE,      // a, b -> f_div_ieee
    F_MIN,           // a, b -> f_min
    F_MAX,           // a, b -> f_max
    F_MIX,           // x, y, a -> f_mix
    F_SINCOS,        // a -> sin, cos
    F_EXP,           // x -> pt_exp<false>
    F_EXP_SELECTED,  // x -> pt_exp<true>
    F_LOG,           // x -> pt_log
    F_POW5,          // x -> pt_pow5
    F_ACES,          // x -> aces_film
    F_INV_GAMMA,     // v -> linear_to_inverse_gamma(v, 2.4f)
    F_UNORM8,        // v -> to_unorm8 (the byte, as a word)
    F_PCG_HASH,      // seed -> word, new seed
    F_RAND01,        // seed -> float, new seed
    F_PIXEL_SEED,    // x, y, frame -> seed                                    (csrc/pt_device.hpp: this row and F_REFLECT .. F_CUBOID_NORMAL)
    F_NORMALIZE,     // v[3] -> v_normalize
    F_REFLECT,       // i[3], n[3] -> f_reflect
    F_REFRACT,       // i[3], n[3], eta -> f_refract
    F_FRESNEL,       // cosTheta, n1, n2 -> fresnel_schlick
    F_HEMI_DIR,      // n[3], z, a -> hemisphere_direction
    F_COS_HEMI,      // n[3], seed -> direction[3], new seed
    F_CUBOID_NORMAL, // mn[3], mx[3], p[3] -> cuboid_normal
    F_REF_RCP,       // x -> the sweeps' double-precision reference 1.0 / (double)x, low word, high word
    F_REF_RSQRT,     // x -> 1.0 / sqrt((double)x)
    F_REF_SQRT,      // x -> sqrt((double)x)
    F_COUNT
};
static const unsigned char kInCols[F_COUNT] = {1, 1, 1, 1, 2, 2, 2, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3, 3, 6, 7, 3, 5, 4, 9, 1, 1, 1};
static const unsigned char kOutCols[F_COUNT] = {1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1, 2, 2, 1, 3, 3, 3, 1, 3, 4, 3, 2, 2, 2};

// which (pt_probe_sweep)
enum {
    S_EXP_SELECTED = 0, // word w: pt_exp<true>(w) against pt_exp<false>(w), words equal or both NaN
    S_RAND01,           // seed w: rand01 against the round-to-nearest-even conversion of pcg_hash's word in integer arithmetic, times 2^-32
    S_RCP,              // word w: |f_rcp(w) - 1.0 / (double)w| in float ulps; a row counts as a mismatch above 0.52 ulp
    S_RSQRT,            //         f_rsqrt against 1.0 / sqrt((double)w), 1.75 ulp
    S_PT_SQRT,          //         pt_sqrt against sqrt((double)w), 0.502 ulp
    S_CUBOID_SCALE,     // index w < 64: cuboid_normal's selected scale against v_scale(n, f_rsqrt(v_dot(n, n))), words equal or both NaN
    S_COUNT
};
// out (pt_probe_sweep), 24 words: [0..1] mismatches (64 bit), [2..3] largest error in ulps (the bits of a double), [4] the word it was
// measured at, [5] offending words recorded (at most 16), [6..21] those words (in the order the lanes got to them), [22..23] unused
#define SWEEP_OUT_WORDS 24

PROBE_FN float as_f(uint32_t u) { return __uint_as_float(u); }
PROBE_FN uint32_t as_u(float f) { return __float_as_uint(f); }
PROBE_FN void put_double(double d, uint32_t *o)
{
    unsigned long long u;
    __builtin_memcpy(&u, &d, 8);
    o[0] = (uint32_t)u;
    o[1] = (uint32_t)(u >> 32);
}
// the double-precision references of the accuracy sweeps (IEEE binary64 divide and square root; checked against numpy through F_REF_*)
PROBE_FN double ref_rcp(float x) { return 1.0 / (double)x; }
PROBE_FN double ref_rsqrt(float x) { return 1.0 / __builtin_sqrt((double)x); }
PROBE_FN double ref_sqrt(float x) { return __builtin_sqrt((double)x); }

// One row.  Returns false for an unknown `which`.
PROBE_FN bool eval_row(int which, const uint32_t *r, uint32_t *o)
{
    switch (which) {
    case F_RCP: o[0] = as_u(f_rcp(as_f(r[0]))); return true;
    case F_RSQRT: o[0] = as_u(f_rsqrt(as_f(r[0]))); return true;
    case F_PT_SQRT: o[0] = as_u(pt_sqrt(as_f(r[0]))); return true;
    case F_SQRT: o[0] = as_u(f_sqrt(as_f(r[0]))); return true;
    case F_DIV_IEEE: o[0] = as_u(f_div_ieee(as_f(r[0]), as_f(r[1]))); return true;
    case F_MIN: o[0] = as_u(f_min(as_f(r[0]), as_f(r[1]))); return true;
    case F_MAX: o[0] = as_u(f_max(as_f(r[0]), as_f(r[1]))); return true;
    case F_MIX: o[0] = as_u(f_mix(as_f(r[0]), as_f(r[1]), as_f(r[2]))); return true;
    case F_SINCOS: {
        float s, c;
        pt_sincos(as_f(r[0]), s, c);
        o[0] = as_u(s); o[1] = as_u(c);
        return true;
    }
    case F_EXP: o[0] = as_u(pt_exp<false>(as_f(r[0]))); return true;
    case F_EXP_SELECTED: o[0] = as_u(pt_exp<true>(as_f(r[0]))); return true;
    case F_LOG: o[0] = as_u(pt_log(as_f(r[0]))); return true;
    case F_POW5: o[0] = as_u(pt_pow5(as_f(r[0]))); return true;
    case F_ACES: o[0] = as_u(aces_film(as_f(r[0]))); return true;
    case F_INV_GAMMA: o[0] = as_u(linear_to_inverse_gamma(as_f(r[0]), 2.4f)); return true;
    case F_UNORM8: o[0] = (uint32_t)to_unorm8(as_f(r[0])); return true;
    case F_PCG_HASH: {
        uint32_t seed = r[0];
        o[0] = pcg_hash(seed); o[1] = seed;
        return true;
    }
    case F_RAND01: {
        uint32_t seed = r[0];
        o[0] = as_u(rand01(seed)); o[1] = seed;
        return true;
    }
    case F_REF_RCP: put_double(ref_rcp(as_f(r[0])), o); return true;
    case F_REF_RSQRT: put_double(ref_rsqrt(as_f(r[0])), o); return true;
    case F_REF_SQRT: put_double(ref_sqrt(as_f(r[0])), o); return true;
    case F_NORMALIZE: {
        v3 v = v_normalize(V(as_f(r[0]), as_f(r[1]), as_f(r[2])));
        o[0] = as_u(v.x); o[1] = as_u(v.y); o[2] = as_u(v.z);
        return true;
    }
    case F_PIXEL_SEED: o[0] = pixel_seed((int)r[0], (int)r[1], (int)r[2]); return true;
    case F_REFLECT: {
        v3 v = f_reflect(V(as_f(r[0]), as_f(r[1]), as_f(r[2])), V(as_f(r[3]), as_f(r[4]), as_f(r[5])));
        o[0] = as_u(v.x); o[1] = as_u(v.y); o[2] = as_u(v.z);
        return true;
    }
    case F_REFRACT: {
        v3 v = f_refract(V(as_f(r[0]), as_f(r[1]), as_f(r[2])), V(as_f(r[3]), as_f(r[4]), as_f(r[5])), as_f(r[6]));
        o[0] = as_u(v.x); o[1] = as_u(v.y); o[2] = as_u(v.z);
        return true;
    }
    case F_FRESNEL: o[0] = as_u(fresnel_schlick(as_f(r[0]), as_f(r[1]), as_f(r[2]))); return true;
    case F_HEMI_DIR: {
        v3 v = hemisphere_direction(V(as_f(r[0]), as_f(r[1]), as_f(r[2])), as_f(r[3]), as_f(r[4]));
        o[0] = as_u(v.x); o[1] = as_u(v.y); o[2] = as_u(v.z);
        return true;
    }
    case F_COS_HEMI: {
        uint32_t seed = r[3];
        v3 v = cosine_sample_hemisphere(V(as_f(r[0]), as_f(r[1]), as_f(r[2])), seed);
        o[0] = as_u(v.x); o[1] = as_u(v.y); o[2] = as_u(v.z); o[3] = seed;
        return true;
    }
    case F_CUBOID_NORMAL: {
        v3 v = cuboid_normal(V(as_f(r[0]), as_f(r[1]), as_f(r[2])), V(as_f(r[3]), as_f(r[4]), as_f(r[5])), V(as_f(r[6]), as_f(r[7]), as_f(r[8])));
        o[0] = as_u(v.x); o[1] = as_u(v.y); o[2] = as_u(v.z);
        return true;
    }
    default: return false;
    }
}

// ---------------------------------------------------------------------------------------------- sweeps
PROBE_FN bool same_word(float a, float b) { return as_u(a) == as_u(b) || (a != a && b != b); } // the project's comparison rule

// uint32 -> binary32, round to nearest even, times 2^-32, in integer arithmetic: the bits of the float
PROBE_FN uint32_t rne_unit_bits(uint32_t w)
{
    if (w == 0u) return 0u;
    int top = 31 - __builtin_clz(w); // position of the leading one
    uint32_t mant;                   // 24 bits, leading one included
    if (top <= 23) {
        mant = w << (23 - top);
    } else {
        const int drop = top - 23;
        const uint32_t rest = w & ((1u << drop) - 1u), half = 1u << (drop - 1);
        mant = w >> drop;
        if (rest > half || (rest == half && (mant & 1u))) mant++;
        if (mant == (1u << 24)) { mant >>= 1; top++; }
    }
    return ((uint32_t)(top - 32 + 127) << 23) | (mant & 0x007FFFFFu); // value mant * 2^(top - 23 - 32): always a normal number
}

// error of `got` against `exact` in units of the float ulp at `exact` (tests/test_oracle_properties.py, _ulp_error): the spacing of
// binary32 at |(float)exact|.  The sweeps stay inside [1e-30, 1e30], where every value involved is a normal number.
PROBE_FN double ulp_error(float got, double exact)
{
    const float e32 = (float)exact;
    const uint32_t eb = as_u(e32) & 0x7F800000u;
    const double ulp = (double)as_f(eb) * 1.1920928955078125e-07; // 2^(exponent - 23)
    return __builtin_fabs((double)got - exact) / ulp;
}

// cuboid_normal's input for combination `idx` (two bits per axis: 0 = on the lower face, 1 = on the upper face, 2 = inside towards
// the lower face, 3 = inside towards the upper face) of the box [-1, 1]^3, and the normal component it stands for
PROBE_FN float combo_point(int s) { return s == 0 ? -1.0f : (s == 1 ? 1.0f : (s == 2 ? -0.5f : 0.5f)); }
PROBE_FN float combo_component(int s) { return s == 0 ? -1.0f : (s == 1 ? 1.0f : (s == 2 ? -0.0f : 0.0f)); }

// One word of a sweep: false = mismatch; err = the error measured (accuracy sweeps; 0 elsewhere).
PROBE_FN bool sweep_word(int which, uint32_t w, double &err)
{
    err = 0.0;
    switch (which) {
    case S_EXP_SELECTED: return same_word(pt_exp<true>(as_f(w)), pt_exp<false>(as_f(w)));
    case S_RAND01: {
        uint32_t s0 = w, s1 = w;
        const float got = rand01(s0);
        return as_u(got) == rne_unit_bits(pcg_hash(s1)) && s0 == s1;
    }
    case S_RCP: err = ulp_error(f_rcp(as_f(w)), ref_rcp(as_f(w))); return err <= 0.52;
    case S_RSQRT: err = ulp_error(f_rsqrt(as_f(w)), ref_rsqrt(as_f(w))); return err <= 1.75;
    case S_PT_SQRT: err = ulp_error(pt_sqrt(as_f(w)), ref_sqrt(as_f(w))); return err <= 0.502;
    case S_CUBOID_SCALE: {
        const int sx = w & 3, sy = (w >> 2) & 3, sz = (w >> 4) & 3;
        const v3 got = cuboid_normal(V(-1.0f, -1.0f, -1.0f), V(1.0f, 1.0f, 1.0f), V(combo_point(sx), combo_point(sy), combo_point(sz)));
        const v3 n = V(combo_component(sx), combo_component(sy), combo_component(sz));
        const v3 want = v_scale(n, f_rsqrt(v_dot(n, n)));
        return same_word(got.x, want.x) && same_word(got.y, want.y) && same_word(got.z, want.z);
    }
    default: return false;
    }
}

#ifndef PT_PROBE_HOST
__global__ __launch_bounds__(256) void probe_eval_kernel(int which, const uint32_t *in, unsigned long long n, int in_cols, uint32_t *out, int out_cols)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += stride)
        eval_row(which, in + i * (unsigned long long)in_cols, out + i * (unsigned long long)out_cols);
}

// Every lane walks its words, keeps its own tally, and adds it to the result once at the end (ordinary vector atomics).
__global__ __launch_bounds__(256) void probe_sweep_kernel(int which, uint32_t first, unsigned long long count, uint32_t *out)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    unsigned long long bad = 0ull;
    double worst = -1.0;
    uint32_t worstWord = 0u;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < count; i += stride) {
        const uint32_t w = first + (uint32_t)i;
        double err;
        if (!sweep_word(which, w, err)) {
            if (bad < 2ull) { // (a lane reports its first two words: nothing to gain from more, and no lane hammers the counter)
                const uint32_t slot = atomicAdd(out + 5, 1u);
                if (slot < 16u) out[6 + slot] = w;
            }
            bad++;
        }
        if (err > worst) { worst = err; worstWord = w; }
    }
    if (bad != 0ull) atomicAdd((unsigned long long *)out, bad);
    if (worst > 0.0) {
        // the largest error and a word it was measured at, in one 64-bit maximum: the error in units of 2^-24 ulp above the word
        // (non-negative doubles order like their bits; the exact double goes to out[2..3] the same way)
        unsigned long long wb;
        __builtin_memcpy(&wb, &worst, 8);
        atomicMax((unsigned long long *)(out + 2), wb);
        const double q = worst * 16777216.0;
        const unsigned long long key = ((unsigned long long)(q >= 4294967295.0 ? 4294967295u : (uint32_t)q) << 32) | worstWord;
        atomicMax((unsigned long long *)(out + 22), key);
    }
}
#endif

static bool eval_args_ok(int which, unsigned long long n, int in_cols, int out_cols, const void *in, const void *out)
{
    return which >= 0 && which < F_COUNT && in_cols == kInCols[which] && out_cols == kOutCols[which] && n <= (1ull << 26) &&
           (n == 0 || (in != nullptr && out != nullptr));
}

#define PROBE_HIP(call)                  \
    do {                                 \
        hipError_t e_ = (call);          \
        if (e_ != hipSuccess && rc == 0) rc = (int)e_; \
    } while (0)

PT_PROBE_API int pt_probe_eval(int which, const uint32_t *in_words, unsigned long long n, int in_cols, uint32_t *out_words, int out_cols)
{
    if (!eval_args_ok(which, n, in_cols, out_cols, in_words, out_words)) return PT_PROBE_E_BAD_ARGUMENT;
    if (n == 0) return 0;
#ifdef PT_PROBE_HOST
    for (unsigned long long i = 0; i < n; i++)
        if (!eval_row(which, in_words + i * in_cols, out_words + i * out_cols)) return PT_PROBE_E_BAD_ARGUMENT;
    return 0;
#else
    int rc = 0;
    uint32_t *din = nullptr, *dout = nullptr;
    const size_t inBytes = (size_t)n * in_cols * 4, outBytes = (size_t)n * out_cols * 4;
    PROBE_HIP(hipMalloc((void **)&din, inBytes));
    if (rc == 0) PROBE_HIP(hipMalloc((void **)&dout, outBytes));
    if (rc == 0) PROBE_HIP(hipMemcpy(din, in_words, inBytes, hipMemcpyHostToDevice));
    if (rc == 0) PROBE_HIP(hipMemset(dout, 0, outBytes));
    if (rc == 0) {
        const unsigned long long blocks = (n + 255ull) / 256ull;
        probe_eval_kernel<<<dim3((unsigned)(blocks < 16384ull ? blocks : 16384ull)), dim3(256)>>>(which, din, n, in_cols, dout, out_cols);
        PROBE_HIP(hipGetLastError());
    }
    if (rc == 0) PROBE_HIP(hipDeviceSynchronize());
    if (rc == 0) PROBE_HIP(hipMemcpy(out_words, dout, outBytes, hipMemcpyDeviceToHost));
    if (din) PROBE_HIP(hipFree(din));
    if (dout) PROBE_HIP(hipFree(dout));
    return rc;
#endif
}

// Words first, first + 1, ..., first + count - 1 (modulo 2^32; count <= 2^32).  out: SWEEP_OUT_WORDS words, see above.
PT_PROBE_API int pt_probe_sweep(int which, uint32_t first_word, unsigned long long count, uint32_t *out)
{
    if (which < 0 || which >= S_COUNT || out == nullptr || count > (1ull << 32) || (which == S_CUBOID_SCALE && (count > 64ull || first_word + count > 64ull)))
        return PT_PROBE_E_BAD_ARGUMENT;
    for (int k = 0; k < SWEEP_OUT_WORDS; k++) out[k] = 0u;
#ifdef PT_PROBE_HOST
    unsigned long long bad = 0ull;
    double worst = 0.0;
    for (unsigned long long i = 0; i < count; i++) {
        const uint32_t w = first_word + (uint32_t)i;
        double err;
        if (!sweep_word(which, w, err)) {
            if (bad < 16ull) out[6 + bad] = w;
            bad++;
        }
        if (err > worst) { worst = err; out[4] = w; }
    }
    out[0] = (uint32_t)bad; out[1] = (uint32_t)(bad >> 32);
    out[5] = (uint32_t)(bad < 16ull ? bad : 16ull);
    put_double(worst, out + 2);
    return 0;
#else
    int rc = 0;
    uint32_t *dout = nullptr;
    PROBE_HIP(hipMalloc((void **)&dout, SWEEP_OUT_WORDS * 4));
    if (rc == 0) PROBE_HIP(hipMemset(dout, 0, SWEEP_OUT_WORDS * 4));
    if (rc == 0 && count != 0ull) {
        const unsigned long long blocks = (count + 255ull) / 256ull;
        probe_sweep_kernel<<<dim3((unsigned)(blocks < 8192ull ? blocks : 8192ull)), dim3(256)>>>(which, first_word, count, dout);
        PROBE_HIP(hipGetLastError());
    }
    if (rc == 0) PROBE_HIP(hipDeviceSynchronize());
    if (rc == 0) PROBE_HIP(hipMemcpy(out, dout, SWEEP_OUT_WORDS * 4, hipMemcpyDeviceToHost));
    if (dout) PROBE_HIP(hipFree(dout));
    if (rc == 0) { // the packed maximum's word moves to its slot; at most 16 offending words were stored
        out[4] = out[22];
        out[22] = out[23] = 0u;
        if (out[5] > 16u) out[5] = 16u;
    }
    return rc;
#endif
}

PT_PROBE_API int pt_probe_columns(int which, int *in_cols, int *out_cols)
{
    if (which < 0 || which >= F_COUNT) return PT_PROBE_E_BAD_ARGUMENT;
    *in_cols = kInCols[which];
    *out_cols = kOutCols[which];
    return 0;
}
