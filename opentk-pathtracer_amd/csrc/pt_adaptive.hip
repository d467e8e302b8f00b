// pt_adaptive.hip — adaptive sampling (pt_adaptive_render): one pass gives every 8x8 tile that is still ACTIVE one
// more sample per pixel — the tile's own frame index k, so a pixel that has received k samples holds bit for bit what k uniform frames
// leave there (a sample depends on (x, y, k) and the inputs only: pixel_seed) — and measures, from the running mean before and after
// the fold, how noisy the tile still is.  The reference has no counterpart: it spends every frame on every pixel (PathTracer.cs:114-129).
// Shape: that of variant 1 (pt_integrate_persistent.hip) and of pt_integrate_reference_kernel — one wavefront per tile, one pixel per
// lane, the spp loop inside the lane, a plain read-modify-write of the image with alpha = 1, the scene staged by stage_scene with the
// materials in LDS, every ray through `radiance` (all spheres, then all cuboids).
// The noise estimate is the definition of DESIGN.md section 3.5, restated in numpy float32 by tests/adaptive_reference.py; the kernel
// reproduces that restatement bit for bit, so every expression of it is a fixed sequence of single IEEE binary32 + - * / operations,
// comparisons and selects under the conventions of pt_denoise.hip: nothing fused (-ffp-contract=off -fno-fast-math), no fminf / fmaxf
// (x > 0 ? x : 0 sends NaN to 0), `/` = the correctly rounded divide.
// Build flags: those of the library.
#include "pt_kernel_common.hpp"

namespace pt {

// resolve_pixel / shade_pixel (pt_device.hpp) with the frame index as an argument instead of a.frame: compute.glsl:101-130 for frame `frame`
PT_DEV float4 resolve_pixel_at(const FrameArgs &a, v3 irr, float4 last, int frame)
{
    irr = v_scale(irr, f_div_ieee(1.0f, (float)a.spp));
    float w = f_div_ieee(1.0f, (float)(frame + 1));
    return make_float4(f_mix(last.x, irr.x, w), f_mix(last.y, irr.y, w), f_mix(last.z, irr.z, w), 1.0f);
}

PT_DEV float4 shade_pixel_at(const FrameArgs &a, const SceneLds &sc, const EnvRef &env, int px, int py, float4 last, int frame)
{
    uint32_t seed = pixel_seed(px, py, frame);
    v3 irr = V(0.0f, 0.0f, 0.0f);
    for (int s = 0; s < a.spp; s++) {
        v3 ro, rd;
        primary_ray(a, px, py, seed, ro, rd);
        irr = v_add(irr, radiance(a, sc, env, ro, rd, seed));
    }
    return resolve_pixel_at(a, irr, last, frame);
}

// the luminance of u's definition, left to right
PT_DEV float adaptive_lum(float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// the decision of a pass, from the stored record (k, k0, err bits, n) and the parameters in force
PT_DEV bool adaptive_active(int4 rec, const AdaptiveArgs &ad)
{
    return rec.x < ad.maxSamples && (rec.x - rec.y < ad.minSamples - 1 || __int_as_float(rec.z) > ad.threshold);
}

// the kernel's second argument re-read from the kernarg segment where it is used (scalar loads; see cold_args in pt_device.hpp)
typedef const __attribute__((address_space(4))) AdaptiveArgs *ColdAdaptive;
static_assert(sizeof(FrameArgs) % alignof(AdaptiveArgs) == 0, "AdaptiveArgs follows FrameArgs in the kernarg segment without padding");
PT_DEV ColdAdaptive cold_adaptive()
{
    const __attribute__((address_space(4))) char *p = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (ColdAdaptive)(p + sizeof(FrameArgs));
}

// One pass.  Workgroup = four consecutive tiles (after the XCD band mapping), as in variant 1.  Every thread loads the workgroup's four
// records (16 bytes each, one line); a workgroup none of whose tiles is active leaves before the scene is staged — the condition is
// workgroup-uniform, so no part of a workgroup skips stage_scene's barrier — and an inactive wavefront of an active workgroup leaves
// behind it.  Lanes outside the image (ragged edge tiles) trace nothing and bring +0 into the tile sum: the six shuffles run with all 64
// lanes in converged control flow.  Per active in-image pixel: 16 B read + 16 B written of the image, 8 B read + 8 B written of
// (M2, e); per active tile 16 B read and written by lane 0.  Scalar registers: the kernel sits at variant 1's 106 and adds one live
// value to it — the exec mask saved around the in-image branch, which variant 1 does not need because its lanes outside the image
// return — so the compiler parks one 64-bit scalar pair in two lanes of a vector register before the sample loop and fetches it behind
// it (2 v_writelane + 2 v_readlane per wavefront and pass, outside every loop; no scratch).
__global__ __launch_bounds__(256) void pt_adaptive_kernel(const FrameArgs a, const AdaptiveArgs ad)
{
    const int tid = threadIdx.x;
    const int b = xcd_band_id(blockIdx.x, gridDim.x);
    const int wave = tid >> 6, lane = tid & 63;
    const int tiles = a.tilesX * a.tilesY;
    int4 rec = make_int4(0, 0, 0, 0);
    bool mine = false, any = false;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int t = b * 4 + w;
        if (t >= tiles) continue;
        const int4 r = ad.tiles[t];
        const bool act = adaptive_active(r, ad);
        any = any || act;
        if (w == wave) {
            rec = r;
            mine = act;
        }
    }
    if (__builtin_amdgcn_readfirstlane((int)any) == 0) return; // (workgroup-uniform)
    SceneLds sc = stage_scene(a);
    if (__builtin_amdgcn_readfirstlane((int)mine) == 0) return; // (wave-uniform)
    EnvRef env{a.env, (LdsFloats)sc.lut, a.envSize, a.envFormat};
    const int tile = b * 4 + wave;
    const int k = rec.x; // the tile's frame index: wave-uniform, kept in a vector register (the bounce loop needs the scalar ones)
    const int tx = tile % a.tilesX, ty = tile / a.tilesX;
    const int px = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3); // row inside this handle's rows
    float e = 0.0f;
    if (px < a.width && ly < a.rows) {
        const size_t idx = (size_t)ly * a.width + px;
        const float4 last = a.accum[idx];                                   // imageLoad  (compute.glsl:126)
        const float4 next = shade_pixel_at(a, sc, env, px, global_row(a, ly), last, k);
        a.accum[idx] = next;                                                // imageStore (compute.glsl:129)
        // the statistics.  What they need besides k is fetched here, behind the bounce loop, as cold_args() does it: nothing of it is
        // kept in scalar registers while the paths run (the loop needs them for its exec-mask nesting)
        ColdAdaptive ca = cold_adaptive();
        const int k0 = ca->tiles[tile].y, kNext = k + 1;
        float2 *stats = ca->stats;
        const float kf = (float)kNext;
        const float lNext = adaptive_lum(next);
        const float d = lNext - adaptive_lum(last);
        float m2 = stats[idx].x;
        if (kNext > k0) m2 = m2 + (kf * (kf - 1.0f)) * (d * d);
        const int j = kNext - k0;
        if (j >= 1) {
            const float v = m2 / ((float)j * kf);
            const float s = 1.0f + lNext;
            const float q = (s * s) * (s * s);
            e = v / q;
            e = e > 0.0f ? e : 0.0f;
        }
        stats[idx] = make_float2(m2, e);
    }
    float s = e;
#pragma unroll
    for (int step = 1; step <= 32; step <<= 1) s = s + __shfl_xor(s, step, 64);
    if (lane == 0) {
        int4 *own = cold_adaptive()->tiles + tile;
        const int4 r = *own; // (k, k0, the old err, n): nobody else writes the record
        *own = make_int4(r.x + 1, r.y, __float_as_int(s / (float)r.w), r.w);
    }
}

// the records of a fresh state: k = F, k0 = max(F, 1), err = +0, n = the tile's in-image pixels
__global__ __launch_bounds__(256) void pt_adaptive_init_kernel(int4 *tiles, int tilesX, int tilesY, int width, int rows, int frame)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= tilesX * tilesY) return;
    const int tx = t % tilesX, ty = t / tilesX;
    const int w = width - tx * 8 < 8 ? width - tx * 8 : 8, h = rows - ty * 8 < 8 ? rows - ty * 8 : 8;
    tiles[t] = make_int4(frame, frame > 1 ? frame : 1, 0, w * h);
}

hipError_t launch_adaptive_init(int4 *tiles, int tilesX, int tilesY, int width, int rows, int frame, hipStream_t stream)
{
    if (tilesX < 1 || tilesY < 1 || frame < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_adaptive_init_kernel, dim3((tilesX * tilesY + 255) / 256), dim3(256), 0, stream, tiles, tilesX, tilesY, width, rows, frame);
    return hipGetLastError();
}

hipError_t launch_adaptive(const FrameArgs &args, const AdaptiveArgs &ad, hipStream_t stream)
{
    FrameArgs a = args;
    a.materialsInLds = 1; // (stage_scene: materials in LDS, no sphere grid)
    a.gridLdsBytes = 0;
    if (a.spp < 1 || a.tilesX < 1 || a.tilesY < 1 || !ad.tiles || !ad.stats) return hipErrorInvalidValue;
    const int tiles = a.tilesX * a.tilesY;
    const size_t lds = scene_lds_bytes(a.numSpheres, a.numCuboids, a.envFormat, true);
    hipLaunchKernelGGL(pt_adaptive_kernel, dim3((tiles + 3) / 4), dim3(256), lds, stream, a, ad);
    return hipGetLastError();
}

} // namespace pt
