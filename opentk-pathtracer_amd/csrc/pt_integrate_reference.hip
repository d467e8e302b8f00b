// pt_integrate_reference.hip — the integrator in the REFERENCE arithmetic (pt_set_arithmetic(h, PT_ARITH_REFERENCE); the arithmetic
// and its specification: pt_math_reference.hpp).  Same shape as variant 1 of pt_integrate_persistent.hip: one wavefront per 8x8 tile,
// one pixel per lane, the spp loop inside the lane, a plain read-modify-write of the accumulation image with alpha = 1 — no tags, no
// batching, no snapshot.  The scene is staged into LDS by stage_scene (geometry, materials, sRGB LUT; its 1 / radius table is the
// contract's and is not read here), and every ray visits all spheres, then all cuboids, in the reference's order.
// Also here: the atmosphere precompute (atmo_precompute_reference_kernel) and the post-process tone map (pt_postprocess_reference_kernel)
// in the same arithmetic, at the end.
// Build flags: those of the library (-ffp-contract=off -fno-fast-math: a written a * b + c keeps two roundings).
#include "pt_kernel_common.hpp"
#include "pt_math_reference.hpp"
#include "pt_atmosphere_reference.hpp"
#include "pt_postprocess_reference.hpp"

namespace pt {

__global__ __launch_bounds__(256) void pt_integrate_reference_kernel(const FrameArgs a)
{
    SceneLds sc = stage_scene(a);
    EnvRef env{a.env, (LdsFloats)sc.lut, a.envSize, a.envFormat};
    const int tid = threadIdx.x;
    const int b = xcd_band_id(blockIdx.x, gridDim.x);
    const int wave = tid >> 6, lane = tid & 63;
    const int tile = b * 4 + wave;
    if (tile >= a.tilesX * a.tilesY) return;
    const int tx = tile % a.tilesX, ty = tile / a.tilesX;
    const int px = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3); // row inside this launch's row block
    if (px >= a.width || ly >= a.rows) return;
    const size_t idx = (size_t)ly * a.width + px;
    const float4 last = a.accum[idx];                                   // imageLoad  (compute.glsl:126)
    const float4 next = ref::shade_pixel_ref(a, sc, env, px, global_row(a, ly), last);
    AUDIT_RESOLVE(a, idx, a.frame, last, next, 1);
    a.accum[idx] = next;                                                // imageStore (compute.glsl:129)
}

hipError_t launch_integrate_reference(const FrameArgs &args, hipStream_t stream)
{
    FrameArgs a = args;
    a.materialsInLds = 1; // (stage_scene: materials in LDS, no sphere grid)
    a.gridLdsBytes = 0;
    if (a.spp < 1 || a.tilesX < 1 || a.tilesY < 1) return hipErrorInvalidValue;
    const int tiles = a.tilesX * a.tilesY;
    const size_t lds = scene_lds_bytes(a.numSpheres, a.numCuboids, a.envFormat, true);
    hipLaunchKernelGGL(pt_integrate_reference_kernel, dim3((tiles + 3) / 4), dim3(256), lds, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- atmosphere
// The atmosphere precompute in the reference arithmetic (pt_atmosphere_set_arithmetic; device functions and the x-mirror shortcut
// with its proof: pt_atmosphere_reference.hpp).  One lane per canonical texel — the lower texel of a mirrored pair or a texel without
// partner — so the grid holds no idle wavefronts; one wavefront per workgroup (no LDS, no barrier, nothing shared: single wavefronts
// are the finest grain the dispatcher can spread over the XCDs — a 256^2 cube is 3,092 wavefronts for 1,024 SIMDs).
__global__ __launch_bounds__(64) void atmo_precompute_reference_kernel(const AtmoArgs a)
{
    const int S = a.size;
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= (size_t)S * ref::atmo_row_lanes_ref(S)) return;
    const ref::AtmoLaneRef o = ref::atmo_lane_ref(a.invProj, &a.invView[0][0], a.lightPos, a.lightIntensity, S, a.iSteps, a.jSteps, i);
    a.out[o.texel[0]] = make_float4(o.col[0].x, o.col[0].y, o.col[0].z, 1.0f);
    if (o.n > 1) a.out[o.texel[1]] = make_float4(o.col[1].x, o.col[1].y, o.col[1].z, 1.0f);
}

hipError_t launch_atmosphere_reference(const AtmoArgs &a, hipStream_t stream)
{
    const size_t n = (size_t)a.size * ref::atmo_row_lanes_ref(a.size);
    hipLaunchKernelGGL(atmo_precompute_reference_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- post-process
// The tone map in the reference arithmetic (pt_present_set_arithmetic; device functions and specification: pt_postprocess_reference.hpp).
// The contract kernel's shape (pt_helper_kernels.hip, pt_postprocess_kernel), for the same reasons: HBM-bound, 16 B read + 4 B written
// per pixel, one whole float4 load and one whole uchar4 store per lane, no LDS; launched beside resident persistent wavefronts by the
// present paths, so it raises its wave priority first.
__global__ __launch_bounds__(256) void pt_postprocess_reference_kernel(const float4 *accum, uchar4 *out, size_t n)
{
    __builtin_amdgcn_s_setprio(3);
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n; i += stride) out[i] = ref::postprocess_pixel_ref(accum[i]);
}

hipError_t launch_postprocess_reference(const float4 *accum, void *outRgba8, size_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    size_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pt_postprocess_reference_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, accum, (uchar4 *)outRgba8, n);
    return hipGetLastError();
}

} // namespace pt
