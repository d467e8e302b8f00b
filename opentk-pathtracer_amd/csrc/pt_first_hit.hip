// pt_first_hit.hip — the first-hit query (pt_first_hit_render / pt_pick): per pixel the primary ray of sample 0 of a frame (or, under
// pt_first_hit_set_ray(PT_RAY_PINHOLE), the pixel-centre pinhole ray: pt_first_hit_pinhole_kernel), the object
// it meets first and the distance RayTrace leaves (compute.glsl:106-121 and :226-258 — what the reference answers on the CPU with other
// formulas, src/Render/Gui.cs:223-233 -> src/MainWindow.cs:302-318).  Contract arithmetic (pt_math.hpp), whatever the three arithmetic
// switches say: the ray and the intersection are the ones variant 1 of pt_integrate_persistent.hip traces for that pixel and frame.
// Shape of pt_integrate_reference_kernel: one wavefront per 8x8 tile, one pixel per lane, 256-thread workgroups, XCD band mapping, the
// scene's geometry staged into LDS by stage_scene; every ray visits all spheres, then all cuboids, through ray_trace_t (no grid, no
// masks: wave-uniform loop indices, broadcast LDS reads).
// Which object won: ray_trace_t hands its caller the winner's MATERIAL (sc.mat + 4 * index, spheres first, then cuboids), not its index.
// The query has no use for materials, so the table it points sc.mat at holds the object's id in the slot of Albedo.x instead (exact in
// binary32: ids are below 2^24); the other 15 words of an entry are never written and never used.
// Build flags: those of the library.
#include "pt_kernel_common.hpp"

namespace pt {

// records: two float4 per pixel — (origin.xyz, t) and (direction.xyz, id bits).  pickTile < 0: every tile of the launch, pixel
// (px, local row ly) at records[2 * (ly * width + px)]; pickTile >= 0: that tile only (one workgroup), lane l at records[2 * l].
__global__ __launch_bounds__(256) void pt_first_hit_kernel(const FrameArgs a, float4 *records, const int pickTile)
{
    SceneLds sc = stage_scene(a); // (geometry only: the launch sets materialsInLds = 0, envFormat = 0, gridLdsBytes = 0)
    const int tid = threadIdx.x;
    const int ns = a.numSpheres, nc = a.numCuboids;
    float4 *ids = g_lds + scene_lds_bytes(ns, nc, 0, false) / sizeof(float4);
    for (int i = tid; i < ns + nc; i += 256) ids[4 * i] = make_float4((float)(i < ns ? i : kFirstHitCuboidBase + (i - ns)), 0.0f, 0.0f, 0.0f);
    __syncthreads();
    sc.mat = ids;
    const int b = xcd_band_id(blockIdx.x, gridDim.x);
    const int wave = tid >> 6, lane = tid & 63;
    const int tile = pickTile >= 0 ? pickTile : b * 4 + wave;
    if (tile >= a.tilesX * a.tilesY || (pickTile >= 0 && wave != 0)) return;
    const int tx = tile % a.tilesX, ty = tile / a.tilesX;
    const int px = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3); // row inside this handle's rows
    if (px >= a.width || ly >= a.rows) return;
#ifdef PT_PROFILE
    unsigned long long prof_dummy[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    uint32_t seed = pixel_seed(px, global_row(a, ly), a.frame); // compute.glsl:106
    v3 ro, rd;
    primary_ray(a, px, global_row(a, ly), seed, ro, rd);        // :113-121, sample 0
    Hit h;
    const bool hit = ray_trace(sc, ns, nc, ro, rd, h PROF_DUMMY); // :226-258
    const float t = hit ? h.T : __builtin_inff();
    const int id = hit ? (int)h.m.albedo.x : -1;
    const size_t at = pickTile >= 0 ? (size_t)lane : (size_t)ly * a.width + px;
    records[2 * at] = make_float4(ro.x, ro.y, ro.z, t);
    records[2 * at + 1] = make_float4(rd.x, rd.y, rd.z, __int_as_float(id));
}

// PT_RAY_PINHOLE (pt_first_hit_set_ray): the same records for the pixel-centre pinhole ray (pinhole_ray) instead of sample 0 — no seed,
// a.frame is not read.  A kernel of its own behind pt_first_hit_kernel, whose code stays as it was.
__global__ __launch_bounds__(256) void pt_first_hit_pinhole_kernel(const FrameArgs a, float4 *records, const int pickTile)
{
    SceneLds sc = stage_scene(a);
    const int tid = threadIdx.x;
    const int ns = a.numSpheres, nc = a.numCuboids;
    float4 *ids = g_lds + scene_lds_bytes(ns, nc, 0, false) / sizeof(float4);
    for (int i = tid; i < ns + nc; i += 256) ids[4 * i] = make_float4((float)(i < ns ? i : kFirstHitCuboidBase + (i - ns)), 0.0f, 0.0f, 0.0f);
    __syncthreads();
    sc.mat = ids;
    const int b = xcd_band_id(blockIdx.x, gridDim.x);
    const int wave = tid >> 6, lane = tid & 63;
    const int tile = pickTile >= 0 ? pickTile : b * 4 + wave;
    if (tile >= a.tilesX * a.tilesY || (pickTile >= 0 && wave != 0)) return;
    const int tx = tile % a.tilesX, ty = tile / a.tilesX;
    const int px = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
    if (px >= a.width || ly >= a.rows) return;
#ifdef PT_PROFILE
    unsigned long long prof_dummy[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    v3 ro, rd;
    pinhole_ray(a, px, global_row(a, ly), ro, rd);
    Hit h;
    const bool hit = ray_trace(sc, ns, nc, ro, rd, h PROF_DUMMY); // :226-258
    const float t = hit ? h.T : __builtin_inff();
    const int id = hit ? (int)h.m.albedo.x : -1;
    const size_t at = pickTile >= 0 ? (size_t)lane : (size_t)ly * a.width + px;
    records[2 * at] = make_float4(ro.x, ro.y, ro.z, t);
    records[2 * at + 1] = make_float4(rd.x, rd.y, rd.z, __int_as_float(id));
}

hipError_t launch_first_hit(const FrameArgs &args, float4 *records, int pickTile, bool pinhole, hipStream_t stream)
{
    FrameArgs a = args;
    a.materialsInLds = 0; // (stage_scene: geometry only — the material table is the kernel's id table)
    a.gridLdsBytes = 0;
    a.envFormat = 0;      // (no environment is read: no sRGB table is staged)
    if (a.tilesX < 1 || a.tilesY < 1 || pickTile >= a.tilesX * a.tilesY) return hipErrorInvalidValue;
    const int tiles = a.tilesX * a.tilesY;
    const size_t lds = scene_lds_bytes(a.numSpheres, a.numCuboids, 0, false) + (size_t)(a.numSpheres + a.numCuboids) * 4 * sizeof(float4);
    const dim3 grid(pickTile >= 0 ? 1 : (tiles + 3) / 4);
    if (pinhole) hipLaunchKernelGGL(pt_first_hit_pinhole_kernel, grid, dim3(256), lds, stream, a, records, pickTile);
    else hipLaunchKernelGGL(pt_first_hit_kernel, grid, dim3(256), lds, stream, a, records, pickTile);
    return hipGetLastError();
}

} // namespace pt
