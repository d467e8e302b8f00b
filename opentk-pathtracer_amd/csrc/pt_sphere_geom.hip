// pt_sphere_geom.hip — the packed sphere geometry behind the device's GameObjectsUBO (pt_kernels.hpp: kSphereGeomOffset), which the scalar
// sphere step of ray_trace_t (pt_device.hpp) reads four spheres at a time: refreshed by pt_upload_game_objects behind every upload.
// Build flags (see __graft_entry__.build): -O3 -ffp-contract=off -fno-fast-math --offload-arch=gfx950
#include "pt_kernels.hpp"

namespace pt {

// sphereGeom[i] = float4 5 i of the std140 block for i in [first, first + count): one 16-byte load and store per lane, no arithmetic.
__global__ __launch_bounds__(256) void pt_sphere_geom_kernel(float *objects, int first, int count)
{
    const int t = (int)threadIdx.x;
    if (t >= count) return;
    const int i = first + t;
    const float4 *src = (const float4 *)objects;
    float4 *geom = (float4 *)((char *)objects + kSphereGeomOffset);
    geom[i] = src[(kSphereStride / 16) * i];
}

hipError_t launch_sphere_geom(float *objects, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    if (first < 0 || first + count > kSphereGeomEntries) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_sphere_geom_kernel, dim3(1), dim3(256), 0, stream, objects, first, count);
    return hipGetLastError();
}

} // namespace pt
