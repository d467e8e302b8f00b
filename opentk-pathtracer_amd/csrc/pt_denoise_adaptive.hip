// pt_denoise_adaptive.hip — the adaptive sampler's noise as the preview denoiser's noise source (pt_denoise_set_adaptive_noise; DESIGN.md
// section 3.5): on a live adaptive state pass 0 of PT_DENOISE_VARIANCE reads a variance formed from the per-pixel Welford estimate e that
// pt_adaptive_kernel keeps (pt_adaptive.hip) and the tile records, instead of stage V's spatial estimate alone.  The reference has no
// counterpart: it shows the raw accumulation image (MainWindow.cs:49-63 -> ScreenEffect.cs:29-37) and spends every frame on every pixel
// (PathTracer.cs:114-129).
// The definition is DESIGN.md section 3.5, restated in numpy float32 by tests/denoise_adaptive_reference.py; stage A reproduces that
// restatement bit for bit, so every expression below is a fixed sequence of single IEEE binary32 + - * / operations, comparisons and
// selects under the conventions of pt_denoise.hip: nothing fused (-ffp-contract=off -fno-fast-math), no fminf / fmaxf, `/` = the
// correctly rounded divide.  No select depends on a value, only on ids and counts.
// Build flags: those of the library.
#include "pt_kernel_common.hpp"

namespace pt {

// ---------------------------------------------------------------------------------------------- stage A
// var_0(p) = ((jf Et) + (K0 V0)) / (jf + K0) with jf = (float)(k_p - k0_p) of p's own 8x8 tile, Et = S / kf_p, S = the mean of e(q) kf_q
// over the pixels q of p's id in the 3x3 window around p (dy outer, dx inner, the centre included, so at least one cell is visited):
// e(q) kf_q is q's PER-SAMPLE variance of u, whatever count q's tile stands at, and Et carries the window's mean back to the variance of
// the mean at p's own count — a neighbour across a tile border tells p its per-sample variance, not its variance of the mean.
// var_0 = V0 on a miss and where k_p - k0_p <= 0 (no statistics yet).  The shape of pt_moments_blend_kernel: 16x16 tiles, one pixel per
// lane; (e kf, id bits) of the tile and a halo of 1 staged into LDS: 18 x 18 cells of 8 bytes, the product formed at staging with the
// record of the cell's own tile.  Cells outside the image hold an id no guide record has, so "outside" and "another id" are one
// comparison.  16 is a multiple of 8: a workgroup covers whole adaptive tiles, and a lane's own record is that of (px >> 3, py >> 3).
// Per pixel: 8 B of (M2, e), 4 B of the id word, 4 B of V0 read, 4 B written; a record of 16 B per 64 pixels.
constexpr int kAdaptiveOutsideId = (int)0x80000000;

__global__ __launch_bounds__(256) void pt_adaptive_blend_kernel(const AdaptiveBlendArgs a)
{
    constexpr int LW = 18;
    __shared__ float2 sV[LW * LW];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
    const int px = x0 + lx, py = y0 + ly;
    for (int i = tid; i < LW * LW; i += 256) {
        const int qx = x0 - 1 + i % LW, qy = y0 - 1 + i / LW;
        float2 cell = make_float2(0.0f, __int_as_float(kAdaptiveOutsideId));
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const size_t at = (size_t)qy * a.width + qx;
            const float kf = (float)a.tiles[(qy >> 3) * a.tilesX + (qx >> 3)].x;
            cell = make_float2(a.stats[at].y * kf, a.guides[2 * at].w);
        }
        sV[i] = cell;
    }
    __syncthreads();
    if (px >= a.width || py >= a.height) return;
    const size_t center = (size_t)py * a.width + px;
    const int lc = (ly + 1) * LW + lx + 1;
    const int idp = __float_as_int(sV[lc].y);
    const int4 rec = a.tiles[(py >> 3) * a.tilesX + (px >> 3)];
    const int j = rec.x - rec.y;
    float v = a.v0[center];
    if (idp != -1 && j > 0) {
        float s = 0.0f, n = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const float2 q = sV[lc + dy * LW + dx];
                const bool visit = __float_as_int(q.y) == idp;
                s = visit ? s + q.x : s;
                n = visit ? n + 1.0f : n;
            }
        }
        const float jf = (float)j;
        const float sm = s / n;
        const float et = sm / (float)rec.x;
        v = ((jf * et) + (a.k0 * v)) / (jf + a.k0);
    }
    a.var0[center] = v;
}

hipError_t launch_adaptive_blend(const AdaptiveBlendArgs &a, hipStream_t stream)
{
    if (a.width < 1 || a.height < 1 || a.tilesX != (a.width + 7) / 8 || !a.stats || !a.tiles) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_adaptive_blend_kernel, dim3((a.width + 15) / 16, (a.height + 15) / 16), dim3(256), 0, stream, a);
    return hipGetLastError();
}

} // namespace pt
