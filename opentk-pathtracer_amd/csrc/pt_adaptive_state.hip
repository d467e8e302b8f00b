// pt_adaptive_state.hip — the derived half of an adaptive state rebuilt from its persistent half (pt_adaptive_write_state; DESIGN.md
// section 3.5).  A state is the image, the frame index F, (k, k0, n) per 8x8 tile and the Welford sum M2 per pixel; the per-pixel estimate e
// and the per-tile err are functions of those — steps 4 and 5 of the sampler's definition evaluated with kNext = k — so a restored state
// need not carry them: this kernel writes them, bit for bit as the pass that left the state wrote them.  The reference has no counterpart:
// it spends every frame on every pixel and keeps nothing across runs but a screenshot (PathTracer.cs:114-129, Gui.cs:28-33).
// Shape: pt_adaptive_kernel's (pt_adaptive.hip) without the tracing — one wavefront per tile, workgroups of four tiles, lane
// (y & 7) 8 + (x & 7), no scene, no LDS.  The expressions are restated here, not shared with pt_adaptive.hip: tests/adaptive_state_reference.py
// restates them a third time in numpy float32, and the kernel reproduces that restatement bit for bit under the conventions of
// pt_denoise.hip: single IEEE binary32 + - * /, nothing fused (-ffp-contract=off -fno-fast-math), no fminf / fmaxf (x > 0 ? x : 0 sends NaN
// to 0), `/` = the correctly rounded divide.
// Build flags: those of the library.
#include "pt_kernel_common.hpp"

namespace pt {

// l(c) = (0.2126 r + 0.7152 g) + 0.0722 b, left to right
PT_DEV float rebuild_lum(float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// A wavefront past the last tile leaves before it touches memory (wave-uniform).  Lanes outside the image (ragged edge tiles) bring +0
// into the tile sum: the six shuffles run with all 64 lanes in converged control flow.  Per in-image pixel: 16 B of the image and the
// 4 B of M2 read, 8 B of (M2, e) written in one store; per tile 16 B read by every lane (one line) and written by lane 0.
__global__ __launch_bounds__(256) void pt_adaptive_rebuild_kernel(const AdaptiveRebuildArgs a)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * 4 + wave;
    if (tile >= a.tilesX * a.tilesY) return;
    const int4 rec = a.tiles[tile]; // (k, k0, err: not read, n)
    const int k = rec.x, j = rec.x - rec.y;
    const int tx = tile % a.tilesX, ty = tile / a.tilesX;
    const int px = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3); // row inside this handle's rows
    float e = 0.0f;
    if (px < a.width && ly < a.rows) {
        const size_t idx = (size_t)ly * a.width + px;
        const float m2 = a.stats[idx].x;
        if (j >= 1) {
            const float kf = (float)k;
            const float v = m2 / ((float)j * kf);
            const float s = 1.0f + rebuild_lum(a.image[idx]);
            const float q = (s * s) * (s * s);
            e = v / q;
            e = e > 0.0f ? e : 0.0f;
        }
        a.stats[idx] = make_float2(m2, e);
    }
    float s = e;
#pragma unroll
    for (int step = 1; step <= 32; step <<= 1) s = s + __shfl_xor(s, step, 64);
    if (lane == 0) a.tiles[tile] = make_int4(rec.x, rec.y, __float_as_int(s / (float)rec.w), rec.w);
}

hipError_t launch_adaptive_rebuild(const AdaptiveRebuildArgs &a, hipStream_t stream)
{
    if (a.width < 1 || a.rows < 1 || a.tilesX != (a.width + 7) / 8 || a.tilesY != (a.rows + 7) / 8 || !a.image || !a.stats || !a.tiles) return hipErrorInvalidValue;
    const int tiles = a.tilesX * a.tilesY;
    hipLaunchKernelGGL(pt_adaptive_rebuild_kernel, dim3((tiles + 3) / 4), dim3(256), 0, stream, a);
    return hipGetLastError();
}

} // namespace pt
