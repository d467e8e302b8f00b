// pt_denoise_moments.hip — the temporal moments of the preview denoiser (pt_denoise_set_moments): a per-pixel
// variance of the image measured ACROSS frames — the temporal-moments half of SVGF (Schied et al. 2017), whose spatial half is
// pt_denoise.hip's stage V — recovered from the accumulation image alone at the moments pt_denoise_render looks at it.  The reference has
// no counterpart: it shows the raw accumulation image (MainWindow.cs:49-63 -> ScreenEffect.cs:29-37).
// The definition is DESIGN.md section 3.5, restated in numpy float32 by tests/denoise_moments_reference.py; stages M and B reproduce
// that restatement bit for bit, so every expression below is a fixed sequence of single IEEE binary32 + - * / operations, comparisons
// and selects under the conventions of pt_denoise.hip: nothing fused (-ffp-contract=off -fno-fast-math), no fminf / fmaxf
// (x > 0 ? x : 0 sends NaN to 0), `/` = the correctly rounded divide.
// Build flags: those of the library.
#include "pt_kernel_common.hpp"

namespace pt {

// ---------------------------------------------------------------------------------------------- stage M
// One observation of the image and the noise map Vm it yields.  Pointwise, 256-thread workgroups, one pixel per lane: one 16-byte load
// of C, an 8-byte read-modify-write of (lprev, M2), the id from word 3 of the guide record, a 4-byte store of Vm.
// l = the luminance of u's definition (0.2126 r + 0.7152 g + 0.0722 b, left to right).  a.observe — 0: the image holds what the last
// observation saw (or nothing), the state stays; 1: the first observation, M2 = 0; 2: the weighted Welford update with the mean b of
// the block of samples since the last look, b = (nf l - npf lprev) / w, M2 += (w (b - lprev)) (b - l).  a.estimate (K >= 2 after this
// observation): Vm = the variance of the mean of the nf samples, s2 / nf with s2 = M2 / (K - 1), carried to u by the square of
// du/dl = g^2, g = 1 / (1 + l); 0 on a miss and where it is not > 0.
__global__ __launch_bounds__(256) void pt_moments_kernel(const MomentsArgs a)
{
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= a.pixels) return;
    const float4 c = a.colIn[at];
    const float l = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
    float m2 = 0.0f;
    if (a.observe != 1) { // (the first observation reads no state: the buffer is as hipMalloc left it)
        const float2 st = a.state[at];
        m2 = st.y;
        if (a.observe == 2) {
            const float b = (a.nf * l - a.npf * st.x) / a.w;
            m2 = m2 + (a.w * (b - st.x)) * (b - l);
        }
    }
    if (a.observe != 0) a.state[at] = make_float2(l, m2);
    float vm = 0.0f;
    if (a.estimate && __float_as_int(a.guides[2 * at].w) != -1) {
        const float s2 = m2 / a.km1;
        const float vl = s2 / a.nf;
        const float g = 1.0f / (1.0f + l);
        const float g2 = g * g;
        const float v = (vl * g2) * g2;
        vm = v > 0.0f ? v : 0.0f;
    }
    a.noise[at] = vm;
}

hipError_t launch_moments(const MomentsArgs &a, hipStream_t stream)
{
    if (a.pixels == 0 || a.observe < 0 || a.observe > 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_moments_kernel, dim3((unsigned)((a.pixels + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- stage B
// var_0(p) = ((Km1 Vt) + (K0 V0)) / (Km1 + K0): the measured variance, Vt = the mean of Vm over the pixels of p's id in the 3x3 window
// around p (dy outer, dx inner, the centre included, so at least one cell is visited), blended with stage V's spatial estimate V0 as a
// prior worth K0 observations; var_0 = V0 on a miss.  16x16 tiles, one pixel per lane; (Vm, id bits) of the tile and a halo of 1 staged
// into LDS: 18 x 18 cells of 8 bytes.  Cells outside the image hold an id no guide record has, as in pt_variance_kernel, so "outside"
// and "another id" are one comparison.
constexpr int kMomentsOutsideId = (int)0x80000000;

__global__ __launch_bounds__(256) void pt_moments_blend_kernel(const MomentsBlendArgs a)
{
    constexpr int LW = 18;
    __shared__ float2 sV[LW * LW];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
    const int px = x0 + lx, py = y0 + ly;
    for (int i = tid; i < LW * LW; i += 256) {
        const int qx = x0 - 1 + i % LW, qy = y0 - 1 + i / LW;
        float2 cell = make_float2(0.0f, __int_as_float(kMomentsOutsideId));
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const size_t at = (size_t)qy * a.width + qx;
            cell = make_float2(a.noise[at], a.guides[2 * at].w);
        }
        sV[i] = cell;
    }
    __syncthreads();
    if (px >= a.width || py >= a.height) return;
    const size_t center = (size_t)py * a.width + px;
    const int lc = (ly + 1) * LW + lx + 1;
    const int idp = __float_as_int(sV[lc].y);
    float v = a.v0[center];
    if (idp != -1) {
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
        const float vt = s / n;
        v = ((a.km1 * vt) + (a.k0 * v)) / (a.km1 + a.k0);
    }
    a.var0[center] = v;
}

hipError_t launch_moments_blend(const MomentsBlendArgs &a, hipStream_t stream)
{
    if (a.width < 1 || a.height < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_moments_blend_kernel, dim3((a.width + 15) / 16, (a.height + 15) / 16), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- noise level
// pt_denoise_noise_level: per 256 consecutive pixels one binary32 partial sum of Vm over the pixels with id >= 0 and their count,
// partial[block] = (sum, count bits); the host adds the partials in index order in double.  The terms are not negative, so whatever the
// order of the 255 additions, the partial sum is within a relative 255 * 2^-24 of the exact one.  Here: a butterfly within each wavefront,
// then the four wavefronts' sums through LDS, added in wavefront order.
__global__ __launch_bounds__(256) void pt_moments_level_kernel(const float *noise, const float4 *guides, float2 *partial, size_t pixels)
{
    __shared__ float sSum[4];
    __shared__ int sCount[4];
    const int tid = threadIdx.x;
    const size_t at = (size_t)blockIdx.x * 256 + tid;
    float s = 0.0f;
    int n = 0;
    if (at < pixels && __float_as_int(guides[2 * at].w) >= 0) {
        s = noise[at];
        n = 1;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s = s + __shfl_down(s, off, 64);
        n = n + __shfl_down(n, off, 64);
    }
    if ((tid & 63) == 0) {
        sSum[tid >> 6] = s;
        sCount[tid >> 6] = n;
    }
    __syncthreads();
    if (tid == 0)
        partial[blockIdx.x] = make_float2(((sSum[0] + sSum[1]) + sSum[2]) + sSum[3], __int_as_float(((sCount[0] + sCount[1]) + sCount[2]) + sCount[3]));
}

hipError_t launch_moments_level(const float *noise, const float4 *guides, float2 *partial, size_t pixels, hipStream_t stream)
{
    if (pixels == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_moments_level_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream, noise, guides, partial, pixels);
    return hipGetLastError();
}

} // namespace pt
