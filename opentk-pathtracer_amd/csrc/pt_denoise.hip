// pt_denoise.hip — the preview denoiser (pt_denoise_render): guide buffers from the integrator's own primary ray, and an edge-avoiding
// 5x5 a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination
// Filtering", HPG 2010) with edge-stopping on object id, shading normal, plane distance and tone-compressed luminance.  The reference
// has no counterpart: it shows the raw accumulation image, which every camera move, GUI edit and pick resets (MainWindow.cs:49-63).
// The filter's definition is DESIGN.md section 3.5, restated in numpy float32 by tests/denoise_reference.py; the kernels reproduce that
// restatement bit for bit, so every expression below is a fixed sequence of single IEEE binary32 + - * / operations, comparisons and
// selects: nothing fused (-ffp-contract=off -fno-fast-math), no transcendentals, no fminf / fmaxf (x > 0 ? x : 0 sends NaN to 0 the way
// np.where does), `/` = the correctly rounded divide (v_div_scale / v_div_fmas / v_div_fixup).
// Build flags: those of the library.
#include "pt_kernel_common.hpp"

namespace pt {

// ---------------------------------------------------------------------------------------------- guides
// Two float4 per pixel, rows like the image: G0 = (P.xyz, id bits), G1 = (N.xyz, t).  id and t as pt_first_hit_kernel writes them
// (the same ray: sample 0 of a.frame, the same ray_trace, the same id table in the Albedo.x slot); N = Hit::normal as ray_trace leaves
// it (compute.glsl:239-240,252-253: not flipped for FromInside); P = origin + direction * t in two roundings per component — the hit
// position of compute.glsl:238,251 without the contract's fused multiply-add, so that a host restates it from a first-hit record.
// Miss: id = -1, t = +inf, P = N = 0.  Shape of pt_first_hit_kernel: one wavefront per 8x8 tile, 256-thread workgroups.
__global__ __launch_bounds__(256) void pt_guides_kernel(const FrameArgs a, float4 *guides)
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
    const int tile = b * 4 + wave;
    if (tile >= a.tilesX * a.tilesY) return;
    const int tx = tile % a.tilesX, ty = tile / a.tilesX;
    const int px = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
    if (px >= a.width || ly >= a.rows) return;
#ifdef PT_PROFILE
    unsigned long long prof_dummy[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    uint32_t seed = pixel_seed(px, global_row(a, ly), a.frame); // compute.glsl:106
    v3 ro, rd;
    primary_ray(a, px, global_row(a, ly), seed, ro, rd);        // :113-121, sample 0
    Hit h;
    const bool hit = ray_trace(sc, ns, nc, ro, rd, h PROF_DUMMY); // :226-258
    float4 g0 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    float4 g1 = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
    if (hit) {
        g0 = make_float4(rd.x * h.T + ro.x, rd.y * h.T + ro.y, rd.z * h.T + ro.z, __int_as_float((int)h.m.albedo.x));
        g1 = make_float4(h.normal.x, h.normal.y, h.normal.z, h.T);
    }
    const size_t at = (size_t)ly * a.width + px;
    guides[2 * at] = g0;
    guides[2 * at + 1] = g1;
}

// (pt_denoise_set_lens on: the same records from the pinhole ray; kernel and launch at the end of the file, behind the kernels that were
// here before)
static void launch_guides_pinhole(const FrameArgs &a, float4 *guides, int tiles, size_t lds, hipStream_t stream);

hipError_t launch_guides(const FrameArgs &args, float4 *guides, bool pinhole, hipStream_t stream)
{
    FrameArgs a = args;
    a.materialsInLds = 0; // (stage_scene: geometry only — the material table is the kernel's id table)
    a.gridLdsBytes = 0;
    a.envFormat = 0;      // (no environment is read: no sRGB table is staged)
    if (a.tilesX < 1 || a.tilesY < 1) return hipErrorInvalidValue;
    const int tiles = a.tilesX * a.tilesY;
    const size_t lds = scene_lds_bytes(a.numSpheres, a.numCuboids, 0, false) + (size_t)(a.numSpheres + a.numCuboids) * 4 * sizeof(float4);
    if (pinhole) launch_guides_pinhole(a, guides, tiles, lds, stream);
    else hipLaunchKernelGGL(pt_guides_kernel, dim3((tiles + 3) / 4), dim3(256), lds, stream, a, guides);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- a-trous pass
// u(c) = l / (1 + l), l = 0.2126 r + 0.7152 g + 0.0722 b (left to right): the luminance the colour weight compares, compressed to [0, 1)
PT_DEV float dn_u(float r, float g, float b)
{
    const float l = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    return l / (1.0f + l);
}

// The two guide weights of a tap q for the centre p, shared by the a-trous passes and the temporal stage: wn = max(N_p . N_q, 0) squared
// normalPower times, wz = max(1 - ((N_p . (P_q - P_p)) / planeDen)^2, 0) with planeDen = sigma_plane * t_p.  Returned apart: each
// caller multiplies them into its own weight in its own order.
PT_DEV void dn_guide_weights(const float4 &g0p, const float4 &g1p, const float4 &g0q, const float4 &g1q, float planeDen, int normalPower,
                             float &wn, float &wz)
{
    const float d = (g1p.x * g1q.x + g1p.y * g1q.y) + g1p.z * g1q.z;
    wn = d > 0.0f ? d : 0.0f;
    for (int k = 0; k < normalPower; k++) wn = wn * wn;
    const float ex = g0q.x - g0p.x, ey = g0q.y - g0p.y, ez = g0q.z - g0p.z;
    const float e = (g1p.x * ex + g1p.y * ey) + g1p.z * ez;
    const float r = e / planeDen;
    const float z = 1.0f - r * r;
    wz = z > 0.0f ? z : 0.0f;
}

// One pass, one pixel per lane, for both modes.  S = 1, 2: the step; the 16x16 tile plus a halo of 2 S pixels — G0, G1 and (r, g, b, u) =
// 48 bytes per pixel — is staged into LDS (S = 2: 24 x 24 x 48 = 27,648 bytes), u evaluated once per staged pixel instead of once per tap.
// S = 0: any step (a.step), 64x4 tiles, every tap read from memory — a wavefront is 64 adjacent pixels of one row, so each tap is one
// coalesced 1 KB load per array; G0 first, G1 and the colour only where the id matches.
// VARIANCE (PT_DENOISE_VARIANCE): the luminance stop is scaled by the centre's variance instead of a.invSigma, and the variance is filtered
// along with the colour (Q += w^2 var_q; output Q / W^2).  The variance of the input travels in colIn's alpha — on pass 0 in a.varIn, the
// estimate of stage V, since the accumulation image's alpha carries frame tags — and that of the output in colOut's alpha (a.last:
// alpha = 1).  S = 1, 2: one more float per staged pixel, 52 bytes per pixel, 29,952 bytes at S = 2; S = 0: read with the colour.  The
// fixed mode has no such array and reads neither a.varIn, a.k2 nor a.last; its alpha is not read and written as 1.
// LENS (pt_denoise_set_lens on, a.cocK > 0): a pixel's blur radius is c = (cocK * |t - focal|) / t, c = cocK on a miss (dn_coc); a tap at
// Chebyshev distance r = step * max(|dx|, |dy|) with r <= c(p) and r <= c(q) is relaxed: taken whatever its id, with wn = wz = 1.
// S = 1, 2: c is evaluated once per staged pixel and staged where t was (no tap reads a neighbour's t; the centre fetches its own from
// memory), so the LDS footprint is that of LENS = false.  S = 0: G1 is loaded where the id matches or r <= c(p), and c(q) divided out
// only in the second case.
PT_DEV float dn_coc(int id, float t, float cocK, float focal)
{
    return id == -1 ? cocK : (cocK * __builtin_fabsf(t - focal)) / t;
}

template <int S, bool VARIANCE, bool LENS>
__global__ __launch_bounds__(256) void pt_atrous_kernel(const AtrousArgs a)
{
    constexpr int TX = S ? 16 : 64, TY = S ? 16 : 4, HALO = 2 * S, LW = TX + 2 * HALO, LH = TY + 2 * HALO;
    __shared__ float4 sG0[S ? LW * LH : 1], sG1[S ? LW * LH : 1], sC[S ? LW * LH : 1];
    __shared__ float sV[S && VARIANCE ? LW * LH : 1];
    const int tid = threadIdx.x, lx = tid % TX, ly = tid / TX;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int px = x0 + lx, py = y0 + ly;
    const int step = S ? S : a.step;
    if constexpr (S != 0) {
        for (int i = tid; i < LW * LH; i += 256) {
            const int qx = x0 - HALO + i % LW, qy = y0 - HALO + i / LW;
            if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) { // (cells outside the image are never read: their taps are skipped)
                const size_t at = (size_t)qy * a.width + qx;
                float4 c = a.colIn[at];
                if constexpr (VARIANCE) sV[i] = a.varIn ? a.varIn[at] : c.w;
                c.w = dn_u(c.x, c.y, c.z);
                const float4 g0 = a.guides[2 * at];
                float4 g1 = a.guides[2 * at + 1];
                if constexpr (LENS) g1.w = dn_coc(__float_as_int(g0.w), g1.w, a.cocK, a.focal);
                sG0[i] = g0;
                sG1[i] = g1;
                sC[i] = c;
            }
        }
        __syncthreads();
    }
    if (px >= a.width || py >= a.height) return;
    const size_t center = (size_t)py * a.width + px;
    const int lc = (ly + HALO) * LW + lx + HALO;
    const float4 g0p = S ? sG0[lc] : a.guides[2 * center];
    const float4 g1p = S ? sG1[lc] : a.guides[2 * center + 1];
    float4 cp = S ? sC[lc] : a.colIn[center];
    float varp = 1.0f; // (fixed mode: the alpha written)
    if constexpr (VARIANCE) varp = S ? sV[lc] : (a.varIn ? a.varIn[center] : cp.w);
    const int idp = __float_as_int(g0p.w);
    float4 out = make_float4(cp.x, cp.y, cp.z, varp);
    if (idp != -1) {
        const float up = S ? cp.w : dn_u(cp.x, cp.y, cp.z);
        const float tp = S && LENS ? a.guides[2 * center + 1].w : g1p.w;
        const float planeDen = a.sigmaPlane * tp;
        float cocp = 0.0f;
        if constexpr (LENS) cocp = S ? g1p.w : dn_coc(idp, tp, a.cocK, a.focal);
        float invp = 0.0f;
        if constexpr (VARIANCE) invp = 1.0f / (a.k2 * varp + 1e-8f);
        float W = 0.0f, Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, Q = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const float kx = dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f);
                const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
                const float hk = kx * ky; // (exact)
                const int qx = px + step * dx, qy = py + step * dy;
                if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) continue;
                const size_t at = (size_t)qy * a.width + qx;
                const int lq = lc + dy * S * LW + dx * S;
                const float4 g0q = S ? sG0[lq] : a.guides[2 * at];
                const int idq = __float_as_int(g0q.w);
                float4 g1q;
                bool relaxed = false;
                if constexpr (LENS) {
                    const float r = (float)(step * ((dx < 0 ? -dx : dx) > (dy < 0 ? -dy : dy) ? (dx < 0 ? -dx : dx) : (dy < 0 ? -dy : dy)));
                    const bool reach = r <= cocp;
                    if (idq != idp && !reach) continue;
                    g1q = S ? sG1[lq] : a.guides[2 * at + 1];
                    if (reach) relaxed = r <= (S ? g1q.w : dn_coc(idq, g1q.w, a.cocK, a.focal));
                    if (idq != idp && !relaxed) continue;
                } else {
                    if (idq != idp) continue;
                    g1q = S ? sG1[lq] : a.guides[2 * at + 1];
                }
                const float4 cq = S ? sC[lq] : a.colIn[at];
                float varq = 0.0f;
                if constexpr (VARIANCE) varq = S ? sV[lq] : (a.varIn ? a.varIn[at] : cq.w);
                float wn, wz;
                dn_guide_weights(g0p, g1p, g0q, g1q, planeDen, a.normalPower, wn, wz);
                if (relaxed) wn = wz = 1.0f; // (w = h * wc)
                const float uq = S ? cq.w : dn_u(cq.x, cq.y, cq.z);
                float c1;
                if constexpr (VARIANCE) {
                    const float du = uq - up;
                    c1 = 1.0f - (du * du) * invp;
                } else {
                    const float da = (uq - up) * a.invSigma;
                    c1 = 1.0f - da * da;
                }
                const float c2 = c1 > 0.0f ? c1 : 0.0f;
                const float wc = c2 * c2;
                const float w = ((hk * wn) * wz) * wc;
                W = W + w;
                Sr = Sr + w * cq.x;
                Sg = Sg + w * cq.y;
                Sb = Sb + w * cq.z;
                if constexpr (VARIANCE) Q = Q + (w * w) * varq;
            }
        }
        if (W > 0.0f) out = make_float4(Sr / W, Sg / W, Sb / W, VARIANCE ? Q / (W * W) : 1.0f);
    }
    if constexpr (VARIANCE)
        if (a.last) out.w = 1.0f;
    a.colOut[center] = out;
}

// the mode's instantiation for the step
template <bool VARIANCE, bool LENS>
void launch_atrous_steps(const AtrousArgs &a, hipStream_t stream)
{
    if (a.step <= 2) {
        const dim3 grid((a.width + 15) / 16, (a.height + 15) / 16);
        if (a.step == 1) hipLaunchKernelGGL((pt_atrous_kernel<1, VARIANCE, LENS>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((pt_atrous_kernel<2, VARIANCE, LENS>), grid, dim3(256), 0, stream, a);
    } else {
        hipLaunchKernelGGL((pt_atrous_kernel<0, VARIANCE, LENS>), dim3((a.width + 63) / 64, (a.height + 3) / 4), dim3(256), 0, stream, a);
    }
}
// (the variance mode's three kernels are instantiated behind stage V: pt_variance_kernel<3> stays the sixth function of the file, and the
// label numbering of its code — which the identity check compares — as it was)
extern template void launch_atrous_steps<true, false>(const AtrousArgs &, hipStream_t);
// (... and the six of LENS behind the temporal stage, at the end of the file)
extern template void launch_atrous_steps<false, true>(const AtrousArgs &, hipStream_t);
extern template void launch_atrous_steps<true, true>(const AtrousArgs &, hipStream_t);

hipError_t launch_atrous(const AtrousArgs &a, hipStream_t stream)
{
    if (a.width < 1 || a.height < 1 || a.step < 1 || (a.lens && !(a.cocK > 0.0f))) return hipErrorInvalidValue;
    if (a.lens) {
        if (a.variance) launch_atrous_steps<true, true>(a, stream);
        else launch_atrous_steps<false, true>(a, stream);
    } else {
        if (a.variance) launch_atrous_steps<true, false>(a, stream);
        else launch_atrous_steps<false, false>(a, stream);
    }
    return hipGetLastError();
}

// iterations = 0: the image itself — RGB copied, alpha = the 1 every observer of the image sees (inside a launch chain alpha carries frame tags)
__global__ void pt_denoise_copy_kernel(const float4 *in, float4 *out, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const float4 c = in[i];
        out[i] = make_float4(c.x, c.y, c.z, 1.0f);
    }
}

hipError_t launch_denoise_copy(const float4 *in, float4 *out, size_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    size_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(pt_denoise_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, in, out, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- variance-guided mode (PT_DENOISE_VARIANCE)
// Stage V: V0(p) = half the mean squared first difference of u over the pixels of p's id in the 7x7 window around p — the
// spatial variance estimate the luminance stop of the variance passes is scaled by.  16x16 tiles, one pixel per lane; (u, id bits) of the
// tile and a halo of 3 towards left / bottom and 4 towards right / top (the +1 of Dx / Dy) staged into LDS: 23 x 23 cells of 8 bytes, u
// divided out once per staged cell.  Cells outside the image hold an id no guide record has, so "outside" and "another id" are one
// comparison.  A lane keeps two window rows of 8 cells in registers (64 ds_read_b64 per pixel); Dx and Dy are formed from them and added
// under selects in the order of the definition (dy outer, dx inner, Dx before Dy).
// R = 3, the window's radius: a template so that the kernel is emitted behind pt_atrous_kernel<S, false, false> and leaves that code as it was.
constexpr int kVarOutsideId = (int)0x80000000;

template <int R>
__global__ __launch_bounds__(256) void pt_variance_kernel(const VarianceArgs a)
{
    static_assert(R == 3, "the definition's 7x7 window");
    constexpr int LW = 23;
    __shared__ float2 sU[LW * LW];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
    const int px = x0 + lx, py = y0 + ly;
    for (int i = tid; i < LW * LW; i += 256) {
        const int qx = x0 - 3 + i % LW, qy = y0 - 3 + i / LW;
        float2 cell = make_float2(0.0f, __int_as_float(kVarOutsideId));
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const size_t at = (size_t)qy * a.width + qx;
            const float4 c = a.colIn[at];
            cell = make_float2(dn_u(c.x, c.y, c.z), a.guides[2 * at].w);
        }
        sU[i] = cell;
    }
    __syncthreads();
    if (px >= a.width || py >= a.height) return;
    const int lc = (ly + 3) * LW + lx + 3;
    const int idp = __float_as_int(sU[lc].y);
    float v = 0.0f;
    if (idp != -1) {
        float n = 0.0f, s = 0.0f;
        float2 cur[8], nxt[8];
#pragma unroll
        for (int k = 0; k < 8; k++) cur[k] = sU[lc - 3 * LW - 3 + k];
#pragma unroll 1
        for (int dy = -3; dy <= 3; dy++) { // (rolled: unrolled, the 98 validity masks are all formed first and spill the scalar registers)
#pragma unroll
            for (int k = 0; k < 8; k++) nxt[k] = sU[lc + (dy + 1) * LW - 3 + k];
#pragma unroll
            for (int k = 0; k < 7; k++) { // q = p + (k - 3, dy)
                const bool visit = __float_as_int(cur[k].y) == idp;
                const bool vx = visit && __float_as_int(cur[k + 1].y) == idp;
                const bool vy = visit && __float_as_int(nxt[k].y) == idp;
                const float ex = cur[k + 1].x - cur[k].x;
                const float Dx = ex * ex;
                n = vx ? n + 1.0f : n;
                s = vx ? s + Dx : s;
                const float ey = nxt[k].x - cur[k].x;
                const float Dy = ey * ey;
                n = vy ? n + 1.0f : n;
                s = vy ? s + Dy : s;
            }
#pragma unroll
            for (int k = 0; k < 8; k++) cur[k] = nxt[k];
        }
        if (n > 0.0f) v = 0.5f * (s / n);
    }
    a.var[(size_t)py * a.width + px] = v;
}

hipError_t launch_variance(const VarianceArgs &a, hipStream_t stream)
{
    if (a.width < 1 || a.height < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_variance_kernel<3>, dim3((a.width + 15) / 16, (a.height + 15) / 16), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template void launch_atrous_steps<true, false>(const AtrousArgs &, hipStream_t);

// ---------------------------------------------------------------------------------------------- temporal stage (pt_denoise_set_temporal)
// I(p) = the image's (C, n) blended with the history set's I reprojected to p: the guide position of p goes through the
// history camera's inverse ray matrix B to a point (fx, fy) of the history image, whose 2x2 neighbours of p's id are weighted by the
// bilinear weight and the a-trous filter's own normal and plane weights (dn_guide_weights), and the weighted mean (colour Hc,
// count m clamped to max_history) is mixed with C by sample counts: I = ((n C + m' Hc) / (n + m'), n + m').  One pixel per lane, 64x4
// tiles as pt_atrous_kernel<0, *, *>: a wavefront is 64 adjacent pixels of one row, so the centre's three 16-byte loads coalesce; the four taps
// are data-dependent gathers — G0 first, G1 and I_h only where the id matches.  Every comparison is false for NaN, so a pixel whose
// projection is not finite passes through.  fx lies in [-1, W) where taps are formed, so x0 = floor(fx) fits an int and every tap is
// bounds-checked before its load.
// TAPS = 2, the footprint's width: a template so that the kernel is emitted behind the others and leaves their code as it was.
template <int TAPS>
__global__ __launch_bounds__(256) void pt_temporal_kernel(const TemporalArgs a)
{
    static_assert(TAPS == 2, "the definition's 2x2 bilinear footprint");
    const int tid = threadIdx.x;
    const int px = blockIdx.x * 64 + (tid & 63), py = blockIdx.y * 4 + (tid >> 6);
    if (px >= a.width || py >= a.height) return;
    const size_t center = (size_t)py * a.width + px;
    const float4 cp = a.colIn[center];
    float4 out = make_float4(cp.x, cp.y, cp.z, a.n);
    if (a.histImage) { // (uniform: a valid history set)
        const float4 g0p = a.guides[2 * center];
        const float4 g1p = a.guides[2 * center + 1];
        const int idp = __float_as_int(g0p.w);
        const float dx = g0p.x - a.O[0], dy = g0p.y - a.O[1], dz = g0p.z - a.O[2];
        const float x = (a.B[0] * dx + a.B[1] * dy) + a.B[2] * dz;
        const float y = (a.B[3] * dx + a.B[4] * dy) + a.B[5] * dz;
        const float z = (a.B[6] * dx + a.B[7] * dy) + a.B[8] * dz;
        const float fw = (float)a.width, fh = (float)a.height;
        const float fx = ((x / z) * 0.5f + 0.5f) * fw - 0.5f;
        const float fy = ((y / z) * 0.5f + 0.5f) * fh - 0.5f;
        if (idp != -1 && z > 0.0f && fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh) {
            const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
            const float ax = fx - flx, ay = fy - fly;
            const int x0 = (int)flx, y0 = (int)fly;
            const float planeDen = a.sigmaPlane * g1p.w;
            float Wh = 0.0f, Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, Mh = 0.0f;
#pragma unroll
            for (int j = 0; j < TAPS; j++) {
#pragma unroll
                for (int i = 0; i < TAPS; i++) {
                    const int qx = x0 + i, qy = y0 + j;
                    if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) continue;
                    const size_t at = (size_t)qy * a.width + qx;
                    const float4 g0q = a.histGuides[2 * at];
                    if (__float_as_int(g0q.w) != idp) continue;
                    const float4 g1q = a.histGuides[2 * at + 1];
                    const float4 hq = a.histImage[at];
                    const float bw = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                    float wn, wz;
                    dn_guide_weights(g0p, g1p, g0q, g1q, planeDen, a.normalPower, wn, wz);
                    const float w = (bw * wn) * wz;
                    Wh = Wh + w;
                    Sr = Sr + w * hq.x;
                    Sg = Sg + w * hq.y;
                    Sb = Sb + w * hq.z;
                    Mh = Mh + w * hq.w;
                }
            }
            if (Wh > 0.0f) {
                const float m = Mh / Wh;
                const float mc = m < a.maxHistory ? m : a.maxHistory;
                const float den = a.n + mc;
                if (den > 0.0f)
                    out = make_float4((a.n * cp.x + mc * (Sr / Wh)) / den, (a.n * cp.y + mc * (Sg / Wh)) / den,
                                      (a.n * cp.z + mc * (Sb / Wh)) / den, den);
            }
        }
    }
    a.out[center] = out;
}

hipError_t launch_temporal(const TemporalArgs &a, hipStream_t stream)
{
    if (a.width < 1 || a.height < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_temporal_kernel<2>, dim3((a.width + 63) / 64, (a.height + 3) / 4), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- lens mode (pt_denoise_set_lens)
// The guide records of the pixel-centre pinhole ray (pinhole_ray) instead of sample 0: the same fields by the same rules — id and t as
// pt_first_hit_pinhole_kernel writes them, P = origin + direction * t in two roundings per component — and a.frame is not read.
// PINHOLE = true: a template so that the kernel is emitted behind the others and leaves their code (its label numbering) as it was;
// sample 0 is pt_guides_kernel.
template <bool PINHOLE>
__global__ __launch_bounds__(256) void pt_guides_ray_kernel(const FrameArgs a, float4 *guides)
{
    static_assert(PINHOLE, "the guides of sample 0 are pt_guides_kernel's");
    SceneLds sc = stage_scene(a);
    const int tid = threadIdx.x;
    const int ns = a.numSpheres, nc = a.numCuboids;
    float4 *ids = g_lds + scene_lds_bytes(ns, nc, 0, false) / sizeof(float4);
    for (int i = tid; i < ns + nc; i += 256) ids[4 * i] = make_float4((float)(i < ns ? i : kFirstHitCuboidBase + (i - ns)), 0.0f, 0.0f, 0.0f);
    __syncthreads();
    sc.mat = ids;
    const int b = xcd_band_id(blockIdx.x, gridDim.x);
    const int wave = tid >> 6, lane = tid & 63;
    const int tile = b * 4 + wave;
    if (tile >= a.tilesX * a.tilesY) return;
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
    float4 g0 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    float4 g1 = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
    if (hit) {
        g0 = make_float4(rd.x * h.T + ro.x, rd.y * h.T + ro.y, rd.z * h.T + ro.z, __int_as_float((int)h.m.albedo.x));
        g1 = make_float4(h.normal.x, h.normal.y, h.normal.z, h.T);
    }
    const size_t at = (size_t)ly * a.width + px;
    guides[2 * at] = g0;
    guides[2 * at + 1] = g1;
}

static void launch_guides_pinhole(const FrameArgs &a, float4 *guides, int tiles, size_t lds, hipStream_t stream)
{
    hipLaunchKernelGGL(pt_guides_ray_kernel<true>, dim3((tiles + 3) / 4), dim3(256), lds, stream, a, guides);
}

template void launch_atrous_steps<false, true>(const AtrousArgs &, hipStream_t);
template void launch_atrous_steps<true, true>(const AtrousArgs &, hipStream_t);

// ---------------------------------------------------------------------------------------------- object tracking (pt_denoise_set_object_tracking)
// pt_temporal_kernel<2> for a render whose scene differs from the history's: the object map entry of p's id says where the
// history of p is — KEEP: at P_p, MOVED: at P' = a * P_p + b (two roundings per component: the object's own translation / resize),
// DROP: nowhere, the pixel passes through — and P' stands in for P_p in the projection and in the plane term of every tap; everything
// else (normal weight, planeDen = sigma_plane * t_p, bilinear weights, tap order, id test, blend) is that kernel's, a.maxHistory the cap
// of a tracked render.  Same shape: 64x4 tiles, one pixel per lane.  The map (10,240 B) is gathered from memory, not staged in LDS: a
// lane needs one 16-byte entry half (the state and a) and the second (b) only where its object moved, a wavefront — 64 adjacent pixels
// of one row — sees a handful of ids, so the gather touches a few cache lines of a table that stays resident in the CU's 32 KiB L1;
// staging would load 640 float4 per 256 pixels (2.5 loads, 2.5 LDS writes and a barrier per lane) to save at most two loads per lane.
// TAPS = 2 as there: a template so that the kernel is emitted behind the others and leaves their code as it was.
template <int TAPS>
__global__ __launch_bounds__(256) void pt_temporal_tracked_kernel(const TemporalArgs a, const float4 *objectMap)
{
    static_assert(TAPS == 2, "the definition's 2x2 bilinear footprint");
    const int tid = threadIdx.x;
    const int px = blockIdx.x * 64 + (tid & 63), py = blockIdx.y * 4 + (tid >> 6);
    if (px >= a.width || py >= a.height) return;
    const size_t center = (size_t)py * a.width + px;
    const float4 cp = a.colIn[center];
    float4 out = make_float4(cp.x, cp.y, cp.z, a.n);
    const float4 g0p = a.guides[2 * center];
    const int idp = __float_as_int(g0p.w);
    if ((unsigned)idp < (unsigned)kObjectMapEntries) { // (a miss, id -1, reads no entry; no guide record holds another id)
        const float4 ma = objectMap[2 * idp];
        const int state = __float_as_int(ma.w);
        if (state == kTrackKeep || state == kTrackMoved) {
            float4 g0t = g0p; // (P', id)
            if (state == kTrackMoved) {
                const float4 mb = objectMap[2 * idp + 1];
                g0t.x = ma.x * g0p.x + mb.x;
                g0t.y = ma.y * g0p.y + mb.y;
                g0t.z = ma.z * g0p.z + mb.z;
            }
            const float4 g1p = a.guides[2 * center + 1];
            const float dx = g0t.x - a.O[0], dy = g0t.y - a.O[1], dz = g0t.z - a.O[2];
            const float x = (a.B[0] * dx + a.B[1] * dy) + a.B[2] * dz;
            const float y = (a.B[3] * dx + a.B[4] * dy) + a.B[5] * dz;
            const float z = (a.B[6] * dx + a.B[7] * dy) + a.B[8] * dz;
            const float fw = (float)a.width, fh = (float)a.height;
            const float fx = ((x / z) * 0.5f + 0.5f) * fw - 0.5f;
            const float fy = ((y / z) * 0.5f + 0.5f) * fh - 0.5f;
            if (z > 0.0f && fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh) {
                const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
                const float ax = fx - flx, ay = fy - fly;
                const int x0 = (int)flx, y0 = (int)fly;
                const float planeDen = a.sigmaPlane * g1p.w;
                float Wh = 0.0f, Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, Mh = 0.0f;
#pragma unroll
                for (int j = 0; j < TAPS; j++) {
#pragma unroll
                    for (int i = 0; i < TAPS; i++) {
                        const int qx = x0 + i, qy = y0 + j;
                        if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) continue;
                        const size_t at = (size_t)qy * a.width + qx;
                        const float4 g0q = a.histGuides[2 * at];
                        if (__float_as_int(g0q.w) != idp) continue;
                        const float4 g1q = a.histGuides[2 * at + 1];
                        const float4 hq = a.histImage[at];
                        const float bw = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                        float wn, wz;
                        dn_guide_weights(g0t, g1p, g0q, g1q, planeDen, a.normalPower, wn, wz); // (the plane term: N_p . (P_h(q) - P'))
                        const float w = (bw * wn) * wz;
                        Wh = Wh + w;
                        Sr = Sr + w * hq.x;
                        Sg = Sg + w * hq.y;
                        Sb = Sb + w * hq.z;
                        Mh = Mh + w * hq.w;
                    }
                }
                if (Wh > 0.0f) {
                    const float m = Mh / Wh;
                    const float mc = m < a.maxHistory ? m : a.maxHistory;
                    const float den = a.n + mc;
                    if (den > 0.0f)
                        out = make_float4((a.n * cp.x + mc * (Sr / Wh)) / den, (a.n * cp.y + mc * (Sg / Wh)) / den,
                                          (a.n * cp.z + mc * (Sb / Wh)) / den, den);
                }
            }
        }
    }
    a.out[center] = out;
}

hipError_t launch_temporal_tracked(const TemporalArgs &a, const float4 *objectMap, hipStream_t stream)
{
    if (a.width < 1 || a.height < 1 || !a.histImage || !a.histGuides || !objectMap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pt_temporal_tracked_kernel<2>, dim3((a.width + 63) / 64, (a.height + 3) / 4), dim3(256), 0, stream, a, objectMap);
    return hipGetLastError();
}

} // namespace pt
