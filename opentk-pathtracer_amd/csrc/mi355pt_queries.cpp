// mi355pt_queries.cpp — the entry points of the C ABI (include/mi355pt.h) that ask something about the image without rendering it: the
// first-hit query (pt_first_hit_*, pt_pick) and the preview denoiser (pt_denoise_*) — and, next to them, adaptive sampling (pt_adaptive_*),
// which does render but only through a kernel of its own.  All stand behind bind_device / join_stripes and use nothing else of the launch
// pipeline of mi355pt_launch.cpp (adaptive sampling: its kernel argument, plain_frame_args); their buffers belong to a size and a tiling
// (free_first_hit, free_denoise, free_adaptive).
#include "pt_renderer.hpp"
#include "pt_object_map.hpp"

#include <cmath>
#include <cstring>
#include <vector>

using ptimpl::bind_device;
using ptimpl::ensure_rgba8;
using ptimpl::fail;
using ptimpl::join_stripes;

namespace ptimpl {

int free_first_hit(pt_handle h)
{
    if (!h->dFirstHit) return PT_OK;
    PT_HIP(h, hipStreamSynchronize(h->stream)); // (a queued pt_first_hit_render may still write it)
    PT_HIP(h, hipFree(h->dFirstHit));
    h->dFirstHit = nullptr;
    return PT_OK;
}

int free_denoise(pt_handle h)
{
    pt_renderer::Denoiser &d = h->denoise;
    d.result = -1;
    d.varianceValid = false;
    d.integratedValid = d.historyUsed = false;
    d.mapValid = d.mapTracked = false;
    d.momentsK = 0; // (the moment set belongs to a size and a tiling)
    d.noiseValid = d.blended = false;
    for (pt_renderer::DenoiseSet &set : d.set) set.valid = false;
    if (!d.allocated()) return PT_OK;
    PT_HIP(h, hipStreamSynchronize(h->stream)); // (a queued pt_denoise_render may still write them)
    PT_HIP(h, d.release());
    return PT_OK;
}

int free_adaptive(pt_handle h)
{
    pt_renderer::Adaptive &ad = h->adaptive;
    ad.started = false; // (the state belongs to a size and a tiling)
    if (!ad.dTiles && !ad.dStats) return PT_OK;
    PT_HIP(h, hipStreamSynchronize(h->stream)); // (a queued pt_adaptive_render may still write them)
    hipError_t first = hipSuccess;
    if (ad.dTiles) first = hipFree(ad.dTiles);
    ad.dTiles = nullptr;
    if (ad.dStats) {
        const hipError_t e = hipFree(ad.dStats);
        if (first == hipSuccess) first = e;
    }
    ad.dStats = nullptr;
    PT_HIP(h, first);
    return PT_OK;
}

} // namespace ptimpl

extern "C" {

// ---- first-hit query (pt_first_hit.hip): what src/Render/Gui.cs:223-233 -> src/MainWindow.cs:302-318 answer on the CPU, for the ray the
// integrator traces.  Reads the camera shadow, the scene blob and the parameters; touches neither the accumulation image, the frame
// counter, the cached tile masks, the environment nor an arithmetic switch.
static_assert(pt::kFirstHitCuboidBase == PT_MAX_SPHERES, "first-hit ids: cuboid j is PT_MAX_SPHERES + j");

// the kernel argument of a first-hit launch over this handle's rows (only the fields stage_scene, primary_ray and global_row read)
static void first_hit_args(pt_handle h, pt::FrameArgs &a, int frame_index)
{
    std::memset(&a, 0, sizeof a);
    std::memcpy(a.invProj, h->basic, 64);
    std::memcpy(a.invView, h->basic + 64, 64);
    std::memcpy(a.viewPos, h->basic + 128, 12);
    a.focalLength = h->focalLength;
    a.apertureDiameter = h->apertureDiameter;
    a.width = h->width;
    a.height = h->height;
    a.invW = 1.0f / (float)h->width; // (as fill_frame_args)
    a.invH = 1.0f / (float)h->height;
    a.y0 = h->y0;
    a.rows = h->rows;
    a.bandRows = h->bandRows;
    a.bandWorld = h->bandWorld;
    a.bandRank = h->bandRank;
    a.numSpheres = h->numSpheres;
    a.numCuboids = h->numCuboids;
    a.rayDepth = 1;
    a.spp = 1;
    a.batchFrames = 1;
    a.frame = frame_index;
    a.objects = h->dObjects; // (the block AND sphereGeom behind it, pt_kernels.hpp kSphereGeomOffset: `objects` always names an allocation of 26,624 + 4,096 bytes)
    a.tilesX = h->tilesX();
    a.tilesY = h->tilesY();
}

PT_API int pt_first_hit_set_ray(pt_handle h, int mode)
{
    PT_CHECK_HANDLE(h);
    if (mode != PT_RAY_SAMPLE0 && mode != PT_RAY_PINHOLE) return fail(h, PT_E_BAD_ARGUMENT, "mode must be PT_RAY_SAMPLE0 or PT_RAY_PINHOLE");
    PT_FAN_OUT(h, pt_first_hit_set_ray(part, mode));
    h->firstHitRay = mode; // (read by the next pt_first_hit_render / pt_pick; what is queued already took its value)
    return PT_OK;
}

PT_API int pt_first_hit_render(pt_handle h, int frame_index)
{
    PT_CHECK_HANDLE(h);
    if (frame_index < 0) return fail(h, PT_E_BAD_ARGUMENT, "frame_index must be >= 0");
    PT_FAN_OUT(h, pt_first_hit_render(part, frame_index));
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc; // (pending frames are launched, an open frame-fed launch is closed: like every non-render entry point)
    if (!h->dFirstHit) PT_HIP(h, hipMalloc((void **)&h->dFirstHit, h->tilePixels() * 2 * sizeof(float4)));
    pt::FrameArgs a;
    first_hit_args(h, a, frame_index);
    PT_HIP(h, pt::launch_first_hit(a, h->dFirstHit, -1, h->firstHitRay == PT_RAY_PINHOLE, h->stream));
    return PT_OK;
}

PT_API int pt_first_hit_read(pt_handle h, void *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (!dst) return fail(h, PT_E_BAD_ARGUMENT, "dst == NULL");
    const size_t rowBytes = (size_t)h->width * 32;
    if (row_pitch_bytes == 0) row_pitch_bytes = rowBytes;
    if (row_pitch_bytes < rowBytes) return fail(h, PT_E_BAD_ARGUMENT, "row pitch smaller than a row");
    if (h->isGroup()) return ptimpl::group_first_hit_read(h, dst, row_pitch_bytes);
    if (!h->dFirstHit) return fail(h, PT_E_BAD_ARGUMENT, "no pt_first_hit_render since the last pt_set_size / pt_set_tile / pt_set_interleaved_tile");
    if (int rc = bind_device(h)) return rc;
    PT_HIP(h, hipMemcpy2DAsync(dst, row_pitch_bytes, h->dFirstHit, rowBytes, rowBytes, (size_t)h->rows, hipMemcpyDeviceToHost, h->stream));
    PT_HIP(h, hipStreamSynchronize(h->stream));
    return PT_OK;
}

PT_API int pt_first_hit_device_ptr(pt_handle h, void **out, size_t *bytes)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) return fail(h, PT_E_BAD_ARGUMENT, "pt_first_hit_device_ptr is not available on a group handle");
    if (!h->dFirstHit) return fail(h, PT_E_BAD_ARGUMENT, "no pt_first_hit_render since the last pt_set_size / pt_set_tile / pt_set_interleaved_tile");
    if (out) *out = h->dFirstHit;
    if (bytes) *bytes = h->tilePixels() * 2 * sizeof(float4);
    return PT_OK;
}

PT_API int pt_pick(pt_handle h, int x, int y, int frame_index, int *out_id, float *out_t, float out_origin[3], float out_dir[3])
{
    PT_CHECK_HANDLE(h);
    if (!out_id) return fail(h, PT_E_BAD_ARGUMENT, "out_id == NULL");
    if (frame_index < 0) return fail(h, PT_E_BAD_ARGUMENT, "frame_index must be >= 0");
    if (x < 0 || x >= h->width || y < 0 || y >= h->height) return fail(h, PT_E_OUT_OF_RANGE, "pixel outside the image");
    if (h->isGroup()) return ptimpl::group_pick(h, x, y, frame_index, out_id, out_t, out_origin, out_dir);
    // image row -> row inside this handle's storage (the inverse of the kernels' global_row)
    int ly;
    if (h->bandRows == 0) {
        ly = y - h->y0;
    } else {
        const int band = y / h->bandRows;
        ly = band % h->bandWorld == h->bandRank ? (band / h->bandWorld) * h->bandRows + y % h->bandRows : -1;
    }
    if (ly < 0 || ly >= h->rows) return fail(h, PT_E_OUT_OF_RANGE, "this handle does not own the pixel's row (pt_set_tile / pt_set_interleaved_tile)");
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc;
    if (!h->dPick) PT_HIP(h, hipMalloc((void **)&h->dPick, 64 * 2 * sizeof(float4)));
    pt::FrameArgs a;
    first_hit_args(h, a, frame_index);
    PT_HIP(h, pt::launch_first_hit(a, h->dPick, (ly >> 3) * a.tilesX + (x >> 3), h->firstHitRay == PT_RAY_PINHOLE, h->stream));
    float rec[8];
    PT_HIP(h, hipMemcpyAsync(rec, h->dPick + 2 * ((ly & 7) * 8 + (x & 7)), sizeof rec, hipMemcpyDeviceToHost, h->stream));
    PT_HIP(h, hipStreamSynchronize(h->stream));
    std::memcpy(out_id, &rec[7], sizeof(int));
    if (out_t) *out_t = rec[3];
    if (out_origin) std::memcpy(out_origin, &rec[0], 12);
    if (out_dir) std::memcpy(out_dir, &rec[4], 12);
    return PT_OK;
}

// ---- preview denoiser (pt_denoise.hip): guides from the integrator's own primary ray + an edge-avoiding a-trous filter of
// the accumulation image, for the first frames after the reset that every camera move and GUI edit causes (MainWindow.cs:49-63); the
// result goes through the tone map of ScreenEffect.cs:29-37.  Reads the image (RGB), the camera shadow, the scene blob and the parameters;
// touches neither the accumulation image, the frame counter, the environment nor an arithmetic switch.
static int denoise_owner(pt_handle h)
{
    if (h->isGroup()) return fail(h, PT_E_BAD_ARGUMENT, "the denoiser is not available on a group handle");
    if (h->rows != h->height || h->bandRows != 0)
        return fail(h, PT_E_BAD_ARGUMENT, "the denoiser needs a handle that owns the whole image (pt_set_tile / pt_set_interleaved_tile in force)");
    return PT_OK;
}

// The camera of a set: the ray generator is linear in the NDC point, wd = A (ndcx, ndcy, 1) with A = [a b c] formed
// from the blob's InvProjection m and InvView v (compute.glsl:352-357 as primary_ray_cam evaluates it); B = A^-1, formed and inverted in
// double and rounded to binary32 once, O = InvView's translation.  false: A is singular or B not finite.
static bool denoise_set_camera(const unsigned char *basic, float B[9], float O[3])
{
    float m[16], v[16];
    std::memcpy(m, basic, 64);
    std::memcpy(v, basic + 64, 64);
    double A[3][3];
    for (int r = 0; r < 3; r++) {
        A[r][0] = (double)v[r] * m[0] + (double)v[4 + r] * m[1];
        A[r][1] = (double)v[r] * m[4] + (double)v[4 + r] * m[5];
        A[r][2] = -((double)v[r] * m[8] + (double)v[4 + r] * m[9]) - (double)v[8 + r];
        O[r] = v[12 + r];
    }
    double C[3][3]; // cofactors: A^-1 = C^T / det
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            C[i][j] = A[i1][j1] * A[i2][j2] - A[i1][j2] * A[i2][j1];
        }
    const double det = A[0][0] * C[0][0] + A[0][1] * C[0][1] + A[0][2] * C[0][2];
    bool ok = std::isfinite(det) && det != 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            B[3 * i + j] = (float)(C[j][i] / det);
            ok = ok && std::isfinite(B[3 * i + j]);
        }
    return ok;
}

// The blur radius per unit of |t - F| / t, in pixels at the image centre: coc_scale (A / 2) / F H / (2 |invProj[5]|) in
// double from the binary32 inputs, rounded once; 0 = no tap is relaxed (no lens, coc_scale 0, or not finite).
static float denoise_coc_k(pt_handle h)
{
    float m5;
    std::memcpy(&m5, h->basic + 5 * sizeof(float), sizeof m5);
    const double A = h->apertureDiameter, F = h->focalLength, s = h->denoise.cocScale;
    if (!(A > 0.0) || !(F > 0.0) || s == 0.0) return 0.0f;
    const float k = (float)(s * (A / 2.0) / F * (double)h->height / (2.0 * std::fabs((double)m5)));
    return std::isfinite(k) ? k : 0.0f;
}

// The object map of a temporal render with tracking on (pt_object_map.hpp): the history set's scene snapshot against the
// scene in force.  -> the tracked kernel has to run
static_assert(pt::kObjectMapEntries == ptmap::kEntries && ptmap::kMaxSpheres == PT_MAX_SPHERES && ptmap::kMaxCuboids == PT_MAX_CUBOIDS, "object map: one entry per guide id");
static_assert(pt::kTrackKeep == PT_TRACK_KEEP && pt::kTrackMoved == PT_TRACK_MOVED && pt::kTrackDrop == PT_TRACK_DROP, "object map states");
static_assert(ptmap::kKeep == PT_TRACK_KEEP && ptmap::kMoved == PT_TRACK_MOVED && ptmap::kDrop == PT_TRACK_DROP, "object map states");
static bool denoise_object_map(const pt_renderer::DenoiseSet &hist, const unsigned char *scene, int ns, int nc, unsigned char *map)
{
    return ptmap::build(hist.scene, hist.numSpheres, hist.numCuboids, scene, ns, nc, map);
}

// The moment set of pt_denoise_set_moments (pt_denoise_moments.hip) is forgotten when it was made in another reset epoch,
// under another spp, or of more samples than the image holds now (a resize or re-tiling forgets it in free_denoise)
static bool moments_forgotten(pt_handle h)
{
    const pt_renderer::Denoiser &d = h->denoise;
    return d.momentsK > 0 && (d.momentsEpoch != h->resetEpoch || d.momentsSpp != h->spp || (long long)h->frame * h->spp < d.momentsN);
}

// Stage M of a full render with the switch on: looks at the accumulation image — an observation unless it holds no sample (n = 0) or
// what the last observation saw (n = nPrev) — and leaves Vm in dNoise.  n, nPrev and n - nPrev are converted to binary32 here.
static int denoise_observe(pt_handle h, const float4 *guides)
{
    pt_renderer::Denoiser &d = h->denoise;
    const size_t pixels = h->tilePixels();
    if (!d.dMoments) PT_HIP(h, hipMalloc((void **)&d.dMoments, pixels * sizeof(float2)));
    if (!d.dNoise) PT_HIP(h, hipMalloc((void **)&d.dNoise, pixels * sizeof(float)));
    if (!d.dVar0) PT_HIP(h, hipMalloc((void **)&d.dVar0, pixels * sizeof(float)));
    if (moments_forgotten(h)) d.momentsK = 0;
    const long long n = (long long)h->frame * h->spp;
    const bool observe = n != 0 && !(d.momentsK > 0 && n == d.momentsN);
    pt::MomentsArgs m;
    m.colIn = h->accum();
    m.guides = guides;
    m.state = d.dMoments;
    m.noise = d.dNoise;
    m.pixels = pixels;
    m.observe = !observe ? 0 : d.momentsK == 0 ? 1 : 2;
    m.nf = (float)n;
    m.npf = (float)d.momentsN;
    m.w = (float)(n - d.momentsN);
    if (observe) {
        d.momentsK += 1;
        d.momentsN = n;
        d.momentsSpp = h->spp;
        d.momentsEpoch = h->resetEpoch;
    }
    m.estimate = d.momentsK >= 2;
    m.km1 = (float)(d.momentsK - 1);
    PT_HIP(h, pt::launch_moments(m, h->stream));
    d.noiseValid = true;
    return PT_OK;
}

// stage kDenoiseAll: everything; -1: the guides only; kDenoiseStageV: stage V of the variance mode only; kDenoiseStageT: the temporal
// kernel only; i >= 0: pass i only (pt_debug_denoise_stage, for timing)
constexpr int kDenoiseStageV = -2, kDenoiseAll = -3, kDenoiseStageT = -4;
static int denoise_run(pt_handle h, int guide_frame_index, int stage)
{
    if (int rc = bind_device(h)) return rc;
    // (the preamble of pt_postprocess_device: pending frames are launched, an open frame-fed launch is closed, an abandoned hand-over is repaired)
    if (int rc = join_stripes(h)) return rc;
    pt_renderer::Denoiser &d = h->denoise;
    const size_t pixels = h->tilePixels();
    const bool variance = d.mode == PT_DENOISE_VARIANCE;
    const bool temporal = d.temporal != 0;
    const bool lens = d.lens != 0;
    const float cocK = lens ? denoise_coc_k(h) : 0.0f;
    if (!temporal && !d.dGuides) PT_HIP(h, hipMalloc((void **)&d.dGuides, pixels * 2 * sizeof(float4)));
    for (float4 *&img : d.dImage)
        if (!img) PT_HIP(h, hipMalloc((void **)&img, pixels * sizeof(float4)));
    if (variance && !d.dVariance) PT_HIP(h, hipMalloc((void **)&d.dVariance, pixels * sizeof(float)));
    if (temporal) {
        for (pt_renderer::DenoiseSet &set : d.set) {
            if (!set.image) PT_HIP(h, hipMalloc((void **)&set.image, pixels * sizeof(float4)));
            if (!set.guides) PT_HIP(h, hipMalloc((void **)&set.guides, pixels * 2 * sizeof(float4)));
        }
        // a current set of an earlier reset epoch becomes the history: a pointer swap (a timing stage works between the sets as they are)
        if (stage == kDenoiseAll && d.set[d.current].valid && d.set[d.current].epoch != h->resetEpoch) {
            d.current ^= 1;
            d.set[d.current].valid = false; // (until this render has made it)
        }
    }
    pt_renderer::DenoiseSet &cur = d.set[d.current];
    const pt_renderer::DenoiseSet &hist = d.set[d.current ^ 1];
    float4 *const guides = temporal ? cur.guides : d.dGuides; // the guides of this render ...
    const float4 *const first = temporal ? cur.image : h->accum(); // ... and C_0, the input of stage V and of pass 0
    if (stage == kDenoiseAll || stage == -1) {
        pt::FrameArgs a;
        first_hit_args(h, a, guide_frame_index);
        PT_HIP(h, pt::launch_guides(a, guides, lens, h->stream));
        if (stage == -1) return PT_OK;
    }
    if (stage == kDenoiseAll) {
        d.noiseValid = d.blended = false;
        if (d.moments)
            if (int rc = denoise_observe(h, guides)) return rc;
    }
    if (temporal && (stage == kDenoiseAll || stage == kDenoiseStageT)) {
        pt::TemporalArgs t;
        t.colIn = h->accum();
        t.guides = guides;
        t.histImage = hist.valid ? hist.image : nullptr;
        t.histGuides = hist.guides;
        t.out = cur.image;
        t.width = h->width;
        t.height = h->rows;
        t.n = (float)((long long)h->frame * h->spp);
        t.maxHistory = (float)d.maxHistory;
        std::memcpy(t.B, hist.B, sizeof t.B);
        std::memcpy(t.O, hist.O, sizeof t.O);
        t.sigmaPlane = d.sigmaPlane;
        t.normalPower = d.normalPower;
        // object tracking: a full render builds the map and, where the scene differs from the history's, uploads it (stream-ordered, as
        // pt_upload_game_objects uploads the blob: a pageable source is staged before the call returns); a timing stage runs the kernel
        // the last full render selected, with the map that render left on the device
        if (stage == kDenoiseAll) {
            d.mapValid = d.tracking != 0 && hist.valid;
            d.mapTracked = d.mapValid && denoise_object_map(hist, h->objectsShadow, h->numSpheres, h->numCuboids, d.objectMap);
            if (d.mapTracked) {
                if (!d.dObjectMap) PT_HIP(h, hipMalloc((void **)&d.dObjectMap, sizeof d.objectMap));
                PT_HIP(h, hipMemcpyAsync(d.dObjectMap, d.objectMap, sizeof d.objectMap, hipMemcpyHostToDevice, h->stream));
            }
        }
        if (d.tracking != 0 && d.mapTracked && hist.valid && d.dObjectMap) {
            if (d.editMaxHistory != 0 && d.editMaxHistory < d.maxHistory) t.maxHistory = (float)d.editMaxHistory; // the cap of a tracked render
            PT_HIP(h, pt::launch_temporal_tracked(t, d.dObjectMap, h->stream));
        } else {
            PT_HIP(h, pt::launch_temporal(t, h->stream));
        }
        if (stage == kDenoiseStageT) return PT_OK;
        cur.valid = denoise_set_camera(h->basic, cur.B, cur.O);
        cur.epoch = h->resetEpoch;
        std::memcpy(cur.scene, h->objectsShadow, sizeof cur.scene); // (whatever the tracking switch says: a later render may compare against it)
        cur.numSpheres = h->numSpheres;
        cur.numCuboids = h->numCuboids;
        d.historyUsed = hist.valid;
    }
    if (stage == kDenoiseAll) {
        d.integratedValid = temporal;
        if (!temporal) d.mapValid = d.mapTracked = false;
    }
    const int n = d.iterations;
    if (n == 0 && stage == kDenoiseAll) PT_HIP(h, pt::launch_denoise_copy(first, d.dImage[0], pixels, h->stream));
    if (variance && n > 0 && (stage == kDenoiseAll || stage == kDenoiseStageV)) {
        pt::VarianceArgs v;
        v.colIn = first;
        v.guides = guides;
        v.var = d.dVariance;
        v.width = h->width;
        v.height = h->rows;
        PT_HIP(h, pt::launch_variance(v, h->stream));
    }
    // stage B: the measured variance blended with V0 into var_0, which pass 0 reads in place of V0 (a timing stage reads what the last
    // full render left).  Not with the temporal stage on: the integrated image's noise is not the accumulation image's
    if (stage == kDenoiseAll && d.noiseValid && variance && n > 0 && !temporal && d.momentsK >= 2) {
        pt::MomentsBlendArgs b;
        b.noise = d.dNoise;
        b.guides = guides;
        b.v0 = d.dVariance;
        b.var0 = d.dVar0;
        b.width = h->width;
        b.height = h->rows;
        b.km1 = (float)(d.momentsK - 1);
        b.k0 = (float)d.priorSamples;
        PT_HIP(h, pt::launch_moments_blend(b, h->stream));
        d.blended = true;
    }
    // stage A: on a live adaptive state (where stage M never ran: pt_denoise_render refuses the moments there) the sampler's own
    // per-pixel estimate e and the tile records take Vm's place — stream-ordered behind the passes already queued, reading the state as
    // they leave it and writing dVar0 only
    if (stage == kDenoiseAll && d.adaptiveNoise && variance && n > 0 && !temporal && h->adaptiveLive() && h->adaptive.dTiles && h->adaptive.dStats) {
        if (!d.dVar0) PT_HIP(h, hipMalloc((void **)&d.dVar0, pixels * sizeof(float)));
        pt::AdaptiveBlendArgs b;
        b.stats = h->adaptive.dStats;
        b.tiles = h->adaptive.dTiles;
        b.guides = guides;
        b.v0 = d.dVariance;
        b.var0 = d.dVar0;
        b.width = h->width;
        b.height = h->rows;
        b.tilesX = h->tilesX();
        b.k0 = (float)d.adaptivePrior;
        PT_HIP(h, pt::launch_adaptive_blend(b, h->stream));
        d.blended = true;
    }
    const bool blended = d.blended && variance && !temporal && d.dVar0;
    for (int i = 0; i < n && stage != kDenoiseStageV; i++) {
        if (stage >= 0 && i != stage) continue;
        pt::AtrousArgs t;
        t.colIn = i == 0 ? first : d.dImage[(i - 1) & 1];
        t.guides = guides;
        t.colOut = d.dImage[i & 1];
        t.width = h->width;
        t.height = h->rows;
        t.step = 1 << i;
        t.sigmaPlane = d.sigmaPlane;
        t.normalPower = d.normalPower;
        // the luminance stop and the alpha channel: what the modes differ in (each kernel reads its own fields only)
        t.variance = variance;
        t.invSigma = variance ? 0.0f : 1.0f / (d.sigmaColor * std::ldexp(1.0f, -i));
        t.k2 = variance ? d.sigmaVariance * d.sigmaVariance : 0.0f;
        t.varIn = variance && i == 0 ? (blended ? d.dVar0 : d.dVariance) : nullptr;
        t.last = variance && i == n - 1;
        t.lens = cocK > 0.0f; // (lens mode with cocK = 0: the pinhole guides under the tap rules of lens = 0)
        t.cocK = cocK;
        t.focal = h->focalLength;
        PT_HIP(h, pt::launch_atrous(t, h->stream));
    }
    if (stage == kDenoiseAll) {
        d.result = n == 0 ? 0 : (n - 1) & 1;
        d.varianceValid = variance && n > 0;
    }
    return PT_OK;
}

PT_API int pt_denoise_set_params(pt_handle h, int iterations, float sigma_color, float sigma_plane, int normal_log2_power)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_owner(h)) return rc;
    if (!std::isfinite(sigma_color) || !std::isfinite(sigma_plane)) return fail(h, PT_E_BAD_ARGUMENT, "sigma_color and sigma_plane must be finite");
    if (iterations < 0 || iterations > 6 || normal_log2_power < 0 || normal_log2_power > 7 || !(sigma_color > 0.0f) || !(sigma_plane > 0.0f))
        return fail(h, PT_E_OUT_OF_RANGE, "iterations 0..6, normal_log2_power 0..7, sigma_color > 0, sigma_plane > 0");
    h->denoise.iterations = iterations; // (read by the next pt_denoise_render; what is queued already took its values)
    h->denoise.sigmaColor = sigma_color;
    h->denoise.sigmaPlane = sigma_plane;
    h->denoise.normalPower = normal_log2_power;
    return PT_OK;
}

PT_API int pt_denoise_set_mode(pt_handle h, int mode, float sigma_variance)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_owner(h)) return rc;
    if (mode != PT_DENOISE_FIXED && mode != PT_DENOISE_VARIANCE) return fail(h, PT_E_BAD_ARGUMENT, "mode must be PT_DENOISE_FIXED or PT_DENOISE_VARIANCE");
    if (!std::isfinite(sigma_variance)) return fail(h, PT_E_BAD_ARGUMENT, "sigma_variance must be finite");
    if (!(sigma_variance > 0.0f)) return fail(h, PT_E_OUT_OF_RANGE, "sigma_variance > 0");
    h->denoise.mode = mode; // (read by the next pt_denoise_render; what is queued already took its values)
    h->denoise.sigmaVariance = sigma_variance;
    return PT_OK;
}

PT_API int pt_denoise_set_lens(pt_handle h, int enable, float coc_scale)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_owner(h)) return rc;
    if (enable != 0 && enable != 1) return fail(h, PT_E_BAD_ARGUMENT, "enable must be 0 or 1");
    if (!std::isfinite(coc_scale)) return fail(h, PT_E_BAD_ARGUMENT, "coc_scale must be finite");
    if (coc_scale < 0.0f) return fail(h, PT_E_OUT_OF_RANGE, "coc_scale >= 0");
    h->denoise.lens = enable; // (read by the next pt_denoise_render; what is queued already took its values)
    h->denoise.cocScale = coc_scale;
    return PT_OK;
}

PT_API int pt_denoise_render(pt_handle h, int guide_frame_index)
{
    PT_CHECK_HANDLE(h);
    if (guide_frame_index < 0) return fail(h, PT_E_BAD_ARGUMENT, "guide_frame_index must be >= 0");
    if (int rc = denoise_owner(h)) return rc;
    if (h->adaptiveLive() && (h->denoise.temporal || h->denoise.moments))
        return fail(h, PT_E_BAD_ARGUMENT, "adaptive accumulation in progress: the temporal stage and the moments rest on frame index x spp (pt_reset first)");
    return denoise_run(h, guide_frame_index, kDenoiseAll);
}

static int denoise_rendered(pt_handle h)
{
    if (int rc = denoise_owner(h)) return rc;
    if (h->denoise.result < 0) return fail(h, PT_E_BAD_ARGUMENT, "no pt_denoise_render since the last pt_set_size / pt_set_tile / pt_set_interleaved_tile");
    return bind_device(h);
}

static int denoise_copy_out(pt_handle h, void *dst, size_t row_pitch_bytes, const void *src, size_t bytesPerPixel)
{
    if (!dst) return fail(h, PT_E_BAD_ARGUMENT, "dst == NULL");
    const size_t rowBytes = (size_t)h->width * bytesPerPixel;
    if (row_pitch_bytes == 0) row_pitch_bytes = rowBytes;
    if (row_pitch_bytes < rowBytes) return fail(h, PT_E_BAD_ARGUMENT, "row pitch smaller than a row");
    PT_HIP(h, hipMemcpy2DAsync(dst, row_pitch_bytes, src, rowBytes, rowBytes, (size_t)h->rows, hipMemcpyDeviceToHost, h->stream));
    PT_HIP(h, hipStreamSynchronize(h->stream));
    return PT_OK;
}

PT_API int pt_denoise_read(pt_handle h, float *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_rendered(h)) return rc;
    return denoise_copy_out(h, dst, row_pitch_bytes, h->denoise.dImage[h->denoise.result], 16);
}

PT_API int pt_denoise_read_guides(pt_handle h, void *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_rendered(h)) return rc;
    return denoise_copy_out(h, dst, row_pitch_bytes, h->denoise.integratedValid ? h->denoise.set[h->denoise.current].guides : h->denoise.dGuides, 32);
}

PT_API int pt_denoise_read_variance(pt_handle h, float *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_rendered(h)) return rc;
    if (!h->denoise.varianceValid)
        return fail(h, PT_E_BAD_ARGUMENT, "the last pt_denoise_render made no variance estimate (PT_DENOISE_FIXED, or iterations = 0)");
    return denoise_copy_out(h, dst, row_pitch_bytes, h->denoise.dVariance, 4);
}

PT_API int pt_denoise_set_temporal(pt_handle h, int enable, int max_history)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_owner(h)) return rc;
    if (enable != 0 && enable != 1) return fail(h, PT_E_BAD_ARGUMENT, "enable must be 0 or 1");
    if (max_history < 1 || max_history > 65535) return fail(h, PT_E_OUT_OF_RANGE, "max_history 1..65535");
    h->denoise.temporal = enable; // (read by the next pt_denoise_render; what is queued already took its values)
    h->denoise.maxHistory = max_history;
    return PT_OK;
}

PT_API int pt_denoise_history_clear(pt_handle h)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_owner(h)) return rc;
    for (pt_renderer::DenoiseSet &set : h->denoise.set) set.valid = false; // (the buffers stay: a queued render may still read them)
    h->denoise.historyUsed = false;
    h->denoise.mapValid = h->denoise.mapTracked = false;
    return PT_OK;
}

PT_API int pt_denoise_set_object_tracking(pt_handle h, int enable, int edit_max_history)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_owner(h)) return rc;
    if (enable != 0 && enable != 1) return fail(h, PT_E_BAD_ARGUMENT, "enable must be 0 or 1");
    if (edit_max_history < 0 || edit_max_history > 65535) return fail(h, PT_E_OUT_OF_RANGE, "edit_max_history 0..65535");
    h->denoise.tracking = enable; // (read by the next pt_denoise_render; what is queued already took its values)
    h->denoise.editMaxHistory = edit_max_history;
    return PT_OK;
}

PT_API int pt_denoise_read_object_map(pt_handle h, void *dst_320x32_bytes, int *out_tracked)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_owner(h)) return rc;
    if (!h->denoise.mapValid)
        return fail(h, PT_E_BAD_ARGUMENT, "the last pt_denoise_render built no object map (temporal stage or tracking off, no history, or nothing rendered since)");
    if (dst_320x32_bytes) std::memcpy(dst_320x32_bytes, h->denoise.objectMap, sizeof h->denoise.objectMap);
    if (out_tracked) *out_tracked = h->denoise.mapTracked ? 1 : 0;
    return PT_OK;
}

PT_API int pt_denoise_read_integrated(pt_handle h, float *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_rendered(h)) return rc;
    if (!h->denoise.integratedValid) return fail(h, PT_E_BAD_ARGUMENT, "the last pt_denoise_render ran with the temporal stage off");
    return denoise_copy_out(h, dst, row_pitch_bytes, h->denoise.set[h->denoise.current].image, 16);
}

PT_API int pt_denoise_read_history(pt_handle h, float *image, void *guides, float out_B[9], float out_O[3])
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_rendered(h)) return rc;
    if (!h->denoise.historyUsed) return fail(h, PT_E_BAD_ARGUMENT, "the last temporal pt_denoise_render had no history");
    const pt_renderer::DenoiseSet &hist = h->denoise.set[h->denoise.current ^ 1];
    if (image)
        if (int rc = denoise_copy_out(h, image, 0, hist.image, 16)) return rc;
    if (guides)
        if (int rc = denoise_copy_out(h, guides, 0, hist.guides, 32)) return rc;
    if (out_B) std::memcpy(out_B, hist.B, sizeof hist.B);
    if (out_O) std::memcpy(out_O, hist.O, sizeof hist.O);
    return PT_OK;
}

PT_API int pt_denoise_set_moments(pt_handle h, int enable, int prior_samples)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_owner(h)) return rc;
    if (enable != 0 && enable != 1) return fail(h, PT_E_BAD_ARGUMENT, "enable must be 0 or 1");
    if (prior_samples < 1 || prior_samples > 65535) return fail(h, PT_E_OUT_OF_RANGE, "prior_samples 1..65535");
    h->denoise.moments = enable; // (read by the next pt_denoise_render; what is queued already took its values)
    h->denoise.priorSamples = prior_samples;
    return PT_OK;
}

// the last pt_denoise_render left a noise map of at least two observations of the image as it still stands
static int denoise_noise_ready(pt_handle h)
{
    if (int rc = denoise_rendered(h)) return rc;
    if (!h->denoise.noiseValid) return fail(h, PT_E_BAD_ARGUMENT, "the last pt_denoise_render ran with pt_denoise_set_moments off");
    if (moments_forgotten(h)) h->denoise.momentsK = 0;
    if (h->denoise.momentsK < 2) return fail(h, PT_E_BAD_ARGUMENT, "fewer than two observations of the image (pt_denoise_render with pt_denoise_set_moments on)");
    return PT_OK;
}

PT_API int pt_denoise_read_noise(pt_handle h, float *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_noise_ready(h)) return rc;
    return denoise_copy_out(h, dst, row_pitch_bytes, h->denoise.dNoise, 4);
}

PT_API int pt_denoise_noise_level(pt_handle h, float *out_mean_variance, int *out_observations, int *out_hit_pixels)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_noise_ready(h)) return rc;
    pt_renderer::Denoiser &d = h->denoise;
    const size_t pixels = h->tilePixels(), blocks = (pixels + 255) / 256;
    if (!d.dNoisePartial) PT_HIP(h, hipMalloc((void **)&d.dNoisePartial, blocks * sizeof(float2)));
    PT_HIP(h, pt::launch_moments_level(d.dNoise, d.integratedValid ? d.set[d.current].guides : d.dGuides, d.dNoisePartial, pixels, h->stream));
    std::vector<float2> partial(blocks);
    PT_HIP(h, hipMemcpyAsync(partial.data(), d.dNoisePartial, blocks * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
    PT_HIP(h, hipStreamSynchronize(h->stream));
    double sum = 0.0;
    long long count = 0;
    for (const float2 &p : partial) { // (in index order)
        int c;
        std::memcpy(&c, &p.y, sizeof c);
        sum += (double)p.x;
        count += c;
    }
    if (out_mean_variance) *out_mean_variance = count > 0 ? (float)(sum / (double)count) : 0.0f;
    if (out_observations) *out_observations = d.momentsK;
    if (out_hit_pixels) *out_hit_pixels = (int)count;
    return PT_OK;
}

PT_API int pt_denoise_set_adaptive_noise(pt_handle h, int enable, int prior_samples)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_owner(h)) return rc;
    if (enable != 0 && enable != 1) return fail(h, PT_E_BAD_ARGUMENT, "enable must be 0 or 1");
    if (prior_samples < 1 || prior_samples > 65535) return fail(h, PT_E_OUT_OF_RANGE, "prior_samples 1..65535");
    h->denoise.adaptiveNoise = enable; // (read by the next pt_denoise_render; what is queued already took its values)
    h->denoise.adaptivePrior = prior_samples;
    return PT_OK;
}

PT_API int pt_denoise_read_variance_used(pt_handle h, float *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_rendered(h)) return rc;
    if (!h->denoise.blended)
        return fail(h, PT_E_BAD_ARGUMENT, "the last pt_denoise_render blended no measured variance into pass 0's (pt_denoise_set_moments / pt_denoise_set_adaptive_noise)");
    return denoise_copy_out(h, dst, row_pitch_bytes, h->denoise.dVar0, 4);
}

PT_API int pt_denoise_device_ptr(pt_handle h, void **out, size_t *bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_rendered(h)) return rc;
    if (out) *out = h->denoise.dImage[h->denoise.result];
    if (bytes) *bytes = h->tilePixels() * sizeof(float4);
    return PT_OK;
}

PT_API int pt_denoise_present_rgba8(pt_handle h, uint8_t *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_rendered(h)) return rc;
    if (!dst) return fail(h, PT_E_BAD_ARGUMENT, "dst == NULL");
    if (row_pitch_bytes != 0 && row_pitch_bytes < (size_t)h->width * 4) return fail(h, PT_E_BAD_ARGUMENT, "row pitch smaller than a row");
    if (int rc = join_stripes(h)) return rc; // (dRgba8 is shared with pt_present_rgba8 / pt_postprocess_device: same ordering as theirs)
    if (int rc = ensure_rgba8(h)) return rc;
    PT_HIP(h, ptimpl::launch_tone_map(h->presentArithmetic, h->denoise.dImage[h->denoise.result], h->dRgba8, h->tilePixels(), h->stream));
    return denoise_copy_out(h, dst, row_pitch_bytes, h->dRgba8, 4);
}

// ---- adaptive sampling (pt_adaptive.hip): per-tile sample counts driven by a noise estimate the passes measure themselves.
// The reference spends every frame on every pixel (PathTracer.cs:114-129); a pass spends one more sample on the tiles that still need it.
// Writes the accumulation image, the tile records and the per-pixel statistics; the frame counter stays where pt_render left it.
static int adaptive_owner(pt_handle h)
{
    if (h->isGroup()) return fail(h, PT_E_BAD_ARGUMENT, "adaptive sampling is not available on a group handle");
    return PT_OK;
}

static int adaptive_live(pt_handle h)
{
    if (int rc = adaptive_owner(h)) return rc;
    if (!h->adaptiveLive() || !h->adaptive.dTiles || !h->adaptive.dStats)
        return fail(h, PT_E_BAD_ARGUMENT, "no adaptive state (no pt_adaptive_render since the last pt_reset / pt_write_result / pt_set_size / pt_set_tile / pt_set_interleaved_tile / pt_bind_result_buffer)");
    return bind_device(h);
}

// the tile records as they stand once everything queued has run
static int adaptive_fetch_tiles(pt_handle h, std::vector<int4> &rec)
{
    rec.resize((size_t)h->tilesPerFrame());
    PT_HIP(h, hipMemcpyAsync(rec.data(), h->adaptive.dTiles, rec.size() * sizeof(int4), hipMemcpyDeviceToHost, h->stream));
    PT_HIP(h, hipStreamSynchronize(h->stream));
    return PT_OK;
}

PT_API int pt_adaptive_set_params(pt_handle h, float threshold, int min_samples, int max_samples)
{
    PT_CHECK_HANDLE(h);
    if (int rc = adaptive_owner(h)) return rc;
    if (!std::isfinite(threshold) || !(threshold >= 0.0f)) return fail(h, PT_E_BAD_ARGUMENT, "threshold must be finite and >= 0");
    if (min_samples < 2 || min_samples > 65535 || max_samples < min_samples || max_samples > 65535)
        return fail(h, PT_E_OUT_OF_RANGE, "min_samples 2..65535, max_samples min_samples..65535");
    h->adaptive.threshold = threshold; // (read by the passes enqueued from now on; what is queued already took its values)
    h->adaptive.minSamples = min_samples;
    h->adaptive.maxSamples = max_samples;
    return PT_OK;
}

PT_API int pt_adaptive_render(pt_handle h, int passes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = adaptive_owner(h)) return rc;
    if (passes < 1 || passes > 65535) return fail(h, PT_E_OUT_OF_RANGE, "passes 1..65535");
    if (h->arithmetic != PT_ARITH_CONTRACT) return fail(h, PT_E_BAD_ARGUMENT, "adaptive sampling renders in the contract arithmetic only (pt_set_arithmetic)");
    if (!h->dEnv) return fail(h, PT_E_NO_ENVIRONMENT, "pt_adaptive_render called before pt_set_environment / pt_atmosphere_render");
    if (h->boundAccum && h->boundBytes < h->tilePixels() * sizeof(float4))
        return fail(h, PT_E_BAD_ARGUMENT, "bound result buffer is smaller than the tile");
    if (int rc = bind_device(h)) return rc;
    // (pending frames are launched, an open frame-fed launch is closed, an abandoned hand-over is repaired, alpha is back to 1)
    if (int rc = ptimpl::fix_alpha(h)) return rc;
    pt_renderer::Adaptive &ad = h->adaptive;
    const int tilesX = h->tilesX(), tilesY = h->tilesY();
    if (!ad.dTiles) PT_HIP(h, hipMalloc((void **)&ad.dTiles, (size_t)tilesX * tilesY * sizeof(int4)));
    if (!ad.dStats) PT_HIP(h, hipMalloc((void **)&ad.dStats, h->tilePixels() * sizeof(float2)));
    pt::FrameArgs a;
    if (int rc = ptimpl::plain_frame_args(h, a, h->frame)) return rc;
    if (!h->adaptiveLive()) {
        PT_HIP(h, pt::launch_adaptive_init(ad.dTiles, tilesX, tilesY, h->width, h->rows, h->frame, h->stream));
        PT_HIP(h, hipMemsetAsync(ad.dStats, 0, h->tilePixels() * sizeof(float2), h->stream));
        ad.started = true;
        ad.epoch = h->resetEpoch;
    }
    pt::AdaptiveArgs p;
    p.tiles = ad.dTiles;
    p.stats = ad.dStats;
    p.threshold = ad.threshold;
    p.minSamples = ad.minSamples;
    p.maxSamples = ad.maxSamples;
    for (int i = 0; i < passes; i++) PT_HIP(h, pt::launch_adaptive(a, p, h->stream));
    return PT_OK;
}

PT_API int pt_adaptive_status(pt_handle h, int *out_active_tiles, int *out_tiles, int64_t *out_pixel_samples, int *out_min_count, int *out_max_count)
{
    PT_CHECK_HANDLE(h);
    if (int rc = adaptive_live(h)) return rc;
    std::vector<int4> rec;
    if (int rc = adaptive_fetch_tiles(h, rec)) return rc;
    const pt_renderer::Adaptive &ad = h->adaptive;
    int active = 0, lo = rec[0].x, hi = rec[0].x;
    long long samples = 0;
    for (const int4 &r : rec) {
        float err;
        std::memcpy(&err, &r.z, sizeof err);
        if (r.x < ad.maxSamples && (r.x - r.y < ad.minSamples - 1 || err > ad.threshold)) active++; // (the kernel's decision)
        samples += (long long)r.x * r.w;
        lo = r.x < lo ? r.x : lo;
        hi = r.x > hi ? r.x : hi;
    }
    if (out_active_tiles) *out_active_tiles = active;
    if (out_tiles) *out_tiles = (int)rec.size();
    if (out_pixel_samples) *out_pixel_samples = (int64_t)(samples * h->spp);
    if (out_min_count) *out_min_count = lo;
    if (out_max_count) *out_max_count = hi;
    return PT_OK;
}

PT_API int pt_adaptive_read_tiles(pt_handle h, void *dst_16_bytes_per_tile)
{
    PT_CHECK_HANDLE(h);
    if (int rc = adaptive_live(h)) return rc;
    if (!dst_16_bytes_per_tile) return fail(h, PT_E_BAD_ARGUMENT, "dst == NULL");
    std::vector<int4> rec;
    if (int rc = adaptive_fetch_tiles(h, rec)) return rc;
    std::memcpy(dst_16_bytes_per_tile, rec.data(), rec.size() * sizeof(int4));
    return PT_OK;
}

// word `word` of the per-pixel (M2, e) pairs, one float per pixel
static int adaptive_copy_stat(pt_handle h, float *dst, size_t row_pitch_bytes, int word)
{
    if (!dst) return fail(h, PT_E_BAD_ARGUMENT, "dst == NULL");
    const size_t rowBytes = (size_t)h->width * 4;
    if (row_pitch_bytes == 0) row_pitch_bytes = rowBytes;
    if (row_pitch_bytes < rowBytes) return fail(h, PT_E_BAD_ARGUMENT, "row pitch smaller than a row");
    std::vector<float2> st(h->tilePixels());
    PT_HIP(h, hipMemcpyAsync(st.data(), h->adaptive.dStats, st.size() * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
    PT_HIP(h, hipStreamSynchronize(h->stream));
    for (int y = 0; y < h->rows; y++) {
        float *row = (float *)((unsigned char *)dst + (size_t)y * row_pitch_bytes);
        const float2 *src = st.data() + (size_t)y * h->width;
        for (int x = 0; x < h->width; x++) row[x] = word ? src[x].y : src[x].x;
    }
    return PT_OK;
}

PT_API int pt_adaptive_read_noise(pt_handle h, float *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = adaptive_live(h)) return rc;
    return adaptive_copy_stat(h, dst, row_pitch_bytes, 1);
}

PT_API int pt_adaptive_read_m2(pt_handle h, float *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = adaptive_live(h)) return rc;
    return adaptive_copy_stat(h, dst, row_pitch_bytes, 0);
}

// A live state installed from its persistent half — the image, F, (k, k0, n) per tile, M2 per pixel; e and err are rebuilt
// (pt_adaptive_state.hip).  Everything is checked before anything of the handle is touched.
PT_API int pt_adaptive_write_state(pt_handle h, const float *image_rgba32f, size_t image_pitch_bytes, int frame_index, const void *tiles_16_bytes_per_tile,
                                   const float *m2, size_t m2_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = adaptive_owner(h)) return rc;
    if (!image_rgba32f || !tiles_16_bytes_per_tile || !m2 || frame_index < 0)
        return fail(h, PT_E_BAD_ARGUMENT, "image == NULL, tiles == NULL, m2 == NULL or negative frame index");
    if (h->rows < 1 || h->width < 1) return fail(h, PT_E_BAD_ARGUMENT, "the handle owns no rows");
    if (h->boundAccum && h->boundBytes < h->tilePixels() * sizeof(float4))
        return fail(h, PT_E_BAD_ARGUMENT, "bound result buffer is smaller than the tile");
    const size_t m2RowBytes = (size_t)h->width * 4;
    if (m2_pitch_bytes == 0) m2_pitch_bytes = m2RowBytes;
    if ((image_pitch_bytes != 0 && image_pitch_bytes < (size_t)h->width * 16) || m2_pitch_bytes < m2RowBytes)
        return fail(h, PT_E_BAD_ARGUMENT, "row pitch smaller than a row");
    const int tilesX = h->tilesX(), tilesY = h->tilesY();
    std::vector<int4> rec((size_t)tilesX * tilesY);
    std::memcpy(rec.data(), tiles_16_bytes_per_tile, rec.size() * sizeof(int4));
    const int k0 = frame_index > 1 ? frame_index : 1;
    for (int t = 0; t < tilesX * tilesY; t++) {
        const int tx = t % tilesX, ty = t / tilesX;
        const int w = h->width - tx * 8 < 8 ? h->width - tx * 8 : 8, r = h->rows - ty * 8 < 8 ? h->rows - ty * 8 : 8;
        int4 &q = rec[(size_t)t];
        if (q.w != w * r || q.y != k0 || q.x < frame_index || q.x > 65535)
            return fail(h, PT_E_OUT_OF_RANGE, "tile record: n = the tile's in-image pixels, k0 = max(frame_index, 1), frame_index <= k <= 65535");
        q.z = 0; // (err is not read: the rebuild writes it)
    }
    std::vector<float2> st(h->tilePixels());
    for (int y = 0; y < h->rows; y++) {
        const float *row = (const float *)((const unsigned char *)m2 + (size_t)y * m2_pitch_bytes);
        float2 *out = st.data() + (size_t)y * h->width;
        for (int x = 0; x < h->width; x++) {
            std::memcpy(&out[x].x, row + x, 4); // (as bits: any float)
            out[x].y = 0.0f;
        }
    }
    // the image: what pt_write_result does — join, upload, alpha = 1, the frame index, a new reset epoch (whatever state was live ends here)
    if (int rc = pt_write_result(h, image_rgba32f, image_pitch_bytes, frame_index)) return rc;
    pt_renderer::Adaptive &ad = h->adaptive;
    if (!ad.dTiles) PT_HIP(h, hipMalloc((void **)&ad.dTiles, rec.size() * sizeof(int4)));
    if (!ad.dStats) PT_HIP(h, hipMalloc((void **)&ad.dStats, st.size() * sizeof(float2)));
    PT_HIP(h, hipMemcpyAsync(ad.dTiles, rec.data(), rec.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
    PT_HIP(h, hipMemcpyAsync(ad.dStats, st.data(), st.size() * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    pt::AdaptiveRebuildArgs a;
    a.image = h->accum();
    a.stats = ad.dStats;
    a.tiles = ad.dTiles;
    a.width = h->width;
    a.rows = h->rows;
    a.tilesX = tilesX;
    a.tilesY = tilesY;
    PT_HIP(h, pt::launch_adaptive_rebuild(a, h->stream));
    PT_HIP(h, hipStreamSynchronize(h->stream)); // (the uploads read this call's own vectors)
    ad.started = true;
    ad.epoch = h->resetEpoch;
    return PT_OK;
}

// Levels every tile to the largest count with the sampler's own kernel — under (threshold 0, min 65535, max kmax) a tile is active exactly
// while k < kmax, since k - k0 < 65534 for every k < 65535 — and leaves the state as pt_bind_result_buffer leaves it: the image then holds
// kmax uniform frames in every pixel, so the accumulation goes on with frame index kmax in the same reset epoch.
PT_API int pt_adaptive_end(pt_handle h, int *out_frame_index)
{
    PT_CHECK_HANDLE(h);
    if (int rc = adaptive_live(h)) return rc;
    std::vector<int4> rec;
    if (int rc = adaptive_fetch_tiles(h, rec)) return rc;
    int lo = rec[0].x, hi = rec[0].x;
    for (const int4 &r : rec) {
        lo = r.x < lo ? r.x : lo;
        hi = r.x > hi ? r.x : hi;
    }
    if (lo < hi) {
        if (h->arithmetic != PT_ARITH_CONTRACT) return fail(h, PT_E_BAD_ARGUMENT, "adaptive sampling renders in the contract arithmetic only (pt_set_arithmetic)");
        if (!h->dEnv) return fail(h, PT_E_NO_ENVIRONMENT, "pt_adaptive_end called before pt_set_environment / pt_atmosphere_render");
        if (h->boundAccum && h->boundBytes < h->tilePixels() * sizeof(float4))
            return fail(h, PT_E_BAD_ARGUMENT, "bound result buffer is smaller than the tile");
        if (int rc = ptimpl::fix_alpha(h)) return rc;
        pt::FrameArgs a;
        if (int rc = ptimpl::plain_frame_args(h, a, h->frame)) return rc;
        pt::AdaptiveArgs p;
        p.tiles = h->adaptive.dTiles;
        p.stats = h->adaptive.dStats;
        p.threshold = 0.0f; // (the host's pt_adaptive_set_params values are neither read nor changed)
        p.minSamples = 65535;
        p.maxSamples = hi;
        for (int i = lo; i < hi; i++) PT_HIP(h, pt::launch_adaptive(a, p, h->stream));
    }
    h->adaptive.started = false;
    h->frame = hi;
    if (out_frame_index) *out_frame_index = hi;
    return PT_OK;
}

// Test aid (not declared in the public header): the per-pixel M2 of the adaptive state, laid out like pt_adaptive_read_noise's map.
extern "C" __attribute__((visibility("default"))) int pt_debug_adaptive_read_m2(pt_handle h, float *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = adaptive_live(h)) return rc;
    return adaptive_copy_stat(h, dst, row_pitch_bytes, 0);
}

// Timing aid (not declared in the public header): one stage of pt_denoise_render on its own — stage -1 = the guide kernel, i >= 0 = pass i
// of the mode in force, -2 = stage V (the variance estimate; PT_DENOISE_VARIANCE only), -4 = the temporal kernel (pt_denoise_set_temporal
// on only; whichever of pt_temporal_kernel / pt_temporal_tracked_kernel the last pt_denoise_render selected, with the object map it
// left) — between the buffers a full render uses (a pt_denoise_render must have run, with the temporal switch as it stands now; the
// result it left is overwritten with a partial one; the sets are neither swapped nor marked).
extern "C" __attribute__((visibility("default"))) int pt_debug_denoise_stage(pt_handle h, int guide_frame_index, int stage)
{
    PT_CHECK_HANDLE(h);
    if (stage == kDenoiseStageV && (h->denoise.mode != PT_DENOISE_VARIANCE || h->denoise.iterations == 0))
        return fail(h, PT_E_BAD_ARGUMENT, "stage -2 needs PT_DENOISE_VARIANCE and iterations > 0");
    if (stage == kDenoiseStageT && !h->denoise.temporal) return fail(h, PT_E_BAD_ARGUMENT, "stage -4 needs pt_denoise_set_temporal on");
    if (guide_frame_index < 0 || stage < kDenoiseStageT || stage == kDenoiseAll || stage >= h->denoise.iterations)
        return fail(h, PT_E_BAD_ARGUMENT, "stage must be -4, -2 .. iterations - 1");
    if (int rc = denoise_rendered(h)) return rc;
    if (h->denoise.integratedValid != (h->denoise.temporal != 0))
        return fail(h, PT_E_BAD_ARGUMENT, "the last pt_denoise_render ran with another setting of pt_denoise_set_temporal");
    return denoise_run(h, guide_frame_index, stage);
}

// Test aid (not declared in the public header): var_0 of the last pt_denoise_render, what pass 0 read in place of V0 — one float per
// pixel, rows like the image; PT_E_BAD_ARGUMENT when that render did not run stage B (pt_denoise_set_moments).
extern "C" __attribute__((visibility("default"))) int pt_debug_denoise_read_var0(pt_handle h, float *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (int rc = denoise_rendered(h)) return rc;
    if (!h->denoise.blended) return fail(h, PT_E_BAD_ARGUMENT, "the last pt_denoise_render did not blend the measured variance into pass 0's");
    return denoise_copy_out(h, dst, row_pitch_bytes, h->denoise.dVar0, 4);
}

} // extern "C"
