// mi355pt.cpp — the C ABI of lifecycle and inputs (include/mi355pt.h): create / destroy, size and tiling, params and uploads, environment
// and atmosphere, reading and writing the result, stream, timer and the variant / arithmetic setters.
//
// Owns the scene and input state at the top level of pt_renderer (what the reference keeps in the C# class PathTracer,
// /root/reference/OpenTK-PathTracer/src/Render/PathTracer.cs:9-141, plus the two UBOs MainWindow owns, src/MainWindow.cs:195-201) and the
// accumulation image.  Every entry point that observes or changes something first calls into mi355pt_launch.cpp (flush_frames) and
// mi355pt_handover.cpp (join_stripes, fix_alpha, settle_handover); teardown asks each mechanism's struct to release what it holds.
// There is deliberately NO CPU fallback: without a HIP device every entry point fails with PT_E_NO_DEVICE.
#include "pt_renderer.hpp"

#include <cmath>
#include <cstring>
#include <new>

namespace {
thread_local std::string g_create_error;
} // namespace

namespace ptimpl {

int fail(pt_handle h, int code, const std::string &msg)
{
    if (h) h->error = msg;
    else g_create_error = msg;
    return code;
}

int hip_fail(pt_handle h, hipError_t e, const char *what)
{
    return fail(h, e == hipErrorOutOfMemory ? PT_E_OUT_OF_MEMORY : PT_E_HIP,
                std::string(what) + ": " + hipGetErrorString(e));
}

int bind_device(pt_handle h)
{
    PT_HIP(h, hipSetDevice(h->device));
    return PT_OK;
}

} // namespace ptimpl

using ptimpl::bind_device;
using ptimpl::fail;
using ptimpl::flush_frames;
using ptimpl::hip_fail;
using ptimpl::join_stripes;

namespace {

// GL 4.5 section 8.24 sRGB decode, evaluated in double and rounded once (same table as the oracle's).
void make_srgb_lut(float *lut)
{
    for (int i = 0; i < 256; i++) {
        double cs = i / 255.0;
        double cl = cs <= 0.04045 ? cs / 12.92 : std::pow((cs + 0.055) / 1.055, 2.4);
        lut[i] = (float)cl;
    }
}

int ensure_accum(pt_handle h)
{
    size_t need = h->tilePixels();
    const size_t tiles = (size_t)h->tilesPerFrame();
    if (need > h->accumCapacity) PT_HIP(h, ptimpl::regrow_buffer(h->dAccum, h->accumCapacity, need, need * sizeof(float4)));
    // cached tile masks (FrameArgs::tileMasks) and FrameArgs::tileFlags: sized with the image so that pt_render never allocates or synchronises
    if (tiles > h->masks.tileMaskTiles) {
        PT_HIP(h, hipStreamSynchronize(h->stream)); // (callers have joined the handle's streams: nothing reads the old buffer any more)
        h->masks.tileMasksValid = false;
        PT_HIP(h, ptimpl::regrow_buffer(h->masks.dTileMasks, h->masks.tileMaskTiles, tiles, tiles * pt::kTileMaskWords * sizeof(unsigned long long)));
    }
    if (tiles > h->handover.tileFlagTiles) {
        PT_HIP(h, hipStreamSynchronize(h->stream));
        PT_HIP(h, ptimpl::regrow_buffer(h->handover.dTileFlags, h->handover.tileFlagTiles, tiles, tiles * sizeof(unsigned int)));
        PT_HIP(h, hipMemsetAsync(h->handover.dTileFlags, 0, tiles * sizeof(unsigned int), h->stream));
    }
#ifdef PT_AUDIT
    if (need > h->auditCapacity) {
        PT_HIP(h, hipStreamSynchronize(h->stream));
        PT_HIP(h, ptimpl::regrow_buffer(h->dAudit, h->auditCapacity, need, need * sizeof(unsigned long long)));
    }
#endif
    return PT_OK;
}

// hand-over audit: the pixels' history is unknown from here on (cleared / restored / re-bound image, frame counter reset).
// Call with the streams joined; stream-ordered on the main stream.
int audit_forget(pt_handle h)
{
    if (h->dAudit) PT_HIP(h, hipMemsetAsync(h->dAudit, 0xFF, h->tilePixels() * sizeof(unsigned long long), h->stream));
    return PT_OK;
}

int clear_accum(pt_handle h)
{
    if (h->boundAccum && h->boundBytes < h->tilePixels() * sizeof(float4))
        return fail(h, PT_E_BAD_ARGUMENT, "bound result buffer is smaller than the tile");
    if (int rc = join_stripes(h)) return rc;
    PT_HIP(h, pt::launch_clear(h->accum(), h->tilePixels(), h->stream));
    h->chain.tagsLive = false;
    return audit_forget(h);
}

// What pt_set_size, pt_set_tile and pt_set_interleaved_tile share.  Before the new size or tiling is stored: the launches so far — and their
// hand-over repair passes — belong to the buffers as they are, the first-hit records and the denoiser's buffers to the size and tiling ...
int leave_tiling(pt_handle h)
{
    if (int rc = join_stripes(h)) return rc;
    if (int rc = ptimpl::free_first_hit(h)) return rc;
    if (int rc = ptimpl::free_denoise(h)) return rc;
    if (int rc = ptimpl::free_adaptive(h)) return rc;
    h->resetEpoch++;
    return PT_OK;
}

// ... and behind it: frame 0 of a cleared image of the new rows
int enter_tiling(pt_handle h)
{
    h->frame = 0; // PathTracer.cs:133
    h->masks.tileMasksValid = false;
    h->masks.launchesSinceInputChange = 0;
    if (int rc = ensure_accum(h)) return rc;
    return clear_accum(h);
}

} // namespace

extern "C" {

PT_API const char *pt_version(void) { return "mi355pt 0.1 (gfx950, pt-f32)"; }

PT_API int pt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

PT_API const char *pt_last_error(pt_handle h)
{
    if (h && h->magic == ptimpl::kAlive) return h->error.c_str();
    return g_create_error.c_str();
}

PT_API int pt_create(int device_id, int width, int height, pt_handle *out)
{
    if (!out) return fail(nullptr, PT_E_BAD_ARGUMENT, "out == NULL");
    *out = nullptr;
    if (width <= 0 || height <= 0) return fail(nullptr, PT_E_BAD_ARGUMENT, "width/height must be positive");
    if (width > PT_MAX_IMAGE_DIM || height > PT_MAX_IMAGE_DIM)
        return fail(nullptr, PT_E_OUT_OF_RANGE, "width/height exceed PT_MAX_IMAGE_DIM (32767)");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, PT_E_NO_DEVICE, "no HIP device available (libmi355pt has no CPU fallback)");
    if (device_id < 0 || device_id >= n) return fail(nullptr, PT_E_BAD_ARGUMENT, "device_id out of range");
    pt_renderer *h = new (std::nothrow) pt_renderer();
    if (!h) return fail(nullptr, PT_E_OUT_OF_MEMORY, "host allocation failed");
    h->device = device_id;
    { // tuning knobs (pt_tuning.hpp: set through pt_debug_set only; the library reads no environment variables)
        const pt::Tuning &t = pt::tuning();
        if (t.drainCompaction >= -1) h->drainCompaction = t.drainCompaction;
        if (t.batchWorkgroupsPerCU >= 1 && t.batchWorkgroupsPerCU <= 8) h->pipeline.batchWorkgroupsPerCU = t.batchWorkgroupsPerCU;
        if (t.frameBatch >= 1 && t.frameBatch <= 64) { h->pipeline.maxBatch = t.frameBatch; h->pipeline.maxBatchExplicit = true; }
        if (t.queueChunk >= 1 && t.queueChunk <= 1024) h->queueChunk = t.queueChunk;
    }
    h->width = width;
    h->height = height;
    h->y0 = 0;
    h->rows = height;
#define PT_CREATE_HIP(call)                                                                                            \
    do {                                                                                                               \
        hipError_t e2_ = (call);                                                                                       \
        if (e2_ != hipSuccess) {                                                                                       \
            int rc_ = hip_fail(nullptr, e2_, #call);                                                                   \
            pt_destroy(h);                                                                                             \
            return rc_;                                                                                                \
        }                                                                                                              \
    } while (0)
    PT_CREATE_HIP(hipSetDevice(device_id));
    PT_CREATE_HIP(hipStreamCreateWithFlags(&h->ownStream, hipStreamNonBlocking));
    h->stream = h->ownStream;
    PT_CREATE_HIP(hipEventCreateWithFlags(&h->stripes.inputsReady, hipEventDisableTiming));
    PT_CREATE_HIP(hipEventCreateWithFlags(&h->group.gatherReady, hipEventDisableTiming));
    PT_CREATE_HIP(hipStreamCreateWithFlags(&h->copyStream, hipStreamNonBlocking));
    PT_CREATE_HIP(hipEventCreate(&h->evBegin));
    PT_CREATE_HIP(hipEventCreate(&h->evEnd));
    // (UBO 1 and, behind it, the packed sphere geometry the scalar sphere step reads: pt_kernels.hpp, kSphereGeomOffset)
    static_assert(pt::kSphereGeomOffset == PT_GAME_OBJECTS_UBO_SIZE && pt::kSphereGeomEntries == PT_MAX_SPHERES, "sphereGeom follows UBO 1");
    PT_CREATE_HIP(hipMalloc((void **)&h->dObjects, PT_GAME_OBJECTS_UBO_SIZE + PT_MAX_SPHERES * 16));
    PT_CREATE_HIP(hipMemsetAsync(h->dObjects, 0, PT_GAME_OBJECTS_UBO_SIZE + PT_MAX_SPHERES * 16, h->stream));
    PT_CREATE_HIP(hipMalloc((void **)&h->dGrid, (ptgrid::kMaxCells + 1) * 2 + ptgrid::kMaxRefs + 16));
    PT_CREATE_HIP(hipMalloc((void **)&h->dLut, 256 * sizeof(float)));
    PT_CREATE_HIP(hipMalloc((void **)&h->dQueue, ptimpl::kQueueWords * sizeof(unsigned int)));
    PT_CREATE_HIP(hipMemsetAsync(h->dQueue, 0, ptimpl::kQueueWords * sizeof(unsigned int), h->stream));
    PT_CREATE_HIP(hipHostMalloc((void **)&h->handover.hostErrWord, sizeof(unsigned int), hipHostMallocMapped));
    *h->handover.hostErrWord = 0;
    PT_CREATE_HIP(hipHostGetDevicePointer((void **)&h->handover.devErrWord, h->handover.hostErrWord, 0));
    PT_CREATE_HIP(hipMalloc((void **)&h->handover.dAbandon, sizeof(unsigned int)));
    PT_CREATE_HIP(hipMemsetAsync(h->handover.dAbandon, 0xFF, sizeof(unsigned int), h->stream)); // ABANDON_NONE
    PT_CREATE_HIP(hipMalloc((void **)&h->handover.dRepairCtl, 4 * sizeof(unsigned int)));
    PT_CREATE_HIP(hipMemsetAsync(h->handover.dRepairCtl, 0, 4 * sizeof(unsigned int), h->stream));
    {
        // the hand-over's wall-clock budget in units of 1,024 ticks of the device's constant-rate counter (100 MHz on gfx950)
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_id) != hipSuccess || khz <= 0) khz = 100000;
        (void)hipGetLastError();
        h->handover.wallClockKhz = khz;
        const pt::Tuning &t = pt::tuning();
        const double unitsPerMs = (double)khz / 1024.0;
        double budget = (double)t.handoverBudgetMs * unitsPerMs, check = (double)t.handoverCheckUs * unitsPerMs / 1000.0;
        if (budget > 1.0e9) budget = 1.0e9; // (the kernels compare signed 32-bit differences: ~2.8 hours)
        if (check > budget / 4.0) check = budget / 4.0; // (short test budgets: look often enough)
        h->handover.waitBudgetUnits = (unsigned int)budget;
        h->handover.waitCheckUnits = (unsigned int)check;
    }
    PT_CREATE_HIP(hipHostMalloc((void **)&h->feed.hostFeed, pt_renderer::kFeedHostWords * sizeof(unsigned int), hipHostMallocMapped | hipHostMallocCoherent));
    for (int i = 0; i < pt_renderer::kFeedHostWords; i++) h->feed.hostFeed[i] = pt::kFeedClosed;
    PT_CREATE_HIP(hipHostMalloc((void **)&h->feed.hostFeedDone, pt_renderer::kFeedHostWords * sizeof(unsigned int), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h->feed.hostFeedDone, 0, pt_renderer::kFeedHostWords * sizeof(unsigned int));
    PT_CREATE_HIP(hipHostGetDevicePointer((void **)&h->feed.devFeedHostDone, h->feed.hostFeedDone, 0));
    PT_CREATE_HIP(hipHostGetDevicePointer((void **)&h->feed.devFeedHost, h->feed.hostFeed, 0));
    PT_CREATE_HIP(hipMalloc((void **)&h->feed.dFeedDev, (size_t)2 * pt::kFeedBcastSlots * pt::kFeedBcastStride * sizeof(unsigned int)));
    PT_CREATE_HIP(hipMemsetAsync(h->feed.dFeedDev, 0, (size_t)2 * pt::kFeedBcastSlots * pt::kFeedBcastStride * sizeof(unsigned int), h->stream));
    PT_CREATE_HIP(hipMalloc((void **)&h->feed.dFeedDone, (size_t)16 * pt::kFeedDoneStride * sizeof(unsigned long long)));
    PT_CREATE_HIP(hipMemsetAsync(h->feed.dFeedDone, 0, (size_t)16 * pt::kFeedDoneStride * sizeof(unsigned long long), h->stream));
    PT_CREATE_HIP(hipHostMalloc((void **)&h->chain.hostStarted, ptimpl::kStartedWords * sizeof(unsigned int), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h->chain.hostStarted, 0, ptimpl::kStartedWords * sizeof(unsigned int));
    PT_CREATE_HIP(hipHostGetDevicePointer((void **)&h->chain.devStarted, h->chain.hostStarted, 0));
#ifdef PT_AUDIT
    {
        const size_t words = 4 + (size_t)pt::kAuditLogRecords * pt::kAuditRecordWords;
        PT_CREATE_HIP(hipHostMalloc((void **)&h->hostAuditLog, words * sizeof(unsigned int), hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(h->hostAuditLog, 0, words * sizeof(unsigned int));
        PT_CREATE_HIP(hipHostGetDevicePointer((void **)&h->devAuditLog, h->hostAuditLog, 0));
    }
#endif
    {
        hipDeviceProp_t prop;
        PT_CREATE_HIP(hipGetDeviceProperties(&prop, device_id));
        h->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    float lut[256];
    make_srgb_lut(lut);
    PT_CREATE_HIP(hipMemcpyAsync(h->dLut, lut, sizeof lut, hipMemcpyHostToDevice, h->stream));
    PT_CREATE_HIP(hipStreamSynchronize(h->stream)); // `lut` is a stack array
#undef PT_CREATE_HIP
    int rc = ensure_accum(h);
    if (rc == PT_OK) rc = clear_accum(h);
    if (rc != PT_OK) {
        g_create_error = h->error;
        pt_destroy(h);
        return rc;
    }
    *out = h;
    return PT_OK;
}

PT_API int pt_destroy(pt_handle h)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) return ptimpl::group_destroy(h);
    h->pipeline.pendingFrames = 0; // frames nobody can observe any more are not worth launching
    (void)hipSetDevice(h->device);
    ptimpl::feed_close(h); // (a frame-fed launch still waiting for frames ends now)
    // (launches may still write present snapshots, tone maps read them: every stream of the handle is drained before they are freed)
    for (int j = 0; j < ptimpl::kMaxStripes; j++)
        if (h->stripes.stripeStream[j]) (void)hipStreamSynchronize(h->stripes.stripeStream[j]);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->copyStream) (void)hipStreamSynchronize(h->copyStream);
    h->snaps.release();
    ptimpl::free_slots(h);
    if (h->copyStream) (void)hipStreamDestroy(h->copyStream);
    if (h->group.gatherReady) (void)hipEventDestroy(h->group.gatherReady);
    for (int j = 0; j < ptimpl::kMaxStripes; j++)
        if (h->stripes.stripeStream[j]) (void)hipStreamSynchronize(h->stripes.stripeStream[j]);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->stripes.release();
    h->handover.release();
    if (h->dObjects) (void)hipFree(h->dObjects);
    if (h->dGrid) (void)hipFree(h->dGrid);
    if (h->dLut) (void)hipFree(h->dLut);
    if (h->dQueue) (void)hipFree(h->dQueue);
    if (h->masks.dTileMasks) (void)hipFree(h->masks.dTileMasks);
    if (h->chain.hostStarted) (void)hipHostFree(h->chain.hostStarted);
    h->feed.release();
    if (h->hostAuditLog) (void)hipHostFree(h->hostAuditLog);
    if (h->dAudit) (void)hipFree(h->dAudit);
    if (h->dEnv) (void)hipFree(h->dEnv);
    if (h->dAccum) (void)hipFree(h->dAccum);
    if (h->dRgba8) (void)hipFree(h->dRgba8);
    if (h->dFirstHit) (void)hipFree(h->dFirstHit);
    if (h->dPick) (void)hipFree(h->dPick);
    (void)h->denoise.release();
    if (h->adaptive.dTiles) (void)hipFree(h->adaptive.dTiles);
    if (h->adaptive.dStats) (void)hipFree(h->adaptive.dStats);
    if (h->dTimeline) (void)hipFree(h->dTimeline);
    if (h->evBegin) (void)hipEventDestroy(h->evBegin);
    if (h->evEnd) (void)hipEventDestroy(h->evEnd);
    if (h->ownStream) (void)hipStreamDestroy(h->ownStream);
    h->magic = 0;
    delete h;
    return PT_OK;
}

PT_API int pt_set_size(pt_handle h, int width, int height)
{
    PT_CHECK_HANDLE(h);
    if (width <= 0 || height <= 0) return fail(h, PT_E_BAD_ARGUMENT, "width/height must be positive");
    if (width > PT_MAX_IMAGE_DIM || height > PT_MAX_IMAGE_DIM)
        return fail(h, PT_E_OUT_OF_RANGE, "width/height exceed PT_MAX_IMAGE_DIM (32767)");
    if (h->isGroup()) return ptimpl::group_set_size(h, width, height);
    if (int rc = flush_frames(h)) return rc; // pending frames were rendered with the inputs as they were
    if (int rc = bind_device(h)) return rc;
    if (int rc = leave_tiling(h)) return rc;
    h->width = width;
    h->height = height;
    h->y0 = 0;
    h->rows = height;
    h->bandRows = 0;
    return enter_tiling(h);
}

PT_API int pt_set_tile(pt_handle h, int y0, int rows)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) return fail(h, PT_E_BAD_ARGUMENT, "a group handle owns its tiling (pt_multi_set_partition)");
    if (int rc = flush_frames(h)) return rc; // pending frames were rendered with the inputs as they were
    if (y0 < 0 || rows <= 0 || y0 + rows > h->height) return fail(h, PT_E_BAD_ARGUMENT, "tile outside the image");
    if (int rc = bind_device(h)) return rc;
    if (int rc = leave_tiling(h)) return rc;
    h->y0 = y0;
    h->rows = rows;
    h->bandRows = 0;
    return enter_tiling(h);
}

PT_API int pt_set_interleaved_tile(pt_handle h, int rank, int world, int band_rows)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) return fail(h, PT_E_BAD_ARGUMENT, "a group handle owns its tiling (pt_multi_set_partition)");
    if (int rc = flush_frames(h)) return rc; // pending frames were rendered with the inputs as they were
    if (world < 1 || rank < 0 || rank >= world || band_rows < 8 || (band_rows & 7))
        return fail(h, PT_E_BAD_ARGUMENT, "need 0 <= rank < world and band_rows a positive multiple of 8");
    if (int rc = bind_device(h)) return rc;
    // rows owned: bands rank, rank + world, ... of band_rows rows (the last band of the image may be partial)
    long long rows = 0;
    for (long long b = rank; b * band_rows < h->height; b += world) {
        long long top = (b + 1) * band_rows;
        rows += (top < h->height ? top : h->height) - b * band_rows;
    }
    if (rows <= 0) return fail(h, PT_E_BAD_ARGUMENT, "this rank owns no rows (image too small for world * band_rows)");
    if (int rc = leave_tiling(h)) return rc;
    h->y0 = 0;
    h->rows = (int)rows;
    h->bandRows = band_rows;
    h->bandWorld = world;
    h->bandRank = rank;
    return enter_tiling(h);
}

PT_API int pt_reset(pt_handle h)
{
    PT_CHECK_HANDLE(h);
    PT_FAN_OUT(h, pt_reset(part));
    if (int rc = flush_frames(h)) return rc; // pending frames were rendered with the inputs as they were
    // (the frame counter goes backwards: the tags in the image must not be mistaken for frames of the new sequence)
    if (int rc = bind_device(h)) return rc;
    if (int rc = ptimpl::fix_alpha(h)) return rc;
    h->frame = 0; // PathTracer.cs:139 — frame 0 weights the old contents by 0, so no clear is needed
    h->resetEpoch++; // (the temporal stage of the denoiser: what it integrated so far belongs to the view that ends here)
    return audit_forget(h);
}

PT_API int pt_set_params(pt_handle h, int num_spheres, int num_cuboids, int ray_depth, int spp, float focal_length,
                         float aperture_diameter)
{
    PT_CHECK_HANDLE(h);
    PT_FAN_OUT(h, pt_set_params(part, num_spheres, num_cuboids, ray_depth, spp, focal_length, aperture_diameter));
    // The reference's setters run whenever the GUI touches a slider, changed or not (PathTracer.cs:11-83): values the renderer already
    // has are not an input change — nothing is flushed, nothing invalidated (bitwise compare: -0.0f / NaN count as changes).
    if (num_spheres == h->numSpheres && num_cuboids == h->numCuboids && ray_depth == h->rayDepth && spp == h->spp &&
        std::memcmp(&focal_length, &h->focalLength, sizeof(float)) == 0 && std::memcmp(&aperture_diameter, &h->apertureDiameter, sizeof(float)) == 0)
        return PT_OK;
    if (num_spheres < 0 || num_spheres > PT_MAX_SPHERES || num_cuboids < 0 || num_cuboids > PT_MAX_CUBOIDS)
        return fail(h, PT_E_OUT_OF_RANGE, "object counts exceed the GameObjectsUBO arrays (256 spheres / 64 cuboids)");
    if (ray_depth < 0 || spp < 1) return fail(h, PT_E_BAD_ARGUMENT, "ray_depth must be >= 0 and spp >= 1");
    // the kernels carry bounce / sample counters in 12-bit fields of their path records
    if (ray_depth > PT_MAX_RAY_DEPTH || spp > PT_MAX_SPP)
        return fail(h, PT_E_OUT_OF_RANGE, "ray_depth / spp exceed PT_MAX_RAY_DEPTH / PT_MAX_SPP (4095)");
    if (int rc = flush_frames(h)) return rc; // pending frames were rendered with the inputs as they were
    if (num_spheres != h->numSpheres) h->gridDirty = true;
    if (num_spheres != h->numSpheres || num_cuboids != h->numCuboids || focal_length != h->focalLength || aperture_diameter != h->apertureDiameter) {
        h->masks.tileMasksValid = false; // (the cached masks cull spheres AND cuboids against the lens' cone)
        h->masks.launchesSinceInputChange = 0;
    }
    h->numSpheres = num_spheres;
    h->numCuboids = num_cuboids;
    h->rayDepth = ray_depth;
    h->spp = spp;
    h->focalLength = focal_length;
    h->apertureDiameter = aperture_diameter;
    return PT_OK;
}

PT_API int pt_upload_basic_data(pt_handle h, int byte_offset, int size, const void *src)
{
    PT_CHECK_HANDLE(h);
    PT_FAN_OUT(h, pt_upload_basic_data(part, byte_offset, size, src));
    if (!src) return fail(h, PT_E_BAD_ARGUMENT, "src == NULL");
    if (byte_offset < 0 || size < 0 || (long long)byte_offset + size > PT_BASIC_DATA_UBO_SIZE)
        return fail(h, PT_E_OUT_OF_RANGE, "BasicDataUBO range outside [0,144)");
    // The reference re-uploads InvView and ViewPos on EVERY focused update, moved or not (MainWindow.cs:131-132): two SubData calls between
    // every pair of Render() calls.  Bytes the renderer already holds are not an input change: no flush (the frames keep pipelining), no
    // invalidation (the cached tile masks stay valid).  A changed byte flushes first — pending frames were rendered with the camera as it was.
    if (std::memcmp(h->basic + byte_offset, src, (size_t)size) == 0) return PT_OK;
    h->statFlushes++;
    if (int rc = flush_frames(h)) return rc;
    std::memcpy(h->basic + byte_offset, src, (size_t)size);
    h->masks.tileMasksValid = false; h->masks.launchesSinceInputChange = 0;
    return PT_OK;
}

PT_API int pt_upload_game_objects(pt_handle h, int byte_offset, int size, const void *src)
{
    PT_CHECK_HANDLE(h);
    PT_FAN_OUT(h, pt_upload_game_objects(part, byte_offset, size, src));
    if (!src) return fail(h, PT_E_BAD_ARGUMENT, "src == NULL");
    if (byte_offset < 0 || size < 0 || (long long)byte_offset + size > PT_GAME_OBJECTS_UBO_SIZE)
        return fail(h, PT_E_OUT_OF_RANGE, "GameObjectsUBO range outside [0,26624)");
    if (size == 0) return PT_OK;
    // (an object the GUI re-uploads unchanged, Gui.cs:212-216, or a scene reload with the same bytes, MainWindow.cs:119-123: see
    // pt_upload_basic_data — nothing is joined, copied or invalidated)
    if (std::memcmp(h->objectsShadow + byte_offset, src, (size_t)size) == 0) return PT_OK;
    h->statFlushes++;
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc;
    // pageable source: HIP stages the bytes before returning, so the caller may reuse `src` immediately
    PT_HIP(h, hipMemcpyAsync((char *)h->dObjects + byte_offset, src, (size_t)size, hipMemcpyHostToDevice, h->stream));
    // (the device block holds the new bytes from here on: shadow and flags follow it before anything else can fail)
    std::memcpy(h->objectsShadow + byte_offset, src, (size_t)size);
    if (byte_offset < PT_MAX_SPHERES * 80) h->gridDirty = true; // (the Spheres[] array ends at byte 20,480)
    h->masks.tileMasksValid = false; // (any object: the cached per-tile masks hold a sphere mask and a cuboid mask)
    h->masks.launchesSinceInputChange = 0;
    {
        // the packed sphere geometry follows on the same stream: whatever is ordered against the copy is ordered against the refresh
        int first, count;
        pt::sphere_geom_range(byte_offset, size, first, count);
        PT_HIP(h, pt::launch_sphere_geom(h->dObjects, first, count, h->stream));
    }
    return PT_OK;
}

PT_API int pt_set_environment(pt_handle h, int face_size, int format, const void *const faces[6])
{
    PT_CHECK_HANDLE(h);
    PT_FAN_OUT(h, pt_set_environment(part, face_size, format, faces));
    if (face_size <= 0 || face_size > 16384) return fail(h, PT_E_BAD_ARGUMENT, "face_size out of range");
    if (format != PT_ENV_RGBA32F && format != PT_ENV_SRGB8_A8) return fail(h, PT_E_BAD_ARGUMENT, "unknown format");
    if (!faces) return fail(h, PT_E_BAD_ARGUMENT, "faces == NULL");
    for (int f = 0; f < 6; f++)
        if (!faces[f]) return fail(h, PT_E_BAD_ARGUMENT, "faces[i] == NULL");
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc;
    size_t faceBytes = (size_t)face_size * face_size * (format == PT_ENV_RGBA32F ? 16 : 4);
    size_t total = faceBytes * 6;
    if (total > h->envBytes) {
        PT_HIP(h, hipStreamSynchronize(h->stream)); // a queued frame may still sample the old cube
        PT_HIP(h, ptimpl::regrow_buffer(h->dEnv, h->envBytes, total, total));
    }
    for (int f = 0; f < 6; f++)
        PT_HIP(h, hipMemcpyAsync((char *)h->dEnv + f * faceBytes, faces[f], faceBytes, hipMemcpyHostToDevice, h->stream));
    h->envSize = face_size;
    h->envFormat = format;
    return PT_OK;
}

} // extern "C"

extern "C" {

PT_API int pt_read_result(pt_handle h, float *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (!dst) return fail(h, PT_E_BAD_ARGUMENT, "dst == NULL");
    size_t rowBytes = (size_t)h->width * 16;
    if (row_pitch_bytes == 0) row_pitch_bytes = rowBytes;
    if (row_pitch_bytes < rowBytes) return fail(h, PT_E_BAD_ARGUMENT, "row pitch smaller than a row");
    if (h->isGroup()) return ptimpl::group_read_result(h, dst, row_pitch_bytes);
    if (int rc = bind_device(h)) return rc;
    // (the frames first, then the hand-over check — a repair pass in the rare case — then the copy of a settled image)
    if (int rc = ptimpl::fix_alpha(h, false)) return rc;
    PT_HIP(h, hipStreamSynchronize(h->stream));
    if (int rc = ptimpl::settle_handover(h)) return rc;
    PT_HIP(h, hipMemcpy2DAsync(dst, row_pitch_bytes, h->accum(), rowBytes, rowBytes, (size_t)h->rows,
                               hipMemcpyDeviceToHost, h->stream));
    PT_HIP(h, hipStreamSynchronize(h->stream));
    return PT_OK;
}

PT_API int pt_write_result(pt_handle h, const float *src, size_t row_pitch_bytes, int frame_index)
{
    PT_CHECK_HANDLE(h);
    if (!src || frame_index < 0) return fail(h, PT_E_BAD_ARGUMENT, "src == NULL or negative frame index");
    size_t rowBytes = (size_t)h->width * 16;
    if (row_pitch_bytes == 0) row_pitch_bytes = rowBytes;
    if (row_pitch_bytes < rowBytes) return fail(h, PT_E_BAD_ARGUMENT, "row pitch smaller than a row");
    if (h->isGroup()) return ptimpl::group_write_result(h, src, row_pitch_bytes, frame_index);
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc;
    PT_HIP(h, hipMemcpy2DAsync(h->accum(), rowBytes, src, row_pitch_bytes, rowBytes, (size_t)h->rows,
                               hipMemcpyHostToDevice, h->stream));
    // alpha is the reference's constant 1 (compute.glsl:129) whatever the file held: inside a pipelined launch alpha
    // carries the frame tag, so a restored 2.0 must never reach the kernel
    PT_HIP(h, pt::launch_set_alpha(h->accum(), h->tilePixels(), h->stream));
    h->chain.tagsLive = false;
    if (int rc = audit_forget(h)) return rc;
    PT_HIP(h, hipStreamSynchronize(h->stream));
    h->frame = frame_index;
    h->resetEpoch++;
    return PT_OK;
}

PT_API int pt_get_frame_index(pt_handle h, int *out)
{
    PT_CHECK_HANDLE(h);
    if (!out) return fail(h, PT_E_BAD_ARGUMENT, "out == NULL");
    *out = h->isGroup() ? h->group.parts[0]->frame : h->frame;
    return PT_OK;
}

PT_API int pt_synchronize(pt_handle h)
{
    PT_CHECK_HANDLE(h);
    PT_FAN_OUT(h, pt_synchronize(part));
    if (int rc = bind_device(h)) return rc;
    if (int rc = ptimpl::fix_alpha(h, false)) return rc; // (a bound buffer is observed after this call)
    PT_HIP(h, hipStreamSynchronize(h->stream));
    return ptimpl::settle_handover(h);
}

PT_API int pt_atmosphere_upload_data(pt_handle h, int byte_offset, int size, const void *src)
{
    PT_CHECK_HANDLE(h);
    PT_FAN_OUT(h, pt_atmosphere_upload_data(part, byte_offset, size, src));
    if (!src) return fail(h, PT_E_BAD_ARGUMENT, "src == NULL");
    if (byte_offset < 0 || size < 0 || (long long)byte_offset + size > PT_ATMOSPHERE_UBO_SIZE)
        return fail(h, PT_E_OUT_OF_RANGE, "AtmosphericDataUBO range outside [0,464)");
    std::memcpy(h->atmoUbo + byte_offset, src, (size_t)size);
    return PT_OK;
}

PT_API int pt_atmosphere_render(pt_handle h, int size, int i_steps, int j_steps, const float light_pos[3],
                                float light_intensity)
{
    PT_CHECK_HANDLE(h);
    // every device of a group computes its own copy of the cube (deterministic kernel: the copies are identical)
    PT_FAN_OUT(h, pt_atmosphere_render(part, size, i_steps, j_steps, light_pos, light_intensity));
    if (size <= 0 || size > 8192 || i_steps < 0 || j_steps < 0 || !light_pos)
        return fail(h, PT_E_BAD_ARGUMENT, "bad atmosphere parameters");
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc;
    size_t total = (size_t)6 * size * size * 16;
    if (total > h->envBytes) {
        PT_HIP(h, hipStreamSynchronize(h->stream));
        PT_HIP(h, ptimpl::regrow_buffer(h->dEnv, h->envBytes, total, total));
    }
    pt::AtmoArgs a;
    std::memcpy(a.invProj, h->atmoUbo, 64);
    std::memcpy(a.invView, h->atmoUbo + 64, 6 * 64);
    a.lightPos[0] = light_pos[0];
    a.lightPos[1] = light_pos[1];
    a.lightPos[2] = light_pos[2];
    a.lightIntensity = light_intensity < 0.0f ? 0.0f : light_intensity; // AtmosphericScatterer.cs:52
    a.size = size;
    a.iSteps = i_steps;
    a.jSteps = j_steps;
    a.out = (float4 *)h->dEnv;
    PT_HIP(h, h->atmoArithmetic == PT_ARITH_REFERENCE ? pt::launch_atmosphere_reference(a, h->stream) : pt::launch_atmosphere(a, h->stream));
    h->envSize = size;
    h->envFormat = PT_ENV_RGBA32F;
    return PT_OK;
}

PT_API int pt_atmosphere_set_arithmetic(pt_handle h, int mode)
{
    PT_CHECK_HANDLE(h);
    if (mode != PT_ARITH_CONTRACT && mode != PT_ARITH_REFERENCE) return fail(h, PT_E_BAD_ARGUMENT, "mode must be PT_ARITH_CONTRACT or PT_ARITH_REFERENCE");
    PT_FAN_OUT(h, pt_atmosphere_set_arithmetic(part, mode));
    h->atmoArithmetic = mode; // (host state only: the current environment and pending frames are untouched)
    return PT_OK;
}

PT_API int pt_read_environment(pt_handle h, float *dst, int *out_face_size)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) {
        int rc = pt_read_environment(h->group.parts[0], dst, out_face_size);
        return rc == PT_OK ? rc : fail(h, rc, h->group.parts[0]->error);
    }
    if (!h->dEnv) return fail(h, PT_E_NO_ENVIRONMENT, "no environment set");
    if (out_face_size) *out_face_size = h->envSize;
    if (!dst) return PT_OK; // size query
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc;
    size_t n = (size_t)6 * h->envSize * h->envSize;
    if (h->envFormat == PT_ENV_RGBA32F) {
        PT_HIP(h, hipMemcpyAsync(dst, h->dEnv, n * 16, hipMemcpyDeviceToHost, h->stream));
        PT_HIP(h, hipStreamSynchronize(h->stream));
        return PT_OK;
    }
    float4 *tmp = nullptr;
    PT_HIP(h, hipMalloc((void **)&tmp, n * 16));
    hipError_t e = pt::launch_env_to_float(h->dEnv, h->envSize, h->envFormat, h->dLut, tmp, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst, tmp, n * 16, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(tmp);
    if (e != hipSuccess) return hip_fail(h, e, "pt_read_environment");
    return PT_OK;
}

PT_API int pt_result_device_ptr(pt_handle h, void **out_ptr, size_t *out_bytes)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) return ptimpl::group_result_device_ptr(h, out_ptr, out_bytes);
    // whatever pt_render deferred is launched and joined into the handle's stream first: work the caller orders behind
    // that stream (or behind pt_synchronize) then sees every frame rendered so far
    if (int rc = bind_device(h)) return rc;
    if (int rc = ptimpl::fix_alpha(h)) return rc;
    if (out_ptr) *out_ptr = h->accum();
    if (out_bytes) *out_bytes = h->tilePixels() * sizeof(float4);
    return PT_OK;
}

PT_API int pt_bind_result_buffer(pt_handle h, void *device_ptr, size_t bytes)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) return fail(h, PT_E_BAD_ARGUMENT, "pt_bind_result_buffer is not available on a group handle");
    if (device_ptr && bytes < h->tilePixels() * sizeof(float4))
        return fail(h, PT_E_BAD_ARGUMENT, "buffer smaller than rows*width*16 bytes");
    if (int rc = bind_device(h)) return rc;
    if (int rc = ptimpl::fix_alpha(h)) return rc; // (the image rendered so far stays behind with alpha = 1)
    h->boundAccum = (float4 *)device_ptr;
    h->boundBytes = device_ptr ? bytes : 0;
    h->adaptive.started = false; // (an adaptive state describes the image it was made on)
    // alpha doubles as the frame tag inside pipelined launches: whatever the caller's memory holds, it starts as 1
    if (device_ptr) PT_HIP(h, pt::launch_set_alpha(h->boundAccum, h->tilePixels(), h->stream));
    return audit_forget(h);
}

PT_API int pt_set_stream(pt_handle h, void *hip_stream)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) return fail(h, PT_E_BAD_ARGUMENT, "pt_set_stream is not available on a group handle");
    if (int rc = bind_device(h)) return rc;
    if (int rc = ptimpl::fix_alpha(h)) return rc;
    PT_HIP(h, hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->ownStream;
    return PT_OK;
}

PT_API int pt_timer_begin(pt_handle h)
{
    PT_CHECK_HANDLE(h);
    PT_FAN_OUT(h, pt_timer_begin(part));
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc;
    PT_HIP(h, hipEventRecord(h->evBegin, h->stream));
    return PT_OK;
}

PT_API int pt_timer_end(pt_handle h, float *out_ms)
{
    PT_CHECK_HANDLE(h);
    if (!out_ms) return fail(h, PT_E_BAD_ARGUMENT, "out == NULL");
    if (h->isGroup()) return ptimpl::group_timer_end(h, out_ms);
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc;
    PT_HIP(h, hipEventRecord(h->evEnd, h->stream));
    PT_HIP(h, hipEventSynchronize(h->evEnd));
    PT_HIP(h, hipEventElapsedTime(out_ms, h->evBegin, h->evEnd));
    return PT_OK;
}

PT_API int pt_set_variant(pt_handle h, int variant)
{
    PT_CHECK_HANDLE(h);
    PT_FAN_OUT(h, pt_set_variant(part, variant));
    if (int rc = flush_frames(h)) return rc; // pending frames were rendered with the inputs as they were
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc; // a different stripe partition must not overlap frames in flight
    h->variant = variant;
    return PT_OK;
}

PT_API int pt_set_arithmetic(pt_handle h, int mode)
{
    PT_CHECK_HANDLE(h);
    if (mode != PT_ARITH_CONTRACT && mode != PT_ARITH_REFERENCE) return fail(h, PT_E_BAD_ARGUMENT, "mode must be PT_ARITH_CONTRACT or PT_ARITH_REFERENCE");
    PT_FAN_OUT(h, pt_set_arithmetic(part, mode));
    if (int rc = flush_frames(h)) return rc; // pending frames keep the arithmetic they were issued under
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc;
    h->arithmetic = mode; // (the accumulation is kept, as pt_set_variant keeps it)
    return PT_OK;
}

PT_API int pt_device_count_of(pt_handle h, int *out_n_devices)
{
    PT_CHECK_HANDLE(h);
    if (!out_n_devices) return fail(h, PT_E_BAD_ARGUMENT, "out == NULL");
    *out_n_devices = h->isGroup() ? (int)h->group.parts.size() : 1;
    return PT_OK;
}

} // extern "C"
