// mi355pt_debug.cpp — every pt_debug_* export (tuning and test aids that include/mi355pt.h does not declare) and the pt_debug_plan_* structs.
//
// Owns no state: reads the handle's counters and buffers, and calls bind_device, join_stripes and the public pt_synchronize.
#include "pt_renderer.hpp"

#include <cstring>
#include <vector>

using ptimpl::bind_device;
using ptimpl::fail;
using ptimpl::join_stripes;

// Tuning aid (not declared in the public header): per-wavefront timestamps of the next persistent-kernel launches.
extern "C" __attribute__((visibility("default"))) int pt_debug_timeline(pt_handle h, unsigned long long *host_out, int max_waves)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) return fail(h, PT_E_BAD_ARGUMENT, "not available on a group handle");
    if (int rc = bind_device(h)) return rc;
    if (int rc = join_stripes(h)) return rc;
    if (!h->dTimeline) {
        PT_HIP(h, hipMalloc((void **)&h->dTimeline, (size_t)65536 * 4 * sizeof(unsigned long long)));
        PT_HIP(h, hipMemsetAsync(h->dTimeline, 0, (size_t)65536 * 4 * sizeof(unsigned long long), h->stream));
        return PT_OK;
    }
    PT_HIP(h, hipStreamSynchronize(h->stream));
    if (host_out) PT_HIP(h, hipMemcpy(host_out, h->dTimeline, (size_t)max_waves * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PT_OK;
}

// Tuning aid (not declared in the public header): set one of pt_tuning.hpp's knobs for this process.  The library reads no environment
// variables; this is the only way a knob changes.  Affects renderers created / frames launched afterwards.
extern "C" __attribute__((visibility("default"))) int pt_debug_set(const char *key, long long value)
{
    if (!key || !pt::tuning_set(key, value)) return fail(nullptr, PT_E_BAD_ARGUMENT, "pt_debug_set: unknown knob");
    return PT_OK;
}

// Test aid (not declared in the public header): the hand-over bound's counters of this handle (all parts of a group together).  Drains the
// handle first.  out[0] = (pixel, frame) pairs the repair passes re-rendered, [1] = pixels whose tag fitted nothing the launch sequence can
// have left (must stay 0), [2] = joins that had something to repair, [3] = times the host found the abandon flag raised.
extern "C" __attribute__((visibility("default"))) int pt_debug_handover_stats(pt_handle h, unsigned int out[4])
{
    PT_CHECK_HANDLE(h);
    if (!out) return fail(h, PT_E_BAD_ARGUMENT, "out == NULL");
    if (int rc = pt_synchronize(h)) return rc;
    out[0] = out[1] = out[2] = out[3] = 0;
    std::vector<pt_handle> hs = h->isGroup() ? h->group.parts : std::vector<pt_handle>{h};
    for (pt_handle p : hs) {
        if (int rc = bind_device(p)) return rc;
        unsigned int ctl[4] = {0, 0, 0, 0};
        PT_HIP(h, hipMemcpy(ctl, p->handover.dRepairCtl, sizeof ctl, hipMemcpyDeviceToHost));
        out[0] += ctl[0];
        out[1] += ctl[1];
        out[2] += ctl[2];
        out[3] += p->handover.abandonEpoch;
    }
    return PT_OK;
}

// Test aid (not declared in the public header): how the handle has been launching.  out[0] = pt_render-driven launch_frames calls (a striped
// frame counts once), [1] = 1 while the cached tile masks are valid, [2] = frames accepted by pt_render and not launched yet, [3] = tile-mask
// rebuilds, [4] = frame counter, [5] = flushes forced by an input change (upload / set_params with different values), [6] = frames published into frame-fed launches, [7] = fed
// launches opened, [8] = fed launches that ended idle, [9] = 1 while one is open, [10] = 1 once the host has pipelined frames (single frames then go
// out as tagged launches).  Does not flush or join.
#ifdef PT_FEED_TIMES
extern "C" __attribute__((visibility("default"))) int pt_debug_feed_times(pt_handle h, unsigned int *out128)
{
    for (int i = 0; i < 64; i++) { out128[i] = h->chain.hostStarted[3000 + i]; out128[64 + i] = h->chain.hostStarted[3100 + i]; }
    return PT_OK;
}
#endif
extern "C" __attribute__((visibility("default"))) int pt_debug_launch_stats(pt_handle h, unsigned long long out[12])
{
    PT_CHECK_HANDLE(h);
    if (!out) return fail(h, PT_E_BAD_ARGUMENT, "out == NULL");
    pt_handle r = h->isGroup() ? h->group.parts[0] : h;
    out[0] = r->statLaunches;
    out[1] = r->masks.tileMasksValid ? 1 : 0;
    out[2] = (unsigned long long)r->pipeline.pendingFrames;
    out[3] = r->statMaskBuilds;
    out[4] = (unsigned long long)r->frame;
    out[5] = r->statFlushes;
    out[6] = r->feed.statPublishes;
    out[7] = r->feed.statFeedOpens;
    out[8] = r->feed.statFeedIdle;
    out[9] = r->feed.open ? 1 : 0;
    out[10] = r->pipeline.sawBatch ? 1 : 0;
    out[11] = 0;
    return PT_OK;
}

// Test aid (not declared in the public header): the sphere grid the NEXT launch would use for the current scene.
// out[0..2] = cells per axis, out[3] = sphere references, out[4] = 1 if a grid exists (else the in-order loop runs).
extern "C" __attribute__((visibility("default"))) int pt_debug_sphere_grid(pt_handle h, int out[5])
{
    PT_CHECK_HANDLE(h);
    if (!out) return fail(h, PT_E_BAD_ARGUMENT, "out == NULL");
    pt_handle r = h->isGroup() ? h->group.parts[0] : h;
    const ptgrid::SphereGrid g = r->gridDirty ? ptgrid::build((const float *)r->objectsShadow, r->numSpheres) : r->grid;
    for (int k = 0; k < 3; k++) out[k] = g.dims[k];
    out[3] = g.numRefs;
    out[4] = g.valid ? 1 : 0;
    return PT_OK;
}

// Test aid (not declared in the public header; needs no GPU): build the sphere grid of a std140 GameObjectsUBO on the host.
// header[0..2] = cells per axis, [3] = references, [4] = valid; box[0..2] = lo, [3..5] = hi, [6..8] = centre, [9] = reach^2;
// packed (capacity bytes) receives uint16 starts[cells + 1] followed by uint8 refs[].  Returns the packed size.
extern "C" __attribute__((visibility("default"))) int pt_debug_build_sphere_grid(const float *objects, int num_spheres, int header[5],
                                                                                 float box[10], unsigned char *packed, int capacity)
{
    if (!objects || !header || !box) return PT_E_BAD_ARGUMENT;
    const ptgrid::SphereGrid g = ptgrid::build(objects, num_spheres);
    for (int k = 0; k < 3; k++) {
        header[k] = g.dims[k];
        box[k] = g.lo[k];
        box[3 + k] = g.hi[k];
        box[6 + k] = g.center[k];
    }
    header[3] = g.numRefs;
    header[4] = g.valid ? 1 : 0;
    box[9] = g.reach2;
    if (packed && capacity >= (int)g.packed.size() && !g.packed.empty()) std::memcpy(packed, g.packed.data(), g.packed.size());
    return (int)g.packed.size();
}

// Test aid (not declared in the public header; needs no GPU): the run bits of the in-order sphere loop (FrameArgs::sphereRunStart) for a
// std140 GameObjectsUBO with num_spheres spheres, exactly as ptgrid::sphere_runs hands them to the kernels: bit i of the 256 = sphere i
// starts a new run.
extern "C" __attribute__((visibility("default"))) int pt_debug_sphere_runs(const float *objects, int num_spheres, unsigned long long out[4])
{
    if (!objects || !out) return PT_E_BAD_ARGUMENT;
    ptgrid::sphere_runs(objects, num_spheres, out);
    return PT_OK;
}

// Test aid (not declared in the public header; needs no GPU): the spheres whose packed geometry (pt_kernels.hpp, sphereGeom) an upload of
// [byte_offset, byte_offset + size) into the GameObjectsUBO refreshes — pt::sphere_geom_range, the function pt_upload_game_objects uses.
// out[0] = first sphere, out[1] = count (0: none).
extern "C" __attribute__((visibility("default"))) int pt_debug_sphere_geom_range(int byte_offset, int size, int out[2])
{
    if (!out) return PT_E_BAD_ARGUMENT;
    pt::sphere_geom_range(byte_offset, size, out[0], out[1]);
    return PT_OK;
}

// Test aid (not declared in the public header): the device's UBO 1 (objects_out, PT_GAME_OBJECTS_UBO_SIZE bytes, may be null) and the packed
// sphere geometry behind it (geom_out, 256 x 4 floats, may be null) of part `part` of a group handle (0 for a plain handle), read behind
// everything queued on the handle's stream.
extern "C" __attribute__((visibility("default"))) int pt_debug_read_sphere_geom(pt_handle h, int part, void *objects_out, float *geom_out)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup() ? (part < 0 || part >= (int)h->group.parts.size()) : part != 0) return fail(h, PT_E_BAD_ARGUMENT, "no such part");
    pt_handle r = h->isGroup() ? h->group.parts[(size_t)part] : h;
    if (int rc = bind_device(r)) return rc;
    PT_HIP(h, hipStreamSynchronize(r->stream));
    if (objects_out) PT_HIP(h, hipMemcpy(objects_out, r->dObjects, PT_GAME_OBJECTS_UBO_SIZE, hipMemcpyDeviceToHost));
    if (geom_out) PT_HIP(h, hipMemcpy(geom_out, (const char *)r->dObjects + pt::kSphereGeomOffset, (size_t)pt::kSphereGeomEntries * 16, hipMemcpyDeviceToHost));
    return PT_OK;
}

// Test aid (not declared in the public header; needs no GPU): what launch_integrate would decide (pt::plan_launch) for a launch with
// these arguments and these values of the kernel-selection knobs.  The process-wide knobs are not consulted and nothing is launched.
// kernelRow: the row of the family's dispatch table the plan names (-1: none, or a family without a table).
// Pointers are only ever tested for null: has* = 1 stands for a non-null one (hasFeed: feed words, display images and display flags).
struct pt_debug_plan_in {
    int width, height, tilesX, tilesY, numSpheres, numCuboids, spp, envFormat, variant, batchFrames, tagged, drainCompaction, queueChunk, numCUs,
        gridBytes, hasGrid, hasTimeline, hasStartedFlags, hasFeed, wantFeed;
    // pt_tuning.hpp: parked_max, park_capacity, park_min, no_batch_pass, batch_pass_min_tiles, no_sphere_grid, force_lean_lds, carry_last, grid_carry
    int parkedMax, parkCapacity, parkMin, noBatchPass, batchPassMinTiles, noSphereGrid, forceLeanLds, carryLast, gridCarry;
};
struct pt_debug_plan_out {
    int error, family, kernelRow, minWavesPerSimd, timeline, spp1, matLds, grid, carry, compact, feed, workgroups, ldsBytes, poolTiles;
    unsigned int ticketsConsumed;
    int fed;
    // FrameArgs as the kernel receives it ("set by the launch"); feedSet / displaySet count the non-null feed words and the non-zero display fields
    int materialsInLds, gridLdsBytes, sceneLdsBytes, parkedMax, contCapacity, contBatchMin, drainCompaction, startedFlagsSet;
    unsigned int tilesFrameMagic, tilesXMagic;
    int feedSet, displaySet;
    // the budget the log_launch line prints
    int workgroupsPerCU, batchPass, queueLdsBytes, staticLdsBytes, fitPerCU;
};
extern "C" __attribute__((visibility("default"))) int pt_debug_plan_launch(const pt_debug_plan_in *in, pt_debug_plan_out *out)
{
    if (!in || !out) return PT_E_BAD_ARGUMENT;
    static unsigned char somewhere[16];
    pt::FrameArgs a;
    std::memset(&a, 0, sizeof a);
    a.width = in->width; a.height = a.rows = in->height; a.tilesX = in->tilesX; a.tilesY = in->tilesY;
    a.numSpheres = in->numSpheres; a.numCuboids = in->numCuboids; a.spp = in->spp; a.envFormat = in->envFormat; a.variant = in->variant;
    a.batchFrames = in->batchFrames; a.tagged = in->tagged; a.drainCompaction = in->drainCompaction; a.queueChunk = in->queueChunk;
    a.numCUs = in->numCUs; a.gridBytes = in->gridBytes;
    if (in->hasGrid) a.grid = somewhere;
    if (in->hasTimeline) a.timeline = (unsigned long long *)somewhere;
    if (in->hasStartedFlags) a.startedFlags = (unsigned int *)somewhere;
    if (in->hasFeed) {
        a.feedHost = (const unsigned int *)somewhere; a.feedBcast = (unsigned int *)somewhere; a.feedDone = (unsigned long long *)somewhere;
        a.displayImages[0] = a.displayImages[1] = a.displayImages[2] = (uchar4 *)somewhere; a.displayPrev = 1; a.displayOn = 1;
    }
    pt::Tuning t;
    t.parkedMax = in->parkedMax; t.parkCapacity = in->parkCapacity; t.parkMin = in->parkMin; t.noBatchPass = in->noBatchPass;
    t.batchPassMinTiles = in->batchPassMinTiles; t.noSphereGrid = in->noSphereGrid; t.forceLeanLds = in->forceLeanLds; t.carryLast = in->carryLast;
    t.gridCarry = in->gridCarry;
    const pt::LaunchPlan p = pt::plan_launch(a, t, in->wantFeed != 0);
    const pt::FrameArgs &o = p.args;
    *out = pt_debug_plan_out{(int)p.error, p.family, pt::launch_kernel_row(p), p.kernel.minWavesPerSimd, p.kernel.timeline, p.kernel.spp1, p.kernel.matLds, p.kernel.grid, p.kernel.carry,
                             p.kernel.compact, p.kernel.feed, p.workgroups, (int)p.ldsBytes, p.poolTiles, p.ticketsConsumed, p.fed, o.materialsInLds, o.gridLdsBytes,
                             o.sceneLdsBytes, o.parkedMax, o.contCapacity, o.contBatchMin, o.drainCompaction, o.startedFlags != nullptr, o.tilesFrameMagic, o.tilesXMagic,
                             (o.feedHost != nullptr) + (o.feedBcast != nullptr) + (o.feedDone != nullptr),
                             (o.displayImages[0] != nullptr) + (o.displayImages[1] != nullptr) + (o.displayImages[2] != nullptr) + (o.displayPrev != 0) + (o.displayOn != 0),
                             p.workgroupsPerCU, p.batchPass, (int)p.queueLdsBytes, (int)p.staticLdsBytes, p.fitPerCU};
    return PT_OK;
}

// Test aid (not declared in the public header): the hand-over audit of the -DPT_AUDIT build.  Drains the handle, then copies up to
// max_records violation records (pt::kAuditRecordWords words each) and returns their number (all parts of a group together), or
// -1000 when the library was built without PT_AUDIT.  The log is cleared.
extern "C" __attribute__((visibility("default"))) int pt_debug_audit_read(pt_handle h, unsigned int *out_records, int max_records)
{
    PT_CHECK_HANDLE(h);
#ifndef PT_AUDIT
    (void)out_records;
    (void)max_records;
    return -1000;
#else
    if (int rc = pt_synchronize(h)) return rc;
    int total = 0, copied = 0;
    std::vector<pt_handle> hs = h->isGroup() ? h->group.parts : std::vector<pt_handle>{h};
    for (pt_handle p : hs) {
        volatile unsigned int *log = p->hostAuditLog;
        if (!log) continue;
        const int n = (int)log[0], kept = n < pt::kAuditLogRecords ? n : pt::kAuditLogRecords;
        for (int i = 0; i < kept && copied < max_records && out_records; i++, copied++)
            for (int k = 0; k < pt::kAuditRecordWords; k++)
                out_records[(size_t)copied * pt::kAuditRecordWords + k] = log[4 + (size_t)i * pt::kAuditRecordWords + k];
        total += n;
        log[0] = 0;
    }
    return total;
#endif
}
