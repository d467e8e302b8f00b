// mi355pt_launch.cpp — the frame pipeline: pt_render, the deferred frames and the three ways a launch reaches the GPU.
//
// Owns pt_renderer::Pipeline, ::Chain, ::TileMasks and ::FeedState (the frame-fed launch), and writes ::Stripes' per-launch fields.  Calls
// into mi355pt_handover.cpp (join_stripes, ensure_stripe, arm_handover, remember_launch, note_abandonment, next_launch_event) and
// mi355pt_present.cpp (flush_with_snapshot: a host that presents every frame gets its frame launched with a snapshot attached).
#include "pt_renderer.hpp"

#include <chrono>
#include <cstring>
#include <thread>

using ptimpl::abandon_raised;
using ptimpl::arm_handover;
using ptimpl::bind_device;
using ptimpl::fail;
using ptimpl::flush_frames;
using ptimpl::hip_fail;
using ptimpl::join_stripes;
using ptimpl::remember_launch;

namespace ptimpl {

// The open frame-fed launch takes no more frames: the host word gets its final count (| kFeedClosed), and everything that depended on
// that count is settled — the launch's repair record, the ticket counter of its stream, the running totals of the per-frame counters.
unsigned int feed_word(const pt_renderer::FeedState &f, bool closed)
{
    return (closed ? pt::kFeedClosed : 0u) | ((unsigned int)f.published << 16) | (f.slots16 & 0xffffu);
}

void feed_close(pt_handle h)
{
    pt_renderer::FeedState &f = h->feed;
    if (!f.open) return;
    f.open = false;
    __atomic_store_n(&h->feed.hostFeed[f.hostWord], feed_word(f, true), __ATOMIC_RELEASE);
    FEED_LOG("close word %d = %08x (first %d published %d pendingSlot %d)", f.hostWord, feed_word(f, true), f.firstFrame, f.published, f.pendingSlot);
    for (pt_renderer::Handover::LaunchRecord &r : h->handover.unverified)
        if (r.a.launchSeq == f.seq) r.a.batchFrames = f.published;
    const unsigned int tickets = (unsigned int)(((long long)f.published * f.tilesFrame + f.queueChunk - 1) / f.queueChunk); // (+ one failing ticket per workgroup: added at the launch)
    queue_base(h, f.streamIdx) += tickets;
    for (int j = 0; j < f.published; j++) h->feed.feedDoneBase[f.streamIdx][j & 7] += f.pixelsPerFrame;
    if (f.published >= 8) h->feed.feedIdleStrikes = 0; // (the host kept a launch fed: not a slow host)
    // fused display: the newest frame was presented, and no later frame of this launch will come to tone-map it — the next join does
    // (from the accumulation image, before anything else is rendered: whoever closes a launch joins, or launches through launch_frames)
    if (f.pendingSlot >= 0) {
        h->feed.fusedOrphanSlot = f.pendingSlot;
        f.pendingSlot = -1;
    }
}

} // namespace ptimpl

namespace {

bool gpu_busy(pt_handle h);

// ---------------------------------------------------------------------------------------------------------------------------------------
// Launching frames [firstFrame, firstFrame + n) with the handle's current inputs, in steps (round 6: what used to be one 326-line function):
//   fill_frame_args      the inputs as the kernels take them (+ the sphere grid of a changed scene)
//   choose_launch_mode   tagged or plain, stripes, kernel variant, workgroups per CU
//   use_tile_masks       cached per-tile cull masks: use / rebuild
//   wait_for_residency   launch chaining: may this launch run BESIDE its predecessor?
//   arm_handover         sequence number + abandon word of a tagged launch; remember_launch: the record its repair pass needs
//   launch_chained / launch_single_stream / launch_striped     the three ways a launch reaches the GPU
// launch_frames() strings them together.  waitUs: how long the call may wait for the predecessor launch to become resident;
// lastOfFlush: this launch holds the newest pending frame (only it may store alpha = 1 last / write a present snapshot).
struct LaunchMode {
    bool tagged = false, chainable = false;
    int stripes = 1, kernelVariant = 0;
};

// Tiles per frame below which a pipelined launch takes 4 tiles per global ticket instead of 8: a small share of an image (a 1/8 share of
// 1080p has 4,050 tiles per frame for 6,144 wavefronts) then keeps fewer frames in flight at once (+5 % there, neutral above).  (The same
// number as the carry threshold of plan_launch and Tuning::feedMinTiles, but a decision of its own.)
constexpr long long kSmallChunkBelowTiles = 12000;
// Tiles per frame below which a handle owns "a small share of an image" (1/8 of 1080p: 4,050): ONE meaning at its three sites — overlapping
// launches lose there, so wait_for_residency does not wait to chain, pt_render does not hold a full batch back for residency, and
// batch_limit makes up for the launch boundaries with 256-frame launches.
constexpr long long kSmallShareBelowTiles = 12000;

// a launch went out on launch stream si (0 = main, 1 = chain) with `done` recorded behind it: what gpu_busy and the next join look at
void note_launch_done(pt_handle h, int si, hipEvent_t done)
{
    if (si == 1) {
        h->chain.chainDone = done;
        h->chain.chainInFlight = h->chain.chainPending = true;
    } else {
        h->chain.mainDone = done;
        h->chain.mainInFlight = true;
    }
}

// ---- step 1: inputs -> FrameArgs (everything that does not depend on how the launch reaches the GPU)
int fill_frame_args(pt_handle h, pt::FrameArgs &a, int firstFrame, int n)
{
    std::memcpy(a.invProj, h->basic, 64);
    std::memcpy(a.invView, h->basic + 64, 64);
    std::memcpy(a.viewPos, h->basic + 128, 12);
    a.focalLength = h->focalLength;
    a.apertureDiameter = h->apertureDiameter;
    a.width = h->width;
    a.height = h->height;
    a.invW = 1.0f / (float)h->width; // (correctly rounded, like the device's f_div_ieee)
    a.invH = 1.0f / (float)h->height;
    a.numSpheres = h->numSpheres;
    a.numCuboids = h->numCuboids;
    a.rayDepth = h->rayDepth;
    a.spp = h->spp;
    a.frame = firstFrame;
    a.batchFrames = n;
    a.envSize = h->envSize;
    a.envFormat = h->envFormat;
    a.objects = h->dObjects; // (the block AND sphereGeom behind it, pt_kernels.hpp kSphereGeomOffset: `objects` always names an allocation of 26,624 + 4,096 bytes)
    a.env = h->dEnv;
    a.srgbLut = h->dLut;
    a.tilesX = h->tilesX();
    a.bandRows = h->bandRows;
    a.bandWorld = h->bandWorld;
    a.bandRank = h->bandRank;
    a.localRow0 = 0;
    a.numCUs = h->numCUs;
    // tiles per global ticket: 8, or 4 for a pipelined launch over a small share of an image (kSmallChunkBelowTiles)
    a.queueChunk = h->queueChunk > 0 ? h->queueChunk : (n > 1 && h->tilesPerFrame() < kSmallChunkBelowTiles ? 4 : 8);
    a.errorWord = h->handover.devErrWord;
    a.startedFlags = nullptr;
    a.launchSeq = 0;
    a.snapshot = nullptr; // (set next to every a.accum when the launch feeds a present)
    a.audit = nullptr;    // (set next to every a.accum)
    a.auditLog = h->devAuditLog;
    a.auditSabotage = 0;
#ifdef PT_AUDIT
    a.auditSabotage = pt::tuning().auditSabotage;
#endif
    a.timeline = h->dTimeline;
    // sphere grid of large scenes: rebuilt here, before the first launch that sees the changed scene.  Launches still in flight
    // read the old grid: join first, then the copy is ordered behind them on the main stream like a scene upload.
    if (h->gridDirty) {
        h->gridDirty = false;
        h->grid = ptgrid::build((const float *)h->objectsShadow, h->numSpheres);
        ptgrid::sphere_runs((const float *)h->objectsShadow, h->numSpheres, h->sphereRunStart);
        if (h->grid.valid) {
            if (int rc = join_stripes(h)) return rc;
            PT_HIP(h, hipMemcpyAsync(h->dGrid, h->grid.packed.data(), h->grid.packed.size(), hipMemcpyHostToDevice, h->stream));
        }
    }
    a.grid = h->grid.valid ? h->dGrid : nullptr;
    a.gridBytes = h->grid.valid ? (int)h->grid.packed.size() : 0;
    a.gridLdsBytes = 0;
    for (int k = 0; k < 3; k++) {
        a.gridDims[k] = h->grid.dims[k];
        a.gridLo[k] = h->grid.lo[k];
        a.gridHi[k] = h->grid.hi[k];
        a.gridCell[k] = h->grid.cell[k];
        a.gridInvCell[k] = h->grid.invCell[k];
        a.gridCenter[k] = h->grid.center[k];
    }
    a.gridReach2 = h->grid.reach2;
    std::memcpy(a.sphereRunStart, h->sphereRunStart, sizeof(a.sphereRunStart));
    a.tileMasks = nullptr; // (use_tile_masks: only launches that run the tile pass over the handle's whole tile)
    a.tagged = 0;
    a.keepTags = 0;
    a.chainTag = 0.0f;
    a.abandonWord = nullptr;
    a.tileFlags = nullptr;
    a.waitBudget = h->handover.waitBudgetUnits;
    a.waitCheckInterval = h->handover.waitCheckUnits;
    return PT_OK;
}

// ---- step 2: how the frames reach the GPU
// variant -> (kernel variant, stripes): 0 = default (2 stripes x 5 workgroups/CU); 20+k / 30+k / 40+k = 2 / 3 / 4
// stripes of the persistent kernel with k+1 workgroups per CU; everything else = one kernel on the main stream.
// Tagged launches (pixels handed over through alpha tags): every launch of more than one frame, and — once the host has
// pipelined frames on this handle — single frames too, so that they can overlap the launches around them (a host that
// presents every frame, or only ever renders one frame at a time, keeps the faster single-frame stripes) ... and single frames
// whenever the GPU still runs earlier frames of this handle: the frame then chains on the other stream and moves into the wavefront
// slots the previous launch's drain frees (0.154 ms per 1080p frame against 0.182 for the two row stripes); a host that lets the GPU
// run dry between its frames (blocking reads / presents) keeps the stripes, which are the faster way to render ONE frame on an idle machine.
LaunchMode choose_launch_mode(pt_handle h, pt::FrameArgs &a, int n)
{
    LaunchMode m;
    m.kernelVariant = h->variant;
    if (h->arithmetic != PT_ARITH_CONTRACT) { // the reference-arithmetic kernel: one plain launch per frame on the main stream
        m.chainable = false;
        m.tagged = false;
        m.stripes = 1;
        m.kernelVariant = 1;
        a.variant = m.kernelVariant;
        a.drainCompaction = 0;
        a.tagged = 0;
        return m;
    }
    const bool noSingleTagged = pt::tuning().noSingleTagged != 0; // A/B runs
    m.chainable = h->variant == 0 && !h->externalStream() && !ptimpl::timeline_blocks_pipelining(h);
    // (also the first frame of a burst on an idle GPU once the host has pipelined frames before: the batch that follows then chains
    // on it instead of waiting behind two joined stripes — the driver's `--steps 20` command: 15.4 instead of 14.8 Gsamples/s)
    m.tagged = h->variant == 0 && (n > 1 || (m.chainable && !noSingleTagged && (gpu_busy(h) || (h->pipeline.sawBatch && h->pipeline.presentCadence != 1))));
    // (short launches — the interactive modes — take 5 workgroups per CU: 112 instead of 32 free VGPRs per SIMD leave the present's
    // tone map and the runtime's copy kernel room BESIDE the resident persistent wavefronts; 6 per CU starve them until the drain,
    // measured: 0.28 instead of 0.16 ms per displayed frame; a single frame also renders 2 % faster with 5)
    const int shortWg = pt::tuning().shortWorkgroupsPerCU;
    if (m.tagged) { m.stripes = 1; m.kernelVariant = 10 + (n < 8 ? shortWg : h->pipeline.batchWorkgroupsPerCU) - 1; h->pipeline.batchLaunched = true; if (n > 1) h->pipeline.sawBatch = true; }
    else if (h->variant == 0 && h->externalStream()) { m.stripes = 1; m.kernelVariant = 14; } // everything ON the caller's stream
    else if (h->variant == 0) { m.stripes = 2; m.kernelVariant = 14; }
    else if (h->variant >= 20 && h->variant < 50) { m.stripes = h->variant / 10; m.kernelVariant = 10 + h->variant % 10; }
    if (h->rows < 16 * m.stripes) m.stripes = 1; // tiny tiles: not worth splitting
    a.variant = m.kernelVariant;
    // Drain compaction (a thin draining wavefront donates its paths to its workgroup's pool) shortens the tail of ONE
    // launch.  With stripes the tail of one launch is covered by the other stripe's (or the next frame's) main phase, and
    // the pool's LDS and the donor traffic only cost: auto = on for single-launch variants, off for striped frames.
    a.drainCompaction = h->drainCompaction >= 0 ? h->drainCompaction : (m.stripes > 1 || m.tagged ? 0 : 32); // a batch drains once per n frames
    a.tagged = m.tagged ? 1 : 0;
    return m;
}

// ---- step 3: cached tile masks (the tile pass of the spp = 1 kernels, the fresh-tile batch passes of the spp > 1 kernel): valid masks are
// simply used; stale ones are rebuilt once the camera / lens / spheres / tiling have been left alone for two launches — the launches still
// in flight read the old buffer, so the rebuild joins the two launch streams first (chainBroken: this launch then starts on the main
// stream, behind the mask kernel).  Call with a.tilesX / a.tilesY / a.y0 / a.rows set.
int use_tile_masks(pt_handle h, pt::FrameArgs &a)
{
    if (pt::tuning().tileMasks == 0) return PT_OK;
    // (counted in FRAMES since round 6 — a frame-fed launch takes up to 64 frames: a host that moves the camera every frame still never
    // gets here with more than one)
    const bool settled = h->masks.launchesSinceInputChange > 2;
    h->masks.launchesSinceInputChange += a.batchFrames;
    if (!h->masks.tileMasksValid && settled) {
        if (int rc = join_stripes(h)) return rc;
        // (the buffer is sized by ensure_accum with the image: nothing is allocated on the render path)
        if ((size_t)a.tilesX * a.tilesY <= h->masks.tileMaskTiles) {
            PT_HIP(h, pt::launch_tile_masks(a, h->masks.dTileMasks, h->stream));
            h->masks.tileMasksValid = true;
            h->statMaskBuilds++;
        }
    }
    if (h->masks.tileMasksValid) a.tileMasks = h->masks.dTileMasks;
    return PT_OK;
}

// ---- step 4: residency.  A launch may run BESIDE its predecessor (on the other stream) only if that launch is fully resident — then it
// can only ever get the slots the predecessor's workgroups give up when they are done; otherwise it goes behind it on the same stream (no
// overlap, always safe).  After an abandonment the device is evidently contended: for a while launches run behind their predecessor.
bool predecessor_resident(pt_handle h)
{
    for (int i = 0; i < h->chain.lastWorkgroups; i++)
        if (((volatile unsigned int *)h->chain.hostStarted)[i] != h->chain.launchSeq) return false;
    return true;
}
bool wait_for_residency(pt_handle h, const pt::FrameArgs &a, long waitUs)
{
    if (pt::tuning().serialLaunches != 0) return false; // (A/B and profile runs: strictly one launch after the other)
    if (h->handover.overlapHoldoff > 0) h->handover.overlapHoldoff--;
    const bool mayChain = !h->chain.chainBroken && h->chain.lastWorkgroups > 0 && h->chain.lastWorkgroups <= ptimpl::kStartedWords && h->handover.overlapHoldoff == 0;
    bool resident = mayChain && predecessor_resident(h);
    // (small shares — a 1/8 share of 1080p has 4,050 tiles per frame — lose 4 % when two launches overlap: the second launch's first
    // frames all wait for the first one's last; measured, tools/emulate_strong.py)
    const bool bigShare = (long long)a.tilesX * a.tilesY >= kSmallShareBelowTiles;
    if (mayChain && !resident && (bigShare || h->pipeline.flushFinal)) {
        // Back-pressure (round 3): the host is more than one launch ahead of the GPU — the predecessor still queues behind ITS
        // predecessor.  Launching behind it on the same stream would expose a full drain + ramp per launch (0.096 ms at 1080p);
        // instead the call waits until the predecessor is resident (i.e. until the launch before it has left the machine) and
        // then chains.  Bounded, so a GPU shared with another process falls back to the always-safe same-stream order.  Round 5:
        // pt_render itself no longer waits here — it keeps frames pending until the predecessor is resident (launch_ready) and
        // only a call that blocks anyway (pt_synchronize, a read, a present) waits, for at most chain_wait_us.
        const auto t0 = std::chrono::steady_clock::now();
        while (!resident) {
            const auto waited = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
            if (waited >= waitUs) break;
            if (waited > 200) std::this_thread::sleep_for(std::chrono::microseconds(20)); // (long waits: do not burn the core)
            resident = predecessor_resident(h);
        }
    }
    return resident;
}

// ---- frame-fed launches (pt_renderer.hpp: FeedState).  Wanted when few frames go out and nothing says the host is about to join: the
// reference's own usage.  Conditions that only cost speed elsewhere: one sample per pixel (the tile-pass kernels), a full-size share.
bool feed_wanted(pt_handle h, const pt::FrameArgs &a, int n, bool lastOfFlush)
{
    if (pt::tuning().feed == 0 || pt::tuning().serialLaunches != 0 || n >= 8 || !lastOfFlush || h->pipeline.flushFinal || a.spp != 1 || (long long)a.tilesX * a.tilesY < pt::tuning().feedMinTiles) return false;
    // ... and a host that has turned deferral OFF (pt_set_frame_batch(1): every Render() is handed to the GPU at once — the interactive
    // setting).  With deferral allowed, frames that arrive while the GPU is busy are collected and go out as one classic launch, which has the
    // lower fixed cost (no open / close hand-shake: the driver's `--steps 20` command measures 17.45 that way against 16.69 Gsamples/s fed)
    if (!h->snaps.snapshotTarget && !(h->pipeline.maxBatchExplicit && h->pipeline.maxBatch == 1)) return false;
    if (h->feed.feedHoldoff > 0) { // (a host too slow to keep a launch fed: see note_abandonment)
        h->feed.feedHoldoff--;
        return false;
    }
    if (h->snaps.snapshotTarget) {
        // A host that shows every frame: the launch tone-maps into the present slots' images itself (fused display) — for slots whose image
        // stays on the device (pt_present_bind_device_image: the interop-style present).  A slot with a host image needs the runtime's copy
        // kernel per frame, which finds no room beside resident wavefronts (measured: it ran when the launch ended) and is PCIe-bound
        // anyway (0.157 ms per 1080p frame): such hosts keep the per-frame launches.
        // The fused display is the CONTRACT tone map (display_pixel in pt_integrate_persistent.hip): a handle whose presents are in the
        // reference arithmetic (pt_present_set_arithmetic) keeps the snapshot / per-frame presents, which launch the kernel of its choice.
        if (pt::tuning().feedDisplay == 0 || n != 1 || !h->pipeline.lastPresentBound || h->presentArithmetic != PT_ARITH_CONTRACT) return false;
        for (const ptimpl::PresentSlot &s : h->slots)
            if (s.boundDev && s.boundBytes < h->tilePixels() * 4) return false;
    }
    return true;
}

// Turn `a` (a chained launch of frames [firstFrame, firstFrame + n) on stream st = launch stream si) into a frame-fed launch: capacity
// kFeedCapacity, n frames published, control words initialised.  *word = the host word it reads, or -1 when none is free (no fed launch now).
int feed_prepare(pt_handle h, pt::FrameArgs &a, int si, hipStream_t st, int firstFrame, int n, int *word)
{
    *word = -1;
    const int w = h->feed.feedWordNext % pt_renderer::kFeedHostWords;
    if (!h->feed.feedWordBusy[w]) PT_HIP(h, hipEventCreateWithFlags(&h->feed.feedWordBusy[w], hipEventDisableTiming));
    else if (hipEventQuery(h->feed.feedWordBusy[w]) != hipSuccess) { // (the launch that read this word eight fed launches ago still runs)
        (void)hipGetLastError();
        return PT_OK;
    }
    if (h->feed.feedCountersStale) {
        // an abandoned launch left the per-frame counters short of the running totals: start them again from zero — only with nothing of
        // the handle in flight that counts or compares them (else: no fed launch yet; the next join resets them as well)
        if (gpu_busy(h) || hipStreamQuery(h->copyStream) != hipSuccess) {
            (void)hipGetLastError();
            return PT_OK;
        }
        PT_HIP(h, hipMemsetAsync(h->feed.dFeedDone, 0, (size_t)16 * pt::kFeedDoneStride * sizeof(unsigned long long), st));
        std::memset(h->feed.feedDoneBase, 0, sizeof h->feed.feedDoneBase);
        h->feed.feedCountersStale = false;
    }
    h->feed.feedWordNext++;
    pt_renderer::FeedState &f = h->feed;
    f.published = n;
    f.slots16 = 0;
    f.pendingSlot = -1;
    f.display = h->snaps.snapshotTarget != nullptr;
    __atomic_store_n(&h->feed.hostFeedDone[w], 0u, __ATOMIC_RELEASE);
    __atomic_store_n(&h->feed.hostFeed[w], ((unsigned int)n << 16), __ATOMIC_RELEASE);
    a.feedHostDone = h->feed.devFeedHostDone + w;
    std::memcpy(a.feedBase, h->feed.feedDoneBase[si], sizeof a.feedBase);
    a.feedPixels = (unsigned long long)h->tilePixels();
    unsigned int *const bcast = h->feed.dFeedDev + (size_t)si * pt::kFeedBcastSlots * pt::kFeedBcastStride; // (one set of broadcast slots per launch stream)
    PT_HIP(h, hipMemsetAsync(bcast, 0, (size_t)pt::kFeedBcastSlots * pt::kFeedBcastStride * sizeof(unsigned int), st)); // (behind the previous launch of this stream)
    a.batchFrames = pt::kFeedCapacity;
    a.keepTags = 1; // (which frame is the last is not known when the launch starts: the host restores alpha = 1 before anything observes the image)
    const int wg = pt::tuning().feedWorkgroupsPerCU;
    a.variant = 10 + (wg >= 1 && wg <= 6 ? wg : 6) - 1;
    a.feedHost = h->feed.devFeedHost + w;
    a.feedBcast = bcast;
    a.feedDone = h->feed.dFeedDone + (size_t)8 * pt::kFeedDoneStride * si;
    const long idleUs = pt::tuning().feedIdleUs;
    a.feedIdleTicks = (unsigned int)((double)(idleUs < 1 ? 1 : (idleUs > 10000000 ? 10000000 : idleUs)) * h->handover.wallClockKhz / 1000.0); // (ticks of the constant-rate counter: 100 MHz on gfx950)
    a.displayImages[0] = a.displayImages[1] = a.displayImages[2] = nullptr;
    a.displayPrev = 0;
    a.displayOn = f.display && pt::tuning().feedDisplay != 2 ? 1 : 0; // (feed_display = 2: debug — the protocol without the tone map)
    if (f.display)
        for (int i = 0; i < PT_PRESENT_SLOTS; i++) a.displayImages[i] = (uchar4 *)h->slots[i].boundDev; // (null: an unbound slot is never entered into the feed word)
    a.snapshot = nullptr;
    f.hostWord = w;
    *word = w;
    return PT_OK;
}

// pt_render with a fed launch open: publish the newest frame (h->frame - 1) into it.  False = it could not take the frame (it has been
// closed: the caller goes on as if there had been none).
bool feed_try_publish(pt_handle h, bool presentsEveryFrame)
{
    pt_renderer::FeedState &f = h->feed;
    const int frame = h->frame - 1;
    const bool ok = f.open && f.published < pt::kFeedCapacity && frame == f.firstFrame + f.published && h->pipeline.pendingFrames == 1 &&
                    f.display == presentsEveryFrame && !abandon_raised(h);
    if (!ok) {
        FEED_LOG("publish refused: open %d published %d frame %d first %d pending %d display %d/%d flag %u", (int)f.open, f.published, frame, f.firstFrame, h->pipeline.pendingFrames,
                 (int)f.display, (int)presentsEveryFrame, h->handover.hostErrWord ? *(volatile unsigned int *)h->handover.hostErrWord : 0u);
        ptimpl::feed_close(h);
        return false;
    }
    // (a launch opened right after an input change runs without cached tile masks: once the inputs have been left alone, let the next
    // launch build them — one launch boundary for ~7 % on every frame after it)
    if (!f.withMasks && pt::tuning().tileMasks != 0 && !h->masks.tileMasksValid && h->masks.launchesSinceInputChange > 2 && f.published >= 3 && f.pendingSlot < 0) {
        ptimpl::feed_close(h);
        return false;
    }
    h->masks.launchesSinceInputChange++;
    const int j = f.published; // this frame's index in the launch
    f.slots16 &= ~(3u << (2 * (j & 7))); // (the entry of frame j - 8 becomes frame j's: not shown so far)
    f.published++;
    __atomic_store_n(&h->feed.hostFeed[f.hostWord], ptimpl::feed_word(f, false), __ATOMIC_RELEASE);
    h->pipeline.pendingFrames = 0;
    h->chain.lastTag = 2.0f + (float)(frame & pt::kFrameTagMask);
    h->snaps.snapFrame = -1;
    h->feed.statPublishes++;
    FEED_LOG("publish frame %d: word %d = %08x pendingSlot %d", frame, f.hostWord, ptimpl::feed_word(f, false), f.pendingSlot);
    if (f.pendingSlot >= 0) { // the frame before this one was presented: its image is complete when this frame is (the launch's monitor says when)
        h->slots[f.pendingSlot].fusedWaiting = false;
        f.pendingSlot = -1;
    }
    return true;
}

// ---- step 6a: chained launch — alternate between the main stream and the chain stream; the pixels' alpha tags order it behind the
// previous launch (which may still be draining on the other stream), nothing else does
int launch_chained(pt_handle h, pt::FrameArgs &a, int firstFrame, int n, long waitUs, bool lastOfFlush)
{
    a.y0 = h->y0;
    a.rows = h->rows;
    a.accum = h->accum();
    a.audit = h->dAudit;
    a.snapshot = h->snaps.snapshotTarget;
    a.tilesY = h->tilesY();
    a.keepTags = (h->pipeline.flushFinal && lastOfFlush) ? 0 : 1;
    if (!lastOfFlush) a.snapshot = nullptr; // (the snapshot shows the flush's LAST frame)
    if (int rc = use_tile_masks(h, a)) return rc;
    const bool resident = wait_for_residency(h, a, waitUs);
    int si = resident ? (h->chain.lastStreamIdx ^ 1) : h->chain.lastStreamIdx;
    if (h->chain.chainBroken) {
        // something else happened since the last tagged launch (an upload, a read, a striped frame ...): it was joined into
        // the main stream; start there again, and let the chain stream see those inputs before its next launch
        if (int rc = join_stripes(h)) return rc;
        si = 0;
        PT_HIP(h, hipEventRecord(h->stripes.inputsReady, h->stream));
        h->chain.chainNeedsInputs = true;
    }
    a.chainTag = h->chain.tagsLive ? h->chain.lastTag : 0.0f;
    hipStream_t st = h->stream;
    if (si == 1) {
        // the chain stream IS the helper stream of stripe 1: the library keeps at most three streams busy (main, this one, copy) —
        // HIP multiplexes streams onto 4 hardware queues, and two of the library's streams that share a queue execute in order
        if (int rc = ptimpl::ensure_stripe(h, 1)) return rc;
        st = h->stripes.stripeStream[1];
        if (h->chain.chainNeedsInputs) {
            PT_HIP(h, hipStreamWaitEvent(st, h->stripes.inputsReady, 0));
            h->chain.chainNeedsInputs = false;
        }
    }
    a.startedFlags = h->chain.devStarted;
    arm_handover(h, a);
    a.queue = ptimpl::queue_word(h, si); // each launch stream draws tickets from its own counter
    a.queueBase = ptimpl::queue_base(h, si);
    unsigned int tickets = 0;
    int workgroups = 0;
    // a frame-fed launch when the host is not far ahead (few frames, not the flush of a call that joins next); else — or when this
    // kernel configuration has no fed instantiation — the classic launch of exactly these n frames
    bool fed = false;
    if (feed_wanted(h, a, n, lastOfFlush)) {
        const pt::FrameArgs classic = a;
        int word = -1;
        if (int rc = feed_prepare(h, a, si, st, firstFrame, n, &word)) return rc;
        if (word >= 0) {
            fed = true;
            const hipError_t e = pt::launch_integrate(a, st, &tickets, &workgroups, &fed);
            if (e != hipSuccess && e != hipErrorNotSupported) return hip_fail(h, e, "launch_integrate (frame-fed)");
            if (e != hipSuccess) {
                fed = false;
                h->feed.feedHoldoff = 256; // (this scene's kernel has no fed instantiation: do not prepare one per launch)
            }
            (void)hipGetLastError();
        }
        if (!fed) a = classic;
    }
    if (!fed) {
        if (a.snapshot && h->snaps.snapReadPending[h->snaps.snapshotIndex]) PT_HIP(h, hipStreamWaitEvent(st, h->snaps.snapRead[h->snaps.snapshotIndex], 0));
        PT_HIP(h, pt::launch_integrate(a, st, &tickets, &workgroups));
    }
    ptimpl::queue_base(h, si) += tickets;
    h->chain.lastWorkgroups = workgroups;
    h->chain.lastStreamIdx = si;
    hipEvent_t done = ptimpl::next_launch_event(h);
    if (!done) return fail(h, PT_E_HIP, "hipEventCreate failed");
    PT_HIP(h, hipEventRecord(done, st));
    remember_launch(h, a, done);
    note_launch_done(h, si, done);
    if (a.snapshot) h->snaps.snapLaunches.push_back({st, done, 0, h->tilePixels()});
    if (fed) { // pt_render publishes the frames that follow into this launch (feed_try_publish) until something closes it
        pt_renderer::FeedState &f = h->feed;
        PT_HIP(h, hipEventRecord(h->feed.feedWordBusy[f.hostWord], st));
        f.open = true;
        f.firstFrame = firstFrame;
        f.published = n;
        f.streamIdx = si;
        f.seq = a.launchSeq;
        f.workgroups = workgroups;
        f.queueChunk = a.queueChunk;
        f.tilesFrame = (long long)a.tilesX * a.tilesY;
        f.pixelsPerFrame = (unsigned long long)h->tilePixels();
        f.withMasks = a.tileMasks != nullptr;
        std::memcpy(f.base, h->feed.feedDoneBase[si], sizeof f.base);
        h->feed.statFeedOpens++;
        FEED_LOG("open: first %d n %d stream %d word %d display %d wg %d", firstFrame, n, si, f.hostWord, (int)f.display, workgroups);
    }
    h->chain.chainBroken = false; // (join_stripes above set it; this launch re-opens the chain)
    h->stripes.mainDirty = true;    // a striped frame that follows must order its helper stripe behind this launch
    h->chain.tagsLive = a.keepTags != 0;
    h->chain.lastTag = 2.0f + (float)((firstFrame + n - 1) & pt::kFrameTagMask); // pt::frame_tag of the launch's last frame
    return PT_OK;
}

// ---- step 6b: one kernel on the main stream (A/B variants, caller-owned streams)
int launch_single_stream(pt_handle h, pt::FrameArgs &a, const LaunchMode &m)
{
    if (int rc = join_stripes(h)) return rc;
    h->chain.tagsLive = false; // (the plain path stores alpha = 1 for every pixel; a tagged launch of an A/B variant stores 1 last)
    a.y0 = h->y0;
    a.rows = h->rows;
    a.accum = h->accum();
    a.audit = h->dAudit;
    a.snapshot = m.kernelVariant >= 10 ? h->snaps.snapshotTarget : nullptr; // (only the persistent kernels write snapshots)
    if (a.snapshot && h->snaps.snapReadPending[h->snaps.snapshotIndex]) PT_HIP(h, hipStreamWaitEvent(h->stream, h->snaps.snapRead[h->snaps.snapshotIndex], 0));
    a.tilesY = h->tilesY();
    a.queue = ptimpl::queue_word(h, 0);
    a.queueBase = ptimpl::queue_base(h, 0);
    if (m.tagged) arm_handover(h, a); // (a tagged launch of an A/B variant: alone on the main stream, but its frames still hand pixels over)
    unsigned int tickets = 0;
    if (h->arithmetic != PT_ARITH_CONTRACT) PT_HIP(h, pt::launch_integrate_reference(a, h->stream)); // (draws no tickets)
    else PT_HIP(h, pt::launch_integrate(a, h->stream, &tickets));
    ptimpl::queue_base(h, 0) += tickets; // unsigned wrap-around is fine: the kernel subtracts queueBase modulo 2^32
    hipEvent_t done = ptimpl::next_launch_event(h);
    if (!done) return fail(h, PT_E_HIP, "hipEventCreate failed");
    PT_HIP(h, hipEventRecord(done, h->stream));
    if (m.tagged) remember_launch(h, a, done);
    note_launch_done(h, 0, done);
    if (a.snapshot) h->snaps.snapLaunches.push_back({h->stream, h->chain.mainDone, 0, h->tilePixels()});
    return PT_OK;
}

// ---- step 6c: one frame as row stripes, each on its own stream.  Inputs uploaded on the main stream (scene, environment, clears) must
// be visible to the stripe streams; a stripe's frame f+1 follows its own frame f in stream order, which is the only dependency between
// frames (the helpers only wait when something other than stripe 0's own frames went onto the main stream since the last striped frame:
// stripe 0 runs there, and the helper stripes must not wait for ITS previous frame — overlapping one stripe's drain with the other's
// main phase is the point of the stripes)
int launch_striped(pt_handle h, pt::FrameArgs &a, const LaunchMode &m)
{
    if (h->chain.chainPending || h->chain.tagsLive) { // a chained launch may still run on the chain stream: the stripes read its pixels plainly
        if (int rc = join_stripes(h)) return rc;
        h->chain.tagsLive = false; // every pixel gets alpha = 1 from this frame
    }
    const bool orderHelpers = h->stripes.mainDirty;
    if (orderHelpers) PT_HIP(h, hipEventRecord(h->stripes.inputsReady, h->stream));
    h->stripes.mainDirty = false;
    for (int j = 0; j < m.stripes; j++) {
        int r0 = (int)((long long)h->rows * j / m.stripes), r1 = (int)((long long)h->rows * (j + 1) / m.stripes);
        r0 &= ~7; // stripe boundaries on 8-row tile boundaries (the last stripe takes the ragged remainder)
        if (j + 1 < m.stripes) r1 &= ~7;
        if (r1 <= r0) continue;
        a.y0 = h->y0 + r0;
        a.localRow0 = r0;
        a.rows = r1 - r0;
        a.accum = h->accum() + (size_t)r0 * h->width;
        a.audit = h->dAudit ? h->dAudit + (size_t)r0 * h->width : nullptr;
        a.snapshot = h->snaps.snapshotTarget ? h->snaps.snapshotTarget + (size_t)r0 * h->width : nullptr;
        a.tilesY = (a.rows + 7) / 8;
        a.queue = h->dQueue + 16 * j;
        a.queueBase = h->stripes.stripeQueueBase[j];
        if (int rc = ptimpl::ensure_stripe(h, j)) return rc;
        h->stripes.stripeRow0[j] = r0;
        h->stripes.stripeRows[j] = r1 - r0;
        hipStream_t st = ptimpl::stripe_stream(h, j);
        if (j > 0 && orderHelpers) PT_HIP(h, hipStreamWaitEvent(st, h->stripes.inputsReady, 0));
        if (a.snapshot && h->snaps.snapReadPending[h->snaps.snapshotIndex]) PT_HIP(h, hipStreamWaitEvent(st, h->snaps.snapRead[h->snaps.snapshotIndex], 0));
        unsigned int tickets = 0;
        PT_HIP(h, pt::launch_integrate(a, st, &tickets));
        h->stripes.stripeQueueBase[j] += tickets;
        PT_HIP(h, hipEventRecord(h->stripes.stripeDone[j], st));
        if (a.snapshot) h->snaps.snapLaunches.push_back({st, h->stripes.stripeDone[j], (size_t)r0 * h->width, (size_t)(r1 - r0) * h->width});
        h->stripes.stripePending[j] = true;
        h->stripes.stripeInFlight[j] = true;
    }
    return PT_OK;
}

int launch_frames(pt_handle h, int firstFrame, int n, long waitUs, bool lastOfFlush)
{
    if (int rc = bind_device(h)) return rc;
    h->statLaunches++;
    if (!h->snaps.snapshotTarget) h->snaps.snapFrame = -1; // frames rendered without a present snapshot: an older snapshot no longer shows the image
    pt::FrameArgs a;
    if (int rc = fill_frame_args(h, a, firstFrame, n)) return rc;
    const LaunchMode m = choose_launch_mode(h, a, n);
    if (m.tagged && abandon_raised(h)) {
        // a launch of this handle was abandoned: put its repair (and that of everything launched since) behind a join before anything new
        // builds on those frames
        if (int rc = join_stripes(h)) return rc;
        if (abandon_raised(h)) ptimpl::note_abandonment(h);
    }
    if (m.tagged && m.chainable) return launch_chained(h, a, firstFrame, n, waitUs, lastOfFlush);
    if (m.stripes == 1) return launch_single_stream(h, a, m);
    return launch_striped(h, a, m);
}

// Is an integrator launch of this handle still running (or queued) on the GPU?  Cheap event queries, no waiting.
bool gpu_busy(pt_handle h)
{
    bool busy = false;
    if (h->chain.mainInFlight) {
        if (hipEventQuery(h->chain.mainDone) == hipErrorNotReady) busy = true;
        else h->chain.mainInFlight = false;
    }
    if (h->chain.chainInFlight) {
        if (hipEventQuery(h->chain.chainDone) == hipErrorNotReady) busy = true;
        else h->chain.chainInFlight = false;
    }
    for (int j = 0; j < ptimpl::kMaxStripes; j++) {
        if (!h->stripes.stripeInFlight[j]) continue;
        if (hipEventQuery(h->stripes.stripeDone[j]) == hipErrorNotReady) busy = true;
        else h->stripes.stripeInFlight[j] = false;
    }
    return busy;
}

} // namespace

namespace ptimpl {

int plain_frame_args(pt_handle h, pt::FrameArgs &a, int frame)
{
    std::memset(&a, 0, sizeof a);
    if (int rc = fill_frame_args(h, a, frame, 1)) return rc;
    a.variant = 1;
    a.y0 = h->y0;
    a.rows = h->rows;
    a.accum = h->accum();
    a.tilesY = h->tilesY();
    a.queue = h->dQueue;
    return PT_OK;
}

// frames one launch may hold for this handle right now (pt_set_frame_batch; automatic: 64, or 256 on a small share)
int batch_limit(pt_handle h)
{
    if (h->arithmetic != PT_ARITH_CONTRACT) return 1; // (the reference-arithmetic kernel renders one frame per launch)
    // (a GPU that owns a small share of the image — fewer than 12,000 tiles per frame, e.g. 1/8 of 1080p — pipelines up to 256 frames
    // per launch when the batch size was left at its default: every launch boundary costs ~0.1 ms of drain + ramp, 7 % of a 64-frame
    // launch there; spp > 1 keeps 64, its kernels carry the frame index in 7 bits)
    if (!h->pipeline.maxBatchExplicit && h->spp == 1 && h->tilesPerFrame() < kSmallShareBelowTiles) return 256;
    return h->pipeline.maxBatch < 1 ? 1 : h->pipeline.maxBatch;
}

// Would a tagged launch issued now start BESIDE its predecessor (the predecessor is resident), or on an idle chain?  (Otherwise it would
// have to queue behind it on the same stream, or wait: pt_render keeps the frames pending instead.)
bool launch_ready(pt_handle h)
{
    if (h->chain.chainBroken || h->chain.lastWorkgroups <= 0 || h->chain.lastWorkgroups > kStartedWords || h->handover.overlapHoldoff > 0 || pt::tuning().serialLaunches != 0) return true; // (no chaining decision to wait for)
    return predecessor_resident(h);
}

// Launch the pending frames, oldest first, in launches of at most batch_limit() frames.  waitUs: how long EACH launch may wait for its
// predecessor to become resident (pt_render passes 0 or a small bound and relies on launch_ready(); blocking entry points pass the
// tuning knob chain_wait_us).  maxLaunches > 0: stop after that many launches (the rest stays pending).
int flush_frames_bounded(pt_handle h, long waitUs, int maxLaunches)
{
    feed_close(h); // (whoever flushes is about to launch, or to change an input: the open fed launch takes no more frames)
    const int limit = batch_limit(h);
    int launches = 0;
    while (h->pipeline.pendingFrames > 0 && (maxLaunches <= 0 || launches < maxLaunches)) {
        const int pending = h->pipeline.pendingFrames;
        // (only the default kernel pipelines: any other configuration never has more than one frame pending)
        const int n = pending < limit ? pending : limit;
        const int first = h->frame - pending;
        h->pipeline.pendingFrames = 0; // (launch_frames calls join_stripes, which flushes what is pending: nothing, while this launch is built)
        const int rc = launch_frames(h, first, n, waitUs, pending == n);
        h->pipeline.pendingFrames = pending - n;
        if (rc) return rc;
        launches++;
    }
    return PT_OK;
}

int flush_frames(pt_handle h) { return flush_frames_bounded(h, pt::tuning().chainWaitUs, 0); }

} // namespace ptimpl

extern "C" {

PT_API int pt_render(pt_handle h, int *out_total_samples)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) {
        int total = 0;
        for (pt_handle part : h->group.parts) {
            int rc = pt_render(part, &total);
            if (rc != PT_OK) return fail(h, rc, part->error);
        }
        h->frame = h->group.parts[0]->frame;
        if (out_total_samples) *out_total_samples = total;
        return PT_OK;
    }
    if (h->adaptiveLive()) return fail(h, PT_E_BAD_ARGUMENT, "adaptive accumulation in progress: pt_reset first");
    if (!h->dEnv) return fail(h, PT_E_NO_ENVIRONMENT, "pt_render called before pt_set_environment / pt_atmosphere_render");
    if (h->boundAccum && h->boundBytes < h->tilePixels() * sizeof(float4))
        return fail(h, PT_E_BAD_ARGUMENT, "bound result buffer is smaller than the tile");
    // Only the default kernel pipelines frames; the A/B variants launch at once.  On a caller-owned stream nothing is
    // deferred: the contract there is that the frame is enqueued on that stream when pt_render returns.
    // A host that presents EVERY frame (MainWindow.cs:49-56) gains nothing from holding a frame back — the present that
    // follows launches it anyway — and loses if it waits for a present slot in between (the GPU would run dry): launch at once.
    // (only the first pt_render after a present is treated that way: a host that goes on rendering without presenting gets
    // its frames pipelined again)
    const bool presentsEveryFrame = h->pipeline.presentCadence == 1 && h->pipeline.rendersSincePresent == 0;
    const bool batchable = h->variant == 0 && h->arithmetic == PT_ARITH_CONTRACT && h->pipeline.maxBatch > 1 && !ptimpl::timeline_blocks_pipelining(h) && !h->externalStream() && !presentsEveryFrame;
    h->pipeline.rendersSincePresent++;
    h->pipeline.pendingFrames++;
    h->frame++; // PathTracer.cs:117 post-increment
    if (out_total_samples) *out_total_samples = h->frame * h->spp; // PathTracer.cs:112
    // Round 6: a frame-fed launch is open — this frame is PUBLISHED into it (one store to a host-mapped word; the resident wavefronts
    // start it when they run out of earlier work) instead of being launched.  If it cannot take the frame it is closed, and the frame
    // goes the usual way below.
    if (h->feed.open && feed_try_publish(h, presentsEveryFrame)) return PT_OK;
    // Round 3: a host that presents every frame through pt_present_rgba8_async gets this frame launched with a present snapshot
    // attached: the launch stores the frame's pixels a second time while it resolves them (FrameArgs::snapshot), the present that
    // follows tone-maps that copy, and the tone map never stands between two frames.  (Launched NOW, not by the present: a host
    // that first waits for a present slot and then presents must find the GPU busy.  If no present follows, the copy is ignored.)
    if (presentsEveryFrame && (h->variant == 0 || h->variant >= 10) && h->arithmetic == PT_ARITH_CONTRACT && !h->externalStream() && !ptimpl::timeline_blocks_pipelining(h))
        return ptimpl::flush_with_snapshot(h, pt::tuning().renderWaitUs);
    // Frames are only held back while the GPU still has integrator work of this handle in flight: deferring can then
    // never idle the device, and a host that leaves time between its frames gets every frame launched at once.
    if (!batchable) return flush_frames(h);
    if (!gpu_busy(h)) return ptimpl::flush_frames_bounded(h, 0, 0); // (idle device: nothing to wait for)
    const int limit = ptimpl::batch_limit(h);
    if (h->pipeline.pendingFrames < limit) return PT_OK;
    // A full batch.  Round 5: pt_render never sits in the back-pressure wait (it was up to chain_wait_us = 60 ms): the batch is launched
    // when it can start beside its predecessor (that one is resident: the launch before it has left the machine); until then the
    // frames simply stay pending — the GPU has two launches' worth of work queued, nothing idles — and whichever call comes next
    // looks again.  Only a host that runs more than 16 launches ahead is held, for at most 2 ms per call, and then queues the batch
    // behind its predecessor.
    // (a small share — fewer than 12,000 tiles — never waited: its launches go behind each other unless the predecessor happens to be
    // resident, which is what it measures best with: tools/emulate_strong.py)
    const bool bigShare = h->tilesPerFrame() >= kSmallShareBelowTiles;
    // (a limit the host set itself bounds latency AND deferral: such a batch is launched at the limit, behind its predecessor if need be)
    if (!bigShare || h->pipeline.maxBatchExplicit || ptimpl::launch_ready(h)) return ptimpl::flush_frames_bounded(h, 0, 1);
    if (h->pipeline.pendingFrames >= 16 * limit) {
        // a host that runs this far ahead is paced: the call waits (at most render_wait_us = 2 ms) for the moment the batch can start beside
        // its predecessor and launches it then; if that moment does not come in time the frames simply stay pending — never a launch BEHIND
        // the predecessor from here (that order costs a drain + ramp per launch: 1.4 % at 1080p; measured as a 2.4 % lower steady rate
        // when this path still did it)
        const long limitUs = pt::tuning().renderWaitUs;
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            if (ptimpl::launch_ready(h)) return ptimpl::flush_frames_bounded(h, 0, 1);
            const auto waited = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
            if (waited >= limitUs) break;
            std::this_thread::sleep_for(std::chrono::microseconds(waited > 200 ? 50 : 5));
        }
    }
    return PT_OK;
}

PT_API int pt_set_frame_batch(pt_handle h, int max_frames)
{
    PT_CHECK_HANDLE(h);
    if (max_frames < 0 || max_frames > 64) return fail(h, PT_E_BAD_ARGUMENT, "max_frames must be 0..64");
    PT_FAN_OUT(h, pt_set_frame_batch(part, max_frames));
    if (int rc = flush_frames(h)) return rc;
    h->pipeline.maxBatch = max_frames > 0 ? max_frames : 64;
    h->pipeline.maxBatchExplicit = max_frames > 0; // (a limit the host asked for bounds latency and deferral: never raised behind its back; 0 = automatic again)
    return PT_OK;
}

} // extern "C"
