// mi355pt_present.cpp — the present path: blocking and non-blocking presents, their slots and the present snapshots.
//
// Owns pt_renderer::Snapshots, the present slots (PresentSlot), dRgba8 and the copy stream's work; reads ::FeedState for the fused display
// (a present entered into the open frame-fed launch).  Calls into mi355pt_launch.cpp (flush_frames*, feed_close) and mi355pt_handover.cpp
// (join_stripes, fix_alpha, settle_handover, note_abandonment, stripe_stream).
#include "pt_renderer.hpp"

#include <chrono>
#include <thread>

using ptimpl::abandon_raised;
using ptimpl::bind_device;
using ptimpl::ensure_rgba8;
using ptimpl::fail;
using ptimpl::flush_frames;
using ptimpl::join_stripes;

namespace ptimpl {

// A present into slot fusedOrphanSlot was left without a successor frame (see feed_close): with every launch joined into h->stream the
// accumulation image IS the frame that was shown — tone-map it the classic way.  Call with the streams joined.
int resolve_fused_orphan(pt_handle h)
{
    if (h->feed.fusedOrphanSlot < 0) return PT_OK;
    FEED_LOG("orphan present of slot %d: tone map from the image", h->feed.fusedOrphanSlot);
    PresentSlot &s = h->slots[h->feed.fusedOrphanSlot];
    h->feed.fusedOrphanSlot = -1;
    if (!s.fusedWaiting) return PT_OK;
    void *const image = s.boundDev ? s.boundDev : s.dRgba8;
    const size_t pixels = (size_t)s.rows * s.width;
    PT_HIP(h, ptimpl::launch_tone_map(s.arithmetic, h->accum(), image, pixels, h->stream));
    PT_HIP(h, hipEventRecord(s.toneMapped, h->stream));
    PT_HIP(h, hipStreamWaitEvent(h->copyStream, s.toneMapped, 0));
    if (!s.boundDev) PT_HIP(h, hipMemcpyAsync(s.host, s.dRgba8, pixels * 4, hipMemcpyDeviceToHost, h->copyStream));
    PT_HIP(h, hipEventRecord(s.copied, h->copyStream));
    s.fusedWaiting = false;
    s.fedPresent = false; // (completed by the events above, like any present tone-mapped behind a join — the join put the repair passes in front)
    s.snapSource = nullptr;
    return PT_OK;
}

int ensure_rgba8(pt_handle h)
{
    size_t need = h->tilePixels();
    if (need > h->rgba8Capacity) {
        if (h->dRgba8) PT_HIP(h, hipStreamSynchronize(h->stream));
        PT_HIP(h, regrow_buffer(h->dRgba8, h->rgba8Capacity, need, need * 4));
    }
    return PT_OK;
}

// PostProcessing/fragment.glsl:17-26 over this handle's rows into `dst`, ordered behind every frame rendered so far
int tone_map_into(pt_handle h, void *dst)
{
    if (int rc = join_stripes(h)) return rc;
    PT_HIP(h, ptimpl::launch_tone_map(h->presentArithmetic, h->accum(), dst, h->tilePixels(), h->stream));
    return PT_OK;
}

int ensure_slot_events(pt_handle h, int slot)
{
    PresentSlot &s = h->slots[slot];
    if (!s.toneMapped) PT_HIP(h, hipEventCreateWithFlags(&s.toneMapped, hipEventDisableTiming));
    if (!s.copied) PT_HIP(h, hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
    return PT_OK;
}

int ensure_slot_device(pt_handle h, int slot, size_t pixels)
{
    PresentSlot &s = h->slots[slot];
    if (pixels > s.devPixels) {
        if (s.dRgba8) {
            if (s.copied && s.inFlight) PT_HIP(h, hipEventSynchronize(s.copied)); // a copy may still read the old buffer
            PT_HIP(h, hipStreamSynchronize(h->stream));
        }
        PT_HIP(h, regrow_buffer(s.dRgba8, s.devPixels, pixels, pixels * 4));
    }
    return PT_OK;
}

int ensure_slot_host(pt_handle h, int slot, size_t pixels)
{
    PresentSlot &s = h->slots[slot];
    if (pixels > s.hostPixels) {
        if (s.host && s.copied && s.inFlight) PT_HIP(h, hipEventSynchronize(s.copied));
        s.valid = false;
        PT_HIP(h, regrow_buffer(s.host, s.hostPixels, pixels, pixels * 4, true));
    }
    return PT_OK;
}

// Launch the pending frames with a present snapshot attached: their launch stores its last frame's pixels into snapshot buffer
// h->snaps.snapNext while it resolves them (FrameArgs::snapshot).  On return h->snaps.snapLaunches lists the launches that write it (empty if
// a kernel variant without snapshot support rendered the frames) and h->snaps.snapFrame is the frame count the snapshot shows.
static int ensure_snapshot_buffer(pt_handle h, int k, size_t pixels)
{
    if (pixels > h->snaps.snapCapacity[k]) {
        // (a launch queued earlier may still write the old buffer, a tone map may still read it: drain the handle's streams first)
        feed_close(h);
        for (int j = 0; j < ptimpl::kMaxStripes; j++)
            if (h->stripes.stripeStream[j]) PT_HIP(h, hipStreamSynchronize(h->stripes.stripeStream[j]));
        PT_HIP(h, hipStreamSynchronize(h->stream));
        PT_HIP(h, hipStreamSynchronize(h->copyStream));
        if (h->snaps.snapReadPending[k]) PT_HIP(h, hipEventSynchronize(h->snaps.snapRead[k]));
        h->snaps.snapReadPending[k] = false;
        PT_HIP(h, regrow_buffer(h->snaps.dSnap[k], h->snaps.snapCapacity[k], pixels, pixels * sizeof(float4)));
    }
    if (!h->snaps.snapRead[k]) PT_HIP(h, hipEventCreateWithFlags(&h->snaps.snapRead[k], hipEventDisableTiming));
    return PT_OK;
}

int flush_with_snapshot(pt_handle h, long waitUs)
{
    const int k = h->snaps.snapNext;
    const size_t pixels = h->tilePixels();
    if (int rc = ensure_snapshot_buffer(h, k, pixels)) return rc;
    h->snaps.snapshotTarget = h->snaps.dSnap[k];
    h->snaps.snapshotIndex = k;
    h->snaps.snapGeneration[k]++;
    h->snaps.snapLaunches.clear();
    h->snaps.snapFrame = -1;
    const int rc = flush_frames_bounded(h, waitUs, 0);
    h->snaps.snapshotTarget = nullptr;
    if (rc) return rc;
    if (!h->snaps.snapLaunches.empty()) {
        h->snaps.snapFrame = h->frame;
        // every snapshot launch takes the next buffer, presented or not: two launches that may run beside each other must never
        // write the same snapshot (their plain stores to one pixel are not ordered by the tags)
        h->snaps.snapNext = (k + 1) % pt_renderer::kSnapshots;
    }
    return PT_OK;
}

// Wait (on the host) until the previous present into slot `s` has left it: an event for the classic paths; for a FUSED present
// (frame-fed launch) the launch's monitor wavefront reports complete frames in a host-mapped word — a fused present whose successor frame
// was never published is first turned into a classic one (close + join: resolve_fused_orphan).  Returns with the slot idle; *abandoned
// is set when a fused present's launch gave up (the caller re-does the image behind a join).
int wait_slot(pt_handle h, PresentSlot &s, bool *abandoned)
{
    if (abandoned) *abandoned = false;
    if (!s.inFlight) return PT_OK;
    if (s.fedPresent && s.fusedWaiting) {
        feed_close(h);
        if (int rc = join_stripes(h)) return rc;
        if (s.fusedWaiting) return fail(h, PT_E_HIP, "present: a fused present was left without its image");
    }
    if (s.fedPresent) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned long spins = 0;; spins++) {
            if (__atomic_load_n(&h->feed.hostFeedDone[s.fusedWord], __ATOMIC_ACQUIRE) >= s.fusedNeed) break;
            if (abandon_raised(h) || h->handover.abandonEpoch != s.abandonEpoch) {
                // its launch was abandoned (a contended device, or it ended idle) — now, or since the present (the host has already noted it)
                if (abandoned) *abandoned = true;
                break;
            }
            if ((spins & 63) == 63) {
                const auto waited = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
                if (waited > 2000000) { // (2 s: nothing of this library takes that long — treat the launch as lost, the join below sorts it out)
                    if (abandoned) *abandoned = true;
                    break;
                }
                if (waited > 100) std::this_thread::yield();
            }
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
        }
    } else {
        PT_HIP(h, hipEventSynchronize(s.copied));
    }
    return PT_OK;
}

void free_slots(pt_handle h)
{
    for (PresentSlot &s : h->slots) {
        if (s.dRgba8) (void)hipFree(s.dRgba8);
        if (s.host) (void)hipHostFree(s.host);
        if (s.toneMapped) (void)hipEventDestroy(s.toneMapped);
        if (s.copied) (void)hipEventDestroy(s.copied);
        s = PresentSlot();
    }
}

} // namespace ptimpl

namespace {

// A present was issued into slot `s`: it now holds frame h->frame of this handle's rows, in flight, in the present arithmetic in force.
// snapSource: what the image is tone-mapped from without a join in between (a snapshot buffer; a fused present's own image), or null
void slot_holds_frame(pt_handle h, ptimpl::PresentSlot &s, const void *snapSource)
{
    s.inFlight = true;
    s.valid = false;
    s.frame = h->frame;
    s.rows = h->rows;
    s.width = h->width;
    s.arithmetic = h->presentArithmetic;
    s.snapSource = snapSource;
}

} // namespace

extern "C" {

PT_API int pt_present_rgba8(pt_handle h, uint8_t *dst, size_t row_pitch_bytes)
{
    PT_CHECK_HANDLE(h);
    if (!dst) return fail(h, PT_E_BAD_ARGUMENT, "dst == NULL");
    size_t rowBytes = (size_t)h->width * 4;
    if (row_pitch_bytes == 0) row_pitch_bytes = rowBytes;
    if (row_pitch_bytes < rowBytes) return fail(h, PT_E_BAD_ARGUMENT, "row pitch smaller than a row");
    if (h->isGroup()) return ptimpl::group_present_rgba8(h, dst, row_pitch_bytes);
    if (int rc = bind_device(h)) return rc;
    if (int rc = ensure_rgba8(h)) return rc;
    if (int rc = ptimpl::tone_map_into(h, h->dRgba8)) return rc; // (behind a join: the hand-over repair passes are in front of the tone map)
    PT_HIP(h, hipMemcpy2DAsync(dst, row_pitch_bytes, h->dRgba8, rowBytes, rowBytes, (size_t)h->rows, hipMemcpyDeviceToHost,
                               h->stream));
    PT_HIP(h, hipStreamSynchronize(h->stream));
    return PT_OK;
}

PT_API int pt_postprocess_device(pt_handle h, void **out_device_ptr, size_t *out_bytes)
{
    PT_CHECK_HANDLE(h);
    if (h->isGroup()) return fail(h, PT_E_BAD_ARGUMENT, "pt_postprocess_device is not available on a group handle");
    if (int rc = bind_device(h)) return rc;
    if (int rc = ensure_rgba8(h)) return rc;
    if (int rc = ptimpl::tone_map_into(h, h->dRgba8)) return rc;
    if (out_device_ptr) *out_device_ptr = h->dRgba8;
    if (out_bytes) *out_bytes = h->tilePixels() * 4;
    return PT_OK;
}

PT_API int pt_present_rgba8_async(pt_handle h, int slot)
{
    PT_CHECK_HANDLE(h);
    if (slot < 0 || slot >= PT_PRESENT_SLOTS) return fail(h, PT_E_BAD_ARGUMENT, "slot must be 0..PT_PRESENT_SLOTS-1");
    if (h->isGroup()) return ptimpl::group_present_async(h, slot);
    if (int rc = bind_device(h)) return rc;
    ptimpl::PresentSlot &s = h->slots[slot];
    const size_t pixels = h->tilePixels();
    h->pipeline.presentCadence = h->pipeline.rendersSincePresent;
    h->pipeline.rendersSincePresent = 0;
    h->pipeline.lastPresentBound = h->slots[slot].boundDev != nullptr;
    // (an open fed launch that does not show its frames itself takes no more of them: this present is about to flush and join — and may
    // allocate first: the launch must not sit waiting for frames meanwhile)
    if (h->feed.open && !h->feed.display) ptimpl::feed_close(h);
    if (int rc = ptimpl::ensure_slot_events(h, slot)) return rc;
    if (s.boundDev) { // the displayed image stays on the device (interop-style present): no slot images of the library's own
        if (s.boundBytes < pixels * 4) return fail(h, PT_E_BAD_ARGUMENT, "bound device image is smaller than rows*width*4 bytes");
    } else {
        if (int rc = ptimpl::ensure_slot_device(h, slot, pixels)) return rc;
        if (int rc = ptimpl::ensure_slot_host(h, slot, pixels)) return rc;
    }
    void *const image = s.boundDev ? s.boundDev : s.dRgba8;
    // ---- snapshot path: the launch of the frames shown writes its last frame into a snapshot buffer while it resolves the pixels;
    // the tone map follows that launch on its stream, the copy on the copy stream, and nothing waits for them: the next pt_render
    // chains its launch beside this one.
    // ---- frame-fed path (round 6), FUSED DISPLAY: the newest frame sits in the open launch.  Nothing is launched, flushed or tone-mapped
    // here: the slot is entered into the feed word, and the tile passes of the NEXT frame — which read every pixel of this one anyway —
    // tone-map it into the slot's image (FrameArgs::displayImages).  The gate that tells when the image is complete is enqueued when that
    // next frame is published (feed_try_publish); if none comes, whoever closes the launch tone-maps the classic way (resolve_fused_orphan).
    if (h->feed.open && h->feed.display && h->pipeline.pendingFrames == 0 && h->feed.pendingSlot < 0 && h->frame == h->feed.firstFrame + h->feed.published &&
        !abandon_raised(h)) {
        pt_renderer::FeedState &f = h->feed;
        if (s.boundDev != nullptr) { // (the launch knows the slots' bound images: binding closes it)
            if (s.inFlight) { // (a host that reuses a slot before having waited for it: wait here)
                if (int rc = ptimpl::wait_slot(h, s, nullptr)) return rc;
                s.inFlight = false;
            }
            if (!f.open) return pt_present_rgba8_async(h, slot); // (the wait closed the launch: the classic way — presentCadence is set again, harmless)
            const int j = f.published - 1;
            f.slots16 = (f.slots16 & ~(3u << (2 * (j & 7)))) | ((unsigned int)(slot + 1) << (2 * (j & 7)));
            f.pendingSlot = slot; // (the word that publishes the next frame carries the entry)
            FEED_LOG("present frame %d into slot %d (fused, waits for the next frame)", h->frame, slot);
            slot_holds_frame(h, s, image); // (snapSource non-null: pt_present_wait looks at the abandon epoch; PT_ARITH_CONTRACT: feed_wanted opens no displaying launch otherwise)
            s.snapGeneration = 0;
            s.abandonEpoch = h->handover.abandonEpoch;
            s.fedPresent = true;
            s.fusedWaiting = true;
            s.fusedWord = f.hostWord;
            s.fusedNeed = (unsigned int)(j + 2); // (frame j + 1 of the launch complete = its tile passes have tone-mapped frame j everywhere)
            return PT_OK;
        }
    }
    if (s.inFlight && s.fedPresent) { // (the slot's previous present was a fused one: no event to order behind — wait for it here)
        if (int rc = ptimpl::wait_slot(h, s, nullptr)) return rc;
        s.inFlight = false;
    }
    s.fedPresent = false;
    const bool snapshotCapable = (h->variant == 0 || h->variant >= 10) && h->arithmetic == PT_ARITH_CONTRACT && !h->externalStream() && !ptimpl::timeline_blocks_pipelining(h);
    if (snapshotCapable && h->pipeline.pendingFrames > 0)
        if (int rc = ptimpl::flush_with_snapshot(h, pt::tuning().renderWaitUs)) return rc;
    if (snapshotCapable && h->pipeline.pendingFrames == 0 && h->snaps.snapFrame == h->frame && !h->snaps.snapLaunches.empty()) {
        // (the frames' launch — flushed just now, or by the pt_render before this call — wrote snapshot buffer snapshotIndex)
        {
            const int k = h->snaps.snapshotIndex;
            // The tone map of a launch's rows runs ON that launch's stream, right behind it (a few microseconds: the kernel raises its
            // wave priority, the next launch is already resident on the other stream).  Only the NEXT-BUT-ONE launch queues behind it.
            // Not on the copy stream: tone map + 150 us copy in one queue would bound the display rate; not on a stream of its own: a
            // fourth busy stream shares a hardware queue with a launch stream and would run behind the next launch.
            // (a slot the host reuses before its previous copy has landed: wait for that copy HERE, on the host — queued on the launch's
            // stream instead, the next-but-one integrator launch would stall behind a PCIe copy.  A host that calls pt_present_wait
            // on a slot before it presents into it again, as the header recommends, never waits here)
            if (s.inFlight && hipEventQuery(s.copied) != hipSuccess) PT_HIP(h, hipEventSynchronize(s.copied));
            (void)hipGetLastError(); // (hipErrorNotReady of the query is not an error)
            for (const pt_renderer::Snapshots::SnapLaunch &l : h->snaps.snapLaunches) {
                PT_HIP(h, ptimpl::launch_tone_map(h->presentArithmetic, h->snaps.dSnap[k] + l.firstPixel, (char *)image + l.firstPixel * 4, l.pixels, l.stream));
                PT_HIP(h, hipEventRecord(l.done, l.stream)); // "launch done" now includes its tone map
                PT_HIP(h, hipStreamWaitEvent(h->copyStream, l.done, 0));
            }
            PT_HIP(h, hipEventRecord(h->snaps.snapRead[k], h->copyStream)); // (behind every tone map that read the snapshot)
            h->snaps.snapReadPending[k] = true;
            if (!s.boundDev) PT_HIP(h, hipMemcpyAsync(s.host, s.dRgba8, pixels * 4, hipMemcpyDeviceToHost, h->copyStream));
            PT_HIP(h, hipEventRecord(s.copied, h->copyStream));
            slot_holds_frame(h, s, h->snaps.dSnap[k]);
            s.snapGeneration = h->snaps.snapGeneration[k];
            s.abandonEpoch = h->handover.abandonEpoch;
            h->snaps.snapFrame = -1; // consumed
            h->snaps.snapLaunches.clear();
            return PT_OK;
        }
    }
    // (nothing pending and no fresh snapshot — the frames were launched by another call, or by a kernel variant that writes none:
    // present from the accumulation image)
    if (int rc = flush_frames(h)) return rc;
    bool striped = false;
    for (int j = 0; j < ptimpl::kMaxStripes; j++) striped = striped || h->stripes.stripePending[j];
    if (striped) {
        // The last frame was launched as row stripes on their own streams.  Tone-map every stripe's rows ON ITS stream:
        // stripe A's next frame then only waits for stripe A's own frame + tone map, never for the other stripe's drain
        // (joining into the main stream here would put a device-wide barrier between consecutive displayed frames).
        for (int j = 0; j < ptimpl::kMaxStripes; j++) {
            if (!h->stripes.stripePending[j]) continue;
            // the slot's previous copy must have left the device image before it is overwritten (device-side wait only)
            hipStream_t st = ptimpl::stripe_stream(h, j);
            if (s.inFlight) PT_HIP(h, hipStreamWaitEvent(st, s.copied, 0));
            const size_t first = (size_t)h->stripes.stripeRow0[j] * h->width, count = (size_t)h->stripes.stripeRows[j] * h->width;
            PT_HIP(h, ptimpl::launch_tone_map(h->presentArithmetic, h->accum() + first, (char *)image + first * 4, count, st));
            PT_HIP(h, hipEventRecord(h->stripes.stripeDone[j], st)); // "stripe done" now includes its tone map
            PT_HIP(h, hipStreamWaitEvent(h->copyStream, h->stripes.stripeDone[j], 0));
        }
    } else {
        if (int rc = join_stripes(h)) return rc;
        if (s.inFlight) PT_HIP(h, hipStreamWaitEvent(h->stream, s.copied, 0));
        PT_HIP(h, ptimpl::launch_tone_map(h->presentArithmetic, h->accum(), image, pixels, h->stream));
        PT_HIP(h, hipEventRecord(s.toneMapped, h->stream));
        // later frames only wait for the tone-map pass (stream order); the PCIe copy runs beside them on the copy stream
        PT_HIP(h, hipStreamWaitEvent(h->copyStream, s.toneMapped, 0));
    }
    if (!s.boundDev) PT_HIP(h, hipMemcpyAsync(s.host, s.dRgba8, pixels * 4, hipMemcpyDeviceToHost, h->copyStream));
    PT_HIP(h, hipEventRecord(s.copied, h->copyStream));
    slot_holds_frame(h, s, nullptr); // (tone-mapped from the accumulation image behind a join: the repair passes ran in front of it)
    return PT_OK;
}

PT_API int pt_present_bind_device_image(pt_handle h, int slot, void *device_rgba8, size_t bytes)
{
    PT_CHECK_HANDLE(h);
    if (slot < 0 || slot >= PT_PRESENT_SLOTS) return fail(h, PT_E_BAD_ARGUMENT, "slot must be 0..PT_PRESENT_SLOTS-1");
    if (h->isGroup()) return fail(h, PT_E_BAD_ARGUMENT, "pt_present_bind_device_image is not available on a group handle");
    if (device_rgba8 && bytes < h->tilePixels() * 4) return fail(h, PT_E_BAD_ARGUMENT, "device image smaller than rows*width*4 bytes");
    if (int rc = bind_device(h)) return rc;
    ptimpl::PresentSlot &s = h->slots[slot];
    if (h->feed.open || h->feed.fusedOrphanSlot >= 0) { // (an open fed launch writes the slots' images as they were when it started)
        ptimpl::feed_close(h);
        if (int rc = join_stripes(h)) return rc;
    }
    if (s.inFlight) { // a present into the slot's previous image may still be running
        if (int rc = ptimpl::wait_slot(h, s, nullptr)) return rc;
        s.inFlight = false;
    }
    s.valid = false;
    s.fedPresent = false;
    s.boundDev = device_rgba8;
    s.boundBytes = device_rgba8 ? bytes : 0;
    return PT_OK;
}

PT_API int pt_present_wait(pt_handle h, int slot, const uint8_t **out_host_rgba8, size_t *out_row_pitch_bytes,
                           int *out_frame_index)
{
    PT_CHECK_HANDLE(h);
    if (slot < 0 || slot >= PT_PRESENT_SLOTS) return fail(h, PT_E_BAD_ARGUMENT, "slot must be 0..PT_PRESENT_SLOTS-1");
    ptimpl::PresentSlot &s = h->slots[slot];
    if (!s.inFlight && !s.valid) return fail(h, PT_E_BAD_ARGUMENT, "nothing was presented into this slot");
    if (int rc = bind_device(h)) return rc;
    if (s.inFlight) {
        // (a fused present whose successor frame has not been published: nobody will tone-map it on the device — wait_slot closes the launch
        // and joins: resolve_fused_orphan tone-maps the frame from the accumulation image, which holds exactly that frame)
        bool fusedAbandoned = false;
        if (int rc = ptimpl::wait_slot(h, s, &fusedAbandoned)) return rc;
        if (fusedAbandoned) s.abandonEpoch = h->handover.abandonEpoch - 1; // (the image is re-done below, behind a join)
        s.inFlight = false;
        s.valid = true;
        // The image's frames are complete (the copy stream is behind them).  An image tone-mapped behind a JOIN had the hand-over repair
        // passes in front of its tone map (group handles, presents from the accumulation image).  A SNAPSHOT present has no join: if a
        // launch of the handle was abandoned since the tone map was enqueued, the snapshot may lack pixels — repair (the pass also
        // completes the snapshot of the launch that wrote it), tone-map again, copy again.
        if (!h->isGroup() && s.snapSource != nullptr) {
            if (abandon_raised(h)) {
                if (int rc = join_stripes(h)) return rc;
                if (abandon_raised(h)) ptimpl::note_abandonment(h);
            }
            if (s.abandonEpoch != h->handover.abandonEpoch && s.fedPresent) {
                // a frame-fed launch was abandoned (a hand-over out of its budget, or it ended idle while this frame was being published):
                // the snapshot may lack pixels and its buffer may already hold later frames.  Behind the join the accumulation image is
                // complete (repair passes): show THAT — every frame rendered so far, at least the frame this slot was presented at
                if (int rc = ptimpl::fix_alpha(h)) return rc;
                void *const image = s.boundDev ? s.boundDev : s.dRgba8;
                const size_t pixels = (size_t)s.rows * s.width;
                PT_HIP(h, ptimpl::launch_tone_map(s.arithmetic, h->accum(), image, pixels, h->stream));
                if (!s.boundDev) PT_HIP(h, hipMemcpyAsync(s.host, s.dRgba8, pixels * 4, hipMemcpyDeviceToHost, h->stream));
                PT_HIP(h, hipStreamSynchronize(h->stream));
                if (int rc = ptimpl::settle_handover(h)) return rc;
                s.abandonEpoch = h->handover.abandonEpoch;
                s.frame = h->frame;
            } else if (s.abandonEpoch != h->handover.abandonEpoch) {
                int k = -1;
                for (int i = 0; i < pt_renderer::kSnapshots; i++)
                    if (h->snaps.dSnap[i] == s.snapSource && h->snaps.snapGeneration[i] == s.snapGeneration) k = i;
                if (k < 0)
                    return fail(h, PT_E_HIP, "present: a launch was abandoned and this slot's snapshot has been reused (call pt_present_wait on a slot before presenting into it again)");
                if (int rc = join_stripes(h)) return rc;
                void *const image = s.boundDev ? s.boundDev : s.dRgba8;
                const size_t pixels = (size_t)s.rows * s.width;
                PT_HIP(h, ptimpl::launch_tone_map(s.arithmetic, h->snaps.dSnap[k], image, pixels, h->stream));
                if (!s.boundDev) PT_HIP(h, hipMemcpyAsync(s.host, s.dRgba8, pixels * 4, hipMemcpyDeviceToHost, h->stream));
                PT_HIP(h, hipStreamSynchronize(h->stream));
                s.abandonEpoch = h->handover.abandonEpoch;
            }
        }
    }
    if (out_host_rgba8) *out_host_rgba8 = s.boundDev ? nullptr : s.host; // (a bound slot's image is in the caller's device memory)
    if (out_row_pitch_bytes) *out_row_pitch_bytes = (size_t)s.width * 4;
    if (out_frame_index) *out_frame_index = s.frame;
    return PT_OK;
}

PT_API int pt_present_set_arithmetic(pt_handle h, int mode)
{
    PT_CHECK_HANDLE(h);
    if (mode != PT_ARITH_CONTRACT && mode != PT_ARITH_REFERENCE) return fail(h, PT_E_BAD_ARGUMENT, "mode must be PT_ARITH_CONTRACT or PT_ARITH_REFERENCE");
    PT_FAN_OUT(h, pt_present_set_arithmetic(part, mode));
    if (mode == h->presentArithmetic) return PT_OK; // (a host that sets the mode every frame keeps its pipelining: nothing to order)
    if (int rc = bind_device(h)) return rc;
    // pending frames are launched and an open frame-fed launch is closed: a present it still owes (fused display) is tone-mapped in the
    // arithmetic it was issued under (PresentSlot::arithmetic), and no displaying launch stays open across the switch (feed_wanted)
    if (int rc = join_stripes(h)) return rc;
    h->presentArithmetic = mode; // (the accumulation image, the frame counter, the environment and the two other switches are untouched)
    return PT_OK;
}

} // extern "C"
