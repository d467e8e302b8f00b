// mi355pt_handover.cpp — joins and the hand-over bound.
//
// Owns pt_renderer::Handover (abandon flag, remembered launches, repair passes, launch-event ring), the join of the handle's streams
// (join_stripes, settle_handover, fix_alpha) and the stripe streams (ensure_stripe, stripe_stream).  Calls into mi355pt_launch.cpp
// (feed_close, flush_frames: a join launches what is pending first) and mi355pt_present.cpp (resolve_fused_orphan, behind a join).
#include "pt_renderer.hpp"

#include <cstring>

namespace ptimpl {

hipEvent_t next_launch_event(pt_handle h)
{
    hipEvent_t &e = h->handover.launchEvents[h->handover.launchEventNext++ % pt_renderer::kLaunchEvents];
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
    return e;
}

// Hand-over repair: the launches since the last join, in launch order, behind the joined streams (call with the helper streams joined
// into h->stream).  On the device each pass is a single load unless a launch was abandoned (pt_repair_kernel).
static int enqueue_repairs(pt_handle h, bool flagWasDown)
{
    // flagWasDown (the caller has NOT just found and cleared the abandon flag): launches seen COMPLETE with the flag DOWN — read in that
    // order: an abandoning launch raises the flag before it ends — ran to their end and need no pass: a host that joins often (a blocking
    // present per frame) enqueues nothing at all on the usual path.  (After note_abandonment the flag is down because the HOST cleared it:
    // then every remembered launch gets its pass.)
    if (flagWasDown) {
        while (!h->handover.unverified.empty() && hipEventQuery(h->handover.unverified.front().done) == hipSuccess && !abandon_raised(h)) {
            FEED_LOG("repairs: launch %u frames [%d,+%d) seen complete with the flag down: no pass", h->handover.unverified.front().a.launchSeq, h->handover.unverified.front().a.frame, h->handover.unverified.front().a.batchFrames);
            h->handover.unverified.pop_front();
        }
        (void)hipGetLastError(); // (hipErrorNotReady of the query is not an error)
    }
    // (nothing remembered and no abandonment noted: nothing to do.  An abandonment noted with nothing remembered — the launches it belongs to
    // had their passes enqueued by an earlier join, before they gave up — still gets the closing kernel: the device's abandon word and
    // ticket counters must never stay behind a flag the host has cleared)
    if (h->handover.unverified.empty() && flagWasDown) return PT_OK;
    for (const pt_renderer::Handover::LaunchRecord &r : h->handover.unverified) {
        FEED_LOG("repairs: pass for launch %u frames [%d,+%d) chainTag %g keepTags %d variant %d", r.a.launchSeq, r.a.frame, r.a.batchFrames, (double)r.a.chainTag, r.a.keepTags, r.a.variant);
        PT_HIP(h, pt::launch_repair(r.a, h->handover.dRepairCtl, h->stream));
    }
    PT_HIP(h, pt::launch_repair_done(h->handover.dAbandon, queue_word(h, 0), queue_base(h, 0), queue_word(h, 1), queue_base(h, 1),
                                     h->handover.dRepairCtl, h->stream));
    h->handover.unverified.clear();
    if (h->feed.feedCountersStale && h->feed.dFeedDone) {
        // an abandoned frame-fed launch counted fewer pixels than the host's running totals say: the counters start again from zero —
        // behind everything joined into h->stream, and behind the gates and tone maps still queued on the copy stream
        if (!h->feed.feedResetEvent) PT_HIP(h, hipEventCreateWithFlags(&h->feed.feedResetEvent, hipEventDisableTiming));
        PT_HIP(h, hipEventRecord(h->feed.feedResetEvent, h->copyStream));
        PT_HIP(h, hipStreamWaitEvent(h->stream, h->feed.feedResetEvent, 0));
        PT_HIP(h, hipMemsetAsync(h->feed.dFeedDone, 0, (size_t)16 * pt::kFeedDoneStride * sizeof(unsigned long long), h->stream));
        std::memset(h->feed.feedDoneBase, 0, sizeof h->feed.feedDoneBase);
        h->feed.feedCountersStale = false;
    }
    return PT_OK;
}

// The host found the abandon flag raised: from here on the device is treated as contended (launches of this handle no longer overlap for a
// while), and present slots tone-mapped from a snapshot since the last epoch are tone-mapped again when they are waited for.
void note_abandonment(pt_handle h)
{
    const unsigned int why = *(volatile unsigned int *)h->handover.hostErrWord;
    *(volatile unsigned int *)h->handover.hostErrWord = 0;
    FEED_LOG("abandon flag %u seen and cleared (frame %d, %zu launches remembered, feed open %d published %d)", why, h->frame, h->handover.unverified.size(), (int)h->feed.open, h->feed.published);
    h->handover.abandonEpoch++;
    // a hand-over that ran out of its budget = a contended device: launches stop overlapping for a while.  A frame-fed launch that ended
    // itself because no frame came (reason "idle") says nothing about the device — only about the host's pace: a host whose fed launches
    // end idle after a frame or two is too slow to feed a resident launch, and gets the classic launches for a (growing) while
    if (why & pt::kAbandonContended) h->handover.overlapHoldoff = 256;
    if (why & pt::kAbandonIdle) {
        h->feed.statFeedIdle++;
        if (h->feed.published <= 2) {
            h->feed.feedIdleStrikes++;
            if (h->feed.feedIdleStrikes >= 2) h->feed.feedHoldoff = h->feed.feedIdleStrikes >= 10 ? 4096 : (16 << (h->feed.feedIdleStrikes - 2));
        } else {
            h->feed.feedIdleStrikes = 0;
        }
    }
    h->feed.feedCountersStale = true; // (an abandoned fed launch counted fewer pixels than the host's running totals say)
    h->handover.repairPendingAll = true; // (the flag is down again because the host cleared it: the launches remembered now all get their repair pass)
    h->handover.repairCheckDue = true; // the next blocking call looks at what the repair passes found (settle_handover)
}

// Launch what pt_render deferred, then make the main stream wait for every stripe kernel still in flight (before
// anything that reads their output or overwrites their inputs).
int join_stripes(pt_handle h, bool repairNow)
{
    FEED_LOG("join (repairNow %d, frame %d, pending %d, tagsLive %d, %zu remembered, flag %u)", (int)repairNow, h->frame, h->pipeline.pendingFrames, (int)h->chain.tagsLive, h->handover.unverified.size(),
             h->handover.hostErrWord ? *(volatile unsigned int *)h->handover.hostErrWord : 0u);
    feed_close(h);
    if (h->pipeline.pendingFrames > 0) {
        // whatever follows a join is ordered by the streams again, so this launch need not leave its tags in the image: its
        // last frame stores the reference's alpha = 1 and the usual render-N-then-read sequence needs no alpha pass at all
        h->pipeline.flushFinal = true;
        int rc = flush_frames(h);
        h->pipeline.flushFinal = false;
        if (rc) return rc;
    }
    h->snaps.snapFrame = -1;   // whoever joins may change the image or the frame counter: a present snapshot written earlier is stale
    h->stripes.mainDirty = true; // whoever joins is about to put other work on the main stream: the next striped frame orders behind it
    h->chain.chainBroken = true; // ... and the next tagged launch re-joins the two launch streams before it starts
    if (h->chain.chainPending) {
        PT_HIP(h, hipStreamWaitEvent(h->stream, h->chain.chainDone, 0));
        h->chain.chainPending = false;
    }
    for (int j = 0; j < kMaxStripes; j++) {
        if (h->stripes.stripePending[j]) {
            if (j > 0) PT_HIP(h, hipStreamWaitEvent(h->stream, h->stripes.stripeDone[j], 0)); // (stripe 0 runs on the main stream itself)
            h->stripes.stripePending[j] = false;
        }
    }
    // hand-over repair of the launches since the last join (everything they wrote is behind h->stream now).  A caller that synchronises
    // h->stream next and then calls settle_handover() leaves it to that — unless the image still carries tags: the alpha pass that
    // follows such a join would wipe out what the repair reads.
    const bool raised = abandon_raised(h);
    if (raised || (!h->handover.unverified.empty() && (repairNow || h->chain.tagsLive))) {
        if (raised) note_abandonment(h);
        if (int rc = enqueue_repairs(h, !raised && !h->handover.repairPendingAll)) return rc;
        h->handover.repairPendingAll = false;
    }
    return resolve_fused_orphan(h);
}

// h->stream has been synchronised behind join_stripes(h, false): every launch of the handle is complete.  Usually that is all there is
// to know (flag down: forget the launches); an abandoned launch is repaired here, behind one more synchronisation.
int settle_handover(pt_handle h)
{
    if (abandon_raised(h)) {
        note_abandonment(h);
        // (the launches the flag belongs to may already have been repaired by an earlier join; then only the closing kernel runs)
        if (int rc = enqueue_repairs(h, false)) return rc;
        h->handover.repairPendingAll = false;
        PT_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (!h->handover.unverified.empty()) FEED_LOG("settle: %zu launches forgotten (synchronised, flag down)", h->handover.unverified.size());
    h->handover.unverified.clear();
    if (h->handover.repairCheckDue) {
        // Repair passes ran since the last look (rare: a contended device).  A pixel whose tag fits nothing the launch sequence can have
        // left means the image cannot be trusted: that is an error of the call that observes it, not a debug counter.
        h->handover.repairCheckDue = false;
        unsigned int ctl[4] = {0, 0, 0, 0};
        PT_HIP(h, hipMemcpy(ctl, h->handover.dRepairCtl, sizeof ctl, hipMemcpyDeviceToHost));
        if (ctl[1] != h->handover.inconsistentSeen) {
            h->handover.inconsistentSeen = ctl[1];
            return fail(h, PT_E_HIP, "hand-over repair: a pixel's frame tag fits no launch of this handle (image inconsistent; pt_reset / pt_set_size start over)");
        }
    }
    return PT_OK;
}

// The host is about to observe the accumulation image (read it, hand out its pointer, synchronise on a bound buffer):
// chained launches leave frame tags in its alpha channel, the reference's constant is 1 (compute.glsl:129).
int fix_alpha(pt_handle h, bool repairNow)
{
    if (int rc = join_stripes(h, repairNow)) return rc;
    if (h->chain.tagsLive) {
        PT_HIP(h, pt::launch_set_alpha(h->accum(), h->tilePixels(), h->stream));
        h->chain.tagsLive = false;
    }
    return PT_OK;
}

// Stripe 0 of a striped frame runs on the handle's main stream, stripe j > 0 on helper stream j, created on first use.  HIP
// multiplexes streams onto a few hardware queues (4 by default) and two streams that share a queue execute in order: the
// fewer streams the library keeps busy, the smaller the chance that two of its concurrent launches (the two stripes, or a
// stripe and the present copy) end up behind each other — the default frame needs main + 1 helper (+ the copy stream).
int ensure_stripe(pt_handle h, int j)
{
    if (j > 0 && !h->stripes.stripeStream[j]) PT_HIP(h, hipStreamCreateWithFlags(&h->stripes.stripeStream[j], hipStreamNonBlocking));
    if (!h->stripes.stripeDone[j]) PT_HIP(h, hipEventCreateWithFlags(&h->stripes.stripeDone[j], hipEventDisableTiming));
    return PT_OK;
}

hipStream_t stripe_stream(pt_handle h, int j) { return j == 0 ? h->stream : h->stripes.stripeStream[j]; }

// ---- step 5: the hand-over bound's bookkeeping (pt_renderer.hpp).  A tagged launch gets a sequence number and the handle's abandon word
// (call with a.chainTag / a.keepTags set), and is remembered — its kernel argument and an event behind it — until a join has put its
// repair pass behind it or it is seen complete with the flag down.
void arm_handover(pt_handle h, pt::FrameArgs &a)
{
    a.launchSeq = ++h->chain.launchSeq;
    if (a.launchSeq == 0 || a.launchSeq >= 0xfffffff0u) a.launchSeq = h->chain.launchSeq = 1; // (0: a fresh roll call; ~0: "no launch abandoned")
    a.abandonWord = h->handover.dAbandon;
    a.tileFlags = a.chainTag == 0.0f ? h->handover.dTileFlags : nullptr; // (the first launch of a chain: alpha = 1 could mean "untouched" or "finished")
}
void remember_launch(pt_handle h, const pt::FrameArgs &a, hipEvent_t done)
{
    // A launch seen COMPLETE with the flag DOWN — read in that order: an abandoning launch raises the flag before it ends — ran to its
    // end and needs no repair pass.
    while (h->handover.unverified.size() > 2 && hipEventQuery(h->handover.unverified.front().done) == hipSuccess && !abandon_raised(h)) {
        FEED_LOG("remember: launch %u frames [%d,+%d) seen complete with the flag down: forgotten", h->handover.unverified.front().a.launchSeq, h->handover.unverified.front().a.frame, h->handover.unverified.front().a.batchFrames);
        h->handover.unverified.pop_front();
    }
    (void)hipGetLastError(); // (hipErrorNotReady of the query is not an error)
    static_assert(pt_renderer::kLaunchEvents / 2 <= pt::kMaxUnverifiedLaunches, "frame-tag window (pt_kernels.hpp)");
    if (h->handover.unverified.size() >= (size_t)pt_renderer::kLaunchEvents / 2) { // (the event ring must not lap a remembered launch; also the frame-tag window's bound)
        (void)hipEventSynchronize(h->handover.unverified.front().done);
        if (!abandon_raised(h)) h->handover.unverified.pop_front();
    }
    h->handover.unverified.push_back({a, done});
    FEED_LOG("launch %u frames [%d,+%d) chainTag %g keepTags %d variant %d spp %d (%zu remembered)", a.launchSeq, a.frame, a.batchFrames, (double)a.chainTag, a.keepTags, a.variant, a.spp, h->handover.unverified.size());
    if (pt::tuning().feedLog >= 2) { // (debug: a blocking look at the device's abandon word and ticket counters)
        unsigned int w = 0, q[2] = {0, 0};
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(&w, h->handover.dAbandon, 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(&q[0], queue_word(h, 0), 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(&q[1], queue_word(h, 1), 4, hipMemcpyDeviceToHost);
        FEED_LOG("  after launch %u: abandon word %08x, tickets main %u (host %u) chain %u (host %u), flag %u", a.launchSeq, w, q[0], queue_base(h, 0), q[1], queue_base(h, 1),
                 h->handover.hostErrWord ? *(volatile unsigned int *)h->handover.hostErrWord : 0u);
    }
}

} // namespace ptimpl
