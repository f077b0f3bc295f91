// tpt_stream_batch.h -- how deep the frame pipeline may be for a number of hardware queues, and how many frames one STREAM launch
// traces for a streaming caller (tptDrawDevice, tptSetStreamBatching), in one place.
//
// A launch cannot be shorter than its slowest pixel's sequential samples.  With 16 launches in flight the others hide each one's tail;
// with two (a host with 4 hardware queues) almost nothing does, and one whole-machine launch per 1280x720x4 frame ran at 0.45 ms per
// frame against 0.28 in the deep pipeline.  So the frames per launch follow from the pipeline depth: the launches in flight
// together carry about what the deep pipeline's did.
// Plain integer functions shared by the host runtime (tpt_host.cpp, tpt_host_pipeline.cpp) and the CPU test of the rule
// (tests/stream_batch_shim.cpp -> tests/test_stream_batch_rule.py).
#pragma once

namespace tpt {

// Trace launches the runtime really runs side by side with `hwQueues` hardware queues (probed or TPT_HW_QUEUES): the ordered resolve
// chain, the scene uploads and the caller's own streams need queues too, so with fewer than ~3 queues per 2 trace streams to spare,
// two frames in flight is the best there is.
inline int queueOverlapCap(int hwQueues, int maxOverlap)
{
    return hwQueues >= maxOverlap ? maxOverlap : (hwQueues >= 8 ? hwQueues - 3 : 2);
}

// Samples per frame from which one frame per launch amortises the launch's fixed cost in a pipeline maxOverlap deep
// (profiles/r03/r03_run19.log: 1 at 1280x720x4, 3.7 M samples; 2 / 4 / 8 for halves / quarters / eighths of the threshold).
const long long kStreamLaunchSamples = 2400000;
// All colour planes of the STREAM launches in flight stay under this many bytes (the slots hold one launch's planes each).
const long long kStreamColourBudget = 1ll << 30;

// Frames per STREAM launch.
//   samples      camera samples of one frame on this rank (rows x width x spp)
//   depth        trace launches in flight (effectiveOverlap); 1: no pipeline, no batches
//   maxOverlap   the deepest pipeline (Context::kMaxOverlap)
//   run          STREAM launches made back to back before this one since the stream (re)started: 0 for the first
//   frameColour  bytes of one frame's colour plane
//   maxBatch     Context::kStreamBatchMax
// Frames under kStreamLaunchSamples get 2 / 4 / maxBatch at every depth.  Larger frames get enough frames per launch that `depth`
// launches carry maxOverlap x kStreamLaunchSamples samples -- 1 at depth 16, 8 for 1280x720x4 at depth 2 -- but a stream starts at
// 2 and doubles per launch up to that: the last launch of a stream traces frames nobody asks for (dropped at the caller's next
// synchronise), and a short stream wastes less that way.
inline int streamBatchFrames(long long samples, int depth, int maxOverlap, int run, long long frameColour, int maxBatch)
{
    if (depth <= 1 || samples <= 0) return 1;
    if (samples < kStreamLaunchSamples)
        return samples >= kStreamLaunchSamples / 2 ? 2 : samples >= kStreamLaunchSamples / 4 ? 4 : maxBatch;
    const long long want = (long long)maxOverlap * kStreamLaunchSamples / depth;
    int k = 1;
    while (k < maxBatch && (long long)k * samples < want) k *= 2;
    const int grown = 2 << (run < 8 ? (run < 0 ? 0 : run) : 8);
    if (k > grown) k = grown;
    while (k > 1 && (long long)k * depth * frameColour > kStreamColourBudget) k /= 2;
    return k;
}

} // namespace tpt
