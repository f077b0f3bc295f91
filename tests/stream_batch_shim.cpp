// TEST INFRASTRUCTURE: csrc/tpt_stream_batch.h -- the pipeline depth for a number of hardware queues and the frames per STREAM launch --
// compiled for the host and exported to tests/test_stream_batch_rule.py.  The two constants are Context's (csrc/tpt_context.h).
#include "tpt_stream_batch.h"

static const int kMaxOverlap = 16;    // Context::kMaxOverlap
static const int kStreamBatchMax = 8; // Context::kStreamBatchMax

extern "C" int sb_overlap_cap(int hwQueues) { return tpt::queueOverlapCap(hwQueues, kMaxOverlap); }
extern "C" int sb_max_overlap() { return kMaxOverlap; }
extern "C" int sb_batch_max() { return kStreamBatchMax; }
extern "C" int sb_frames(long long samples, int depth, int run, long long frameColour)
{
    return tpt::streamBatchFrames(samples, depth, kMaxOverlap, run, frameColour, kStreamBatchMax);
}
