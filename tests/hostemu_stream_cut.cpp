// tests/hostemu_stream_cut.cpp -- TEST INFRASTRUCTURE ONLY: what the host runtime built against tests/hostemu knows about the cut of a
// closed stream batch (csrc/tpt_frame_pools.h), for tests/test_stream_cut_host.py: the STREAM entry at the front of the launch queue
// and the cut words in (emulated) pinned host memory.  It changes nothing.
#include "tpt_context.h"

using namespace tpth;

// the open STREAM entry: 1 and {slot, serial of its launch (0: no pool per frame), frames served, frames traced}, or 0 when none is pending
extern "C" __attribute__((visibility("default"))) int hostemuStreamFront(int* out4)
{
    if (!g.pending.holds(PendingLaunch::STREAM)) return 0;
    const PendingLaunch& F = g.pending.e[0];
    out4[0] = F.T.slot; out4[1] = (int)F.T.cutSerial; out4[2] = F.next; out4[3] = F.T.batch;
    return 1;
}
extern "C" __attribute__((visibility("default"))) unsigned hostemuCutWord(int slot)
{
    return g.hCut && slot >= 0 && slot < Context::kMaxSlots ? g.hCut[slot] : 0xffffffffu;
}
extern "C" __attribute__((visibility("default"))) unsigned hostemuNewestCutSerial() { return g.cutSerial; }
