// tests/hostemu_flow.cpp -- TEST INFRASTRUCTURE ONLY: tptMotionVectorsDevice's launcher for the host runtime built against tests/hostemu
// (tests/test_flow_abi.py, beside hostemu_temporal.cpp, whose constants the test compares with).  It computes nothing.  It counts the
// calls that reach it and keeps of the last 64 what the host handed over -- the frames of the launch, the size, the plane pointers and
// the table's address -- so that a test can read the launch plan of an accepted call.  And it enqueues one unit of work on the stream
// it is given, which reads the launch's records out of the constants table WHEN IT RUNS, as the kernel would: under the lazy schedule
// that is after every later call was enqueued, so a call that rewrites what an earlier call's copy still has to read shows.
#include <string.h>

#include "tpt_device.h"

struct FlowLaunch {
    int frames, width, height, nObjects;
    const void* albedo;
    const void* normalDepth;
    const void* object;
    const void* prevAlbedo;
    const void* prevNormalDepth;
    const void* prevObject;
    const void* motion;
    const void* out;
    const void* consts;
    int ran; // 1 once the launch's unit of work has run
};
static const int kKept = 64, kFrames = 64;
static int gLaunches = 0;
static FlowLaunch gLaunch[kKept];
static tptFlowConsts gSeen[kKept][kFrames]; // the first 64 records of each launch, as its work found them

struct FlowWork {
    int slot, frames;
    const tptFlowConsts* consts;
};
static void runFlow(void* p)
{
    const FlowWork& t = *static_cast<const FlowWork*>(p);
    memcpy(gSeen[t.slot], t.consts, sizeof(tptFlowConsts) * (size_t)(t.frames < kFrames ? t.frames : kFrames));
    gLaunch[t.slot].ran = 1;
}
hipError_t tptLaunchFlow(const float* albedo, const float* normalDepth, const int32_t* object, const float* prevAlbedo,
                         const float* prevNormalDepth, const int32_t* prevObject, const float* motion, int nObjects, float* out, int width,
                         int height, int frames, const tptFlowConsts* deviceConsts, hipStream_t stream)
{
    const int slot = gLaunches % kKept;
    gLaunch[slot] = {frames, width, height, nObjects, albedo, normalDepth, object, prevAlbedo, prevNormalDepth, prevObject, motion, out,
                     deviceConsts, 0};
    ++gLaunches;
    const FlowWork t = {slot, frames, deviceConsts};
    hostemuEnqueue(stream, runFlow, &t, sizeof t);
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuFlowLaunches() { return gLaunches; }
extern "C" __attribute__((visibility("default"))) const FlowLaunch* hostemuFlowLaunch(int launch) { return &gLaunch[launch % kKept]; }
extern "C" __attribute__((visibility("default"))) const float* hostemuFlowConstsSeen(int launch, int frame) { return gSeen[launch % kKept][frame].o; }
extern "C" __attribute__((visibility("default"))) int hostemuFlowConstsFloats() { return (int)(sizeof(tptFlowConsts) / sizeof(float)); }
