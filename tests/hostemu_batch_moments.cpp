// tests/hostemu_batch_moments.cpp -- TEST INFRASTRUCTURE ONLY: counting launchers for the host runtime built against tests/hostemu
// (tests/test_batch_moments_abi.py).  They run nothing.  tptLaunchFoldBatch is defined here and records what it was handed; the trace and
// blend launchers, which tests/hostemu/hostemu_kernels.cpp defines, are taken over with the linker's --wrap (the test passes the option
// per symbol): the host runtime's calls arrive at the __wrap_ functions below, which record the launch and return, so a test can tell
// how many launches of each kind a call made and with which pointers -- and that a refused call made none.
#include "tpt_device.h"
#include <vector>

namespace {
struct TraceRec {
    long long frames, firstFrame, colour, moments, albedo, normalDepth, aovPlane, framePlane, cams, centres, rayCounter, rayStride, queue;
};
struct FoldRec {
    long long tile, moments, albedo, normalDepth, sColour, sMoments, sAlbedo, sNormalDepth, nPixels, nFrames, frameRays, totalRays;
    float lerp[32];
};
std::vector<TraceRec> gTraces;
std::vector<FoldRec> gFolds;
long long gResolves = 0;
long long addr(const void* p) { return (long long)reinterpret_cast<uintptr_t>(p); }
void recordTrace(const tpt::KernelArgs& a, bool queue)
{
    gTraces.push_back(TraceRec{a.batchFrames, a.fc.frame, addr(a.frameColour), addr(a.momentsOut), addr(a.aovAlbedo), addr(a.aovNormalDepth),
                               a.aovPlane, a.framePlane, addr(a.viewCams), addr(a.moveCentres), addr(a.rayCounter), a.rayCounterStride, queue ? 1 : 0});
}
} // namespace

hipError_t wrapTraceQueue(const tpt::KernelArgs& a, bool, int, size_t, hipStream_t) __asm__("__wrap__Z19tptLaunchTraceQueueRKN3tpt10KernelArgsEbimP12ihipStream_t");
hipError_t wrapTraceQueue(const tpt::KernelArgs& a, bool, int, size_t, hipStream_t)
{
    recordTrace(a, true);
    return hipSuccess;
}
hipError_t wrapTrace(const tpt::KernelArgs& a, int, int, bool, int, size_t, hipStream_t) __asm__("__wrap__Z14tptLaunchTraceRKN3tpt10KernelArgsEiibimP12ihipStream_t");
hipError_t wrapTrace(const tpt::KernelArgs& a, int, int, bool, int, size_t, hipStream_t)
{
    recordTrace(a, false);
    return hipSuccess;
}
hipError_t wrapResolve(float*, const tpt::f4*, int, float, float*, unsigned long long*, unsigned long long*, const unsigned long long*, hipStream_t)
    __asm__("__wrap__Z16tptLaunchResolvePfPKN3tpt2f4EifS_PyS4_PKyP12ihipStream_t");
hipError_t wrapResolve(float*, const tpt::f4*, int, float, float*, unsigned long long*, unsigned long long*, const unsigned long long*, hipStream_t)
{
    ++gResolves;
    return hipSuccess;
}
hipError_t wrapResolveBatch(float*, const tpt::f4*, int, int, int, const tptLerpTable&, float*, unsigned long long*, unsigned long long*, hipStream_t)
    __asm__("__wrap__Z21tptLaunchResolveBatchPfPKN3tpt2f4EiiiRK12tptLerpTableS_PyS7_P12ihipStream_t");
hipError_t wrapResolveBatch(float*, const tpt::f4*, int, int, int, const tptLerpTable&, float*, unsigned long long*, unsigned long long*, hipStream_t)
{
    ++gResolves;
    return hipSuccess;
}

hipError_t tptLaunchFoldBatch(float* tile, float* moments, float* albedo, float* normalDepth, const tpt::f4* stagedColour, const tpt::f4* stagedMoments,
                              const tpt::f4* stagedAlbedo, const tpt::f4* stagedNormalDepth, int nPixels, int nFrames, const tptLerpTable& lerp,
                              const unsigned long long* frameRays, unsigned long long* totalRays, hipStream_t)
{
    FoldRec r = {addr(tile), addr(moments), addr(albedo), addr(normalDepth), addr(stagedColour), addr(stagedMoments), addr(stagedAlbedo),
                 addr(stagedNormalDepth), nPixels, nFrames, addr(frameRays), addr(totalRays), {}};
    for (int j = 0; j < 32; ++j) r.lerp[j] = lerp.v[j];
    gFolds.push_back(r);
    return hipSuccess;
}

#define EXPORT extern "C" __attribute__((visibility("default")))
EXPORT void hostemuBmCounts(long long* out3)
{
    out3[0] = (long long)gTraces.size();
    out3[1] = (long long)gFolds.size();
    out3[2] = gResolves;
}
EXPORT void hostemuBmReset()
{
    gTraces.clear();
    gFolds.clear();
    gResolves = 0;
}
EXPORT void hostemuBmTrace(int i, long long* out13) // frames, firstFrame, colour, moments, albedo, normalDepth, aovPlane, framePlane, cams, centres, rayCounter, rayStride, queue
{
    const TraceRec& t = gTraces[(size_t)i];
    const long long v[13] = {t.frames, t.firstFrame, t.colour, t.moments, t.albedo, t.normalDepth, t.aovPlane, t.framePlane, t.cams, t.centres,
                             t.rayCounter, t.rayStride, t.queue};
    for (int k = 0; k < 13; ++k) out13[k] = v[k];
}
EXPORT void hostemuBmFold(int i, long long* out12, float* lerp32) // the launcher's arguments in its order
{
    const FoldRec& f = gFolds[(size_t)i];
    const long long v[12] = {f.tile, f.moments, f.albedo, f.normalDepth, f.sColour, f.sMoments, f.sAlbedo, f.sNormalDepth, f.nPixels, f.nFrames,
                             f.frameRays, f.totalRays};
    for (int k = 0; k < 12; ++k) out12[k] = v[k];
    for (int j = 0; j < 32; ++j) lerp32[j] = f.lerp[j];
}
EXPORT int hostemuBmFramesPerLaunch(int w, int h, int planes) { return tptFoldFramesPerLaunch((size_t)w * (size_t)h * 16u, planes); }
EXPORT int hostemuBmFoldBlocksPerPlane() { return TPT_FOLD_BLOCKS_PER_PLANE; }
