// tests/hostemu_batch_moments_flow.cpp -- TEST INFRASTRUCTURE ONLY: launchers for the host runtime built against tests/hostemu that RUN
// something, as work of the stream they are given, so that tests/test_batch_moments_abi.py can follow tptDrawDeviceBatchMoments' data flow
// -- which staging plane every launch writes and every fold reads, the alternating halves, the staging that grows between calls, the lerp
// table, the ray counts -- without a GPU.  The path-queue trace launcher of tests/hostemu/hostemu_kernels.cpp is taken over with the
// linker's --wrap (the test passes the option): its stand-in writes planes that depend on the frame number, the pixel, the plane and the
// channel (standIn below; the test restates it in numpy), and counts standInRays(frame) rays where the kernel would.  The fold stand-in is
// the statement of include/tpt_hip.h in plain C++.  HOSTEMU_FOLD_MUTANT=slot makes it read staged frame j + 1 for frame j where the launch
// has one, =lerp makes it take the lerp table one entry late: what the test's mutation check must see.
#include "tpt_device.h"
#include <stdlib.h>
#include <string.h>

static float standIn(long long frame, long long pixel, int plane, int channel)
{
    return (float)((frame * 131 + pixel * 7 + plane * 17 + channel * 3) % 1009) / 64.0f + 0.5f;
}
static unsigned long long standInRays(long long frame) { return 1000ull + 37ull * (unsigned long long)frame; }

static void runTraceStandIn(void* p)
{
    const tpt::KernelArgs& a = *static_cast<const tpt::KernelArgs*>(p);
    const long long nPixels = (long long)a.nLocalRows * a.fc.width;
    for (int j = 0; j < a.batchFrames; ++j) {
        const long long frame = a.fc.frame + j;
        tpt::f4* const planes[4] = {a.frameColour + (size_t)j * a.framePlane, a.momentsOut + (size_t)j * a.framePlane,
                                    a.aovAlbedo ? a.aovAlbedo + (size_t)j * a.aovPlane : nullptr,
                                    a.aovNormalDepth ? a.aovNormalDepth + (size_t)j * a.aovPlane : nullptr};
        for (int k = 0; k < 4; ++k)
            for (long long i = 0; planes[k] && i < nPixels; ++i)
                planes[k][i] = tpt::f4{standIn(frame, i, k, 0), standIn(frame, i, k, 1), standIn(frame, i, k, 2), standIn(frame, i, k, 3)};
        a.rayCounter[(size_t)j * a.rayCounterStride] += standInRays(frame);
    }
}
hipError_t wrapTraceQueue(const tpt::KernelArgs& a, bool, int, size_t, hipStream_t) __asm__("__wrap__Z19tptLaunchTraceQueueRKN3tpt10KernelArgsEbimP12ihipStream_t");
hipError_t wrapTraceQueue(const tpt::KernelArgs& a, bool, int, size_t, hipStream_t stream)
{
    if (!a.momentsOut || !a.frameColour || a.batchFrames < 1 || a.batchFrames > 32) return hipErrorInvalidValue; // (this file serves the moments draws only)
    hostemuEnqueue(stream, runTraceStandIn, &a, sizeof a);
    return hipSuccess;
}

struct FoldWork {
    tpt::f4 *dst[4];
    const tpt::f4* src[4];
    int nPixels, nFrames;
    tptLerpTable lerp;
    const unsigned long long* frameRays;
    unsigned long long* totalRays;
};
static void runFold(void* p)
{
    const FoldWork& f = *static_cast<const FoldWork*>(p);
    const char* mutant = getenv("HOSTEMU_FOLD_MUTANT");
    const bool wrongSlot = mutant && !strcmp(mutant, "slot"), wrongLerp = mutant && !strcmp(mutant, "lerp");
    for (int j = 0; f.frameRays && j < f.nFrames; ++j) *f.totalRays += f.frameRays[j];
    for (int k = 0; k < 4; ++k) {
        if (!f.dst[k]) continue;
        for (int i = 0; i < f.nPixels; ++i) {
            tpt::f4 r = f.dst[k][i];
            for (int j = 0; j < f.nFrames; ++j) {
                const int slot = wrongSlot && j + 1 < f.nFrames ? j + 1 : j;
                const tpt::f4 c = f.src[k][(size_t)slot * (size_t)f.nPixels + (size_t)i];
                const float lerp = f.lerp.v[wrongLerp && j > 0 ? j - 1 : j], one = 1 - lerp;
                r.x = r.x * lerp + c.x * one;
                r.y = r.y * lerp + c.y * one;
                r.z = r.z * lerp + c.z * one;
                if (k >= 2) r.w = r.w * lerp + c.w * one; // (the tile's alpha and the moments' .w are nobody's to write)
            }
            f.dst[k][i] = r;
        }
    }
}
hipError_t tptLaunchFoldBatch(float* tile, float* moments, float* albedo, float* normalDepth, const tpt::f4* stagedColour, const tpt::f4* stagedMoments,
                              const tpt::f4* stagedAlbedo, const tpt::f4* stagedNormalDepth, int nPixels, int nFrames, const tptLerpTable& lerp,
                              const unsigned long long* frameRays, unsigned long long* totalRays, hipStream_t stream)
{
    const FoldWork f = {{reinterpret_cast<tpt::f4*>(tile), reinterpret_cast<tpt::f4*>(moments), reinterpret_cast<tpt::f4*>(albedo),
                         reinterpret_cast<tpt::f4*>(normalDepth)},
                        {stagedColour, stagedMoments, stagedAlbedo, stagedNormalDepth}, nPixels, nFrames, lerp, frameRays, totalRays};
    hostemuEnqueue(stream, runFold, &f, sizeof f);
    return hipSuccess;
}
