// tests/hostemu_clip_denoise.cpp -- TEST INFRASTRUCTURE ONLY: tptDenoiseClipDevice's a-trous launcher for the host runtime built against
// tests/hostemu (tests/test_clip_denoise_abi.py, beside hostemu_temporal.cpp and hostemu_objects.cpp, which count the temporal
// launches).  It runs nothing; it counts the calls that reach it and keeps of the last 64 what the host handed over -- the frames and
// iterations of the launch, the size, and the six plane pointers -- so that a test can read the launch plan of an accepted call.
#include "tpt_device.h"

struct FramesAtrousLaunch {
    int frames, iterations, width, height;
    const void* colour;
    const void* albedo;
    const void* normalDepth;
    const void* moments;
    const void* out;
    const void* scratch;
};
static int gLaunches = 0;
static FramesAtrousLaunch gLaunch[64];
hipError_t tptLaunchFramesAtrous(const float* colour, const float* albedo, const float* normalDepth, const float* moments, float* out,
                                 float* scratch, int width, int height, int frames, int iterations, float, float, float, float, bool,
                                 hipStream_t)
{
    gLaunch[gLaunches % 64] = {frames, iterations, width, height, colour, albedo, normalDepth, moments, out, scratch};
    ++gLaunches;
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuFramesAtrousLaunches() { return gLaunches; }
extern "C" __attribute__((visibility("default"))) const FramesAtrousLaunch* hostemuFramesAtrousLaunch(int launch) { return &gLaunch[launch % 64]; }
