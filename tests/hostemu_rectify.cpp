// tests/hostemu_rectify.cpp -- TEST INFRASTRUCTURE ONLY: tptRectifyHistoryDevice's launcher for the host runtime built against
// tests/hostemu (tests/test_rectify_abi.py).  It runs nothing; it counts the calls that reach it, so a test can tell accepted calls from
// refused ones, and keeps what the last one was handed so that the test can see that the host passed its arguments on unchanged.
#include "tpt_device.h"

struct RectifyLaunch {
    const void* planes[7]; // colour, moments, accColour, accMoments, outColour, outMoments, outVariance
    int width, height, radius;
    float gamma;
    const void* stream;
};
static int gLaunches = 0;
static RectifyLaunch gLast;
hipError_t tptLaunchRectify(const float* colour, const float* moments, const float* accColour, const float* accMoments, float* outColour,
                            float* outMoments, float* outVariance, int width, int height, int radius, float gamma, hipStream_t stream)
{
    ++gLaunches;
    gLast = {{colour, moments, accColour, accMoments, outColour, outMoments, outVariance}, width, height, radius, gamma, (const void*)stream};
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuRectifyLaunches() { return gLaunches; }
extern "C" __attribute__((visibility("default"))) const RectifyLaunch* hostemuRectifyLast() { return &gLast; }
