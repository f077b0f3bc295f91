// tests/hostemu_spatial_variance.cpp -- TEST INFRASTRUCTURE ONLY: tptSpatialVarianceDevice's launcher for the host runtime built against
// tests/hostemu (tests/test_spatial_variance_abi.py).  It runs nothing; it counts the calls that reach it, so a test can tell accepted
// calls from refused ones, and keeps what the last one was handed -- the grid it would launch included -- so that the test can see
// that the host passed its arguments on unchanged and formed the guides' constants as it states.
#include "tpt_device.h"

struct SpreadLaunch {
    const void* planes[3]; // moments, normalDepth, out
    int width, height, frames, radius;
    float samplesPerFrame, minSamples, in, id;
    unsigned grid[3];
    const void* stream;
};
static int gLaunches = 0;
static SpreadLaunch gLast;
hipError_t tptLaunchSpread(const float* moments, const float* normalDepth, float* out, int width, int height, int frames,
                           float samplesPerFrame, float minSamples, int radius, float in, float id, hipStream_t stream)
{
    ++gLaunches;
    gLast = {{moments, normalDepth, out}, width, height, frames, radius, samplesPerFrame, minSamples, in, id,
             {(unsigned)(width + TPT_RECTIFY_TILE_W - 1) / TPT_RECTIFY_TILE_W, (unsigned)(height + TPT_RECTIFY_TILE_H - 1) / TPT_RECTIFY_TILE_H,
              (unsigned)frames},
             (const void*)stream};
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuSpreadLaunches() { return gLaunches; }
extern "C" __attribute__((visibility("default"))) const SpreadLaunch* hostemuSpreadLast() { return &gLast; }
