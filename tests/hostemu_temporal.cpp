// tests/hostemu_temporal.cpp -- TEST INFRASTRUCTURE ONLY: tptTemporalAccumulateDevice's launcher for the host runtime built against
// tests/hostemu (tests/test_temporal_abi.py).  It runs nothing; it counts the calls that reach it, so a test can tell accepted calls
// from refused ones, and keeps the constants of the last one so that the test can see what the host made of the cameras.
#include "tpt_device.h"

static int gLaunches = 0;
static tptTemporalConsts gLast;
hipError_t tptLaunchTemporal(const float*, const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                             float*, float*, float*, float*, int, int, const tptTemporalConsts& k, hipStream_t)
{
    ++gLaunches;
    gLast = k;
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuTemporalLaunches() { return gLaunches; }
extern "C" __attribute__((visibility("default"))) const float* hostemuTemporalConsts() { return gLast.o; }
