// tests/hostemu_adaptive.cpp -- TEST INFRASTRUCTURE ONLY: the launchers of tptDrawDeviceAdaptive's blend and of tptAdaptiveSamplesDevice
// for the host runtime built against tests/hostemu (tests/test_adaptive_abi.py).  They run nothing; they count the calls that reach them,
// so a test can tell accepted calls from refused ones.
#include "tpt_device.h"

static int gResolves = 0, gPlans = 0;
hipError_t tptLaunchAdaptiveResolve(float*, float*, const tpt::f4*, const tpt::f4*, const int32_t*, int, bool, hipStream_t)
{
    ++gResolves;
    return hipSuccess;
}
hipError_t tptLaunchAdaptivePlan(const float*, int32_t*, float*, int64_t*, int, int, float, int, int, hipStream_t)
{
    ++gPlans;
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuAdaptiveResolves() { return gResolves; }
extern "C" __attribute__((visibility("default"))) int hostemuAdaptivePlans() { return gPlans; }
