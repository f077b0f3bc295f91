// tests/hostemu_variance.cpp -- TEST INFRASTRUCTURE ONLY: tptDenoiseDeviceVariance's launcher for the host runtime built against
// tests/hostemu (tests/test_moments_abi.py).  It runs nothing; it counts the calls that reach it, so a test can tell accepted calls from
// refused ones.
static int gLaunches = 0;
hipError_t tptLaunchDenoiseVariance(const float*, const float*, const float*, const float*, float*, float*, int, int, int, float, float,
                                    float, float, bool, hipStream_t)
{
    ++gLaunches;
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuVarianceLaunches() { return gLaunches; }
