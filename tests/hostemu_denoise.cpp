// tests/hostemu_denoise.cpp -- TEST INFRASTRUCTURE ONLY: tptDenoiseDevice's launcher for the host runtime built against tests/hostemu
// (tests/test_denoise_abi.py).  It runs nothing; it counts the calls that reach it, so a test can tell accepted calls from refused ones.
static int gLaunches = 0;
hipError_t tptLaunchDenoise(const float*, const float*, const float*, float*, float*, int, int, int, float, float, float, bool, hipStream_t)
{
    ++gLaunches;
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuDenoiseLaunches() { return gLaunches; }
