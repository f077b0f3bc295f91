// tests/hostemu_objects.cpp -- TEST INFRASTRUCTURE ONLY: the launchers of tptObjectPlaneDevice and tptTemporalAccumulateObjectsDevice for
// the host runtime built against tests/hostemu (tests/test_objects_abi.py).  They run nothing; they count the calls that reach them, so a
// test can tell accepted calls from refused ones, and keep what the host handed over: of the object plane the last 8 launches'
// constants (18 floats each: camera o, ll, H, V, then the centres of spheres 1 and 8), sphere counts and output planes, of the
// accumulation pass the last launch's constants and table size.
#include "tpt_device.h"

static int gPlanes = 0, gPasses = 0, gLastObjects = -1, gCounts[8];
static tptObjectPlaneConsts gPlaneConsts[8];
static const void* gPlaneOut[8];
static tptReprojectConsts gLast;
hipError_t tptLaunchObjectPlane(const tpt::f4*, int nSpheres, int32_t* out, int, int, const tptObjectPlaneConsts& k, hipStream_t)
{
    gPlaneConsts[gPlanes % 8] = k;
    gCounts[gPlanes % 8] = nSpheres;
    gPlaneOut[gPlanes % 8] = out;
    ++gPlanes;
    return hipSuccess;
}
hipError_t tptLaunchReprojectObjects(const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                                     const float*, float*, float*, float*, float*, const int32_t*, const int32_t*, const float*, int nObjects,
                                     int, int, const tptReprojectConsts& k, hipStream_t)
{
    ++gPasses;
    gLast = k;
    gLastObjects = nObjects;
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuObjectPlaneLaunches() { return gPlanes; }
extern "C" __attribute__((visibility("default"))) const float* hostemuObjectPlaneConsts(int launch) { return gPlaneConsts[launch % 8].o; }
extern "C" __attribute__((visibility("default"))) int hostemuObjectPlaneSpheres(int launch) { return gCounts[launch % 8]; }
extern "C" __attribute__((visibility("default"))) const void* hostemuObjectPlaneOut(int launch) { return gPlaneOut[launch % 8]; }
extern "C" __attribute__((visibility("default"))) int hostemuObjectPassLaunches() { return gPasses; }
extern "C" __attribute__((visibility("default"))) const float* hostemuObjectPassConsts() { return gLast.t.o; }
extern "C" __attribute__((visibility("default"))) int hostemuObjectPassObjects() { return gLastObjects; }
