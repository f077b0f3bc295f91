// tests/hostemu_clip_chain.cpp -- TEST INFRASTRUCTURE ONLY: launchers for the host runtime built against tests/hostemu that RUN something,
// as work of the stream they are given, so that tests/test_clip_denoise_abi.py can follow tptDenoiseClipDevice's data flow -- which
// plane of the staging every launch reads and writes, the copies at a chunk seam, deviceHistory -- without a GPU.  They are not the
// filters: each output is an exact elementwise sum of the launch's inputs (the test restates them in numpy), chosen so that a frame
// that read a stale or clobbered predecessor, or a stack at the wrong offset, changes the result.
//   temporal pass:  outColour = colour + prevColour;  outAlbedo = albedo + prevAlbedo;  outMoments = moments + prevMoments + prevNormalDepth;
//                   outVariance = colour + moments            (the prev terms absent on a first frame)
//   a-trous:        out_j = colour_j + albedo_j + normalDepth_j + moments_j for every frame j of the stack; with more than one
//                   iteration the scratch planes of those frames are overwritten with 123 first, as the ping-pong would
#include "tpt_device.h"

struct TemporalWork {
    const float *c, *a, *m, *pc, *pa, *pnd, *pm;
    float *oc, *oa, *om, *ov;
    size_t n;
};
static void runTemporal(void* p)
{
    const TemporalWork& t = *static_cast<const TemporalWork*>(p);
    for (size_t i = 0; i < t.n; ++i) {
        const float c = t.c[i], m = t.m[i];
        t.oc[i] = t.pc ? c + t.pc[i] : c;
        t.oa[i] = t.pa ? t.a[i] + t.pa[i] : t.a[i];
        t.om[i] = t.pm ? (m + t.pm[i]) + t.pnd[i] : m;
        t.ov[i] = c + m;
    }
}
hipError_t tptLaunchTemporal(const float* colour, const float* albedo, const float*, const float* moments, const float* prevColour,
                             const float* prevAlbedo, const float* prevNormalDepth, const float* prevMoments, float* outColour,
                             float* outAlbedo, float* outMoments, float* outVariance, int width, int height, const tptTemporalConsts&,
                             hipStream_t stream)
{
    const TemporalWork t = {colour, albedo, moments, prevColour, prevAlbedo, prevNormalDepth, prevMoments, outColour, outAlbedo, outMoments,
                            outVariance, (size_t)width * (size_t)height * 4u};
    hostemuEnqueue(stream, runTemporal, &t, sizeof t);
    return hipSuccess;
}

struct AtrousWork {
    const float *c, *a, *nd, *m;
    float *out, *scratch;
    size_t n;
    int iterations;
};
static void runAtrous(void* p)
{
    const AtrousWork& t = *static_cast<const AtrousWork*>(p);
    for (size_t i = 0; t.iterations > 1 && i < t.n; ++i) t.scratch[i] = 123.0f;
    for (size_t i = 0; i < t.n; ++i) t.out[i] = ((t.c[i] + t.a[i]) + t.nd[i]) + t.m[i];
}
hipError_t tptLaunchFramesAtrous(const float* colour, const float* albedo, const float* normalDepth, const float* moments, float* out,
                                 float* scratch, int width, int height, int frames, int iterations, float, float, float, float, bool,
                                 hipStream_t stream)
{
    const AtrousWork t = {colour, albedo, normalDepth, moments, out, scratch, (size_t)width * (size_t)height * 4u * (size_t)frames, iterations};
    hostemuEnqueue(stream, runAtrous, &t, sizeof t);
    return hipSuccess;
}
