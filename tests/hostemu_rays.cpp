// tests/hostemu_rays.cpp -- TEST INFRASTRUCTURE ONLY: tptLaunchTraceRays for the host runtime built against tests/hostemu
// (tests/test_rays_abi.py).  As tests/hostemu/hostemu_kernels.cpp restates the lane-refill kernel for pixels (traceLaneRefill), this
// restates its ray mode with the product's own lane headers -- laneBeginRay, hitSpheres, rayHitRecord, lanePost -- ray by ray in chunk
// order, and does with the argument block what the kernel does: where a ray's records go, which word the rays are counted into, how the
// work counters are found and re-armed.  It refuses a launch whose constants are not the ray mode's, and counts the launches, so a test
// can tell accepted calls from refused ones.
#include "tpt_device.h"
#include <stdio.h>
#include <stdlib.h>

using namespace tpt;

namespace {
int gLaunches = 0;
struct RayJob {
    KernelArgs a;
    int hs, fold;
    bool ldsScene;
};

template <int HS, int FOLD>
void traceRays(const KernelArgs& a)
{
    const SceneView& sv = a.scene;
    f4 stackMem[TPT_MAX_DEPTH];
    BounceStack stack;
    stack.base = stackMem;
    stack.stride = 1;
    stack.fastLevels = a.ldsStackLevels > TPT_MAX_DEPTH ? TPT_MAX_DEPTH : a.ldsStackLevels;
    stack.spill = stackMem + stack.fastLevels;
    stack.spillStride = 1;
    unsigned long long total = 0;
    for (int c = 0; c < a.numChunks; ++c) {
        const int first = c * a.chunkSize, last = first + a.chunkSize < a.numItems ? first + a.chunkSize : a.numItems;
        for (int i = first; i < last; ++i) {
            Lane L;
            L.rays = 0;
            L.active = false;
            laneBeginRay(L, a.rays[2 * (size_t)i], a.rays[2 * (size_t)i + 1], i);
            for (;;) {
                const bool firstOfRay = L.depth == 0 && L.kind == KIND_MAIN;
                float t;
                const int id = (HS != HS_SIMPLE && firstOfRay && !rayDirFitsFilter(L.dir))
                                   ? hitSpheres<HS_SIMPLE>(sv, L.orig, L.dir, TPT_MIN_T, TPT_MAX_T, t)
                                   : hitSpheres<HS>(sv, L.orig, L.dir, TPT_MIN_T, TPT_MAX_T, t);
                L.rays++;
                if (firstOfRay && a.rayHits) rayHitRecord(sv, L.orig, L.dir, id, t, a.rayHits[2 * (size_t)L.pix], a.rayHits[2 * (size_t)L.pix + 1]);
                if ((firstOfRay && !a.rayRadiance) || lanePost<FOLD>(L, id, t, sv, a.fc, stack)) break;
            }
            if (a.rayRadiance) {
                f4 v;
                v.x = L.col.x; v.y = L.col.y; v.z = L.col.z; v.w = (float)L.rays;
                a.rayRadiance[L.pix] = v;
            }
            total += L.rays;
        }
    }
    a.rayCounter[0] += total;
}

void runRays(void* p)
{
    const RayJob& J = *static_cast<const RayJob*>(p);
    const KernelArgs& a = J.a;
    // the kernel relies on the previous launch on this block having re-armed the counters (and nobody else touching them)
    if (a.work[0] != 0u || a.work[1] != 0u) {
        fprintf(stderr, "hostemu: a ray launch found its work counters at %u / %u: two launches share a counter block in flight\n", a.work[0], a.work[1]);
        abort();
    }
    a.work[0] = (unsigned)a.numChunks + 1u; // (what the counters look like while the launch runs)
    a.work[1] = 1u;
    const bool groups = !J.ldsScene;
    if (J.hs == HS_SIMPLE) {
        if (J.fold == FOLD_FORWARD) traceRays<HS_SIMPLE, FOLD_FORWARD>(a);
        else traceRays<HS_SIMPLE, FOLD_RECURSIVE>(a);
    } else if (groups) {
        if (J.fold == FOLD_FORWARD) traceRays<HS_TWO_PHASE_GROUPS, FOLD_FORWARD>(a);
        else traceRays<HS_TWO_PHASE_GROUPS, FOLD_RECURSIVE>(a);
    } else {
        if (J.fold == FOLD_FORWARD) traceRays<HS_TWO_PHASE, FOLD_FORWARD>(a);
        else traceRays<HS_TWO_PHASE, FOLD_RECURSIVE>(a);
    }
    a.work[0] = 0u; // the last wave re-arms the counters
    a.work[1] = 0u;
}
} // namespace

hipError_t tptLaunchTraceRays(const KernelArgs& a, int hs, int fold, bool ldsScene, int blocks, size_t lds, hipStream_t stream)
{
    const FrameConsts& fc = a.fc;
    const bool consts = fc.spp == 1 && fc.invSpp == 1.0f && fc.seedMode == SEED_PER_PIXEL && fc.width == 1 && a.batchFrames == 1 && a.laneCap == 64 &&
                        a.noRefill == 0 && !a.chunkOrder && !a.chunkCost && (a.chunkSize == 256 || a.chunkSize == 64) &&
                        a.numChunks == (a.numItems + a.chunkSize - 1) / a.chunkSize && a.numItems >= 1;
    if (!consts || !a.rays || (!a.rayRadiance && !a.rayHits) || !a.rayCounter || !a.work) return hipErrorInvalidValue;
    if (blocks < 1 || blocks > a.numChunks || (unsigned)blocks != a.totalWaves || lds > 160 * 1024) return hipErrorInvalidValue;
    if (fold == FOLD_RECURSIVE && a.ldsStackLevels < TPT_MAX_DEPTH && (!a.stackBuf || a.stackStride != blocks * TPT_BLOCK)) return hipErrorInvalidValue;
    ++gLaunches;
    RayJob J; J.a = a; J.hs = hs; J.fold = fold; J.ldsScene = ldsScene;
    hostemuEnqueue(stream, runRays, &J, sizeof(J));
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuRayLaunches() { return gLaunches; }
