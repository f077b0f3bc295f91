// tests/hostemu_lens.cpp -- TEST INFRASTRUCTURE ONLY: tptLaunchTraceLens for the host runtime built against tests/hostemu
// (tests/test_lens_abi.py).  As tests/hostemu/hostemu_kernels.cpp restates the lane-refill kernel for the camera's pixels
// (traceLaneRefill), this restates its lens mode with the product's own lane headers -- mapItem, laneBeginPixel, laneLens, hitSpheres,
// lanePost, lanePixelColour -- pixel by pixel in chunk order, and does with the argument block what the kernel does: which pixel an item
// is, where its colour goes, which word the rays are counted into, how the work counters are found and re-armed.  It refuses a launch
// whose constants are not the lens mode's, and counts the launches, so a test can tell accepted calls from refused ones.  It keeps the
// plan of the last launch it accepted (hostemuLensPlan: the work items, the chunks and the grid as KernelArgs and the launch hold them),
// and on request (hostemuLensPlanOnly) records the plan and answers hipErrorNotReady without running anything, so that a test can
// read the plan of an image it has no time to draw.
#include "tpt_device.h"
#include "tpt_queue_layout.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace tpt;

namespace {
int gLaunches = 0;
bool gPlanOnly = false;
long long gPlan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
struct LensJob {
    KernelArgs a;
    int hs, fold;
    bool ldsScene;
};

template <int HS, int FOLD>
void traceLens(const KernelArgs& a)
{
    const FrameConsts& fc = a.fc;
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
        for (int item = first; item < last; ++item) {
            int x, ly;
            if (!mapItem(a, item, x, ly)) continue;
            Lane L;
            L.rays = 0;
            L.active = false;
            laneBeginPixel(L, fc, x, localRowToGlobal(a, ly), ly * fc.width + x, true);
            for (;;) { // the kernel's step: a sample starts at the lens, HitWorld, everything behind it
                if (L.needCamera) laneLens<FOLD>(L, fc, &a.lens);
                float t;
                const int id = hitSpheres<HS>(sv, L.orig, L.dir, TPT_MIN_T, TPT_MAX_T, t);
                L.rays++;
                if (lanePost<FOLD>(L, id, t, sv, fc, stack)) break;
            }
            const f3 col = lanePixelColour(L, fc);
            f4 v; v.x = col.x; v.y = col.y; v.z = col.z; v.w = 0.0f;
            a.frameColour[L.pix] = v;
            total += L.rays;
        }
    }
    a.rayCounter[0] += total;
}

void runLens(void* p)
{
    const LensJob& J = *static_cast<const LensJob*>(p);
    const KernelArgs& a = J.a;
    // the kernel relies on the previous launch on this block having re-armed the counters (and nobody else touching them)
    if (a.work[0] != 0u || a.work[1] != 0u) {
        fprintf(stderr, "hostemu: a lens launch found its work counters at %u / %u: two launches share a counter block in flight\n", a.work[0], a.work[1]);
        abort();
    }
    a.work[0] = (unsigned)a.numChunks + 1u; // (what the counters look like while the launch runs)
    a.work[1] = 1u;
    const bool groups = !J.ldsScene;
    if (J.hs == HS_SIMPLE) {
        if (J.fold == FOLD_FORWARD) traceLens<HS_SIMPLE, FOLD_FORWARD>(a);
        else traceLens<HS_SIMPLE, FOLD_RECURSIVE>(a);
    } else if (groups) {
        if (J.fold == FOLD_FORWARD) traceLens<HS_TWO_PHASE_GROUPS, FOLD_FORWARD>(a);
        else traceLens<HS_TWO_PHASE_GROUPS, FOLD_RECURSIVE>(a);
    } else {
        if (J.fold == FOLD_FORWARD) traceLens<HS_TWO_PHASE, FOLD_FORWARD>(a);
        else traceLens<HS_TWO_PHASE, FOLD_RECURSIVE>(a);
    }
    a.work[0] = 0u; // the last wave re-arms the counters
    a.work[1] = 0u;
}
} // namespace

hipError_t tptLaunchTraceLens(const KernelArgs& a, int hs, int fold, bool ldsScene, int blocks, size_t lds, hipStream_t stream)
{
    const FrameConsts& fc = a.fc;
    const int tilesX = (fc.width + 7) / 8, tilesY = (fc.height + 7) / 8;
    const bool consts = fc.spp >= 1 && fc.invSpp == 1.0f / (float)fc.spp && fc.seedMode == SEED_PER_PIXEL && fc.width >= 1 && fc.height >= 1 &&
                        fc.invWidth == 1.0f / (float)fc.width && fc.invHeight == 1.0f / (float)fc.height && a.nLocalRows == fc.height &&
                        a.stripeRows == fc.height && a.stripeStride == fc.height && a.stripeOffset == 0 && a.tilesX == tilesX &&
                        a.numItems == tilesX * tilesY * 64 && a.batchFrames == 1 && a.laneCap == 64 && a.noRefill == 0 && !a.chunkOrder &&
                        !a.chunkCost && (a.chunkSize == 256 || a.chunkSize == 64) &&
                        a.numChunks == (a.numItems + a.chunkSize - 1) / a.chunkSize;
    if (!consts || a.lens.kind < LENS_EQUIRECT || a.lens.kind > LENS_ORTHO || a.rays || a.rayRadiance || a.rayHits || !a.frameColour ||
        !a.rayCounter || !a.work)
        return hipErrorInvalidValue;
    if (blocks < 1 || blocks > a.numChunks || (unsigned)blocks != a.totalWaves || lds > 160 * 1024) return hipErrorInvalidValue;
    if (fold == FOLD_RECURSIVE && a.ldsStackLevels < TPT_MAX_DEPTH && (!a.stackBuf || a.stackStride != blocks * TPT_BLOCK)) return hipErrorInvalidValue;
    gPlan[0] = a.numItems; gPlan[1] = a.chunkSize; gPlan[2] = a.chunkShift; gPlan[3] = a.numChunks;
    gPlan[4] = blocks; gPlan[5] = (long long)lds; gPlan[6] = a.tilesX; gPlan[7] = a.chunksPerFrame;
    if (gPlanOnly) return hipErrorNotReady;
    ++gLaunches;
    LensJob J; J.a = a; J.hs = hs; J.fold = fold; J.ldsScene = ldsScene;
    hostemuEnqueue(stream, runLens, &J, sizeof(J));
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuLensLaunches() { return gLaunches; }
// {numItems, chunkSize, chunkShift, numChunks, workgroups, LDS bytes, tilesX, chunksPerFrame} of the last launch that passed the checks
extern "C" __attribute__((visibility("default"))) void hostemuLensPlan(long long* out8) { memcpy(out8, gPlan, sizeof gPlan); }
extern "C" __attribute__((visibility("default"))) void hostemuLensPlanOnly(int on) { gPlanOnly = on != 0; }
