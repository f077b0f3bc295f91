// tpt_host_pipeline.cpp -- one frame through the pipeline: plan, per-slot buffers, trace launch on its own stream, the ordered blend; tail helpers; tptDrawDevice / tptDrawDeviceBatch and the blocking calls (replaces the fan-out / join of DrawTest, Test.cpp:344-367)
// (one of the host runtime's translation units: tpt_context.h lists them)
#include "tpt_context.h"

using namespace tpt;
using namespace tpth;

namespace tpth {

// Everything decided about a frame before anything is enqueued.
struct FramePlan {
    KernelArgs a;
    bool rowSerial = false, queued = false, ldsScene = false, useOrder = false;
    size_t lds = 0;
    int occ = 0, threadsPerBlock = 0, blocks = 0;
    int nOverlap = 1;           // launches that may run side by side (trace streams in use)
    int nSlots = 1, slot = 0;   // frames that may be enqueued ahead / this frame's slot (colour, stack buffers, events)
    int batch = 1;              // frames traced by this launch (tptDrawDeviceBatch)
    bool plainFrame = true;     // one frame, no planes, no per-frame table: what the lane-refill kernel traces as well
    const char* entry = "tptDrawDevice"; // (whose launch this is, for a refusal)
};

// Per-slot device buffers (frame colour, bounce stacks) are allocated for ALL slots of the pipeline at
// once, sized for the largest grid this kernel can ever be launched with at this frame shape -- never on the per-frame
// path: a lazily grown slot drained the whole pipeline (two stream syncs + hipFree/hipMalloc) on every first use, and with
// fewer warm-up frames than slots those drains landed inside the caller's timed region (round-1 driver bench: 17 instead
// of 35 Gray/s).  A re-allocation happens only when the frame shape / kernel variant / overlap asks for MORE than any
// earlier frame did; it synchronises everything once.
int syncAllStreams();
int reserveSlotBuffers(int nSlots, size_t colourBytes, size_t stackBytes)
{ // (stack buffers are used while the kernel runs only: indexed by stream, allocated for the first kMaxOverlap slots)
    // Memory that a large batched frame pinned is given back when the caller returns to frames a quarter of that size and more
    // than 1 GiB of colour slots is held (one drain, like a growth); anything smaller stays (no churn between similar shapes).
    // ... and only after 8 launches in a row were that small: a caller that alternates large batches with a small tail chunk
    // (33..40 frames through tptDrawDeviceBatch: 32 + 1..8) must not free and re-allocate gigabytes on every call.
    const bool small = colourBytes * 4 <= g.colourCap && g.colourCap * (size_t)g.slotsReserved > (1ull << 30);
    g.smallStreak = small ? g.smallStreak + 1 : 0;
    // ... and never while a launch traced ahead of its call (g.pending) still waits for its blends: its ticket points into the very
    // buffers a shrink frees.
    const bool shrink = small && g.smallStreak >= 8 && g.pending.empty();
    if (shrink) g.smallStreak = 0;
    if (!shrink && nSlots <= g.slotsReserved && colourBytes <= g.colourCap && stackBytes <= g.stackCap) return 0;
    // ... nor may the slots GROW under such a frame: growth frees and re-allocates every colour slot (found by the round-4 advisor:
    // the second row-serial batch asking for more than the first had got).  The caller retries with less or drops its look-ahead.
    if (!g.pending.empty() && colourBytes > g.colourCap)
        return refuse("frame buffers: the colour slots are held by frames traced ahead of their call; a larger launch has to wait for them");
    int rc = syncAllStreams();
    if (rc) return rc;
    if (shrink) {
        for (int k = 0; k < g.slotsReserved; ++k) {
            if (g.dColour[k]) HIPCHK(hipFree(g.dColour[k]));
            g.dColour[k] = nullptr;
        }
        g.colourCap = 0;
    }
    const size_t cb = colourBytes > g.colourCap ? colourBytes : g.colourCap, sb = stackBytes > g.stackCap ? stackBytes : g.stackCap;
    const int n = nSlots > g.slotsReserved ? nSlots : g.slotsReserved;
    {
        // refuse BEFORE anything is freed when the device cannot hold the request (a failed hipMalloc half-way would leave the
        // context without its buffers)
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
            size_t need = 0;
            for (int k = 0; k < n; ++k) {
                const bool fresh = k >= g.slotsReserved;
                if (fresh || cb > g.colourCap) need += cb;
                if ((fresh || sb > g.stackCap) && k < Context::kMaxOverlap) need += sb;
            }
            const size_t held = (cb > g.colourCap ? g.colourCap * (size_t)g.slotsReserved : 0);
            if (need > freeB + held)
                return refuse("frame buffers: " + std::to_string(need >> 20) + " MiB needed for " + std::to_string(n) + " frame slots, " +
                            std::to_string((freeB + held) >> 20) + " MiB available on the device (smaller batch / frame, or fewer frames in flight: tptSetFrameOverlap)");
        }
    }
    auto grow = [&]() -> int {
        for (int k = 0; k < n; ++k) {
            const bool fresh = k >= g.slotsReserved;
            if (fresh || cb > g.colourCap) {
                if (g.dColour[k]) HIPCHK(hipFree(g.dColour[k]));
                g.dColour[k] = nullptr;
                if (cb) HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dColour[k]), cb));
            }
            if (fresh || sb > g.stackCap) {
                if (g.dStack[k]) HIPCHK(hipFree(g.dStack[k]));
                g.dStack[k] = nullptr;
                if (sb && k < Context::kMaxOverlap) HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dStack[k]), sb));
            }
        }
        return 0;
    };
    if ((rc = grow())) {
        // an allocation failed half-way (the memory check above is advisory: another process may have taken the memory): no slot may
        // keep a capacity its buffer does not have -- give everything back, the next frame reserves afresh
        for (int k = 0; k < Context::kMaxSlots; ++k) {
            (void)hipFree(g.dColour[k]); g.dColour[k] = nullptr;
            (void)hipFree(g.dStack[k]); g.dStack[k] = nullptr;
        }
        (void)hipGetLastError();
        g.colourCap = g.stackCap = 0; g.slotsReserved = 0;
        // ... and no pending launch may keep pointing into a buffer that is gone: a later serve would blend from freed memory, and
        // every later enqueueTrace would be refused with "colour slots are held by frames traced ahead".  (Everything was drained
        // before the buffers grew: nothing to wait for.)
        g.pending.n = 0;
        return rc;
    }
    g.colourCap = cb; g.stackCap = sb; g.slotsReserved = n;
    g.slotReservations++;
    return 0;
}

// The context is set up for the path-queue kernel: persistent 3, two-phase HitSpheres, per-pixel seeds, the recursive fold, and at most
// 2047 spp (its 64-B path record holds 11 bits of sample index).  chooseKernel adds what a frame and a scene must fit.
static bool pathQueueContext(int spp)
{
    return g.persist == 3 && g.hs == HS_TWO_PHASE && g.seedMode == SEED_PER_PIXEL && g.foldMode == FOLD_RECURSIVE && spp <= 2047;
}
static bool pathQueueContext() { return pathQueueContext(g.spp); }

// A CU's LDS, and how many path-queue workgroups of `lds` bytes it holds: each is counted with a 256-B margin, except that a workgroup
// that fits the CU on its own is one workgroup, margin or not (never 0 for lds <= kCuLdsBytes: sizeGrid and maxGridBlocks size the grid
// by it).
static const size_t kCuLdsBytes = 160 * 1024;
static int queueOccupancy(size_t lds)
{
    const int n = (int)(kCuLdsBytes / (lds + 256));
    return n < 1 && lds <= kCuLdsBytes ? 1 : n;
}
// Lights whose table (32 B each) the path-queue kernel's LDS holds beside everything else this launch keeps there.
static int queueLightRoom(KernelArgs a, bool ldsScene)
{
    a.scene.nLights = 0;
    const size_t rest = tptQueueLdsBytes(a, ldsScene);
    const size_t room = rest < kCuLdsBytes ? (kCuLdsBytes - rest) / 32 : 0;
    return room < (size_t)TPT_MAX_LIGHTS ? (int)room : TPT_MAX_LIGHTS;
}

// The lane-refill kernel's share of the plan (chooseKernel for a launch that is not queued; tptTraceRaysDevice): whether the scene is
// staged in LDS, the bounce-stack levels kept there (a.ldsStackLevels), and the bytes both take.
size_t laneRefillLds(KernelArgs& a, bool& ldsScene)
{
    // LDS scene staging: default when {centre, r^2} + 1/r (20 B per padded sphere) + 48 B of material per sphere fit in
    // 40 KB (46 spheres: 3.2 KB; up to ~600 spheres)
    const int nPad = a.scene.nPairs * 2;
    ldsScene = g.ldsScene < 0 ? ((size_t)nPad * 20 + (size_t)a.scene.nSpheres * 48 <= 40960) : (g.ldsScene != 0);
    if (a.scene.nGroups > 0) ldsScene = false; // the LDS-staging kernels are built without the grouped traversal
    // bounce stack: the lane-refill kernel keeps the first levels in LDS and spills the rare deep ones to global memory
    a.ldsStackLevels = g.foldMode == FOLD_RECURSIVE ? g.ldsStackLevels : TPT_MAX_DEPTH;
    return tptLdsBytes(a, g.foldMode, ldsScene);
}
bool fitsCuLds(size_t lds) { return lds <= kCuLdsBytes; }
// ... and its workgroups per CU at that size, as the runtime answers for the context's instantiation
// (the runtime's answer is remembered per kernel and LDS size, to the 16 bytes the sizes are multiples of: a coarser key once
//  handed a launch the occupancy of a neighbour 32 bytes smaller)
int laneRefillOccupancy(bool ldsScene, size_t lds)
{
    const int key = (g.hs ? 8 : 0) | (g.foldMode ? 4 : 0) | (ldsScene ? 1 : 0) | ((int)(lds / 16) << 5);
    auto it = g.occCache.find(key);
    if (it != g.occCache.end()) return it->second;
    const int occ = tptTraceOccupancy(g.hs, g.foldMode, ldsScene, lds);
    g.occCache[key] = occ;
    return occ;
}

// Which kernel runs this frame, how much LDS it takes, how many workgroups fit on a CU.
int chooseKernel(FramePlan& P)
{
    KernelArgs& a = P.a;
    P.rowSerial = g.seedMode == SEED_ROW_SERIAL;
    const size_t ldsV1 = laneRefillLds(a, P.ldsScene);
    // path-queue kernel: it packs a pixel as x | y << 16 and a path id as 16 bits (larger frames take the lane-refill kernel), and its
    // path record 16 bits of sphere id
    // (a launch with a sample count per pixel, tptDrawDeviceAdaptive: the context's spp plays no part)
    P.queued = pathQueueContext(a.sampleCounts ? 1 : g.spp) && a.fc.width <= 65535 && a.fc.height <= 65535 && a.scene.nSpheres <= 65534;
    // grouped scene on the path-queue kernel: the second level of the bounds filter reads the groups' pair records per lane -- from LDS
    // when they fit the area the grouped instantiation's smaller path pool leaves (<= 544 groups), else from global memory; the host
    // that asked for the FLAT filter (hitSpheres variant 3: the A/B) or for the matrix cores (variant 4) gets neither
    a.ldsGroupPairs = -1;
    if (P.queued && !P.ldsScene && a.scene.nGroups > 0 && a.scene.gmxTiles == 0 && a.scene.nSuperPairs > 0 && g.useMatrix)
        a.ldsGroupPairs = tptQueueGroupPairsInLds(a.scene.nGroups, a.scene.nSuperPairs);
    P.lds = P.queued ? tptQueueLdsBytes(a, P.ldsScene) : ldsV1;
    if (P.queued && a.ldsGroupPairs > 0 && queueOccupancy(P.lds) < 2) {
        // the groups' bounds in LDS would cost the second workgroup per CU (many lights beside them): second level from global memory
        a.ldsGroupPairs = 0;
        P.lds = tptQueueLdsBytes(a, P.ldsScene);
    }
    if (a.scene.nLights > TPT_MAX_LIGHTS)
        return fail("tptDrawDevice: too many emissive spheres for the LDS light table (" + std::to_string(TPT_MAX_LIGHTS) + " at most)");
    if (P.queued && P.lds > kCuLdsBytes && !(P.ldsScene && g.ldsScene > 0)) {
        // The light table beside the path records is more than a CU's LDS holds.  A single frame without planes or tables is
        // traced by the lane-refill kernel, whose LDS has room for every light table up to the cap; the launches that exist on the
        // path-queue kernel only say how many lights they take beside this scene.
        if (!P.plainFrame || ldsV1 > kCuLdsBytes)
            return fail(std::string(P.entry) + ": " + std::to_string(a.scene.nLights) + " emissive spheres, and the path-queue kernel's LDS holds the light table of at most " +
                        std::to_string(queueLightRoom(a, P.ldsScene)) + " beside this scene (tptDrawDevice and tptDraw take up to " + std::to_string(TPT_MAX_LIGHTS) +
                        " on the lane-refill kernel)");
        P.queued = false;
        a.ldsGroupPairs = -1;
        P.lds = ldsV1;
    }
    if (P.lds > kCuLdsBytes) return fail("tptDrawDevice: scene too large for LDS staging; use tptSetKernelVariant(.., .., 0)");
    if (P.queued) {
        a.ldsStackLevels = 1; // level 0 of the bounce stack sits in the path record (LDS), levels 1-9 in global memory
        // two workgroups per CU are worth more than the scene in LDS: a scene that costs the second workgroup its place
        // is read from global memory (L2) instead
        if (g.ldsScene < 0 && P.ldsScene && queueOccupancy(P.lds) < 2 && queueOccupancy(tptQueueLdsBytes(a, false)) >= 2) {
            P.ldsScene = false;
            P.lds = tptQueueLdsBytes(a, false);
        }
    }
    if (P.queued) {
        P.occ = queueOccupancy(P.lds); // (arithmetic: nothing to remember)
    } else {
        P.occ = laneRefillOccupancy(P.ldsScene, P.lds);
    }
    P.threadsPerBlock = P.queued ? tptQueueThreadsPerBlock() : TPT_BLOCK;
    return 0;
}

// Work items, chunk size and the number of workgroups of this launch.
void sizeGrid(FramePlan& P)
{
    KernelArgs& a = P.a;
    const int resident = g.traceCUs * P.occ; // workgroups that can be co-resident (on the CUs the trace streams may use)
    const int wavesPerBlock = P.threadsPerBlock / 64;
    int chunk = P.rowSerial ? 1 : TPT_CHUNK_PIXELS;
    // small frames: hand out single 8x8 tiles so every resident wave gets several chunks
    if (!P.rowSerial && a.numItems / TPT_CHUNK_PIXELS < 8 * resident * wavesPerBlock) chunk = 64;
    if (P.queued) chunk = 64; // the path-queue kernel accounts its pixel pools in 64-pixel chunks
    a.chunkSize = chunk;
    a.numChunks = (a.numItems + chunk - 1) / chunk;
    a.chunksPerFrame = a.numChunks;
    a.numChunks *= P.batch; // a batched launch hands out the chunks of all its frames, frame after frame
    int blocks = (a.numChunks + wavesPerBlock - 1) / wavesPerBlock;
    a.laneCap = 64;
    a.noRefill = (g.persist == 0 && !P.rowSerial && !P.queued) ? 1 : 0; // (one thread per pixel: tptSetKernelVariant persistent 0)
    if (P.rowSerial && !P.queued) {
        // Row-serial seeds: a work item is a whole image row (thousands of sequential rays), and there are few of them -- rows x
        // frames of the batch.  A wave that fills all 64 lanes leaves most SIMDs idle; a SIMD runs one wave's instructions at
        // the same rate whether 8 or 64 of its lanes are alive, so the items are dealt out over as many waves as there are
        // SIMDs (4 per CU), at least 4 lanes each.
        // (k launches in flight -- the deepest pipeline this caller has built so far -- share the SIMDs: k times the lanes)
        const int simds = g.traceCUs * 4, k = g.depthOverride > 0 ? g.depthOverride : (g.streamDepth > 1 ? g.streamDepth : 1);
        int cap = (int)(((long long)a.numChunks * k + simds - 1) / simds);
        cap = cap < 4 ? 4 : (cap > 64 ? 64 : cap);
        a.laneCap = cap;
        blocks = (a.numChunks + cap - 1) / cap;
    }
    // Frames in flight share the machine: with k trace kernels side by side each one gets fill / k of the resident
    // workgroups -- its pools then stay in steady state longer before they drain, and the launches behind it fill the
    // gaps.  fill = 200 % on a single GPU (measured best), 100 % when the frame is sharded over ranks (oversubscription
    // buys nothing on small tiles).  A caller that synchronises every frame has nothing in flight and gets the full grid.
    int cap;
    if (g.gridDiv > 0) {
        cap = resident / g.gridDiv;
    } else {
        // fill = how many times the machine the launches in flight ask for together: 200 % on a single GPU (64 workgroups per
        // launch at 16 in flight: long steady states; 100 %: 54.6 vs 55.9 Gray/s), 100 % when the frame is sharded over ranks
        // (oversubscription buys nothing on small tiles).  Rounds 2-3 gave the first 24 frames after an idle pipeline 400 %:
        // worth +4.5 % on a burst of exactly 20 frames (whose last launches then fill the machine as it empties), but -8 % on 30
        // frames and -1.5 % on 100 (profiles/r04/r04_run9.log) and 1.8x the memory traffic per launch -- a constant fitted to
        // one command line; removed in round 4.
        const int fill = g.gridFill > 0 ? g.gridFill : (g.numParts > 1 ? 100 : 200);
        // k = how many launches share the machine.  Not just what is in flight right now: a caller that streams frames
        // (enqueue, enqueue, ..., synchronise once) starts every burst with an empty pipeline, and whole-machine grids
        // for the first frames of a burst serialise them (each with its own tail) -- a 20-frame burst ran at 24 instead
        // of 33 Gray/s.  So the deepest pipeline this caller has built is remembered (streamDepth) and only forgotten
        // when two consecutive frames find the pipeline empty: that is a caller who synchronises every frame
        // (the reference's DrawTest contract) and gets the whole machine.
        const int inFlight = framesInFlight(P.nSlots);
        if (inFlight == 0 && g.prevInFlight == 0) g.streamDepth = 1;
        if (inFlight + 1 > g.streamDepth) g.streamDepth = inFlight + 1;
        g.prevInFlight = inFlight;
        int k = g.streamDepth;
        if (g.depthOverride > 0) k = g.depthOverride; // the host-pointer path knows exactly how deep its pipeline is
        if (k > P.nOverlap) k = P.nOverlap;
        cap = (int)((long long)resident * fill / (100ll * k));
        if (cap > resident) cap = resident;
        const int floorBlocks = resident / (2 * (P.nOverlap > 1 ? P.nOverlap : 1));
        if (cap < floorBlocks) cap = floorBlocks;
    }
    if (P.rowSerial && !P.queued) cap = resident; // (row-serial launches are latency-bound: one short wave per SIMD, whatever else is in flight)
    if (cap < 1) cap = 1;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    P.blocks = blocks;
    a.totalWaves = (unsigned)(blocks * wavesPerBlock);
}

// Largest number of workgroups sizeGrid can ever pick for this kernel at this frame shape.
int maxGridBlocks(const FramePlan& P)
{
    const KernelArgs& a = P.a;
    const int wavesPerBlock = P.threadsPerBlock / 64;
    const int resident = g.traceCUs * P.occ;
    const int minChunk = P.rowSerial ? 1 : 64;
    const int byWork = (((a.numItems + minChunk - 1) / minChunk) * P.batch + wavesPerBlock - 1) / wavesPerBlock;
    int m = resident < byWork ? resident : byWork;
    return m < 1 ? 1 : m;
}

// Per-slot buffers of this frame: colour, bounce-stack spill / per-path stacks.
int ensureFrameBuffers(FramePlan& P, int w)
{
    KernelArgs& a = P.a;
    const int slot = P.slot;
    const int maxBlocks = maxGridBlocks(P);
    const bool needStack = g.foldMode == FOLD_RECURSIVE && a.ldsStackLevels < TPT_MAX_DEPTH;
    const size_t maxColumns = (size_t)maxBlocks * (size_t)(P.queued ? tptQueuePathsPerBlock() : P.threadsPerBlock);
    const size_t stackBytes = needStack ? maxColumns * (size_t)(TPT_MAX_DEPTH - a.ldsStackLevels) * sizeof(f4) : 0;
    int rc = reserveSlotBuffers(P.nSlots, (size_t)a.nLocalRows * w * sizeof(f4) * (size_t)P.batch, stackBytes);
    if (rc) return rc;
    a.frameColour = g.dColour[slot];
    a.work = g.dWork + 16 * slot;
    a.rayCounter = g.dRays;
    a.stackBuf = nullptr;
    a.stackStride = 0;
    if (needStack) {
        a.stackBuf = g.dStack[slot % P.nOverlap];
        a.stackStride = P.queued ? P.blocks * tptQueuePathsPerBlock() : P.blocks * P.threadsPerBlock;
        // the columns of a helper grid (workgroups blocks .. 2 * blocks - 1 at most) lie behind the launch's own: one stride for both
        if (P.queued) a.stackStride = (2 * P.blocks < maxBlocks ? 2 * P.blocks : maxBlocks) * tptQueuePathsPerBlock();
    }
    a.pathBuf = nullptr;
    return 0;
}

// ... and the staged scene's light table fits beside that kernel's path records: what decides whether frames are traced several to a
// launch (chooseKernel sends a single frame whose lights do not fit to the lane-refill kernel; a batch has no such way out).
static bool pathQueueTakesScene()
{
    if (!pathQueueContext()) return false;
    if (!activeSet()) return true; // (nothing staged yet: the launch itself decides)
    FramePlan P;
    P.a = KernelArgs{};
    P.a.scene = deviceView();
    P.a.fc.width = P.a.fc.height = 8;
    P.a.batchFrames = 1;
    return chooseKernel(P) == 0 && P.queued;
}

int syncAllStreams()
{
    for (int k = 0; k < Context::kMaxOverlap; ++k) HIPCHK(hipStreamSynchronize(g.traceStream[k]));
    for (int k = 0; k < Context::kMaxSlots; ++k) g.hrec[k].valid = false; // (nothing is in flight any more)
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

// The caller is about to block: give the newest launches that have not finished a second grid each (tpt_device.h).  The newest launches
// first -- they have the most left -- and at most helperMax of them; a launch is helped once.  hipEventQuery is a hint only: a launch
// that finishes a microsecond later closes its counter block and the helpers leave at once.
int launchTailHelpers()
{
    if (!g.helpersOn) return 0;
    int order[Context::kMaxSlots], n = 0;
    for (int s = 0; s < Context::kMaxSlots; ++s) {
        Context::HelperRec& R = g.hrec[s];
        if (!R.valid) continue;
        if (hipEventQuery(g.evTrace[s]) == hipSuccess) { R.valid = false; continue; }
        (void)hipGetLastError();
        order[n++] = s; // every launch still in flight, helped already or not
    }
    if (n < 2) return 0; // (a caller that waits for every frame has nothing to rebalance)
    for (int i = 1; i < n; ++i) // newest first
        for (int j = i; j > 0 && (int)(g.hrec[order[j]].a.gen - g.hrec[order[j - 1]].a.gen) > 0; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    // The k-th newest launch is helped from the stream of the k-th OLDEST launch that has nothing queued behind it: that stream is
    // the next to fall idle for good -- a burst longer than the 16 streams has its last launches queued behind its first ones, and a
    // helper placed there would start when everything is over (profiles/r04/r04_run23.log).  The helper may well start before the
    // launch it helps (it only waits for what that launch waits for): the pool is simply part-consumed when the launch arrives.
    // (Streams of their own were tried first: four more streams in the process cost the whole pipeline a factor 2.4 -- the
    // runtime's hardware queues are a small shared pool; r04_run21.log, r04_run22.log.)
    hipStream_t freeSoon[Context::kMaxSlots];
    int nFree = 0;
    for (int i = n - 1; i >= 0; --i) { // oldest first
        hipStream_t ts = g.hrec[order[i]].ts;
        int queued = 0;
        for (int j = 0; j < n; ++j) queued += g.hrec[order[j]].ts == ts ? 1 : 0;
        if (queued == 1) freeSoon[nFree++] = ts;
    }
    for (int i = 0; i < n / 2 && i < Context::kHelperMax && i < nFree; ++i) {
        Context::HelperRec& R = g.hrec[order[i]];
        if (R.helped) continue;
        R.helped = true;
        int extra = R.maxBlocks - R.blocks;
        if (extra > R.blocks) extra = R.blocks; // (two and three times the launch's own grid measured no better, profiles/r05/r05_run2.log)
        if (extra < 1) continue;
        KernelArgs h = R.a;
        h.helperBase = R.blocks;
        h.helperPct = Context::kHelperPct;
        hipStream_t hs = freeSoon[i];
        if (hs == R.ts) continue; // (its own stream: it would run after the launch it is meant to help)
        HIPCHK(hipStreamWaitEvent(hs, g.evPre[order[i]], 0));
        HIPCHK(tptLaunchTraceQueue(h, R.ldsScene, extra, R.lds, hs));
        g.helperLaunches++;
    }
    return 0;
}

// Cost-ordered work distribution of the lane-refill kernel: statistics and order tables for this chunk count.
int prepareChunkOrder(FramePlan& P)
{
    KernelArgs& a = P.a;
    a.chunkOrder = nullptr;
    a.chunkCost = nullptr;
    a.chunkShift = 6;
    P.useOrder = g.costOrder && !P.rowSerial && !P.queued && a.numChunks > 1 &&
                 (a.chunkSize & (a.chunkSize - 1)) == 0;
    if (!P.useOrder) return 0;
    int sh = 0;
    while ((1 << sh) < a.chunkSize) ++sh;
    a.chunkShift = sh;
    const size_t bytes = sizeof(unsigned) * (size_t)a.numChunks;
    if (a.numChunks > g.chunkCap) {
        int rc = syncAllStreams();
        if (rc) return rc;
        if (g.dChunkCost) HIPCHK(hipFree(g.dChunkCost));
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dChunkCost), bytes));
        for (int k = 0; k < Context::kOrderTables; ++k) {
            if (g.dChunkOrder[k]) HIPCHK(hipFree(g.dChunkOrder[k]));
            g.dChunkOrder[k] = nullptr;
            HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dChunkOrder[k]), bytes));
        }
        for (int k = 0; k < Context::kMaxOverlap; ++k) {
            if (g.dChunkSnap[k]) HIPCHK(hipFree(g.dChunkSnap[k]));
            g.dChunkSnap[k] = nullptr;
            HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dChunkSnap[k]), bytes));
        }
        g.chunkCap = a.numChunks;
        g.chunkCount = 0;
    }
    if (g.chunkCount != a.numChunks) { // new resolution / sharding: statistics start over
        int rc = syncAllStreams();
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(g.dChunkCost, 0, bytes, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        g.chunkCount = a.numChunks;
        g.orderSeq = 0;
    }
    a.chunkCost = g.dChunkCost;
    return 0;
}

// Give the launch on `ts` an order table: re-sorted from the statistics gathered so far (every frame until the first
// frames' statistics have certainly arrived -- the sort runs beside up to nOverlap unfinished frames -- then every
// 32nd), or the most recent one.  Tables rotate over kOrderTables buffers (> frames in flight): a trace kernel still in
// flight keeps reading the one it was given.
int enqueueChunkOrder(FramePlan& P, hipStream_t ts)
{
    if (!P.useOrder) return 0;
    if (g.orderSeq > 0) {
        const int fresh = (int)(g.orderSeq % Context::kOrderTables);
        if (g.orderSeq <= (unsigned long long)(2 * P.nSlots + 2) || (g.orderSeq & 31ull) == 0ull) {
            HIPCHK(tptLaunchChunkOrder(g.dChunkCost, g.dChunkSnap[P.slot % P.nOverlap], g.dChunkOrder[fresh], P.a.numChunks, ts));
            HIPCHK(hipEventRecord(g.evOrder, ts));
            g.orderStream = ts;
            g.lastOrderTable = fresh;
        } else if (g.orderStream && g.orderStream != ts) {
            // the most recent table may still be being written by another stream's sort kernel
            HIPCHK(hipStreamWaitEvent(ts, g.evOrder, 0));
        }
        P.a.chunkOrder = g.dChunkOrder[g.lastOrderTable];
    }
    g.orderSeq++;
    return 0;
}

static const size_t kViewCamBytes = sizeof(CameraPOD) * kMaxBatch; // a slot's cameras; its centres lie behind them when a launch takes both
// tptDrawDeviceViews: the per-slot camera tables and view ray counters (Context::ViewSlot), allocated by the first views call (a
// context that never draws views never holds them).
int ensureViewSlots()
{
    if (g.dViews) return 0;
    // (a slot's table: the cameras, then the centres of a launch that takes both -- tptDrawDeviceCameraClip --, then the ray counters)
    // (the widest centres table: tptDrawDeviceKeyframeClip's, TPT_Q_KEYS_MAX centres per frame)
    static_assert(TPT_Q_KEY_TABLE_BYTES >= 2 * sizeof(f4) * kMaxBatch && TPT_Q_KEY_TABLE_BYTES == TPT_Q_KEYS_MAX * sizeof(f4) * kMaxBatch, "one table area serves both kinds of centres");
    const size_t camBytes = kViewCamBytes, tableBytes = camBytes + TPT_Q_KEY_TABLE_BYTES, perSlot = tableBytes + sizeof(unsigned long long) * kMaxBatch;
    static_assert(kViewCamBytes % 16 == 0, "the centres and the ray counters behind a slot's cameras stay aligned");
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dViews), perSlot * Context::kMaxSlots));
    if (hipHostMalloc(reinterpret_cast<void**>(&g.hViewsStage), tableBytes * Context::kMaxSlots, 0) != hipSuccess) {
        (void)hipFree(g.dViews);
        g.dViews = nullptr;
        g.hViewsStage = nullptr;
        return hipFail(hipErrorOutOfMemory, "tptDrawDeviceViews: pinned camera staging");
    }
    for (int k = 0; k < Context::kMaxSlots; ++k) {
        Context::ViewSlot& V = g.views[k];
        V.dev = reinterpret_cast<CameraPOD*>(g.dViews + perSlot * k);
        V.rays = reinterpret_cast<unsigned long long*>(g.dViews + perSlot * k + tableBytes);
        V.stage = reinterpret_cast<CameraPOD*>(reinterpret_cast<char*>(g.hViewsStage) + tableBytes * k);
        V.copyEnqueued = false;
        if (!V.evUploaded) HIPCHK(hipEventCreateWithFlags(&V.evUploaded, kOrderingEvent));
    }
    return 0;
}

// tptDrawDeviceAov: the per-path sums (Context::dAovSums) for the largest grid this frame shape can take, and the ordering event;
// made by the first AOV call, grown (after a drain) when a later one asks for more.  tptDrawDeviceMoments (`momentsBytes` > 0): a
// third f4 per path, and the frame's moments plane (Context::dMoments) of that many bytes -- one plane per frame of the launch for
// tptDrawDeviceAnimationMoments, which (`halves` 2) takes both buffers twice: its launches alternate between the halves (Context::evClip).
int ensureAovSums(const FramePlan& P, size_t momentsBytes, int halves)
{
    if (!g.evAov) HIPCHK(hipEventCreateWithFlags(&g.evAov, kOrderingEvent));
    for (hipEvent_t& e : g.evClip)
        if (!e) HIPCHK(hipEventCreateWithFlags(&e, kOrderingEvent));
    const size_t need = (momentsBytes ? 3 : 2) * sizeof(f4) * (size_t)maxGridBlocks(P) * (size_t)tptQueuePathsPerBlock() * (size_t)halves;
    momentsBytes *= (size_t)halves;
    if (need <= g.aovSumsBytes && momentsBytes <= g.momentsBytes) return 0;
    int rc = syncAllStreams(); // (an earlier AOV launch, or its blend, may still be reading the old buffers)
    if (rc) return rc;
    if (need > g.aovSumsBytes) {
        (void)hipFree(g.dAovSums);
        g.dAovSums = nullptr;
        g.aovSumsBytes = 0;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dAovSums), need));
        g.aovSumsBytes = need;
    }
    if (momentsBytes > g.momentsBytes) {
        (void)hipFree(g.dMoments);
        g.dMoments = nullptr;
        g.momentsBytes = 0;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dMoments), momentsBytes));
        g.momentsBytes = momentsBytes;
    }
    return 0;
}

// First half of a frame: plan, buffers, trace kernel on the slot's stream.  `frameRays`: where the kernel adds its ray
// count (the context's counter, or a per-slot one for frames that are traced ahead of their DrawTest call).
// `table` (tptDrawDeviceViews, tptDrawDeviceAnimation): what differs between the batch's frames (host memory, copied to the slot's
// table on the frame's stream) -- cameras: `batch` views of frame frameCount, traced by the views kernel; centres: `batch` frames of an
// animated scene, traced by the animation kernel; neither: the plain kernel; both (with the planes of a clip, tptDrawDeviceCameraClip): a
// camera and the centres per frame, every frame with its own seeds.  Every frame counts its rays into the slot's counters.
// `aov` (tptDrawDeviceAov, a single frame): the caller's first-hit planes, written by the AOV kernel behind the context stream.  With
// moments and a centres table (tptDrawDeviceAnimationMoments): the planes of `batch` frames, h * w pixels apart, and as many moments planes.
int enqueueTrace(int frameCount, int w, int h, unsigned testFlags, unsigned long long* frameRays, TraceTicket& T, int batch, int rayStride,
                 const BatchTable* table, const AovPlanes* aov)
{
    const CameraPOD* viewCams = table ? table->cams : nullptr;
    const f4* centres = table ? table->centres : nullptr;
    const f4* keyCentres = table ? table->keyCentres : nullptr; // (tptDrawDeviceKeyframeClip: the caller's centres, beside the cameras)
    if (g.sceneDirty || (g.curSet < 0 && g.pendingSet < 0)) { // tptSetScene after the last tptUpdate
        int rc = stageScene();
        if (rc) return rc;
    }
    FramePlan P;
    KernelArgs& a = P.a;
    a.scene = deviceView(); // pointers of the set this frame reads; its upload is enqueued below, on the frame's stream
    a.fc = makeFrameConsts(g.cam, w, h, g.spp, frameCount, testFlags, g.seedMode, g.config, g.animateSmoothing);
    a.nLocalRows = localRows(h);
    if (g.numParts > 1 && g.stripeRows > 0) {
        a.stripeRows = g.stripeRows;
        a.stripeStride = g.stripeRows * g.numParts;
        a.stripeOffset = g.stripeRows * g.part;
    } else {
        a.stripeRows = h > 0 ? h : 1;
        a.stripeStride = a.stripeRows;
        a.stripeOffset = 0;
    }
    T.valid = false;
    if (a.nLocalRows <= 0) return 0; // nothing to do on this rank
    a.tilesX = (w + 7) / 8;
    const int tilesY = (a.nLocalRows + 7) / 8;
    a.numItems = g.seedMode == SEED_ROW_SERIAL ? a.nLocalRows : a.tilesX * tilesY * 64;
    P.batch = batch;
    a.batchFrames = batch;
    a.framePlane = a.nLocalRows * w;
    a.chunksPerFrame = 0; // (sizeGrid)
    P.nOverlap = effectiveOverlap();
    // Twice as many colour slots as trace streams for frames up to 32 MB of colour (2 M pixels): the blends are ordered
    // (frame f after f - 1) but the trace kernels finish out of order, so with one slot per stream a stream whose kernel
    // finished early sits idle until every earlier frame has been blended.  With a spare slot its next kernel starts at
    // once.  Worth +3-8 % on tiles of a sharded C2 frame (rank 0 of 2 / 4 / 8), nothing at C2 on one GPU (the machine is
    // full either way), and -4 % at C3, where 16 launches of 190 ms running at once only crowd the caches: large frames
    // keep one slot per stream (profiles/r02/r02_run42.log, r02_evidence2.log).
    P.nSlots = P.nOverlap;
    const size_t colourBytesPerSlot = (size_t)a.nLocalRows * (size_t)w * sizeof(f4) * (size_t)batch;
    if (P.nOverlap > 1 && g.slotFactor > 1 && colourBytesPerSlot <= (32ull << 20)) P.nSlots = 2 * P.nOverlap;
    // Every slot is sized for the largest frame seen, so the number of slots bounds the memory a large (batched) frame pins:
    // all colour slots together stay under 8 GiB (1280x720 x 32 frames per launch: 16 slots x 472 MB = 7.5 GB; a 4K x 8-frame
    // batch: 4 slots instead of 16), never fewer than 2 (one being traced, one being blended); a single slot above 4 GiB is
    // refused here, before anything is drained or freed.
    if (colourBytesPerSlot > (4ull << 30))
        return refuse("tptDrawDeviceBatch: " + std::to_string(colourBytesPerSlot >> 20) + " MiB of frame colour per launch (rows x width x 16 B x frames): over the 4096 MiB limit, use a smaller batch");
    while (P.nSlots > 2 && colourBytesPerSlot * (size_t)P.nSlots > (8ull << 30)) P.nSlots /= 2;
    if (rayStride > 0 && g.seedMode == SEED_ROW_SERIAL && P.nSlots > 4) P.nSlots = 4; // (the host path's row-serial batches: two alive at a time)
    if (P.nOverlap > P.nSlots) P.nOverlap = P.nSlots;
    P.slot = (int)(g.frameSeq % (unsigned long long)P.nSlots);
    g.frameSeq++;
    struct SeqGuard { // an enqueue that fails before its launch does not consume a slot of the pipeline
        bool launched = false;
        ~SeqGuard() { if (!launched) g.frameSeq--; }
    } seqGuard;

    int rc = 0;
    a.viewCams = nullptr;
    a.moveCentres = nullptr;
    a.keyCentres = nullptr;
    a.keyMask = 0;
    a.keyCount = 0;
    a.sampleCounts = aov ? aov->sampleCounts : nullptr; // (before chooseKernel: the context's spp plays no part in such a launch)
    if (table) {
        if ((rc = ensureViewSlots())) return rc;
        // (before chooseKernel: the views and animation kernels' LDS differs)
        if (viewCams) a.viewCams = g.views[P.slot].dev;
        if (centres) a.moveCentres = reinterpret_cast<const f4*>(reinterpret_cast<const char*>(g.views[P.slot].dev) + (viewCams ? kViewCamBytes : 0));
        if (keyCentres) {
            a.keyCentres = reinterpret_cast<const f4*>(reinterpret_cast<const char*>(g.views[P.slot].dev) + kViewCamBytes);
            a.keyMask = table->keyMask;
            a.keyCount = table->keyCount;
        }
        frameRays = g.views[P.slot].rays; // every frame counts its own rays (the blends add them to the running total)
        rayStride = 1;
    }
    P.plainFrame = batch == 1 && !aov && !viewCams && !centres && !keyCentres;
    P.entry = keyCentres ? "tptDrawDeviceKeyframeClip" : (viewCams && centres ? "tptDrawDeviceCameraClip" : (viewCams ? "tptDrawDeviceViews" :
              (centres ? (aov ? "tptDrawDeviceAnimationMoments" : "tptDrawDeviceAnimation") :
              (aov ? (aov->sampleCounts ? "tptDrawDeviceAdaptive" : (aov->moments ? "tptDrawDeviceMoments" : "tptDrawDeviceAov")) : (batch > 1 ? "tptDrawDeviceBatch" : "tptDrawDevice")))));
    if (aov && aov->entry) P.entry = aov->entry;
    if ((rc = chooseKernel(P))) return rc;
    if (viewCams && !P.queued)
        return refuse("tptDrawDeviceViews: needs the path-queue kernel (per-pixel seeds, recursive fold, two-phase HitSpheres, at most 2047 spp)");
    if ((centres || keyCentres) && (!P.queued || a.scene.nGroups > 0))
        return refuse(std::string(keyCentres ? "tptDrawDeviceKeyframeClip" : "tptDrawDeviceAnimation") + ": one launch per batch needs the path-queue kernel and a flat scene");
    const bool clip = aov && aov->moments && (centres || keyCentres); // (the frames of an animated clip with their planes: tptTraceClipKernel, tptCameraClipKernel, tptKeyframeKernel)
    if (viewCams && centres && !clip) return fail("enqueueTrace: a camera and the centres per frame go with a clip's planes");
    if (keyCentres && (!clip || !viewCams || centres)) return fail("enqueueTrace: the caller's centres per frame go with a clip's cameras and planes");
    if (aov && (!P.queued || !(clip || (batch == 1 && !viewCams && !centres))))
        return refuse("tptDrawDeviceAov: needs the path-queue kernel (per-pixel seeds, recursive fold, two-phase HitSpheres, at most 2047 spp)");
    // a batch is traced by the path-queue kernel (per-pixel seeds) or, in the reference's own seed mode, by the lane-refill
    // kernel: one lane per (frame, row) -- rows AND frames are independent RNG streams there (Test.cpp:280)
    if (batch > 1 && (!(P.queued || P.rowSerial) || w > 8192 || h > 8192 || (long long)a.nLocalRows * w * batch > (1ll << 30)))
        return refuse("tptDrawDeviceBatch: needs the path-queue kernel (per-pixel seeds, recursive fold, two-phase HitSpheres) or row-serial seeds, and a frame of at most 8192 x 8192 (2^30 pixels per batch)");
    sizeGrid(P);
    if ((rc = ensureFrameBuffers(P, w))) return rc;
    a.aovSums = a.aovAlbedo = a.aovNormalDepth = a.momentsOut = nullptr;
    if (aov) {
        if ((rc = ensureAovSums(P, aov->moments ? (size_t)a.nLocalRows * (size_t)w * sizeof(f4) * (size_t)batch : 0, clip ? 2 : 1))) return rc;
        // (a clip launch's half: the second one starts half the CAPACITY in, in whole f4 -- the buffers only change after a drain, so
        //  launches of different sizes agree where it lies)
        const size_t half = clip ? (size_t)(g.clipSeq & 1u) : 0;
        a.aovSums = g.dAovSums + half * (g.aovSumsBytes / (2 * sizeof(f4)));
        a.aovAlbedo = aov->albedo;
        a.aovNormalDepth = aov->normalDepth;
        if (aov->moments) a.momentsOut = g.dMoments + half * (g.momentsBytes / (2 * sizeof(f4)));
        a.aovPlane = clip ? h * w : 0;
    }
    if (frameRays) a.rayCounter = frameRays;
    a.rayCounterStride = rayStride; // (batched row-serial launch for the host path: one counter per frame of the batch)
    if ((rc = prepareChunkOrder(P))) return rc;
    g.lastBlocksPerCU = P.occ;
    g.lastLds = (int)P.lds;
    g.lastGrid = P.blocks;

    // trace(f) on its own stream (no dependency on the previous frame); the ordered blend follows on g.stream
    const int slot = P.slot;
    const bool pipelined = P.nOverlap > 1;
    hipStream_t ts = pipelined ? g.traceStream[slot % P.nOverlap] : g.stream;
    if (pipelined && g.resolveRecorded[slot]) {
        // Host pacing: the caller's thread waits here until the slot's previous frame has been blended, so it never runs more
        // than nSlots frames ahead and the queue's barrier below is already satisfied when the command processor reaches it.
        // A host that runs far ahead leaves every queue with an unsatisfied barrier at its head, and the command processor
        // polls them all: small frames retire at half the rate (C1, 400 frames: 6.7 -> 13.6 Gray/s; rank 0 of 8: 99 -> 128
        // aggregate; C2 unchanged; profiles/r02/r02_run40.log).  Pacing only: the stream wait below is what orders the work
        // (an event query may report "done" early on a re-recorded event).
        if (g.hostPace) {
            // (bounded: a caller whose stream is blocked behind something it will only enqueue later must not hang here)
            const auto t0 = std::chrono::steady_clock::now();
            unsigned spins = 0;
            while (hipEventQuery(g.evResolve[slot]) == hipErrorNotReady) {
                std::this_thread::yield();
                if ((++spins & 255u) == 0u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;
            }
            (void)hipGetLastError();
        }
        HIPCHK(hipStreamWaitEvent(ts, g.evResolve[slot], 0)); // colour buffer free again
    }
    if ((rc = enqueueSceneUpload(ts))) return rc; // behind the wait above: nobody reads the set being replaced any more
    if (aov && ts != g.stream) {
        // the caller's planes: written after everything enqueued on the context stream before this call (its blend, like the tile's,
        // follows the launch there); this also keeps the AOV launches, and their one buffer of sums, one after the other
        // ... except the later launches of one tptDrawDeviceAnimationMoments call, which alternate between two halves of the sums and
        // the staging and write planes of their own: each waits for the blends of the launch before the previous one (Context::evClip)
        if (clip) {
            const unsigned h = g.clipSeq & 1u;
            HIPCHK(hipEventRecord(g.evClip[h ^ 1u], g.stream)); // (behind the previous launch's blends: what the next launch waits for)
            HIPCHK(hipStreamWaitEvent(ts, aov->continues ? g.evClip[h] : g.evClip[h ^ 1u], 0));
        } else {
            HIPCHK(hipEventRecord(g.evAov, g.stream));
            HIPCHK(hipStreamWaitEvent(ts, g.evAov, 0));
        }
    }
    if (clip) g.clipSeq++;
    if (viewCams || centres || keyCentres) {
        // the launch's table, behind the same wait: the slot's previous launch has read its table; the previous copy out of the
        // slot's pinned staging (an earlier call on this slot) has left the host before the staging is overwritten
        static_assert(2 * sizeof(f4) * kMaxBatch <= sizeof(CameraPOD) * kMaxBatch, "a batch's moving centres fit the slot's camera table");
        Context::ViewSlot& V = g.views[slot];
        const f4* behind = keyCentres ? keyCentres : centres; // (the centres of this launch, of either kind)
        const size_t camBytes = sizeof(CameraPOD) * (size_t)batch, centreBytes = (keyCentres ? (size_t)TPT_Q_KEYS_MAX : 2) * sizeof(f4) * (size_t)batch;
        const size_t bytes = viewCams && behind ? kViewCamBytes + centreBytes : (viewCams ? camBytes : centreBytes); // (both: one copy, the centres behind the whole camera table)
        if (V.copyEnqueued) HIPCHK(hipEventSynchronize(V.evUploaded));
        if (viewCams) memcpy(V.stage, viewCams, camBytes);
        if (behind) memcpy(reinterpret_cast<char*>(V.stage) + (viewCams ? kViewCamBytes : 0), behind, centreBytes);
        HIPCHK(hipMemcpyAsync(V.dev, V.stage, bytes, hipMemcpyHostToDevice, ts));
        HIPCHK(hipEventRecord(V.evUploaded, ts));
        V.copyEnqueued = true;
    }
    if ((rc = enqueueChunkOrder(P, ts))) return rc;
    if (frameRays && frameRays != g.dRays) HIPCHK(hipMemsetAsync(frameRays, 0, sizeof(unsigned long long) * (size_t)(rayStride > 0 ? batch : 1), ts));
    const bool helpable = P.queued && pipelined && batch == 1 && !P.rowSerial && !table && !aov; // (single frames of the path-queue kernel)
    // the plain batched kernel (tptDrawDeviceBatch, STREAM launches) deals its workgroups to the frames, a pool of chunks per frame
    a.framePools = framePoolsOfLaunch(batch, P.blocks, P.queued && !P.rowSerial && !table && !aov, helpable);
    a.cutWord = nullptr;
    a.cutSerial = 0u;
    T.cutSerial = 0u;
    if (a.framePools > 0) {
        // the launch's cut word (tpt_frame_pools.h): the slot's, not cut.  The slot's previous launch has left the queue that held it
        // (LaunchQueue: served in full, or cut and dropped), so the host writes that launch's word no more, and whatever serial a late
        // reader of the old launch finds here is not its own.
        g.cutSerial = frameCutNextSerial(g.cutSerial);
        a.cutWord = g.hCut + slot;
        a.cutSerial = g.cutSerial;
        T.cutSerial = g.cutSerial;
        __atomic_store_n(g.hCut + slot, g.cutPreset > 0 ? frameCutWord(g.cutSerial, (unsigned)g.cutPreset) : 0u, __ATOMIC_RELEASE);
        g.cutPreset = 0;
    }
    a.helperBase = 0;
    a.helperPct = 0;
    a.gen = 0u;
    g.hrec[slot].valid = false;
    if (helpable) {
        if (++g.launchGen == 0u) g.launchGen = 1u;
        a.gen = g.launchGen;
        HIPCHK(hipEventRecord(g.evPre[slot], ts)); // the set upload and the slot's previous users are behind this point
    }
    const bool timeIt = g.kernelTiming && g.ktUsed < g.ktStart.size();
    if (timeIt) HIPCHK(hipEventRecord(g.ktStart[g.ktUsed], ts));
    if (P.queued)
        HIPCHK(tptLaunchTraceQueue(a, P.ldsScene, P.blocks, P.lds, ts));
    else
        HIPCHK(tptLaunchTrace(a, g.hs, g.foldMode, P.ldsScene, P.blocks, P.lds, ts));
    seqGuard.launched = true;
    if (timeIt) {
        HIPCHK(hipEventRecord(g.ktStop[g.ktUsed], ts));
        g.ktUsed++;
    }
    if (pipelined) HIPCHK(hipEventRecord(g.evTrace[slot], ts));
    if (helpable) {
        Context::HelperRec& R = g.hrec[slot];
        R.a = a; R.ldsScene = P.ldsScene; R.blocks = P.blocks; R.maxBlocks = maxGridBlocks(P); R.lds = P.lds;
        R.helped = false; R.valid = true; R.ts = ts;
    }
    T.slot = slot;
    T.nPixels = a.nLocalRows * w;
    T.pipelined = pipelined;
    T.lerpFac = a.fc.lerpFac;
    T.colour = a.frameColour;
    T.moments = a.momentsOut;
    T.batch = batch;
    for (int j = 0; j < batch && batch > 1; ++j)
        T.lerp.v[j] = makeFrameConsts(g.cam, w, h, g.spp, frameCount + j, testFlags, g.seedMode, g.config, g.animateSmoothing).lerpFac;
    T.valid = true;
    return 0;
}

// Second half: the progressive blend of the frame's colour into the accumulation tile (Test.cpp:293-295), in frame order
// on g.stream.  `frameRays` (host path): a per-slot ray count the kernel also adds to the context's running total.
int enqueueResolve(const TraceTicket& T, float* deviceTile, const unsigned long long* frameRays)
{
    if (!T.valid) return 0;
    if (T.pipelined) HIPCHK(hipStreamWaitEvent(g.stream, g.evTrace[T.slot], 0));
    if (T.batch > 1)
        HIPCHK(tptLaunchResolveBatch(deviceTile, T.colour, T.nPixels, T.nPixels, T.batch, T.lerp, g.mirror, g.dRays, g.mirrorCounter, g.stream));
    else
        HIPCHK(tptLaunchResolve(deviceTile, T.colour, T.nPixels, T.lerpFac, g.mirror, g.dRays, g.mirrorCounter, frameRays, g.stream));
    if (T.pipelined) {
        HIPCHK(hipEventRecord(g.evResolve[T.slot], g.stream));
        g.resolveRecorded[T.slot] = true;
    }
    return 0;
}


// What the draws beside the frame pipeline (tptDrawDeviceViews, tptDrawDeviceAov, tptDrawDeviceMoments, tptDrawDeviceAnimation) refuse,
// in the order they check it.  `fn`: the entry point; `things`: its output with the verb of the messages ("views are", "animation is").
// `own()`: the entry's own check, right behind the frame size (0 when it passes).  kQueueKernel: the configuration of the path-queue
// kernel (Views leave its spp limit to enqueueTrace; Animation needs none of it, it falls back to one launch per frame), kQueueSpp: its
// spp limit.
enum { kQueueKernel = 1, kQueueSpp = 2 };
template <typename Own>
static int checkPathQueueDraw(const char* fn, const char* things, int w, int h, unsigned checks, Own own)
{
    const std::string f(fn);
    if (!g.updated || w != g.updatedW || h != g.updatedH) return fail(f + ": call tptUpdate (UpdateTest) at this size first");
    if (w > 8192 || h > 8192) return fail(f + ": frames of at most 8192 x 8192");
    if (int rc = own()) return rc;
    if (checks & kQueueKernel) {
        if (g.seedMode == SEED_ROW_SERIAL) return fail(f + ": needs per-pixel seeds (tptSetSeedMode(1)); row-serial " + things + " not supported");
        if (g.foldMode != FOLD_RECURSIVE) return fail(f + ": needs the recursive fold (tptSetFoldMode(0))");
        if (g.persist != 3 || g.hs != HS_TWO_PHASE) return fail(f + ": needs the path-queue kernel (tptSetKernelVariant(0, 3, ..))");
    }
    if ((checks & kQueueSpp) && g.spp > 2047) return fail(f + ": at most 2047 samples per pixel (the path-queue kernel)");
    if (g.numParts > 1 || g.shard.active) return fail(f + ": not with row sharding or a communicator (sharded " + things + " not supported)");
    if (g.mirror) return fail(f + ": not with a tile mirror (tptSetTileMirror)");
    return 0;
}

// The blends of a launch whose frames count their rays apart (tptDrawDeviceViews, tptDrawDeviceAnimation), in frame order on the
// context's stream.  Frame j is blended into tiles + j * tileStep floats -- with the launch's lerp factor (views: n cameras of one frame)
// or, `ownLerp`, its own (the frames of an animation) -- and adds its rays to the running total; given `images`, the tile as it then
// stands is written to image j.  The per-frame counts go to `rays` first: the slot's counters are free again once its last blend has
// run (the next launch on this slot waits for that).  Given `moments` (tptDrawDeviceAnimationMoments), frame j's plane of the moments
// staging is blended into it right behind frame j's tile blend, with the same lerp factor (.w kept), and `momentImages`, if given,
// receives the plane as it then stands.
static int enqueuePlaneResolves(const TraceTicket& T, float* tiles, size_t tileStep, bool ownLerp, float* images, int64_t* rays,
                                float* moments = nullptr, float* momentImages = nullptr)
{
    const Context::ViewSlot& V = g.views[T.slot];
    if (T.pipelined) HIPCHK(hipStreamWaitEvent(g.stream, g.evTrace[T.slot], 0));
    if (rays) HIPCHK(hipMemcpyAsync(rays, V.rays, sizeof(unsigned long long) * (size_t)T.batch, hipMemcpyDeviceToDevice, g.stream));
    const size_t plane = (size_t)T.nPixels * 4;
    for (int j = 0; j < T.batch; ++j) {
        const TraceTicket P = T.plane(j);
        HIPCHK(tptLaunchResolve(tiles + (size_t)j * tileStep, P.colour, T.nPixels, ownLerp ? P.lerpFac : T.lerpFac,
                                images ? images + (size_t)j * plane : nullptr, g.dRays, nullptr, V.rays + j, g.stream));
        if (moments)
            HIPCHK(tptLaunchResolve(moments, T.moments + (size_t)j * (size_t)T.nPixels, T.nPixels, ownLerp ? P.lerpFac : T.lerpFac,
                                    momentImages ? momentImages + (size_t)j * plane : nullptr, g.dRays, nullptr, nullptr, g.stream));
    }
    if (T.pipelined) {
        HIPCHK(hipEventRecord(g.evResolve[T.slot], g.stream));
        g.resolveRecorded[T.slot] = true;
    }
    return 0;
}

// A view {lookFrom, lookAt, vfovDegrees, aperture, focusDist} as tptSetCamera stores it (vup (0, 1, 0)), and its camera exactly as
// tptSetCamera + tptUpdate at this size would build it (Test.cpp:309-319, 341).
static CameraSetup viewSetup(const float* p)
{
    CameraSetup cs = defaultCameraSetup(); // (vup (0, 1, 0))
    for (int i = 0; i < 3; ++i) {
        cs.lookFrom[i] = p[i];
        cs.lookAt[i] = p[3 + i];
    }
    cs.vfov = p[6];
    cs.aperture = p[7];
    cs.focusDist = p[8];
    return cs;
}
static CameraPOD viewCamera(CameraSetup cs, int w, int h)
{
    if (g.config & CFG_MITSUBA_COMPARE) cs.aperture = 0.0f; // Test.cpp:312-313
    return makeCamera(cs, float(w) / float(h));
}

// The launches and blends of tptDrawDeviceAnimation and, with `planes`, tptDrawDeviceAnimationMoments and tptDrawDeviceCameraClip, behind
// their checks: frames traced ahead are dropped, the camera is the one every tptUpdate of the sequence builds -- given `views`, frame j's
// own, as tptSetCamera(views[j]) before its tptUpdate leaves it (also written to outCameras[j], if given) --, then `perLaunch` frames per
// launch.  A launch of several frames with `views` takes both tables (tptCameraClipKernel); when nothing moves, its centres table repeats
// the scene's own centres of spheres 1 and 8: the kernel's exact tests read the same numbers from the table as from the scene.
// Given `keys` (tptDrawDeviceKeyframeClip, with `views` and `planes`, never with `animate`): the motion is the caller's -- frame j has sphere
// ids[k] at centres[(j * nMoved + k) * 3 ..].  A launch of several frames takes the cameras and a table of those centres
// (tptKeyframeKernel: TPT_Q_KEYS_MAX per frame in ascending sphere index, the spheres named by a mask); frame by frame the spheres are set
// and staged per frame.  Either way the context's spheres end at the launch's last frame and that scene is staged, as the animated path
// leaves it.  `objects`: a plane of first-hit sphere indices per frame (tptObjectPlaneKernel over the frame's own {centre, r^2} array,
// on the context stream).
struct ClipPlanes {
    float *moments, *frameAlbedo, *frameNormalDepth, *frameMoments; // (deviceMoments, and the per-frame outputs or null)
};
struct KeyMotion {
    int nMoved;
    const int32_t* ids;
    const float* centres;
    int32_t* objects; // (deviceFrameObjects or null)
};
// The {centre, r^2} arrays of one launch's frames (f .. f + n - 1 of the call) for the object planes, filled into the next half of the
// pinned twin and copied on the context stream (Context::dKeySph: two halves of `perLaunch` frames, whatever the call's length).  The
// spheres that stand still are the context's, which the call never moves; the moved ones take the frame's centres.  `hf`: the half taken.
static int uploadKeySpheres(int f, int n, int perLaunch, const KeyMotion& keys, int& hf)
{
    const size_t count = g.spheres.size(), half = sizeof(f4) * count * (size_t)perLaunch;
    for (int i = 0; i < 2; ++i)
        if (!g.evKeySph[i]) HIPCHK(hipEventCreateWithFlags(&g.evKeySph[i], kOrderingEvent));
    if (half > g.keySphBytes) {
        if (int rc = syncAllStreams()) return rc; // (an earlier call's object launches may still read the old arrays)
        (void)hipFree(g.dKeySph);
        if (g.hKeySph) (void)hipHostFree(g.hKeySph);
        g.dKeySph = g.hKeySph = nullptr;
        g.keySphBytes = 0;
        g.keySphCopied[0] = g.keySphCopied[1] = false;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dKeySph), 2 * half));
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&g.hKeySph), 2 * half, hipHostMallocDefault));
        g.keySphBytes = half;
    }
    hf = (int)(g.keySphSeq++ & 1u);
    if (g.keySphCopied[hf]) HIPCHK(hipEventSynchronize(g.evKeySph[hf])); // the half's previous copy has left the pinned twin
    f4* const host = g.hKeySph + (size_t)hf * (g.keySphBytes / sizeof(f4));
    for (int j = 0; j < n; ++j) {
        f4* sph = host + count * (size_t)j;
        for (size_t i = 0; i < count; ++i) sph[i] = f4{g.spheres[i].cx, g.spheres[i].cy, g.spheres[i].cz, g.spheres[i].radius * g.spheres[i].radius}; // (packScene's records)
        for (int k = 0; k < keys.nMoved; ++k) {
            const float* c = keys.centres + ((size_t)(f + j) * (size_t)keys.nMoved + (size_t)k) * 3;
            f4& v = sph[keys.ids[k]];
            v.x = c[0]; v.y = c[1]; v.z = c[2];
        }
    }
    HIPCHK(hipMemcpyAsync(g.dKeySph + (size_t)hf * (g.keySphBytes / sizeof(f4)), host, sizeof(f4) * count * (size_t)n, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipEventRecord(g.evKeySph[hf], g.stream));
    g.keySphCopied[hf] = true;
    return 0;
}
static int enqueueAnimation(int firstFrame, int nFrames, const float* times, int w, int h, float* deviceTile, float* deviceFrameImages,
                            int64_t* deviceFrameRays, unsigned testFlags, bool animate, int perLaunch, const ClipPlanes* planes,
                            const float* views = nullptr, CameraPOD* outCameras = nullptr, const KeyMotion* keys = nullptr)
{
    int rc = g.pending.discard();
    if (rc) return rc;
    // tptDrawDeviceKeyframeClip: the moved spheres as a mask and each one's place in a frame's table, the number of moved spheres below it
    unsigned long long keyMask = 0;
    int keySlot[TPT_Q_KEYS_MAX] = {};
    if (keys && perLaunch > 1) {
        for (int k = 0; k < keys->nMoved; ++k) keyMask |= 1ull << (63 - keys->ids[k]);
        for (int k = 0; k < keys->nMoved; ++k)
            for (int m = 0; m < keys->nMoved; ++m) keySlot[k] += keys->ids[m] < keys->ids[k] ? 1 : 0;
    }
    // the camera as every tptUpdate of the sequence builds it (Test.cpp:309-313, 341)
    g.cam = viewCamera(g.camSetup, w, h);
    if (views) g.configEpoch++; // (as every tptSetCamera of the sequence)
    for (int f = 0; f < nFrames; f += perLaunch) {
        const int n = nFrames - f < perLaunch ? nFrames - f : perLaunch;
        BatchTable table;
        f4 centres[2 * kMaxBatch];
        f4 keyCentres[TPT_Q_KEYS_MAX * kMaxBatch];
        CameraPOD cams[kMaxBatch];
        if (views) {
            // each frame's camera; the context's camera ends at the launch's last view
            for (int j = 0; j < n; ++j) {
                g.camSetup = viewSetup(views + 9 * (size_t)(f + j));
                cams[j] = viewCamera(g.camSetup, w, h);
                if (outCameras) outCameras[f + j] = cams[j];
            }
            g.cam = cams[n - 1];
            if (perLaunch > 1) {
                table.cams = cams;
                if (keys) { // the caller's centres of the launch's frames
                    memset(keyCentres, 0, sizeof keyCentres);
                    for (int j = 0; j < n; ++j)
                        for (int k = 0; k < keys->nMoved; ++k) {
                            const float* c = keys->centres + ((size_t)(f + j) * (size_t)keys->nMoved + (size_t)k) * 3;
                            keyCentres[TPT_Q_KEYS_MAX * j + keySlot[k]] = f4{c[0], c[1], c[2], 0.0f};
                        }
                    table.keyCentres = keyCentres;
                    table.keyMask = keyMask;
                    table.keyCount = keys->nMoved;
                } else if (!animate) { // nothing moves: every frame's centres are the scene's own
                    const SpherePOD s1 = g.spheres[1], s8 = g.spheres[8];
                    for (int j = 0; j < n; ++j) {
                        centres[2 * j] = f4{s1.cx, s1.cy, s1.cz, 0.0f};
                        centres[2 * j + 1] = f4{s8.cx, s8.cy, s8.cz, 0.0f};
                    }
                    table.centres = centres;
                }
            }
        }
        if (animate) {
            // each frame's centres of spheres 1 and 8 exactly as tptUpdate moves them (a non-finite time touches its own frame only); the
            // context's spheres end at the batch's last time
            const SpherePOD s1 = g.spheres[1], s8 = g.spheres[8];
            for (int j = 0; j < n; ++j) {
                const float t = times[f + j];
                centres[2 * j] = f4{s1.cx, animatedY1(t), s1.cz, 0.0f};
                centres[2 * j + 1] = f4{s8.cx, s8.cy, animatedZ8(t), 0.0f};
            }
            g.spheres[1].cy = centres[2 * (n - 1)].y;
            g.spheres[8].cz = centres[2 * (n - 1) + 1].z;
            // the staged scene is the batch's last frame: exact for the spheres that do not move, and the animation kernel reads spheres
            // 1 and 8 from the table and tests them for every ray (tpt_trace.h, movedSphere)
            if (perLaunch > 1) table.centres = centres;
            if ((rc = stageScene())) return rc;
        }
        if (keys && keys->nMoved > 0) {
            // the context's spheres at the launch's last frame (frame by frame: at the frame), that scene staged: exact for the spheres that
            // stand still, and the keyframe kernel reads the moved ones from the table and tests them for every ray (tpt_trace.h, keyedSphere)
            for (int k = 0; k < keys->nMoved; ++k) {
                const float* c = keys->centres + ((size_t)(f + n - 1) * (size_t)keys->nMoved + (size_t)k) * 3;
                SpherePOD& sp = g.spheres[keys->ids[k]];
                sp.cx = c[0]; sp.cy = c[1]; sp.cz = c[2];
            }
            if ((rc = stageScene())) return rc;
        }
        TraceTicket T;
        AovPlanes aov; // (the launch's frames' planes in the caller's per-frame buffers)
        const size_t at = (size_t)f * (size_t)h * (size_t)w * 4;
        if (planes) {
            aov.albedo = planes->frameAlbedo ? reinterpret_cast<f4*>(planes->frameAlbedo + at) : nullptr;
            aov.normalDepth = planes->frameNormalDepth ? reinterpret_cast<f4*>(planes->frameNormalDepth + at) : nullptr;
            aov.moments = true;
            aov.continues = f > 0;
        }
        if ((rc = enqueueTrace(firstFrame + f, w, h, testFlags, nullptr, T, n, 1, &table, planes ? &aov : nullptr))) return rc;
        if (keys && keys->objects) { // the launch's frames' object planes, on the context stream in front of their blends
            const size_t count = g.spheres.size();
            int hf = 0;
            if ((rc = uploadKeySpheres(f, n, perLaunch, *keys, hf))) return rc;
            const size_t at0 = (size_t)hf * (g.keySphBytes / sizeof(f4));
            for (int j = 0; j < n; ++j) {
                const f4* host = g.hKeySph + at0 + count * (size_t)j;
                tptObjectPlaneConsts k = {};
                float c[12];
                memcpy(c, &cams[j], sizeof c);
                memcpy(k.o, c, 12); memcpy(k.ll, c + 3, 12); memcpy(k.H, c + 6, 12); memcpy(k.V, c + 9, 12);
                if (count > 1) { k.c1[0] = host[1].x; k.c1[1] = host[1].y; k.c1[2] = host[1].z; }
                if (count > 8) { k.c8[0] = host[8].x; k.c8[1] = host[8].y; k.c8[2] = host[8].z; }
                HIPCHK(tptLaunchObjectPlane(g.dKeySph + at0 + count * (size_t)j, (int)count, keys->objects + (size_t)(f + j) * (size_t)w * (size_t)h, w, h, k, g.stream));
            }
        }
        // the blends, in frame order, each into the one tile with its frame's lerp factor (and the frame's moments behind it)
        if (T.valid && (rc = enqueuePlaneResolves(T, deviceTile, 0, true, deviceFrameImages ? deviceFrameImages + at : nullptr,
                                                  deviceFrameRays ? deviceFrameRays + f : nullptr, planes ? planes->moments : nullptr,
                                                  planes && planes->frameMoments ? planes->frameMoments + at : nullptr)))
            return rc;
    }
    return 0;
}

// What tptDrawDeviceAnimationMoments and (`cameras`: a view per frame) tptDrawDeviceCameraClip share: the checks, in one order and with
// the entry point's name, then enqueueAnimation with the planes.  A refused call has touched nothing.  `keys` (tptDrawDeviceKeyframeClip,
// with `cameras`): the caller's motion in the place of `times`, its own checks behind the shared ones, and an eighth buffer, the object planes.
static int drawClip(const char* name, int firstFrame, int nFrames, const float* times, bool cameras, const float* views, int w, int h,
                    float* deviceTile, const ClipPlanes& planes, float* deviceFrameImages, int64_t* deviceFrameRays, CameraPOD* outCameras,
                    unsigned testFlags, const KeyMotion* keys = nullptr)
{
    const std::string fn = name;
    float* const deviceMoments = planes.moments;
    if (int rc_ = flushShardDeferred()) return rc_; // (see tptDrawDevice)
    if (requireInit()) return -1;
    if (nFrames < 1) return fail(fn + ": nFrames must be at least 1");
    if ((!keys && !times) || (cameras && !views) || !deviceTile || !deviceMoments || w <= 0 || h <= 0)
        return fail(fn + (keys ? ": bad arguments (views, deviceTile, deviceMoments, size)"
                               : (cameras ? ": bad arguments (times, views, deviceTile, deviceMoments, size)" : ": bad arguments (times, deviceTile, deviceMoments, size)")));
    if (keys) {
        if (keys->nMoved < 0) return fail(fn + ": nMoved must not be negative");
        if (keys->nMoved > 0 && (!keys->ids || !keys->centres)) return fail(fn + ": movedIds and centres are required with nMoved > 0");
        if (testFlags & ~(unsigned)TPT_FLAG_PROGRESSIVE)
            return fail(fn + ": TPT_FLAG_PROGRESSIVE is the only flag (the centres are the motion: TPT_FLAG_ANIMATE is not applied on top of them)");
    }
    const bool animate = !keys && (testFlags & TPT_FLAG_ANIMATE) && g.spheres.size() > 8; // (the tptUpdate guard, Test.cpp:304)
    // one launch per kMaxBatch frames on a flat scene: while it moves, or -- with a camera per frame, where the kernel takes a centres
    // table anyway -- whenever it has the two spheres the table is about; with the caller's motion, when the table holds it: at most
    // TPT_Q_KEYS_MAX moved spheres, all among the first 64 (the candidate mask of the filters' first chunk)
    const bool flat = g.spheres.size() < TPT_GROUP_MIN_SPHERES;
    int perLaunch = flat && (animate || (cameras && g.spheres.size() > 8)) ? kMaxBatch : 1;
    if (keys) {
        perLaunch = flat && keys->nMoved <= TPT_Q_KEYS_MAX ? kMaxBatch : 1;
        for (int k = 0; k < keys->nMoved && k < TPT_Q_KEYS_MAX; ++k)
            if (keys->ids[k] < 0 || keys->ids[k] >= 64) perLaunch = 1; // (an id outside the scene is refused below)
    }
    int rc = checkPathQueueDraw(fn.c_str(), "clip planes are", w, h, kQueueKernel | kQueueSpp, [&] {
        const size_t plane = (size_t)h * (size_t)w * sizeof(f4), staged = 2 * plane * (size_t)(nFrames < perLaunch ? nFrames : perLaunch);
        if (staged > (4ull << 30))
            return refuse(fn + ": " + std::to_string(staged >> 20) + " MiB of frame colour and moments per launch: over the 4096 MiB limit");
        if (g.spheres.size() > 65534) return fail(fn + ": at most 65534 spheres (the path-queue kernel)");
        if (keys) {
            const int count = (int)g.spheres.size();
            if (keys->nMoved > count) return fail(fn + ": nMoved is larger than the sphere count");
            std::vector<bool> seen((size_t)count, false);
            for (int k = 0; k < keys->nMoved; ++k) {
                if (keys->ids[k] < 0 || keys->ids[k] >= count) return fail(fn + ": a moved id lies outside 0 .. count - 1");
                if (seen[(size_t)keys->ids[k]]) return fail(fn + ": a moved id is repeated");
                seen[(size_t)keys->ids[k]] = true;
            }
            for (size_t i = 0; i < (size_t)nFrames * (size_t)keys->nMoved * 3; ++i)
                if (!(fabsf(keys->centres[i]) <= 3.40282347e38f)) return fail(fn + ": a centre is not finite");
            // the object planes are tptObjectPlaneDevice's over the call's cameras, and so is what it refuses of a camera
            for (int j = 0; keys->objects && j < nFrames; ++j) {
                const CameraPOD cam = viewCamera(viewSetup(views + 9 * (size_t)j), w, h);
                float c[12];
                memcpy(c, &cam, sizeof c);
                for (int i = 0; i < 12; ++i)
                    if (!(fabsf(c[i]) <= 3.40282347e38f))
                        return fail(fn + ": deviceFrameObjects with a view whose camera has a non-finite origin, lowerLeftCorner, horizontal or vertical");
            }
        }
        // the seven buffers (with the caller's motion eight: the object planes), each at its full extent: no two may share a byte
        const struct { const void* p; size_t bytes; } bufs[8] = {
            {deviceTile, plane}, {deviceMoments, plane}, {deviceFrameImages, plane * (size_t)nFrames}, {planes.frameAlbedo, plane * (size_t)nFrames},
            {planes.frameNormalDepth, plane * (size_t)nFrames}, {planes.frameMoments, plane * (size_t)nFrames},
            {deviceFrameRays, sizeof(int64_t) * (size_t)nFrames},
            {keys ? keys->objects : nullptr, sizeof(int32_t) * (size_t)h * (size_t)w * (size_t)nFrames}};
        for (int i = 0; i < 8; ++i)
            for (int k = i + 1; k < 8; ++k) {
                const uintptr_t a = reinterpret_cast<uintptr_t>(bufs[i].p), b = reinterpret_cast<uintptr_t>(bufs[k].p);
                if (a && b && a < b + bufs[k].bytes && b < a + bufs[i].bytes) return fail(fn + ": two of the tile, moments and per-frame buffers overlap");
            }
        return 0;
    });
    if (rc) return rc;
    if (keys && keys->objects && !tptLaunchObjectPlane) return fail(fn + ": this build has no object plane kernel");
    return enqueueAnimation(firstFrame, nFrames, times, w, h, deviceTile, deviceFrameImages, deviceFrameRays, testFlags, animate, perLaunch, &planes,
                            views, outCameras, keys);
}

} // namespace tpth

extern "C" {

int tptDrawDevice(float time, int frameCount, int w, int h, float* deviceTile, unsigned testFlags)
{
    (void)time; // stored but never read by the reference either (Test.cpp:257,347)
    // (a host that mixes sharded and plain frames on one context: sharded frames accepted earlier go out first, in call order.  The
    //  sharded path itself comes through here with nothing pending.)
    if (int rc_ = flushShardDeferred()) return rc_;
    if (requireInit()) return -1;
    if (!g.updated) return fail("tptDrawDevice: call tptUpdate (UpdateTest) first");
    if (!deviceTile || w <= 0 || h <= 0) return fail("tptDrawDevice: bad arguments");
    // A caller that waits for every frame before it asks for the next (the reference's DrawTest contract, on a device tile)
    // would leave each frame alone on the GPU, bound by its longest paths: 0.98 ms per C2 frame against 0.45 in a stream.
    // Such a caller shows: when its call arrives, the previous frame's blend has already completed.  After two such calls
    // for consecutive frames of one configuration the next frames are traced ahead of it, exactly as tptDraw does for the
    // host-pointer path (same bookkeeping, same per-slot ray counters; a wrong guess costs GPU time only).  A caller that
    // streams frames never meets the condition and takes the plain path below.
    Context::DeviceCaller& D = g.devCaller;
    const unsigned long long key = g.configEpoch;
    const bool pipelined = effectiveOverlap() > 1;
    const bool stable = !g.sceneDirty && g.pendingSet < 0 && !(testFlags & TPT_FLAG_ANIMATE);
    bool prevDone = false;
    if (D.lastSlot >= 0 && g.resolveRecorded[D.lastSlot]) {
        prevDone = hipEventQuery(g.evResolve[D.lastSlot]) == hipSuccess;
        (void)hipGetLastError();
    }
    D.syncStreak = prevDone ? D.syncStreak + 1 : 0;
    const int seqStreak = D.seq.next(frameCount, w, h, testFlags, key);
    const bool lookAhead = pipelined && stable && !g.mirror && g.lookahead > 0 && D.syncStreak >= 2 && seqStreak >= 2;

    LaunchQueue& Q = g.pending;
    TraceTicket T;
    const unsigned long long* rays = nullptr;
    int rc;
    const bool hit = stable && !g.mirror && Q.frontMatches(PendingLaunch::AHEAD, frameCount, w, h, testFlags, key);
    if (!hit && !lookAhead) {
        // ---- a streaming caller.  With SMALL frames (tiles of a sharded frame, 640x360) a launch cannot be shorter than its longest
        //      pixel's sequential samples, so frame by frame such a caller is bound by launch latency, not by arithmetic.  When the
        //      calls are consecutive frames of one static configuration, the next calls' frames are traced in the SAME launch (a
        //      STREAM batch of 2-8 frames, tptDrawDeviceBatch's kernel path, a ray counter per frame) and each later call only blends
        //      its own plane -- every frame is still delivered, in order, with its own ray count.  A wrong guess costs GPU time only.
        //      (No !g.mirror here: the sharded path mirrors its tile.)
        if (stable && Q.frontMatches(PendingLaunch::STREAM, frameCount, w, h, testFlags, key)) {
            Q.serveFront(true, T, rays);
        } else {
            // (a batch used up by the previous call, continued by this one: the stream goes on, and its batches may grow)
            const bool continues = Q.empty() && seqStreak >= 2 && frameCount == g.streamNext;
            if ((rc = Q.discard())) return rc; // (also closes a stream batch that did not continue as guessed)
            g.streamNext = -1;
            int nBatch = 1;
            if (g.streamBatch && pipelined && stable && seqStreak >= 2 && pathQueueTakesScene() && w <= 8192 && h <= 8192) {
                // how many frames make a launch long enough to amortise its fixed cost at this pipeline depth (tpt_stream_batch.h)
                g.streamRun = continues ? g.streamRun + 1 : 0;
                nBatch = streamBatchFrames((long long)localRows(h) * w * g.spp, effectiveOverlap(), Context::kMaxOverlap, g.streamRun,
                                           (long long)localRows(h) * w * (long long)sizeof(f4), Context::kStreamBatchMax);
            }
            if (nBatch > 1) {
                PendingLaunch S;
                S.kind = PendingLaunch::STREAM;
                S.firstFrame = frameCount; S.w = w; S.h = h; S.flags = testFlags; S.key = key;
                S.rays = g.dRaysStream + (g.streamBatches % (unsigned long long)Context::kStreamRing) * Context::kStreamBatchMax;
                rc = enqueueTrace(frameCount, w, h, testFlags, S.rays, S.T, nBatch, 1);
                if (rc == kRefused && localRows(h) * (long long)w * g.spp >= kStreamLaunchSamples) {
                    nBatch = 1; // (a large frame's batch the device has no memory for: this frame alone, as without batching)
                } else if (rc) {
                    return rc;
                } else if (S.T.valid) {
                    g.lastStreamRays = S.rays;
                    g.lastStreamFrames = nBatch;
                    g.streamBatches++;
                    g.streamNext = frameCount + nBatch;
                    if ((rc = Q.push(S))) return rc;
                    Q.serveFront(false, T, rays);
                }
            }
            if (nBatch == 1 && (rc = enqueueTrace(frameCount, w, h, testFlags, nullptr, T)))
                return rc; // (the plain path: the kernel adds its rays to the running total itself)
        }
        rc = enqueueResolve(T, deviceTile, rays);
        if (T.valid) D.lastSlot = T.slot;
        return rc;
    }
    // one frame more than the host-pointer path looks ahead: there the PCIe copies fill the caller's time (2 ahead: 0.88 ms
    // per frame, 3: 0.92), here nothing does (2: 0.598 ms, 3: 0.561; profiles/r02/r02_run50.log)
    const int devAhead = g.lookahead + 1 < 3 ? g.lookahead + 1 : 3;
    DepthScope depthScope(1 + devAhead);
    if (hit) {
        Q.serveFront(true, T, rays);
    } else {
        if ((rc = Q.discard())) return rc;
        unsigned long long* own = g.dRaysAhead + g.frameSeq % (unsigned long long)Context::kMaxSlots;
        if ((rc = enqueueTrace(frameCount, w, h, testFlags, own, T))) return rc;
        rays = T.valid ? own : nullptr;
    }
    if (lookAhead && T.valid && (rc = traceAhead(frameCount, w, h, testFlags, key, devAhead))) return rc;
    rc = enqueueResolve(T, deviceTile, rays);
    if (T.valid) D.lastSlot = T.slot;
    return rc;
}

// nFrames consecutive frames (frameCount = firstFrame ... firstFrame + nFrames - 1) of the scene and camera as of the last
// tptUpdate, traced by ONE launch and blended in frame order by one: the same bits as nFrames tptDrawDevice calls.
int tptDrawDeviceBatch(float time, int firstFrame, int nFrames, int w, int h, float* deviceTile, unsigned testFlags)
{
    (void)time;
    if (int rc_ = flushShardDeferred()) return rc_; // (see tptDrawDevice)
    if (requireInit()) return -1;
    if (!g.updated) return fail("tptDrawDeviceBatch: call tptUpdate (UpdateTest) first");
    if (!deviceTile || w <= 0 || h <= 0 || nFrames < 1) return fail("tptDrawDeviceBatch: bad arguments");
    if (nFrames > 1 && (testFlags & TPT_FLAG_ANIMATE))
        return fail("tptDrawDeviceBatch: an animated scene changes every frame (Test.cpp:304-308): one tptUpdate + tptDrawDevice per frame");
    int rc = g.pending.discard();
    if (rc) return rc;
    for (int f = 0; f < nFrames; f += kMaxBatch) {
        const int n = nFrames - f < kMaxBatch ? nFrames - f : kMaxBatch;
        TraceTicket T;
        if ((rc = enqueueTrace(firstFrame + f, w, h, testFlags, nullptr, T, n))) return rc;
        if ((rc = enqueueResolve(T, deviceTile, nullptr))) return rc;
    }
    return 0;
}

// nViews cameras of the scene as of the last tptUpdate, traced by ONE launch (the frames of a batch, a camera each, the seeds of
// frameCount for all), each view blended into its own tile: the same bits and ray counts as nViews tptSetCamera / tptUpdate /
// tptDrawDevice sequences.  Not a continuation of anything: frames traced ahead and stream-batch planes are dropped, the caller's
// camera and the bookkeeping of later tptDrawDevice calls are left as they were.
int tptDrawDeviceViews(float time, int frameCount, int w, int h, int nViews, const float* views, float* deviceTiles, int64_t* deviceViewRays,
                       unsigned testFlags)
{
    (void)time; // (the scene state is that of the last tptUpdate, as for tptDrawDevice)
    if (int rc_ = flushShardDeferred()) return rc_; // (see tptDrawDevice)
    if (requireInit()) return -1;
    if (nViews < 1 || nViews > kMaxBatch) return fail("tptDrawDeviceViews: nViews must be 1.." + std::to_string(kMaxBatch));
    if (!views || !deviceTiles || w <= 0 || h <= 0) return fail("tptDrawDeviceViews: bad arguments (views, deviceTiles, size)");
    int rc = checkPathQueueDraw("tptDrawDeviceViews", "views are", w, h, kQueueKernel, [&] {
        const size_t colour = (size_t)h * (size_t)w * sizeof(f4) * (size_t)nViews;
        return colour > (4ull << 30) ? refuse("tptDrawDeviceViews: " + std::to_string(colour >> 20) + " MiB of view colour per launch: over the 4096 MiB limit, use fewer views") : 0;
    });
    if (rc) return rc;
    // the cameras exactly as tptSetCamera + tptUpdate at this size would build them (Test.cpp:309-319, 341)
    CameraPOD cams[kMaxBatch];
    for (int v = 0; v < nViews; ++v) cams[v] = viewCamera(viewSetup(views + 9 * v), w, h);
    if ((rc = g.pending.discard())) return rc;
    // one launch: the views are the frames of a batch (colour planes nPixels apart in the slot's buffer, a ray counter each)
    TraceTicket T;
    BatchTable table;
    table.cams = cams;
    if ((rc = enqueueTrace(frameCount, w, h, testFlags, nullptr, T, nViews, 1, &table))) return rc;
    // the blends, in view order, each into its own tile with the frame's lerp factor
    return T.valid ? enqueuePlaneResolves(T, deviceTiles, (size_t)T.nPixels * 4, false, nullptr, deviceViewRays) : 0;
}

// nFrames frames of the scene as tptUpdate(times[j], firstFrame + j, ...) animates it, each followed by tptDrawDevice: the same bits,
// the same ray counts.  Up to kMaxBatch frames per launch (tptTraceAnimationKernel: each frame's centres of the two moving spheres in
// a table and tested for every ray; on a static scene the batched kernel), blended in
// frame order one frame at a time, each blend also writing the tile as it stands to the frame's image.  Configurations the batched
// kernels do not serve take one launch per frame.  Like tptDrawDeviceViews, not a continuation of anything: frames traced ahead and
// stream-batch planes are dropped; unlike it, the context is left as the sequence leaves it (spheres, staged scene, camera).
int tptDrawDeviceAnimation(int firstFrame, int nFrames, const float* times, int w, int h, float* deviceTile, float* deviceFrameImages,
                           int64_t* deviceFrameRays, unsigned testFlags)
{
    if (int rc_ = flushShardDeferred()) return rc_; // (see tptDrawDevice)
    if (requireInit()) return -1;
    if (nFrames < 1) return fail("tptDrawDeviceAnimation: nFrames must be at least 1");
    if (!times || !deviceTile || w <= 0 || h <= 0) return fail("tptDrawDeviceAnimation: bad arguments (times, deviceTile, size)");
    // (the tptUpdate guard, Test.cpp:304: a scene of 8 spheres or fewer does not move)
    const bool animate = (testFlags & TPT_FLAG_ANIMATE) && g.spheres.size() > 8;
    // one launch per kMaxBatch frames on the path-queue kernel; the animation kernel also wants a flat scene (its exact tests are
    // those of the flat filters); everything else: one launch per frame, the kernels of tptDrawDevice
    if (g.updated && (g.sceneDirty || !activeSet())) { // (tptSetScene after the last tptUpdate: what is staged decides the launches below)
        if (int rc_ = stageScene()) return rc_;
    }
    const int perLaunch = pathQueueTakesScene() && (!animate || g.spheres.size() < TPT_GROUP_MIN_SPHERES) ? kMaxBatch : 1;
    int rc = checkPathQueueDraw("tptDrawDeviceAnimation", "animation is", w, h, 0, [&] {
        const size_t colour = (size_t)h * (size_t)w * sizeof(f4) * (size_t)(nFrames < perLaunch ? nFrames : perLaunch);
        return colour > (4ull << 30) ? refuse("tptDrawDeviceAnimation: " + std::to_string(colour >> 20) + " MiB of frame colour per launch: over the 4096 MiB limit") : 0;
    });
    if (rc) return rc;
    return enqueueAnimation(firstFrame, nFrames, times, w, h, deviceTile, deviceFrameImages, deviceFrameRays, testFlags, animate, perLaunch, nullptr);
}

// nFrames frames of the scene as tptUpdate(times[j], firstFrame + j, ...) animates it, each followed by tptDrawDeviceMoments into the
// frame's own albedo and normal / depth planes: the same bits, the same ray counts.  tptDrawDeviceAnimation's loop with the planes
// beside the centres table: up to kMaxBatch frames per launch (tptTraceClipKernel) while the scene moves and is flat; a scene that does
// not move, or a grouped one, goes frame by frame through the single-frame moments kernel.  The moments of a launch's frames are staged in
// Context::dMoments, a plane per frame, and blended into deviceMoments behind each frame's tile blend.
int tptDrawDeviceAnimationMoments(int firstFrame, int nFrames, const float* times, int w, int h, float* deviceTile, float* deviceMoments,
                                  float* deviceFrameImages, float* deviceFrameAlbedo, float* deviceFrameNormalDepth, float* deviceFrameMoments,
                                  int64_t* deviceFrameRays, unsigned testFlags)
{
    const ClipPlanes planes{deviceMoments, deviceFrameAlbedo, deviceFrameNormalDepth, deviceFrameMoments};
    return drawClip("tptDrawDeviceAnimationMoments", firstFrame, nFrames, times, false, nullptr, w, h, deviceTile, planes, deviceFrameImages,
                    deviceFrameRays, nullptr, testFlags);
}

// tptDrawDeviceAnimationMoments with a camera per frame: frame j as tptSetCamera(views[j]), tptUpdate(times[j], firstFrame + j, ...) and
// tptDrawDeviceMoments trace it -- the same bits, the same ray counts --, its Camera record written to outCameras[j] at call time.  Up to
// kMaxBatch frames per launch (tptCameraClipKernel: the cameras beside the centres table) on a flat scene of more than 8 spheres, whether
// it moves or not; smaller and grouped scenes go frame by frame through the single-frame moments kernel with the camera set per frame.
// The context is left as the sequence leaves it: the camera set-up of the last view, the spheres at the last time.
int tptDrawDeviceCameraClip(int firstFrame, int nFrames, const float* times, const float* views, int w, int h, float* deviceTile,
                            float* deviceMoments, float* deviceFrameImages, float* deviceFrameAlbedo, float* deviceFrameNormalDepth,
                            float* deviceFrameMoments, int64_t* deviceFrameRays, void* outCameras, unsigned testFlags)
{
    const ClipPlanes planes{deviceMoments, deviceFrameAlbedo, deviceFrameNormalDepth, deviceFrameMoments};
    return drawClip("tptDrawDeviceCameraClip", firstFrame, nFrames, times, true, views, w, h, deviceTile, planes, deviceFrameImages,
                    deviceFrameRays, static_cast<CameraPOD*>(outCameras), testFlags);
}

// tptDrawDeviceCameraClip with the motion given by the CALLER: frame j as tptSetScene(S_j), tptSetCamera(views[j]), tptUpdate(0, firstFrame
// + j, ...) and tptDrawDeviceMoments trace it -- the same bits, the same ray counts --, S_j the context's spheres with the centres of
// movedIds replaced by frame j's.  Up to kMaxBatch frames per launch (tptKeyframeKernel: the cameras beside a table of the moved centres,
// the moved spheres named by a mask and tested for every ray) on a flat scene with at most TPT_Q_KEYS_MAX moved spheres among the first
// 64; everything else goes frame by frame through the single-frame moments kernel with the spheres and the camera set per frame.  The
// object planes are tptObjectPlaneKernel's over one {centre, r^2} array per frame.  The context is left as the sequence leaves it.
int tptDrawDeviceKeyframeClip(int firstFrame, int nFrames, const float* views, int nMoved, const int32_t* movedIds, const float* centres, int w,
                              int h, float* deviceTile, float* deviceMoments, float* deviceFrameImages, float* deviceFrameAlbedo,
                              float* deviceFrameNormalDepth, float* deviceFrameMoments, int64_t* deviceFrameRays, int32_t* deviceFrameObjects,
                              void* outCameras, unsigned testFlags)
{
    const ClipPlanes planes{deviceMoments, deviceFrameAlbedo, deviceFrameNormalDepth, deviceFrameMoments};
    const KeyMotion keys{nMoved, movedIds, centres, deviceFrameObjects};
    return drawClip("tptDrawDeviceKeyframeClip", firstFrame, nFrames, nullptr, true, views, w, h, deviceTile, planes, deviceFrameImages,
                    deviceFrameRays, static_cast<CameraPOD*>(outCameras), testFlags, &keys);
}

// One frame blended into the tile exactly as tptDrawDevice blends it (same bits, same ray count), plus the first-hit planes of its
// samples: albedo and coverage, normal and t, averaged over the samples (tptTraceAovKernel).  The planes are overwritten, not blended, and
// are ordered on the context stream like the tile.  Like tptDrawDeviceViews, not a continuation of anything: frames traced ahead and
// stream-batch planes are dropped; the camera and the scene are left as they were.
int tptDrawDeviceAov(float time, int frameCount, int w, int h, float* deviceTile, float* deviceAlbedo, float* deviceNormalDepth, unsigned testFlags)
{
    (void)time; // (the scene state is that of the last tptUpdate, as for tptDrawDevice)
    if (int rc_ = flushShardDeferred()) return rc_; // (see tptDrawDevice)
    if (requireInit()) return -1;
    if (!deviceTile || (!deviceAlbedo && !deviceNormalDepth) || w <= 0 || h <= 0)
        return fail("tptDrawDeviceAov: bad arguments (deviceTile, at least one of deviceAlbedo / deviceNormalDepth, size)");
    int rc = checkPathQueueDraw("tptDrawDeviceAov", "planes are", w, h, kQueueKernel | kQueueSpp, [] { return 0; });
    if (rc || (rc = g.pending.discard())) return rc;
    TraceTicket T;
    AovPlanes aov;
    aov.albedo = reinterpret_cast<f4*>(deviceAlbedo);
    aov.normalDepth = reinterpret_cast<f4*>(deviceNormalDepth);
    if ((rc = enqueueTrace(frameCount, w, h, testFlags, nullptr, T, 1, 0, nullptr, &aov))) return rc;
    return enqueueResolve(T, deviceTile, nullptr); // (the kernel added its rays to the running total itself, as tptDrawDevice's plain path)
}

// tptDrawDeviceAov plus the luminance moments of the frame's samples (tptTraceMomentsKernel into the context's moments plane), blended
// into deviceMoments by a second resolve launch right behind the tile's, with the tile's lerp factor.  The next moments launch waits
// for the context stream (evAov) before it overwrites the plane, so one plane serves every call.
int tptDrawDeviceMoments(float time, int frameCount, int w, int h, float* deviceTile, float* deviceAlbedo, float* deviceNormalDepth,
                         float* deviceMoments, unsigned testFlags)
{
    (void)time; // (the scene state is that of the last tptUpdate, as for tptDrawDevice)
    if (int rc_ = flushShardDeferred()) return rc_; // (see tptDrawDevice)
    if (requireInit()) return -1;
    if (!deviceTile || !deviceMoments || w <= 0 || h <= 0)
        return fail("tptDrawDeviceMoments: bad arguments (deviceTile, deviceMoments, size)");
    int rc = checkPathQueueDraw("tptDrawDeviceMoments", "moments are", w, h, kQueueKernel | kQueueSpp, [&] {
        return overlapsAny(deviceMoments, {deviceTile, deviceAlbedo, deviceNormalDepth}, (uintptr_t)w * (uintptr_t)h * 16u)
                   ? fail("tptDrawDeviceMoments: deviceMoments overlaps the tile or a plane") : 0;
    });
    if (rc || (rc = g.pending.discard())) return rc;
    TraceTicket T;
    AovPlanes aov;
    aov.albedo = reinterpret_cast<f4*>(deviceAlbedo);
    aov.normalDepth = reinterpret_cast<f4*>(deviceNormalDepth);
    aov.moments = true;
    if ((rc = enqueueTrace(frameCount, w, h, testFlags, nullptr, T, 1, 0, nullptr, &aov))) return rc;
    if ((rc = enqueueResolve(T, deviceTile, nullptr))) return rc;
    if (!T.valid) return 0;
    // (behind the tile's blend, so behind the trace; .xyz blended, .w kept; no ray count: the tile's blend has taken it)
    HIPCHK(tptLaunchResolve(deviceMoments, g.dMoments, T.nPixels, T.lerpFac, nullptr, g.dRays, nullptr, nullptr, g.stream));
    return 0;
}

// nFrames tptDrawDeviceMoments calls on the scene and camera of the last tptUpdate, the guide planes averaged as the tile is: the same
// bits, the same ray counts (include/tpt_hip.h states the sequence).  On a flat scene of more than 8 spheres the camera-clip path traces
// up to kMaxBatch frames per launch -- the camera table repeats the context's camera, the centres table the scene's own centres, so the
// kernel reads the numbers tptTraceMomentsKernel reads --; every other scene takes tptDrawDeviceMoments' kernel, a frame per launch.
// Either way the frames' colour (the slot's buffer), moments (Context::dMoments) and guide planes (Context::dGuideStage) are staged a
// plane per frame, and ONE launch of the fold kernel behind each trace launch blends them into the caller's four planes; the launches of
// a call alternate between the halves of the staging as tptDrawDeviceAnimationMoments' do (Context::evClip).
int tptDrawDeviceBatchMoments(float time, int firstFrame, int nFrames, int w, int h, float* deviceTile, float* deviceMoments,
                              float* deviceAlbedo, float* deviceNormalDepth, unsigned testFlags)
{
    (void)time; // (the scene state is that of the last tptUpdate, as for tptDrawDevice)
    const std::string fn = "tptDrawDeviceBatchMoments";
    if (int rc_ = flushShardDeferred()) return rc_; // (see tptDrawDevice)
    if (requireInit()) return -1;
    if (nFrames < 1) return fail(fn + ": nFrames must be at least 1");
    if (firstFrame < 0 || firstFrame > 0x7fffffff - (nFrames - 1)) return fail(fn + ": firstFrame .. firstFrame + nFrames - 1 must be frame numbers 0 .. 2^31 - 1");
    if (!deviceTile || !deviceMoments || w <= 0 || h <= 0) return fail(fn + ": bad arguments (deviceTile, deviceMoments, size)");
    if (testFlags & ~(unsigned)TPT_FLAG_PROGRESSIVE)
        return fail(fn + ": TPT_FLAG_PROGRESSIVE is the only flag (nothing moves between the frames: TPT_FLAG_ANIMATE belongs to tptDrawDeviceAnimationMoments)");
    int rc = checkPathQueueDraw(fn.c_str(), "moments are", w, h, kQueueKernel | kQueueSpp, [&] {
        const void* const planes[4] = {deviceTile, deviceMoments, deviceAlbedo, deviceNormalDepth};
        for (int i = 0; i < 4; ++i)
            for (int k = i + 1; k < 4; ++k)
                if (planes[i] && overlapsAny(planes[i], {planes[k]}, (uintptr_t)w * (uintptr_t)h * 16u))
                    return fail(fn + ": two of the tile, the moments and the guide planes overlap");
        return 0;
    });
    if (rc) return rc;
    if (!tptLaunchFoldBatch) return fail(fn + ": this build has no fold kernel");
    if ((rc = g.pending.discard())) return rc;
    const int nGuides = (deviceAlbedo ? 1 : 0) + (deviceNormalDepth ? 1 : 0);
    const size_t nPixels = (size_t)h * (size_t)w, planeBytes = nPixels * sizeof(f4);
    const bool clipPath = g.spheres.size() > 8 && g.spheres.size() < TPT_GROUP_MIN_SPHERES;
    const int perLaunch = clipPath ? tptFoldFramesPerLaunch(planeBytes, 2 + nGuides) : 1;
    // the guide staging: two halves of the largest launch's planes
    const size_t half = planeBytes * (size_t)nGuides * (size_t)(nFrames < perLaunch ? nFrames : perLaunch);
    if (2 * half > g.guideStageBytes) {
        if ((rc = syncAllStreams())) return rc; // (an earlier call's launches and folds may still use the old staging)
        (void)hipFree(g.dGuideStage);
        g.dGuideStage = nullptr;
        g.guideStageBytes = 0;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dGuideStage), 2 * half));
        g.guideStageBytes = 2 * half;
    }
    CameraPOD cams[kMaxBatch];
    f4 centres[2 * kMaxBatch];
    BatchTable table;
    if (clipPath) { // what does not change from frame to frame, as the camera-clip kernel's tables
        const SpherePOD s1 = g.spheres[1], s8 = g.spheres[8];
        for (int j = 0; j < kMaxBatch; ++j) {
            cams[j] = g.cam;
            centres[2 * j] = f4{s1.cx, s1.cy, s1.cz, 0.0f};
            centres[2 * j + 1] = f4{s8.cx, s8.cy, s8.cz, 0.0f};
        }
        table.cams = cams;
        table.centres = centres;
    }
    for (int f = 0; f < nFrames; f += perLaunch) {
        const int n = nFrames - f < perLaunch ? nFrames - f : perLaunch;
        // the launch's half of the guide staging: the one enqueueTrace gives it of the sums and the moments
        f4* const stage = g.dGuideStage + (clipPath ? (size_t)(g.clipSeq & 1u) * (g.guideStageBytes / (2 * sizeof(f4))) : 0);
        TraceTicket T;
        AovPlanes aov;
        aov.albedo = deviceAlbedo ? stage : nullptr;
        aov.normalDepth = deviceNormalDepth ? stage + (deviceAlbedo ? (size_t)n * nPixels : 0) : nullptr;
        aov.moments = true;
        aov.continues = f > 0;
        aov.entry = "tptDrawDeviceBatchMoments";
        if ((rc = clipPath ? enqueueTrace(firstFrame + f, w, h, testFlags, nullptr, T, n, 1, &table, &aov)
                           : enqueueTrace(firstFrame + f, w, h, testFlags, nullptr, T, 1, 0, nullptr, &aov)))
            return rc;
        if (!T.valid) continue;
        tptLerpTable lerp = {};
        for (int j = 0; j < n; ++j)
            lerp.v[j] = makeFrameConsts(g.cam, w, h, g.spp, firstFrame + f + j, testFlags, g.seedMode, g.config, g.animateSmoothing).lerpFac;
        // the fold, behind the trace on the context stream; the clip path's frames have counted their rays apart (the slot's counters)
        if (T.pipelined) HIPCHK(hipStreamWaitEvent(g.stream, g.evTrace[T.slot], 0));
        HIPCHK(tptLaunchFoldBatch(deviceTile, deviceMoments, deviceAlbedo, deviceNormalDepth, T.colour, T.moments, aov.albedo, aov.normalDepth,
                                  T.nPixels, n, lerp, clipPath ? g.views[T.slot].rays : nullptr, g.dRays, g.stream));
        if (T.pipelined) { // (what enqueueResolve records: the slot's colour plane and counters are free again behind this fold)
            HIPCHK(hipEventRecord(g.evResolve[T.slot], g.stream));
            g.resolveRecorded[T.slot] = true;
        }
    }
    return 0;
}

// tptDrawDeviceMoments with a sample count per pixel (tptTraceAdaptiveKernel reads the caller's plane) and a blend weighted by samples:
// one launch of the adaptive resolve kernel takes the place of the tile's and the moments' blends.  It follows the trace on the context
// stream like them; the kernel has added its rays to the running total itself.
int tptDrawDeviceAdaptive(float time, int frameCount, int w, int h, float* deviceTile, float* deviceAlbedo, float* deviceNormalDepth,
                          float* deviceMoments, const int32_t* deviceSampleCounts, unsigned testFlags)
{
    (void)time; // (the scene state is that of the last tptUpdate, as for tptDrawDevice)
    const std::string fn = "tptDrawDeviceAdaptive";
    if (int rc_ = flushShardDeferred()) return rc_; // (see tptDrawDevice)
    if (requireInit()) return -1;
    if (!deviceTile || !deviceMoments || !deviceSampleCounts || w <= 0 || h <= 0)
        return fail(fn + ": bad arguments (deviceTile, deviceMoments, deviceSampleCounts, size)");
    int rc = checkPathQueueDraw(fn.c_str(), "sample counts are", w, h, kQueueKernel, [&] {
        const uintptr_t plane = (uintptr_t)w * (uintptr_t)h * 16u, counts = (uintptr_t)w * (uintptr_t)h * 4u;
        if (overlapsAny(deviceMoments, {deviceTile, deviceAlbedo, deviceNormalDepth}, plane))
            return fail(fn + ": deviceMoments overlaps the tile or a plane");
        const uintptr_t c = reinterpret_cast<uintptr_t>(deviceSampleCounts);
        for (const void* out : {(const void*)deviceTile, (const void*)deviceMoments, (const void*)deviceAlbedo, (const void*)deviceNormalDepth}) {
            const uintptr_t o = reinterpret_cast<uintptr_t>(out);
            if (out && c < o + plane && o < c + counts) return fail(fn + ": deviceSampleCounts overlaps the tile, the moments or a plane");
        }
        return 0;
    });
    if (rc) return rc;
    if (!tptLaunchAdaptiveResolve) return fail(fn + ": this build has no adaptive blend kernel");
    if ((rc = g.pending.discard())) return rc;
    TraceTicket T;
    AovPlanes aov;
    aov.albedo = reinterpret_cast<f4*>(deviceAlbedo);
    aov.normalDepth = reinterpret_cast<f4*>(deviceNormalDepth);
    aov.moments = true;
    aov.sampleCounts = deviceSampleCounts;
    if ((rc = enqueueTrace(frameCount, w, h, testFlags, nullptr, T, 1, 0, nullptr, &aov))) return rc;
    if (!T.valid) return 0;
    if (T.pipelined) HIPCHK(hipStreamWaitEvent(g.stream, g.evTrace[T.slot], 0));
    HIPCHK(tptLaunchAdaptiveResolve(deviceTile, deviceMoments, T.colour, T.moments, deviceSampleCounts, T.nPixels,
                                    (testFlags & TPT_FLAG_PROGRESSIVE) != 0, g.stream));
    if (T.pipelined) { // (what enqueueResolve records: the slot's colour plane is free again behind this blend)
        HIPCHK(hipEventRecord(g.evResolve[T.slot], g.stream));
        g.resolveRecorded[T.slot] = true;
    }
    return 0;
}

int tptRayCounterRead(int64_t* outTotalRays)
{
    if (int rc_ = flushShardDeferred()) return rc_;
    if (requireInit()) return -1;
    g.pending.closeStream(); // (the caller waits: tpt_host_draw.cpp)
    unsigned long long v = 0;
    HIPCHK(hipMemcpyAsync(&v, g.dRays, sizeof(v), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    if (outTotalRays) *outTotalRays = (int64_t)v;
    return 0;
}

int tptSetTileMirror(float* deviceMirror, void* deviceCounterOut)
{
    g.mirror = deviceMirror;
    g.mirrorCounter = deviceMirror ? static_cast<unsigned long long*>(deviceCounterOut) : nullptr;
    return 0;
}

int tptSetRayCounter(void* deviceU64)
{
    if (int rc_ = flushShardDeferred()) return rc_;
    if (requireInit()) return -1;
    if (g.pending.discard()) return -2;
    HIPCHK(hipStreamSynchronize(g.stream));
    g.dRays = deviceU64 ? static_cast<unsigned long long*>(deviceU64) : g.dRaysOwn;
    int64_t total = 0;
    int rc = tptRayCounterRead(&total);
    if (rc) return rc;
    g.lastTotal = total; // DrawTest reports per-frame differences of the active counter
    return 0;
}

int tptSynchronize(void)
{
    if (int rc_ = flushShardDeferred()) return rc_;
    if (requireInit()) return -1;
    g.pending.closeStream();
    if (int rc = launchTailHelpers()) return rc;
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int tptTimerBegin(void)
{
    if (requireInit()) return -1;
    HIPCHK(hipEventRecord(g.ev0, g.stream));
    return 0;
}
int tptTimerEnd(float* outMs)
{
    if (int rc_ = flushShardDeferred()) return rc_;
    if (requireInit()) return -1;
    HIPCHK(hipEventRecord(g.ev1, g.stream));
    // a wait like tptSynchronize: the open stream batch is closed FIRST -- its launch is told that its unasked frames are no longer
    // wanted while it still runs (tpt_frame_pools.h), which after the wait below would be too late
    g.pending.closeStream();
    if (int rc = launchTailHelpers()) return rc;
    HIPCHK(hipEventSynchronize(g.ev1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, g.ev0, g.ev1));
    if (outMs) *outMs = ms;
    return 0;
}

} // extern "C"
