// tpt_host_draw.cpp -- the launches traced ahead of their call (LaunchQueue); DrawTest on the caller's HOST backbuffer (Test.cpp:344-367,
// synchronous): look-ahead, row-serial batches, banded copies; the display conversion; and the entry points that run on the context
// stream outside the frame pipeline -- the post-process passes, the object plane and motion table, the caller's rays, the lens draw --
// with the checks, the buffer growth and the launch plan they share (Span .. checkObjectCount, laneRefillScene, laneRefillChunks)
// (one of the host runtime's translation units: tpt_context.h lists them)
#include "tpt_context.h"

using namespace tpt;
using namespace tpth;

namespace tpth {

bool LaunchQueue::frontMatches(PendingLaunch::Kind kind, int frame, int w, int h, unsigned flags, unsigned long long key) const
{
    const PendingLaunch& F = e[0];
    return holds(kind) && frame == F.firstFrame + F.next && F.w == w && F.h == h && F.flags == flags && F.key == key;
}

// The front launch's next frame becomes the caller's: its plane of the launch and its ray counter.  wasOpen: the launch was pending
// when the call arrived (not pushed by it); its AHEAD and ROW_SERIAL frames then count as look-ahead hits.
void LaunchQueue::serveFront(bool wasOpen, TraceTicket& T, const unsigned long long*& rays)
{
    PendingLaunch& F = e[0];
    if (wasOpen && F.kind != PendingLaunch::STREAM) g.aheadHits++;
    T = F.T.plane(F.next);
    rays = F.rays + F.next;
    if (++F.next < F.T.batch) return;
    for (int k = 0; k + 1 < n; ++k) e[k] = e[k + 1]; // used up: the launch after it moves to the front
    --n;
}

int LaunchQueue::push(const PendingLaunch& L)
{
    if (n == kCap || (n > 0 && !holds(L.kind))) return fail("internal: launch queue full or of another kind");
    e[n++] = L;
    return 0;
}

// The launches traced ahead belong to a sequence that did not continue as predicted (or another path is about to be used): let
// them finish and forget them.  Their colour planes were never blended into anything.  (An open STREAM batch needs no wait: its
// unserved planes are simply never blended.)
int LaunchQueue::discard()
{
    if (n > 0 && !holds(PendingLaunch::STREAM))
        for (int k = 0; k < Context::kMaxOverlap; ++k) HIPCHK(hipStreamSynchronize(g.traceStream[k]));
    cutFront();
    n = 0;
    return 0;
}

// A STREAM entry is about to be dropped with frames next .. batch - 1 unserved: nobody will blend them, so its launch -- which may
// still be running, or not even have started -- is told to trace frames < next only (tpt_frame_pools.h: the slot's cut word, a plain
// store to pinned host memory that the kernel polls; no stream, no queue).  next >= 1: a STREAM batch is served on push.  A launch
// without a pool per frame (a grid too small for one) has no word and runs to its end as before.
void LaunchQueue::cutFront()
{
    if (!holds(PendingLaunch::STREAM) || !g.hCut) return;
    const PendingLaunch& F = e[0];
    if (F.T.valid && F.T.cutSerial != 0u && F.next >= 1 && F.next < F.T.batch)
        __atomic_store_n(g.hCut + F.T.slot, frameCutWord(F.T.cutSerial, (unsigned)F.next), __ATOMIC_RELEASE);
}

// The caller waits (tptSynchronize, tptRayCounterRead): an open STREAM batch is dropped, so that no frame traced before the wait is
// served after it, and the next call starts a stream afresh.  No wait and no ray lost: a STREAM frame's rays are folded in when it is
// served.  AHEAD and ROW_SERIAL launches stay (a synchronous caller's look-ahead).
void LaunchQueue::closeStream()
{
    cutFront();
    if (holds(PendingLaunch::STREAM)) n = 0;
    g.streamNext = -1;
}

// Trace the frames after `frameCount` ahead of the caller, up to tptSetHostLookahead of them: the reference's hosts call
// DrawTest(f), DrawTest(f + 1), ... with nothing else changing (TestWin.cpp:313-316, Renderer.mm:225, main.cpp:59-60); a
// frame alone on the GPU is bound by its longest paths (one frame in flight: 1.0 ms, three: 0.55 ms per frame).
int traceAhead(int frameCount, int w, int h, unsigned testFlags, unsigned long long key, int want)
{
    LaunchQueue& Q = g.pending;
    int nextFrame = Q.n ? Q.e[Q.n - 1].firstFrame + 1 : frameCount + 1;
    // every frame traced but not yet blended holds a slot (its colour buffer): this one plus the ones ahead must leave one
    // slot spare, whatever the hardware-queue probe clamped the pipeline to
    const int nSlots = effectiveOverlap();
    const int maxAhead = want < nSlots - 2 ? want : nSlots - 2;
    while (Q.n < maxAhead) {
        PendingLaunch A; // (an AHEAD launch: the default kind)
        A.firstFrame = nextFrame++; A.w = w; A.h = h; A.flags = testFlags; A.key = key;
        A.rays = g.dRaysAhead + g.frameSeq % (unsigned long long)Context::kMaxSlots;
        int rc = enqueueTrace(A.firstFrame, w, h, testFlags, A.rays, A.T);
        if (rc) return rc;
        if (!A.T.valid) break;
        if ((rc = Q.push(A))) return rc;
    }
    return 0;
}

static_assert(sizeof(CameraPOD) == 22 * sizeof(float), "the reference's Camera: the callers' camera arrays are read as records of this size");

// A caller's buffer at its full extent, and whether two of them share a byte (a null one shares none).
struct Span {
    const void* p;
    uintptr_t bytes;
};
static bool overlaps(Span a, Span b)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a.p), y = reinterpret_cast<uintptr_t>(b.p);
    return x && y && x < y + b.bytes && y < x + a.bytes;
}
// Does one of `outs` share a byte with one of `ins`?
static bool anyOverlaps(std::initializer_list<Span> outs, std::initializer_list<Span> ins)
{
    for (const Span& o : outs)
        for (const Span& i : ins)
            if (overlaps(o, i)) return true;
    return false;
}
// Do two of `spans` share a byte?
static bool anyTwoOverlap(std::initializer_list<Span> spans)
{
    for (const Span* a = spans.begin(); a != spans.end(); ++a)
        for (const Span* b = a + 1; b != spans.end(); ++b)
            if (overlaps(*a, *b)) return true;
    return false;
}

// A device buffer that only the context stream uses, grown to `need` bytes when it holds fewer (`held`; kept until tptShutdown).  The
// stream is drained first: an earlier call's work may still be using the buffer that goes.  `zero`: the new buffer is cleared on the stream.
template <class T>
static int growStreamBuffer(T*& buffer, size_t& held, size_t need, bool zero = false)
{
    if (need <= held) return 0;
    HIPCHK(hipStreamSynchronize(g.stream));
    (void)hipFree(buffer);
    buffer = nullptr;
    held = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&buffer), need));
    held = need;
    if (zero) HIPCHK(hipMemsetAsync(buffer, 0, need, g.stream));
    return 0;
}

// The scalars' rules the passes share.  (NaN fails every comparison, +inf the upper one.)
static bool finiteAtLeast(float v, float lo) { return v >= lo && v <= 3.40282347e38f; }
static bool sigmaOk(float s) { return s == 0.0f || (s >= 1e-6f && s <= 1e6f); }
static float inv2(float s) { return s > 0.0f ? 1.0f / (s * s) : 0.0f; } // (what the kernels take of a sigma; 0: the guide is off)

// What the calls with a motion table refuse of it (f: the entry point; tableName: its parameter): the count's range, then that table
// and count are given together.
static int checkObjectCount(const std::string& f, const char* tableName, const void* table, int nObjects)
{
    if (nObjects < 0 || nObjects > 65534) return fail(f + ": nObjects must lie in 0..65534");
    if ((table != nullptr) != (nObjects > 0)) return fail(f + ": " + tableName + " and nObjects must be given together");
    return 0;
}

// What tptDenoiseDevice and tptDenoiseDeviceVariance refuse, in the order they check it (fn: the entry point).  The variance filter
// (`variance`) also requires deviceMoments, an input like the others, and checks `samples` and its luminance sigma (`sigma0`) before the
// guides' sigmas; the plain filter checks its colour sigma (`sigma0`) with them.
static int checkDenoise(const char* fn, bool variance, int w, int h, const float* colour, const float* albedo, const float* normalDepth,
                        const float* moments, const float* out, int iterations, float samples, float sigma0, float sigmaNormal,
                        float sigmaDepth, unsigned flags)
{
    const std::string f(fn);
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return fail(f + ": w and h must lie in 1..8192");
    if (!colour || !out) return fail(f + ": deviceColour and deviceOut are required");
    if (variance && !moments) return fail(f + ": deviceMoments is required");
    if (overlapsAny(out, {colour, albedo, normalDepth, moments}, (uintptr_t)w * (uintptr_t)h * 16u)) return fail(f + ": deviceOut overlaps an input");
    if (iterations < 1 || iterations > 8) return fail(f + ": iterations must lie in 1..8");
    if (variance) {
        if (!finiteAtLeast(samples, 1.0f)) return fail(f + ": samples must be finite and at least 1");
        if (!(sigma0 > 0.0f && sigma0 <= 1e6f)) return fail(f + ": sigmaLuminance must lie in (0, 1e6]");
        if (!sigmaOk(sigmaNormal) || !sigmaOk(sigmaDepth)) return fail(f + ": sigmaNormal and sigmaDepth must be 0 or lie in [1e-6, 1e6]");
    } else if (!sigmaOk(sigma0) || !sigmaOk(sigmaNormal) || !sigmaOk(sigmaDepth)) {
        return fail(f + ": every sigma must be 0 or lie in [1e-6, 1e6]");
    }
    if ((sigmaNormal != 0.0f || sigmaDepth != 0.0f) && !normalDepth) return fail(f + ": sigmaNormal and sigmaDepth need deviceNormalDepth");
    if (flags & ~(unsigned)TPT_DENOISE_DEMODULATE) return fail(f + ": unknown flag bits");
    if ((flags & TPT_DENOISE_DEMODULATE) && !albedo) return fail(f + ": TPT_DENOISE_DEMODULATE needs deviceAlbedo");
    return 0;
}

// What the temporal passes refuse of their scalars and of the two cameras (prevCamera may be null), in the order they check it, and
// what the kernels need of the cameras, made here in the stated order (k): the second half of checkTemporal, which
// tptDenoiseClipDevice runs on its own for every frame of its clip.
static int temporalConsts(const std::string& f, const void* camera, const void* prevCamera, float maxHistory, float depthTolerance,
                          float normalTolerance, float coverageTolerance, tptTemporalConsts& k)
{
    if (!(maxHistory >= 1.0f && maxHistory <= 65536.0f)) return fail(f + ": maxHistory must lie in 1..65536"); // (NaN fails)
    if (!finiteAtLeast(depthTolerance, 0.0f) || !finiteAtLeast(normalTolerance, 0.0f) || !finiteAtLeast(coverageTolerance, 0.0f))
        return fail(f + ": every tolerance must be finite and at least 0");
    auto dot3 = [](const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
    // The reference's Camera is 22 consecutive floats: origin, lowerLeftCorner, horizontal, vertical, uu, vv, ww, lensRadius.  A camera
    // the pass can project through is finite, its frame spans two directions and lies in front of its origin; a = ll - o, f = -dot(a, ww).
    auto cameraOk = [&](const float* c, float* a, float& fc) {
        for (int i = 0; i < 22; ++i)
            if (!(fabsf(c[i]) <= 3.40282347e38f)) return false;
        for (int i = 0; i < 3; ++i) a[i] = c[3 + i] - c[i];
        fc = -dot3(a, c + 18);
        return dot3(c + 6, c + 6) != 0.0f && dot3(c + 9, c + 9) != 0.0f && fc > 0.0f;
    };
    float cam[22], prev[22], a[3], fc;
    k = {};
    memcpy(cam, camera, sizeof cam);
    if (!cameraOk(cam, a, fc)) return fail(f + ": camera has a non-finite field, a degenerate frame or its frame behind its origin");
    memcpy(k.o, cam, 12); memcpy(k.ll, cam + 3, 12); memcpy(k.H, cam + 6, 12); memcpy(k.V, cam + 9, 12);
    if (prevCamera) {
        memcpy(prev, prevCamera, sizeof prev);
        if (!cameraOk(prev, k.pa, k.pf)) return fail(f + ": prevCamera has a non-finite field, a degenerate frame or its frame behind its origin");
        memcpy(k.po, prev, 12); memcpy(k.pH, prev + 6, 12); memcpy(k.pV, prev + 9, 12); memcpy(k.pw, prev + 18, 12);
        k.phh = dot3(prev + 6, prev + 6);
        k.pvv = dot3(prev + 9, prev + 9);
    }
    k.maxHistory = maxHistory; k.depthTol = depthTolerance; k.normalTol = normalTolerance; k.coverageTol = coverageTolerance;
    return 0;
}

// What tptTemporalAccumulateDevice and tptTemporalAccumulateObjectsDevice refuse, in the order they check it (f: the entry point), and
// what the kernels need of the two cameras, made here in the stated order (k).
static int checkTemporal(const std::string& f, int w, int h, const void* camera, const void* prevCamera, const float* deviceColour,
                         const float* deviceAlbedo, const float* deviceNormalDepth, const float* deviceMoments,
                         const float* devicePrevColour, const float* devicePrevAlbedo, const float* devicePrevNormalDepth,
                         const float* devicePrevMoments, float* deviceOutColour, float* deviceOutAlbedo, float* deviceOutMoments,
                         float* deviceOutVariance, float maxHistory, float depthTolerance, float normalTolerance, float coverageTolerance,
                         tptTemporalConsts& k)
{
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return fail(f + ": w and h must lie in 1..8192");
    if (!camera) return fail(f + ": camera is required");
    if (!deviceColour || !deviceAlbedo || !deviceNormalDepth || !deviceMoments) return fail(f + ": the four planes of this frame are required");
    if (!deviceOutColour || !deviceOutAlbedo || !deviceOutMoments || !deviceOutVariance) return fail(f + ": the four output planes are required");
    const int nPrev = (prevCamera != nullptr) + (devicePrevColour != nullptr) + (devicePrevAlbedo != nullptr) +
                      (devicePrevNormalDepth != nullptr) + (devicePrevMoments != nullptr);
    if (nPrev != 0 && nPrev != 5) return fail(f + ": prevCamera and the four prev planes must be all NULL or all given");
    const uintptr_t bytes = (uintptr_t)w * (uintptr_t)h * 16u;
    const float* outs[4] = {deviceOutColour, deviceOutAlbedo, deviceOutMoments, deviceOutVariance};
    for (int i = 0; i < 4; ++i) {
        if (overlapsAny(outs[i], {deviceColour, deviceAlbedo, deviceNormalDepth, deviceMoments, devicePrevColour, devicePrevAlbedo,
                                  devicePrevNormalDepth, devicePrevMoments}, bytes))
            return fail(f + ": an output overlaps an input");
        for (int j = 0; j < i; ++j)
            if (overlapsAny(outs[i], {outs[j]}, bytes)) return fail(f + ": two outputs overlap");
    }
    return temporalConsts(f, camera, prevCamera, maxHistory, depthTolerance, normalTolerance, coverageTolerance, k);
}

} // namespace tpth

extern "C" {

int tptSetHostBufferMode(int hostBufferOnlyWrittenByDrawTest)
{
    g.hostTrust = hostBufferOnlyWrittenByDrawTest ? 1 : 0;
    g.tileSrc = nullptr; // next DrawTest uploads once
    return 0;
}

int tptSetStreamBatching(int enable)
{
    if (requireInit()) return -1;
    int rc = g.pending.discard();
    if (rc) return rc;
    g.streamBatch = enable ? 1 : 0;
    return 0;
}

int tptSetHostLookahead(int frames)
{
    if (frames < 0 || frames > 3) return fail("tptSetHostLookahead: 0..3");
    if (g.inited) {
        int rc = g.pending.discard();
        if (rc) return rc;
    }
    g.lookahead = frames;
    return 0;
}

int tptDraw(float time, int frameCount, int w, int h, float* backbuffer, int* outRayCount, unsigned testFlags)
{
    if (int rc_ = flushShardDeferred()) return rc_;
    (void)time;
    if (requireInit()) return -1;
    if (!g.updated) return fail("tptDraw: call tptUpdate (UpdateTest) first");
    if (!backbuffer || w <= 0 || h <= 0) return fail("tptDraw: bad arguments");
    const int rows = localRows(h);
    const size_t rowBytes = (size_t)w * 4 * sizeof(float);
    const size_t need = rowBytes * (size_t)(rows > 0 ? rows : 1);
    if (need > g.frameCap) {
        int rc = g.pending.discard();
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(g.stream));
        if (g.dFrame) HIPCHK(hipFree(g.dFrame));
        g.dFrame = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dFrame), need));
        g.frameCap = need;
        g.tileSrc = nullptr;
    }
    const bool sharded = g.numParts > 1 && g.stripeRows > 0;
    const bool pipelined = effectiveOverlap() > 1;
    // What a traced frame depends on besides (frameCount, w, h, flags): scene, camera, spp, seed / fold mode, kernel variant,
    // sharding.  Every call that changes one of them bumps configEpoch; a pending scene change (tptSetScene, kFlagAnimate)
    // shows as sceneDirty / a pending scene set.
    const unsigned long long key = g.configEpoch;
    const bool stable = !g.sceneDirty && g.pendingSet < 0 && !(testFlags & TPT_FLAG_ANIMATE);

    // ---- 1. this frame's trace: traced ahead by an earlier call, or now
    DepthScope depthScope(pipelined && stable ? 1 + (g.lookahead < 3 ? g.lookahead : 3) : 1);
    LaunchQueue& Q = g.pending;
    TraceTicket T;
    const unsigned long long* rayPtr = nullptr;
    bool servedFromBatch = false;
    Context::HostCaller& HC = g.hostCaller;
    const int streak = HC.seq.next(frameCount, w, h, testFlags, key);
    const bool batchRefused = HC.refusedKey == key && HC.refusedW == w && HC.refusedH == h;
    if (g.seedMode == SEED_ROW_SERIAL && stable && pipelined && !sharded && g.lookahead > 0 && rows > 0 && !g.mirror && !batchRefused) {
        // ---- 1r. the reference's own seed mode: a frame alone is `rows` lanes of work, so the frames AHEAD are traced as one
        //          launch (rows x frames lanes) and served one by one.  A batch is 32 frames of GPU work for one delivered
        //          frame, so it is only launched for a caller that has shown its pattern -- the third consecutive frame of one
        //          configuration (a one-shot DrawTest, or a host that jumps about, takes the plain path below).  A batch the pipeline
        //          refuses (frame wider than 8192, over 4 GiB of colour planes, not enough device memory) is retried at half the size, down to 2 frames; if nothing fits
        //          the configuration is served frame by frame: DrawTest never fails because of the look-ahead.
        auto launch = [&](int firstFrame) -> int { // the first batch (empty queue) or the one behind the batch being served
            const PendingLaunch* F = Q.empty() ? nullptr : &Q.e[0];
            PendingLaunch B;
            B.kind = PendingLaunch::ROW_SERIAL;
            B.firstFrame = firstFrame; B.w = w; B.h = h; B.flags = testFlags; B.key = key;
            B.rays = g.dRaysBatch + (F && F->rays == g.dRaysBatch ? kMaxBatch : 0); // (two banks of counters: the other one than F's)
            // the batch behind one that is being served starts at THAT batch's size: a larger one would have to grow the colour
            // slots the first still reads (refused now) after draining the pipeline to find that out
            for (int n = F ? F->T.batch : kMaxBatch; n >= 2; n /= 2) {
                if (w > 8192 || h > 8192 || (long long)rows * w * n > (1ll << 30) || (unsigned long long)rows * w * 16ull * n > (4ull << 30)) continue;
                const int rc = enqueueTrace(firstFrame, w, h, testFlags, B.rays, B.T, n, 1);
                if (rc == 0) return B.T.valid ? Q.push(B) : 0;
                if (rc != kRefused) return rc; // a real failure (HIP error, no scene): not something a smaller batch cures
            }
            if (!F) { HC.refusedKey = key; HC.refusedW = w; HC.refusedH = h; } // nothing fits: frame by frame from here on
            return 0;
        };
        const bool open = Q.frontMatches(PendingLaunch::ROW_SERIAL, frameCount, w, h, testFlags, key);
        if (!open && (streak >= 2 || Q.holds(PendingLaunch::ROW_SERIAL))) {
            int rc = Q.discard();
            if (rc) return rc;
            if (streak >= 2 && (rc = launch(frameCount))) return rc;
        }
        if (Q.holds(PendingLaunch::ROW_SERIAL)) { // (matched, or launched just now)
            // (the batch after this one is launched at once: holding it back until the first hit -- the batch above only completes
            //  when its slowest row has, 60-90 ms -- serialises the batches and costs the sequential caller 2.7x: 1.6 instead of
            //  4.3 Gray/s, profiles/r04/r04_evidence.log; the caller has shown three consecutive frames by now)
            if (Q.n == 1) {
                int rc = launch(Q.e[0].firstFrame + Q.e[0].T.batch);
                if (rc) return rc;
            }
            Q.serveFront(open, T, rayPtr);
            servedFromBatch = true;
        }
    }
    if (servedFromBatch) {
        // (nothing more to trace)
    } else if (stable && Q.frontMatches(PendingLaunch::AHEAD, frameCount, w, h, testFlags, key)) {
        Q.serveFront(true, T, rayPtr);
    } else {
        int rc = Q.discard();
        if (rc) return rc;
        unsigned long long* rays = g.dRaysAhead + g.frameSeq % (unsigned long long)Context::kMaxSlots;
        if ((rc = enqueueTrace(frameCount, w, h, testFlags, rays, T))) return rc;
        rayPtr = T.valid ? rays : nullptr;
    }
    // ---- 2. trace the next frames ahead (a wrong guess costs GPU time only)
    // (in the reference's own seed mode the batches above ARE the look-ahead: single frames traced ahead would be 60-90 ms of
    //  GPU work each, dropped again when the batch is launched -- only a configuration whose batch was refused gets them)
    const bool rowSerialBatches = g.seedMode == SEED_ROW_SERIAL && !batchRefused && !sharded && !g.mirror && rows > 0;
    if (pipelined && stable && T.valid && !servedFromBatch && !rowSerialBatches) {
        int rc = traceAhead(frameCount, w, h, testFlags, key, g.lookahead);
        if (rc) return rc;
    }
    // ---- 3. the previous image: the host buffer is the source of truth (previous frame's RGB, caller-owned alpha) unless
    //         the caller has promised that only DrawTest writes it (tptSetHostBufferMode): then the device tile is, and the
    //         upload happens once per buffer.  Then blend and download.
    const bool upload = rows > 0 && !(g.hostTrust && g.tileSrc == backbuffer && g.tileW == w && g.tileH == h && frameCount != 0);
    if (upload) { g.tileSrc = backbuffer; g.tileW = w; g.tileH = h; }
    if (upload && !sharded && T.valid && T.pipelined && rows >= 64 && !g.mirror) {
        // Banded: rows in four bands, alternating between two streams, each band upload -> blend -> download, so that a
        // band's blend and download do not wait for the whole upload.  The caller's buffer is pageable (page-locking the
        // CALLER's memory is not ours to do -- it may be freed between calls), and a copy on pageable memory does not return
        // before it is done: the two directions do NOT overlap on the link (profiles/r03/r03_h2d_probe.log: 0.27-0.30 ms each
        // way at 50-55 GB/s, 0.28 ms for half up + half down "at once").  Going through a pinned staging buffer filled and
        // emptied by helper threads does overlap them and was tried in round 3: 0.74-0.78 instead of 0.80 ms per frame in a
        // plain process, 0.97-1.07 instead of 0.81 in one whose HIP context torch had initialised -- dropped.
        const int kBands = 4;
        HIPCHK(hipEventRecord(g.evBand, g.stream)); // (orders stream 2 behind everything earlier on g.stream)
        HIPCHK(hipStreamWaitEvent(g.hostStream2, g.evBand, 0));
        // Trace still running (nothing was traced ahead)?  Then all uploads go first, beside it; otherwise they are interleaved
        // with the downloads.  The query only picks the ORDER of the copies: the blends wait for the trace event either way
        // (an event query that said "done" too early made a blend read the colour buffer before its frame was in it).
        const bool traceDone = hipEventQuery(g.evTrace[T.slot]) == hipSuccess;
        (void)hipGetLastError();
        if (traceDone) {
            HIPCHK(hipStreamWaitEvent(g.stream, g.evTrace[T.slot], 0));
            HIPCHK(hipStreamWaitEvent(g.hostStream2, g.evTrace[T.slot], 0));
        }
        for (int pass = 0; pass < 2; ++pass) {
            for (int b = 0; b < kBands; ++b) {
                const int r0 = (int)((long long)rows * b / kBands), r1 = (int)((long long)rows * (b + 1) / kBands);
                hipStream_t st = (b & 1) ? g.hostStream2 : g.stream;
                char* hb = reinterpret_cast<char*>(backbuffer) + rowBytes * r0;
                float* db = g.dFrame + (size_t)r0 * w * 4;
                if (pass == 0) HIPCHK(hipMemcpyAsync(db, hb, rowBytes * (size_t)(r1 - r0), hipMemcpyHostToDevice, st));
                if (pass == 0 && !traceDone) continue;
                HIPCHK(tptLaunchResolve(db, T.colour + (size_t)r0 * w, (r1 - r0) * w, T.lerpFac, nullptr, g.dRays, nullptr, b == 0 ? rayPtr : nullptr, st));
                HIPCHK(hipMemcpyAsync(hb, db, rowBytes * (size_t)(r1 - r0), hipMemcpyDeviceToHost, st));
            }
            if (traceDone) break;
            if (pass == 0) { // uploads are on their way: now the blends wait for the trace
                HIPCHK(hipStreamWaitEvent(g.stream, g.evTrace[T.slot], 0));
                HIPCHK(hipStreamWaitEvent(g.hostStream2, g.evTrace[T.slot], 0));
            }
        }
        HIPCHK(hipEventRecord(g.evBandEnd, g.hostStream2));
        HIPCHK(hipStreamWaitEvent(g.stream, g.evBandEnd, 0));
        HIPCHK(hipEventRecord(g.evResolve[T.slot], g.stream));
        g.resolveRecorded[T.slot] = true;
    } else {
        if (upload) {
            int rc = uploadBackbuffer(backbuffer, w, h);
            if (rc) return rc;
        }
        int rc = enqueueResolve(T, g.dFrame, rayPtr);
        if (rc) return rc;
        if (rows > 0) {
            if (!sharded) {
                HIPCHK(hipMemcpyAsync(backbuffer, g.dFrame, rowBytes * rows, hipMemcpyDeviceToHost, g.stream));
            } else {
                for (int ly = 0; ly < rows; ly += g.stripeRows) {
                    int n = rows - ly < g.stripeRows ? rows - ly : g.stripeRows;
                    HIPCHK(hipMemcpyAsync(reinterpret_cast<char*>(backbuffer) + rowBytes * localToGlobal(ly),
                                          reinterpret_cast<const char*>(g.dFrame) + rowBytes * ly, rowBytes * n,
                                          hipMemcpyDeviceToHost, g.stream));
                }
            }
        }
    }
    unsigned long long frameRays = 0;
    if (T.valid) HIPCHK(hipMemcpyAsync(&frameRays, rayPtr, sizeof(frameRays), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    if (outRayCount) *outRayCount = (int)frameRays;
    return 0;
}

// Display conversion (Cpp/Emscripten/main.cpp:63-79): linear float tile -> RGBA8, top row first.
int tptDisplayRGBA8(const float* deviceTile, int w, int h, unsigned char* deviceRGBA)
{
    if (requireInit()) return -1;
    if (!deviceTile || !deviceRGBA || w <= 0 || h <= 0) return fail("tptDisplayRGBA8: bad arguments");
    HIPCHK(tptLaunchDisplay(deviceTile, deviceRGBA, w, h, g.stream));
    return 0;
}

// The a-trous denoiser (include/tpt_hip.h states the filter): a post-process on the context stream like the display conversion above.
// It touches no trace state -- frames traced ahead, stream batches, scene and camera stay as they are -- only the context's scratch
// plane, which the iterations ping-pong through beside deviceOut.
int tptDenoiseDevice(int w, int h, const float* deviceColour, const float* deviceAlbedo, const float* deviceNormalDepth, float* deviceOut,
                     int iterations, float sigmaColour, float sigmaNormal, float sigmaDepth, unsigned denoiseFlags)
{
    if (requireInit()) return -1;
    int rc = checkDenoise("tptDenoiseDevice", false, w, h, deviceColour, deviceAlbedo, deviceNormalDepth, nullptr, deviceOut, iterations, 0.0f,
                          sigmaColour, sigmaNormal, sigmaDepth, denoiseFlags);
    if (rc) return rc;
    if (!tptLaunchDenoise) return fail("tptDenoiseDevice: this build has no a-trous kernel");
    if (iterations > 1 && (rc = growStreamBuffer(g.dDenoise, g.denoiseBytes, (size_t)w * (size_t)h * sizeof(f4)))) return rc;
    HIPCHK(tptLaunchDenoise(deviceColour, deviceAlbedo, deviceNormalDepth, deviceOut, reinterpret_cast<float*>(g.dDenoise), w, h,
                            iterations, inv2(sigmaColour), inv2(sigmaNormal), inv2(sigmaDepth), (denoiseFlags & TPT_DENOISE_DEMODULATE) != 0,
                            g.stream));
    return 0;
}

// The variance-guided a-trous filter (include/tpt_hip.h states it): tptDenoiseDevice's checks, plus the moments plane, the sample
// count and the luminance sigma; the same scratch plane, which carries the variance in .w between the iterations.
int tptDenoiseDeviceVariance(int w, int h, const float* deviceColour, const float* deviceAlbedo, const float* deviceNormalDepth,
                             const float* deviceMoments, float samples, float* deviceOut, int iterations, float sigmaLuminance,
                             float sigmaNormal, float sigmaDepth, unsigned denoiseFlags)
{
    if (requireInit()) return -1;
    int rc = checkDenoise("tptDenoiseDeviceVariance", true, w, h, deviceColour, deviceAlbedo, deviceNormalDepth, deviceMoments, deviceOut,
                          iterations, samples, sigmaLuminance, sigmaNormal, sigmaDepth, denoiseFlags);
    if (rc) return rc;
    if (!tptLaunchDenoiseVariance) return fail("tptDenoiseDeviceVariance: this build has no variance-guided a-trous kernel");
    if (iterations > 1 && (rc = growStreamBuffer(g.dDenoise, g.denoiseBytes, (size_t)w * (size_t)h * sizeof(f4)))) return rc;
    HIPCHK(tptLaunchDenoiseVariance(deviceColour, deviceAlbedo, deviceNormalDepth, deviceMoments, deviceOut,
                                    reinterpret_cast<float*>(g.dDenoise), w, h, iterations, samples, sigmaLuminance * sigmaLuminance,
                                    inv2(sigmaNormal), inv2(sigmaDepth), (denoiseFlags & TPT_DENOISE_DEMODULATE) != 0, g.stream));
    return 0;
}

// The temporal accumulation pass (include/tpt_hip.h states it): a post-process on the context stream like the two filters, one launch,
// no scratch plane.  Both cameras are read here; what the kernel needs of them is made in the stated order and travels by value.
int tptTemporalAccumulateDevice(int w, int h, const void* camera, const void* prevCamera, const float* deviceColour,
                                const float* deviceAlbedo, const float* deviceNormalDepth, const float* deviceMoments,
                                const float* devicePrevColour, const float* devicePrevAlbedo, const float* devicePrevNormalDepth,
                                const float* devicePrevMoments, float* deviceOutColour, float* deviceOutAlbedo, float* deviceOutMoments,
                                float* deviceOutVariance, float maxHistory, float depthTolerance, float normalTolerance,
                                float coverageTolerance)
{
    if (requireInit()) return -1;
    const std::string f("tptTemporalAccumulateDevice");
    tptTemporalConsts k;
    int rc = checkTemporal(f, w, h, camera, prevCamera, deviceColour, deviceAlbedo, deviceNormalDepth, deviceMoments, devicePrevColour,
                           devicePrevAlbedo, devicePrevNormalDepth, devicePrevMoments, deviceOutColour, deviceOutAlbedo, deviceOutMoments,
                           deviceOutVariance, maxHistory, depthTolerance, normalTolerance, coverageTolerance, k);
    if (rc) return rc;
    if (!tptLaunchTemporal) return fail(f + ": this build has no temporal accumulation kernel");
    HIPCHK(tptLaunchTemporal(deviceColour, deviceAlbedo, deviceNormalDepth, deviceMoments, devicePrevColour, devicePrevAlbedo,
                             devicePrevNormalDepth, devicePrevMoments, deviceOutColour, deviceOutAlbedo, deviceOutMoments,
                             deviceOutVariance, w, h, k, g.stream));
    return 0;
}

// History rectification (include/tpt_hip.h states it): a post-process on the context stream behind either temporal pass, one launch,
// no scratch plane and no constants but the radius and gamma.  A pixel reads no accumulated value but its own, so the colour and
// moments outputs may BE the accumulated planes; every other shared byte is refused.
int tptRectifyHistoryDevice(int w, int h, const float* deviceColour, const float* deviceMoments, const float* deviceAccColour,
                            const float* deviceAccMoments, float* deviceOutColour, float* deviceOutMoments, float* deviceOutVariance,
                            int radius, float gamma)
{
    if (requireInit()) return -1;
    const std::string f("tptRectifyHistoryDevice");
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return fail(f + ": w and h must lie in 1..8192");
    if (!deviceColour || !deviceMoments || !deviceAccColour || !deviceAccMoments)
        return fail(f + ": this frame's colour and moments planes and the accumulated ones are required");
    if (!deviceOutColour || !deviceOutMoments || !deviceOutVariance) return fail(f + ": the three output planes are required");
    if (radius < 1 || radius > TPT_RECTIFY_MAX_RADIUS) return fail(f + ": radius must lie in 1..3");
    if (!finiteAtLeast(gamma, 0.0f)) return fail(f + ": gamma must be finite and at least 0");
    const uintptr_t bytes = (uintptr_t)w * (uintptr_t)h * 16u;
    const float* ins[4] = {deviceColour, deviceMoments, deviceAccColour, deviceAccMoments};
    const float* outs[3] = {deviceOutColour, deviceOutMoments, deviceOutVariance};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) {
            if (i < 2 && j == 2 + i && outs[i] == ins[j]) continue; // in place: the accumulated plane of the output's own kind, exactly
            if (overlapsAny(outs[i], {ins[j]}, bytes)) return fail(f + ": an output overlaps an input (other than in place)");
        }
        for (int j = 0; j < i; ++j)
            if (overlapsAny(outs[i], {outs[j]}, bytes)) return fail(f + ": two outputs overlap");
    }
    if (!tptLaunchRectify) return fail(f + ": this build has no history rectification kernel");
    HIPCHK(tptLaunchRectify(deviceColour, deviceMoments, deviceAccColour, deviceAccMoments, deviceOutColour, deviceOutMoments,
                            deviceOutVariance, w, h, radius, gamma, g.stream));
    return 0;
}

// The spatial variance estimate (include/tpt_hip.h states it): a post-process on the context stream between the chain's moments planes
// and its filter, one launch over the whole stack of frames, no scratch plane.  The sigmas are checked and inverted as
// tptDenoiseDevice's are.
int tptSpatialVarianceDevice(int screenWidth, int screenHeight, int nFrames, const float* deviceFrameMoments,
                             const float* deviceFrameNormalDepth, float* deviceFrameOutVariance, float samplesPerFrame, float minSamples,
                             int radius, float sigmaNormal, float sigmaDepth)
{
    if (requireInit()) return -1;
    const std::string f("tptSpatialVarianceDevice");
    const int w = screenWidth, h = screenHeight;
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return fail(f + ": screenWidth and screenHeight must lie in 1..8192");
    if (nFrames < 1 || nFrames > 4096) return fail(f + ": nFrames must lie in 1..4096");
    if (!deviceFrameMoments || !deviceFrameOutVariance) return fail(f + ": deviceFrameMoments and deviceFrameOutVariance are required");
    if (radius < 1 || radius > TPT_SPREAD_MAX_RADIUS) return fail(f + ": radius must lie in 1..3");
    if (!finiteAtLeast(samplesPerFrame, 1.0f)) return fail(f + ": samplesPerFrame must be finite and at least 1");
    if (!(minSamples >= 1.0f)) return fail(f + ": minSamples must be at least 1 (+infinity: every pixel is estimated)"); // (NaN fails)
    if (!sigmaOk(sigmaNormal) || !sigmaOk(sigmaDepth)) return fail(f + ": sigmaNormal and sigmaDepth must be 0 or lie in [1e-6, 1e6]");
    if ((sigmaNormal != 0.0f || sigmaDepth != 0.0f) && !deviceFrameNormalDepth)
        return fail(f + ": sigmaNormal and sigmaDepth need deviceFrameNormalDepth");
    const uintptr_t bytes = (uintptr_t)w * (uintptr_t)h * 16u * (uintptr_t)nFrames;
    if (overlapsAny(deviceFrameOutVariance, {deviceFrameMoments, deviceFrameNormalDepth}, bytes))
        return fail(f + ": deviceFrameOutVariance overlaps an input");
    if (!tptLaunchSpread) return fail(f + ": this build has no spatial variance kernel");
    HIPCHK(tptLaunchSpread(deviceFrameMoments, deviceFrameNormalDepth, deviceFrameOutVariance, w, h, nFrames, samplesPerFrame, minSamples,
                           radius, inv2(sigmaNormal), inv2(sigmaDepth), g.stream));
    return 0;
}

// The temporal pass that follows objects (include/tpt_hip.h states it): the plain pass's checks, then those of the object planes and
// the motion table; one launch of its own kernel.
int tptTemporalAccumulateObjectsDevice(int w, int h, const void* camera, const void* prevCamera, const float* deviceColour,
                                       const float* deviceAlbedo, const float* deviceNormalDepth, const float* deviceMoments,
                                       const float* devicePrevColour, const float* devicePrevAlbedo, const float* devicePrevNormalDepth,
                                       const float* devicePrevMoments, float* deviceOutColour, float* deviceOutAlbedo,
                                       float* deviceOutMoments, float* deviceOutVariance, float maxHistory, float depthTolerance,
                                       float normalTolerance, float coverageTolerance, const int32_t* deviceObject,
                                       const int32_t* devicePrevObject, const float* deviceObjectMotion, int nObjects)
{
    if (requireInit()) return -1;
    const std::string f("tptTemporalAccumulateObjectsDevice");
    tptReprojectConsts k;
    int rc = checkTemporal(f, w, h, camera, prevCamera, deviceColour, deviceAlbedo, deviceNormalDepth, deviceMoments, devicePrevColour,
                           devicePrevAlbedo, devicePrevNormalDepth, devicePrevMoments, deviceOutColour, deviceOutAlbedo, deviceOutMoments,
                           deviceOutVariance, maxHistory, depthTolerance, normalTolerance, coverageTolerance, k.t);
    if (rc) return rc;
    if (!deviceObject) return fail(f + ": deviceObject is required");
    if ((devicePrevObject != nullptr) != (prevCamera != nullptr))
        return fail(f + ": devicePrevObject must be given exactly when prevCamera and the prev planes are");
    if ((rc = checkObjectCount(f, "deviceObjectMotion", deviceObjectMotion, nObjects))) return rc;
    // no output may share a byte with an object plane or the table, each at its full extent
    const uintptr_t pixels = (uintptr_t)w * (uintptr_t)h, plane = pixels * 16u;
    if (anyOverlaps({{deviceOutColour, plane}, {deviceOutAlbedo, plane}, {deviceOutMoments, plane}, {deviceOutVariance, plane}},
                    {{deviceObject, pixels * 4u}, {devicePrevObject, pixels * 4u}, {deviceObjectMotion, (uintptr_t)nObjects * 16u}}))
        return fail(f + ": an output overlaps an object plane or the motion table");
    if (!tptLaunchReprojectObjects) return fail(f + ": this build has no object-following accumulation kernel");
    HIPCHK(tptLaunchReprojectObjects(deviceColour, deviceAlbedo, deviceNormalDepth, deviceMoments, devicePrevColour, devicePrevAlbedo,
                                     devicePrevNormalDepth, devicePrevMoments, deviceOutColour, deviceOutAlbedo, deviceOutMoments,
                                     deviceOutVariance, deviceObject, devicePrevObject, deviceObjectMotion, nObjects, w, h, k, g.stream));
    return 0;
}

// A clip through the denoising chain (include/tpt_hip.h states it, and the staging's layout): per chunk one temporal launch per frame --
// the per-frame entry points' launchers, writing T_j into the staging's stacks -- then the filter's iterations, one launch each for
// the whole chunk.  Everything is checked, and every frame's camera constants are made, before the first launch.
int tptDenoiseClipDevice(const tptClipDenoiseArgs* args)
{
    if (requireInit()) return -1;
    const std::string f("tptDenoiseClipDevice");
    if (!args) return fail(f + ": args is required");
    const tptClipDenoiseArgs& A = *args;
    const int w = A.screenWidth, h = A.screenHeight, nFrames = A.nFrames;
    if (nFrames < 1 || nFrames > 4096) return fail(f + ": nFrames must lie in 1..4096");
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return fail(f + ": w and h must lie in 1..8192");
    if (A.clipFlags & ~(unsigned)TPT_CLIP_DENOISE_SPATIAL_ONLY) return fail(f + ": unknown clipFlags bits");
    const bool spatial = (A.clipFlags & TPT_CLIP_DENOISE_SPATIAL_ONLY) != 0, objects = A.deviceFrameObjects != nullptr;
    if (!A.deviceFrameImages || !A.deviceFrameMoments || !A.deviceFrameOut)
        return fail(f + ": deviceFrameImages, deviceFrameMoments and deviceFrameOut are required");
    if (spatial) {
        if (A.deviceFrameObjects || A.deviceFrameObjectMotion || A.nObjects != 0)
            return fail(f + ": TPT_CLIP_DENOISE_SPATIAL_ONLY takes no object planes and no motion tables");
        if (A.prevCamera || A.devicePrevNormalDepth || A.devicePrevObject || A.deviceHistory)
            return fail(f + ": TPT_CLIP_DENOISE_SPATIAL_ONLY takes no continuation (prevCamera, the prev planes, deviceHistory)");
    } else {
        if (!A.deviceFrameAlbedo || !A.deviceFrameNormalDepth || !A.cameras)
            return fail(f + ": deviceFrameAlbedo, deviceFrameNormalDepth and cameras are required without TPT_CLIP_DENOISE_SPATIAL_ONLY");
        if (A.prevCamera) {
            if (!A.deviceHistory || !A.devicePrevNormalDepth) return fail(f + ": prevCamera needs deviceHistory and devicePrevNormalDepth");
            if ((A.devicePrevObject != nullptr) != objects)
                return fail(f + ": with prevCamera, devicePrevObject must be given exactly when deviceFrameObjects is");
        } else if (A.devicePrevNormalDepth || A.devicePrevObject) {
            return fail(f + ": devicePrevNormalDepth and devicePrevObject need prevCamera");
        }
    }
    int rc = checkDenoise(f.c_str(), true, w, h, A.deviceFrameImages, A.deviceFrameAlbedo, A.deviceFrameNormalDepth, A.deviceFrameMoments,
                          A.deviceFrameOut, A.iterations, A.samples, A.sigmaLuminance, A.sigmaNormal, A.sigmaDepth, A.denoiseFlags);
    if (rc) return rc;
    if ((rc = checkObjectCount(f, "deviceFrameObjectMotion", A.deviceFrameObjectMotion, A.nObjects))) return rc;
    if (A.deviceFrameObjectMotion && !objects) return fail(f + ": deviceFrameObjectMotion needs deviceFrameObjects");
    std::vector<tptTemporalConsts> consts(spatial ? 0 : (size_t)nFrames);
    for (int j = 0; !spatial && j < nFrames; ++j) {
        const char* cam = static_cast<const char*>(A.cameras) + sizeof(CameraPOD) * (size_t)j;
        if ((rc = temporalConsts(f, cam, j > 0 ? cam - sizeof(CameraPOD) : A.prevCamera, A.maxHistory, A.depthTolerance, A.normalTolerance,
                                 A.coverageTolerance, consts[j])))
            return rc;
    }
    // the chunk length: the largest count <= 32 whose staging, in planes, stays within 4096 MiB
    const size_t pixels = (size_t)w * (size_t)h, planeBytes = pixels * 16u, budget = ((size_t)4096 << 20) / planeBytes;
    const size_t fit = spatial ? budget : (budget >= 4 ? (budget - 4) / 4 : 0);
    if (fit < 1) return fail(f + ": not even one frame's staging stays within 4096 MiB");
    const int chunk = fit < 32 ? (int)fit : 32, held = chunk < nFrames ? chunk : nFrames;
    // no output may share a byte with an input or with the other output, each at its full extent
    const uintptr_t stack = (uintptr_t)planeBytes * (uintptr_t)nFrames;
    const Span out = {A.deviceFrameOut, stack}, history = {A.deviceHistory, (uintptr_t)planeBytes * 3u};
    if (anyOverlaps({out, history},
                    {{A.deviceFrameImages, stack}, {A.deviceFrameMoments, stack}, {A.deviceFrameAlbedo, stack}, {A.deviceFrameNormalDepth, stack},
                     {A.deviceFrameObjects, (uintptr_t)pixels * 4u * (uintptr_t)nFrames},
                     {A.deviceFrameObjectMotion, (uintptr_t)nFrames * (uintptr_t)A.nObjects * 16u}, {A.devicePrevNormalDepth, planeBytes},
                     {A.devicePrevObject, (uintptr_t)pixels * 4u}}))
        return fail(f + ": deviceFrameOut or deviceHistory overlaps an input");
    if (overlaps(out, history)) return fail(f + ": deviceFrameOut overlaps deviceHistory");
    if (!tptLaunchFramesAtrous) return fail(f + ": this build has no frame-stack a-trous kernel");
    if (!spatial && !(objects ? (bool)tptLaunchReprojectObjects : (bool)tptLaunchTemporal))
        return fail(f + ": this build has no temporal accumulation kernel");
    if ((!spatial || A.iterations > 1) &&
        (rc = growStreamBuffer(g.dClipStage, g.clipStageBytes, planeBytes * (spatial ? (size_t)held : 4u * (size_t)held + 4u))))
        return rc;

    const float sl2 = A.sigmaLuminance * A.sigmaLuminance, in = inv2(A.sigmaNormal), id = inv2(A.sigmaDepth);
    const bool demod = (A.denoiseFlags & TPT_DENOISE_DEMODULATE) != 0;
    const size_t plane = pixels * 4u; // (floats)
    float* const stage = reinterpret_cast<float*>(g.dClipStage);
    if (spatial) {
        for (int c0 = 0; c0 < nFrames; c0 += chunk) {
            const int m = nFrames - c0 < chunk ? nFrames - c0 : chunk;
            const size_t at = plane * (size_t)c0;
            HIPCHK(tptLaunchFramesAtrous(A.deviceFrameImages + at, A.deviceFrameAlbedo ? A.deviceFrameAlbedo + at : nullptr,
                                         A.deviceFrameNormalDepth ? A.deviceFrameNormalDepth + at : nullptr, A.deviceFrameMoments + at,
                                         A.deviceFrameOut + at, stage, w, h, m, A.iterations, A.samples, sl2, in, id, demod, g.stream));
        }
        return 0;
    }
    // the staging: T's colour and albedo in stacks of held + 1 planes (slot 0: the chunk's predecessor, slot 1 + i: frame i of the
    // chunk), its variance and the ping-pong planes in stacks of `held`, its moments in two planes that the frames alternate between
    float* const tColour = stage;
    float* const tAlbedo = tColour + plane * (size_t)(held + 1);
    float* const tVariance = tAlbedo + plane * (size_t)(held + 1);
    float* const pingPong = tVariance + plane * (size_t)held;
    float* const tMoments = pingPong + plane * (size_t)held;
    int last = 0; // the slot of the clip's last frame
    for (int c0 = 0; c0 < nFrames; c0 += chunk) {
        const int m = nFrames - c0 < chunk ? nFrames - c0 : chunk;
        for (int i = 0; i < m; ++i) {
            const int j = c0 + i;
            const size_t at = plane * (size_t)j;
            const bool history = j > 0 || A.prevCamera;
            const float* pColour = !history ? nullptr : j > 0 ? tColour + plane * (size_t)i : A.deviceHistory;
            const float* pAlbedo = !history ? nullptr : j > 0 ? tAlbedo + plane * (size_t)i : A.deviceHistory + plane;
            const float* pMoments = !history ? nullptr : j > 0 ? tMoments + plane * (size_t)((j - 1) & 1) : A.deviceHistory + 2 * plane;
            const float* pNormalDepth = !history ? nullptr : j > 0 ? A.deviceFrameNormalDepth + at - plane : A.devicePrevNormalDepth;
            float* oColour = tColour + plane * (size_t)(i + 1);
            float* oAlbedo = tAlbedo + plane * (size_t)(i + 1);
            float* oMoments = tMoments + plane * (size_t)(j & 1);
            float* oVariance = tVariance + plane * (size_t)i;
            if (objects) {
                tptReprojectConsts k;
                k.t = consts[j];
                const int32_t* pObject = !history ? nullptr : j > 0 ? A.deviceFrameObjects + pixels * (size_t)(j - 1) : A.devicePrevObject;
                HIPCHK(tptLaunchReprojectObjects(A.deviceFrameImages + at, A.deviceFrameAlbedo + at, A.deviceFrameNormalDepth + at,
                                                 A.deviceFrameMoments + at, pColour, pAlbedo, pNormalDepth, pMoments, oColour, oAlbedo, oMoments,
                                                 oVariance, A.deviceFrameObjects + pixels * (size_t)j, pObject,
                                                 A.deviceFrameObjectMotion ? A.deviceFrameObjectMotion + 4u * (size_t)A.nObjects * (size_t)j : nullptr,
                                                 A.nObjects, w, h, k, g.stream));
            } else {
                HIPCHK(tptLaunchTemporal(A.deviceFrameImages + at, A.deviceFrameAlbedo + at, A.deviceFrameNormalDepth + at,
                                         A.deviceFrameMoments + at, pColour, pAlbedo, pNormalDepth, pMoments, oColour, oAlbedo, oMoments,
                                         oVariance, w, h, consts[j], g.stream));
            }
        }
        HIPCHK(tptLaunchFramesAtrous(tColour + plane, tAlbedo + plane, A.deviceFrameNormalDepth + plane * (size_t)c0, tVariance,
                                     A.deviceFrameOut + plane * (size_t)c0, pingPong, w, h, m, A.iterations, A.samples, sl2, in, id, demod,
                                     g.stream));
        last = m;
        if (c0 + m < nFrames) { // the next chunk overwrites slots 1 ..: its first frame finds this chunk's last in slot 0
            HIPCHK(hipMemcpyAsync(tColour, tColour + plane * (size_t)m, planeBytes, hipMemcpyDeviceToDevice, g.stream));
            HIPCHK(hipMemcpyAsync(tAlbedo, tAlbedo + plane * (size_t)m, planeBytes, hipMemcpyDeviceToDevice, g.stream));
        }
    }
    if (A.deviceHistory) {
        HIPCHK(hipMemcpyAsync(A.deviceHistory, tColour + plane * (size_t)last, planeBytes, hipMemcpyDeviceToDevice, g.stream));
        HIPCHK(hipMemcpyAsync(A.deviceHistory + plane, tAlbedo + plane * (size_t)last, planeBytes, hipMemcpyDeviceToDevice, g.stream));
        HIPCHK(hipMemcpyAsync(A.deviceHistory + 2 * plane, tMoments + plane * (size_t)((nFrames - 1) & 1), planeBytes, hipMemcpyDeviceToDevice,
                              g.stream));
    }
    return 0;
}

// tptMotionVectorsDevice's table (Context::dFlowConsts) and the two halves of its pinned twin, grown to `records` records when a call
// needs more: the next half is filled with `consts` and copied into the table on the context stream.  `dev`: the table.
static int uploadFlowConsts(const tptFlowConsts* consts, size_t records, const tptFlowConsts*& dev)
{
    const size_t half = sizeof(tptFlowConsts) * records;
    for (int i = 0; i < 2; ++i)
        if (!g.evFlow[i]) HIPCHK(hipEventCreateWithFlags(&g.evFlow[i], kOrderingEvent));
    if (half > g.flowConstsBytes) {
        // (an earlier call's copy or launches may still be using the table being replaced; only the context stream uses it)
        HIPCHK(hipStreamSynchronize(g.stream));
        (void)hipFree(g.dFlowConsts);
        if (g.hFlowConsts) (void)hipHostFree(g.hFlowConsts);
        g.dFlowConsts = g.hFlowConsts = nullptr;
        g.flowConstsBytes = 0;
        g.flowCopied[0] = g.flowCopied[1] = false;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dFlowConsts), half));
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&g.hFlowConsts), 2 * half, hipHostMallocDefault));
        g.flowConstsBytes = half;
    }
    const int hf = (int)(g.flowSeq++ & 1u);
    if (g.flowCopied[hf]) HIPCHK(hipEventSynchronize(g.evFlow[hf])); // the half's previous copy has left the pinned twin
    tptFlowConsts* const host = g.hFlowConsts + (size_t)hf * (g.flowConstsBytes / sizeof(tptFlowConsts));
    memcpy(host, consts, half);
    // (one table: its copy and the launches that read it are ordered on the context stream, behind the previous call's launches)
    HIPCHK(hipMemcpyAsync(g.dFlowConsts, host, half, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipEventRecord(g.evFlow[hf], g.stream));
    g.flowCopied[hf] = true;
    dev = g.dFlowConsts;
    return 0;
}

// A clip's motion vectors (include/tpt_hip.h states them): frame j's depend on the planes of frames j and j - 1 as traced and on
// nothing accumulated, so all frames whose predecessor lies in the stacks go through in one launch (more only where a launch would pass
// 2^31 lanes), frame 0 in one more on the prev planes, or zeroed where it has no predecessor.  Everything is checked, and every
// frame's camera constants are made -- by temporalConsts, the temporal passes' own rules and arithmetic -- before the first enqueue; the
// constants travel in one copy per call.
int tptMotionVectorsDevice(const tptMotionVectorsArgs* args)
{
    if (requireInit()) return -1;
    const std::string f("tptMotionVectorsDevice");
    if (!args) return fail(f + ": args is required");
    const tptMotionVectorsArgs& A = *args;
    const int w = A.screenWidth, h = A.screenHeight, nFrames = A.nFrames;
    if (nFrames < 1 || nFrames > 4096) return fail(f + ": nFrames must lie in 1..4096");
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return fail(f + ": w and h must lie in 1..8192");
    if (A.flags != 0) return fail(f + ": flags must be 0");
    if (!A.cameras || !A.deviceFrameAlbedo || !A.deviceFrameNormalDepth || !A.deviceFrameMotion)
        return fail(f + ": cameras, deviceFrameAlbedo, deviceFrameNormalDepth and deviceFrameMotion are required");
    const bool objects = A.deviceFrameObjects != nullptr;
    if (A.prevCamera) {
        if (!A.devicePrevAlbedo || !A.devicePrevNormalDepth) return fail(f + ": prevCamera needs devicePrevAlbedo and devicePrevNormalDepth");
        if ((A.devicePrevObject != nullptr) != objects)
            return fail(f + ": with prevCamera, devicePrevObject must be given exactly when deviceFrameObjects is");
    } else if (A.devicePrevAlbedo || A.devicePrevNormalDepth || A.devicePrevObject) {
        return fail(f + ": devicePrevAlbedo, devicePrevNormalDepth and devicePrevObject need prevCamera");
    }
    if (A.deviceFrameObjectMotion && !objects) return fail(f + ": deviceFrameObjectMotion needs deviceFrameObjects");
    if (int rc = checkObjectCount(f, "deviceFrameObjectMotion", A.deviceFrameObjectMotion, A.nObjects)) return rc;
    std::vector<tptFlowConsts> consts((size_t)nFrames);
    for (int j = 0; j < nFrames; ++j) {
        const char* cam = static_cast<const char*>(A.cameras) + sizeof(CameraPOD) * (size_t)j;
        tptTemporalConsts t; // (a history length the temporal passes accept: this call has none)
        if (int rc = temporalConsts(f, cam, j > 0 ? cam - sizeof(CameraPOD) : A.prevCamera, 1.0f, A.depthTolerance, A.normalTolerance,
                                    A.coverageTolerance, t))
            return rc;
        tptFlowConsts& k = consts[j];
        static_assert(offsetof(tptFlowConsts, depthTol) == offsetof(tptTemporalConsts, maxHistory), "tptTemporalConsts' fields, in its order");
        memcpy(&k, &t, offsetof(tptFlowConsts, depthTol));
        k.depthTol = t.depthTol; k.normalTol = t.normalTol; k.coverageTol = t.coverageTol;
    }
    // the output may not share a byte with an input, each at its full extent
    const size_t pixels = (size_t)w * (size_t)h, planeBytes = pixels * 16u;
    const uintptr_t stack = (uintptr_t)planeBytes * (uintptr_t)nFrames;
    if (anyOverlaps({{A.deviceFrameMotion, stack}},
                    {{A.deviceFrameAlbedo, stack}, {A.deviceFrameNormalDepth, stack}, {A.deviceFrameObjects, (uintptr_t)pixels * 4u * (uintptr_t)nFrames},
                     {A.deviceFrameObjectMotion, (uintptr_t)nFrames * (uintptr_t)A.nObjects * 16u}, {A.devicePrevAlbedo, planeBytes},
                     {A.devicePrevNormalDepth, planeBytes}, {A.devicePrevObject, (uintptr_t)pixels * 4u}}))
        return fail(f + ": deviceFrameMotion overlaps an input");
    if (!tptLaunchFlow) return fail(f + ": this build has no motion-vector kernel");

    const int first = A.prevCamera ? 0 : 1; // the first frame with a predecessor
    const tptFlowConsts* table = nullptr;   // (its record 0 is frame `first`'s)
    if (first < nFrames)
        if (int rc = uploadFlowConsts(consts.data() + first, (size_t)(nFrames - first), table)) return rc;
    const size_t plane = pixels * 4u; // (floats)
    if (A.prevCamera)
        HIPCHK(tptLaunchFlow(A.deviceFrameAlbedo, A.deviceFrameNormalDepth, A.deviceFrameObjects, A.devicePrevAlbedo, A.devicePrevNormalDepth,
                             A.devicePrevObject, A.deviceFrameObjectMotion, A.nObjects, A.deviceFrameMotion, w, h, 1, table, g.stream));
    else
        HIPCHK(hipMemsetAsync(A.deviceFrameMotion, 0, planeBytes, g.stream)); // (no predecessor: four +0 per pixel)
    // frames 1 .. nFrames-1: the predecessor of each is the plane before it; at most 2^31 lanes a launch (32 frames of 8192 x 8192)
    const size_t lanes = (size_t)((w + 63) / 64 * 64) * (size_t)((h + 3) / 4 * 4), most = ((size_t)1 << 31) / lanes;
    for (int j = 1; j < nFrames;) {
        const int m = (size_t)(nFrames - j) < most ? nFrames - j : (int)most;
        const size_t at = plane * (size_t)j, ids = pixels * (size_t)j;
        HIPCHK(tptLaunchFlow(A.deviceFrameAlbedo + at, A.deviceFrameNormalDepth + at, objects ? A.deviceFrameObjects + ids : nullptr,
                             A.deviceFrameAlbedo + at - plane, A.deviceFrameNormalDepth + at - plane,
                             objects ? A.deviceFrameObjects + ids - pixels : nullptr,
                             A.deviceFrameObjectMotion ? A.deviceFrameObjectMotion + 4u * (size_t)A.nObjects * (size_t)j : nullptr, A.nObjects,
                             A.deviceFrameMotion + at, w, h, m, table + (j - first), g.stream));
        j += m;
    }
    return 0;
}

// The object plane (include/tpt_hip.h states it): per frame one launch on the context stream over the scene set of the last tptUpdate,
// with the frame's camera and its centres of spheres 1 and 8 by value.  The host's spheres, camera, the launch queue and every setting
// stay as they are.  One thing moves: a scene set that tptUpdate staged and no launch has uploaded yet is uploaded here, on the context
// stream instead of the next draw's trace stream, and becomes the current set (enqueueSceneUpload).  Later launches wait for its
// evUploaded as they do for any set another stream carried, so they read the same scene either way.
int tptObjectPlaneDevice(int nFrames, const float* times, const void* cameras, int w, int h, int32_t* deviceFrameObjects,
                         unsigned testFlags)
{
    if (requireInit()) return -1;
    const std::string f("tptObjectPlaneDevice");
    if (!g.updated) return fail(f + ": call tptUpdate first");
    if (nFrames < 1 || nFrames > 4096) return fail(f + ": nFrames must lie in 1..4096");
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return fail(f + ": w and h must lie in 1..8192");
    if (!deviceFrameObjects) return fail(f + ": deviceFrameObjects is required");
    if (!cameras && (w != g.updatedW || h != g.updatedH)) return fail(f + ": without cameras the size must be the last tptUpdate's");
    if (testFlags & ~(unsigned)(TPT_FLAG_ANIMATE | TPT_FLAG_PROGRESSIVE)) return fail(f + ": unknown flag bits");
    for (int j = 0; cameras && j < nFrames; ++j) {
        float c[12];
        memcpy(c, static_cast<const char*>(cameras) + sizeof(CameraPOD) * (size_t)j, sizeof c);
        for (int i = 0; i < 12; ++i)
            if (!(fabsf(c[i]) <= 3.40282347e38f)) return fail(f + ": a camera has a non-finite origin, lowerLeftCorner, horizontal or vertical");
    }
    Context::SceneSet* S = activeSet();
    if (!S || !S->dev || S->nSpheres < 1) return fail(f + ": no scene staged (call tptUpdate first)");
    if (!tptLaunchObjectPlane) return fail(f + ": this build has no object plane kernel");
    // the scene as tptUpdate staged it: the records the kernel reads, and their host copy for the centres of spheres 1 and 8
    const f4* staged = reinterpret_cast<const f4*>(S->stage + S->offSph4);
    const f4* dev = reinterpret_cast<const f4*>(S->dev + S->offSph4);
    const int n = S->nSpheres;
    const bool animate = times && (testFlags & TPT_FLAG_ANIMATE) && n > 8; // (the tptUpdate guard, Test.cpp:304)
    int rc = enqueueSceneUpload(g.stream);
    if (rc) return rc;
    for (int j = 0; j < nFrames; ++j) {
        tptObjectPlaneConsts k = {};
        float c[12];
        memcpy(c, cameras ? static_cast<const char*>(cameras) + sizeof(CameraPOD) * (size_t)j : reinterpret_cast<const char*>(&g.cam), sizeof c);
        memcpy(k.o, c, 12); memcpy(k.ll, c + 3, 12); memcpy(k.H, c + 6, 12); memcpy(k.V, c + 9, 12);
        if (n > 1) { k.c1[0] = staged[1].x; k.c1[1] = staged[1].y; k.c1[2] = staged[1].z; }
        if (n > 8) { k.c8[0] = staged[8].x; k.c8[1] = staged[8].y; k.c8[2] = staged[8].z; }
        if (animate) {
            k.c1[1] = animatedY1(times[j]);
            k.c8[2] = animatedZ8(times[j]);
        }
        HIPCHK(tptLaunchObjectPlane(dev, n, deviceFrameObjects + (size_t)j * (size_t)w * (size_t)h, w, h, k, g.stream));
    }
    return 0;
}

// The plan of a lane-refill launch outside the frame pipeline (tptTraceRaysDevice, tptDrawDeviceLens), in two pieces; between them the
// caller looks for its launcher and fills in its work items (a.numItems).  The first (f: the entry point): the scene set the context
// last staged, and how the kernel takes it -- a.scene, whether it is staged in LDS, the launch's LDS bytes (laneRefillLds) -- refused
// where chooseKernel refuses a frame.
static int laneRefillScene(const std::string& f, KernelArgs& a, bool& ldsScene, size_t& lds)
{
    Context::SceneSet* S = activeSet();
    if (!S || !S->dev || S->nSpheres < 1) return fail(f + ": no scene staged (call tptUpdate first)");
    if (S->nLights > TPT_MAX_LIGHTS)
        return fail(f + ": too many emissive spheres for the LDS light table (" + std::to_string(TPT_MAX_LIGHTS) + " at most)");
    a.scene = deviceView();
    lds = laneRefillLds(a, ldsScene);
    if (!fitsCuLds(lds)) return fail(f + ": scene too large for LDS staging; use tptSetKernelVariant(.., .., 0)");
    return 0;
}

// The second: sizeGrid's chunks for a.numItems work items -- 256 a chunk, 64 when that leaves a resident wave fewer than eight -- and the
// grid, a workgroup per chunk up to what is resident at once.  Returns the workgroups.
static int laneRefillChunks(KernelArgs& a, bool ldsScene, size_t lds)
{
    const int occ = laneRefillOccupancy(ldsScene, lds), resident = g.traceCUs * occ;
    a.chunkSize = a.numItems / TPT_CHUNK_PIXELS < 8 * resident ? 64 : TPT_CHUNK_PIXELS;
    a.chunkShift = a.chunkSize == 64 ? 6 : 8;
    a.numChunks = (a.numItems + a.chunkSize - 1) / a.chunkSize;
    a.chunksPerFrame = a.numChunks;
    int blocks = a.numChunks < resident ? a.numChunks : resident;
    if (blocks < 1) blocks = 1;
    a.totalWaves = (unsigned)blocks;
    return blocks;
}

// The buffers of a lane-refill launch outside the frame pipeline (tptTraceRaysDevice, tptDrawDeviceLens; tpt_context.h: dRayStack,
// dRayWork): the bounce-stack spill for `blocks` workgroups, grown on demand, the counter block, and the word the rays are counted into
// -- the caller's, or the block's own.
static int rayLaunchBuffers(KernelArgs& a, int blocks, unsigned long long* deviceRayCount)
{
    if (!g.dRayWork) {
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&g.dRayWork), 16 * sizeof(unsigned) + sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(g.dRayWork, 0, 16 * sizeof(unsigned) + sizeof(unsigned long long), g.stream));
    }
    const bool needStack = g.foldMode == FOLD_RECURSIVE && a.ldsStackLevels < TPT_MAX_DEPTH;
    const size_t stackBytes = needStack ? (size_t)blocks * TPT_BLOCK * (size_t)(TPT_MAX_DEPTH - a.ldsStackLevels) * sizeof(f4) : 0;
    if (int rc = growStreamBuffer(g.dRayStack, g.rayStackBytes, stackBytes, true)) return rc;
    a.stackBuf = needStack ? g.dRayStack : nullptr;
    a.stackStride = needStack ? blocks * TPT_BLOCK : 0;
    a.work = g.dRayWork;
    a.rayCounter = deviceRayCount ? deviceRayCount : reinterpret_cast<unsigned long long*>(g.dRayWork + 16);
    return 0;
}

// Radiance and first hits along the caller's rays (include/tpt_hip.h states them): one launch of the lane-refill kernel on the context
// stream with the rays as its work items (KernelArgs::rays), planned as chooseKernel plans that kernel for a frame -- LDS scene, bounce
// stack levels, occupancy -- and sized as sizeGrid sizes it, without the frame pipeline: no colour slot, no trace stream, no blend, no
// chunk order.  The scene set is the object plane's: what the context last staged, uploaded here if no launch has yet, and from then on
// the current set, which a later tptUpdate does not touch -- it stages into the ring's next set, as it does under a draw's launch.
// The launch has a spill buffer and a counter block of its own (Context::dRayStack, dRayWork).  The kernel's last wave re-arms the
// counters, and two ray calls cannot share the block in flight: both launches are on the context stream, so the second starts after
// the first has ended.
int tptTraceRaysDevice(const tptTraceRaysArgs* args)
{
    if (requireInit()) return -1;
    const std::string f("tptTraceRaysDevice");
    if (!args) return fail(f + ": args is required");
    const tptTraceRaysArgs& A = *args;
    if (!g.updated) return fail(f + ": call tptUpdate first");
    if (A.nRays < 1 || A.nRays > 16777216) return fail(f + ": nRays must lie in 1..16777216");
    if (A.flags != 0) return fail(f + ": flags must be 0");
    if (!A.deviceRays) return fail(f + ": deviceRays is required");
    if (!A.deviceRadiance && !A.deviceHits) return fail(f + ": deviceRadiance or deviceHits is required");
    // the input and the three outputs, each at its own extent: no output may share a byte with the input or with another output
    const uintptr_t n = (uintptr_t)A.nRays;
    const Span radiance = {A.deviceRadiance, n * 16u}, hits = {A.deviceHits, n * 32u}, count = {A.deviceRayCount, sizeof(unsigned long long)};
    if (anyOverlaps({radiance, hits, count}, {{A.deviceRays, n * 32u}})) return fail(f + ": an output overlaps deviceRays");
    if (anyTwoOverlap({radiance, hits, count})) return fail(f + ": two outputs overlap");
    KernelArgs a = KernelArgs{};
    bool ldsScene = false;
    size_t lds = 0;
    int rc = laneRefillScene(f, a, ldsScene, lds);
    if (rc) return rc;
    if (!tptLaunchTraceRays) return fail(f + ": this build has no ray launcher");

    memset(&a.fc, 0, sizeof a.fc); // (the camera plays no part)
    a.fc.width = a.fc.height = 1;
    a.fc.spp = 1; // with per-pixel seeds and one sample lanePost ends a lane after one path
    a.fc.invWidth = a.fc.invHeight = a.fc.invSpp = 1.0f;
    a.fc.seedMode = SEED_PER_PIXEL;
    a.fc.config = g.config;
    a.nLocalRows = 1; a.stripeRows = 1; a.stripeStride = 1; a.tilesX = 1;
    a.numItems = A.nRays;
    a.batchFrames = 1;
    a.laneCap = 64;
    const int blocks = laneRefillChunks(a, ldsScene, lds); // (256 rays a chunk, or 64)

    if ((rc = rayLaunchBuffers(a, blocks, A.deviceRayCount))) return rc;
    a.rays = reinterpret_cast<const f4*>(A.deviceRays);
    a.rayRadiance = reinterpret_cast<f4*>(A.deviceRadiance);
    a.rayHits = reinterpret_cast<f4*>(A.deviceHits);
    if ((rc = enqueueSceneUpload(g.stream))) return rc;
    HIPCHK(tptLaunchTraceRays(a, g.hs, g.foldMode, ldsScene, blocks, lds, g.stream));
    return 0;
}

// Why a lens record is refused, or null (include/tpt_hip.h lists the rules; the Python binding states them again before the call).
static const char* lensFault(const tptLens& L)
{
    if (L.kind != TPT_LENS_EQUIRECT && L.kind != TPT_LENS_FISHEYE && L.kind != TPT_LENS_ORTHO) return "unknown lens kind";
    const float* vecs[4] = {L.origin, L.right, L.up, L.forward};
    for (const float* v : vecs)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(v[k])) return "a non-finite lens field";
    if (!std::isfinite(L.sx) || !std::isfinite(L.sy) || !std::isfinite(L.maxAngle)) return "a non-finite lens field";
    for (int i = 1; i < 4; ++i) {
        const double dd = (double)vecs[i][0] * vecs[i][0] + (double)vecs[i][1] * vecs[i][1] + (double)vecs[i][2] * vecs[i][2];
        if (!(dd >= 0.99 && dd <= 1.01)) return "a basis vector is not of unit length (its squared length must lie in 0.99..1.01)";
        for (int k = i + 1; k < 4; ++k) {
            const double d = (double)vecs[i][0] * vecs[k][0] + (double)vecs[i][1] * vecs[k][1] + (double)vecs[i][2] * vecs[k][2];
            if (!(d >= -0.01 && d <= 0.01)) return "two basis vectors are not orthogonal (their dot product must lie in -0.01..0.01)";
        }
    }
    if (!(L.sx > 0.0f) || !(L.sy > 0.0f)) return "sx and sy must be positive";
    if (L.kind == TPT_LENS_EQUIRECT && (L.sx > 6.2831855f || L.sy > 3.1415927f)) return "an equirectangular span beyond 2 pi x pi";
    if (L.kind == TPT_LENS_FISHEYE && (L.sx > 4.0f || L.sy > 4.0f)) return "a fisheye scale beyond 4";
    if (L.kind == TPT_LENS_FISHEYE && !(L.maxAngle > 0.0f && L.maxAngle <= 3.1415927f)) return "a fisheye maxAngle outside (0, pi]";
    if (L.kind != TPT_LENS_FISHEYE && L.maxAngle != 0.0f) return "maxAngle must be 0 for this lens kind";
    return nullptr;
}

// tptDrawDevice's contract through another lens (include/tpt_hip.h states it): one launch of the lane-refill kernel in its pixel mode
// on the context stream, its samples started at KernelArgs::lens, then the blend of the context's own colour plane into the caller's
// tile.  Planned as tptTraceRaysDevice plans its launch, whose scene set, spill buffer and counter block it shares, outside the frame
// pipeline: no colour slot, no trace stream, no chunk order, no frame traced ahead.
int tptDrawDeviceLens(const tptDrawLensArgs* args)
{
    if (requireInit()) return -1;
    const std::string f("tptDrawDeviceLens");
    if (!args) return fail(f + ": args is required");
    const tptDrawLensArgs& A = *args;
    if (!g.updated) return fail(f + ": call tptUpdate first");
    const int w = A.screenWidth, h = A.screenHeight;
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return fail(f + ": screenWidth and screenHeight must lie in 1..8192");
    if (A.frameCount < 0) return fail(f + ": frameCount must not be negative");
    if (A.flags != 0 && A.flags != (unsigned)TPT_FLAG_PROGRESSIVE) return fail(f + ": flags must be 0 or TPT_FLAG_PROGRESSIVE");
    if (!A.deviceTile) return fail(f + ": deviceTile is required");
    const size_t nPixels = (size_t)w * (size_t)h;
    if (overlaps({A.deviceRayCount, sizeof(unsigned long long)}, {A.deviceTile, nPixels * sizeof(f4)}))
        return fail(f + ": deviceRayCount lies inside the tile");
    if (const char* why = lensFault(A.lens)) return fail(f + ": " + why);
    KernelArgs a = KernelArgs{};
    bool ldsScene = false;
    size_t lds = 0;
    int rc = laneRefillScene(f, a, ldsScene, lds);
    if (rc) return rc;
    if (!tptLaunchTraceLens) return fail(f + ": this build has no lens launcher");

    // (the camera plays no part; seeds per pixel, the flags' blend)
    a.fc = makeFrameConsts(g.cam, w, h, g.spp, A.frameCount, A.flags, SEED_PER_PIXEL, g.config, g.animateSmoothing);
    static_assert(sizeof(LensPOD) == sizeof(tptLens) && sizeof(tptLens) == 64, "the kernel reads the caller's record as it is");
    memcpy(&a.lens, &A.lens, sizeof a.lens);
    a.nLocalRows = h; a.stripeRows = h; a.stripeStride = h; a.stripeOffset = 0;
    a.tilesX = (w + 7) / 8;
    a.numItems = a.tilesX * ((h + 7) / 8) * 64;
    a.batchFrames = 1;
    a.framePlane = h * w;
    a.laneCap = 64;
    const int blocks = laneRefillChunks(a, ldsScene, lds); // (256 pixels a chunk, or single 8x8 tiles)

    if ((rc = rayLaunchBuffers(a, blocks, A.deviceRayCount))) return rc;
    if ((rc = growStreamBuffer(g.dLensColour, g.lensColourBytes, nPixels * sizeof(f4)))) return rc;
    a.frameColour = g.dLensColour;
    if ((rc = enqueueSceneUpload(g.stream))) return rc;
    HIPCHK(tptLaunchTraceLens(a, g.hs, g.foldMode, ldsScene, blocks, lds, g.stream));
    HIPCHK(tptLaunchResolve(A.deviceTile, g.dLensColour, (int)nPixels, a.fc.lerpFac, nullptr, g.dRays, nullptr, nullptr, g.stream));
    return 0;
}

// The animated scene's displacement per sphere between two times (include/tpt_hip.h states it): host arithmetic only.
int tptObjectMotionTable(float time, float prevTime, unsigned testFlags, float* outTable, int capacity)
{
    if (requireInit()) return -1;
    const std::string f("tptObjectMotionTable");
    if (!outTable) return fail(f + ": outTable is required");
    if (g.spheres.empty()) defaultScene(g.spheres, g.mats);
    const int count = (int)g.spheres.size();
    if (capacity < count) return fail(f + ": capacity is smaller than the object count");
    memset(outTable, 0, sizeof(float) * 4 * (size_t)count);
    if ((testFlags & TPT_FLAG_ANIMATE) && count > 8) { // (the tptUpdate guard, Test.cpp:304)
        outTable[4 * 1 + 1] = animatedY1(prevTime) - animatedY1(time);
        outTable[4 * 8 + 2] = animatedZ8(prevTime) - animatedZ8(time);
    }
    return 0;
}

// The plan pass of adaptive sampling (include/tpt_hip.h states it): a post-process on the context stream like the filters, one launch
// (and the memset of the total it adds to).
int tptAdaptiveSamplesDevice(int w, int h, const float* deviceMoments, float targetError, int minSamples, int maxSamples,
                             int32_t* deviceSampleCounts, float* deviceOutVariance, int64_t* deviceTotalSamples)
{
    if (requireInit()) return -1;
    const std::string f("tptAdaptiveSamplesDevice");
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return fail(f + ": w and h must lie in 1..8192");
    if (!deviceMoments || !deviceSampleCounts) return fail(f + ": deviceMoments and deviceSampleCounts are required");
    if (!(targetError > 0.0f && targetError <= 1e6f)) return fail(f + ": targetError must lie in (0, 1e6]"); // (NaN fails)
    if (minSamples < 0 || maxSamples > 2047 || minSamples > maxSamples) return fail(f + ": 0 <= minSamples <= maxSamples <= 2047 expected");
    // the input and the three outputs, each at its own extent: no output may share a byte with the input or with another output
    const uintptr_t pixels = (uintptr_t)w * (uintptr_t)h;
    const Span counts = {deviceSampleCounts, pixels * 4u}, variance = {deviceOutVariance, pixels * 16u}, total = {deviceTotalSamples, sizeof(int64_t)};
    if (anyOverlaps({counts, variance, total}, {{deviceMoments, pixels * 16u}})) return fail(f + ": an output overlaps deviceMoments");
    if (anyTwoOverlap({counts, variance, total})) return fail(f + ": two outputs overlap");
    if (!tptLaunchAdaptivePlan) return fail(f + ": this build has no adaptive plan kernel");
    HIPCHK(tptLaunchAdaptivePlan(deviceMoments, deviceSampleCounts, deviceOutVariance, deviceTotalSamples, w, h, targetError, minSamples,
                                 maxSamples, g.stream));
    return 0;
}

} // extern "C"
