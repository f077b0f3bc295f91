// tpt_context.h -- the host runtime's state (one context per process, like the reference's statics Test.cpp:13-69, 237) and the
// functions its translation units share.  Not an interface of the library: include/tpt_hip.h is.
//
//   tpt_host.cpp           context, initialisation, scene staging, the setters, UpdateTest, the reference's C++ symbols
//   tpt_host_pipeline.cpp  one frame: plan, buffers, trace launch, ordered blend; tail helpers; tptDrawDevice and its variants (Batch,
//                          Views, Animation, AnimationMoments, CameraClip, KeyframeClip, Aov, Moments, BatchMoments, Adaptive); the
//                          blocking calls
//   tpt_host_draw.cpp      the queue of launches traced ahead of their call (LaunchQueue, traceAhead); DrawTest on a host backbuffer
//                          (tptDraw: look-ahead, row-serial batches, banded copies) and its three setters; the display conversion;
//                          the entry points that run on the context stream outside the frame pipeline: the post-process passes (the
//                          a-trous filters, temporal accumulation, rectification, spatial variance, the clip chain, motion vectors,
//                          the adaptive plan), the object plane and motion table, the caller's rays, the lens draw
//   tpt_host_shard.cpp     multi-GPU inside the library: RCCL (dlopen), tptDrawSharded, tptShardedFinish
//   tpt_host_hooks.cpp     unit-test / profiling entry points (include/tpt_test_hooks.h; the second build only)
// and, of the headers they share with the kernels (tpt_kernels.hip): tpt_device.h, the kernels' argument block and the launch functions;
// tpt_queue_layout.h, the path-queue kernel's LDS layout, the sizes the plan derives from it (tptLdsBytes, tptQueueLdsBytes,
// tptQueuePathsPerBlock, tptQueueGroupPairsInLds, tptQueueThreadsPerBlock) and the variant a launch takes (tptQueueVariant).
#pragma once
#include "../../include/tpt_hip.h"
#if defined(TPT_TEST_HOOKS)
#include "../../include/tpt_test_hooks.h" // unit-test / profiling entry points: the second build only (csrc/build.sh)
#endif
#include "../../include/tpt_test_api.h"
#include "tpt_device.h"
#include "tpt_queue_layout.h"
#include "tpt_scene.h"
#include "tpt_shard.h"
#include "tpt_stream_batch.h"
#include "tpt_animation.h"
#include <hip/hip_runtime.h>
#include <thread>
#include <rccl/rccl.h> // types and prototypes only: the library is dlopen()ed when tptCommInit is called
#include <chrono>
#include <dlfcn.h>
#include <map>
#include <stdio.h>
#include <stdlib.h>
#include <string>


namespace tpth {
using namespace tpt;

// What a trace launch leaves behind for the blend that follows it (now, or -- host path with look-ahead -- later).
const int kMaxBatch = 32; // frames per batched launch (tptDrawDeviceBatch): 6 bits in the path record, 32 lerp factors by value
static_assert(kMaxBatch == TPT_Q_VIEWS_MAX, "a batch's cameras, centres and ray counts have their places in the path-queue kernel's LDS");
struct TraceTicket {
    int slot = 0, nPixels = 0;
    bool pipelined = false, valid = false;
    float lerpFac = 0;
    const f4* colour = nullptr;
    int batch = 1;           // frames traced by the launch; their colour planes lie nPixels apart
    tptLerpTable lerp = {};  // batch > 1: each frame's lerp factor
    const f4* moments = nullptr; // a launch with moments: where it staged them (Context::dMoments; a clip launch's half), a plane per frame
    unsigned cutSerial = 0;      // a launch with a pool per frame: the serial its slot's cut word must carry (tpt_frame_pools.h); 0: none
    TraceTicket plane(int j) const // frame j of the launch, as a ticket of its own (a single-frame launch: plane 0 is itself)
    {
        TraceTicket t = *this;
        t.colour = colour + (size_t)j * (size_t)nPixels;
        if (batch > 1) t.lerpFac = lerp.v[j];
        t.batch = 1;
        return t;
    }
};

// Are a caller's calls consecutive frames of one (w, h, flags, configuration)?  n: how many in a row (0: not a continuation).
struct Streak {
    int frame = 0, w = 0, h = 0, n = 0;
    unsigned flags = 0;
    unsigned long long key = 0;
    int next(int frame_, int w_, int h_, unsigned flags_, unsigned long long key_)
    {
        n = frame_ == frame + 1 && w_ == w && h_ == h && flags_ == flags && key_ == key ? n + 1 : 0;
        frame = frame_; w = w_; h = h_; flags = flags_; key = key_;
        return n;
    }
};

// A launch traced ahead of the calls that will blend its frames, one frame per call, in frame order.  Its kind says who serves it:
//   AHEAD       a single frame traced ahead (tptSetHostLookahead): tptDraw and tptDrawDevice;
//   ROW_SERIAL  a batch in the reference's own seed mode (one launch of rows x frames lanes): tptDraw only;
//   STREAM      a batch of frames for a streaming caller (tptSetStreamBatching, tpt_stream_batch.h): tptDrawDevice only (and tptDrawSharded
//               through it); dropped when the caller waits (closeStream).
struct PendingLaunch {
    enum Kind { AHEAD, ROW_SERIAL, STREAM } kind = AHEAD;
    TraceTicket T;                      // T.batch frames: firstFrame, firstFrame + 1, ...
    int firstFrame = 0, next = 0;       // frame firstFrame + next is served next
    int w = 0, h = 0;                   // what the launch was traced for ...
    unsigned flags = 0;
    unsigned long long key = 0;         // ... and Context::configEpoch at the time: everything else a trace depends on
    unsigned long long* rays = nullptr; // per-frame ray counters: rays[j] for frame firstFrame + j
};
// The pending launches, oldest first (tpt_host_draw.cpp).  All of one kind: push refuses another kind, so a caller discards first.
// At most three AHEAD frames, two ROW_SERIAL batches (the one being served and the one after it) or one STREAM batch.  A launch's
// colour planes sit in frame slots that reserveSlotBuffers may neither shrink nor grow while the queue is not empty.
struct LaunchQueue {
    static const int kCap = 4;
    PendingLaunch e[kCap];
    int n = 0;
    bool empty() const { return n == 0; }
    bool holds(PendingLaunch::Kind kind) const { return n > 0 && e[0].kind == kind; }
    bool frontMatches(PendingLaunch::Kind kind, int frame, int w, int h, unsigned flags, unsigned long long key) const;
    void serveFront(bool wasOpen, TraceTicket& T, const unsigned long long*& rays);
    int push(const PendingLaunch& L);
    int discard();
    void closeStream();
    void cutFront(); // (a STREAM entry with unserved frames is about to be dropped: tell its launch, tpt_frame_pools.h)
};

struct Context {
    static const int kMaxOverlap = 16;              // frames in flight (trace streams, colour buffers, ...): one hardware queue each
    static const int kMaxSlots = 2 * kMaxOverlap;   // frame slots (colour buffers, events): a frame holds its slot from trace to blend
    static const int kOrderTables = kMaxSlots + 2;  // rotating chunk-order tables: more than frames in flight
    bool inited = false;
    int device = 0, numCUs = 0;
    int traceCUs = 0;      // what a trace launch can occupy (= numCUs)
    std::string deviceName, err;
    hipStream_t ownStream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    // host scene state (the reference's statics, Test.cpp:13-69)
    std::vector<SpherePOD> spheres;
    std::vector<MaterialPOD> mats;
    CameraSetup camSetup = defaultCameraSetup();
    CameraPOD cam;
    PackedScene packed;
    bool sceneDirty = true; // host arrays changed since last pack
    bool updated = false;   // tptUpdate ran at least once
    int updatedW = 0, updatedH = 0; // ... at this size (the aspect of g.cam; tptDrawDeviceViews builds its cameras for it)

    // device scene: a ring of scene sets, so that an animated scene (kFlagAnimate re-packs every frame,
    // Test.cpp:304-308,321-339) is uploaded asynchronously while earlier frames still read the older sets.
    // One device blob + one pinned host staging blob per set, laid out pairs | sph4 | invR | mats | lights.
    // A frame uploads at most one set, a set is reused after kSceneSets uploads, at most kMaxSlots frames
    // are in flight and the upload is stream-ordered behind the resolve of frame f - overlap: no kernel still reads the
    // set that is being overwritten.
    static const int kSceneSets = 2 * kMaxSlots;
    struct SceneSet {
        char* dev = nullptr;
        char* stage = nullptr; // pinned
        size_t cap = 0, bytes = 0;
        size_t offSph4 = 0, offInvR = 0, offMats = 0, offLights = 0;
        size_t offGPairs = 0, offGSph = 0, offGId = 0, offBSph = 0, offBId = 0; // grouped representation (large scenes)
        size_t offSPairs = 0;                                                    // ... and the super-group bounds over it
        int nSuperPairs = 0;
        size_t offAmat = 0; // matrix-core filter table (small scenes)
        int mxR1 = -1;
        size_t offGmat = 0; // the same for the group bounds of a grouped scene
        int gmxTiles = 0;
        int flags = 0;
        int nSpheres = 0, nPairs = 0, nLights = 0;
        int nGroups = 0, nGroupPairs = 0, nBig = 0;
        hipEvent_t evUploaded = nullptr;
        hipStream_t uploadStream = nullptr;
        bool copyEnqueued = false, copyDone = false;
    } sets[kSceneSets];
    int curSet = -1, pendingSet = -1;
    unsigned uploadSeq = 0;

    // run-time versions of the reference's compile-time switches
    int spp = 4;                     // DO_SAMPLES_PER_PIXEL, Config.h:22
    int config = CFG_LIGHT_SAMPLING; // DO_LIGHT_SAMPLING 1, DO_MITSUBA_COMPARE 0, Config.h:24-25
    float animateSmoothing = 0.9f;   // DO_ANIMATE_SMOOTHING, Config.h:23
    int seedMode = SEED_PER_PIXEL;
    int foldMode = FOLD_RECURSIVE;
    int allowGroups = 1; // hitSpheres variant 2 = two-phase, brute force even for large scenes
    int useMatrix = 1;   // phase 1 of HitSpheres on the matrix cores where it applies (hitSpheres variant 3 = VALU filter everywhere)
    int groupMatrix = 0; // grouped scenes: the groups' bounds on the matrix cores (hitSpheres variant 4; opt-in: DESIGN.md 2.2) instead of the two-level VALU filter
    int hs = HS_TWO_PHASE, persist = 3, ldsScene = -1; // persist 3 = path queues (falls back to 1 where they do not apply)
    int stripeRows = 0, numParts = 1, part = 0;
    int gridFill = 0;                           // env TPT_GRID_FILL: % of the resident slots all in-flight launches ask for
    int gridDiv = 0;                            // env TPT_GRID_DIV: launch resident/gridDiv workgroups per frame; 0 = adaptive
    unsigned long long oldestPending = 0;       // adaptive grid: oldest frame whose trace kernel may still be running
    int streamDepth = 1, prevInFlight = -1;     // adaptive grid: deepest pipeline the caller has built / in flight at the previous enqueue
    int depthOverride = 0;                      // > 0: frames that share the machine, known to the caller of enqueueTrace (tptDraw)
    int ldsStackLevels = 6;                     // recursive fold, lane-refill kernel: bounce-stack levels kept in LDS

    float* mirror = nullptr;                    // tptSetTileMirror: second destination of the resolve kernel
    unsigned long long* mirrorCounter = nullptr;
    unsigned* dWork = nullptr;
    unsigned long long* dRays = nullptr;    // the counter kernels add to (own or caller-provided)
    unsigned long long* dRaysOwn = nullptr;
    long long lastTotal = 0;

    f4* dStack[kMaxSlots] = {};         // recursive fold: global bounce stacks / spill levels (one per trace stream: the first kMaxOverlap entries)
    size_t stackCap = 0, colourCap = 0; // bytes per slot; all reserved slots have the same capacities
    int slotsReserved = 0;              // slots [0, slotsReserved) hold buffers of those capacities
    int smallStreak = 0;                // consecutive launches that needed a quarter of the reserved colour slot or less (reserveSlotBuffers)
    int slotReservations = 0;           // how often the slot buffers were (re-)allocated (tptGetPipelineInfo)
    // cost-ordered chunk distribution (persistent kernel)
    unsigned* dChunkCost = nullptr;
    unsigned* dChunkOrder[kOrderTables] = {};
    unsigned* dChunkSnap[kMaxOverlap] = {}; // per trace stream: cost snapshot of the sort kernel
    int chunkCap = 0, chunkCount = 0; // chunkCount: numChunks the statistics belong to
    int costOrder = 1;                // expensive tiles first (lane-refill kernel)
    hipEvent_t evOrder = nullptr;     // the last sort of an order table (recorded on the stream that ran it)
    hipStream_t orderStream = nullptr;
    unsigned long long orderSeq = 0;
    int lastOrderTable = 0;
    float* dFrame = nullptr; // device tile behind the host-pointer DrawTest
    // ---- host-pointer path (tptDraw / DrawTest)
    hipStream_t hostStream2 = nullptr;  // second stream of the banded upload / blend / download (full-duplex PCIe)
    hipEvent_t evBand = nullptr, evBandEnd = nullptr;
    int hostTrust = 0;                  // tptSetHostBufferMode(1): only DrawTest writes the backbuffer -> never re-upload it
    const float* tileSrc = nullptr;     // which host buffer (and size) the device tile g.dFrame currently mirrors
    int tileW = 0, tileH = 0;
    int lookahead = 2;                  // tptSetHostLookahead: frames traced ahead of the caller's next DrawTest
    LaunchQueue pending;                // launches traced ahead of the calls that will blend their frames
    struct HostCaller {                 // tptDraw: are the calls consecutive frames of one configuration?  (gates the row-serial batches)
        Streak seq;
        // a configuration whose batched launch was refused (frame too large for a batch, not enough device memory): served frame
        // by frame from then on instead of failing (or retrying the reservation) on every call
        int refusedW = 0, refusedH = 0;
        unsigned long long refusedKey = 0;
    } hostCaller;
    static const int kStreamBatchMax = 8, kStreamRing = 64;
    unsigned long long streamBatches = 0;       // stream batches launched (index into their ring of ray counters)
    int streamRun = 0, streamNext = -1;         // stream batches launched back to back before the newest / the frame that continues it (-1: none)
    int streamBatch = 1;                        // on by default since round 4; tptSetStreamBatching(0) / env TPT_STREAM_BATCH=0 turn it off
    // The cut words of the launches with a pool per frame (tpt_frame_pools.h), one per frame slot, in PINNED HOST memory: the host
    // writes a word while the launch it is meant for runs, without a stream or a hardware queue -- with few queues a copy or a
    // one-thread kernel can sit behind the very launch it is meant to cut.  A slot's word is zeroed when a launch is enqueued on it
    // (stream-ordered behind the slot's previous launch by then: nobody reads the old word any more) and written at most once after.
    unsigned* hCut = nullptr;
    unsigned cutSerial = 0;                     // serial of the newest such launch (24 bits, never 0 once used)
    int cutPreset = 0;                          // hooks build, tptTestPresetStreamCut: the next such launch starts with this `keep` in its word
    unsigned long long* lastStreamRays = nullptr; // per-frame ray counters of the newest STREAM launch, and its frames (hooks build's read-back)
    int lastStreamFrames = 0;
    // tptDrawDevice: is the caller synchronous (the previous frame's blend has completed by the time the next call arrives)
    // and are its calls consecutive frames of one configuration?  Then the next frames are traced ahead for it too.
    struct DeviceCaller {
        int lastSlot = -1, syncStreak = 0;
        Streak seq;
    } devCaller;
    // tptDrawDeviceViews / tptDrawDeviceAnimation: per frame slot, the launch's BatchTable (device table the kernel stages in LDS, pinned
    // host staging) and its frames' ray counters.  Per slot, because up to kMaxSlots launches are in flight: the table of one call must
    // not be overwritten while an earlier launch still reads it (the upload is stream-ordered behind the slot's previous blend, like its
    // colour buffer).  The moving centres of an animation batch (2 x 16 B per frame) take the room of its first 12 cameras; a launch
    // that takes both tables (tptDrawDeviceCameraClip) has its centres behind the whole camera table, and so has a launch with the
    // caller's centres (tptDrawDeviceKeyframeClip: TPT_Q_KEYS_MAX x 16 B per frame).
    struct ViewSlot {
        CameraPOD* dev = nullptr;       // [kMaxBatch] cameras (or [kMaxBatch][2] centres), then [kMaxBatch][2 or TPT_Q_KEYS_MAX] centres beside cameras
        unsigned long long* rays = nullptr; // [kMaxBatch] rays of each view
        CameraPOD* stage = nullptr;     // pinned, the same layout
        hipEvent_t evUploaded = nullptr;
        bool copyEnqueued = false;
    } views[kMaxSlots];
    char* dViews = nullptr;             // one allocation behind every slot's dev + rays (made by the first views call)
    CameraPOD* hViewsStage = nullptr;   // pinned, behind every slot's stage
    // tptDrawDeviceAov: the per-path first-hit sums (KernelArgs::aovSums, 2 x f4 per path column of the largest grid seen), made by the
    // first AOV call.  One buffer serves every AOV launch: each waits for the context stream (evAov), and the context stream waits for
    // each, so two of them never run at the same time.
    f4* dAovSums = nullptr;
    size_t aovSumsBytes = 0;
    hipEvent_t evAov = nullptr;         // recorded on the context stream by an AOV call; its trace stream waits for it
    // tptDrawDeviceMoments: the frame's moments plane (KernelArgs::momentsOut, [nLocalRows][w] f4 of the largest frame seen), written
    // by the moments kernel and blended into the caller's plane on the context stream; AOV launches run one at a time (evAov), so
    // one plane serves them all.  Its sums are a third f4 per path column of dAovSums.
    f4* dMoments = nullptr;
    size_t momentsBytes = 0;
    // tptDrawDeviceAnimationMoments: the launches of one call alternate between two halves of dAovSums and dMoments (both twice the
    // launch's need), so launch k + 1 waits only for the blends of launch k - 1, whose halves it takes over, and is traced beside the
    // blends of launch k.  evClip[h]: recorded on the context stream when a launch on half h ^ 1 is enqueued, i.e. behind the blends of
    // the previous launch on half h.  The first launch of a call waits for the whole context stream, as every other AOV launch does.
    hipEvent_t evClip[2] = {nullptr, nullptr};
    unsigned clipSeq = 0;
    // tptDrawDeviceBatchMoments: where a launch's frames leave their albedo and normal / depth planes for the fold behind it (the caller's
    // planes are running means, not per-frame buffers).  Two halves of guideStageBytes / 2, taken by the launches as they take the halves of
    // dMoments; in a half the albedo planes of the launch's n frames, then its normal / depth planes (a plane the caller left out takes no
    // room).  Grown on demand (after a drain), kept until tptShutdown.
    f4* dGuideStage = nullptr;
    size_t guideStageBytes = 0;
    // tptDrawDeviceKeyframeClip's object planes: one {centre, r^2} array per frame of a LAUNCH (SceneView::sph4's records, the moved spheres
    // at the frame's centres) for tptObjectPlaneKernel, copied on the context stream out of a pinned twin.  Two halves of keySphBytes each,
    // taken in turn (keySphSeq), so that the host fills one launch's arrays while the previous launch's copy is still queued: at most
    // 2 x 32 frames x count x 16 B of device memory and as much pinned, whatever the call's length; grown on demand (after a drain), kept
    // until tptShutdown.  evKeySph[h]: half h's last copy has left the host (the launch after the next waits for it before it refills h).
    f4* dKeySph = nullptr;
    f4* hKeySph = nullptr;
    size_t keySphBytes = 0;
    hipEvent_t evKeySph[2] = {nullptr, nullptr};
    bool keySphCopied[2] = {false, false};
    unsigned keySphSeq = 0;
    // tptDenoiseDevice: the plane the a-trous iterations ping-pong through beside the caller's output ([h][w] f4 of the largest frame
    // denoised so far), made by the first call that iterates more than once, grown when a later one needs more, freed by tptShutdown.
    // Only the context stream uses it, so stream order alone keeps one call's iterations from another's.
    f4* dDenoise = nullptr;
    size_t denoiseBytes = 0;
    // tptDenoiseClipDevice: its staging (include/tpt_hip.h states the layout: per chunk frame the temporal outputs the filter reads and
    // the ping-pong plane, and the planes that carry the history from frame to frame), made by the first call that needs it, grown when
    // a later one needs more, freed by tptShutdown.  Only the context stream uses it.
    f4* dClipStage = nullptr;
    size_t clipStageBytes = 0;
    // tptMotionVectorsDevice: the table of per-frame camera constants its kernel reads (one tptFlowConsts per frame of a call), copied on the
    // context stream out of a pinned twin.  The device table is single: its copy and the launches that read it are ordered on the
    // context stream, the only one that uses it.  The pinned twin has two halves of flowConstsBytes each, taken in turn (flowSeq) as
    // hKeySph's are: a call fills its half while the previous call's copy may still be queued on the other, so that copy reads what its
    // own call wrote.  evFlow[h]: half h's last copy has left the host (the call after the next waits for it before it refills h).
    // Grown on demand (after a drain of the context stream), kept until tptShutdown.
    tptFlowConsts* dFlowConsts = nullptr;
    tptFlowConsts* hFlowConsts = nullptr;
    size_t flowConstsBytes = 0;
    hipEvent_t evFlow[2] = {nullptr, nullptr};
    bool flowCopied[2] = {false, false};
    unsigned flowSeq = 0;
    // tptTraceRaysDevice: the launch's own bounce-stack spill (KernelArgs::stackBuf, a column per thread of the largest grid seen) and
    // its own counter block -- 16 words as KernelArgs::work, then the u64 the rays are counted into when the caller gives no word.
    // Made by the first call, the spill grown on demand (after a drain of the context stream), zeroed when allocated, kept until
    // tptShutdown.  Only the context stream uses them.
    f4* dRayStack = nullptr;
    size_t rayStackBytes = 0;
    unsigned* dRayWork = nullptr;
    // tptDrawDeviceLens: the draw's own colour plane (KernelArgs::frameColour, [h][w] f4 of the largest image seen), grown like the
    // spill above; the launch shares that spill and counter block with the ray calls -- all of them run on the context stream.
    f4* dLensColour = nullptr;
    size_t lensColourBytes = 0;
    long long aheadHits = 0;            // frames that were found traced ahead when their call arrived (tptGetLookaheadHits)
    // per-frame ray counters of the pending launches, one allocation: [kMaxSlots] AHEAD frames (indexed by the frame's sequence number
    // at enqueue), [2][kMaxBatch] ROW_SERIAL batches (two banks, alternating), [kStreamRing][kStreamBatchMax] STREAM batches (a ring)
    unsigned long long *dRaysAhead = nullptr, *dRaysBatch = nullptr, *dRaysStream = nullptr;
    unsigned long long configEpoch = 1;       // bumped by every call that changes what a frame looks like

    // ---- multi-GPU inside the library (one process per GPU, RCCL): tptCommInit .. tptDrawSharded
    struct Shard {
        static const int kRing = 4;     // send snapshots: a gather may trail the renderer by this many frames
        void* lib = nullptr;            // librccl, loaded on first use (no link-time dependency: a single-GPU host never needs it)
        ncclComm_t comm = nullptr;
        bool active = false, loopback = false; // loopback: rank 0 of nRanks with a device copy in place of the gather (tptCommInitLoopback)
        int nRanks = 0, rank = 0, stripeRows = 8;
        int w = 0, h = 0, padRows = 0;
        hipStream_t commStream = nullptr;
        float* tile = nullptr;          // this rank's resident accumulation tile [localRows][w] f4
        float* send[kRing] = {};        // snapshots [padRows + 1][w] f4: blended tile + the row carrying the ray counter
        float* gathered = nullptr;      // rank 0: [nRanks][padRows + 1][w] f4
        hipEvent_t evSnap[kRing] = {}, evSent[kRing] = {};
        bool sentRecorded[kRing] = {};
        unsigned long long frames = 0;  // exchanges enqueued (index into the snapshot ring)
        // Exchange interval (tptSetShardExchangeInterval): with small tiles the chain behind a frame -- trace launch, blend + snapshot,
        // gather, de-interleave: four dispatches, each a ~40 us quantum beside a machine full of trace workgroups -- bounds the frame
        // rate, not the arithmetic.  tptDrawSharded then DEFERS such frames: k consecutive frames of one configuration are
        // issued as one tptDrawShardedBatch (one trace launch, one blend, one exchange) when the k-th arrives, when anything about the
        // configuration is about to change, or when the caller waits (tptShardedFinish, tptSynchronize, tptRayCounterRead).
        int exchangeEvery = 0;          // 0 = automatic (1 for tiles of >= 2.4 M samples per frame, 2 / 4 / 8 below), else the host's choice
        int pendCount = 0, pendFirst = 0, pendW = 0, pendH = 0; // frames accepted but not issued yet: [pendFirst, pendFirst + pendCount)
        unsigned pendFlags = 0;
        float pendTime = 0.0f;
        float* lastImage = nullptr;     // the root's image pointer of the most recent call (a deferred batch writes there)
        decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
        decltype(&ncclCommInitRank) CommInitRank = nullptr;
        decltype(&ncclCommDestroy) CommDestroy = nullptr;
        decltype(&ncclGather) Gather = nullptr;
        decltype(&ncclCommCount) CommCount = nullptr;
        decltype(&ncclCommUserRank) CommUserRank = nullptr;
        decltype(&ncclGetErrorString) GetErrorString = nullptr;
    } shard;
    size_t frameCap = 0;

    // frame pipelining: trace kernels of consecutive frames run on alternating internal streams and write
    // their own per-frame colour buffer; the (ordered) resolve kernels run on g.stream
    int overlap = 16;
    hipStream_t traceStream[kMaxOverlap] = {};
    hipEvent_t evTrace[kMaxSlots] = {}, evResolve[kMaxSlots] = {};
    bool resolveRecorded[kMaxSlots] = {};
    f4* dColour[kMaxSlots] = {};
    int hwQueues = 0, overlapCap = kMaxOverlap; // measured at tptInitialize (probeHardwareQueues)
    int slotFactor = 2;                         // colour slots per trace stream (enqueueTrace)
    // tail helpers (tpt_device.h): second grids for the launches still in flight when the caller blocks
    hipEvent_t evPre[kMaxSlots] = {};           // recorded on the slot's stream right before its trace launch: what a helper grid has to wait for
    struct HelperRec {
        KernelArgs a;
        bool ldsScene = false, valid = false, helped = false;
        hipStream_t ts = nullptr;
        int blocks = 0, maxBlocks = 0;
        size_t lds = 0;
    } hrec[kMaxSlots];
    unsigned launchGen = 0;
    int helpersOn = 1;                          // env TPT_TAIL_HELPERS=0: no second grids (the launches still close their counter blocks)
    static const int kHelperPct = 3;            // a helper workgroup joins only while this % of its launch's pool is unclaimed
    static const int kHelperMax = 8;            // launches helped per wait (the newest half of those in flight; sweep: profiles/r05/r05_run2.log)
    long long helperLaunches = 0;
    int hostPace = 1;                           // env TPT_HOST_PACE=0: let the host run ahead of the pipeline (enqueueTrace)
    int shardOverlapCap = kMaxOverlap;          // 8 while the frame is sharded over more than two parts (tptSetRowShard)
    unsigned long long frameSeq = 0;

    // per-launch timing of the trace kernel: hipEvent pairs on the stream each launch goes to
    bool kernelTiming = false;
    std::vector<hipEvent_t> ktStart, ktStop;
    size_t ktUsed = 0;

    std::map<int, int> occCache;
    int lastBlocksPerCU = 0, lastLds = 0, lastGrid = 0;
};

extern Context g;

// Launches made inside the scope share the machine with d frames (this one and the ones traced ahead), not with a deep device-path
// pipeline (sizeGrid).
struct DepthScope {
    explicit DepthScope(int d) { g.depthOverride = d; }
    ~DepthScope() { g.depthOverride = 0; }
};

// Events that order work between the streams of this context (trace -> resolve -> next use of a colour buffer, scene
// upload -> trace, order-table sort -> trace).  Plain events: hipEventDisableSystemFence was measured (no gain: the
// fences are not what bounds small frames) and dropped again -- a dependency between kernels on different streams is
// exactly where the release/acquire of an event matters, and one unexplained mismatch in a full test run was not worth it.
const unsigned kOrderingEvent = hipEventDisableTiming;
const unsigned kTimingEvent = hipEventDefault;

inline int fail(const std::string& what)
{
    g.err = what;
    return -1;
}
inline int hipFail(hipError_t e, const char* what)
{
    g.err = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError(); // clear the runtime's sticky error: the next launch's hipGetLastError() must not report this one again
    return -2;
}
// A request the pipeline declines -- too large for a batch, not enough device memory, frame slots still held by frames traced
// ahead -- as opposed to something that went wrong: callers that can retry with less (the row-serial batches of tptDraw) do so
// on this code only and pass every other error on.
const int kRefused = -4;
inline int refuse(const std::string& what)
{
    g.err = what;
    return kRefused;
}
// Does the buffer at p share a byte with one of `others` (null ones skipped)?  All are `bytes` long.
inline bool overlapsAny(const void* p, std::initializer_list<const void*> others, uintptr_t bytes)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    for (const void* other : others) {
        const uintptr_t o = reinterpret_cast<uintptr_t>(other);
        if (other && a < o + bytes && o < a + bytes) return true;
    }
    return false;
}
#define HIPCHK(x)                                   \
    do {                                            \
        hipError_t _e = (x);                        \
        if (_e != hipSuccess) return hipFail(_e, #x); \
    } while (0)

// tpt_host.cpp
int localRows(int h);
int localToGlobal(int ly);
int stageScene();
Context::SceneSet* activeSet();
SceneView deviceView();
int enqueueSceneUpload(hipStream_t ts);
int framesInFlight(int nOverlap);
int uploadBackbuffer(const float* backbuffer, int w, int h);
int requireInit();
int drainPipeline();
int effectiveOverlap();
// tpt_host_pipeline.cpp
// What differs between the frames of one launch besides their seeds (tptDrawDeviceViews, tptDrawDeviceAnimation).  The table is copied
// to the slot's device table on the frame's stream, and every frame counts its rays into the slot's counters (Context::ViewSlot).  With
// neither table the launch is the plain (batched) kernel with those per-frame counters; with both (and the planes of a clip) it is
// tptCameraClipKernel: a camera and the centres per frame, every frame with its own seeds.
struct BatchTable {
    const CameraPOD* cams = nullptr; // [batch] cameras, every frame with the seeds of frameCount: tptTraceViewsKernel
    const f4* centres = nullptr;     // [batch][2] {x, y, z, -} of spheres 1 and 8 (Test.cpp:304-308): tptTraceAnimationKernel
    // tptDrawDeviceKeyframeClip (with cams and a clip's planes, without centres): [batch][TPT_Q_KEYS_MAX] {x, y, z, -} of the keyCount spheres
    // of keyMask (sphere i at bit 63 - i) in ascending index, unused entries zero: tptKeyframeKernel
    const f4* keyCentres = nullptr;
    unsigned long long keyMask = 0;
    int keyCount = 0;
};
// The caller's first-hit planes of a single frame (tptDrawDeviceAov): device [h][w] f4 each, either may be null (not both); the launch
// is tptTraceAovKernel, ordered behind everything enqueued on the context stream so far.
struct AovPlanes {
    f4* albedo = nullptr;
    f4* normalDepth = nullptr;
    bool moments = false; // tptDrawDeviceMoments: tptTraceMomentsKernel, into Context::dMoments
    bool continues = false; // tptDrawDeviceAnimationMoments: a later launch of the call (Context::evClip)
    const int32_t* sampleCounts = nullptr; // tptDrawDeviceAdaptive (with moments): the caller's count per pixel, tptTraceAdaptiveKernel
    const char* entry = nullptr; // whose launch this is, for a refusal, where the tables and planes do not say it (tptDrawDeviceBatchMoments)
};
int enqueueTrace(int frameCount, int w, int h, unsigned testFlags, unsigned long long* frameRays, TraceTicket& T, int batch = 1, int rayStride = 0,
                 const BatchTable* table = nullptr, const AovPlanes* aov = nullptr);
int enqueueResolve(const TraceTicket& T, float* deviceTile, const unsigned long long* frameRays);
size_t laneRefillLds(KernelArgs& a, bool& ldsScene); // (the lane-refill kernel's plan: chooseKernel, tptTraceRaysDevice, tptDrawDeviceLens)
bool fitsCuLds(size_t lds);
int laneRefillOccupancy(bool ldsScene, size_t lds);
int syncAllStreams();
int launchTailHelpers();
int flushShardDeferred(); // tpt_host_shard.cpp: issue the sharded frames tptDrawSharded has accepted but deferred (none: nothing happens)
// tpt_host_draw.cpp (and LaunchQueue)
int traceAhead(int frameCount, int w, int h, unsigned testFlags, unsigned long long key, int want);

} // namespace tpth
