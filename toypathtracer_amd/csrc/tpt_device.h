// tpt_device.h -- kernel argument block shared by tpt_kernels.hip (device) and tpt_host.cpp (host), and the launch functions.  The LDS
// layout of the path-queue kernel, the sizes derived from it (tptLdsBytes, tptQueueLdsBytes, tptQueuePathsPerBlock, ...) and the
// variant a launch takes (tptQueueVariant): tpt_queue_layout.h, which includes this header.
#pragma once
#include "tpt_trace.h"
#include "tpt_frame_pools.h"

#ifndef TPT_BLOCK
#define TPT_BLOCK 64         // threads per workgroup: one wave, so a finished wave frees its LDS/VGPRs at once
#endif
#define TPT_CHUNK_PIXELS 256 // pixels a persistent wave pulls per atomic (4 tiles of 8x8)
// Tail helpers: when the caller BLOCKS (tptSynchronize, tptTimerEnd, tptShardedFinish) while path-queue launches are still in flight,
// the newest of them get a second grid of workgroups that takes chunks from the same pool -- the last launches of a burst otherwise
// finish on a half-empty machine (the anatomy of the driver's command: 20 frames 47.5 -> 50 k Mray/s).  The launch's counter
// block (KernelArgs::work) carries the hand-shake: [2] helper workgroups registered, [3] serial of the last launch that CLOSED on this
// block.  A helper registers, then looks: closed (or a later launch's block) -> it leaves without touching anything; the launch's
// last wave closes, then waits for the registered helpers before it re-arms the counters and lets the kernel end -- so "launch
// complete" still means "frame complete" for the ordered blend behind it.  Model-checked (tests/test_helper_handshake_model.py), run
// under the emulated runtime's schedules (tests/test_host_logic.py); env TPT_TAIL_HELPERS=0 switches the second grids off.

namespace tpt {

struct KernelArgs {
    SceneView scene;
    FrameConsts fc;
    f4* frameColour;   // device, [nLocalRows][width] f4: THIS frame's colour per pixel (xyz; w unused), written once
                       // per pixel by the trace kernel and blended into the accumulation tile by tptResolveKernel
    // row sharding: local row ly <-> image row (ly / stripeRows) * stripeStride + stripeOffset + ly % stripeRows
    int nLocalRows, stripeRows, stripeStride, stripeOffset;
    int tilesX;     // 8x8 tiles per row of tiles
    int numItems;   // pixels incl. tile padding (PER_PIXEL) or rows (ROW_SERIAL)
    int numChunks, chunkSize;
    // Batched launch (path-queue kernel, tptDrawDeviceBatch): the launch traces batchFrames consecutive frames of the same
    // scene and camera -- chunk c belongs to frame fc.frame + c / chunksPerFrame -- and writes their colour planes one
    // after the other into frameColour (framePlane pixels apart).  1 = a single frame (chunksPerFrame == numChunks).
    int batchFrames, chunksPerFrame, framePlane;
    unsigned totalWaves;
    int laneCap;    // lane-refill kernel: lanes of a wave that take work items (64; fewer for row-serial seeds, whose items are whole rows)
    int noRefill;   // lane-refill kernel: 1 = a wave takes 64 pixels and every lane keeps ITS pixel until all 64 are done (the north_star's one-thread-per-pixel shape, tptSetKernelVariant persistent 0: an A/B instantiation); 0 = idle lanes are re-filled at once
    // FOLD_RECURSIVE bounce stack: the first ldsStackLevels levels live in LDS (per thread), deeper ones in
    // stackBuf [TPT_MAX_DEPTH - ldsStackLevels][stackStride] (global, one column per thread of the launch).
    f4* stackBuf;
    int stackStride;
    int ldsStackLevels;
    f4* pathBuf;                     // path-queue kernel: cold path state [workgroups][paths][4] f4 (global, L2-resident)
    // cost-ordered work distribution (persistent kernel): chunk c of the queue is chunkOrder[c]; every finished pixel
    // adds its ray count to chunkCost[chunk] (running sum over frames); tptChunkOrderKernel re-sorts, expensive first
    const unsigned* chunkOrder;      // may be null: image order
    unsigned* chunkCost;             // may be null
    int chunkShift;                  // log2(chunkSize)
    unsigned* work;                  // [0] next chunk, [1] finished waves (persistent variants), [2] [3] tail helpers, [4..11] next chunk of frame j (framePools)
    unsigned long long* rayCounter;  // monotonic total of rays traced by this context
    int rayCounterStride;            // batched row-serial launch: frame j of the batch counts into rayCounter[j * stride] (0: one counter)
    unsigned gen;                    // tail helpers: serial of this launch (1, 2, ...; 0: takes no helpers)
    int helperBase;                  // 0: the launch itself; > 0: its helper grid, whose workgroup b plays workgroup helperBase + b (stack columns)
    int helperPct;                   // a helper workgroup joins only while at least this % of the pool is unclaimed
    int ldsGroupPairs;               // grouped scenes, path-queue kernel, the two-level bounds filter: > 0 pair records of the groups' bounds staged in
                                     // LDS (whole super-groups), 0 = read them from global memory (too many for the LDS area), < 0 = flat filter over all groups
    // Several views in one launch (tptDrawDeviceViews): batchFrames cameras, one per frame of the batch, in device memory; the launch
    // takes tptTraceViewsKernel, which stages them in LDS and seeds every view with fc.frame.  Null for every other launch.
    const CameraPOD* viewCams = nullptr;
    // Frames of an animated scene in one launch (tptDrawDeviceAnimation): batchFrames x {sphere 1, sphere 8} centres {x, y, z, -}, one
    // pair per frame of the batch, in device memory; the launch takes tptTraceAnimationKernel, which stages them in LDS and reads the
    // path's frame's centres wherever the exact data of sphere 1 or 8 is used.  Null for every other launch.
    const f4* moveCentres = nullptr;
    // A single frame with its first-hit planes (tptDrawDeviceAov): per path two f4 of sums {albedo, coverage} {normal, t}, at
    // aovSums[2 x column], the column numbered like the bounce stack's (workgroup + helperBase, then path); the launch takes
    // tptTraceAovKernel, which stores the means into aovAlbedo / aovNormalDepth ([nLocalRows][width] f4 each; either may be null).
    // aovSums is null for every other launch.
    f4* aovSums = nullptr;
    f4* aovAlbedo = nullptr;
    f4* aovNormalDepth = nullptr;
    // ... and its luminance moments (tptDrawDeviceMoments): a third f4 of sums per path, aovSums[3 x column .. + 2], and the frame's
    // means {l, l^2, 0, 0} stored into momentsOut ([nLocalRows][width] f4); the launch takes tptTraceMomentsKernel.  Null otherwise.
    f4* momentsOut = nullptr;
    // The frames of an animated clip with their planes (tptDrawDeviceAnimationMoments: moveCentres and aovSums both given, the launch
    // takes tptTraceClipKernel): frame j of the batch stores its first-hit planes at aovAlbedo / aovNormalDepth + j * aovPlane pixels (the
    // caller's per-frame buffers) and its moments at momentsOut + j * framePlane (staging, beside its colour plane).
    int aovPlane = 0;
    // ... with a camera per frame (tptDrawDeviceCameraClip: viewCams and moveCentres both given, with aovSums and momentsOut; the launch
    // takes tptCameraClipKernel): frame j reads camera viewCams[j] where a sample starts, its seeds stay those of frame fc.frame + j.
    // A single frame with its planes and moments whose pixels take a sample count each (tptDrawDeviceAdaptive): [nLocalRows][width]
    // int32 in device memory, read where a lane claims a pixel and clamped there to 0 .. 2047 (0: the pixel is not traced, nothing of it
    // is stored); fc.spp and fc.invSpp play no part.  The launch takes tptTraceAdaptiveKernel.  Null for every other launch.
    const int32_t* sampleCounts = nullptr;
    // The frames of a clip whose spheres the CALLER moves, with their planes and a camera per frame (tptDrawDeviceKeyframeClip: keyCentres
    // given with viewCams, aovSums and momentsOut, moveCentres null; the launch takes tptKeyframeKernel): batchFrames x TPT_Q_KEYS_MAX
    // centres {x, y, z, -} in device memory, frame j's at keyCentres[TPT_Q_KEYS_MAX x j ..], one per moved sphere in ascending sphere
    // index (unused entries zero).  keyMask: the moved spheres, sphere i (< 64) at bit 63 - i, keyCount (<= TPT_Q_KEYS_MAX) of them;
    // launch-uniform.  Everything else is the camera clip's.  Null / 0 for every other launch.
    const f4* keyCentres = nullptr;
    unsigned long long keyMask = 0;
    int keyCount = 0;
    // A pool of chunks per frame of a plain batched launch (tpt_frame_pools.h): 0 = one shared pool, work[0] counting to numChunks;
    // n = batchFrames = n pools, work[4 + j] counting frame j's chunks to chunksPerFrame, and workgroup b serves frame
    // framePoolOfBlock(b, n, grid) alone; the launch takes tptFramePoolsKernel.  0 for every other launch.
    int framePools = 0;
    // ... and the launch's cut word (tpt_frame_pools.h): one word of the context's array in pinned host memory, read by the pools kernel
    // where a workgroup starts, and the serial a word must carry to mean this launch.  Null / 0 for
    // every other launch.
    const unsigned* cutWord = nullptr;
    unsigned cutSerial = 0;
    // The caller's rays instead of a camera's (tptTraceRaysDevice; the lane-refill kernel through tptLaunchTraceRays): numItems records of
    // two f4 in device memory, {origin, seed bits} {direction, -}; work item i is ray i, one path each (fc: spp 1, per-pixel seeds,
    // width 1).  rayRadiance ([numItems] f4, may be null: the paths end after their first HitWorld) receives {colour, HitWorld calls of
    // the path}, rayHits ([numItems][2] f4, may be null) the first hit {pos, t} {normal, bits(id)}.  No frameColour, no chunk order or
    // cost, one frame.  Null for every other launch.
    const f4* rays = nullptr;
    f4* rayRadiance = nullptr;
    f4* rayHits = nullptr;
    // A lens instead of the camera (tptDrawDeviceLens; the lane-refill kernel through tptLaunchTraceLens): every sample of the launch
    // starts at lensGetRay(lens, u, v) where it would start at cameraGetRay(fc.cam, ..); everything else is the pixel mode.  At the
    // tail, so that no other field moves; read by the kernel only where a sample starts.  kind 0 for every other launch.
    LensPOD lens = LensPOD{};
};

} // namespace tpt

hipError_t tptLaunchTrace(const tpt::KernelArgs& a, int hs, int fold, bool ldsScene, int blocks, size_t lds, hipStream_t stream);
int tptTraceOccupancy(int hs, int fold, bool ldsScene, size_t lds);
// tptTraceRaysDevice: tptLaunchTrace's kernels with a.rays given (the ray source of the lane-refill kernel; no kernel of its own).  Weak
// for the same reason as tptLaunchDenoise below.
__attribute__((weak)) hipError_t tptLaunchTraceRays(const tpt::KernelArgs& a, int hs, int fold, bool ldsScene, int blocks, size_t lds,
                                                    hipStream_t stream);
// tptDrawDeviceLens: tptLaunchTrace's kernels with a.lens given (a mode of the lane-refill kernel; no kernel of its own).  Weak for the
// same reason as tptLaunchDenoise below.
__attribute__((weak)) hipError_t tptLaunchTraceLens(const tpt::KernelArgs& a, int hs, int fold, bool ldsScene, int blocks, size_t lds,
                                                    hipStream_t stream);
hipError_t tptLaunchTraceQueue(const tpt::KernelArgs& a, bool ldsScene, int blocks, size_t lds, hipStream_t stream);
int tptQueueMatrixFilter();
int tptQueueGroupMatrixBounds(); // 1: this build carries the groups' bounds on the matrix cores (hooks build only)
hipError_t tptLaunchDisplay(const float* tile, unsigned char* rgba, int width, int height, hipStream_t stream);
// tptDenoiseDevice: `iterations` launches of the a-trous kernel, ping-ponging between out and scratch (both [h][w] f4, neither
// overlapping an input) so that the last one writes out; albedo / normalDepth may be null (ic, in, id: the first iteration's
// inverse squared sigmas).  Weak: the host runtime is also linked against the CPU suite's emulated kernels, which have no
// a-trous kernel; tptDenoiseDevice fails there instead of the library failing to load.
__attribute__((weak)) hipError_t tptLaunchDenoise(const float* colour, const float* albedo, const float* normalDepth, float* out,
                                                  float* scratch, int width, int height, int iterations, float ic, float in, float id,
                                                  bool demodulate, hipStream_t stream);
// tptDenoiseDeviceVariance: `iterations` launches of the variance-guided a-trous kernel, ping-ponging between out and scratch as
// tptLaunchDenoise does; albedo / normalDepth may be null (sl2 = sigmaLuminance^2; in, id: the inverse squared guide sigmas).  Weak for
// the same reason as tptLaunchDenoise.
__attribute__((weak)) hipError_t tptLaunchDenoiseVariance(const float* colour, const float* albedo, const float* normalDepth,
                                                          const float* moments, float* out, float* scratch, int width, int height,
                                                          int iterations, float samples, float sl2, float in, float id, bool demodulate,
                                                          hipStream_t stream);
// tptDenoiseClipDevice: tptLaunchDenoiseVariance for `frames` (1..32) frames at once, one launch per iteration.  Every pointer is the
// first of `frames` consecutive [h][w] f4 planes -- colour, moments, out and scratch always, albedo / normalDepth when given -- and frame
// j is filtered exactly as tptLaunchDenoiseVariance filters plane j of each.  Weak for the same reason as tptLaunchDenoise.
__attribute__((weak)) hipError_t tptLaunchFramesAtrous(const float* colour, const float* albedo, const float* normalDepth,
                                                       const float* moments, float* out, float* scratch, int width, int height, int frames,
                                                       int iterations, float samples, float sl2, float in, float id, bool demodulate,
                                                       hipStream_t stream);
// tptTemporalAccumulateDevice: what the kernel needs of the two cameras and the call, made on the host in the order include/tpt_hip.h
// states (host and device are built with -ffp-contract=off); by value in the kernel arguments.
struct tptTemporalConsts {
    float o[3], ll[3], H[3], V[3];          // this frame's camera
    float po[3], pa[3], pw[3], pH[3], pV[3]; // the previous camera: origin, a = ll' - o', ww, horizontal, vertical
    float pf, phh, pvv;                      // f = -dot(a, w'), dot(H', H'), dot(V', V')
    float maxHistory, depthTol, normalTol, coverageTol;
};
// One launch of the temporal accumulation kernel; the four prev planes are all null (first frame: k's previous camera is unused) or
// all given.  Weak for the same reason as tptLaunchDenoise.
__attribute__((weak)) hipError_t tptLaunchTemporal(const float* colour, const float* albedo, const float* normalDepth, const float* moments,
                                                   const float* prevColour, const float* prevAlbedo, const float* prevNormalDepth,
                                                   const float* prevMoments, float* outColour, float* outAlbedo, float* outMoments,
                                                   float* outVariance, int width, int height, const tptTemporalConsts& k,
                                                   hipStream_t stream);
// tptObjectPlaneDevice: one frame's camera {origin, lowerLeftCorner, horizontal, vertical} and where spheres 1 and 8 stand in that
// frame (the scene's own centres when nothing moves; unused entries for scenes without such a sphere); by value in the kernel arguments.
struct tptObjectPlaneConsts {
    float o[3], ll[3], H[3], V[3];
    float c1[3], c8[3];
};
// One launch of the object-plane kernel: `out` ([h][w] int32) receives the index of the first sphere the ray through each pixel's
// centre meets, -1 for none; sph4 = SceneView::sph4 of nSpheres records in device memory.  Weak for the same reason as tptLaunchDenoise.
__attribute__((weak)) hipError_t tptLaunchObjectPlane(const tpt::f4* sph4, int nSpheres, int32_t* out, int width, int height,
                                                      const tptObjectPlaneConsts& k, hipStream_t stream);
// tptTemporalAccumulateObjectsDevice: the plain pass's constants, made the same way.  (A struct of its own name: it is part of the two
// kernels' shipped symbols, which tests/kernel_manifest.py and profiles/ look them up by; folding it into tptTemporalConsts renames both.)
struct tptReprojectConsts {
    tptTemporalConsts t;
};
// One launch of the object-following accumulation kernel; the four prev planes and prevObject are all null (first frame) or all
// given; motion ([nObjects] f4 in device memory) may be null with nObjects == 0.  Weak for the same reason as tptLaunchDenoise.
__attribute__((weak)) hipError_t tptLaunchReprojectObjects(const float* colour, const float* albedo, const float* normalDepth,
                                                           const float* moments, const float* prevColour, const float* prevAlbedo,
                                                           const float* prevNormalDepth, const float* prevMoments, float* outColour,
                                                           float* outAlbedo, float* outMoments, float* outVariance,
                                                           const int32_t* object, const int32_t* prevObject, const float* motion,
                                                           int nObjects, int width, int height, const tptReprojectConsts& k,
                                                           hipStream_t stream);
// tptMotionVectorsDevice: what the kernel needs of one frame's camera, of its predecessor's and of the call, made on the host like
// tptTemporalConsts (the same fields in the same order, without the history length).  One record per frame of the clip in a table in
// device memory: 32 frames of them do not fit in kernel arguments.  (Its name is part of the kernels' shipped symbols, like tptReprojectConsts.)
struct tptFlowConsts {
    float o[3], ll[3], H[3], V[3];
    float po[3], pa[3], pw[3], pH[3], pV[3];
    float pf, phh, pvv;
    float depthTol, normalTol, coverageTol;
};
// One launch of the motion-vector kernel over `frames` consecutive frames: every plane pointer is the first of `frames` planes ([h][w]
// f4, the object planes [h][w] int32), the prev pointers those of the first frame's predecessor (for frames inside a clip the same
// stacks one plane earlier), `motion` the first frame's table of `frames` tables of nObjects f4 (null with nObjects == 0), deviceConsts
// the first frame's record of `frames` records in device memory.  object / prevObject both null: the plain form.  Weak for the same
// reason as tptLaunchDenoise.
__attribute__((weak)) hipError_t tptLaunchFlow(const float* albedo, const float* normalDepth, const int32_t* object, const float* prevAlbedo,
                                               const float* prevNormalDepth, const int32_t* prevObject, const float* motion, int nObjects,
                                               float* out, int width, int height, int frames, const tptFlowConsts* deviceConsts,
                                               hipStream_t stream);
// tptRectifyHistoryDevice: one launch over the image.  Every pointer is a plane of [h][w] f4; outColour / outMoments may be accColour /
// accMoments themselves.  radius 1..3 picks the instantiation.  The tile of the kernel's LDS layout: TPT_RECTIFY_TILE_W x
// TPT_RECTIFY_TILE_H pixels a workgroup, one lane each.  Weak for the same reason as tptLaunchDenoise.
#define TPT_RECTIFY_TILE_W 64
#define TPT_RECTIFY_TILE_H 4
#define TPT_RECTIFY_MAX_RADIUS 3
__attribute__((weak)) hipError_t tptLaunchRectify(const float* colour, const float* moments, const float* accColour, const float* accMoments,
                                                  float* outColour, float* outMoments, float* outVariance, int width, int height,
                                                  int radius, float gamma, hipStream_t stream);
// tptSpatialVarianceDevice: one launch over `frames` consecutive planes of [h][w] f4 each (grid.z is the frame).  normalDepth may be
// null (then in and id are 0 and the taps' weights are 1); in, id: the inverse squared sigmas, as tptLaunchDenoise takes them.
// radius 1..3 and the presence of normalDepth pick the instantiation.  The tile is the rectification kernel's.  Weak for the same
// reason as tptLaunchDenoise.
#define TPT_SPREAD_MAX_RADIUS 3
__attribute__((weak)) hipError_t tptLaunchSpread(const float* moments, const float* normalDepth, float* out, int width, int height,
                                                 int frames, float samplesPerFrame, float minSamples, int radius, float in, float id,
                                                 hipStream_t stream);
// tptDrawDeviceAdaptive's blend: tile.rgb and moments.xyz with lerp = S / (S + n) per pixel, S the running sample count in moments.w
// (0 unless `progressive`), n the pixel's clamped count; moments.w = S + n; pixels with n == 0 untouched.  Weak for the same reason as
// tptLaunchDenoise.
__attribute__((weak)) hipError_t tptLaunchAdaptiveResolve(float* tile, float* moments, const tpt::f4* frameColour, const tpt::f4* stagedMoments,
                                                          const int32_t* counts, int nPixels, bool progressive, hipStream_t stream);
// tptAdaptiveSamplesDevice: one launch of the plan kernel (outVariance / totalSamples may be null; totalSamples is zeroed first).  Weak
// for the same reason as tptLaunchDenoise.
__attribute__((weak)) hipError_t tptLaunchAdaptivePlan(const float* moments, int32_t* counts, float* outVariance, int64_t* totalSamples,
                                                       int width, int height, float targetError, int minSamples, int maxSamples,
                                                       hipStream_t stream);
hipError_t tptLaunchAssemble(const float* gathered, float* image, int width, int height, int stripeRows, int nRanks, int padRows, hipStream_t stream);
hipError_t tptLaunchQueueProbe(unsigned long long ticks, hipStream_t stream);
hipError_t tptLaunchChunkOrder(const unsigned* cost, unsigned* snap, unsigned* order, int numChunks, hipStream_t stream);
struct tptLerpTable { float v[32]; }; // lerp factor of each frame of a batch (Test.cpp:272-276), by value in the kernel arguments
hipError_t tptLaunchResolveBatch(float* tile, const tpt::f4* frameColour, int nPixels, int planeStride, int nFrames, const tptLerpTable& lerp,
                                 float* mirror, unsigned long long* rayCounter, unsigned long long* counterOut, hipStream_t stream);
hipError_t tptLaunchResolve(float* tile, const tpt::f4* frameColour, int nPixels, float lerpFac, float* mirror,
                            unsigned long long* rayCounter, unsigned long long* counterOut, const unsigned long long* frameRays, hipStream_t stream);
// tptDrawDeviceBatchMoments' blends: one launch folds the nFrames (1..32) staged planes of a trace launch, nPixels f4 apart, into the
// caller's four running means in frame order with lerp.v[j] -- tile.xyz and moments.xyz (.w kept), all four channels of albedo and
// normalDepth (either may be null, its staging then unused) -- and adds frameRays[0 .. nFrames - 1] to *totalRays (frameRays null: the
// trace kernel has counted into the total itself).  TPT_FOLD_BLOCKS_PER_PLANE: the workgroups it stops at per plane, 256 pixels a pass
// each.  Weak for the same reason as tptLaunchDenoise.
#define TPT_FOLD_BLOCKS_PER_PLANE 128
// Frames per launch of tptDrawDeviceBatchMoments: the most, up to 32, whose staging -- `planes` planes of planeBytes per frame: colour,
// moments and each guide plane that is given -- stays within the clip draws' 4096 MiB per launch; never fewer than one.
inline int tptFoldFramesPerLaunch(size_t planeBytes, int planes)
{
    const size_t perFrame = planeBytes * (size_t)planes, m = perFrame ? (4ull << 30) / perFrame : 32;
    return m > 32 ? 32 : (m < 1 ? 1 : (int)m);
}
__attribute__((weak)) hipError_t tptLaunchFoldBatch(float* tile, float* moments, float* albedo, float* normalDepth, const tpt::f4* stagedColour,
                                                    const tpt::f4* stagedMoments, const tpt::f4* stagedAlbedo,
                                                    const tpt::f4* stagedNormalDepth, int nPixels, int nFrames, const tptLerpTable& lerp,
                                                    const unsigned long long* frameRays, unsigned long long* totalRays, hipStream_t stream);
hipError_t tptLaunchMathTest(int op, const float* a, const float* b, float* out, int n, hipStream_t stream);
hipError_t tptLaunchMathExhaustive(int op, unsigned lo, unsigned hi, unsigned long long* nBad, unsigned* firstBad, hipStream_t stream);
hipError_t tptLaunchMatrixFilterTest(const tpt::KernelArgs& a, const float* rays, unsigned long long* outMask, int* outId, float* outT, int n, hipStream_t stream);
hipError_t tptSetDealCapacitiesForTest(int ca, int cb, int cs); // (hooks build)
hipError_t tptLaunchGroupFilterTest(const tpt::KernelArgs& a, const float* rays, int n, int nPad, unsigned long long* out4, hipStream_t stream);
hipError_t tptLaunchHitTest(const tpt::KernelArgs& a, int hs, const float* rays, int* outId, float* outT, int n, hipStream_t stream);
int tptReadStats(unsigned long long* out64);  // profiling build (-DTPT_STATS) only, else -1
int tptResetStats();
