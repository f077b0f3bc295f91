// tpt_queue_layout.h -- what a launch of the path-queue kernel is built from, stated once for the kernels (tpt_kernels.hip), the host
// runtime (chooseKernel and the buffers it sizes) and the CPU suite's emulated kernels: the layout of a workgroup's LDS, the sizes
// derived from it, which of the kernel's variants a launch's argument block asks for, and which pixel a work item is.  Plain C++.
#pragma once
#include "tpt_device.h"
#include "tpt_shard.h"

#ifndef TPT_Q_WAVES
#define TPT_Q_WAVES 8
#endif
#define TPT_Q_T (64 * TPT_Q_WAVES)
#ifndef TPT_Q_P
#define TPT_Q_P 1024 // capacity of every ring (power of two)
#endif
#ifndef TPT_MATRIX_FILTER
#define TPT_MATRIX_FILTER 1 // phase 1 of HitSpheres on the matrix cores (v_mfma_f32_32x32x16_f16, f16-split operands) for scenes with a table; 0: packed VALU filter only
#endif
#ifndef TPT_GROUP_DEAL
// Grouped traversal of large scenes (the kernel instantiated without LDS scene staging): 1 = the (ray, group) pairs of a wave
// are dealt out evenly over its lanes through a pair list in LDS (hitSpheresGroupedDeal); 0 = every lane walks the groups its
// own ray touches (tpt_trace.h hitSpheresGrouped: 10.5 trips per wave at 20 busy lanes for 4.0 groups per ray on the
// 4096-sphere scene, tools/stats_c5.py, profiles/r04/r04_run4.log)
#define TPT_GROUP_DEAL 1
#endif
#ifndef TPT_GROUP_MATRIX_BOUNDS
// The groups' bounds on the matrix cores (hitSpheres variant 4) are compiled into the HOOKS build only: a wave that has executed that
// path is not safe in a time-sliced process, it is no faster than the two-level VALU filter any more, and without it
// the product's grouped instantiation executes no MFMA at all -- and needs fewer registers.
#if defined(TPT_TEST_HOOKS)
#define TPT_GROUP_MATRIX_BOUNDS 1
#else
#define TPT_GROUP_MATRIX_BOUNDS 0
#endif
#endif
#ifndef TPT_GROUP_DEAL_EXACT
#define TPT_GROUP_DEAL_EXACT 1 // the members that pass the member filter are dealt out again for their exact tests (see hitSpheresGroupedDeal)
#endif
#ifndef TPT_DEAL_HALF_LINE
#define TPT_DEAL_HALF_LINE 1 // the three-stage dealing drops bounds that lie wholly behind the ray's origin (tpt_trace.h phase1PairT<true>); 0: line test only
#endif
#ifndef TPT_MEMBER_UNROLL
#define TPT_MEMBER_UNROLL 8 // member records requested together in the member filter of a (ray, group) pair: all eight (a latency-bound gather from L2; 4: -3 %, profiles/r06/r06_run14.log)
#endif
#ifndef TPT_GROUP_DEAL_CAP
// pair-list entries per wave and round of the FLAT variants (hitSpheres 3 / 4: one (path, group) list filled by the owners, a multiple
// of 64).  The sweeps that chose 448 (128 ... 640 entries against the path pool they leave: profiles/r06/r06_run14-16.log, r06_run26.log)
// were made while the default traversal used this list too; it deals in three stages now (TPT_DEAL_CA / CB / CS below).
#define TPT_GROUP_DEAL_CAP 448
#endif
// The three-stage dealing (dealThreeStage) cuts the wave's list area into (path, super-group) entries of a round, the stack of (path,
// group) entries waiting for a member pass and the stack of survivors waiting for an exact pass; the flat / matrix-core variants use the
// first TPT_GROUP_DEAL_CAP entries as one pair list.  Four counters behind the entries.
#ifndef TPT_DEAL_CA
#define TPT_DEAL_CA (TPT_SUPER == 8 ? 256 : 192)
#endif
#ifndef TPT_DEAL_CB
#define TPT_DEAL_CB (TPT_SUPER == 8 ? 256 : 320) // (a sub-round of 64 super-group entries leaves ~90 group entries on average -- more with super-groups of 16 --, 64 x TPT_SUPER at most; fewer than 64 wait when it starts)
#endif
#ifndef TPT_DEAL_CS
#define TPT_DEAL_CS 128 // (a member pass leaves 17 survivors on average, 512 at most; fewer than 64 wait when it starts)
#endif
#define TPT_GROUP_DEAL_ENTRIES (TPT_DEAL_CA + TPT_DEAL_CB + TPT_DEAL_CS)
static_assert(TPT_GROUP_DEAL_ENTRIES >= TPT_GROUP_DEAL_CAP, "the flat variants' pair list lives in the same area");
#define TPT_GROUP_DEAL_WAVE_BYTES (TPT_GROUP_DEAL_ENTRIES * 4 + 16)
#define TPT_Q_SPH_FIXED 1024 /* bytes at LDS offset 0 for {centre, r^2} of scenes of <= 64 spheres: DS offsets fold into the instructions */
#ifndef TPT_Q_PATHS
// paths per workgroup (<= TPT_Q_P): what the path records in LDS are sized for.  960 with the matrix filter: its 4-KB operand
// table and the fixed 1-KB sphere area have to fit beside them for two workgroups per CU (2 x 80 KB minus the launch code's
// 256-B margin per workgroup: chooseKernel); 960 measured no slower than 1024 (profiles/r03/r03_run10.log)
#define TPT_Q_PATHS (TPT_MATRIX_FILTER ? 952 : TPT_Q_P)
#endif
// Several views in one launch (tptTraceViewsKernel): the views' cameras sit in LDS (32 x 88 B), and the instantiation owns 44 paths
// fewer than its single-view twin to make room for them (44 x 64 B of path records = 32 x 88 B): the LDS a launch takes stays what it
// was, so the default scene keeps two workgroups per CU and the matrix-core filter (chooseKernel drops both when it does not fit).
#define TPT_Q_VIEWS_MAX 32
#define TPT_Q_VIEW_CAM_BYTES (TPT_Q_VIEWS_MAX * 88)
#define TPT_Q_VIEW_PATHS ((TPT_Q_VIEW_CAM_BYTES + TPT_Q_NF4 * 16 - 1) / (TPT_Q_NF4 * 16))
// Frames of an animated scene in one launch (tptTraceAnimationKernel): each frame's centres of spheres 1 and 8 sit in LDS (32 x 2 x 16 B),
// in the place of 16 path records (16 x 64 B): the same LDS per launch as the single-frame twin, as for the views.
#define TPT_Q_ANIM_TABLE_BYTES (TPT_Q_VIEWS_MAX * 2 * 16)
#define TPT_Q_ANIM_PATHS ((TPT_Q_ANIM_TABLE_BYTES + TPT_Q_NF4 * 16 - 1) / (TPT_Q_NF4 * 16))
// A camera per frame of a clip (tptCameraClipKernel): both tables, in the place of TPT_Q_VIEW_PATHS + TPT_Q_ANIM_PATHS path records.
// A clip whose spheres the caller moves (tptKeyframeKernel): the cameras, and each frame's centres of up to TPT_Q_KEYS_MAX moved spheres at
// a fixed stride of TPT_Q_KEYS_MAX entries per frame (32 x 8 x 16 B = 4096 B) in the place of 64 path records, on top of the cameras' 44.
#define TPT_Q_KEYS_MAX 8
#define TPT_Q_KEY_TABLE_BYTES (TPT_Q_VIEWS_MAX * TPT_Q_KEYS_MAX * 16)
#define TPT_Q_KEY_PATHS ((TPT_Q_KEY_TABLE_BYTES + TPT_Q_NF4 * 16 - 1) / (TPT_Q_NF4 * 16))
#ifndef TPT_Q_PATHS_GROUPED
// ... and of the instantiation for GROUPED scenes (no scene staging, no matrix-filter table): 608.  The LDS the smaller pool frees holds
// the entry areas of the three-stage dealing (640 entries per wave) and the groups' bounding spheres (pair records, 144 B per super-group
// of 8 groups, for up to TPT_Q_GROUP_LDS_BYTES: stage B reads them per lane, and from L2 that stage would be latency-bound).  624 ... 752
// paths measured within 1 % of each other (profiles/r06/r06_run26.log).
#define TPT_Q_PATHS_GROUPED 608
#endif
// The groups' pair records in LDS: a super-group's four records (128 B) are read per lane by lanes that hold DIFFERENT super-groups. At a
// stride of 128 B every lane's read of "record q, half h" lands on one of two 16-byte bank groups of the 16 -- an 8-way conflict on
// every read (68 % of the LDS's active cycles were conflict cycles, profiles/r06/r06_run30.log).  Nine bank groups per super-group
// (144 B: 16 B of padding) spread consecutive super-groups over all sixteen.
#define TPT_GPAIR_FLOATS ((TPT_SUPER / 2) * 8) /* floats of a super-group's pair records: 32 (64 for super-groups of 16) */
#define TPT_GPAIR_LDS_STRIDE (TPT_GPAIR_FLOATS + 4) /* floats per super-group in LDS: 9 (17) bank groups of 16 bytes */
#define TPT_Q_GROUP_LDS_BYTES 9808 /* group pair records in LDS at most: 68 super-groups x 144 B + 16 (a launch that would lose its second workgroup per CU to them reads them from global memory instead: chooseKernel) */
#ifndef TPT_Q_FUSE_MIN
#define TPT_Q_FUSE_MIN 48 // a batch intersects its own rays when at least this many lanes still hold one
#endif
#define TPT_Q_NF4 4

namespace tpt {

enum { Q_FREE = 0, Q_INT = 1, Q_END = 2, Q_DIEL = 3, Q_METAL = 4, Q_LAMBERT = 5, Q_COUNT = 6 };
// The frame-pools kernel for scenes staged in LDS (tptFramePoolsKernel<true>: the headline's steady state) alone has a seventh ring:
// Q_LAST, the ended samples that are their pixel's LAST one.  (Its grouped twin keeps the six: there the split measured slower.)
// There a path's next class is decided by its sample number where it is pushed, so a popped END batch holds only paths with a
// further sample -- every lane makes a camera ray, the batch intersects 64 rays of 64 -- and a LAST batch stores its pixels and
// starts the next pixels in the same lanes (the FREE code), which fills it again.  With one END class a quarter of a batch's lanes
// at 4 spp went to FREE, and a batch left with fewer than TPT_Q_FUSE_MIN rays sent them all through INT.
// The ring (TPT_Q_P x 2 B) takes the LDS of TPT_Q_LAST_PATHS path records, which that instantiation gives up: a launch's LDS is its
// twin's, byte for byte (tptQueueLdsBytes below knows no difference).
enum { Q_LAST = Q_COUNT, Q_COUNT_POOLS = Q_COUNT + 1 };
#define TPT_Q_LAST_PATHS ((TPT_Q_P * 2) / (TPT_Q_NF4 * 16))
static_assert(TPT_Q_LAST_PATHS * TPT_Q_NF4 * 16 == TPT_Q_P * 2, "the seventh ring takes exactly the LDS of the path records it replaces");
struct QueueCtl {
    unsigned head[8];
    unsigned tail[8];
    unsigned poolTotal;       // pixels sitting in the private chunk pools of this workgroup's waves (+ fetches in flight)
    unsigned globalExhausted; // some wave saw the global chunk counter run out
    unsigned frameRays[32];   // batched launch: rays traced for each frame of the batch by this workgroup (flushed to the global counter every 2^31: see the push)
};
// One frame index per frame of a batch, everywhere: the cameras / centres tables and the per-frame ray counts above, the lerp factors
// of the blend, 6 bits of the path record (>> 26).
static_assert(sizeof(QueueCtl::frameRays) / 4 == TPT_Q_VIEWS_MAX, "one ray count per frame of a batch");
static_assert(sizeof(tptLerpTable::v) / sizeof(float) == TPT_Q_VIEWS_MAX, "one lerp factor per frame of a batch");
static_assert(TPT_Q_VIEWS_MAX <= 64, "the path record holds 6 bits of frame index");

// Two workgroups per CU is what the path-queue kernel is tuned for; the launch code (chooseKernel) drops the LDS scene --
// and with it the matrix-core filter: 58 -> 41 Gray/s -- as soon as 2 x (LDS + 256-B margin) exceeds 160 KB.  The built-in
// 46-sphere scene with 2 lights must fit: checked at compile time, because a few hundred bytes too many are silent at run time.
constexpr size_t kQueueLdsFixedPart = (size_t)TPT_Q_NF4 * TPT_Q_PATHS * 16 + (size_t)Q_COUNT * TPT_Q_P * 2 + ((sizeof(tpt::QueueCtl) + 63) & ~(size_t)63) +
                                      ((sizeof(tpt::FrameConsts) + 15) & ~(size_t)15);
constexpr size_t kDefaultSceneLds = TPT_Q_SPH_FIXED + ((46 * 4 + 15) & ~15) + 46 * 48 + 2 * 32 + (TPT_MATRIX_FILTER ? TPT_MXH_TABLE_DWORDS * 4 + 64 : 0);
static_assert(2 * (kQueueLdsFixedPart + kDefaultSceneLds + 256) <= 160 * 1024, "the default scene no longer fits two path-queue workgroups per CU: shrink TPT_Q_PATHS");
static_assert(TPT_Q_VIEW_CAM_BYTES <= TPT_Q_NF4 * TPT_Q_VIEW_PATHS * 16, "the views' cameras take no more LDS than the path records they replace");
static_assert(sizeof(tpt::CameraPOD) == 88 && sizeof(tpt::CameraPOD) % 4 == 0, "cameras are staged in LDS as 22 words");
static_assert(TPT_Q_ANIM_TABLE_BYTES == TPT_Q_NF4 * TPT_Q_ANIM_PATHS * 16, "the moving centres take exactly the LDS of the path records they replace");
static_assert(TPT_Q_KEY_TABLE_BYTES == TPT_Q_NF4 * TPT_Q_KEY_PATHS * 16 && TPT_Q_KEY_PATHS == 64, "the keyed centres take exactly the LDS of the 64 path records they replace");
static_assert(TPT_Q_KEYS_MAX <= 64 && TPT_Q_VIEW_PATHS + TPT_Q_KEY_PATHS < TPT_Q_PATHS_GROUPED, "a keyed sphere's slot is a popcount of the 64-bit mask; path records are left");

// Which pixel a work item of a launch is (both trace kernels).
// idx -> pixel.  Returns false for padding slots of partially covered tiles.
TPT_HD bool mapItem(const KernelArgs& a, int idx, int& x, int& ly)
{
    if (a.fc.seedMode == SEED_ROW_SERIAL) {
        x = 0;
        ly = idx;
        return ly < a.nLocalRows;
    }
    int tile = idx >> 6, within = idx & 63;
    const int tilesX = uniformHere(a.tilesX);
    int tx = tile % tilesX, ty = tile / tilesX;
    x = tx * 8 + (within & 7);
    ly = ty * 8 + (within >> 3);
    return x < a.fc.width && ly < a.nLocalRows;
}
TPT_HD int localRowToGlobal(const KernelArgs& a, int ly) { return shardKernelLocalToGlobal(ly, uniformHere(a.stripeRows), uniformHere(a.stripeStride), a.stripeOffset); }
TPT_HD int globalRowToLocal(const KernelArgs& a, int gy) { return shardKernelGlobalToLocal(gy, uniformHere(a.stripeRows), uniformHere(a.stripeStride), a.stripeOffset); } // rows of this rank

} // namespace tpt

// Which variant of the path-queue kernel a launch takes: what its argument block holds decides, here and nowhere else.  QV_INVALID: a
// combination no entry point builds (tptLaunchTraceQueue refuses it).
enum QueueVariant { QV_FRAME, QV_BATCH, QV_VIEWS, QV_ANIMATION, QV_AOV, QV_MOMENTS, QV_CLIP, QV_ADAPTIVE, QV_KEYFRAME_CLIP, QV_FRAME_POOLS, QV_CAMERA_CLIP, QV_INVALID };
inline QueueVariant tptQueueVariant(const tpt::KernelArgs& a)
{
    if (a.framePools != 0) { // (a pool of chunks per frame, tpt_frame_pools.h: a plain batched launch of 2 .. kFramePoolsMax frames, one pool each, no helper grid)
        if (a.framePools != a.batchFrames || a.framePools < 2 || a.framePools > tpt::kFramePoolsMax || a.helperBase > 0 || a.viewCams || a.moveCentres ||
            a.keyCentres || a.sampleCounts || a.aovSums || a.fc.seedMode == tpt::SEED_ROW_SERIAL)
            return QV_INVALID;
        return QV_FRAME_POOLS;
    }
    if (a.keyCentres) { // (tptDrawDeviceKeyframeClip: 1 .. TPT_Q_VIEWS_MAX frames of the batch with their planes, a camera and the keyed centres per frame, a flat scene)
        if (a.batchFrames < 1 || a.batchFrames > TPT_Q_VIEWS_MAX || a.scene.nGroups > 0 || !a.viewCams || a.moveCentres || a.sampleCounts || !a.aovSums ||
            !a.momentsOut || a.keyCount < 0 || a.keyCount > TPT_Q_KEYS_MAX)
            return QV_INVALID;
        return QV_KEYFRAME_CLIP;
    }
    if (a.sampleCounts) { // (tptDrawDeviceAdaptive: a single frame with its planes and moments, a sample count per pixel)
        if (a.batchFrames != 1 || a.viewCams || a.moveCentres || !a.aovSums || !a.momentsOut) return QV_INVALID;
        return QV_ADAPTIVE;
    }
    if (a.viewCams && a.moveCentres) { // (tptDrawDeviceCameraClip: 1 .. TPT_Q_VIEWS_MAX frames of the batch with their planes, a camera and the centres per frame, a flat scene)
        if (a.batchFrames < 1 || a.batchFrames > TPT_Q_VIEWS_MAX || a.scene.nGroups > 0 || !a.aovSums || !a.momentsOut) return QV_INVALID;
        return QV_CAMERA_CLIP;
    }
    if (a.viewCams) { // (tptDrawDeviceViews: 1 .. TPT_Q_VIEWS_MAX views, the frames of the batch)
        if (a.batchFrames < 1 || a.batchFrames > TPT_Q_VIEWS_MAX) return QV_INVALID;
        return QV_VIEWS;
    }
    if (a.aovSums && a.moveCentres) { // (tptDrawDeviceAnimationMoments: 1 .. TPT_Q_VIEWS_MAX frames of the batch with their planes, a flat scene)
        if (a.batchFrames < 1 || a.batchFrames > TPT_Q_VIEWS_MAX || a.scene.nGroups > 0 || !a.momentsOut) return QV_INVALID;
        return QV_CLIP;
    }
    if (a.aovSums) { // (tptDrawDeviceAov, tptDrawDeviceMoments with a.momentsOut: a single frame)
        if (a.batchFrames != 1 || a.viewCams || a.moveCentres) return QV_INVALID;
        return a.momentsOut ? QV_MOMENTS : QV_AOV;
    }
    if (a.moveCentres) { // (tptDrawDeviceAnimation: 1 .. TPT_Q_VIEWS_MAX frames of the batch, a flat scene)
        if (a.batchFrames < 1 || a.batchFrames > TPT_Q_VIEWS_MAX || a.scene.nGroups > 0) return QV_INVALID;
        return QV_ANIMATION;
    }
    return a.batchFrames > 1 ? QV_BATCH : QV_FRAME;
}

inline size_t tptLdsBytes(const tpt::KernelArgs& a, int fold, bool ldsScene) // (the lane-refill kernel; uses a.ldsStackLevels)
{
    const int nPad = a.scene.nPairs * 2;
    size_t bytes = 0;
    if (ldsScene) bytes += (size_t)nPad * 16 + (((size_t)nPad * 4 + 15) & ~(size_t)15);
    bytes += (size_t)a.scene.nLights * 32;
    if (ldsScene) bytes += (size_t)a.scene.nSpheres * 48;
    if (fold == tpt::FOLD_RECURSIVE) bytes += (size_t)a.ldsStackLevels * TPT_BLOCK * 16;
    return bytes;
}
inline size_t tptQueueLdsBytes(const tpt::KernelArgs& a, bool ldsScene)
{
    using namespace tpt;
    const int nPad = a.scene.nPairs * 2;
    const QueueVariant variant = tptQueueVariant(a);
    const bool views = variant == QV_VIEWS || variant == QV_CAMERA_CLIP || variant == QV_KEYFRAME_CLIP; // (tptTraceViewsKernel: the cameras in LDS, TPT_Q_VIEW_PATHS path records fewer)
    const bool moving = variant == QV_ANIMATION || variant == QV_CLIP || variant == QV_CAMERA_CLIP; // (tptTraceAnimationKernel: the centres in LDS, TPT_Q_ANIM_PATHS path records fewer)
    // (tptCameraClipKernel: both tables, in the place of both shares of path records; tptKeyframeKernel: the cameras and the keyed centres,
    //  in the place of TPT_Q_VIEW_PATHS + TPT_Q_KEY_PATHS path records)
    // (tptTraceAovKernel, tptTraceMomentsKernel, tptTraceAdaptiveKernel and tptTraceClipKernel, a.aovSums: the LDS of their twin without
    //  planes -- their sums live in global memory; tptCameraClipKernel likewise)
    size_t bytes = 0;
    if (ldsScene) bytes += TPT_Q_SPH_FIXED + ((size_t)nPad * 16 <= TPT_Q_SPH_FIXED ? 0 : (size_t)nPad * 16) + (((size_t)nPad * 4 + 15) & ~(size_t)15) + (size_t)a.scene.nSpheres * 48;
    bytes += (size_t)a.scene.nLights * 32;
    bytes += (size_t)TPT_Q_NF4 * (ldsScene ? TPT_Q_PATHS : TPT_Q_PATHS_GROUPED) * 16 + (size_t)Q_COUNT * TPT_Q_P * 2 + ((sizeof(QueueCtl) + 63) & ~(size_t)63) + ((sizeof(FrameConsts) + 15) & ~(size_t)15);
    if (views) bytes += (size_t)TPT_Q_VIEW_CAM_BYTES - (size_t)TPT_Q_NF4 * TPT_Q_VIEW_PATHS * 16;
    if (moving) bytes += (size_t)TPT_Q_ANIM_TABLE_BYTES - (size_t)TPT_Q_NF4 * TPT_Q_ANIM_PATHS * 16;
    if (variant == QV_KEYFRAME_CLIP) bytes += (size_t)TPT_Q_KEY_TABLE_BYTES - (size_t)TPT_Q_NF4 * TPT_Q_KEY_PATHS * 16;
    if (!ldsScene && TPT_GROUP_DEAL) bytes += (size_t)TPT_Q_WAVES * TPT_GROUP_DEAL_WAVE_BYTES;
    if (!ldsScene && a.ldsGroupPairs > 0) bytes += 16 + (size_t)(a.ldsGroupPairs / (TPT_SUPER / 2)) * TPT_GPAIR_LDS_STRIDE * 4; // the groups' bounds for the second filter level (tptQueueGroupPairsInLds), padded stride
#if TPT_MATRIX_FILTER
    if (ldsScene && a.scene.mxR1 >= 0) bytes += TPT_MXH_TABLE_DWORDS * sizeof(uint32_t) + 64;
#endif
    return bytes;
}
inline int tptQueuePathsPerBlock() { return TPT_Q_PATHS; } // (the larger of the two pools: what per-workgroup buffers are sized for)
// Pair records of the groups' bounds the grouped instantiation keeps in LDS for a scene of nGroups groups: whole super-groups
// (padded), or 0 when they do not fit the area the smaller path pool leaves (the flat filter runs over all groups then)
inline int tptQueueGroupPairsInLds(int nGroups, int nSuperPairs)
{
    if (nGroups <= 0 || nSuperPairs <= 0) return 0;
    const int pairs = ((nGroups + TPT_SUPER - 1) / TPT_SUPER) * (TPT_SUPER / 2);
    return (size_t)(pairs / (TPT_SUPER / 2)) * TPT_GPAIR_LDS_STRIDE * 4 + 16 <= (size_t)TPT_Q_GROUP_LDS_BYTES ? pairs : 0;
}
inline int tptQueueThreadsPerBlock() { return TPT_Q_T; }
