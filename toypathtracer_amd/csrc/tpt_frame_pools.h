// tpt_frame_pools.h -- when a batched launch of the path-queue kernel hands out its chunks from one pool per FRAME instead of one
// shared pool, and which frame a workgroup then serves, in one place.
//
// With one pool, chunks go out frame-major to every workgroup of the launch: they all run dry at the same moment and drain their
// paths in partial batches side by side, and the next launch's workgroups, which enter as these leave, form one cohort again
// (DESIGN 3.2, 3.4).  With a pool per frame a workgroup serves ONE frame of the batch and leaves when that frame's pool is dry and its
// own paths are done -- it takes no chunk of another frame -- so the drains of a launch spread over its frames the way the drains of
// the deep pipeline's one-frame launches do.
// Plain integer functions shared by the kernel (tpt_kernels.hip), the host runtime (tpt_host_pipeline.cpp) and the CPU test of the
// rule (tests/frame_pools_shim.cpp -> tests/test_frame_pools_rule.py).
#pragma once

#if defined(__HIPCC__)
#define TPT_FP_HD __host__ __device__ inline
#else
#define TPT_FP_HD inline
#endif

namespace tpt {

// The launch's counter block (KernelArgs::work, 16 words) holds the pools' chunk counters at work[kFramePoolBase + frame].
const int kFramePoolBase = 4;
const int kFramePoolsMax = 8; // (Context::kStreamBatchMax: work[4..11])

// Pools of a launch: 0 = the shared pool (work[0]), else `batch` pools, one per frame.
//   batch     frames of the launch
//   blocks    workgroups of its grid
//   plain     the plain batched path-queue kernel with per-pixel seeds (tptDrawDeviceBatch, STREAM launches): not the views / animation /
//             clip / keyframe kernels, not a row-serial batch
//   helpable  a helper grid can attach to the launch (its workgroups would have no frame of their own)
// Two workgroups per frame at least: with one, a frame's tail is a single workgroup's tail.
TPT_FP_HD int framePoolsOfLaunch(int batch, int blocks, bool plain, bool helpable)
{
    return (plain && !helpable && batch >= 2 && batch <= kFramePoolsMax && blocks >= 2 * batch) ? batch : 0;
}

// The frame of the batch that workgroup `block` of a grid of `blocks` serves (pools > 0, blocks >= pools): monotonic in `block` --
// the dispatcher starts workgroups in index order, so a waiting launch's frames enter one after the other -- and every frame gets
// blocks / pools workgroups, rounded down or up.
TPT_FP_HD unsigned framePoolOfBlock(unsigned block, unsigned pools, unsigned blocks)
{
    return block * pools / blocks;
}

} // namespace tpt
