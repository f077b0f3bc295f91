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

// A STREAM launch whose caller waited before asking for all of its frames is CUT: frames >= keep of the batch will never be blended,
// so nobody needs to trace them.  One 32-bit word per launch slot in pinned host memory says so: serial << 8 | keep, the serial (24
// bits, never 0) naming the launch the word is meant for -- a slot's word left over from an earlier launch, a word not written yet
// (0) and a word that keeps nothing or everything all read as "not cut".  The host writes it when it drops the launch's unserved
// frames from its queue (LaunchQueue::closeStream, discard) and never otherwise, so whatever the kernel reads, and whenever, frames
// < keep are wanted and traced in full.
// The kernel reads the word ONCE per workgroup, where it starts: a few hundred single reads of host memory per launch.  A workgroup
// whose own frame is cut by then serves a kept frame instead (frameServedUnderCut); one that is already running finishes its frame's
// pool as before.  The last launch of a stream mostly starts after the caller's wait -- it queues behind the launches in flight -- so
// that is where the gain is.  Reading the word again where a wave fetches a chunk was measured and dropped: 50 million fetches a
// second in the headline run, and every form of it -- the word in host memory, or a copy relayed into the launch's counter block,
// beside the pool counters or read with a clock-elected poll -- made the steady launches three to five times as long
// (profiles/stream_cut/README.md).
TPT_FP_HD unsigned frameCutWord(unsigned serial, unsigned keep)
{
    return serial << 8 | (keep & 0xffu);
}
// The next launch's serial: 1, 2, ... 2^24 - 1, 1, ...
TPT_FP_HD unsigned frameCutNextSerial(unsigned serial)
{
    return (serial & 0xffffffu) == 0xffffffu ? 1u : (serial & 0xffffffu) + 1u;
}
// Frames of a launch of `pools` frames with serial `serial` that are still wanted, given the slot's word: `pools` = not cut.
TPT_FP_HD unsigned framesKeptUnderCut(unsigned word, unsigned serial, unsigned pools)
{
    // (one subtraction and one comparison: word - (serial << 8) lies in 1 .. pools - 1 <= 254 exactly when the word carries this
    //  serial and such a keep)
    const unsigned keep = word - (serial << 8);
    return (serial != 0u && keep - 1u < pools - 1u) ? keep : pools;
}
// The frame workgroup `block` serves when only frames < keep are wanted (1 <= keep <= pools): its own while that is wanted, else it
// helps frame block % keep -- the cut frames' workgroups spread evenly over the kept ones, each of which keeps its own workgroups.
TPT_FP_HD unsigned frameServedUnderCut(unsigned block, unsigned pools, unsigned blocks, unsigned keep)
{
    const unsigned own = framePoolOfBlock(block, pools, blocks);
    return own < keep ? own : block % keep;
}

} // namespace tpt
