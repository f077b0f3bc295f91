// TEST INFRASTRUCTURE: csrc/tpt_frame_pools.h -- when a batched launch takes a pool of chunks per frame, and the frame a workgroup then
// serves -- compiled for the host and exported to tests/test_frame_pools_rule.py.
#include "tpt_frame_pools.h"

extern "C" int fp_pools(int batch, int blocks, int plain, int helpable) { return tpt::framePoolsOfLaunch(batch, blocks, plain != 0, helpable != 0); }
extern "C" int fp_frame_of_block(int block, int pools, int blocks) { return (int)tpt::framePoolOfBlock((unsigned)block, (unsigned)pools, (unsigned)blocks); }
extern "C" int fp_base() { return tpt::kFramePoolBase; }
extern "C" int fp_max() { return tpt::kFramePoolsMax; }
