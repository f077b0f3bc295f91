// tests/frame_cut_shim.cpp -- TEST INFRASTRUCTURE ONLY: the cut rule of csrc/tpt_frame_pools.h (the header the kernel and the host runtime
// include) compiled for the host, for tests/test_frame_cut_rule.py.
#include "tpt_frame_pools.h"

extern "C" unsigned fc_word(unsigned serial, unsigned keep) { return tpt::frameCutWord(serial, keep); }
extern "C" unsigned fc_next_serial(unsigned serial) { return tpt::frameCutNextSerial(serial); }
extern "C" unsigned fc_kept(unsigned word, unsigned serial, unsigned pools) { return tpt::framesKeptUnderCut(word, serial, pools); }
extern "C" unsigned fc_served(unsigned block, unsigned pools, unsigned blocks, unsigned keep) { return tpt::frameServedUnderCut(block, pools, blocks, keep); }
extern "C" unsigned fc_own(unsigned block, unsigned pools, unsigned blocks) { return tpt::framePoolOfBlock(block, pools, blocks); }
// every workgroup of one (pools, blocks, keep): served[b] for the caller to look at (blocks entries)
extern "C" void fc_served_all(unsigned pools, unsigned blocks, unsigned keep, unsigned* served, unsigned* own)
{
    for (unsigned b = 0; b < blocks; ++b) {
        served[b] = tpt::frameServedUnderCut(b, pools, blocks, keep);
        own[b] = tpt::framePoolOfBlock(b, pools, blocks);
    }
}
