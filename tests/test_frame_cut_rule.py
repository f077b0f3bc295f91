"""The cut of a closed stream batch (csrc/tpt_frame_pools.h), on the CPU: which frames a launch still traces given its slot's cut word,
and which frame a workgroup serves then.  The header the kernel and the host runtime include, compiled for the host
(tests/frame_cut_shim.cpp -> tests/_build/)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "toypathtracer_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "frame_cut_shim.cpp")
HDR = os.path.join(INC, "tpt_frame_pools.h")


@pytest.fixture(scope="module")
def rule():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libframe_cut_shim.so")
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INC, SRC, "-o", so])
    lib = C.CDLL(so)
    for f in (lib.fc_word, lib.fc_next_serial, lib.fc_kept, lib.fc_served, lib.fc_own):
        f.restype = C.c_uint
        f.argtypes = [C.c_uint] * {"fc_word": 2, "fc_next_serial": 1, "fc_kept": 3, "fc_served": 4, "fc_own": 3}[f.__name__]
    lib.fc_served_all.restype = None
    lib.fc_served_all.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    return lib


def served_all(rule, pools, blocks, keep):
    served, own = np.empty(blocks, np.uint32), np.empty(blocks, np.uint32)
    rule.fc_served_all(pools, blocks, keep, served.ctypes.data, own.ctypes.data)
    return served, own


@pytest.mark.parametrize("pools", range(2, 9))
def test_every_workgroup_serves_a_kept_frame_and_every_kept_frame_keeps_its_share(rule, pools):
    for blocks in range(2 * pools, 1025):
        for keep in range(1, pools):
            served, own = served_all(rule, pools, blocks, keep)
            assert int(served.max()) < keep, (pools, blocks, keep)
            mine = own < keep
            assert (served[mine] == own[mine]).all(), (pools, blocks, keep)  # a wanted frame's workgroups stay with it
            counts = np.bincount(served, minlength=keep)
            assert int(counts.min()) >= blocks // pools, (pools, blocks, keep, counts.tolist())
            # ... and the cut frames' workgroups go round the kept ones: no kept frame gets two more of them than another
            helpers = np.bincount(served[~mine], minlength=keep)
            assert int(helpers.max()) - int(helpers.min()) <= 1, (pools, blocks, keep, helpers.tolist())


@pytest.mark.parametrize("pools", range(2, 9))
def test_keeping_every_frame_is_the_identity(rule, pools):
    for blocks in range(2 * pools, 1025):
        served, own = served_all(rule, pools, blocks, pools)
        assert (served == own).all(), (pools, blocks)


def test_single_values(rule):
    assert rule.fc_own(511, 8, 512) == 7 and rule.fc_served(511, 8, 512, 2) == 1 and rule.fc_served(510, 8, 512, 2) == 0
    assert rule.fc_served(64, 8, 512, 2) == 1 and rule.fc_served(63, 8, 512, 2) == 0  # (own frames 1 and 0: kept)
    assert rule.fc_served(200, 8, 512, 1) == 0


def test_cut_word(rule):
    serial = 0x123456
    for pools in range(2, 9):
        for keep in range(0, 12):
            word = rule.fc_word(serial, keep)
            assert word == (serial << 8 | keep)
            want = keep if 1 <= keep < pools else pools  # keep 0 and keep >= pools: not cut
            assert rule.fc_kept(word, serial, pools) == want, (pools, keep)
            # a word meant for another launch is ignored, whatever it keeps
            for other in (serial + 1, serial - 1, 1, 0xffffff, serial ^ 0x800000):
                assert rule.fc_kept(word, other, pools) == pools
        assert rule.fc_kept(0, serial, pools) == pools          # (the word of a launch that has not been cut)
        assert rule.fc_kept(3, 0, pools) == pools               # (serial 0 is no launch's)
    assert rule.fc_word(0xffffff, 7) == 0xffffff07              # the serial fills the upper 24 bits


def test_serials_are_24_bit_and_never_zero(rule):
    assert rule.fc_next_serial(0) == 1 and rule.fc_next_serial(1) == 2
    assert rule.fc_next_serial(0xfffffe) == 0xffffff and rule.fc_next_serial(0xffffff) == 1
    s, seen = 0, set()
    for _ in range(1000):
        s = rule.fc_next_serial(s)
        assert 1 <= s <= 0xffffff and s not in seen
        seen.add(s)
