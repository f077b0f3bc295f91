"""The host side of the cut of a closed stream batch (csrc/tpt_frame_pools.h) on the CPU: tptSynchronize, tptRayCounterRead, tptTimerEnd
and a discard store serial << 8 | frames served into the dropped launch's cut word, a batch served in full writes nothing, and the
stream goes on exactly after each: the next call starts a launch of its own, with the next serial.  Through the host-emulation build of the runtime (tests/hostemu_stream_cut_driver.py, under the eager,
lazy and a random schedule of the emulated device; see tests/test_host_logic.py)."""
import os
import subprocess
import sys

import pytest

from test_host_logic import build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("policy", ["eager", "lazy", "random:5"])
def test_dropping_an_open_stream_batch_writes_its_cut_word(policy):
    lib = build("libtpt_hostemu_stream_cut.so", [os.path.join(HERE, "hostemu_stream_cut.cpp")])
    env = dict(os.environ, TPT_LIB=lib, HOSTEMU_POLICY=policy)
    env.pop("TPT_LIB_DIR", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "hostemu_stream_cut_driver.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    text = p.stdout.decode()
    lines = [ln for ln in text.splitlines() if ln.startswith(("OK", "FAIL"))]
    assert p.returncode == 0 and len(lines) == 7 and all(ln.startswith("OK") for ln in lines), text[-3000:]
