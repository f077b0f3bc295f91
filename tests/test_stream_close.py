"""A wait in the middle of a stream (tptSynchronize, tptRayCounterRead) drops the open STREAM batch: the next call is traced anew, and
images and ray totals stay exact.  Run on the CPU through the host-emulation build of the runtime (tests/hostemu_stream_close_driver.py,
under the eager, lazy and a random schedule of the emulated device; see tests/test_host_logic.py)."""
import os
import subprocess
import sys

import pytest

from test_host_logic import build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("policy", ["eager", "lazy", "random:3"])
def test_wait_drops_the_open_stream_batch(policy):
    lib = build("libtpt_hostemu.so", [])
    env = dict(os.environ, TPT_LIB=lib, HOSTEMU_POLICY=policy)
    env.pop("TPT_LIB_DIR", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "hostemu_stream_close_driver.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    text = p.stdout.decode()
    lines = [ln for ln in text.splitlines() if ln.startswith(("OK", "FAIL"))]
    assert p.returncode == 0 and len(lines) == 3 and all(ln.startswith("OK") for ln in lines), text[-3000:]
