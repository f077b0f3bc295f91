"""What the ABI and ISA tests share (a plain module they import, not a conftest): the gfx950 code object inside the shipped library,
disassembled (the `code_object` fixture, count()); the library's exported symbols; the parameters of an entry point as include/tpt_hip.h
declares it; and the run of a refusal script against the host runtime compiled for tests/hostemu (a refused call returns before anything
is enqueued).  No GPU needed: the fat binary is unbundled and disassembled with the ROCm LLVM tools.  The kernels' names are
tests/kernel_manifest.py's."""
import collections
import functools
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

from oracle_lib import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
BUNDLER = os.path.join(LLVM, "clang-offload-bundler")
OBJDUMP = os.path.join(LLVM, "llvm-objdump")
READELF = os.path.join(LLVM, "llvm-readelf")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
HAVE_TOOLS = all(os.path.exists(p) for p in (BUNDLER, OBJDUMP, READELF)) and shutil.which("objcopy") is not None


def _stamp(path):
    """what a cached reading of the file at `path` is keyed by: a rebuilt library is read again"""
    st = os.stat(path)
    return path, st.st_mtime_ns, st.st_size


@functools.lru_cache(maxsize=None)
def _extract(path, mtime, size):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "kernels.co")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat])
        targets = subprocess.check_output([BUNDLER, "--list", "--type=o", "--input=" + fat]).decode().split()
        assert [t for t in targets if t.startswith("hipv4-amdgcn")] == [TARGET], "the library carries gfx950 code only: %r" % targets
        subprocess.check_call([BUNDLER, "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co])
        dis = subprocess.check_output([OBJDUMP, "-d", co]).decode()
        notes = subprocess.check_output([READELF, "--notes", co]).decode()
    bodies = {}
    for m in re.finditer(r"^[0-9a-f]+ <(\w+)>:\n(.*?)(?=^[0-9a-f]+ <\w+>:|\Z)", dis, flags=re.S | re.M):
        # one instruction per line: "\t<mnemonic> operands  // address: encoding"
        bodies[m.group(1)] = [ln.split("//")[0].split() for ln in m.group(2).splitlines() if ln.startswith("\t")]
    meta = {}
    for blk in re.split(r"\n\s+- (?=\.agpr_count)", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, flags=re.M)}
    return bodies, meta


@pytest.fixture(scope="module")
def code_object():
    """(bodies, meta) of the shipped library's gfx950 code object: each kernel's instructions as [mnemonic, operands...] and its
    metadata (register counts, spills, LDS, scratch) as ints.  Extracted once per process and library file; the modules share it and
    leave it as it is."""
    if not HAVE_TOOLS:
        pytest.skip("ROCm LLVM tools not installed")
    from toypathtracer_amd import api
    return _extract(*_stamp(api.library_path()))


@functools.lru_cache(maxsize=None)
def _nm(path, mtime, size):
    return subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()


def exported_symbols(path):
    """`nm -D --defined-only` of the library at `path`, as text: an entry point NAME is exported where "T NAME" stands in it"""
    return _nm(*_stamp(path))


def no_library():
    """stands in for api.load_library where a binding must refuse its arguments before it reaches the library"""
    raise AssertionError("the library was called")


def count(body, pattern):
    """instructions of `body` whose mnemonic matches `pattern`"""
    rx = re.compile(pattern)
    return sum(1 for ins in body if ins and rx.match(ins[0]))


def header():
    """include/tpt_hip.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tpt_hip.h")).read(), flags=re.S)


def header_params(name):
    """the parameters of entry point `name` as include/tpt_hip.h declares it, whitespace normalised"""
    decl = re.search(r"TPT_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert decl, "%s is not declared in include/tpt_hip.h" % name
    return [" ".join(p.split()) for p in decl.group(1).split(",")]


def run_refusals(script, lib="libtpt_hostemu.so", extra_sources=()):
    """`script` (given ROOT as argv[1]) against the host runtime built for tests/hostemu (with `extra_sources` beside the emulated
    kernels, as `lib`), under the lazy schedule; it must end with "ok".  Returns its output."""
    from test_host_logic import build
    path = build(lib, [os.path.join(ROOT, "tests", s) for s in extra_sources])
    env = dict(os.environ, TPT_LIB=path, HOSTEMU_POLICY="lazy")
    env.pop("TPT_LIB_DIR", None)
    p = subprocess.run([sys.executable, "-c", script, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.rstrip().endswith("ok"), out[-3000:]
    return out


def refusal_messages(out):
    """what a refusal script's "refused: <case> -- <message>" lines report: {message: how many cases reported it}.  A test holds this
    against the messages written out character for character, so a message that changes, or a case that reports another rule than it
    did (two rules violated: the order of the checks), fails."""
    return dict(collections.Counter(ln.split(" -- ", 1)[1] for ln in out.splitlines() if ln.startswith("refused:") and " -- " in ln))


def refused_without_its_launcher(body, message, lib="libtpt_hostemu.so", extra_sources=()):
    """The host runtime with the emulated kernels alone (the launcher is a weak symbol nobody defines; `lib` and `extra_sources`: a
    build that has some launchers and lacks others): after InitializeTest, `body` -- Python source with tpt (the binding), lib, C and
    np in scope -- makes calls and leaves the last one's return value in `rc`; that call is refused with exactly `message`."""
    script = ("import ctypes as C, sys\nimport numpy as np\nsys.path.insert(0, sys.argv[1])\nfrom toypathtracer_amd import api as tpt\n"
              "lib = tpt.load_library()\nmsg = lambda: lib.tptGetLastError().decode()\ntpt.InitializeTest()\n" + body +
              "\nassert rc != 0 and msg() == %r, (rc, msg())\ntpt.ShutdownTest()\nprint('ok')\n" % message)
    return run_refusals(script, lib, extra_sources)
