"""The C-ABI library loads, exports every symbol include/tpt_hip.h declares plus the reference's own
C++ symbols, keeps the reference's struct sizes, and fails loudly (no CPU fallback) without a GPU."""
import os
import re
import subprocess

import pytest

from isa_lib import exported_symbols, header
from oracle_lib import ROOT


def header_symbols(name="tpt_hip.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tpt[A-Z]\w*)\s*\(", text)))


def exported(path):
    return sorted(line.split()[-1] for line in exported_symbols(path).splitlines() if line.strip())


def test_library_exports_every_declared_symbol():
    from toypathtracer_amd import api
    lib = api.load_library()
    declared = header_symbols()
    assert len(declared) >= 25
    assert sorted(api.C_ABI_SYMBOLS) == declared, "api.C_ABI_SYMBOLS out of sync with include/tpt_hip.h"
    assert sorted(set(re.findall(r"TPT_API\s+[\w\s*]+?\b(tpt\w+)\s*\(", header()))) == declared, "a declared function is not TPT_API"
    for name in declared:
        assert hasattr(lib, name), name


def test_library_exports_exactly_its_abi():
    """-fvisibility=hidden + csrc/exports.map: the dynamic symbol table of the product library is the C ABI of include/tpt_hip.h
    plus the reference's six C++ symbols and NOTHING else -- no internal helper, no kernel stub, no libstdc++ instantiation, no
    unit-test hook.  The hooks build (the GPU suite's unit tests) adds exactly include/tpt_test_hooks.h."""
    from toypathtracer_amd import api
    assert exported(api.library_path()) == sorted(header_symbols() + api.CXX_ABI_SYMBOLS)
    hooks = header_symbols("tpt_test_hooks.h")
    assert sorted(hooks) == sorted(api.HOOK_SYMBOLS)
    assert exported(api.hooks_library_path()) == sorted(header_symbols() + hooks + api.CXX_ABI_SYMBOLS)


def test_library_exports_reference_cxx_symbols():
    """Link-level drop-in: the mangled names `nm` shows for the reference's compiled Test.cpp."""
    from toypathtracer_amd import api
    out = exported_symbols(api.library_path())
    for sym in api.CXX_ABI_SYMBOLS:
        assert re.search(r"\bT %s\b" % re.escape(sym), out), sym


def test_layout_contract():
    from toypathtracer_amd import api
    assert api.GetObjectCount() == (46, 20, 36, 88)  # TestWin.cpp:132-134


def test_scene_desc_matches_reference_without_gpu():
    import numpy as np
    from common import golden_scene
    from toypathtracer_amd import api
    s, m, _cam, em = api.GetSceneDesc()
    gs, gm, _gc, gem = golden_scene()
    assert s.tobytes() == gs.tobytes() and m.tobytes() == gm.tobytes() and list(em) == list(gem)


def test_no_cpu_fallback():
    import torch
    from toypathtracer_amd import api
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(api.TptError, match="no HIP device"):
        api.InitializeTest()
    import numpy as np
    with pytest.raises(api.TptError):
        api.DrawTest(0.0, 0, 8, 8, np.zeros((8, 8, 4), np.float32), 2)


def test_product_never_references_oracle():
    """toypathtracer_amd/ and include/ must not import, link or mention anything under oracle/."""
    bad = []
    for base in ("toypathtracer_amd", "include"):
        for dirpath, _d, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".h", ".hip", ".cpp", ".sh")):
                    text = open(os.path.join(dirpath, f)).read()
                    if re.search(r"oracle/|oracle_lib|tpt_oracle|libtpt_ref", text) and "pinned" not in f:
                        for line in text.splitlines():
                            if re.search(r"#include|import |CDLL|dlopen|-l", line) and re.search(r"oracle|libtpt_ref", line):
                                bad.append((f, line))
    assert not bad, bad


def test_host_written_against_the_reference_header_links(tmp_path):
    """Link-level drop-in, from the other side: examples/headless_host.cpp compiled against the REFERENCE's own Test.h
    (-DUSE_REFERENCE_HEADER, nothing of this repo's include/ on the path; oracle/build_ref.sh compiles it into
    oracle/_ref/headless_host_refheader.o) links against libtoypathtracer_hip.so with no unresolved symbol.  Link only."""
    from toypathtracer_amd import api
    obj = os.path.join(ROOT, "oracle", "_ref", "headless_host_refheader.o")
    if not os.path.exists(obj):
        pytest.skip("oracle/_ref/headless_host_refheader.o not built (needs the reference's sources: oracle/build_ref.sh)")
    exe = str(tmp_path / "host_ref_header")
    lib_dir = os.path.dirname(api.library_path())
    subprocess.check_call(["g++", obj, "-L", lib_dir, "-ltoypathtracer_hip", "-Wl,-rpath," + lib_dir, "-Wl,--no-undefined", "-o", exe])
    out = subprocess.check_output(["nm", "-u", exe]).decode()
    for sym in api.CXX_ABI_SYMBOLS[:4]:  # InitializeTest, ShutdownTest, UpdateTest, DrawTest are what the host calls
        assert sym in out, sym
