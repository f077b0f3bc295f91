"""ctypes mirror of the reference's Test API (Cpp/Source/Test.h:10-17) over libtoypathtracer_hip.so.

Function names, argument order and meaning follow the reference so that tests read like a host of
the reference would (Cs/Program.cs:16-31, Cpp/Windows/TestWin.cpp:308-340):

    InitializeTest(); UpdateTest(t, frame, w, h, flags); rays = DrawTest(t, frame, w, h, backbuffer, flags)

Only plain pointers/ints/floats cross the boundary (include/tpt_hip.h).  Errors raise TptError;
nothing here renders on the CPU.
"""
import ctypes as C
import os

import numpy as np

kFlagAnimate = 1 << 0      # Test.h:6
kFlagProgressive = 1 << 1  # Test.h:7
SEED_ROW_SERIAL, SEED_PER_PIXEL = 0, 1
FOLD_RECURSIVE, FOLD_FORWARD = 0, 1
FLAG_ANIMATE, FLAG_PROGRESSIVE = 1, 2  # include/tpt_hip.h: TPT_FLAG_*

# layout contract of the reference (TestWin.cpp:132-134): 20 / 36 / 88 bytes
SPHERE_DT = np.dtype([("cx", "<f4"), ("cy", "<f4"), ("cz", "<f4"), ("radius", "<f4"), ("invRadius", "<f4")])
MATERIAL_DT = np.dtype([("type", "<i4"), ("albedo", "<f4", 3), ("emissive", "<f4", 3), ("roughness", "<f4"), ("ri", "<f4")])
CAMERA_DT = np.dtype([("origin", "<f4", 3), ("lowerLeftCorner", "<f4", 3), ("horizontal", "<f4", 3), ("vertical", "<f4", 3),
                      ("uu", "<f4", 3), ("vv", "<f4", 3), ("ww", "<f4", 3), ("lensRadius", "<f4")])


class TptError(RuntimeError):
    pass


_lib = None        # the library the module's functions currently talk to
_product = None    # libtoypathtracer_hip.so
_hooks = None      # libtoypathtracer_hip_hooks.so (the same sources + include/tpt_test_hooks.h), loaded by using_hooks()

# every symbol include/tpt_hip.h declares (checked by tests/test_abi.py)
C_ABI_SYMBOLS = [
    "tptInitialize", "tptShutdown", "tptUpdate", "tptDraw", "tptGetObjectCount", "tptGetSceneDesc",
    "tptSetSamplesPerPixel", "tptSetConfig", "tptSetSeedMode", "tptSetFoldMode", "tptSetScene", "tptSetCamera", "tptSetStream",
    "tptSetRowShard", "tptLocalRowCount", "tptLocalRowToGlobal", "tptDrawDevice", "tptRayCounterRead", "tptSetRayCounter", "tptSetFrameOverlap", "tptDisplayRGBA8", "tptKernelTimingBegin", "tptKernelTimingEnd",
    "tptSynchronize", "tptTimerBegin", "tptTimerEnd", "tptSetKernelVariant",
    "tptDrawDeviceBatch", "tptDrawDeviceViews", "tptDrawDeviceAnimation", "tptDrawDeviceAov", "tptDenoiseDevice", "tptDrawDeviceMoments", "tptDrawDeviceBatchMoments", "tptDrawDeviceAnimationMoments", "tptDrawDeviceCameraClip", "tptDrawDeviceKeyframeClip", "tptDenoiseDeviceVariance", "tptTemporalAccumulateDevice", "tptObjectPlaneDevice", "tptObjectMotionTable", "tptTemporalAccumulateObjectsDevice", "tptDenoiseClipDevice", "tptMotionVectorsDevice", "tptRectifyHistoryDevice", "tptSpatialVarianceDevice", "tptTraceRaysDevice", "tptDrawDeviceLens", "tptDrawDeviceAdaptive", "tptAdaptiveSamplesDevice", "tptDrawShardedBatch", "tptGetLookaheadHits", "tptCommGetUniqueId", "tptCommInit", "tptCommInitLoopback", "tptCommInfo", "tptCommDestroy", "tptDrawSharded", "tptSetShardExchangeInterval", "tptShardedFinish", "tptGetLaunchInfo", "tptGetPipelineInfo", "tptGetSceneInfo", "tptSetHostBufferMode", "tptSetHostLookahead", "tptSetStreamBatching", "tptSetTileMirror", "tptGetLastError", "tptSetErrorHandler", "tptGetDeviceName",
]
# include/tpt_test_hooks.h: exported by the second build (libtoypathtracer_hip_hooks.so) only
HOOK_SYMBOLS = ["tptTestMath", "tptTestMathExhaustive", "tptTestHitSpheres", "tptTestMatrixFilter", "tptTestGroupFilter", "tptTestSetDealCapacities", "tptDebugStats", "tptDebugChunkOrder", "tptTestPresetStreamCut", "tptTestStreamFrameRays"]
# the reference's own C++ symbols (nm of the compiled Test.cpp), exported for link-level drop-in
CXX_ABI_SYMBOLS = [
    "_Z14InitializeTestv", "_Z12ShutdownTestv", "_Z10UpdateTestfiiij", "_Z8DrawTestfiiiPfRij",
    "_Z14GetObjectCountRiS_S_S_", "_Z12GetSceneDescPvS_S_S_Pi",
]


class ClipDenoiseArgs(C.Structure):
    """include/tpt_hip.h: tptClipDenoiseArgs (tests/test_clip_denoise_abi.py holds the layout against the header)"""
    _fields_ = ([("screenWidth", C.c_int), ("screenHeight", C.c_int), ("nFrames", C.c_int), ("clipFlags", C.c_uint)]
                + [(name, C.c_void_p) for name in ("deviceFrameImages", "deviceFrameMoments", "deviceFrameAlbedo", "deviceFrameNormalDepth",
                                                   "cameras", "deviceFrameObjects", "deviceFrameObjectMotion", "deviceFrameOut",
                                                   "prevCamera", "devicePrevNormalDepth", "devicePrevObject", "deviceHistory")]
                + [("nObjects", C.c_int), ("iterations", C.c_int), ("denoiseFlags", C.c_uint)]
                + [(name, C.c_float) for name in ("samples", "sigmaLuminance", "sigmaNormal", "sigmaDepth", "maxHistory", "depthTolerance",
                                                  "normalTolerance", "coverageTolerance")])


class MotionVectorsArgs(C.Structure):
    """include/tpt_hip.h: tptMotionVectorsArgs (tests/test_flow_abi.py holds the layout against the header)"""
    _fields_ = ([("screenWidth", C.c_int), ("screenHeight", C.c_int), ("nFrames", C.c_int), ("flags", C.c_uint)]
                + [(name, C.c_void_p) for name in ("cameras", "deviceFrameAlbedo", "deviceFrameNormalDepth", "deviceFrameObjects",
                                                   "deviceFrameObjectMotion", "deviceFrameMotion", "prevCamera", "devicePrevAlbedo",
                                                   "devicePrevNormalDepth", "devicePrevObject")]
                + [("nObjects", C.c_int)]
                + [(name, C.c_float) for name in ("depthTolerance", "normalTolerance", "coverageTolerance")])


class TraceRaysArgs(C.Structure):
    """include/tpt_hip.h: tptTraceRaysArgs (tests/test_rays_abi.py holds the layout against the header)"""
    _fields_ = [("nRays", C.c_int), ("flags", C.c_uint), ("deviceRays", C.c_void_p), ("deviceRadiance", C.c_void_p),
                ("deviceHits", C.c_void_p), ("deviceRayCount", C.c_void_p)]


class Lens(C.Structure):
    """include/tpt_hip.h: tptLens (tests/test_lens_abi.py holds the layout against the header)"""
    _fields_ = [("kind", C.c_int), ("origin", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("forward", C.c_float * 3), ("sx", C.c_float), ("sy", C.c_float), ("maxAngle", C.c_float)]


class DrawLensArgs(C.Structure):
    """include/tpt_hip.h: tptDrawLensArgs"""
    _fields_ = [("screenWidth", C.c_int), ("screenHeight", C.c_int), ("frameCount", C.c_int), ("flags", C.c_uint), ("lens", Lens),
                ("deviceTile", C.c_void_p), ("deviceRayCount", C.c_void_p)]


def _lib_dir():
    # TPT_LIB_DIR: a directory holding another build of BOTH libraries (csrc/build.sh with TPT_OUT_DIR / TPT_EXTRA_FLAGS)
    return os.environ.get("TPT_LIB_DIR") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")


def library_path():
    # TPT_LIB selects an alternative BUILD OF THE SAME HIP LIBRARY (e.g. the -DTPT_STATS profiling build)
    return os.environ.get("TPT_LIB") or os.path.join(_lib_dir(), "libtoypathtracer_hip.so")


def hooks_library_path():
    # (a profiling build selected with TPT_LIB carries the hooks itself: tools/build_variant.sh passes -DTPT_TEST_HOOKS)
    return os.environ.get("TPT_LIB") or os.path.join(_lib_dir(), "libtoypathtracer_hip_hooks.so")


def _bind(path, hooks):
    lib = C.CDLL(path)
    i, f, u, p = C.c_int, C.c_float, C.c_uint, C.c_void_p
    sigs = {
        "tptInitialize": [], "tptShutdown": [], "tptUpdate": [f, i, i, i, u],
        "tptDraw": [f, i, i, i, p, C.POINTER(i), u],
        "tptGetObjectCount": [C.POINTER(i)] * 4, "tptGetSceneDesc": [p, p, p, p, C.POINTER(i)],
        "tptSetSamplesPerPixel": [i], "tptSetConfig": [i, f, i], "tptSetSeedMode": [i], "tptSetFoldMode": [i], "tptSetScene": [p, p, i],
        "tptSetCamera": [p, p, f, f, f], "tptSetStream": [p], "tptSetRowShard": [i, i, i], "tptLocalRowCount": [i],
        "tptLocalRowToGlobal": [i], "tptDrawDevice": [f, i, i, i, p, u], "tptRayCounterRead": [C.POINTER(C.c_int64)],
        "tptSetRayCounter": [p], "tptSetTileMirror": [p, p], "tptSetFrameOverlap": [i], "tptDisplayRGBA8": [p, i, i, p], "tptKernelTimingBegin": [i],
        "tptKernelTimingEnd": [C.POINTER(f), C.POINTER(i)],
        "tptSynchronize": [], "tptTimerBegin": [], "tptTimerEnd": [C.POINTER(f)], "tptSetKernelVariant": [i, i, i],
        "tptGetLaunchInfo": [C.POINTER(i)] * 4, "tptGetPipelineInfo": [C.POINTER(i)] * 4, "tptGetSceneInfo": [C.POINTER(i)] * 3, "tptCommGetUniqueId": [p], "tptCommInit": [p, i, i, i], "tptCommInitLoopback": [i, i], "tptCommInfo": [C.POINTER(i)] * 3, "tptCommDestroy": [], "tptDrawSharded": [f, i, i, i, p, u], "tptSetShardExchangeInterval": [i], "tptDrawShardedBatch": [f, i, i, i, i, p, u], "tptDrawDeviceBatch": [f, i, i, i, i, p, u], "tptDrawDeviceViews": [f, i, i, i, i, p, p, p, u], "tptDrawDeviceAnimation": [i, i, p, i, i, p, p, p, u], "tptDrawDeviceAov": [f, i, i, i, p, p, p, u], "tptDenoiseDevice": [i, i, p, p, p, p, i, f, f, f, u], "tptDrawDeviceMoments": [f, i, i, i, p, p, p, p, u], "tptDrawDeviceBatchMoments": [f, i, i, i, i, p, p, p, p, u], "tptDrawDeviceAnimationMoments": [i, i, p, i, i] + [p] * 7 + [u], "tptDrawDeviceCameraClip": [i, i, p, p, i, i] + [p] * 8 + [u], "tptDrawDeviceKeyframeClip": [i, i, p, i, p, p, i, i] + [p] * 9 + [u], "tptDenoiseDeviceVariance": [i, i, p, p, p, p, f, p, i, f, f, f, u], "tptTemporalAccumulateDevice": [i, i] + [p] * 14 + [f] * 4, "tptObjectPlaneDevice": [i, p, p, i, i, p, u], "tptObjectMotionTable": [f, f, u, p, i], "tptTemporalAccumulateObjectsDevice": [i, i] + [p] * 14 + [f] * 4 + [p, p, p, i], "tptDenoiseClipDevice": [C.POINTER(ClipDenoiseArgs)], "tptMotionVectorsDevice": [C.POINTER(MotionVectorsArgs)], "tptRectifyHistoryDevice": [i, i] + [p] * 7 + [i, f], "tptSpatialVarianceDevice": [i, i, i, p, p, p, f, f, i, f, f], "tptTraceRaysDevice": [C.POINTER(TraceRaysArgs)], "tptDrawDeviceLens": [C.POINTER(DrawLensArgs)], "tptDrawDeviceAdaptive": [f, i, i, i, p, p, p, p, p, u], "tptAdaptiveSamplesDevice": [i, i, p, f, i, i, p, p, p], "tptShardedFinish": [C.POINTER(C.c_int64)], "tptSetHostBufferMode": [i], "tptGetLookaheadHits": [C.POINTER(C.c_longlong)], "tptSetHostLookahead": [i], "tptSetStreamBatching": [i],
    }
    if hooks:
        sigs.update({"tptDebugStats": [p, i], "tptDebugChunkOrder": [p, p, i], "tptTestMath": [i, p, p, p, i], "tptTestMathExhaustive": [i, u, u, p, p],
                     "tptTestHitSpheres": [i, p, p, p, i], "tptTestMatrixFilter": [p, p, p, p, i], "tptTestGroupFilter": [p, i, p, p, p], "tptTestSetDealCapacities": [i, i, i], "tptTestPresetStreamCut": [i], "tptTestStreamFrameRays": [p, i]})
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = i
    lib.tptGetLastError.restype = C.c_char_p
    lib.tptGetDeviceName.restype = C.c_char_p
    return lib


def _preload():
    try:  # torch ships its own HIP runtime: load it first so both sides share one libamdhip64 in the process
        import torch  # noqa: F401
    except ImportError:
        pass


def load_library():
    """dlopen the HIP library (built by __graft_entry__.build() / csrc/build.sh). Fails loudly."""
    global _lib, _product
    if _lib is not None:
        return _lib
    _preload()
    path = library_path()
    if not os.path.exists(path):
        raise TptError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(toypathtracer_amd/csrc/build.sh). There is no CPU fallback.")
    _product = _bind(path, hooks=bool(os.environ.get("TPT_LIB")) and _has_hooks(path))
    _lib = _product
    return _lib


def _has_hooks(path):
    try:
        return hasattr(C.CDLL(path), "tptTestMath")
    except OSError:
        return False


class using_hooks:
    """Context manager: inside it every function of this module talks to the HOOKS build of the library
    (libtoypathtracer_hip_hooks.so: the same sources plus the unit-test entry points of include/tpt_test_hooks.h), which is
    initialised on first use and has its own context -- scene, knobs and pipeline are separate from the product library's.
    Used by the GPU suite for math / HitSpheres / filter unit tests; every render test runs on the product library."""

    def __enter__(self):
        global _lib, _hooks
        load_library()
        if _hooks is None:
            path = hooks_library_path()
            if path == library_path():
                _hooks = _product
            else:
                if not os.path.exists(path):
                    raise TptError(f"{path} is missing (toypathtracer_amd/csrc/build.sh builds it beside the product library)")
                _hooks = _bind(path, hooks=True)
        self._prev = _lib
        _lib = _hooks
        _chk(_lib.tptInitialize(), "tptInitialize (hooks build)")
        return self

    def __exit__(self, *exc):
        # the hooks context is shut down again: its 16 trace streams would otherwise share the process's hardware queues with the
        # product library for the rest of the session (more streams than queues is a cliff: DESIGN 3.4)
        global _lib
        if _lib is not _product:
            _lib.tptShutdown()
        _lib = self._prev
        return False


def shutdown_hooks():
    global _hooks
    if _hooks is not None and _hooks is not _product:
        _hooks.tptShutdown()
    _hooks = None


def _hook(name):
    """an entry point of include/tpt_test_hooks.h: only the hooks build has it"""
    fn = getattr(load_library(), name, None)
    if fn is None:
        raise TptError(f"{name} is a unit-test hook (include/tpt_test_hooks.h): call it inside `with api.using_hooks():` -- the product library does not export it")
    return fn


def _chk(rc, where):
    if rc != 0:
        raise TptError(f"{where}: {_lib.tptGetLastError().decode()}")


# ---------------------------------------------------------------- the reference API
def InitializeTest():
    _chk(load_library().tptInitialize(), "InitializeTest")


def ShutdownTest():
    _chk(load_library().tptShutdown(), "ShutdownTest")


def UpdateTest(time, frameCount, screenWidth, screenHeight, testFlags):
    _chk(load_library().tptUpdate(time, frameCount, screenWidth, screenHeight, testFlags), "UpdateTest")


def DrawTest(time, frameCount, screenWidth, screenHeight, backbuffer, testFlags):
    """backbuffer: C-contiguous float32 numpy array of screenWidth*screenHeight*4, modified in place.
    Returns outRayCount."""
    assert isinstance(backbuffer, np.ndarray) and backbuffer.dtype == np.float32 and backbuffer.flags.c_contiguous
    assert backbuffer.size == screenWidth * screenHeight * 4
    rays = C.c_int(0)
    _chk(load_library().tptDraw(time, frameCount, screenWidth, screenHeight, backbuffer.ctypes.data, C.byref(rays),
                                testFlags), "DrawTest")
    return rays.value


def GetObjectCount():
    v = [C.c_int() for _ in range(4)]
    _chk(load_library().tptGetObjectCount(*[C.byref(x) for x in v]), "GetObjectCount")
    return tuple(x.value for x in v)


def GetSceneDesc():
    n, so, sm, sc = GetObjectCount()
    assert (so, sm, sc) == (SPHERE_DT.itemsize, MATERIAL_DT.itemsize, CAMERA_DT.itemsize)
    s, m, cam = np.zeros(n, SPHERE_DT), np.zeros(n, MATERIAL_DT), np.zeros(1, CAMERA_DT)
    em = np.zeros(n, np.int32)
    cnt = C.c_int()
    _chk(load_library().tptGetSceneDesc(s.ctypes.data, m.ctypes.data, cam.ctypes.data, em.ctypes.data, C.byref(cnt)),
         "GetSceneDesc")
    return s, m, cam, em[:cnt.value].copy()


# ---------------------------------------------------------------- run-time knobs / device path
def set_samples_per_pixel(spp):
    _chk(load_library().tptSetSamplesPerPixel(spp), "tptSetSamplesPerPixel")


def set_config(light_sampling=True, animate_smoothing=0.9, mitsuba_compare=False):
    _chk(load_library().tptSetConfig(1 if light_sampling else 0, animate_smoothing, 1 if mitsuba_compare else 0), "tptSetConfig")


def set_seed_mode(mode):
    _chk(load_library().tptSetSeedMode(mode), "tptSetSeedMode")


def set_fold_mode(mode):
    _chk(load_library().tptSetFoldMode(mode), "tptSetFoldMode")


ERROR_HANDLER = C.CFUNCTYPE(None, C.c_char_p, C.c_char_p)
_error_handler_keepalive = None


def set_error_handler(fn):
    """tptSetErrorHandler: fn(where: bytes, message: bytes) is called when one of the reference's void functions fails, instead of
    abort(); None restores the default."""
    global _error_handler_keepalive
    cb = ERROR_HANDLER(fn) if fn is not None else C.cast(None, ERROR_HANDLER)
    lib = load_library()
    lib.tptSetErrorHandler.argtypes = [ERROR_HANDLER]
    _chk(lib.tptSetErrorHandler(cb), "tptSetErrorHandler")
    _error_handler_keepalive = cb


def set_kernel_variant(hit_spheres=0, persistent=3, lds_scene=-1):
    _chk(load_library().tptSetKernelVariant(hit_spheres, persistent, lds_scene), "tptSetKernelVariant")


def set_scene(spheres=None, materials=None):
    lib = load_library()
    if spheres is None:
        _chk(lib.tptSetScene(None, None, 0), "tptSetScene")
        return
    s = np.ascontiguousarray(spheres, SPHERE_DT)
    m = np.ascontiguousarray(materials, MATERIAL_DT)
    assert len(s) == len(m)
    _chk(lib.tptSetScene(s.ctypes.data, m.ctypes.data, len(s)), "tptSetScene")


def set_camera(look_from=None, look_at=None, vfov=60.0, aperture=0.02, focus_dist=3.0):
    lib = load_library()
    if look_from is None:
        _chk(lib.tptSetCamera(None, None, 0.0, 0.0, 0.0), "tptSetCamera")
        return
    a = np.asarray(look_from, np.float32)
    b = np.asarray(look_at, np.float32)
    _chk(lib.tptSetCamera(a.ctypes.data, b.ctypes.data, vfov, aperture, focus_dist), "tptSetCamera")


def set_stream(stream_handle):
    _chk(load_library().tptSetStream(C.c_void_p(stream_handle) if stream_handle else None), "tptSetStream")


def set_row_shard(stripe_rows, num_parts, part):
    _chk(load_library().tptSetRowShard(stripe_rows, num_parts, part), "tptSetRowShard")


def local_row_count(height):
    return load_library().tptLocalRowCount(height)


def local_row_to_global(local_row):
    return load_library().tptLocalRowToGlobal(local_row)


def draw_device(time, frameCount, screenWidth, screenHeight, device_ptr, testFlags):
    """Asynchronous DrawTest into a device-resident tile (raw device pointer, e.g. tensor.data_ptr())."""
    _chk(load_library().tptDrawDevice(time, frameCount, screenWidth, screenHeight, C.c_void_p(device_ptr), testFlags),
         "tptDrawDevice")


def ray_counter_read():
    v = C.c_int64()
    _chk(load_library().tptRayCounterRead(C.byref(v)), "tptRayCounterRead")
    return v.value


def set_frame_overlap(frames):
    _chk(load_library().tptSetFrameOverlap(frames), "tptSetFrameOverlap")


def display_rgba8(device_tile_ptr, width, height, device_rgba_ptr):
    """linear float4 image (device) -> RGBA8 (device), the reference's sqrt display transform, top row first"""
    _chk(load_library().tptDisplayRGBA8(C.c_void_p(device_tile_ptr), width, height, C.c_void_p(device_rgba_ptr)), "tptDisplayRGBA8")


def write_tga(path, rgba):
    """rgba: uint8 [h, w, 4], top row first.  Uncompressed 32-bit TGA like the reference's only image writer
    (Cs/Program.cs:33-59: BGRA, bottom-left origin)."""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    header = bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, w & 0xFF, (w >> 8) & 0xFF, h & 0xFF, (h >> 8) & 0xFF, 32, 0])
    with open(path, "wb") as f:
        f.write(header)
        f.write(rgba[::-1, :, [2, 1, 0, 3]].tobytes())


def set_ray_counter(device_ptr):
    """device_ptr: address of one zeroed int64 in device memory (tensor.data_ptr()), or None/0 for the internal one."""
    _chk(load_library().tptSetRayCounter(C.c_void_p(device_ptr) if device_ptr else None), "tptSetRayCounter")


def set_tile_mirror(mirror_ptr, counter_out_ptr=None):
    """The resolve kernel also writes the blended tile to `mirror_ptr` and the ray counter to `counter_out_ptr` (device
    addresses; None/0 turns it off)."""
    _chk(load_library().tptSetTileMirror(C.c_void_p(mirror_ptr) if mirror_ptr else None,
                                         C.c_void_p(counter_out_ptr) if counter_out_ptr else None), "tptSetTileMirror")


def synchronize():
    _chk(load_library().tptSynchronize(), "tptSynchronize")


def timer_begin():
    _chk(load_library().tptTimerBegin(), "tptTimerBegin")


def timer_end():
    ms = C.c_float()
    _chk(load_library().tptTimerEnd(C.byref(ms)), "tptTimerEnd")
    return ms.value


def kernel_timing_begin(max_launches):
    _chk(load_library().tptKernelTimingBegin(max_launches), "tptKernelTimingBegin")


def kernel_timing_end():
    """-> (sum of the individual trace-launch durations in ms, number of launches)"""
    ms, n = C.c_float(), C.c_int()
    _chk(load_library().tptKernelTimingEnd(C.byref(ms), C.byref(n)), "tptKernelTimingEnd")
    return ms.value, n.value


def launch_info():
    v = [C.c_int() for _ in range(4)]
    load_library().tptGetLaunchInfo(*[C.byref(x) for x in v])
    return dict(blocks_per_cu=v[0].value, lds_bytes=v[1].value, grid_blocks=v[2].value, num_cus=v[3].value)


def comm_get_unique_id():
    buf = (C.c_char * 128)()
    _chk(load_library().tptCommGetUniqueId(buf), "tptCommGetUniqueId")
    return bytes(buf)


def comm_init(unique_id, n_ranks, rank, stripe_rows=8):
    _chk(load_library().tptCommInit(C.c_char_p(unique_id), n_ranks, rank, stripe_rows), "tptCommInit")


def comm_init_loopback(n_ranks, stripe_rows=8):
    """Measurement aid: play rank 0 of an n_ranks-way sharded run alone (device copy in place of the gather)."""
    _chk(load_library().tptCommInitLoopback(n_ranks, stripe_rows), "tptCommInitLoopback")


def comm_info():
    """(ranks, rank, loopback) as the communicator itself reports them (ncclCommCount / ncclCommUserRank)"""
    v = [C.c_int() for _ in range(3)]
    _chk(load_library().tptCommInfo(*[C.byref(x) for x in v]), "tptCommInfo")
    return v[0].value, v[1].value, bool(v[2].value)


def comm_destroy():
    _chk(load_library().tptCommDestroy(), "tptCommDestroy")


def draw_sharded(time, frameCount, screenWidth, screenHeight, device_image_ptr, testFlags):
    _chk(load_library().tptDrawSharded(time, frameCount, screenWidth, screenHeight, device_image_ptr, testFlags), "tptDrawSharded")


def set_shard_exchange_interval(k):
    """0 = automatic (every frame for big tiles, every 2nd / 4th for small ones), k >= 1 = every k-th frame; same on every rank"""
    _chk(load_library().tptSetShardExchangeInterval(k), "tptSetShardExchangeInterval")


def draw_sharded_batch(time, firstFrame, nFrames, screenWidth, screenHeight, device_image_ptr, testFlags):
    _chk(load_library().tptDrawShardedBatch(time, firstFrame, nFrames, screenWidth, screenHeight, device_image_ptr, testFlags), "tptDrawShardedBatch")


def draw_device_batch(time, firstFrame, nFrames, screenWidth, screenHeight, device_tile_ptr, testFlags):
    """nFrames consecutive frames in one launch (static scene); same bits as nFrames draw_device calls."""
    _chk(load_library().tptDrawDeviceBatch(time, firstFrame, nFrames, screenWidth, screenHeight, device_tile_ptr, testFlags), "tptDrawDeviceBatch")


def draw_device_views(time, frame, w, h, views, device_tiles_ptr, testFlags, view_rays_ptr=None):
    """len(views) cameras of one frame in one launch.  views: array-like (N, 9) of {lookFrom xyz, lookAt xyz, vfov, aperture,
    focusDist}; device_tiles_ptr: N consecutive device tiles of h*w*4 floats; view_rays_ptr: None or N int64 in device memory,
    overwritten with each view's rays.  View v equals set_camera(views[v]) + UpdateTest + draw_device on its tile."""
    v = np.ascontiguousarray(views, dtype=np.float32)
    if v.ndim != 2 or v.shape[1] != 9:
        raise ValueError("views: shape (N, 9) expected, got %r" % (v.shape,))
    _chk(load_library().tptDrawDeviceViews(time, frame, w, h, v.shape[0], v.ctypes.data if v.size else None, device_tiles_ptr,
                                           view_rays_ptr, testFlags), "tptDrawDeviceViews")


def draw_device_animation(times, first_frame, w, h, tile_ptr, flags, frame_images_ptr=None, frame_rays_ptr=None):
    """len(times) frames of the animated scene in launches of up to 32 frames.  Frame j equals UpdateTest(times[j], first_frame + j)
    + draw_device on tile_ptr; frame_images_ptr: None or len(times) device tiles of h*w*4 floats, tile j = the tile right after frame j;
    frame_rays_ptr: None or len(times) int64 in device memory, overwritten with each frame's rays."""
    t = np.ascontiguousarray(times, dtype=np.float32)
    if t.ndim != 1:
        raise ValueError("times: a 1-D sequence expected, got shape %r" % (t.shape,))
    _chk(load_library().tptDrawDeviceAnimation(first_frame, t.shape[0], t.ctypes.data if t.size else None, w, h, tile_ptr,
                                               frame_images_ptr, frame_rays_ptr, flags), "tptDrawDeviceAnimation")


def _positive_ints(*named):
    """(name, value) pairs: ValueError for the first value that is not an int > 0"""
    for name, v in named:
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v <= 0:
            raise ValueError("%s: a positive int expected, got %r" % (name, v))


def _pointers(*named):
    """(name, value) pairs: ValueError for the first value that is neither None nor a device pointer (an int >= 0)"""
    for name, v in named:
        if v is not None and (not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 0):
            raise ValueError("%s: a device pointer (int) or None expected, got %r" % (name, v))


def _sigmas(*named):
    """(name, value) pairs: ValueError for the first value that is not a finite number >= 0"""
    for name, v in named:
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool) or not v >= 0 or v == float("inf"):
            raise ValueError("%s: a finite float >= 0 expected, got %r" % (name, v))


def draw_device_aov(time, frame, w, h, tile_ptr, flags, albedo_ptr=None, normal_depth_ptr=None):
    """draw_device on tile_ptr (same bits, same ray count) plus the first-hit planes of the samples: albedo_ptr / normal_depth_ptr, device
    buffers of h*w*4 floats (None = not wanted; at least one), overwritten with {albedo, coverage} / {normal, depth} averaged over the
    samples.  Ordered on the context's stream like the tile."""
    _positive_ints(("w", w), ("h", h))
    _pointers(("tile_ptr", tile_ptr), ("albedo_ptr", albedo_ptr), ("normal_depth_ptr", normal_depth_ptr))
    if not tile_ptr:
        raise ValueError("tile_ptr: a device tile is required")
    if not albedo_ptr and not normal_depth_ptr:
        raise ValueError("albedo_ptr, normal_depth_ptr: at least one plane is required")
    _chk(load_library().tptDrawDeviceAov(time, frame, w, h, C.c_void_p(tile_ptr), C.c_void_p(albedo_ptr) if albedo_ptr else None,
                                         C.c_void_p(normal_depth_ptr) if normal_depth_ptr else None, flags), "tptDrawDeviceAov")


DENOISE_DEMODULATE = 1  # include/tpt_hip.h: TPT_DENOISE_DEMODULATE
# denoise_device's defaults, chosen by tools/denoise_rate.py's sweep
DENOISE_DEFAULTS = dict(iterations=5, sigma_colour=32.0, sigma_normal=0.03, sigma_depth=0.5)


def denoise_device(w, h, colour_ptr, out_ptr, albedo_ptr=None, normal_depth_ptr=None, iterations=DENOISE_DEFAULTS["iterations"],
                   sigma_colour=DENOISE_DEFAULTS["sigma_colour"], sigma_normal=DENOISE_DEFAULTS["sigma_normal"],
                   sigma_depth=DENOISE_DEFAULTS["sigma_depth"], demodulate=None):
    """tptDenoiseDevice: the edge-avoiding a-trous filter of the tile at colour_ptr into out_ptr (device buffers of h*w*4 floats), guided
    by draw_device_aov's planes (None = not given).  A guide's sigma is ignored (passed as 0) when its plane is not given; demodulate=None
    means "on if an albedo plane is given".  The default sigmas are DESIGN.md's measured choice.  Ordered on the context's stream."""
    _positive_ints(("w", w), ("h", h), ("iterations", iterations))
    _pointers(("colour_ptr", colour_ptr), ("out_ptr", out_ptr), ("albedo_ptr", albedo_ptr), ("normal_depth_ptr", normal_depth_ptr))
    if not colour_ptr or not out_ptr:
        raise ValueError("colour_ptr, out_ptr: device buffers are required")
    _sigmas(("sigma_colour", sigma_colour), ("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth))
    if demodulate is None:
        demodulate = bool(albedo_ptr)
    if demodulate and not albedo_ptr:
        raise ValueError("demodulate: needs albedo_ptr")
    if not normal_depth_ptr:
        sigma_normal = sigma_depth = 0.0
    _chk(load_library().tptDenoiseDevice(w, h, C.c_void_p(colour_ptr), C.c_void_p(albedo_ptr) if albedo_ptr else None,
                                         C.c_void_p(normal_depth_ptr) if normal_depth_ptr else None, C.c_void_p(out_ptr), iterations,
                                         sigma_colour, sigma_normal, sigma_depth, DENOISE_DEMODULATE if demodulate else 0), "tptDenoiseDevice")


def draw_device_moments(time, frame, w, h, tile_ptr, moments_ptr, flags, albedo_ptr=None, normal_depth_ptr=None):
    """draw_device_aov (same tile bits, same ray count, the same planes where given; both may be None) plus the luminance moments of the
    frame's samples, blended into moments_ptr (a device buffer of h*w*4 floats) with the tile's lerp factor: {mean l, mean l^2, 0} of
    l = (0.2126 r + 0.7152 g) + 0.0722 b, .w kept.  Ordered on the context's stream like the tile."""
    _positive_ints(("w", w), ("h", h))
    _pointers(("tile_ptr", tile_ptr), ("moments_ptr", moments_ptr), ("albedo_ptr", albedo_ptr), ("normal_depth_ptr", normal_depth_ptr))
    if not tile_ptr or not moments_ptr:
        raise ValueError("tile_ptr, moments_ptr: device buffers are required")
    _chk(load_library().tptDrawDeviceMoments(time, frame, w, h, C.c_void_p(tile_ptr), C.c_void_p(albedo_ptr) if albedo_ptr else None,
                                             C.c_void_p(normal_depth_ptr) if normal_depth_ptr else None, C.c_void_p(moments_ptr), flags),
         "tptDrawDeviceMoments")


def draw_device_batch_moments(time, first_frame, n_frames, w, h, tile_ptr, moments_ptr, flags, albedo_ptr=None, normal_depth_ptr=None):
    """n_frames consecutive frames (first_frame ...) of the scene and camera of the last UpdateTest, up to 32 per launch, folded into the
    four planes denoise_device_variance reads: the same bits and ray counts as n_frames draw_device_moments calls on tile_ptr and
    moments_ptr, with each frame's guide planes blended into albedo_ptr / normal_depth_ptr (None = not wanted) with the tile's lerp factor,
    all four channels: a progressive still ends with guides averaged as the tile is.  flags: kFlagProgressive or 0.  Afterwards
    samples = moment_samples(spp, first_frame + n_frames - 1, flags).  Ordered on the context's stream like the tile."""
    _positive_ints(("w", w), ("h", h), ("n_frames", n_frames))
    if not isinstance(first_frame, (int, np.integer)) or isinstance(first_frame, bool) or first_frame < 0 or first_frame + n_frames - 1 > 0x7fffffff:
        raise ValueError("first_frame: an int >= 0 with first_frame + n_frames - 1 < 2**31 expected, got %r" % (first_frame,))
    _pointers(("tile_ptr", tile_ptr), ("moments_ptr", moments_ptr), ("albedo_ptr", albedo_ptr), ("normal_depth_ptr", normal_depth_ptr))
    if not tile_ptr or not moments_ptr:
        raise ValueError("tile_ptr, moments_ptr: device buffers are required")
    _chk(load_library().tptDrawDeviceBatchMoments(time, int(first_frame), n_frames, w, h, C.c_void_p(tile_ptr), C.c_void_p(moments_ptr),
                                                  C.c_void_p(albedo_ptr) if albedo_ptr else None,
                                                  C.c_void_p(normal_depth_ptr) if normal_depth_ptr else None, int(flags)),
         "tptDrawDeviceBatchMoments")


def draw_device_animation_moments(times, first_frame, w, h, tile_ptr, moments_ptr, flags, images_ptr=None, albedo_ptr=None,
                                  normal_depth_ptr=None, frame_moments_ptr=None, rays_ptr=None):
    """len(times) frames of the animated scene with their denoiser planes, in launches of up to 32 frames.  Frame j equals
    UpdateTest(times[j], first_frame + j) + draw_device_moments on tile_ptr and moments_ptr with plane j of albedo_ptr / normal_depth_ptr
    (None or len(times) device planes of h*w*4 floats each).  images_ptr / frame_moments_ptr: None or len(times) planes, plane j = the
    tile / the moments right after frame j; rays_ptr: None or len(times) int64 in device memory, overwritten with each frame's rays."""
    t = np.ascontiguousarray(times, dtype=np.float32)
    if t.ndim != 1:
        raise ValueError("times: a 1-D sequence expected, got shape %r" % (t.shape,))
    _positive_ints(("w", w), ("h", h))
    outs = (("images_ptr", images_ptr), ("albedo_ptr", albedo_ptr), ("normal_depth_ptr", normal_depth_ptr),
            ("frame_moments_ptr", frame_moments_ptr), ("rays_ptr", rays_ptr))
    _pointers(("tile_ptr", tile_ptr), ("moments_ptr", moments_ptr), *outs)
    if not tile_ptr or not moments_ptr:
        raise ValueError("tile_ptr, moments_ptr: device buffers are required")
    _chk(load_library().tptDrawDeviceAnimationMoments(first_frame, t.shape[0], t.ctypes.data if t.size else None, w, h, C.c_void_p(tile_ptr),
                                                      C.c_void_p(moments_ptr), *[C.c_void_p(v) if v else None for _, v in outs], flags),
         "tptDrawDeviceAnimationMoments")


def draw_device_camera_clip(times, views, first_frame, w, h, tile_ptr, moments_ptr, flags, images_ptr=None, albedo_ptr=None,
                            normal_depth_ptr=None, frame_moments_ptr=None, rays_ptr=None, cameras=True):
    """draw_device_animation_moments with a camera per frame, in launches of up to 32 frames.  views: array-like (N, 9) of {lookFrom xyz,
    lookAt xyz, vfov, aperture, focusDist} with N = len(times).  Frame j equals set_camera(views[j]) + UpdateTest(times[j],
    first_frame + j) + draw_device_moments on tile_ptr and moments_ptr with plane j of albedo_ptr / normal_depth_ptr; the other outputs
    as draw_device_animation_moments'.  Returns the frames' cameras as a CAMERA_DT array of N records, each what GetSceneDesc()[2] is
    after that frame's UpdateTest and ready for temporal_accumulate_device (cameras=False: not asked for, returns None)."""
    t = np.ascontiguousarray(times, dtype=np.float32)
    if t.ndim != 1:
        raise ValueError("times: a 1-D sequence expected, got shape %r" % (t.shape,))
    v = np.ascontiguousarray(views, dtype=np.float32)
    if v.ndim != 2 or v.shape[1] != 9:
        raise ValueError("views: shape (N, 9) expected, got %r" % (v.shape,))
    if v.shape[0] != t.shape[0]:
        raise ValueError("views: one view per time expected, got %d views for %d times" % (v.shape[0], t.shape[0]))
    _positive_ints(("w", w), ("h", h))
    outs = (("images_ptr", images_ptr), ("albedo_ptr", albedo_ptr), ("normal_depth_ptr", normal_depth_ptr),
            ("frame_moments_ptr", frame_moments_ptr), ("rays_ptr", rays_ptr))
    _pointers(("tile_ptr", tile_ptr), ("moments_ptr", moments_ptr), *outs)
    if not tile_ptr or not moments_ptr:
        raise ValueError("tile_ptr, moments_ptr: device buffers are required")
    cams = np.zeros(t.shape[0], CAMERA_DT) if cameras else None
    _chk(load_library().tptDrawDeviceCameraClip(first_frame, t.shape[0], t.ctypes.data if t.size else None, v.ctypes.data if v.size else None,
                                                w, h, C.c_void_p(tile_ptr), C.c_void_p(moments_ptr),
                                                *[C.c_void_p(x) if x else None for _, x in outs],
                                                cams.ctypes.data if cameras and cams.size else None, flags), "tptDrawDeviceCameraClip")
    return cams


def draw_device_keyframe_clip(views, moved_ids, centres, first_frame, w, h, tile_ptr, moments_ptr, flags, images_ptr=None, albedo_ptr=None,
                              normal_depth_ptr=None, frame_moments_ptr=None, rays_ptr=None, objects_ptr=None, cameras=True):
    """draw_device_camera_clip with the motion given by the caller, in launches of up to 32 frames.  views: array-like (N, 9); moved_ids:
    (K,) distinct sphere indices; centres: (N, K, 3), centres[j, k] where sphere moved_ids[k] stands in frame j (K = 0: nothing moves).
    Frame j equals set_scene(S_j) + set_camera(views[j]) + UpdateTest(0, first_frame + j) + draw_device_moments on tile_ptr and
    moments_ptr with plane j of albedo_ptr / normal_depth_ptr, S_j the context's spheres with the moved centres replaced; the other
    outputs as draw_device_camera_clip's.  objects_ptr: None or N device planes of h*w int32, plane j what object_plane_device gives for
    frame j's camera over S_j.  flags: kFlagProgressive or 0 (kFlagAnimate is refused).  Returns the frames' cameras as a CAMERA_DT array
    (cameras=False: not asked for, returns None)."""
    v = np.ascontiguousarray(views, dtype=np.float32)
    if v.ndim != 2 or v.shape[1] != 9:
        raise ValueError("views: shape (N, 9) expected, got %r" % (v.shape,))
    ids = np.asarray(moved_ids)
    if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
        raise ValueError("moved_ids: a 1-D sequence of integers expected, got shape %r of %s" % (ids.shape, ids.dtype))
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    c = np.ascontiguousarray(centres, dtype=np.float32)
    if ids.size == 0 and c.size == 0:
        c = np.zeros((v.shape[0], 0, 3), np.float32)
    if c.ndim != 3 or c.shape != (v.shape[0], ids.shape[0], 3):
        raise ValueError("centres: shape (N, K, 3) = (%d, %d, 3) expected, got %r" % (v.shape[0], ids.shape[0], c.shape))
    _positive_ints(("w", w), ("h", h))
    outs = (("images_ptr", images_ptr), ("albedo_ptr", albedo_ptr), ("normal_depth_ptr", normal_depth_ptr),
            ("frame_moments_ptr", frame_moments_ptr), ("rays_ptr", rays_ptr), ("objects_ptr", objects_ptr))
    _pointers(("tile_ptr", tile_ptr), ("moments_ptr", moments_ptr), *outs)
    if not tile_ptr or not moments_ptr:
        raise ValueError("tile_ptr, moments_ptr: device buffers are required")
    cams = np.zeros(v.shape[0], CAMERA_DT) if cameras else None
    _chk(load_library().tptDrawDeviceKeyframeClip(first_frame, v.shape[0], v.ctypes.data if v.size else None, ids.shape[0],
                                                  ids.ctypes.data if ids.size else None, c.ctypes.data if c.size else None, w, h,
                                                  C.c_void_p(tile_ptr), C.c_void_p(moments_ptr),
                                                  *[C.c_void_p(x) if x else None for _, x in outs],
                                                  cams.ctypes.data if cameras and cams.size else None, flags), "tptDrawDeviceKeyframeClip")
    return cams


def moment_samples(spp, frame=None, flags=0):
    """The `samples` argument of denoise_device_variance: how many samples the colour and the moments average.  A single frame (frame
    None, or flags without kFlagProgressive): spp.  A static progressive caller after its frame `frame`: spp * (frame + 1).  An animated
    progressive caller (kFlagAnimate) blends with a smoothed lerp factor, so no count follows from the frame number: it passes its own."""
    if not isinstance(spp, (int, np.integer)) or isinstance(spp, bool) or spp < 1:
        raise ValueError("spp: a positive int expected, got %r" % (spp,))
    if frame is None or not (flags & kFlagProgressive):
        return float(spp)
    if flags & kFlagAnimate:
        raise ValueError("an animated progressive caller's moments average no fixed number of samples: pass samples explicitly")
    if not isinstance(frame, (int, np.integer)) or isinstance(frame, bool) or frame < 0:
        raise ValueError("frame: an int >= 0 expected, got %r" % (frame,))
    return float(spp * (frame + 1))


# denoise_device_variance's defaults, chosen by tools/denoise_variance_rate.py's sweep
DENOISE_VARIANCE_DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.03, sigma_depth=0.5)


def denoise_device_variance(w, h, colour_ptr, moments_ptr, samples, out_ptr, albedo_ptr=None, normal_depth_ptr=None,
                            iterations=DENOISE_VARIANCE_DEFAULTS["iterations"], sigma_luminance=DENOISE_VARIANCE_DEFAULTS["sigma_luminance"],
                            sigma_normal=DENOISE_VARIANCE_DEFAULTS["sigma_normal"], sigma_depth=DENOISE_VARIANCE_DEFAULTS["sigma_depth"],
                            demodulate=None):
    """tptDenoiseDeviceVariance: the variance-guided a-trous filter of the tile at colour_ptr into out_ptr, its luminance term scaled by
    the per-pixel variance of draw_device_moments' moments (moments_ptr) over `samples` samples (moment_samples).  Guides and demodulate
    as denoise_device; a progressive caller passes guide planes averaged over its frames like the tile (include/tpt_hip.h).  Ordered on
    the context's stream."""
    _positive_ints(("w", w), ("h", h), ("iterations", iterations))
    _pointers(("colour_ptr", colour_ptr), ("moments_ptr", moments_ptr), ("out_ptr", out_ptr), ("albedo_ptr", albedo_ptr),
              ("normal_depth_ptr", normal_depth_ptr))
    if not colour_ptr or not out_ptr or not moments_ptr:
        raise ValueError("colour_ptr, moments_ptr, out_ptr: device buffers are required")
    if not isinstance(samples, (int, float, np.integer, np.floating)) or isinstance(samples, bool) or not 1 <= samples < float("inf"):
        raise ValueError("samples: a finite number >= 1 expected, got %r" % (samples,))
    if not isinstance(sigma_luminance, (int, float, np.integer, np.floating)) or isinstance(sigma_luminance, bool) or not 0 < sigma_luminance <= 1e6:
        raise ValueError("sigma_luminance: a float in (0, 1e6] expected, got %r" % (sigma_luminance,))
    _sigmas(("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth))
    if demodulate is None:
        demodulate = bool(albedo_ptr)
    if demodulate and not albedo_ptr:
        raise ValueError("demodulate: needs albedo_ptr")
    if not normal_depth_ptr:
        sigma_normal = sigma_depth = 0.0
    _chk(load_library().tptDenoiseDeviceVariance(w, h, C.c_void_p(colour_ptr), C.c_void_p(albedo_ptr) if albedo_ptr else None,
                                                 C.c_void_p(normal_depth_ptr) if normal_depth_ptr else None, C.c_void_p(moments_ptr),
                                                 samples, C.c_void_p(out_ptr), iterations, sigma_luminance, sigma_normal, sigma_depth,
                                                 DENOISE_DEMODULATE if demodulate else 0), "tptDenoiseDeviceVariance")


# temporal_accumulate_device's defaults, chosen by tools/temporal_rate.py's sweep
TEMPORAL_DEFAULTS = dict(max_history=4.0, depth_tolerance=0.1, normal_tolerance=0.25, coverage_tolerance=0.0)


def _camera_bytes(name, cam):
    """a CAMERA_DT record (GetSceneDesc's third result, or one element of it) -> its 88 bytes as a ctypes buffer; ValueError otherwise"""
    if not isinstance(cam, (np.ndarray, np.void)) or cam.dtype != CAMERA_DT or cam.size != 1:
        raise ValueError("%s: one CAMERA_DT record expected, got %r" % (name, cam))
    return C.create_string_buffer(np.ascontiguousarray(cam).tobytes(), CAMERA_DT.itemsize)


def temporal_accumulate_device(w, h, camera, colour_ptr, albedo_ptr, normal_depth_ptr, moments_ptr, out_colour_ptr, out_albedo_ptr,
                               out_moments_ptr, out_variance_ptr, prev=None, max_history=TEMPORAL_DEFAULTS["max_history"],
                               depth_tolerance=TEMPORAL_DEFAULTS["depth_tolerance"],
                               normal_tolerance=TEMPORAL_DEFAULTS["normal_tolerance"],
                               coverage_tolerance=TEMPORAL_DEFAULTS["coverage_tolerance"]):
    """tptTemporalAccumulateDevice: this frame's planes (one non-progressive draw_device_moments call on a zeroed tile and moments plane)
    blended with the history reprojected through the previous camera, into the four out planes (device buffers of h*w*4 floats each).
    camera: this frame's CAMERA_DT record (GetSceneDesc()[2]).  prev: None for the first frame of a sequence, else (camera, colour_ptr,
    albedo_ptr, normal_depth_ptr, moments_ptr) -- the previous frame's camera, the previous call's out_colour / out_albedo / out_moments
    and the previous frame's own normal/depth plane.  out_moments' .w carries the per-pixel history length; out_variance is the plane
    for denoise_device_variance's moments_ptr with samples = spp, beside out_colour, out_albedo and this frame's normal/depth plane.
    Ordered on the context's stream."""
    _positive_ints(("w", w), ("h", h))
    cur = (("colour_ptr", colour_ptr), ("albedo_ptr", albedo_ptr), ("normal_depth_ptr", normal_depth_ptr), ("moments_ptr", moments_ptr),
           ("out_colour_ptr", out_colour_ptr), ("out_albedo_ptr", out_albedo_ptr), ("out_moments_ptr", out_moments_ptr),
           ("out_variance_ptr", out_variance_ptr))
    _pointers(*cur)
    if not all(v for _, v in cur):
        raise ValueError("%s: device buffers are required" % ", ".join(n for n, v in cur if not v))
    cam = _camera_bytes("camera", camera)
    prev_cam, prev_ptrs = None, (None,) * 4
    if prev is not None:
        if not isinstance(prev, (tuple, list)) or len(prev) != 5:
            raise ValueError("prev: None or (camera, colour_ptr, albedo_ptr, normal_depth_ptr, moments_ptr) expected, got %r" % (prev,))
        prev_cam = _camera_bytes("prev camera", prev[0])
        named = tuple(zip(("prev colour_ptr", "prev albedo_ptr", "prev normal_depth_ptr", "prev moments_ptr"), prev[1:]))
        _pointers(*named)
        if not all(v for _, v in named):
            raise ValueError("prev: all four device buffers are required")
        prev_ptrs = tuple(C.c_void_p(v) for v in prev[1:])
    if not isinstance(max_history, (int, float, np.integer, np.floating)) or isinstance(max_history, bool) or not 1 <= max_history <= 65536:
        raise ValueError("max_history: a number in 1..65536 expected, got %r" % (max_history,))
    _sigmas(("depth_tolerance", depth_tolerance), ("normal_tolerance", normal_tolerance), ("coverage_tolerance", coverage_tolerance))
    _chk(load_library().tptTemporalAccumulateDevice(w, h, cam, prev_cam, C.c_void_p(colour_ptr), C.c_void_p(albedo_ptr),
                                                    C.c_void_p(normal_depth_ptr), C.c_void_p(moments_ptr), *prev_ptrs,
                                                    C.c_void_p(out_colour_ptr), C.c_void_p(out_albedo_ptr), C.c_void_p(out_moments_ptr),
                                                    C.c_void_p(out_variance_ptr), max_history, depth_tolerance, normal_tolerance,
                                                    coverage_tolerance), "tptTemporalAccumulateDevice")


# rectify_history_device's defaults, chosen from tools/rectify_rate.py's table
RECTIFY_DEFAULTS = dict(radius=1, gamma=2.0)
RECTIFY_MAX_RADIUS = 3  # include/tpt_hip.h: tptRectifyHistoryDevice's radius


def rectify_history_device(w, h, colour_ptr, moments_ptr, acc_colour_ptr, acc_moments_ptr, out_colour_ptr, out_moments_ptr,
                           out_variance_ptr, radius=RECTIFY_DEFAULTS["radius"], gamma=RECTIFY_DEFAULTS["gamma"]):
    """tptRectifyHistoryDevice: the accumulated colour of temporal_accumulate_device or temporal_accumulate_objects_device clamped to
    what this frame's (2*radius + 1)^2 window makes plausible (mean +- gamma standard deviations, widened to hold this frame's own
    value), and the history shortened where it had to be clamped.  colour_ptr, moments_ptr: this frame's planes as traced (the pass's
    current planes); acc_colour_ptr, acc_moments_ptr: the pass's out_colour and out_moments.  The three outputs (device buffers of
    h*w*4 floats) replace the pass's colour, moments and variance planes downstream: colour and moments are the next frame's prev
    planes, colour and variance go to denoise_device_variance.  out_colour_ptr may be acc_colour_ptr and out_moments_ptr
    acc_moments_ptr (in place).  Ordered on the context's stream."""
    _positive_ints(("w", w), ("h", h))
    named = (("colour_ptr", colour_ptr), ("moments_ptr", moments_ptr), ("acc_colour_ptr", acc_colour_ptr),
             ("acc_moments_ptr", acc_moments_ptr), ("out_colour_ptr", out_colour_ptr), ("out_moments_ptr", out_moments_ptr),
             ("out_variance_ptr", out_variance_ptr))
    _pointers(*named)
    if not all(v for _, v in named):
        raise ValueError("%s: device buffers are required" % ", ".join(n for n, v in named if not v))
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool) or not 1 <= radius <= RECTIFY_MAX_RADIUS:
        raise ValueError("radius: an int in 1..%d expected, got %r" % (RECTIFY_MAX_RADIUS, radius))
    _sigmas(("gamma", gamma))
    _chk(load_library().tptRectifyHistoryDevice(w, h, *[C.c_void_p(v) for _, v in named], int(radius), gamma), "tptRectifyHistoryDevice")


# spatial_variance_device's defaults, confirmed by tools/spatial_variance_rate.py's table
SPATIAL_VARIANCE_DEFAULTS = dict(min_samples=2.0, radius=1, sigma_normal=0.03, sigma_depth=0.5)
SPATIAL_VARIANCE_MAX_RADIUS = 3  # include/tpt_hip.h: tptSpatialVarianceDevice's radius
SPATIAL_VARIANCE_MAX_FRAMES = 4096  # ... and its nFrames


def spatial_variance_device(w, h, moments_ptr, out_variance_ptr, normal_depth_ptr=None, frames=1, samples_per_frame=1.0,
                            min_samples=SPATIAL_VARIANCE_DEFAULTS["min_samples"], radius=SPATIAL_VARIANCE_DEFAULTS["radius"],
                            sigma_normal=SPATIAL_VARIANCE_DEFAULTS["sigma_normal"], sigma_depth=SPATIAL_VARIANCE_DEFAULTS["sigma_depth"]):
    """tptSpatialVarianceDevice: a variance plane {0, v/N, 0, N} for denoise_device_variance (as its moments_ptr, with samples =
    samples_per_frame) or for denoise_clip_device in spatial-only mode, from any moments plane of the chain: draw_device_moments' own,
    a clip draw's stack, or the out_moments of a temporal pass or of rectify_history_device (.w = N).  A pixel with
    samples_per_frame * N < min_samples takes its variance from the (2*radius + 1)^2 window's weighted moments, every other pixel its
    own (the temporal pass's variance bytes).  moments_ptr, out_variance_ptr, normal_depth_ptr: `frames` consecutive device planes of
    h*w*4 floats.  A guide's sigma is ignored (passed as 0) when normal_depth_ptr is not given.  min_samples may be float("inf"):
    every pixel is estimated.  Ordered on the context's stream."""
    _positive_ints(("w", w), ("h", h), ("frames", frames))
    if frames > SPATIAL_VARIANCE_MAX_FRAMES:
        raise ValueError("frames: at most %d, got %r" % (SPATIAL_VARIANCE_MAX_FRAMES, frames))
    _pointers(("moments_ptr", moments_ptr), ("out_variance_ptr", out_variance_ptr), ("normal_depth_ptr", normal_depth_ptr))
    if not moments_ptr or not out_variance_ptr:
        raise ValueError("moments_ptr, out_variance_ptr: device buffers are required")
    _sigmas(("samples_per_frame", samples_per_frame), ("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth))
    if not samples_per_frame >= 1:
        raise ValueError("samples_per_frame: a finite float >= 1 expected, got %r" % (samples_per_frame,))
    if not isinstance(min_samples, (int, float, np.integer, np.floating)) or isinstance(min_samples, bool) or not min_samples >= 1:
        raise ValueError("min_samples: a float >= 1 (or +inf) expected, got %r" % (min_samples,))
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool) or not 1 <= radius <= SPATIAL_VARIANCE_MAX_RADIUS:
        raise ValueError("radius: an int in 1..%d expected, got %r" % (SPATIAL_VARIANCE_MAX_RADIUS, radius))
    if not normal_depth_ptr:
        sigma_normal = sigma_depth = 0.0
    _chk(load_library().tptSpatialVarianceDevice(w, h, frames, C.c_void_p(moments_ptr), C.c_void_p(normal_depth_ptr or None),
                                                 C.c_void_p(out_variance_ptr), samples_per_frame, min_samples, int(radius), sigma_normal,
                                                 sigma_depth), "tptSpatialVarianceDevice")


TRACE_RAYS_MAX = 16777216  # include/tpt_hip.h: tptTraceRaysDevice's nRays


def trace_rays_device(n, rays_ptr, radiance_ptr=None, hits_ptr=None, ray_count_ptr=None):
    """tptTraceRaysDevice: what comes back along n caller-given rays and what each meets first.  rays_ptr: a device buffer of n x 8
    floats, {ox, oy, oz, seed bits} {dx, dy, dz, unused} per ray (the direction is used as given, not normalised).  radiance_ptr: None,
    or n x 4 floats for {colour, HitWorld calls of the path}; hits_ptr: None, or n x 8 floats for the first hit {pos, t} {normal,
    bits(id)} (id -1 and zeros for a miss); at least one of the two.  Without radiance_ptr the paths end at their first hit.
    ray_count_ptr: None, or a device u64 the call adds its HitWorld calls to.  The scene is the last UpdateTest's; light sampling, fold
    mode and the hitSpheres variant are the context's.  The context is left as it is.  Ordered on the context's stream."""
    if not isinstance(n, (int, np.integer)) or isinstance(n, bool) or not 1 <= n <= TRACE_RAYS_MAX:
        raise ValueError("n: an int in 1..%d expected, got %r" % (TRACE_RAYS_MAX, n))
    _pointers(("rays_ptr", rays_ptr), ("radiance_ptr", radiance_ptr), ("hits_ptr", hits_ptr), ("ray_count_ptr", ray_count_ptr))
    if not rays_ptr:
        raise ValueError("rays_ptr: a device buffer is required")
    if not radiance_ptr and not hits_ptr:
        raise ValueError("radiance_ptr, hits_ptr: at least one device buffer is required")
    a = TraceRaysArgs(nRays=int(n), flags=0, deviceRays=rays_ptr, deviceRadiance=radiance_ptr or None, deviceHits=hits_ptr or None,
                      deviceRayCount=ray_count_ptr or None)
    _chk(load_library().tptTraceRaysDevice(C.byref(a)), "tptTraceRaysDevice")


LENS_EQUIRECT, LENS_FISHEYE, LENS_ORTHO = 1, 2, 3  # include/tpt_hip.h: TPT_LENS_*
LENS_MAX_SIDE = 8192  # include/tpt_hip.h: tptDrawDeviceLens's screenWidth / screenHeight
_LENS_TWO_PI, _LENS_PI = float(np.float32(6.2831855)), float(np.float32(3.1415927))


def _lens_basis(origin, forward, up):
    """an orthonormal basis from a viewing direction and an up hint, made in float64 and rounded to binary32: (origin, right, up, forward)"""
    o, f, u = (np.asarray(v, np.float64).reshape(-1) for v in (origin, forward, up))
    if o.shape != (3,) or f.shape != (3,) or u.shape != (3,) or not (np.isfinite(o).all() and np.isfinite(f).all() and np.isfinite(u).all()):
        raise ValueError("origin, forward, up: three finite numbers each expected")
    if not np.linalg.norm(f) > 0:
        raise ValueError("forward: a direction of non-zero length expected")
    f = f / np.linalg.norm(f)
    r = np.cross(f, u)
    if not np.linalg.norm(r) > 1e-6 * max(np.linalg.norm(u), 1e-300):
        raise ValueError("up: must not be parallel to forward (or zero)")
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    return tuple(tuple(float(x) for x in v.astype(np.float32)) for v in (o, r, u, f))


def _lens(kind, origin, forward, up, sx, sy, max_angle):
    o, r, u, f = _lens_basis(origin, forward, up)
    lens = Lens(kind=kind, sx=sx, sy=sy, maxAngle=max_angle)
    lens.origin[:], lens.right[:], lens.up[:], lens.forward[:] = o, r, u, f
    _check_lens(lens)
    return lens


def lens_equirect(origin=(0.0, 1.0, 0.0), forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), lon_span=_LENS_TWO_PI, lat_span=_LENS_PI):
    """a tptLens for a panorama: longitude (about `up`, 0 at `forward`, growing towards the right) across the image's width, latitude
    across its height; the spans in radians, at most 2 pi by pi (the defaults: the whole sphere)"""
    return _lens(LENS_EQUIRECT, origin, forward, up, lon_span, lat_span, 0.0)


def lens_fisheye(origin=(0.0, 1.0, 0.0), forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), max_angle=_LENS_PI / 2, sx=2.0, sy=2.0):
    """a tptLens for an equidistant fisheye: the angle from `forward` grows linearly with the distance r from the image centre and is
    max_angle (radians, at most pi) at r = 1; sx, sy scale the image plane (2, 2 on a square image: the circle touches the edges; for a
    wide image 2 * w / h, 2)"""
    return _lens(LENS_FISHEYE, origin, forward, up, sx, sy, max_angle)


def lens_ortho(origin=(0.0, 1.0, 3.0), forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), width=4.0, height=4.0):
    """a tptLens for an orthographic view: parallel rays along `forward` from a window of width x height world units centred on origin"""
    return _lens(LENS_ORTHO, origin, forward, up, width, height, 0.0)


def _check_lens(lens):
    """include/tpt_hip.h's rules for a tptLens, before the library is reached: ValueError for the first one broken"""
    if not isinstance(lens, Lens):
        raise ValueError("lens: a Lens expected (lens_equirect, lens_fisheye, lens_ortho), got %r" % (lens,))
    if lens.kind not in (LENS_EQUIRECT, LENS_FISHEYE, LENS_ORTHO):
        raise ValueError("lens.kind: LENS_EQUIRECT, LENS_FISHEYE or LENS_ORTHO expected, got %r" % lens.kind)
    vecs = [np.array(v[:], np.float64) for v in (lens.origin, lens.right, lens.up, lens.forward)]
    scalars = (lens.sx, lens.sy, lens.maxAngle)
    if not all(np.isfinite(v).all() for v in vecs) or not np.isfinite(scalars).all():
        raise ValueError("lens: every field must be finite")
    for i in range(1, 4):
        if not 0.99 <= float(vecs[i] @ vecs[i]) <= 1.01:
            raise ValueError("lens: a basis vector is not of unit length")
        for k in range(i + 1, 4):
            if not -0.01 <= float(vecs[i] @ vecs[k]) <= 0.01:
                raise ValueError("lens: two basis vectors are not orthogonal")
    if not (lens.sx > 0 and lens.sy > 0):
        raise ValueError("lens.sx, lens.sy: positive numbers expected")
    if lens.kind == LENS_EQUIRECT and (lens.sx > _LENS_TWO_PI or lens.sy > _LENS_PI):
        raise ValueError("lens: an equirectangular span of at most 2 pi x pi expected")
    if lens.kind == LENS_FISHEYE and (lens.sx > 4 or lens.sy > 4 or not 0 < lens.maxAngle <= _LENS_PI):
        raise ValueError("lens: a fisheye scale of at most 4 and a maxAngle in (0, pi] expected")
    if lens.kind != LENS_FISHEYE and lens.maxAngle != 0:
        raise ValueError("lens.maxAngle: 0 expected for this kind")


def draw_device_lens(frame, w, h, tile_ptr, lens, flags=0, ray_count_ptr=None):
    """tptDrawDeviceLens: draw_device's contract through `lens` (lens_equirect, lens_fisheye, lens_ortho) instead of the camera.  All
    set_samples_per_pixel samples of a pixel are traced in one launch from the pixel's own random stream (per-pixel seeds) and blended
    into tile_ptr (a device buffer of h*w*4 floats, row 0 at the bottom): lerp = frame / (frame + 1) under FLAG_PROGRESSIVE (flags 2),
    else 0.  ray_count_ptr: None, or a device u64 the call adds its HitWorld calls to; the context's counter is not touched.  The
    scene is the last UpdateTest's; light sampling, fold mode and the hitSpheres variant are the context's.  Ordered on the context's
    stream."""
    for name, v in (("w", w), ("h", h)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 1 <= v <= LENS_MAX_SIDE:
            raise ValueError("%s: an int in 1..%d expected, got %r" % (name, LENS_MAX_SIDE, v))
    if not isinstance(frame, (int, np.integer)) or isinstance(frame, bool) or not 0 <= frame < 2 ** 31:
        raise ValueError("frame: an int >= 0 expected, got %r" % (frame,))
    if isinstance(flags, bool) or flags not in (0, FLAG_PROGRESSIVE):
        raise ValueError("flags: 0 or FLAG_PROGRESSIVE (2) expected, got %r" % (flags,))
    _pointers(("tile_ptr", tile_ptr), ("ray_count_ptr", ray_count_ptr))
    if not tile_ptr:
        raise ValueError("tile_ptr: a device buffer is required")
    if ray_count_ptr and tile_ptr - 8 < ray_count_ptr < tile_ptr + 16 * int(w) * int(h):
        raise ValueError("ray_count_ptr: lies inside the tile")
    _check_lens(lens)
    a = DrawLensArgs(screenWidth=int(w), screenHeight=int(h), frameCount=int(frame), flags=int(flags), lens=lens, deviceTile=tile_ptr,
                     deviceRayCount=ray_count_ptr or None)
    _chk(load_library().tptDrawDeviceLens(C.byref(a)), "tptDrawDeviceLens")


OBJECT_PLANE_MAX_FRAMES = 4096  # include/tpt_hip.h: tptObjectPlaneDevice's nFrames
OBJECT_MOTION_MAX_OBJECTS = 65534  # include/tpt_hip.h: tptTemporalAccumulateObjectsDevice's nObjects


def object_plane_device(w, h, objects_ptr, flags=0, times=None, cameras=None, frames=None):
    """tptObjectPlaneDevice: the index of the first sphere the ray through each pixel's centre meets (-1: none) into objects_ptr, a
    device buffer of N consecutive planes of h*w int32.  cameras: None (the camera of the last UpdateTest for every frame, whose size
    w x h must be) or a CAMERA_DT array of N records (draw_device_camera_clip's result, GetSceneDesc()[2]).  times: None or N floats;
    with kFlagAnimate spheres 1 and 8 of frame j stand where UpdateTest(times[j]) puts them.  N is len(cameras), len(times) or
    `frames` (default 1); what is given must agree.  The context is left as it is.  Ordered on the context's stream."""
    _positive_ints(("w", w), ("h", h))
    _pointers(("objects_ptr", objects_ptr))
    if not objects_ptr:
        raise ValueError("objects_ptr: a device buffer is required")
    if not isinstance(flags, (int, np.integer)) or isinstance(flags, bool) or flags & ~(kFlagAnimate | kFlagProgressive):
        raise ValueError("flags: kFlagAnimate | kFlagProgressive bits expected, got %r" % (flags,))
    counts = []
    t = c = None
    if times is not None:
        t = np.ascontiguousarray(times, dtype=np.float32)
        if t.ndim != 1:
            raise ValueError("times: a 1-D sequence expected, got shape %r" % (t.shape,))
        counts.append(t.shape[0])
    if cameras is not None:
        if not isinstance(cameras, np.ndarray) or cameras.dtype != CAMERA_DT or cameras.ndim != 1:
            raise ValueError("cameras: a 1-D CAMERA_DT array expected, got %r" % (cameras,))
        c = np.ascontiguousarray(cameras)
        counts.append(c.shape[0])
    if frames is not None:
        _positive_ints(("frames", frames))
        counts.append(frames)
    n = counts[0] if counts else 1
    if any(k != n for k in counts):
        raise ValueError("times, cameras, frames: one frame count expected, got %r" % (counts,))
    if not 1 <= n <= OBJECT_PLANE_MAX_FRAMES:
        raise ValueError("frames: 1..%d expected, got %d" % (OBJECT_PLANE_MAX_FRAMES, n))
    _chk(load_library().tptObjectPlaneDevice(n, t.ctypes.data if t is not None else None, c.ctypes.data if c is not None else None, w, h,
                                             C.c_void_p(objects_ptr), flags), "tptObjectPlaneDevice")


def object_motion_table(time, prev_time, flags):
    """tptObjectMotionTable: float32 (count, 4), entry i = {where sphere i stood at prev_time minus where it stands at time, 0} under
    UpdateTest's animation rule (kFlagAnimate: spheres 1 and 8; zero otherwise).  Set .w (the history caps) and upload it for
    temporal_accumulate_objects_device."""
    for name, v in (("time", time), ("prev_time", prev_time)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool):
            raise ValueError("%s: a number expected, got %r" % (name, v))
    if not isinstance(flags, (int, np.integer)) or isinstance(flags, bool) or flags < 0:
        raise ValueError("flags: an int >= 0 expected, got %r" % (flags,))
    n = GetObjectCount()[0]
    table = np.zeros((n, 4), np.float32)
    _chk(load_library().tptObjectMotionTable(time, prev_time, flags, table.ctypes.data, n), "tptObjectMotionTable")
    return table


def motion_table(prev_spheres, cur_spheres, caps=None):
    """The table of temporal_accumulate_objects_device for a caller who moves spheres with set_scene: two GetSceneDesc sphere arrays
    (SPHERE_DT, the same length) -> float32 (count, 4), .xyz = previous centre minus current centre (one float32 subtraction each),
    .w = caps (None: 0, no cap; a number, or one per sphere)."""
    for name, s in (("prev_spheres", prev_spheres), ("cur_spheres", cur_spheres)):
        if not isinstance(s, np.ndarray) or s.dtype != SPHERE_DT or s.ndim != 1:
            raise ValueError("%s: a 1-D SPHERE_DT array expected, got %r" % (name, s))
    if prev_spheres.shape != cur_spheres.shape:
        raise ValueError("prev_spheres, cur_spheres: the same length expected, got %d and %d" % (len(prev_spheres), len(cur_spheres)))
    table = np.zeros((len(cur_spheres), 4), np.float32)
    for k, field in enumerate(("cx", "cy", "cz")):
        table[:, k] = prev_spheres[field] - cur_spheres[field]
    if caps is not None:
        w = np.asarray(caps, dtype=np.float32)
        if w.ndim > 1 or (w.ndim == 1 and w.shape[0] != len(cur_spheres)) or not np.all(w >= 0):
            raise ValueError("caps: a number >= 0 or one per sphere expected, got %r" % (caps,))
        table[:, 3] = w
    return table


def temporal_accumulate_objects_device(w, h, camera, colour_ptr, albedo_ptr, normal_depth_ptr, moments_ptr, object_ptr, out_colour_ptr,
                                       out_albedo_ptr, out_moments_ptr, out_variance_ptr, prev=None, motion_ptr=None, n_objects=0,
                                       max_history=TEMPORAL_DEFAULTS["max_history"],
                                       depth_tolerance=TEMPORAL_DEFAULTS["depth_tolerance"],
                                       normal_tolerance=TEMPORAL_DEFAULTS["normal_tolerance"],
                                       coverage_tolerance=TEMPORAL_DEFAULTS["coverage_tolerance"]):
    """tptTemporalAccumulateObjectsDevice: temporal_accumulate_device that follows objects.  object_ptr: this frame's object plane
    (object_plane_device; h*w int32).  prev: None for the first frame, else (camera, colour_ptr, albedo_ptr, normal_depth_ptr,
    moments_ptr, object_ptr) of the previous frame.  motion_ptr: None (nothing moves, nothing is capped; n_objects 0) or a device buffer
    of n_objects x 4 floats (object_motion_table / motion_table, uploaded): .xyz where the object's points stood in the previous frame
    minus where they stand now, .w its history cap (0: none).  A tap counts only where the previous object plane holds the pixel's id.
    Ordered on the context's stream."""
    _positive_ints(("w", w), ("h", h))
    cur = (("colour_ptr", colour_ptr), ("albedo_ptr", albedo_ptr), ("normal_depth_ptr", normal_depth_ptr), ("moments_ptr", moments_ptr),
           ("object_ptr", object_ptr), ("out_colour_ptr", out_colour_ptr), ("out_albedo_ptr", out_albedo_ptr),
           ("out_moments_ptr", out_moments_ptr), ("out_variance_ptr", out_variance_ptr))
    _pointers(*cur)
    if not all(v for _, v in cur):
        raise ValueError("%s: device buffers are required" % ", ".join(n for n, v in cur if not v))
    cam = _camera_bytes("camera", camera)
    prev_cam, prev_ptrs = None, (None,) * 5
    if prev is not None:
        if not isinstance(prev, (tuple, list)) or len(prev) != 6:
            raise ValueError("prev: None or (camera, colour_ptr, albedo_ptr, normal_depth_ptr, moments_ptr, object_ptr) expected, got %r"
                             % (prev,))
        prev_cam = _camera_bytes("prev camera", prev[0])
        named = tuple(zip(("prev colour_ptr", "prev albedo_ptr", "prev normal_depth_ptr", "prev moments_ptr", "prev object_ptr"), prev[1:]))
        _pointers(*named)
        if not all(v for _, v in named):
            raise ValueError("prev: all five device buffers are required")
        prev_ptrs = tuple(C.c_void_p(v) for v in prev[1:])
    _pointers(("motion_ptr", motion_ptr))
    if not isinstance(n_objects, (int, np.integer)) or isinstance(n_objects, bool) or not 0 <= n_objects <= OBJECT_MOTION_MAX_OBJECTS:
        raise ValueError("n_objects: an int in 0..%d expected, got %r" % (OBJECT_MOTION_MAX_OBJECTS, n_objects))
    if bool(motion_ptr) != (n_objects > 0):
        raise ValueError("motion_ptr, n_objects: both or neither expected, got %r and %r" % (motion_ptr, n_objects))
    if not isinstance(max_history, (int, float, np.integer, np.floating)) or isinstance(max_history, bool) or not 1 <= max_history <= 65536:
        raise ValueError("max_history: a number in 1..65536 expected, got %r" % (max_history,))
    _sigmas(("depth_tolerance", depth_tolerance), ("normal_tolerance", normal_tolerance), ("coverage_tolerance", coverage_tolerance))
    _chk(load_library().tptTemporalAccumulateObjectsDevice(
        w, h, cam, prev_cam, C.c_void_p(colour_ptr), C.c_void_p(albedo_ptr), C.c_void_p(normal_depth_ptr), C.c_void_p(moments_ptr),
        *prev_ptrs[:4], C.c_void_p(out_colour_ptr), C.c_void_p(out_albedo_ptr), C.c_void_p(out_moments_ptr), C.c_void_p(out_variance_ptr),
        max_history, depth_tolerance, normal_tolerance, coverage_tolerance, C.c_void_p(object_ptr), prev_ptrs[4],
        C.c_void_p(motion_ptr) if motion_ptr else None, n_objects), "tptTemporalAccumulateObjectsDevice")


CLIP_DENOISE_SPATIAL_ONLY = 1  # include/tpt_hip.h: TPT_CLIP_DENOISE_SPATIAL_ONLY
CLIP_DENOISE_MAX_FRAMES = 4096  # include/tpt_hip.h: tptDenoiseClipDevice's nFrames


def denoise_clip_device(w, h, frames, images_ptr, moments_ptr, out_ptr, samples, albedo_ptr=None, normal_depth_ptr=None, cameras=None,
                        objects_ptr=None, motion_ptr=None, n_objects=0, prev=None, history_ptr=None, spatial_only=False,
                        iterations=DENOISE_VARIANCE_DEFAULTS["iterations"], sigma_luminance=DENOISE_VARIANCE_DEFAULTS["sigma_luminance"],
                        sigma_normal=DENOISE_VARIANCE_DEFAULTS["sigma_normal"], sigma_depth=DENOISE_VARIANCE_DEFAULTS["sigma_depth"],
                        demodulate=None, max_history=TEMPORAL_DEFAULTS["max_history"],
                        depth_tolerance=TEMPORAL_DEFAULTS["depth_tolerance"], normal_tolerance=TEMPORAL_DEFAULTS["normal_tolerance"],
                        coverage_tolerance=TEMPORAL_DEFAULTS["coverage_tolerance"]):
    """tptDenoiseClipDevice: `frames` frames of a clip draw (draw_device_animation_moments, draw_device_camera_clip,
    draw_device_keyframe_clip, each without kFlagProgressive) through temporal_accumulate_[objects_]device and denoise_device_variance,
    the filter's iterations one launch per chunk of up to 32 frames.  images_ptr, moments_ptr, albedo_ptr, normal_depth_ptr, out_ptr:
    `frames` consecutive device planes of h*w*4 floats each (the clip draw's images_ptr, frame_moments_ptr, albedo_ptr and
    normal_depth_ptr; out_ptr receives the denoised frames).  cameras: the clip draw's result, a CAMERA_DT array of `frames` records.
    objects_ptr: None, or the clip's object planes (h*w int32 each): the temporal pass then follows objects, with motion_ptr / n_objects
    None / 0 or `frames` tables of n_objects x 4 floats in device memory, table j between frames j-1 and j.  prev: None (frame 0 starts
    a sequence) or (camera, normal_depth_ptr) -- with objects_ptr (camera, normal_depth_ptr, object_ptr) -- of the frame before frame 0,
    whose temporal outputs history_ptr holds.  history_ptr: None or 3 device planes {colour, albedo, moments}, read when prev is given
    and overwritten with the last frame's temporal outputs: pass it call after call.  spatial_only=True: no temporal pass, every frame
    filtered on its own (albedo_ptr / normal_depth_ptr optional; cameras ignored; objects, prev and history not allowed).  The filter's
    arguments are denoise_device_variance's, the temporal ones temporal_accumulate_device's.  Ordered on the context's stream."""
    _positive_ints(("w", w), ("h", h), ("frames", frames), ("iterations", iterations))
    if frames > CLIP_DENOISE_MAX_FRAMES:
        raise ValueError("frames: 1..%d expected, got %d" % (CLIP_DENOISE_MAX_FRAMES, frames))
    named = (("images_ptr", images_ptr), ("moments_ptr", moments_ptr), ("out_ptr", out_ptr), ("albedo_ptr", albedo_ptr),
             ("normal_depth_ptr", normal_depth_ptr), ("objects_ptr", objects_ptr), ("motion_ptr", motion_ptr), ("history_ptr", history_ptr))
    _pointers(*named)
    if not images_ptr or not moments_ptr or not out_ptr:
        raise ValueError("images_ptr, moments_ptr, out_ptr: device buffers are required")
    prev_cam, prev_ptrs = None, (None, None)
    if spatial_only:
        if objects_ptr or motion_ptr or n_objects or prev is not None or history_ptr:
            raise ValueError("spatial_only: objects_ptr, motion_ptr, n_objects, prev and history_ptr are not allowed")
    else:
        if not albedo_ptr or not normal_depth_ptr:
            raise ValueError("albedo_ptr, normal_depth_ptr: device buffers are required unless spatial_only")
        if not isinstance(cameras, np.ndarray) or cameras.dtype != CAMERA_DT or cameras.shape != (frames,):
            raise ValueError("cameras: a CAMERA_DT array of %d records expected, got %r" % (frames, cameras))
        cameras = np.ascontiguousarray(cameras)
        if prev is not None:
            if not isinstance(prev, (tuple, list)) or len(prev) != (3 if objects_ptr else 2):
                raise ValueError("prev: None or (camera, normal_depth_ptr%s) expected, got %r" % (", object_ptr" if objects_ptr else "", prev))
            prev_cam = _camera_bytes("prev camera", prev[0])
            more = tuple(zip(("prev normal_depth_ptr", "prev object_ptr"), prev[1:]))
            _pointers(*more)
            if not all(v for _, v in more):
                raise ValueError("prev: every device buffer is required")
            if not history_ptr:
                raise ValueError("history_ptr: required with prev")
            prev_ptrs = tuple(prev[1:]) + (None,) * (3 - len(prev))
    if not isinstance(n_objects, (int, np.integer)) or isinstance(n_objects, bool) or not 0 <= n_objects <= OBJECT_MOTION_MAX_OBJECTS:
        raise ValueError("n_objects: an int in 0..%d expected, got %r" % (OBJECT_MOTION_MAX_OBJECTS, n_objects))
    if bool(motion_ptr) != (n_objects > 0):
        raise ValueError("motion_ptr, n_objects: both or neither expected, got %r and %r" % (motion_ptr, n_objects))
    if motion_ptr and not objects_ptr:
        raise ValueError("motion_ptr: needs objects_ptr")
    if not isinstance(samples, (int, float, np.integer, np.floating)) or isinstance(samples, bool) or not 1 <= samples < float("inf"):
        raise ValueError("samples: a finite number >= 1 expected, got %r" % (samples,))
    if not isinstance(sigma_luminance, (int, float, np.integer, np.floating)) or isinstance(sigma_luminance, bool) or not 0 < sigma_luminance <= 1e6:
        raise ValueError("sigma_luminance: a float in (0, 1e6] expected, got %r" % (sigma_luminance,))
    _sigmas(("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth))
    if demodulate is None:
        demodulate = bool(albedo_ptr)
    if demodulate and not albedo_ptr:
        raise ValueError("demodulate: needs albedo_ptr")
    if not normal_depth_ptr:
        sigma_normal = sigma_depth = 0.0
    if not isinstance(max_history, (int, float, np.integer, np.floating)) or isinstance(max_history, bool) or not 1 <= max_history <= 65536:
        raise ValueError("max_history: a number in 1..65536 expected, got %r" % (max_history,))
    _sigmas(("depth_tolerance", depth_tolerance), ("normal_tolerance", normal_tolerance), ("coverage_tolerance", coverage_tolerance))
    a = ClipDenoiseArgs(
        screenWidth=w, screenHeight=h, nFrames=frames, clipFlags=CLIP_DENOISE_SPATIAL_ONLY if spatial_only else 0,
        deviceFrameImages=images_ptr, deviceFrameMoments=moments_ptr, deviceFrameAlbedo=albedo_ptr or None,
        deviceFrameNormalDepth=normal_depth_ptr or None, cameras=None if spatial_only else cameras.ctypes.data,
        deviceFrameObjects=objects_ptr or None, deviceFrameObjectMotion=motion_ptr or None, deviceFrameOut=out_ptr,
        prevCamera=C.addressof(prev_cam) if prev_cam is not None else None, devicePrevNormalDepth=prev_ptrs[0],
        devicePrevObject=prev_ptrs[1], deviceHistory=history_ptr or None, nObjects=n_objects, iterations=iterations,
        denoiseFlags=DENOISE_DEMODULATE if demodulate else 0, samples=samples, sigmaLuminance=sigma_luminance, sigmaNormal=sigma_normal,
        sigmaDepth=sigma_depth, maxHistory=max_history, depthTolerance=depth_tolerance, normalTolerance=normal_tolerance,
        coverageTolerance=coverage_tolerance)
    _chk(load_library().tptDenoiseClipDevice(C.byref(a)), "tptDenoiseClipDevice")  # (cameras and prev_cam live until here)


def motion_vectors_device(w, h, frames, albedo_ptr, normal_depth_ptr, motion_out_ptr, cameras, objects_ptr=None, motion_ptr=None,
                          n_objects=0, prev=None, depth_tolerance=TEMPORAL_DEFAULTS["depth_tolerance"],
                          normal_tolerance=TEMPORAL_DEFAULTS["normal_tolerance"],
                          coverage_tolerance=TEMPORAL_DEFAULTS["coverage_tolerance"]):
    """tptMotionVectorsDevice: per pixel of `frames` frames of a clip draw, {mv.x, mv.y, e, W} into motion_out_ptr (`frames` device
    planes of h*w*4 floats): mv where, in pixels, the pixel's surface point stood in the previous frame relative to this pixel, e its
    distance from the previous camera, W in [0, 1] how much of the bilinear footprint there shows the same surface (0: disoccluded,
    outside the image, another surface; all four 0 where the point does not project).  albedo_ptr, normal_depth_ptr: the clip draw's
    planes, `frames` of h*w*4 floats each.  cameras: the clip draw's result, a CAMERA_DT array of `frames` records.  objects_ptr: None,
    or the clip's object planes (h*w int32 each): points then move with their object, by motion_ptr / n_objects -- None / 0, or
    `frames` tables of n_objects x 4 floats in device memory, table j between frames j-1 and j -- and a tap counts only on the same
    object.  prev: None (frame 0 has no predecessor: its plane is zeroed) or (camera, albedo_ptr, normal_depth_ptr) -- with
    objects_ptr (camera, albedo_ptr, normal_depth_ptr, object_ptr) -- of the frame before frame 0.  The tolerances are
    temporal_accumulate_device's.  Ordered on the context's stream."""
    _positive_ints(("w", w), ("h", h), ("frames", frames))
    if frames > CLIP_DENOISE_MAX_FRAMES:
        raise ValueError("frames: 1..%d expected, got %d" % (CLIP_DENOISE_MAX_FRAMES, frames))
    named = (("albedo_ptr", albedo_ptr), ("normal_depth_ptr", normal_depth_ptr), ("motion_out_ptr", motion_out_ptr),
             ("objects_ptr", objects_ptr), ("motion_ptr", motion_ptr))
    _pointers(*named)
    if not albedo_ptr or not normal_depth_ptr or not motion_out_ptr:
        raise ValueError("albedo_ptr, normal_depth_ptr, motion_out_ptr: device buffers are required")
    if not isinstance(cameras, np.ndarray) or cameras.dtype != CAMERA_DT or cameras.shape != (frames,):
        raise ValueError("cameras: a CAMERA_DT array of %d records expected, got %r" % (frames, cameras))
    cameras = np.ascontiguousarray(cameras)
    prev_cam, prev_ptrs = None, (None, None, None)
    if prev is not None:
        if not isinstance(prev, (tuple, list)) or len(prev) != (4 if objects_ptr else 3):
            raise ValueError("prev: None or (camera, albedo_ptr, normal_depth_ptr%s) expected, got %r"
                             % (", object_ptr" if objects_ptr else "", prev))
        prev_cam = _camera_bytes("prev camera", prev[0])
        more = tuple(zip(("prev albedo_ptr", "prev normal_depth_ptr", "prev object_ptr"), prev[1:]))
        _pointers(*more)
        if not all(v for _, v in more):
            raise ValueError("prev: every device buffer is required")
        prev_ptrs = tuple(prev[1:]) + (None,) * (4 - len(prev))
    if not isinstance(n_objects, (int, np.integer)) or isinstance(n_objects, bool) or not 0 <= n_objects <= OBJECT_MOTION_MAX_OBJECTS:
        raise ValueError("n_objects: an int in 0..%d expected, got %r" % (OBJECT_MOTION_MAX_OBJECTS, n_objects))
    if bool(motion_ptr) != (n_objects > 0):
        raise ValueError("motion_ptr, n_objects: both or neither expected, got %r and %r" % (motion_ptr, n_objects))
    if motion_ptr and not objects_ptr:
        raise ValueError("motion_ptr: needs objects_ptr")
    _sigmas(("depth_tolerance", depth_tolerance), ("normal_tolerance", normal_tolerance), ("coverage_tolerance", coverage_tolerance))
    a = MotionVectorsArgs(
        screenWidth=w, screenHeight=h, nFrames=frames, flags=0, cameras=cameras.ctypes.data, deviceFrameAlbedo=albedo_ptr,
        deviceFrameNormalDepth=normal_depth_ptr, deviceFrameObjects=objects_ptr or None, deviceFrameObjectMotion=motion_ptr or None,
        deviceFrameMotion=motion_out_ptr, prevCamera=C.addressof(prev_cam) if prev_cam is not None else None,
        devicePrevAlbedo=prev_ptrs[0], devicePrevNormalDepth=prev_ptrs[1], devicePrevObject=prev_ptrs[2], nObjects=n_objects,
        depthTolerance=depth_tolerance, normalTolerance=normal_tolerance, coverageTolerance=coverage_tolerance)
    _chk(load_library().tptMotionVectorsDevice(C.byref(a)), "tptMotionVectorsDevice")  # (cameras and prev_cam live until here)


ADAPTIVE_MAX_SAMPLES = 2047  # one pixel's samples of one launch (include/tpt_hip.h: 11 bits of sample index in the path record)


def draw_device_adaptive(time, frame, w, h, tile_ptr, moments_ptr, counts_ptr, flags, albedo_ptr=None, normal_depth_ptr=None):
    """tptDrawDeviceAdaptive: draw_device_moments with a sample count per pixel.  counts_ptr: a device buffer of h*w int32, row-major like
    the tile, each clamped to 0..2047 by the kernel; a pixel with 0 is not traced and nothing of it is written.  The blend is weighted by
    samples: moments_ptr's .w carries each pixel's running sample count (include/tpt_hip.h).  Ordered on the context's stream."""
    _positive_ints(("w", w), ("h", h))
    _pointers(("tile_ptr", tile_ptr), ("moments_ptr", moments_ptr), ("counts_ptr", counts_ptr), ("albedo_ptr", albedo_ptr),
              ("normal_depth_ptr", normal_depth_ptr))
    if not tile_ptr or not moments_ptr or not counts_ptr:
        raise ValueError("tile_ptr, moments_ptr, counts_ptr: device buffers are required")
    _chk(load_library().tptDrawDeviceAdaptive(time, frame, w, h, C.c_void_p(tile_ptr), C.c_void_p(albedo_ptr) if albedo_ptr else None,
                                              C.c_void_p(normal_depth_ptr) if normal_depth_ptr else None, C.c_void_p(moments_ptr),
                                              C.c_void_p(counts_ptr), flags), "tptDrawDeviceAdaptive")


def adaptive_samples_device(w, h, moments_ptr, target_error, counts_ptr, min_samples=0, max_samples=64, out_variance_ptr=None,
                            total_ptr=None):
    """tptAdaptiveSamplesDevice: draw_device_adaptive's moments (moments_ptr, .w the samples so far) -> the next pass's count per pixel
    in counts_ptr (h*w int32), in min_samples..max_samples, for a relative standard error of target_error of the mean luminance.
    out_variance_ptr: None or h*w*4 floats, the plane for denoise_device_variance's moments_ptr with samples = 1.  total_ptr: None or one
    int64 in device memory, overwritten with the sum of the counts.  A launch lasts at least as long as max_samples samples of one pixel
    take.  Ordered on the context's stream."""
    _positive_ints(("w", w), ("h", h))
    _pointers(("moments_ptr", moments_ptr), ("counts_ptr", counts_ptr), ("out_variance_ptr", out_variance_ptr), ("total_ptr", total_ptr))
    if not moments_ptr or not counts_ptr:
        raise ValueError("moments_ptr, counts_ptr: device buffers are required")
    if not isinstance(target_error, (int, float, np.integer, np.floating)) or isinstance(target_error, bool) or not 0 < target_error <= 1e6:
        raise ValueError("target_error: a float in (0, 1e6] expected, got %r" % (target_error,))
    for name, v in (("min_samples", min_samples), ("max_samples", max_samples)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= v <= ADAPTIVE_MAX_SAMPLES:
            raise ValueError("%s: an int in 0..%d expected, got %r" % (name, ADAPTIVE_MAX_SAMPLES, v))
    if min_samples > max_samples:
        raise ValueError("min_samples: at most max_samples (%d) expected, got %d" % (max_samples, min_samples))
    _chk(load_library().tptAdaptiveSamplesDevice(w, h, C.c_void_p(moments_ptr), target_error, min_samples, max_samples,
                                                 C.c_void_p(counts_ptr), C.c_void_p(out_variance_ptr) if out_variance_ptr else None,
                                                 C.c_void_p(total_ptr) if total_ptr else None), "tptAdaptiveSamplesDevice")


def sharded_finish():
    v = C.c_int64()
    _chk(load_library().tptShardedFinish(C.byref(v)), "tptShardedFinish")
    return v.value


def set_host_buffer_mode(only_written_by_drawtest):
    _chk(load_library().tptSetHostBufferMode(1 if only_written_by_drawtest else 0), "tptSetHostBufferMode")


def set_host_lookahead(frames):
    _chk(load_library().tptSetHostLookahead(frames), "tptSetHostLookahead")


def set_stream_batching(enable):
    _chk(load_library().tptSetStreamBatching(1 if enable else 0), "tptSetStreamBatching")


def lookahead_hits():
    v = C.c_longlong()
    _chk(load_library().tptGetLookaheadHits(C.byref(v)), "tptGetLookaheadHits")
    return v.value


def pipeline_info():
    v = [C.c_int() for _ in range(4)]
    _chk(load_library().tptGetPipelineInfo(*[C.byref(x) for x in v]), "tptGetPipelineInfo")
    return dict(hw_queues=v[0].value, overlap_effective=v[1].value, stream_depth=v[2].value, slot_reservations=v[3].value)


def scene_info():
    """what the next launch does with the scene: spheres, groups (0: flat), groups' bounds on the matrix cores (False: packed VALU filter)"""
    v = [C.c_int() for _ in range(3)]
    _chk(load_library().tptGetSceneInfo(*[C.byref(x) for x in v]), "tptGetSceneInfo")
    return dict(spheres=v[0].value, groups=v[1].value, bounds_on_matrix_cores=bool(v[2].value))


def debug_stats(reset=True):
    """profiling build only (TPT_LIB=... built with -DTPT_STATS)"""
    out = np.zeros(128, np.uint64)
    _chk(_hook("tptDebugStats")(out.ctypes.data, 1 if reset else 0), "tptDebugStats")
    return out


def debug_chunk_order(capacity=1 << 20):
    cost = np.zeros(capacity, np.uint32)
    order = np.zeros(capacity, np.uint32)
    n = _hook("tptDebugChunkOrder")(cost.ctypes.data, order.ctypes.data, capacity)
    if n < 0:
        raise TptError("tptDebugChunkOrder: " + _lib.tptGetLastError().decode())
    return cost[:n].copy(), order[:n].copy()


def device_name():
    return load_library().tptGetDeviceName().decode()


def test_math(op, a, b=None):
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty_like(a)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, np.float32)
        bp = b.ctypes.data
    _chk(_hook("tptTestMath")(op, a.ctypes.data, bp, out.ctypes.data, a.size), "tptTestMath")
    return out


def test_math_exhaustive(op, lo=0, hi=0xFFFFFFFF):
    """fast correctly-rounded sqrt (op 0) / 1/sqrt-then-reciprocal (op 1) vs the compiler's expansions for every bit
    pattern in [lo, hi], on the device -> (mismatches, first offending inputs)"""
    bad = C.c_ulonglong(0)
    first = (C.c_uint * 8)()
    _chk(_hook("tptTestMathExhaustive")(op, lo, hi, C.byref(bad), first), "tptTestMathExhaustive")
    return int(bad.value), [int(v) for v in first][: min(8, int(bad.value))]


def test_hit_spheres(rays, hit_spheres=0):
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    ids = np.empty(n, np.int32)
    ts = np.empty(n, np.float32)
    _chk(_hook("tptTestHitSpheres")(hit_spheres, rays.ctypes.data, ids.ctypes.data, ts.ctypes.data, n),
         "tptTestHitSpheres")
    return ids, ts


def test_matrix_filter(rays, hits=False):
    """phase 1 of HitSpheres on the matrix cores for the current scene (<= 64 spheres): candidate masks (sphere p at bit
    63 - p); hits=True: (masks, ids, ts) with the nearest hit through the filter + the exact test of its candidates"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    masks = np.empty(n, np.uint64)
    ids = np.empty(n, np.int32) if hits else None
    ts = np.empty(n, np.float32) if hits else None
    _chk(_hook("tptTestMatrixFilter")(rays.ctypes.data, masks.ctypes.data, ids.ctypes.data if hits else None,
                                            ts.ctypes.data if hits else None, n), "tptTestMatrixFilter")
    return (masks, ids, ts) if hits else masks


def test_set_deal_capacities(super_group_entries=0, group_entries=0, survivor_entries=0):
    """hooks build: run-time sizes of the three entry areas of the grouped traversal (0, 0, 0: the compiled ones)"""
    _chk(_hook("tptTestSetDealCapacities")(super_group_entries, group_entries, survivor_entries), "tptTestSetDealCapacities")


def test_group_filter(rays):
    """the matrix-core filter over the group bounds of the current grouped scene vs the reference's discriminant of every member:
    (violations, groups kept per ray, members with a positive discriminant per ray)"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    v = [C.c_ulonglong(0) for _ in range(3)]
    _chk(_hook("tptTestGroupFilter")(rays.ctypes.data, n, C.byref(v[0]), C.byref(v[1]), C.byref(v[2])), "tptTestGroupFilter")
    return int(v[0].value), v[1].value / n, v[2].value / n


def test_preset_stream_cut(keep):
    """hooks build: the next stream-batch launch with a pool per frame starts cut to its first `keep` frames (0: no preset)"""
    _chk(_hook("tptTestPresetStreamCut")(int(keep)), "tptTestPresetStreamCut")


def test_stream_frame_rays():
    """hooks build: the per-frame ray counters of the newest stream-batch launch (drains the pipeline first)"""
    out = np.zeros(8, np.uint64)
    n = _hook("tptTestStreamFrameRays")(out.ctypes.data, 8)
    if n < 0:
        raise TptError(f"tptTestStreamFrameRays: {_lib.tptGetLastError().decode()}")
    return [int(v) for v in out[:n]]
