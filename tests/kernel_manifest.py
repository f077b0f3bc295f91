"""The kernels of the shipped library's gfx950 code object, stated once (a plain module: neither a conftest nor a test).

Every family is a mangled-name template and the parameter tuples it is instantiated with.  tests/test_isa_contract.py holds the code
object to exactly ALL; the ABI and ISA tests of a feature look its kernels up by the templates.  A new kernel enters the suite through its
line here, and a kernel's name is just its name: no test decides anything by the words in it beyond its own family's.  (The unit-test
kernels of the hooks build are not listed: they are no part of the product.)"""
from itertools import product

FAMILIES = {}  # template -> the parameter tuples of its instantiations


def _family(template, *ranges):
    FAMILIES[template] = tuple(product(*ranges))
    return template


def family(template):
    """the mangled names of a family's instantiations"""
    return [template % p for p in FAMILIES[template]]


B = (0, 1)  # a bool template parameter
R = (1, 2, 3)  # a window radius

# ---- the trace kernels: the path-queue kernel, its variants (one KernelArgs each), and the lane-refill fallback
QUEUE = _family("_ZN3tpt19tptTraceQueueKernelILb%dELb%dEEEvNS_10KernelArgsE", B, B)  # <LDS_SCENE, BATCH>
VIEWS = _family("_ZN3tpt19tptTraceViewsKernelILb%dEEEvNS_10KernelArgsE", B)  # <LDS_SCENE>
ANIM = _family("_ZN3tpt23tptTraceAnimationKernelILb%dEEEvNS_10KernelArgsE", B)  # <LDS_SCENE>
AOV = _family("_ZN3tpt17tptTraceAovKernelILb%dEEEvNS_10KernelArgsE", B)  # <LDS_SCENE>
MOMENTS = _family("_ZN3tpt21tptTraceMomentsKernelILb%dEEEvNS_10KernelArgsE", B)  # <LDS_SCENE>
CLIP = _family("_ZN3tpt18tptTraceClipKernelILb%dEEEvNS_10KernelArgsE", B)  # <LDS_SCENE>
ADAPTIVE = _family("_ZN3tpt22tptTraceAdaptiveKernelILb%dEEEvNS_10KernelArgsE", B)  # <LDS_SCENE>
CAMERA_CLIP = _family("_ZN3tpt19tptCameraClipKernelILb%dEEEvNS_10KernelArgsE", B)  # <LDS_SCENE>
KEYFRAME = _family("_ZN3tpt17tptKeyframeKernelILb%dEEEvNS_10KernelArgsE", B)  # <LDS_SCENE>
POOLS = _family("_ZN3tpt19tptFramePoolsKernelILb%dEEEvNS_10KernelArgsE", B)  # <LDS_SCENE>
TRACE = _family("_ZN3tpt14tptTraceKernelILi%dELi%dELb%dEEEvNS_10KernelArgsE", B, B, B)  # <HS, PERSIST, LDS_SCENE>
# ---- what the trace launches run beside them
RESOLVE = _family("_ZN3tpt16tptResolveKernelEPfPKNS_2f4EifPKyPy")
RESOLVE_MIRROR = _family("_ZN3tpt22tptResolveMirrorKernelEPfPKNS_2f4EifPS1_PyS5_PKy")
RESOLVE_BATCH = _family("_ZN3tpt21tptResolveBatchKernelEPfPKNS_2f4Eiii12tptLerpTablePS1_PKyPy")
ASSEMBLE = _family("_ZN3tpt17tptAssembleKernelEPKNS_2f4EPS0_iiiii")
DISPLAY = _family("_ZN3tpt16tptDisplayKernelEPKNS_2f4EPjii")
CHUNK_ORDER = _family("_ZN3tpt19tptChunkOrderKernelEPKjPjS2_i")
QUEUE_PROBE = _family("_ZN3tpt19tptQueueProbeKernelEyPj")
FOLD = _family("_ZN3tpt18tptFoldBatchKernelEPNS_2f4ES1_S1_S1_PKS0_S3_S3_S3_ii12tptLerpTablePKyiPy")
ADAPTIVE_RESOLVE = _family("_ZN3tpt24tptAdaptiveResolveKernelEPfS0_PKNS_2f4ES3_PKiii")
ADAPTIVE_PLAN = _family("_ZN3tpt21tptAdaptivePlanKernelEPKNS_2f4EPiPS0_Pyiifii")
# ---- the post-process kernels
DENOISE = _family("_ZN3tpt16tptDenoiseKernelILb%dELb%dELb%dEEEvPKNS_2f4ES3_S3_PS1_iiifffi", B, B, B)  # <FIRST, LAST, GUIDE>
VARIANCE = _family("_ZN3tpt23tptVarianceAtrousKernelILb%dELb%dELb%dEEEvPKNS_2f4ES3_S3_S3_S3_PS1_iiiffffi", B, B, B)  # <FIRST, LAST, GUIDE>
FRAMES = _family("_ZN3tpt21tptFramesAtrousKernelILb%dELb%dELb%dEEEvPKNS_2f4ES3_S3_S3_S3_PS1_iiiffffi", B, B, B)  # <FIRST, LAST, GUIDE>
TEMPORAL = _family("_ZN3tpt17tptTemporalKernelILb%dEEEvPKNS_2f4ES3_S3_S3_S3_S3_S3_S3_PS1_S4_S4_S4_ii17tptTemporalConsts", B)  # <HISTORY>
REPROJECT = _family("_ZN3tpt25tptReprojectObjectsKernelILb%dEEEvPKNS_2f4ES3_S3_S3_S3_S3_S3_S3_PS1_S4_S4_S4_PKiS6_S3_iii18tptReprojectConsts",
                    B)  # <HISTORY>
OBJECT_PLANE = _family("_ZN3tpt20tptObjectPlaneKernelEPKNS_2f4EiPiii20tptObjectPlaneConsts")
FLOW = _family("_ZN3tpt13tptFlowKernelILb%dEEEvPKNS_2f4ES3_PKiS3_S3_S5_S3_iPS1_iiPK13tptFlowConsts", B)  # <OBJECTS>
RECTIFY = _family("_ZN3tpt16tptRectifyKernelILi%dEEEvPKNS_2f4ES3_S3_S3_PS1_S4_S4_iif", R)  # <R>
SPREAD = _family("_ZN3tpt15tptSpreadKernelILi%dELi%dEEEvPKNS_2f4ES3_PS1_iiffff", R, B)  # <R, GUIDE>

ALL = frozenset(n for t in FAMILIES for n in family(t))
