/* tpt_hip.h -- C ABI of the MI355X (gfx950, HIP) implementation of ToyPathTracer's
 * Trace / HitWorld / Scatter hot path.
 *
 * Drop-in boundary: the first block mirrors, one to one, the reference's "Test API"
 * (/root/reference/Cpp/Source/Test.h:10-17) that every reference host links against
 * (Cpp/Windows/TestWin.cpp:76,258,265,315-316; Cpp/Apple/Renderer.mm:155,181,225,234;
 * Cpp/Emscripten/main.cpp:59-60).  The shared library ALSO exports those six functions with the
 * reference's C++ linkage and exact signatures (see tpt_test_api.h), so a host compiled against the
 * reference's own Test.h links against libtoypathtracer_hip.so instead of Test.cpp+Maths.cpp+enkiTS
 * without source changes.  Precedent for an extern "C" veneer over this API in the reference:
 * Cpp/Emscripten/main.cpp:46-61.
 *
 * Everything is plain C: pointers, ints, floats.  No HIP / torch types appear in any signature
 * (streams and device buffers travel as void* / float*).  All functions return 0 on success and a
 * negative code on failure (tptGetLastError() has the text); nothing throws across the boundary.
 * The reference API itself has no error channel (all void): the C++-linkage wrappers print the error
 * to stderr and abort() -- there is NO CPU fallback.
 *
 * Not thread-safe / not re-entrant, like the reference (global scheduler + global scene,
 * Test.cpp:13,34,46,66-69,237).  One context per process == one GPU per process.
 */
#ifndef TPT_HIP_H
#define TPT_HIP_H
#include <stdint.h>

/* The library is built with -fvisibility=hidden: exactly the functions declared here (and the six C++ symbols of
 * tpt_test_api.h) are exported, nothing else (tests/test_abi.py compares `nm -D` with these headers). */
#if defined(__GNUC__)
#define TPT_API __attribute__((visibility("default")))
#else
#define TPT_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- TestFlags, Test.h:4-8 */
enum { TPT_FLAG_ANIMATE = 1 << 0, TPT_FLAG_PROGRESSIVE = 1 << 1 };

/* ================= 1. the reference Test API (Test.h:10-17), C spelling ================= */

/* InitializeTest(), Test.h:10 / Test.cpp:240-246.  Picks the HIP device (env TPT_DEVICE, else
 * LOCAL_RANK, else 0), creates the stream, uploads the built-in 46-sphere scene. */
TPT_API int tptInitialize(void);
/* ShutdownTest(), Test.h:11 / Test.cpp:248-253. */
TPT_API int tptShutdown(void);
/* UpdateTest(time, frameCount, screenWidth, screenHeight, testFlags), Test.h:13 / Test.cpp:302-342:
 * animate spheres 1 and 8 if TPT_FLAG_ANIMATE, derive 1/r and r^2, emissive list, camera;
 * uploads the scene arrays when they changed. */
TPT_API int tptUpdate(float time, int frameCount, int screenWidth, int screenHeight, unsigned testFlags);
/* DrawTest(time, frameCount, w, h, backbuffer, outRayCount, testFlags), Test.h:14 / Test.cpp:344-367.
 * `backbuffer` is a HOST pointer to w*h*4 floats, read-modify-written in place (RGB blended with the
 * previous contents, alpha untouched); synchronous: on return the frame and *outRayCount are final.
 * With row sharding active (tptSetRowShard) only this rank's rows are touched. */
TPT_API int tptDraw(float time, int frameCount, int screenWidth, int screenHeight, float* backbuffer, int* outRayCount,
            unsigned testFlags);
/* The host-pointer path above keeps the reference's contract (synchronous, the caller's buffer read-modify-written in
 * place); three things make it fast, none changes a byte of the result:
 *  - the upload of the previous image, the blend and the download are done in four row bands on two streams, so that a
 *    band's blend and download do not wait for the whole upload.  The caller's memory is NOT page-locked: it is the
 *    caller's to free between calls, and both directions run at link speed from pageable memory (measured: 0.27-0.30 ms
 *    each for 1280x720; they do not overlap -- a copy on pageable memory returns when it is done);
 *  - tptSetHostBufferMode(1): the caller promises that nobody but DrawTest writes the backbuffer between calls (true of
 *    every reference host: TestWin.cpp:73-74,315-316; Renderer.mm:225; Emscripten/main.cpp:59-60) -- the device-resident
 *    accumulation tile is then the source of truth and the buffer is uploaded once per buffer / size / frameCount == 0
 *    instead of every frame.  Default 0: upload every frame, exactly as the reference's semantics demand;
 *  - tptSetHostLookahead(n), default 2: after DrawTest(f) the library traces frames f+1 .. f+n AHEAD, guessing that the
 *    host goes on with the same size / flags / scene (what every reference host does); the next DrawTest then only
 *    blends and downloads.  A frame alone on the GPU is bound by its longest paths (1.0 ms at 1280x720x4); with three in
 *    flight the pipeline delivers one every 0.55 ms.  A wrong guess (other frame number, size, flags, scene, spp, ...) only
 *    costs GPU time: the frames traced ahead are dropped and the frame is traced again.  Never used with kFlagAnimate.
 *    In seed mode 0 (the reference's own pixels) any n > 0 means: this frame and the 31 after it as one batched launch, the
 *    batch after that as soon as this one is being served.
 *    The same look-ahead serves tptDrawDevice for a SYNCHRONOUS caller -- one whose previous frame has already been blended
 *    when its next call arrives, twice in a row, for consecutive frames of one configuration (a caller that streams frames
 *    never meets that and is unaffected): 0.98 -> ~0.55 ms per 1280x720x4 frame for a host that waits for every frame. */
TPT_API int tptSetHostBufferMode(int hostBufferOnlyWrittenByDrawTest);
TPT_API int tptSetHostLookahead(int frames);
/* how many frames were found traced ahead when their DrawTest / tptDrawDevice call arrived (monotonic; diagnostics, tests) */
TPT_API int tptGetLookaheadHits(long long* outHits);
/* GetObjectCount / GetSceneDesc, Test.h:16-17 / Test.cpp:369-384: sizes are 20 / 36 / 88 bytes and
 * the copies are byte-compatible with the reference's Sphere / Material / Camera structs. */
TPT_API int tptGetObjectCount(int* outCount, int* outObjectSize, int* outMaterialSize, int* outCamSize);
TPT_API int tptGetSceneDesc(void* outObjects, void* outMaterials, void* outCam, void* outEmissives, int* outEmissiveCount);

/* ================= 2. what the reference fixes at compile time, as run-time state ================= */

/* DO_SAMPLES_PER_PIXEL, Config.h:22 (default 4). */
TPT_API int tptSetSamplesPerPixel(int spp);
/* DO_LIGHT_SAMPLING (default 1), DO_ANIMATE_SMOOTHING (default 0.9f), DO_MITSUBA_COMPARE (default 0), Config.h:23-25 /
 * Test.cpp:95,143-145,209-214,226-227,273-274,312-313.  Without light sampling Lambert hits shoot no shadow rays and
 * emission is never suppressed; "Mitsuba compare" is the reference's only correctness method (readme.md:30): metal
 * roughness 0, constant sky (0.15, 0.21, 0.3), aperture 0 (takes effect at the next tptUpdate). */
TPT_API int tptSetConfig(int lightSampling, float animateSmoothing, int mitsubaCompare);
/* RNG seeding.  0 = ROW_SERIAL: one XorShift stream per image row carried along x (Test.cpp:280);
 * bit-identical to the reference CPU image.  A frame alone is parallel over rows only (720 lanes of work), but rows AND
 * frames are independent streams: for a static scene DrawTest / tptDraw trace the next 32 frames ahead as ONE launch (rows x
 * frames lanes) and serve them one by one (3.7 ms instead of 60-90 ms per 1280x720x4 frame), and tptDrawDeviceBatch takes up
 * to 32 frames per call (8-10 Gray/s).
 * 1 = PER_PIXEL (default): one stream per pixel, the reference's own GPU formula
 * (Cpp/Windows/ComputeShader.hlsl:380); parallel over pixels. */
TPT_API int tptSetSeedMode(int mode);
/* Colour fold.  0 = RECURSIVE (default): matE + lightE + attenuation*Trace(...) nesting of
 * Test.cpp:216, bit-identical colours.  1 = FORWARD: radiance += throughput*e (same rays, colours
 * equal up to rounding, no LDS bounce stack). */
TPT_API int tptSetFoldMode(int mode);
/* Replace the static scene tables (Test.cpp:13-31, 46-64).  spheres: count x 20 B {center xyz, radius,
 * invRadius(ignored)}; materials: count x 36 B {int type; albedo xyz; emissive xyz; roughness; ri}.
 * count <= 0 or NULL restores the built-in scene.
 * A scene may have up to TPT_MAX_LIGHTS emissive spheres (a material with a positive emissive channel, Test.cpp:334): every trace kernel
 * keeps the light table, 32 B a light, in LDS.  tptDrawDevice, tptDraw and tptDrawDeviceAnimation render every such scene -- where the
 * table does not fit beside the path-queue kernel's path records (about 2860 lights on a grouped scene) they take the lane-refill kernel,
 * frame by frame, with the same bits.  The launches that exist on the path-queue kernel only (tptDrawDeviceBatch, Views, Aov, Moments,
 * Adaptive and the clips) refuse such a scene with the number of lights they take beside it; a draw of more than TPT_MAX_LIGHTS
 * lights is refused by every entry point. */
#define TPT_MAX_LIGHTS 3072
TPT_API int tptSetScene(const void* spheres, const void* materials, int count);
/* Camera ctor arguments (Maths.h:418; defaults Test.cpp:309-319).  NULL lookFrom restores defaults. */
TPT_API int tptSetCamera(const float* lookFrom, const float* lookAt, float vfovDegrees, float aperture, float focusDist);

/* ================= 3. device-resident / multi-GPU path ================= */

/* Use an existing HIP stream (hipStream_t passed as void*, e.g. torch.cuda.current_stream().cuda_stream).
 * NULL -> the context's own stream. */
TPT_API int tptSetStream(void* hipStream);
/* Row sharding for one-process-per-GPU rendering: the image's rows are dealt out in stripes of
 * `stripeRows` rows, round-robin over `numParts` ranks; this context renders the stripes of `part`
 * into a COMPACT local tile (tptLocalRowCount(h) rows).  Seeds depend on the global (x,y) only, so
 * the union of the tiles is bit-identical to a 1-GPU render.  (0,1,0) or numParts<=1 disables. */
TPT_API int tptSetRowShard(int stripeRows, int numParts, int part);
TPT_API int tptLocalRowCount(int screenHeight);
/* global image row of local tile row `localRow` */
TPT_API int tptLocalRowToGlobal(int localRow);
/* Asynchronous draw into a DEVICE buffer holding this rank's tile: localRows*w*4 floats, the
 * accumulation buffer stays resident in HBM across frames.  Enqueued on the context's stream;
 * returns immediately.  Ray counts accumulate in a device counter (tptRayCounterRead).
 * Any positive size, sample count and sphere count: with the default configuration the path-queue kernel traces the frame up to
 * 65535 columns and rows, 2047 samples per pixel and 65534 spheres (what its packed path and pixel records hold); a frame past any
 * of these is traced by the lane-refill kernel, without a word and with the same bits and ray count (tptGetLaunchInfo shows which
 * one ran).  tptDraw takes the same route.
 * The blend is the reference's (Test.cpp:293-295), tile.rgb = tile.rgb * lerp + colour * (1 - lerp) in binary32, and it READS the tile
 * even where lerp is 0 (frame 0, or no kFlagProgressive): a NaN or an infinity the caller left in the tile comes out as NaN
 * (inf * 0) also there, while every finite previous value, -0 and subnormals included, leaves frame 0's colour as it is.  The
 * tile's alpha is returned bit for bit -- a NaN's payload included; no arithmetic touches it.  The same holds for tptDrawDeviceBatch,
 * tptDrawDeviceBatchMoments (also for its moments' .w, and for all four channels of its guide planes' previous values) and
 * tptDrawDeviceAdaptive (with its own lerp factor), and a tile mirror (tptSetTileMirror) receives the blended pixel with that alpha. */
TPT_API int tptDrawDevice(float time, int frameCount, int screenWidth, int screenHeight, float* deviceTile, unsigned testFlags);
/* Several frames per launch: frames firstFrame .. firstFrame + nFrames - 1 of the scene and camera as of the last tptUpdate
 * (what the reference's main loop renders while nothing moves: TestWin.cpp:313-316 with kFlagAnimate off), traced by ONE
 * kernel launch and blended into the tile in frame order by one more.  Bit-identical to nFrames tptDrawDevice calls; a
 * launch's fixed costs (pool ramp-up and drain, no launch shorter than its longest pixel, queue latencies) are paid once
 * per batch instead of once per frame -- what bounds small frames and tiles of a sharded frame.  Path-queue kernel only
 * (the default; so at most 2047 samples per pixel and 65534 spheres, unless the seeds are row-serial); frames up to 8192 x 8192, 32
 * to a launch (a longer call is several launches); kFlagAnimate is refused (the scene changes every frame: tptDrawDeviceAnimation).
 * nFrames = 1 is tptDrawDevice, with everything it accepts. */
TPT_API int tptDrawDeviceBatch(float time, int firstFrame, int nFrames, int screenWidth, int screenHeight, float* deviceTile, unsigned testFlags);
/* Frames of an ANIMATED scene at times the caller knows (a clip at a fixed frame rate, a video export, a dataset), up to 32 per
 * launch.  Frame j (0 <= j < nFrames) is bit-identical to tptUpdate(times[j], firstFrame + j, w, h, testFlags) followed by
 * tptDrawDevice(times[j], firstFrame + j, w, h, deviceTile, testFlags), with the same ray count: seeds, lerp factor (with
 * animateSmoothing), light list and all.  deviceTile ends as that sequence leaves it.  deviceFrameImages: NULL or nFrames consecutive
 * device tiles of h*w*4 floats; tile j receives the tile as it stands right after frame j is blended (what a host reading the tile
 * after each DrawTest sees).  deviceFrameRays: NULL or nFrames int64 in device memory, OVERWRITTEN with each frame's rays; the
 * context's counter advances by their sum.  Asynchronous on the context's stream.
 * Afterwards the context is where the sequence leaves it: spheres 1 and 8 at times[nFrames - 1] (tptGetSceneDesc), that frame's scene
 * staged (a tptDrawDevice without tptUpdate draws what it draws after the sequence), the camera of tptUpdate; frames traced ahead and
 * stream-batch planes are dropped first.  Without kFlagAnimate, or with 8 spheres or fewer, nothing moves: the frames are those of
 * tptDrawDeviceBatch(times[0], firstFrame, nFrames, ...), plus the optional outputs.
 * One launch per 32 frames with per-pixel seeds, the recursive fold and the path-queue kernel (the defaults), on scenes under 256
 * spheres (any size when nothing moves); row-serial seeds, the forward fold and other kernel variants -- animated or not -- and
 * animated scenes of 256 spheres and more take one launch per frame, with the same bits.  A non-finite time affects its own frame only.
 * Refused (non-zero, tptGetLastError, no tile or ray count written, the context untouched): nFrames < 1, times or deviceTile NULL,
 * no tptUpdate at this size, w or h over 8192, colour planes over 4096 MiB per launch, row sharding or a communicator, a tile mirror.
 * A failure after the first launch was enqueued (a HIP error; a scene tptDrawDevice would refuse too) returns non-zero with the
 * earlier launches' frames enqueued and the context where the sequence stood at the failing launch's last frame. */
TPT_API int tptDrawDeviceAnimation(int firstFrame, int nFrames, const float* times, int screenWidth, int screenHeight,
                                   float* deviceTile, float* deviceFrameImages, int64_t* deviceFrameRays, unsigned testFlags);
/* One frame with the first-hit planes a denoiser takes as guides.  deviceTile is blended exactly as tptDrawDevice(time, frameCount,
 * w, h, deviceTile, testFlags) blends it, with the same ray count.  deviceAlbedo / deviceNormalDepth: device buffers of h*w*4 floats,
 * row-major like the tile, either may be NULL (not both); OVERWRITTEN (never blended: the progressive flag applies to the colour only).
 * For every sample s of pixel (x, y), r_s is the sample's camera ray (its jitter and lens draws from the pixel's RNG stream as the
 * trace reaches them) and h_s = HitWorld(r_s) its nearest hit (ties to the lowest sphere index).  On a hit: albedo a_s = the material's
 * albedo, normal n_s = (pos - centre) * invRadius, depth d_s = t, coverage c_s = 1; on a miss all four are 0.  Then
 *   albedo[px]      = {sum a_s, sum c_s} * (1.0f / spp)      normalDepth[px] = {sum n_s, sum d_s} * (1.0f / spp)
 * float sums from +0 in sample order.  The scene is that of the last tptUpdate.  Asynchronous on the context's stream: work enqueued
 * there before the call finishes before the planes are written, work enqueued after it sees them.  Frames traced ahead and
 * stream-batch planes are dropped (the call does not continue a sequence); the camera and the scene are unchanged.
 * Refused (non-zero, tptGetLastError, no tile or plane written): deviceTile NULL or both planes NULL, no tptUpdate at this size, w or h
 * over 8192, row-serial seeds, the forward fold, a kernel variant other than the path-queue kernel, spp over 2047, more than 65534
 * spheres, row sharding or a communicator, a tile mirror. */
TPT_API int tptDrawDeviceAov(float time, int frameCount, int screenWidth, int screenHeight, float* deviceTile,
                             float* deviceAlbedo, float* deviceNormalDepth, unsigned testFlags);
/* An edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) of a tile, guided by the planes of tptDrawDeviceAov.  All five
 * buffers are device buffers of h*w*4 floats, row-major like the tile; deviceAlbedo and deviceNormalDepth may be NULL.  Binary32, in
 * the order written, no FMA, correctly rounded division, sums from +0:
 *   hk = {1/16, 1/4, 3/8, 1/4, 1/16};  ic0 = sigmaColour > 0 ? 1 / sigmaColour^2 : 0  (in, id likewise)
 *   cur_0 = DEMODULATE ? (albedo.c > 0 ? colour.c / albedo.c : colour.c) : colour           (per channel r, g, b)
 *   iteration i (0 .. iterations-1), step s = 1 << i, ic = ic0 * 4^i; for each pixel p, the 5 x 5 taps q = p + (k - 2) s (ky outer)
 *   that lie inside the image (no clamping):
 *     den = 1 + ((dr*dr + dg*dg) + db*db) * ic          (d = cur_i[q] - cur_i[p])
 *     with normalDepth: den *= 1 + ((dnx*dnx + dny*dny) + dnz*dnz) * in;  den *= 1 + (dd*dd) * id    (dd = nd[q].w - nd[p].w)
 *     w = (hk[ky] * hk[kx]) / den;  cur_{i+1}[p].rgb = sum(w cur_i[q].rgb) / sum(w)
 *   out.rgb = DEMODULATE ? (albedo.c > 0 ? cur_N.c * albedo.c : cur_N.c) : cur_N;  out.a = colour.a
 * Asynchronous on the context's stream (ordered like tptDisplayRGBA8); needs tptInitialize only; leaves every other state alone
 * (frames traced ahead and stream batches are kept).  The inputs are never written.  Refused (non-zero, tptGetLastError, nothing
 * enqueued, deviceOut untouched): no context; w or h outside 1..8192; deviceColour or deviceOut NULL; deviceOut overlapping an input;
 * iterations outside 1..8; a sigma negative, NaN, infinite, inside (0, 1e-6) or above 1e6; sigmaNormal or sigmaDepth non-zero without
 * deviceNormalDepth; TPT_DENOISE_DEMODULATE without deviceAlbedo; an unknown flag bit. */
enum { TPT_DENOISE_DEMODULATE = 1 << 0 };
TPT_API int tptDenoiseDevice(int screenWidth, int screenHeight, const float* deviceColour, const float* deviceAlbedo,
                             const float* deviceNormalDepth, float* deviceOut, int iterations, float sigmaColour,
                             float sigmaNormal, float sigmaDepth, unsigned denoiseFlags);
/* One frame with the per-pixel luminance moments of its samples, for tptDenoiseDeviceVariance.  deviceTile is blended exactly as
 * tptDrawDevice blends it, with the same ray count; deviceAlbedo / deviceNormalDepth (either or both may be NULL) are overwritten
 * byte for byte as tptDrawDeviceAov writes them.  deviceMoments (required): h*w*4 floats, row-major like the tile.  For every sample s
 * of a pixel, c_s is the colour the trace adds to the pixel's sum and l_s = (0.2126f*c_s.x + 0.7152f*c_s.y) + 0.0722f*c_s.z (binary32,
 * no FMA); the frame's moments are {sum l_s, sum l_s*l_s, 0} * (1.0f / spp), float sums from +0 in sample order, and they are blended
 * into deviceMoments.xyz with the tile's own arithmetic (the same lerp factor; .w untouched): a progressive caller holds running
 * means of l and l^2 over all its samples.  Ordering, state and refusals are tptDrawDeviceAov's (asynchronous on the context stream,
 * ordered behind earlier work there; frames traced ahead and stream-batch planes dropped; camera and scene unchanged), and also
 * refused: deviceMoments NULL, or overlapping the tile or a given plane.  A refused call writes nothing. */
TPT_API int tptDrawDeviceMoments(float time, int frameCount, int screenWidth, int screenHeight, float* deviceTile,
                                 float* deviceAlbedo, float* deviceNormalDepth, float* deviceMoments, unsigned testFlags);
/* Progressive frames with averaged guides: nFrames consecutive frames of the scene and camera of the last tptUpdate, up to 32 per
 * launch, folded into the four planes tptDenoiseDeviceVariance reads.  deviceTile and deviceMoments are required; deviceAlbedo and
 * deviceNormalDepth may each be NULL; all four are h*w*4 floats in device memory.  For j = 0 .. nFrames-1, in order, the call is byte
 * for byte, and ray for ray, this sequence:
 *   tptDrawDeviceMoments(time, firstFrame + j, w, h, deviceTile, A_j, ND_j, deviceMoments, testFlags);
 *   deviceAlbedo      = deviceAlbedo      * lerp_j + A_j  * (1 - lerp_j)      (all four channels)
 *   deviceNormalDepth = deviceNormalDepth * lerp_j + ND_j * (1 - lerp_j)      (all four channels)
 * A_j and ND_j are scratch planes; lerp_j is the factor tptDrawDevice blends frame firstFrame + j's tile with under testFlags
 * (Test.cpp:272-276).  The blend is the tile's: binary32, in the order written, no FMA, 1 - lerp_j formed in binary32.  The tile's alpha
 * and the .w of the moments are untouched.  Without TPT_FLAG_PROGRESSIVE lerp is 0 and the planes end as the last frame's.  As for the
 * tile, the planes must hold finite values before the first call (a caller zeroes them once).  Afterwards the four planes are the
 * inputs of tptDenoiseDeviceVariance with samples = spp * (firstFrame + nFrames) (progressive; spp otherwise).
 * The scene and camera are those of the last tptUpdate and are unchanged afterwards; frames traced ahead and stream-batch planes are
 * dropped first; the ray counter advances by the frames' rays, exactly once.  Asynchronous on the context stream, ordered behind
 * earlier work there; the launches of one call may overlap as tptDrawDeviceAnimationMoments' do.  Frames per launch: the most, up to
 * 32, whose staging (colour, moments and each given guide plane, h*w*16 bytes each per frame) stays within 4096 MiB -- a large frame
 * lowers the count and is never refused for it; scenes of 8 spheres or fewer, or of 256 or more, are traced a frame per launch.
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, no byte written): everything tptDrawDeviceMoments refuses;
 * nFrames < 1; firstFrame < 0 or a last frame number that does not fit an int; any flag bit other than TPT_FLAG_PROGRESSIVE
 * (TPT_FLAG_ANIMATE belongs to tptDrawDeviceAnimationMoments); any two of the four planes sharing a byte; a scene with more lights
 * than the path-queue kernel takes. */
TPT_API int tptDrawDeviceBatchMoments(float time, int firstFrame, int nFrames, int screenWidth, int screenHeight, float* deviceTile,
                                      float* deviceMoments, float* deviceAlbedo, float* deviceNormalDepth, unsigned testFlags);
/* The frames of an ANIMATED clip, each with the planes the denoising chain reads (tptTemporalAccumulateDevice, tptDenoiseDeviceVariance),
 * up to 32 per launch: tptDrawDeviceAnimation with tptDrawDeviceMoments' outputs.  Frame j (0 <= j < nFrames) is bit-identical to
 *   tptUpdate(times[j], firstFrame + j, w, h, testFlags);
 *   tptDrawDeviceMoments(times[j], firstFrame + j, w, h, deviceTile, albedo_j, normalDepth_j, deviceMoments, testFlags);
 * with albedo_j = deviceFrameAlbedo + j*h*w*4 (NULL if deviceFrameAlbedo is NULL), likewise normalDepth_j, and the same ray count.
 * deviceTile and deviceMoments (both required, h*w*4 floats) end as that sequence leaves them: blended with the tile's lerp factor per
 * frame, .w of the moments untouched.  The five per-frame outputs are each optional (NULL): deviceFrameImages, deviceFrameAlbedo,
 * deviceFrameNormalDepth, deviceFrameMoments -- nFrames consecutive device planes of h*w*4 floats each -- and deviceFrameRays, nFrames
 * int64 in device memory.  Image j is the tile, and moments plane j is deviceMoments (all four channels), as they stand right after
 * frame j's blends (what a host copying them after each frame sees); deviceFrameRays[j] is OVERWRITTEN with frame j's rays and the
 * context's counter advances by their sum.  Without TPT_FLAG_PROGRESSIVE every frame image and moments plane is that frame's own:
 * plane j of each per-frame output is the input tptTemporalAccumulateDevice asks for.  Asynchronous on the context's stream, ordered
 * behind earlier work there.  Afterwards the context is where tptDrawDeviceAnimation leaves it: spheres 1 and 8 at times[nFrames - 1],
 * that scene staged, the camera of tptUpdate; frames traced ahead and stream-batch planes are dropped first.  A non-finite time affects
 * its own frame only.
 * One trace launch per 32 frames while the scene moves (kFlagAnimate, more than 8 spheres) and has fewer than 256 spheres.  Animated
 * scenes of 256 spheres and more, and scenes in which nothing moves (no kFlagAnimate, or 8 spheres or fewer), take one launch per
 * frame (tptDrawDeviceMoments' kernel), with the same bits.  The launches of one call overlap (each waits for the blends of the launch
 * before the previous one only); separate calls are ordered on the context stream, so a long clip is best passed in one call.  The
 * library stages colour and moments of a launch's frames: up to 3 * h*w*16 bytes per frame of a launch beside the colour slots.
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, no buffer written, spheres not moved): nFrames < 1; times,
 * deviceTile or deviceMoments NULL; no tptUpdate at this size; w or h over 8192; colour and moments staging of one launch (2 * h*w*16
 * bytes per frame of the launch) over 4096 MiB; any two of the seven buffers overlapping, each taken at its full extent; row-serial
 * seeds, the forward fold, a kernel variant other than the path-queue kernel, spp over 2047, more than 65534 spheres; row sharding or a
 * communicator; a tile mirror.  A failure after the first launch was enqueued is tptDrawDeviceAnimation's. */
TPT_API int tptDrawDeviceAnimationMoments(int firstFrame, int nFrames, const float* times, int screenWidth, int screenHeight,
                                          float* deviceTile, float* deviceMoments,
                                          float* deviceFrameImages, float* deviceFrameAlbedo, float* deviceFrameNormalDepth,
                                          float* deviceFrameMoments, int64_t* deviceFrameRays, unsigned testFlags);
/* tptDrawDeviceAnimationMoments with a CAMERA PER FRAME: a turntable or fly-through with the planes the denoising chain reads, or the
 * views of a multi-view dataset with depth, normal and albedo each, up to 32 per launch.  views: host memory, nFrames x 9 floats in
 * tptDrawDeviceViews' layout {lookFrom[3], lookAt[3], vfovDegrees, aperture, focusDist}.  Frame j (0 <= j < nFrames) is bit-identical to
 *   tptSetCamera(views + 9*j, views + 9*j + 3, views[9*j + 6], views[9*j + 7], views[9*j + 8]);
 *   tptUpdate(times[j], firstFrame + j, w, h, testFlags);
 *   tptDrawDeviceMoments(times[j], firstFrame + j, w, h, deviceTile, albedo_j, normalDepth_j, deviceMoments, testFlags);
 * with the same ray count: the seeds are those of frame firstFrame + j (not one frame's for all, as tptDrawDeviceViews'), the lerp factor
 * is the frame's own, spheres 1 and 8 stand at times[j] (kFlagAnimate), the aperture is 0 in Mitsuba-compare mode, the aspect is w / h
 * and vup (0, 1, 0).  Every other argument, the per-frame outputs (plane j of the images and of the moments: the tile and deviceMoments
 * as they stand after frame j's blends) and the ordering are tptDrawDeviceAnimationMoments'.  outCameras: NULL, or host memory of
 * nFrames * 88 bytes, written AT CALL TIME with each frame's Camera record -- byte for byte what tptGetSceneDesc returns after that
 * frame's tptUpdate, the record tptTemporalAccumulateDevice takes as curCamera / prevCamera.
 * Afterwards the context is where that sequence leaves it: the camera set-up is views[nFrames - 1] (as after tptSetCamera), the camera
 * that of its tptUpdate, spheres 1 and 8 at times[nFrames - 1], that scene staged; frames traced ahead and stream-batch planes are
 * dropped first.
 * One trace launch per 32 frames on a scene of more than 8 and fewer than 256 spheres, whether it moves (kFlagAnimate) or not: the
 * kernel reads each frame's camera and its centres of spheres 1 and 8 from tables, and for a clip in which nothing moves the centres
 * table repeats the scene's own.  Scenes of 8 spheres or fewer and of 256 and more take one launch per frame (tptDrawDeviceMoments'
 * kernel, the camera set per frame), with the same bits.  The launches of one call overlap as tptDrawDeviceAnimationMoments' do.
 * Refused (non-zero, tptGetLastError names this function, nothing enqueued, no buffer and no byte of outCameras written, camera and
 * spheres unchanged): everything tptDrawDeviceAnimationMoments refuses -- the overlap rule covers the same seven device buffers --, and
 * views NULL. */
TPT_API int tptDrawDeviceCameraClip(int firstFrame, int nFrames, const float* times, const float* views,
                                    int screenWidth, int screenHeight, float* deviceTile, float* deviceMoments,
                                    float* deviceFrameImages, float* deviceFrameAlbedo, float* deviceFrameNormalDepth,
                                    float* deviceFrameMoments, int64_t* deviceFrameRays, void* outCameras, unsigned testFlags);
/* tptDrawDeviceCameraClip with the motion given by the CALLER instead of by times: a clip of a scene the caller animates (a video export,
 * a dataset of clips), with the planes the denoising chain reads, up to 32 frames per launch.  views: host memory, nFrames x 9 floats, as
 * tptDrawDeviceCameraClip's (required).  movedIds: host memory, nMoved distinct sphere indices; centres: host memory, nFrames x nMoved x 3
 * floats, frame-major: centres[(j*nMoved + k)*3 ..] is where sphere movedIds[k] stands in frame j.  nMoved == 0: both may be NULL and
 * nothing moves.  Radii and materials are the scene's own: spheres only translate, as in tptTemporalAccumulateObjectsDevice's table.
 * Let S_j be the context's spheres (tptGetSceneDesc) with the centres of the moved ids replaced by frame j's.  Frame j (0 <= j < nFrames)
 * is bit-identical, with the same ray count, to
 *   tptSetScene(S_j, materials, count);
 *   tptSetCamera(views + 9*j, views + 9*j + 3, views[9*j + 6], views[9*j + 7], views[9*j + 8]);
 *   tptUpdate(0.0f, firstFrame + j, w, h, testFlags);
 *   tptDrawDeviceMoments(0.0f, firstFrame + j, w, h, deviceTile, albedo_j, normalDepth_j, deviceMoments, testFlags);
 * the seeds are those of frame firstFrame + j, the lerp factor is the frame's own, the light list holds the moved centres of emissive
 * spheres, the aperture is 0 in Mitsuba-compare mode.  deviceTile, deviceMoments, the five per-frame outputs, outCameras (written at call
 * time) and the ordering are tptDrawDeviceCameraClip's.  deviceFrameObjects: NULL, or nFrames device planes of h*w int32; plane j holds
 * the bytes tptObjectPlaneDevice(1, NULL, outCameras_j, w, h, plane_j, 0) writes right after frame j's tptUpdate in the sequence above:
 * the centre ray's HitWorld id over S_j, -1 for a miss -- with the call's cameras and api.motion_table(S_{j-1}, S_j) the inputs of
 * tptTemporalAccumulateObjectsDevice.
 * testFlags: TPT_FLAG_PROGRESSIVE or 0.  TPT_FLAG_ANIMATE is REFUSED: the table is the motion, and the reference's rule for spheres 1 and 8
 * is not applied on top of it (a caller who wants it passes those centres).
 * Afterwards the context is where that sequence leaves it: its spheres are S_{nFrames-1} and that scene is staged, the camera set-up is
 * views[nFrames - 1] (as after tptSetCamera), the camera that of its tptUpdate; frames traced ahead and stream-batch planes are dropped
 * first.
 * One trace launch per 32 frames when the scene has fewer than 256 spheres, nMoved <= 8 and every moved id is below 64: the kernel reads
 * each frame's camera and its moved centres from tables and tests the moved spheres for every ray.  Every other accepted call -- nMoved
 * over 8, an id of 64 or above, 256 spheres or more -- goes frame by frame (tptDrawDeviceMoments' kernel, the spheres and the camera set
 * per frame), with the same bits.  The launches of one call overlap as tptDrawDeviceAnimationMoments' do.  For a call that asks for object
 * planes the library keeps the {centre, r^2} arrays of two launches' frames, filled and copied launch by launch: at most
 * 2 x 32 x count x 16 bytes of device memory and as much pinned host memory whatever nFrames is (67 MB each at 65534 spheres, 94 KB for
 * the built-in scene), until tptShutdown.
 * Refused (non-zero, tptGetLastError names this function, nothing enqueued, no buffer and no byte of outCameras written, camera and
 * spheres unchanged): what tptDrawDeviceCameraClip refuses of sizes, a missing tptUpdate at this size, staging over 4096 MiB, seed mode,
 * fold, kernel variant, spp over 2047, more than 65534 spheres, sharding or a communicator, a tile mirror, views NULL; nMoved < 0 or above
 * the sphere count; movedIds or centres NULL with nMoved > 0; an id outside 0 .. count-1; a repeated id; a centre that is not finite; any
 * flag bit other than TPT_FLAG_PROGRESSIVE; any two of the eight device buffers -- the camera clip's seven and the object planes --
 * overlapping, each taken at its full extent; with deviceFrameObjects, a view whose camera tptObjectPlaneDevice refuses (a non-finite
 * origin, lowerLeftCorner, horizontal or vertical). */
TPT_API int tptDrawDeviceKeyframeClip(int firstFrame, int nFrames, const float* views,
                                      int nMoved, const int32_t* movedIds, const float* centres,
                                      int screenWidth, int screenHeight, float* deviceTile, float* deviceMoments,
                                      float* deviceFrameImages, float* deviceFrameAlbedo, float* deviceFrameNormalDepth,
                                      float* deviceFrameMoments, int64_t* deviceFrameRays, int32_t* deviceFrameObjects,
                                      void* outCameras, unsigned testFlags);
/* The spatial filter of SVGF (Schied et al., HPG 2017) in tptDenoiseDevice's rational form: an a-trous filter whose luminance term is
 * scaled by a per-pixel variance made from tptDrawDeviceMoments' moments and carried through the iterations.  All six buffers are
 * device buffers of h*w*4 floats; deviceAlbedo and deviceNormalDepth may be NULL.  samples: how many samples the colour and the moments
 * average (spp * (frameCount + 1) for a static progressive caller, spp for a single frame).  Binary32, in the order written, no FMA,
 * correctly rounded division, sums from +0 in the order written (ky, jy outer):
 *   lum(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b;  hk = {1/16, 1/4, 3/8, 1/4, 1/16};  gk = {1/4, 1/2, 1/4}
 *   sl2 = sigmaLuminance * sigmaLuminance;  in, id = 1 / sigma^2 (0 for a sigma of 0), as tptDenoiseDevice's
 *   cur_0 = colour, demodulated as tptDenoiseDevice does under TPT_DENOISE_DEMODULATE
 *   v_0[p] = (d > 0 ? d : 0) / samples,  d = m.y - m.x*m.x,  m = moments[p]
 *            with DEMODULATE and la2 = la*la > 0 (la = lum(albedo[p])):  v_0[p] = v_0[p] / la2
 *   iteration i (0 .. iterations-1), step s = 1 << i; for each pixel p:
 *     g  = sum of (gk[jy]*gk[jx]) * v_i[q'] over the 3x3 unit-spaced q' = p + (j - 1) inside the image, / sum of those (gk[jy]*gk[jx])
 *     il = s / (sl2 * g + TPT_DENOISE_VARIANCE_EPS)     (the step: sigma^2 halved per iteration)
 *     over the 5x5 taps q = p + (k - 2) s inside the image:
 *       den = 1 + (dl*dl) * il     (dl = lum(cur_i[q]) - lum(cur_i[p]));  with normalDepth den *= the normal and depth factors of
 *       tptDenoiseDevice (not scaled per iteration);  w = (hk[ky]*hk[kx]) / den
 *     cur_{i+1}[p].rgb = sum(w cur_i[q].rgb) / sum(w);   v_{i+1}[p] = sum((w*w) v_i[q]) / (sum(w)*sum(w))
 *   out.rgb = cur_N remodulated under DEMODULATE (as tptDenoiseDevice);  out.a = colour.a
 * The step in il's numerator makes each iteration twice as strict as the one before; the carried variance alone let 5 iterations blur
 * a 64-frame image past its own noise.  The guides should describe the same samples as the colour: a progressive
 * caller averages the albedo and normal / depth planes over its frames as the tile is averaged (one frame's 4-spp planes beside
 * a 256-sample colour mis-demodulate and mis-guide the edges): tptDrawDeviceBatchMoments does that, and states the blend.  Asynchronous on the context stream; needs
 * tptInitialize only and leaves every other state alone.  The inputs are never written.  Refused (non-zero, tptGetLastError, nothing
 * enqueued, deviceOut untouched): tptDenoiseDevice's refusals (sigmaNormal, sigmaDepth, iterations, flags, sizes, overlaps), and
 * deviceMoments NULL or overlapping deviceOut, samples not finite or below 1, sigmaLuminance not in (0, 1e6]. */
#define TPT_DENOISE_VARIANCE_EPS 1e-4f
TPT_API int tptDenoiseDeviceVariance(int screenWidth, int screenHeight, const float* deviceColour, const float* deviceAlbedo,
                                     const float* deviceNormalDepth, const float* deviceMoments, float samples, float* deviceOut,
                                     int iterations, float sigmaLuminance, float sigmaNormal, float sigmaDepth, unsigned denoiseFlags);
/* The temporal part of SVGF: this frame's planes blended with a history that is fetched through the previous camera and kept only where
 * it shows the same surface.  Its outputs feed tptDenoiseDeviceVariance.  camera / prevCamera: HOST pointers to 88-byte Camera records
 * (tptGetSceneDesc's outCam), read at call time.  All twelve device buffers are h*w*4 floats, row-major like the tile.  deviceColour,
 * deviceAlbedo, deviceNormalDepth, deviceMoments: what one tptDrawDeviceMoments call without TPT_FLAG_PROGRESSIVE on a zeroed tile and
 * moments plane writes.  devicePrevColour / devicePrevAlbedo / devicePrevMoments: the OUTPUTS of the previous call of this function;
 * devicePrevNormalDepth: the previous frame's own normal / depth plane; prevCamera: the camera that frame was traced with (a caller
 * ping-pongs two sets).  The four prev planes and prevCamera are all NULL for the first frame of a sequence.  deviceOutMoments.w carries
 * the pixel's history length N (>= 1); devicePrevMoments.w is read as N.
 * Binary32, in the order written, no FMA, correctly rounded division and square root, sums from +0;  dot(a, b) = (a.x*b.x + a.y*b.y)
 * + a.z*b.z;  vectors component by component.  Camera fields o = origin, ll = lowerLeftCorner, H = horizontal, V = vertical, w = ww;
 * primed: prevCamera's.  Once per call:  a = ll' - o';  f = -dot(a, w');  hh = dot(H', H');  vv = dot(V', V').
 * Per pixel p = (x, y), with cur = the four current planes at p and c = albedo[p].w (the coverage):
 *   1. s = (x + 0.5f) / width;  t = (y + 0.5f) / height;  v = ((ll + s*H) + t*V) - o;  dir = v * (1.0f / sqrt(dot(v, v)))
 *      c > 0:  d = nd[p].w / c;  n = nd[p].xyz / c;  rel = (o + dir*d) - o'        otherwise (sky):  rel = dir
 *   2. z = -dot(rel, w');  no history unless z > 0.  k = f / z;  q = rel*k - a;  s' = dot(q, H') / hh;  t' = dot(q, V') / vv;
 *      px = s' * width - 0.5f;  py = t' * height - 0.5f;  no history unless px and py are finite
 *   3. ix = floor(px);  fx = px - ix;  fx < TPT_TEMPORAL_SNAP: fx = 0;  else fx > 1 - TPT_TEMPORAL_SNAP: ix = ix + 1, fx = 0;  likewise
 *      iy, fy  (a camera that has not moved reads exactly its own pixel)
 *   4. the taps (ix + i, iy + j), i, j in {0, 1}, j outer, with b = (i ? fx : 1 - fx) * (j ? fy : 1 - fy).  A tap counts if b > 0, it
 *      lies inside the image, N' = prevMoments.w of the tap is finite and >= 1, prevColour.rgb of the tap is finite, and, with
 *      c' = prevAlbedo.w of the tap,  |c - c'| <= coverageTolerance  and either
 *        c == 0 and c' == 0  (sky), or
 *        c > 0 and c' > 0,  |e - d'| <= depthTolerance * e  with e = sqrt(dot(rel, rel)), d' = prevNd.w / c',  and
 *        (dx*dx + dy*dy) + dz*dz <= normalTolerance  with (dx, dy, dz) = n - prevNd.xyz / c'
 *   5. B = sum of b over the counted taps.  None counted, no history, or the first frame:  N = 1 and out = cur.  Otherwise
 *      hist = (sum of b * value') / B  for colour.rgb, albedo.xyzw, moments.xy and N';  N = histN + 1, maxHistory if that is smaller;
 *      lerp = (N - 1) / N;  out = hist * lerp + cur * (1 - lerp)  -- the tile's own blend: with agreeing history and an unmoved camera
 *      the colour is the progressive tile of N frames, byte for byte
 *   6. outColour = {out.rgb, colour[p].a};  outAlbedo = out.xyzw;  outMoments = {m.x, m.y, 0, N};
 *      outVariance = {0, (dd > 0 ? dd : 0) / N, 0, N},  dd = m.y - m.x*m.x,  m = out's moments
 * deviceOutVariance is the plane to hand to tptDenoiseDeviceVariance as its deviceMoments with samples = spp: its first component is 0,
 * so the filter's v_0 becomes variance / (spp * N) per pixel -- a freshly disoccluded pixel is filtered as the one-frame pixel it is.
 * The filter's other inputs are deviceOutColour, deviceOutAlbedo and this frame's normal / depth plane.  The coverage test keeps a
 * silhouette pixel from inheriting a fully covered neighbour's history.  Objects that move are not followed: their
 * points are reprojected as if they stood still, and the depth and normal tests decide (tptTemporalAccumulateObjectsDevice below follows them).
 * Asynchronous on the context stream; needs tptInitialize only and leaves every other state alone.  The inputs are never written.
 * Refused (non-zero, tptGetLastError, nothing enqueued, no output written): no context; w or h outside 1..8192; camera NULL; a current
 * plane or an output NULL; the prev planes and prevCamera neither all NULL nor all given; an output overlapping an input or another
 * output; maxHistory not in [1, 65536]; a tolerance negative, NaN or infinite; a camera with a non-finite field, dot(H, H) == 0,
 * dot(V, V) == 0 or f <= 0. */
#define TPT_TEMPORAL_SNAP (1.0f / 128)
TPT_API int tptTemporalAccumulateDevice(int screenWidth, int screenHeight, const void* camera, const void* prevCamera,
                                        const float* deviceColour, const float* deviceAlbedo, const float* deviceNormalDepth,
                                        const float* deviceMoments, const float* devicePrevColour, const float* devicePrevAlbedo,
                                        const float* devicePrevNormalDepth, const float* devicePrevMoments, float* deviceOutColour,
                                        float* deviceOutAlbedo, float* deviceOutMoments, float* deviceOutVariance, float maxHistory,
                                        float depthTolerance, float normalTolerance, float coverageTolerance);
/* THE OBJECT PLANE: which sphere each pixel sees first, for nFrames frames.  deviceFrameObjects (required): nFrames consecutive DEVICE
 * planes of h*w int32, row-major like the tile (row 0 at the bottom).  cameras: HOST memory, nFrames x 88-byte Camera records
 * (tptDrawDeviceCameraClip's outCameras, or tptGetSceneDesc's outCam), or NULL: the camera of the last tptUpdate for every frame, and
 * w x h must then be that update's size.  times: HOST memory, nFrames floats, or NULL.
 * The scene of frame j is the context's scene as of the last tptUpdate; when times is given, TPT_FLAG_ANIMATE is set and the scene has
 * more than 8 spheres, spheres 1 and 8 stand where tptUpdate(times[j], ...) puts them (centre 1's y = cosf(t) + 1.0f, centre 8's
 * z = sinf(t) * 0.3f, the same bits).  The context's own spheres are not moved.  A non-finite time affects its own frame only.
 * (More exactly the scene is what the context last staged for a launch: tptDrawDeviceAnimation, tptDrawDeviceAnimationMoments and
 * tptDrawDeviceCameraClip stage their last frame's scene, and leave the context's spheres there, as the tptUpdate calls they stand for
 * would.  It shows only when times is NULL: after such a clip the plane is that of the clip's last frame.)
 * Binary32, in the order written, no FMA; correctly rounded division and square root; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  Per
 * pixel (x, y) of frame j, with o, ll, H, V the camera's origin, lowerLeftCorner, horizontal and vertical:
 *   s = (x + 0.5f) / width;  t = (y + 0.5f) / height;  v = ((ll + s*H) + t*V) - o;  dir = v * (1.0f / sqrt(dot(v, v)))
 *   (step 1 of tptTemporalAccumulateDevice: the ray through the pixel's centre and the lens centre, whatever spp is)
 *   id = HitWorld({o, dir}, 0.001f, 1e7f) in the reference's arithmetic and order (Maths.cpp:165-202): every sphere in index order, the
 *   nearest hit wins and equal distances go to the lowest index.  The plane receives id, or -1 for a miss.
 * An id cannot be averaged over samples: a silhouette pixel carries the id of its centre ray, whatever its coverage says.
 * Asynchronous on the context stream, ordered like tptDenoiseDevice; one launch per frame, the exact test for every sphere (grouped
 * scenes too: DESIGN.md 3.12 has the cost).  Leaves every context state alone: frames traced ahead and stream batches are kept,
 * camera and scene are unchanged.
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, nothing written): no context; no tptUpdate yet; nFrames
 * outside 1..4096; w or h outside 1..8192; deviceFrameObjects NULL; cameras NULL with a size other than the last update's; a camera
 * with a non-finite field in origin, lowerLeftCorner, horizontal or vertical; a flag bit other than the two TPT_FLAG_*. */
TPT_API int tptObjectPlaneDevice(int nFrames, const float* times, const void* cameras, int screenWidth, int screenHeight,
                                 int32_t* deviceFrameObjects, unsigned testFlags);
/* The animated scene's displacement per sphere between two times, for tptTemporalAccumulateObjectsDevice's table.  Host arithmetic only.
 * outTable: HOST memory, count x 4 floats, count = tptGetObjectCount's.  Entry i = {prevCentre_i - centre_i, 0} under tptUpdate's
 * animation rule: all zero, except that with TPT_FLAG_ANIMATE and more than 8 spheres
 *   entry 1's .y = (cosf(prevTime) + 1.0f) - (cosf(time) + 1.0f)      entry 8's .z = sinf(prevTime) * 0.3f - sinf(time) * 0.3f
 * (the two centres as tptUpdate computes them, then one subtraction).  The .w (the history cap) is 0: the caller sets caps, and uploads
 * the table.  Needs tptInitialize only; no GPU work, no state change.  Refused: no context; outTable NULL; capacity < count. */
TPT_API int tptObjectMotionTable(float time, float prevTime, unsigned testFlags, float* outTable, int capacity);
/* TEMPORAL ACCUMULATION THAT FOLLOWS OBJECTS: tptTemporalAccumulateDevice with the object planes of both frames and a table of what
 * each object did in between.  The first twenty parameters are tptTemporalAccumulateDevice's.  deviceObject (required): h*w int32, this
 * frame's object plane (tptObjectPlaneDevice).  devicePrevObject: the previous frame's plane, NULL exactly when prevCamera and the prev
 * planes are NULL.  deviceObjectMotion: DEVICE memory, nObjects x 4 floats, entry i = m_i = {where object i's points stood in the previous
 * frame minus where they stand now, m.w = the longest history a pixel of that object may carry; 0: no cap}; NULL with nObjects == 0:
 * nothing moves and nothing is capped.  The statement is tptTemporalAccumulateDevice's, with three changes:
 *   1. id = object[p].  If c > 0, the table is given and 0 <= id < nObjects:  m = motion[id]  and  rel = ((o + dir*d) + m.xyz) - o'.
 *      In every other case no entry is read and rel is exactly the plain pass's (nothing is added, so no zero changes its sign).
 *   4. a tap additionally counts only if prevObject[tap] == id -- one rule for hits, misses (-1) and silhouette pixels whose centre ray
 *      misses.  The depth test keeps its form: e = sqrt(dot(rel, rel)) is now the distance of the MOVED point from the previous
 *      camera.  The normal test is unchanged: spheres only translate.
 *   5. after N = histN + 1, maxHistory if that is smaller:  if m was read and m.w >= 1 and m.w < N, then N = m.w;  then the lerp as before.
 *      (A cap of 1 leaves a mirror or a glass sphere, whose reflections do not move with its surface, this frame's values alone.)
 * With the table NULL the pass differs from the plain one by the id test alone.  Ordering and state are tptTemporalAccumulateDevice's;
 * the inputs are never written.
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, no output written): everything tptTemporalAccumulateDevice
 * refuses; deviceObject NULL; devicePrevObject given without the prev planes or NULL with them; nObjects < 0 or > 65534; exactly one of
 * deviceObjectMotion and nObjects set; an output overlapping an object plane or the table, each taken at its full extent. */
TPT_API int tptTemporalAccumulateObjectsDevice(int screenWidth, int screenHeight, const void* camera, const void* prevCamera,
                                               const float* deviceColour, const float* deviceAlbedo, const float* deviceNormalDepth,
                                               const float* deviceMoments, const float* devicePrevColour, const float* devicePrevAlbedo,
                                               const float* devicePrevNormalDepth, const float* devicePrevMoments, float* deviceOutColour,
                                               float* deviceOutAlbedo, float* deviceOutMoments, float* deviceOutVariance, float maxHistory,
                                               float depthTolerance, float normalTolerance, float coverageTolerance,
                                               const int32_t* deviceObject, const int32_t* devicePrevObject,
                                               const float* deviceObjectMotion, int nObjects);
/* A CLIP THROUGH THE DENOISING CHAIN: the frames the clip draws leave (tptDrawDeviceAnimationMoments, tptDrawDeviceCameraClip,
 * tptDrawDeviceKeyframeClip, each without TPT_FLAG_PROGRESSIVE) taken through the temporal pass and the variance-guided filter by one
 * call.  The temporal pass is a recurrence over frames and stays one launch per frame; the filter's iterations are one launch per
 * CHUNK of frames each instead of one per frame.
 * The planes: every deviceFrame* pointer is nFrames consecutive device planes, h*w*4 floats each (deviceFrameObjects: h*w int32 each),
 * plane j frame j's -- the per-frame outputs of the clip draws as they are laid out.
 *   deviceFrameImages, deviceFrameMoments   required: the clip draws' deviceFrameImages and deviceFrameMoments
 *   deviceFrameAlbedo, deviceFrameNormalDepth   required, except in spatial-only mode, where each is optional as in
 *                                           tptDenoiseDeviceVariance
 *   cameras              HOST memory, nFrames x 88-byte Camera records (the clip draws' outCameras), read during the call; required
 *                        except in spatial-only mode, where it is ignored
 *   deviceFrameObjects   NULL, or the object planes (tptDrawDeviceKeyframeClip's, tptObjectPlaneDevice's): non-NULL selects
 *                        tptTemporalAccumulateObjectsDevice as the temporal pass
 *   deviceFrameObjectMotion, nObjects   DEVICE memory, nFrames x nObjects x 4 floats: table j is tptTemporalAccumulateObjectsDevice's
 *                        table between frame j-1 and frame j (table 0 is read only when the call continues a history); NULL with
 *                        nObjects == 0 as in that function; allowed only with deviceFrameObjects
 *   deviceFrameOut       required: the denoised frames
 *   samples, iterations, sigmaLuminance, sigmaNormal, sigmaDepth, denoiseFlags   tptDenoiseDeviceVariance's, for every frame
 *   maxHistory, depthTolerance, normalTolerance, coverageTolerance   the temporal pass's, for every frame
 *   clipFlags            TPT_CLIP_DENOISE_SPATIAL_ONLY or 0
 *   prevCamera (HOST, 88 bytes), devicePrevNormalDepth, devicePrevObject, deviceHistory   the continuation, below
 * Every byte of deviceFrameOut is what the existing entry points write:
 *   spatial-only: plane j is what tptDenoiseDeviceVariance(w, h, images_j, albedo_j, normalDepth_j, moments_j, samples, out_j,
 *     iterations, the sigmas, denoiseFlags) writes -- nFrames independent jobs (the views of a multi-view clip).
 *   otherwise: for j = 0 .. nFrames-1, T_j = the four outputs of tptTemporalAccumulateDevice(w, h, cameras_j, cameras_{j-1}, images_j,
 *     albedo_j, normalDepth_j, moments_j, T_{j-1}.colour, T_{j-1}.albedo, normalDepth_{j-1}, T_{j-1}.moments, ..., the four tolerances)
 *     -- with deviceFrameObjects of tptTemporalAccumulateObjectsDevice, with objects_j, objects_{j-1}, table j and nObjects -- and plane
 *     j is what tptDenoiseDeviceVariance(w, h, T_j.colour, T_j.albedo, normalDepth_j, T_j.variance, samples, out_j, ...) writes.
 * Continuation.  prevCamera NULL: frame 0 is the first frame of a sequence (its prev arguments are NULL); devicePrevNormalDepth and
 * devicePrevObject must be NULL.  prevCamera given: frame 0 has a predecessor, frame -1, read from prevCamera, devicePrevNormalDepth
 * (required), devicePrevObject (required exactly when deviceFrameObjects is given) and deviceHistory (required): 3 consecutive planes
 * of h*w*4 floats, T_{-1}'s colour, albedo and moments.  deviceHistory, whenever it is given, is WRITTEN at the end of the call with
 * T_{nFrames-1}'s colour, albedo and moments -- in stream order after it was read, so one buffer may be passed call after call, and a
 * clip cut into calls of any lengths gives the bytes of one call.  In spatial-only mode all four must be NULL.
 * Chunks and staging.  The call works through the clip in chunks of n frames (the last one shorter), n the largest count <= 32 whose
 * staging stays within 4096 MiB (the clip draws' limit), in planes of h*w*16 bytes: n in spatial-only mode (the iterations' ping-pong
 * plane per frame), 4n + 4 otherwise (per frame T_j's colour, albedo and variance and the ping-pong plane; T's moments of two
 * consecutive frames; and the colour and albedo of the chunk's predecessor, which the last frame of a chunk is copied to before the
 * next chunk overwrites its staging).  The library owns the staging: allocated for min(n, nFrames) frames by the first call that
 * needs it (a spatial-only call with iterations == 1 needs none), grown on demand, kept until tptShutdown.
 * Asynchronous on the context stream, ordered like tptDenoiseDevice; needs tptInitialize only.  The inputs are never written; frames
 * traced ahead, stream batches, scene and camera are left alone.
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, no byte written): args NULL; no context; nFrames outside
 * 1..4096; w or h outside 1..8192; an unknown clipFlags bit; a required pointer NULL; the mode rules above violated (a camera, an
 * object, a motion or a continuation field in spatial-only mode; a table without deviceFrameObjects; a prev plane without prevCamera,
 * or a missing one with it); everything tptDenoiseDeviceVariance refuses of its scalars and flags; everything the temporal passes
 * refuse of their scalars and of every camera given; nObjects outside 0..65534, or exactly one of table and nObjects set; not even
 * one frame's staging within 4096 MiB; deviceFrameOut or deviceHistory overlapping any input or each other, each taken at its full
 * extent (nFrames planes, 3 planes, one plane for the prev planes, nFrames x nObjects x 16 bytes for the tables). */
enum { TPT_CLIP_DENOISE_SPATIAL_ONLY = 1 << 0 };
typedef struct tptClipDenoiseArgs {
    int screenWidth, screenHeight, nFrames;
    unsigned clipFlags;
    const float* deviceFrameImages;
    const float* deviceFrameMoments;
    const float* deviceFrameAlbedo;
    const float* deviceFrameNormalDepth;
    const void* cameras;
    const int32_t* deviceFrameObjects;
    const float* deviceFrameObjectMotion;
    float* deviceFrameOut;
    const void* prevCamera;
    const float* devicePrevNormalDepth;
    const int32_t* devicePrevObject;
    float* deviceHistory;
    int nObjects;
    int iterations;
    unsigned denoiseFlags;
    float samples, sigmaLuminance, sigmaNormal, sigmaDepth;
    float maxHistory, depthTolerance, normalTolerance, coverageTolerance;
} tptClipDenoiseArgs;
TPT_API int tptDenoiseClipDevice(const tptClipDenoiseArgs* args);
/* A CLIP'S MOTION VECTORS: for every pixel of every frame of a clip, where its surface point stood in the previous frame, how far from
 * that frame's camera, and how much of the bilinear footprint there shows the same surface (0: disoccluded) -- what steps 1-4 of
 * tptTemporalAccumulateDevice and tptTemporalAccumulateObjectsDevice derive for their own blend, written out: backward optical flow
 * with an occlusion mask, with the library's own motion tables, snap and surface tests.
 * The planes: every deviceFrame* pointer is nFrames consecutive device planes, h*w*4 floats each (deviceFrameObjects: h*w int32 each),
 * plane j frame j's, laid out as the clip draws and tptDenoiseClipDevice lay them out.
 *   cameras              HOST memory, nFrames x 88-byte Camera records (the clip draws' outCameras), read during the call; required
 *   deviceFrameAlbedo, deviceFrameNormalDepth   required: the clip draws' planes; albedo.w is the coverage
 *   deviceFrameObjects   NULL, or the object planes: non-NULL selects the object-following form
 *   deviceFrameObjectMotion, nObjects   DEVICE memory, nFrames x nObjects x 4 floats: table j is tptTemporalAccumulateObjectsDevice's
 *                        table between frame j-1 and frame j (table 0 is read only when prevCamera is given); NULL with nObjects == 0
 *                        as in that function; allowed only with deviceFrameObjects.  The entries' .w, the history cap, is ignored here
 *   deviceFrameMotion    required: the output, nFrames planes of h*w*4 floats
 *   prevCamera (HOST, 88 bytes), devicePrevAlbedo, devicePrevNormalDepth, devicePrevObject   frame -1, the predecessor of frame 0: all
 *                        NULL (frame 0 has no predecessor), or prevCamera and both planes given, and devicePrevObject given exactly
 *                        when deviceFrameObjects is
 *   depthTolerance, normalTolerance, coverageTolerance   the temporal pass's, for every frame
 *   flags                must be 0
 * Frame j's predecessor is plane j-1 of the same stacks with camera j-1; frame 0's is the prev set.
 * Binary32, in the order written, no FMA, correctly rounded division and square root, sums from +0;  dot(a, b) = (a.x*b.x + a.y*b.y)
 * + a.z*b.z;  vectors component by component;  every comparison with a NaN is false.  Camera fields o = origin, ll = lowerLeftCorner,
 * H = horizontal, V = vertical, w = ww; unprimed: frame j's camera; primed: its predecessor's.  Once per frame, on the host, in this
 * order:  a = ll' - o';  f = -dot(a, w');  hh = dot(H', H');  vv = dot(V', V').
 * Per pixel p = (x, y) of a frame with a predecessor, with c = albedo_j[p].w and, in the object form, id = objects_j[p]:
 *   1. s = (x + 0.5f) / width;  t = (y + 0.5f) / height;  v = ((ll + s*H) + t*V) - o;  dir = v * (1.0f / sqrt(dot(v, v)))
 *      c > 0:  d = nd_j[p].w / c;  n = nd_j[p].xyz / c;  at = o + dir*d;  in the object form, with the table given and
 *              0 <= id < nObjects:  at = at + motion_j[id].xyz  (in every other case nothing is added);  rel = at - o'
 *      otherwise (sky):  rel = dir
 *   2. z = -dot(rel, w');  k = f / z;  q = rel*k - a;  px = dot(q, H') / hh * width - 0.5f;  py = dot(q, V') / vv * height - 0.5f
 *      The pixel PROJECTS if z > 0 and px and py are finite.  If it does not, motion_j[p] = {0, 0, 0, 0}.
 *   3. fx0 = floor(px);  fx = px - fx0;  fx < TPT_TEMPORAL_SNAP: fx = 0;  else fx > 1 - TPT_TEMPORAL_SNAP: fx0 = fx0 + 1, fx = 0;
 *      likewise fy0, fy.  mv = {(fx0 + fx) - (float)x, (fy0 + fy) - (float)y}  -- the sum is formed after the snap, so a camera and a
 *      scene that stand still give exactly {0, 0}.  e = sqrt(dot(rel, rel))
 *   4. W = 0.  Only if px >= -1, px < width, py >= -1 and py < height:  ix = (int)fx0, iy = (int)fy0, and the taps are
 *      (ix + i, iy + j), i, j in {0, 1}, j outer, with b = (i ? fx : 1 - fx) * (j ? fy : 1 - fy).  A tap counts if b > 0, it lies
 *      inside the image, in the object form objects'[tap] == id, and, with c' = albedo'[tap].w,  |c - c'| <= coverageTolerance  and
 *      either
 *        c == 0 and c' == 0  (sky), or
 *        c > 0 and c' > 0,  |e - d'| <= depthTolerance * e  with d' = nd'[tap].w / c',  and
 *        (dx*dx + dy*dy) + dz*dz <= normalTolerance  with (dx, dy, dz) = n - nd'[tap].xyz / c'
 *      W = the sum of b over the counted taps.
 *   5. motion_j[p] = {mv.x, mv.y, e, W}:  mv says where, in pixels, the point stood in the previous frame, relative to this pixel;  e is
 *      its distance from the previous camera;  W in [0, 1] is how much of the bilinear footprint there shows the same surface -- 0 means
 *      disoccluded, outside the image, or another surface.
 * A frame 0 without prevCamera has no predecessor: every pixel of plane 0 is {0, 0, 0, 0}.
 * The taps read the previous frame's OWN albedo and normal / depth planes (primed: plane j-1 as traced), not an accumulated history,
 * and they do not ask for a history length or a finite colour.  That is the only difference from step 4 of
 * tptTemporalAccumulate[Objects]Device, and it is what makes the frames independent: this is no recurrence, and a clip cut into calls
 * (the prev set pointing at the last plane and camera of the call before) gives the bytes of one call.  Where the temporal pass is fed
 * frame j-1 as a first frame, W > 0 exactly where it finds a history.
 * Asynchronous on the context stream, ordered like tptDenoiseDevice; needs tptInitialize only.  The inputs are never written; frames
 * traced ahead, stream batches, scene and camera are left alone.  The cameras' constants travel in a table the library owns (one copy
 * per call, grown on demand, kept until tptShutdown).
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, no byte written): args NULL; no context; nFrames outside
 * 1..4096; w or h outside 1..8192; flags != 0; a required pointer NULL; the prev set neither all given nor all NULL (devicePrevObject
 * counts exactly when deviceFrameObjects is given, and is refused without it); a table without deviceFrameObjects; nObjects outside
 * 0..65534, or exactly one of table and nObjects set; a tolerance negative, NaN or infinite; every camera the temporal passes refuse
 * (a non-finite field, dot(H, H) == 0, dot(V, V) == 0 or f <= 0), for every record in cameras and for prevCamera; deviceFrameMotion
 * overlapping any input, each taken at its full extent (nFrames planes, one plane for the prev planes, nFrames x nObjects x 16 bytes
 * for the tables). */
typedef struct tptMotionVectorsArgs {
    int screenWidth, screenHeight, nFrames;
    unsigned flags;
    const void* cameras;
    const float* deviceFrameAlbedo;
    const float* deviceFrameNormalDepth;
    const int32_t* deviceFrameObjects;
    const float* deviceFrameObjectMotion;
    float* deviceFrameMotion;
    const void* prevCamera;
    const float* devicePrevAlbedo;
    const float* devicePrevNormalDepth;
    const int32_t* devicePrevObject;
    int nObjects;
    float depthTolerance, normalTolerance, coverageTolerance;
} tptMotionVectorsArgs;
TPT_API int tptMotionVectorsDevice(const tptMotionVectorsArgs* args);
/* HISTORY RECTIFICATION: the accumulated colour of either temporal pass clamped to what this frame's neighbourhood makes plausible,
 * and the history shortened where it had to be clamped -- the remedy for lighting that changed on a surface that itself passes every
 * geometric test (a light switched, a moving sphere's shadow or reflection).  A pass of its own behind tptTemporalAccumulateDevice or
 * tptTemporalAccumulateObjectsDevice.  All seven device buffers are h*w*4 floats, row-major like the tile (row 0 at the bottom).
 *   deviceColour, deviceMoments         this frame's planes as traced: the ones the temporal pass was given as its current planes
 *   deviceAccColour, deviceAccMoments   that pass's deviceOutColour and deviceOutMoments (.w = the history length N)
 *   deviceOutColour, deviceOutMoments, deviceOutVariance   replace the pass's colour, moments and variance planes everywhere
 *                                       downstream: colour and moments are the next frame's devicePrevColour / devicePrevMoments, colour
 *                                       and variance go to tptDenoiseDeviceVariance.  The albedo plane is a surface property: untouched
 *   radius                              1..3: the window is (2*radius + 1)^2 pixels
 *   gamma                               the window's half-width in standard deviations
 * Clamping the history hist to [lo, hi] before the blend out = hist*lerp + cur*(1 - lerp) is clamping out to [lo*lerp + cur*(1 - lerp),
 * hi*lerp + cur*(1 - lerp)] after it, and lerp follows from N: that is why this needs nothing of the pass but its outputs.
 * Binary32, in the order written, no FMA, correctly rounded division and square root, sums from +0;  rgb component by component;
 * every comparison with a NaN is false;  finite(v): |v| <= FLT_MAX.  Per pixel p = (x, y), with cur = colour[p].rgb,
 * acc = accColour[p].rgb, M = accMoments[p], N = M.w:
 *   0. V = {0, (dd > 0 ? dd : 0) / N, 0, N},  dd = M.y - M.x*M.x  -- the variance the temporal pass writes from those moments.
 *      PASS-THROUGH unless N is finite, N > 1 and all of cur and acc are finite:  outColour = accColour[p], outMoments = M (all four
 *      components, byte for byte), outVariance = V.
 *   1. The window: the pixels q = (x + i, y + j), -radius <= i, j <= radius, that lie inside the image and whose colour[q].rgb are
 *      all finite (p itself is one).  Per row j, from i = -radius to radius (left to right):  n_j = the number of its pixels,
 *      s_j = sum of colour[q].rgb,  t_j = sum of colour[q].rgb * colour[q].rgb  (a row without pixels: 0, +0, +0).  Then from
 *      j = -radius to radius (bottom to top):  n = sum of n_j,  S1 = sum of s_j,  S2 = sum of t_j.
 *      mean = S1 / n;  var = S2 / n - mean*mean;  var < 0: var = 0;  sd = sqrt(var);  g = gamma*sd
 *      lo = mean - g;  unless lo < cur: lo = cur.   hi = mean + g;  unless hi > cur: hi = cur   (so lo <= cur <= hi, also with a NaN)
 *   2. lerp = (N - 1) / N;  one = 1 - lerp  (the passes' own);   L = lo*lerp + cur*one;  U = hi*lerp + cur*one
 *      out = acc;  out < L: out = L;  out > U: out = U   (in this order)
 *   3. per channel:  a_c = 0 if out == acc (nothing clipped);  otherwise q = (acc - out) / (acc - cur), and a_c = 1 if q is not finite,
 *      0 if q < 0, 1 if q > 1, else q.   a = a_r;  a_g > a: a = a_g;  a_b > a: a = a_b
 *   4. a == 0 (nothing clipped):  the outputs of PASS-THROUGH, byte for byte what the temporal pass wrote.  Otherwise
 *      k = 1 - a;  N' = 1 + (N - 1)*k;  m.x = M.x*k + moments[p].x*a;  m.y = M.y*k + moments[p].y*a
 *      outColour = {out.rgb, accColour[p].a};  outMoments = {m.x, m.y, 0, N'};
 *      outVariance = {0, (dd > 0 ? dd : 0) / N', 0, N'},  dd = m.y - m.x*m.x
 * 1 <= N' <= N: the filter treats a rectified pixel as the short-history pixel it now is, and the next frame starts it from N'.
 * A pixel reads no accumulated value but its own, so deviceOutColour == deviceAccColour and deviceOutMoments == deviceAccMoments (exact
 * equality, either or both) rectify in place.  Asynchronous on the context stream, ordered like tptDenoiseDevice; needs tptInitialize
 * only and leaves every other state alone.  The inputs are never written (but for the in-place form).
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, no byte written): no context; w or h outside 1..8192; any
 * of the seven pointers NULL; radius outside 1..3; gamma negative, NaN or infinite; an output sharing a byte with an input or with
 * another output, each plane taken at its full extent, other than the two exact equalities above. */
TPT_API int tptRectifyHistoryDevice(int w, int h, const float* deviceColour, const float* deviceMoments,
                                    const float* deviceAccColour, const float* deviceAccMoments, float* deviceOutColour,
                                    float* deviceOutMoments, float* deviceOutVariance, int radius, float gamma);
/* SPATIAL VARIANCE ESTIMATE: the luminance variance of a pixel that has too few samples for its own moments to mean anything, taken
 * from its neighbours' first and second moments -- SVGF's fallback.  At 1 spp a frame's moments are {l, l*l}, so m.y - m.x*m.x is
 * exactly 0 and tptDenoiseDeviceVariance's luminance weights collapse; the same holds wherever a temporal pass wrote N = 1 at 1 spp
 * (every pixel of frame 0 and after a cut, every view of a 1-spp multi-view stack).  This call sits between the planes the chain has
 * and the filter it has and changes neither.  Every pointer is nFrames consecutive device planes of h*w*4 floats, plane j frame j's,
 * row-major like the tile (row 0 at the bottom), laid out as the clip draws and tptDenoiseClipDevice lay them out; nFrames == 1 is the
 * per-frame form.
 *   deviceFrameMoments      any moments plane of the chain: tptDrawDeviceMoments' own (or a stack of them from the clip draws; .w is
 *                           whatever the caller left there), or the deviceOutMoments of either temporal pass or of
 *                           tptRectifyHistoryDevice (.w = the history length N)
 *   deviceFrameNormalDepth  the normal / depth planes (normal in .xyz, depth in .w), or NULL: then both sigmas must be 0
 *   deviceFrameOutVariance  a variance plane in the temporal pass's form, {0, v/N, 0, N}: tptDenoiseDeviceVariance's deviceMoments with
 *                           samples = samplesPerFrame, or (spatial-only mode) tptDenoiseClipDevice's deviceFrameMoments
 *   samplesPerFrame         the samples per pixel of one traced frame;  minSamples: a pixel is estimated while samplesPerFrame * N is
 *                           below it (+infinity: every pixel);  radius 1..3: the window is (2*radius + 1)^2 pixels
 *   sigmaNormal, sigmaDepth tptDenoiseDevice's: a tap's weight falls with the guides' distance to the pixel's own
 * Binary32, in the order written, no FMA, correctly rounded division, sums from +0;  every comparison with a NaN is false;
 * finite(v): |v| <= FLT_MAX;  in, id = 1 / sigma^2 (0 for a sigma of 0), formed on the host as tptDenoiseDevice's.  Per pixel p of a
 * frame, with M = moments[p]:
 *   0. N = M.w;  unless N is finite and N >= 1: N = 1.   dd = M.y - M.x*M.x;   Vt = {0, (dd > 0 ? dd : 0) / N, 0, N}  -- step 6 of the
 *      temporal pass, byte for byte wherever that pass wrote N.
 *      PASS-THROUGH, out = Vt, unless samplesPerFrame * N < minSamples (the product formed in binary32).
 *   1. The window: q = p + (i, j), -radius <= i, j <= radius, j outer (bottom to top), i left to right; a window never leaves its own
 *      frame's plane.  A tap counts if it lies inside the image, moments[q].x and .y are finite, and den is finite, where
 *        without a normal / depth plane  den = 1
 *        with one                        dn = nd[q].xyz - nd[p].xyz;  den = 1 + ((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) * in;
 *                                        dz = nd[q].w - nd[p].w;  den = den * (1 + (dz*dz) * id)
 *      (the raw plane values: the same factors as tptDenoiseDevice's).  w = 1 / den;  W = sum of w;  S1 = sum of w*moments[q].x;
 *      S2 = sum of w*moments[q].y.  p itself is a tap with w = 1, and it can fail to count like any other.
 *   2. No tap counted: out = Vt.  Otherwise e1 = S1 / W;  e2 = S2 / W;  ds = e2 - e1*e1;  out = {0, (ds > 0 ? ds : 0) / N, 0, N}.
 * Two consequences.  A raw moments plane whose pixels all pass through comes back as {0, max(dd, 0), 0, 1}, which the filter reads to
 * the very same v_0 as the raw plane: its output is byte for byte the one on the raw plane.  Behind a temporal pass, every pixel with
 * samplesPerFrame * N >= minSamples carries that pass's own variance bytes.
 * Asynchronous on the context stream, ordered like tptDenoiseDevice; needs tptInitialize only; frames traced ahead, stream batches,
 * scene and camera are left alone.  The inputs are never written.
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, no byte written): no context; w or h outside 1..8192;
 * nFrames outside 1..4096; moments or output NULL; radius outside 1..3; samplesPerFrame not finite or below 1; minSamples NaN or below
 * 1; a sigma that tptDenoiseDevice refuses; a non-zero sigma without the normal / depth plane; the output sharing a byte with an
 * input, each taken at its full extent of nFrames planes. */
TPT_API int tptSpatialVarianceDevice(int screenWidth, int screenHeight, int nFrames,
                                     const float* deviceFrameMoments, const float* deviceFrameNormalDepth,
                                     float* deviceFrameOutVariance, float samplesPerFrame, float minSamples,
                                     int radius, float sigmaNormal, float sigmaDepth);
/* THE CALLER'S RAYS: what comes back along ray i, and what it meets first -- the tracer without its camera, for panorama, fisheye,
 * orthographic and stereo cameras, light and irradiance probes, picking and visibility queries, re-tracing chosen pixels, a cost map.
 * Every pointer is DEVICE memory, 16-byte aligned (deviceRayCount: 8), read or written by the kernel only:
 *   deviceRays      nRays records of 8 floats, r0 = {ox, oy, oz, seed bits}, r1 = {dx, dy, dz, unused}
 *   deviceRadiance  nRays x 4 floats {c.x, c.y, c.z, (float)k}, or NULL: first hits only
 *   deviceHits      nRays records of 8 floats {pos.x, pos.y, pos.z, t}, {normal.x, normal.y, normal.z, bits(id)}, or NULL
 *   deviceRayCount  a u64 the call ADDS the sum of its k to, or NULL
 * The scene is what the context last staged for a launch, as for tptObjectPlaneDevice with times == NULL; light sampling and the
 * mitsuba switch are tptSetConfig's, the fold tptSetFoldMode's, the HitSpheres variant tptSetKernelVariant's (the lane-refill kernel
 * traces the rays whatever `persistent` says; all variants give the same bits).  Samples per pixel and the seed mode play no part.
 * Binary32, in the order written, no FMA, correctly rounded division and square root.  Per ray i:
 *   state = bits(r0.w), or 1 where that is 0 (an xorshift32 state of 0 never leaves 0, and the reference never has one)
 *   o = r0.xyz;  d = r1.xyz, taken as given: it is NOT normalised.  Defined for finite o and finite non-zero d; any other record
 *   affects its own outputs only: its records are written, its k is counted, its path ends within the depth limit.  A defined ray
 *   whose arithmetic leaves binary32's range (|d|^2 overflows for a component near 3e38, underflows to 0 below 1e-23) gets what that
 *   arithmetic gives, Inf and NaN included; the bit pattern of a NaN in an output is not specified.
 *   hits:     id = HitWorld({o, d}, 0.001f, 1e7f) in the reference's arithmetic and order (Maths.cpp:165-202): every sphere in index
 *             order, the nearest hit wins and equal distances go to the lowest index.  A hit: pos = o + d*t, normal = (pos - centre) *
 *             invRadius, hits[i] = {pos, t}, {normal, bits(id)}.  A miss: {0, 0, 0, 0}, {0, 0, 0, bits(-1)}.
 *   radiance: c = 0.0f + Trace({o, d}, depth 0, state, doMaterialE = true) (Test.cpp:195-234; a -0 becomes +0, as in a pixel's
 *             sample sum); with tptSetFoldMode(1) Trace is the forward fold of the same path.  k = the HitWorld calls of this path,
 *             shadow rays included (what Test.cpp:122,199 count).  radiance[i] = {c, (float)k}.
 *   deviceRadiance == NULL: the path ends after its first HitWorld: k = 1, no random number drawn, nothing scattered.
 *   *deviceRayCount += the sum of k over the call.  The context's own counter (tptRayCounterRead) is not touched.
 * A ray made as the camera makes pixel (x, y)'s first sample of frame f -- the pixel's seed, two jitter draws, Camera::GetRay, the
 * state left behind as the seed word -- gives tptDrawDevice's colour of that pixel at 1 spp with per-pixel seeds, frame f, on a
 * zeroed tile.
 * Asynchronous on the context stream, ordered like tptDenoiseDevice.  Camera, scene, frames traced ahead, stream batches and row
 * sharding are left alone; a tptSetScene or tptUpdate that follows does not reach the scene the running call reads.
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, no byte written): args NULL; no context; no tptUpdate yet;
 * nRays outside 1..16777216; flags != 0; deviceRays NULL; deviceRadiance and deviceHits both NULL; an output sharing a byte with
 * deviceRays or with another output, each taken at its full extent; more than TPT_MAX_LIGHTS emissive spheres; a scene whose LDS
 * does not fit a compute unit (tptSetKernelVariant(.., .., 0) reads it from global memory). */
typedef struct tptTraceRaysArgs {
    int nRays;                          /* 1 .. 16777216 */
    unsigned flags;                     /* 0 */
    const float* deviceRays;            /* nRays x 8 floats: {ox, oy, oz, seed bits}, {dx, dy, dz, unused} */
    float* deviceRadiance;              /* nRays x 4 floats, or NULL: first hits only */
    float* deviceHits;                  /* nRays x 8 floats, or NULL */
    unsigned long long* deviceRayCount; /* device u64 the call ADDS its HitWorld calls to, or NULL */
} tptTraceRaysArgs;
TPT_API int tptTraceRaysDevice(const tptTraceRaysArgs* args);
/* OTHER LENSES: tptDrawDevice's contract with a panorama (equirectangular), fisheye (equidistant) or orthographic lens in the
 * camera's place.  All tptSetSamplesPerPixel samples of a pixel come from the pixel's own random stream in one launch and are blended
 * into the caller's tile; nothing is made on the host and no ray record is uploaded.  deviceTile: h*w*4 floats in DEVICE memory, row 0
 * at the bottom, 16-byte aligned; deviceRayCount: a device u64 (8-byte aligned) the call ADDS its HitWorld calls to, or NULL.
 * The scene is what the context last staged for a launch, as for tptTraceRaysDevice; light sampling and the mitsuba switch are
 * tptSetConfig's, the fold tptSetFoldMode's, the HitSpheres variant tptSetKernelVariant's (the lane-refill kernel traces the draw
 * whatever `persistent` says; all variants give the same bits).  The seeds are per pixel whatever tptSetSeedMode says.
 * Binary32, in the order written, no FMA, correctly rounded division and square root.  Per pixel (x, y), w = screenWidth,
 * h = screenHeight:
 *   state = (x*1973 + y*9277 + frameCount*26699) | 1;  invWidth = 1.0f / (float)w;  invHeight = 1.0f / (float)h;  colour = 0
 *   for each of the spp samples, in sequence from that one stream:
 *     u = ((float)x + RandomFloat01(state)) * invWidth;  v = ((float)y + RandomFloat01(state)) * invHeight   (Test.cpp:286-287)
 *     a = (u - 0.5f) * sx;  b = (v - 0.5f) * sy
 *     EQUIRECT: (sa, ca) = sincosf(a); (sb, cb) = sincosf(b);
 *               q = right*(cb*sa) + up*sb + forward*(cb*ca);  o = origin
 *     FISHEYE:  r = sqrtf(a*a + b*b); (st, ct) = sincosf(r * maxAngle); k = r > 0 ? st / r : 0.0f;
 *               q = right*(a*k) + up*(b*k) + forward*ct;      o = origin
 *     ORTHO:    q = forward;                                  o = (origin + right*a) + up*b
 *     d = normalize(q)  (the reference's normalize, Maths.h:301, as Camera::GetRay applies it)
 *     colour += Trace({o, d}, depth 0, state, doMaterialE = true)  (Test.cpp:195-234; with tptSetFoldMode(1) the forward fold)
 *   colour *= 1.0f / (float)spp
 *   lerp = (float)frameCount / (float)(frameCount + 1) under TPT_FLAG_PROGRESSIVE, else 0  (Test.cpp:272-276)
 *   tile.rgb = prev * lerp + colour * (1 - lerp); the alpha is untouched; prev is always read
 * Each vector*scalar is three multiplies, sums go left to right.  sincosf is glibc's sinf / cosf.  No lens draws a further random
 * number: these lenses have no aperture.
 *   *deviceRayCount += the HitWorld calls of the call, shadow rays included.  The context's own counter (tptRayCounterRead) is not
 *   touched.
 * A 1-spp draw of frame f on a zeroed tile equals tptTraceRaysDevice's colours on the rays made as above with the state left behind as
 * the seed word.
 * Asynchronous on the context stream, ordered like tptDenoiseDevice.  Camera, scene, frames traced ahead, stream batches and row
 * sharding are left alone.
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, no byte written): args NULL; no context; no tptUpdate yet;
 * screenWidth or screenHeight outside 1..8192; frameCount < 0; flags other than 0 or TPT_FLAG_PROGRESSIVE; deviceTile NULL; the tile
 * sharing a byte with the counter; an unknown kind; any non-finite field; a basis vector whose squared length lies outside
 * 0.99..1.01; a pair of basis vectors whose dot product lies outside -0.01..0.01; sx or sy not positive; EQUIRECT with
 * sx > 6.2831855f or sy > 3.1415927f; FISHEYE with sx or sy > 4 or maxAngle outside (0, 3.1415927f]; maxAngle != 0 for the other
 * kinds; more than TPT_MAX_LIGHTS emissive spheres; a scene whose LDS does not fit a compute unit.  The basis check keeps |q| near 1,
 * so normalize yields the unit direction the HitSpheres filters are made for; the angle bounds keep every sincosf argument below 9. */
enum { TPT_LENS_EQUIRECT = 1, TPT_LENS_FISHEYE = 2, TPT_LENS_ORTHO = 3 };
typedef struct tptLens {
    int   kind;
    float origin[3];
    float right[3], up[3], forward[3];  /* the caller's basis, used as given */
    float sx, sy;                       /* EQUIRECT: longitude / latitude span in radians; FISHEYE: scale of the image
                                           plane (2, 2 on a square image: the image circle touches the edges); ORTHO:
                                           width / height of the window in world units */
    float maxAngle;                     /* FISHEYE: the angle from `forward` at r = 1 (equidistant projection); else 0 */
} tptLens;
typedef struct tptDrawLensArgs {
    int screenWidth, screenHeight;      /* 1 .. 8192 each */
    int frameCount;                     /* >= 0: seeds and blend, as tptDrawDevice */
    unsigned flags;                     /* 0 or TPT_FLAG_PROGRESSIVE */
    tptLens lens;
    float* deviceTile;                  /* h*w*4 floats, row 0 at the bottom, 16-byte aligned */
    unsigned long long* deviceRayCount; /* device u64 the call ADDS its HitWorld calls to, or NULL */
} tptDrawLensArgs;
TPT_API int tptDrawDeviceLens(const tptDrawLensArgs* args);
/* ADAPTIVE SAMPLING: tptDrawDeviceMoments with a sample count per pixel, so that the moments can steer the next pass (the counts come
 * from tptAdaptiveSamplesDevice below, or from the caller).  deviceSampleCounts (required): h*w int32 in DEVICE memory, row-major like the
 * tile, read by the kernels only.  Per pixel p, n = deviceSampleCounts[p] clamped to 0 .. 2047 (the path record holds 11 bits of sample
 * index); the value of tptSetSamplesPerPixel plays no part.
 *   n == 0: the pixel is not traced.  Its entries of deviceTile, deviceMoments (all four channels), deviceAlbedo and deviceNormalDepth are
 *           left untouched, and it adds no rays.
 *   n >= 1: the frame's values are byte for byte what tptDrawDeviceMoments computes for that pixel and frameCount under
 *           tptSetSamplesPerPixel(n): the pixel's own seed, its n samples drawn in sequence from that one stream, the same rays;
 *           colour = sum * (1.0f / n), moments {sum l, sum l*l, 0} * (1.0f / n), the albedo and normal / depth means * (1.0f / n)
 *           (overwritten), 1.0f / n a correctly rounded binary32 quotient.
 * The blend is weighted by SAMPLES, not by frame number, and deviceMoments.w carries the pixel's running sample count (binary32):
 *   S = deviceMoments[p].w if TPT_FLAG_PROGRESSIVE is set and that value is finite and >= 1, else 0;   S' = S + n;
 *   lerp = S / S' (correctly rounded);   tile.rgb = tile.rgb * lerp + colour * (1 - lerp), deviceMoments.xyz likewise;
 *   deviceMoments.w = S';   the tile's alpha is untouched.
 * A caller whose counts are all n and whose moments plane starts zeroed gets lerp = frame / (frame + 1): tile and moments.xyz are then
 * byte-identical to tptDrawDeviceMoments at n spp.  TPT_FLAG_ANIMATE moves the scene through tptUpdate as always, but the
 * animate-smoothing factor (tptSetConfig) does NOT enter this blend.
 * One pixel's samples run one after another in one path (the single random stream per pixel is what makes the output checkable), so a
 * launch lasts at least as long as its largest count takes: a few pixels at 2047 bound the launch from below.
 * Ordering, state and the ray counter are tptDrawDeviceMoments' (asynchronous on the context stream, ordered behind earlier work there;
 * the counter advances by the rays traced; frames traced ahead and stream-batch planes dropped; camera and scene unchanged).
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, nothing written): everything tptDrawDeviceMoments refuses
 * except a context spp over 2047; deviceSampleCounts NULL; deviceSampleCounts overlapping the tile, the moments or a given plane;
 * deviceMoments overlapping the tile or a given plane. */
TPT_API int tptDrawDeviceAdaptive(float time, int frameCount, int screenWidth, int screenHeight, float* deviceTile, float* deviceAlbedo,
                                  float* deviceNormalDepth, float* deviceMoments, const int32_t* deviceSampleCounts,
                                  unsigned testFlags);
/* Moments to sample counts: how many MORE samples each pixel should get for the relative standard error of its mean luminance to reach
 * targetError.  deviceMoments: h*w*4 floats as tptDrawDeviceAdaptive leaves them ({mean l, mean l*l, 0, S}, S the samples so far).
 * Binary32, in the order written, no FMA, correctly rounded division, sums from +0 in the order written (jy outer);
 * gk = {1/4, 1/2, 1/4}.  Per pixel p:
 *   1. m = moments[p];  S = m.w;  p is VALID if S is finite and >= 1
 *   2. d = m.y - m.x*m.x;  var = d > 0 ? d : 0
 *   3. b = m.x + TPT_ADAPTIVE_LUM_FLOOR;  r = var / (b*b)            (the relative variance of one sample)
 *   4. R = sum of (gk[jy]*gk[jx]) * r[q] over the VALID q = p + (j - 1) of the 3x3 unit neighbourhood inside the image,
 *          / sum of those (gk[jy]*gk[jx])                             (guards a 4-sample pixel whose samples happen to agree)
 *   5. p invalid, or no q valid:  n = minSamples > 1 ? minSamples : 1;  steps 6 and 7 are skipped
 *   6. need = R / (targetError*targetError);  extra = need - S
 *   7. n = minSamples if !(extra > minSamples);  else maxSamples if extra >= maxSamples;  else (int)ceilf(extra)   (a NaN: minSamples)
 * deviceSampleCounts (required, h*w int32) receives n.  deviceOutVariance (optional, h*w*4 floats) receives {0, var / S, 0, S} for valid
 * pixels and {0, 0, 0, 0} for the others -- the form of tptTemporalAccumulateDevice's variance plane: tptDenoiseDeviceVariance(...,
 * deviceMoments = that plane, samples = 1) then filters each pixel by the variance of its own mean.  deviceTotalSamples (optional, one
 * int64 in device memory) is overwritten with the sum of n over the image: the next pass's budget, known before it is launched.
 * maxSamples bounds more than the budget: one pixel's samples are traced one after another (tptDrawDeviceAdaptive), so the next
 * launch lasts at least as long as maxSamples samples of one pixel take.
 * Asynchronous on the context stream; needs tptInitialize only and leaves every other state alone.  The input is never written.
 * Refused (non-zero, tptGetLastError names the function, nothing enqueued, no output written): no context; w or h outside 1..8192;
 * deviceMoments or deviceSampleCounts NULL; targetError not finite or not in (0, 1e6]; minSamples < 0; maxSamples > 2047;
 * minSamples > maxSamples; an output overlapping the input or another output. */
#define TPT_ADAPTIVE_LUM_FLOOR 1e-2f
TPT_API int tptAdaptiveSamplesDevice(int screenWidth, int screenHeight, const float* deviceMoments, float targetError, int minSamples,
                                     int maxSamples, int32_t* deviceSampleCounts, float* deviceOutVariance,
                                     int64_t* deviceTotalSamples);
/* nViews (1..32) cameras of the scene as of the last tptUpdate, traced by ONE launch.  views: nViews x 9 floats
 * {lookFrom xyz, lookAt xyz, vfovDegrees, aperture, focusDist} -- tptSetCamera's arguments; aspect = w / h, vup (0,1,0),
 * aperture forced to 0 in Mitsuba-compare mode, as tptUpdate does.  deviceTiles: nViews consecutive device tiles of h*w*4
 * floats, each blended exactly like tptDrawDevice blends its tile (frameCount, testFlags).  deviceViewRays: NULL or nViews
 * int64 in device memory, OVERWRITTEN with this call's rays per view; the context's counter (tptRayCounterRead) advances
 * by their sum.  Asynchronous on the context's stream.
 * View v is bit-identical to tptSetCamera(views[v]...), tptUpdate(time, frameCount, w, h, testFlags), tptDrawDevice(..., tile v, ...)
 * on a tile holding the same previous contents, with the same ray count; every view uses the seeds of frameCount.  The context's
 * own camera is not changed; frames traced ahead and stream-batch planes are dropped (the call does not continue a sequence).
 * Refused (non-zero, tptGetLastError, no tile written): nViews outside 1..32, views or deviceTiles NULL, no tptUpdate at this size,
 * w or h over 8192, colour planes over 4096 MiB, row-serial seeds, the forward fold, a kernel variant other than the path-queue
 * kernel, spp over 2047, more than 65534 spheres, row sharding or a communicator, a tile mirror. */
TPT_API int tptDrawDeviceViews(float time, int frameCount, int screenWidth, int screenHeight, int nViews, const float* views,
                               float* deviceTiles, int64_t* deviceViewRays, unsigned testFlags);
/* Frame pipelining of the asynchronous path: the trace kernels of up to `frames` consecutive tptDrawDevice
 * calls may be in flight at once (each on its own internal stream, writing its own per-frame colour
 * buffer); the progressive blend into the tile (Test.cpp:293-295) is a separate, ordered kernel on the
 * context's stream, so results are bit-identical to frames=1.  1..16, default 16: the tail of frame f (a few long
 * paths) overlaps the following frames, and each launch takes only its share of the machine (2/frames-in-flight of
 * the resident workgroups; a caller that synchronises every frame gets whole-machine launches).
 * Needs one hardware queue per in-flight kernel: the host decides how many the process gets (the HIP runtime's
 * GPU_MAX_HW_QUEUES, read when the runtime starts; the library never sets it; streams that share a queue serialise, and
 * see INTEGRATION.md "Streams are not free").  tptInitialize MEASURES how many streams really run side by side and
 * clamps the pipeline to that (tptGetPipelineInfo).  Twice as many frames may be ENQUEUED ahead
 * (frames f and f + frames share a stream). */
TPT_API int tptSetFrameOverlap(int frames);
/* Stream batching (default ON since round 4; tptSetStreamBatching(0) or env TPT_STREAM_BATCH=0 turns it off): a caller that streams consecutive frames of one static configuration with SMALL frames -- fewer
 * than 2.4 M samples (rows x width x spp): tiles of a sharded frame, 640x360 -- is bound by the latency of a launch (no launch is
 * shorter than its longest pixel's sequential samples), not by arithmetic.  For such a caller tptDrawDevice / tptDrawSharded trace
 * the frames of the next 1-7 calls in the SAME launch (2 / 4 / 8 frames per launch for halves / quarters / eighths of 1280x720x4)
 * and every later call only blends its own colour plane: each frame is still delivered, in order, with its own ray count (the
 * counter and the mirrored snapshot are exact per frame), bit-identical to one launch per frame.  A call that does not continue
 * the sequence (other frame number, size, flags, scene, ...) drops the unserved planes: GPU time only.
 * Larger frames are batched too when the pipeline is shallow (few hardware queues: two launches in flight at 4 queues): enough frames
 * per launch that the launches in flight carry what 16 did, 2 then 4 then 8 at 1280x720x4 as the stream goes on; with the full
 * 16-deep pipeline they keep one frame per launch.  tptSynchronize, tptTimerEnd and tptRayCounterRead drop an open batch's unserved
 * planes, so a frame traced before the caller waited is never served after it; the next call starts a stream afresh.  The launch of a
 * dropped batch is told so while it runs: it stops tracing the frames nobody asked for, and their workgroups that have not started
 * yet trace the asked frames instead -- same bits, same ray counts, the wait is only shorter. */
TPT_API int tptSetStreamBatching(int enable);
/* Display conversion of a device-resident FULL image (w*h float4, row 0 = bottom) into w*h RGBA8 in device memory,
 * top row first: the reference's own conversion for its C++ path, Cpp/Emscripten/main.cpp:63-79
 * (c8 = min(sqrtf(c)*255, 255), alpha 255).  Enqueued on the context's stream; 4x less data to download than
 * the float buffer.  Per colour channel, in binary32: s = sqrt(c) * 255 (a correctly rounded root); a channel whose s is NaN -- c a
 * NaN or negative, which the reference converts with undefined behaviour -- or not > 0 (c either zero) is 0: a poisoned pixel shows
 * black, never white; every other channel is min(s, 255) truncated, so +infinity is 255.  The tile's alpha is ignored whatever it
 * holds (NaN included): every output alpha is 255.  The tile is not written, and nothing is written past w*h*4 bytes. */
TPT_API int tptDisplayRGBA8(const float* deviceTile, int screenWidth, int screenHeight, unsigned char* deviceRGBA);
/* Synchronise the stream and return the monotonic total of rays traced by this context. */
TPT_API int tptRayCounterRead(int64_t* outTotalRays);
/* Let the caller own the ray counter: `deviceU64` points to one zero-initialised 64-bit word in device
 * memory (e.g. a torch int64 tensor) that the kernels atomically add to; NULL -> the internal counter.
 * Lets the multi-GPU host sum-reduce the counters with RCCL without a host round trip. */
TPT_API int tptSetRayCounter(void* deviceU64);
/* Sharded hosts: from the next tptDrawDevice on, the progressive blend also writes every blended pixel of the tile to
 * `deviceMirror` (same size and layout as the tile) and the current ray-counter value to the 8 bytes at
 * `deviceCounterOut` (may be NULL) -- the snapshot handed to the collective while later frames keep accumulating into
 * the tile -- in the SAME kernel, so the frame's dependency chain stays one kernel long.  NULL turns it off.  The
 * pointers are read at enqueue time; call again to rotate buffers.  The counter written is the context's RUNNING TOTAL at
 * the moment of the blend, not a per-frame count: with later frames already tracing it includes their rays so far, and
 * is exact for "all frames up to f" only once nothing later is in flight (the last frame's snapshot after a synchronise,
 * which is what tptShardedFinish and sharding.finish() read). */
TPT_API int tptSetTileMirror(float* deviceMirror, void* deviceCounterOut);
TPT_API int tptSynchronize(void);

/* ---- multi-GPU inside the library: one process per GPU, RCCL over xGMI (replaces the row fan-out / join of
 * DrawTest, Test.cpp:357-361, across GPUs).  A C++ host needs nothing but these five calls and a way to hand 128 bytes from
 * rank 0 to the other processes (pipe, file, MPI, ...): examples/multi_gpu_host.cpp.
 *   rank 0: tptCommGetUniqueId(id);  every rank: tptInitialize (TPT_DEVICE / LOCAL_RANK picks the GPU), tptCommInit(id, n, rank, 8);
 *   per frame, every rank: tptUpdate(...); tptDrawSharded(time, f, w, h, imageOnRank0, flags);   (asynchronous)
 *   tptShardedFinish(&rays);  ...  tptCommDestroy() / tptShutdown().
 * The image's rows are dealt out in stripes of `stripeRows` rows round-robin over the ranks (cost is not uniform in y); each
 * rank keeps its compact accumulation tile resident; per frame exactly ONE collective -- ncclGather (rccl.h:745) of the
 * blended tile plus one row whose first 8 bytes carry the rank's 64-bit ray counter -- on a communication stream, from a
 * ring of 4 snapshots written by the blend kernel itself, so it overlaps the tracing of the next frames; rank 0
 * de-interleaves the gathered tiles into `deviceImageOnRoot` (w*h*4 floats, device memory; ignored on other ranks).  RNG seeds
 * depend on the global (x, y) only: the assembled image is bit-identical to a 1-GPU render.  librccl is dlopen()ed by
 * tptCommInit / tptCommGetUniqueId; a single-GPU host never loads it. */
#define TPT_COMM_ID_BYTES 128
TPT_API int tptCommGetUniqueId(void* outId128);
TPT_API int tptCommInit(const void* id128, int nRanks, int rank, int stripeRows);
/* Measurement aid, no RCCL: this process plays rank 0 of an nRanks-way run alone -- same tile, snapshot ring, events and
 * assemble kernel, a device copy of its own slice in place of the gather (the other ranks' rows of the image stay zero).
 * Shows what one GPU sustains as rank 0 of N (bench.py --emulate-ranks N).  Paired with tptCommDestroy like tptCommInit. */
TPT_API int tptCommInitLoopback(int nRanks, int stripeRows);
/* size of the communicator and this process's rank as RCCL reports them (ncclCommCount / ncclCommUserRank), loopback flag */
TPT_API int tptCommInfo(int* outRanks, int* outRank, int* outLoopback);
TPT_API int tptCommDestroy(void);
TPT_API int tptDrawSharded(float time, int frameCount, int screenWidth, int screenHeight, float* deviceImageOnRoot, unsigned testFlags);
/* How many consecutive frames tptDrawSharded collects into ONE trace launch + blend + exchange.  0 (default) = automatic: 1 when a
 * rank's tile is 2.4 M samples per frame or more (rows x width x spp) and for animated scenes; 2 / 4 / 8 below 2.4 / 1.2 / 0.6 M -- with small tiles the
 * chain behind a frame (trace launch, blend + snapshot, gather, de-interleave: four dispatches beside a machine full of trace
 * workgroups) bounds the frame rate, not the arithmetic.  k = 1..32 = the host's choice.  A frame that is collected is issued when the
 * k-th arrives, when anything it depends on is about to change (every setter, tptUpdate with another size), or when the caller waits
 * (tptShardedFinish, tptSynchronize, tptRayCounterRead): same bits as frame-by-frame calls; the image on rank 0 is current after a
 * batch has gone out and after tptShardedFinish.  EVERY rank must choose the same. */
TPT_API int tptSetShardExchangeInterval(int everyKFrames);
/* nFrames (1..32) consecutive frames per call, traced by one launch per rank (tptDrawDeviceBatch) and followed by ONE exchange:
 * rank 0's image is that of the batch's last frame.  Same bits as nFrames tptDrawSharded calls. */
TPT_API int tptDrawShardedBatch(float time, int firstFrame, int nFrames, int screenWidth, int screenHeight, float* deviceImageOnRoot, unsigned testFlags);
/* waits for every exchange enqueued so far; rank 0: sum of all ranks' ray counters as of the last gathered frame, other
 * ranks: their own.  Counters are running totals since tptInitialize / tptSetRayCounter (before the first sharded frame:
 * this rank's own running total), so callers take differences. */
TPT_API int tptShardedFinish(int64_t* outTotalRays);

/* hipEvent bracket on the context's stream, for kernel-only timing (as the reference times its
 * Dispatch with timestamp queries, TestWin.cpp:299-302). */
TPT_API int tptTimerBegin(void);
/* tptTimerEnd is a wait like tptSynchronize: it records the end event, closes an open stream batch (tptSetStreamBatching: the
 * frames traced for calls that have not come yet are dropped, and the next tptDrawDevice starts a launch of its own), then blocks
 * until the end event has completed. */
TPT_API int tptTimerEnd(float* outMilliseconds);

/* Per-launch timing of the trace kernel: between Begin and End every tptDrawDevice brackets its trace
 * launch with a hipEvent pair recorded on the stream that launch goes to (the internal trace streams when
 * frames overlap).  End synchronises and returns the SUM of the individual launch durations and their
 * number -- the same per-dispatch durations a rocprofv3 kernel trace reports. */
TPT_API int tptKernelTimingBegin(int maxLaunches);
TPT_API int tptKernelTimingEnd(float* outSumMilliseconds, int* outLaunches);

/* ================= 4. tuning and diagnostics (unit-test entry points: tpt_test_hooks.h, a separate build) ================= */

/* hitSpheres: 0 = two-phase (default: a conservative filter + the reference's exact test for what passes.  The filter runs
 * on the matrix cores for scenes of <= 64 spheres that binary16 operands can carry, as packed FP32 on the VALU otherwise;
 * scenes of 256 spheres or more are traversed through compact groups of <= 8 spheres with bounding spheres, the groups' own
 * bounds through a two-level packed filter (super-groups of 8 groups, then the groups of what passes) -- same hits, same
 * tie-break, several times faster on the 4096-sphere scene), 1 = simple loop (exact test for every sphere), 2 = two-phase
 * without grouping (brute force over all spheres, the reference's cost model), 3 = two-phase with the FLAT packed VALU filter
 * everywhere (no matrix-core table, no second level over the groups), 4 = as 0 with the bounds of a GROUPED scene on the matrix cores as well -- compiled into the
 * hooks build only (the product library refuses it): in a process the device time-slices (more than ~22 hardware queues, or
 * anything else on the GPU) waves that have run that path lose a hit in ~1e-9 of their rays, and the two-level
 * VALU filter is no slower.  persistent: 3 = path queues in LDS (default; per-pixel seeds, recursive fold, two-phase
 * only -- anything else falls back to 1), 1 = persistent waves with lane refill, 0 = ONE THREAD PER PIXEL: the same kernel with re-filling
 * off -- a wave takes an 8x8 tile and every lane keeps its pixel until the tile is done (the shape of the reference's compute shaders,
 * ComputeShader.hlsl:353-395, and of BASELINE.json's north_star; with hitSpheres 1 also its brute-force loop): kept as a live A/B,
 * 4-6 x slower than the default.  ldsScene:
 * 1 = stage sphere records and materials in LDS (default when they fit), 0 = read them from global memory, -1 = auto.
 * All variants produce identical bits. */
TPT_API int tptSetKernelVariant(int hitSpheres, int persistent, int ldsScene);
/* What the next launch will do with the scene: its sphere count, the number of sphere groups (0: the scene is traversed flat -- up to 255
 * spheres, or a scene the grouping refuses), and whether the groups' bounding spheres are filtered on the matrix cores (1: only after
 * tptSetKernelVariant(4, ..)) or by the packed VALU filter (0: the default). */
TPT_API int tptGetSceneInfo(int* outSpheres, int* outGroups, int* outBoundsOnMatrixCores);
/* kernel resource facts for DESIGN/bench: occupancy (blocks/CU), LDS bytes/block, grid size of the last launch */
TPT_API int tptGetLaunchInfo(int* outBlocksPerCU, int* outLdsBytes, int* outGridBlocks, int* outNumCUs);
/* Facts about the frame pipeline: hardware queues the runtime really runs side by side for this process (measured at
 * tptInitialize with one spinning wave per trace stream: GPU_MAX_HW_QUEUES only counts if it was set before the HIP
 * runtime started), the frames-in-flight limit that results (tptSetFrameOverlap's value clamped to what those queues can
 * carry), the deepest pipeline the caller has built so far (decides the grid of a launch), and how often the per-slot
 * buffers were (re-)allocated (once per frame shape; never on the steady-state path). */
TPT_API int tptGetPipelineInfo(int* outHwQueues, int* outOverlapEffective, int* outStreamDepth, int* outSlotReservations);
TPT_API const char* tptGetLastError(void);
/* The reference's six functions (include/tpt_test_api.h == Test.h:10-17) return void: when one of them fails -- no GPU, a HIP error, DrawTest
 * before UpdateTest -- the library by default prints the message and abort()s (there is no CPU path to fall back to; a frame that silently
 * was not rendered is worse than a stop).  A host that wants to decide itself installs a handler: it is called on the calling thread with
 * the entry point's name and the message, and the failed call then RETURNS without effect (DrawTest leaves the buffer alone and reports 0
 * rays).  NULL restores the default.  The tpt* functions never abort: they return a negative code. */
typedef void (*tptErrorHandler)(const char* where, const char* message);
TPT_API int tptSetErrorHandler(tptErrorHandler handler);
TPT_API const char* tptGetDeviceName(void);

#ifdef __cplusplus
}
#endif
#endif
