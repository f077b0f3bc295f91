/* tests/object_checker.c -- TEST INFRASTRUCTURE ONLY: the CPU statements of tptObjectPlaneDevice and tptTemporalAccumulateObjectsDevice
 * (include/tpt_hip.h), written from the specification alone (nothing of the product is included).  Compiled with oracle/Makefile's
 * CFLAGS (-ffp-contract=off, no fast math): binary32, in the order written, IEEE division and square root, sums from +0.
 *
 * The checker of oracle/tpt_oracle.c is included, not modified: the object plane's first hit is its tpto_hit_spheres (HitSpheres,
 * Maths.cpp:165-202) and the animated scene its tpto_animate (Test.cpp:304-308).
 *
 *   object_plane(nFrames, times or NULL, cameras [nFrames][22], w, h, spheres, count, flags, out [nFrames][h][w] int32)
 *   object_accumulate(temporal_checker.c's twenty arguments, object, prevObject or NULL, motion [nObjects][4] or NULL, nObjects)
 *
 * Both return 0, or -1 for arguments the product refuses (overlapping planes are the caller's business here). */
#include "../oracle/tpt_oracle.c"

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define OBJ_SNAP (1.0f / 128) /* include/tpt_hip.h: TPT_TEMPORAL_SNAP */

typedef struct { float x, y, z; } ov3;
static ov3 o_ld(const float* p) { ov3 r = {p[0], p[1], p[2]}; return r; }
static ov3 o_add(ov3 a, ov3 b) { ov3 r = {a.x + b.x, a.y + b.y, a.z + b.z}; return r; }
static ov3 o_sub(ov3 a, ov3 b) { ov3 r = {a.x - b.x, a.y - b.y, a.z - b.z}; return r; }
static ov3 o_scale(ov3 a, float s) { ov3 r = {a.x * s, a.y * s, a.z * s}; return r; }
static float o_dot(ov3 a, ov3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static int o_finite(float v) { return fabsf(v) <= FLT_MAX; } /* (false for NaN) */

/* the ray through the centre of pixel (x, y) and the lens centre: step 1 of both statements */
static ov3 centre_ray(const float* cam, int x, int y, int w, int h)
{
    const ov3 o = o_ld(cam), ll = o_ld(cam + 3), H = o_ld(cam + 6), V = o_ld(cam + 9);
    const float s = ((float)x + 0.5f) / (float)w, t = ((float)y + 0.5f) / (float)h;
    const ov3 v = o_sub(o_add(o_add(ll, o_scale(H, s)), o_scale(V, t)), o);
    return o_scale(v, 1.0f / sqrtf(o_dot(v, v)));
}

int object_plane(int nFrames, const float* times, const float* cameras, int w, int h, const TptoSphere* spheres, int count, unsigned flags,
                 int32_t* out)
{
    if (nFrames < 1 || nFrames > 4096 || w < 1 || w > 8192 || h < 1 || h > 8192 || !cameras || !spheres || count < 1 || !out) return -1;
    if (flags & ~(unsigned)(TPTO_FLAG_ANIMATE | TPTO_FLAG_PROGRESSIVE)) return -1;
    for (int j = 0; j < nFrames; ++j)
        for (int i = 0; i < 12; ++i)
            if (!o_finite(cameras[22 * (size_t)j + i])) return -1;
    TptoSphere* scene = (TptoSphere*)malloc(sizeof(TptoSphere) * (size_t)count);
    for (int j = 0; j < nFrames; ++j) {
        const float* cam = cameras + 22 * (size_t)j;
        memcpy(scene, spheres, sizeof(TptoSphere) * (size_t)count);
        if (times && (flags & TPTO_FLAG_ANIMATE) && count > 8) tpto_animate(scene, times[j]); /* (UpdateTest's guard, Test.cpp:304) */
        int32_t* plane = out + (size_t)j * (size_t)w * (size_t)h;
#pragma omp parallel for schedule(dynamic, 1) /* (pixels are independent: the same ids on any number of threads) */
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const ov3 dir = centre_ray(cam, x, y, w, h);
                const float d[3] = {dir.x, dir.y, dir.z};
                plane[(size_t)y * w + x] = tpto_hit_spheres(scene, count, cam, d, 0.001f, 1.0e7f, NULL, NULL, NULL);
            }
    }
    free(scene);
    return 0;
}

static int camera_ok(const float* c)
{
    for (int i = 0; i < 22; ++i)
        if (!o_finite(c[i])) return 0;
    const ov3 H = o_ld(c + 6), V = o_ld(c + 9);
    const float f = -o_dot(o_sub(o_ld(c + 3), o_ld(c)), o_ld(c + 18));
    return o_dot(H, H) != 0.0f && o_dot(V, V) != 0.0f && f > 0.0f;
}
static int tolerance_ok(float t) { return t >= 0.0f && t <= FLT_MAX; }

int object_accumulate(int w, int h, const float* cam, const float* prevCam, const float* colour, const float* albedo, const float* nd,
                      const float* moments, const float* prevColour, const float* prevAlbedo, const float* prevNd,
                      const float* prevMoments, float* outColour, float* outAlbedo, float* outMoments, float* outVariance,
                      float maxHistory, float depthTolerance, float normalTolerance, float coverageTolerance, const int32_t* object,
                      const int32_t* prevObject, const float* motion, int nObjects)
{
    if (w < 1 || w > 8192 || h < 1 || h > 8192 || !cam || !colour || !albedo || !nd || !moments) return -1;
    if (!outColour || !outAlbedo || !outMoments || !outVariance) return -1;
    const int nPrev = (prevCam != NULL) + (prevColour != NULL) + (prevAlbedo != NULL) + (prevNd != NULL) + (prevMoments != NULL);
    if (nPrev != 0 && nPrev != 5) return -1;
    if (!(maxHistory >= 1.0f && maxHistory <= 65536.0f)) return -1;
    if (!tolerance_ok(depthTolerance) || !tolerance_ok(normalTolerance) || !tolerance_ok(coverageTolerance)) return -1;
    if (!camera_ok(cam) || (prevCam && !camera_ok(prevCam))) return -1;
    if (!object || (prevObject != NULL) != (prevCam != NULL)) return -1;
    if (nObjects < 0 || nObjects > 65534 || (motion != NULL) != (nObjects > 0)) return -1;
    const ov3 o = o_ld(cam);
    ov3 po = o, pw = o, pH = o, pV = o, a = o;
    float f = 0.0f, hh = 0.0f, vv = 0.0f;
    if (prevCam) {
        po = o_ld(prevCam);
        pH = o_ld(prevCam + 6);
        pV = o_ld(prevCam + 9);
        pw = o_ld(prevCam + 18);
        a = o_sub(o_ld(prevCam + 3), po);
        f = -o_dot(a, pw);
        hh = o_dot(pH, pH);
        vv = o_dot(pV, pV);
    }
#pragma omp parallel for schedule(static) /* (pixels are independent: the same bits on any number of threads) */
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t p1 = (size_t)y * w + x, p = 4 * p1;
            /* cur, then out: colour rgb, albedo xyzw, moments xy */
            float cur[9] = {colour[p], colour[p + 1], colour[p + 2], albedo[p], albedo[p + 1], albedo[p + 2], albedo[p + 3],
                            moments[p], moments[p + 1]};
            float N = 1.0f;
            float B = 0.0f, hist[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, histN = 0.0f;
            float cap = 0.0f; /* m.w where an entry was read */
            if (prevCam) {
                const float c = albedo[p + 3];
                const int32_t id = object[p1];
                /* 1. the surface of p, moved to where it stood in the previous frame */
                const ov3 dir = centre_ray(cam, x, y, w, h);
                ov3 rel = dir, n = {0.0f, 0.0f, 0.0f};
                if (c > 0.0f) {
                    const float d = nd[p + 3] / c;
                    n.x = nd[p] / c;
                    n.y = nd[p + 1] / c;
                    n.z = nd[p + 2] / c;
                    if (motion && id >= 0 && id < nObjects) {
                        const float* m = motion + 4 * (size_t)id;
                        cap = m[3];
                        rel = o_sub(o_add(o_add(o, o_scale(dir, d)), o_ld(m)), po);
                    } else {
                        rel = o_sub(o_add(o, o_scale(dir, d)), po);
                    }
                }
                /* 2. into the previous camera */
                const float z = -o_dot(rel, pw);
                if (z > 0.0f) {
                    const float k = f / z;
                    const ov3 q = o_sub(o_scale(rel, k), a);
                    const float px = o_dot(q, pH) / hh * (float)w - 0.5f;
                    const float py = o_dot(q, pV) / vv * (float)h - 0.5f;
                    if (o_finite(px) && o_finite(py)) {
                        /* 3. snap */
                        float ix = floorf(px), iy = floorf(py);
                        float fx = px - ix, fy = py - iy;
                        if (fx < OBJ_SNAP) fx = 0.0f;
                        else if (fx > 1.0f - OBJ_SNAP) { ix = ix + 1.0f; fx = 0.0f; }
                        if (fy < OBJ_SNAP) fy = 0.0f;
                        else if (fy > 1.0f - OBJ_SNAP) { iy = iy + 1.0f; fy = 0.0f; }
                        const float e = sqrtf(o_dot(rel, rel));
                        /* 4. the taps */
                        for (int j = 0; j < 2; ++j)
                            for (int i = 0; i < 2; ++i) {
                                const float b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                                const float qx = ix + (float)i, qy = iy + (float)j;
                                if (!(b > 0.0f)) continue;
                                if (!(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1))) continue;
                                const size_t t1 = (size_t)qy * w + (size_t)qx, t4 = 4 * t1;
                                if (prevObject[t1] != id) continue;
                                const float N1 = prevMoments[t4 + 3];
                                if (!(N1 >= 1.0f && N1 <= FLT_MAX)) continue;
                                if (!o_finite(prevColour[t4]) || !o_finite(prevColour[t4 + 1]) || !o_finite(prevColour[t4 + 2])) continue;
                                const float c1 = prevAlbedo[t4 + 3];
                                if (!(fabsf(c - c1) <= coverageTolerance)) continue;
                                if (c > 0.0f && c1 > 0.0f) {
                                    const float d1 = prevNd[t4 + 3] / c1;
                                    if (!(fabsf(e - d1) <= depthTolerance * e)) continue;
                                    const float dx = n.x - prevNd[t4] / c1, dy = n.y - prevNd[t4 + 1] / c1, dz = n.z - prevNd[t4 + 2] / c1;
                                    if (!((dx * dx + dy * dy) + dz * dz <= normalTolerance)) continue;
                                } else if (!(c == 0.0f && c1 == 0.0f)) {
                                    continue;
                                }
                                B += b;
                                for (int m = 0; m < 3; ++m) hist[m] += b * prevColour[t4 + m];
                                for (int m = 0; m < 4; ++m) hist[3 + m] += b * prevAlbedo[t4 + m];
                                for (int m = 0; m < 2; ++m) hist[7 + m] += b * prevMoments[t4 + m];
                                histN += b * N1;
                            }
                    }
                }
            }
            /* 5. the history, capped by the object's entry */
            if (B > 0.0f) {
                N = histN / B + 1.0f;
                if (N > maxHistory) N = maxHistory;
                if (cap >= 1.0f && cap < N) N = cap;
                const float lerp = (N - 1.0f) / N;
                for (int m = 0; m < 9; ++m) cur[m] = (hist[m] / B) * lerp + cur[m] * (1.0f - lerp);
            }
            /* 6. the outputs */
            outColour[p] = cur[0];
            outColour[p + 1] = cur[1];
            outColour[p + 2] = cur[2];
            outColour[p + 3] = colour[p + 3];
            for (int m = 0; m < 4; ++m) outAlbedo[p + m] = cur[3 + m];
            outMoments[p] = cur[7];
            outMoments[p + 1] = cur[8];
            outMoments[p + 2] = 0.0f;
            outMoments[p + 3] = N;
            const float dd = cur[8] - cur[7] * cur[7];
            outVariance[p] = 0.0f;
            outVariance[p + 1] = (dd > 0.0f ? dd : 0.0f) / N;
            outVariance[p + 2] = 0.0f;
            outVariance[p + 3] = N;
        }
    return 0;
}
