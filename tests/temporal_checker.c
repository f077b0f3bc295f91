/* tests/temporal_checker.c -- TEST INFRASTRUCTURE ONLY: the CPU statement of tptTemporalAccumulateDevice (include/tpt_hip.h), written
 * from the specification alone (it includes nothing of the product).  Compiled with oracle/Makefile's CFLAGS (-ffp-contract=off, no
 * fast math): binary32, in the order written, IEEE division and square root, sums from +0.
 *
 *   temporal_accumulate(w, h, camera, prevCamera or NULL, colour, albedo, normalDepth, moments, prevColour, prevAlbedo, prevNormalDepth,
 *                       prevMoments (all four NULL with prevCamera), outColour, outAlbedo, outMoments, outVariance, maxHistory,
 *                       depthTolerance, normalTolerance, coverageTolerance)
 *
 * A camera is the reference's 22 floats {origin, lowerLeftCorner, horizontal, vertical, uu, vv, ww, lensRadius}; every plane is
 * [h][w][4] floats.  Returns 0, or -1 for arguments the product refuses (overlapping planes are the caller's business here). */
#include <float.h>
#include <math.h>
#include <stddef.h>

#define TEMPORAL_SNAP (1.0f / 128) /* include/tpt_hip.h: TPT_TEMPORAL_SNAP */

typedef struct { float x, y, z; } v3;
static v3 ld(const float* p) { v3 r = {p[0], p[1], p[2]}; return r; }
static v3 add(v3 a, v3 b) { v3 r = {a.x + b.x, a.y + b.y, a.z + b.z}; return r; }
static v3 sub(v3 a, v3 b) { v3 r = {a.x - b.x, a.y - b.y, a.z - b.z}; return r; }
static v3 scale(v3 a, float s) { v3 r = {a.x * s, a.y * s, a.z * s}; return r; }
static float dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static int finite32(float v) { return fabsf(v) <= FLT_MAX; } /* (false for NaN) */

static int camera_ok(const float* c)
{
    for (int i = 0; i < 22; ++i)
        if (!finite32(c[i])) return 0;
    const v3 H = ld(c + 6), V = ld(c + 9);
    const float f = -dot(sub(ld(c + 3), ld(c)), ld(c + 18));
    return dot(H, H) != 0.0f && dot(V, V) != 0.0f && f > 0.0f;
}
static int tolerance_ok(float t) { return t >= 0.0f && t <= FLT_MAX; }

int temporal_accumulate(int w, int h, const float* cam, const float* prevCam, const float* colour, const float* albedo, const float* nd,
                        const float* moments, const float* prevColour, const float* prevAlbedo, const float* prevNd,
                        const float* prevMoments, float* outColour, float* outAlbedo, float* outMoments, float* outVariance,
                        float maxHistory, float depthTolerance, float normalTolerance, float coverageTolerance)
{
    if (w < 1 || w > 8192 || h < 1 || h > 8192 || !cam || !colour || !albedo || !nd || !moments) return -1;
    if (!outColour || !outAlbedo || !outMoments || !outVariance) return -1;
    const int nPrev = (prevCam != NULL) + (prevColour != NULL) + (prevAlbedo != NULL) + (prevNd != NULL) + (prevMoments != NULL);
    if (nPrev != 0 && nPrev != 5) return -1;
    if (!(maxHistory >= 1.0f && maxHistory <= 65536.0f)) return -1;
    if (!tolerance_ok(depthTolerance) || !tolerance_ok(normalTolerance) || !tolerance_ok(coverageTolerance)) return -1;
    if (!camera_ok(cam) || (prevCam && !camera_ok(prevCam))) return -1;
    const v3 o = ld(cam), ll = ld(cam + 3), H = ld(cam + 6), V = ld(cam + 9);
    v3 po = o, pw = o, pH = o, pV = o, a = o;
    float f = 0.0f, hh = 0.0f, vv = 0.0f;
    if (prevCam) {
        po = ld(prevCam);
        pH = ld(prevCam + 6);
        pV = ld(prevCam + 9);
        pw = ld(prevCam + 18);
        a = sub(ld(prevCam + 3), po);
        f = -dot(a, pw);
        hh = dot(pH, pH);
        vv = dot(pV, pV);
    }
#pragma omp parallel for schedule(static) /* (pixels are independent: the same bits on any number of threads) */
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t p = 4 * ((size_t)y * w + x);
            /* cur, then out: colour rgb, albedo xyzw, moments xy */
            float cur[9] = {colour[p], colour[p + 1], colour[p + 2], albedo[p], albedo[p + 1], albedo[p + 2], albedo[p + 3],
                            moments[p], moments[p + 1]};
            float N = 1.0f;
            float B = 0.0f, hist[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, histN = 0.0f;
            if (prevCam) {
                const float c = albedo[p + 3];
                /* 1. the surface of p */
                const float s = ((float)x + 0.5f) / (float)w, t = ((float)y + 0.5f) / (float)h;
                const v3 v = sub(add(add(ll, scale(H, s)), scale(V, t)), o);
                const v3 dir = scale(v, 1.0f / sqrtf(dot(v, v)));
                v3 rel = dir, n = {0.0f, 0.0f, 0.0f};
                if (c > 0.0f) {
                    const float d = nd[p + 3] / c;
                    n.x = nd[p] / c;
                    n.y = nd[p + 1] / c;
                    n.z = nd[p + 2] / c;
                    rel = sub(add(o, scale(dir, d)), po);
                }
                /* 2. into the previous camera */
                const float z = -dot(rel, pw);
                if (z > 0.0f) {
                    const float k = f / z;
                    const v3 q = sub(scale(rel, k), a);
                    const float px = dot(q, pH) / hh * (float)w - 0.5f;
                    const float py = dot(q, pV) / vv * (float)h - 0.5f;
                    if (finite32(px) && finite32(py)) {
                        /* 3. snap (floor and the tap coordinates kept as floats: they are integers of any size) */
                        float ix = floorf(px), iy = floorf(py);
                        float fx = px - ix, fy = py - iy;
                        if (fx < TEMPORAL_SNAP) fx = 0.0f;
                        else if (fx > 1.0f - TEMPORAL_SNAP) { ix = ix + 1.0f; fx = 0.0f; }
                        if (fy < TEMPORAL_SNAP) fy = 0.0f;
                        else if (fy > 1.0f - TEMPORAL_SNAP) { iy = iy + 1.0f; fy = 0.0f; }
                        const float e = sqrtf(dot(rel, rel));
                        /* 4. the taps */
                        for (int j = 0; j < 2; ++j)
                            for (int i = 0; i < 2; ++i) {
                                const float b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                                const float qx = ix + (float)i, qy = iy + (float)j;
                                if (!(b > 0.0f)) continue;
                                if (!(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1))) continue;
                                const size_t t4 = 4 * ((size_t)qy * w + (size_t)qx);
                                const float N1 = prevMoments[t4 + 3];
                                if (!(N1 >= 1.0f && N1 <= FLT_MAX)) continue;
                                if (!finite32(prevColour[t4]) || !finite32(prevColour[t4 + 1]) || !finite32(prevColour[t4 + 2])) continue;
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
            /* 5. the history */
            if (B > 0.0f) {
                N = histN / B + 1.0f;
                if (N > maxHistory) N = maxHistory;
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
