/* tests/flow_checker.c -- TEST INFRASTRUCTURE ONLY: the CPU statement of tptMotionVectorsDevice (include/tpt_hip.h), written from the
 * specification alone (nothing of the product is included).  Compiled with oracle/Makefile's CFLAGS (-ffp-contract=off, no fast math):
 * binary32, in the order written, IEEE division and square root, sums from +0.
 *
 *   flow_motion(w, h, nFrames, cameras [nFrames][22], albedo, nd [nFrames][h][w][4], objects [nFrames][h][w] int32 or NULL,
 *               motion [nFrames][nObjects][4] or NULL, nObjects, prevCamera [22] or NULL, prevAlbedo, prevNd [h][w][4] or NULL,
 *               prevObject [h][w] or NULL, depthTolerance, normalTolerance, coverageTolerance, out [nFrames][h][w][4])
 *
 * Returns 0, or -1 for arguments the product refuses (overlapping planes are the caller's business here). */
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define FLOW_SNAP (1.0f / 128) /* include/tpt_hip.h: TPT_TEMPORAL_SNAP */

typedef struct { float x, y, z; } fv3;
static fv3 f_ld(const float* p) { fv3 r = {p[0], p[1], p[2]}; return r; }
static fv3 f_add(fv3 a, fv3 b) { fv3 r = {a.x + b.x, a.y + b.y, a.z + b.z}; return r; }
static fv3 f_sub(fv3 a, fv3 b) { fv3 r = {a.x - b.x, a.y - b.y, a.z - b.z}; return r; }
static fv3 f_scale(fv3 a, float s) { fv3 r = {a.x * s, a.y * s, a.z * s}; return r; }
static float f_dot(fv3 a, fv3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static int f_finite(float v) { return fabsf(v) <= FLT_MAX; } /* (false for NaN) */

static int camera_ok(const float* c)
{
    for (int i = 0; i < 22; ++i)
        if (!f_finite(c[i])) return 0;
    const fv3 H = f_ld(c + 6), V = f_ld(c + 9);
    const float f = -f_dot(f_sub(f_ld(c + 3), f_ld(c)), f_ld(c + 18));
    return f_dot(H, H) != 0.0f && f_dot(V, V) != 0.0f && f > 0.0f;
}
static int tolerance_ok(float t) { return t >= 0.0f && t <= FLT_MAX; }

/* one frame: cam and its planes against the predecessor's; motion: this frame's table or NULL */
static void flow_frame(int w, int h, const float* cam, const float* albedo, const float* nd, const int32_t* object, const float* motion,
                       int nObjects, const float* prevCam, const float* prevAlbedo, const float* prevNd, const int32_t* prevObject,
                       float depthTolerance, float normalTolerance, float coverageTolerance, float* out)
{
    const fv3 o = f_ld(cam), ll = f_ld(cam + 3), H = f_ld(cam + 6), V = f_ld(cam + 9);
    const fv3 po = f_ld(prevCam), pH = f_ld(prevCam + 6), pV = f_ld(prevCam + 9), pw = f_ld(prevCam + 18);
    /* once per frame */
    const fv3 a = f_sub(f_ld(prevCam + 3), po);
    const float f = -f_dot(a, pw);
    const float hh = f_dot(pH, pH);
    const float vv = f_dot(pV, pV);
#pragma omp parallel for schedule(static) /* (pixels are independent: the same bits on any number of threads) */
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t p1 = (size_t)y * w + x, p = 4 * p1;
            float* r = out + p;
            r[0] = r[1] = r[2] = r[3] = 0.0f;
            const float c = albedo[p + 3];
            const int32_t id = object ? object[p1] : 0;
            /* 1. the point in this frame */
            const float s = ((float)x + 0.5f) / (float)w, t = ((float)y + 0.5f) / (float)h;
            const fv3 v = f_sub(f_add(f_add(ll, f_scale(H, s)), f_scale(V, t)), o);
            const fv3 dir = f_scale(v, 1.0f / sqrtf(f_dot(v, v)));
            fv3 rel = dir, n = {0.0f, 0.0f, 0.0f};
            if (c > 0.0f) {
                const float d = nd[p + 3] / c;
                n.x = nd[p] / c;
                n.y = nd[p + 1] / c;
                n.z = nd[p + 2] / c;
                fv3 at = f_add(o, f_scale(dir, d));
                if (object && motion && id >= 0 && id < nObjects) at = f_add(at, f_ld(motion + 4 * (size_t)id));
                rel = f_sub(at, po);
            }
            /* 2. into the predecessor */
            const float z = -f_dot(rel, pw);
            const float k = f / z;
            const fv3 q = f_sub(f_scale(rel, k), a);
            const float px = f_dot(q, pH) / hh * (float)w - 0.5f;
            const float py = f_dot(q, pV) / vv * (float)h - 0.5f;
            if (!(z > 0.0f && f_finite(px) && f_finite(py))) continue;
            /* 3. snap and motion */
            float fx0 = floorf(px), fy0 = floorf(py);
            float fx = px - fx0, fy = py - fy0;
            if (fx < FLOW_SNAP) fx = 0.0f;
            else if (fx > 1.0f - FLOW_SNAP) { fx0 = fx0 + 1.0f; fx = 0.0f; }
            if (fy < FLOW_SNAP) fy = 0.0f;
            else if (fy > 1.0f - FLOW_SNAP) { fy0 = fy0 + 1.0f; fy = 0.0f; }
            const float e = sqrtf(f_dot(rel, rel));
            /* 4. the taps */
            float W = 0.0f;
            if (px >= -1.0f && px < (float)w && py >= -1.0f && py < (float)h) {
                const int ix = (int)fx0, iy = (int)fy0;
                for (int j = 0; j < 2; ++j)
                    for (int i = 0; i < 2; ++i) {
                        const float b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                        const int qx = ix + i, qy = iy + j;
                        if (!(b > 0.0f)) continue;
                        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                        const size_t t1 = (size_t)qy * w + (size_t)qx, t4 = 4 * t1;
                        if (object && prevObject[t1] != id) continue;
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
                        W += b;
                    }
            }
            /* 5. the output */
            r[0] = (fx0 + fx) - (float)x;
            r[1] = (fy0 + fy) - (float)y;
            r[2] = e;
            r[3] = W;
        }
}

int flow_motion(int w, int h, int nFrames, const float* cameras, const float* albedo, const float* nd, const int32_t* objects,
                const float* motion, int nObjects, const float* prevCam, const float* prevAlbedo, const float* prevNd,
                const int32_t* prevObject, float depthTolerance, float normalTolerance, float coverageTolerance, float* out)
{
    if (nFrames < 1 || nFrames > 4096 || w < 1 || w > 8192 || h < 1 || h > 8192) return -1;
    if (!cameras || !albedo || !nd || !out) return -1;
    if (prevCam) {
        if (!prevAlbedo || !prevNd || (prevObject != NULL) != (objects != NULL)) return -1;
    } else if (prevAlbedo || prevNd || prevObject) {
        return -1;
    }
    if (motion && !objects) return -1;
    if (nObjects < 0 || nObjects > 65534 || (motion != NULL) != (nObjects > 0)) return -1;
    if (!tolerance_ok(depthTolerance) || !tolerance_ok(normalTolerance) || !tolerance_ok(coverageTolerance)) return -1;
    for (int j = 0; j < nFrames; ++j)
        if (!camera_ok(cameras + 22 * (size_t)j)) return -1;
    if (prevCam && !camera_ok(prevCam)) return -1;
    const size_t pixels = (size_t)w * (size_t)h;
    for (int j = 0; j < nFrames; ++j) {
        float* o = out + 4 * pixels * (size_t)j;
        if (j == 0 && !prevCam) { /* no predecessor */
            for (size_t i = 0; i < 4 * pixels; ++i) o[i] = 0.0f;
            continue;
        }
        const size_t at = 4 * pixels * (size_t)j, ids = pixels * (size_t)j;
        flow_frame(w, h, cameras + 22 * (size_t)j, albedo + at, nd + at, objects ? objects + ids : NULL,
                   motion ? motion + 4 * (size_t)nObjects * (size_t)j : NULL, nObjects, j ? cameras + 22 * (size_t)(j - 1) : prevCam,
                   j ? albedo + at - 4 * pixels : prevAlbedo, j ? nd + at - 4 * pixels : prevNd,
                   objects ? (j ? objects + ids - pixels : prevObject) : NULL, depthTolerance, normalTolerance, coverageTolerance, o);
    }
    return 0;
}
