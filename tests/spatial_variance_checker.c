/* tests/spatial_variance_checker.c -- TEST INFRASTRUCTURE ONLY: the CPU statement of tptSpatialVarianceDevice (include/tpt_hip.h),
 * written from the specification alone (it includes nothing of the product).  Compiled with oracle/Makefile's CFLAGS
 * (-ffp-contract=off, no fast math): binary32, in the order written, IEEE division, sums from +0.
 *
 *   spatial_variance(w, h, frames, moments, normalDepth, out, samplesPerFrame, minSamples, radius, sigmaNormal, sigmaDepth)
 *
 * Every plane is [frames][h][w][4] floats; normalDepth may be NULL.  Returns 0, or -1 for arguments the product refuses (overlapping
 * planes are the caller's business here). */
#include <float.h>
#include <math.h>
#include <stddef.h>

static int finite32(float v) { return fabsf(v) <= FLT_MAX; } /* (false for NaN) */
static int sigma_ok(float s) { return s == 0.0f || (s >= 1e-6f && s <= 1e6f); }
static float inv2(float s) { return s > 0.0f ? 1.0f / (s * s) : 0.0f; }

int spatial_variance(int w, int h, int frames, const float* moments, const float* normalDepth, float* out, float samplesPerFrame,
                     float minSamples, int radius, float sigmaNormal, float sigmaDepth)
{
    if (w < 1 || w > 8192 || h < 1 || h > 8192 || frames < 1 || frames > 4096) return -1;
    if (!moments || !out || radius < 1 || radius > 3) return -1;
    if (!(samplesPerFrame >= 1.0f && samplesPerFrame <= FLT_MAX) || !(minSamples >= 1.0f)) return -1;
    if (!sigma_ok(sigmaNormal) || !sigma_ok(sigmaDepth)) return -1;
    if ((sigmaNormal != 0.0f || sigmaDepth != 0.0f) && !normalDepth) return -1;
    const float in = inv2(sigmaNormal), id = inv2(sigmaDepth);
    for (int f = 0; f < frames; ++f) {
        const size_t plane = (size_t)f * (size_t)w * (size_t)h * 4;
        const float* mo = moments + plane;
        const float* nd = normalDepth ? normalDepth + plane : NULL;
        float* o = out + plane;
#pragma omp parallel for schedule(static) /* (pixels are independent: the same bits on any number of threads) */
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t p = 4 * ((size_t)y * w + x);
                /* 0. the pixel's own variance, and whether that is all */
                float N = mo[p + 3];
                if (!(finite32(N) && N >= 1.0f)) N = 1.0f;
                const float dd = mo[p + 1] - mo[p] * mo[p];
                float v = dd > 0.0f ? dd : 0.0f;
                const float have = samplesPerFrame * N;
                if (have < minSamples) {
                    /* 1. the window */
                    float W = 0.0f, S1 = 0.0f, S2 = 0.0f;
                    int counted = 0;
                    for (int j = -radius; j <= radius; ++j)
                        for (int i = -radius; i <= radius; ++i) {
                            const int qx = x + i, qy = y + j;
                            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                            const size_t q = 4 * ((size_t)qy * w + qx);
                            if (!finite32(mo[q]) || !finite32(mo[q + 1])) continue;
                            float den = 1.0f;
                            if (nd) {
                                const float dx = nd[q] - nd[p], dy = nd[q + 1] - nd[p + 1], dz = nd[q + 2] - nd[p + 2];
                                den = 1.0f + ((dx * dx + dy * dy) + dz * dz) * in;
                                const float dw = nd[q + 3] - nd[p + 3];
                                den = den * (1.0f + (dw * dw) * id);
                            }
                            if (!finite32(den)) continue;
                            const float wt = 1.0f / den;
                            ++counted;
                            W += wt;
                            S1 += wt * mo[q];
                            S2 += wt * mo[q + 1];
                        }
                    /* 2. the estimate */
                    if (counted) {
                        const float e1 = S1 / W, e2 = S2 / W;
                        const float ds = e2 - e1 * e1;
                        v = ds > 0.0f ? ds : 0.0f;
                    }
                }
                o[p] = 0.0f;
                o[p + 1] = v / N;
                o[p + 2] = 0.0f;
                o[p + 3] = N;
            }
    }
    return 0;
}
