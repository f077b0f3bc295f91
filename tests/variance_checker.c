/* tests/variance_checker.c -- TEST INFRASTRUCTURE ONLY: the CPU statement of tptDenoiseDeviceVariance's variance-guided a-trous filter
 * (include/tpt_hip.h), written from the specification alone (it includes nothing of the product).  Compiled with oracle/Makefile's
 * CFLAGS (-ffp-contract=off, no fast math): binary32, in the order written, IEEE division, sums from +0.
 *
 *   denoise_variance(w, h, colour, albedo or NULL, normalDepth or NULL, moments, samples, out, iterations, sigmaLuminance, sigmaNormal,
 *                    sigmaDepth, flags)
 *
 * Every plane is [h][w][4] floats.  Returns 0, or -1 for arguments the product refuses. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define DENOISE_DEMODULATE 1u
#define VARIANCE_EPS 1e-4f /* include/tpt_hip.h: TPT_DENOISE_VARIANCE_EPS */

static const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
static const float gk[3] = {0.25f, 0.5f, 0.25f};

static int sigma_ok(float s) { return s == 0.0f || (s >= 1e-6f && s <= 1e6f); }
static float inv2(float s) { return s > 0.0f ? 1.0f / (s * s) : 0.0f; }
static float lum(const float* c) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }

int denoise_variance(int w, int h, const float* colour, const float* albedo, const float* nd, const float* moments, float samples,
                     float* out, int iterations, float sigmaLuminance, float sigmaNormal, float sigmaDepth, unsigned flags)
{
    if (w < 1 || w > 8192 || h < 1 || h > 8192 || !colour || !out || !moments || iterations < 1 || iterations > 8) return -1;
    if (!(samples >= 1.0f && samples <= 3.40282347e38f)) return -1;
    if (!(sigmaLuminance > 0.0f && sigmaLuminance <= 1e6f)) return -1;
    if (!sigma_ok(sigmaNormal) || !sigma_ok(sigmaDepth)) return -1;
    if ((sigmaNormal != 0.0f || sigmaDepth != 0.0f) && !nd) return -1;
    if ((flags & ~DENOISE_DEMODULATE) || ((flags & DENOISE_DEMODULATE) && !albedo)) return -1;
    const int demod = (flags & DENOISE_DEMODULATE) != 0;
    const size_t n = (size_t)w * h;
    float* cur = malloc(n * 4 * sizeof(float)); /* {colour, v} */
    float* nxt = malloc(n * 4 * sizeof(float));
    if (!cur || !nxt) {
        free(cur);
        free(nxt);
        return -1;
    }
    for (size_t p = 0; p < n; ++p) {
        for (int c = 0; c < 3; ++c) {
            const float v = colour[4 * p + c];
            const float a = albedo ? albedo[4 * p + c] : 0.0f;
            cur[4 * p + c] = demod && a > 0.0f ? v / a : v;
        }
        const float* m = moments + 4 * p;
        const float d = m[1] - m[0] * m[0];
        float v = (d > 0.0f ? d : 0.0f) / samples;
        if (demod) {
            const float la = lum(albedo + 4 * p);
            const float la2 = la * la;
            if (la2 > 0.0f) v = v / la2;
        }
        cur[4 * p + 3] = v;
    }
    const float sl2 = sigmaLuminance * sigmaLuminance, in = inv2(sigmaNormal), id = inv2(sigmaDepth);
    for (int i = 0; i < iterations; ++i) {
        const int s = 1 << i;
#pragma omp parallel for schedule(static) /* (pixels are independent: the same bits on any number of threads) */
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const float* cp = cur + 4 * ((size_t)y * w + x);
                const float* np = nd ? nd + 4 * ((size_t)y * w + x) : NULL;
                float gv = 0.0f, gw = 0.0f;
                for (int jy = 0; jy < 3; ++jy)
                    for (int jx = 0; jx < 3; ++jx) {
                        const int qx = x + jx - 1, qy = y + jy - 1;
                        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                        const float k = gk[jy] * gk[jx];
                        gv += k * cur[4 * ((size_t)qy * w + qx) + 3];
                        gw += k;
                    }
                const float g = gv / gw;
                const float il = (float)s / (sl2 * g + VARIANCE_EPS);
                const float lp = lum(cp);
                float sumW = 0.0f, sumR = 0.0f, sumG = 0.0f, sumB = 0.0f, sumV = 0.0f;
                for (int ky = 0; ky < 5; ++ky)
                    for (int kx = 0; kx < 5; ++kx) {
                        const int qx = x + (kx - 2) * s, qy = y + (ky - 2) * s;
                        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                        const float* cq = cur + 4 * ((size_t)qy * w + qx);
                        const float dl = lum(cq) - lp;
                        float den = 1.0f + (dl * dl) * il;
                        if (nd) {
                            const float* nq = nd + 4 * ((size_t)qy * w + qx);
                            const float dnx = nq[0] - np[0], dny = nq[1] - np[1], dnz = nq[2] - np[2];
                            const float dn = (dnx * dnx + dny * dny) + dnz * dnz;
                            den = den * (1.0f + dn * in);
                            const float dd = nq[3] - np[3];
                            den = den * (1.0f + (dd * dd) * id);
                        }
                        const float wt = (hk[ky] * hk[kx]) / den;
                        sumW += wt;
                        sumR += wt * cq[0];
                        sumG += wt * cq[1];
                        sumB += wt * cq[2];
                        sumV += (wt * wt) * cq[3];
                    }
                float* o = nxt + 4 * ((size_t)y * w + x);
                o[0] = sumR / sumW;
                o[1] = sumG / sumW;
                o[2] = sumB / sumW;
                o[3] = sumV / (sumW * sumW);
            }
        float* t = cur;
        cur = nxt;
        nxt = t;
    }
    for (size_t p = 0; p < n; ++p) {
        for (int c = 0; c < 3; ++c) {
            const float f = cur[4 * p + c];
            const float a = albedo ? albedo[4 * p + c] : 0.0f;
            out[4 * p + c] = demod && a > 0.0f ? f * a : f;
        }
        out[4 * p + 3] = colour[4 * p + 3];
    }
    free(cur);
    free(nxt);
    return 0;
}
