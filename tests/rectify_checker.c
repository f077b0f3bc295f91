/* tests/rectify_checker.c -- TEST INFRASTRUCTURE ONLY: the CPU statement of tptRectifyHistoryDevice (include/tpt_hip.h), written from
 * the specification alone (it includes nothing of the product).  Compiled with oracle/Makefile's CFLAGS (-ffp-contract=off, no fast
 * math): binary32, in the order written, IEEE division and square root, sums from +0.
 *
 *   rectify_history(w, h, colour, moments, accColour, accMoments, outColour, outMoments, outVariance, radius, gamma)
 *
 * Every plane is [h][w][4] floats.  An output may be the accumulated plane of its kind (a pixel reads no accumulated value but its
 * own, and reads it before it writes).  Returns 0, or -1 for arguments the product refuses (overlapping planes are the caller's
 * business here). */
#include <float.h>
#include <math.h>
#include <stddef.h>

static int finite32(float v) { return fabsf(v) <= FLT_MAX; } /* (false for NaN) */

static void variance_of(float mx, float my, float N, float* out)
{
    const float dd = my - mx * mx;
    out[0] = 0.0f;
    out[1] = (dd > 0.0f ? dd : 0.0f) / N;
    out[2] = 0.0f;
    out[3] = N;
}

int rectify_history(int w, int h, const float* colour, const float* moments, const float* accColour, const float* accMoments,
                    float* outColour, float* outMoments, float* outVariance, int radius, float gamma)
{
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return -1;
    if (!colour || !moments || !accColour || !accMoments || !outColour || !outMoments || !outVariance) return -1;
    if (radius < 1 || radius > 3 || !(gamma >= 0.0f && gamma <= FLT_MAX)) return -1;
#pragma omp parallel for schedule(static) /* (pixels are independent: the same bits on any number of threads) */
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t p = 4 * ((size_t)y * w + x);
            const float cur[3] = {colour[p], colour[p + 1], colour[p + 2]};
            const float acc[4] = {accColour[p], accColour[p + 1], accColour[p + 2], accColour[p + 3]};
            const float M[4] = {accMoments[p], accMoments[p + 1], accMoments[p + 2], accMoments[p + 3]};
            const float N = M[3];
            int through = !(finite32(N) && N > 1.0f);
            for (int c = 0; c < 3; ++c)
                if (!finite32(cur[c]) || !finite32(acc[c])) through = 1;
            float out[3] = {acc[0], acc[1], acc[2]}, a = 0.0f;
            if (!through) {
                /* 1. the window */
                float n = 0.0f, S1[3] = {0.0f, 0.0f, 0.0f}, S2[3] = {0.0f, 0.0f, 0.0f};
                for (int j = -radius; j <= radius; ++j) {
                    float nj = 0.0f, s[3] = {0.0f, 0.0f, 0.0f}, t[3] = {0.0f, 0.0f, 0.0f};
                    for (int i = -radius; i <= radius; ++i) {
                        const int qx = x + i, qy = y + j;
                        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                        const float* q = colour + 4 * ((size_t)qy * w + qx);
                        if (!finite32(q[0]) || !finite32(q[1]) || !finite32(q[2])) continue;
                        nj += 1.0f;
                        for (int c = 0; c < 3; ++c) {
                            s[c] += q[c];
                            t[c] += q[c] * q[c];
                        }
                    }
                    n += nj;
                    for (int c = 0; c < 3; ++c) {
                        S1[c] += s[c];
                        S2[c] += t[c];
                    }
                }
                /* 2. the bounds and the clamp; 3. the pull */
                const float lerp = (N - 1.0f) / N, one = 1.0f - lerp;
                for (int c = 0; c < 3; ++c) {
                    const float mean = S1[c] / n;
                    float var = S2[c] / n - mean * mean;
                    if (var < 0.0f) var = 0.0f;
                    const float g = gamma * sqrtf(var);
                    float lo = mean - g, hi = mean + g;
                    if (!(lo < cur[c])) lo = cur[c];
                    if (!(hi > cur[c])) hi = cur[c];
                    const float L = lo * lerp + cur[c] * one, U = hi * lerp + cur[c] * one;
                    if (out[c] < L) out[c] = L;
                    if (out[c] > U) out[c] = U;
                    float ac = 0.0f;
                    if (!(out[c] == acc[c])) {
                        const float q = (acc[c] - out[c]) / (acc[c] - cur[c]);
                        ac = !finite32(q) ? 1.0f : q < 0.0f ? 0.0f : q > 1.0f ? 1.0f : q;
                    }
                    if (ac > a) a = ac;
                }
            }
            if (through || a == 0.0f) {
                for (int c = 0; c < 4; ++c) {
                    outColour[p + c] = acc[c];
                    outMoments[p + c] = M[c];
                }
                variance_of(M[0], M[1], N, outVariance + p);
            } else {
                /* 4. the shortened history */
                const float k = 1.0f - a, N1 = 1.0f + (N - 1.0f) * k;
                const float mx = M[0] * k + moments[p] * a, my = M[1] * k + moments[p + 1] * a;
                outColour[p] = out[0];
                outColour[p + 1] = out[1];
                outColour[p + 2] = out[2];
                outColour[p + 3] = acc[3];
                outMoments[p] = mx;
                outMoments[p + 1] = my;
                outMoments[p + 2] = 0.0f;
                outMoments[p + 3] = N1;
                variance_of(mx, my, N1, outVariance + p);
            }
        }
    return 0;
}
