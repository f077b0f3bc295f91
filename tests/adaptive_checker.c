/* tests/adaptive_checker.c -- TEST INFRASTRUCTURE ONLY: the CPU reference of tptDrawDeviceAdaptive and tptAdaptiveSamplesDevice.
 *
 * MomentRows of tests/moments_checker.c (included, not modified) restated with a plane of sample counts: pixel p takes
 * n = counts[p] clamped to 0 .. 2047 samples from its own seed; n == 0 leaves every entry of the pixel alone and traces nothing; the
 * means are the sums x (1.0f / n); and the blend is weighted by samples as include/tpt_hip.h states it -- S = moments.w if progressive
 * and finite and >= 1, else 0; S' = S + n; lerp = S / S'; tile.rgb and moments.xyz blended, moments.w = S'.  adaptive_plan is the header's
 * statement of tptAdaptiveSamplesDevice, step by step.  Built with oracle/Makefile's CFLAGS (no FMA contraction).
 */
#include "moments_checker.c"

#define ADAPTIVE_LUM_FLOOR 1e-2f /* include/tpt_hip.h: TPT_ADAPTIVE_LUM_FLOOR */

static int adaptiveValid(float S) { return S >= 1.0f && S <= 3.40282347e38f; } /* finite and >= 1 (false for a NaN) */

static int64_t AdaptiveRows(const Scene* sc, const TptoParams* p, int start, int end, float* backbufferBase, float* albedoBase,
                            float* normalDepthBase, float* momentsBase, const int32_t* countsBase)
{
    float* backbuffer = backbufferBase + (size_t)start * p->width * 4;
    aov4* albedo = (aov4*)albedoBase + (size_t)start * p->width;
    aov4* normalDepth = (aov4*)normalDepthBase + (size_t)start * p->width;
    float* moments = momentsBase + (size_t)start * p->width * 4;
    const int32_t* counts = countsBase + (size_t)start * p->width;
    float invWidth = 1.0f / p->width;
    float invHeight = 1.0f / p->height;
    int64_t rayCount = 0;
    for (uint32_t y = (uint32_t)start; y < (uint32_t)end; ++y) {
        for (int x = 0; x < p->width; ++x, backbuffer += 4, moments += 4, albedo++, normalDepth++, counts++) {
            int n = *counts;
            n = n < 0 ? 0 : (n > 2047 ? 2047 : n);
            if (n == 0) continue; /* not traced: nothing of the pixel is written */
            uint32_t state = ((uint32_t)x * 1973u + y * 9277u + (uint32_t)p->frame * 26699u) | 1u; /* per-pixel seeds only */
            f3 col = mk(0, 0, 0);
            aov4 sa = {0.0f, 0.0f, 0.0f, 0.0f}, sn = {0.0f, 0.0f, 0.0f, 0.0f};
            float sl = 0.0f, sl2 = 0.0f;
            for (int s = 0; s < n; s++) {
                float u = ((float)x + RND(&state)) * invWidth;
                float v = ((float)y + RND(&state)) * invHeight;
                Ray r = CameraGetRay(sc->cam, u, v, &state);
                Hit h;
                const int id = HitSpheres(sc, &r, kMinT, kMaxT, &h);
                aov4 a = {0.0f, 0.0f, 0.0f, 0.0f}, nn = {0.0f, 0.0f, 0.0f, 0.0f};
                if (id != -1) {
                    a.x = sc->mats[id].albedo[0];
                    a.y = sc->mats[id].albedo[1];
                    a.z = sc->mats[id].albedo[2];
                    a.w = 1.0f;
                    nn.x = h.normal.x;
                    nn.y = h.normal.y;
                    nn.z = h.normal.z;
                    nn.w = h.t;
                }
                sa.x = sa.x + a.x; sa.y = sa.y + a.y; sa.z = sa.z + a.z; sa.w = sa.w + a.w;
                sn.x = sn.x + nn.x; sn.y = sn.y + nn.y; sn.z = sn.z + nn.z; sn.w = sn.w + nn.w;
                f3 c = Trace(sc, &r, 0, &rayCount, &state, 1);
                col = add(col, c);
                const float l = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
                sl = sl + l;
                sl2 = sl2 + l * l;
            }
            const float inv = 1.0f / (float)n;
            const float S = ((p->flags & TPTO_FLAG_PROGRESSIVE) && adaptiveValid(moments[3])) ? moments[3] : 0.0f;
            const float S1 = S + (float)n;
            const float lerpFac = S / S1;
            col = muls(col, inv);
            f3 prev = mk(backbuffer[0], backbuffer[1], backbuffer[2]);
            col = add(muls(prev, lerpFac), muls(col, 1 - lerpFac));
            backbuffer[0] = col.x;
            backbuffer[1] = col.y;
            backbuffer[2] = col.z;
            f3 m = mk(sl * inv, sl2 * inv, 0.0f * inv);
            f3 mprev = mk(moments[0], moments[1], moments[2]);
            m = add(muls(mprev, lerpFac), muls(m, 1 - lerpFac));
            moments[0] = m.x;
            moments[1] = m.y;
            moments[2] = m.z;
            moments[3] = S1;
            if (albedoBase) { albedo->x = sa.x * inv; albedo->y = sa.y * inv; albedo->z = sa.z * inv; albedo->w = sa.w * inv; }
            if (normalDepthBase) { normalDepth->x = sn.x * inv; normalDepth->y = sn.y * inv; normalDepth->z = sn.z * inv; normalDepth->w = sn.w * inv; }
        }
    }
    return rayCount;
}

/* moments_render with a count per pixel (per-pixel seeds, the recursive fold: what the product's entry point accepts); albedo and
 * normalDepth may be NULL */
int64_t adaptive_render(const TptoSphere* spheres, const TptoMaterial* mats, int count, const TptoCamera* cam, const TptoParams* p,
                        float* backbuffer, float* albedo, float* normalDepth, float* moments, const int32_t* counts)
{
    Scene* sc = (Scene*)calloc(1, sizeof(Scene));
    if (count < 0) count = 0;
    sc->emissive = (int*)malloc(sizeof(int) * (size_t)(count > 0 ? count : 1));
    sc->spheres = spheres;
    sc->mats = mats;
    sc->count = count;
    sc->cam = cam;
    sc->math_mode = p->math_mode;
    sc->fold_mode = p->fold_mode;
    sc->no_light_sampling = p->no_light_sampling;
    sc->mitsuba_compare = p->mitsuba_compare;
    float* soa = (float*)malloc(sizeof(float) * 5 * (size_t)(count > 0 ? count : 1));
    sc->cx = soa; sc->cy = soa + count; sc->cz = soa + 2 * count; sc->sqR = soa + 3 * count; sc->invR = soa + 4 * count;
    for (int i = 0; i < count; ++i) { /* as tpto_render fills them (Test.cpp:321-339) */
        sc->cx[i] = spheres[i].cx;
        sc->cy[i] = spheres[i].cy;
        sc->cz[i] = spheres[i].cz;
        sc->sqR[i] = spheres[i].radius * spheres[i].radius;
        sc->invR[i] = spheres[i].invRadius;
        if (mats[i].emissive[0] > 0 || mats[i].emissive[1] > 0 || mats[i].emissive[2] > 0)
            sc->emissive[sc->emissiveCount++] = i;
    }
    int64_t rays = 0;
#ifdef _OPENMP
    int nt = p->threads > 0 ? p->threads : omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : rays) num_threads(nt)
#endif
    for (int y = 0; y < p->height; ++y) rays += AdaptiveRows(sc, p, y, y + 1, backbuffer, albedo, normalDepth, moments, counts);
    free(soa);
    free(sc->emissive);
    free(sc);
    return rays;
}

/* tptAdaptiveSamplesDevice as include/tpt_hip.h states it; outVariance may be NULL.  Returns the sum of the counts, or -1 for
 * arguments the product refuses. */
int64_t adaptive_plan(int w, int h, const float* moments, float targetError, int minSamples, int maxSamples, int32_t* counts,
                      float* outVariance)
{
    static const float gk[3] = {0.25f, 0.5f, 0.25f};
    if (w < 1 || w > 8192 || h < 1 || h > 8192 || !moments || !counts) return -1;
    if (!(targetError > 0.0f && targetError <= 1e6f) || minSamples < 0 || maxSamples > 2047 || minSamples > maxSamples) return -1;
    int64_t total = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t p = (size_t)y * w + x;
            const float* m = moments + p * 4;
            const float S = m[3];
            const int valid = adaptiveValid(S);
            const float d = m[1] - m[0] * m[0];
            const float var = d > 0.0f ? d : 0.0f;
            float gv = 0.0f, gw = 0.0f;
            for (int jy = 0; jy < 3; ++jy)
                for (int jx = 0; jx < 3; ++jx) {
                    const int qy = y + jy - 1, qx = x + jx - 1;
                    if (qy < 0 || qy >= h || qx < 0 || qx >= w) continue;
                    const float* mq = moments + ((size_t)qy * w + qx) * 4;
                    if (!adaptiveValid(mq[3])) continue;
                    const float dq = mq[1] - mq[0] * mq[0];
                    const float varq = dq > 0.0f ? dq : 0.0f;
                    const float b = mq[0] + ADAPTIVE_LUM_FLOOR;
                    const float r = varq / (b * b);
                    const float k = gk[jy] * gk[jx];
                    gv = gv + k * r;
                    gw = gw + k;
                }
            int n = minSamples > 1 ? minSamples : 1;
            if (valid && gw > 0.0f) {
                const float R = gv / gw;
                const float need = R / (targetError * targetError);
                const float extra = need - S;
                if (!(extra > (float)minSamples)) n = minSamples;
                else if (extra >= (float)maxSamples) n = maxSamples;
                else n = (int)ceilf(extra);
            }
            counts[p] = n;
            total += n;
            if (outVariance) {
                float* o = outVariance + p * 4;
                o[0] = 0.0f; o[1] = valid ? var / S : 0.0f; o[2] = 0.0f; o[3] = valid ? S : 0.0f;
            }
        }
    return total;
}
