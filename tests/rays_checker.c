/* tests/rays_checker.c -- TEST INFRASTRUCTURE ONLY: the CPU reference of tptTraceRaysDevice.
 *
 * The checker of oracle/tpt_oracle.c (included, not modified: its statics are reached from here) asked the one question the entry
 * point answers: what comes back along this ray, and what does it meet first?  Per ray, as include/tpt_hip.h states it, with the
 * oracle's own HitSpheres, Trace and TraceForward:
 *   state = the seed word's bits, or 1 where they are 0;  o, d as given (d is not normalised)
 *   hits[i]     = {pos, t} {normal, bits(id)} of HitSpheres({o, d}, kMinT, kMaxT), or {0,0,0,0} {0,0,0,bits(-1)}
 *   radiance[i] = {0.0f + Trace({o, d}, 0, state, 1), (float)k}, k the HitWorld calls Trace counted for this ray
 *   without a radiance buffer k = 1: the path ends after its first HitWorld
 * camera_rays makes the rays a frame's first samples start with (TraceRows' pixel seed, two jitter draws, CameraGetRay), so that the
 * checker on them can be held against tpto_render at 1 spp (tests/test_rays_checker.py).  Built with oracle/Makefile's CFLAGS.
 */
#include "../oracle/tpt_oracle.c"

static uint32_t f2bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float bits2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

/* The rays of frame `frame`'s first sample per pixel, pixel (x, y) at out[(y * w + x) * 8] (row 0 at the bottom, like the backbuffer):
 * {origin, bits(state after the ray was made)}, {direction, 0} */
void camera_rays(const TptoCamera* cam, int w, int h, int frame, float* out)
{
    const float invWidth = 1.0f / w, invHeight = 1.0f / h;
    for (uint32_t y = 0; y < (uint32_t)h; ++y)
        for (int x = 0; x < w; ++x) {
            uint32_t state = ((uint32_t)x * 1973u + y * 9277u + (uint32_t)frame * 26699u) | 1u; /* ComputeShader.hlsl:380 */
            const float u = ((float)x + RND(&state)) * invWidth;
            const float v = ((float)y + RND(&state)) * invHeight;
            const Ray r = CameraGetRay(cam, u, v, &state);
            float* o = out + ((size_t)y * w + x) * 8;
            o[0] = r.orig.x; o[1] = r.orig.y; o[2] = r.orig.z; o[3] = bits2f(state);
            o[4] = r.dir.x; o[5] = r.dir.y; o[6] = r.dir.z; o[7] = 0.0f;
        }
}

/* tptTraceRaysDevice on the host: radiance (nRays x 4 floats) and hits (nRays x 8 floats) may each be NULL; p gives fold_mode,
 * math_mode, no_light_sampling and mitsuba_compare (everything else of it is unused).  Returns the sum of k. */
int64_t rays_trace(const TptoSphere* spheres, const TptoMaterial* mats, int count, const TptoParams* p, int nRays, const float* rays,
                   float* radiance, float* hits)
{
    Scene* sc = (Scene*)calloc(1, sizeof(Scene));
    if (count < 0) count = 0;
    sc->emissive = (int*)malloc(sizeof(int) * (size_t)(count > 0 ? count : 1));
    sc->spheres = spheres;
    sc->mats = mats;
    sc->count = count;
    sc->cam = NULL;
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
    int64_t total = 0;
#ifdef _OPENMP
    int nt = p->threads > 0 ? p->threads : omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : total) num_threads(nt)
#endif
    for (int i = 0; i < nRays; ++i) {
        const float* rec = rays + (size_t)i * 8;
        uint32_t state = f2bits(rec[3]);
        if (state == 0u) state = 1u;
        Ray r;
        r.orig = mk(rec[0], rec[1], rec[2]);
        r.dir = mk(rec[4], rec[5], rec[6]);
        if (hits) {
            Hit h;
            const int id = HitSpheres(sc, &r, kMinT, kMaxT, &h);
            float* o = hits + (size_t)i * 8;
            for (int k = 0; k < 7; ++k) o[k] = 0.0f;
            o[7] = bits2f((uint32_t)id);
            if (id != -1) {
                o[0] = h.pos.x; o[1] = h.pos.y; o[2] = h.pos.z; o[3] = h.t;
                o[4] = h.normal.x; o[5] = h.normal.y; o[6] = h.normal.z;
            }
        }
        int64_t k = 1;
        if (radiance) {
            k = 0;
            f3 c = sc->fold_mode == TPTO_FOLD_FORWARD ? TraceForward(sc, r, &k, &state) : Trace(sc, &r, 0, &k, &state, 1);
            c = add(mk(0.0f, 0.0f, 0.0f), c);
            float* o = radiance + (size_t)i * 4;
            o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = (float)k;
        }
        total += k;
    }
    free(soa);
    free(sc->emissive);
    free(sc);
    return total;
}
