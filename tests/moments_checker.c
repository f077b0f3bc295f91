/* tests/moments_checker.c -- TEST INFRASTRUCTURE ONLY: the CPU reference of tptDrawDeviceMoments.
 *
 * The checker of oracle/tpt_oracle.c (included, not modified: its statics are reached from here) with TraceRows' per-pixel sample
 * loop restated once more, as tests/aov_checker.c restates it: each sample's camera ray goes through HitSpheres first (no random
 * numbers drawn) for the first-hit planes, then through Trace exactly as the oracle traces it.  Each sample's Trace colour c_s is
 * captured as it is added to the pixel's sum, and the moments are what include/tpt_hip.h defines:
 *   l_s = (0.2126f*c_s.x + 0.7152f*c_s.y) + 0.0722f*c_s.z      frame moments = {sum l_s, sum l_s*l_s, 0} * (1.0f / spp)
 * float sums from +0 in sample order, blended into the moments plane's .xyz like the tile (same lerp factor, .w kept).  The colour and
 * the ray count are the oracle's (tests/test_moments_checker.py holds them against tpto_render).  Built with oracle/Makefile's CFLAGS.
 */
#include "../oracle/tpt_oracle.c"

typedef struct { float x, y, z, w; } aov4;

/* TraceRows (Test.cpp:266-300) for rows [start, end), plus the planes (full-image addressing, like the backbuffer) */
static int64_t MomentRows(const Scene* sc, const TptoParams* p, int start, int end, float* backbufferBase, float* albedoBase, float* normalDepthBase,
                          float* momentsBase)
{
    float* backbuffer = backbufferBase + (size_t)start * p->width * 4;
    aov4* albedo = (aov4*)albedoBase + (size_t)start * p->width;
    aov4* normalDepth = (aov4*)normalDepthBase + (size_t)start * p->width;
    float* moments = momentsBase + (size_t)start * p->width * 4;
    float invWidth = 1.0f / p->width;
    float invHeight = 1.0f / p->height;
    float lerpFac = (float)p->frame / (float)(p->frame + 1);
    if (p->flags & TPTO_FLAG_ANIMATE) lerpFac *= p->has_animate_smoothing ? p->animate_smoothing : 0.9f;
    if (!(p->flags & TPTO_FLAG_PROGRESSIVE)) lerpFac = 0;
    int64_t rayCount = 0;
    for (uint32_t y = (uint32_t)start; y < (uint32_t)end; ++y) {
        uint32_t state = (y * 9781u + (uint32_t)p->frame * 6271u) | 1u;
        for (int x = 0; x < p->width; ++x) {
            if (p->seed_mode == TPTO_SEED_PER_PIXEL)
                state = ((uint32_t)x * 1973u + y * 9277u + (uint32_t)p->frame * 26699u) | 1u;
            f3 col = mk(0, 0, 0);
            aov4 sa = {0.0f, 0.0f, 0.0f, 0.0f}, sn = {0.0f, 0.0f, 0.0f, 0.0f};
            float sl = 0.0f, sl2 = 0.0f;
            for (int s = 0; s < p->spp; s++) {
                float u = ((float)x + RND(&state)) * invWidth;
                float v = ((float)y + RND(&state)) * invHeight;
                Ray r = CameraGetRay(sc->cam, u, v, &state);
                /* the sample's first hit: HitWorld(r_s, kMinT, kMaxT), what Trace's first call computes */
                Hit h;
                const int id = HitSpheres(sc, &r, kMinT, kMaxT, &h);
                aov4 a = {0.0f, 0.0f, 0.0f, 0.0f}, n = {0.0f, 0.0f, 0.0f, 0.0f};
                if (id != -1) {
                    a.x = sc->mats[id].albedo[0];
                    a.y = sc->mats[id].albedo[1];
                    a.z = sc->mats[id].albedo[2];
                    a.w = 1.0f;
                    n.x = h.normal.x;
                    n.y = h.normal.y;
                    n.z = h.normal.z;
                    n.w = h.t;
                }
                sa.x = sa.x + a.x; sa.y = sa.y + a.y; sa.z = sa.z + a.z; sa.w = sa.w + a.w;
                sn.x = sn.x + n.x; sn.y = sn.y + n.y; sn.z = sn.z + n.z; sn.w = sn.w + n.w;
                f3 c = sc->fold_mode == TPTO_FOLD_FORWARD ? TraceForward(sc, r, &rayCount, &state)
                                                         : Trace(sc, &r, 0, &rayCount, &state, 1);
                col = add(col, c);
                const float l = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
                sl = sl + l;
                sl2 = sl2 + l * l;
            }
            const float inv = 1.0f / (float)p->spp;
            col = muls(col, inv);
            f3 prev = mk(backbuffer[0], backbuffer[1], backbuffer[2]);
            col = add(muls(prev, lerpFac), muls(col, 1 - lerpFac));
            backbuffer[0] = col.x;
            backbuffer[1] = col.y;
            backbuffer[2] = col.z;
            backbuffer += 4;
            f3 m = mk(sl * inv, sl2 * inv, 0.0f * inv);
            f3 mprev = mk(moments[0], moments[1], moments[2]);
            m = add(muls(mprev, lerpFac), muls(m, 1 - lerpFac));
            moments[0] = m.x;
            moments[1] = m.y;
            moments[2] = m.z;
            moments += 4;
            albedo->x = sa.x * inv; albedo->y = sa.y * inv; albedo->z = sa.z * inv; albedo->w = sa.w * inv;
            normalDepth->x = sn.x * inv; normalDepth->y = sn.y * inv; normalDepth->z = sn.z * inv; normalDepth->w = sn.w * inv;
            albedo++;
            normalDepth++;
        }
    }
    return rayCount;
}

/* tpto_render with the planes and the moments: backbuffer and moments (h * w * 4 floats each) are blended as tpto_render blends the
 * backbuffer; albedo and normalDepth are overwritten for every pixel */
int64_t moments_render(const TptoSphere* spheres, const TptoMaterial* mats, int count, const TptoCamera* cam, const TptoParams* p,
                       float* backbuffer, float* albedo, float* normalDepth, float* moments)
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
    for (int y = 0; y < p->height; ++y) rays += MomentRows(sc, p, y, y + 1, backbuffer, albedo, normalDepth, moments);
    free(soa);
    free(sc->emissive);
    free(sc);
    return rays;
}
