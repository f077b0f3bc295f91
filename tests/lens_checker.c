/* tests/lens_checker.c -- TEST INFRASTRUCTURE ONLY: the CPU reference of tptDrawDeviceLens.
 *
 * The checker of oracle/tpt_oracle.c (included, not modified: its statics are reached from here) with a panorama, fisheye or
 * orthographic lens in the camera's place, as include/tpt_hip.h states the draw:
 *   lens_ray     one sample's ray {o, d} for (u, v), written with tptm_sinf / tptm_cosf, sqrtf, IEEE division and the oracle's normalize
 *   lens_render  TraceRows with per-pixel seeds and lens_ray where CameraGetRay stands: all spp samples of a pixel from the pixel's
 *                stream, colour * (1.0f / spp), the blend with lerp = frame / (frame + 1) under TPTO_FLAG_PROGRESSIVE, else 0
 *   lens_rays    tptTraceRaysDevice records of every pixel's FIRST sample: the seed, two draws, the lens ray, and the state left
 *                behind as the seed word -- so that tests/rays_checker.c on them can be held against lens_render at 1 spp
 *   lens_sincos  tptm_sinf / tptm_cosf of n arguments (the device's tsincosf is held against them on the lenses' argument domain)
 * Built with oracle/Makefile's CFLAGS (no FMA contraction).
 */
#include "../oracle/tpt_oracle.c"

enum { LENS_EQUIRECT = 1, LENS_FISHEYE = 2, LENS_ORTHO = 3 };
typedef struct Lens { /* include/tpt_hip.h: tptLens */
    int kind;
    float origin[3], right[3], up[3], forward[3];
    float sx, sy, maxAngle;
} Lens;

static float bits2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static Ray LensGetRay(const Lens* l, float u, float v)
{
    const float a = (u - 0.5f) * l->sx, b = (v - 0.5f) * l->sy;
    const f3 right = ld3(l->right), up = ld3(l->up), forward = ld3(l->forward);
    Ray r;
    f3 q;
    r.orig = ld3(l->origin);
    if (l->kind == LENS_EQUIRECT) {
        const float sa = tptm_sinf(a), ca = tptm_cosf(a), sb = tptm_sinf(b), cb = tptm_cosf(b);
        q = add(add(muls(right, cb * sa), muls(up, sb)), muls(forward, cb * ca));
    } else if (l->kind == LENS_FISHEYE) {
        const float rr = sqrtf(a * a + b * b);
        const float st = tptm_sinf(rr * l->maxAngle), ct = tptm_cosf(rr * l->maxAngle);
        const float k = rr > 0 ? st / rr : 0.0f;
        q = add(add(muls(right, a * k), muls(up, b * k)), muls(forward, ct));
    } else {
        q = forward;
        r.orig = add(add(r.orig, muls(right, a)), muls(up, b));
    }
    r.dir = normalize(q);
    return r;
}

void lens_sincos(int n, const float* x, float* outSin, float* outCos)
{
    for (int i = 0; i < n; ++i) {
        outSin[i] = tptm_sinf(x[i]);
        outCos[i] = tptm_cosf(x[i]);
    }
}

/* out6 = {o, d} */
void lens_ray(const Lens* lens, float u, float v, float* out6)
{
    const Ray r = LensGetRay(lens, u, v);
    out6[0] = r.orig.x; out6[1] = r.orig.y; out6[2] = r.orig.z;
    out6[3] = r.dir.x; out6[4] = r.dir.y; out6[5] = r.dir.z;
}

static Scene* make_scene(const TptoSphere* spheres, const TptoMaterial* mats, int count, const TptoParams* p)
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
    return sc;
}
static void free_scene(Scene* sc)
{
    free(sc->cx);
    free(sc->emissive);
    free(sc);
}

/* tptDrawDeviceLens on the host: p gives width, height, spp, frame, flags (TPTO_FLAG_PROGRESSIVE or 0), fold_mode, math_mode,
 * no_light_sampling, mitsuba_compare and threads; the backbuffer ([h][w][4], row 0 at the bottom) is blended into.  Returns the
 * HitWorld calls. */
int64_t lens_render(const TptoSphere* spheres, const TptoMaterial* mats, int count, const Lens* lens, const TptoParams* p, float* backbuffer)
{
    Scene* sc = make_scene(spheres, mats, count, p);
    const int w = p->width, h = p->height;
    const float invWidth = 1.0f / w, invHeight = 1.0f / h;
    float lerpFac = (float)p->frame / (float)(p->frame + 1); /* Test.cpp:272 */
    if (!(p->flags & TPTO_FLAG_PROGRESSIVE)) lerpFac = 0;
    int64_t total = 0;
#ifdef _OPENMP
    int nt = p->threads > 0 ? p->threads : omp_get_max_threads();
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : total) num_threads(nt)
#endif
    for (int yy = 0; yy < h; ++yy) {
        const uint32_t y = (uint32_t)yy;
        int64_t rayCount = 0;
        for (int x = 0; x < w; ++x) {
            uint32_t state = ((uint32_t)x * 1973u + y * 9277u + (uint32_t)p->frame * 26699u) | 1u; /* ComputeShader.hlsl:380 */
            f3 col = mk(0, 0, 0);
            for (int s = 0; s < p->spp; s++) {
                const float u = ((float)x + RND(&state)) * invWidth;
                const float v = ((float)y + RND(&state)) * invHeight;
                Ray r = LensGetRay(lens, u, v);
                f3 c = sc->fold_mode == TPTO_FOLD_FORWARD ? TraceForward(sc, r, &rayCount, &state) : Trace(sc, &r, 0, &rayCount, &state, 1);
                col = add(col, c);
            }
            col = muls(col, 1.0f / (float)p->spp);
            float* px = backbuffer + ((size_t)yy * w + x) * 4;
            const f3 prev = mk(px[0], px[1], px[2]);
            col = add(muls(prev, lerpFac), muls(col, 1 - lerpFac));
            px[0] = col.x; px[1] = col.y; px[2] = col.z;
        }
        total += rayCount;
    }
    free_scene(sc);
    return total;
}

/* The rays of frame `frame`'s first sample per pixel, pixel (x, y) at out[(y * w + x) * 8]: {origin, bits(state after the two
 * draws)}, {direction, 0} */
void lens_rays(const Lens* lens, int w, int h, int frame, float* out)
{
    const float invWidth = 1.0f / w, invHeight = 1.0f / h;
    for (uint32_t y = 0; y < (uint32_t)h; ++y)
        for (int x = 0; x < w; ++x) {
            uint32_t state = ((uint32_t)x * 1973u + y * 9277u + (uint32_t)frame * 26699u) | 1u;
            const float u = ((float)x + RND(&state)) * invWidth;
            const float v = ((float)y + RND(&state)) * invHeight;
            const Ray r = LensGetRay(lens, u, v);
            float* o = out + ((size_t)y * w + x) * 8;
            o[0] = r.orig.x; o[1] = r.orig.y; o[2] = r.orig.z; o[3] = bits2f(state);
            o[4] = r.dir.x; o[5] = r.dir.y; o[6] = r.dir.z; o[7] = 0.0f;
        }
}
