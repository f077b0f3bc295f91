// TEST INFRASTRUCTURE: what the animation kernel's HitSpheres does with the filter data of ONE staged scene over a batch of frames
// (tptDrawDeviceAnimation), restated on the host from the same headers: the batch's last frame packed by packScene, each frame's
// centres of spheres 1 and 8 from tpt_animation.h; phase 1 as phase1MatrixHRef (matrix-core table) and phase1Chunk (packed VALU pair
// records), phase 2 as hitSpheresCandidates<true> / hitSpheresTwoPhase<true>.  Held against the reference's loop over every sphere of
// the frame's own scene (hitSpheresSimple) on near-tangent rays of the moving spheres.  Exported to tests/test_animation_abi.py.
#include <math.h>
#include <stdint.h>
#include <vector>
#include "tpt_animation.h"
#include "tpt_scene.h"
using namespace tpt;

static double urand(uint64_t& s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }

// the default scene with spheres 1 and 8 of radius r1 / r8 (small radii: the spheres move many radii during a batch), nFrames times
// `times`; out[0] rays, out[1] / out[2] rays whose (id, t) differ from the reference with the matrix / VALU filter, out[3] rays that
// hit a moving sphere the staged filter data alone rejects (the case the forced candidates exist for), out[4] hits of a moving sphere
extern "C" int an_filter_check(float r1, float r8, const float* times, int nFrames, int raysPerFrame, unsigned long long seed, long long* out)
{
    std::vector<SpherePOD> S;
    std::vector<MaterialPOD> M;
    defaultScene(S, M);
    S[1].radius = r1;
    S[8].radius = r8;
    S[1].cy = animatedY1(times[nFrames - 1]); // the staged scene: the batch's last frame
    S[8].cz = animatedZ8(times[nFrames - 1]);
    PackedScene staged;
    packScene(S, M, staged);
    if (staged.mxR1 < 0) return -1;
    const SceneView sv = viewOf(staged);
    uint64_t s = seed | 1;
    for (int k = 0; k < 5; ++k) out[k] = 0;
    for (int j = 0; j < nFrames; ++j) {
        std::vector<SpherePOD> F = S;
        F[1].cy = animatedY1(times[j]);
        F[8].cz = animatedZ8(times[j]);
        PackedScene frame;
        packScene(F, M, frame);
        const SceneView fv = viewOf(frame);
        const f4 moved[2] = {{F[1].cx, F[1].cy, F[1].cz, 0.0f}, {F[8].cx, F[8].cy, F[8].cz, 0.0f}};
        for (int i = 0; i < raysPerFrame; ++i) {
            // a ray that grazes sphere 1 or 8 of this frame: passes c + n r (1 + eps), eps in +-[1e-9, 1e-2], from up to 10 units away
            const int k = (i & 1) ? 8 : 1;
            const double c[3] = {F[k].cx, F[k].cy, F[k].cz}, r = F[k].radius;
            double n[3], t[3];
            for (int a = 0; a < 3; ++a) { n[a] = 2 * urand(s) - 1; t[a] = 2 * urand(s) - 1; }
            double nl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            for (int a = 0; a < 3; ++a) n[a] /= nl;
            const double tn = t[0] * n[0] + t[1] * n[1] + t[2] * n[2];
            for (int a = 0; a < 3; ++a) t[a] -= tn * n[a];
            const double eps = pow(10.0, -9 + 7 * urand(s)) * (urand(s) < 0.5 ? -1 : 1), L = 0.05 + 10 * urand(s);
            double o[3];
            for (int a = 0; a < 3; ++a) o[a] = c[a] + n[a] * r * (1 + eps) - t[a] * L;
            const f3 of = mk3((float)o[0], (float)o[1], (float)o[2]);
            const f3 df = normalize(mk3((float)t[0], (float)t[1], (float)t[2]));
            float tr, tm, tv;
            const int want = hitSpheresSimple(fv, of, df, TPT_MIN_T, TPT_MAX_T, tr);
            const uint64_t cand = phase1MatrixHRef(sv.amatH, sv.mxR1, sv.nSpheres, of, df);
            const int gm = hitSpheresCandidates<true>(sv, cand, of, df, TPT_MIN_T, TPT_MAX_T, tm, moved);
            const int gv = hitSpheresTwoPhase<true>(sv, of, df, TPT_MIN_T, TPT_MAX_T, tv, moved);
            out[0]++;
            out[1] += gm != want || f2u(tm) != f2u(tr);
            out[2] += gv != want || f2u(tv) != f2u(tr);
            if (want == 1 || want == 8) {
                out[4]++;
                // would the staged data alone have kept it?  (either filter dropping it is what the forced candidates answer)
                const uint64_t bit = 0x8000000000000000ull >> want;
                float td;
                const int pv = hitSpheresTwoPhase(sv, of, df, TPT_MIN_T, TPT_MAX_T, td); // (static data, no forcing: sphere at its last position)
                out[3] += !(cand & bit) && pv != want;
            }
        }
    }
    return 0;
}
extern "C" float an_y1(float time) { return animatedY1(time); }
extern "C" float an_z8(float time) { return animatedZ8(time); }
