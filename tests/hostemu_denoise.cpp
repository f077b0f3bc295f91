// tests/hostemu_denoise.cpp -- TEST INFRASTRUCTURE ONLY: tptDenoiseDevice's launcher for the host runtime built against tests/hostemu
// (tests/test_denoise_abi.py).  It counts the calls that reach it, so a test can tell accepted calls from refused ones, and runs nothing
// -- unless the test has asked for the filter (hostemuDenoiseRun(1)): then every iteration is a piece of work of the stream it is given,
// reading and writing the planes the product's launcher gives its kernels (iteration i of n writes the scratch plane where n - 1 - i is
// odd, the output otherwise, and reads what the one before it wrote), the arithmetic restated from include/tpt_hip.h in the order
// tests/denoise_checker.c writes it.
#include <stddef.h>

namespace {
int gLaunches = 0;
bool gRun = false;
struct Iteration {
    const float *src, *albedo, *nd;
    float* dst;
    int w, h, step;
    float ic, in, id;
    bool demodIn, demodOut;
};
void runIteration(void* p)
{
    const Iteration& J = *static_cast<const Iteration*>(p);
    static const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    // (a pixel's colour as the iteration reads it: the first one divides the albedo out)
    auto load = [&](size_t at, float* c) {
        for (int k = 0; k < 3; ++k) {
            const float v = J.src[4 * at + k], a = J.demodIn ? J.albedo[4 * at + k] : 0.0f;
            c[k] = a > 0.0f ? v / a : v;
        }
    };
    for (int y = 0; y < J.h; ++y)
        for (int x = 0; x < J.w; ++x) {
            const size_t at = (size_t)y * J.w + x;
            float cp[3], cq[3], sumW = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f};
            load(at, cp);
            for (int ky = 0; ky < 5; ++ky)
                for (int kx = 0; kx < 5; ++kx) {
                    const int qx = x + (kx - 2) * J.step, qy = y + (ky - 2) * J.step;
                    if (qx < 0 || qx >= J.w || qy < 0 || qy >= J.h) continue;
                    const size_t q = (size_t)qy * J.w + qx;
                    load(q, cq);
                    const float dr = cq[0] - cp[0], dg = cq[1] - cp[1], db = cq[2] - cp[2];
                    float den = 1.0f + ((dr * dr + dg * dg) + db * db) * J.ic;
                    if (J.nd) {
                        const float *nq = J.nd + 4 * q, *np = J.nd + 4 * at;
                        const float dx = nq[0] - np[0], dy = nq[1] - np[1], dz = nq[2] - np[2], dd = nq[3] - np[3];
                        den = den * (1.0f + ((dx * dx + dy * dy) + dz * dz) * J.in);
                        den = den * (1.0f + (dd * dd) * J.id);
                    }
                    const float wt = (hk[ky] * hk[kx]) / den;
                    sumW += wt;
                    for (int k = 0; k < 3; ++k) sum[k] += wt * cq[k];
                }
            for (int k = 0; k < 3; ++k) {
                const float f = sum[k] / sumW, a = J.demodOut ? J.albedo[4 * at + k] : 0.0f;
                J.dst[4 * at + k] = a > 0.0f ? f * a : f;
            }
            J.dst[4 * at + 3] = J.src[4 * at + 3];
        }
}
} // namespace

hipError_t tptLaunchDenoise(const float* colour, const float* albedo, const float* normalDepth, float* out, float* scratch, int width, int height,
                            int iterations, float ic, float in, float id, bool demodulate, hipStream_t stream)
{
    ++gLaunches;
    if (!gRun) return hipSuccess;
    if (iterations > 1 && !scratch) return hipErrorInvalidValue;
    const float* src = colour;
    for (int i = 0; i < iterations; ++i) {
        float* dst = ((iterations - 1 - i) & 1) ? scratch : out;
        const Iteration J = {src, albedo, normalDepth, dst, width, height, 1 << i, ic * (float)(1u << (2 * i)), in, id, demodulate && i == 0,
                             demodulate && i == iterations - 1};
        hostemuEnqueue(stream, runIteration, &J, sizeof(J));
        src = dst;
    }
    return hipSuccess;
}
extern "C" __attribute__((visibility("default"))) int hostemuDenoiseLaunches() { return gLaunches; }
extern "C" __attribute__((visibility("default"))) void hostemuDenoiseRun(int on) { gRun = on != 0; }
