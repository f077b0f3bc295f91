// tpt_animation.h -- the animated scene of kFlagAnimate (Test.cpp:304-308) in one place: where spheres 1 and 8 are at a time.
// tptUpdate moves the context's spheres with it; tptDrawDeviceAnimation computes every frame's centres of a batch with it on the host
// (the same binary32 cosf / sinf, so the same bits) and ships them to tptTraceAnimationKernel as a table.
#pragma once
#include <cmath>

namespace tpt {

// UpdateTest's animation, Test.cpp:304-308: s_Spheres[1].center.y and s_Spheres[8].center.z at `time`
inline float animatedY1(float time) { return cosf(time) + 1.0f; }
inline float animatedZ8(float time) { return sinf(time) * 0.3f; }

} // namespace tpt
