// rtg_reproject.h — the device functions k_temporal (rtg_temporal.hip) and k_svgf_temporal (rtg_svgf.hip)
// share: the projection into the history's camera and the three-term dot of the admission tests (rtg_svgf.hip's
// variance and filter kernels use the dot too). IEEE float32 without contraction, the operations in the order
// written: the numpy restatements pin every bit (tests/temporal_ref.py, tests/svgf_ref.py).
// The 2 x 2 tap loop and the blend stay written out in each of the two kernels. Shared as a __forceinline__
// template <bool MOMENTS> they compute the same bits, but the compiler orders the operands of some packed
// multiplies and mask ANDs the other way round in both kernels, and these kernels must stay
// the instructions that were measured. A change to one loop goes into the other as well.
#pragma once
#include "rtg_filter_state.h"

static __device__ __forceinline__ float rp_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// Camera::projectOntoCamera (Scene.h:55-69) in project_onto_camera's operation order (rtg_light.hip)
static __device__ __forceinline__ bool rp_project(const TemporalProj& c, float px, float py, float pz, float& x,
                                                  float& y) {
    const float* m = c.C2V;
    const float vx = ((px * m[0] + py * m[1]) + pz * m[2]) + m[3];
    const float vy = ((px * m[4] + py * m[5]) + pz * m[6]) + m[7];
    const float vz = ((px * m[8] + py * m[9]) + pz * m[10]) + m[11];
    const float* q = c.P;
    const float v1x = ((vx * q[0] + vy * q[1]) + vz * q[2]) + q[3];
    const float v1y = ((vx * q[4] + vy * q[5]) + vz * q[6]) + q[7];
    float w = (((q[12] * vx) + (q[13] * vy)) + (q[14] * vz)) + q[15];
    w = 1.0f / w;
    x = ((v1x * w) + 1.0f) * 0.5f;
    y = ((v1y * w) + 1.0f) * 0.5f;
    if (x < 0 || x > 1.0f || y < 0 || y > 1.0f) return false;
    x = x * c.W;
    y = 1.0f - y;
    y = y * c.H;
    return true;
}
