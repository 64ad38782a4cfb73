// reproj_gates.h — the viewing gates of the reprojection matchers, shared by K2 (reproj_match.hip, 256-bit descriptors) and
// K13 (l2_match.hip, float descriptors).  Include only in translation units built with -ffp-contract=off.
#pragma once
#include "tri_core.h"

// The viewing gates once the point's observations are accumulated (src/MapPoint.cpp:24-45): `normal` the sum of the unit
// rays from the observing keyframes, nearest / furthest their distance range; center = Frame::camera_center.
__device__ __forceinline__ bool k2_view_gates(float* normal, float nearest, float furthest, const float* X, const float* center)
{
    const float ray[3] = {X[0] - center[0], X[1] - center[1], X[2] - center[2]};
    normalize3f(normal);
    float rn[3] = {ray[0], ray[1], ray[2]};
    normalize3f(rn);
    if (dot3f(normal, rn) < 0.5f) return false;                         // :62-66
    const float distance = sqrtf(dot3f(ray, ray));
    return !(distance < nearest / 2.0f || distance > furthest * 1.25f);  // :69-73
}
