// point_core.h — the per-point bodies of K12 (Mapper::cull_points' error, reference src/Mapper.cpp:411-420) and K13 (the
// re-anchoring of Mapper::bundle_adjust's tail, :380-393), shared by the flattened forms in tracks.hip and the
// resident-map forms in map_keyframe.hip: ONE body each, so that both forms execute the same f32 operations in the same
// order.  Include only in translation units built with -ffp-contract=off (tri_core.h).
#pragma once
#include "tri_core.h"

// K13: in_camera = R_before X + t_before; X' = R_after^T (in_camera - t_after), all f32.  B and A are rows 0..2 of the two
// row-major poses (12 floats are read of each).  A 3-term dot product is (a0 b0 + a1 b1) + a2 b2 as everywhere in this
// library (Eigen's own order is unspecified upstream).
__device__ __forceinline__ void reanchor_f32(const float* B, const float* A, const float* X, float* out)
{
    float c[3], d[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        c[r] = ((B[4 * r] * X[0] + B[4 * r + 1] * X[1]) + B[4 * r + 2] * X[2]) + B[4 * r + 3];     // :389
        d[r] = c[r] - A[4 * r + 3];
    }
#pragma unroll
    for (int r = 0; r < 3; r++)                                                                       // :390
        out[r] = (A[r] * d[0] + A[4 + r] * d[1]) + A[8 + r] * d[2];
}

// K12: the f32 sum over observations [o0, o1), in that order, of (project(pose, X) - pixel).norm() (:413).  The pose of
// observation o is poses[obs_pose[o]]; its pixel is uv[uv_row[o]], or uv[o] when uv_row is null.  *esum (null: not
// wanted) gets the f64 sum of the same f32 errors (Slam::reprojection_error).
__device__ __forceinline__ float point_error_sum_f32(const TriParams& k, const float* __restrict__ poses,
                                                     const int32_t* __restrict__ obs_pose, const float2* __restrict__ uv,
                                                     const int32_t* __restrict__ uv_row, const float* X, int o0, int o1,
                                                     double* esum)
{
    float err = 0.0f;
    double es = 0.0;
    for (int o = o0; o < o1; o++) {
        float T[16];
        load_pose(poses, obs_pose[o], T);
        const float2 pr = project_f32(k, T, X);
        const float2 px = uv[uv_row ? uv_row[o] : o];
        const float dx = pr.x - px.x, dy = pr.y - px.y;
        const float e = sqrtf(dx * dx + dy * dy);
        err += e;                                                    // :413
        es += (double)e;
    }
    if (esum) *esum = es;
    return err;
}

// the culling rule (:416, :420): *mean = err / cnt (0 without observations); true = cull
__device__ __forceinline__ bool point_cull_rule_f32(float err, int cnt, float max_mean_error, float* mean)
{
    *mean = cnt > 0 ? err / (float)cnt : 0.0f;
    return cnt > 0 && *mean > max_mean_error;
}
