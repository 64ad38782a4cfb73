// map_keyframe.hip — the two per-key-frame stages of Mapper::insert that run on the resident map's device image
// (map.hip: rs_map_reanchor, rs_map_cull_points), one lane per point slot:
//
//   KF1 k_kf_reanchor   the tail of Mapper::bundle_adjust (reference src/Mapper.cpp:379-393): a slot that is alive, has
//                       exactly one observation and whose observer is a listed key frame moves rigidly with that key
//                       frame, X' = R_after^T((R_before X + t_before) - t_after) — K13's body (point_core.h), "after" read
//                       from the image's pose table.  A point has one observer here, so no slot is written twice.
//   KF2 k_kf_cull       Mapper::cull_points (:396-431): a slot that is alive and observed by a listed key frame is local;
//                       its error over ALL of its observations, in the CSR's order, is K12's body (point_core.h) with the
//                       pose from the pose table and the pixel from the key-point pool.
//   KF3 k_kf_compact    the selected slots in ascending order with their positions, and the two counts, by one workgroup
//                       (an ordered scan over the per-slot flag bytes in chunks of 1024).
//
// Built with -ffp-contract=off like tracks.hip, whose K12 / K13 share the bodies: both forms then execute the same IEEE
// operations.  The launch functions take raw device pointers; map.hip owns the image, the staging and the read-back.
#include "point_core.h"

// flag bytes: bit 0 = selected (moved / culled), bit 1 = local (KF2 only)
__global__ __launch_bounds__(256) void k_kf_reanchor(int P, const uint8_t* __restrict__ alive, const int32_t* __restrict__ obs_ptr,
                                                     const int32_t* __restrict__ obs_kf, const int32_t* __restrict__ win_of_kf,
                                                     const float* __restrict__ before, const float* __restrict__ poses,
                                                     float* __restrict__ pos, uint8_t* __restrict__ flag)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int o0 = obs_ptr[p], o1 = obs_ptr[p + 1];
    int w = -1, kf = 0;
    if (alive[p] != 0 && o1 - o0 == 1) {                              // :387
        kf = obs_kf[o0];
        w = win_of_kf[kf];                                            // list index, -1: not listed
    }
    flag[p] = w >= 0 ? 1 : 0;
    if (w < 0) return;
    float B[16], A[16];
    load_pose(before, w, B);
    load_pose(poses, kf, A);
    const float X[3] = {pos[3 * (size_t)p], pos[3 * (size_t)p + 1], pos[3 * (size_t)p + 2]};
    reanchor_f32(B, A, X, pos + 3 * (size_t)p);
}

__global__ __launch_bounds__(256) void k_kf_cull(int P, const uint8_t* __restrict__ alive, const int32_t* __restrict__ obs_ptr,
                                                 const int32_t* __restrict__ obs_kf, const int32_t* __restrict__ obs_desc,
                                                 const int32_t* __restrict__ win_of_kf, const float* __restrict__ poses,
                                                 const float2* __restrict__ kp_pool, const float* __restrict__ pos, TriParams k,
                                                 float max_mean_error, uint8_t* __restrict__ flag)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int o0 = obs_ptr[p], o1 = obs_ptr[p + 1];
    bool local = false;
    if (alive[p] != 0)
        for (int o = o0; o < o1; o++) local = local || win_of_kf[obs_kf[o]] >= 0;      // :398-408
    uint8_t f = 0;
    if (local) {
        const float X[3] = {pos[3 * (size_t)p], pos[3 * (size_t)p + 1], pos[3 * (size_t)p + 2]};
        const float err = point_error_sum_f32(k, poses, obs_kf, kp_pool, obs_desc, X, o0, o1, nullptr);
        float mean;
        f = point_cull_rule_f32(err, o1 - o0, max_mean_error, &mean) ? 3 : 2;          // :420
    }
    flag[p] = f;
}

// out: [0] selected, [1] local, then the selected slots [P], then their positions [P][3] (as 32-bit words)
__global__ __launch_bounds__(1024) void k_kf_compact(int P, const uint8_t* __restrict__ flag, const float* __restrict__ pos,
                                                     int32_t* __restrict__ out)
{
    int32_t* list = out + 2;
    float* xyz = (float*)(out + 2 + P);
    int carry = 0, nlocal = 0;
    for (int base = 0; base < P; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const int f = i < P ? flag[i] : 0;
        nlocal += (f >> 1) & 1;
        int tot;
        const int off = carry + rs_block_exclusive_scan(f & 1, &tot);
        if (f & 1) {
            list[off] = i;
#pragma unroll
            for (int c = 0; c < 3; c++) xyz[3 * (size_t)off + c] = pos[3 * (size_t)i + c];
        }
        carry += tot;
    }
    int tl;
    (void)rs_block_exclusive_scan(nlocal, &tl);
    if (threadIdx.x == 0) { out[0] = carry; out[1] = tl; }
}

void rs_kf_launch_reanchor(rs_context* ctx, int P, const uint8_t* d_alive, const int32_t* d_obs_ptr, const int32_t* d_obs_kf,
                           const int32_t* d_win_of_kf, const float* d_before, const float* d_poses, float* d_pos, uint8_t* d_sel,
                           int32_t* d_out)
{
    {
        rs_prof_scope ps(ctx, "KF1_map_reanchor");
        hipLaunchKernelGGL(k_kf_reanchor, dim3((P + 255) / 256), dim3(256), 0, ctx->stream, P, d_alive, d_obs_ptr, d_obs_kf, d_win_of_kf,
                           d_before, d_poses, d_pos, d_sel);
    }
    rs_prof_scope ps(ctx, "KF3_map_compact");
    hipLaunchKernelGGL(k_kf_compact, dim3(1), dim3(1024), 0, ctx->stream, P, d_sel, d_pos, d_out);
}

void rs_kf_launch_cull(rs_context* ctx, int P, const uint8_t* d_alive, const int32_t* d_obs_ptr, const int32_t* d_obs_kf,
                       const int32_t* d_obs_desc, const int32_t* d_win_of_kf, const float* d_poses, const float* d_kp_pool,
                       const float* d_pos, const float h_intrinsics[4], float max_mean_error, uint8_t* d_sel, int32_t* d_out)
{
    const TriParams k = {h_intrinsics[0], h_intrinsics[1], h_intrinsics[2], h_intrinsics[3], 0.f, 0.f};
    {
        rs_prof_scope ps(ctx, "KF2_map_cull");
        hipLaunchKernelGGL(k_kf_cull, dim3((P + 255) / 256), dim3(256), 0, ctx->stream, P, d_alive, d_obs_ptr, d_obs_kf, d_obs_desc,
                           d_win_of_kf, d_poses, (const float2*)d_kp_pool, d_pos, k, max_mean_error, d_sel);
    }
    rs_prof_scope ps(ctx, "KF3_map_compact");
    hipLaunchKernelGGL(k_kf_compact, dim3(1), dim3(1024), 0, ctx->stream, P, d_sel, d_pos, d_out);
}
