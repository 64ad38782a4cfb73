// frame_matches.hip — the tail of Tracker::track on the device (reference src/Tracker.cpp:83-86): a frame's match table
// (Frame::m_map_matches, keypoint -> point slot or -1) lives in rs_frame::d_kp_point, and the three stages that read and
// write it run against the resident map with no host walk over map objects and no list traffic:
//
//   k_fm_add       Frame::add_map_match (src/Frame.cpp:80-102) for a whole list, equal to applying it entry by entry.  In a
//                  table whose points are unique (every writer here keeps them so) the sequential rule has a closed form:
//                  keypoint k ends with the point of the LAST entry that names k, if that entry is also the last one
//                  that names its point, else with nothing; a keypoint no entry names keeps its point unless some entry
//                  names that point.  One workgroup: last entry per keypoint by atomicMax in LDS, last entry per point in
//                  an LDS hash table keyed through the list itself, then one pass over the table.
//   k_fm_carry     Tracker::track_from_last_frame (:197-230).  One workgroup over the inlier list: the :209 gate against
//                  the map, the count gate, then acceptance in list order.  A list without repeated keypoints or points
//                  (what the tracker produces) is accepted in parallel; repeats are found by first-claim tables (LDS per
//                  keypoint, rs_map's mark array per point) and send the walk to one lane, which applies :222-228 literally.
//   k_fm_gather    optimization::refine_pose's walk over Frame::map_matches() (the shim's Optimization.cpp:70-81): an
//                  ordered compaction of the table into K11's point / pixel arrays and a device-side count.
//   k_fm_flags, k_fm_scatter     match_with_last_key_frame / match_with_map (:232-248) around rs_reproj_match: the
//                  keypoint-matched bytes and the map's point flags from the table, and the accepted pairs back into it.
//
// A dead point slot in a table (the reference: a dangling MapPoint*, undefined behaviour) counts as a match of its
// keypoint (Frame::is_matched) but is never a carry-over candidate and never enters the refit.
#include "common.h"

#define FM_THREADS 1024
#define FM_MAX 8192                 // keypoints per frame and entries per list (frame.hip's FRAME_MAX_POINTS)
#define FM_PER (FM_MAX / FM_THREADS)

__device__ __forceinline__ int fm_count(const int32_t* d_count, int max_n)
{
    if (!d_count) return max_n;
    const int c = d_count[0];
    return c < 0 ? 0 : (c > max_n ? max_n : c);
}

__device__ __forceinline__ uint32_t fm_hash(int32_t p) { return (uint32_t)p * 2654435761u >> 7; }

// slot = the largest entry index whose point is the slot's key; the key of a slot is pt[its value] and never changes
__device__ __forceinline__ void fm_hash_insert(int32_t* hash, uint32_t hmask, const int32_t* __restrict__ pt, int32_t p, int i)
{
    uint32_t h = fm_hash(p) & hmask;
    while (true) {                                   // (at most half the slots are ever taken)
        int cur = __atomic_load_n(&hash[h], __ATOMIC_RELAXED);
        if (cur < 0) {
            cur = atomicCAS(&hash[h], -1, i);
            if (cur < 0) return;
        }
        if (pt[cur] == p) { atomicMax(&hash[h], i); return; }
        h = (h + 1) & hmask;
    }
}

__device__ __forceinline__ int fm_hash_find(const int32_t* hash, uint32_t hmask, const int32_t* __restrict__ pt, int32_t p)
{
    uint32_t h = fm_hash(p) & hmask;
    int cur;
    while ((cur = hash[h]) >= 0) {
        if (pt[cur] == p) return cur;
        h = (h + 1) & hmask;
    }
    return -1;
}

// dynamic LDS: last entry per keypoint [n_kp] | hash [hmask + 1]
__global__ __launch_bounds__(FM_THREADS) void k_fm_add(int n_kp, int32_t* __restrict__ table, const int32_t* __restrict__ kp,
                                                      const int32_t* __restrict__ pt, const int32_t* __restrict__ d_count, int max_n,
                                                      uint32_t hmask)
{
    extern __shared__ int32_t fm_lds[];
    int32_t* lastk = fm_lds, *hash = fm_lds + n_kp;
    const int n = fm_count(d_count, max_n), tid = threadIdx.x;
    for (int k = tid; k < n_kp; k += FM_THREADS) lastk[k] = -1;
    for (uint32_t h = tid; h <= hmask; h += FM_THREADS) hash[h] = -1;
    __syncthreads();
    for (int i = tid; i < n; i += FM_THREADS) {
        const int32_t k = kp[i], p = pt[i];
        if ((uint32_t)k >= (uint32_t)n_kp || p < 0) continue;        // not an entry
        atomicMax(&lastk[k], i);
        fm_hash_insert(hash, hmask, pt, p, i);
    }
    __syncthreads();
    for (int k = tid; k < n_kp; k += FM_THREADS) {
        const int t = lastk[k];
        if (t >= 0) {
            const int32_t p = pt[t];
            table[k] = fm_hash_find(hash, hmask, pt, p) == t ? p : -1;
        } else {
            const int32_t p = table[k];
            if (p >= 0 && fm_hash_find(hash, hmask, pt, p) >= 0) table[k] = -1;
        }
    }
}

#define FM_EXISTING 0xFFFFFFFFu         // d_mark: the point is in next's table
#define FM_CLAIM(i) (0xFFFFFFFEu - (uint32_t)(i))      // ... or claimed by candidate i (atomicMax: the first one keeps it)

struct FmCarryEntry { int kp_next; int32_t point; };

// entry i of the list: next's keypoint and the point prev holds for it, or point < 0 when it is no candidate (:204-214)
__device__ __forceinline__ FmCarryEntry fm_carry_entry(int i, int P, const uint8_t* __restrict__ alive, const int32_t* __restrict__ obs_ptr,
                                                       const uint8_t* __restrict__ consistent, const int32_t* __restrict__ prev_table, int n_prev,
                                                       int n_next, const int32_t* __restrict__ prev_index,
                                                       const int32_t* __restrict__ inlier_index, int max_n)
{
    FmCarryEntry e{inlier_index ? inlier_index[i] : i, -1};
    if ((uint32_t)e.kp_next >= (uint32_t)(n_next < max_n ? n_next : max_n)) return e;
    const int32_t kq = prev_index[e.kp_next];
    if ((uint32_t)kq >= (uint32_t)n_prev) return e;
    const int32_t p = prev_table[kq];
    if ((uint32_t)p >= (uint32_t)P || !alive[p]) return e;           // unmatched, or a dead slot: no candidate
    if (obs_ptr[p + 1] - obs_ptr[p] < 2 && !consistent[p]) return e;  // :209
    e.point = p;
    return e;
}

__global__ __launch_bounds__(FM_THREADS) void k_fm_carry(int P, const uint8_t* __restrict__ alive, const int32_t* __restrict__ obs_ptr,
                                                        const uint8_t* __restrict__ consistent, uint32_t* __restrict__ mark,
                                                        const int32_t* __restrict__ prev_table, int n_prev, int32_t* __restrict__ next_table,
                                                        int n_next, const int32_t* __restrict__ prev_index,
                                                        const int32_t* __restrict__ inlier_index, const int32_t* __restrict__ d_count, int max_n,
                                                        int min_points, int32_t* __restrict__ stats)
{
    __shared__ int firstk[FM_MAX];
    __shared__ uint8_t state[FM_MAX];       // 0 no candidate, 1 candidate that next's table already refuses, 2 live
    __shared__ int repeats;
    const int n = fm_count(d_count, max_n), tid = threadIdx.x;
    if (tid == 0) repeats = 0;
    for (int k = tid; k < n_next; k += FM_THREADS) {
        firstk[k] = 0x7FFFFFFF;
        const int32_t p = next_table[k];
        if ((uint32_t)p < (uint32_t)P) mark[p] = FM_EXISTING;
    }
    int mine = 0;
    for (int i = tid; i < n; i += FM_THREADS) {
        const FmCarryEntry e = fm_carry_entry(i, P, alive, obs_ptr, consistent, prev_table, n_prev, n_next, prev_index, inlier_index, max_n);
        state[i] = e.point >= 0 ? 1 : 0;
        mine += e.point >= 0 ? 1 : 0;
    }
    int candidates, accepted = 0;
    rs_block_exclusive_scan(mine, &candidates);       // (its barriers order the marks and states above)
    if (candidates >= min_points) {                   // :216-219
        for (int i = tid; i < n; i += FM_THREADS) {
            if (!state[i]) continue;
            const FmCarryEntry e = fm_carry_entry(i, P, alive, obs_ptr, consistent, prev_table, n_prev, n_next, prev_index, inlier_index, max_n);
            if (next_table[e.kp_next] >= 0 || __atomic_load_n(&mark[e.point], __ATOMIC_RELAXED) == FM_EXISTING) continue;      // :223, by the table as it came
            state[i] = 2;
            atomicMin(&firstk[e.kp_next], i);
            atomicMax(&mark[e.point], FM_CLAIM(i));
        }
        __syncthreads();
        for (int i = tid; i < n; i += FM_THREADS) {
            if (state[i] != 2) continue;
            const FmCarryEntry e = fm_carry_entry(i, P, alive, obs_ptr, consistent, prev_table, n_prev, n_next, prev_index, inlier_index, max_n);
            if (firstk[e.kp_next] != i || __atomic_load_n(&mark[e.point], __ATOMIC_RELAXED) != FM_CLAIM(i)) repeats = 1;
        }
        __syncthreads();
        mine = 0;
        if (!repeats) {
            for (int i = tid; i < n; i += FM_THREADS) {
                if (state[i] != 2) continue;
                const FmCarryEntry e = fm_carry_entry(i, P, alive, obs_ptr, consistent, prev_table, n_prev, n_next, prev_index, inlier_index, max_n);
                next_table[e.kp_next] = e.point;
                mine++;
            }
        } else if (tid == 0) {
            // a keypoint or a point twice among the live candidates: :222-228 as written, one entry after the other
            for (int i = 0; i < n; i++) {
                if (state[i] != 2) continue;
                const FmCarryEntry e = fm_carry_entry(i, P, alive, obs_ptr, consistent, prev_table, n_prev, n_next, prev_index, inlier_index, max_n);
                if (next_table[e.kp_next] >= 0 || mark[e.point] == FM_EXISTING) continue;
                next_table[e.kp_next] = e.point;
                mark[e.point] = FM_EXISTING;
                mine++;
            }
        }
        rs_block_exclusive_scan(mine, &accepted);
    }
    __syncthreads();
    // the mark array goes back to all-zero: every point of next's table (old and new) and every candidate's
    for (int k = tid; k < n_next; k += FM_THREADS) {
        const int32_t p = next_table[k];
        if ((uint32_t)p < (uint32_t)P) mark[p] = 0;
    }
    for (int i = tid; i < n; i += FM_THREADS) {
        if (!state[i]) continue;
        const FmCarryEntry e = fm_carry_entry(i, P, alive, obs_ptr, consistent, prev_table, n_prev, n_next, prev_index, inlier_index, max_n);
        mark[e.point] = 0;
    }
    if (tid == 0 && stats) { stats[0] = candidates; stats[1] = accepted; }
}

// thread t owns keypoints t * per .. ; one scan carries both counts (kept | matched << 16, each <= 8192)
__global__ __launch_bounds__(FM_THREADS) void k_fm_gather(int n_kp, const int32_t* __restrict__ table, const float2* __restrict__ kp, int P,
                                                         const uint8_t* __restrict__ alive, const int32_t* __restrict__ obs_ptr,
                                                         const float* __restrict__ pos, int min_matches, double* __restrict__ out_pts,
                                                         float2* __restrict__ out_uv, int32_t* __restrict__ out_n)
{
    const int per = (n_kp + FM_THREADS - 1) / FM_THREADS, k0 = threadIdx.x * per;
    int32_t pt[FM_PER];
    int run = 0;
#pragma unroll
    for (int q = 0; q < FM_PER; q++) {
        pt[q] = -1;
        const int k = k0 + q;
        if (q >= per || k >= n_kp) continue;
        const int32_t p = table[k];
        if (p < 0) continue;
        run += 0x10000;                                                                 // Frame::num_map_matches
        if ((uint32_t)p < (uint32_t)P && alive[p] && obs_ptr[p + 1] - obs_ptr[p] >= 2) { pt[q] = p; run++; }   // MIN_OBSERVATIONS_TO_OPTIMIZE
    }
    int total;
    int at = rs_block_exclusive_scan(run, &total) & 0xFFFF;
    if (threadIdx.x == 0) out_n[0] = (total >> 16) < min_matches ? -1 : (total & 0xFFFF);
#pragma unroll
    for (int q = 0; q < FM_PER; q++) {
        if (pt[q] < 0) continue;
        const float* x = pos + 3 * (size_t)pt[q];
        out_pts[3 * (size_t)at] = (double)x[0]; out_pts[3 * (size_t)at + 1] = (double)x[1]; out_pts[3 * (size_t)at + 2] = (double)x[2];
        out_uv[at] = kp[k0 + q];
        at++;
    }
}

// set != 0: matched[k] = Frame::is_matched(k) and bit 0 of the map's flag byte of every matched point; else the bits cleared
__global__ __launch_bounds__(256) void k_fm_flags(int n_kp, const int32_t* __restrict__ table, int P, uint8_t* __restrict__ matched,
                                                 uint8_t* __restrict__ flag, int set)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_kp) return;
    const int32_t p = table[k];
    if (set) matched[k] = p >= 0 ? 1 : 0;
    if ((uint32_t)p >= (uint32_t)P) return;
    unsigned int* w = (unsigned int*)(flag + (p & ~3));
    const unsigned int msk = 1u << (8 * (p & 3));
    if (set) atomicOr(w, msk); else atomicAnd(w, ~msk);
}

// the accepted pairs are disjoint from the table and unique on both sides (replace = 0): a plain scatter
__global__ __launch_bounds__(256) void k_fm_scatter(int n_kp, const int32_t* __restrict__ match_kp, const int32_t* __restrict__ match_point,
                                                   const int32_t* __restrict__ count, int32_t* __restrict__ table)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = count[0] < n_kp ? count[0] : n_kp;
    if (i >= n) return;
    const int32_t k = match_kp[i];
    if ((uint32_t)k < (uint32_t)n_kp) table[k] = match_point[i];
}

// ---------------------------------------------------------------------- host
static int fm_frame_ok(rs_context* ctx, const rs_frame* f, const char* what)
{
    if (!ctx || !f || f->ctx != ctx) return RS_ERR_INVALID;
    if (f->n > FM_MAX) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "%s: %d keypoints, at most %d", what, f->n, FM_MAX);
    return RS_OK;
}

extern "C" int rs_frame_matches_clear(rs_context* ctx, rs_frame* f)
{
    if (!ctx || !f || f->ctx != ctx) return RS_ERR_INVALID;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t m = f->cap > 0 ? (size_t)f->cap : (f->n > 0 ? (size_t)f->n : 1);
    RS_HIP(ctx, hipMemsetAsync(f->d_kp_point, 0xFF, sizeof(int32_t) * m, ctx->stream));
    return RS_OK;
}

extern "C" int rs_frame_matches_add(rs_context* ctx, rs_frame* f, const int32_t* d_kp, const int32_t* d_point, const int32_t* d_count, int max_n)
{
    int rc = fm_frame_ok(ctx, f, "rs_frame_matches_add");
    if (rc) return rc;
    if (max_n < 0) return rs_fail(ctx, RS_ERR_INVALID, "rs_frame_matches_add: negative max_n");
    if (max_n > FM_MAX) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "rs_frame_matches_add: max_n %d, at most %d", max_n, FM_MAX);
    if (max_n == 0 || f->n == 0) return RS_OK;
    if (!d_kp || !d_point) return rs_fail(ctx, RS_ERR_INVALID, "rs_frame_matches_add: null list");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t slots = 64;
    while (slots < 2 * (uint32_t)max_n) slots *= 2;
    const size_t lds = sizeof(int32_t) * ((size_t)f->n + slots);
    if (lds > 48 * 1024) RS_HIP(ctx, rs_lds_attr((const void*)k_fm_add, lds));
    rs_prof_scope ps(ctx, "KM_matches_add");
    hipLaunchKernelGGL(k_fm_add, dim3(1), dim3(FM_THREADS), lds, ctx->stream, f->n, f->d_kp_point, d_kp, d_point, d_count, max_n, slots - 1);
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_frame_matches_download(rs_context* ctx, const rs_frame* f, int32_t* h_kp_point, int* h_count)
{
    if (!ctx || !f || f->ctx != ctx) return RS_ERR_INVALID;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> tab((size_t)f->n);
    if (f->n > 0) RS_HIP(ctx, hipMemcpyAsync(tab.data(), f->d_kp_point, sizeof(int32_t) * (size_t)f->n, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int c = 0;
    for (const int32_t p : tab) c += p >= 0 ? 1 : 0;
    if (h_kp_point && f->n > 0) memcpy(h_kp_point, tab.data(), sizeof(int32_t) * (size_t)f->n);
    if (h_count) *h_count = c;
    return RS_OK;
}

extern "C" int rs_map_carry_matches(rs_context* ctx, rs_map* m, const rs_frame* prev, rs_frame* next, const int32_t* d_prev_index,
                                    const int32_t* d_inlier_index, const int32_t* d_count, int max_n, int min_points, int32_t* d_stats)
{
    if (!ctx || !m || rs_map_context(m) != ctx) return RS_ERR_INVALID;
    int rc = fm_frame_ok(ctx, prev, "rs_map_carry_matches");
    if (rc) return rc;
    if ((rc = fm_frame_ok(ctx, next, "rs_map_carry_matches"))) return rc;
    if (prev == next) return rs_fail(ctx, RS_ERR_INVALID, "rs_map_carry_matches: one frame twice");
    if (max_n < 0) return rs_fail(ctx, RS_ERR_INVALID, "rs_map_carry_matches: negative max_n");
    if (max_n > FM_MAX) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "rs_map_carry_matches: max_n %d, at most %d", max_n, FM_MAX);
    if (max_n > 0 && !d_prev_index) return rs_fail(ctx, RS_ERR_INVALID, "rs_map_carry_matches: null index list");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_map_track_view v;
    if ((rc = rs_map_track_sync(m, 0, &v))) return rc;
    if (v.mv.n_points == 0 || max_n == 0) {          // no point can be a candidate
        if (d_stats) RS_HIP(ctx, hipMemsetAsync(d_stats, 0, 2 * sizeof(int32_t), ctx->stream));
        return RS_OK;
    }
    rs_prof_scope ps(ctx, "KM_carry_matches");
    hipLaunchKernelGGL(k_fm_carry, dim3(1), dim3(FM_THREADS), 0, ctx->stream, v.mv.n_points, v.d_alive, v.mv.d_obs_ptr, v.d_consistent, v.d_mark,
                       (const int32_t*)prev->d_kp_point, prev->n, next->d_kp_point, next->n, d_prev_index, d_inlier_index, d_count, max_n,
                       min_points, d_stats);
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_map_refine_pose(rs_context* ctx, rs_map* m, const rs_frame* f, double h_camera[6], const float h_intrinsics[4],
                                  int min_matches, int kind, const double h_predicted[9], double sigma_radians,
                                  const double h_prev_pose[6], const double h_prev_velocity[3], const double h_prev_bias[6],
                                  const rs_imu_factor* h_delta, const double h_gravity[3], double h_velocity[3],
                                  const rs_ba_options* options, rs_ba_summary* h_summary, int* h_n_used)
{
    if (!ctx || !h_summary) return RS_ERR_INVALID;
    memset(h_summary, 0, sizeof *h_summary);         // a refused call leaves a zeroed summary too
    if (!m || rs_map_context(m) != ctx) return RS_ERR_INVALID;
    int rc = fm_frame_ok(ctx, f, "rs_map_refine_pose");
    if (rc) return rc;
    if (!h_camera || !h_intrinsics || !h_n_used) return rs_fail(ctx, RS_ERR_INVALID, "rs_map_refine_pose: null pointer");
    if (kind < 0 || kind > 2) return rs_fail(ctx, RS_ERR_INVALID, "kind must be 0, 1 or 2");
    *h_n_used = f->n == 0 && min_matches > 0 ? -1 : 0;
    if (f->n == 0) return RS_OK;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_map_track_view v;
    if ((rc = rs_map_track_sync(m, 0, &v))) return rc;
    {
        rs_prof_scope ps(ctx, "KM_refine_gather");
        hipLaunchKernelGGL(k_fm_gather, dim3(1), dim3(FM_THREADS), 0, ctx->stream, f->n, (const int32_t*)f->d_kp_point, (const float2*)f->d_kp,
                           v.mv.n_points, v.d_alive, v.mv.d_obs_ptr, v.mv.d_positions, min_matches, v.d_gather_pts, (float2*)v.d_gather_uv,
                           v.d_gather_n);
    }
    return rs_refine_pose_device_n(ctx, h_camera, v.d_gather_pts, v.d_gather_uv, v.d_gather_n, f->n, h_intrinsics, kind, h_predicted,
                                   sigma_radians, h_prev_pose, h_prev_velocity, h_prev_bias, h_delta, h_gravity, h_velocity, options,
                                   h_summary, h_n_used);
}

extern "C" int rs_map_match_frame(rs_context* ctx, rs_map* m, rs_frame* f, const float h_pose[16], const float h_intrinsics[4], int width,
                                  int height, int required_observer_kf, int max_distance, int* h_count)
{
    if (!ctx || !m || rs_map_context(m) != ctx || !h_pose || !h_intrinsics || !h_count) return RS_ERR_INVALID;
    int rc = fm_frame_ok(ctx, f, "rs_map_match_frame");
    if (rc) return rc;
    *h_count = 0;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    // every buffer is grown before the first launch, and the flag bits are cleared by the launch right behind the
    // eligibility kernel, whatever happens later: the flag table is all-zero between calls
    rs_map_track_view v;
    const int N = f->n;
    if ((rc = rs_map_track_sync(m, N, &v))) return rc;
    if (required_observer_kf >= v.n_kf) return rs_fail(ctx, RS_ERR_INVALID, "unknown key frame");
    const int P = v.mv.n_points;
    if (N == 0 || P == 0) return RS_OK;
    if ((rc = rs_stage_begin(ctx))) return rc;
    hipStream_t s = ctx->stream;
    const dim3 grid((N + 255) / 256);
    {
        rs_prof_scope ps(ctx, "KM_match_flags");
        hipLaunchKernelGGL(k_fm_flags, grid, dim3(256), 0, s, N, (const int32_t*)f->d_kp_point, P, f->d_matched, v.d_flag, 1);
    }
    rs_map_launch_eligible(m, required_observer_kf);
    {
        rs_prof_scope ps(ctx, "KM_match_unflag");
        hipLaunchKernelGGL(k_fm_flags, grid, dim3(256), 0, s, N, (const int32_t*)f->d_kp_point, P, f->d_matched, v.d_flag, 0);
    }
    int32_t* pk = v.d_out, *pd = pk + P, *pp = pd + P, *pdist = pp + N, *mkp = pdist + N, *mpt = mkp + N, *cnt = mpt + N;
    rs_frame_view fv{};
    memcpy(fv.pose, h_pose, sizeof fv.pose);
    fv.fx = h_intrinsics[0]; fv.fy = h_intrinsics[1]; fv.cx = h_intrinsics[2]; fv.cy = h_intrinsics[3];
    fv.width = width; fv.height = height; fv.n_keypoints = N;
    fv.d_keypoints = f->d_kp; fv.d_descriptors = f->d_desc; fv.d_kp_matched = f->d_matched;
    fv.d_kd_node_kp = f->d_kd; fv.d_kd_left = f->d_kd + N; fv.d_kd_right = f->d_kd + 2 * (size_t)N; fv.kd_root = f->kd_root;
    fv.d_kd_packed = f->d_packed;
    if ((rc = rs_frame_grid(ctx, f, width, height, &fv.d_kd_grid))) return rc;
    if ((rc = rs_reproj_match(ctx, &fv, &v.mv, 0, max_distance, pk, pd, pp, pdist, mkp, mpt, cnt))) return rc;
    {
        rs_prof_scope ps(ctx, "KM_match_scatter");
        hipLaunchKernelGGL(k_fm_scatter, grid, dim3(256), 0, s, N, (const int32_t*)mkp, (const int32_t*)mpt, (const int32_t*)cnt, f->d_kp_point);
    }
    RS_HIP(ctx, hipGetLastError());
    int32_t n_out = 0;
    if ((rc = rs_stage_download(ctx, cnt, sizeof(int32_t), &n_out))) return rc;
    if ((rc = rs_stage_sync(ctx))) return rc;
    *h_count = n_out;
    return RS_OK;
}
