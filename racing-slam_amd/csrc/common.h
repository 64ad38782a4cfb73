// common.h — internal declarations shared by the HIP translation units of librsgpu.so.
// gfx950 (MI355X) only: 64-lane wavefronts, no portability layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/rsgpu.h"
#include "dev_array.h"

#define RS_WAVE 64

struct rs_prof_slot {
    char name[32];
    int launches;
    std::vector<hipEvent_t> ev;   // pairs (start, stop)
};

// grow-only bump arena (device or pinned host memory); slabs that became too small are retired and freed at the
// next reset, after the stream has drained
struct rs_arena {
    char* base = nullptr;
    size_t cap = 0, used = 0;
    std::vector<void*> retired;
};
struct rs_pending_download { const void* pinned; void* user; size_t bytes; };

struct rs_context {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // grow-only device workspace (never freed inside an enqueue path)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    // "known zero" region of the workspace (the landmark grouping's histogram / cursors of the last bundle adjustment, left
    // at zero by its finalize kernel) and the highest workspace byte any OTHER caller may have written since (rs_workspace)
    int32_t* grp_zero_ptr = nullptr;
    int grp_zero_n = 0;
    size_t ws_dirty_hi = 0;
    // pinned host scratch for small result read-back
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    // staging pool of the boundary (rs_stage_*): inputs flattened by a shim travel host -> pinned -> device with
    // asynchronous copies on the context stream; outputs come back the same way
    rs_arena stage_dev, stage_pin;
    std::vector<rs_pending_download> stage_down;
    // profiling
    bool prof_on = false;
    std::vector<rs_prof_slot> prof;
    // RCCL (loaded with dlopen; see comm.hip)
    void* comm = nullptr;
    int n_ranks = 1;
    int rank = 0;
    // in-process group of contexts (rs_comm_init_local): the same exchange step without RCCL
    struct rs_local_group* local = nullptr;
    // cached BA graph / buffers live in ba.hip
    void* ba_cache = nullptr;
    // per-iteration record of the last rs_bundle_adjust (points into the pinned block; rs_ba_get_trace)
    const void* ba_trace = nullptr;
    int ba_trace_n = 0;
    int ba_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // rs_ba_get_stats
    int ba_item = 0;                    // landmarks per item of a single solve: 0 = by window size (40 / 64), or 32 / 40 / 64
    int ba_batch_item = 0;              // landmarks per item of rs_bundle_adjust_batch's grid mode: 0 = default (32), or 32 / 40 / 64
    int ba_band_mode = 0;               // blocked reduced solve: 0 = the banded factorisation (two-sided) when S is block-banded, 1 = never, 2 = banded in one workgroup
    int ba_s_replicas = 0;              // replicas of S on the local-window path (0 = library default; "ba_s_replicas")
    int ba_handoff_timeout_us = 4000;   // fused K7 + K8 launch: how long a K8 workgroup waits for its hand-off word ("ba_handoff_timeout_us")
    const double* ba_cams = nullptr;    // cameras after the last rs_bundle_adjust, mirrored in the pinned block
    int ba_cams_n = 0;
    // speculative trust-region radii per BA round (0 = library default; rs_context_set_int "ba_speculative_sets")
    int ba_sets = 0;
    int n_cu = 256;                     // compute units of the device
    int ba_fuse_mode = 0;               // local-window BA: 0 = K7 + K8 in one launch when this is the only solve in flight, 1 = never,
                                        // 2 = K7 + K8 in one launch wherever possible, 3 = the whole round (K5 + K7 + K8) wherever possible
    int k2_mode = 0;                    // rs_reproj_match: 0 = eight lanes per map point where the KD-tree fits in LDS, 1 = always one lane per point
    int k2_grid = 1;                    // rs_reproj_match under k2_mode 0: 1 = the cell-grid kernel where the view carries a usable grid, 0 = never
    int ba_imu_mode = 0;                // inertial solves: 0 = z blocks eliminated around the LDS K7 where possible, 1 = always the N x N blocked solve
    int ba_batch_mode = 0;              // rs_bundle_adjust_batch: 0 = one grid for all windows where possible, 1 = lanes only
    int bow_score_mode = 0;             // rs_bow_database_score: 0 = the query's dense word table, 1 = binary search in its sorted words
    int loop_verify_streams = 0;        // rs_map_verify_loop: 0 = one forked child context per candidate, 1 = every candidate's chain on the context stream
    int gftt_round_launches = 12;       // rs_detect_features: gftt_round launches before the finisher, 0 .. 12 (= GFTT_ROUNDS, gftt.hip)
    // child contexts of rs_bundle_adjust_batch (own stream / workspace each), created on first use
    std::vector<rs_context*> batch_lanes;
    std::vector<hipStream_t> batch_streams;
    // proposal table of rs_reproj_match: persistent, always left at all-ones by the accept tail
    rs_dev_array<unsigned long long> prop;
    hipEvent_t sync_ev = nullptr;       // rs_context_wait_for: "everything enqueued on this context so far"
    void* tri_pin = nullptr;            // pinned in / out block + completion flag of rs_triangulate_host's one-launch path
    int tri_ticket = 0;
    rs_dev_array<uint2> k1_top;         // [batch][nq] {best, second} packed keys of rs_match_descriptors; all-ones between calls
};

// A frame's keypoints, descriptors and flattened KD-tree on the device (frame.hip: built on the host and uploaded by
// rs_frame_create, or filled from device arrays by rs_frame_assign_device).
struct rs_frame {
    rs_context* ctx = nullptr;
    int n = 0;
    rs_dev_block block;                 // every device array below but the grid
    rs_pin_block pin;                   // h_n
    float* d_kp = nullptr; uint8_t* d_desc = nullptr; int32_t* d_kd = nullptr;   // node_kp | left | right, stride n
    uint8_t* d_matched = nullptr;
    void* d_packed = nullptr;           // {x, y, left, right}[n] + keypoint[n]: what K2 stages in LDS (rs_kdtree_pack layout)
    int kd_root = -1;
    // rs_frame_create_device: every buffer above holds `cap` keypoints and is refilled by rs_frame_assign_device
    int cap = 0;                        // 0 = built by rs_frame_create: exactly n, not assignable
    uint32_t* d_rank = nullptr;         // [cap] rank_x | rank_y << 16 of the last assign
    int32_t* d_n = nullptr;             // [1] n of the last assign
    int32_t* h_n = nullptr;             // pinned word the one read-back per assign lands in
    // Frame::m_map_matches (frame_matches.hip): point slot matched by keypoint i or -1; [cap], or [n] after rs_frame_create
    int32_t* d_kp_point = nullptr;
    // the keypoints in K2's cell grid (rs_frame_grid): made when a match first asks for it, since only the match knows the
    // image size; grow-only, rebuilt after every assign
    rs_dev_array<unsigned char> grid;
    int grid_w = 0, grid_h = 0;
    bool grid_built = false;            // the grid holds this frame's keypoints for grid_w x grid_h
    bool finite = false;                // every keypoint coordinate is known to be finite: the only thing a grid over this library's own tree needs
};
// frame.hip: the frame's cell grid for an image of width x height in *d_grid, or null where the frame has none (see `finite`)
int rs_frame_grid(rs_context* ctx, rs_frame* f, int width, int height, const void** d_grid);

int rs_fail(rs_context* ctx, int code, const char* fmt, ...);
// the whole of a *_destroy whose object holds only owners (dev_array.h): make the device current, drain the stream, delete
template <class T>
static inline int rs_drain_and_delete(T* o)
{
    if (!o) return RS_OK;
    (void)hipSetDevice(o->ctx->device);
    (void)hipStreamSynchronize(o->ctx->stream);
    delete o;
    return RS_OK;
}

// reproj_match.hip: the cell grids K2 may use in place of its walk, remembered per process (a view travels between contexts).
// rs_k2_grid_enqueue launches a build on the context stream without waiting for its verdict; a caller that knows the tree to be
// this library's own over finite coordinates remembers the grid itself.
int rs_k2_grid_enqueue(rs_context* ctx, int n, int kd_root, const void* d_packed, int width, int height, void* d_grid, bool validate, bool* built);
void rs_k2_grid_remember(const void* d_grid, int n);
void rs_k2_grid_forget(const void* d_grid);
bool rs_k2_grid_usable(const void* d_grid, int n);

// What loop.hip reads of an rs_map (map.hip: rs_map_loop_sync brings the device image up to date first).
struct rs_map_loop_view {
    rs_context* ctx = nullptr;              // the map's context
    int n_kf = 0, n_points = 0;
    const uint8_t* d_pool = nullptr;        // [pool rows][32]
    const float* d_kp_pool = nullptr;       // [pool rows][2]
    const int32_t* d_kp_point = nullptr;    // [pool rows] point slot of the keypoint or -1
    const float* d_pos = nullptr;           // [points][3]
    const float* d_centres = nullptr;       // [key frames][3]
};
int rs_map_loop_sync(rs_map* m, rs_map_loop_view* out);
rs_context* rs_map_context(const rs_map* m);
// key frame kf of the mirror: keypoints, first pool row, keypoints with a map match; false = no such key frame
bool rs_map_loop_keyframe(const rs_map* m, int kf, int* n, int* pool_row, int* n_matched);

// What map_fuse.hip reads and writes of an rs_map (map.hip: rs_map_fuse_sync).  The image's key-frame tables are the fuse's working
// tables: the caller marks them dirty before its first launch.
struct MapMirror;
struct rs_map_fuse_view {
    rs_context* ctx = nullptr;
    MapMirror* mirror = nullptr;
    void** scratch = nullptr;               // rs_map::fuse
    const float* d_pos = nullptr; const uint8_t* d_alive = nullptr;
    const int32_t *d_obs_ptr = nullptr, *d_obs_kf = nullptr, *d_obs_desc = nullptr;
    const float* d_centres = nullptr; const uint8_t* d_pool = nullptr; const float* d_kp_pool = nullptr;
    int32_t* d_kp_point = nullptr;
    size_t n_obs = 0, pool_rows = 0;
};
int rs_map_fuse_sync(rs_map* m, int sync, rs_map_fuse_view* out);
void rs_map_fuse_release(void* scratch);      // map_fuse.hip
// frame.hip: a device-built frame refilled from n keypoints / descriptor rows on the device, n known to the host (d_count[0] == n):
// the three launches of rs_frame_assign_device without its synchronisation
int rs_frame_assign_enqueue(rs_context* ctx, rs_frame* f, const float* d_pt, const int32_t* d_count, const uint8_t* d_desc, int n);

// What frame_matches.hip reads and writes of an rs_map (map.hip: rs_map_track_sync brings the device image up to date first).
struct rs_map_track_view {
    int n_kf = 0;                           // key frames
    rs_map_view mv;                         // the whole map as rs_reproj_match takes it (d_eligible: rs_map_launch_eligible's output)
    const uint8_t* d_alive = nullptr;       // [points]
    const uint8_t* d_consistent = nullptr;  // [points] MapPoint::track_consistent
    uint8_t* d_flag = nullptr;              // [points] bit 0 = the frame already matches the point; all zero between calls
    uint32_t* d_mark = nullptr;             // [points] scratch of the carry-over; all zero between calls
    double* d_gather_pts = nullptr;         // [8192][3] the refit's points ...
    float* d_gather_uv = nullptr;           // [8192][2] ... pixels ...
    int32_t* d_gather_n = nullptr;          // [1] ... and count (-1: too few matches)
    int32_t* d_out = nullptr;               // rs_reproj_match's outputs for a frame of n_out_kp keypoints (rs_map_match's layout)
};
int rs_map_track_sync(rs_map* m, int n_keypoints, rs_map_track_view* out);
void rs_map_launch_eligible(rs_map* m, int required_kf);      // K2p over the synced image into mv.d_eligible, on the context stream
// refine_pose.hip: K11 on device arrays whose count *d_n is read on the device (<= 0: no solve).  *h_n_used = that count.
int rs_refine_pose_device_n(rs_context* ctx, double h_camera[6], const double* d_points, const float* d_uv, const int32_t* d_n, int max_n,
                            const float h_intrinsics[4], int kind, const double h_predicted[9], double sigma_radians,
                            const double h_prev_pose[6], const double h_prev_velocity[3], const double h_prev_bias[6],
                            const rs_imu_factor* h_delta, const double h_gravity[3], double h_velocity[3],
                            const rs_ba_options* options, rs_ba_summary* h_summary, int* h_n_used);

// map_keyframe.hip: the per-key-frame stages over the resident image (P > 0 slots; d_sel [P] selection bytes; d_out 2 + 4 P words:
// selected count, local count, the selected slots ascending, their positions).  Two launches each on the context stream.
void rs_kf_launch_reanchor(rs_context* ctx, int P, const uint8_t* d_alive, const int32_t* d_obs_ptr, const int32_t* d_obs_kf,
                           const int32_t* d_win_of_kf, const float* d_before, const float* d_poses, float* d_pos, uint8_t* d_sel,
                           int32_t* d_out);
void rs_kf_launch_cull(rs_context* ctx, int P, const uint8_t* d_alive, const int32_t* d_obs_ptr, const int32_t* d_obs_kf,
                       const int32_t* d_obs_desc, const int32_t* d_win_of_kf, const float* d_poses, const float* d_kp_pool,
                       const float* d_pos, const float h_intrinsics[4], float max_mean_error, uint8_t* d_sel, int32_t* d_out);

#define RS_HIP(ctx, call)                                                                  \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess)                                                             \
            return rs_fail((ctx), RS_ERR_HIP, "%s failed: %s (%s:%d)", #call,              \
                           hipGetErrorString(e__), __FILE__, __LINE__);                    \
    } while (0)

int rs_k1_reserve(rs_context* ctx, size_t entries);   // hamming.hip: K1's top-2 table for `entries` keys (grow-only)
// workspace: returns a device pointer with at least `bytes` bytes, 256-B aligned.
int rs_workspace(rs_context* ctx, size_t bytes, void** out);
int rs_workspace_quiet(rs_context* ctx, size_t bytes, void** out);   // does not mark the bytes as possibly written (ba.hip keeps its own account)
int rs_pinned(rs_context* ctx, size_t bytes, void** out);
// a per-call block cut by a layout (carve.h): sized on a null carver, fetched with `get` (one of the three above), placed
template <class L>
static inline int rs_carve_from(rs_context* ctx, int (*get)(rs_context*, size_t, void**), L&& layout)
{
    rs_carve size, place;
    layout(size);
    const int rc = get(ctx, size.bytes(), (void**)&place.base);
    if (!rc) layout(place);
    return rc;
}
// hipFuncSetAttribute(fn, MaxDynamicSharedMemorySize, bytes), but only when `bytes` exceeds what was already set for
// `fn` in this process: the attribute is sticky and the driver call costs microseconds of host time per launch.
hipError_t rs_lds_attr(const void* fn, size_t bytes);


// profiling brackets around a kernel launch
void rs_prof_start(rs_context* ctx, const char* name);
void rs_prof_stop(rs_context* ctx, const char* name);

struct rs_prof_scope {
    rs_context* c;
    const char* n;
    rs_prof_scope(rs_context* ctx, const char* name) : c(ctx), n(name) { if (c->prof_on) rs_prof_start(c, n); }
    ~rs_prof_scope() { if (c->prof_on) rs_prof_stop(c, n); }
};

// Exclusive prefix sum of one int per thread over the workgroup (any size up to 1024, multiple of 64);
// returns this thread's offset and the workgroup total.
__device__ __forceinline__ int rs_block_exclusive_scan(int v, int* total)
{
    __shared__ int rs_scan_w[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(x, off, 64);
        if (lane >= off) x += t;
    }
    if (lane == 63) rs_scan_w[wave] = x;
    __syncthreads();
    int pre = 0, tot = 0;
    for (int w = 0; w < nw; w++) { const int c = rs_scan_w[w]; if (w < wave) pre += c; tot += c; }
    __syncthreads();
    *total = tot;
    return pre + x - v;
}

// sum all-reduce of f64 on the context stream over the attached communicator (RCCL or the in-process group);
// no-op without one
int rs_allreduce_f64(rs_context* ctx, double* d_buf, size_t count, bool is_max);
int rs_allreduce_min_u64(rs_context* ctx, unsigned long long* d_buf, size_t count);   // element-wise minimum of unsigned 64-bit keys
static inline bool rs_comm_active(const rs_context* ctx) { return ctx->comm != nullptr || ctx->local != nullptr; }

