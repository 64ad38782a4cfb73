// map.hip — the map, resident on the device across frames.
//
// The reference's map is a pointer graph on the host (Map owns MapPoint objects, each with an
// unordered_map<KeyFrame*, size_t> of observations; key frames own their descriptor matrices — reference
// src/Map.cpp:63-124, src/MapPoint.cpp, src/Frame.cpp:80-116), and MapMatcher::match walks ALL of it twice per frame
// (src/MapMatcher.cpp:165-175).  A drop-in that re-flattens and re-uploads that graph on every call spends 100x the
// kernel time doing so (bench.py `boundary`: 5.4 ms per match_map for a 45 us kernel).  rs_map keeps the flat form:
//
//   host mirror (this file)      per point: position, alive flag, observation list (key frame, keypoint) in insertion
//                                order; per key frame: pose, keypoints, keypoint -> point table (Frame::map_matches),
//                                row offset of its descriptors in the device pool.  O(1) updates, mirroring the calls
//                                the reference makes: create_point / remove_point / associate / disassociate /
//                                set_position / set_pose.
//   device image                 positions, alive flags, observation CSR (key frame, descriptor row), key-frame centres,
//                                descriptor pool (append only: a key frame's rows are uploaded ONCE).  Re-flattened from
//                                the mirror and uploaded only when the map changed since the last use — i.e. once per
//                                KEY FRAME, not per frame; positions / centres alone when only those moved (after BA).
//
// Point slots are never reused, so ascending slot = creation order = the reference's map order (Map::remove_point erases
// in place, src/Map.cpp:63-76), which is what decides ties between points (src/MapMatcher.cpp:95-97).  Observation order
// within a point = insertion order (the reference iterates an unordered_map: unspecified upstream).
//
// rs_frame (frame.hip) is the per-frame counterpart; a frame that becomes a key frame hands its descriptor rows and keypoints
// to the pools device-to-device.
#include <algorithm>

#include "common.h"
#include "map_mirror.h"

// (MapObs, MapKeyFrame and the mirror's fields and edits: map_mirror.h)
#define MAP_FIRST 1024                  // first capacity, in entries, of every array below that has no other (32 pool rows, 64 poses)
#define MAP_FIRST_POINTS 4096           // ... of the per-point arrays, in slots
#define MAP_FIRST_OBS 16384             // ... of the per-observation arrays

struct rs_map : MapMirror {
    rs_context* ctx = nullptr;
    // device image.  Per point slot, reserved together (map_reserve_points); d_flag and d_mark are all zero between calls, and
    // d_consistent and d_mark belong to the tracker's per-frame stages (frame_matches.hip):
    rs_dev_array<float> d_pos;
    rs_dev_array<int32_t> d_obs_ptr;
    rs_dev_array<uint8_t> d_alive, d_elig, d_flag, d_consistent;
    rs_dev_array<uint32_t> d_mark;
    rs_dev_array<int32_t> d_obs_kf, d_obs_desc;     // per observation, reserved together (map_reserve_obs)
    rs_dev_array<float> d_centres, d_poses;         // [KF][3]; [KF][16] the poses (hipMalloc: 16-byte aligned for load_pose), uploaded with the centres
    rs_dev_array<uint8_t> d_pool;                   // [pool rows][32] descriptors, append only
    rs_dev_array<float> d_kp_pool;                  // [pool rows][2] keypoints of the key frames, row for row with the descriptor pool
    rs_dev_array<int32_t> d_kp_point;               // [pool rows] point slot of each key-frame keypoint or -1, row for row with the pool:
    size_t kp_point_rows = 0;                       // rewritten after a topology change by rs_map_loop_sync, its only reader's entry
    rs_dev_array<int32_t> d_win;                    // scratch of rs_map_bundle_adjust: pid [P] | obs offset [P]; flags [P] of the key-frame stages
    size_t pool_rows = 0, n_obs = 0;
    rs_dev_array<int32_t> d_out;                    // scratch for match results
    std::vector<int32_t> h_obs_ptr, h_obs_kf, h_obs_desc, h_kp_point;
    std::vector<float> h_centres, h_poses;
    rs_dev_array<double> d_gather;                  // pts [8192][3] f64 | uv [8192][2] f32 | n: the refit's gathered problem
    void* fuse = nullptr;                           // scratch of rs_map_fuse_loop (map_fuse.hip owns and frees it)
};

extern "C" int rs_map_create(rs_context* ctx, rs_map** out)
{
    if (!ctx || !out) return RS_ERR_INVALID;
    rs_map* m = new rs_map();
    m->ctx = ctx;
    *out = m;
    return RS_OK;
}

extern "C" int rs_map_destroy(rs_map* m)
{
    if (!m) return RS_OK;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    rs_map_fuse_release(m->fuse);
    delete m;                           // every device array frees itself
    return RS_OK;
}

// ------------------------------------------------------------------------------------------------ updates
static void centre_of(const float* T, float c[3])      // Frame::camera_center = -R^T t, src/Frame.cpp:39-42
{
    for (int i = 0; i < 3; i++) c[i] = (-T[i] * T[3] + -T[4 + i] * T[7]) + -T[8 + i] * T[11];
}

extern "C" int rs_map_add_keyframe(rs_map* m, const rs_frame* f, const float h_pose[16], int* out_kf)
{
    if (!m || !f || !h_pose || !out_kf || f->ctx != m->ctx) return RS_ERR_INVALID;
    rs_context* ctx = m->ctx;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rows = m->pool_rows + (size_t)f->n;
    int rc = m->d_pool.reserve(ctx, 32 * (rows > 0 ? rows : 1), MAP_FIRST, 32 * m->pool_rows);      // both keep the rows already there
    if (rc) return rc;
    rc = m->d_kp_pool.reserve(ctx, 2 * (rows > 0 ? rows : 1), MAP_FIRST, 2 * m->pool_rows);
    if (rc) return rc;
    MapKeyFrame k;
    k.n = f->n;
    k.pool_row = (int)m->pool_rows;
    memcpy(k.pose, h_pose, sizeof k.pose);
    k.kp_point.assign((size_t)f->n, -1);
    if (f->n > 0)
        RS_HIP(ctx, hipMemcpyAsync(m->d_pool + 32 * m->pool_rows, f->d_desc, 32 * (size_t)f->n, hipMemcpyDeviceToDevice, ctx->stream));
    if (f->n > 0)
        RS_HIP(ctx, hipMemcpyAsync(m->d_kp_pool + 2 * m->pool_rows, f->d_kp, sizeof(float) * 2 * (size_t)f->n, hipMemcpyDeviceToDevice, ctx->stream));
    m->pool_rows = rows;
    m->kfs.push_back(std::move(k));
    m->dirty_centres = true;
    *out_kf = (int)m->kfs.size() - 1;
    return RS_OK;
}

extern "C" int rs_map_set_keyframe_pose(rs_map* m, int kf, const float h_pose[16])
{
    if (!m || !h_pose || kf < 0 || kf >= (int)m->kfs.size()) return RS_ERR_INVALID;
    memcpy(m->kfs[(size_t)kf].pose, h_pose, sizeof(float) * 16);
    m->dirty_centres = true;
    return RS_OK;
}

extern "C" int rs_map_add_point(rs_map* m, const float xyz[3], int* out_point)
{
    if (!m || !xyz || !out_point) return RS_ERR_INVALID;
    *out_point = mirror_add_point(m, xyz);
    return RS_OK;
}

static bool point_ok(const rs_map* m, int p) { return mirror_point_ok(m, p); }

extern "C" int rs_map_set_position(rs_map* m, int point, const float xyz[3])
{
    if (!m || !xyz || !point_ok(m, point)) return RS_ERR_INVALID;
    memcpy(&m->pos[3 * (size_t)point], xyz, sizeof(float) * 3);
    m->dirty_positions = true;
    return RS_OK;
}

extern "C" int rs_map_remove_observation(rs_map* m, int point, int kf)
{
    if (!m) return RS_ERR_INVALID;
    return mirror_remove_observation(m, point, kf);
}

// Map::associate (src/Map.cpp:95-113): map_mirror.h
extern "C" int rs_map_add_observation(rs_map* m, int point, int kf, int keypoint)
{
    if (!m) return RS_ERR_INVALID;
    return mirror_add_observation(m, point, kf, keypoint);
}

extern "C" int rs_map_remove_point(rs_map* m, int point)
{
    if (!m) return RS_ERR_INVALID;
    return mirror_remove_point(m, point);
}

extern "C" int rs_map_counts(const rs_map* m, int h_out[4])
{
    if (!m || !h_out) return RS_ERR_INVALID;
    size_t no = 0;
    for (const auto& v : m->obs) no += v.size();
    h_out[0] = (int)m->alive.size(); h_out[1] = m->n_alive; h_out[2] = (int)no; h_out[3] = (int)m->kfs.size();
    return RS_OK;
}

extern "C" int rs_map_get_positions(const rs_map* m, int first, int count, float* h_xyz)
{
    if (!m || first < 0 || count < 0 || (size_t)first + (size_t)count > m->alive.size() || (count > 0 && !h_xyz)) return RS_ERR_INVALID;
    if (count) memcpy(h_xyz, &m->pos[3 * (size_t)first], sizeof(float) * 3 * (size_t)count);
    return RS_OK;
}

// ------------------------------------------------------------------------------------------------ device image
// The seven per-point arrays for P slots.  Nothing is kept: each is uploaded, recomputed or zeroed after it grew.  d_flag goes
// first and its new capacity S (4096 doubled) is the slot capacity: every other array is reserved for S slots, not for P, so
// all hold S of them (d_obs_ptr S + 1: its capacity 4097 doubled as often exceeds it) and none lags behind the others.  d_alive
// goes last: only when all seven hold S slots does the compare below let a later call pass.
static int map_reserve_points(rs_map* m, size_t P)
{
    if (P <= m->d_alive.cap) return RS_OK;
    rs_context* ctx = m->ctx;
    const size_t F = MAP_FIRST_POINTS;
    bool zero_flag = false, zero_mark = false;
    int rc;
    if ((rc = m->d_flag.reserve(ctx, P, F, 0, &zero_flag))) return rc;
    if (zero_flag) RS_HIP(ctx, hipMemsetAsync(m->d_flag, 0, m->d_flag.cap, ctx->stream));
    const size_t S = m->d_flag.cap;
    if ((rc = m->d_mark.reserve(ctx, S, F, 0, &zero_mark))) return rc;
    if (zero_mark) RS_HIP(ctx, hipMemsetAsync(m->d_mark, 0, sizeof(uint32_t) * m->d_mark.cap, ctx->stream));
    if ((rc = m->d_pos.reserve(ctx, 3 * S, 3 * F, 0, &m->dirty_positions)) || (rc = m->d_consistent.reserve(ctx, S, F, 0, &m->dirty_consistent)) ||
        (rc = m->d_obs_ptr.reserve(ctx, S + 1, F + 1)) || (rc = m->d_elig.reserve(ctx, S, F)))
        return rc;
    return m->d_alive.reserve(ctx, S, F);
}

static int map_reserve_obs(rs_map* m, size_t n_obs)      // the two per-observation arrays, uploaded whole after every topology change
{
    const int rc = m->d_obs_kf.reserve(m->ctx, n_obs, MAP_FIRST_OBS);
    return rc ? rc : m->d_obs_desc.reserve(m->ctx, n_obs, MAP_FIRST_OBS);
}

static int map_sync_device(rs_map* m)
{
    rs_context* ctx = m->ctx;
    const size_t P = m->alive.size(), KF = m->kfs.size();
    hipStream_t s = ctx->stream;
    if (m->dirty_topology) {
        m->h_obs_ptr.resize(P + 1);
        m->h_obs_kf.clear();
        m->h_obs_desc.clear();
        for (size_t p = 0; p < P; p++) {
            m->h_obs_ptr[p] = (int32_t)m->h_obs_kf.size();
            for (const auto& o : m->obs[p]) {
                m->h_obs_kf.push_back(o.kf);
                m->h_obs_desc.push_back(m->kfs[(size_t)o.kf].pool_row + o.kp);
            }
        }
        m->h_obs_ptr[P] = (int32_t)m->h_obs_kf.size();
        m->n_obs = m->h_obs_kf.size();
        int rc = map_reserve_points(m, P);
        if (!rc) rc = map_reserve_obs(m, m->n_obs);
        if (rc) return rc;
        // pageable sources: these three copies complete before returning only because of the synchronisation below
        if (P) RS_HIP(ctx, hipMemcpyAsync(m->d_alive, m->alive.data(), P, hipMemcpyHostToDevice, s));
        RS_HIP(ctx, hipMemcpyAsync(m->d_obs_ptr, m->h_obs_ptr.data(), sizeof(int32_t) * (P + 1), hipMemcpyHostToDevice, s));
        if (m->n_obs) {
            RS_HIP(ctx, hipMemcpyAsync(m->d_obs_kf, m->h_obs_kf.data(), sizeof(int32_t) * m->n_obs, hipMemcpyHostToDevice, s));
            RS_HIP(ctx, hipMemcpyAsync(m->d_obs_desc, m->h_obs_desc.data(), sizeof(int32_t) * m->n_obs, hipMemcpyHostToDevice, s));
        }
    }
    if (m->dirty_positions && P) RS_HIP(ctx, hipMemcpyAsync(m->d_pos, m->pos.data(), sizeof(float) * 3 * P, hipMemcpyHostToDevice, s));
    if (m->dirty_centres) {
        m->h_centres.resize(3 * (KF ? KF : 1));
        for (size_t k = 0; k < KF; k++) centre_of(m->kfs[k].pose, &m->h_centres[3 * k]);
        int rc = m->d_centres.reserve(ctx, 3 * (KF ? KF : 1), MAP_FIRST);
        if (rc) return rc;
        if (KF) RS_HIP(ctx, hipMemcpyAsync(m->d_centres, m->h_centres.data(), sizeof(float) * 3 * KF, hipMemcpyHostToDevice, s));
        // the poses themselves, for the key-frame stages (rs_map_reanchor, rs_map_cull_points)
        m->h_poses.resize(16 * (KF ? KF : 1));
        for (size_t k = 0; k < KF; k++) memcpy(&m->h_poses[16 * k], m->kfs[k].pose, sizeof(float) * 16);
        if ((rc = m->d_poses.reserve(ctx, 16 * (KF ? KF : 1), MAP_FIRST))) return rc;
        if (KF) RS_HIP(ctx, hipMemcpyAsync(m->d_poses, m->h_poses.data(), sizeof(float) * 16 * KF, hipMemcpyHostToDevice, s));
    }
    if (m->dirty_topology || m->dirty_positions || m->dirty_centres) RS_HIP(ctx, hipStreamSynchronize(s));
    m->dirty_topology = m->dirty_positions = m->dirty_centres = false;
    return RS_OK;
}

// loop.hip's window into the map: the device image brought up to date, and a key frame of the mirror
int rs_map_loop_sync(rs_map* m, rs_map_loop_view* out)
{
    int rc = map_sync_device(m);
    if (rc) return rc;
    // d_kp_point follows the topology, but only here: the other users of the device image never read it and pay nothing
    if (m->dirty_kp_point || m->kp_point_rows != m->pool_rows) {         // (a new key frame adds rows of -1)
        rs_context* ctx = m->ctx;
        m->h_kp_point.clear();
        for (const auto& k : m->kfs) m->h_kp_point.insert(m->h_kp_point.end(), k.kp_point.begin(), k.kp_point.end());
        if ((rc = m->d_kp_point.reserve(ctx, m->pool_rows ? m->pool_rows : 1, MAP_FIRST))) return rc;
        if (m->pool_rows) {             // pageable source: complete before returning
            RS_HIP(ctx, hipMemcpyAsync(m->d_kp_point, m->h_kp_point.data(), sizeof(int32_t) * m->pool_rows, hipMemcpyHostToDevice, ctx->stream));
            RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        m->kp_point_rows = m->pool_rows;
        m->dirty_kp_point = false;
    }
    *out = rs_map_loop_view{m->ctx, (int)m->kfs.size(), (int)m->alive.size(), m->d_pool, m->d_kp_pool, m->d_kp_point, m->d_pos, m->d_centres};
    return RS_OK;
}

rs_context* rs_map_context(const rs_map* m) { return m->ctx; }

// map_fuse.hip's window into the map: the mirror, and (sync != 0, a map with at least one point slot) the device image with the
// key-frame tables brought up to date
int rs_map_fuse_sync(rs_map* m, int sync, rs_map_fuse_view* out)
{
    *out = rs_map_fuse_view{};
    out->ctx = m->ctx; out->mirror = m; out->scratch = &m->fuse;
    if (!sync) return RS_OK;
    rs_map_loop_view lv;
    const int rc = rs_map_loop_sync(m, &lv);
    if (rc) return rc;
    out->d_pos = m->d_pos; out->d_alive = m->d_alive; out->d_obs_ptr = m->d_obs_ptr; out->d_obs_kf = m->d_obs_kf;
    out->d_obs_desc = m->d_obs_desc; out->d_centres = m->d_centres; out->d_pool = m->d_pool; out->d_kp_pool = m->d_kp_pool;
    out->d_kp_point = m->d_kp_point; out->n_obs = m->n_obs; out->pool_rows = m->pool_rows;
    return RS_OK;
}

extern "C" int rs_map_fuse_points(rs_map* m, int kept, int discarded)
{
    if (!m) return RS_ERR_INVALID;
    return mirror_fuse(m, kept, discarded);
}

extern "C" int rs_map_get_observations(const rs_map* m, int point, int32_t* h_kf, int32_t* h_kp, int capacity, int* h_n)
{
    if (!m || !h_n || point < 0 || point >= (int)m->alive.size()) return RS_ERR_INVALID;
    const auto& v = m->obs[(size_t)point];
    *h_n = (int)v.size();
    for (size_t i = 0; i < v.size() && (int)i < capacity; i++) {
        if (h_kf) h_kf[i] = v[i].kf;
        if (h_kp) h_kp[i] = v[i].kp;
    }
    return RS_OK;
}

extern "C" int rs_map_get_keyframe_matches(const rs_map* m, int kf, int32_t* h_kp_point, int capacity, int* h_n)
{
    if (!m || !h_n || !mirror_kf_ok(m, kf)) return RS_ERR_INVALID;
    const auto& t = m->kfs[(size_t)kf].kp_point;
    *h_n = (int)t.size();
    for (size_t i = 0; i < t.size() && (int)i < capacity; i++)
        if (h_kp_point) h_kp_point[i] = t[i];
    return RS_OK;
}

extern "C" int rs_map_set_track_consistent(rs_map* m, int point)
{
    if (!m) return RS_ERR_INVALID;
    return mirror_set_track_consistent(m, point);
}

#define MAP_GATHER_MAX 8192             // keypoints of a frame (frame.hip's FRAME_MAX_POINTS)

// frame_matches.hip's window into the map: the device image brought up to date, the flags of part 2 with it, and the
// scratch of its three stages (rs_reproj_match's outputs sized for a frame of n_keypoints)
int rs_map_track_sync(rs_map* m, int n_keypoints, rs_map_track_view* out)
{
    rs_context* ctx = m->ctx;
    const size_t P = m->alive.size();
    int rc = P ? map_sync_device(m) : RS_OK;        // (an empty map has no image yet, and nothing reads one)
    if (rc) return rc;
    if (m->dirty_consistent && P && m->d_consistent) {      // pageable source: complete before returning
        RS_HIP(ctx, hipMemcpyAsync(m->d_consistent, m->consistent.data(), P, hipMemcpyHostToDevice, ctx->stream));
        RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        m->dirty_consistent = false;
    }
    if ((rc = m->d_gather.reserve(ctx, (size_t)MAP_GATHER_MAX * 4 + 32, (size_t)MAP_GATHER_MAX * 4 + 32))) return rc;      // one size, made once
    const size_t N = (size_t)(n_keypoints > 0 ? n_keypoints : 0);
    if ((rc = m->d_out.reserve(ctx, 2 * P + 4 * N + 1, MAP_FIRST))) return rc;
    *out = rs_map_track_view{};
    out->n_kf = (int)m->kfs.size();
    out->mv = rs_map_view{(int)P, m->d_pos, m->d_elig, m->d_obs_ptr, m->d_obs_kf, m->d_obs_desc, m->d_centres, m->d_pool};
    out->d_alive = m->d_alive; out->d_consistent = m->d_consistent; out->d_flag = m->d_flag; out->d_mark = m->d_mark;
    out->d_gather_pts = m->d_gather;
    out->d_gather_uv = (float*)(m->d_gather + 3 * (size_t)MAP_GATHER_MAX);
    out->d_gather_n = (int32_t*)(out->d_gather_uv + 2 * (size_t)MAP_GATHER_MAX);
    out->d_out = m->d_out;
    return RS_OK;
}

bool rs_map_loop_keyframe(const rs_map* m, int kf, int* n, int* pool_row, int* n_matched)
{
    if (kf < 0 || kf >= (int)m->kfs.size()) return false;
    const MapKeyFrame& k = m->kfs[(size_t)kf];
    int c = 0;
    for (const int32_t p : k.kp_point) c += p >= 0 ? 1 : 0;
    *n = k.n; *pool_row = k.pool_row; *n_matched = c;
    return true;
}

// per-call eligibility (src/MapMatcher.cpp:53, :169): alive, not already matched by the frame, and — for
// match_key_frame — observed by the required key frame
// flag table [P], all zero between calls: bit 0 = the frame already matches the point
__global__ __launch_bounds__(256) void k_map_flag(const int32_t* __restrict__ idx, int n, uint8_t* __restrict__ flag, uint8_t bit, int set)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        unsigned int* w = (unsigned int*)(flag + (idx[i] & ~3));
        const unsigned int msk = (unsigned int)bit << (8 * (idx[i] & 3));
        if (set) atomicOr(w, msk); else atomicAnd(w, ~msk);
    }
}

__global__ __launch_bounds__(256) void k_map_eligible(int P, const uint8_t* __restrict__ alive, const uint8_t* __restrict__ flag,
                                                      const int32_t* __restrict__ obs_ptr, const int32_t* __restrict__ obs_kf,
                                                      int required_kf, int listed_only, uint8_t* __restrict__ elig)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    bool e = alive[p] != 0 && (flag[p] & 1) == 0 && (!listed_only || (flag[p] & 2) != 0);
    if (e && required_kf >= 0) {
        bool seen = false;
        for (int o = obs_ptr[p]; o < obs_ptr[p + 1]; o++) seen = seen || obs_kf[o] == required_kf;
        e = seen;
    }
    elig[p] = e ? 1 : 0;
}

void rs_map_launch_eligible(rs_map* m, int required_kf)
{
    rs_prof_scope ps(m->ctx, "K2p_map_eligible");
    const int P = (int)m->alive.size();
    hipLaunchKernelGGL(k_map_eligible, dim3((P + 255) / 256), dim3(256), 0, m->ctx->stream, P, m->d_alive, m->d_flag, m->d_obs_ptr, m->d_obs_kf,
                       required_kf, 0, m->d_elig);
}

// MapMatcher::match_map / match_key_frame / match_for_fuse against the resident map.
//   h_kp_matched [n]       Frame::is_matched(keypoint)                    (src/MapMatcher.cpp:81)
//   h_matched_points       the point slots the frame already matches      (:53)
//   required_observer_kf   >= 0: only points observed by that key frame (:169); -1: none
//   h_only_points          match_for_fuse (:117-127): only these slots take part (n_only < 0: the whole map).  They
//                          compete for a keypoint in LIST order, as the reference's loop over its vector does (:120-126)
//                          and as the flattened path does (the shim flattens the vector in order): the listed points are
//                          gathered from the mirror into a small view of their own, point i of it = h_only_points[i].
//                          Dead slots in the list are skipped like the reference's null pointers (:121-123).
// Every host list is validated and every buffer is grown BEFORE the first launch, and the flag table is cleared by the
// same launches that follow the eligibility kernel whatever happens later: it is all-zero between calls.
extern "C" int rs_map_match(rs_context* ctx, rs_map* m, rs_frame* f, const float h_pose[16], const float h_intrinsics[4],
                            int width, int height, const uint8_t* h_kp_matched, const int32_t* h_matched_points,
                            int n_matched_points, int required_observer_kf, const int32_t* h_only_points, int n_only,
                            int replace, int max_distance, int32_t* h_match_kp, int32_t* h_match_point, int* h_count)
{
    if (!ctx || !m || !f || m->ctx != ctx || f->ctx != ctx || !h_pose || !h_intrinsics || !h_count) return RS_ERR_INVALID;
    if (n_matched_points < 0 || (n_matched_points > 0 && !h_matched_points)) return rs_fail(ctx, RS_ERR_INVALID, "matched point list");
    if (required_observer_kf >= (int)m->kfs.size()) return rs_fail(ctx, RS_ERR_INVALID, "unknown key frame");
    *h_count = 0;
    const int N = f->n, P = (int)m->alive.size();
    if (N == 0 || P == 0) return RS_OK;
    if (!h_match_kp || !h_match_point) return rs_fail(ctx, RS_ERR_INVALID, "null output");
    if (n_only > 0 && !h_only_points) return rs_fail(ctx, RS_ERR_INVALID, "null point list");
    for (int i = 0; i < n_matched_points; i++)
        if (h_matched_points[i] < 0 || h_matched_points[i] >= P) return rs_fail(ctx, RS_ERR_INVALID, "matched point %d out of range", i);
    for (int i = 0; i < n_only; i++)
        if (h_only_points[i] < 0 || h_only_points[i] >= P) return rs_fail(ctx, RS_ERR_INVALID, "listed point %d out of range", i);
    if (n_only == 0) return RS_OK;                       // an empty list: nothing takes part
    RS_HIP(ctx, hipSetDevice(ctx->device));
    int rc = map_sync_device(m);
    if (rc) return rc;
    const bool listed = n_only > 0;
    const int Pv = listed ? n_only : P;                  // points of the view the matcher runs on
    const size_t need = 2 * (size_t)Pv + 4 * (size_t)N + 1;
    if ((rc = m->d_out.reserve(ctx, need, MAP_FIRST))) return rc;
    rc = rs_stage_begin(ctx);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    // the frame's per-call state: which keypoints / points it already matches
    uint8_t* d_matched = nullptr;
    if (h_kp_matched) { rc = rs_stage_upload(ctx, h_kp_matched, (size_t)N, (void**)&d_matched); if (rc) return rc; }
    else { rc = rs_stage_alloc(ctx, (size_t)N, (void**)&d_matched); if (rc) return rc; RS_HIP(ctx, hipMemsetAsync(d_matched, 0, (size_t)N, s)); }
    rs_map_view mv{P, m->d_pos, m->d_elig, m->d_obs_ptr, m->d_obs_kf, m->d_obs_desc, m->d_centres, m->d_pool};
    if (listed) {
        // the listed points as a view of their own, in list order, from the mirror (map_sync_device has just rebuilt the
        // observation tables): a fuse list is a few hundred points
        std::vector<uint8_t> taken((size_t)P, 0), elig((size_t)n_only);
        for (int i = 0; i < n_matched_points; i++) taken[(size_t)h_matched_points[i]] = 1;
        std::vector<float> pos(3 * (size_t)n_only);
        std::vector<int32_t> optr((size_t)n_only + 1), okf, odesc;
        for (int i = 0; i < n_only; i++) {
            const size_t p = (size_t)h_only_points[i];
            memcpy(&pos[3 * (size_t)i], &m->pos[3 * p], sizeof(float) * 3);
            optr[(size_t)i] = (int32_t)okf.size();
            bool e = m->alive[p] != 0 && !taken[p];
            bool seen = required_observer_kf < 0;
            for (int32_t o = m->h_obs_ptr[p]; o < m->h_obs_ptr[p + 1]; o++) {
                okf.push_back(m->h_obs_kf[(size_t)o]);
                odesc.push_back(m->h_obs_desc[(size_t)o]);
                seen = seen || m->h_obs_kf[(size_t)o] == required_observer_kf;
            }
            elig[(size_t)i] = (e && seen) ? 1 : 0;
        }
        optr[(size_t)n_only] = (int32_t)okf.size();
        if (okf.empty()) { okf.push_back(0); odesc.push_back(0); }
        float* d_p = nullptr; uint8_t* d_e = nullptr; int32_t *d_op = nullptr, *d_ok = nullptr, *d_od = nullptr;
        if ((rc = rs_stage_upload(ctx, pos.data(), sizeof(float) * pos.size(), (void**)&d_p))) return rc;
        if ((rc = rs_stage_upload(ctx, elig.data(), elig.size(), (void**)&d_e))) return rc;
        if ((rc = rs_stage_upload(ctx, optr.data(), sizeof(int32_t) * optr.size(), (void**)&d_op))) return rc;
        if ((rc = rs_stage_upload(ctx, okf.data(), sizeof(int32_t) * okf.size(), (void**)&d_ok))) return rc;
        if ((rc = rs_stage_upload(ctx, odesc.data(), sizeof(int32_t) * odesc.size(), (void**)&d_od))) return rc;
        mv = rs_map_view{n_only, d_p, d_e, d_op, d_ok, d_od, m->d_centres, m->d_pool};
    } else {
        int32_t* d_mp = nullptr;
        if (n_matched_points > 0) {
            rc = rs_stage_upload(ctx, h_matched_points, sizeof(int32_t) * (size_t)n_matched_points, (void**)&d_mp);
            if (rc) return rc;
            hipLaunchKernelGGL(k_map_flag, dim3((n_matched_points + 255) / 256), dim3(256), 0, s, d_mp, n_matched_points, m->d_flag, (uint8_t)1, 1);
        }
        {
            rs_prof_scope ps(ctx, "K2p_map_eligible");
            hipLaunchKernelGGL(k_map_eligible, dim3((P + 255) / 256), dim3(256), 0, s, P, m->d_alive, m->d_flag, m->d_obs_ptr, m->d_obs_kf,
                               required_observer_kf, 0, m->d_elig);
        }
        if (n_matched_points > 0)       // leave the flag table all-zero for the next call (enqueued before anything below can fail)
            hipLaunchKernelGGL(k_map_flag, dim3((n_matched_points + 255) / 256), dim3(256), 0, s, d_mp, n_matched_points, m->d_flag, (uint8_t)1, 0);
    }
    int32_t* pk = m->d_out, *pd = pk + Pv, *pp = pd + Pv, *pdist = pp + N, *mkp = pdist + N, *mpt = mkp + N, *cnt = mpt + N;
    rs_frame_view fv{};
    memcpy(fv.pose, h_pose, sizeof fv.pose);
    fv.fx = h_intrinsics[0]; fv.fy = h_intrinsics[1]; fv.cx = h_intrinsics[2]; fv.cy = h_intrinsics[3];
    fv.width = width; fv.height = height; fv.n_keypoints = N;
    fv.d_keypoints = f->d_kp; fv.d_descriptors = f->d_desc; fv.d_kp_matched = d_matched;
    fv.d_kd_node_kp = f->d_kd; fv.d_kd_left = f->d_kd + N; fv.d_kd_right = f->d_kd + 2 * (size_t)N; fv.kd_root = f->kd_root;
    fv.d_kd_packed = f->d_packed;
    if ((rc = rs_frame_grid(ctx, f, width, height, &fv.d_kd_grid))) return rc;
    rc = rs_reproj_match(ctx, &fv, &mv, replace, max_distance, pk, pd, pp, pdist, mkp, mpt, cnt);
    if (rc) return rc;
    int32_t n_out = 0;
    rc = rs_stage_download(ctx, cnt, sizeof(int32_t), &n_out);
    if (rc) return rc;
    rc = rs_stage_download(ctx, mkp, sizeof(int32_t) * (size_t)N, h_match_kp);      // at most N matches: one read-back
    if (rc) return rc;
    rc = rs_stage_download(ctx, mpt, sizeof(int32_t) * (size_t)N, h_match_point);
    if (rc) return rc;
    rc = rs_stage_sync(ctx);
    if (rc) return rc;
    if (listed)
        for (int i = 0; i < n_out; i++) h_match_point[i] = h_only_points[h_match_point[i]];      // view index -> map slot
    *h_count = n_out;
    return RS_OK;
}

// ------------------------------------------------------------------------------------------------ local BA
// optimization::bundle_adjust on the resident map (reference src/Optimization.cpp:269-374).  The window's problem — free
// points, observation CSR by landmark, observation pixels, f64 points — is built ON THE DEVICE from the resident image
// (observation CSR by point, key-point pool): three small kernels over the map's point slots instead of three host passes
// over 20 x 2000 key-point tables plus 1 MB of uploads.  The host packs the <= ~40 poses, reads back two counters, calls
// rs_bundle_adjust, and on a usable solve a write-back kernel puts the positions into the device image while the mirror
// and the caller get them through one download.
//   free points      alive, >= 2 observations in the whole map, matched by an optimised frame of the list (:287-302), in
//                    ascending SLOT order (the reference walks its frames' match tables; the set is the same, and the
//                    order only decides f64 summation order);
//   residual blocks  every listed frame x its matched free points (:304-315), CSR by point, frames in list order.
//   h_out_poses [n_kfs][16]           (rows of fixed key frames are their unchanged poses)
//   h_out_points [cap], h_out_xyz [cap][3], *h_n_points    the free points (slots) and their new positions
__global__ __launch_bounds__(256) void k_win_count(int P, const uint8_t* __restrict__ alive, const int32_t* __restrict__ obs_ptr,
                                                   const int32_t* __restrict__ obs_kf, const int32_t* __restrict__ win_of_kf,
                                                   int32_t* __restrict__ flag, int32_t* __restrict__ cnt)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int o0 = obs_ptr[p], o1 = obs_ptr[p + 1];
    int c = 0, fr = 0;
    for (int o = o0; o < o1; o++) {
        const int w = win_of_kf[obs_kf[o]];       // -1: not in the list; else list index | free << 16
        if (w >= 0) { c++; fr |= w >> 16; }
    }
    const int f = (alive[p] != 0 && o1 - o0 >= 2 && fr) ? 1 : 0;
    flag[p] = f;
    cnt[p] = f ? c : 0;
}

// exclusive scans of flag -> pid and cnt -> obs offset in place, totals to h_tot (one workgroup; the map has 1e4 - 1e5 slots)
__global__ __launch_bounds__(1024) void k_win_scan(int P, int32_t* __restrict__ flag, int32_t* __restrict__ cnt, int32_t* __restrict__ tot)
{
    __shared__ int carry[2];
    if (threadIdx.x == 0) { carry[0] = 0; carry[1] = 0; }
    __syncthreads();
    for (int base = 0; base < P; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const int f = i < P ? flag[i] : 0, c = i < P ? cnt[i] : 0;
        int tf, tc;
        const int of = rs_block_exclusive_scan(f, &tf);
        const int oc = rs_block_exclusive_scan(c, &tc);
        if (i < P) { flag[i] = f ? carry[0] + of : -1; cnt[i] = carry[1] + oc; }
        __syncthreads();
        if (threadIdx.x == 0) { carry[0] += tf; carry[1] += tc; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { tot[0] = carry[0]; tot[1] = carry[1]; }
}

__global__ __launch_bounds__(256) void k_win_fill(int P, int C, const int32_t* __restrict__ pid, const int32_t* __restrict__ off,
                                                  const int32_t* __restrict__ obs_ptr, const int32_t* __restrict__ obs_kf,
                                                  const int32_t* __restrict__ obs_desc, const int32_t* __restrict__ win_of_kf,
                                                  const float* __restrict__ pos, const float2* __restrict__ kp_pool,
                                                  double* __restrict__ pts, int32_t* __restrict__ list, int32_t* __restrict__ optr,
                                                  int32_t* __restrict__ ocam, float2* __restrict__ ouv, int n_free, int n_obs)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) optr[n_free] = n_obs;
    if (p >= P) return;
    const int q = pid[p];
    if (q < 0) return;
    list[q] = p;
#pragma unroll
    for (int k = 0; k < 3; k++) pts[3 * (size_t)q + k] = (double)pos[3 * (size_t)p + k];
    int w = off[p];
    optr[q] = w;
    const int o0 = obs_ptr[p], o1 = obs_ptr[p + 1];
    // frames in LIST order (a point has at most one observation per key frame)
    for (int c = 0; c < C; c++)
        for (int o = o0; o < o1; o++) {
            const int wk = win_of_kf[obs_kf[o]];
            if (wk >= 0 && (wk & 0xFFFF) == c) { ocam[w] = c; ouv[w] = kp_pool[obs_desc[o]]; w++; }
        }
}

__global__ __launch_bounds__(256) void k_win_writeback(int n_free, const int32_t* __restrict__ list, const double* __restrict__ pts,
                                                       float* __restrict__ pos, float* __restrict__ oxyz)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_free) return;
    const int p = list[q];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float v = (float)pts[3 * (size_t)q + k];                              // :369-372
        pos[3 * (size_t)p + k] = v;
        oxyz[3 * (size_t)q + k] = v;
    }
}

// list index | free << 16 per key frame (-1: not listed), refusing unknown and repeated key frames
static int window_of_kf(rs_context* ctx, const rs_map* m, const int32_t* h_kfs, const uint8_t* h_free, size_t C, std::vector<int32_t>* win)
{
    const size_t KF = m->kfs.size();
    if (C > 65535) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "more than 65535 frames in a window");
    win->assign(KF ? KF : 1, -1);
    for (size_t c = 0; c < C; c++) {
        if (h_kfs[c] < 0 || h_kfs[c] >= (int)KF) return rs_fail(ctx, RS_ERR_INVALID, "unknown key frame");
        if ((*win)[(size_t)h_kfs[c]] >= 0) return rs_fail(ctx, RS_ERR_INVALID, "key frame %d listed twice", h_kfs[c]);
        (*win)[(size_t)h_kfs[c]] = (int32_t)c | (h_free && h_free[c] ? 1 << 16 : 0);       // (h_free null: no frame is free)
    }
    return RS_OK;
}

// The window's problem in staging memory (valid until the next rs_stage_begin); Pf == 0 or M == 0: nothing was filled.
struct MapWindow {
    size_t Pf = 0, M = 0;
    double* pts = nullptr; int32_t *ptr = nullptr, *cam = nullptr, *list = nullptr; float* uv = nullptr;
};

// What map_window_build and map_keyframe_stage start with: the image brought up to date, d_win made, the staging pool begun and
// the list's table of key frames in it.  d_win is the window build's pid [P] | obs offset [P] | totals [2] and the key-frame
// stages' selection bytes [P] (nothing else uses it between calls); both size it 2 P + 2 words, so that the two users never
// reallocate it in turn.
static int map_stage_begin(rs_context* ctx, rs_map* m, const std::vector<int32_t>& win, int32_t** d_winkf)
{
    RS_HIP(ctx, hipSetDevice(ctx->device));
    int rc = map_sync_device(m);
    if (rc) return rc;
    if ((rc = m->d_win.reserve(ctx, 2 * m->alive.size() + 2, MAP_FIRST))) return rc;
    if ((rc = rs_stage_begin(ctx))) return rc;
    return rs_stage_upload(ctx, win.data(), sizeof(int32_t) * win.size(), (void**)d_winkf);
}

static int map_window_build(rs_context* ctx, rs_map* m, const std::vector<int32_t>& win, size_t C, MapWindow* w)
{
    const size_t P = m->alive.size();
    int32_t* d_winkf = nullptr;
    int rc = map_stage_begin(ctx, m, win, &d_winkf);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    int32_t *d_pid = m->d_win, *d_off = d_pid + P, *d_tot = d_off + P;
    const int pb = (int)((P + 255) / 256);
    {
        rs_prof_scope ps(ctx, "K9_window_build");
        hipLaunchKernelGGL(k_win_count, dim3(pb), dim3(256), 0, s, (int)P, m->d_alive, m->d_obs_ptr, m->d_obs_kf, d_winkf, d_pid, d_off);
        hipLaunchKernelGGL(k_win_scan, dim3(1), dim3(1024), 0, s, (int)P, d_pid, d_off, d_tot);
    }
    int32_t tot[2] = {0, 0};
    if ((rc = rs_stage_download(ctx, d_tot, sizeof tot, tot))) return rc;
    if ((rc = rs_stage_sync(ctx))) return rc;
    w->Pf = (size_t)tot[0];
    w->M = (size_t)tot[1];
    if (w->Pf == 0 || w->M == 0) return RS_OK;
    if ((rc = rs_stage_alloc(ctx, sizeof(double) * 3 * w->Pf, (void**)&w->pts))) return rc;
    if ((rc = rs_stage_alloc(ctx, sizeof(int32_t) * (w->Pf + 1), (void**)&w->ptr))) return rc;
    if ((rc = rs_stage_alloc(ctx, sizeof(int32_t) * w->M, (void**)&w->cam))) return rc;
    if ((rc = rs_stage_alloc(ctx, sizeof(float) * 2 * w->M, (void**)&w->uv))) return rc;
    if ((rc = rs_stage_alloc(ctx, sizeof(int32_t) * w->Pf, (void**)&w->list))) return rc;
    {
        rs_prof_scope ps(ctx, "K9_window_build");
        hipLaunchKernelGGL(k_win_fill, dim3(pb), dim3(256), 0, s, (int)P, (int)C, d_pid, d_off, m->d_obs_ptr, m->d_obs_kf, m->d_obs_desc, d_winkf,
                           m->d_pos, (const float2*)m->d_kp_pool.p, w->pts, w->list, w->ptr, w->cam, (float2*)w->uv, (int)w->Pf, (int)w->M);
    }
    return RS_OK;
}

extern "C" int rs_map_bundle_adjust(rs_context* ctx, rs_map* m, const int32_t* h_kfs, const uint8_t* h_free, int n_kfs,
                                    const float h_intrinsics[4], const rs_ba_options* options, rs_ba_summary* h_summary,
                                    float* h_out_poses, int32_t* h_out_points, float* h_out_xyz, int capacity, int* h_n_points)
{
    if (!ctx || !m || m->ctx != ctx || !h_kfs || !h_free || n_kfs < 0 || !h_intrinsics || !h_summary || !h_n_points) return RS_ERR_INVALID;
    *h_n_points = 0;
    memset(h_summary, 0, sizeof *h_summary);
    const size_t C = (size_t)n_kfs, P = m->alive.size();
    std::vector<int32_t> win;
    int rc = window_of_kf(ctx, m, h_kfs, h_free, C, &win);
    if (rc) return rc;
    auto keep_poses = [&]() {
        if (h_out_poses) for (size_t c = 0; c < C; c++) memcpy(h_out_poses + 16 * c, m->kfs[(size_t)h_kfs[c]].pose, sizeof(float) * 16);
    };
    if (P == 0 || C == 0) { h_summary->termination = RS_BA_FAILURE; keep_poses(); return RS_OK; }
    MapWindow w;
    if ((rc = map_window_build(ctx, m, win, C, &w))) return rc;
    const size_t Pf = w.Pf, M = w.M;
    if (Pf == 0 || M == 0) { h_summary->termination = RS_BA_FAILURE; keep_poses(); return RS_OK; }
    hipStream_t s = ctx->stream;
    std::vector<double> cams(6 * C);
    for (size_t c = 0; c < C; c++) rs_pack_pose(m->kfs[(size_t)h_kfs[c]].pose, &cams[6 * c]);
    double* d_cams = nullptr;
    float* d_oxyz = nullptr;
    if ((rc = rs_stage_upload(ctx, cams.data(), sizeof(double) * 6 * C, (void**)&d_cams))) return rc;
    if ((rc = rs_stage_alloc(ctx, sizeof(float) * 3 * Pf, (void**)&d_oxyz))) return rc;
    rc = rs_bundle_adjust(ctx, (int)C, (int)Pf, (int)M, d_cams, h_free, w.pts, w.ptr, w.cam, w.uv, h_intrinsics, options, h_summary);
    if (rc) return rc;
    if (!h_summary->usable) { keep_poses(); return RS_OK; }
    rc = rs_ba_get_cameras(ctx, cams.data(), (int)C);
    if (rc) return rc;
    hipLaunchKernelGGL(k_win_writeback, dim3((int)((Pf + 255) / 256)), dim3(256), 0, s, (int)Pf, w.list, w.pts, m->d_pos, d_oxyz);
    std::vector<int32_t> list(Pf);
    std::vector<float> xyz(3 * Pf);
    if ((rc = rs_stage_download(ctx, w.list, sizeof(int32_t) * Pf, list.data()))) return rc;
    if ((rc = rs_stage_download(ctx, d_oxyz, sizeof(float) * 3 * Pf, xyz.data()))) return rc;
    if ((rc = rs_stage_sync(ctx))) return rc;
    for (size_t c = 0; c < C; c++) {
        MapKeyFrame& k = m->kfs[(size_t)h_kfs[c]];
        if (h_free[c]) { rs_unpack_pose(&cams[6 * c], k.pose); m->dirty_centres = true; }     // :363-368
        if (h_out_poses) memcpy(h_out_poses + 16 * c, k.pose, sizeof(float) * 16);
    }
    for (size_t q = 0; q < Pf; q++) memcpy(&m->pos[3 * (size_t)list[q]], &xyz[3 * q], sizeof(float) * 3);   // the mirror follows the device image
    const size_t nout = Pf < (size_t)(capacity > 0 ? capacity : 0) ? Pf : (size_t)(capacity > 0 ? capacity : 0);
    if (h_out_points && h_out_xyz && nout) {
        memcpy(h_out_points, list.data(), sizeof(int32_t) * nout);
        memcpy(h_out_xyz, xyz.data(), sizeof(float) * 3 * nout);
    }
    *h_n_points = (int)Pf;
    return RS_OK;
}

// The problem rs_map_bundle_adjust would solve for this window, built by the same kernels and copied out unsolved.
extern "C" int rs_map_window(rs_context* ctx, rs_map* m, const int32_t* h_kfs, const uint8_t* h_free, int n_kfs,
                             int32_t* h_points, double* h_xyz, int32_t* h_obs_ptr, int32_t* h_obs_cam, float* h_obs_uv,
                             int cap_points, int cap_obs, int* h_n_points, int* h_n_obs)
{
    if (!ctx || !m || m->ctx != ctx || !h_kfs || !h_free || n_kfs < 0 || !h_n_points || !h_n_obs) return RS_ERR_INVALID;
    *h_n_points = 0;
    *h_n_obs = 0;
    const size_t C = (size_t)n_kfs;
    std::vector<int32_t> win;
    int rc = window_of_kf(ctx, m, h_kfs, h_free, C, &win);
    if (rc) return rc;
    if (m->alive.empty() || C == 0) return RS_OK;
    MapWindow w;
    if ((rc = map_window_build(ctx, m, win, C, &w))) return rc;
    if (w.Pf == 0 || w.M == 0) return RS_OK;
    if (w.Pf <= (size_t)(cap_points > 0 ? cap_points : 0) && w.M <= (size_t)(cap_obs > 0 ? cap_obs : 0)) {
        if (!h_points || !h_xyz || !h_obs_ptr || !h_obs_cam || !h_obs_uv) return rs_fail(ctx, RS_ERR_INVALID, "null output");
        if ((rc = rs_stage_download(ctx, w.list, sizeof(int32_t) * w.Pf, h_points))) return rc;
        if ((rc = rs_stage_download(ctx, w.pts, sizeof(double) * 3 * w.Pf, h_xyz))) return rc;
        if ((rc = rs_stage_download(ctx, w.ptr, sizeof(int32_t) * (w.Pf + 1), h_obs_ptr))) return rc;
        if ((rc = rs_stage_download(ctx, w.cam, sizeof(int32_t) * w.M, h_obs_cam))) return rc;
        if ((rc = rs_stage_download(ctx, w.uv, sizeof(float) * 2 * w.M, h_obs_uv))) return rc;
    }
    if ((rc = rs_stage_sync(ctx))) return rc;
    *h_n_points = (int)w.Pf;
    *h_n_obs = (int)w.M;
    return RS_OK;
}

// ------------------------------------------------------------------------------------------------ key-frame insertion
// Mapper::insert (reference src/Mapper.cpp:152-174) on the resident map: the two mirror halves (adoption of the frame's
// matches, creation of the triangulated points) and the two device stages that follow the adjustment (map_keyframe.hip).
extern "C" int rs_map_insert_keyframe(rs_context* ctx, rs_map* m, const rs_frame* f, const float h_pose[16], int* out_kf, int* h_n_adopted)
{
    if (!ctx || !m || m->ctx != ctx || !f || f->ctx != ctx || !h_pose || !out_kf || !h_n_adopted) return RS_ERR_INVALID;
    *h_n_adopted = 0;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    // the frame's table first: a failed read-back leaves the map without the key frame
    std::vector<int32_t> tab((size_t)(f->n > 0 ? f->n : 1));
    int in_table = 0;
    int rd = rs_frame_matches_download(ctx, f, tab.data(), &in_table);
    if (rd) return rd;
    const int rc = rs_map_add_keyframe(m, f, h_pose, out_kf);
    if (rc) return rc;
    *h_n_adopted = mirror_adopt_table(m, *out_kf, tab.data(), f->n);                     // :157-159
    return RS_OK;
}

extern "C" int rs_map_add_track_points(rs_map* m, int kf, const rs_track_results* results, const int32_t* h_window_kfs, int n_window,
                                       int32_t* h_new_points)
{
    if (!m) return RS_ERR_INVALID;
    const int rc = mirror_add_track_points(m, kf, results, h_window_kfs, n_window, h_new_points);
    if (rc && results && results->n_pairs > results->capacity_pairs)
        return rs_fail(m->ctx, rc, "rs_map_add_track_points: %d key-frame sightings, room for %d: the pairs are incomplete", results->n_pairs,
                       results->capacity_pairs);
    if (rc) return rs_fail(m->ctx, rc, "rs_map_add_track_points: bad argument");
    return RS_OK;
}

// The image brought up to date, the list's table of key frames staged, the selection bytes and the output block made:
// what both device stages start with.  d_out: 2 + 4 P words (rs_kf_launch_*).
static int map_keyframe_stage(rs_context* ctx, rs_map* m, const std::vector<int32_t>& win, int32_t** d_winkf, uint8_t** d_sel, int32_t** d_out)
{
    int rc = map_stage_begin(ctx, m, win, d_winkf);
    if (rc) return rc;
    if ((rc = rs_stage_alloc(ctx, sizeof(int32_t) * (2 + 4 * m->alive.size()), (void**)d_out))) return rc;
    *d_sel = (uint8_t*)m->d_win.p;                    // (not rs_map::d_flag, the matcher's table that is all zero between calls)
    return RS_OK;
}

extern "C" int rs_map_reanchor(rs_context* ctx, rs_map* m, const int32_t* h_kfs, const float* h_before, int n_kfs,
                               int32_t* h_out_points, float* h_out_xyz, int capacity, int* h_n_points)
{
    if (!ctx || !m || m->ctx != ctx || n_kfs < 0 || (n_kfs > 0 && (!h_kfs || !h_before)) || !h_n_points) return RS_ERR_INVALID;
    *h_n_points = 0;
    const size_t C = (size_t)n_kfs, P = m->alive.size();
    std::vector<int32_t> win;
    int rc = window_of_kf(ctx, m, h_kfs, nullptr, C, &win);
    if (rc) return rc;
    if (P == 0 || C == 0) return RS_OK;
    int32_t *d_winkf = nullptr, *d_out = nullptr;
    uint8_t* d_sel = nullptr;
    float* d_before = nullptr;
    if ((rc = map_keyframe_stage(ctx, m, win, &d_winkf, &d_sel, &d_out))) return rc;
    if ((rc = rs_stage_upload(ctx, h_before, sizeof(float) * 16 * C, (void**)&d_before))) return rc;
    // From the launch on the image's positions are ahead of the mirror's.  Until the mirror has taken them the positions count
    // as dirty: if the read-back fails, the next use uploads the mirror's and the two agree again (the mirror wins).
    m->dirty_positions = true;
    rs_kf_launch_reanchor(ctx, (int)P, m->d_alive, m->d_obs_ptr, m->d_obs_kf, d_winkf, d_before, m->d_poses, m->d_pos, d_sel, d_out);
    RS_HIP(ctx, hipGetLastError());
    std::vector<int32_t> out(2 + 4 * P);
    if ((rc = rs_stage_download(ctx, d_out, sizeof(int32_t) * out.size(), out.data()))) return rc;      // one read-back
    if ((rc = rs_stage_sync(ctx))) return rc;
    const size_t n = (size_t)out[0];
    if (n > P) return rs_fail(ctx, RS_ERR_INTERNAL, "rs_map_reanchor: %zu moved points of %zu slots", n, P);
    const int32_t* list = out.data() + 2;
    const float* xyz = (const float*)(out.data() + 2 + P);
    for (size_t q = 0; q < n; q++)
        if (list[q] < 0 || (size_t)list[q] >= P) return rs_fail(ctx, RS_ERR_INTERNAL, "rs_map_reanchor: slot %d out of range", list[q]);
    for (size_t q = 0; q < n; q++) memcpy(&m->pos[3 * (size_t)list[q]], xyz + 3 * q, sizeof(float) * 3);
    m->dirty_positions = false;                      // the mirror has followed: the image is current, nothing to upload
    const size_t cap = (size_t)(capacity > 0 ? capacity : 0), nout = n < cap ? n : cap;
    if (h_out_points && nout) memcpy(h_out_points, list, sizeof(int32_t) * nout);
    if (h_out_xyz && nout) memcpy(h_out_xyz, xyz, sizeof(float) * 3 * nout);
    *h_n_points = (int)n;
    return RS_OK;
}

extern "C" int rs_map_cull_points(rs_context* ctx, rs_map* m, const int32_t* h_kfs, int n_kfs, const float h_intrinsics[4],
                                  float max_mean_error, int apply, int32_t* h_removed, float* h_removed_xyz, int capacity,
                                  int* h_n_removed, int* h_n_local)
{
    if (!ctx || !m || m->ctx != ctx || n_kfs < 0 || (n_kfs > 0 && !h_kfs) || !h_intrinsics || !h_n_removed) return RS_ERR_INVALID;
    *h_n_removed = 0;
    if (h_n_local) *h_n_local = 0;
    if (capacity > 0 && !h_removed) return rs_fail(ctx, RS_ERR_INVALID, "rs_map_cull_points: null output");
    const size_t C = (size_t)n_kfs, P = m->alive.size();
    std::vector<int32_t> win;
    int rc = window_of_kf(ctx, m, h_kfs, nullptr, C, &win);
    if (rc) return rc;
    if (P == 0 || C == 0) return RS_OK;
    int32_t *d_winkf = nullptr, *d_out = nullptr;
    uint8_t* d_sel = nullptr;
    if ((rc = map_keyframe_stage(ctx, m, win, &d_winkf, &d_sel, &d_out))) return rc;
    rs_kf_launch_cull(ctx, (int)P, m->d_alive, m->d_obs_ptr, m->d_obs_kf, m->d_obs_desc, d_winkf, m->d_poses, m->d_kp_pool, m->d_pos,
                      h_intrinsics, max_mean_error, d_sel, d_out);
    RS_HIP(ctx, hipGetLastError());
    std::vector<int32_t> out(2 + 4 * P);
    if ((rc = rs_stage_download(ctx, d_out, sizeof(int32_t) * out.size(), out.data()))) return rc;      // one read-back
    if ((rc = rs_stage_sync(ctx))) return rc;
    const size_t n = (size_t)out[0];
    if (n > P || (size_t)out[1] > P) return rs_fail(ctx, RS_ERR_INTERNAL, "rs_map_cull_points: %zu culled points of %zu slots", n, P);
    *h_n_removed = (int)n;
    if (h_n_local) *h_n_local = out[1];
    if (n > (size_t)(capacity > 0 ? capacity : 0))
        return rs_fail(ctx, RS_ERR_INVALID, "rs_map_cull_points: %zu points to remove, room for %d: nothing was removed", n, capacity);
    const int32_t* list = out.data() + 2;
    for (size_t q = 0; q < n; q++)
        if (!point_ok(m, list[q])) return rs_fail(ctx, RS_ERR_INTERNAL, "rs_map_cull_points: slot %d is not an alive point", list[q]);
    if (n) memcpy(h_removed, list, sizeof(int32_t) * n);
    if (h_removed_xyz && n) memcpy(h_removed_xyz, out.data() + 2 + P, sizeof(float) * 3 * n);      // diagnostics.culled, :426-428
    if (apply)
        for (size_t q = 0; q < n; q++) mirror_remove_point(m, list[q]);                            // :429, ascending slot
    return RS_OK;
}

// ------------------------------------------------------------------------------------------------ loop closure
// optimization::pose_graph (src/Optimization.cpp:540-639) on the resident map.
extern "C" int rs_map_pose_graph(rs_context* ctx, rs_map* m, const rs_pose_graph_edge* h_loops, int n_loops, int four_dof,
                                 const double h_gravity[3], const rs_ba_options* options, float* h_out_poses,
                                 float* h_velocity_rotation, rs_ba_summary* h_summary)
{
    if (!ctx || !m || m->ctx != ctx || !h_summary || n_loops < 0 || (n_loops > 0 && !h_loops)) return RS_ERR_INVALID;
    const size_t KF = m->kfs.size(), P = m->alive.size();
    std::vector<float> before(16 * (KF ? KF : 1)), after(16 * (KF ? KF : 1));
    for (size_t k = 0; k < KF; k++) memcpy(&before[16 * k], m->kfs[k].pose, sizeof(float) * 16);
    int rc = rs_pose_graph((int)KF, before.data(), h_loops, n_loops, four_dof, h_gravity, options, after.data(),
                           h_velocity_rotation, h_summary, nullptr, 0, nullptr);
    if (rc) return rs_fail(ctx, rc, "rs_pose_graph rejected its arguments");
    if (h_out_poses && KF) memcpy(h_out_poses, after.data(), sizeof(float) * 16 * KF);
    if (!h_summary->usable) return RS_OK;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = map_sync_device(m))) return rc;                 // the device image (positions, observation CSR) is current
    for (size_t k = 0; k < KF; k++) memcpy(m->kfs[k].pose, &after[16 * k], sizeof(float) * 16);      // Frame::set_pose, :503
    m->dirty_centres = true;
    if (P == 0) return RS_OK;
    if ((rc = rs_stage_begin(ctx))) return rc;
    float *d_before = nullptr, *d_after = nullptr;
    if ((rc = rs_stage_upload(ctx, before.data(), sizeof(float) * 16 * KF, (void**)&d_before))) return rc;
    if ((rc = rs_stage_upload(ctx, after.data(), sizeof(float) * 16 * KF, (void**)&d_after))) return rc;
    if ((rc = rs_transform_points(ctx, (int)P, m->d_obs_ptr, m->d_obs_kf, d_before, d_after, (int)KF, m->d_pos))) return rc;
    if ((rc = rs_stage_download(ctx, m->d_pos, sizeof(float) * 3 * P, m->pos.data()))) return rc;     // the mirror follows
    return rs_stage_sync(ctx);
}
