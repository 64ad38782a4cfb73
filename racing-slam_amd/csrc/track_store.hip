// track_store.hip — TrackStore on the device (reference src/TrackStore.cpp) and the key-frame decision's two counts
// (src/Mapper.cpp:91-140), so that a frame tracked against the resident map needs no list on the host:
//
//   k_ts_carry     TrackStore::carry_forward (:12-35) from rs_track_features' kept-index list and rs_estimate_pose's inlier
//                  list.  One workgroup; the first entry naming a previous keypoint and, among those, the first naming a
//                  current keypoint are found by atomicMin tables in LDS (frame_matches.hip's first-claim idiom): no serial
//                  walk even with repeats.  A carried track keeps its row: only keypoint -> row is rewritten.
//   k_ts_extend    TrackStore::extend (:37-54).  One workgroup: an exclusive scan over the unassigned keypoints hands out ids
//                  in keypoint order, an ordered scan over the in-use flags lists the free rows, then every track of the
//                  frame appends its sighting.
//   k_ts_query     Mapper::covisible_points and Mapper::unmapped_tracks (:91-120) plus the store's census: six integers.
//   k_ts_pack      the live tracks in ascending id order (a bitonic sort of (id - smallest id) << 13 | row in LDS) flattened
//                  to rs_triangulate_tracks' inputs, their sightings copied by k_ts_pack_copy, one wave per track; k_ts_results filters the accepted tracks' key-frame sightings;
//                  k_ts_erase applies the inconsistent list through the pack's order array.
//
// Layout: a pool of max_points rows of max_sightings sightings that never move; keypoint -> row is the only table carry
// rewrites.  Travel is sqrtf(fl(fl(dx dx) + fl(dy dy))): built with -ffp-contract=off.
#include <algorithm>

#include "common.h"

#define TS_THREADS 1024
#define TS_MAX 8192                 // keypoints per frame = rows of the pool (frame.hip's FRAME_MAX_POINTS)
#define TS_PER (TS_MAX / TS_THREADS)
#define TS_MAX_SIGHTINGS 128
#define TS_ROW_BITS 13              // a row index in a sort key

struct TsSighting { int32_t frame; float x, y; int32_t kf; int32_t kp; };      // 20 bytes, the download's five words

struct rs_track_store {
    rs_context* ctx = nullptr;
    int cap = 0, max_s = 0;
    rs_dev_block block;                         // every device array below is a piece of it
    rs_pin_block pin;                           // h_pin
    int32_t* d_kp_row = nullptr;                // [cap] keypoint of the current frame -> row or -1
    uint8_t* d_used = nullptr;                  // [cap] row in use
    unsigned long long* d_id = nullptr;         // [cap] per row
    int32_t* d_row_kp = nullptr;                // [cap]
    int32_t* d_count = nullptr;                 // [cap] sightings held
    TsSighting* d_sight = nullptr;              // [cap][max_s]
    unsigned long long* d_next_id = nullptr;    // [1]
    int32_t* d_query = nullptr;                 // [6] of 8
    // rs_triangulate_tracks' inputs and outputs for the tracks of the last pack
    int32_t* d_order = nullptr;                 // [cap] row of packed track t
    float* d_track_uv = nullptr; uint8_t* d_skip = nullptr; int32_t* d_sight_ptr = nullptr; int32_t* d_sight_pose = nullptr;
    float* d_sight_uv = nullptr; uint8_t* d_status = nullptr; float* d_xyz = nullptr; float* d_pc = nullptr; float* d_rc = nullptr;
    int32_t* d_accepted = nullptr; int32_t* d_inconsistent = nullptr;
    int32_t* d_counts = nullptr;                // [4] rs_triangulate_tracks' counts, tracks with a sighting outside the pose range
    int32_t* d_result = nullptr;                // header [8] | keypoint, sightings [T] | kf_ptr [T + 1] | track, inconsistent, parallax, required [T] | xyz [3 T] | pairs
    int32_t* h_pin = nullptr;                   // pinned: query [8] then the result block
    size_t result_ints = 0;
    // host bookkeeping: no call synchronises to learn these
    int n_live = 0;                             // live tracks where the host knows them (clear, extend, query), else -1
    int n_packed = -1;                          // tracks of the last pack while its order array still describes the store
    int n_inconsistent = 0;                     // counts[2] the last triangulate call read back
};

__device__ __forceinline__ int ts_count(const int32_t* d_count, int max_n)
{
    if (!d_count) return max_n;
    const int c = d_count[0];
    return c < 0 ? 0 : (c > max_n ? max_n : c);
}

// entry i of the list: current keypoint j and previous keypoint q; false = not an entry (out of range, or q holds no track)
__device__ __forceinline__ bool ts_entry(int i, int lim, int cap, const int32_t* __restrict__ kp_row, const int32_t* __restrict__ prev_index,
                                         const int32_t* __restrict__ inlier_index, int* j, int* q)
{
    *j = inlier_index ? inlier_index[i] : i;
    if ((uint32_t)*j >= (uint32_t)lim) return false;
    *q = prev_index[*j];
    return (uint32_t)*q < (uint32_t)cap && kp_row[*q] >= 0;
}

// dynamic LDS: new keypoint -> row [cap] | first entry per previous keypoint [cap] | per current keypoint [cap] | kept rows [cap] u8
__global__ __launch_bounds__(TS_THREADS) void k_ts_carry(int cap, int32_t* __restrict__ kp_row, uint8_t* __restrict__ used,
                                                        int32_t* __restrict__ row_kp, const int32_t* __restrict__ prev_index,
                                                        const int32_t* __restrict__ inlier_index, const int32_t* __restrict__ d_count, int max_n)
{
    extern __shared__ int32_t ts_lds[];
    int32_t* newrow = ts_lds, *firstq = ts_lds + cap, *firstj = ts_lds + 2 * cap;
    uint8_t* keep = (uint8_t*)(ts_lds + 3 * cap);
    const int n = ts_count(d_count, max_n), lim = max_n < cap ? max_n : cap, tid = threadIdx.x;
    for (int k = tid; k < cap; k += TS_THREADS) { newrow[k] = -1; firstq[k] = 0x7FFFFFFF; firstj[k] = 0x7FFFFFFF; keep[k] = 0; }
    __syncthreads();
    int j, q;
    for (int i = tid; i < n; i += TS_THREADS)
        if (ts_entry(i, lim, cap, kp_row, prev_index, inlier_index, &j, &q)) atomicMin(&firstq[q], i);
    __syncthreads();
    for (int i = tid; i < n; i += TS_THREADS)
        if (ts_entry(i, lim, cap, kp_row, prev_index, inlier_index, &j, &q) && firstq[q] == i) atomicMin(&firstj[j], i);
    __syncthreads();
    for (int i = tid; i < n; i += TS_THREADS) {
        if (!ts_entry(i, lim, cap, kp_row, prev_index, inlier_index, &j, &q) || firstq[q] != i || firstj[j] != i) continue;
        const int r = kp_row[q];
        newrow[j] = r;
        keep[r] = 1;
        row_kp[r] = j;
    }
    __syncthreads();
    for (int k = tid; k < cap; k += TS_THREADS) { kp_row[k] = newrow[k]; used[k] = keep[k]; }
}

// thread t owns keypoints and rows t * per ..: ids in keypoint order, free rows in row order
__global__ __launch_bounds__(TS_THREADS) void k_ts_extend(int cap, int max_s, int n, const float2* __restrict__ kp, int32_t* __restrict__ kp_row,
                                                         uint8_t* __restrict__ used, unsigned long long* __restrict__ id,
                                                         int32_t* __restrict__ row_kp, int32_t* __restrict__ count,
                                                         TsSighting* __restrict__ sight, unsigned long long* __restrict__ next_id,
                                                         int frame_index, int key_frame)
{
    __shared__ int32_t freelist[TS_MAX];
    const int per = (cap + TS_THREADS - 1) / TS_THREADS, k0 = threadIdx.x * per;
    const unsigned long long base = next_id[0];
    int nu = 0, nf = 0;
    for (int k = k0; k < k0 + per && k < cap; k++) {
        nu += (k < n && kp_row[k] < 0) ? 1 : 0;
        nf += used[k] ? 0 : 1;
    }
    int tot_u, tot_f;
    int ou = rs_block_exclusive_scan(nu, &tot_u);
    int of = rs_block_exclusive_scan(nf, &tot_f);
    for (int k = k0; k < k0 + per && k < cap; k++)
        if (!used[k]) freelist[of++] = k;
    __syncthreads();
    for (int k = k0; k < k0 + per && k < n; k++) {
        int r = kp_row[k];
        if (r < 0) {
            if (ou >= tot_f) continue;       // (live + unassigned <= cap: never taken)
            r = freelist[ou];
            used[r] = 1; id[r] = base + (unsigned long long)ou; row_kp[r] = k; count[r] = 0; kp_row[k] = r;
            ou++;
        }
        const int c = count[r];
        if (c < max_s) {
            const float2 p = kp[k];
            sight[(size_t)r * max_s + c] = TsSighting{frame_index, p.x, p.y, key_frame, k};
            count[r] = c + 1;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) next_id[0] = base + (unsigned long long)tot_u;
}

__global__ __launch_bounds__(TS_THREADS) void k_ts_query(int cap, int max_s, int n, const int32_t* __restrict__ table, int P,
                                                        const uint8_t* __restrict__ alive, const int32_t* __restrict__ obs_ptr,
                                                        const int32_t* __restrict__ obs_kf, int last_kf, const uint8_t* __restrict__ used,
                                                        const int32_t* __restrict__ row_kp, const int32_t* __restrict__ count,
                                                        const TsSighting* __restrict__ sight, int min_sightings, float min_travel,
                                                        const unsigned long long* __restrict__ next_id, int32_t* __restrict__ out)
{
    __shared__ int acc[5];
    const int tid = threadIdx.x;
    if (tid < 4) acc[tid] = 0;
    if (tid == 4) acc[4] = 0x7FFFFFFF;
    __syncthreads();
    int cov = 0, mat = 0, wait = 0, live = 0, first = 0x7FFFFFFF;
    for (int k = tid; k < n; k += TS_THREADS) {
        const int32_t p = table[k];
        if (p < 0) continue;
        mat++;                                                                  // Frame::num_map_matches
        if ((uint32_t)p >= (uint32_t)P || !alive[p] || last_kf < 0) continue;     // a removed point is not covisible
        for (int o = obs_ptr[p]; o < obs_ptr[p + 1]; o++)
            if (obs_kf[o] == last_kf) { cov++; break; }                         // MapPoint::is_observed_by, :96
    }
    for (int r = tid; r < cap; r += TS_THREADS) {
        if (!used[r]) continue;
        live++;
        const int c = count[r];
        if (c <= 0) continue;
        const TsSighting* s = sight + (size_t)r * max_s;
        first = min(first, s[0].frame);
        if (c < min_sightings) continue;                                        // :107
        const int k = row_kp[r];
        if ((uint32_t)k < (uint32_t)n && table[k] >= 0) continue;                // :110
        const float dx = s[c - 1].x - s[0].x, dy = s[c - 1].y - s[0].y;
        const float travel = sqrtf(dx * dx + dy * dy);                          // :113
        if (travel < min_travel) continue;                                      // :114
        wait++;
    }
    if (cov) atomicAdd(&acc[0], cov);
    if (mat) atomicAdd(&acc[1], mat);
    if (wait) atomicAdd(&acc[2], wait);
    if (live) atomicAdd(&acc[3], live);
    if (first != 0x7FFFFFFF) atomicMin(&acc[4], first);
    __syncthreads();
    if (tid == 0) {
        out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2]; out[3] = acc[3];
        out[4] = acc[3] ? acc[4] : -1;
        out[5] = (int32_t)(uint32_t)next_id[0];
    }
}

// dynamic LDS: n2 sort keys (n2 = a power of two >= T).  T is the host's count of live tracks; the kernel packs
// min(T, live rows) tracks and pads the rest as skipped tracks without sightings.  The host contract makes T the live
// count; were there more live rows than n2, the rows left out of the sort would be the highest ROWS, not the largest
// ids — memory-safe, but not the documented order.
__global__ __launch_bounds__(TS_THREADS) void k_ts_pack(int cap, int max_s, int T, int n2, int n, const float2* __restrict__ kp,
                                                       const int32_t* __restrict__ table, const uint8_t* __restrict__ used,
                                                       const unsigned long long* __restrict__ id, const int32_t* __restrict__ row_kp,
                                                       const int32_t* __restrict__ count, const TsSighting* __restrict__ sight,
                                                       int pose_base, int n_poses, int32_t* __restrict__ order, float2* __restrict__ track_uv,
                                                       uint8_t* __restrict__ skip, int32_t* __restrict__ sight_ptr,
                                                       int32_t* __restrict__ sight_pose, float2* __restrict__ sight_uv,
                                                       int32_t* __restrict__ n_out_of_range)
{
    extern __shared__ unsigned long long ts_keys[];
    __shared__ unsigned long long min_id;
    const int tid = threadIdx.x, per = (cap + TS_THREADS - 1) / TS_THREADS, r0 = tid * per;
    if (tid == 0) min_id = ~0ull;
    for (int i = tid; i < n2; i += TS_THREADS) ts_keys[i] = ~0ull;
    __syncthreads();
    int mine = 0;
    unsigned long long lo = ~0ull;
    for (int r = r0; r < r0 + per && r < cap; r++)
        if (used[r]) { mine++; lo = id[r] < lo ? id[r] : lo; }
    if (mine) atomicMin(&min_id, lo);
    int live;
    int at = rs_block_exclusive_scan(mine, &live);
    for (int r = r0; r < r0 + per && r < cap; r++)
        if (used[r] && at < n2) ts_keys[at++] = (id[r] - min_id) << TS_ROW_BITS | (unsigned long long)r;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += TS_THREADS) {
                const int x = i ^ j;
                if (x <= i) continue;
                const unsigned long long a = ts_keys[i], b = ts_keys[x];
                if ((a > b) == ((i & k) == 0)) { ts_keys[i] = b; ts_keys[x] = a; }
            }
            __syncthreads();
        }
    const int packed = live < T ? live : T, chunk = (T + TS_THREADS - 1) / TS_THREADS;
    const int t0 = min(tid * chunk, T), t1 = min(t0 + chunk, T);
    int ns = 0;
    for (int t = t0; t < t1; t++)
        if (t < packed) ns += count[(int)(ts_keys[t] & (TS_MAX - 1))];
    int total;
    int sp = rs_block_exclusive_scan(ns, &total);
    for (int t = t0; t < t1; t++) {
        const int row = t < packed ? (int)(ts_keys[t] & (TS_MAX - 1)) : -1;
        const int k = row >= 0 ? row_kp[row] : -1;
        const bool has_kp = (uint32_t)k < (uint32_t)n;
        order[t] = row;
        track_uv[t] = has_kp ? kp[k] : make_float2(0.f, 0.f);
        skip[t] = (!has_kp || table[k] >= 0) ? 1 : 0;                    // KeyFrame::is_matched, src/Mapper.cpp:248
        sight_ptr[t] = sp;
        sp += row >= 0 ? count[row] : 0;
    }
    if (tid == 0) { sight_ptr[T] = total; n_out_of_range[0] = 0; }
}

// the sightings of the packed tracks, one wave per track over the whole device (in one workgroup this copy was a chain of
// dependent loads per track and four fifths of the pack's time); a frame outside the pose range makes the track skipped
#define TS_COPY_WAVES 4
__global__ __launch_bounds__(64 * TS_COPY_WAVES) void k_ts_pack_copy(int max_s, int T, const int32_t* __restrict__ order,
                                                                     const int32_t* __restrict__ count, const TsSighting* __restrict__ sight,
                                                                     const int32_t* __restrict__ sight_ptr, int pose_base, int n_poses,
                                                                     uint8_t* __restrict__ skip, int32_t* __restrict__ sight_pose,
                                                                     float2* __restrict__ sight_uv, int32_t* __restrict__ n_out_of_range)
{
    const int lane = threadIdx.x & 63, t = blockIdx.x * TS_COPY_WAVES + (threadIdx.x >> 6);
    if (t >= T) return;                              // (the whole wave)
    const int row = order[t];
    const int c = row >= 0 ? min(count[row], max_s) : 0, s0 = sight_ptr[t];
    bool bad = false;
    for (int s = lane; s < c; s += 64) {
        const TsSighting g = sight[(size_t)row * max_s + s];
        const int pi = (int)((uint32_t)g.frame - (uint32_t)pose_base);
        sight_pose[s0 + s] = pi;
        sight_uv[s0 + s] = make_float2(g.x, g.y);
        bad |= (uint32_t)pi >= (uint32_t)n_poses;
    }
    if (__any(bad) && lane == 0) { skip[t] = 1; atomicAdd(n_out_of_range, 1); }
}

// the accepted tracks in rs_triangulate_tracks' order: keypoint, sighting count, position, and of the sightings only those
// made in a key frame as (handle, keypoint) pairs in CSR
__global__ __launch_bounds__(TS_THREADS) void k_ts_results(int T, int max_s, const int32_t* __restrict__ counts, const int32_t* __restrict__ accepted,
                                                          const int32_t* __restrict__ order, const int32_t* __restrict__ row_kp,
                                                          const int32_t* __restrict__ count, const TsSighting* __restrict__ sight,
                                                          const float* __restrict__ xyz, const float* __restrict__ pcs,
                                                          const float* __restrict__ rcs, const int32_t* __restrict__ inconsistent,
                                                          int32_t* __restrict__ out)
{
    int32_t* o_kp = out + 8, *o_ns = o_kp + T, *o_ptr = o_ns + T, *o_track = o_ptr + T + 1, *o_inc = o_track + T;
    float* o_pc = (float*)(o_inc + T), *o_rc = o_pc + T, *o_xyz = o_rc + T;
    int32_t* o_pair = (int32_t*)(o_xyz + 3 * (size_t)T);
    for (int i = threadIdx.x; i < min(max(counts[2], 0), T); i += TS_THREADS) o_inc[i] = inconsistent[i];
    const int na = min(max(counts[0], 0), T), chunk = (na + TS_THREADS - 1) / TS_THREADS;
    const int a0 = min((int)threadIdx.x * chunk, na), a1 = min(a0 + chunk, na);
    int np = 0;
    for (int a = a0; a < a1; a++) {
        const int t = accepted[a], row = (uint32_t)t < (uint32_t)T ? order[t] : -1;
        const int c = row >= 0 ? count[row] : 0;
        for (int s = 0; s < c; s++) np += sight[(size_t)row * max_s + s].kf >= 0 ? 1 : 0;
    }
    int total;
    int at = rs_block_exclusive_scan(np, &total);
    for (int a = a0; a < a1; a++) {
        const int t = accepted[a], row = (uint32_t)t < (uint32_t)T ? order[t] : -1;
        const int c = row >= 0 ? count[row] : 0;
        o_kp[a] = row >= 0 ? row_kp[row] : -1;
        o_ns[a] = c;
        o_ptr[a] = at;
        o_track[a] = t;
        o_pc[a] = row >= 0 ? pcs[t] : 0.f;
        o_rc[a] = row >= 0 ? rcs[t] : 0.f;
        for (int q = 0; q < 3; q++) o_xyz[3 * (size_t)a + q] = row >= 0 ? xyz[3 * (size_t)t + q] : 0.f;
        for (int s = 0; s < c; s++) {
            const TsSighting g = sight[(size_t)row * max_s + s];
            if (g.kf < 0) continue;
            o_pair[2 * (size_t)at] = g.kf; o_pair[2 * (size_t)at + 1] = g.kp;
            at++;
        }
    }
    if (threadIdx.x == 0) {
        o_ptr[na] = total;
        out[0] = counts[0]; out[1] = counts[1]; out[2] = counts[2]; out[3] = counts[3]; out[4] = T; out[5] = total; out[6] = 0; out[7] = 0;
    }
}

// TrackStore::erase for the inconsistent tracks of the last triangulate call (src/Mapper.cpp:333-335)
__global__ __launch_bounds__(TS_THREADS) void k_ts_erase(int T, int cap, const int32_t* __restrict__ counts, const int32_t* __restrict__ inconsistent,
                                                        const int32_t* __restrict__ order, uint8_t* __restrict__ used,
                                                        const int32_t* __restrict__ row_kp, int32_t* __restrict__ kp_row)
{
    const int ni = min(max(counts[2], 0), T);
    for (int i = threadIdx.x; i < ni; i += TS_THREADS) {
        const int t = inconsistent[i], row = (uint32_t)t < (uint32_t)T ? order[t] : -1;
        if (row < 0 || !used[row]) continue;
        used[row] = 0;
        const int k = row_kp[row];
        if ((uint32_t)k < (uint32_t)cap && kp_row[k] == row) kp_row[k] = -1;
    }
}

// ---------------------------------------------------------------------- host
static int ts_ok(rs_context* ctx, const rs_track_store* s) { return (ctx && s && s->ctx == ctx) ? RS_OK : RS_ERR_INVALID; }

static int ts_frame_ok(rs_context* ctx, const rs_track_store* s, const rs_frame* f, const char* what)
{
    if (!f || f->ctx != ctx) return rs_fail(ctx, RS_ERR_INVALID, "%s: no frame of this context", what);
    if (f->n > s->cap) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "%s: %d keypoints, the store holds %d", what, f->n, s->cap);
    return RS_OK;
}

extern "C" int rs_track_store_clear(rs_context* ctx, rs_track_store* s)
{
    if (ts_ok(ctx, s)) return RS_ERR_INVALID;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    RS_HIP(ctx, hipMemsetAsync(s->d_kp_row, 0xFF, sizeof(int32_t) * (size_t)s->cap, ctx->stream));
    RS_HIP(ctx, hipMemsetAsync(s->d_used, 0, (size_t)s->cap, ctx->stream));
    RS_HIP(ctx, hipMemsetAsync(s->d_next_id, 0, sizeof(unsigned long long), ctx->stream));
    RS_HIP(ctx, hipMemsetAsync(s->d_counts, 0, 4 * sizeof(int32_t), ctx->stream));
    s->n_live = 0; s->n_packed = -1; s->n_inconsistent = 0;
    return RS_OK;
}

extern "C" int rs_track_store_destroy(rs_track_store* s)
{
    if (!s) return RS_OK;
    if (s->ctx) {
        (void)hipSetDevice(s->ctx->device);
        (void)hipStreamSynchronize(s->ctx->stream);
    }
    delete s;
    return RS_OK;
}

extern "C" int rs_track_store_create(rs_context* ctx, int max_points, int max_sightings, rs_track_store** out)
{
    if (!ctx || !out) return RS_ERR_INVALID;
    *out = nullptr;
    if (max_points < 1 || max_points > TS_MAX)
        return rs_fail(ctx, RS_ERR_UNSUPPORTED, "rs_track_store_create: max_points %d outside 1 .. %d", max_points, TS_MAX);
    if (max_sightings < 1 || max_sightings > TS_MAX_SIGHTINGS)
        return rs_fail(ctx, RS_ERR_UNSUPPORTED, "rs_track_store_create: max_sightings %d outside 1 .. %d", max_sightings, TS_MAX_SIGHTINGS);
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_track_store* s = new rs_track_store;
    s->ctx = ctx; s->cap = max_points; s->max_s = max_sightings;
    const size_t cap = (size_t)max_points, all = cap * (size_t)max_sightings;
    s->result_ints = 8 + 10 * cap + 1 + 2 * all;
    int rc = s->block.carve(ctx, "rs_track_store_create: device block", [&](rs_carve& c) {
        s->d_kp_row = c.take<int32_t>(cap);
        s->d_used = c.take<uint8_t>(cap);
        s->d_id = c.take<unsigned long long>(cap);
        s->d_row_kp = c.take<int32_t>(cap);
        s->d_count = c.take<int32_t>(cap);
        s->d_sight = c.take<TsSighting>(all);
        s->d_next_id = c.take<unsigned long long>(1);
        s->d_query = c.take<int32_t>(8);
        s->d_order = c.take<int32_t>(cap);
        s->d_track_uv = c.take<float>(2 * cap);
        s->d_skip = c.take<uint8_t>(cap);
        s->d_sight_ptr = c.take<int32_t>(cap + 1);
        s->d_sight_pose = c.take<int32_t>(all);
        s->d_sight_uv = c.take<float>(2 * all);
        s->d_status = c.take<uint8_t>(cap);
        s->d_xyz = c.take<float>(3 * cap);
        s->d_pc = c.take<float>(cap);
        s->d_rc = c.take<float>(cap);
        s->d_accepted = c.take<int32_t>(cap);
        s->d_inconsistent = c.take<int32_t>(cap);
        s->d_counts = c.take<int32_t>(4);
        s->d_result = c.take<int32_t>(s->result_ints);
    });
    if (!rc) rc = s->pin.carve(ctx, "rs_track_store_create: pinned block", [&](rs_carve& c) { s->h_pin = c.take<int32_t>(8 + s->result_ints); });
    if (rc) { rs_track_store_destroy(s); return rc; }
    hipError_t e = hipMemsetAsync(s->block.p, 0, s->block.bytes, ctx->stream);
    if (e == hipSuccess) e = rs_lds_attr((const void*)k_ts_carry, 13 * (size_t)TS_MAX);
    if (e == hipSuccess) e = rs_lds_attr((const void*)k_ts_pack, 8 * (size_t)TS_MAX);
    rc = e == hipSuccess ? rs_track_store_clear(ctx, s) : rs_fail(ctx, RS_ERR_HIP, "rs_track_store_create: %s", hipGetErrorString(e));
    if (rc) { rs_track_store_destroy(s); return rc; }
    *out = s;
    return RS_OK;
}

extern "C" int rs_track_store_carry(rs_context* ctx, rs_track_store* s, const int32_t* d_prev_index, const int32_t* d_inlier_index,
                                    const int32_t* d_count, int max_n)
{
    if (ts_ok(ctx, s)) return RS_ERR_INVALID;
    if (max_n < 0) return rs_fail(ctx, RS_ERR_INVALID, "rs_track_store_carry: negative max_n");
    if (max_n > TS_MAX) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "rs_track_store_carry: max_n %d, at most %d", max_n, TS_MAX);
    if (max_n > 0 && !d_prev_index) return rs_fail(ctx, RS_ERR_INVALID, "rs_track_store_carry: null index list");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_prof_scope ps(ctx, "KT_carry");
    hipLaunchKernelGGL(k_ts_carry, dim3(1), dim3(TS_THREADS), 13 * (size_t)s->cap, ctx->stream, s->cap, s->d_kp_row, s->d_used, s->d_row_kp,
                       d_prev_index, d_inlier_index, d_count, max_n);
    RS_HIP(ctx, hipGetLastError());
    s->n_live = max_n == 0 ? 0 : -1;
    s->n_packed = -1;
    return RS_OK;
}

extern "C" int rs_track_store_extend(rs_context* ctx, rs_track_store* s, const rs_frame* f, int frame_index, int key_frame_handle)
{
    if (ts_ok(ctx, s)) return RS_ERR_INVALID;
    int rc = ts_frame_ok(ctx, s, f, "rs_track_store_extend");
    if (rc) return rc;
    s->n_packed = -1;
    if (f->n == 0) return RS_OK;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_prof_scope ps(ctx, "KT_extend");
    hipLaunchKernelGGL(k_ts_extend, dim3(1), dim3(TS_THREADS), 0, ctx->stream, s->cap, s->max_s, f->n, (const float2*)f->d_kp, s->d_kp_row,
                       s->d_used, s->d_id, s->d_row_kp, s->d_count, s->d_sight, s->d_next_id, frame_index, key_frame_handle < 0 ? -1 : key_frame_handle);
    RS_HIP(ctx, hipGetLastError());
    s->n_live = -1;             // (tracks carried to a keypoint beyond this frame stay alive: only the device counts them)
    return RS_OK;
}

extern "C" int rs_track_store_query(rs_context* ctx, rs_track_store* s, rs_map* m, const rs_frame* f, int last_key_frame, int min_sightings,
                                    float min_travel, int32_t h_out[6])
{
    if (ts_ok(ctx, s) || !h_out) return RS_ERR_INVALID;
    if (m && rs_map_context(m) != ctx) return rs_fail(ctx, RS_ERR_INVALID, "rs_track_store_query: a map of another context");
    int rc = ts_frame_ok(ctx, s, f, "rs_track_store_query");
    if (rc) return rc;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_map_track_view v{};
    if (m && (rc = rs_map_track_sync(m, 0, &v))) return rc;
    if (m && last_key_frame >= v.n_kf) return rs_fail(ctx, RS_ERR_INVALID, "rs_track_store_query: unknown key frame");
    {
        rs_prof_scope ps(ctx, "KT_query");
        hipLaunchKernelGGL(k_ts_query, dim3(1), dim3(TS_THREADS), 0, ctx->stream, s->cap, s->max_s, f->n, (const int32_t*)f->d_kp_point,
                           m ? v.mv.n_points : 0, v.d_alive, v.mv.d_obs_ptr, v.mv.d_obs_kf, m ? last_key_frame : -1, (const uint8_t*)s->d_used,
                           (const int32_t*)s->d_row_kp, (const int32_t*)s->d_count, (const TsSighting*)s->d_sight, min_sightings, min_travel,
                           (const unsigned long long*)s->d_next_id, s->d_query);
    }
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipMemcpyAsync(s->h_pin, s->d_query, 6 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(h_out, s->h_pin, 6 * sizeof(int32_t));
    s->n_live = h_out[3];
    return RS_OK;
}

extern "C" int rs_needs_key_frame(const int32_t h_query[6], int frame_gap, int last_key_frame_matches, int max_key_frame_gap,
                                  int new_tracks_threshold, int min_covisible_points, float min_covisible_fraction, int* h_out)
{
    if (!h_query || !h_out) return RS_ERR_INVALID;
    const int covisible = h_query[0], waiting = h_query[2];
    bool need;
    if (frame_gap < 0 || frame_gap >= max_key_frame_gap) need = true;                      // :125-128 (the gap is unsigned upstream)
    else if (waiting >= new_tracks_threshold) need = true;                                 // :134-136
    else need = covisible < min_covisible_points ||
                (float)covisible < min_covisible_fraction * (float)last_key_frame_matches;  // :137-139
    *h_out = need ? 1 : 0;
    return RS_OK;
}

extern "C" int rs_track_store_triangulate(rs_context* ctx, rs_track_store* s, rs_map* m, const rs_frame* f, const float* d_poses, int n_poses,
                                          int pose_base, int kf_pose, const float h_intrinsics[4], float any_parallax_cosine,
                                          float max_reprojection_error, float min_parallax_cosine, float rotation_parallax_factor,
                                          int min_new_points, const float* d_required_by_pose, rs_track_results* res)
{
    if (ts_ok(ctx, s) || !res) return RS_ERR_INVALID;
    if (m && rs_map_context(m) != ctx) return rs_fail(ctx, RS_ERR_INVALID, "rs_track_store_triangulate: a map of another context");
    int rc = ts_frame_ok(ctx, s, f, "rs_track_store_triangulate");
    if (rc) return rc;
    if (s->n_live < 0) return rs_fail(ctx, RS_ERR_INVALID, "rs_track_store_triangulate: the number of live tracks is not known: call rs_track_store_query first");
    const int T = s->n_live;
    if (res->capacity_tracks < T || res->capacity_pairs < 0 || (T > 0 && (!res->h_keypoint || !res->h_xyz || !res->h_sightings || !res->h_kf_ptr)) ||
        (res->capacity_pairs > 0 && !res->h_kf_pairs))
        return rs_fail(ctx, RS_ERR_INVALID, "rs_track_store_triangulate: results hold %d tracks, %d are live", res->capacity_tracks, T);
    if (n_poses < 1 || kf_pose < 0 || kf_pose >= n_poses || !d_poses || !h_intrinsics)
        return rs_fail(ctx, RS_ERR_INVALID, "rs_track_store_triangulate: poses");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    res->counts[0] = res->counts[1] = res->counts[2] = 0;
    res->out_of_range = 0; res->n_tracks = T; res->n_pairs = 0;
    s->n_packed = -1; s->n_inconsistent = 0;        // (a pack is valid only once every launch below was issued)
    if (T == 0) {
        RS_HIP(ctx, hipMemsetAsync(s->d_counts, 0, 4 * sizeof(int32_t), ctx->stream));
        if (res->h_kf_ptr) res->h_kf_ptr[0] = 0;
        s->n_packed = 0;
        return RS_OK;
    }
    int n2 = 2;
    while (n2 < T) n2 *= 2;
    {
        rs_prof_scope ps(ctx, "KT_pack");
        hipLaunchKernelGGL(k_ts_pack, dim3(1), dim3(TS_THREADS), sizeof(unsigned long long) * (size_t)n2, ctx->stream, s->cap, s->max_s, T, n2, f->n,
                           (const float2*)f->d_kp, (const int32_t*)f->d_kp_point, (const uint8_t*)s->d_used, (const unsigned long long*)s->d_id,
                           (const int32_t*)s->d_row_kp, (const int32_t*)s->d_count, (const TsSighting*)s->d_sight, pose_base, n_poses, s->d_order,
                           (float2*)s->d_track_uv, s->d_skip, s->d_sight_ptr, s->d_sight_pose, (float2*)s->d_sight_uv, s->d_counts + 3);
    }
    {
        rs_prof_scope ps(ctx, "KT_pack_copy");
        hipLaunchKernelGGL(k_ts_pack_copy, dim3((T + TS_COPY_WAVES - 1) / TS_COPY_WAVES), dim3(64 * TS_COPY_WAVES), 0, ctx->stream, s->max_s, T,
                           (const int32_t*)s->d_order, (const int32_t*)s->d_count, (const TsSighting*)s->d_sight, (const int32_t*)s->d_sight_ptr,
                           pose_base, n_poses, s->d_skip, s->d_sight_pose, (float2*)s->d_sight_uv, s->d_counts + 3);
    }
    RS_HIP(ctx, hipGetLastError());
    if ((rc = rs_triangulate_tracks(ctx, T, s->d_track_uv, s->d_skip, s->d_sight_ptr, s->d_sight_pose, s->d_sight_uv, d_poses, n_poses, kf_pose,
                                    h_intrinsics, any_parallax_cosine, max_reprojection_error, min_parallax_cosine, rotation_parallax_factor,
                                    min_new_points, s->d_status, s->d_xyz, s->d_pc, s->d_rc, s->d_accepted, s->d_inconsistent, s->d_counts,
                                    d_required_by_pose)))
        return rc;
    {
        rs_prof_scope ps(ctx, "KT_results");
        hipLaunchKernelGGL(k_ts_results, dim3(1), dim3(TS_THREADS), 0, ctx->stream, T, s->max_s, (const int32_t*)s->d_counts,
                           (const int32_t*)s->d_accepted, (const int32_t*)s->d_order, (const int32_t*)s->d_row_kp, (const int32_t*)s->d_count,
                           (const TsSighting*)s->d_sight, (const float*)s->d_xyz, (const float*)s->d_pc, (const float*)s->d_rc,
                           (const int32_t*)s->d_inconsistent, s->d_result);
    }
    RS_HIP(ctx, hipGetLastError());
    s->n_packed = T;
    // one read-back of the head and of as many pairs as a key frame usually has (two per track); only a key frame with
    // more than that pays a second copy and synchronisation for the rest, so the download stays as small as the filter made it
    const size_t all = (size_t)s->cap * (size_t)s->max_s, head = 8 + 10 * (size_t)T + 1;
    const size_t room = std::min((size_t)res->capacity_pairs, all), first = std::min(room, 2 * (size_t)T);
    int32_t* h = s->h_pin + 8;
    RS_HIP(ctx, hipMemcpyAsync(h, s->d_result, sizeof(int32_t) * (head + 2 * first), hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t pairs = std::min(room, (size_t)std::max(h[5], 0));
    if (pairs > first) {
        RS_HIP(ctx, hipMemcpyAsync(h + head + 2 * first, s->d_result + head + 2 * first, sizeof(int32_t) * 2 * (pairs - first),
                                   hipMemcpyDeviceToHost, ctx->stream));
        RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    memcpy(res->counts, h, 3 * sizeof(int32_t));
    res->out_of_range = h[3]; res->n_pairs = h[5];
    const size_t na = (size_t)std::min(std::max(h[0], 0), T), ni = (size_t)std::min(std::max(h[2], 0), T);
    const int32_t* p = h + 8;
    memcpy(res->h_keypoint, p, 4 * na); p += T;
    memcpy(res->h_sightings, p, 4 * na); p += T;
    memcpy(res->h_kf_ptr, p, 4 * (na + 1)); p += T + 1;
    if (res->h_track) memcpy(res->h_track, p, 4 * na);
    p += T;
    if (res->h_inconsistent) memcpy(res->h_inconsistent, p, 4 * ni);
    p += T;
    if (res->h_parallax_cos) memcpy(res->h_parallax_cos, p, 4 * na);
    p += T;
    if (res->h_required_cos) memcpy(res->h_required_cos, p, 4 * na);
    p += T;
    memcpy(res->h_xyz, p, 12 * na); p += 3 * (size_t)T;
    if (pairs) memcpy(res->h_kf_pairs, p, 8 * pairs);
    s->n_inconsistent = std::min(std::max(h[2], 0), T);
    return RS_OK;
}

extern "C" int rs_track_store_erase_inconsistent(rs_context* ctx, rs_track_store* s)
{
    if (ts_ok(ctx, s)) return RS_ERR_INVALID;
    if (s->n_packed <= 0) return RS_OK;          // no triangulate call since the store last changed: nothing to apply
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_prof_scope ps(ctx, "KT_erase");
    hipLaunchKernelGGL(k_ts_erase, dim3(1), dim3(TS_THREADS), 0, ctx->stream, s->n_packed, s->cap, (const int32_t*)s->d_counts,
                       (const int32_t*)s->d_inconsistent, (const int32_t*)s->d_order, s->d_used, (const int32_t*)s->d_row_kp, s->d_kp_row);
    RS_HIP(ctx, hipGetLastError());
    if (s->n_live >= 0) s->n_live -= s->n_inconsistent;
    s->n_packed = -1; s->n_inconsistent = 0;
    return RS_OK;
}

extern "C" int rs_track_store_download(rs_context* ctx, const rs_track_store* s, int* h_n, uint64_t* h_next_id, uint64_t* h_id, int32_t* h_keypoint,
                                       int32_t* h_count, int32_t* h_sightings)
{
    if (ts_ok(ctx, s)) return RS_ERR_INVALID;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cap = (size_t)s->cap;
    std::vector<uint8_t> used(cap);
    std::vector<unsigned long long> id(cap);
    std::vector<int32_t> kp(cap), cnt(cap);
    unsigned long long next = 0;
    RS_HIP(ctx, hipMemcpyAsync(used.data(), s->d_used, cap, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipMemcpyAsync(id.data(), s->d_id, 8 * cap, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipMemcpyAsync(kp.data(), s->d_row_kp, 4 * cap, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipMemcpyAsync(cnt.data(), s->d_count, 4 * cap, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipMemcpyAsync(&next, s->d_next_id, 8, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int> rows;
    for (size_t r = 0; r < cap; r++)
        if (used[r]) rows.push_back((int)r);
    std::sort(rows.begin(), rows.end(), [&](int a, int b) { return id[(size_t)a] < id[(size_t)b]; });
    if (h_n) *h_n = (int)rows.size();
    if (h_next_id) *h_next_id = next;
    const size_t row_bytes = sizeof(TsSighting) * (size_t)s->max_s;
    std::vector<TsSighting> pool;
    if (h_sightings && !rows.empty()) {
        pool.resize(cap * (size_t)s->max_s);
        RS_HIP(ctx, hipMemcpy(pool.data(), s->d_sight, row_bytes * cap, hipMemcpyDeviceToHost));
    }
    for (size_t t = 0; t < rows.size(); t++) {
        const size_t r = (size_t)rows[t];
        if (h_id) h_id[t] = id[r];
        if (h_keypoint) h_keypoint[t] = kp[r];
        if (h_count) h_count[t] = cnt[r];
        if (h_sightings)
            memcpy((char*)h_sightings + t * row_bytes, (const char*)pool.data() + r * row_bytes,
                   sizeof(TsSighting) * (size_t)std::min(std::max(cnt[r], 0), s->max_s));
    }
    return RS_OK;
}

extern "C" int rs_track_store_download_packed(rs_context* ctx, const rs_track_store* s, int* h_n_tracks, int* h_n_sightings, float* h_track_uv,
                                              uint8_t* h_skip, int32_t* h_sight_ptr, int32_t* h_sight_pose, float* h_sight_uv,
                                              int capacity_sightings)
{
    if (ts_ok(ctx, s) || !h_n_tracks || !h_n_sightings) return RS_ERR_INVALID;
    *h_n_tracks = *h_n_sightings = 0;
    if (s->n_packed <= 0) return RS_OK;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t T = (size_t)s->n_packed;
    int32_t S = 0;
    RS_HIP(ctx, hipMemcpy(&S, s->d_sight_ptr + T, 4, hipMemcpyDeviceToHost));
    *h_n_tracks = (int)T; *h_n_sightings = S;
    if (h_track_uv) RS_HIP(ctx, hipMemcpy(h_track_uv, s->d_track_uv, 8 * T, hipMemcpyDeviceToHost));
    if (h_skip) RS_HIP(ctx, hipMemcpy(h_skip, s->d_skip, T, hipMemcpyDeviceToHost));
    if (h_sight_ptr) RS_HIP(ctx, hipMemcpy(h_sight_ptr, s->d_sight_ptr, 4 * (T + 1), hipMemcpyDeviceToHost));
    if (S > 0 && S <= capacity_sightings) {
        if (h_sight_pose) RS_HIP(ctx, hipMemcpy(h_sight_pose, s->d_sight_pose, 4 * (size_t)S, hipMemcpyDeviceToHost));
        if (h_sight_uv) RS_HIP(ctx, hipMemcpy(h_sight_uv, s->d_sight_uv, 8 * (size_t)S, hipMemcpyDeviceToHost));
    }
    return RS_OK;
}
