// map_fuse.hip — Mapper::fuse_loop (reference src/Mapper.cpp:41-77,176-220) on the resident map: rs_map_fuse_loop.
//
// What the reference's loop requires:
//   1  the old set (candidate + covisibles, their points) is fixed at entry; an old point is only ever kept, so the sources of
//      match_for_fuse stay alive and their observation rows only grow;
//   2  the window's frames depend on each other: a fuse in frame i moves observations (and with them descriptors, the viewing
//      normal, the distance range, and "already observed by frame j") that frame j > i must see — the device state evolves
//      frame by frame;
//   3  the accepted matches of ONE frame touch disjoint rows and table entries (distinct keypoints, distinct sources, distinct
//      discarded points, none of them a source): they are applied in parallel, one lane per match;
//   4  sources compete in ascending slot order; covisibles rank by count descending, handle ascending.
//
// Two host synchronisations per call (the old frames + S; the journal) plus the map's lazy upload; a third read-back with
// options->check.  The first call at a size also synchronises where it allocates, and the staging pool is drained once
// between stage 1 and stage 3: never between two window frames.
//
// The working state of stage 3 is: the sources' observation rows as a dense CSR of their own (rebuilt per frame into the
// other of two buffers: count, scan, copy, append), the image's key-frame tables (d_kp_point, marked dirty on the mirror
// before the first launch), and a copy of the alive bytes.  A discarded point is never a source, never gains an observation
// and loses them only by dying, so its row is read from the map's image, which stage 3 never writes.  The map keeps tables
// and observation lists consistent (table[kf][kp] == p  <=>  (kf, kp) is an observation of p), so "the key frame matches the
// point" is read from the point's row.  The mirror's replay of the journal recomputes every outcome with the reference's
// full conditions; the device supplies matches, not decisions.
//
//   FL1 k_fuse_shared     one lane per candidate keypoint walks its point's row: shared[kf]++ (integer atomics)
//   FL2 k_fuse_rank       one workgroup: up to max_covisible rounds of "largest (count, -handle) below the last winner"
//   FL3 k_fuse_mark_old   a byte per point slot from the old frames' table rows
//   FL4 k_fuse_compact    the sources in ascending slot order (ordered scan, chunks of 1024)
//   FL5 k_fuse_scan       row offsets of the next CSR: exclusive scan of (old length + appended) in one workgroup
//   FL6 k_fuse_gather     the source view from the image (rows, positions)
//   FL7 k_fuse_eligible   alive and not observed by the frame, from the current rows
//   FL8 k_fuse_count / k_fuse_copy / k_fuse_apply     the fuses of one frame
#include "common.h"
#include "map_mirror.h"

#define FUSE_MAX_KP 8192
#define FUSE_HDR (RS_FUSE_MAX_COVISIBLE + 3)      // old frames [65] | n_old | S

#define FUSE_FIRST 4096                           // first capacity of the three scratch arrays; nothing in them outlives a call
struct FuseScratch {
    rs_frame* frame = nullptr;                    // the reusable internal frame of stage 3
    rs_dev_array<int32_t> d_pro;                  // prologue: shared [KF] | hdr [FUSE_HDR] | src_slot [P]
    rs_dev_array<int32_t> d_win;                  // stage 3 (carved in rs_map_fuse_loop)
    rs_dev_array<uint8_t> d_u8;                   // is_old [P] | alive copy [P] | eligible [P] | zeros [FUSE_MAX_KP]
};

void rs_map_fuse_release(void* scratch)           // (rs_map_destroy has made the device current and drained the stream)
{
    FuseScratch* s = (FuseScratch*)scratch;
    if (!s) return;
    if (s->frame) (void)rs_frame_destroy(s->frame);
    delete s;
}

// ------------------------------------------------------------------------------------------------ prologue
__global__ __launch_bounds__(256) void k_fuse_shared(int n, int row0, int candidate, const int32_t* __restrict__ kp_point,
                                                     const int32_t* __restrict__ obs_ptr, const int32_t* __restrict__ obs_kf,
                                                     int P, int KF, int32_t* __restrict__ shared)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = kp_point[row0 + i];
    if (p < 0 || p >= P) return;
    for (int o = obs_ptr[p]; o < obs_ptr[p + 1]; o++) {
        const int kf = obs_kf[o];
        if (kf != candidate && kf >= 0 && kf < KF) atomicAdd(&shared[kf], 1);       // src/Mapper.cpp:46
    }
}

// hdr: [0 .. 64] the old frames, [65] their number, [66] S (k_fuse_compact)
__global__ __launch_bounds__(1024) void k_fuse_rank(int KF, const int32_t* __restrict__ shared, int candidate, int min_shared,
                                                    int max_covisible, int32_t* __restrict__ hdr)
{
    __shared__ unsigned long long best;
    unsigned long long prev = ~0ull;
    int n_old = 1;
    for (int r = 0; r < max_covisible; r++) {
        if (threadIdx.x == 0) best = 0ull;
        __syncthreads();
        unsigned long long lmax = 0ull;
        for (int k = threadIdx.x; k < KF; k += blockDim.x) {
            const int c = shared[k];
            if (c > 0 && c >= min_shared) {
                const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)k);
                if (key < prev && key > lmax) lmax = key;
            }
        }
        if (lmax) atomicMax(&best, lmax);
        __syncthreads();
        const unsigned long long b = best;
        __syncthreads();
        if (b == 0ull) break;                      // (uniform: every lane read the same word)
        if (threadIdx.x == 0) hdr[n_old] = (int32_t)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull));
        prev = b;
        n_old++;
    }
    if (threadIdx.x == 0) { hdr[0] = candidate; hdr[RS_FUSE_MAX_COVISIBLE + 1] = n_old; }
}

// grid.y = position in the old list
__global__ __launch_bounds__(256) void k_fuse_mark_old(const int32_t* __restrict__ hdr, const int32_t* __restrict__ kf_row,
                                                       const int32_t* __restrict__ kf_n, const int32_t* __restrict__ kp_point, int P,
                                                       uint8_t* __restrict__ is_old)
{
    if ((int)blockIdx.y >= hdr[RS_FUSE_MAX_COVISIBLE + 1]) return;
    const int kf = hdr[blockIdx.y];
    const int n = kf_n[kf], r0 = kf_row[kf];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int p = kp_point[r0 + i];
        if (p >= 0 && p < P) is_old[p] = 1;        // (every writer of a byte stores the same value)
    }
}

__global__ __launch_bounds__(1024) void k_fuse_compact(int P, const uint8_t* __restrict__ is_old, int32_t* __restrict__ src_slot,
                                                       int32_t* __restrict__ n_src)
{
    int carry = 0;
    for (int base = 0; base < P; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const int f = i < P ? is_old[i] : 0;
        int tot;
        const int off = carry + rs_block_exclusive_scan(f, &tot);
        if (f) src_slot[off] = i;
        carry += tot;
    }
    if (threadIdx.x == 0) n_src[0] = carry;
}

// ------------------------------------------------------------------------------------------------ the source view
// ptr[s] = exclusive scan of (old row length + add[s]); ptr[S] = the total.  old_ptr NULL: lengths are add alone.
__global__ __launch_bounds__(1024) void k_fuse_scan(int S, const int32_t* __restrict__ old_ptr, const int32_t* __restrict__ add,
                                                    int32_t* __restrict__ ptr)
{
    int carry = 0;
    for (int base = 0; base < S; base += 1024) {
        const int s = base + (int)threadIdx.x;
        const int v = s < S ? (old_ptr ? old_ptr[s + 1] - old_ptr[s] : 0) + add[s] : 0;
        int tot;
        const int off = carry + rs_block_exclusive_scan(v, &tot);
        if (s < S) ptr[s] = off;
        carry += tot;
    }
    if (threadIdx.x == 0) ptr[S] = carry;
}

__global__ __launch_bounds__(256) void k_fuse_row_len(int S, const int32_t* __restrict__ src_slot, const int32_t* __restrict__ obs_ptr,
                                                      int32_t* __restrict__ len)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) len[s] = obs_ptr[src_slot[s] + 1] - obs_ptr[src_slot[s]];
}

__global__ __launch_bounds__(256) void k_fuse_gather(int S, const int32_t* __restrict__ src_slot, const int32_t* __restrict__ obs_ptr,
                                                     const int32_t* __restrict__ obs_kf, const int32_t* __restrict__ obs_desc,
                                                     const float* __restrict__ pos, const int32_t* __restrict__ ptr,
                                                     int32_t* __restrict__ v_kf, int32_t* __restrict__ v_desc, float* __restrict__ v_pos)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int p = src_slot[s], o0 = obs_ptr[p], n = obs_ptr[p + 1] - o0, w = ptr[s];
    for (int k = 0; k < n; k++) { v_kf[w + k] = obs_kf[o0 + k]; v_desc[w + k] = obs_desc[o0 + k]; }
#pragma unroll
    for (int c = 0; c < 3; c++) v_pos[3 * (size_t)s + c] = pos[3 * (size_t)p + c];
}

// src/MapMatcher.cpp:53 for match_for_fuse: the frame does not observe the point, read from the point's CURRENT row
__global__ __launch_bounds__(256) void k_fuse_eligible(int S, const int32_t* __restrict__ src_slot, const uint8_t* __restrict__ alive,
                                                       const int32_t* __restrict__ ptr, const int32_t* __restrict__ v_kf, int frame_kf,
                                                       uint8_t* __restrict__ elig)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    bool e = alive[src_slot[s]] != 0;
    for (int o = ptr[s]; o < ptr[s + 1]; o++) e = e && v_kf[o] != frame_kf;
    elig[s] = e ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ the fuses of one frame
struct FuseFrame {
    int kf, row0, n;                        // the window key frame: handle, first pool row, keypoints
    int S, P;
    const int32_t* cnt;                     // [1] accepted matches (K3)
    const int32_t* m_kp;                    // [n] their keypoints, ascending
    const int32_t* m_view;                  // [n] their sources (view index)
    int32_t* m_slot;                        // [n] out: the sources' point slots (the journal)
    const int32_t* src_slot;
    const uint8_t* is_old;
    const int32_t *obs_ptr, *obs_kf, *obs_desc;      // the map's image: rows of the discarded points
    const int32_t *ptr, *v_kf, *v_desc;     // current source rows
};

__device__ __forceinline__ bool fuse_row_has(const FuseFrame& f, int s, int kf)
{
    for (int o = f.ptr[s]; o < f.ptr[s + 1]; o++)
        if (f.v_kf[o] == kf) return true;
    return false;
}

// Mapper::fuse_match for match i on the device's state.  Returns the number of observations source s gains and the discarded
// point (-1: none; then a gain of 1 is the association of the free keypoint).
__device__ __forceinline__ int fuse_decide(const FuseFrame& f, const int32_t* __restrict__ kp_point, int i, int* s_out, int* d_out)
{
    const int kp = f.m_kp[i], s = f.m_view[i];
    *s_out = s; *d_out = -1;
    if (kp < 0 || kp >= f.n || s < 0 || s >= f.S) return 0;
    const int existing = kp_point[f.row0 + kp];
    if (existing < 0) return fuse_row_has(f, s, f.kf) ? 0 : 1;           // src/Mapper.cpp:184-190
    if (existing >= f.P || existing == f.src_slot[s] || f.is_old[existing]) return 0;      // :192
    *d_out = existing;
    int gain = 0;
    for (int o = f.obs_ptr[existing]; o < f.obs_ptr[existing + 1]; o++)   // src/Map.cpp:84-90
        gain += fuse_row_has(f, s, f.obs_kf[o]) ? 0 : 1;
    return gain;
}

__global__ __launch_bounds__(256) void k_fuse_count(FuseFrame f, const int32_t* __restrict__ kp_point, int32_t* __restrict__ add)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = min(max(f.cnt[0], 0), f.n);
    if (i >= n) return;
    int s, d;
    const int gain = fuse_decide(f, kp_point, i, &s, &d);
    const bool in = s >= 0 && s < f.S;
    f.m_slot[i] = in ? f.src_slot[s] : -1;
    if (in) add[s] = gain;                  // (a source is accepted by at most one keypoint of a frame)
}

__global__ __launch_bounds__(256) void k_fuse_copy(int S, const int32_t* __restrict__ ptr, const int32_t* __restrict__ v_kf,
                                                   const int32_t* __restrict__ v_desc, const int32_t* __restrict__ new_ptr,
                                                   int32_t* __restrict__ n_kf, int32_t* __restrict__ n_desc)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int o0 = ptr[s], n = ptr[s + 1] - o0, w = new_ptr[s];
    for (int k = 0; k < n; k++) { n_kf[w + k] = v_kf[o0 + k]; n_desc[w + k] = v_desc[o0 + k]; }
}

// The appended observations go behind the copied row in the discarded point's observation order; the tables and the alive copy follow.
__global__ __launch_bounds__(256) void k_fuse_apply(FuseFrame f, int32_t* __restrict__ kp_point, uint8_t* __restrict__ alive,
                                                    const int32_t* __restrict__ new_ptr, int32_t* __restrict__ n_kf,
                                                    int32_t* __restrict__ n_desc)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = min(max(f.cnt[0], 0), f.n);
    if (i >= n) return;
    int s, d;
    const int gain = fuse_decide(f, kp_point, i, &s, &d);
    if (s < 0 || s >= f.S) return;
    const int kept = f.src_slot[s];
    int w = new_ptr[s] + (f.ptr[s + 1] - f.ptr[s]);
    const int end = new_ptr[s + 1];         // (w + gain == end by k_fuse_count; the bound keeps a contradiction inside the row)
    if (d < 0) {
        if (gain == 1 && w < end) {                                       // Map::associate at a free keypoint
            n_kf[w] = f.kf; n_desc[w] = f.row0 + f.m_kp[i];
            kp_point[f.row0 + f.m_kp[i]] = kept;
        }
        return;
    }
    for (int o = f.obs_ptr[d]; o < f.obs_ptr[d + 1]; o++) {
        const int kf = f.obs_kf[o], row = f.obs_desc[o];
        if (fuse_row_has(f, s, kf)) { if (kp_point[row] == d) kp_point[row] = -1; continue; }       // disassociated, kept already there
        if (w < end) { n_kf[w] = kf; n_desc[w] = row; w++; }
        kp_point[row] = kept;
    }
    alive[d] = 0;                                                         // Map::remove_point
}

// ------------------------------------------------------------------------------------------------ the call
static int fuse_bad(rs_context* ctx, int code, const char* what) { return rs_fail(ctx, code, "rs_map_fuse_loop: %s", what); }

extern "C" int rs_map_fuse_loop(rs_context* ctx, rs_map* map, int query_kf, int candidate_kf, const int32_t* h_inlier_kp,
                                const int32_t* h_inlier_point, int n_inliers, const int32_t* h_window_kfs, int n_window,
                                const rs_fuse_options* opt, rs_fuse_report* rep, int32_t* h_section_ptr, int32_t* h_kp, int32_t* h_point,
                                int32_t* h_outcome, int capacity, int* h_n_entries)
{
    if (!ctx || !map || !opt || !rep || rs_map_context(map) != ctx) return RS_ERR_INVALID;
    if (n_inliers < 0 || n_window < 0 || (n_inliers > 0 && (!h_inlier_kp || !h_inlier_point)) || (n_window > 0 && !h_window_kfs))
        return fuse_bad(ctx, RS_ERR_INVALID, "null or negative list");
    rs_map_fuse_view mv;
    int rc = rs_map_fuse_sync(map, 0, &mv);
    if (rc) return rc;
    MapMirror* m = mv.mirror;
    const int KF = (int)m->kfs.size();
    if (!mirror_kf_ok(m, query_kf) || !mirror_kf_ok(m, candidate_kf)) return fuse_bad(ctx, RS_ERR_INVALID, "unknown key frame");
    // The order is deliberate: every window entry is checked to be a key frame BEFORE it indexes `listed` [KF], and unknown or
    // repeated entries are refused (RS_ERR_INVALID) before the envelope is looked at (RS_ERR_UNSUPPORTED), whatever n_window is.
    std::vector<uint8_t> listed((size_t)KF, 0);
    for (int w = 0; w < n_window; w++) {
        if (!mirror_kf_ok(m, h_window_kfs[w])) return fuse_bad(ctx, RS_ERR_INVALID, "unknown key frame in the window");
        if (listed[(size_t)h_window_kfs[w]]) return fuse_bad(ctx, RS_ERR_INVALID, "key frame listed twice in the window");
        listed[(size_t)h_window_kfs[w]] = 1;
    }
    if (n_window > RS_FUSE_MAX_WINDOW || n_inliers > RS_FUSE_MAX_INLIERS || opt->max_covisible < 0 || opt->max_covisible > RS_FUSE_MAX_COVISIBLE)
        return fuse_bad(ctx, RS_ERR_UNSUPPORTED, "window, inlier list or max_covisible outside the envelope");
    if (m->kfs[(size_t)query_kf].n > FUSE_MAX_KP || m->kfs[(size_t)candidate_kf].n > FUSE_MAX_KP)
        return fuse_bad(ctx, RS_ERR_UNSUPPORTED, "a key frame of more than 8192 keypoints");
    for (int w = 0; w < n_window; w++)
        if (m->kfs[(size_t)h_window_kfs[w]].n > FUSE_MAX_KP) return fuse_bad(ctx, RS_ERR_UNSUPPORTED, "a key frame of more than 8192 keypoints");
    // what stage 3 reads of the map rests on tables and observation lists agreeing; the self-check makes that testable
    if (opt->check && !mirror_consistent(m)) return fuse_bad(ctx, RS_ERR_INTERNAL, "the key-frame tables and the observation lists disagree");
    // ---- every check is done: from here on the map is edited
    const int rep_src_cap = opt->h_sources ? opt->capacity_sources : 0;
    int32_t* const rep_rem = opt->h_removed; const int rep_rem_cap = opt->h_removed ? opt->capacity_removed : 0;
    int bad_rank = 0;                       // check: the device's old frames against mirror_loop_old_frames
    rep->n_old_frames = 1; rep->old_frames[0] = candidate_kf; rep->n_sources = 0; rep->n_removed = 0; rep->device_state_mismatches = -1;
    for (int k = 0; k < 6; k++) rep->outcomes[k] = 0;
    if (h_n_entries) *h_n_entries = 0;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t P = m->alive.size();
    FuseScratch* fs = (FuseScratch*)*mv.scratch;
    if (!fs) { fs = new FuseScratch(); *mv.scratch = fs; }
    std::vector<int32_t> hdr(FUSE_HDR, 0), sources;
    hdr[0] = candidate_kf; hdr[RS_FUSE_MAX_COVISIBLE + 1] = 1;
    int32_t *d_shared = nullptr, *d_hdr = nullptr, *d_src = nullptr;
    uint8_t *d_old = nullptr, *d_alive_w = nullptr, *d_elig = nullptr, *d_zero = nullptr;
    if (P > 0) {
        // ---- stage 1: the prologue on the entry image
        if ((rc = rs_map_fuse_sync(map, 1, &mv))) return rc;
        if ((rc = fs->d_pro.reserve(ctx, (size_t)KF + FUSE_HDR + P, FUSE_FIRST))) return rc;
        if ((rc = fs->d_u8.reserve(ctx, 3 * P + FUSE_MAX_KP, FUSE_FIRST))) return rc;
        d_shared = fs->d_pro; d_hdr = d_shared + KF; d_src = d_hdr + FUSE_HDR;
        d_old = fs->d_u8; d_alive_w = d_old + P; d_elig = d_alive_w + P; d_zero = d_elig + P;
        std::vector<int32_t> kf_tab(2 * (size_t)KF);
        for (int k = 0; k < KF; k++) { kf_tab[(size_t)k] = m->kfs[(size_t)k].pool_row; kf_tab[(size_t)KF + k] = m->kfs[(size_t)k].n; }
        if ((rc = rs_stage_begin(ctx))) return rc;
        int32_t* d_kf_tab = nullptr;
        if ((rc = rs_stage_upload(ctx, kf_tab.data(), sizeof(int32_t) * kf_tab.size(), (void**)&d_kf_tab))) return rc;
        RS_HIP(ctx, hipMemsetAsync(d_shared, 0, sizeof(int32_t) * ((size_t)KF + FUSE_HDR), st));
        RS_HIP(ctx, hipMemsetAsync(d_old, 0, P, st));
        const MapKeyFrame& ck = m->kfs[(size_t)candidate_kf];
        {
            rs_prof_scope ps(ctx, "FL_fuse_prologue");
            if (ck.n > 0)
                hipLaunchKernelGGL(k_fuse_shared, dim3((ck.n + 255) / 256), dim3(256), 0, st, ck.n, ck.pool_row, candidate_kf, mv.d_kp_point,
                                   mv.d_obs_ptr, mv.d_obs_kf, (int)P, KF, d_shared);
            hipLaunchKernelGGL(k_fuse_rank, dim3(1), dim3(1024), 0, st, KF, d_shared, candidate_kf, opt->min_shared, opt->max_covisible, d_hdr);
            hipLaunchKernelGGL(k_fuse_mark_old, dim3(8, RS_FUSE_MAX_COVISIBLE + 1), dim3(256), 0, st, d_hdr, d_kf_tab, d_kf_tab + KF,
                               mv.d_kp_point, (int)P, d_old);
            hipLaunchKernelGGL(k_fuse_compact, dim3(1), dim3(1024), 0, st, (int)P, d_old, d_src, d_hdr + RS_FUSE_MAX_COVISIBLE + 2);
        }
        RS_HIP(ctx, hipGetLastError());
        if ((rc = rs_stage_download(ctx, d_hdr, sizeof(int32_t) * FUSE_HDR, hdr.data()))) return rc;      // read-back 1
        if ((rc = rs_stage_sync(ctx))) return rc;
    }
    const int n_old = hdr[RS_FUSE_MAX_COVISIBLE + 1], S = hdr[RS_FUSE_MAX_COVISIBLE + 2];
    if (n_old < 1 || n_old > opt->max_covisible + 1 || S < 0 || (size_t)S > P) return fuse_bad(ctx, RS_ERR_INTERNAL, "old set outside the map");
    std::vector<uint8_t> in_old((size_t)KF, 0);
    for (int j = 0; j < n_old; j++) {
        if (!mirror_kf_ok(m, hdr[(size_t)j])) return fuse_bad(ctx, RS_ERR_INTERNAL, "old frame outside the map");
        in_old[(size_t)hdr[(size_t)j]] = 1;
        rep->old_frames[j] = hdr[(size_t)j];
    }
    rep->n_old_frames = n_old;
    rep->n_sources = S;
    // the old points on the host: the mirror's tables are what the image's were made from
    std::vector<int32_t> old_frames(hdr.begin(), hdr.begin() + n_old);
    std::vector<uint8_t> is_old;
    mirror_loop_points(m, old_frames, &is_old);
    if (opt->check) {
        std::vector<int32_t> want;
        mirror_loop_old_frames(m, candidate_kf, opt->min_shared, opt->max_covisible, &want);
        bad_rank += want.size() != old_frames.size() ? 1 : 0;
        for (size_t j = 0; j < want.size() && j < old_frames.size(); j++) bad_rank += want[j] != old_frames[j] ? 1 : 0;
        int n_flag = 0;
        for (const uint8_t f : is_old) n_flag += f;
        bad_rank += n_flag != S ? 1 : 0;
    }
    // ---- stage 2: the inliers, on the mirror
    std::vector<int32_t> j_kp, j_pt, j_oc, sec((size_t)n_window + 2, 0), removed;
    j_kp.assign(h_inlier_kp, h_inlier_kp + n_inliers);
    j_pt.assign(h_inlier_point, h_inlier_point + n_inliers);
    j_oc.resize((size_t)n_inliers);
    mirror_replay_fuse(m, query_kf, j_kp.data(), j_pt.data(), n_inliers, is_old.data(), is_old.size(), j_oc.data(), &removed, rep->outcomes);
    sec[1] = n_inliers;
    // ---- stage 3: the window, on the device
    std::vector<int> todo;                  // window entries that run
    size_t sum_n = 0; int max_n = 0;
    for (int w = 0; w < n_window && S > 0; w++) {
        const MapKeyFrame& k = m->kfs[(size_t)h_window_kfs[w]];
        if (in_old[(size_t)h_window_kfs[w]] || k.n == 0) continue;
        todo.push_back(w);
        sum_n += (size_t)k.n;
        max_n = k.n > max_n ? k.n : max_n;
    }
    std::vector<int32_t> h_jcnt, h_jkp, h_jpt;
    std::vector<size_t> joff(todo.size() + 1, 0);
    int32_t *d_ptr[2] = {nullptr, nullptr}, *d_vkf[2] = {nullptr, nullptr}, *d_vdesc[2] = {nullptr, nullptr};
    int cur = 0;
    size_t capO = 0;
    if (!todo.empty()) {
        if ((rc = rs_map_fuse_sync(map, 1, &mv))) return rc;              // the image follows the inliers' edits
        int fcap = 1024;
        while (fcap < max_n) fcap *= 2;
        if (!fs->frame || fs->frame->cap < fcap) {
            if (fs->frame) { (void)rs_frame_destroy(fs->frame); fs->frame = nullptr; }
            if ((rc = rs_frame_create_device(ctx, fcap, &fs->frame))) return rc;
        }
        capO = mv.n_obs + sum_n + 1;         // (+ 1: never an empty buffer)
        const size_t Sz = (size_t)S, T = todo.size();
        // ptr x2 [S+1] | add [S] | point_kp [S] | point_dist [S] | prop_point, prop_dist [max_n] | counts [T] | jkp, jview, jpt [sum_n]
        // | view positions [3 S] | rows x2 x (kf, desc) [capO]
        const size_t words = 2 * (Sz + 1) + 3 * Sz + 2 * (size_t)max_n + T + 3 * sum_n + 3 * Sz + 4 * capO;
        if ((rc = fs->d_win.reserve(ctx, words, FUSE_FIRST))) return rc;
        int32_t* q = fs->d_win;
        d_ptr[0] = q; q += Sz + 1; d_ptr[1] = q; q += Sz + 1;
        int32_t* d_add = q; q += Sz;
        int32_t* d_pkp = q; q += Sz; int32_t* d_pdist = q; q += Sz;
        int32_t* d_pp = q; q += max_n; int32_t* d_ppd = q; q += max_n;
        int32_t* d_jcnt = q; q += T;
        int32_t* d_fn = nullptr;            // the frames' keypoint counts travel through the staging pool
        int32_t* d_jkp = q; q += sum_n; int32_t* d_jview = q; q += sum_n; int32_t* d_jpt = q; q += sum_n;
        float* d_vpos = (float*)q; q += 3 * Sz;
        for (int b = 0; b < 2; b++) { d_vkf[b] = q; q += capO; d_vdesc[b] = q; q += capO; }
        std::vector<int32_t> fn(T);
        for (size_t t = 0; t < T; t++) {
            fn[t] = m->kfs[(size_t)h_window_kfs[todo[t]]].n;
            joff[t + 1] = joff[t] + (size_t)fn[t];
        }
        if ((rc = rs_stage_begin(ctx))) return rc;
        if ((rc = rs_stage_upload(ctx, fn.data(), sizeof(int32_t) * T, (void**)&d_fn))) return rc;
        RS_HIP(ctx, hipMemsetAsync(d_jcnt, 0, sizeof(int32_t) * T, st));
        RS_HIP(ctx, hipMemsetAsync(d_zero, 0, FUSE_MAX_KP, st));
        RS_HIP(ctx, hipMemcpyAsync(d_alive_w, mv.d_alive, P, hipMemcpyDeviceToDevice, st));
        const int sb = (S + 255) / 256;
        m->dirty_kp_point = true;           // the image's tables are the working tables from here on
        {
            rs_prof_scope ps(ctx, "FL_fuse_view");
            hipLaunchKernelGGL(k_fuse_row_len, dim3(sb), dim3(256), 0, st, S, d_src, mv.d_obs_ptr, d_add);
            hipLaunchKernelGGL(k_fuse_scan, dim3(1), dim3(1024), 0, st, S, (const int32_t*)nullptr, d_add, d_ptr[0]);
            hipLaunchKernelGGL(k_fuse_gather, dim3(sb), dim3(256), 0, st, S, d_src, mv.d_obs_ptr, mv.d_obs_kf, mv.d_obs_desc, mv.d_pos, d_ptr[0],
                               d_vkf[0], d_vdesc[0], d_vpos);
        }
        for (size_t t = 0; t < T; t++) {
            const int kf = h_window_kfs[todo[t]];
            const MapKeyFrame& k = m->kfs[(size_t)kf];
            const int N = k.n;
            rs_frame* f = fs->frame;
            if ((rc = rs_frame_assign_enqueue(ctx, f, mv.d_kp_pool + 2 * (size_t)k.pool_row, d_fn + t, mv.d_pool + 32 * (size_t)k.pool_row, N))) return rc;
            hipLaunchKernelGGL(k_fuse_eligible, dim3(sb), dim3(256), 0, st, S, d_src, d_alive_w, d_ptr[cur], d_vkf[cur], kf, d_elig);
            rs_frame_view fv{};
            memcpy(fv.pose, k.pose, sizeof fv.pose);
            fv.fx = opt->intrinsics[0]; fv.fy = opt->intrinsics[1]; fv.cx = opt->intrinsics[2]; fv.cy = opt->intrinsics[3];
            fv.width = opt->width; fv.height = opt->height; fv.n_keypoints = N;
            fv.d_keypoints = f->d_kp; fv.d_descriptors = f->d_desc; fv.d_kp_matched = d_zero;
            fv.d_kd_node_kp = f->d_kd; fv.d_kd_left = f->d_kd + N; fv.d_kd_right = f->d_kd + 2 * (size_t)N; fv.kd_root = f->kd_root;
            fv.d_kd_packed = f->d_packed;
            if ((rc = rs_frame_grid(ctx, f, opt->width, opt->height, &fv.d_kd_grid))) return rc;      // (none: the host never sees these keypoints)
            rs_map_view sv{S, d_vpos, d_elig, d_ptr[cur], d_vkf[cur], d_vdesc[cur], mv.d_centres, mv.d_pool};
            if ((rc = rs_reproj_match(ctx, &fv, &sv, 1, opt->max_distance, d_pkp, d_pdist, d_pp, d_ppd, d_jkp + joff[t], d_jview + joff[t], d_jcnt + t)))
                return rc;
            FuseFrame ff{kf, k.pool_row, N, S, (int)P, d_jcnt + t, d_jkp + joff[t], d_jview + joff[t], d_jpt + joff[t], d_src, d_old,
                         mv.d_obs_ptr, mv.d_obs_kf, mv.d_obs_desc, d_ptr[cur], d_vkf[cur], d_vdesc[cur]};
            const int nb = (N + 255) / 256, nxt = cur ^ 1;
            RS_HIP(ctx, hipMemsetAsync(d_add, 0, sizeof(int32_t) * Sz, st));
            {
                rs_prof_scope ps(ctx, "FL_fuse_apply");
                hipLaunchKernelGGL(k_fuse_count, dim3(nb), dim3(256), 0, st, ff, (const int32_t*)mv.d_kp_point, d_add);
                hipLaunchKernelGGL(k_fuse_scan, dim3(1), dim3(1024), 0, st, S, (const int32_t*)d_ptr[cur], d_add, d_ptr[nxt]);
                hipLaunchKernelGGL(k_fuse_copy, dim3(sb), dim3(256), 0, st, S, d_ptr[cur], d_vkf[cur], d_vdesc[cur], d_ptr[nxt], d_vkf[nxt], d_vdesc[nxt]);
                hipLaunchKernelGGL(k_fuse_apply, dim3(nb), dim3(256), 0, st, ff, mv.d_kp_point, d_alive_w, d_ptr[nxt], d_vkf[nxt], d_vdesc[nxt]);
            }
            cur = nxt;
        }
        RS_HIP(ctx, hipGetLastError());
        h_jcnt.resize(T); h_jkp.resize(sum_n); h_jpt.resize(sum_n);
        if ((rc = rs_stage_download(ctx, d_jcnt, sizeof(int32_t) * T, h_jcnt.data()))) return rc;          // read-back 2: the journal
        if ((rc = rs_stage_download(ctx, d_jkp, sizeof(int32_t) * sum_n, h_jkp.data()))) return rc;
        if ((rc = rs_stage_download(ctx, d_jpt, sizeof(int32_t) * sum_n, h_jpt.data()))) return rc;
        if ((rc = rs_stage_sync(ctx))) return rc;
        for (size_t t = 0; t < T; t++)
            if (h_jcnt[t] < 0 || (size_t)h_jcnt[t] > joff[t + 1] - joff[t]) return fuse_bad(ctx, RS_ERR_INTERNAL, "journal count outside its frame");
    }
    // ---- stage 4: the mirror replays the journal
    {
        size_t t = 0;
        for (int w = 0; w < n_window; w++) {
            if (t < todo.size() && todo[t] == w) {
                const size_t n = (size_t)h_jcnt[t], at = j_kp.size();
                j_kp.insert(j_kp.end(), h_jkp.begin() + (long)joff[t], h_jkp.begin() + (long)(joff[t] + n));
                j_pt.insert(j_pt.end(), h_jpt.begin() + (long)joff[t], h_jpt.begin() + (long)(joff[t] + n));
                j_oc.resize(at + n);
                mirror_replay_fuse(m, h_window_kfs[w], j_kp.data() + at, j_pt.data() + at, (int)n, is_old.data(), is_old.size(), j_oc.data() + at,
                                   &removed, rep->outcomes);
                t++;
            }
            sec[(size_t)w + 2] = (int32_t)j_kp.size();
        }
    }
    rep->n_removed = (int)removed.size();
    for (size_t i = 0; i < removed.size() && (int)i < rep_rem_cap; i++) rep_rem[i] = removed[i];
    if (rep_src_cap > 0) {
        int c = 0;
        for (size_t p = 0; p < is_old.size() && c < rep_src_cap; p++)
            if (is_old[p]) opt->h_sources[c++] = (int32_t)p;
    }
    const size_t total = j_kp.size(), ncopy = total < (size_t)(capacity > 0 ? capacity : 0) ? total : (size_t)(capacity > 0 ? capacity : 0);
    if (h_section_ptr) memcpy(h_section_ptr, sec.data(), sizeof(int32_t) * sec.size());
    if (h_kp && ncopy) memcpy(h_kp, j_kp.data(), sizeof(int32_t) * ncopy);
    if (h_point && ncopy) memcpy(h_point, j_pt.data(), sizeof(int32_t) * ncopy);
    if (h_outcome && ncopy) memcpy(h_outcome, j_oc.data(), sizeof(int32_t) * ncopy);
    if (h_n_entries) *h_n_entries = (int)total;
    // ---- the self-check: the device's final working state against the replayed mirror
    if (opt->check) {
        int bad = bad_rank;
        if (!todo.empty()) {
            const size_t Sz = (size_t)S;
            std::vector<int32_t> ptr(Sz + 1), vkf(capO), vdesc(capO), tab(mv.pool_rows ? mv.pool_rows : 1), src(Sz);
            std::vector<uint8_t> alive(P);
            if ((rc = rs_stage_begin(ctx))) return rc;
            if ((rc = rs_stage_download(ctx, d_ptr[cur], sizeof(int32_t) * (Sz + 1), ptr.data()))) return rc;
            if ((rc = rs_stage_download(ctx, d_vkf[cur], sizeof(int32_t) * capO, vkf.data()))) return rc;
            if ((rc = rs_stage_download(ctx, d_vdesc[cur], sizeof(int32_t) * capO, vdesc.data()))) return rc;
            if ((rc = rs_stage_download(ctx, d_src, sizeof(int32_t) * Sz, src.data()))) return rc;
            if (mv.pool_rows && (rc = rs_stage_download(ctx, mv.d_kp_point, sizeof(int32_t) * mv.pool_rows, tab.data()))) return rc;
            if ((rc = rs_stage_download(ctx, d_alive_w, P, alive.data()))) return rc;
            if ((rc = rs_stage_sync(ctx))) return rc;
            size_t c = 0;
            for (size_t p = 0; p < P; p++) {
                bad += alive[p] != m->alive[p] ? 1 : 0;
                if (!is_old[p]) continue;
                if (c >= Sz || src[c] != (int32_t)p) { bad++; continue; }
                const auto& row = m->obs[p];
                const int32_t o0 = ptr[c], o1 = ptr[c + 1];
                if (o0 < 0 || o1 < o0 || (size_t)o1 > capO || (size_t)(o1 - o0) != row.size()) { bad += 1 + (int)row.size(); c++; continue; }
                for (size_t k = 0; k < row.size(); k++)
                    bad += (vkf[(size_t)o0 + k] != row[k].kf ? 1 : 0) + (vdesc[(size_t)o0 + k] != m->kfs[(size_t)row[k].kf].pool_row + row[k].kp ? 1 : 0);
                c++;
            }
            bad += c != Sz ? 1 : 0;
            for (const MapKeyFrame& k : m->kfs)
                for (int i = 0; i < k.n; i++) bad += tab[(size_t)k.pool_row + (size_t)i] != k.kp_point[(size_t)i] ? 1 : 0;
        }
        rep->device_state_mismatches = bad;
    }
    return RS_OK;
}
