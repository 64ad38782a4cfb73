// reproj_match.hip — K2/K3: reprojection-gated map-point <-> keypoint matching.
//
// Replaces MapMatcher::match / match_map / match_key_frame / match_for_fuse
// (reference src/MapMatcher.cpp:45-98,107-127,165-175) together with the
// per-point helpers it calls: Camera::project / is_in_image (src/Camera.cpp:25-37),
// MapPoint::avg_viewing_normal / observed_distance_range (src/MapPoint.cpp:24-45)
// and KDTree2D::radius_search (src/KDTree.cpp:45-82).
//
// K2 is three kernels with identical outputs.  Where the frame carries a usable cell grid (rs_kdtree_grid_build, below) a
// point's candidates come from the grid's cells around its projection (k2_reproj_match_grid, the default: eight lanes per
// map point, no LDS, ties between equally distant keypoints decided by the reference's visiting order computed from their
// node ids).  The other two walk the KD-tree: eight lanes per map point when the tree fits in LDS
// (k2_reproj_match_grouped), one lane per point otherwise or under k2_mode 1 (k2_reproj_match).  Those two differ
// in how a point's observations are spread over lanes — the accumulation of the viewing normal and the descriptor
// compares of phase B — and share every other step, each defined once below (k2_project and k2_view_gates with the grid
// kernel too):
//   k2_project      Camera::project + is_in_image (tri_core.h's f32 forms)
//   k2_view_gates   the viewing-angle and distance-range gates, given the accumulated normal and range
//   k2_stage_tree   the frame's KD-tree into LDS, one K2Node per node
//   K2_WALK         the radius search with an explicit stack in LDS, visiting nodes in exactly the reference's recursion
//                   order (node, near child, far child) so that "first candidate wins ties" is preserved
//   k2_candidate    what the walk does with an in-range, open keypoint: queue it for phase B, or compare it on the spot
//   K2Lds           a point's columns of the workgroup's LDS tables; k2_lds_bytes is their size on the host
// Every candidate is compared against all observations of the point with 8 xor + 8 v_bcnt, every comparison a strict
// '<'.  The winner per point goes into a packed 64-bit atomicMin on the keypoint's slot (dist << 32 | map order), which
// reproduces the reference's sequential strict-'<' proposal table: min distance, earliest point on ties.
// K3: one workgroup decodes the table and emits accepted_matches() in ascending keypoint order.
// Built with -ffp-contract=off so the f32 gates execute the oracle's operations.
#include "common.h"
#include "tri_core.h"
#include "reproj_gates.h"      // k2_view_gates: the viewing-angle and distance-range gates

#include <mutex>

#define K2_THREADS 128           // one lane per point
#define K2G 8                    // lanes per point of the grouped kernel
#define K2G_THREADS 512          // its workgroup: 64 map points (256 / 1024 threads: slower)
#define K2_STACK 40
#define K2_PRE 8         // observations of a map point whose centre / descriptor row are preloaded
#define K2_MAXC 16       // in-radius candidates queued per map point before their descriptors are compared (phase B)
#define K2_MAX_LDS_NODES 6144    // 16 B per node: the whole KD-tree of a frame (2000 keypoints = 32 KB) sits in LDS

struct K2Frame {
    float T[16];
    float fx, fy, cx, cy;
    int width, height, n_keypoints, kd_root;
    const float2* kp;
    const uint4* desc;
    const uint8_t* kp_matched;
    const int32_t* kd_node_kp;
    const int32_t* kd_left;
    const int32_t* kd_right;
    const float4* packed;      // optional: {x, y, left, right}[n] then int32 keypoint[n] (rs_kdtree_pack), or null
};

struct K2Map {
    int n_points;
    int point_base;          // map order of this view's point 0 (a shard of a larger map: rs_reproj_match_sharded); 0 otherwise
    const float* pos;
    const uint8_t* eligible;
    const int32_t* obs_ptr;
    const int32_t* obs_kf;
    const int32_t* obs_desc;
    const float* kf_centers;
    const uint4* pool;
};

__device__ __forceinline__ int hamming256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1)
{
    int d = __builtin_popcount(a0.x ^ b0.x);
    d += __builtin_popcount(a0.y ^ b0.y);
    d += __builtin_popcount(a0.z ^ b0.z);
    d += __builtin_popcount(a0.w ^ b0.w);
    d += __builtin_popcount(a1.x ^ b1.x);
    d += __builtin_popcount(a1.y ^ b1.y);
    d += __builtin_popcount(a1.z ^ b1.z);
    d += __builtin_popcount(a1.w ^ b1.w);
    return d;
}

// K3 with the thread's chunk of at most CH keypoints held in registers: the table is read ONCE (one global round trip
// on the path from kernel start to the last store instead of two), counted, scanned and written from the registers.
// CH is the smallest of 1, 2, 4, 8 that holds the chunk: the one workgroup issues every load through one CU's
// address path, where 16 waves x 8 clamped 64-bit loads cost more than the round trip they overlap.
template <int CH>
__device__ __forceinline__ void k3_accept_held(unsigned long long* __restrict__ prop, int lo, int hi, int max_distance,
                                               int32_t* __restrict__ prop_point, int32_t* __restrict__ prop_dist,
                                               int32_t* __restrict__ match_kp, int32_t* __restrict__ match_point,
                                               int32_t* __restrict__ match_count)
{
    unsigned long long v[CH];
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < CH; u++) v[u] = __builtin_nontemporal_load(&prop[max(min(lo + u, hi - 1), 0)]);   // clamped: no branches
#pragma unroll
    for (int u = 0; u < CH; u++) cnt += (lo + u < hi && v[u] != ~0ull) ? 1 : 0;
    int total;
    int off = rs_block_exclusive_scan(cnt, &total);
#pragma unroll
    for (int u = 0; u < CH; u++) {
        const int i = lo + u;
        if (i < hi) {
            int pt = -1, dist = max_distance;
            if (v[u] != ~0ull) {
                pt = (int)(unsigned)(v[u] & 0xFFFFFFFFull);
                dist = (int)(v[u] >> 32);
                match_kp[off] = i;                                       // accepted_matches :34-43
                match_point[off] = pt;
                off++;
                prop[i] = ~0ull;
            }
            prop_point[i] = pt;
            prop_dist[i] = dist;
        }
    }
    if (threadIdx.x == 0) *match_count = total;
}

// Ordered acceptance of the proposal table (accepted_matches, src/MapMatcher.cpp:34-43) by ONE workgroup
// of any size; resets the table to all-ones for the next call.
__device__ __forceinline__ void k3_accept_body(unsigned long long* __restrict__ prop, int n, int max_distance,
                                               int32_t* __restrict__ prop_point, int32_t* __restrict__ prop_dist,
                                               int32_t* __restrict__ match_kp, int32_t* __restrict__ match_point,
                                               int32_t* __restrict__ match_count)
{
    // every thread owns a contiguous chunk of keypoints: count, one workgroup scan, ordered write.
    const int T = blockDim.x, chunk = (n + T - 1) / T;
    const int lo = min((int)threadIdx.x * chunk, n), hi = min(lo + chunk, n);
    // up to 8 keypoints per thread (n <= 8 T; workgroup-uniform): held in registers
    if (chunk <= 1) return k3_accept_held<1>(prop, lo, hi, max_distance, prop_point, prop_dist, match_kp, match_point, match_count);
    if (chunk <= 2) return k3_accept_held<2>(prop, lo, hi, max_distance, prop_point, prop_dist, match_kp, match_point, match_count);
    if (chunk <= 4) return k3_accept_held<4>(prop, lo, hi, max_distance, prop_point, prop_dist, match_kp, match_point, match_count);
    if (chunk <= 8) return k3_accept_held<8>(prop, lo, hi, max_distance, prop_point, prop_dist, match_kp, match_point, match_count);
    // larger tables: two passes.  Loads go out in batches of 8 (clamped addresses, no branches) so that their latencies overlap.
    int cnt = 0;
    for (int i0 = lo; i0 < hi; i0 += 8) {
        unsigned long long v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = __builtin_nontemporal_load(&prop[min(i0 + u, hi - 1)]);
#pragma unroll
        for (int u = 0; u < 8; u++) cnt += (i0 + u < hi && v[u] != ~0ull) ? 1 : 0;
    }
    int total;
    int off = rs_block_exclusive_scan(cnt, &total);
    for (int i0 = lo; i0 < hi; i0 += 8) {
        unsigned long long v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = __builtin_nontemporal_load(&prop[min(i0 + u, hi - 1)]);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int i = i0 + u;
            if (i >= hi) break;
            int pt = -1, dist = max_distance;
            if (v[u] != ~0ull) {
                pt = (int)(unsigned)(v[u] & 0xFFFFFFFFull);
                dist = (int)(v[u] >> 32);
                match_kp[off] = i;                                       // accepted_matches :34-43
                match_point[off] = pt;
                off++;
                prop[i] = ~0ull;
            }
            prop_point[i] = pt;
            prop_dist[i] = dist;
        }
    }
    if (threadIdx.x == 0) *match_count = total;
}

// LDS node of the frame's KD-tree: everything a visit needs in ONE ds_read_b128.
//   x, y     keypoint of the node
//   lr       left | right << 16, 0xFFFF = no child (the tree has at most K2_MAX_LDS_NODES < 65535 nodes)
//   kp       keypoint index | (already matched && !replace) << 31   (:65, :81 become a sign test)
struct K2Node { float x, y; unsigned lr; int kp; };

// Dynamic LDS of a workgroup that holds `pts` map points: [K2_STACK][pts] traversal stacks, [K2_MAXC][pts] candidate
// queue, [K2_MAXC][pts] running minima of the queued candidates, then the tree.  A K2Lds is ONE point's column of the
// three tables: entry i of a table is table[i * pts].
#define K2_COL_INTS (K2_STACK + 2 * K2_MAXC)
extern __shared__ __attribute__((aligned(16))) int k2_lds[];

struct K2Lds {
    int* stack;
    int* queue;
    int* qmin;
    K2Node* tree;
    int pts;
};

__device__ __forceinline__ K2Lds k2_lds_view(int pts, int col)
{
    K2Lds L;
    L.pts = pts;
    L.stack = k2_lds + col;
    L.queue = L.stack + K2_STACK * pts;
    L.qmin = L.queue + K2_MAXC * pts;
    L.tree = (K2Node*)(k2_lds + K2_COL_INTS * pts);
    return L;
}

static size_t k2_lds_bytes(int pts, int nodes) { return sizeof(int) * K2_COL_INTS * pts + sizeof(K2Node) * (size_t)nodes; }

// The frame's KD-tree into LDS by a workgroup of THREADS (a constant: blockDim.x would cost registers).  Eight nodes per
// thread and pass in three phases — the index loads, the loads that depend on them, the LDS writes — so that all loads of
// a phase are in flight together.
template <int THREADS>
__device__ __forceinline__ void k2_stage_tree(const K2Frame& f, int replace, K2Node* tree)
{
    for (int base = threadIdx.x; base < f.n_keypoints; base += 8 * THREADS) {
        int kpi[8], l[8], r[8];
        float x[8], y[8];
        bool taken[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int i = base + q * THREADS;
            kpi[q] = 0; l[q] = -1; r[q] = -1; x[q] = 0.f; y[q] = 0.f;
            if (i < f.n_keypoints) {
                if (f.packed) {        // packed once per frame (rs_kdtree_pack): straight copies instead of dependent gathers
                    const float4 nd = f.packed[i];
                    kpi[q] = ((const int*)(f.packed + f.n_keypoints))[i];
                    x[q] = nd.x; y[q] = nd.y; l[q] = __float_as_int(nd.z); r[q] = __float_as_int(nd.w);
                } else {
                    kpi[q] = f.kd_node_kp[i]; l[q] = f.kd_left[i]; r[q] = f.kd_right[i];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const bool in = base + q * THREADS < f.n_keypoints;
            taken[q] = in && !replace && f.kp_matched[kpi[q]] != 0;
            if (in && !f.packed) { const float2 k = f.kp[kpi[q]]; x[q] = k.x; y[q] = k.y; }
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int i = base + q * THREADS;
            if (i < f.n_keypoints) {
                K2Node nd;
                nd.x = x[q]; nd.y = y[q];
                nd.lr = (unsigned)(l[q] & 0xFFFF) | ((unsigned)(r[q] & 0xFFFF) << 16);
                nd.kp = kpi[q] | (taken[q] ? (int)0x80000000 : 0);
                tree[i] = nd;
            }
        }
    }
}

// Camera::project (src/Camera.cpp:25-32) and is_in_image (:34-37, src/MapMatcher.cpp:58); false: not in the image.
// T is the kernel's own copy of f.T: each kernel reads the pose in its body, where it is used.  With f.T itself handed
// to these helpers the compiler reads all of K2Frame into SGPRs at kernel entry, and k2_reproj_match spills.
__device__ __forceinline__ bool k2_project(const K2Frame& f, const float* T, const float* X, float& u, float& v)
{
    const TriParams k = {f.fx, f.fy, f.cx, f.cy, 0.0f, 0.0f};
    const float2 uv = project_f32(k, T, X);
    u = uv.x; v = uv.y;
    return u >= 0.0f && u < (float)f.width && v >= 0.0f && v < (float)f.height;
}

// An in-range, open keypoint met by the walk (src/MapMatcher.cpp:84-91).  The first K2_MAXC are QUEUED in visiting
// order, their descriptors compared in phase B.  (Comparing inside the walk costs one global-memory round trip per
// iteration in which ANY lane of the wave has a candidate — nearly every one; queued, the round trips are one per four
// candidates of the busiest lane.)  Candidates beyond K2_MAXC are compared on the spot, against every descriptor of the
// point o0 .. o1, into a second running best: they come later in visiting order than every queued one, so the queue
// wins ties when the kernels merge the two.
__device__ __forceinline__ void k2_candidate(const K2Frame& f, const K2Map& m, int o0, int o1, int kp, const K2Lds& L,
                                             int& nc, int& over_d, int& over_kp)
{
    if (nc < K2_MAXC) { L.queue[nc++ * L.pts] = kp; return; }
    const uint4 a0 = f.desc[2 * (size_t)kp], a1 = f.desc[2 * (size_t)kp + 1];
    int d = 0x7fffffff;
    for (int o = o0; o < o1; o++) {
        const size_t row = (size_t)m.obs_desc[o];
        d = min(d, hamming256(a0, a1, m.pool[2 * row], m.pool[2 * row + 1]));
    }
    if (d < over_d) { over_d = d; over_kp = kp; }
}

// KDTree2D::radius_search around (u, v), r = 20 px (src/MapMatcher.cpp:75, src/KDTree.cpp:45-82), by one lane for one
// point: the near child is visited next without going through the stack, only far children are pushed, with the depth
// parity of their level.  IN_LDS (a literal): the nodes are L.tree's.  Both children of a node are read while the node is
// examined (their indices are in the node), so the LDS latency of the next visit overlaps this visit's arithmetic; only
// a node popped from the stack pays a read of its own.  Otherwise (trees too large for LDS) the same walk fetches each
// node from global memory when it is visited.
// (l2_match.hip's l2_reproj_match carries a hand copy of the global-memory branch: keep the two in step.)
// A macro over the kernel's f, m, replace, o0, o1, u, v, L, nc, over_d and over_kp, not a function: as an inlined
// function the compiler splits this loop into a descent loop inside a pop loop, in which a lane that has to pop waits
// for the wave's last descent to end (K2 on the benchmark scene: 22.4 us instead of 20.9).
#define K2_WALK(IN_LDS) do {                                                                                        \
    const float r2 = 20.0f * 20.0f;                                                                                 \
    int sp = 0;                                                                                                     \
    int cur = f.kd_root, odd = 0;                                                                                   \
    K2Node nd, ndl, ndr;                                                                                            \
    if (IN_LDS && cur >= 0) nd = L.tree[cur];                                                                       \
    while (cur >= 0) {                                                                                              \
        int l, r, kp;                                                                                               \
        float dx, dy;                                                                                               \
        if (IN_LDS) {                                                                                               \
            l = (int)(nd.lr & 0xFFFFu); r = (int)(nd.lr >> 16);                                                     \
            l = l == 0xFFFF ? -1 : l; r = r == 0xFFFF ? -1 : r;                                                     \
            ndl = L.tree[l >= 0 ? l : 0]; ndr = L.tree[r >= 0 ? r : 0];                                             \
            kp = nd.kp;                                                                                             \
            dx = nd.x - u; dy = nd.y - v;                                                                           \
        } else {                                                                                                    \
            kp = f.kd_node_kp[cur];                                                                                 \
            const float2 q = f.kp[kp];                                                                              \
            l = f.kd_left[cur]; r = f.kd_right[cur];                                                                \
            dx = q.x - u; dy = q.y - v;                                                                             \
        }                                                                                                           \
        const float d2 = dx * dx + dy * dy;                                                                         \
        if (d2 <= r2 && (IN_LDS ? kp >= 0 : (replace || !f.kp_matched[kp])))     /* in range and open (:65, :81) */   \
            k2_candidate(f, m, o0, o1, kp, L, nc, over_d, over_kp);                                                 \
        const float delta = odd ? dy : dx;                                                                          \
        const bool left_near = delta > 0;                                                                           \
        const int near_child = left_near ? l : r;                                                                   \
        const int far_child = left_near ? r : l;                                                                    \
        odd ^= 1;                                                                /* depth parity of the children */ \
        if (delta * delta <= r2 && far_child >= 0 && sp < K2_STACK) L.stack[sp++ * L.pts] = far_child | (odd << 30); \
        if (near_child >= 0) { cur = near_child; if (IN_LDS) nd = left_near ? ndl : ndr; }                          \
        else if (sp > 0) {                                                                                          \
            const int e = L.stack[--sp * L.pts];                                                                    \
            cur = e & 0x3FFFFFFF; odd = (e >> 30) & 1;                                                              \
            if (IN_LDS) nd = L.tree[cur];                                                                           \
        }                                                                                                           \
        else cur = -1;                                                                                              \
    }                                                                                                               \
} while (0)

#ifndef RS_STAMPS
#define RS_STAMPS 0
#endif
#if RS_STAMPS
// diagnostic build (RS_STAMPS=1 python build.py): phase ends of the first wave of the middle workgroup, 10 ns ticks
__device__ unsigned long long k2_stamps[8];
#define K2_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == gridDim.x / 2) k2_stamps[i] = wall_clock64(); } while (0)
#define K2_STAMP0() K2_STAMP(0)
extern "C" int rs_k2_stamps(unsigned long long* h_out, int reset)
{
    if (hipMemcpyFromSymbol(h_out, HIP_SYMBOL(k2_stamps), sizeof(unsigned long long) * 8) != hipSuccess) return RS_ERR_HIP;
    if (reset) {
        unsigned long long z[8] = {~0ull, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(k2_stamps), z, sizeof z) != hipSuccess) return RS_ERR_HIP;
    }
    return RS_OK;
}
#else
#define K2_STAMP(i) do { } while (0)
#define K2_STAMP0() do { } while (0)
#endif

// One lane per map point: the lane accumulates the point's observations in batches of K2_PRE, walks the tree (in LDS or,
// when it does not fit, in global memory) and compares the queued candidates against K2_PRE descriptor rows per pass.
__global__ __launch_bounds__(K2_THREADS) void k2_reproj_match(K2Frame f, K2Map m, int replace, int max_distance, int tree_in_lds,
                                                             int32_t* __restrict__ point_kp,
                                                             int32_t* __restrict__ point_dist,
                                                             unsigned long long* __restrict__ prop)
{
    const K2Lds L = k2_lds_view(K2_THREADS, threadIdx.x);
    // this lane's map point: every load that needs only p goes out before the tree is staged
    const int p = blockIdx.x * K2_THREADS + threadIdx.x;
    const bool have = p < m.n_points;
    const int pc = have ? p : 0;
    const bool elig = have && m.eligible[pc] != 0;
    const int o0 = m.obs_ptr[pc], o1 = m.obs_ptr[pc + 1];
    const int nobs = elig ? o1 - o0 : 0;
    const float X[3] = {m.pos[3 * (size_t)pc], m.pos[3 * (size_t)pc + 1], m.pos[3 * (size_t)pc + 2]};
    // the first K2_PRE observations of the point: keyframe centre and descriptor row, loaded as two
    // batches (not as nobs dependent pairs inside the loops below); further observations come in batches of K2_PRE too
    int rowv[K2_PRE];
    float Cv[K2_PRE][3];
    {
        int kfv[K2_PRE];
#pragma unroll
        for (int j = 0; j < K2_PRE; j++) {
            kfv[j] = 0; rowv[j] = 0;
            if (j < nobs) { kfv[j] = m.obs_kf[o0 + j]; rowv[j] = m.obs_desc[o0 + j]; }
        }
#pragma unroll
        for (int j = 0; j < K2_PRE; j++) {
            Cv[j][0] = Cv[j][1] = Cv[j][2] = 0.f;
            if (j < nobs) {
                const float* C = m.kf_centers + 3 * (size_t)kfv[j];
                Cv[j][0] = C[0]; Cv[j][1] = C[1]; Cv[j][2] = C[2];
            }
        }
    }
    if (tree_in_lds) {
        k2_stage_tree<K2_THREADS>(f, replace, L.tree);
        __syncthreads();
    }
    int out_kp = -1, out_d = max_distance;
    if (have) do {
        if (!elig) break;
        float T[16];                                                     // see k2_project
#pragma unroll
        for (int i = 0; i < 16; i++) T[i] = f.T[i];
        float u, v;
        if (!k2_project(f, T, X, u, v)) break;
        float center[3];
        camera_center_f32(T, center);
        float normal[3] = {0.0f, 0.0f, 0.0f};
        float nearest = 3.402823466e+38f, furthest = 0.0f;
        auto add_obs = [&](const float Cx, const float Cy, const float Cz) {   // src/MapPoint.cpp:24-45
            float d[3] = {X[0] - Cx, X[1] - Cy, X[2] - Cz};
            const float dist = sqrtf(dot3f(d, d));
            nearest = dist < nearest ? dist : nearest;
            furthest = furthest < dist ? dist : furthest;
            normalize3f(d);
            normalize3f(d);
            normal[0] += d[0]; normal[1] += d[1]; normal[2] += d[2];
        };
#pragma unroll
        for (int j = 0; j < K2_PRE; j++)
            if (j < nobs) add_obs(Cv[j][0], Cv[j][1], Cv[j][2]);
        for (int ob = K2_PRE; ob < nobs; ob += K2_PRE) {                  // long-lived points: K2_PRE centres per round trip,
            int kfv[K2_PRE];                                              // accumulated in observation order
            float Cx[K2_PRE][3];
#pragma unroll
            for (int j = 0; j < K2_PRE; j++) kfv[j] = (ob + j < nobs) ? m.obs_kf[o0 + ob + j] : 0;
#pragma unroll
            for (int j = 0; j < K2_PRE; j++) {
                const float* C = m.kf_centers + 3 * (size_t)kfv[j];
                Cx[j][0] = Cx[j][1] = Cx[j][2] = 0.f;
                if (ob + j < nobs) { Cx[j][0] = C[0]; Cx[j][1] = C[1]; Cx[j][2] = C[2]; }
            }
#pragma unroll
            for (int j = 0; j < K2_PRE; j++)
                if (ob + j < nobs) add_obs(Cx[j][0], Cx[j][1], Cx[j][2]);
        }
        if (!k2_view_gates(normal, nearest, furthest, X, center)) break;

        int best_kp = 0, best_d = max_distance;
        // One candidate keypoint against every descriptor of the point (:84-91).  The reference keeps a running best with
        // a strict '<' over (candidate, observation) pairs; the winner's keypoint is the FIRST candidate (in visiting
        // order) whose minimum over the observations is the overall minimum, so per candidate only that minimum matters
        // and the observations may be taken in any order.
        auto rows_min = [&](const uint4 a0, const uint4 a1, const uint4* b0, const uint4* b1, int nb) {
            int d = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < K2_PRE; j++)
                if (j < nb) d = min(d, hamming256(a0, a1, b0[j], b1[j]));
            return d;
        };
        // Phase A: the walk queues the candidates
        int nc = 0, over_kp = 0, over_d = max_distance;
        if (tree_in_lds) K2_WALK(true);
        else K2_WALK(false);
        // Phase B: K2_PRE descriptor rows of the point per pass (the first pass's row numbers are already here), the
        // queued candidates four at a time (their row loads go out together); each candidate's minimum over the
        // observations accumulates in LDS across passes
        if (nc > 0) {
            for (int ob = 0; ob < nobs; ob += K2_PRE) {
                const int nb = min(K2_PRE, nobs - ob);
                int rows[K2_PRE];
#pragma unroll
                for (int j = 0; j < K2_PRE; j++) rows[j] = ob == 0 ? rowv[j] : (j < nb ? m.obs_desc[o0 + ob + j] : 0);
                uint4 b0[K2_PRE], b1[K2_PRE];
#pragma unroll
                for (int j = 0; j < K2_PRE; j++) {
                    b0[j] = make_uint4(0, 0, 0, 0); b1[j] = b0[j];
                    if (j < nb) { b0[j] = m.pool[2 * (size_t)rows[j]]; b1[j] = m.pool[2 * (size_t)rows[j] + 1]; }
                }
                for (int c = 0; c < nc; c += 4) {
                    int kq[4];
                    uint4 a0[4], a1[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        kq[q] = (c + q < nc) ? L.queue[(c + q) * L.pts] : -1;
                        a0[q] = make_uint4(0, 0, 0, 0); a1[q] = a0[q];
                        if (kq[q] >= 0) { a0[q] = f.desc[2 * (size_t)kq[q]]; a1[q] = f.desc[2 * (size_t)kq[q] + 1]; }
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (kq[q] >= 0) {
                            const int d = rows_min(a0[q], a1[q], b0, b1, nb);
                            L.qmin[(c + q) * L.pts] = ob == 0 ? d : min(d, L.qmin[(c + q) * L.pts]);
                        }
                }
            }
            if (nobs > 0)
                for (int c = 0; c < nc; c++) {
                    const int d = L.qmin[c * L.pts];
                    if (d < best_d) { best_d = d; best_kp = L.queue[c * L.pts]; }       // :88-91, visiting order
                }
        }
        if (over_d < best_d) { best_d = over_d; best_kp = over_kp; }
        if (best_d < max_distance) {
            out_kp = best_kp;
            out_d = best_d;
            // :95-97 sequential strict-'<' over map order == atomicMin of (dist, map order)
            atomicMin(&prop[best_kp], ((unsigned long long)(unsigned)best_d << 32) | (unsigned)(m.point_base + p));
        }
    } while (0);
    if (p < m.n_points) {
        point_kp[p] = out_kp;
        point_dist[p] = out_d;
    }
}

// K2g: EIGHT lanes per map point (trees that fit in LDS).  With one lane per point a 64-wide wave walks 64 trees in lock
// step and then compares every candidate against the point's descriptors one after the other; here a wave holds 8
// points, lane 0 of a group walks the tree and queues the candidates, and the group's lanes each own ONE observation of
// the point: its keyframe centre (viewing-normal gate) and its descriptor row (loaded before the tree is staged), so a
// candidate costs one 256-bit compare per lane and a 3-step DPP minimum.  The normal's f32 sum is taken in observation
// order, as k2_reproj_match takes it — the outputs are bit-identical (tests/test_gpu_parity.py runs both).
__device__ __forceinline__ int group8_min(int v)
{
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true));     // quad_perm [1,0,3,2]
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true));     // quad_perm [2,3,0,1]
    v = min(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, true));    // row_half_mirror: the other quad of the eight
    return v;
}

__global__ __launch_bounds__(K2G_THREADS) void k2_reproj_match_grouped(K2Frame f, K2Map m, int replace, int max_distance,
                                                                     int32_t* __restrict__ point_kp,
                                                                     int32_t* __restrict__ point_dist,
                                                                     unsigned long long* __restrict__ prop)
{
    constexpr int K2G_PTS = K2G_THREADS / K2G;
    K2_STAMP0();
    const int g = threadIdx.x / K2G, sub = threadIdx.x % K2G;
    const K2Lds L = k2_lds_view(K2G_PTS, g);
    const int p = blockIdx.x * K2G_PTS + g;
    const bool have = p < m.n_points;
    const int pc = have ? p : 0;
    const bool elig = have && m.eligible[pc] != 0;
    const int o0 = m.obs_ptr[pc], o1 = m.obs_ptr[pc + 1];
    const int nobs = elig ? o1 - o0 : 0;
    const float X[3] = {m.pos[3 * (size_t)pc], m.pos[3 * (size_t)pc + 1], m.pos[3 * (size_t)pc + 2]};
    // this lane's observations of the first sixteen (sub and sub + 8): keyframe centre and descriptor row, in flight
    // while the tree is staged; later ones are fetched inside the passes below
    float C0[3] = {0.f, 0.f, 0.f}, C1[3] = {0.f, 0.f, 0.f};
    uint4 b0 = make_uint4(0, 0, 0, 0), b1 = b0, b2 = b0, b3 = b0;
    {
        const bool h0 = sub < nobs, h1 = K2G + sub < nobs;
        const int kf0 = h0 ? m.obs_kf[o0 + sub] : 0, kf1 = h1 ? m.obs_kf[o0 + K2G + sub] : 0;
        const size_t row0 = h0 ? (size_t)m.obs_desc[o0 + sub] : 0, row1 = h1 ? (size_t)m.obs_desc[o0 + K2G + sub] : 0;
        if (h0) {
            const float* C = m.kf_centers + 3 * (size_t)kf0;
            C0[0] = C[0]; C0[1] = C[1]; C0[2] = C[2];
            b0 = m.pool[2 * row0]; b1 = m.pool[2 * row0 + 1];
        }
        if (h1) {
            const float* C = m.kf_centers + 3 * (size_t)kf1;
            C1[0] = C[0]; C1[1] = C[1]; C1[2] = C[2];
            b2 = m.pool[2 * row1]; b3 = m.pool[2 * row1 + 1];
        }
    }
    k2_stage_tree<K2G_THREADS>(f, replace, L.tree);
    K2_STAMP(1);
    __syncthreads();
    K2_STAMP(2);
    // everything below is uniform within a group of eight lanes except where `sub` appears
    int out_kp = -1, out_d = max_distance;
    if (have) do {
        if (!elig) break;
        float T[16];                                                     // see k2_project
#pragma unroll
        for (int i = 0; i < 16; i++) T[i] = f.T[i];
        float u, v;
        if (!k2_project(f, T, X, u, v)) break;
        float center[3];
        camera_center_f32(T, center);
        float normal[3] = {0.0f, 0.0f, 0.0f};
        float nearest = 3.402823466e+38f, furthest = 0.0f;
        for (int ob = 0; ob < nobs; ob += K2G) {                          // src/MapPoint.cpp:24-45, eight observations per pass
            float Cx[3] = {ob == 0 ? C0[0] : C1[0], ob == 0 ? C0[1] : C1[1], ob == 0 ? C0[2] : C1[2]};
            if (ob > K2G && ob + sub < nobs) {
                const float* C = m.kf_centers + 3 * (size_t)m.obs_kf[o0 + ob + sub];
                Cx[0] = C[0]; Cx[1] = C[1]; Cx[2] = C[2];
            }
            float d[3] = {X[0] - Cx[0], X[1] - Cx[1], X[2] - Cx[2]};
            const float dist = sqrtf(dot3f(d, d));
            normalize3f(d);
            normalize3f(d);
#pragma unroll
            for (int j = 0; j < K2G; j++) {                               // summed in observation order by every lane
                const float dj0 = __shfl(d[0], j, K2G), dj1 = __shfl(d[1], j, K2G), dj2 = __shfl(d[2], j, K2G);
                const float distj = __shfl(dist, j, K2G);
                if (ob + j < nobs) {
                    nearest = distj < nearest ? distj : nearest;
                    furthest = furthest < distj ? distj : furthest;
                    normal[0] += dj0; normal[1] += dj1; normal[2] += dj2;
                }
            }
        }
        if (!k2_view_gates(normal, nearest, furthest, X, center)) break;

        K2_STAMP(3);
        int nc = 0, over_kp = 0, over_d = max_distance;
        if (sub == 0) K2_WALK(true);                                     // lane 0 of the group
        K2_STAMP(4);
        nc = __shfl(nc, 0, K2G);
        over_d = __shfl(over_d, 0, K2G);
        over_kp = __shfl(over_kp, 0, K2G);
        // the queued candidates (visiting order), four per round trip; each lane compares its observation's row
        int best_kp = 0, best_d = max_distance;
        if (nc > 0 && nobs > 0) {
            for (int ob = 0; ob < nobs; ob += K2G) {
                uint4 r0 = ob == 0 ? b0 : b2, r1 = ob == 0 ? b1 : b3;
                const bool mine = ob + sub < nobs;
                if (ob > K2G && mine) {
                    const size_t row = (size_t)m.obs_desc[o0 + ob + sub];
                    r0 = m.pool[2 * row]; r1 = m.pool[2 * row + 1];
                }
                for (int c = 0; c < nc; c += 4) {
                    int kq[4];
                    uint4 a0[4], a1[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        kq[q] = L.queue[min(c + q, nc - 1) * L.pts];
                        a0[q] = f.desc[2 * (size_t)kq[q]]; a1[q] = f.desc[2 * (size_t)kq[q] + 1];
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int d = group8_min(mine ? hamming256(a0[q], a1[q], r0, r1) : 0x7fffffff);
                        if (c + q < nc) {
                            if (ob == 0) { if (d < best_d) { best_d = d; best_kp = kq[q]; } }   // :88-91, visiting order
                            if (nobs > K2G) L.qmin[(c + q) * L.pts] = ob == 0 ? d : min(d, L.qmin[(c + q) * L.pts]);
                        }
                    }
                }
            }
            if (nobs > K2G) {                                             // more than eight observations: minima over all passes
                best_kp = 0; best_d = max_distance;
                for (int c = 0; c < nc; c++) {
                    const int d = L.qmin[c * L.pts];
                    if (d < best_d) { best_d = d; best_kp = L.queue[c * L.pts]; }
                }
            }
        }
        K2_STAMP(5);
        if (over_d < best_d) { best_d = over_d; best_kp = over_kp; }
        if (best_d < max_distance) {
            out_kp = best_kp;
            out_d = best_d;
            // :95-97 sequential strict-'<' over map order == atomicMin of (dist, map order)
            if (sub == 0) atomicMin(&prop[best_kp], ((unsigned long long)(unsigned)best_d << 32) | (unsigned)(m.point_base + p));
        }
    } while (0);
    if (have && sub == 0) {
        point_kp[p] = out_kp;
        point_dist[p] = out_d;
    }
    K2_STAMP(6);
}

// ------------------------------------------------------------------------------------------------ the cell grid
// A frame's keypoints in a uniform grid over the image, built once per frame (rs_kdtree_grid_build) from the packed tree:
//   K2Grid header | cell_start[nx * ny + 1] (padded to 16 bytes) | entries[n] {x, y, keypoint, node id} | build scratch [2 n]
// entries are sorted by cell (row-major), inside a cell by node id: a pure function of the input.  A coordinate's cell
// is floor(c * K2_CELL_INV) clamped into the grid — monotone in c, so a keypoint within 20 px of (u, v) lies in the cell
// range of [u - 20.5, u + 20.5] x [v - 20.5, v + 20.5] whatever the grid's extent (keypoints outside it sit in border
// cells), and that range spans at most 3 cells per axis.  The exact dx * dx + dy * dy <= 400 test of the walk decides.
#define K2_CELL 40
#define K2_CELL_INV 0.025f
#define K2_GRID_MAX_N 65536        // the build ranks entries inside their cell by counting pairs
#define K2_GRID_MAX_DIM 256        // cells per axis; a larger image gets wider border cells
#define K2_GRID_MAX_IMAGE 65536    // pixels per axis up to which the 0.5 px margin above covers the f32 rounding of u -+ 20
#define K2C_THREADS 256            // the grid kernel's workgroup: 32 map points (no LDS, no barrier: any size would do)

struct K2Grid { int nx, ny, cell, n, usable, pad[3]; };

static inline int k2_grid_dim(int pixels)
{
    if (pixels <= 0) return 1;
    const int d = pixels / K2_CELL + 1;
    return d > K2_GRID_MAX_DIM ? K2_GRID_MAX_DIM : d;
}
__host__ __device__ static inline size_t k2_grid_start_ints(int nx, int ny) { return ((size_t)nx * ny + 1 + 3) & ~(size_t)3; }

__device__ __forceinline__ int k2_cell_of(float c, int cells)
{
    return (int)fminf(fmaxf(floorf(c * K2_CELL_INV), 0.0f), (float)(cells - 1));
}

// Which of two in-radius nodes the reference's recursion (src/KDTree.cpp:52-82) reaches first; true: node b before the
// running best a.  Node ids are positions mid = (start + end) / 2 of the implicit tree, so the lowest common ancestor L
// is integer arithmetic on a, b and n.  L == a or L == b: the ancestor comes first.  Otherwise the node in L's near
// subtree, near being the left child when L.coord[depth % 2] - query > 0 in f32, as K2_WALK computes delta.
__device__ __forceinline__ bool k2_visited_before(int b, int a, int n, const float4* __restrict__ packed, float u, float v)
{
    int s = 0, e = n, odd = 0, L;
    for (;;) {
        L = (s + e) >> 1;
        if (a == L) return false;
        if (b == L) return true;
        if ((a < L) != (b < L)) break;
        if (a < L) e = L; else s = L + 1;
        odd ^= 1;
    }
    const float4 nd = packed[L];
    const float delta = odd ? nd.y - v : nd.x - u;
    return (b < L) == (delta > 0);
}

// K2c: eight lanes per map point as in k2_reproj_match_grouped, the candidates from the frame's cell grid instead of a
// walk: the cell ranges of the at most 3 rows (one contiguous range per row), their entries eight per step and one per
// lane, the in-radius ones up to four at a time through the 256-bit compare.  The running best resolves an equal
// distance on the spot by k2_visited_before: the recursion order is total, so the result is the walk's.  No LDS.
__global__ __launch_bounds__(K2C_THREADS) void k2_reproj_match_grid(K2Frame f, K2Map m, const int* __restrict__ grid, int replace,
                                                                   int max_distance, int32_t* __restrict__ point_kp,
                                                                   int32_t* __restrict__ point_dist,
                                                                   unsigned long long* __restrict__ prop)
{
    constexpr int PTS = K2C_THREADS / K2G;
    K2_STAMP0();
    const int g = threadIdx.x / K2G, sub = threadIdx.x % K2G;
    const int p = blockIdx.x * PTS + g;
    const bool have = p < m.n_points;
    const int pc = have ? p : 0;
    const bool elig = have && m.eligible[pc] != 0;
    const int o0 = m.obs_ptr[pc], o1 = m.obs_ptr[pc + 1];
    const int nobs = elig ? o1 - o0 : 0;
    const float X[3] = {m.pos[3 * (size_t)pc], m.pos[3 * (size_t)pc + 1], m.pos[3 * (size_t)pc + 2]};
    // this lane's observations of the first sixteen (sub and sub + 8): keyframe centre and descriptor row
    float C0[3] = {0.f, 0.f, 0.f}, C1[3] = {0.f, 0.f, 0.f};
    uint4 b0 = make_uint4(0, 0, 0, 0), b1 = b0, b2 = b0, b3 = b0;
    const bool h0 = sub < nobs, h1 = K2G + sub < nobs;
    {
        const int kf0 = h0 ? m.obs_kf[o0 + sub] : 0, kf1 = h1 ? m.obs_kf[o0 + K2G + sub] : 0;
        const size_t row0 = h0 ? (size_t)m.obs_desc[o0 + sub] : 0, row1 = h1 ? (size_t)m.obs_desc[o0 + K2G + sub] : 0;
        if (h0) {
            const float* C = m.kf_centers + 3 * (size_t)kf0;
            C0[0] = C[0]; C0[1] = C[1]; C0[2] = C[2];
            b0 = m.pool[2 * row0]; b1 = m.pool[2 * row0 + 1];
        }
        if (h1) {
            const float* C = m.kf_centers + 3 * (size_t)kf1;
            C1[0] = C[0]; C1[1] = C[1]; C1[2] = C[2];
            b2 = m.pool[2 * row1]; b3 = m.pool[2 * row1 + 1];
        }
    }
    K2_STAMP(1);
    // everything below is uniform within a group of eight lanes except where `sub` appears
    int out_kp = -1, out_d = max_distance;
    if (have) do {
        if (!elig) break;
        float T[16];                                                     // see k2_project
#pragma unroll
        for (int i = 0; i < 16; i++) T[i] = f.T[i];
        float u, v;
        if (!k2_project(f, T, X, u, v)) break;
        // the disc's cells: lane r < 3 reads the range of row cy0 + r.  These loads and the first eight entries need only
        // (u, v): they are under way while the viewing gates are computed
        const int nx = grid[0], ny = grid[1];
        const int* __restrict__ cell_start = grid + sizeof(K2Grid) / sizeof(int);
        const uint4* __restrict__ entries = (const uint4*)(cell_start + k2_grid_start_ints(nx, ny));
        const int cx0 = k2_cell_of(u - 20.5f, nx), cx1 = k2_cell_of(u + 20.5f, nx);
        const int cy0 = k2_cell_of(v - 20.5f, ny), cy1 = k2_cell_of(v + 20.5f, ny);
        int rs = 0, re = 0;
        if (sub < 3 && cy0 + sub <= cy1) {
            const int row = (cy0 + sub) * nx;
            rs = cell_start[row + cx0]; re = cell_start[row + cx1 + 1];
        }
        const int s0 = __shfl(rs, 0, K2G), s1 = __shfl(rs, 1, K2G), s2 = __shfl(rs, 2, K2G);
        const int l0 = __shfl(re, 0, K2G) - s0, l01 = l0 + __shfl(re, 1, K2G) - s1, total = l01 + __shfl(re, 2, K2G) - s2;
        auto entry_at = [&](int idx) {
            uint4 e = make_uint4(0, 0, 0, 0);
            if (idx < total) e = entries[idx < l0 ? s0 + idx : (idx < l01 ? s1 + (idx - l0) : s2 + (idx - l01))];
            return e;
        };
        uint4 ent = entry_at(sub);
        K2_STAMP(2);
        float center[3];
        camera_center_f32(T, center);
        float normal[3] = {0.0f, 0.0f, 0.0f};
        float nearest = 3.402823466e+38f, furthest = 0.0f;
        for (int ob = 0; ob < nobs; ob += K2G) {                          // src/MapPoint.cpp:24-45, eight observations per pass
            float Cx[3] = {ob == 0 ? C0[0] : C1[0], ob == 0 ? C0[1] : C1[1], ob == 0 ? C0[2] : C1[2]};
            if (ob > K2G && ob + sub < nobs) {
                const float* C = m.kf_centers + 3 * (size_t)m.obs_kf[o0 + ob + sub];
                Cx[0] = C[0]; Cx[1] = C[1]; Cx[2] = C[2];
            }
            float d[3] = {X[0] - Cx[0], X[1] - Cx[1], X[2] - Cx[2]};
            const float dist = sqrtf(dot3f(d, d));
            normalize3f(d);
            normalize3f(d);
#pragma unroll
            for (int j = 0; j < K2G; j++) {                               // summed in observation order by every lane
                const float dj0 = __shfl(d[0], j, K2G), dj1 = __shfl(d[1], j, K2G), dj2 = __shfl(d[2], j, K2G);
                const float distj = __shfl(dist, j, K2G);
                if (ob + j < nobs) {
                    nearest = distj < nearest ? distj : nearest;
                    furthest = furthest < distj ? distj : furthest;
                    normal[0] += dj0; normal[1] += dj1; normal[2] += dj2;
                }
            }
        }
        if (!k2_view_gates(normal, nearest, furthest, X, center)) break;
        K2_STAMP(3);

        const float r2 = 20.0f * 20.0f;
        const int first_lane = (int)(threadIdx.x & 63u) & ~(K2G - 1);
        int best_kp = 0, best_node = 0, best_d = max_distance;
        for (int base = 0; base < total; base += K2G) {
            if (base > 0) ent = entry_at(base + sub);
            bool in = false;
            if (base + sub < total) {
                const float dx = __uint_as_float(ent.x) - u, dy = __uint_as_float(ent.y) - v;
                const float d2 = dx * dx + dy * dy;
                in = d2 <= r2;                                            // in range (:65)
            }
            unsigned mask = (unsigned)(__ballot(in) >> first_lane) & 0xFFu;
            if (base == 0) K2_STAMP(4);                                   // the first eight entries are here
            while (mask) {                                                // the group's in-radius entries, four per round trip
                int kq[4], nq[4];
                bool val[4], open[4];
                uint4 a0[4], a1[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    val[q] = mask != 0;
                    const int src = val[q] ? __ffs(mask) - 1 : 0;
                    mask &= mask - 1;
                    kq[q] = __shfl((int)ent.z, src, K2G);
                    nq[q] = __shfl((int)ent.w, src, K2G);
                    a0[q] = make_uint4(0, 0, 0, 0); a1[q] = a0[q];
                    open[q] = false;
                    if (val[q]) {
                        a0[q] = f.desc[2 * (size_t)kq[q]]; a1[q] = f.desc[2 * (size_t)kq[q] + 1];
                        open[q] = replace || !f.kp_matched[kq[q]];       // read live (:65, :81): it changes between the calls of a frame
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (!val[q]) continue;
                    int d = h0 ? hamming256(a0[q], a1[q], b0, b1) : 0x7fffffff;
                    if (h1) d = min(d, hamming256(a0[q], a1[q], b2, b3));
                    for (int ob = 2 * K2G; ob < nobs; ob += K2G)          // long-lived points: this lane's further rows
                        if (ob + sub < nobs) {
                            const size_t row = (size_t)m.obs_desc[o0 + ob + sub];
                            d = min(d, hamming256(a0[q], a1[q], m.pool[2 * row], m.pool[2 * row + 1]));
                        }
                    d = group8_min(d);
                    // :88-91: the first candidate in visiting order among those at the minimal distance
                    if (open[q] && (d < best_d || (d == best_d && d < max_distance && k2_visited_before(nq[q], best_node, f.n_keypoints, f.packed, u, v)))) {
                        best_d = d; best_kp = kq[q]; best_node = nq[q];
                    }
                }
            }
        }
        K2_STAMP(5);
        if (best_d < max_distance) {
            out_kp = best_kp;
            out_d = best_d;
            // :95-97 sequential strict-'<' over map order == atomicMin of (dist, map order)
            if (sub == 0) atomicMin(&prop[best_kp], ((unsigned long long)(unsigned)best_d << 32) | (unsigned)(m.point_base + p));
        }
    } while (0);
    if (have && sub == 0) {
        point_kp[p] = out_kp;
        point_dist[p] = out_d;
    }
    K2_STAMP(6);
}

// K3: one workgroup decodes the proposal table, compacts the accepted matches in order and resets the table
// (tried as a tail of K2's last workgroup: no cheaper than this launch)
__global__ __launch_bounds__(1024) void k3_accept(unsigned long long* __restrict__ prop, int n,
                                                  int max_distance, int32_t* __restrict__ prop_point,
                                                  int32_t* __restrict__ prop_dist, int32_t* __restrict__ match_kp,
                                                  int32_t* __restrict__ match_point, int32_t* __restrict__ match_count)
{
    k3_accept_body(prop, n, max_distance, prop_point, prop_dist, match_kp, match_point, match_count);
}

// the map sharded over ranks (point_base = map order of this shard's first point).  Every rank runs
// K2 on its points; the per-keypoint proposal table — packed (distance << 32 | GLOBAL map order), built with atomicMin —
// is then MIN-all-reduced over the communicator (one ncclAllReduce(min, u64) of 8 N bytes; the in-process group: an
// on-device minimum), so that every rank's K3 accepts the same winners: exactly the unsharded result, ties included
// (src/MapMatcher.cpp:95-97: first in map order wins).  d_prop_point / d_match_point hold GLOBAL map indices;
// d_point_kp / d_point_dist are this shard's.
static int reproj_match_impl(rs_context* ctx, const rs_frame_view* fr, const rs_map_view* mp, int point_base, bool reduce, int replace,
                             int max_distance, int32_t* d_point_kp, int32_t* d_point_dist,
                             int32_t* d_prop_point, int32_t* d_prop_dist, int32_t* d_match_kp,
                             int32_t* d_match_point, int32_t* d_match_count)
{
    if (!ctx || !fr || !mp) return RS_ERR_INVALID;
    const int N = fr->n_keypoints, P = mp->n_points;
    if (N < 0 || P < 0 || point_base < 0) return rs_fail(ctx, RS_ERR_INVALID, "negative size");
    if (!d_match_count) return rs_fail(ctx, RS_ERR_INVALID, "null match_count");
    if (N >= (1 << 30)) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "too many keypoints");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    if (N == 0) {
        RS_HIP(ctx, hipMemsetAsync(d_match_count, 0, sizeof(int32_t), ctx->stream));
        if (P > 0 && d_point_kp) RS_HIP(ctx, hipMemsetAsync(d_point_kp, 0xFF, sizeof(int32_t) * (size_t)P, ctx->stream));
        return RS_OK;
    }
    if (!d_prop_point || !d_prop_dist || !d_match_kp || !d_match_point)
        return rs_fail(ctx, RS_ERR_INVALID, "null output");
    if (P > 0 && (!d_point_kp || !d_point_dist || !mp->d_positions || !mp->d_eligible || !mp->d_obs_ptr))
        return rs_fail(ctx, RS_ERR_INVALID, "null map pointer");
    bool fresh = false;                  // grow-only, in steps of 4096; all-ones once, every call leaves it all-ones again
    const int prc = ctx->prop.reserve(ctx, (size_t)N, 4096, 0, &fresh, RS_GROW_ROUND_UP);
    if (prc) return prc;
    if (fresh) RS_HIP(ctx, hipMemsetAsync(ctx->prop, 0xFF, sizeof(unsigned long long) * ctx->prop.cap, ctx->stream));
    unsigned long long* prop = ctx->prop;
    if (P > 0) {
        K2Frame f;
        memcpy(f.T, fr->pose, sizeof f.T);
        f.fx = fr->fx; f.fy = fr->fy; f.cx = fr->cx; f.cy = fr->cy;
        f.width = fr->width; f.height = fr->height; f.n_keypoints = N; f.kd_root = fr->kd_root;
        f.kp = (const float2*)fr->d_keypoints; f.desc = (const uint4*)fr->d_descriptors;
        f.kp_matched = fr->d_kp_matched; f.kd_node_kp = fr->d_kd_node_kp; f.kd_left = fr->d_kd_left;
        f.kd_right = fr->d_kd_right;
        f.packed = (const float4*)fr->d_kd_packed;
        if (((uintptr_t)f.packed) & 15) return rs_fail(ctx, RS_ERR_INVALID, "d_kd_packed must be 16-byte aligned");
        K2Map m;
        m.n_points = P; m.point_base = point_base; m.pos = mp->d_positions; m.eligible = mp->d_eligible; m.obs_ptr = mp->d_obs_ptr;
        m.obs_kf = mp->d_obs_kf; m.obs_desc = mp->d_obs_desc; m.kf_centers = mp->d_kf_centers;
        m.pool = (const uint4*)mp->d_desc_pool;
        const int tree_in_lds = N <= K2_MAX_LDS_NODES ? 1 : 0;
        rs_prof_scope ps(ctx, "K2_reproj_match");
        if (ctx->k2_mode == 0 && ctx->k2_grid && f.packed && rs_k2_grid_usable(fr->d_kd_grid, N) && fr->width <= K2_GRID_MAX_IMAGE &&
            fr->height <= K2_GRID_MAX_IMAGE) {                            // eight lanes per map point, candidates from the cell grid
            const int pts = K2C_THREADS / K2G;
            hipLaunchKernelGGL(k2_reproj_match_grid, dim3((P + pts - 1) / pts), dim3(K2C_THREADS), 0, ctx->stream, f, m,
                               (const int*)fr->d_kd_grid, replace, max_distance, d_point_kp, d_point_dist, prop);
        } else if (tree_in_lds && ctx->k2_mode == 0) {                    // eight lanes per map point
            const int pts = K2G_THREADS / K2G;
            const size_t lds = k2_lds_bytes(pts, N);
            if (lds > 48 * 1024)
                RS_HIP(ctx, rs_lds_attr((const void*)k2_reproj_match_grouped, lds));
            hipLaunchKernelGGL(k2_reproj_match_grouped, dim3((P + pts - 1) / pts), dim3(K2G_THREADS), lds,
                               ctx->stream, f, m, replace, max_distance, d_point_kp, d_point_dist, prop);
        } else {
            const size_t lds = k2_lds_bytes(K2_THREADS, tree_in_lds ? N : 0);
            if (lds > 48 * 1024)
                RS_HIP(ctx, rs_lds_attr((const void*)k2_reproj_match, lds));
            hipLaunchKernelGGL(k2_reproj_match, dim3((P + K2_THREADS - 1) / K2_THREADS), dim3(K2_THREADS), lds,
                               ctx->stream, f, m, replace, max_distance, tree_in_lds, d_point_kp, d_point_dist, prop);
        }
    }
    if (reduce && rs_comm_active(ctx)) {
        rs_prof_scope ps(ctx, "C3_allreduce_min_proposals");
        const int rc = rs_allreduce_min_u64(ctx, prop, (size_t)N);
        if (rc) return rc;
    }
    {
        rs_prof_scope ps(ctx, "K3_accept");
        hipLaunchKernelGGL(k3_accept, dim3(1), dim3(1024), 0, ctx->stream, prop, N, max_distance, d_prop_point,
                           d_prop_dist, d_match_kp, d_match_point, d_match_count);
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_reproj_match(rs_context* ctx, const rs_frame_view* fr, const rs_map_view* mp, int replace,
                               int max_distance, int32_t* d_point_kp, int32_t* d_point_dist,
                               int32_t* d_prop_point, int32_t* d_prop_dist, int32_t* d_match_kp,
                               int32_t* d_match_point, int32_t* d_match_count)
{
    return reproj_match_impl(ctx, fr, mp, 0, false, replace, max_distance, d_point_kp, d_point_dist, d_prop_point, d_prop_dist, d_match_kp,
                             d_match_point, d_match_count);
}

extern "C" int rs_reproj_match_sharded(rs_context* ctx, const rs_frame_view* fr, const rs_map_view* mp_shard, int point_base, int replace,
                                       int max_distance, int32_t* d_point_kp, int32_t* d_point_dist,
                                       int32_t* d_prop_point, int32_t* d_prop_dist, int32_t* d_match_kp,
                                       int32_t* d_match_point, int32_t* d_match_count)
{
    return reproj_match_impl(ctx, fr, mp_shard, point_base, true, replace, max_distance, d_point_kp, d_point_dist, d_prop_point, d_prop_dist,
                             d_match_kp, d_match_point, d_match_count);
}

// rs_kdtree_pack: the frame's KD-tree as K2 wants it in LDS — {x, y, left, right} per node, then the node's keypoint
// index — so that the workgroups of the (two) match calls of a frame copy it instead of gathering it.
__global__ __launch_bounds__(256) void k2_pack_tree(int n, const float2* __restrict__ kp, const int32_t* __restrict__ node_kp,
                                                    const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                    float4* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int kpi = node_kp[i];
    const float2 q = kp[kpi];
    out[i] = make_float4(q.x, q.y, __int_as_float(left[i]), __int_as_float(right[i]));
    ((int*)(out + n))[i] = kpi;
}

extern "C" int rs_kdtree_pack(rs_context* ctx, const rs_frame_view* fr, void* d_packed)
{
    if (!ctx || !fr) return RS_ERR_INVALID;
    const int n = fr->n_keypoints;
    if (n < 0) return rs_fail(ctx, RS_ERR_INVALID, "negative size");
    if (n == 0) return RS_OK;
    if (!d_packed || !fr->d_keypoints || !fr->d_kd_node_kp || !fr->d_kd_left || !fr->d_kd_right) return rs_fail(ctx, RS_ERR_INVALID, "null pointer");
    if (((uintptr_t)d_packed) & 15) return rs_fail(ctx, RS_ERR_INVALID, "d_packed must be 16-byte aligned");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k2_pack_tree, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, (const float2*)fr->d_keypoints,
                       fr->d_kd_node_kp, fr->d_kd_left, fr->d_kd_right, (float4*)d_packed);
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

// ------------------------------------------------------------------------------------------------ rs_kdtree_grid_build
// Three small launches, once per frame.  k2_grid_classify_rank also decides `usable` when asked to: the grid kernel may stand
// in for the walk only if (a) the tree has the implicit shape (children are the mids of the node's half ranges), (b) every
// node lies on the correct side of each ancestor on that ancestor's axis (left: coord <= ancestor's, right: >=), so that the
// walk's pruning never hides an in-radius node and k2_visited_before's order is the recursion's, and (c) every coordinate
// is finite (a NaN sends the reference's walk right and makes it miss the left subtree).
__global__ __launch_bounds__(256) void k2_grid_init(int* __restrict__ grid, int nx, int ny, int n, int* __restrict__ rank)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        K2Grid h = {nx, ny, K2_CELL, n, 1, {0, 0, 0}};
        *(K2Grid*)grid = h;
    }
    if (i < nx * ny + 1) grid[sizeof(K2Grid) / sizeof(int) + i] = 0;
    if (i < n) rank[i] = 0;
}

// Tiles of 256 nodes i x 256 nodes j with j0 <= i0: rank[i] = #{j < i in i's cell}, one integer atomic per tile (exact,
// order-free).  The tiles of the first column also count their nodes into the cells and, if `validate`, check them.
__global__ __launch_bounds__(256) void k2_grid_classify_rank(int* __restrict__ grid, int nx, int ny, int n, const float4* __restrict__ packed,
                                                             int validate, int* __restrict__ cell_of_node, int* __restrict__ rank)
{
    __shared__ int cj[256];
    const int i0 = blockIdx.x * 256, j0 = blockIdx.y * 256;
    if (j0 > i0 || i0 >= n) return;
    const int t = threadIdx.x;
    cj[t] = -1;
    if (j0 + t < n) {
        const float4 q = packed[j0 + t];
        cj[t] = k2_cell_of(q.y, ny) * nx + k2_cell_of(q.x, nx);
    }
    __syncthreads();
    const int i = i0 + t;
    if (i >= n) return;
    const float4 nd = packed[i];
    const int ci = k2_cell_of(nd.y, ny) * nx + k2_cell_of(nd.x, nx), lim = min(256, i - j0);
    int cnt = 0;
    for (int q = 0; q < lim; q++) cnt += cj[q] == ci ? 1 : 0;
    if (cnt) atomicAdd(&rank[i], cnt);
    if (j0 != 0) return;
    cell_of_node[i] = ci;
    atomicAdd(&grid[sizeof(K2Grid) / sizeof(int) + ci + 1], 1);
    if (!validate) return;
    const int kp = ((const int*)(packed + n))[i];
    bool ok = isfinite(nd.x) && isfinite(nd.y) && (unsigned)kp < (unsigned)n;
    int s = 0, e = n, odd = 0, mid;
    for (;;) {                                                            // root -> i by arithmetic: at most log2(n) + 1 ancestors
        mid = (s + e) >> 1;
        if (mid == i) break;
        const float4 a = packed[mid];
        const float ca = odd ? a.y : a.x, cn = odd ? nd.y : nd.x;
        if (i < mid) { ok = ok && cn <= ca; e = mid; }
        else { ok = ok && cn >= ca; s = mid + 1; }
        odd ^= 1;
    }
    const int left = s < mid ? (s + mid) >> 1 : -1, right = mid + 1 < e ? (mid + 1 + e) >> 1 : -1;
    ok = ok && __float_as_int(nd.z) == left && __float_as_int(nd.w) == right;
    if (!ok) ((K2Grid*)grid)->usable = 0;
}

// One workgroup: cell_start[k] = number of keypoints in cells < k, in place over the counts at [k + 1]; then every node
// into its cell's range at its rank.
__global__ __launch_bounds__(1024) void k2_grid_scan_scatter(int* __restrict__ grid, int nx, int ny, int n, const float4* __restrict__ packed,
                                                             const int* __restrict__ cell_of_node, const int* __restrict__ rank)
{
    const int cells = nx * ny;
    int* cs = grid + sizeof(K2Grid) / sizeof(int);
    {
        int* c1 = cs + 1;
        const int chunk = (cells + 1023) / 1024, lo = min((int)threadIdx.x * chunk, cells), hi = min(lo + chunk, cells);
        int sum = 0;
        for (int k = lo; k < hi; k++) sum += c1[k];
        int total;
        int run = rs_block_exclusive_scan(sum, &total);
        for (int k = lo; k < hi; k++) { run += c1[k]; c1[k] = run; }
    }
    __syncthreads();
    uint4* entries = (uint4*)(cs + k2_grid_start_ints(nx, ny));
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float4 nd = packed[i];
        const int pos = min(cs[cell_of_node[i]] + rank[i], n - 1);        // (always below n: the counts are these cells')
        entries[pos] = make_uint4(__float_as_uint(nd.x), __float_as_uint(nd.y), (uint32_t)((const int*)(packed + n))[i], (uint32_t)i);
    }
}

extern "C" size_t rs_kdtree_grid_bytes(int n_keypoints, int width, int height)
{
    const size_t n = n_keypoints > 0 ? (size_t)n_keypoints : 0;
    return sizeof(K2Grid) + sizeof(int) * k2_grid_start_ints(k2_grid_dim(width), k2_grid_dim(height)) + 16 * n + 8 * n;
}

// Which grids may stand in for the walk is host knowledge (the kernel is chosen at launch), kept per process, not per
// context: a frame's view is handed to forked child contexts (the benchmark's front end runs its two matches on two of them).
static std::mutex k2_grids_mutex;
static std::vector<std::pair<const void*, int>> k2_grids;      // {grid, n}

static void k2_grid_forget_locked(const void* d_grid)
{
    for (size_t i = 0; i < k2_grids.size();)
        if (k2_grids[i].first == d_grid) k2_grids.erase(k2_grids.begin() + (long)i); else i++;
}

void rs_k2_grid_forget(const void* d_grid)
{
    std::lock_guard<std::mutex> lock(k2_grids_mutex);
    k2_grid_forget_locked(d_grid);
}

void rs_k2_grid_remember(const void* d_grid, int n)
{
    std::lock_guard<std::mutex> lock(k2_grids_mutex);
    k2_grid_forget_locked(d_grid);
    if (k2_grids.size() >= 4096) k2_grids.erase(k2_grids.begin());      // a forgotten grid only means the walk
    k2_grids.push_back({d_grid, n});
}

bool rs_k2_grid_usable(const void* d_grid, int n)
{
    if (!d_grid) return false;
    std::lock_guard<std::mutex> lock(k2_grids_mutex);
    for (const auto& g : k2_grids)
        if (g.first == d_grid) return g.second == n;
    return false;
}

// the launches, on the context stream; false in *built: no grid for this frame (too many keypoints, or the root is not n / 2).
// validate 0: the caller knows the tree to be this library's own over finite coordinates.
int rs_k2_grid_enqueue(rs_context* ctx, int n, int kd_root, const void* d_packed, int width, int height, void* d_grid, bool validate, bool* built)
{
    *built = false;
    if (n <= 0 || n > K2_GRID_MAX_N || kd_root != n / 2) return RS_OK;
    const int nx = k2_grid_dim(width), ny = k2_grid_dim(height);
    int* grid = (int*)d_grid;
    const float4* packed = (const float4*)d_packed;
    int* cell_of_node = (int*)((char*)d_grid + rs_kdtree_grid_bytes(n, width, height) - 8 * (size_t)n), *rank = cell_of_node + n;
    hipStream_t s = ctx->stream;
    rs_prof_scope ps(ctx, "K2g_grid_build");
    const int nb = (n + 255) / 256, most = max(n, nx * ny + 1);
    hipLaunchKernelGGL(k2_grid_init, dim3((most + 255) / 256), dim3(256), 0, s, grid, nx, ny, n, rank);
    hipLaunchKernelGGL(k2_grid_classify_rank, dim3(nb, nb), dim3(256), 0, s, grid, nx, ny, n, packed, validate ? 1 : 0, cell_of_node, rank);
    hipLaunchKernelGGL(k2_grid_scan_scatter, dim3(1), dim3(1024), 0, s, grid, nx, ny, n, packed, (const int*)cell_of_node, (const int*)rank);
    RS_HIP(ctx, hipGetLastError());
    *built = true;
    return RS_OK;
}

extern "C" int rs_kdtree_grid_build(rs_context* ctx, const rs_frame_view* fr, void* d_grid)
{
    if (!ctx || !fr) return RS_ERR_INVALID;
    const int n = fr->n_keypoints;
    if (n < 0) return rs_fail(ctx, RS_ERR_INVALID, "negative size");
    if (!d_grid) return rs_fail(ctx, RS_ERR_INVALID, "null pointer");
    if (((uintptr_t)d_grid) & 15) return rs_fail(ctx, RS_ERR_INVALID, "d_grid must be 16-byte aligned");
    rs_k2_grid_forget(d_grid);
    if (n == 0) return RS_OK;
    if (!fr->d_kd_packed) return rs_fail(ctx, RS_ERR_INVALID, "rs_kdtree_grid_build needs the frame's d_kd_packed");
    if (((uintptr_t)fr->d_kd_packed) & 15) return rs_fail(ctx, RS_ERR_INVALID, "d_kd_packed must be 16-byte aligned");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    bool built = false;
    int rc = rs_k2_grid_enqueue(ctx, n, fr->kd_root, fr->d_kd_packed, fr->width, fr->height, d_grid, true, &built);
    if (rc || !built) return rc;
    // once per frame: whether the grid may stand in for the walk is decided on the device and remembered on the host
    K2Grid h;
    RS_HIP(ctx, hipMemcpyAsync(&h, d_grid, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h.usable) rs_k2_grid_remember(d_grid, n);
    return RS_OK;
}
