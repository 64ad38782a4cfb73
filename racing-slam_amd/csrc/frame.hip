// frame.hip — rs_frame: keypoints, descriptors and the flattened KD-tree, uploaded once and shared by the match calls of a
// frame.  rs_frame_create builds the tree on the host (rs_kdtree_build, host.cpp; reference src/Frame.cpp:8-15,
// src/KDTree.cpp:8-43).  The rest of this file is an rs_frame (re)filled from DEVICE arrays: the front end's keypoint lists
// and descriptor rows go into the frame's buffers and its KD-tree is built on the device, bit-identical to what
// rs_frame_create builds from the same data.
//
// rs_kdtree_build orders keypoints by the total order (coordinate, keypoint index); the node of a segment [s, e) at depth
// d is THE element of rank mid = (s + e) / 2 of that segment under axis d % 2, and its node id is mid.  Hence root, left[]
// and right[] depend on n alone and only node_kp[] on the data: there is one correct answer (tests/frame_ref.py restates
// what follows in numpy; tests/test_frame_ref_cpu.py holds it against rs_kdtree_build).
//
//   k_frame_gather   n_a / n_b by rs_describe_features' clamp, read on the device; keypoints a_0 .. b_0 .. and the first
//                    n descriptor rows into the frame; n to a device word; the rank table zeroed and the match table
//                    (frame_matches.hip) cleared to -1.
//   k_frame_rank     rank_x[i] = #{j : (key_x[j], j) < (key_x[i], i)}, likewise y, key = ordered_key(coordinate): a grid of
//                    (256 i) x (256 j) tiles, each adding its count with one INTEGER atomic (rank_x | rank_y << 16; exact,
//                    so repeated calls write the same bytes).  The ranks are two permutations of 0 .. n-1.
//   k_frame_build    one workgroup, integer only, on 16-bit ranks in LDS.  Per position p two lists: `cur`, sorted by the
//                    level's axis inside every segment, and `oth`, sorted by the other axis.  Per level every segment
//                    takes cur[mid] as its node (kept in a register; all are written out after the last level),
//                    then its part of `oth` is stably partitioned by rank_cur < rank_cur(node): one prefix sum over all
//                    positions, segment counts by difference.  The halves of `cur` are already sorted by the level's
//                    axis and become the children's `oth`.  floor(log2 n) + 1 levels, segment bounds from n alone.
#include "common.h"

#include <cmath>

#define FRAME_MAX_POINTS 8192          // the describer's and the detector's envelope
#define FB_THREADS 1024
#define FB_PER (FRAME_MAX_POINTS / FB_THREADS)      // consecutive positions per thread of k_frame_build

// f32 bits -> u32 whose unsigned order is the float order; -0 and +0 (equal as floats, then ordered by index) share a key
__device__ __forceinline__ uint32_t ordered_key(uint32_t b)
{
    if ((b << 1) == 0) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ void frame_counts(const int32_t* count_a, const int32_t* count_b, int cap, int* na, int* nb)
{
    int a = count_a ? count_a[0] : 0, b = count_b ? count_b[0] : 0;
    a = a < 0 ? 0 : (a > cap ? cap : a);
    b = b < 0 ? 0 : (b > cap - a ? cap - a : b);
    *na = a; *nb = b;
}

// one thread per 16 bytes of descriptor (two per row); thread t < cap also moves keypoint t and clears rank word t
__global__ __launch_bounds__(256) void k_frame_gather(int cap, const uint32_t* __restrict__ pt_a, const int32_t* __restrict__ count_a,
                                                      const uint32_t* __restrict__ pt_b, const int32_t* __restrict__ count_b,
                                                      const uint8_t* __restrict__ desc, int desc_aligned, uint32_t* __restrict__ kp,
                                                      uint8_t* __restrict__ out_desc, uint32_t* __restrict__ rank, int32_t* __restrict__ d_n,
                                                      int32_t* __restrict__ kp_point)
{
    int na, nb;
    frame_counts(pt_a ? count_a : nullptr, pt_b ? count_b : nullptr, cap, &na, &nb);
    const int n = na + nb;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) { d_n[0] = n; d_n[1] = 0; }              // [1]: every coordinate finite, set by k_frame_build
    if (t < cap) { rank[t] = 0; kp_point[t] = -1; }      // (the match table: no match yet)
    if (t < n) {
        const uint32_t* src = t < na ? pt_a + 2 * (size_t)t : pt_b + 2 * (size_t)(t - na);
        kp[2 * (size_t)t] = src[0];
        kp[2 * (size_t)t + 1] = src[1];
    }
    if (t < 2 * n) {
        if (desc_aligned) ((uint4*)out_desc)[t] = ((const uint4*)desc)[t];
        else
            for (int k = 0; k < 16; k++) out_desc[16 * (size_t)t + k] = desc[16 * (size_t)t + k];
    }
}

__global__ __launch_bounds__(256) void k_frame_rank(const int32_t* __restrict__ d_n, const uint32_t* __restrict__ kp, uint32_t* __restrict__ rank)
{
    __shared__ uint32_t kx[256], ky[256];
    const int n = d_n[0];
    const int i0 = blockIdx.x * 256, j0 = blockIdx.y * 256;
    if (i0 >= n || j0 >= n) return;
    const int jn = n - j0 < 256 ? n - j0 : 256;
    const int t = threadIdx.x;
    if (t < jn) { kx[t] = ordered_key(kp[2 * (size_t)(j0 + t)]); ky[t] = ordered_key(kp[2 * (size_t)(j0 + t) + 1]); }
    __syncthreads();
    const int i = i0 + t;
    if (i >= n) return;
    const uint32_t xi = ordered_key(kp[2 * (size_t)i]), yi = ordered_key(kp[2 * (size_t)i + 1]);
    // (key_j, j) < (key_i, i): key_j < key_i, or equal keys and j < i
    const int jlow = i - j0;              // j < i  <=>  its offset in the tile < jlow
    uint32_t cx = 0, cy = 0;
#pragma unroll 4
    for (int q = 0; q < jn; q++) {
        const uint32_t xj = kx[q], yj = ky[q];
        const bool before = q < jlow;
        cx += (xj < xi || (xj == xi && before)) ? 1u : 0u;
        cy += (yj < yi || (yj == yi && before)) ? 1u : 0u;
    }
    atomicAdd(&rank[i], cx | (cy << 16));
}

// dynamic LDS, in 16-bit words: rank_x [n] | rank_y [n] | three position lists [n] (cur, oth, the one being filled),
// then as u32 the prefix counts inside each thread's run of positions [n] and the threads' bases [FB_THREADS]
__global__ __launch_bounds__(FB_THREADS) void k_frame_build(int32_t* __restrict__ d_n, const uint32_t* __restrict__ rank,
                                                           const uint2* __restrict__ kp, int32_t* __restrict__ kd, uint4* __restrict__ packed)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t fb_lds[];
    const int n = d_n[0];
    if (n <= 0 || n > FRAME_MAX_POINTS) return;
    const int np = (n + 7) & ~7;          // every array starts 16-byte aligned
    uint16_t* rk[2] = {fb_lds, fb_lds + np};
    uint16_t* cur = fb_lds + 2 * np, *oth = fb_lds + 3 * np, *nxt = fb_lds + 4 * np;
    uint32_t* pre = (uint32_t*)(fb_lds + 5 * np), *tbase = pre + np;
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += FB_THREADS) {
        const uint32_t r = rank[i];
        const uint32_t rx = r & 0xFFFFu, ry = r >> 16;
        rk[0][i] = (uint16_t)rx; rk[1][i] = (uint16_t)ry;
        // ranks are permutations of 0 .. n-1 by construction; the clamp only keeps a corrupted table inside the arrays
        cur[rx < (uint32_t)n ? rx : n - 1] = (uint16_t)i;
        oth[ry < (uint32_t)n ? ry : n - 1] = (uint16_t)i;
    }
    // Each thread owns `per` = 1, 2, 4 or 8 consecutive positions p0 .. (the fewest that cover n: more threads, shorter
    // chains).  Their segments [s, e) as s | e << 16; bit 15 set: the position is a node already (or >= n) and the word
    // keeps the segment it was the middle of.
    const int shift = n <= FB_THREADS ? 0 : (n <= 2 * FB_THREADS ? 1 : (n <= 4 * FB_THREADS ? 2 : 3)), per = 1 << shift;
    const int p0 = tid << shift;
    uint32_t seg[FB_PER];
    int node[FB_PER];
#pragma unroll
    for (int k = 0; k < FB_PER; k++) { seg[k] = k < per && p0 + k < n ? (uint32_t)n << 16 : 0x8000u; node[k] = 0; }
    const int levels = 32 - __clz(n);
    __syncthreads();
    for (int depth = 0; depth < levels; depth++) {
        const uint16_t* r = rk[depth & 1];
        // 1: this thread's elements of `oth`: below the node's rank (low half) / the node itself (high half), counted
        uint32_t run = 0;
#pragma unroll
        for (int k = 0; k < FB_PER; k++) {
            if (k >= per) break;
            if (p0 + k < n) pre[p0 + k] = run;
            if (!(seg[k] & 0x8000u)) {
                const int m = (int)((seg[k] & 0xFFFFu) + (seg[k] >> 16)) >> 1;
                const int pivot = cur[m], v = oth[p0 + k];
                run += v == pivot ? 0x10000u : (r[v] < r[pivot] ? 1u : 0u);
            }
        }
        int total;
        const uint32_t base = (uint32_t)rs_block_exclusive_scan((int)run, &total);
        tbase[tid] = base;
        __syncthreads();
        // 2: scatter into the children's `cur`; the node of each segment is final
#pragma unroll
        for (int k = 0; k < FB_PER; k++) {
            if (k >= per) break;
            if (seg[k] & 0x8000u) continue;
            const int p = p0 + k, s = (int)(seg[k] & 0xFFFFu), e = (int)(seg[k] >> 16), m = (s + e) >> 1;
            const int pivot = cur[m], v = oth[p];
            const uint32_t d = base + pre[p] - (tbase[s >> shift] + pre[s]);
            const int lb = (int)(d & 0xFFFFu), pb = (int)(d >> 16);
            int dest = v == pivot ? m : (r[v] < r[pivot] ? s + lb : m + 1 + (p - s - lb - pb));
            dest = dest < 0 ? 0 : (dest >= n ? n - 1 : dest);      // (always inside [s, e) for permutation ranks)
            nxt[dest] = (uint16_t)v;
            if (p == m) { node[k] = pivot < n ? pivot : n - 1; seg[k] |= 0x8000u; }
            else if (p < m) seg[k] = (uint32_t)s | ((uint32_t)m << 16);
            else seg[k] = (uint32_t)(m + 1) | ((uint32_t)e << 16);
        }
        __syncthreads();
        uint16_t* t = oth; oth = cur; cur = nxt; nxt = t;
    }
    // every position is a node now: the flat arrays and the packed form, children from the segment alone
    int nonfinite = 0;
#pragma unroll
    for (int k = 0; k < FB_PER; k++) {
        const int p = p0 + k;
        if (k >= per || p >= n) break;
        const int s = (int)(seg[k] & 0x7FFFu), e = (int)(seg[k] >> 16), m = (s + e) >> 1;      // m == p
        const int left = s < m ? (s + m) >> 1 : -1, right = m + 1 < e ? (m + 1 + e) >> 1 : -1;
        const uint2 xy = kp[node[k]];
        kd[p] = node[k]; kd[(size_t)n + p] = left; kd[2 * (size_t)n + p] = right;
        packed[p] = make_uint4(xy.x, xy.y, (uint32_t)left, (uint32_t)right);
        ((int32_t*)(packed + n))[p] = node[k];
        nonfinite |= ((xy.x & 0x7F800000u) == 0x7F800000u || (xy.y & 0x7F800000u) == 0x7F800000u) ? 1 : 0;
    }
    nonfinite = __syncthreads_or(nonfinite);
    if (tid == 0) d_n[1] = nonfinite ? 0 : 1;
}

static size_t frame_build_lds(int cap)
{
    const size_t np = ((size_t)cap + 7) & ~(size_t)7;
    return 2 * 5 * np + 4 * np + 4 * FB_THREADS;
}

// The buffers of a frame of `rows` keypoints, its match table at -1 (no map match yet).  A frame with a tree has d_packed (one
// of no keypoints has none); an assignable frame (rs_frame_create_device) also gets the rank table, the two count words and
// the pinned word.  Both constructors go through here.
static int frame_alloc(rs_context* ctx, rs_frame* f, size_t rows, bool assignable)
{
    int rc = f->block.carve(ctx, "frame buffers", [&](rs_carve& c) {
        f->d_kp = c.take<float>(2 * rows);
        f->d_desc = c.take<uint8_t>(32 * rows);
        f->d_kd = c.take<int32_t>(3 * rows);
        f->d_matched = c.take<uint8_t>(rows);
        f->d_kp_point = c.take<int32_t>(rows);
        if (assignable || f->n > 0) f->d_packed = c.take<uint8_t>(20 * rows);
        if (assignable) {
            f->d_rank = c.take<uint32_t>(rows);
            f->d_n = c.take<int32_t>(2);
        }
    });
    if (!rc && assignable) rc = f->pin.carve(ctx, "frame count word", [&](rs_carve& c) { f->h_n = c.take<int32_t>(2); });
    if (rc) return rc;
    RS_HIP(ctx, hipMemsetAsync(f->d_kp_point, 0xFF, sizeof(int32_t) * rows, ctx->stream));
    return RS_OK;
}

// rs_frame_create's uploads: the caller's arrays, the tree rs_kdtree_build made of them (kd: node_kp | left | right, stride n)
// and its packed form (rs_kdtree_pack's layout).  Integer and copy work only: nothing here depends on this file's
// -ffp-contract=off.
static int frame_upload(rs_context* ctx, rs_frame* f, const float* h_kp, const uint8_t* h_desc, const std::vector<int32_t>& kd)
{
    const size_t m = (size_t)f->n;
    hipStream_t s = ctx->stream;
    std::vector<int32_t> packed(5 * m);
    for (size_t i = 0; i < m; i++) {
        const int32_t kpi = kd[i];
        memcpy(&packed[4 * i], &h_kp[2 * (size_t)kpi], 8);
        packed[4 * i + 2] = kd[m + i];
        packed[4 * i + 3] = kd[2 * m + i];
        packed[4 * m + i] = kpi;
    }
    RS_HIP(ctx, hipMemcpyAsync(f->d_kp, h_kp, sizeof(float) * 2 * m, hipMemcpyHostToDevice, s));
    RS_HIP(ctx, hipMemcpyAsync(f->d_desc, h_desc, 32 * m, hipMemcpyHostToDevice, s));
    RS_HIP(ctx, hipMemcpyAsync(f->d_kd, kd.data(), sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice, s));
    RS_HIP(ctx, hipMemcpyAsync(f->d_packed, packed.data(), 20 * m, hipMemcpyHostToDevice, s));
    RS_HIP(ctx, hipStreamSynchronize(s));       // the sources are the caller's / this call's memory
    return RS_OK;
}

extern "C" int rs_frame_create(rs_context* ctx, const float* h_kp, const uint8_t* h_desc, int n, rs_frame** out)
{
    if (!ctx || !out || n < 0 || (n > 0 && (!h_kp || !h_desc))) return RS_ERR_INVALID;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_frame* f = new rs_frame();
    f->ctx = ctx;
    f->n = n;
    const size_t m = n > 0 ? (size_t)n : 1;
    std::vector<int32_t> kd(3 * m);
    if (n > 0) rs_kdtree_build(h_kp, n, kd.data(), kd.data() + m, kd.data() + 2 * m, &f->kd_root);     // src/Frame.cpp:8-15
    int rc = frame_alloc(ctx, f, m, false);
    if (!rc && n > 0) rc = frame_upload(ctx, f, h_kp, h_desc, kd);       // (n == 0: no tree, d_packed stays null)
    f->finite = n > 0;
    for (size_t i = 0; i < 2 * (size_t)n; i++) f->finite = f->finite && std::isfinite(h_kp[i]);
    if (rc) { rs_frame_destroy(f); return rc; }
    *out = f;
    return RS_OK;
}

extern "C" int rs_frame_create_device(rs_context* ctx, int max_points, rs_frame** out)
{
    if (!ctx || !out) return RS_ERR_INVALID;
    if (max_points < 1 || max_points > FRAME_MAX_POINTS) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "rs_frame_create_device: max_points %d outside 1 .. %d", max_points, FRAME_MAX_POINTS);
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_frame* f = new rs_frame();
    f->ctx = ctx;
    f->cap = max_points;
    const int rc = frame_alloc(ctx, f, (size_t)max_points, true);
    if (rc) { rs_frame_destroy(f); return rc; }
    *f->h_n = 0;
    *out = f;
    return RS_OK;
}

extern "C" int rs_frame_destroy(rs_frame* f)
{
    if (!f) return RS_OK;
    (void)hipSetDevice(f->ctx->device);
    (void)hipStreamSynchronize(f->ctx->stream);
    rs_k2_grid_forget(f->grid.p);
    delete f;
    return RS_OK;
}

// the three launches of an assign on the context stream; rank tiles cover the first rank_n keypoints (cap when n is on the device only)
static int frame_enqueue(rs_context* ctx, rs_frame* f, const float* d_pt_a, const int32_t* d_count_a, const float* d_pt_b,
                         const int32_t* d_count_b, const uint8_t* d_desc, int rank_n)
{
    hipStream_t s = ctx->stream;
    const int cap = f->cap;
    rs_k2_grid_forget(f->grid.p);      // the grid, if any, is the previous keypoints'
    f->grid_built = false;
    f->finite = false;
    {
        rs_prof_scope ps(ctx, "KF_frame_gather");
        hipLaunchKernelGGL(k_frame_gather, dim3((2 * cap + 255) / 256), dim3(256), 0, s, cap, (const uint32_t*)d_pt_a, d_count_a,
                           (const uint32_t*)d_pt_b, d_count_b, d_desc, ((uintptr_t)d_desc & 15) == 0 ? 1 : 0, (uint32_t*)f->d_kp, f->d_desc,
                           f->d_rank, f->d_n, f->d_kp_point);
    }
    if (rank_n > 0) {
        rs_prof_scope ps(ctx, "KF_frame_rank");
        const int tiles = (rank_n + 255) / 256;
        hipLaunchKernelGGL(k_frame_rank, dim3(tiles, tiles), dim3(256), 0, s, f->d_n, (const uint32_t*)f->d_kp, f->d_rank);
    }
    {
        rs_prof_scope ps(ctx, "KF_frame_build");
        const size_t lds = frame_build_lds(cap);
        if (lds > 48 * 1024) RS_HIP(ctx, rs_lds_attr((const void*)k_frame_build, lds));
        hipLaunchKernelGGL(k_frame_build, dim3(1), dim3(FB_THREADS), lds, s, f->d_n, f->d_rank, (const uint2*)f->d_kp, f->d_kd, (uint4*)f->d_packed);
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_frame_assign_device(rs_context* ctx, rs_frame* f, const float* d_pt_a, const int32_t* d_count_a, const float* d_pt_b,
                                      const int32_t* d_count_b, const uint8_t* d_desc, int* h_n)
{
    if (!ctx || !f || f->ctx != ctx) return RS_ERR_INVALID;
    if (f->cap <= 0) return rs_fail(ctx, RS_ERR_INVALID, "rs_frame_assign_device: the frame was not made by rs_frame_create_device");
    if ((d_pt_a == nullptr) != (d_count_a == nullptr) || (d_pt_b == nullptr) != (d_count_b == nullptr))
        return rs_fail(ctx, RS_ERR_INVALID, "rs_frame_assign_device: a list is its points and its count together");
    if ((d_pt_a || d_pt_b) && !d_desc) return rs_fail(ctx, RS_ERR_INVALID, "rs_frame_assign_device: null descriptors");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int cap = f->cap;
    const int rc = frame_enqueue(ctx, f, d_pt_a, d_count_a, d_pt_b, d_count_b, d_desc, cap);
    if (rc) return rc;
    RS_HIP(ctx, hipMemcpyAsync(f->h_n, f->d_n, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    // the one host synchronisation: rs_map_match sizes its launches and rs_map_add_keyframe books pool rows by the host-side n
    RS_HIP(ctx, hipStreamSynchronize(s));
    const int n = *f->h_n;
    if (n < 0 || n > cap) return rs_fail(ctx, RS_ERR_HIP, "rs_frame_assign_device: count %d outside the frame", n);
    f->n = n;
    f->kd_root = n > 0 ? n / 2 : -1;
    f->finite = n > 0 && f->h_n[1] == 1;
    if (h_n) *h_n = n;
    return RS_OK;
}

int rs_frame_assign_enqueue(rs_context* ctx, rs_frame* f, const float* d_pt, const int32_t* d_count, const uint8_t* d_desc, int n)
{
    if (!ctx || !f || f->ctx != ctx || f->cap <= 0 || n < 0 || n > f->cap || !d_pt || !d_count || !d_desc) return RS_ERR_INVALID;
    const int rc = frame_enqueue(ctx, f, d_pt, d_count, nullptr, nullptr, d_desc, n);      // the host knows n: no rank tile beyond it
    if (rc) return rc;
    f->n = n;
    f->kd_root = n > 0 ? n / 2 : -1;
    return RS_OK;
}

extern "C" int rs_frame_download(rs_context* ctx, const rs_frame* f, int* h_n, float* h_kp, uint8_t* h_desc, int32_t* h_kd, int32_t* h_root,
                                 void* h_packed)
{
    if (!ctx || !f || f->ctx != ctx) return RS_ERR_INVALID;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)f->n;
    if (h_n) *h_n = f->n;
    if (h_root) *h_root = f->kd_root;
    if (n > 0) {
        if (h_kp) RS_HIP(ctx, hipMemcpyAsync(h_kp, f->d_kp, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, s));
        if (h_desc) RS_HIP(ctx, hipMemcpyAsync(h_desc, f->d_desc, 32 * n, hipMemcpyDeviceToHost, s));
        if (h_kd) RS_HIP(ctx, hipMemcpyAsync(h_kd, f->d_kd, sizeof(int32_t) * 3 * n, hipMemcpyDeviceToHost, s));
        if (h_packed) RS_HIP(ctx, hipMemcpyAsync(h_packed, f->d_packed, 20 * n, hipMemcpyDeviceToHost, s));
    }
    RS_HIP(ctx, hipStreamSynchronize(s));
    return RS_OK;
}

// The frame's cell grid for K2 (reproj_match.hip), made on the first match after the frame was filled: the tree is this
// file's own — implicit shape, every node on the correct side of its ancestors — so finite coordinates are all the grid
// needs, and those the host knows (rs_frame_create sees them, rs_frame_assign_device reads the verdict back with n).  A
// frame refilled by rs_frame_assign_enqueue, whose keypoints the host has never seen, has no grid: K2 walks its tree.
int rs_frame_grid(rs_context* ctx, rs_frame* f, int width, int height, const void** d_grid)
{
    *d_grid = nullptr;
    if (!f->finite || f->n <= 0 || !f->d_packed) return RS_OK;
    if (!(f->grid_built && f->grid_w == width && f->grid_h == height)) {
        rs_k2_grid_forget(f->grid.p);
        f->grid_built = false;
        const int rc = f->grid.reserve(ctx, rs_kdtree_grid_bytes(f->cap > 0 ? f->cap : f->n, width, height), 4096, 0, nullptr, RS_GROW_ROUND_UP);
        if (rc) return rc;
        bool built = false;
        const int rc2 = rs_k2_grid_enqueue(ctx, f->n, f->kd_root, f->d_packed, width, height, f->grid.p, false, &built);
        if (rc2 || !built) return rc2;
        rs_k2_grid_remember(f->grid.p, f->n);
        f->grid_built = true; f->grid_w = width; f->grid_h = height;
    }
    *d_grid = f->grid.p;
    return RS_OK;
}
