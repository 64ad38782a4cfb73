// l2_match.hip — K12 / K13: the two matchers for FLOAT descriptors under the L2 norm (MapMatcher constructed with
// cv::NORM_L2: rows of `dim` f32, dim % 4 == 0, 4 .. 1024).
//
// K12 (rs_l2_knn2, rs_match_descriptors_f32): brute-force 2-NN.  The specification ("D-dot", include/rsgpu.h) is all f32:
//   s = fmaf chain of q[k] * t[k] over ascending k;  nq2, nt2 the same chain of a row with itself;
//   d2 = fmaxf(fmaf(-2, s, nq2 + nt2), 0);  dist = sqrtf(d2);  candidates ordered by (d2, train index).
// The chain is what v_mfma_f32_32x32x2_f32 computes over ascending k on ONE accumulator: a step adds k (lanes 0..31) and
// then k + 1 (lanes 32..63) to C with one rounding per product.  Mapping: a workgroup of four waves owns 32 queries (the B
// operand, so a result's query is its lane's column) and walks its share of the train rows 128 at a time, each wave a
// 32-row tile (the A operand: a lane's 16 results are 16 train rows of ONE query).  Operands go through LDS in chunks of
// 32 k, row stride 33 words (conflict-free reads in the lane map A[l & 31][l >> 5], B[l >> 5][l & 31]); the
// accumulator lives across the chunks, so k is never split.  Rows past nq / nt are staged as zeros and masked at the
// insert.  Every lane keeps the two smallest keys (d2 bits << 32 | train index) of its query; lanes l and l + 32, the
// four waves (LDS) and the train splits (a table in the workspace, no atomics) are merged by minima of unique keys.
// K12b: one workgroup per batch item merges the splits, takes the square roots, applies the filters of
// src/MapMatcher.cpp:150-161 and writes the accepted queries in ascending order.
//
// K13 (rs_reproj_match_l2): the reprojection-gated matcher.  Sixteen lanes per map point: the gates and the KD-tree walk
// (global memory, explicit stack, the recursion's order) are uniform over the group; in-radius open keypoints are queued
// sixteen at a time, one per lane's register, and a full queue is flushed: its (candidate, observation) pairs are dealt
// over the lanes, ONE lane computing a pair's whole chain ("D-diff": four accumulators r[k & 3] = fmaf(e, e, r[k & 3]),
// e = q[k] - t[k], d2 = (r0 + r1) + (r2 + r3), dist = sqrtf(d2)), and the flush's winner is the minimum of
// dist bits << 32 | pair ordinal among dist < max_distance.  A later flush replaces the running best only on a strictly
// smaller distance: the reference's strict '<' over candidates in visiting order and observations in list order.  The
// per-keypoint table is K2's (packed u64 atomicMin, all-ones between calls), decoded by K13b with float distances.
// Built with -ffp-contract=off: every fused operation is an explicit fmaf.
#include "common.h"
#include "tri_core.h"
#include "reproj_gates.h"

#include <algorithm>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

#define L2_WAVES 4
#define L2_TILE 32               // one MFMA tile: 32 train rows x 32 queries
#define L2_KC 32                 // k per LDS chunk
#define L2_STRIDE (L2_KC + 1)    // LDS row stride in words
#define L2_KEY_NONE (~0ull)
#define L2_MAX_ROWS (0x7fffffff - L2_WAVES * L2_TILE)     // nq, nt: rounding up to a 128-row pass stays inside int

__device__ __forceinline__ void l2_top2_insert(u64& k0, u64& k1, u64 key)
{
    const u64 hi = k0 > key ? k0 : key;
    k1 = k1 < hi ? k1 : hi;
    k0 = k0 < key ? k0 : key;
}

// nq2 / nt2: one lane per row, the same ascending fmaf chain as the products
// (query rows first, then train rows, in one launch: a lane's loads stride dim floats from its neighbour's, which the caches
// absorb at these sizes; a launch more would cost more than that)
__global__ __launch_bounds__(256) void l2_row_norms(const float4* __restrict__ q_rows, size_t nq_rows, const float4* __restrict__ t_rows,
                                                    size_t nt_rows, int dim4, float* __restrict__ q_out, float* __restrict__ t_out)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq_rows + nt_rows) return;
    const bool is_q = i < nq_rows;
    if (!is_q) i -= nq_rows;
    float* out = is_q ? q_out : t_out;
    const float4* r = (is_q ? q_rows : t_rows) + i * (size_t)dim4;
    float s = 0.0f;
    for (int k = 0; k < dim4; k++) {
        const float4 v = r[k];
        s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
    }
    out[i] = s;
}

__global__ __launch_bounds__(64 * L2_WAVES) void l2_knn2_mfma(
    const float* __restrict__ query, int nq, const float* __restrict__ train, int nt, int dim,
    const float* __restrict__ qnorm, const float* __restrict__ tnorm, int passes_per_split, int n_passes, int nsplit, int nqb,
    ulonglong2* __restrict__ part)
{
    __shared__ float Qs[L2_TILE][L2_STRIDE];
    __shared__ float Ts[L2_WAVES * L2_TILE][L2_STRIDE];
    __shared__ u64 mk[L2_WAVES][2][L2_TILE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int per_pair = nqb * nsplit;
    const int b = (int)blockIdx.x / per_pair, rem = (int)blockIdx.x % per_pair;
    const int split = rem / nqb, q0 = (rem % nqb) * L2_TILE;
    const float* q = query + (size_t)b * nq * dim;
    const float* t = train + (size_t)b * nt * dim;
    const float* tn = tnorm + (size_t)b * nt;
    const int col = lane & 31, half = lane >> 5;
    const int qi = q0 + col;
    const float nq2 = qi < nq ? qnorm[(size_t)b * nq + qi] : 0.0f;

    u64 k0 = L2_KEY_NONE, k1 = L2_KEY_NONE;
    const int pass_end = min((split + 1) * passes_per_split, n_passes);
    for (int pass = split * passes_per_split; pass < pass_end; pass++) {
        const int tbase = pass * (L2_WAVES * L2_TILE);
        const int tile0 = tbase + wave * L2_TILE;                 // this wave's 32 train rows
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.0f;
        for (int kb = 0; kb < dim; kb += L2_KC) {
            const int kc = min(L2_KC, dim - kb);                  // a multiple of 4: no k is ever padded
            __syncthreads();                                      // the previous chunk has been read
#pragma unroll
            for (int it = 0; it < (L2_TILE + L2_WAVES * L2_TILE) * (L2_KC / 4) / (64 * L2_WAVES); it++) {
                const int idx = it * (64 * L2_WAVES) + (int)threadIdx.x;
                const int row = idx / (L2_KC / 4), kq = (idx % (L2_KC / 4)) * 4;
                if (kq < kc) {
                    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    float* dst;
                    if (row < L2_TILE) {
                        if (q0 + row < nq) v = *(const float4*)(q + (size_t)(q0 + row) * dim + kb + kq);
                        dst = &Qs[row][kq];
                    } else {
                        const int tr = tbase + row - L2_TILE;
                        if (tr < nt) v = *(const float4*)(t + (size_t)tr * dim + kb + kq);
                        dst = &Ts[row - L2_TILE][kq];
                    }
                    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
                }
            }
            __syncthreads();
            if (tile0 < nt)                                       // (wave-uniform) a tile wholly past nt has nothing to insert
                for (int kk = 0; kk < kc; kk += 2) {
                    const float a = Ts[wave * L2_TILE + col][kk + half];      // A[i = l & 31][k = l >> 5]: train rows
                    const float bq = Qs[col][kk + half];                      // B[k = l >> 5][j = l & 31]: queries
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq, acc, 0, 0, 0);
                }
        }
        // C/D: column = lane & 31 (the query), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (the train row of the tile)
        if (qi < nq) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int tr = tile0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (tr < nt) {
                    const float d2 = fmaxf(fmaf(-2.0f, acc[r], nq2 + tn[tr]), 0.0f);
                    l2_top2_insert(k0, k1, ((u64)__float_as_uint(d2) << 32) | (unsigned)tr);
                }
            }
        }
    }
    {   // lanes l and l + 32 hold disjoint train rows of the same query
        const u64 o0 = __shfl_xor(k0, 32), o1 = __shfl_xor(k1, 32);
        l2_top2_insert(k0, k1, o0);
        l2_top2_insert(k0, k1, o1);
    }
    if (half == 0) { mk[wave][0][col] = k0; mk[wave][1][col] = k1; }
    __syncthreads();
    if (wave == 0 && half == 0 && qi < nq) {
#pragma unroll
        for (int w = 1; w < L2_WAVES; w++) {
            l2_top2_insert(k0, k1, mk[w][0][col]);
            l2_top2_insert(k0, k1, mk[w][1][col]);
        }
        ulonglong2 o;
        o.x = k0; o.y = k1;
        part[((size_t)b * nq + qi) * nsplit + split] = o;
    }
}

// K12b: one workgroup per batch item; a query per thread and pass, so thread order is query order
__global__ __launch_bounds__(1024) void l2_merge_filter(
    const ulonglong2* __restrict__ part, int nq, int nt, int nsplit, float max_distance, int do_filter,
    int32_t* __restrict__ idx0, float* __restrict__ dist0, int32_t* __restrict__ idx1, float* __restrict__ dist1,
    int32_t* __restrict__ match_query, int32_t* __restrict__ match_train, int32_t* __restrict__ match_count)
{
    const int b = blockIdx.x;
    int running = 0;
    for (int base = 0; base < nq; base += 1024) {
        const int qi = base + (int)threadIdx.x;
        const bool live = qi < nq;
        u64 k0 = L2_KEY_NONE, k1 = L2_KEY_NONE;
        if (live)
            for (int s = 0; s < nsplit; s++) {
                const ulonglong2 v = part[((size_t)b * nq + qi) * nsplit + s];
                l2_top2_insert(k0, k1, v.x);
                l2_top2_insert(k0, k1, v.y);
            }
        const bool has1 = k1 != L2_KEY_NONE;
        const int i0 = (int)(unsigned)(k0 & 0xFFFFFFFFull), i1 = has1 ? (int)(unsigned)(k1 & 0xFFFFFFFFull) : -1;
        const float d0 = sqrtf(__uint_as_float((unsigned)(k0 >> 32)));
        const float d1 = has1 ? sqrtf(__uint_as_float((unsigned)(k1 >> 32))) : -1.0f;
        if (live) {
            const size_t o = (size_t)b * nq + qi;
            if (idx0) idx0[o] = i0;
            if (dist0) dist0[o] = d0;
            if (idx1) idx1[o] = i1;
            if (dist1) dist1[o] = d1;
        }
        if (!do_filter) continue;
        // :152 and :156 as acceptances: a NaN max_distance or NaN dist fails both.  (Non-finite ROWS are outside the contract:
        // fmaxf turns a NaN d2 into 0, so such a pair has distance 0 here and in the restatement alike.)
        const bool ok = live && d0 <= max_distance && (nt < 2 || d0 <= 0.75f * d1);
        int total;
        const int off = running + rs_block_exclusive_scan(ok ? 1 : 0, &total);
        if (ok) {
            match_query[(size_t)b * nq + off] = qi;
            match_train[(size_t)b * nq + off] = i0;
        }
        running += total;
    }
    if (do_filter && threadIdx.x == 0) match_count[b] = running;
}

static bool l2_dim_ok(int dim) { return dim >= 4 && dim <= 1024 && dim % 4 == 0; }

static int l2_knn2_launch(rs_context* ctx, const float* d_query, int nq, const float* d_train, int nt, int dim, int batch,
                          float max_distance, int do_filter, int32_t* mq, int32_t* mt, int32_t* mc, int32_t* i0, float* d0,
                          int32_t* i1, float* d1)
{
    if (!ctx) return RS_ERR_INVALID;
    if (nq < 0 || nt < 0 || batch < 0) return rs_fail(ctx, RS_ERR_INVALID, "negative size");
    if (!l2_dim_ok(dim)) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "dim must be a multiple of 4 in 4 .. 1024");
    // row numbers are rounded up to whole tiles and passes in int arithmetic, on the host and in the kernel
    if (nq > L2_MAX_ROWS || nt > L2_MAX_ROWS) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "nq and nt must be at most 2^31 - 129");
    if (batch == 0) return RS_OK;
    RS_HIP(ctx, hipSetDevice(ctx->device));
    if (nq == 0 || nt == 0) {   // empty guard, src/MapMatcher.cpp:139-141
        if (do_filter && mc) RS_HIP(ctx, hipMemsetAsync(mc, 0, sizeof(int32_t) * (size_t)batch, ctx->stream));
        return RS_OK;
    }
    if (!d_query || !d_train) return rs_fail(ctx, RS_ERR_INVALID, "null descriptor pointer");
    if (((uintptr_t)d_query | (uintptr_t)d_train) & 15) return rs_fail(ctx, RS_ERR_INVALID, "descriptors must be 16-byte aligned");
    if (do_filter && (!mq || !mt || !mc)) return rs_fail(ctx, RS_ERR_INVALID, "null match output");

    const int nqb = (nq + L2_TILE - 1) / L2_TILE;
    const int n_passes = (nt + L2_WAVES * L2_TILE - 1) / (L2_WAVES * L2_TILE);
    // aim at ~4 workgroups per compute unit; a split is at least one pass of 128 train rows
    const size_t wgs = (size_t)nqb * batch;
    int nsplit = (int)std::min<size_t>((size_t)n_passes, (4 * (size_t)ctx->n_cu + wgs - 1) / wgs);
    if (nsplit < 1) nsplit = 1;
    const int passes_per_split = (n_passes + nsplit - 1) / nsplit;
    nsplit = (n_passes + passes_per_split - 1) / passes_per_split;          // no empty split
    if (wgs * nsplit > 0x7fffffffu) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "too many query blocks for one launch");
    const size_t q_rows = (size_t)batch * nq, t_rows = (size_t)batch * nt;
    if ((q_rows + t_rows + 255) / 256 > 0x7fffffffu)
        return rs_fail(ctx, RS_ERR_UNSUPPORTED, "too many descriptor rows for one launch");
    float *qn = nullptr, *tn = nullptr;
    ulonglong2* part = nullptr;
    const int rc = rs_carve_from(ctx, rs_workspace, [&](rs_carve& c) {
        qn = c.take<float>(q_rows); tn = c.take<float>(t_rows); part = c.take<ulonglong2>(q_rows * nsplit);
    });
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    {
        rs_prof_scope ps(ctx, "K12p_l2_norms");
        hipLaunchKernelGGL(l2_row_norms, dim3((unsigned)((q_rows + t_rows + 255) / 256)), dim3(256), 0, s, (const float4*)d_query, q_rows,
                           (const float4*)d_train, t_rows, dim / 4, qn, tn);
    }
    {
        rs_prof_scope ps(ctx, "K12_l2_knn2");
        hipLaunchKernelGGL(l2_knn2_mfma, dim3((unsigned)(wgs * nsplit)), dim3(64 * L2_WAVES), 0, s, d_query, nq, d_train, nt, dim,
                           (const float*)qn, (const float*)tn, passes_per_split, n_passes, nsplit, nqb, part);
    }
    {
        rs_prof_scope ps(ctx, "K12b_merge_filter");
        hipLaunchKernelGGL(l2_merge_filter, dim3(batch), dim3(1024), 0, s, (const ulonglong2*)part, nq, nt, nsplit, max_distance,
                           do_filter, i0, d0, i1, d1, mq, mt, mc);
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_l2_knn2(rs_context* ctx, const float* d_query, int nq, const float* d_train, int nt, int dim, int batch,
                          int32_t* d_idx0, float* d_dist0, int32_t* d_idx1, float* d_dist1)
{
    return l2_knn2_launch(ctx, d_query, nq, d_train, nt, dim, batch, 0.0f, 0, nullptr, nullptr, nullptr, d_idx0, d_dist0, d_idx1, d_dist1);
}

extern "C" int rs_match_descriptors_f32(rs_context* ctx, const float* d_query, int nq, const float* d_train, int nt, int dim,
                                        int batch, float max_distance, int32_t* d_match_query, int32_t* d_match_train,
                                        int32_t* d_match_count, int32_t* d_idx0, float* d_dist0, int32_t* d_idx1, float* d_dist1)
{
    return l2_knn2_launch(ctx, d_query, nq, d_train, nt, dim, batch, max_distance, 1, d_match_query, d_match_train, d_match_count,
                          d_idx0, d_dist0, d_idx1, d_dist1);
}

// ------------------------------------------------------------------------------------------------ K13
#define L2R_G 16                 // lanes per map point: the candidate queue is one keypoint per lane
#define L2R_THREADS 256
#define L2R_PTS (L2R_THREADS / L2R_G)
#define L2R_STACK 40             // far children pending: at most one per level of the tree

struct L2Frame {
    float T[16];
    float fx, fy, cx, cy;
    int width, height, n_keypoints, kd_root;
    const float2* kp;
    const float* desc;
    const uint8_t* kp_matched;
    const int32_t* kd_node_kp;
    const int32_t* kd_left;
    const int32_t* kd_right;
};

struct L2Map {
    int n_points;
    const float* pos;
    const uint8_t* eligible;
    const int32_t* obs_ptr;
    const int32_t* obs_kf;
    const int32_t* obs_desc;
    const float* kf_centers;
    const float* pool;
};

__device__ __forceinline__ u64 l2_group_min(u64 v)
{
#pragma unroll
    for (int off = 1; off < L2R_G; off <<= 1) {
        const u64 o = __shfl_xor(v, off, L2R_G);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(L2R_THREADS) void l2_reproj_match(L2Frame f, L2Map m, int dim4, int replace, float max_distance,
                                                               int32_t* __restrict__ point_kp, float* __restrict__ point_dist,
                                                               u64* __restrict__ prop)
{
    // every lane of a group writes the same word and reads back what it wrote: no hand-off between lanes
    __shared__ int stack[L2R_STACK][L2R_PTS];
    const int g = threadIdx.x / L2R_G, sub = threadIdx.x % L2R_G;
    const int p = blockIdx.x * L2R_PTS + g;
    const bool have = p < m.n_points;
    const int pc = have ? p : 0;
    const bool elig = have && m.eligible[pc] != 0;
    const int o0 = m.obs_ptr[pc], o1 = m.obs_ptr[pc + 1];
    const int nobs = elig ? o1 - o0 : 0;
    const float X[3] = {m.pos[3 * (size_t)pc], m.pos[3 * (size_t)pc + 1], m.pos[3 * (size_t)pc + 2]};
    // everything below is uniform within a group of sixteen lanes except where `sub` appears
    int out_kp = -1;
    float out_d = max_distance;
    if (have) do {
        if (!elig) break;
        float T[16];
#pragma unroll
        for (int i = 0; i < 16; i++) T[i] = f.T[i];
        // Camera::project (src/Camera.cpp:25-32) and is_in_image (:34-37, src/MapMatcher.cpp:58)
        const TriParams k = {f.fx, f.fy, f.cx, f.cy, 0.0f, 0.0f};
        const float2 uv = project_f32(k, T, X);
        const float u = uv.x, v = uv.y;
        if (!(u >= 0.0f && u < (float)f.width && v >= 0.0f && v < (float)f.height)) break;
        float center[3];
        camera_center_f32(T, center);
        float normal[3] = {0.0f, 0.0f, 0.0f};
        float nearest = 3.402823466e+38f, furthest = 0.0f;
        for (int o = 0; o < nobs; o++) {                                   // src/MapPoint.cpp:24-45, in observation order
            const float* C = m.kf_centers + 3 * (size_t)m.obs_kf[o0 + o];
            float d[3] = {X[0] - C[0], X[1] - C[1], X[2] - C[2]};
            const float dist = sqrtf(dot3f(d, d));
            nearest = dist < nearest ? dist : nearest;
            furthest = furthest < dist ? dist : furthest;
            normalize3f(d);
            normalize3f(d);
            normal[0] += d[0]; normal[1] += d[1]; normal[2] += d[2];
        }
        if (!k2_view_gates(normal, nearest, furthest, X, center)) break;

        int best_kp = 0;
        float best_d = max_distance;
        int nc = 0, my_kp = 0;                                             // lane `sub` holds candidate `sub` of the queue
        // the queue's (candidate, observation) pairs, sixteen per step, one whole chain per lane (:84-91)
        auto flush = [&]() {
            const int npairs = nc * nobs;
            u64 best = L2_KEY_NONE;
            for (int base = 0; base < npairs; base += L2R_G) {
                const int i = base + sub;
                const bool valid = i < npairs;
                const int c = valid ? i / nobs : 0, o = valid ? i % nobs : 0;
                const int kp = __shfl(my_kp, c, L2R_G);
                if (valid) {
                    const float4* a = (const float4*)f.desc + (size_t)kp * dim4;
                    const float4* t = (const float4*)m.pool + (size_t)m.obs_desc[o0 + o] * dim4;
                    float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
                    for (int k4 = 0; k4 < dim4; k4++) {
                        const float4 x = a[k4], y = t[k4];
                        const float e0 = x.x - y.x, e1 = x.y - y.y, e2 = x.z - y.z, e3 = x.w - y.w;
                        r0 = fmaf(e0, e0, r0); r1 = fmaf(e1, e1, r1); r2 = fmaf(e2, e2, r2); r3 = fmaf(e3, e3, r3);
                    }
                    const float dist = sqrtf((r0 + r1) + (r2 + r3));
                    if (dist < max_distance) {
                        const u64 key = ((u64)__float_as_uint(dist) << 32) | (unsigned)i;
                        best = key < best ? key : best;
                    }
                }
            }
            best = l2_group_min(best);
            const int cw = best != L2_KEY_NONE ? (int)(unsigned)(best & 0xFFFFFFFFull) / nobs : 0;
            const int kw = __shfl(my_kp, cw, L2R_G);
            if (best != L2_KEY_NONE) {
                const float dw = __uint_as_float((unsigned)(best >> 32));
                if (dw < best_d) { best_d = dw; best_kp = kw; }            // an earlier flush keeps a tie
            }
            nc = 0;
        };
        // KDTree2D::radius_search around (u, v), r = 20 px (src/MapMatcher.cpp:75, src/KDTree.cpp:45-82): node, near child,
        // far child; only far children are pushed, with the depth parity of their level.
        // KEEP IN STEP BY HAND with K2_WALK's global-memory branch (reproj_match.hip), of which this is a copy: same f32
        // operations, same visiting order, same drop of a far child when the stack is full (never at depth <= 40); the
        // observation loop above likewise copies k2_reproj_match's add_obs, the double normalize3f included.
        const float r2 = 20.0f * 20.0f;
        int sp = 0, cur = f.kd_root, odd = 0;
        while (cur >= 0) {
            const int kp = f.kd_node_kp[cur];
            const float2 q = f.kp[kp];
            const int l = f.kd_left[cur], r = f.kd_right[cur];
            const float dx = q.x - u, dy = q.y - v;
            const float d2 = dx * dx + dy * dy;
            if (d2 <= r2 && (replace || !f.kp_matched[kp]) && nobs > 0) {   // in range and open (:65, :81)
                if (sub == nc) my_kp = kp;
                if (++nc == L2R_G) flush();
            }
            const float delta = odd ? dy : dx;
            const bool left_near = delta > 0;
            const int near_child = left_near ? l : r, far_child = left_near ? r : l;
            odd ^= 1;
            if (delta * delta <= r2 && far_child >= 0 && sp < L2R_STACK) stack[sp++][g] = far_child | (odd << 30);
            if (near_child >= 0) cur = near_child;
            else if (sp > 0) {
                const int e = stack[--sp][g];
                cur = e & 0x3FFFFFFF; odd = (e >> 30) & 1;
            } else cur = -1;
        }
        if (nc > 0) flush();
        if (best_d < max_distance) {
            out_kp = best_kp;
            out_d = best_d;
            // :95-97 sequential strict-'<' over map order == atomicMin of (dist, map order)
            if (sub == 0) atomicMin(&prop[best_kp], ((u64)__float_as_uint(best_d) << 32) | (unsigned)p);
        }
    } while (0);
    if (have && sub == 0) {
        point_kp[p] = out_kp;
        point_dist[p] = out_d;
    }
}

// K13b: accepted_matches (src/MapMatcher.cpp:34-43) by one workgroup, a keypoint per thread and pass; puts the table
// back to all-ones
__global__ __launch_bounds__(1024) void l2_accept(u64* __restrict__ prop, int n, float max_distance, int32_t* __restrict__ prop_point,
                                                  float* __restrict__ prop_dist, int32_t* __restrict__ match_kp,
                                                  int32_t* __restrict__ match_point, int32_t* __restrict__ match_count)
{
    int running = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const u64 v = i < n ? prop[i] : L2_KEY_NONE;
        const bool has = v != L2_KEY_NONE;
        int total;
        const int off = running + rs_block_exclusive_scan(has ? 1 : 0, &total);
        if (i < n) {
            int pt = -1;
            float dist = max_distance;
            if (has) {
                pt = (int)(unsigned)(v & 0xFFFFFFFFull);
                dist = __uint_as_float((unsigned)(v >> 32));
                match_kp[off] = i;
                match_point[off] = pt;
                prop[i] = L2_KEY_NONE;
            }
            prop_point[i] = pt;
            prop_dist[i] = dist;
        }
        running += total;
    }
    if (threadIdx.x == 0) *match_count = running;
}

__global__ __launch_bounds__(256) void l2_fill(float* __restrict__ out, int n, float value)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = value;
}

extern "C" int rs_reproj_match_l2(rs_context* ctx, const rs_frame_view* fr, const rs_map_view* mp, const float* d_frame_desc,
                                  const float* d_desc_pool, int dim, int replace, float max_distance, int32_t* d_point_kp,
                                  float* d_point_dist, int32_t* d_prop_point, float* d_prop_dist, int32_t* d_match_kp,
                                  int32_t* d_match_point, int32_t* d_match_count)
{
    if (!ctx || !fr || !mp) return RS_ERR_INVALID;
    const int N = fr->n_keypoints, P = mp->n_points;
    if (N < 0 || P < 0) return rs_fail(ctx, RS_ERR_INVALID, "negative size");
    if (!l2_dim_ok(dim)) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "dim must be a multiple of 4 in 4 .. 1024");
    if (!d_match_count) return rs_fail(ctx, RS_ERR_INVALID, "null match_count");
    if (N >= (1 << 30)) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "too many keypoints");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    if (N == 0) {                        // no keypoint: no point has a match
        RS_HIP(ctx, hipMemsetAsync(d_match_count, 0, sizeof(int32_t), ctx->stream));
        if (P > 0 && d_point_kp) RS_HIP(ctx, hipMemsetAsync(d_point_kp, 0xFF, sizeof(int32_t) * (size_t)P, ctx->stream));
        if (P > 0 && d_point_dist) {
            hipLaunchKernelGGL(l2_fill, dim3(((unsigned)P + 255u) / 256u), dim3(256), 0, ctx->stream, d_point_dist, P, max_distance);
            RS_HIP(ctx, hipGetLastError());
        }
        return RS_OK;
    }
    if (!d_prop_point || !d_prop_dist || !d_match_kp || !d_match_point) return rs_fail(ctx, RS_ERR_INVALID, "null output");
    if (P > 0 && (!d_point_kp || !d_point_dist || !mp->d_positions || !mp->d_eligible || !mp->d_obs_ptr || !d_frame_desc || !d_desc_pool))
        return rs_fail(ctx, RS_ERR_INVALID, "null map or descriptor pointer");
    if (((uintptr_t)d_frame_desc | (uintptr_t)d_desc_pool) & 15) return rs_fail(ctx, RS_ERR_INVALID, "descriptors must be 16-byte aligned");
    bool fresh = false;                  // K2's proposal table: grow-only, all-ones once, every call leaves it all-ones again
    const int prc = ctx->prop.reserve(ctx, (size_t)N, 4096, 0, &fresh, RS_GROW_ROUND_UP);
    if (prc) return prc;
    if (fresh) RS_HIP(ctx, hipMemsetAsync(ctx->prop, 0xFF, sizeof(u64) * ctx->prop.cap, ctx->stream));
    u64* prop = ctx->prop;
    if (P > 0) {
        L2Frame f;
        memcpy(f.T, fr->pose, sizeof f.T);
        f.fx = fr->fx; f.fy = fr->fy; f.cx = fr->cx; f.cy = fr->cy;
        f.width = fr->width; f.height = fr->height; f.n_keypoints = N; f.kd_root = fr->kd_root;
        f.kp = (const float2*)fr->d_keypoints; f.desc = d_frame_desc;
        f.kp_matched = fr->d_kp_matched; f.kd_node_kp = fr->d_kd_node_kp; f.kd_left = fr->d_kd_left; f.kd_right = fr->d_kd_right;
        L2Map m;
        m.n_points = P; m.pos = mp->d_positions; m.eligible = mp->d_eligible; m.obs_ptr = mp->d_obs_ptr;
        m.obs_kf = mp->d_obs_kf; m.obs_desc = mp->d_obs_desc; m.kf_centers = mp->d_kf_centers; m.pool = d_desc_pool;
        rs_prof_scope ps(ctx, "K13_reproj_match_l2");
        hipLaunchKernelGGL(l2_reproj_match, dim3((P + L2R_PTS - 1) / L2R_PTS), dim3(L2R_THREADS), 0, ctx->stream, f, m, dim / 4,
                           replace, max_distance, d_point_kp, d_point_dist, prop);
    }
    {
        rs_prof_scope ps(ctx, "K13b_accept");
        hipLaunchKernelGGL(l2_accept, dim3(1), dim3(1024), 0, ctx->stream, prop, N, max_distance, d_prop_point, d_prop_dist, d_match_kp,
                           d_match_point, d_match_count);
    }
    RS_HIP(ctx, hipGetLastError());
    return RS_OK;
}
