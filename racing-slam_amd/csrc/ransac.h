// ransac.h — the RANSAC frame of the pose stages, once.  pose.hip instantiates it for (S = 5, M = 10, D = 9) and pnp.hip
// for (S = 4, M = 4, D = 12): S indices per sample, up to M models per hypothesis, D doubles per model.  A stage adds its
// own solver (the *_hyp kernel), its residual (*_score) and what follows the best model (*_final).
//   the draw      hypothesis h takes its first S distinct finite indices of RANSAC_MAX_DRAWS hashed draws
//                 (tests/essential_ref.draw / sample)
//   the table     samples [H][S], nmod [H], models [H][M][D], scores [H][M]; reset by every call, so no entry outlives it
//   the key       (count << 32) | ~slot, slot = M h + m: one 64-bit atomicMax keeps the best count, the lowest slot on ties
//   the stop      after each round of RANSAC_ROUND: drawn >= log(1 - confidence) / log(1 - w^S), w = best count / n
//                 (tests/essential_ref.needed_hypotheses)
//   the inliers   the u8 mask over max_n and the ascending index list
// and, on the host, the table's layout / first fill / download and the argument checks of the entry points.
#pragma once
#include <algorithm>
#include <cmath>

#include "common.h"

#define RANSAC_MAX_POINTS 8192
#define RANSAC_MAX_HYP 4096
#define RANSAC_ROUND 256
#define RANSAC_MAX_DRAWS 64
#define RANSAC_STATUS_OK 0
#define RANSAC_STATUS_FEW 1             // fewer usable correspondences than a model needs
#define RANSAC_STATUS_FAILED 2          // no model with enough inliers

struct RansacTable {
    int32_t *samples, *nmod, *scores;
    double* models;
};

struct RansacState {
    unsigned long long best_key;
    int stop, drawn, n, scored, best_index, best_count;
};

__host__ __device__ __forceinline__ unsigned long long splitmix64(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the S indices of hypothesis h into idx (draw order); seed_hash = splitmix64(seed).  false = fewer than S found
template <int S>
__device__ __forceinline__ bool ransac_draw(unsigned long long seed_hash, int h, int n, const uint8_t* fin, int* idx)
{
    int k = 0;
    for (int j = 0; j < RANSAC_MAX_DRAWS && k < S; j++) {
        const unsigned long long u = splitmix64(seed_hash + (((unsigned long long)h << 16) | (unsigned long long)j));
        const int i = (int)(((u >> 32) * (unsigned long long)n) >> 32);
        bool dup = !fin[i];
        for (int q = 0; q < k; q++) dup |= idx[q] == i;
        if (!dup) idx[k++] = i;
    }
    return k == S;
}

// the estimator's whole table, by the whole grid
template <int S, int M>
__device__ __forceinline__ void ransac_reset_table(const RansacTable& t, int table_hyp)
{
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int h = tid; h < table_hyp; h += stride) {
        t.nmod[h] = -1;
#pragma unroll
        for (int k = 0; k < S; k++) t.samples[S * h + k] = -1;
#pragma unroll
        for (int k = 0; k < M; k++) t.scores[M * h + k] = 0;
    }
}

__device__ __forceinline__ unsigned long long ransac_key(int count, int slot)
{
    return ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)slot);
}

__device__ __forceinline__ int ransac_key_count(unsigned long long key) { return (int)(key >> 32); }

__device__ __forceinline__ int ransac_key_slot(unsigned long long key) { return (int)~(unsigned)(key & 0xFFFFFFFFull); }

// one thread, after round `round` was scored
template <int S>
__device__ __forceinline__ void ransac_stop(RansacState* st, int round, int max_hyp, double log1mconf)
{
    const int drawn = min((round + 1) * RANSAC_ROUND, max_hyp);
    st->drawn = drawn;
    const int cnt = ransac_key_count(st->best_key), n = st->n;
    double needed = INFINITY;
    if (n > 0 && cnt > 0) {
        const double w = (double)cnt / (double)n;
        double p = w;
#pragma unroll
        for (int k = 1; k < S; k++) p = p * w;
        if (p >= 1.0) needed = 0.0;
        else {
            const double d = log(1.0 - p);
            if (d < 0.0) needed = log1mconf / d;
        }
    }
    if ((double)drawn >= needed || drawn >= max_hyp) st->stop = 1;
}

// one workgroup: d_inlier [max_n] = ok && i < n && mask[i], d_inlier_index = those i ascending; returns their number
__device__ __forceinline__ int write_inliers(bool ok, int n, int max_n, const uint8_t* mask, uint8_t* __restrict__ d_inlier,
                                             int32_t* __restrict__ d_inlier_index)
{
    int base = 0;
    for (int c0 = 0; c0 < max_n; c0 += blockDim.x) {
        const int i = c0 + threadIdx.x;
        const int f = (ok && i < n && mask[i]) ? 1 : 0;
        if (i < max_n) d_inlier[i] = (uint8_t)f;
        int tot;
        const int off = rs_block_exclusive_scan(f, &tot);
        if (f) d_inlier_index[base + off] = i;
        base += tot;
    }
    return base;
}

// ------------------------------------------------------------------------------------------------ host side
struct RansacEstimator {                // what rs_pose_estimator and rs_pnp_estimator begin with
    rs_context* ctx = nullptr;
    int max_points = 0, max_hyp = 0;
    RansacTable t = {};                 // [max_hyp] entries
    rs_dev_block block;                 // the table and the stage's own arrays
};

// the stage's state at zero and the table as a call's reset would leave it (models 0); synchronises the stream
template <class E>
static inline int ransac_first_fill(rs_context* ctx, E* e, size_t H, int S, int M, int D)
{
    const RansacTable& t = e->t;
    hipStream_t stream = ctx->stream;
    RS_HIP(ctx, hipMemsetAsync(e->st, 0, sizeof *e->st, stream));
    RS_HIP(ctx, hipMemsetAsync(t.samples, 0xFF, S * H * sizeof(int32_t), stream));
    RS_HIP(ctx, hipMemsetAsync(t.nmod, 0xFF, H * sizeof(int32_t), stream));
    RS_HIP(ctx, hipMemsetAsync(t.scores, 0, M * H * sizeof(int32_t), stream));
    RS_HIP(ctx, hipMemsetAsync(t.models, 0, (size_t)M * D * H * sizeof(double), stream));
    RS_HIP(ctx, hipStreamSynchronize(stream));
    return RS_OK;
}

// the body of rs_*_hypotheses: the whole table to the host arrays that are not null
static inline int ransac_table_download(rs_context* ctx, const RansacEstimator* e, int S, int M, int D, int32_t* h_samples,
                                        int32_t* h_nmodels, double* h_models, int32_t* h_scores)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!e) return rs_fail(ctx, RS_ERR_INVALID, "null estimator");
    RS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t H = e->max_hyp;
    const RansacTable& t = e->t;
    if (h_samples) RS_HIP(ctx, hipMemcpyAsync(h_samples, t.samples, S * H * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (h_nmodels) RS_HIP(ctx, hipMemcpyAsync(h_nmodels, t.nmod, H * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (h_models) RS_HIP(ctx, hipMemcpyAsync(h_models, t.models, (size_t)M * D * H * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (h_scores) RS_HIP(ctx, hipMemcpyAsync(h_scores, t.scores, M * H * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    RS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RS_OK;
}

// rs_*_estimator_create: a new E with one block; own(e, carver) lays out what the stage adds (its state e->st included),
// the table follows it
template <class E>
static inline int ransac_create(rs_context* ctx, int max_points, int max_hypotheses, E** out, int S, int M, int D, const char* what,
                                void (*own)(E*, rs_carve&))
{
    if (!ctx || !out) return RS_ERR_INVALID;
    *out = nullptr;
    if (max_points < 1 || max_points > RANSAC_MAX_POINTS) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_points 1 .. %d", RANSAC_MAX_POINTS);
    if (max_hypotheses < 1 || max_hypotheses > RANSAC_MAX_HYP)
        return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_hypotheses 1 .. %d", RANSAC_MAX_HYP);
    RS_HIP(ctx, hipSetDevice(ctx->device));
    E* e = new E();
    e->ctx = ctx;
    e->max_points = max_points;
    e->max_hyp = max_hypotheses;
    const size_t H = max_hypotheses;
    int rc = e->block.carve(ctx, what, [&](rs_carve& c) {
        own(e, c);
        e->t.samples = c.take<int32_t>(S * H);
        e->t.nmod = c.take<int32_t>(H);
        e->t.models = c.take<double>((size_t)M * D * H);
        e->t.scores = c.take<int32_t>(M * H);
    });
    if (rc == RS_OK) rc = ransac_first_fill(ctx, e, H, S, M, D);
    if (rc != RS_OK) { delete e; return rc; }
    *out = e;
    return RS_OK;
}

// what every entry point checks: estimator, intrinsics, outputs, max_n, the two point arrays, K
static inline int ransac_check_call(rs_context* ctx, const RansacEstimator* e, const void* pts_a, const void* pts_b, int max_n,
                                    const float* K, const float* d_pose, const uint8_t* d_inlier, const int32_t* d_index,
                                    const int32_t* d_cnt, const int32_t* d_status)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!e || !K) return rs_fail(ctx, RS_ERR_INVALID, "null estimator / intrinsics");
    if (!d_pose || !d_inlier || !d_index || !d_cnt || !d_status) return rs_fail(ctx, RS_ERR_INVALID, "null output");
    if (max_n < 0) return rs_fail(ctx, RS_ERR_INVALID, "negative point count");
    if (max_n > e->max_points) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "points 0 .. %d (the estimator's max_points)", e->max_points);
    if (max_n > 0 && (!pts_a || !pts_b)) return rs_fail(ctx, RS_ERR_INVALID, "null points");
    if (!(K[0] > 0.f) || !(K[1] > 0.f) || !std::isfinite(K[2]) || !std::isfinite(K[3]))
        return rs_fail(ctx, RS_ERR_INVALID, "intrinsics fx, fy > 0, finite cx, cy");
    return RS_OK;
}

// what the two hashed RANSACs check on top of it
static inline int ransac_check_options(rs_context* ctx, const RansacEstimator* e, const int32_t* d_count, int max_hypotheses,
                                       double threshold_px, double confidence)
{
    if (!d_count) return rs_fail(ctx, RS_ERR_INVALID, "null count");
    if (max_hypotheses < 1 || max_hypotheses > e->max_hyp)
        return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_hypotheses 1 .. %d (the estimator's)", e->max_hyp);
    if (!(threshold_px > 0.0) || !(confidence > 0.0 && confidence < 1.0))
        return rs_fail(ctx, RS_ERR_INVALID, "threshold_px > 0, confidence in (0, 1)");
    return RS_OK;
}

// workgroups of 256 for a *_prep kernel: enough for the points and for the table, at most 64
static inline int ransac_blocks(int max_n, int max_hyp) { return std::max(1, std::min((std::max(max_n, max_hyp) + 255) / 256, 64)); }
