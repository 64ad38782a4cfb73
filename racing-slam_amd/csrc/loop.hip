// loop.hip — the "Loop verify" stage of LoopDetector::query (reference src/LoopDetector.cpp:501-506) against the resident
// map: verify_pnp (:176-229) of the query key frame against each ranked candidate, specified by tests/loop_ref.py.
//
// MapMatcher::match_descriptors (K1, hamming.hip) and cv::solvePnPRansac (pnp.hip) already run on the device; what
// verify_pnp does around them ran on the host: walk the candidate's map matches, gather their descriptor rows and point
// positions, upload, call twice, download, finish.  Here both key frames live in an rs_map, and per candidate
//   loop_gather    one workgroup per candidate, ONE launch for all: ordered compaction of the candidate's n pool rows whose
//                  keypoint has a map match (d_kp_point >= 0, ascending keypoint = Frame::map_matches() order) in chunks of
//                  the block size with rs_block_exclusive_scan -> train rows, point positions, keypoints, point slots and
//                  the count.  The host knows that count from the mirror (it sizes K1's launch); the kernel's own is checked
//                  against it after the call.  Bound by the latency of ceil(n / 256) dependent chunks of 40-byte reads.
//   K1             rs_match_descriptors, unchanged: all query rows x the gathered rows.
//   loop_gate      one thread: the count PnP reads is the match count, or 0 below MIN_PNP_CORRESPONDENCES (:183-186), which
//                  PnP answers with its own status 1 without drawing a hypothesis.
//   PnP            rs_estimate_pose_pnp, unchanged: the match lists are its index arrays.
//   loop_verdict   one workgroup per candidate, ONE launch for all: the status rule, the listed correspondences (query
//                  keypoint, point slot, candidate keypoint) written straight into the pinned result block, min / max of
//                  the listed query x by a fixed shuffle / LDS tree, and by one thread the f32 verdict of
//                  finish_verification (:146-174) without contraction.  Bound by launch latency and the host-memory writes.
// and ONE synchronisation at the end for all candidates.  The chains between gather and verdict run on a child context per
// candidate between a fork and a join ("loop_verify_streams" 0, the default) or on the context stream one after the other
// (1); they share no buffer, so both forms return the same bytes.  Two thirds of a PnP call is a one-workgroup kernel, so
// the chains overlap: 3 candidates of 1200 rows against 2000 query rows take 0.79 ms forked and 2.03 ms on one stream
// (tools/loop_time.py, profiles/loop_time.json).
#include "ransac.h"

#define LOOP_MAX_CANDIDATES 8
#define LOOP_MIN_CORRESPONDENCES 12         // MIN_PNP_CORRESPONDENCES
#define LOOP_MIN_INLIERS 20                 // MIN_PNP_INLIERS
#define LOOP_MIN_RATIO 0.35f                // MIN_PNP_INLIER_RATIO
#define LOOP_MIN_SPREAD 0.25f               // MIN_SPREAD_FRAC
#define LOOP_BLOCK 256

enum { LS_GATHERED = 0, LS_MATCHES, LS_GATED, LS_INLIERS, LS_PNP_STATUS, LS_WORDS = 8 };

struct LoopChain {                          // one candidate's buffers (device)
    uint8_t* rows;                          // [max_points][32] gathered train rows
    float* pos;                             // [max_points][3] their points' positions
    int32_t *kp, *slot;                     // [max_points] their keypoints in the candidate, their point slots
    int32_t *mq, *mt;                       // [max_points] K1's match lists
    int32_t* scal;                          // [LS_WORDS]
    float* pose;                            // [16] PnP's outputs
    uint8_t* inlier;                        // [max_points]
    int32_t* inlier_index;                  // [max_points]
};

struct LoopJob { int n, pool_row, kf, nt; };

struct LoopArgs {
    LoopChain c[LOOP_MAX_CANDIDATES];
    LoopJob j[LOOP_MAX_CANDIDATES];
};

struct LoopPinned {                         // what the verdict kernel writes into host memory
    rs_loop_result* result;                 // [max_candidates]
    int32_t* gathered;                      // [max_candidates]
    int32_t *query_kp, *point, *cand_kp;    // [max_candidates][max_points]
};

struct rs_loop_verifier {
    rs_context* ctx = nullptr;
    int max_points = 0, max_candidates = 0, max_hyp = 0;
    rs_dev_block slab;                      // every LoopChain buffer
    rs_pin_block pinned;                    // what `pin` points into
    LoopChain chain[LOOP_MAX_CANDIDATES];
    LoopPinned pin = {};
    rs_pnp_estimator* est[LOOP_MAX_CANDIDATES] = {};
    rs_context* child[LOOP_MAX_CANDIDATES] = {};
    hipStream_t child_stream[LOOP_MAX_CANDIDATES] = {};
    int last_n = 0, last_nq = 0;            // of the last call (rs_loop_verifier_download)
};

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(LOOP_BLOCK) void loop_gather(LoopArgs a, int max_points, const uint4* __restrict__ pool,
                                                          const int32_t* __restrict__ kp_point, const float* __restrict__ pos)
{
    const LoopJob j = a.j[blockIdx.x];
    const LoopChain c = a.c[blockIdx.x];
    int base = 0;
    for (int c0 = 0; c0 < j.n; c0 += LOOP_BLOCK) {
        const int i = c0 + (int)threadIdx.x;
        const int slot = i < j.n ? kp_point[(size_t)j.pool_row + i] : -1;
        const int f = slot >= 0 ? 1 : 0;
        int tot;
        const int o = base + rs_block_exclusive_scan(f, &tot);
        if (f && o < max_points) {
            const uint4* src = pool + 2 * ((size_t)j.pool_row + i);
            uint4* dst = (uint4*)c.rows + 2 * (size_t)o;
            dst[0] = src[0];
            dst[1] = src[1];
#pragma unroll
            for (int k = 0; k < 3; k++) c.pos[3 * (size_t)o + k] = pos[3 * (size_t)slot + k];
            c.kp[o] = i;
            c.slot[o] = slot;
        }
        base += tot;
    }
    if (threadIdx.x == 0) c.scal[LS_GATHERED] = base;
}

__global__ __launch_bounds__(64) void loop_gate(int32_t* __restrict__ scal)
{
    if (threadIdx.x == 0) {
        const int cnt = scal[LS_MATCHES];
        scal[LS_GATED] = cnt >= LOOP_MIN_CORRESPONDENCES ? cnt : 0;
    }
}

// Frame::camera_center = -R^T t in the operation order of map.hip's centre_of
__device__ __forceinline__ float loop_centre(const float* T, int i)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(-T[i], T[3]), __fmul_rn(-T[4 + i], T[7])), __fmul_rn(-T[8 + i], T[11]));
}

// |a - b| of two 3-vectors: the differences, (d0^2 + d1^2) + d2^2, the square root (Eigen's norm() of a fixed 3-vector)
__device__ __forceinline__ float loop_distance(const float* a, const float* b)
{
    const float d0 = __fsub_rn(a[0], b[0]), d1 = __fsub_rn(a[1], b[1]), d2 = __fsub_rn(a[2], b[2]);
    // sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS that intrinsic is the native (1 ulp) square root
    return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
}

__global__ __launch_bounds__(LOOP_BLOCK) void loop_verdict(LoopArgs a, int max_points, int n_query, int query_row, int query_kf, int width,
                                                           const float2* __restrict__ kp_pool, const float* __restrict__ centres,
                                                           LoopPinned out)
{
    __shared__ float s_min[LOOP_BLOCK / 64], s_max[LOOP_BLOCK / 64];
    const int cand = blockIdx.x;
    const LoopJob j = a.j[cand];
    const LoopChain c = a.c[cand];
    const int cnt = min(max(c.scal[LS_MATCHES], 0), n_query);
    const int pnp_status = c.scal[LS_PNP_STATUS];
    const int pin = min(max(c.scal[LS_INLIERS], 0), cnt);
    const int status = cnt < LOOP_MIN_CORRESPONDENCES ? 1 : ((pnp_status != 0 || pin == 0) ? 2 : 0);
    const int listed = status == 0 ? pin : cnt;
    float lo = INFINITY, hi = -INFINITY;
    const size_t row = (size_t)cand * max_points;
    for (int k = threadIdx.x; k < listed; k += LOOP_BLOCK) {
        const int m = status == 0 ? c.inlier_index[k] : k;
        const int q = c.mq[m], t = c.mt[m];
        // the row t came from keypoint kp[t] of the candidate, which IS the point's observation in that key frame
        // (kp_point and the observation list are one fact in rs_map): set_correspondences' search (:129-138) always finds it
        out.query_kp[row + k] = q;
        out.point[row + k] = c.slot[t];
        out.cand_kp[row + k] = c.kp[t];
        const float x = kp_pool[(size_t)query_row + q].x;
        lo = fminf(lo, x);
        hi = fmaxf(hi, x);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { s_min[threadIdx.x >> 6] = lo; s_max[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < LOOP_BLOCK / 64; w++) { lo = fminf(lo, s_min[w]); hi = fmaxf(hi, s_max[w]); }
    rs_loop_result r;
    r.status = status;
    r.correspondences = cnt;
    r.listed = listed;
    r.inliers = 0; r.ok = 0; r.spread = 0.f; r.drift = 0.f; r.gap = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) r.pose[k] = (k % 5 == 0) ? 1.f : 0.f;
    if (status == 0) {
        r.inliers = pin;
#pragma unroll
        for (int k = 0; k < 16; k++) r.pose[k] = c.pose[k];
        r.spread = (listed < 2 || width <= 0) ? 0.f : __fdiv_rn(__fsub_rn(hi, lo), (float)width);      // keypoint_spread, :146-158
        float rc[3];
#pragma unroll
        for (int k = 0; k < 3; k++) rc[k] = loop_centre(r.pose, k);
        r.drift = loop_distance(rc, centres + 3 * (size_t)query_kf);                                     // :166
        r.gap = loop_distance(rc, centres + 3 * (size_t)j.kf);                                           // :167
        const float ratio = cnt == 0 ? 0.f : __fdiv_rn((float)pin, (float)cnt);                          // :169-171
        r.ok = (pin >= LOOP_MIN_INLIERS && ratio >= LOOP_MIN_RATIO && r.spread >= LOOP_MIN_SPREAD) ? 1 : 0;
    }
    out.result[cand] = r;
    out.gathered[cand] = c.scal[LS_GATHERED];
}

// ------------------------------------------------------------------------------------------------ C-ABI
// The child contexts of the forked form, the default: own stream, own K1 table sized for max_points.  Created with the
// verifier, so that no call allocates.
static int loop_children(rs_loop_verifier* v, int n)
{
    rs_context* ctx = v->ctx;
    for (int c = 0; c < n; c++) {
        if (v->child[c]) continue;
        rs_context* k = nullptr;
        int rc = rs_context_create(ctx->device, &k);
        if (rc) return rs_fail(ctx, rc, "cannot create a child context");
        if (hipStreamCreateWithFlags(&v->child_stream[c], hipStreamNonBlocking) != hipSuccess) {
            rs_context_destroy(k);
            v->child_stream[c] = nullptr;
            return rs_fail(ctx, RS_ERR_HIP, "hipStreamCreate");
        }
        k->stream = v->child_stream[c];
        v->child[c] = k;
        if ((rc = rs_k1_reserve(k, (size_t)v->max_points)) || hipStreamSynchronize(k->stream) != hipSuccess)
            return rs_fail(ctx, rc ? rc : RS_ERR_HIP, "child context %d: %s", c, rs_last_error(k));
    }
    return RS_OK;
}

extern "C" int rs_loop_verifier_destroy(rs_loop_verifier* v)
{
    if (!v) return RS_OK;
    (void)hipSetDevice(v->ctx->device);
    (void)hipStreamSynchronize(v->ctx->stream);
    for (int c = 0; c < LOOP_MAX_CANDIDATES; c++) {
        if (v->child[c]) { (void)hipStreamSynchronize(v->child[c]->stream); }
        if (v->est[c]) rs_pnp_estimator_destroy(v->est[c]);
        if (v->child[c]) rs_context_destroy(v->child[c]);
        if (v->child_stream[c]) (void)hipStreamDestroy(v->child_stream[c]);
    }
    delete v;
    return RS_OK;
}

extern "C" int rs_loop_verifier_create(rs_context* ctx, int max_points, int max_candidates, int max_hypotheses, rs_loop_verifier** out)
{
    if (!ctx || !out) return RS_ERR_INVALID;
    *out = nullptr;
    if (max_points < 1 || max_points > RANSAC_MAX_POINTS) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_points 1 .. %d", RANSAC_MAX_POINTS);
    if (max_candidates < 1 || max_candidates > LOOP_MAX_CANDIDATES)
        return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_candidates 1 .. %d", LOOP_MAX_CANDIDATES);
    if (max_hypotheses < 1 || max_hypotheses > RANSAC_MAX_HYP) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_hypotheses 1 .. %d", RANSAC_MAX_HYP);
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_loop_verifier* v = new rs_loop_verifier();
    v->ctx = ctx;
    v->max_points = max_points;
    v->max_candidates = max_candidates;
    v->max_hyp = max_hypotheses;
    const size_t m = (size_t)max_points, C = (size_t)max_candidates;
    int rc = v->slab.carve(ctx, "loop verifier scratch", [&](rs_carve& s) {
        for (size_t c = 0; c < C; c++) {
            LoopChain& k = v->chain[c];
            k.rows = s.take<uint8_t>(32 * m);
            k.pos = s.take<float>(3 * m);
            k.kp = s.take<int32_t>(m);
            k.slot = s.take<int32_t>(m);
            k.mq = s.take<int32_t>(m);
            k.mt = s.take<int32_t>(m);
            k.inlier_index = s.take<int32_t>(m);
            k.scal = s.take<int32_t>(LS_WORDS);
            k.pose = s.take<float>(16);
            k.inlier = s.take<uint8_t>(m);
        }
    });
    if (!rc)
        rc = v->pinned.carve(ctx, "loop verifier results", [&](rs_carve& p) {
            v->pin.result = p.take<rs_loop_result>(C);
            v->pin.gathered = p.take<int32_t>(C);
            v->pin.query_kp = p.take<int32_t>(C * m);
            v->pin.point = p.take<int32_t>(C * m);
            v->pin.cand_kp = p.take<int32_t>(C * m);
        });
    if (!rc && hipMemsetAsync(v->slab.p, 0, v->slab.bytes, ctx->stream) != hipSuccess) rc = rs_fail(ctx, RS_ERR_HIP, "hipMemsetAsync");
    if (!rc) memset(v->pinned.p, 0, v->pinned.bytes);
    for (size_t c = 0; c < C && !rc; c++) rc = rs_pnp_estimator_create(ctx, max_points, max_hypotheses, &v->est[c]);
    if (!rc) rc = loop_children(v, max_candidates);
    if (!rc) rc = rs_k1_reserve(ctx, m);
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = rs_fail(ctx, RS_ERR_HIP, "hipStreamSynchronize");
    if (rc) { rs_loop_verifier_destroy(v); return rc; }
    *out = v;
    return RS_OK;
}

extern "C" int rs_map_verify_loop(rs_context* ctx, rs_loop_verifier* v, rs_map* map, int query_kf, const int32_t* h_candidate_kfs,
                                  int n_candidates, const float* h_intrinsics, int width, int max_distance, double threshold_px,
                                  double confidence, int max_hypotheses, uint64_t seed, rs_loop_result* h_result,
                                  int32_t* h_listed_query_kp, int32_t* h_listed_point, int32_t* h_listed_candidate_kp)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!v || !map || v->ctx != ctx || rs_map_context(map) != ctx) return rs_fail(ctx, RS_ERR_INVALID, "null verifier / map, or of another context");
    if (n_candidates < 0 || n_candidates > v->max_candidates)
        return rs_fail(ctx, RS_ERR_INVALID, "candidates 0 .. %d (the verifier's max_candidates)", v->max_candidates);
    if (n_candidates == 0) return RS_OK;
    if (!h_candidate_kfs || !h_result || !h_intrinsics) return rs_fail(ctx, RS_ERR_INVALID, "null candidates / result / intrinsics");
    const float* K = h_intrinsics;
    if (!(K[0] > 0.f) || !(K[1] > 0.f) || !std::isfinite(K[2]) || !std::isfinite(K[3]))
        return rs_fail(ctx, RS_ERR_INVALID, "intrinsics fx, fy > 0, finite cx, cy");
    if (!(threshold_px > 0.0) || !(confidence > 0.0 && confidence < 1.0)) return rs_fail(ctx, RS_ERR_INVALID, "threshold_px > 0, confidence in (0, 1)");
    if (max_hypotheses < 1 || max_hypotheses > v->max_hyp) return rs_fail(ctx, RS_ERR_UNSUPPORTED, "max_hypotheses 1 .. %d (the verifier's)", v->max_hyp);
    int nq = 0, qrow = 0, qm = 0;
    if (!rs_map_loop_keyframe(map, query_kf, &nq, &qrow, &qm)) return rs_fail(ctx, RS_ERR_INVALID, "unknown query key frame %d", query_kf);
    if (nq > v->max_points) return rs_fail(ctx, RS_ERR_INVALID, "query key frame of %d keypoints (the verifier's max_points is %d)", nq, v->max_points);
    const bool forked = ctx->loop_verify_streams == 0;
    int rc = RS_OK;
    LoopArgs a;
    for (int c = 0; c < n_candidates; c++) {
        LoopJob& j = a.j[c];
        j.kf = h_candidate_kfs[c];
        if (j.kf == query_kf) return rs_fail(ctx, RS_ERR_INVALID, "candidate %d is the query key frame", c);
        if (!rs_map_loop_keyframe(map, j.kf, &j.n, &j.pool_row, &j.nt)) return rs_fail(ctx, RS_ERR_INVALID, "unknown candidate key frame %d", j.kf);
        if (j.n > v->max_points) return rs_fail(ctx, RS_ERR_INVALID, "candidate key frame of %d keypoints (the verifier's max_points is %d)", j.n, v->max_points);
        a.c[c] = v->chain[c];
    }
    for (int c = n_candidates; c < LOOP_MAX_CANDIDATES; c++) { a.c[c] = v->chain[0]; a.j[c] = LoopJob{0, 0, 0, 0}; }
    RS_HIP(ctx, hipSetDevice(ctx->device));
    rs_map_loop_view mv;
    if ((rc = rs_map_loop_sync(map, &mv))) return rc;
    hipStream_t s = ctx->stream;
    {
        rs_prof_scope ps(ctx, "LOOP0_gather");
        hipLaunchKernelGGL(loop_gather, dim3(n_candidates), dim3(LOOP_BLOCK), 0, s, a, v->max_points, (const uint4*)mv.d_pool, mv.d_kp_point, mv.d_pos);
    }
    if (forked && (rc = rs_context_fork(ctx, v->child, n_candidates))) return rc;
    const uint8_t* d_query = mv.d_pool + 32 * (size_t)qrow;
    const float* d_pixels = mv.d_kp_pool + 2 * (size_t)qrow;
    int first_rc = RS_OK;
    for (int c = 0; c < n_candidates; c++) {
        rs_context* cc = forked ? v->child[c] : ctx;
        const LoopChain& k = v->chain[c];
        int r = rs_match_descriptors(cc, d_query, nq, k.rows, a.j[c].nt, 1, max_distance, k.mq, k.mt, k.scal + LS_MATCHES, nullptr, nullptr,
                                     nullptr, nullptr);
        if (!r) {
            hipLaunchKernelGGL(loop_gate, dim3(1), dim3(64), 0, cc->stream, k.scal);
            r = rs_estimate_pose_pnp(cc, v->est[c], k.pos, k.mt, d_pixels, k.mq, k.scal + LS_GATED, nq > 0 ? nq : 1, h_intrinsics, threshold_px,
                                     confidence, max_hypotheses, seed, k.pose, k.inlier, k.inlier_index, k.scal + LS_INLIERS,
                                     k.scal + LS_PNP_STATUS);
        }
        if (r && !first_rc) first_rc = forked ? rs_fail(ctx, r, "candidate %d: %s", c, rs_last_error(cc)) : r;
    }
    if (forked) {
        const int wrc = rs_context_wait_for(ctx, v->child, n_candidates);       // joined whatever the chains' status
        if (wrc && !first_rc) first_rc = wrc;
    }
    if (first_rc) { (void)hipStreamSynchronize(s); return first_rc; }
    {
        rs_prof_scope ps(ctx, "LOOP1_verdict");
        hipLaunchKernelGGL(loop_verdict, dim3(n_candidates), dim3(LOOP_BLOCK), 0, s, a, v->max_points, nq, qrow, query_kf, width,
                           (const float2*)mv.d_kp_pool, mv.d_centres, v->pin);
    }
    RS_HIP(ctx, hipGetLastError());
    RS_HIP(ctx, hipStreamSynchronize(s));
    v->last_n = n_candidates;
    v->last_nq = nq;
    const size_t m = (size_t)v->max_points;
    for (int c = 0; c < n_candidates; c++) {
        if (v->pin.gathered[c] != a.j[c].nt)
            return rs_fail(ctx, RS_ERR_INTERNAL, "candidate %d: the device gathered %d rows, the mirror has %d", c, v->pin.gathered[c], a.j[c].nt);
        h_result[c] = v->pin.result[c];
        const size_t n = (size_t)h_result[c].listed, o = m * (size_t)c;
        if (h_listed_query_kp) memcpy(h_listed_query_kp + o, v->pin.query_kp + o, 4 * n);
        if (h_listed_point) memcpy(h_listed_point + o, v->pin.point + o, 4 * n);
        if (h_listed_candidate_kp) memcpy(h_listed_candidate_kp + o, v->pin.cand_kp + o, 4 * n);
    }
    return RS_OK;
}

extern "C" int rs_loop_verifier_download(rs_context* ctx, const rs_loop_verifier* v, int candidate, int32_t* h_nt, uint8_t* h_rows,
                                         int32_t* h_slots, int32_t* h_keypoints, float* h_positions, int32_t* h_match_query,
                                         int32_t* h_match_train, int32_t* h_match_count, int32_t* h_inlier_index, int32_t* h_inlier_count)
{
    if (!ctx) return RS_ERR_INVALID;
    if (!v || v->ctx != ctx) return rs_fail(ctx, RS_ERR_INVALID, "null verifier, or of another context");
    if (candidate < 0 || candidate >= v->last_n) return rs_fail(ctx, RS_ERR_INVALID, "candidate %d of the last call's %d", candidate, v->last_n);
    RS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const LoopChain& k = v->chain[candidate];
    int32_t scal[LS_WORDS];
    RS_HIP(ctx, hipMemcpyAsync(scal, k.scal, sizeof scal, hipMemcpyDeviceToHost, s));
    RS_HIP(ctx, hipStreamSynchronize(s));
    const size_t nt = (size_t)std::min(std::max(scal[LS_GATHERED], 0), v->max_points);
    const size_t cnt = (size_t)std::min(std::max(scal[LS_MATCHES], 0), v->last_nq);
    // below the gate PnP was told of no correspondences: its status 1, no inliers
    const size_t inl = (size_t)std::min(std::max(scal[LS_INLIERS], 0), (int)cnt);
    if (h_nt) *h_nt = (int32_t)nt;
    if (h_match_count) *h_match_count = (int32_t)cnt;
    if (h_inlier_count) *h_inlier_count = (int32_t)inl;
    if (h_rows && nt) RS_HIP(ctx, hipMemcpyAsync(h_rows, k.rows, 32 * nt, hipMemcpyDeviceToHost, s));
    if (h_slots && nt) RS_HIP(ctx, hipMemcpyAsync(h_slots, k.slot, 4 * nt, hipMemcpyDeviceToHost, s));
    if (h_keypoints && nt) RS_HIP(ctx, hipMemcpyAsync(h_keypoints, k.kp, 4 * nt, hipMemcpyDeviceToHost, s));
    if (h_positions && nt) RS_HIP(ctx, hipMemcpyAsync(h_positions, k.pos, 12 * nt, hipMemcpyDeviceToHost, s));
    if (h_match_query && cnt) RS_HIP(ctx, hipMemcpyAsync(h_match_query, k.mq, 4 * cnt, hipMemcpyDeviceToHost, s));
    if (h_match_train && cnt) RS_HIP(ctx, hipMemcpyAsync(h_match_train, k.mt, 4 * cnt, hipMemcpyDeviceToHost, s));
    if (h_inlier_index && inl) RS_HIP(ctx, hipMemcpyAsync(h_inlier_index, k.inlier_index, 4 * inl, hipMemcpyDeviceToHost, s));
    RS_HIP(ctx, hipStreamSynchronize(s));
    return RS_OK;
}
