/*
 * rsgpu.h — C-ABI of librsgpu.so: the MI355X (gfx950) implementation of the
 * Racing-SLAM per-frame hot path (descriptor matching -> triangulation ->
 * local-window bundle adjustment).
 *
 * This header is the whole drop-in boundary.  The reference has no FFI layer
 * (SURVEY.md §8b): its boundary is link-time, four translation units
 *   src/MapMatcher.cpp, src/Triangulation.cpp, src/Optimization.cpp,
 *   src/LocalWindow.cpp
 * behind four headers.  A maintainer replaces those four .cpp files with the
 * shims shown in INTEGRATION.md; every shim function flattens the reference's
 * pointer graph (Frame / MapPoint / Map) to the SoA arrays below and calls one
 * entry point of this header.  Each entry point cites the reference code it
 * replaces.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only; no exceptions cross the ABI.
 *  - Every function returns an rs_status (0 = RS_OK).  rs_last_error() returns
 *    a human-readable message for the last failure on that context.
 *  - Pointers named d_* are DEVICE pointers (HBM of the context's GPU).
 *    Pointers named h_* are HOST pointers.  Small fixed-size parameters
 *    (poses, intrinsics, options) are host memory and are copied by value.
 *  - All work is enqueued on the context's stream (rs_context_set_stream);
 *    functions that return results in host memory synchronise that stream.
 *  - Matrices are ROW-MAJOR unless stated (Eigen's default is column-major:
 *    the shim transposes 16 floats).  A pose is the 4x4 world->camera
 *    transform exactly as Frame::pose() (src/Frame.h:46).
 *  - Descriptors are 32-byte rows (256-bit ORB, src/features/OrbFeatureExtractor.h:14-22),
 *    row i at byte offset 32*i; device descriptor arrays must be 16-byte aligned.
 *    The *_f32 / *_l2 entry points alone take FLOAT descriptors instead (rows of `dim` f32 under the L2 norm); the
 *    resident map (rs_frame, rs_map), bag-of-words and the track store are ORB-only.
 *  - One context per GPU / per process rank; a context is not re-entrant
 *    (the reference's callers are single threaded, SURVEY.md §8b "Threading").
 */
#ifndef RSGPU_H
#define RSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSGPU_ABI_VERSION 3
#define RS_DESC_BYTES 32

typedef enum rs_status {
    RS_OK = 0,
    RS_ERR_INVALID = 1,     /* bad argument (null pointer, negative size, unsorted CSR ...) */
    RS_ERR_HIP = 2,         /* a HIP runtime call failed; see rs_last_error */
    RS_ERR_NOMEM = 3,       /* workspace allocation failed */
    RS_ERR_UNSUPPORTED = 4, /* valid request outside the implemented envelope */
    RS_ERR_RCCL = 5,        /* RCCL missing or a collective failed */
    RS_ERR_NO_DEVICE = 6,   /* no gfx950 device visible: there is NO CPU fallback */
    RS_ERR_INTERNAL = 7     /* a result of the device contradicts the host mirror; see rs_last_error */
} rs_status;

typedef struct rs_context rs_context;

/* ------------------------------------------------------------------ context */

int rs_abi_version(void);

/* Creates a context bound to HIP device `device_id`.  Fails with
 * RS_ERR_NO_DEVICE when no GPU is visible: the product path never falls back
 * to the CPU. */
int rs_context_create(int device_id, rs_context** out_ctx);
int rs_context_destroy(rs_context* ctx);
/* `hip_stream` is a hipStream_t (NULL = the legacy default stream). */
int rs_context_set_stream(rs_context* ctx, void* hip_stream);
int rs_context_synchronize(rs_context* ctx);
/* Stream ordering between contexts of one process, without the host: everything enqueued on `ctx` after this call
 * waits for everything enqueued so far on each of `others[0 .. n)` (one event record + one stream wait per context).
 * For hosts that run independent calls side by side — the reference's match_map, match_key_frame,
 * triangulate_tracks and match_descriptors -> triangulate_points chains share no data — on contexts of their own and
 * join them before the call that needs all their results (bench.py's pass does). */
int rs_context_wait_for(rs_context* ctx, rs_context* const* others, int n);
/* The other direction with ONE event: everything enqueued on each of `others` after this call waits for everything
 * enqueued so far on `ctx` (the fork in front of side-by-side chains). */
int rs_context_fork(rs_context* ctx, rs_context* const* others, int n);
/* Tuning knobs (integers by name).  "ba_speculative_sets": at most 1 .. 5 trust-region radii evaluated per round of
 * rs_bundle_adjust on the local-window path (0 = library default: 5; inertial solves and batches of windows: 3).  A round
 * evaluates one radius where a step is most likely accepted (first round, after two accepted steps in a row), all of them
 * while the trust region is uncalibrated (no rejection streak resolved by an accepted step yet, or the last round rejected
 * to its last set), three once it is, and never more than the iterations left.  The LM schedule, iteration count and results
 * do not depend on any of this (tests/test_gpu_parity.py), only the number of launches does.  "ba_fuse_mode" 3 needs <= 3.
 * "ba_imu_mode": rs_bundle_adjust_inertial — 0 (default) the velocity / bias blocks are eliminated around the
 * local-window reduced solve where the window allows it, 1 always the blocked solve of the full camera-side system.
 * "ba_fuse_mode": rs_bundle_adjust on a single local window (vision only, one rank) — the reduced solve and the
 * back-substitution / candidate cost of a round as ONE launch (the latter's workgroups wait for the former's hand-off
 * words inside the launch, holding a CU each): 0 (default) when no other solve of this process is in flight (lower
 * latency for one session; several sessions on one GPU get more aggregate throughput from two launches), 1 never,
 * 2 wherever possible, 3 the WHOLE round — linearisation, reduced solve, back-substitution — as one launch wherever the
 * window allows it (every workgroup resident at once: one item of landmarks per compute unit); same results.
 * "ba_band_mode": windows beyond the local-window kernels (more than 21 optimised cameras) — 0 (default) when no landmark is
 * seen by key frames more than 9 slots apart the reduced camera matrix is block-banded and is factorised by ONE launch
 * (the sparsity the reference's SPARSE_SCHUR solve exploits, src/Optimization.cpp:360): two workgroups eliminate from
 * both ends of the band towards a separator block, which a launch of its own factors; 1 always the general
 * blocked factorisation (two launches per 48 columns); 2 the banded factorisation by one workgroup from one end; same
 * results to rounding.
 * "ba_item_landmarks": landmarks per workgroup of the linearisation / Schur kernel of a single solve — 0 (default) 40
 * for windows of at most 10240 landmarks (one workgroup per compute unit), 64 beyond; or 32 / 40 / 48 / 56 / 64.
 * "ba_handoff_timeout_us": how long (1 .. 1000000, default 4000) a workgroup of that fused launch waits for a hand-off
 * word before it gives up; a solve in which that happened is re-run once as separate launches from its untouched
 * inputs (rs_ba_get_stats [4] counts them) — the caller sees the same result either way.
 * "k2_mode": rs_reproj_match — 0 (default) eight lanes per map point where the frame has a usable cell grid
 * (rs_kdtree_grid_build) or its KD-tree fits in LDS (<= 6144 keypoints), 1 always one lane per point walking the tree;
 * the outputs are identical.
 * "k2_grid": rs_reproj_match under k2_mode 0 — 1 (default) search the frame's cell grid where it has a usable one,
 * 0 always walk the KD-tree; the outputs are identical.
 * "ba_batch_mode": how rs_bundle_adjust_batch runs its windows — 0 (default) one launch sequence for all of them
 * where the windows allow it, 1 always the lanes.
 * "gftt_round_launches": rs_detect_features — how many launches of the parallel minimum-distance round (0 .. 12,
 * default 12) run before the single-workgroup finisher decides what they left undecided; 0 leaves every decision to
 * the finisher.  The detected corners do not depend on it, only the launches and rs_detector_stats' round counts do.
 * "bow_score_mode": rs_bow_database_score — 0 (default) the query's values are found through the rs_bow's dense
 * word table, 1 by binary search in its sorted words; the scores are identical.
 * "loop_verify_streams": rs_map_verify_loop — 0 (default) each candidate's chain runs on a child context of its own
 * between a fork and a join, 1 the chains follow one another on the context stream; the results are identical. */
int rs_context_set_int(rs_context* ctx, const char* name, int value);
const char* rs_last_error(const rs_context* ctx);

/* ------------------------------------------------------------ staging pool */

/* What a drop-in translation unit does around every entry point below: upload a few freshly flattened host arrays,
 * get device scratch for the outputs, read some results back.  The pool is two grow-only bump allocators (device and
 * pinned host memory) per context; copies are asynchronous on the context stream.  Typical shim body:
 *     rs_stage_begin(ctx);                                    // recycles the pool (waits for copies still in flight)
 *     rs_stage_upload(ctx, h_desc, bytes, (void**)&d_desc);   // host -> pinned -> device, async
 *     rs_stage_alloc(ctx, out_bytes, (void**)&d_out);         // device scratch
 *     rs_xxx(ctx, d_desc, ..., d_out);                        // kernels, same stream
 *     rs_stage_download(ctx, d_out, out_bytes, h_out);        // device -> pinned, async
 *     rs_stage_sync(ctx);                                     // one synchronisation; h_out is filled on return
 * Device pointers obtained from the pool are valid until the next rs_stage_begin on the context. */
int rs_stage_begin(rs_context* ctx);
int rs_stage_alloc(rs_context* ctx, size_t bytes, void** d_out);
int rs_stage_upload(rs_context* ctx, const void* h_src, size_t bytes, void** d_out);
int rs_stage_download(rs_context* ctx, const void* d_src, size_t bytes, void* h_dst);
int rs_stage_sync(rs_context* ctx);

/* --------------------------------------------------- a4: match_descriptors */

/* Brute-force 2-nearest-neighbour search under 256-bit Hamming distance.
 * Replaces cv::BFMatcher(NORM_HAMMING).knnMatch(query, train, knn, 2) at
 * src/MapMatcher.cpp:147-148.
 *
 * d_query [batch][nq][32] u8, d_train [batch][nt][32] u8.
 * Outputs, each [batch][nq] int32:
 *   d_idx0/d_dist0 = nearest train row and its distance,
 *   d_idx1/d_dist1 = second nearest (idx1 = -1, dist1 = -1 when nt == 1).
 * Ties: the lower train index is the nearer neighbour (OpenCV batchDistance
 * inserts with strict compares).  Bit-exact integer results.
 * nq == 0 or nt == 0 is valid: nothing is written.  nt must be below 2^20 (the train index is
 * packed into 20 bits): nt >= 2^20 returns RS_ERR_UNSUPPORTED and leaves the context usable.  nq, batch: any. */
int rs_hamming_knn2(rs_context* ctx,
                    const uint8_t* d_query, int nq,
                    const uint8_t* d_train, int nt, int batch,
                    int32_t* d_idx0, int32_t* d_dist0,
                    int32_t* d_idx1, int32_t* d_dist1);

/* knnMatch + the two filters of MapMatcher::match_descriptors
 * (src/MapMatcher.cpp:150-161): keep query q iff
 *   dist0 <= max_distance                       (:152, note '>' rejects)
 *   and (nt < 2 or 4*dist0 <= 3*dist1)          (:156, MATCH_RATIO 0.75 :18)
 * Accepted matches are emitted in ascending query order (the order knn is
 * iterated in), compacted per batch item:
 *   d_match_query [batch][nq], d_match_train [batch][nq], d_match_count [batch].
 * Entries past d_match_count[b] are unspecified.
 * Any of d_idx0..d_dist1 may be NULL when the raw kNN result is not wanted. */
int rs_match_descriptors(rs_context* ctx,
                         const uint8_t* d_query, int nq,
                         const uint8_t* d_train, int nt, int batch,
                         int max_distance,
                         int32_t* d_match_query, int32_t* d_match_train,
                         int32_t* d_match_count,
                         int32_t* d_idx0, int32_t* d_dist0,
                         int32_t* d_idx1, int32_t* d_dist1);

/* The same two calls for FLOAT descriptors under the L2 norm (MapMatcher constructed with cv::NORM_L2 and a float
 * max_descriptor_distance, src/Tracker.cpp:42).  d_query [batch][nq][dim] f32, d_train [batch][nt][dim] f32, row-major,
 * 16-byte aligned, dim % 4 == 0 and 4 <= dim <= 1024 (any other dim: RS_ERR_UNSUPPORTED, the context stays usable).
 * The specification is this library's own (agreement with cv::BFMatcher's rounding is not claimed); all arithmetic is f32:
 *   s    = 0; for k ascending: s = fmaf(q[k], t[k], s)       (what a chain of f32 MFMA steps on one accumulator computes)
 *   nq2, nt2 = the same chain of a row with itself
 *   d2   = fmaxf(fmaf(-2.0f, s, nq2 + nt2), 0.0f),  dist = sqrtf(d2) correctly rounded
 * Candidates are ordered by (d2, train index): the lower train index wins a tie.  Results are bit-exact against that
 * restatement (tests/match_l2_ref.py) and reproducible from run to run; d2 lies within
 * gamma (sum q^2 + sum t^2 + 2 sum |q t|), gamma = (dim + 2) u / (1 - (dim + 2) u), u = 2^-24, of the exact value.
 * The contract covers finite inputs; non-finite values do not fault.
 *   d_idx0 / d_idx1 [batch][nq] int32, d_dist0 / d_dist1 [batch][nq] f32; idx1 = -1, dist1 = -1.0f when nt == 1.
 * (fmaxf turns a NaN d2 into 0, here and in the restatement alike: a pair with non-finite rows is outside the contract.)
 * nq == 0 or nt == 0 is valid: nothing is written (rs_match_descriptors_f32: the counts are zeroed).  nq and nt may be
 * up to 2^31 - 129 (row numbers are rounded up to whole 128-row passes in int); beyond: RS_ERR_UNSUPPORTED. */
int rs_l2_knn2(rs_context* ctx,
               const float* d_query, int nq,
               const float* d_train, int nt, int dim, int batch,
               int32_t* d_idx0, float* d_dist0,
               int32_t* d_idx1, float* d_dist1);

/* rs_l2_knn2 + the filters of src/MapMatcher.cpp:150-161 on dist: keep query q iff
 *   dist0 <= max_distance  and  (nt < 2 or dist0 <= 0.75f * dist1)      (one f32 product; a NaN max_distance fails both)
 * Outputs as rs_match_descriptors: ascending query order, compacted per batch item; any of d_idx0..d_dist1 may be NULL. */
int rs_match_descriptors_f32(rs_context* ctx,
                             const float* d_query, int nq,
                             const float* d_train, int nt, int dim, int batch,
                             float max_distance,
                             int32_t* d_match_query, int32_t* d_match_train,
                             int32_t* d_match_count,
                             int32_t* d_idx0, float* d_dist0,
                             int32_t* d_idx1, float* d_dist1);

/* ------------------------------------------- a2/a3: reprojection-gated match */

/* KD-tree over a frame's keypoints, flattened.  Mirrors KDTree2D
 * (src/KDTree.cpp:8-43): median split on x at even depth, y at odd depth,
 * mid = (start+end)/2.  Node i of the arrays is a tree node; root is node
 * `root`.  rs_kdtree_build (host) fills the three arrays (each [n]).
 * Equal-coordinate ties are resolved by (coordinate, keypoint index): the
 * reference leaves that to std::nth_element (unspecified). */
int rs_kdtree_build(const float* h_keypoints /*[n][2]*/, int n,
                    int32_t* h_node_kp /*[n] keypoint index of node*/,
                    int32_t* h_node_left /*[n] child node or -1*/,
                    int32_t* h_node_right /*[n]*/,
                    int32_t* h_root /*[1]*/);

typedef struct rs_frame_view {
    float pose[16];          /* world->camera, row-major (Frame::pose, src/Frame.h:46) */
    float fx, fy, cx, cy;    /* Camera intrinsics (src/Camera.cpp:5-13) */
    int width, height;       /* Camera::is_in_image bounds (src/Camera.cpp:34-37) */
    int n_keypoints;
    const float* d_keypoints;      /* [n][2] pixel coordinates */
    const uint8_t* d_descriptors;  /* [n][32] */
    const uint8_t* d_kp_matched;   /* [n] Frame::is_matched(index) (src/Frame.cpp:143-146) */
    const int32_t* d_kd_node_kp;   /* [n] from rs_kdtree_build */
    const int32_t* d_kd_left;      /* [n] */
    const int32_t* d_kd_right;     /* [n] */
    int kd_root;
    const void* d_kd_packed;       /* optional (NULL = not provided): the tree packed by rs_kdtree_pack for this frame,
                                      20 * n bytes, 16-byte aligned.  A frame is matched at least twice
                                      (src/Tracker.cpp:232-248): packing once saves every workgroup of both calls the
                                      dependent gathers node -> keypoint -> coordinates */
    const void* d_kd_grid;         /* optional (NULL = none; a zero-initialised view has none): the frame's keypoints in a
                                      cell grid, built by rs_kdtree_grid_build in this process for this frame */
} rs_frame_view;

/* Packs the flattened KD-tree of `frame` (its d_keypoints, d_kd_* arrays) into d_packed [n] x 20 bytes for
 * rs_frame_view::d_kd_packed. */
int rs_kdtree_pack(rs_context* ctx, const rs_frame_view* frame, void* d_packed);

/* The frame's keypoints in a uniform grid of 40-pixel cells over width x height, for rs_frame_view::d_kd_grid: with it
 * rs_reproj_match finds a point's keypoints within its 20-pixel radius in the cells the disc touches instead of walking
 * the KD-tree, and decides ties between equally distant keypoints by the order in which the reference's recursion would
 * have met them, computed from their node ids.  The outputs are identical.  Built once per frame from d_kd_packed
 * (required) and kd_root; the keypoint positions must not change afterwards, d_kp_matched may (it is read by every
 * call).  d_grid: rs_kdtree_grid_bytes(n_keypoints, width, height) bytes, 16-byte aligned; the arrangement is a pure
 * function of the input.  The build also decides whether the grid may stand in for the walk: only if the tree has the
 * shape rs_kdtree_build gives it (root n / 2, children the mids of the two half ranges), every node lies on the correct
 * side of each of its ancestors, and every coordinate is finite.  Otherwise (or above 65536 keypoints) the call still
 * succeeds and rs_reproj_match keeps walking the tree for this frame.  The library remembers the verdict per process, for
 * every context (a view may be matched on forked child contexts), so the call waits for the build (once per frame); a
 * pointer it has not built a usable grid at is ignored.  Rebuild, or build an empty frame, at d_grid before its memory
 * is reused for something else.
 * "k2_grid" (rs_context_set_int): 1 (default) use a frame's grid under k2_mode 0, 0 never. */
size_t rs_kdtree_grid_bytes(int n_keypoints, int width, int height);
int rs_kdtree_grid_build(rs_context* ctx, const rs_frame_view* frame, void* d_grid);

typedef struct rs_map_view {
    int n_points;                  /* candidate points, in MAP ORDER (src/Map.h:66) */
    const float* d_positions;      /* [P][3] MapPoint::position */
    const uint8_t* d_eligible;     /* [P] 1 = run the point.  The shim clears it for
                                      points the frame already matches (src/MapMatcher.cpp:53)
                                      and points not seen by required_observer (:169);
                                      match_for_fuse skips nulls the same way (:121-123). */
    const int32_t* d_obs_ptr;      /* [P+1] CSR: observations of point p are
                                      d_obs_ptr[p] .. d_obs_ptr[p+1]-1, in the order
                                      MapPoint::observations() is iterated */
    const int32_t* d_obs_kf;       /* [M] observing keyframe (index into d_kf_centers) */
    const int32_t* d_obs_desc;     /* [M] row of that observation's descriptor in d_desc_pool */
    const float* d_kf_centers;     /* [KF][3] Frame::camera_center (src/Frame.cpp:39-42) */
    const uint8_t* d_desc_pool;    /* [rows][32] descriptors of all keyframes */
} rs_map_view;

/* MapMatcher::match / match_for_fuse (src/MapMatcher.cpp:45-98,117-127,165-175).
 * For every eligible point: project, in-image, viewing-angle (>= 0.5) and
 * distance-range gates in f32, KD radius search r = 20 px in the reference's
 * traversal order, min Hamming over (candidate keypoint x observation) with a
 * strict '<' starting from max_distance, then per-keypoint strict-'<' argmin
 * over points in map order.
 *   replace = 0: match_map / match_key_frame (already-matched keypoints skipped)
 *   replace = 1: match_for_fuse
 * Outputs:
 *   d_point_kp   [P] best keypoint for the point or -1;  d_point_dist [P] (max_distance if none)
 *   d_prop_point [N] winning point (map order index) per keypoint or -1; d_prop_dist [N]
 *   d_match_kp / d_match_point [N] + d_match_count[1]: accepted_matches()
 *   (src/MapMatcher.cpp:34-43), ascending keypoint index.
 * Integer outputs are bit-exact against the oracle; the f32 gates follow the
 * operation order documented in oracle/reproj_match.c.
 * Up to 6144 keypoints (K2_MAX_LDS_NODES) K2 stages the frame's KD-tree in LDS; beyond that it walks the tree in
 * global memory (one lane per point, whatever k2_mode says): same outputs, any n_keypoints below 2^30.
 * max_distance may be any int; a point proposes only at a distance strictly below it, so <= 0 proposes nothing. */
int rs_reproj_match(rs_context* ctx, const rs_frame_view* frame,
                    const rs_map_view* map, int replace, int max_distance,
                    int32_t* d_point_kp, int32_t* d_point_dist,
                    int32_t* d_prop_point, int32_t* d_prop_dist,
                    int32_t* d_match_kp, int32_t* d_match_point,
                    int32_t* d_match_count);

/* SURVEY.md 8(e) row 2 — the same match with the MAP SHARDED over the ranks of the attached communicator (RCCL or the
 * in-process group): mp_shard holds this rank's points, point_base the map order of its first point.  The per-keypoint
 * proposal table (distance << 32 | global map order) is MIN-all-reduced before the accept step — one
 * ncclAllReduce(min, u64) of 8 N bytes — so every rank returns the unsharded result, ties included.  d_prop_point and
 * d_match_point hold GLOBAL map indices; d_point_kp / d_point_dist cover the shard.  Every rank must make the call (an
 * empty shard is valid).  Without a communicator it is rs_reproj_match with an index offset.  Worth it for maps far
 * beyond 1e5 points; smaller maps are better served by replicas. */
int rs_reproj_match_sharded(rs_context* ctx, const rs_frame_view* frame, const rs_map_view* mp_shard, int point_base,
                            int replace, int max_distance,
                            int32_t* d_point_kp, int32_t* d_point_dist,
                            int32_t* d_prop_point, int32_t* d_prop_dist,
                            int32_t* d_match_kp, int32_t* d_match_point, int32_t* d_match_count);

/* rs_reproj_match for FLOAT descriptors under the L2 norm: d_frame_desc [N][dim] f32 are the frame's rows,
 * d_desc_pool [rows][dim] f32 the pool that map->d_obs_desc indexes (16-byte aligned, dim % 4 == 0, 4 .. 1024; any
 * other dim: RS_ERR_UNSUPPORTED).  Of the views it reads the pose, intrinsics, image size, keypoints, d_kp_matched,
 * d_kd_node_kp / left / right, kd_root and the map's CSR, positions, eligibility and centres; both u8 descriptor
 * pointers, d_kd_packed and d_kd_grid are ignored.  Gates, walk order and f32 operation order are rs_reproj_match's.
 * The distance of a (candidate, observation) pair, all f32:
 *   r0..r3 = 0; for k ascending: e = q[k] - t[k]; r[k & 3] = fmaf(e, e, r[k & 3])
 *   d2 = (r0 + r1) + (r2 + r3),  dist = sqrtf(d2) correctly rounded
 * Comparisons are the reference's (src/MapMatcher.cpp:77-97): a running best from max_distance with a strict '<' on dist
 * over candidates in the KD recursion's order and observations in list order; per keypoint a strict '<' over points in map
 * order.  So max_distance <= 0 (or NaN) proposes nothing.  Outputs as rs_reproj_match with f32 distances
 * (d_point_dist / d_prop_dist = max_distance where there is none; with no keypoint the count is zeroed and every point
 * gets -1 and max_distance); bit-exact against tests/match_l2_ref.py. */
int rs_reproj_match_l2(rs_context* ctx, const rs_frame_view* frame, const rs_map_view* map,
                       const float* d_frame_desc, const float* d_desc_pool, int dim,
                       int replace, float max_distance,
                       int32_t* d_point_kp, float* d_point_dist,
                       int32_t* d_prop_point, float* d_prop_dist,
                       int32_t* d_match_kp, int32_t* d_match_point, int32_t* d_match_count);

/* ---------------------------------------- §8(f) rank 4: the map, resident on the device */

/* MapMatcher::match walks the whole map twice per frame (src/MapMatcher.cpp:165-175); flattening the reference's
 * pointer graph for rs_reproj_match on every call costs ~100x the kernels.  rs_map keeps the flat map on the device
 * across frames; the calls below mirror, one for one, the operations the reference performs on Map / MapPoint / KeyFrame
 * (src/Map.cpp:44-124, src/MapPoint.cpp, src/Frame.cpp:80-116), each O(1) on the host; the device image is brought up
 * to date lazily, at the next use, and only for what changed (topology once per key frame; positions / key-frame
 * centres after a bundle adjustment).  Handles are small integers: point slots are never reused and ascending slot =
 * creation order = the reference's map order, which decides ties; observations of a point keep insertion order.
 * rs_frame holds a frame's keypoints, descriptors and KD-tree on the device (built and uploaded once, shared by the
 * calls of that frame); a frame promoted to a key frame hands its descriptor rows to the map device-to-device. */
typedef struct rs_map rs_map;
typedef struct rs_frame rs_frame;
int rs_map_create(rs_context* ctx, rs_map** out_map);
int rs_map_destroy(rs_map* map);
int rs_frame_create(rs_context* ctx, const float* h_keypoints /*[n][2]*/, const uint8_t* h_descriptors /*[n][32]*/, int n,
                    rs_frame** out_frame);                                        /* Frame::Frame, src/Frame.cpp:8-15 */
int rs_frame_destroy(rs_frame* frame);
/* A reusable frame (re)filled FROM DEVICE ARRAYS: what rs_track_features, rs_detect_features and rs_describe_features
 * leave on the device becomes an rs_frame without a host pass.  rs_frame_create_device allocates once for max_points
 * keypoints (envelope 1 .. 8192, the describer's and the detector's; outside it RS_ERR_UNSUPPORTED) and leaves n = 0.
 * rs_frame_assign_device gathers list a then list b with rs_describe_features' rule, read on the device —
 * n_a = clamp(d_count_a[0], 0, max_points), n_b = clamp(d_count_b[0], 0, max_points - n_a); either list may be NULL
 * (points and count together) — copies the first n = n_a + n_b rows of d_desc [>= n][32] and builds the KD-tree and its
 * packed form (rs_kdtree_pack's layout) on the device, byte for byte what rs_frame_create builds from the same arrays
 * (finite coordinates; with NaN the tree is still a permutation of the keypoints, but rs_kdtree_build's comparator is no
 * ordering then and nothing is promised about equality).  Stream-ordered on the context stream, no allocation per call;
 * it may be called again and again on one frame (nothing of the previous contents shows through; a key frame added from
 * it keeps its own copy of the rows).  ONE host synchronisation per call, to read n (4 bytes): rs_map_match sizes its
 * launches and outputs and rs_map_add_keyframe books pool rows by the host-side n; removing that read means device-side
 * n in the matching kernels and is not done here.  h_n (NULL = not wanted) receives n.
 * A frame from rs_frame_create has no capacity and is refused (RS_ERR_INVALID), as is a frame of another context.
 * rs_map_match, rs_map_add_keyframe and rs_frame_destroy take both kinds of frame. */
int rs_frame_create_device(rs_context* ctx, int max_points, rs_frame** out_frame);
int rs_frame_assign_device(rs_context* ctx, rs_frame* frame,
                           const float* d_pt_a, const int32_t* d_count_a,     /* rs_track_features' d_kept_pt / d_count */
                           const float* d_pt_b, const int32_t* d_count_b,     /* rs_detect_features' d_pt / d_counts + 1 */
                           const uint8_t* d_desc,                            /* rs_describe_features' d_desc */
                           int* h_n);
/* Diagnostic (synchronises): what a frame of either kind holds on the device.  Any pointer may be NULL.
 * h_kp [n][2], h_desc [n][32], h_kd [3][n] = node_kp | left | right, h_root [1], h_packed 20 n bytes. */
int rs_frame_download(rs_context* ctx, const rs_frame* frame, int* h_n, float* h_kp, uint8_t* h_desc,
                      int32_t* h_kd, int32_t* h_root, void* h_packed);
int rs_map_add_keyframe(rs_map* map, const rs_frame* frame, const float h_pose[16], int* out_kf);
int rs_map_set_keyframe_pose(rs_map* map, int kf, const float h_pose[16]);      /* Frame::set_pose */
int rs_map_add_point(rs_map* map, const float h_xyz[3], int* out_point);        /* Map::add_point / create_point */
int rs_map_set_position(rs_map* map, int point, const float h_xyz[3]);         /* MapPoint::set_position */
int rs_map_remove_point(rs_map* map, int point);                                /* Map::remove_point, src/Map.cpp:63-76 */
int rs_map_add_observation(rs_map* map, int point, int kf, int keypoint);       /* Map::associate, src/Map.cpp:95-113 */
int rs_map_remove_observation(rs_map* map, int point, int kf);                 /* Map::disassociate, src/Map.cpp:115-124 */
int rs_map_counts(const rs_map* map, int h_out[4]);   /* point slots, alive points, observations, key frames */
/* MapPoint::position() of the point slots [first, first + count) from the library's mirror (removed points keep
 * their last position); what a caller copies into its own objects after rs_map_pose_graph moved the whole map. */
int rs_map_get_positions(const rs_map* map, int first, int count, float* h_xyz /*[count][3]*/);

/* MapMatcher::match_map / match_key_frame / match_for_fuse (src/MapMatcher.cpp:107-127,165-175) against the resident
 * map; results identical to rs_reproj_match on the flattened map.
 *   h_kp_matched [n] or NULL: Frame::is_matched(keypoint) (:81);  h_matched_points: slots of the points the frame already
 *   matches (:53);  required_observer_kf >= 0: match_key_frame (:169);  n_only >= 0: match_for_fuse — only the listed
 *   slots take part, and they compete for a keypoint in LIST order, as the reference's loop over its vector does
 *   (:120-126) and as the flattened path does when the shim flattens that vector in order: ONE rule on both paths
 *   (dead slots in the list are skipped like the reference's null pointers);  replace as rs_reproj_match.
 * Outputs (host, capacity n each): the accepted matches in ascending keypoint order as (keypoint, point slot). */
int rs_map_match(rs_context* ctx, rs_map* map, rs_frame* frame, const float h_pose[16], const float h_intrinsics[4],
                 int width, int height, const uint8_t* h_kp_matched, const int32_t* h_matched_points, int n_matched_points,
                 int required_observer_kf, const int32_t* h_only_points, int n_only, int replace, int max_distance,
                 int32_t* h_match_kp, int32_t* h_match_point, int* h_count);

/* ---- the tail of Tracker::track on the resident map (src/Tracker.cpp:83-86): carry-over, pose refit, two matches.
 * An rs_frame of either kind owns the frame's match table, Frame::m_map_matches: keypoint -> point slot or -1 (a frame
 * from rs_frame_create_device: room for max_points; rs_frame_assign_device clears it for the new contents).  The calls
 * below read and write it on the device; none walks map objects on the host and none moves a list.  Envelope: frames of
 * at most 8192 keypoints and lists of at most 8192 entries (RS_ERR_UNSUPPORTED beyond), replace = 0 matching only
 * (match_for_fuse stays on rs_map_match).  A table may hold the slot of a point that was removed since (the reference:
 * a dangling pointer, undefined behaviour).  Here such a slot still counts as a match of its keypoint
 * (Frame::is_matched, Frame::num_map_matches) but is never a carry-over candidate and never enters the refit.
 * What still synchronises: the refit's completion flag, one count per match, rs_frame_assign_device's 4-byte n (and the
 * map's lazy upload after an edit, as everywhere). */
int rs_frame_matches_clear(rs_context* ctx, rs_frame* frame);
/* Frame::add_map_match (src/Frame.cpp:80-102) for a list, applied in LIST ORDER: entry i sets table[d_kp[i]] =
 * d_point[i] and clears any OTHER keypoint holding d_point[i]; repeated keypoints and repeated points resolve as the
 * sequential rule does (the last writer of a keypoint wins, a point lives at its last keypoint).  The count is read on
 * the device: n = clamp(d_count[0], 0, max_n), or max_n when d_count is NULL.  Entries with a keypoint outside the frame
 * or a negative point are skipped.  Stream-ordered, no host synchronisation. */
int rs_frame_matches_add(rs_context* ctx, rs_frame* frame, const int32_t* d_kp, const int32_t* d_point, const int32_t* d_count, int max_n);
/* Diagnostic (synchronises): h_kp_point [n] (NULL = not wanted), *h_count = Frame::num_map_matches(). */
int rs_frame_matches_download(rs_context* ctx, const rs_frame* frame, int32_t* h_kp_point, int* h_count);

int rs_map_set_track_consistent(rs_map* map, int point);      /* MapPoint::set_track_consistent; host O(1), the device flag follows lazily */
/* Tracker::track_from_last_frame (:197-230).  List entry i names keypoint j = d_inlier_index[i] of `next` (rs_estimate_pose's
 * inlier list: positions into the tracked list, which are next's first keypoints; NULL: j = i) and keypoint
 * d_prev_index[j] of `prev` (rs_track_features' d_kept_index).  n = clamp(d_count[0], 0, max_n) (NULL: max_n); both index
 * lists hold at least max_n entries, and an entry whose j is outside [0, min(max_n, next's n)) or whose previous keypoint
 * is outside prev is skipped.  An entry is a candidate when prev's table holds a point there that is alive and has >= 2
 * observations or is track-consistent (:209).  Fewer than min_points candidates (MIN_TRACKED_MAP_POINTS = 15): nothing is
 * written (:216-219).  Otherwise candidates are accepted in list order unless next already matches that keypoint or that
 * point (:223).  d_stats [2] (device, NULL = not wanted): candidates, accepted.  Stream-ordered, no host synchronisation. */
int rs_map_carry_matches(rs_context* ctx, rs_map* map, const rs_frame* prev, rs_frame* next, const int32_t* d_prev_index,
                         const int32_t* d_inlier_index, const int32_t* d_count, int max_n, int min_points, int32_t* d_stats);
/* (rs_map_refine_pose, Tracker::optimize_pose on the table: behind rs_refine_pose_inertial below) */
/* match_with_last_key_frame / match_with_map (:232-248): rs_map_match with replace = 0 whose "already matched" keypoints
 * and points are the frame's table, and whose accepted pairs go back into it (they are disjoint from it and unique on
 * both sides: a scatter).  Only *h_count comes back.  The map's flag table is all-zero again afterwards. */
int rs_map_match_frame(rs_context* ctx, rs_map* map, rs_frame* frame, const float h_pose[16], const float h_intrinsics[4],
                       int width, int height, int required_observer_kf, int max_distance, int* h_count);

/* ---- feature tracks on the device: TrackStore (src/TrackStore.cpp) and Mapper::needs_key_frame (src/Mapper.cpp:91-140).
 * rs_track_store holds every live track — a 64-bit id, its keypoint in the current frame and up to max_sightings sightings
 * {frame index, pixel, key-frame handle or -1, keypoint} — in a pool of max_points rows (1 .. 8192, the envelope of
 * rs_frame_create_device; max_sightings 1 .. 128, the reference uses 100; outside either: RS_ERR_UNSUPPORTED).  Every
 * call is ordered on the context stream and allocates nothing after creation.  Between rs_map_match_frame and the next
 * rs_track_features a per-frame caller makes carry, query, extend: one read-back of 24 bytes (the query's).
 * A frame of another context is RS_ERR_INVALID, a frame with more keypoints than max_points RS_ERR_UNSUPPORTED. */
typedef struct rs_track_store rs_track_store;
int rs_track_store_create(rs_context* ctx, int max_points, int max_sightings, rs_track_store** out_store);
int rs_track_store_destroy(rs_track_store* store);
int rs_track_store_clear(rs_context* ctx, rs_track_store* store);           /* a fresh TrackStore: no tracks, the id counter at 0 */
/* TrackStore::carry_forward (:12-35) in rs_map_carry_matches' list form: entry i names current keypoint
 * j = d_inlier_index[i] (NULL: j = i) and previous keypoint d_prev_index[j]; n = clamp(d_count[0], 0, max_n) read on the
 * device (NULL: max_n; max_n <= 8192).  An entry whose j is outside [0, min(max_n, max_points)) or whose previous keypoint
 * is outside the store or holds no track is skipped.  The track of a named previous keypoint moves to keypoint j with its
 * id and sightings; every other track is dropped and its row freed (n = 0 drops everything).  Repeats: the FIRST entry
 * naming a previous keypoint decides for its track, and of those entries the first naming a current keypoint gets it — a
 * track whose deciding entry loses its keypoint is dropped.  No host synchronisation. */
int rs_track_store_carry(rs_context* ctx, rs_track_store* store, const int32_t* d_prev_index, const int32_t* d_inlier_index,
                         const int32_t* d_count, int max_n);
/* TrackStore::extend (:37-54): every keypoint of `frame` without a track gets a new one, ids ascending with the keypoint
 * index from the store's counter; then every track of a keypoint of the frame that holds fewer than max_sightings
 * sightings appends {frame_index, the keypoint's pixel bit for bit, key_frame_handle (negative: -1), keypoint}.
 * No host synchronisation. */
int rs_track_store_extend(rs_context* ctx, rs_track_store* store, const rs_frame* frame, int frame_index, int key_frame_handle);
/* Mapper::covisible_points and unmapped_tracks (:91-120) from the frame's match table, ONE read-back of six integers:
 *   [0] covisible: table entries whose point is alive and observed by key frame last_key_frame (a removed point is not
 *       covisible; map NULL or last_key_frame < 0: 0)      [1] Frame::num_map_matches
 *   [2] waiting: tracks with >= min_sightings sightings, whose keypoint the table does not match, whose travel
 *       sqrtf(fl(fl(dx dx) + fl(dy dy))) between the last and the first sighting is not below min_travel (:107-117)
 *   [3] live tracks   [4] the smallest first-sighting frame index among them (-1 without tracks)
 *   [5] the id counter's low 32 bits (diagnostic). */
int rs_track_store_query(rs_context* ctx, rs_track_store* store, rs_map* map, const rs_frame* frame, int last_key_frame,
                         int min_sightings, float min_travel, int32_t h_out[6]);
/* Host function (no context, no device): Mapper::needs_key_frame's decision (:122-140) on rs_track_store_query's integers:
 * frame_gap >= max_key_frame_gap (a negative gap is the reference's unsigned wrap: true), or waiting >=
 * new_tracks_threshold, or covisible < min_covisible_points, or (float)covisible < min_covisible_fraction *
 * (float)last_key_frame_matches in f32.  The reference's constants (:21-26): 20, 200, 50, 0.7f; the other two of that
 * block, MIN_SIGHTINGS_FOR_TRACK = 3 and MIN_TRACK_TRAVEL_PIXELS = 20, are the query's parameters.  *h_out = 0 / 1. */
int rs_needs_key_frame(const int32_t h_query[6], int frame_gap, int last_key_frame_matches, int max_key_frame_gap,
                       int new_tracks_threshold, int min_covisible_points, float min_covisible_fraction, int* h_out);
/* What Mapper::triangulate_tracks needs back (:306-330), filled by ONE read-back (a second copy and synchronisation
 * follow only when the accepted tracks hold more than two key-frame sightings per packed track on average).  In: the capacities.  The accepted tracks
 * come in rs_triangulate_tracks' order (creation order, the top-up last); entry a: h_keypoint[a] its keypoint in the frame,
 * h_xyz[a] its position, h_sightings[a] its sighting count (the >= 3 rule of :326), and its KEY-FRAME sightings only as
 * pairs (handle, keypoint) h_kf_pairs[2 h_kf_ptr[a] .. 2 h_kf_ptr[a + 1]) in sighting order.  capacity_tracks >= the live
 * tracks of the last query (h_kf_ptr: one more entry); when n_pairs exceeds capacity_pairs only the first capacity_pairs
 * pairs were copied. */
typedef struct rs_track_results {
    int capacity_tracks, capacity_pairs;
    int32_t counts[3];          /* rs_triangulate_tracks' d_counts: accepted, of which top-up, inconsistent */
    int32_t out_of_range;       /* tracks with a sighting outside the pose range: packed as skipped */
    int32_t n_tracks;           /* tracks packed */
    int32_t n_pairs;
    int32_t* h_keypoint;        /* [capacity_tracks] */
    float* h_xyz;               /* [capacity_tracks][3] */
    int32_t* h_sightings;       /* [capacity_tracks] */
    int32_t* h_kf_ptr;          /* [capacity_tracks + 1] */
    int32_t* h_kf_pairs;        /* [capacity_pairs][2] */
    /* the rest of tracks::Selection, each NULL = not wanted: per accepted track its index among the packed tracks (id
     * order) and its parallax / required cosine; h_inconsistent [counts[2]] the packed indices the erase call will drop */
    int32_t* h_track;           /* [capacity_tracks] */
    float* h_parallax_cos;      /* [capacity_tracks] */
    float* h_required_cos;      /* [capacity_tracks] */
    int32_t* h_inconsistent;    /* [capacity_tracks] */
} rs_track_results;
/* Mapper::triangulate_tracks' loop (:246-305) from the store: the live tracks are packed on the device in ascending id
 * order (the order of the reference's std::map) into rs_triangulate_tracks' inputs — d_track_uv from the frame's keypoints,
 * d_skip from its match table (a track whose keypoint is outside the frame is skipped too), d_sight_ptr by a scan of the
 * counts, d_sight_pose = frame index - pose_base, d_sight_uv — and rs_triangulate_tracks runs on them unchanged (its
 * parameters as there; d_poses [n_poses][16] holds Trajectory::pose_at(pose_base + i)).  A track with a sighting outside
 * [pose_base, pose_base + n_poses) is packed as skipped and counted in out_of_range.  The number of tracks is the live count
 * the last rs_track_store_query read (no synchronisation of its own for it): a store changed since by carry or extend is
 * refused with RS_ERR_INVALID.  `map` is not read (NULL is fine).  Window membership, is_matched checks, create_point and
 * associate (:306-330) stay with the caller. */
int rs_track_store_triangulate(rs_context* ctx, rs_track_store* store, rs_map* map, const rs_frame* frame, const float* d_poses,
                               int n_poses, int pose_base, int kf_pose, const float h_intrinsics[4], float any_parallax_cosine,
                               float max_reprojection_error, float min_parallax_cosine, float rotation_parallax_factor,
                               int min_new_points, const float* d_required_by_pose, rs_track_results* results);
/* The tracks.erase loop (:333-335) for the inconsistent tracks of the last rs_track_store_triangulate, on the device;
 * nothing comes back.  Their keypoints get new tracks at the next extend.  Without a triangulate call since the store last
 * changed it does nothing. */
int rs_track_store_erase_inconsistent(rs_context* ctx, rs_track_store* store);
/* Diagnostics (synchronise).  The live tracks in ascending id order: *h_n of them, *h_next_id the id counter, h_id [n],
 * h_keypoint [n], h_count [n], h_sightings [n][max_sightings][5] 32-bit words {frame, x bits, y bits, key frame, keypoint}
 * (the first h_count[t] of row t are written); arrays hold max_points rows, any may be NULL.
 * rs_track_store_download_packed: the inputs the last rs_track_store_triangulate packed — h_track_uv [T][2], h_skip [T],
 * h_sight_ptr [T + 1], and h_sight_pose [S] / h_sight_uv [S][2] when S <= capacity_sightings. */
int rs_track_store_download(rs_context* ctx, const rs_track_store* store, int* h_n, uint64_t* h_next_id, uint64_t* h_id,
                            int32_t* h_keypoint, int32_t* h_count, int32_t* h_sightings);
int rs_track_store_download_packed(rs_context* ctx, const rs_track_store* store, int* h_n_tracks, int* h_n_sightings,
                                   float* h_track_uv, uint8_t* h_skip, int32_t* h_sight_ptr, int32_t* h_sight_pose,
                                   float* h_sight_uv, int capacity_sightings);

/* (rs_map_bundle_adjust: see the optimisation section below) */

/* ------------------------------------------------------ a5-a7: triangulation */

/* triangulation::triangulate_points (src/Triangulation.cpp:37-106), batched.
 * Correspondence i uses pose table entries d_pose_idx1[i] / d_pose_idx2[i]
 * (NULL = entry 0 / entry 1: the two-frame overload :28-35; per-item indices
 * give Mapper::triangulate_tracks' pattern, src/Mapper.cpp:246-259, in one
 * launch).  P = K*[R|t] in f32 (src/Camera.cpp:47-57), DLT rows
 * x*P[2]-P[0], y*P[2]-P[1] per view, f64 one-sided Jacobi SVD, right singular
 * vector of the smallest singular value rounded to f32, then the f32 gates:
 * cheirality (:78), parallax cosine > min_parallax_cosine rejects (:83-88),
 * reprojection error > max_reprojection_error rejects (:95-100).
 *   d_xyz  [n][3] dehomogenised point of EVERY correspondence (kept or not)
 *   d_keep [n]    1 = passed all gates
 *   d_out_index [n], d_out_xyz [n][3], d_out_count[1]: the compacted
 *   TriangulatedPoint list in input order (match_index = input index).
 * n == 0 is valid (empty guard :46-48). */
int rs_triangulate(rs_context* ctx,
                   const float* d_uv1 /*[n][2]*/, const float* d_uv2 /*[n][2]*/, int n,
                   const float* d_poses /*[n_poses][16] row-major*/, int n_poses,
                   const int32_t* d_pose_idx1, const int32_t* d_pose_idx2,
                   const float h_intrinsics[4] /*fx,fy,cx,cy*/,
                   float min_parallax_cosine, float max_reprojection_error,
                   float* d_xyz, uint8_t* d_keep,
                   int32_t* d_out_index, float* d_out_xyz, int32_t* d_out_count);

/* The same function as the reference's callers see it — host vectors in, the TriangulatedPoint list out
 * (src/Triangulation.h:24-37; called with ONE correspondence per call by Mapper::triangulate_tracks, src/Mapper.cpp:253,
 * and with a handful by pose::recover_pose, src/PoseEstimation.cpp:48).  Up to 256 correspondences run as one launch of
 * one workgroup whose inputs are kernel arguments / a pinned block and whose compacted result lands in pinned memory
 * behind a completion flag: no staging copies, no stream synchronisation.  Larger n goes through the staging pool and
 * rs_triangulate.  Results are bit-identical to rs_triangulate's.
 *   h_uv1, h_uv2 [n][2];  h_out_index [n], h_out_xyz [n][3] (capacity n), *h_count = points kept. */
int rs_triangulate_host(rs_context* ctx, const float* h_uv1, const float* h_uv2, int n,
                        const float h_pose1[16], const float h_pose2[16], const float h_intrinsics[4],
                        float min_parallax_cosine, float max_reprojection_error,
                        int32_t* h_out_index, float* h_out_xyz, int* h_count);

/* triangulate_points(frame1, frame2, matches, camera) (src/Triangulation.cpp:28-35) with
 * get_matching_points (:11-26) fused and the match list left on the device:
 * correspondence i = (d_kp1[d_match_train[i]], d_kp2[d_match_query[i]]) for
 * i < min(*d_n_matches, max_matches); poses = {pose of frame1, pose of frame2}.
 * Feeds rs_match_descriptors' output straight into the triangulation with no
 * host round trip.  Outputs as rs_triangulate, indexed by match position;
 * entries at i >= *d_n_matches are not written. */
int rs_triangulate_matches(rs_context* ctx,
                           const float* d_kp1 /*[n1][2] frame1 = train side*/,
                           const float* d_kp2 /*[n2][2] frame2 = query side*/,
                           const int32_t* d_match_train, const int32_t* d_match_query,
                           const int32_t* d_n_matches /*[1] device*/, int max_matches,
                           const float* d_poses /*[2][16]*/, const float h_intrinsics[4],
                           float min_parallax_cosine, float max_reprojection_error,
                           float* d_xyz, uint8_t* d_keep,
                           int32_t* d_out_index, float* d_out_xyz, int32_t* d_out_count);

/* BASELINE.json configs[3] (64 key-frame pairs x 2k keypoints): rs_triangulate_matches for `batch` independent
 * frame pairs in one launch pair; consumes rs_match_descriptors' batched output in place.  Every array is the
 * single-pair array with a leading batch dimension: d_kp1 [batch][n1][2], d_kp2 [batch][n2][2],
 * d_match_train / d_match_query [batch][max_matches], d_n_matches [batch], d_poses [batch][2][16] (frame1, frame2),
 * d_xyz [batch][max_matches][3], d_keep / d_out_index [batch][max_matches], d_out_xyz [batch][max_matches][3],
 * d_out_count [batch].  Results per pair are those of batch single calls, bit for bit. */
int rs_triangulate_matches_batch(rs_context* ctx, int batch,
                                 const float* d_kp1, int n1, const float* d_kp2, int n2,
                                 const int32_t* d_match_train, const int32_t* d_match_query,
                                 const int32_t* d_n_matches, int max_matches,
                                 const float* d_poses, const float h_intrinsics[4],
                                 float min_parallax_cosine, float max_reprojection_error,
                                 float* d_xyz, uint8_t* d_keep,
                                 int32_t* d_out_index, float* d_out_xyz, int32_t* d_out_count);

/* §8(f) rank 1 — the body of Mapper::triangulate_tracks (reference src/Mapper.cpp:246-305):
 * per track t (track-id order, the order of the reference's std::map<TrackId, Track>,
 * src/TrackStore.h:38) with sightings CSR d_sight_ptr[t] .. d_sight_ptr[t+1] (pose index into
 * d_poses = Trajectory::pose_at(frame_index), and pixel), key-frame pixel d_track_uv[t]:
 *   - d_skip[t] != 0 or no sightings: nothing (the host-side filters of :247-250);
 *   - triangulate (first sighting, key-frame pixel) under (pose of the first sighting, d_poses[kf_pose])
 *     with gates (any_parallax_cosine = 1.0, max_reprojection_error = 4.0), :252-262;
 *   - reproject into every sighting's pose, first error > max_reprojection_error => inconsistent,
 *     :264-275 (the caller erases those tracks, :332-334);
 *   - parallax cosine and required = min(min_parallax_cosine, cos(rotation_parallax_factor * turn)),
 *     :277-288;
 * then the selection :291-304: candidates with parallax <= required in track order, and, while
 * fewer than min_new_points, the remaining candidates by parallax cosine ascending (ties: track
 * order; std::sort leaves them unspecified upstream).  A NaN cosine (a non-finite pixel: every gate
 * is a comparison that NaN fails, so the track is a candidate with a NaN point) sorts after every
 * number, NaN among NaN in track order: the key is a total order, where std::sort's `<` is none.
 * Outputs, all device: d_status[t] 0 none / 1 candidate / 2 inconsistent; d_xyz[t][3];
 * d_parallax_cos[t]; d_required_cos[t]; d_accepted[0..counts[0]) track indices in creation order
 * (the last counts[1] of them are the top-up); d_inconsistent[0..counts[2]); d_counts[3].
 * Point creation / association (:306-330) is pointer work and stays with the caller.
 * d_required_by_pose [n_poses] or NULL: `required` depends only on the pair (pose of the first sighting, key-frame pose),
 * and it is the one quantity of this function that goes through libm (std::acos, std::cos, :282-288).  With the table —
 * rs_parallax_requirements, a HOST function using the host's libm like the reference does — required, and therefore the
 * accepted list, are bit-identical to the CPU path; with NULL the device's acosf / cosf are used (<= 3e-7 apart, which may
 * decide a track that sits exactly on its requirement differently). */
int rs_triangulate_tracks(rs_context* ctx, int n_tracks, const float* d_track_uv /*[T][2]*/,
                          const uint8_t* d_skip /*[T] or NULL*/, const int32_t* d_sight_ptr /*[T+1]*/,
                          const int32_t* d_sight_pose /*[S]*/, const float* d_sight_uv /*[S][2]*/,
                          const float* d_poses /*[n_poses][16]*/, int n_poses, int kf_pose,
                          const float h_intrinsics[4], float any_parallax_cosine,
                          float max_reprojection_error, float min_parallax_cosine,
                          float rotation_parallax_factor, int min_new_points, uint8_t* d_status,
                          float* d_xyz, float* d_parallax_cos, float* d_required_cos,
                          int32_t* d_accepted, int32_t* d_inconsistent, int32_t* d_counts /*[3]*/,
                          const float* d_required_by_pose /*[n_poses] or NULL*/);
/* Host function (no context): h_required[p] = min(min_parallax_cosine, cos(rotation_parallax_factor * turn(p))) with
 * turn(p) = acos(clamp((trace(R_kf R_p^T) - 1) / 2)) in f32, operation for operation src/Mapper.cpp:281-288. */
int rs_parallax_requirements(const float* h_poses /*[n_poses][16]*/, int n_poses, int kf_pose,
                             float min_parallax_cosine, float rotation_parallax_factor, float* h_required /*[n_poses]*/);

/* §8(f) rank 3 — the arithmetic of Mapper::cull_points (reference src/Mapper.cpp:396-431) and of
 * Slam::reprojection_error (src/Slam.cpp:302-317): for every point p with observations CSR
 * d_obs_ptr[p] .. d_obs_ptr[p+1] (pose index into d_poses, pixel) the mean over its observations of
 * |Camera::project(pose, X_p) - pixel| in f32, summed in CSR order (the reference iterates an
 * unordered_map); d_cull[p] = 1 when the point has observations and the mean exceeds max_mean_error
 * (MAX_POINT_REPROJECTION_ERROR = 3.0, src/Mapper.cpp:39); d_cull_idx[0 .. *d_cull_count) lists the culled
 * points in ascending order; d_sums = {sum of all per-observation errors (f64 sum of the f32 values),
 * number of observations}: reprojection_error() = sums[0] / sums[1].  The caller selects the local points
 * (:398-408) and removes them from the map (:426-429). */
int rs_point_errors(rs_context* ctx, int n_points, const float* d_positions /*[P][3]*/,
                    const int32_t* d_obs_ptr /*[P+1]*/, const int32_t* d_obs_pose /*[M]*/,
                    const float* d_obs_uv /*[M][2]*/, const float* d_poses /*[n_poses][16]*/, int n_poses,
                    const float h_intrinsics[4], float max_mean_error, float* d_mean_err /*[P]*/,
                    uint8_t* d_cull /*[P]*/, int32_t* d_cull_idx /*[P]*/, int32_t* d_cull_count /*[1]*/,
                    double* d_sums /*[2]*/);

/* The tail of Mapper::bundle_adjust (reference src/Mapper.cpp:366-393): single-observation points are excluded from
 * the optimisation (MIN_OBSERVATIONS_TO_OPTIMIZE, src/Optimization.cpp:98) and afterwards moved rigidly with the
 * free frame that observes them:  X' = R_after^T ((R_before X + t_before) - t_after), in f32.
 * Entry i moves point d_point_idx[i] (NULL = point i) of d_positions [.][3] with frame d_frame_idx[i];
 * d_poses_before / d_poses_after [n_frames][16] are Frame::pose() before and after rs_bundle_adjust.  A point must
 * be listed at most once (it has one observation); an entry whose frame index is outside [0, n_frames) is skipped. */
int rs_reanchor_points(rs_context* ctx, int n, const int32_t* d_point_idx, const int32_t* d_frame_idx,
                       const float* d_poses_before, const float* d_poses_after, int n_frames,
                       float* d_positions);
/* The same with the poses where the reference keeps them — on the HOST (Frame::pose(), src/Mapper.cpp:366-393):
 * h_poses_before / h_poses_after [n_frames][16] are read before the call returns.  Up to 32 frames travel as kernel
 * arguments (no upload, no extra launch: a local window has 20); more are copied to the device first. */
int rs_reanchor_points_host_poses(rs_context* ctx, int n, const int32_t* d_point_idx, const int32_t* d_frame_idx,
                                  const float* h_poses_before, const float* h_poses_after, int n_frames,
                                  float* d_positions);

/* ----------------------------------------------------- a9-a13: optimisation */

typedef enum rs_ba_termination {
    RS_BA_NO_CONVERGENCE = 0,     /* max_num_iterations reached */
    RS_BA_CONVERGENCE_FUNCTION = 1,
    RS_BA_CONVERGENCE_PARAMETER = 2,
    RS_BA_CONVERGENCE_GRADIENT = 3,
    RS_BA_CONVERGENCE_RADIUS = 4,
    RS_BA_FAILURE = 5             /* too many consecutive invalid steps / non-finite cost */
} rs_ba_termination;

/* Ceres 2.x trust-region defaults restated; solve() in the
 * reference only sets the iteration cap (src/Optimization.cpp:127-134). */
typedef struct rs_ba_options {
    int max_num_iterations;             /* BA_ITERATIONS / POSE_ITERATIONS = 10 (:118-119) */
                                        /* 0 .. 1000; 0: the cost and the gradient at the input, no step (NO_CONVERGENCE, usable) */
    double huber_delta;                 /* sqrt(5.991) (:219,:311) */
    double initial_trust_region_radius; /* 1e4 */
    double max_trust_region_radius;     /* 1e16 */
    double min_trust_region_radius;     /* 1e-32 */
    double min_relative_decrease;       /* 1e-3 */
    double min_lm_diagonal;             /* 1e-6 */
    double max_lm_diagonal;             /* 1e32 */
    double function_tolerance;          /* 1e-6 */
    double gradient_tolerance;          /* 1e-10 */
    double parameter_tolerance;         /* 1e-8 */
    int max_num_consecutive_invalid_steps; /* 5 */
    int jacobi_scaling;                 /* 1 */
} rs_ba_options;

void rs_ba_default_options(rs_ba_options* opt);

typedef struct rs_ba_summary {
    int termination;        /* rs_ba_termination */
    int iterations;         /* LM iterations run (successful + unsuccessful) */
    int successful_steps;
    int usable;             /* the reference's accept rule (src/Optimization.cpp:136-141):
                               termination != FAILURE && isfinite(final) && final <= initial */
    double initial_cost;    /* 1/2 sum rho(|r|^2) at the input */
    double final_cost;
    double final_radius;
} rs_ba_summary;

/* optimization::bundle_adjust's solve (src/Optimization.cpp:269-374): Huber-robust
 * reprojection residuals (:21-72), Levenberg-Marquardt with point-block Schur
 * elimination, all in f64.
 *   d_cameras [C][6] f64 in/out: angle-axis(R_cw) then camera centre (pack_pose :144-149)
 *   h_cam_free [C] u8: FrameConfig::optimize; fixed cameras keep their residuals (:304-315)
 *   d_points  [P][3] f64 in/out: the FREE points (>= 2 observations and seen by a
 *             free frame, :287-302); points that are not free are not passed
 *   observations sorted by point (CSR): d_obs_ptr [P+1], d_obs_cam [M], d_obs_uv [M][2] f32
 * d_cameras / d_points are overwritten only when summary.usable is 1, exactly
 * like the reference writes back only on an accepted solve (:360-372).  They are
 * STREAM-ordered results: the call returns as soon as the summary (and the pinned
 * camera mirror, rs_ba_get_cameras) is on the host, possibly while the copy into
 * d_cameras / d_points is still running on the context's stream; anything that
 * reads them on that stream is ordered behind it, any other reader synchronises
 * first (rs_context_synchronize).
 * With an RCCL communicator attached (rs_comm_init_rank) the points/observations
 * are this rank's landmark shard, cameras are replicated, and the reduced
 * camera system and the cost are all-reduced every LM step. */
int rs_bundle_adjust(rs_context* ctx,
                     int n_cameras, int n_points, int n_obs,
                     double* d_cameras, const uint8_t* h_cam_free,
                     double* d_points,
                     const int32_t* d_obs_ptr, const int32_t* d_obs_cam,
                     const float* d_obs_uv,
                     const float h_intrinsics[4],
                     const rs_ba_options* options /*NULL = defaults*/,
                     rs_ba_summary* h_summary);

/* optimization::bundle_adjust (src/Optimization.cpp:269-374, vision-only) on the resident map: the window
 * (h_kfs [n_kfs] key-frame handles in FrameConfig order, h_free [n_kfs] = FrameConfig::optimize) is flattened ON THE
 * DEVICE from the resident image (three small kernels over the map's point slots), solved with rs_bundle_adjust, and on
 * a usable solve the map — device image and mirror — takes the result.  The caller gets the same for its own objects:
 * h_out_poses [n_kfs][16] (unchanged rows for fixed key frames / unusable solves) and the free points, in ascending
 * slot order, with their new positions (h_out_points / h_out_xyz, `capacity` entries; *h_n_points = how many there
 * were).  Free points: alive, >= 2 observations, matched by an optimised frame of the list (:287-302).  The flattened
 * path (host mirror / shim -> rs_bundle_adjust) lists the same set in first-seen order (the reference's, :287-302): the
 * f64 summation order inside the solve differs, so the two agree to the solver's noise (1e-9 relative), not bit for bit. */
int rs_map_bundle_adjust(rs_context* ctx, rs_map* map, const int32_t* h_kfs, const uint8_t* h_free, int n_kfs,
                         const float h_intrinsics[4], const rs_ba_options* options, rs_ba_summary* h_summary,
                         float* h_out_poses, int32_t* h_out_points, float* h_out_xyz, int capacity, int* h_n_points);

/* The problem rs_map_bundle_adjust would solve for the same window, built by the same kernels and copied out without
 * solving: h_points [cap_points] free slots (ascending), h_xyz [cap_points][3] their f64 positions, h_obs_ptr
 * [cap_points + 1] CSR by point, h_obs_cam [cap_obs] list index of the observing key frame (list order within a point),
 * h_obs_uv [cap_obs][2] keypoints.  *h_n_points / *h_n_obs = the full sizes; nothing is copied unless both fit.  For
 * tests and diagnostics: it neither solves nor changes the map. */
int rs_map_window(rs_context* ctx, rs_map* map, const int32_t* h_kfs, const uint8_t* h_free, int n_kfs,
                  int32_t* h_points, double* h_xyz, int32_t* h_obs_ptr, int32_t* h_obs_cam, float* h_obs_uv,
                  int cap_points, int cap_obs, int* h_n_points, int* h_n_obs);

/* ---- Mapper::insert (src/Mapper.cpp:152-174) on the resident map.  With rs_track_store_triangulate, rs_track_store_
 * erase_inconsistent and rs_map_bundle_adjust the five calls below take a key frame from "the tracker's frame with its device
 * match table" to "inserted, adjusted, re-anchored, culled" without a host pass over map objects:
 *   rs_map_insert_keyframe -> rs_track_store_triangulate -> rs_map_add_track_points -> rs_track_store_erase_inconsistent
 *   -> rs_map_bundle_adjust -> rs_map_reanchor -> rs_map_cull_points.
 *
 * rs_map_insert_keyframe: rs_map_add_keyframe followed by the adoption loop (:157-159).  The frame's device match table is
 * read back once (one synchronisation); in ascending keypoint order every entry whose point is alive is associated with the
 * new key frame by rs_map_add_observation's rule (Map::associate: a point named by two keypoints ends up at the later one).
 * An entry that names a removed slot, or a slot the map never had, is skipped (a dangling pointer in the reference).
 * *out_kf = the handle, *h_n_adopted = the associations made.  RS_ERR_INVALID: null argument, a map or frame of another
 * context. */
int rs_map_insert_keyframe(rs_context* ctx, rs_map* map, const rs_frame* frame, const float h_pose[16], int* out_kf,
                           int* h_n_adopted);
/* Mapper::triangulate_tracks' creation loop (:310-331) for the accepted tracks of rs_track_store_triangulate's results, in
 * their order.  Host only (mirror edits, no kernel, no synchronisation).  Per accepted track a: rs_map_add_point at h_xyz[a],
 * associate it with key frame kf at h_keypoint[a] (Map::create_point, :312), then its key-frame sighting pairs (handle,
 * keypoint) in sighting order: a pair is skipped when its handle is negative, equals kf, or is not in h_window_kfs [n_window]
 * (:316-318), or when the observer already matches that keypoint or that point (:319-321); otherwise it is associated
 * (:322).  h_sightings[a] >= 3 sets track-consistent (:326-329).  h_new_points [counts[0]] (NULL: not wanted) gets the new
 * slots.  RS_ERR_INVALID with the map unchanged: n_pairs > capacity_pairs (the pairs are incomplete), counts[0] outside
 * 0 .. capacity_tracks, an unknown key frame in the window list, a keypoint outside its key frame, a null array. */
int rs_map_add_track_points(rs_map* map, int kf, const rs_track_results* results, const int32_t* h_window_kfs, int n_window,
                            int32_t* h_new_points);
/* The tail of Mapper::bundle_adjust (:379-393) on the device image: h_kfs [n_kfs] the OPTIMISED key frames of the window,
 * h_before [n_kfs][16] their poses before the adjustment; "after" is the map's current pose.  One lane per point slot: a slot
 * that is alive, has exactly one observation and whose observer is listed moves to
 *     X' = R_after^T ((R_before X + t_before) - t_after)            (f32, rs_reanchor_points' body and operation order)
 * in the image, in place; the moved slots come back in ascending order with their new positions through one read-back, the
 * mirror takes them, and the caller gets them in h_out_points / h_out_xyz (`capacity` entries, either may be NULL;
 * *h_n_points = how many there were, as rs_map_bundle_adjust).  The image stays current: the next use of the map uploads
 * nothing.  RS_ERR_INVALID: an unknown key frame or one listed twice, a null list, a map of another context. */
int rs_map_reanchor(rs_context* ctx, rs_map* map, const int32_t* h_kfs, const float* h_before, int n_kfs,
                    int32_t* h_out_points, float* h_out_xyz, int capacity, int* h_n_points);
/* Mapper::cull_points (:396-431) on the device image.  Local points (:398-408): alive and observed by a key frame of h_kfs
 * [n_kfs] (the window's key frames plus the new one; the map keeps a key frame's match table and the points' observation
 * lists consistent, so "matched by the frame" is "observed by it").  Per local point, over ALL of its observations in
 * insertion order: err += sqrtf(dx dx + dy dy) of Camera::project under the observer's pose against its keypoint, in f32
 * (rs_point_errors' body); culled when cnt > 0 && err / (float)cnt > max_mean_error (:420; the reference's
 * MAX_POINT_REPROJECTION_ERROR is 3).  h_removed [capacity] the culled slots ascending, h_removed_xyz [capacity][3] (NULL:
 * not wanted) their positions (diagnostics.culled, :426-428); *h_n_removed their number, *h_n_local (NULL: not wanted) the
 * local points.  apply = 0 reports and changes nothing; apply = 1 removes each listed point as rs_map_remove_point does, in
 * ascending order (the device image is re-flattened at its next use).  One synchronisation and one read-back per call.
 * RS_ERR_INVALID: *h_n_removed > capacity (the count is reported, nothing is removed), an unknown key frame or one listed
 * twice, a null argument, a map of another context. */
int rs_map_cull_points(rs_context* ctx, rs_map* map, const int32_t* h_kfs, int n_kfs, const float h_intrinsics[4],
                       float max_mean_error, int apply, int32_t* h_removed, float* h_removed_xyz, int capacity,
                       int* h_n_removed, int* h_n_local);

/* ---- Mapper::fuse_loop (src/Mapper.cpp:41-77,176-220) on the resident map: after rs_map_verify_loop accepted a candidate
 * and rs_map_pose_graph moved the map, the duplicated points are fused; rs_map_bundle_adjust with the oldest window frame
 * fixed follows (Mapper::bundle_adjust(query, true)).
 *
 * Two orders that the reference leaves unspecified are fixed here:
 *   source order       the old points compete for a keypoint in ascending point slot (map order), earliest wins (the
 *                      reference builds its list from an unordered_set);
 *   covisible ranking  shared count descending, key-frame handle ascending (the reference sorts an unordered_map by count).
 * Agreement with a particular standard library is not claimed.
 *
 * Outcome of one (keypoint, point) entry, by Mapper::fuse_match's branches: */
enum {
    RS_FUSE_SKIPPED = 0,        /* keypoint outside the key frame, or the point is dead or unknown: a no-op (the reference
                                   would follow a dangling pointer) */
    RS_FUSE_ASSOCIATED = 1,     /* the keypoint was free: the point is associated with it */
    RS_FUSE_POINT_MATCHED = 2,  /* the keypoint was free but the key frame already matches the point */
    RS_FUSE_SAME = 3,           /* the keypoint already holds that point */
    RS_FUSE_OLD = 4,            /* the keypoint's point is an old point: nothing is fused */
    RS_FUSE_FUSED = 5           /* the keypoint's point was fused into the entry's point and removed */
};
/* Map::fuse (src/Map.cpp:78-95): every observation of `discarded`, in its insertion order, moves to `kept` unless the
 * observer already sees `kept`; `discarded` hands over its track-consistent flag and is removed.  Host only, O(observations).
 * kept == discarded is a no-op.  RS_ERR_INVALID: a dead or unknown slot. */
int rs_map_fuse_points(rs_map* map, int kept, int discarded);
/* Diagnostics, host only.  The observations of a point slot as (key frame, keypoint) in INSERTION order — the order the
 * viewing normal is summed in — and a key frame's keypoint -> point table (-1 = unmatched).  *h_n = how many there are;
 * the first min(*h_n, capacity) are copied (the arrays may be NULL with capacity 0).  A removed slot has no observations.
 * RS_ERR_INVALID: a slot the map never had / an unknown key frame, a null count. */
int rs_map_get_observations(const rs_map* map, int point, int32_t* h_kf, int32_t* h_kp, int capacity, int* h_n);
int rs_map_get_keyframe_matches(const rs_map* map, int kf, int32_t* h_kp_point, int capacity, int* h_n);

#define RS_FUSE_MAX_WINDOW 64
#define RS_FUSE_MAX_COVISIBLE 64
#define RS_FUSE_MAX_INLIERS 8192
typedef struct rs_fuse_options {
    float intrinsics[4];        /* fx fy cx cy */
    int width, height;
    int max_distance;           /* descriptor gate of match_for_fuse; the reference's extractor: 64 */
    int min_shared;             /* MIN_LOOP_COVISIBLE = 15 */
    int max_covisible;          /* LOOP_COVISIBLE_KFS = 20; 0 .. RS_FUSE_MAX_COVISIBLE */
    int check;                  /* 1: refuse (RS_ERR_INTERNAL, map unchanged) a map whose tables and observation lists disagree;
                                   compare the device's old frames with the host ranking and the device's final working
                                   state with the replayed mirror (one more read-back) */
    int32_t* h_sources; int capacity_sources;       /* optional (NULL): receives the sources, ascending slot (first capacity) */
    int32_t* h_removed; int capacity_removed;       /* optional (NULL): receives the removed slots in the order they were fused */
} rs_fuse_options;
typedef struct rs_fuse_report {
    int n_old_frames;                               /* 1 + covisibles */
    int32_t old_frames[RS_FUSE_MAX_COVISIBLE + 1];  /* the candidate first, then by rank */
    int n_sources;                                  /* old points = the sources of match_for_fuse */
    int outcomes[6];                                /* entries per RS_FUSE_* outcome, inliers and window together */
    int n_removed;                                  /* fused-away points (= outcomes[RS_FUSE_FUSED]) */
    int device_state_mismatches;                    /* check = 1: differing words; -1 = not checked */
} rs_fuse_report;                                   /* outputs only: the call writes every field and reads none */
/* Mapper::fuse_loop.  h_inlier_kp / h_inlier_point [n_inliers]: rs_loop_verifier_download's inlier list (keypoint of the
 * query, point slot).  h_window_kfs [n_window]: the caller's bundle-adjustment window in its order (the policy `first = size -
 * BA_WINDOW` stays with the caller, as in rs_map_cull_points).
 *   1  prologue on the device image: shared counts per key frame (one lane per candidate keypoint walks its point's
 *      observation row), the ranking above in one workgroup, a flag per point slot from the old frames' table rows, the
 *      sources by one ordered compaction; read-back 1: the old frames and the number of sources S.
 *   2  the inliers, on the host mirror, in list order (each an O(1) edit).
 *   3  per window key frame that is not an old frame, in order, with no host synchronisation between frames: its KD-tree
 *      from its pool keypoints, the sources' eligibility from the CURRENT source rows, rs_reproj_match (replace = 1) on the
 *      source view, then the fuses of the accepted matches applied to the device's working state (source observation rows
 *      rebuilt dense by count / scan / copy / append into the other of two buffers; the key-frame tables; an alive copy).
 *      Appended observations keep the discarded point's observation order.
 *   4  read-back 2: the accepted (keypoint, point) pairs of every frame.  The mirror replays them and recomputes every
 *      outcome; the image is re-flattened at its next use, as after every edit.
 * So: two synchronisations per call plus the map's lazy upload (twice when the inliers edited the map); a third read-back
 * with options->check.  Scratch is allocated on first use at a given size and kept: the first call at a size also
 * synchronises where it allocates (its scratch, rs_reproj_match's proposal table), and the staging pool is drained once
 * between stage 1 and stage 3; none of this lies between two window frames.
 * Journal (each array optional, NULL = not wanted): section 0 = the inliers, section 1 + w = window entry w (empty for an old
 * frame); h_section_ptr [n_window + 2]; entry e = (h_kp[e], h_point[e], h_outcome[e]).  *h_n_entries = the total; when
 * capacity is smaller the first `capacity` entries are copied and the map is edited all the same.
 * Envelope: key frames (query, candidate, window) of at most 8192 keypoints, n_window 0 .. RS_FUSE_MAX_WINDOW, max_covisible
 * 0 .. RS_FUSE_MAX_COVISIBLE, n_inliers 0 .. RS_FUSE_MAX_INLIERS; outside it RS_ERR_UNSUPPORTED.  RS_ERR_INVALID with the
 * map unchanged: an unknown key frame, a key frame listed twice in the window, a null argument, a map of another context.
 * Every argument check runs before the first edit or launch. */
int rs_map_fuse_loop(rs_context* ctx, rs_map* map, int query_kf, int candidate_kf,
                     const int32_t* h_inlier_kp, const int32_t* h_inlier_point, int n_inliers,
                     const int32_t* h_window_kfs, int n_window,
                     const rs_fuse_options* options, rs_fuse_report* report,
                     int32_t* h_section_ptr, int32_t* h_kp, int32_t* h_point, int32_t* h_outcome, int capacity,
                     int* h_n_entries);

/* Throughput mode: B INDEPENDENT windows (several sessions / maps served by one GPU) in one call.  A local-window
 * solve is a chain of small dependent launches that leaves most of the 256 CUs idle.
 *   grid mode (default)  every kernel of the solve runs ONCE for all windows (grid z = window, per-window arguments in a
 *                        device table): B x 157 workgroups in the Schur kernel, B x 3 in the reduced solve, one launch
 *                        per round instead of one per window and round.  For windows of at most 64 cameras on the
 *                        local-window kernels (what a local window is); the host follows the slowest window's progress.
 *   lanes                otherwise (or "ba_batch_mode" = 1): up to `RS_BA_BATCH_LANES` child contexts (own stream, own
 *                        workspace), one host thread each, ordinary solves side by side.
 * Results per window are those of rs_bundle_adjust: the same schedule, values to summation-order noise.
 * Ordering: in both modes the windows' d_cameras / d_points are complete for anything ordered behind the call on THIS
 * context's stream (the lanes' streams are joined into it before the call returns), and rs_context_synchronize(ctx)
 * covers them.
 * h_problems[i] is the argument list of rs_bundle_adjust.  rs_ba_get_trace / _cameras refer to single solves only. */
#define RS_BA_BATCH_LANES 8
typedef struct rs_ba_problem {
    int n_cameras, n_points, n_obs;
    double* d_cameras;
    const uint8_t* h_cam_free;
    double* d_points;
    const int32_t* d_obs_ptr;
    const int32_t* d_obs_cam;
    const float* d_obs_uv;
    float intrinsics[4];
} rs_ba_problem;
int rs_bundle_adjust_batch(rs_context* ctx, int n_problems, const rs_ba_problem* h_problems,
                           const rs_ba_options* options /*NULL = defaults*/, rs_ba_summary* h_summaries /*[n_problems]*/);

/* Per-iteration record of the last rs_bundle_adjust on this context: what ceres::Solve prints with
 * minimizer_progress_to_stdout (the reference prints summary.BriefReport(), src/Optimization.cpp:135).
 * Entry i describes LM iteration i + 1.  outcome: 1 successful step, 0 rejected step, -1 invalid step
 * (linear solver failure or model_cost_change <= 0), 2 terminated by the parameter / function
 * tolerance test of this step.  Valid until the next optimisation call on the context. */
typedef struct rs_ba_iteration {
    double cost;               /* cost at x when the step was computed */
    double candidate_cost;     /* cost at x + step (0 for an invalid step) */
    double model_cost_change;
    double radius;             /* trust-region radius of this step */
    double step_norm, x_norm;  /* the two norms of the parameter-tolerance test */
    int outcome;
    int reserved0;
    double reserved1;
} rs_ba_iteration;
int rs_ba_get_trace(rs_context* ctx, rs_ba_iteration* h_out, int capacity, int* h_count);
/* The cameras as rs_bundle_adjust left them in d_cameras, from a pinned-memory mirror the last kernel of the solve
 * wrote: no device read-back, no synchronisation.  The reference keeps poses in host objects (Frame::set_pose after
 * unpack_pose, src/Optimization.cpp:363-368); the shim calls this, then rs_unpack_poses.  n_cameras must be the
 * solve's.  Valid until the next optimisation call on the context. */
int rs_ba_get_cameras(rs_context* ctx, double* h_cameras /*[n_cameras][6]*/, int n_cameras);
/* Launch accounting of the last rs_bundle_adjust: h_out[0] = rounds that did work (one K5 + K7 + K8 each),
 * [1] = rounds that relinearised (the others only re-damped after a rejected step), [2] = speculative sets
 * evaluated in total (= LM steps solved for, >= iterations), [3] = rounds enqueued by the host, [4] = solves of this
 * context (since it was created) that were run a second time as separate launches because a workgroup of the fused
 * solve + back-substitution launch timed out waiting for its hand-off word ("ba_handoff_timeout_us", default 4000:
 * a scheduling event — queue preemption, another process on the GPU — not a solver failure), [5..7] reserved (0). */
int rs_ba_get_stats(rs_context* ctx, int h_out[8]);

/* optimization::refine_pose (src/Optimization.cpp:194-267), vision-only:
 * the same residual with the points held constant, 6 unknowns.
 *   h_camera [6] f64 in/out;  d_points [n][3] f64;  d_uv [n][2] f32.
 * n == 0 returns RS_OK with summary.usable = 0 ("nothing to constrain", :227-229). */
int rs_refine_pose(rs_context* ctx, double h_camera[6],
                   const double* d_points, const float* d_uv, int n,
                   const float h_intrinsics[4],
                   const rs_ba_options* options, rs_ba_summary* h_summary);

/* ------------------------------------------- a15 / §8(f) rank 2: inertial residual blocks */

/* One IMU factor pair between two consecutive OPTIMISED frames of rs_bundle_adjust_inertial's camera list
 * (reference src/Optimization.cpp:317-346): imu::Preintegrated exactly as imu::preintegrate left it (src/Imu.h:30-40,
 * src/Imu.cpp:71-134 — that small sequential host code stays the reference's), matrices ROW-major, plus the two bias
 * random-walk densities of imu::NoiseDensity (src/Imu.h:46-48).  Each factor adds the 9-residual preintegration block
 * over (pose_i, velocity_i, bias_i, pose_j, velocity_j) whitened by L^-1 of the covariance's LLT (identity when it is not
 * positive definite, src/ImuFactor.cpp:10-17) and the 6-residual bias random walk over (bias_i, bias_j) with
 * sigma = density * sqrt(max(duration, 1e-9)) (:111-117); no loss function on either. */
typedef struct rs_imu_factor {
    int cam_i, cam_j;
    double duration;
    double rotation[9];
    double velocity[3], position[3];
    double covariance[81];
    double bias_gyro[3], bias_accel[3];     /* bias the preintegration was run with */
    double bias_jacobian[54];               /* 9 x 6 */
    double gyro_bias_sigma, accel_bias_sigma;
} rs_imu_factor;

/* optimization::bundle_adjust with InertialInput::usable() (src/Optimization.cpp:269-374 incl. :317-346).  As
 * rs_bundle_adjust, plus per-camera velocity (3) and bias (6: gyro, accel) parameter blocks for the frames the factors
 * touch: h_velocity [C][3], h_bias [C][6] in/out (host: they live in Frame::inertial(), src/Frame.h:13-16), written
 * back for the free frames on a usable solve (unpack_inertial, :363-368).  n_factors == 0 is rs_bundle_adjust.
 * The reduced camera system has 6 unknowns per free camera + 9 per inertial frame. */
int rs_bundle_adjust_inertial(rs_context* ctx,
                              int n_cameras, int n_points, int n_obs,
                              double* d_cameras, const uint8_t* h_cam_free,
                              double* d_points,
                              const int32_t* d_obs_ptr, const int32_t* d_obs_cam,
                              const float* d_obs_uv,
                              const float h_intrinsics[4],
                              double* h_velocity, double* h_bias,
                              const rs_imu_factor* h_factors, int n_factors,
                              const double h_gravity[3],
                              const rs_ba_options* options /*NULL = defaults*/,
                              rs_ba_summary* h_summary);

/* optimization::refine_pose with an InertialConstraint (src/Optimization.cpp:231-267).
 *   kind 0: none (= rs_refine_pose)
 *   kind 1: RotationPrior — h_predicted [9] row-major world->camera rotation, sigma_radians (> 0, else ignored)
 *   kind 2: InertialDelta — the previous frame's pose / velocity / bias are constant blocks (h_prev_pose [6] packed
 *           like a camera, h_prev_velocity [3], h_prev_bias [6]), h_delta its preintegration summary, h_gravity [3];
 *           this frame's velocity h_velocity [3] is a free block, written back on a usable solve (ignored when
 *           h_delta->duration <= 0, InertialDelta::enabled) */
int rs_refine_pose_inertial(rs_context* ctx, double h_camera[6],
                            const double* d_points, const float* d_uv, int n,
                            const float h_intrinsics[4], int kind,
                            const double h_predicted[9], double sigma_radians,
                            const double h_prev_pose[6], const double h_prev_velocity[3], const double h_prev_bias[6],
                            const rs_imu_factor* h_delta, const double h_gravity[3], double h_velocity[3],
                            const rs_ba_options* options, rs_ba_summary* h_summary);

/* Tracker::optimize_pose -> optimization::refine_pose on the frame's table: a gather kernel walks it in ascending
 * keypoint order (Frame::map_matches()), keeps the entries whose point is alive with >= 2 observations
 * (MIN_OBSERVATIONS_TO_OPTIMIZE) and writes their positions (f32 widened to f64) and pixels; K11 runs on those arrays
 * with the count read on the device — the result is bit for bit rs_refine_pose_inertial's on the same arrays.  The gates
 * are evaluated on the device: fewer than min_matches table entries (:307, before the observation filter) or none kept
 * -> no solve, h_camera untouched, zeroed summary (usable = 0); *h_n_used = the number of observations, or -1 for the
 * first gate.  The constraint arguments are rs_refine_pose_inertial's.  Two launches, one wait on the completion flag.
 * motion::is_rotation_plausible (:314) stays the caller's. */
int rs_map_refine_pose(rs_context* ctx, rs_map* map, const rs_frame* frame, double h_camera[6], const float h_intrinsics[4],
                       int min_matches, int kind, const double h_predicted[9], double sigma_radians,
                       const double h_prev_pose[6], const double h_prev_velocity[3], const double h_prev_bias[6],
                       const rs_imu_factor* h_delta, const double h_gravity[3], double h_velocity[3],
                       const rs_ba_options* options, rs_ba_summary* h_summary, int* h_n_used);

/* ------------------------------------------------------------------ a14: pose graph
 * optimization::pose_graph (src/Optimization.cpp:540-639), called once per detected loop (src/Slam.cpp:258-268).
 * HOST function (no GPU work, no context): a few hundred 6-residual edges whose sparse normal equations factor in a
 * short dependent chain; the reference runs Ceres' SPARSE_NORMAL_CHOLESKY on the CPU at the same place.  The
 * data-parallel part of a loop closure, moving the map points, is rs_transform_points below.
 *   h_poses [n_kf][16]     Frame::pose() of ALL key frames in index order (Mapper::key_frames())
 *   h_loops                PoseGraphConstraint: from / to = positions in that list, relative = measured
 *                          T_from T_to^-1, row-major; entries out of range or with from == to are skipped (:590-592)
 *   four_dof, h_gravity    yaw + position only, about up = -gravity / |gravity| (falls back to SE(3) when
 *                          |gravity|^2 < 1e-6, :550-557)
 *   options                NULL = Ceres defaults with PGO_ITERATIONS = 20 (:120)
 *   h_out_poses [n_kf][16] the corrected poses, written as apply_corrected_pose (:499-504) writes them; equal to the
 *                          input when summary.usable == 0 (<=> the reference returns false and changes nothing) and
 *                          for n_kf < 3 or no loops (:546-548).  May alias h_poses.
 *   h_velocity_rotation    optional [n_kf][9] row-major R_delta of :505-509 (the caller rotates
 *                          InertialState::velocity by it); identity where nothing moved
 *   h_trace                optional per-iteration record, as rs_ba_get_trace; *h_trace_count = iterations recorded */
typedef struct rs_pose_graph_edge {
    int32_t from, to;
    double relative[16];
} rs_pose_graph_edge;
int rs_pose_graph(int n_kf, const float* h_poses, const rs_pose_graph_edge* h_loops, int n_loops, int four_dof,
                  const double h_gravity[3], const rs_ba_options* options, float* h_out_poses,
                  float* h_velocity_rotation, rs_ba_summary* h_summary, rs_ba_iteration* h_trace, int trace_capacity,
                  int* h_trace_count);
/* pose_relative (:494-497): T_from (widened) * inverse(T_to) (f32 cofactor inverse, widened) — what the sequential
 * edges measure; exposed so that a caller can build loop constraints the same way. */
void rs_pose_relative(const float h_from[16], const float h_to[16], double h_relative[16]);
/* transform_points (:512-536) on the device: every point with observations moves rigidly with its owner, the
 * observing key frame of smallest index:  X' = R_after^T ((R_before X + t_before) - t_after), f32.
 * Observation CSR as in rs_map_view (d_obs_ptr [n_points + 1], d_obs_kf [.] = position in the key-frame list);
 * d_poses_before / d_poses_after [n_kf][16], 16-byte aligned. */
int rs_transform_points(rs_context* ctx, int n_points, const int32_t* d_obs_ptr, const int32_t* d_obs_kf,
                        const float* d_poses_before, const float* d_poses_after, int n_kf, float* d_positions);
/* pose_graph on the resident map: poses from the mirror (every key frame of the map, in handle order), rs_pose_graph,
 * and on a usable solve the key frames take the corrected poses and K14 moves the points on the device (the mirror
 * follows).  h_out_poses [n_kf][16] / h_velocity_rotation [n_kf][9] (optional) are for the caller's own objects;
 * returns summary.usable == 0 and changes nothing exactly when the reference returns false. */
int rs_map_pose_graph(rs_context* ctx, rs_map* map, const rs_pose_graph_edge* h_loops, int n_loops, int four_dof,
                      const double h_gravity[3], const rs_ba_options* options, float* h_out_poses,
                      float* h_velocity_rotation, rs_ba_summary* h_summary);

/* pack_pose / unpack_pose (src/Optimization.cpp:144-159, a10).  Host only:
 * R -> angle-axis in f32 through a quaternion (ceres::RotationMatrixToAngleAxis<float>),
 * centre = -R^T t (src/Frame.cpp:39-42), widened to f64; and back. */
void rs_pack_pose(const float h_pose[16], double h_camera[6]);
void rs_unpack_pose(const double h_camera[6], float h_pose[16]);
/* the loops around them (src/Optimization.cpp:273-282, 363-368); h_mask (NULL = all) selects the frames written */
void rs_pack_poses(const float* h_poses /*[n][16]*/, int n, double* h_cameras /*[n][6]*/);
void rs_unpack_poses(const double* h_cameras /*[n][6]*/, int n, const uint8_t* h_mask /*[n] or NULL*/, float* h_poses /*[n][16]*/);

/* ------------------------------------------------------- a8: local window */

/* optimization::build_local_window (src/LocalWindow.cpp:10-52).  Host only.
 * Keyframes are 0..n_key_frames-1 in Mapper order; new_frame is the index of
 * the new frame in that list, or -1 when it is not (yet) a keyframe.
 * The covisibility input is CSR: frame f matches points
 * h_frame_pt[h_frame_ptr[f] .. h_frame_ptr[f+1]-1]; rows 0..n_key_frames-1 are
 * the key frames (h_frame_ptr has n_key_frames + 1 entries) and, only when
 * new_frame == -1, row n_key_frames is the new frame (n_key_frames + 2
 * entries); point p is observed by
 * keyframes h_pt_obs[h_pt_ptr[p] .. h_pt_ptr[p+1]-1].
 * Output (capacity n_key_frames+1): h_out_frame[i] (n_key_frames = the new
 * non-keyframe), h_out_optimize[i]; *h_out_count entries. */
int rs_build_local_window(int n_key_frames, int new_frame, int window_size, int fix_oldest,
                          const int32_t* h_frame_ptr, const int32_t* h_frame_pt,
                          const int32_t* h_pt_ptr, const int32_t* h_pt_obs,
                          int32_t* h_out_frame, uint8_t* h_out_optimize, int32_t* h_out_count);

/* ------------------------------------------------------ KLT: track_features */

/* Tracker::track_features (src/Tracker.cpp:90-131; the same pattern Initialization.cpp:79-90): two pyramidal Lucas-Kanade
 * passes and the forward-backward filter, on device-resident image pyramids.  The specification is
 * cv::calcOpticalFlowPyrLK (Bouguet) as restated in tests/klt_ref.py, with one deliberate difference: window sums are
 * exact int64 sums converted to f32 once (OpenCV accumulates in f32; the difference is below f32 rounding of the sums).
 *
 * rs_image holds one frame: the grey level 0, the pyrDown levels (reflect-101) and their int16 Scharr derivatives,
 * every level padded by `win` (images reflect-101, derivatives zeros).  It is allocated once by rs_image_create and
 * reused by every upload: a tracker keeps two and swaps them, so each frame is uploaded once and its pyramid is the
 * "previous" image of the next frame.  Levels above the first whose size is <= win in either direction are not built
 * (buildOpticalFlowPyramid's clamp).  Envelope: width, height 1 .. 4096; win odd, 5 .. 31; max_level 0 .. 6;
 * up to 8192 points per call.  Outside it: RS_ERR_UNSUPPORTED. */
typedef struct rs_image rs_image;
int rs_image_create(rs_context* ctx, int width, int height, int max_level, int win, rs_image** out_img);
int rs_image_destroy(rs_image* img);
/* *h_levels = levels built (1 + the highest level); h_sizes [2 * levels] or NULL: (width, height) of every level. */
int rs_image_levels(const rs_image* img, int* h_levels, int* h_sizes);
/* One frame, row pitch in bytes, channels 1 (grey, passed through) or 3 (BGR: cv::cvtColor BGR2GRAY's 8-bit
 * fixed point, (1868 B + 9617 G + 4899 R + 8192) >> 14; to_gray, src/Tracker.cpp:24-32).  The host buffer may be reused
 * on return; the pyramid is built asynchronously on the context stream. */
int rs_image_upload(rs_context* ctx, rs_image* img, const uint8_t* h_pixels, int pitch, int channels);
/* The same for a frame already on the device (d_pixels must stay valid until the stream reaches this call). */
int rs_image_upload_device(rs_context* ctx, rs_image* img, const uint8_t* d_pixels, int pitch, int channels);
/* Diagnostic: the padded level `level`: h_img [(h+2 win)][(w+2 win)] u8 and / or h_deriv [(h+2 win)][(w+2 win)][2] int16
 * (dx, dy); either may be NULL.  Synchronises the stream. */
int rs_image_download(rs_context* ctx, const rs_image* img, int level, uint8_t* h_img, int16_t* h_deriv);
/* cv::calcOpticalFlowPyrLK(from, to, pts, next, status, noArray(), Size(win, win), max_level,
 * TermCriteria(COUNT + EPS, max_iter, eps), d_guess ? OPTFLOW_USE_INITIAL_FLOW : 0, min_eig) (src/Tracker.cpp:107-110):
 * d_pts [n][2], d_guess [n][2] or NULL, d_next [n][2], d_status [n] (1 = tracked).  Both images must come from
 * rs_image_create with the same size and window, win <= that window, max_iter 1 .. 100; the number of levels used is
 * min(max_level, the clamp for win), which both pyramids must have built. */
int rs_klt_track(rs_context* ctx, const rs_image* from, const rs_image* to, const float* d_pts, int n, const float* d_guess,
                 int win, int max_level, int max_iter, double eps, double min_eig, float* d_next, uint8_t* d_status);
/* Steps 2-4 of track_features in one launch + an ordered compaction (src/Tracker.cpp:107-126): forward LK prev -> next,
 * backward LK next -> prev from the forward result (window and levels of rs_image_create, 30 iterations, eps 0.01,
 * minEig 1e-4), then point i is kept iff both passes tracked it, |prev_i - back_i| <= fb_max (f32 difference, f64 norm,
 * cv::norm), (cvRound(next_i.x), cvRound(next_i.y)) lies inside the image and, with d_mask [height][width] u8 (the static
 * mask, NULL = none), the mask there is non-zero.  Outputs: d_kept_index [n] ascending, d_kept_pt [n][2] = next_i of each
 * kept point (capacity n each), d_count [1] (device) — exactly what feeds matches / features.keypoints at :128-131. */
int rs_track_features(rs_context* ctx, const rs_image* prev, const rs_image* next, const float* d_prev_pts, int n,
                      const uint8_t* d_mask, float fb_max, int32_t* d_kept_index, float* d_kept_pt, int32_t* d_count);

/* ------------------------------------------------- GFTT: feature replenishment */

/* The replenishment half of Tracker::track_features (src/Tracker.cpp:127-146) with the ORB extractor
 * (features/OrbFeatureExtractor.cpp:5-27: cv::GFTTDetector::create(3000, 0.005, 5), then cv::ORB::compute's border
 * filter; Initialization.cpp:47 and :105 call the same detector with the static mask alone), on level 0 of an rs_image.
 * The specification is cv::goodFeaturesToTrack(blockSize 3, gradientSize 3, useHarris false) as restated in
 * tests/gftt_ref.py, with one deliberate difference: the structure-tensor sums are exact integers (OpenCV: f32 sums of
 * dx, dy scaled by 1 / 3060).  ORB description is NOT done here: descriptors stay with the caller's extractor.
 *
 * rs_detector holds the scratch of one image size (allocated once; no allocation per call).  Envelope: width, height
 * 1 .. 4096 (an rs_image of the same size), max_corners 1 .. 8192, block_size = gradient_size = 3.  Outside it:
 * RS_ERR_UNSUPPORTED. */
typedef struct rs_detector rs_detector;
int rs_detector_create(rs_context* ctx, int width, int height, int max_corners, int block_size, int gradient_size,
                       rs_detector** out_det);
int rs_detector_destroy(rs_detector* det);
/* :127-146 in one call on the context stream, with no host synchronisation:
 *   replenish mask  d_mask [height][width] u8 (the static mask; NULL = all set) with cv::circle(.., cvRound(pt),
 *                   exclude_radius, 0, FILLED) (:131) at each of the d_exclude_count[0] points d_exclude_pt [][2]; both
 *                   are DEVICE pointers, exactly rs_track_features' d_kept_pt / d_count, and the count is read on the
 *                   device; both NULL = nothing excluded.
 *   detect          goodFeaturesToTrack(level 0, max_corners, quality, min_distance, replenish mask) (:138), then
 *                   runByImageBorder(border) (cv::ORB::compute: 31), order kept.
 *   budget          :140-146: max_total < 0 = no budget (Initialization), else max(0, max_total - d_exclude_count[0]).
 * Outputs (device): d_pt [max_corners][2] and d_response [max_corners] (the min-eigenvalue, KeyPoint::response) of the
 * detected corners strongest first; d_counts[0] = corners detected after the border filter (what the reference logs as
 * "replenished"), d_counts[1] = how many of them the budget appends (a prefix of the list).
 * Envelope: max_corners 1 .. the detector's, quality in (0, 1], min_distance 0 .. 16 (< 1: no distance filter),
 * exclude_radius 0 .. 16, border >= 0; up to 8192 excluded points are read. */
int rs_detect_features(rs_context* ctx, rs_detector* det, const rs_image* img, const uint8_t* d_mask, const float* d_exclude_pt,
                       const int32_t* d_exclude_count, int exclude_radius, int max_corners, double quality, double min_distance,
                       int border, int max_total, float* d_pt, float* d_response, int32_t* d_counts);
/* Diagnostic: cornerMinEigenVal(level 0, 3, 3) as restated (before the threshold), d_eig [height][width] f32 (device). */
int rs_corner_response(rs_context* ctx, rs_detector* det, const rs_image* img, float* d_eig);
/* Diagnostic of the last rs_detect_features on `det` (synchronises the stream): h_stats[5] = candidates, accepted by
 * the distance filter (uncapped), selection rounds used (0 without a filter), rounds run by the single-workgroup
 * finisher (0 when the fixed round launches sufficed), corners kept by the cap. */
int rs_detector_stats(rs_context* ctx, const rs_detector* det, int32_t* h_stats);

/* ------------------------------------------------- ORB: keypoint description */

/* The description stage of Tracker::track_features: OrbFeatureExtractor::refresh_descriptors
 * (features/OrbFeatureExtractor.cpp:29-61, called at src/Tracker.cpp:150), cv::ORB::compute with the ORB::create()
 * defaults (patch 31, WTA_K 2, one level) on keypoints of octave 0 and angle -1, on level 0 of an rs_image; with no
 * carried rows it is extract_features' compute (OrbFeatureExtractor.cpp:24; Initialization.cpp:47, :105).  The
 * specification is tests/orb_ref.py: GaussianBlur(7x7, sigma 2, reflect-101) in sepFilter2D's f32 form, the border
 * filter runByImageBorder(border) with cvRound'ed positions, and the 256 tests of OpenCV's bit_pattern_31_ at
 * (cvRound(x), cvRound(y)), bit k of byte i = test 8 i + k.  Results are bit-identical to it.  IC-angle orientation and
 * multi-octave keypoints are not implemented (the reference never uses them).
 *
 * rs_describer holds the blurred plane of one image size (allocated once; no allocation per call).  Envelope: width,
 * height 1 .. 4096 (an rs_image of the same size), max_points 1 .. 8192.  Outside it: RS_ERR_UNSUPPORTED. */
typedef struct rs_describer rs_describer;
int rs_describer_create(rs_context* ctx, int width, int height, int max_points, rs_describer** out_desc);
int rs_describer_destroy(rs_describer* d);
/* refresh_descriptors over list a followed by list b, in one pass on the context stream with no host synchronisation:
 *   list a   d_pt_a [][2] f32 and its count d_count_a[0] (DEVICE pointers, exactly rs_track_features' d_kept_pt /
 *            d_count); point i carries row d_carry_desc[d_carry_index[i]] (rs_track_features' d_kept_index and the
 *            previous frame's rows, :130), or row i when d_carry_index is NULL; n_carry = rows of d_carry_desc (an
 *            index outside [0, n_carry) carries zeros); d_carry_desc NULL (n_carry 0) = list a carries zeros.
 *   list b   d_pt_b [][2] f32 and its count d_count_b[0] (rs_detect_features' d_pt and d_counts + 1: the appended
 *            corners); they carry zeros (the zero rows of the caller edit, :142).
 *   Either list may be NULL (points and count together).  Counts are clamped: n_a = clamp(d_count_a[0], 0, max_points),
 *   n_b = clamp(d_count_b[0], 0, max_points - n_a); the caller's arrays hold at least that many points.
 * Outputs (device): d_desc [max_points][32] u8: row i < n_a + n_b is the fresh descriptor of point i (a_0 .. a_{n_a-1},
 * b_0 ..) when border <= cvRound(x) <= W-1-border and likewise for y (cvRound: half to even; non-finite points are
 * never kept), else the carried row; d_fresh [max_points] u8 (NULL = not written) = 1 for a fresh row; d_n[0] (NULL =
 * not written) = n_a + n_b.  Rows from n_a + n_b on are not written.  border: 31 in the reference (ORB's
 * edgeThreshold); envelope border >= 16 (the pattern's 13 px plus the blur's 3: no sample depends on the image
 * border's rule). */
int rs_describe_features(rs_context* ctx, rs_describer* d, const rs_image* img, const float* d_pt_a, const int32_t* d_count_a,
                         const int32_t* d_carry_index, const uint8_t* d_carry_desc, int n_carry, const float* d_pt_b,
                         const int32_t* d_count_b, int border, uint8_t* d_desc, uint8_t* d_fresh, int32_t* d_n);
/* Diagnostic: the blurred level 0 the descriptors sample, d_blur [height][width] u8 (device). */
int rs_orb_blur(rs_context* ctx, rs_describer* d, const rs_image* img, uint8_t* d_blur);

/* ------------------------------------------------- relative pose: essential-matrix RANSAC */

/* Tracker::initial_pose_estimate's pose::estimate_pose (src/PoseEstimation.cpp:59-88, with recover_pose_from_essential
 * :23-57; called at src/Tracker.cpp:162) and pose::estimate_pose_with_known_rotation (:110-227; Initialization.cpp:153).
 * The reference runs cv::findEssentialMat(USAC_ACCURATE, 0.99, 1.0 px), which cannot be restated bit for bit; the
 * specification is tests/essential_ref.py: hashed samples, Nister's five-point solver (Sturm bisection), integer
 * inlier counts (squared Sampson distance < t^2, t = threshold_px / ((fx + fy) / 2)), the adaptive stop after each
 * round of 256 hypotheses, up to 4 linear 8-point LO refits, decomposeEssentialMat on a one-sided Jacobi SVD and the
 * reference's cheirality vote (triangulate_points over EVERY finite match, 0.9999, 2.0 px; the first strict maximum).
 * Agreement with OpenCV's USAC is not claimed.  No nonlinear polish.
 *
 * rs_pose_estimator holds the scratch (allocated once; no allocation per call).  Envelope: max_points 1 .. 8192,
 * max_hypotheses 1 .. 4096.  Outside it: RS_ERR_UNSUPPORTED.  Creation synchronises the context stream only. */
typedef struct rs_pose_estimator rs_pose_estimator;
int rs_pose_estimator_create(rs_context* ctx, int max_points, int max_hypotheses, rs_pose_estimator** out_est);
int rs_pose_estimator_destroy(rs_pose_estimator* est);
/* One stream-ordered chain with no host synchronisation.  Inputs (device): the "from" pixels d_pts_from [][2] f32, read
 * as d_pts_from[d_from_index[i]] (rs_track_features' d_kept_index over the previous frame's points; a negative index
 * is a non-finite point; indices must lie inside the caller's array) or d_pts_from[i] when d_from_index is NULL; the
 * "to" pixels d_pts_to [][2] (rs_track_features' d_kept_pt); the count n = clamp(d_count[0], 0, max_n), read on the
 * device.  h_intrinsics = fx, fy, cx, cy.  Hypotheses h = 0 .. max_hypotheses-1 (<= the estimator's) in rounds of 256;
 * seed selects the samples.  Outputs (device): d_pose [16] f32 row-major (X_to = R X_from + t, |t| = 1),
 * d_inlier [max_n] u8 (entries from n on are 0), d_inlier_index [max_n] (ascending), d_inlier_count [1],
 * d_status [1]: 0 = ok, 1 = fewer than 5 points, 2 = no model with >= 5 inliers (both: identity pose, no inliers; the
 * reference would throw inside OpenCV).  A point with a non-finite coordinate is never sampled, never an inlier and
 * not triangulated. */
int rs_estimate_pose(rs_context* ctx, rs_pose_estimator* est, const float* d_pts_from, const int32_t* d_from_index,
                     const float* d_pts_to, const int32_t* d_count, int max_n, const float* h_intrinsics, double threshold_px,
                     double confidence, int max_hypotheses, uint64_t seed, float* d_pose, uint8_t* d_inlier,
                     int32_t* d_inlier_index, int32_t* d_inlier_count, int32_t* d_status);
/* estimate_pose_with_known_rotation (:110-227) in f32 with the same outputs: n points (host count), h_rotation [9]
 * row-major, d_pairs [n_iter][2] (the reference draws 200 with std::mt19937(0) and uniform_int_distribution<size_t>;
 * a pair with i == j, or an index outside [0, n), is skipped), max_epipolar_px (2.0 in the reference), focal = fx.
 * Status 1 = fewer than 8 points, 2 = best support below 8; both leave the pose [R | 0].  With fewer than 8 points no
 * pair is evaluated: rs_pose_estimator_stats reports drawn = 0 and rs_pose_hypotheses an all -1 table.  The refit takes the smallest
 * eigenvector of the f64 normal matrix of the inlier constraints (the reference: JacobiSVD of the stack).  n_iter
 * 1 .. the estimator's max_hypotheses. */
int rs_estimate_pose_known_rotation(rs_context* ctx, rs_pose_estimator* est, const float* d_pts_from, const int32_t* d_from_index,
                                    const float* d_pts_to, int n, const float* h_intrinsics, const float* h_rotation,
                                    const int32_t* d_pairs, int n_iter, float max_epipolar_px, float* d_pose, uint8_t* d_inlier,
                                    int32_t* d_inlier_index, int32_t* d_inlier_count, int32_t* d_status);
/* Diagnostic of the last call (synchronises the stream): h_stats[14] = hypotheses drawn, models scored, best index
 * (10 h + m; the pair index after the known-rotation form), best count, LO refits kept, the four cheirality counts
 * (known rotation: +t, -t, 0, 0), chosen candidate, status, inlier count, n, known-rotation flag; h_E [9] the final
 * E (f64, unit norm); h_candidates [4][16] f32 the decomposition's poses.  Any pointer may be NULL. */
int rs_pose_estimator_stats(rs_context* ctx, const rs_pose_estimator* est, int32_t* h_stats, double* h_E, float* h_candidates);
/* Diagnostic (synchronises) of the last call, over the estimator's whole table h < max_hypotheses (every call resets
 * it: nothing of an earlier call survives): h_samples [][5] (-1: not drawn, or a sample that could not find 5 distinct
 * finite points), h_nmodels [] (-1: not drawn), h_models [][10][9] f64 (row m valid for m < nmodels[h]) and
 * h_scores [][10] (0 past nmodels[h]).  After the known-rotation form: samples[h][0..1] = the pair (-1 past n_iter),
 * nmodels 1 = scored, 0 = skipped, -1 = past n_iter; the translation in models[h][0][0..2] when scored; the support
 * in scores[h][0] (-1: skipped or past n_iter).  Any pointer may be NULL. */
int rs_pose_hypotheses(rs_context* ctx, const rs_pose_estimator* est, int32_t* h_samples, int32_t* h_nmodels, double* h_models,
                       int32_t* h_scores);

/* ------------------------------------------------- absolute pose: P3P RANSAC with an EPnP refit */

/* The two cv::solvePnPRansac(..., 200, threshold, 0.99, inliers, cv::SOLVEPNP_EPNP) calls of the reference: LoopDetector's
 * verify_pnp (src/LoopDetector.cpp:176-229) and Initialization's third-view check (src/Initialization.cpp:188-228, 2.0 px).
 * OpenCV's RNG and RANSAC internals cannot be restated bit for bit; the specification is tests/pnp_ref.py: hashed
 * samples of 4, Grunert's P3P on the first three (the quartic's real roots by bisection between the roots of its
 * derivatives; the distance ratios polished by two Newton steps in the cosine laws, and taken from the third cosine
 * law where the quartic's quotient is 0 / 0; R, t from the orthonormal frames of the two triangles; at most 4 models
 * per sample, the first 4 in ascending root order), every model scored by its integer count of
 * points with positive depth and squared reprojection error < threshold_px^2, the adaptive stop after each round of
 * 256 hypotheses (sample size 4), and one EPnP refit (normalised coordinates; beta cases N = 1, 2, 3 with 5
 * Gauss-Newton steps each) over the best model's inliers when there are >= 6, kept iff its count over all points is
 * >= the minimal model's.  Agreement with cv::solvePnPRansac is not claimed.
 *
 * rs_pnp_estimator holds the scratch (allocated once; no allocation per call).  Envelope: max_points 1 .. 8192,
 * max_hypotheses 1 .. 4096.  Outside it: RS_ERR_UNSUPPORTED.  Creation synchronises the context stream only. */
typedef struct rs_pnp_estimator rs_pnp_estimator;
int rs_pnp_estimator_create(rs_context* ctx, int max_points, int max_hypotheses, rs_pnp_estimator** out_est);
int rs_pnp_estimator_destroy(rs_pnp_estimator* est);
/* One stream-ordered chain with no host synchronisation.  Inputs (device): correspondence i pairs the object point
 * d_object[d_object_index[i]] ([][3] f32, world) with the pixel d_pixels[d_pixel_index[i]] ([][2] f32); either index
 * array may be NULL (then i itself).  rs_match_descriptors' d_match_train / d_match_query / d_match_count serve as
 * d_object_index / d_pixel_index / d_count.  A negative index is a non-finite correspondence; indices must lie inside
 * the caller's arrays.  n = clamp(d_count[0], 0, max_n), read on the device.  h_intrinsics = fx, fy, cx, cy.
 * Hypotheses h = 0 .. max_hypotheses-1 (<= the estimator's; the reference passes 200) in rounds of 256; seed selects
 * the samples.  Outputs (device): d_pose [16] f32 row-major world -> camera (X_cam = R X + t), d_inlier [max_n] u8
 * (entries from n on are 0), d_inlier_index [max_n] (the first d_inlier_count entries, ascending; the entries from
 * d_inlier_count on are not written and keep what the caller had there), d_inlier_count [1], d_status [1]: 0 = ok, 1 = fewer
 * than 4 finite correspondences, 2 = no model with >= 4 inliers (both: identity pose, no inliers; the reference gets
 * solved == false).  A correspondence with a non-finite coordinate is never sampled, never an inlier, never refitted. */
int rs_estimate_pose_pnp(rs_context* ctx, rs_pnp_estimator* est, const float* d_object, const int32_t* d_object_index,
                         const float* d_pixels, const int32_t* d_pixel_index, const int32_t* d_count, int max_n,
                         const float* h_intrinsics, double threshold_px, double confidence, int max_hypotheses, uint64_t seed,
                         float* d_pose, uint8_t* d_inlier, int32_t* d_inlier_index, int32_t* d_inlier_count, int32_t* d_status);
/* Diagnostic of the last call (synchronises the stream): h_stats[9] = hypotheses drawn, models scored, best index
 * (4 h + m), best count, refit kept (0 / 1), the refit's beta case (1 .. 3; 0 = none), status, inlier count, n;
 * h_pose [12] the final [R | t] (f64, row-major 3 x 4; the identity unless status is 0).  Any pointer may be NULL. */
int rs_pnp_estimator_stats(rs_context* ctx, const rs_pnp_estimator* est, int32_t* h_stats, double* h_pose);
/* Diagnostic (synchronises) of the last call, over the estimator's whole table h < max_hypotheses (every call resets
 * it): h_samples [][4] (-1: not drawn, or a sample that could not find 4 distinct finite correspondences), h_nmodels []
 * (-1: not drawn), h_models [][4][12] f64 ([R | t]; row m valid for m < nmodels[h]) and h_scores [][4] (0 past
 * nmodels[h]).  Any pointer may be NULL. */
int rs_pnp_hypotheses(rs_context* ctx, const rs_pnp_estimator* est, int32_t* h_samples, int32_t* h_nmodels, double* h_models,
                      int32_t* h_scores);

/* ------------------------------------------------- key-frame recognition: vocabulary tree, BoW, L1 scores */

/* The "Loop retrieval" stage of LoopDetector::query (src/LoopDetector.cpp:346-373 score_candidates, :231-265
 * rank_candidates, timed at :492): a key frame's ORB rows descend the DBoW2 vocabulary tree to a bag-of-words vector
 * (thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1066-1122, :1218-1259; BowVector.cpp:34-84), which is scored against
 * every earlier key frame's vector (L1Scoring::score, ScoringObject.cpp:23-68).  The specification is tests/bow_ref.py.
 * Word ids, occurrence counts and word lists equal it exactly; values, norms and scores are f64 sums in a fixed order
 * (count x weight for TF_IDF / TF), within 2e-12 relative / 1e-11 absolute of it, and the same bytes on every run.
 * FeatureVector (levelsup), scoring types other than L1 and vocabulary training are not implemented.
 *
 * rs_vocabulary: a tree of n_nodes nodes.  Node 0 is the root; node i > 0 has h_parent[i] < i (h_parent[0] is ignored),
 * a 32-byte descriptor and an f64 weight.  A node's children are the nodes that name it as parent, in ascending node id
 * (loadFromTextFile's push_back order, :1338-1424); a node without children is a leaf; leaves are words 0 .. W-1 in
 * ascending node id.  weighting: 0 = TF_IDF, 1 = TF, 2 = IDF, 3 = BINARY; scoring: 0 = L1_NORM.  The tree need not be
 * complete: a leaf may sit above depth L and a node may have 1 .. k children.  Refused with RS_ERR_INVALID (the
 * reference would index out of range): a node with more than k children, a parent that is not below its node, an
 * unknown weighting and, in a text file, a leaf flag that contradicts the node's children or a malformed line; with
 * RS_ERR_UNSUPPORTED: a scoring type other than L1 and sizes outside the envelope k 1 .. 20, L 1 .. 10, n_nodes
 * 2 .. 4194304.  The arrays are copied; creation synchronises. */
typedef struct rs_vocabulary rs_vocabulary;
int rs_vocabulary_create(rs_context* ctx, int k, int L, int weighting, int scoring, int n_nodes, const int32_t* h_parent /*[n]*/,
                         const uint8_t* h_descriptors /*[n][32]*/, const double* h_weight /*[n]*/, rs_vocabulary** out_voc);
/* saveToTextFile's layout: line 1 "k L scoring weighting", then one line per node after the root, "parent is_leaf b0 ..
 * b31 weight" (node id = line number - 1).  Trailing blank lines are ignored: the extra node the reference's
 * while(!f.eof()) loop makes from the empty last line is not reproduced. */
int rs_vocabulary_load_text(rs_context* ctx, const char* path, rs_vocabulary** out_voc);
/* h_info[6] = k, L, weighting, scoring, nodes, words. */
int rs_vocabulary_info(const rs_vocabulary* voc, int32_t* h_info);
/* Diagnostic: the arrays as given (or as read), in node order; h_parent[0] = -1.  Any pointer may be NULL. */
int rs_vocabulary_arrays(const rs_vocabulary* voc, int32_t* h_parent, uint8_t* h_descriptors, double* h_weight);
int rs_vocabulary_destroy(rs_vocabulary* voc);

/* rs_bow holds the scratch of the transform and ONE resulting vector (allocated once; nothing is allocated per call),
 * for a vocabulary that outlives it.  Envelope: max_points 1 .. 8192; beyond: RS_ERR_UNSUPPORTED. */
typedef struct rs_bow rs_bow;
int rs_bow_create(rs_context* ctx, rs_vocabulary* voc, int max_points, rs_bow** out_bow);
int rs_bow_destroy(rs_bow* bow);
/* TemplatedVocabulary::transform of rows d_desc [][32] (device, 16-byte aligned), one stream-ordered chain with no host
 * synchronisation.  n = clamp(d_count[0], 0, min(max_n, max_points)) is read on the device: rs_describe_features'
 * d_desc and d_n serve as d_desc and d_count.  Every feature steps from the root to the child of smallest Hamming
 * distance (the first child among equals) until a leaf.  d_word [max_n] i32 (NULL = not written): the word of feature
 * i < n (a stopped word, weight <= 0, is still reported), -1 from n on.  The vector stays in the object, on the device:
 * the sorted unique words whose weight is > 0, their occurrence counts, their values (TF_IDF / TF: weight once per
 * occurrence, IDF / BINARY: the weight once; divided by their sum if it is > 0), the word count and that sum. */
int rs_bow_transform(rs_context* ctx, rs_bow* bow, const uint8_t* d_desc, const int32_t* d_count, int max_n, int32_t* d_word);
/* Diagnostic (synchronises the stream): the object's vector.  h_words, h_counts [max_points] i32, h_values [max_points]
 * f64 (the first *h_n_words entries are written), *h_norm the sum the values were divided by.  Any pointer may be NULL. */
int rs_bow_download(rs_context* ctx, const rs_bow* bow, int32_t* h_words, int32_t* h_counts, double* h_values,
                    int32_t* h_n_words, double* h_norm);

/* rs_bow_database: the vectors of the key frames so far, a packed CSR on the device (allocated once).  Envelope:
 * max_entries 1 .. 1048576, max_total_words 1 .. 2^30. */
typedef struct rs_bow_database rs_bow_database;
int rs_bow_database_create(rs_context* ctx, rs_vocabulary* voc, int max_entries, int max_total_words, rs_bow_database** out_db);
int rs_bow_database_destroy(rs_bow_database* db);
/* Appends the object's current vector as entry *h_entry (0, 1, ...) with device-to-device copies.  One 4-byte
 * read-back of the vector's word count synchronises the stream (as rs_frame_assign_device's does): the capacities are
 * checked on the host, and an entry or words that would not fit return RS_ERR_NOMEM with the database unchanged;
 * nothing is ever written past a capacity.  Where the reference computes bow_of lazily per candidate (:366-368), the
 * caller adds every key frame once. */
int rs_bow_database_add(rs_context* ctx, rs_bow_database* db, const rs_bow* bow, int32_t* h_entry);
/* L1Scoring::score of the object's vector against entries first .. first + count - 1: d_score [count] f64 (device), no
 * host synchronisation.  Over the words present in both vectors s = sum(|v - w| - |v| - |w|), the score is -s / 2: 0 in
 * magnitude when no word is shared, when the entry is empty or when the object's vector is. */
int rs_bow_database_score(rs_context* ctx, const rs_bow_database* db, const rs_bow* bow, int first, int count, double* d_score);
int rs_bow_database_counts(const rs_bow_database* db, int32_t* h_entries, int32_t* h_total_words);

/* LoopDetector's score_candidates gates and rank_candidates (src/LoopDetector.cpp:346-373, :231-265, percentile
 * :64-73).  Host only.  The query is key frame n_entries; h_score [n_entries] f64 are its scores against entries
 * 0 .. n_entries-1 (rs_bow_database_score), h_frame_index [n_entries] their frame indices.  Entry i is considered
 * unless n_entries - i < min_keyframe_gap or double(query_frame_index - h_frame_index[i]) * seconds_per_frame <
 * min_loop_seconds; its score is cast to float there.  threshold = max(min_score, median * peak_over_median) with
 * the median at index min(size - 1, size_t(0.5f * float(size - 1))) of the sorted considered scores; kept are the
 * considered entries at or above it that are not below either neighbour in the considered list (a missing neighbour
 * counts as 0), by descending score, equal scores in their considered order (the reference's std::sort leaves that
 * unspecified), the first `top` of them.  The reference's constants: min_keyframe_gap 50, min_loop_seconds 10.0,
 * min_score 0.02f, peak_over_median 1.25f, top 3.  Outputs: h_out_entry, h_out_score [top], *h_out_count; when nothing
 * is kept and something was considered, *h_rejected_entry / *h_rejected_score are the first considered entry of
 * greatest score (the one the reference prints), else -1 / 0. */
int rs_rank_loop_candidates(const double* h_score, const int64_t* h_frame_index, int n_entries, int64_t query_frame_index,
                            double seconds_per_frame, int min_keyframe_gap, double min_loop_seconds, float min_score,
                            float peak_over_median, int top, int32_t* h_out_entry, float* h_out_score, int32_t* h_out_count,
                            int32_t* h_rejected_entry, float* h_rejected_score);

/* ------------------------------------------------- loop verification against the resident map */

/* The "Loop verify" stage of LoopDetector::query (src/LoopDetector.cpp:501-506): verify_pnp (:176-229) of the query key
 * frame against each ranked candidate, both key frames of an rs_map.  The specification is tests/loop_ref.py, which
 * composes tests/match_ref.py and tests/pnp_ref.py.  Per candidate, as one stream-ordered chain:
 *   gather    the candidate's keypoints i with a map match (kp_point[i] >= 0), ascending i — Frame::map_matches() order
 *             (src/Frame.cpp:14, :100): descriptor row, point position, keypoint index, point slot;
 *   match     rs_match_descriptors of ALL the query key frame's rows against the gathered rows (MapMatcher::match_descriptors,
 *             src/MapMatcher.cpp:129-163);
 *   pose      rs_estimate_pose_pnp over the matches (object point = the matched row's point, pixel = the query keypoint),
 *             skipped on the device below 12 correspondences (MIN_PNP_CORRESPONDENCES, :183-186);
 *   verdict   status 1 = fewer than 12 correspondences, 2 = PnP status != 0 or no inliers (:215-218), 0 otherwise.  The
 *             listed correspondences are the PnP inliers (ascending) for status 0 and all correspondences otherwise (what
 *             the early returns hand to set_correspondences); correspondence j is (query keypoint, point slot, candidate
 *             keypoint).  For status 0, in f32 without contraction and in the reference's operation order (:146-174):
 *             spread = (max_x - min_x) / width over the listed query keypoints (0 with fewer than 2 or width <= 0), the
 *             recovered centre -R^T t, drift / gap = its distance to the query's / the candidate's centre,
 *             ok = inliers >= 20 && inliers / correspondences >= 0.35f && spread >= 0.25f.  For status 1 and 2: no inliers,
 *             ok false, spread, drift, gap 0 and the identity pose. */
typedef struct rs_loop_result {
    int32_t status, ok, correspondences, inliers, listed;
    float spread, drift, gap;
    float pose[16];                 /* row-major world -> camera */
} rs_loop_result;

/* rs_loop_verifier owns every buffer of max_candidates chains (gathered rows, match lists, one rs_pnp_estimator per
 * candidate and its outputs, one child context per candidate, a pinned result block): nothing is allocated per call.
 * Envelope: max_points 1 .. 8192 (keypoints of any key frame involved), max_candidates 1 .. 8, max_hypotheses 1 .. 4096;
 * outside it RS_ERR_UNSUPPORTED.  Creation synchronises the context stream. */
typedef struct rs_loop_verifier rs_loop_verifier;
int rs_loop_verifier_create(rs_context* ctx, int max_points, int max_candidates, int max_hypotheses, rs_loop_verifier** out_verifier);
int rs_loop_verifier_destroy(rs_loop_verifier* verifier);
/* Verifies h_candidate_kfs [n_candidates] (key frames of `map`; one may appear twice) against query_kf with ONE
 * synchronisation, at the end, for all of them.  h_intrinsics = fx, fy, cx, cy; width = the image width in pixels;
 * max_distance, threshold_px, confidence, max_hypotheses, seed as rs_match_descriptors / rs_estimate_pose_pnp take them
 * (the reference: 64, PNP_REPROJ_ERROR, 0.99, 200); every candidate uses the same seed.  Outputs (host):
 * h_result [n_candidates]; h_listed_query_kp / h_listed_point / h_listed_candidate_kp [n_candidates][max_points] i32 (row
 * stride = the verifier's max_points; the first h_result[c].listed entries of row c are written; any of the three may be
 * NULL).  n_candidates == 0 is valid and writes nothing.  RS_ERR_INVALID: a candidate equal to query_kf, a key frame that
 * does not exist or has more than max_points keypoints, n_candidates outside 0 .. max_candidates; RS_ERR_UNSUPPORTED:
 * max_hypotheses above the verifier's.  The context stays usable after every error.
 * "loop_verify_streams" (rs_context_set_int): 0 (default, the faster by measurement: 0.79 against 2.03 ms for three
 * candidates) one child context per candidate, forked from the context stream after the gather and joined before the
 * verdict; 1 every chain on the context stream, one after the other.  Both forms return the same bytes. */
int rs_map_verify_loop(rs_context* ctx, rs_loop_verifier* verifier, rs_map* map, int query_kf, const int32_t* h_candidate_kfs,
                       int n_candidates, const float* h_intrinsics, int width, int max_distance, double threshold_px,
                       double confidence, int max_hypotheses, uint64_t seed, rs_loop_result* h_result,
                       int32_t* h_listed_query_kp, int32_t* h_listed_point, int32_t* h_listed_candidate_kp);
/* Diagnostic of chain `candidate` of the last call (synchronises): *h_nt gathered rows; h_rows [nt][32] u8, h_slots,
 * h_keypoints [nt] i32 and h_positions [nt][3] f32 as gathered; the raw match lists h_match_query / h_match_train (the
 * first *h_match_count entries, at most the query's keypoints) and the PnP inlier index list h_inlier_index (the first
 * *h_inlier_count).  Arrays are sized by the caller for max_points entries; any pointer may be NULL. */
int rs_loop_verifier_download(rs_context* ctx, const rs_loop_verifier* verifier, int candidate, int32_t* h_nt, uint8_t* h_rows,
                              int32_t* h_slots, int32_t* h_keypoints, float* h_positions, int32_t* h_match_query,
                              int32_t* h_match_train, int32_t* h_match_count, int32_t* h_inlier_index, int32_t* h_inlier_count);

/* LoopDetector's best_candidate (src/LoopDetector.cpp:267-285) and Impl::update_streak (:375-442).  Host only.  The
 * caller keeps the constraints (from, to, relative pose, inlier pairs); the state is what update_streak reads of its
 * streak: its length and the last hit's query and candidate index. */
typedef struct rs_loop_streak {
    int32_t length;
    int64_t last_query, last_candidate;
} rs_loop_streak;
/* The verified candidate of most inliers (the first among equals); without a verified one, of most inliers; 0 for n == 1;
 * RS_ERR_INVALID for n < 1. */
int rs_loop_best_candidate(const rs_loop_result* h_results, int n, int32_t* h_best);
/* One query: `from` = the query's index among the key frames, h_candidate_index [n] the ranked candidates' indices,
 * h_results [n] their verdicts, h_constraint_from / h_constraint_to [n_constraints] the constraints so far.  n == 0 (nothing
 * ranked) clears the streak, as LoopDetector::query does (:495-499).  *h_chosen = the candidate that entered the streak
 * (-1: the streak was cleared and nothing entered); *h_new_constraint = 1 when the streak reached MIN_CONSISTENT = 3 and no
 * constraint lies within MIN_LOOP_SEPARATION = 15 of (from, h_candidate_index[chosen]) on both ends: the caller then
 * appends the constraint from -> h_candidate_index[chosen] with relative = pose * inverse(candidate pose) in f64 and the
 * chosen candidate's listed (keypoint, point) pairs.  CONSISTENCY_WINDOW = 15. */
int rs_loop_update_streak(rs_loop_streak* state, int64_t from, const int64_t* h_candidate_index, const rs_loop_result* h_results,
                          int n, const int64_t* h_constraint_from, const int64_t* h_constraint_to, int n_constraints,
                          int32_t* h_chosen, int32_t* h_new_constraint);

/* ------------------------------------------------------------- multi-GPU */

#define RS_COMM_ID_BYTES 128
/* One process per GPU.  Rank 0 calls rs_comm_get_unique_id, the host program
 * distributes the bytes (bench.py: torch.distributed broadcast), every rank
 * calls rs_comm_init_rank.  Only rs_bundle_adjust communicates (sum all-reduce
 * of the reduced camera system + cost over RCCL/xGMI); matching and
 * triangulation shard with no collective. */
int rs_comm_get_unique_id(uint8_t h_id[RS_COMM_ID_BYTES]);
int rs_comm_init_rank(rs_context* ctx, const uint8_t h_id[RS_COMM_ID_BYTES], int n_ranks, int rank);
int rs_comm_destroy(rs_context* ctx);
/* The same exchange step WITHOUT RCCL for n <= 8 contexts of one process (one host thread each, each with its own
 * stream, on one device or on peer-accessible devices): context i becomes rank i of an in-process group whose
 * all-reduce is a deterministic on-device sum in rank order.  Every member must then make the same sequence of
 * rs_bundle_adjust calls, each from its own thread.  Used to run landmark shards side by side on one GPU and to
 * test the N > 1 path on a one-GPU box.  rs_comm_destroy on every member releases the group.
 * A group in which an exchange step failed (a member's HIP error, or a member that did not arrive within 30 s) stays
 * failed: every later exchange step of every member returns RS_ERR_HIP at once ("... failed in an earlier exchange
 * step"); destroy the group on every member and create it again. */
int rs_comm_init_local(rs_context** ctxs, int n);
/* Evidence of what the exchange step runs over: *h_ranks = number of ranks of the attached communicator as RCCL
 * itself reports it (ncclCommCount) or the size of the in-process group; *h_kind = 0 none, 1 RCCL, 2 in-process. */
int rs_comm_count(rs_context* ctx, int* h_ranks, int* h_kind);

/* ------------------------------------------------------------- profiling */

/* Per-kernel HIP-event timing on the context's stream (the hipEvent analogue
 * of the reference's time_it(), src/Helpers.h:8-25).  Between begin and end
 * every kernel the library launches is bracketed by events; end synchronises
 * and returns the totals.  Kernel names are stable identifiers (K1..K9). */
#define RS_PROF_MAX 32
typedef struct rs_prof_entry {
    char name[32];
    int launches;
    double total_ms;
} rs_prof_entry;
int rs_prof_begin(rs_context* ctx);
int rs_prof_end(rs_context* ctx, rs_prof_entry* h_entries /*[RS_PROF_MAX]*/, int* h_count);
/* Diagnostic: shader-cycle totals per in-kernel phase of the last rs_bundle_adjust
 * call (thread 0 of workgroup 0 stamps s_memtime at phase boundaries; slots 0-6
 * K7, 8-14 K5).  n <= 64. */
int rs_prof_counters(rs_context* ctx, uint64_t* h_out, int n);
/* Launch latency of this device as the library's own launches see it ("state the measured empty-launch
 * latency next to the numbers"): n back-to-back launches of an empty one-workgroup kernel on the context stream
 * between two HIP events; *h_us = microseconds per launch. */
int rs_prof_empty_launch(rs_context* ctx, int n, double* h_us);

#ifdef __cplusplus
}
#endif
#endif /* RSGPU_H */
