"""ctypes binding of librsgpu.so (include/rsgpu.h) for the Python harness.

PyTorch is plumbing only here: device memory (torch tensors) and the stream.
Every call goes through the C-ABI; a missing library or a missing GPU raises —
there is no CPU fallback in the product path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RS_STAMPS=1 selects the instrumented build (tools/*_stamps.py); the product library otherwise
# RS_LIB=<file name in this directory> selects an A/B build (build.py, RS_VARIANT)
LIB_PATH = os.path.join(_HERE, os.environ.get("RS_LIB") or ("librsgpu_stamps.so" if os.environ.get("RS_STAMPS") else "librsgpu.so"))

EXPORTS = [
    "rs_abi_version", "rs_context_create", "rs_context_destroy", "rs_context_set_stream", "rs_context_wait_for", "rs_context_fork",
    "rs_context_synchronize", "rs_context_set_int", "rs_stage_begin", "rs_stage_alloc", "rs_stage_upload", "rs_stage_download", "rs_stage_sync", "rs_last_error", "rs_hamming_knn2", "rs_match_descriptors",
    "rs_l2_knn2", "rs_match_descriptors_f32", "rs_reproj_match_l2",
    "rs_kdtree_build", "rs_kdtree_pack", "rs_kdtree_grid_bytes", "rs_kdtree_grid_build", "rs_reproj_match", "rs_reproj_match_sharded", "rs_map_create", "rs_map_destroy", "rs_frame_create", "rs_frame_destroy",
    "rs_frame_create_device", "rs_frame_assign_device", "rs_frame_download",
    "rs_frame_matches_clear", "rs_frame_matches_add", "rs_frame_matches_download",
    "rs_map_set_track_consistent", "rs_map_carry_matches", "rs_map_refine_pose", "rs_map_match_frame",
    "rs_track_store_create", "rs_track_store_destroy", "rs_track_store_clear", "rs_track_store_carry", "rs_track_store_extend",
    "rs_track_store_query", "rs_needs_key_frame", "rs_track_store_triangulate", "rs_track_store_erase_inconsistent",
    "rs_track_store_download", "rs_track_store_download_packed",
    "rs_map_insert_keyframe", "rs_map_add_track_points", "rs_map_reanchor", "rs_map_cull_points",
    "rs_map_fuse_points", "rs_map_get_observations", "rs_map_get_keyframe_matches", "rs_map_fuse_loop",
    "rs_map_add_keyframe", "rs_map_set_keyframe_pose", "rs_map_add_point", "rs_map_set_position", "rs_map_remove_point",
    "rs_map_add_observation", "rs_map_remove_observation", "rs_map_counts", "rs_map_get_positions", "rs_map_match", "rs_map_pose_graph", "rs_pose_graph", "rs_pose_relative", "rs_transform_points", "rs_map_bundle_adjust", "rs_map_window", "rs_triangulate", "rs_triangulate_host", "rs_triangulate_matches", "rs_triangulate_matches_batch", "rs_triangulate_tracks", "rs_parallax_requirements", "rs_point_errors", "rs_ba_default_options",
    "rs_bundle_adjust", "rs_bundle_adjust_batch", "rs_ba_get_trace", "rs_ba_get_stats", "rs_ba_get_cameras", "rs_reanchor_points", "rs_reanchor_points_host_poses", "rs_refine_pose", "rs_bundle_adjust_inertial", "rs_refine_pose_inertial", "rs_pack_pose", "rs_unpack_pose", "rs_pack_poses", "rs_unpack_poses", "rs_build_local_window",
    "rs_image_create", "rs_image_destroy", "rs_image_levels", "rs_image_upload", "rs_image_upload_device", "rs_image_download",
    "rs_klt_track", "rs_track_features",
    "rs_detector_create", "rs_detector_destroy", "rs_detect_features", "rs_corner_response", "rs_detector_stats",
    "rs_describer_create", "rs_describer_destroy", "rs_describe_features", "rs_orb_blur",
    "rs_pose_estimator_create", "rs_pose_estimator_destroy", "rs_estimate_pose", "rs_estimate_pose_known_rotation",
    "rs_pose_estimator_stats", "rs_pose_hypotheses",
    "rs_pnp_estimator_create", "rs_pnp_estimator_destroy", "rs_estimate_pose_pnp", "rs_pnp_estimator_stats", "rs_pnp_hypotheses",
    "rs_vocabulary_create", "rs_vocabulary_load_text", "rs_vocabulary_info", "rs_vocabulary_arrays", "rs_vocabulary_destroy",
    "rs_bow_create", "rs_bow_destroy", "rs_bow_transform", "rs_bow_download",
    "rs_bow_database_create", "rs_bow_database_destroy", "rs_bow_database_add", "rs_bow_database_score", "rs_bow_database_counts",
    "rs_rank_loop_candidates",
    "rs_loop_verifier_create", "rs_loop_verifier_destroy", "rs_map_verify_loop", "rs_loop_verifier_download",
    "rs_loop_best_candidate", "rs_loop_update_streak",
    "rs_comm_get_unique_id", "rs_comm_init_rank", "rs_comm_destroy", "rs_comm_init_local", "rs_comm_count", "rs_prof_begin", "rs_prof_end", "rs_prof_counters", "rs_prof_empty_launch",
]

_lib = None


class RsError(RuntimeError):
    pass


def load():
    """Loads librsgpu.so.  torch is imported first so that the HIP runtime the
    library binds to (soname libamdhip64.so.7) is the one torch already mapped."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RsError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                          "(hipcc, gfx950); there is no CPU fallback")
        import torch  # noqa: F401
        _lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        _lib.rs_last_error.restype = C.c_char_p
        _lib.rs_last_error.argtypes = [C.c_void_p]
        if hasattr(_lib, "rs_kdtree_grid_bytes"):        # (an A/B library named by RS_LIB may predate the cell grid)
            _lib.rs_kdtree_grid_bytes.restype = C.c_size_t
        if hasattr(_lib, "rs_l2_knn2"):                  # the float-descriptor entries take a float by value: declared in full
            p, i, f = C.c_void_p, C.c_int, C.c_float
            _lib.rs_l2_knn2.argtypes = [p, p, i, p, i, i, i, p, p, p, p]
            _lib.rs_match_descriptors_f32.argtypes = [p, p, i, p, i, i, i, f, p, p, p, p, p, p, p]
            _lib.rs_reproj_match_l2.argtypes = [p, p, p, p, p, i, i, f, p, p, p, p, p, p, p]
    return _lib


class FrameView(C.Structure):
    _fields_ = [("pose", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("width", C.c_int), ("height", C.c_int), ("n_keypoints", C.c_int),
                ("d_keypoints", C.c_void_p), ("d_descriptors", C.c_void_p), ("d_kp_matched", C.c_void_p),
                ("d_kd_node_kp", C.c_void_p), ("d_kd_left", C.c_void_p), ("d_kd_right", C.c_void_p),
                ("kd_root", C.c_int), ("d_kd_packed", C.c_void_p), ("d_kd_grid", C.c_void_p)]


class MapView(C.Structure):
    _fields_ = [("n_points", C.c_int), ("d_positions", C.c_void_p), ("d_eligible", C.c_void_p),
                ("d_obs_ptr", C.c_void_p), ("d_obs_kf", C.c_void_p), ("d_obs_desc", C.c_void_p),
                ("d_kf_centers", C.c_void_p), ("d_desc_pool", C.c_void_p)]


class BaOptions(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int), ("huber_delta", C.c_double),
                ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double), ("max_num_consecutive_invalid_steps", C.c_int),
                ("jacobi_scaling", C.c_int)]


class BaSummary(C.Structure):
    _fields_ = [("termination", C.c_int), ("iterations", C.c_int), ("successful_steps", C.c_int),
                ("usable", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("final_radius", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BaIteration(C.Structure):
    _fields_ = [("cost", C.c_double), ("candidate_cost", C.c_double), ("model_cost_change", C.c_double),
                ("radius", C.c_double), ("step_norm", C.c_double), ("x_norm", C.c_double),
                ("outcome", C.c_int), ("reserved0", C.c_int), ("reserved1", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class ImuFactor(C.Structure):
    """rs_imu_factor"""
    _fields_ = [("cam_i", C.c_int), ("cam_j", C.c_int), ("duration", C.c_double), ("rotation", C.c_double * 9),
                ("velocity", C.c_double * 3), ("position", C.c_double * 3), ("covariance", C.c_double * 81),
                ("bias_gyro", C.c_double * 3), ("bias_accel", C.c_double * 3), ("bias_jacobian", C.c_double * 54),
                ("gyro_bias_sigma", C.c_double), ("accel_bias_sigma", C.c_double)]


def imu_factor_array(imu):
    """synth.make_imu(...) dict -> ctypes array of rs_imu_factor."""
    n = len(imu["cam_i"])
    arr = (ImuFactor * max(n, 1))()
    for f in range(n):
        a = arr[f]
        a.cam_i, a.cam_j, a.duration = int(imu["cam_i"][f]), int(imu["cam_j"][f]), float(imu["duration"][f])
        for name in ("rotation", "velocity", "position", "covariance", "bias_gyro", "bias_accel", "bias_jacobian"):
            getattr(a, name)[:] = list(np.asarray(imu[name][f], np.float64).ravel())
        a.gyro_bias_sigma, a.accel_bias_sigma = float(imu["gyro_bias_sigma"]), float(imu["accel_bias_sigma"])
    return arr, n


class BaProblem(C.Structure):
    """rs_ba_problem"""
    _fields_ = [("n_cameras", C.c_int), ("n_points", C.c_int), ("n_obs", C.c_int), ("d_cameras", C.c_void_p),
                ("h_cam_free", C.c_void_p), ("d_points", C.c_void_p), ("d_obs_ptr", C.c_void_p), ("d_obs_cam", C.c_void_p),
                ("d_obs_uv", C.c_void_p), ("intrinsics", C.c_float * 4)]


class ProfEntry(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int), ("total_ms", C.c_double)]


def default_options():
    o = BaOptions()
    load().rs_ba_default_options(C.byref(o))
    return o


def _dp(t):
    """device pointer of a torch tensor (or None).  Checked and boxed once per tensor object (cached on it: a
    benchmark pass makes ~60 of these conversions, at ~1 us each they rival the kernels they feed); tensors handed to
    the library must not be resized afterwards."""
    if t is None:
        return None
    p = t.__dict__.get("_rs_ptr")
    if p is None:
        assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA/HIP tensors"
        p = C.c_void_p(t.data_ptr())
        t._rs_ptr = p
    return p


# ---- host-only helpers (no GPU needed) ---------------------------------------
class PoseGraphEdge(C.Structure):
    """rs_pose_graph_edge"""
    _fields_ = [("from_", C.c_int32), ("to", C.c_int32), ("relative", C.c_double * 16)]


def pose_graph_edges(loops):
    """[(from, to, relative 4x4), ...] -> ctypes array of rs_pose_graph_edge"""
    arr = (PoseGraphEdge * max(len(loops), 1))()
    for i, (a, b, rel) in enumerate(loops):
        arr[i].from_, arr[i].to = int(a), int(b)
        arr[i].relative[:] = list(np.asarray(rel, np.float64).reshape(16))
    return arr


def pose_graph(poses, loops, four_dof=False, gravity=(0.0, 0.0, 0.0), options=None):
    """optimization::pose_graph (host function).  Returns (poses' [n,4,4] f32, velocity rotations [n,3,3] f32, summary, trace)."""
    P = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    out, rot = np.zeros_like(P), np.zeros((len(P), 9), np.float32)
    g = (C.c_double * 3)(*[float(v) for v in gravity])
    s = BaSummary()
    cap = 256
    buf = (BaIteration * cap)()
    cnt = C.c_int(0)
    L = load()
    L.rs_pose_graph.restype = C.c_int
    rc = L.rs_pose_graph(len(P), P.ctypes.data_as(C.c_void_p), pose_graph_edges(loops), len(loops), int(bool(four_dof)), g,
                         None if options is None else C.byref(options), out.ctypes.data_as(C.c_void_p),
                         rot.ctypes.data_as(C.c_void_p), C.byref(s), buf, cap, C.byref(cnt))
    if rc:
        raise RuntimeError(f"rs_pose_graph failed with {rc}")
    return out.reshape(-1, 4, 4), rot.reshape(-1, 3, 3), s.as_dict(), [buf[i].as_dict() for i in range(min(cnt.value, cap))]


def pose_relative(pose_from, pose_to):
    rel = np.zeros(16)
    a = np.ascontiguousarray(pose_from, np.float32).reshape(16)
    b = np.ascontiguousarray(pose_to, np.float32).reshape(16)
    load().rs_pose_relative(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), rel.ctypes.data_as(C.c_void_p))
    return rel.reshape(4, 4)


def pack_pose(pose):
    p = np.ascontiguousarray(pose, np.float32).reshape(16)
    cam = np.zeros(6)
    load().rs_pack_pose(p.ctypes.data_as(C.c_void_p), cam.ctypes.data_as(C.c_void_p))
    return cam


def unpack_pose(cam):
    c = np.ascontiguousarray(cam, np.float64)
    p = np.zeros(16, np.float32)
    load().rs_unpack_pose(c.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p))
    return p.reshape(4, 4)


_HOST_PTR = {}


def _hp(a):
    """Boxed address of a host array, cached per array object (ndarray.ctypes costs ~2 us a time; the per-frame calls of a
    pass hand the same few arrays over and over).  The cache keeps the array alive; arrays must not be resized."""
    e = _HOST_PTR.get(id(a))
    if e is None or e[0] is not a:
        if len(_HOST_PTR) > 256:
            _HOST_PTR.clear()
        e = _HOST_PTR[id(a)] = (a, C.c_void_p(a.ctypes.data))
    return e[1]


def unpack_poses(cams, mask, out):
    """In place: out [n][16] f32 rows of the frames selected by mask [n] u8 (None = all) are rewritten."""
    c = np.ascontiguousarray(cams, np.float64)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == 16 * len(c)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    load().rs_unpack_poses(_hp(c), len(c), None if m is None else _hp(m), _hp(out))
    return out


def parallax_requirements(poses, kf_pose, min_parallax_cosine=0.999848, rotation_parallax_factor=0.20):
    """rs_parallax_requirements (host, the host's libm): required parallax cosine per first-sighting pose [n] f32."""
    P = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    out = np.zeros(len(P), np.float32)
    rc = load().rs_parallax_requirements(P.ctypes.data_as(C.c_void_p), len(P), int(kf_pose), C.c_float(min_parallax_cosine),
                                         C.c_float(rotation_parallax_factor), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise RsError(f"rs_parallax_requirements -> {rc}")
    return out


def kdtree_build(keypoints):
    kp = np.ascontiguousarray(keypoints, np.float32)
    n = len(kp)
    node_kp = np.zeros(max(n, 1), np.int32)
    left = np.zeros(max(n, 1), np.int32)
    right = np.zeros(max(n, 1), np.int32)
    root = np.zeros(1, np.int32)
    rc = load().rs_kdtree_build(kp.ctypes.data_as(C.c_void_p), n, node_kp.ctypes.data_as(C.c_void_p),
                                left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p),
                                root.ctypes.data_as(C.c_void_p))
    if rc:
        raise RsError(f"rs_kdtree_build -> {rc}")
    return node_kp[:n], left[:n], right[:n], int(root[0])


def build_local_window(n_kf, new_frame, window, fix_oldest, frame_ptr, frame_pt, pt_ptr, pt_obs):
    a = [np.ascontiguousarray(x, np.int32) for x in (frame_ptr, frame_pt, pt_ptr, pt_obs)]
    of = np.zeros(n_kf + 1, np.int32)
    oo = np.zeros(n_kf + 1, np.uint8)
    cnt = np.zeros(1, np.int32)
    rc = load().rs_build_local_window(n_kf, new_frame, window, int(fix_oldest),
                                      *[x.ctypes.data_as(C.c_void_p) for x in a],
                                      of.ctypes.data_as(C.c_void_p), oo.ctypes.data_as(C.c_void_p),
                                      cnt.ctypes.data_as(C.c_void_p))
    if rc:
        raise RsError(f"rs_build_local_window -> {rc}")
    n = int(cnt[0])
    return of[:n].copy(), oo[:n].copy()


def rank_loop_candidates(scores, frame_index, query_frame_index, seconds_per_frame, min_keyframe_gap=50, min_loop_seconds=10.0,
                         min_score=0.02, peak_over_median=1.25, top=3):
    """rs_rank_loop_candidates (host): LoopDetector's gates and rank_candidates over the query's scores against every
    earlier entry.  dict(entries [<= top] i32, scores f32, rejected: (entry, score) of the best considered entry when
    nothing is kept and something was considered, else None).  The defaults are the reference's constants."""
    sc = np.ascontiguousarray(scores, np.float64)
    fi = np.ascontiguousarray(frame_index, np.int64)
    assert len(sc) == len(fi)
    oe, os_ = np.zeros(max(top, 1), np.int32), np.zeros(max(top, 1), np.float32)
    cnt, re_ = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rs_ = np.zeros(1, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)         # noqa: E731
    rc = load().rs_rank_loop_candidates(vp(sc), vp(fi), len(sc), C.c_int64(int(query_frame_index)), C.c_double(seconds_per_frame),
                                        int(min_keyframe_gap), C.c_double(min_loop_seconds), C.c_float(min_score),
                                        C.c_float(peak_over_median), int(top), vp(oe), vp(os_), vp(cnt), vp(re_), vp(rs_))
    if rc:
        raise RsError(f"rs_rank_loop_candidates -> {rc}")
    n = int(cnt[0])
    return dict(entries=oe[:n].copy(), scores=os_[:n].copy(), rejected=None if re_[0] < 0 else (int(re_[0]), rs_[0]))


class LoopResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("ok", C.c_int32), ("correspondences", C.c_int32), ("inliers", C.c_int32),
                ("listed", C.c_int32), ("spread", C.c_float), ("drift", C.c_float), ("gap", C.c_float), ("pose", C.c_float * 16)]


class LoopStreakState(C.Structure):
    _fields_ = [("length", C.c_int32), ("last_query", C.c_int64), ("last_candidate", C.c_int64)]


def _loop_results(verifications):
    arr = (LoopResult * max(len(verifications), 1))()
    for r, v in zip(arr, verifications):
        r.ok, r.inliers = int(bool(v["ok"])), int(v["inliers"])
    return arr


def loop_best_candidate(verifications):
    """rs_loop_best_candidate (host): LoopDetector's best_candidate over dicts with ok and inliers."""
    best = C.c_int32(-1)
    rc = load().rs_loop_best_candidate(_loop_results(verifications), len(verifications), C.byref(best))
    if rc:
        raise RsError(f"rs_loop_best_candidate -> {rc}")
    return best.value


def loop_update_streak(state, frm, candidate_index, verifications, constraints=()):
    """rs_loop_update_streak (host): one query of LoopDetector's update_streak.  state: a LoopStreakState (updated in
    place); candidate_index [n] the ranked candidates' key-frame indices; verifications [n] dicts with ok and inliers;
    constraints: (from, to) pairs so far.  Returns (chosen or -1, new_constraint bool)."""
    ci = np.ascontiguousarray(candidate_index, np.int64)
    cf = np.ascontiguousarray([c[0] for c in constraints], np.int64)
    ct = np.ascontiguousarray([c[1] for c in constraints], np.int64)
    assert len(ci) == len(verifications)
    chosen, new = C.c_int32(-1), C.c_int32(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)         # noqa: E731
    rc = load().rs_loop_update_streak(C.byref(state), C.c_int64(int(frm)), vp(ci), _loop_results(verifications), len(ci), vp(cf),
                                      vp(ct), len(cf), C.byref(chosen), C.byref(new))
    if rc:
        raise RsError(f"rs_loop_update_streak -> {rc}")
    return chosen.value, bool(new.value)


class LoopStreak:
    """The streak and the constraints of LoopDetector::Impl over rs_loop_update_streak (the Python form of
    slam::LoopStreak): update() per query, consume_new_loop() and constraints as the reference exposes them.  A constraint
    is dict(from, to, relative [4][4] f64 = pose * inverse(candidate pose), pairs [k][2] (query keypoint, point slot))."""

    def __init__(self):
        self.state, self.constraints, self._new = LoopStreakState(0, 0, 0), [], False

    def update(self, frm, candidate_index, verifications, candidate_poses):
        chosen, new = loop_update_streak(self.state, frm, candidate_index, verifications,
                                         [(c["from"], c["to"]) for c in self.constraints])
        if new:
            v = verifications[chosen]
            inv = np.linalg.inv(np.asarray(candidate_poses[chosen], np.float64).reshape(4, 4))
            self.constraints.append({"from": int(frm), "to": int(candidate_index[chosen]),
                                     "relative": np.asarray(v["pose"], np.float64).reshape(4, 4) @ inv,
                                     "pairs": np.stack([v["query_kp"], v["point"]], 1)})
            self._new = True
        return chosen

    def consume_new_loop(self):
        added, self._new = self._new, False
        return added


# ---- GPU context -------------------------------------------------------------
class Context:
    def __init__(self, device=0):
        import torch
        self.lib = load()
        self.torch = torch
        if not torch.cuda.is_available():
            raise RsError("no GPU visible: librsgpu has no CPU fallback")
        self.device = torch.device("cuda", device)
        self.h = C.c_void_p()
        rc = self.lib.rs_context_create(int(device), C.byref(self.h))
        if rc:
            raise RsError(f"rs_context_create -> {rc}")
        self.use_stream(torch.cuda.current_stream(self.device))

    def use_stream(self, stream):
        self._check(self.lib.rs_context_set_stream(self.h, C.c_void_p(stream.cuda_stream if stream is not None else None)), "set_stream")

    def wait_for(self, *others):
        """Everything enqueued on this context from now on waits for what is enqueued so far on `others` (no host wait)."""
        arr = self.__dict__.setdefault("_wait_arrays", {}).get(others)
        if arr is None:
            arr = self._wait_arrays[others] = (C.c_void_p * len(others))(*[o.h.value for o in others])
        self._check(self.lib.rs_context_wait_for(self.h, arr, len(others)), "rs_context_wait_for")

    def fork(self, *others):
        """Everything enqueued on `others` from now on waits for what is enqueued so far on this context (one event)."""
        arr = self.__dict__.setdefault("_wait_arrays", {}).get(others)
        if arr is None:
            arr = self._wait_arrays[others] = (C.c_void_p * len(others))(*[o.h.value for o in others])
        self._check(self.lib.rs_context_fork(self.h, arr, len(others)), "rs_context_fork")

    def set_int(self, name, value):
        self._check(self.lib.rs_context_set_int(self.h, name.encode(), int(value)), "rs_context_set_int")

    def close(self):
        if self.h:
            self.lib.rs_context_destroy(self.h)
            self.h = C.c_void_p()

    def _check(self, rc, what):
        if rc:
            msg = self.lib.rs_last_error(self.h)
            raise RsError(f"{what} -> status {rc}: {msg.decode() if msg else ''}")

    def dev(self, a, dtype=None):
        t = self.torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype)))
        return t.to(self.device)

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.device)

    # -- a4
    def hamming_knn2(self, d_query, d_train, nq, nt, batch=1):
        t = self.torch
        outs = [self.empty((batch, max(nq, 1)), t.int32) for _ in range(4)]
        self._check(self.lib.rs_hamming_knn2(self.h, _dp(d_query), nq, _dp(d_train), nt, batch,
                                             *[_dp(o) for o in outs]), "rs_hamming_knn2")
        return outs

    def match_descriptors(self, d_query, d_train, nq, nt, batch=1, max_distance=64, raw=False, out=None):
        t = self.torch
        if out is None:
            out = dict(mq=self.empty((batch, max(nq, 1)), t.int32), mt=self.empty((batch, max(nq, 1)), t.int32),
                       cnt=self.empty((batch,), t.int32))
            if raw:
                out["raw"] = [self.empty((batch, max(nq, 1)), t.int32) for _ in range(4)]
        rawp = [_dp(o) for o in out["raw"]] if "raw" in out else [None] * 4
        self._check(self.lib.rs_match_descriptors(self.h, _dp(d_query), nq, _dp(d_train), nt, batch,
                                                  int(max_distance), _dp(out["mq"]), _dp(out["mt"]),
                                                  _dp(out["cnt"]), *rawp), "rs_match_descriptors")
        return out

    # -- a2/a3
    def make_frame_view(self, frame, pack=False):
        """frame: dict of numpy arrays (synth.make_match_scene); returns (FrameView, keepalive)."""
        fv = FrameView()
        keep = {}
        fv.pose[:] = list(np.asarray(frame["pose"], np.float32).reshape(16))
        fv.fx, fv.fy, fv.cx, fv.cy = [float(v) for v in frame["K"]]
        fv.width, fv.height = int(frame["width"]), int(frame["height"])
        fv.n_keypoints = len(frame["keypoints"])
        for name, key, dt in (("d_keypoints", "keypoints", np.float32), ("d_descriptors", "descriptors", np.uint8),
                              ("d_kp_matched", "kp_matched", np.uint8), ("d_kd_node_kp", "kd_node_kp", np.int32),
                              ("d_kd_left", "kd_left", np.int32), ("d_kd_right", "kd_right", np.int32)):
            keep[name] = self.dev(frame[key], dt)
            setattr(fv, name, keep[name].data_ptr())
        fv.kd_root = int(frame["kd_root"])
        fv.d_kd_packed = None
        fv.d_kd_grid = None
        if pack and fv.n_keypoints > 0:        # once per frame: shared by the match calls of that frame
            keep["d_kd_packed"] = self.empty((5 * fv.n_keypoints,), self.torch.int32)
            self._check(self.lib.rs_kdtree_pack(self.h, C.byref(fv), _dp(keep["d_kd_packed"])), "rs_kdtree_pack")
            fv.d_kd_packed = keep["d_kd_packed"].data_ptr()
            if os.environ.get("RS_LIB") and not hasattr(self.lib, "rs_kdtree_grid_build"):
                return fv, keep
            # and its cell grid (rs_kdtree_grid_build): what K2 searches instead of walking the tree, where the tree allows it
            nbytes = self.lib.rs_kdtree_grid_bytes(fv.n_keypoints, fv.width, fv.height)
            keep["d_kd_grid"] = self.empty(((nbytes + 15) // 16 * 4,), self.torch.int32)
            self._check(self.lib.rs_kdtree_grid_build(self.h, C.byref(fv), _dp(keep["d_kd_grid"])), "rs_kdtree_grid_build")
            fv.d_kd_grid = keep["d_kd_grid"].data_ptr()
        return fv, keep

    def make_map_view(self, mp):
        mv = MapView()
        keep = {}
        mv.n_points = len(mp["positions"])
        for name, key, dt in (("d_positions", "positions", np.float32), ("d_eligible", "eligible", np.uint8),
                              ("d_obs_ptr", "obs_ptr", np.int32), ("d_obs_kf", "obs_kf", np.int32),
                              ("d_obs_desc", "obs_desc", np.int32), ("d_kf_centers", "kf_centers", np.float32),
                              ("d_desc_pool", "desc_pool", np.uint8)):
            keep[name] = self.dev(mp[key], dt)
            setattr(mv, name, keep[name].data_ptr())
        return mv, keep

    def reproj_match_sharded(self, fv, mv, point_base, replace=0, max_distance=64):
        """rs_reproj_match_sharded: mv is this rank's shard, point_base its first point's map order."""
        t = self.torch
        N, P = fv.n_keypoints, mv.n_points
        out = dict(point_kp=self.empty((max(P, 1),), t.int32), point_dist=self.empty((max(P, 1),), t.int32),
                   prop_point=self.empty((max(N, 1),), t.int32), prop_dist=self.empty((max(N, 1),), t.int32),
                   match_kp=self.empty((max(N, 1),), t.int32), match_point=self.empty((max(N, 1),), t.int32),
                   count=self.empty((1,), t.int32))
        self._check(self.lib.rs_reproj_match_sharded(self.h, C.byref(fv), C.byref(mv), int(point_base), int(replace), int(max_distance),
                                                     _dp(out["point_kp"]), _dp(out["point_dist"]), _dp(out["prop_point"]),
                                                     _dp(out["prop_dist"]), _dp(out["match_kp"]), _dp(out["match_point"]),
                                                     _dp(out["count"])), "rs_reproj_match_sharded")
        return out

    def reproj_match(self, fv, mv, replace=0, max_distance=64, out=None):
        t = self.torch
        N, P = fv.n_keypoints, mv.n_points
        if out is None:
            out = dict(point_kp=self.empty((max(P, 1),), t.int32), point_dist=self.empty((max(P, 1),), t.int32),
                       prop_point=self.empty((max(N, 1),), t.int32), prop_dist=self.empty((max(N, 1),), t.int32),
                       match_kp=self.empty((max(N, 1),), t.int32), match_point=self.empty((max(N, 1),), t.int32),
                       count=self.empty((1,), t.int32))
        self._check(self.lib.rs_reproj_match(self.h, C.byref(fv), C.byref(mv), int(replace), int(max_distance),
                                             _dp(out["point_kp"]), _dp(out["point_dist"]), _dp(out["prop_point"]),
                                             _dp(out["prop_dist"]), _dp(out["match_kp"]), _dp(out["match_point"]),
                                             _dp(out["count"])), "rs_reproj_match")
        return out

    # -- the same three for float descriptors under L2 (rows of `dim` f32)
    def l2_knn2(self, d_query, d_train, nq, nt, dim, batch=1):
        t = self.torch
        outs = [self.empty((batch, max(nq, 1)), dt) for dt in (t.int32, t.float32, t.int32, t.float32)]
        self._check(self.lib.rs_l2_knn2(self.h, _dp(d_query), nq, _dp(d_train), nt, int(dim), batch,
                                        *[_dp(o) for o in outs]), "rs_l2_knn2")
        return outs

    def match_descriptors_f32(self, d_query, d_train, nq, nt, dim, batch=1, max_distance=0.7, raw=False, out=None):
        t = self.torch
        if out is None:
            out = dict(mq=self.empty((batch, max(nq, 1)), t.int32), mt=self.empty((batch, max(nq, 1)), t.int32),
                       cnt=self.empty((batch,), t.int32))
            if raw:
                out["raw"] = [self.empty((batch, max(nq, 1)), dt) for dt in (t.int32, t.float32, t.int32, t.float32)]
        rawp = [_dp(o) for o in out["raw"]] if "raw" in out else [None] * 4
        self._check(self.lib.rs_match_descriptors_f32(self.h, _dp(d_query), nq, _dp(d_train), nt, int(dim), batch,
                                                      float(max_distance), _dp(out["mq"]), _dp(out["mt"]),
                                                      _dp(out["cnt"]), *rawp), "rs_match_descriptors_f32")
        return out

    def reproj_match_l2(self, fv, mv, d_frame_desc, d_desc_pool, dim, replace=0, max_distance=0.7, out=None):
        """rs_reproj_match_l2: fv / mv as for reproj_match (their u8 descriptor pointers are not read), the float rows
        of the frame's keypoints and of the pool that mv's d_obs_desc indexes."""
        t = self.torch
        N, P = fv.n_keypoints, mv.n_points
        if out is None:
            out = dict(point_kp=self.empty((max(P, 1),), t.int32), point_dist=self.empty((max(P, 1),), t.float32),
                       prop_point=self.empty((max(N, 1),), t.int32), prop_dist=self.empty((max(N, 1),), t.float32),
                       match_kp=self.empty((max(N, 1),), t.int32), match_point=self.empty((max(N, 1),), t.int32),
                       count=self.empty((1,), t.int32))
        self._check(self.lib.rs_reproj_match_l2(self.h, C.addressof(fv), C.addressof(mv), _dp(d_frame_desc), _dp(d_desc_pool),
                                                int(dim), int(replace), float(max_distance),
                                                _dp(out["point_kp"]), _dp(out["point_dist"]), _dp(out["prop_point"]),
                                                _dp(out["prop_dist"]), _dp(out["match_kp"]), _dp(out["match_point"]),
                                                _dp(out["count"])), "rs_reproj_match_l2")
        return out

    # -- a5-a7
    def triangulate(self, d_uv1, d_uv2, n, d_poses, n_poses, K, d_idx1=None, d_idx2=None,
                    min_parallax_cosine=0.9999, max_reproj=2.0, out=None):
        t = self.torch
        if out is None:
            out = dict(xyz=self.empty((max(n, 1), 3), t.float32), keep=self.empty((max(n, 1),), t.uint8),
                       out_index=self.empty((max(n, 1),), t.int32), out_xyz=self.empty((max(n, 1), 3), t.float32),
                       count=self.empty((1,), t.int32))
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self._check(self.lib.rs_triangulate(self.h, _dp(d_uv1), _dp(d_uv2), int(n), _dp(d_poses), int(n_poses),
                                            _dp(d_idx1), _dp(d_idx2), Kc, C.c_float(min_parallax_cosine),
                                            C.c_float(max_reproj), _dp(out["xyz"]), _dp(out["keep"]),
                                            _dp(out["out_index"]), _dp(out["out_xyz"]), _dp(out["count"])),
                    "rs_triangulate")
        return out

    def triangulate_host(self, uv1, uv2, pose1, pose2, K, min_parallax_cosine=0.9999, max_reproj=2.0):
        """rs_triangulate_host: numpy in, (match_index [m], xyz [m][3]) out; one launch for n <= 256."""
        a = np.ascontiguousarray(uv1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(uv2, np.float32).reshape(-1, 2)
        n = len(a)
        p1 = np.ascontiguousarray(pose1, np.float32).reshape(16)
        p2 = np.ascontiguousarray(pose2, np.float32).reshape(16)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        idx, xyz = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 3), np.float32)
        cnt = C.c_int(0)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
        self._check(self.lib.rs_triangulate_host(self.h, vp(a), vp(b), n, vp(p1), vp(p2), Kc, C.c_float(min_parallax_cosine),
                                                 C.c_float(max_reproj), vp(idx), vp(xyz), C.byref(cnt)), "rs_triangulate_host")
        return idx[:cnt.value].copy(), xyz[:cnt.value].copy()

    def triangulate_matches(self, d_kp1, d_kp2, d_mt, d_mq, d_cnt, max_matches, d_poses, K,
                            min_parallax_cosine=0.9999, max_reproj=2.0, out=None):
        t = self.torch
        n = max_matches
        if out is None:
            out = dict(xyz=self.empty((max(n, 1), 3), t.float32), keep=self.empty((max(n, 1),), t.uint8),
                       out_index=self.empty((max(n, 1),), t.int32), out_xyz=self.empty((max(n, 1), 3), t.float32),
                       count=self.empty((1,), t.int32))
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self._check(self.lib.rs_triangulate_matches(self.h, _dp(d_kp1), _dp(d_kp2), _dp(d_mt), _dp(d_mq), _dp(d_cnt),
                                                    int(n), _dp(d_poses), Kc, C.c_float(min_parallax_cosine),
                                                    C.c_float(max_reproj), _dp(out["xyz"]), _dp(out["keep"]),
                                                    _dp(out["out_index"]), _dp(out["out_xyz"]), _dp(out["count"])),
                    "rs_triangulate_matches")
        return out

    def triangulate_matches_batch(self, d_kp1, d_kp2, d_mt, d_mq, d_cnt, d_poses, K,
                                  min_parallax_cosine=0.9999, max_reproj=2.0, out=None):
        """cfg 4: d_kp1 [B][n1][2], d_kp2 [B][n2][2], d_mt / d_mq [B][stride], d_cnt [B], d_poses [B][2][16]."""
        t = self.torch
        B, n1, n2, stride = int(d_kp1.shape[0]), int(d_kp1.shape[1]), int(d_kp2.shape[1]), int(d_mt.shape[1])
        if out is None:
            out = dict(xyz=self.empty((B, stride, 3), t.float32), keep=self.empty((B, stride), t.uint8),
                       out_index=self.empty((B, stride), t.int32), out_xyz=self.empty((B, stride, 3), t.float32),
                       count=self.empty((B,), t.int32))
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self._check(self.lib.rs_triangulate_matches_batch(
            self.h, B, _dp(d_kp1), n1, _dp(d_kp2), n2, _dp(d_mt), _dp(d_mq), _dp(d_cnt), stride, _dp(d_poses), Kc,
            C.c_float(min_parallax_cosine), C.c_float(max_reproj), _dp(out["xyz"]), _dp(out["keep"]),
            _dp(out["out_index"]), _dp(out["out_xyz"]), _dp(out["count"])), "rs_triangulate_matches_batch")
        return out

    # -- §8(f) rank 1: Mapper::triangulate_tracks body
    def triangulate_tracks(self, d_track_uv, d_sight_ptr, d_sight_pose, d_sight_uv, d_poses, kf_pose, K, d_skip=None,
                           any_parallax_cosine=1.0, max_reproj=4.0, min_parallax_cosine=0.999848,
                           rotation_parallax_factor=0.20, min_new_points=100, out=None, d_required=None):
        t = self.torch
        n = int(d_track_uv.shape[0])
        m = max(n, 1)
        if out is None:
            out = dict(status=self.empty((m,), t.uint8), xyz=self.empty((m, 3), t.float32),
                       parallax_cos=self.empty((m,), t.float32), required_cos=self.empty((m,), t.float32),
                       accepted=self.empty((m,), t.int32), inconsistent=self.empty((m,), t.int32),
                       counts=self.empty((3,), t.int32))
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self._check(self.lib.rs_triangulate_tracks(
            self.h, n, _dp(d_track_uv), None if d_skip is None else _dp(d_skip), _dp(d_sight_ptr), _dp(d_sight_pose),
            _dp(d_sight_uv), _dp(d_poses), int(d_poses.shape[0]), int(kf_pose), Kc, C.c_float(any_parallax_cosine),
            C.c_float(max_reproj), C.c_float(min_parallax_cosine), C.c_float(rotation_parallax_factor),
            int(min_new_points), _dp(out["status"]), _dp(out["xyz"]), _dp(out["parallax_cos"]),
            _dp(out["required_cos"]), _dp(out["accepted"]), _dp(out["inconsistent"]), _dp(out["counts"]),
            None if d_required is None else _dp(d_required)),
            "rs_triangulate_tracks")
        return out

    # -- §8(f) rank 3: Mapper::cull_points / Slam::reprojection_error arithmetic
    def point_errors(self, d_positions, d_obs_ptr, d_obs_pose, d_obs_uv, d_poses, K, max_mean_error=3.0, out=None):
        t = self.torch
        n = int(d_positions.shape[0])
        m = max(n, 1)
        if out is None:
            out = dict(mean_err=self.empty((m,), t.float32), cull=self.empty((m,), t.uint8),
                       cull_idx=self.empty((m,), t.int32), cull_count=self.empty((1,), t.int32),
                       sums=self.empty((2,), t.float64))
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self._check(self.lib.rs_point_errors(self.h, n, _dp(d_positions), _dp(d_obs_ptr), _dp(d_obs_pose), _dp(d_obs_uv),
                                             _dp(d_poses), int(d_poses.shape[0]), Kc, C.c_float(max_mean_error),
                                             _dp(out["mean_err"]), _dp(out["cull"]), _dp(out["cull_idx"]),
                                             _dp(out["cull_count"]), _dp(out["sums"])), "rs_point_errors")
        return out

    # -- a9-a13
    def bundle_adjust(self, d_cams, cam_free, d_points, d_obs_ptr, d_obs_cam, d_obs_uv, K, options=None):
        cam_free = np.ascontiguousarray(cam_free, np.uint8)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        s = BaSummary()
        self._check(self.lib.rs_bundle_adjust(self.h, int(d_cams.shape[0]), int(d_points.shape[0]),
                                              int(d_obs_cam.shape[0]), _dp(d_cams),
                                              cam_free.ctypes.data_as(C.c_void_p), _dp(d_points), _dp(d_obs_ptr),
                                              _dp(d_obs_cam), _dp(d_obs_uv), Kc,
                                              None if options is None else C.byref(options), C.byref(s)),
                    "rs_bundle_adjust")
        return s.as_dict()

    def bundle_adjust_inertial(self, d_cams, cam_free, d_points, d_obs_ptr, d_obs_cam, d_obs_uv, K, imu, options=None):
        """rs_bundle_adjust_inertial; imu = synth.make_imu dict.  Returns (summary, velocity [C][3], bias [C][6])."""
        cam_free = np.ascontiguousarray(cam_free, np.uint8)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        vel = np.array(imu["cam_velocity"], np.float64, order="C")
        bias = np.array(imu["cam_bias"], np.float64, order="C")
        g = np.ascontiguousarray(imu["gravity"], np.float64)
        arr, nf = imu_factor_array(imu)
        s = BaSummary()
        self._check(self.lib.rs_bundle_adjust_inertial(
            self.h, int(d_cams.shape[0]), int(d_points.shape[0]), int(d_obs_cam.shape[0]), _dp(d_cams),
            cam_free.ctypes.data_as(C.c_void_p), _dp(d_points), _dp(d_obs_ptr), _dp(d_obs_cam), _dp(d_obs_uv), Kc,
            vel.ctypes.data_as(C.c_void_p), bias.ctypes.data_as(C.c_void_p), arr, nf, g.ctypes.data_as(C.c_void_p),
            None if options is None else C.byref(options), C.byref(s)), "rs_bundle_adjust_inertial")
        return s.as_dict(), vel, bias

    def refine_pose_inertial(self, cam, d_points, d_uv, K, prior=None, delta=None, options=None):
        """rs_refine_pose_inertial; prior = (predicted 3x3, sigma) or delta = dict(imu=<one-factor dict>, prev_pose,
        prev_velocity, prev_bias, velocity).  Returns cam, velocity, summary."""
        cam = np.array(cam, np.float64, order="C")
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        s = BaSummary()
        vel = np.zeros(3)
        vp = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)      # noqa: E731
        kind, pred, sigma, keep, args = 0, None, 0.0, [], [None, None, None, None, None]
        if prior is not None:
            kind, sigma = 1, float(prior[1])
            keep.append(np.ascontiguousarray(prior[0], np.float64))
            pred = keep[-1].ctypes.data_as(C.c_void_p)
        if delta is not None:
            kind = 2
            farr, _ = imu_factor_array(delta["imu"])
            keep += [np.ascontiguousarray(delta[k], np.float64) for k in ("prev_pose", "prev_velocity", "prev_bias")]
            keep.append(np.ascontiguousarray(delta["imu"]["gravity"], np.float64))
            vel = np.array(delta["velocity"], np.float64)
            args = [keep[-4].ctypes.data_as(C.c_void_p), keep[-3].ctypes.data_as(C.c_void_p), keep[-2].ctypes.data_as(C.c_void_p),
                    farr, keep[-1].ctypes.data_as(C.c_void_p)]
        del vp
        self._check(self.lib.rs_refine_pose_inertial(
            self.h, cam.ctypes.data_as(C.c_void_p), _dp(d_points), _dp(d_uv), int(d_points.shape[0]), Kc, kind, pred,
            C.c_double(sigma), args[0], args[1], args[2], args[3], args[4], vel.ctypes.data_as(C.c_void_p),
            None if options is None else C.byref(options), C.byref(s)), "rs_refine_pose_inertial")
        return cam, vel, s.as_dict()

    def bundle_adjust_batch(self, problems, options=None):
        """rs_bundle_adjust_batch; problems = list of (d_cams, cam_free, d_points, d_obs_ptr, d_obs_cam, d_obs_uv, K).
        Returns the list of summaries."""
        n = len(problems)
        arr = (BaProblem * max(n, 1))()
        keep = []
        for i, (dc, free, dp, optr, ocam, ouv, K) in enumerate(problems):
            f = np.ascontiguousarray(free, np.uint8)
            keep.append(f)
            a = arr[i]
            a.n_cameras, a.n_points, a.n_obs = int(dc.shape[0]), int(dp.shape[0]), int(ocam.shape[0])
            a.d_cameras, a.h_cam_free, a.d_points = dc.data_ptr(), f.ctypes.data, dp.data_ptr()
            a.d_obs_ptr, a.d_obs_cam, a.d_obs_uv = optr.data_ptr(), ocam.data_ptr(), ouv.data_ptr()
            a.intrinsics[:] = [float(v) for v in K]
        out = (BaSummary * max(n, 1))()
        self._check(self.lib.rs_bundle_adjust_batch(self.h, n, arr, None if options is None else C.byref(options), out),
                    "rs_bundle_adjust_batch")
        return [out[i].as_dict() for i in range(n)]

    def ba_trace(self):
        """Per-iteration record of the last bundle_adjust on this context (list of dicts)."""
        cap = 1024
        buf = (BaIteration * cap)()
        n = C.c_int(0)
        self._check(self.lib.rs_ba_get_trace(self.h, buf, cap, C.byref(n)), "rs_ba_get_trace")
        return [buf[i].as_dict() for i in range(min(n.value, cap))]

    def ba_cameras(self, out):
        """Cameras after the last bundle_adjust from the pinned mirror (no device read-back); out [C][6] f64."""
        assert out.dtype == np.float64 and out.flags.c_contiguous
        self._check(self.lib.rs_ba_get_cameras(self.h, _hp(out), int(out.shape[0])), "rs_ba_get_cameras")
        return out

    def ba_stats(self):
        buf = (C.c_int * 8)()
        self._check(self.lib.rs_ba_get_stats(self.h, buf), "rs_ba_get_stats")
        return dict(rounds=buf[0], fresh_rounds=buf[1], set_evaluations=buf[2], rounds_enqueued=buf[3], handoff_retries=buf[4])

    def reanchor_points(self, d_point_idx, d_frame_idx, d_before, d_after, d_positions):
        """Mapper::bundle_adjust's tail (src/Mapper.cpp:380-393); d_positions [P][3] f32 is updated in place."""
        n = int(d_frame_idx.shape[0])
        self._check(self.lib.rs_reanchor_points(self.h, n, None if d_point_idx is None else _dp(d_point_idx),
                                                _dp(d_frame_idx), _dp(d_before), _dp(d_after), int(d_before.shape[0]),
                                                _dp(d_positions)), "rs_reanchor_points")

    def reanchor_points_host_poses(self, d_point_idx, d_frame_idx, h_before, h_after, d_positions):
        """rs_reanchor_points with the poses in host arrays ([n_frames][16] f32, C order), as the reference holds them."""
        assert h_before.dtype == np.float32 and h_after.dtype == np.float32 and h_before.flags.c_contiguous and h_after.flags.c_contiguous
        n = int(d_frame_idx.shape[0])
        self._check(self.lib.rs_reanchor_points_host_poses(self.h, n, None if d_point_idx is None else _dp(d_point_idx),
                                                           _dp(d_frame_idx), _hp(h_before), _hp(h_after),
                                                           int(h_before.shape[0]), _dp(d_positions)), "rs_reanchor_points_host_poses")

    def transform_points(self, d_obs_ptr, d_obs_kf, d_before, d_after, d_positions):
        """transform_points of the pose graph (src/Optimization.cpp:512-536); d_positions [P][3] f32 is updated in place."""
        self._check(self.lib.rs_transform_points(self.h, int(d_positions.shape[0]), _dp(d_obs_ptr), _dp(d_obs_kf), _dp(d_before),
                                                 _dp(d_after), int(d_before.shape[0]), _dp(d_positions)), "rs_transform_points")

    def refine_pose(self, cam, d_points, d_uv, K, options=None):
        cam = np.array(cam, np.float64, order="C")
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        s = BaSummary()
        self._check(self.lib.rs_refine_pose(self.h, cam.ctypes.data_as(C.c_void_p), _dp(d_points), _dp(d_uv),
                                            int(d_points.shape[0]), Kc,
                                            None if options is None else C.byref(options), C.byref(s)),
                    "rs_refine_pose")
        return cam, s.as_dict()

    # -- multi-GPU
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        rc = load().rs_comm_get_unique_id(buf)
        if rc:
            raise RsError(f"rs_comm_get_unique_id -> {rc}")
        return bytes(buf)

    def comm_init(self, uid, n_ranks, rank):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self.lib.rs_comm_init_rank(self.h, buf, int(n_ranks), int(rank)), "rs_comm_init_rank")

    @staticmethod
    def comm_init_local(contexts):
        """In-process group: contexts[i] becomes rank i (see rs_comm_init_local)."""
        arr = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
        rc = load().rs_comm_init_local(arr, len(contexts))
        if rc:
            raise RsError(f"rs_comm_init_local -> {rc}")

    def comm_destroy(self):
        self._check(self.lib.rs_comm_destroy(self.h), "rs_comm_destroy")

    def comm_count(self):
        """(ranks as the communicator itself reports them, kind: 0 none / 1 RCCL / 2 in-process group)"""
        n, k = C.c_int(0), C.c_int(0)
        self._check(self.lib.rs_comm_count(self.h, C.byref(n), C.byref(k)), "rs_comm_count")
        return n.value, k.value

    # -- profiling
    def prof_begin(self):
        self._check(self.lib.rs_prof_begin(self.h), "rs_prof_begin")

    def prof_end(self):
        ent = (ProfEntry * 32)()
        n = C.c_int(0)
        self._check(self.lib.rs_prof_end(self.h, ent, C.byref(n)), "rs_prof_end")
        return {ent[i].name.decode(): (ent[i].launches, ent[i].total_ms) for i in range(n.value)}

    def prof_counters(self, n=16):
        buf = (C.c_uint64 * n)()
        self._check(self.lib.rs_prof_counters(self.h, buf, n), "rs_prof_counters")
        return list(buf)

    def empty_launch_us(self, n=2000):
        us = C.c_double(0.0)
        self._check(self.lib.rs_prof_empty_launch(self.h, int(n), C.byref(us)), "rs_prof_empty_launch")
        return us.value

    # -- KLT (Tracker::track_features)
    def image(self, width, height, max_level=4, win=21, frame=None):
        """rs_image: a device-resident pyramid (grow-free, reused across frames); `frame` (grey [h][w] or BGR [h][w][3]
        u8, numpy or a device tensor) is uploaded if given."""
        im = Image(self, width, height, max_level, win)
        if frame is not None:
            im.upload(frame)
        return im

    def klt_track(self, src, dst, d_pts, n, d_guess=None, win=21, max_level=4, max_iter=30, eps=0.01, min_eig=1e-4, out=None):
        """rs_klt_track (calcOpticalFlowPyrLK): dict(next [n][2] f32, status [n] u8), device tensors."""
        t = self.torch
        if out is None:
            out = dict(next=self.empty((max(n, 1), 2), t.float32), status=self.empty((max(n, 1),), t.uint8))
        self._check(self.lib.rs_klt_track(self.h, src.h, dst.h, _dp(d_pts), int(n), _dp(d_guess), int(win), int(max_level),
                                          int(max_iter), C.c_double(eps), C.c_double(min_eig), _dp(out["next"]),
                                          _dp(out["status"])), "rs_klt_track")
        return out

    def track_features(self, prev, nxt, d_pts, n, d_mask=None, fb_max=1.0, out=None):
        """rs_track_features (src/Tracker.cpp:107-126): dict(index [n] i32, pts [n][2] f32, count [1] i32), device
        tensors; the first count entries are the kept points."""
        t = self.torch
        if out is None:
            out = dict(index=self.empty((max(n, 1),), t.int32), pts=self.empty((max(n, 1), 2), t.float32),
                       count=self.empty((1,), t.int32))
        self._check(self.lib.rs_track_features(self.h, prev.h, nxt.h, _dp(d_pts), int(n), _dp(d_mask), C.c_float(fb_max),
                                               _dp(out["index"]), _dp(out["pts"]), _dp(out["count"])), "rs_track_features")
        return out

    # -- GFTT (Tracker::track_features' replenishment)
    def detector(self, width, height, max_corners=3000):
        """rs_detector: the scratch of the corner detector for one image size (allocated once, reused across frames)."""
        return Detector(self, width, height, max_corners)

    def detect_features(self, det, img, d_mask=None, d_exclude_pt=None, d_exclude_count=None, exclude_radius=5,
                        max_corners=3000, quality=0.005, min_distance=5.0, border=31, max_total=-1, out=None):
        """rs_detect_features (src/Tracker.cpp:127-146): dict(pts [max_corners][2] f32, response [max_corners] f32,
        counts [2] i32 = (detected, appended)), device tensors; the first counts[0] entries are the detected corners."""
        t = self.torch
        if out is None:
            out = dict(pts=self.empty((max_corners, 2), t.float32), response=self.empty((max_corners,), t.float32),
                       counts=self.empty((2,), t.int32))
        self._check(self.lib.rs_detect_features(self.h, det.h, img.h, _dp(d_mask), _dp(d_exclude_pt), _dp(d_exclude_count),
                                                int(exclude_radius), int(max_corners), C.c_double(quality),
                                                C.c_double(min_distance), int(border), int(max_total), _dp(out["pts"]),
                                                _dp(out["response"]), _dp(out["counts"])), "rs_detect_features")
        return out

    def corner_response(self, det, img, out=None):
        """rs_corner_response: the min-eigenvalue map [height][width] f32 (device) before the threshold."""
        if out is None:
            out = self.empty((det.height, det.width), self.torch.float32)
        self._check(self.lib.rs_corner_response(self.h, det.h, img.h, _dp(out)), "rs_corner_response")
        return out

    # -- ORB (Tracker::track_features' refresh_descriptors)
    def describer(self, width, height, max_points=8192):
        """rs_describer: the blurred plane of the ORB describer for one image size (allocated once, reused)."""
        return Describer(self, width, height, max_points)

    def describe_features(self, d, img, d_pt_a=None, d_count_a=None, d_carry_index=None, d_carry_desc=None, n_carry=0,
                          d_pt_b=None, d_count_b=None, border=31, out=None):
        """rs_describe_features (OrbFeatureExtractor::refresh_descriptors): dict(desc [max_points][32] u8,
        fresh [max_points] u8, n [1] i32), device tensors; the first n rows are list a's points then list b's."""
        t = self.torch
        if out is None:
            out = dict(desc=self.empty((d.max_points, 32), t.uint8), fresh=self.empty((d.max_points,), t.uint8),
                       n=self.empty((1,), t.int32))
        self._check(self.lib.rs_describe_features(self.h, d.h, img.h, _dp(d_pt_a), _dp(d_count_a), _dp(d_carry_index),
                                                  _dp(d_carry_desc), int(n_carry), _dp(d_pt_b), _dp(d_count_b), int(border),
                                                  _dp(out["desc"]), _dp(out["fresh"]), _dp(out["n"])), "rs_describe_features")
        return out

    def orb_blur(self, d, img, out=None):
        """rs_orb_blur: the blurred level 0 [height][width] u8 (device) that the descriptors sample."""
        if out is None:
            out = self.empty((d.height, d.width), self.torch.uint8)
        self._check(self.lib.rs_orb_blur(self.h, d.h, img.h, _dp(out)), "rs_orb_blur")
        return out

    # -- relative pose (Tracker::initial_pose_estimate)
    def pose_estimator(self, max_points=8192, max_hypotheses=1000):
        """rs_pose_estimator: the scratch of the relative-pose RANSAC (allocated once, reused)."""
        return PoseEstimator(self, max_points, max_hypotheses)

    def _pose_out(self, max_n, out):
        t = self.torch
        if out is None:
            m = max(int(max_n), 1)
            out = dict(pose=self.empty((4, 4), t.float32), inlier=self.empty((m,), t.uint8),
                       inlier_index=self.empty((m,), t.int32), inlier_count=self.empty((1,), t.int32),
                       status=self.empty((1,), t.int32))
        return out

    def estimate_pose(self, est, d_from, d_to, d_count, max_n, K, d_from_index=None, threshold_px=1.0, confidence=0.99,
                      max_hypotheses=1000, seed=0, out=None):
        """rs_estimate_pose (pose::estimate_pose): dict(pose [4][4] f32, inlier [max_n] u8, inlier_index [max_n] i32,
        inlier_count [1], status [1]), device tensors; d_count is a device [1] i32."""
        out = self._pose_out(max_n, out)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self._check(self.lib.rs_estimate_pose(self.h, est.h, _dp(d_from), _dp(d_from_index), _dp(d_to), _dp(d_count),
                                              int(max_n), Kc, C.c_double(threshold_px), C.c_double(confidence),
                                              int(max_hypotheses), C.c_uint64(int(seed) & (2 ** 64 - 1)), _dp(out["pose"]),
                                              _dp(out["inlier"]), _dp(out["inlier_index"]), _dp(out["inlier_count"]),
                                              _dp(out["status"])), "rs_estimate_pose")
        return out

    def estimate_pose_known_rotation(self, est, d_from, d_to, n, K, R, d_pairs, n_iter, d_from_index=None,
                                     max_epipolar_px=2.0, out=None):
        """rs_estimate_pose_known_rotation (pose::estimate_pose_with_known_rotation); outputs as estimate_pose."""
        out = self._pose_out(n, out)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        Rc = (C.c_float * 9)(*[float(v) for v in np.asarray(R, np.float32).ravel()])
        self._check(self.lib.rs_estimate_pose_known_rotation(
            self.h, est.h, _dp(d_from), _dp(d_from_index), _dp(d_to), int(n), Kc, Rc, _dp(d_pairs), int(n_iter),
            C.c_float(max_epipolar_px), _dp(out["pose"]), _dp(out["inlier"]), _dp(out["inlier_index"]),
            _dp(out["inlier_count"]), _dp(out["status"])), "rs_estimate_pose_known_rotation")
        return out

    # -- absolute pose (LoopDetector's verify_pnp, Initialization's third-view check)
    def pnp_estimator(self, max_points=8192, max_hypotheses=1000):
        """rs_pnp_estimator: the scratch of the absolute-pose RANSAC (allocated once, reused)."""
        return PnpEstimator(self, max_points, max_hypotheses)

    def estimate_pose_pnp(self, est, d_object, d_pixels, d_count, max_n, K, d_object_index=None, d_pixel_index=None,
                          threshold_px=2.0, confidence=0.99, max_hypotheses=200, seed=0, out=None):
        """rs_estimate_pose_pnp: dict(pose [4][4] f32 world -> camera, inlier [max_n] u8, inlier_index [max_n] i32,
        inlier_count [1], status [1]), device tensors; d_count is a device [1] i32."""
        out = self._pose_out(max_n, out)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self._check(self.lib.rs_estimate_pose_pnp(self.h, est.h, _dp(d_object), _dp(d_object_index), _dp(d_pixels),
                                                  _dp(d_pixel_index), _dp(d_count), int(max_n), Kc, C.c_double(threshold_px),
                                                  C.c_double(confidence), int(max_hypotheses),
                                                  C.c_uint64(int(seed) & (2 ** 64 - 1)), _dp(out["pose"]), _dp(out["inlier"]),
                                                  _dp(out["inlier_index"]), _dp(out["inlier_count"]), _dp(out["status"])),
                    "rs_estimate_pose_pnp")
        return out

    # -- key-frame recognition (LoopDetector's "Loop retrieval")
    def vocabulary(self, k, L, weighting, scoring, parent, desc, weight):
        """rs_vocabulary from host arrays in node order (parent [n] i32, desc [n][32] u8, weight [n] f64)."""
        return Vocabulary(self, k, L, weighting, scoring, parent, desc, weight)

    def vocabulary_from_text(self, path):
        return Vocabulary(self, path=path)

    def bow(self, voc, max_points=8192):
        """rs_bow: the transform's scratch and one resulting vector."""
        return Bow(self, voc, max_points)

    def bow_database(self, voc, max_entries, max_total_words):
        return BowDatabase(self, voc, max_entries, max_total_words)

    # -- loop verification (LoopDetector's "Loop verify")
    def loop_verifier(self, max_points=8192, max_candidates=3, max_hypotheses=200):
        """rs_loop_verifier: every buffer of max_candidates verify_pnp chains (allocated once, reused)."""
        return LoopVerifier(self, max_points, max_candidates, max_hypotheses)

    def synchronize(self):
        self._check(self.lib.rs_context_synchronize(self.h), "rs_context_synchronize")


class Image:
    """rs_image: one frame's padded pyramid and Scharr derivatives on the device."""

    def __init__(self, ctx, width, height, max_level=4, win=21):
        self.ctx, self.width, self.height, self.win = ctx, int(width), int(height), int(win)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.rs_image_create(ctx.h, self.width, self.height, int(max_level), self.win, C.byref(self.h)),
                   "rs_image_create")

    def upload(self, frame):
        """grey [h][w] or BGR [h][w][3] u8, numpy or a device tensor.  Rows may lie further apart than w * channels bytes
        (a view into a wider buffer, as a cv::Mat ROI hands over): that row stride is passed as the pitch."""
        ch = 1 if frame.ndim == 2 else int(frame.shape[2])
        inner, row = ((1,) if frame.ndim == 2 else (ch, 1)), int(frame.shape[1]) * ch
        if isinstance(frame, np.ndarray):
            a = frame
            if a.dtype != np.uint8 or a.strides[1:] != inner or a.strides[0] < row:
                a = np.ascontiguousarray(a, np.uint8)
            self.ctx._check(self.ctx.lib.rs_image_upload(self.ctx.h, self.h, a.ctypes.data_as(C.c_void_p), a.strides[0], ch),
                            "rs_image_upload")
        else:
            t = frame
            if tuple(t.stride()[1:]) != inner or t.stride(0) < row:
                t = t.contiguous()
            assert t.is_cuda and t.dtype == self.ctx.torch.uint8
            self.ctx._check(self.ctx.lib.rs_image_upload_device(self.ctx.h, self.h, C.c_void_p(t.data_ptr()), int(t.stride(0)), ch),
                            "rs_image_upload_device")
        return self

    def levels(self):
        n = C.c_int(0)
        sizes = (C.c_int * 16)()
        self.ctx._check(self.ctx.lib.rs_image_levels(self.h, C.byref(n), sizes), "rs_image_levels")
        return [(sizes[2 * i], sizes[2 * i + 1]) for i in range(n.value)]

    def download(self, level):
        """padded level: (img [h+2win][w+2win] u8, dx, dy [h+2win][w+2win] int16)"""
        w, h = self.levels()[level]
        img = np.zeros((h + 2 * self.win, w + 2 * self.win), np.uint8)
        der = np.zeros((h + 2 * self.win, w + 2 * self.win, 2), np.int16)
        self.ctx._check(self.ctx.lib.rs_image_download(self.ctx.h, self.h, int(level), img.ctypes.data_as(C.c_void_p),
                                                       der.ctypes.data_as(C.c_void_p)), "rs_image_download")
        return img, der[..., 0].copy(), der[..., 1].copy()

    def close(self):
        if self.h:
            self.ctx.lib.rs_image_destroy(self.h)
            self.h = C.c_void_p()


class Detector:
    """rs_detector: the corner detector's device scratch for one image size."""

    def __init__(self, ctx, width, height, max_corners=3000):
        self.ctx, self.width, self.height, self.max_corners = ctx, int(width), int(height), int(max_corners)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.rs_detector_create(ctx.h, self.width, self.height, self.max_corners, 3, 3, C.byref(self.h)),
                   "rs_detector_create")

    def stats(self):
        """Diagnostic of the last detect_features: dict(candidates, accepted, rounds, finisher_rounds, capped)."""
        s = (C.c_int32 * 5)()
        self.ctx._check(self.ctx.lib.rs_detector_stats(self.ctx.h, self.h, s), "rs_detector_stats")
        return dict(zip(("candidates", "accepted", "rounds", "finisher_rounds", "capped"), list(s)))

    def close(self):
        if self.h:
            self.ctx.lib.rs_detector_destroy(self.h)
            self.h = C.c_void_p()


class Describer:
    """rs_describer: the ORB describer's device plane for one image size."""

    def __init__(self, ctx, width, height, max_points=8192):
        self.ctx, self.width, self.height, self.max_points = ctx, int(width), int(height), int(max_points)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.rs_describer_create(ctx.h, self.width, self.height, self.max_points, C.byref(self.h)),
                   "rs_describer_create")

    def close(self):
        if self.h:
            self.ctx.lib.rs_describer_destroy(self.h)
            self.h = C.c_void_p()


class _RansacEstimator:
    """The device scratch of a RANSAC stage.  PREFIX names its rs_<PREFIX>_estimator_* / rs_<PREFIX>_hypotheses exports;
    SHAPE = (S, M, D): indices per sample, models per hypothesis, doubles per model."""

    def __init__(self, ctx, max_points=8192, max_hypotheses=1000):
        self.ctx, self.max_points, self.max_hypotheses = ctx, int(max_points), int(max_hypotheses)
        self.h = C.c_void_p()
        name = f"rs_{self.PREFIX}_estimator_create"
        ctx._check(getattr(ctx.lib, name)(ctx.h, self.max_points, self.max_hypotheses, C.byref(self.h)), name)

    def hypotheses(self):
        """Diagnostic of the last call: dict(samples [H][S], nmodels [H], models [H][M][D] f64, scores [H][M])."""
        H, (S, M, D) = self.max_hypotheses, self.SHAPE
        out = dict(samples=np.zeros((H, S), np.int32), nmodels=np.zeros(H, np.int32), models=np.zeros((H, M, D)),
                   scores=np.zeros((H, M), np.int32))
        name = f"rs_{self.PREFIX}_hypotheses"
        self.ctx._check(getattr(self.ctx.lib, name)(self.ctx.h, self.h, *[out[k].ctypes.data_as(C.c_void_p) for k in
                                                                          ("samples", "nmodels", "models", "scores")]), name)
        return out

    def close(self):
        if self.h:
            getattr(self.ctx.lib, f"rs_{self.PREFIX}_estimator_destroy")(self.h)
            self.h = C.c_void_p()


class PoseEstimator(_RansacEstimator):
    """rs_pose_estimator: the relative-pose RANSAC's device scratch; hypotheses(): samples [H][5], models [H][10][9]."""

    PREFIX, SHAPE = "pose", (5, 10, 9)
    STATS = ("drawn", "scored", "best_index", "best_count", "lo_kept", "cheir0", "cheir1", "cheir2", "cheir3", "chosen",
             "status", "inliers", "n", "known")

    def stats(self):
        """Diagnostic of the last call: dict of STATS, cheir [4], E [9] f64, candidates [4][4][4] f32."""
        s = np.zeros(14, np.int32)
        E = np.zeros(9, np.float64)
        cand = np.zeros((4, 4, 4), np.float32)
        self.ctx._check(self.ctx.lib.rs_pose_estimator_stats(self.ctx.h, self.h, s.ctypes.data_as(C.c_void_p),
                                                             E.ctypes.data_as(C.c_void_p), cand.ctypes.data_as(C.c_void_p)),
                        "rs_pose_estimator_stats")
        d = {k: int(v) for k, v in zip(self.STATS, s)}
        d.update(cheir=[d["cheir0"], d["cheir1"], d["cheir2"], d["cheir3"]], E=E, candidates=cand)
        return d


class PnpEstimator(_RansacEstimator):
    """rs_pnp_estimator: the absolute-pose RANSAC's device scratch; hypotheses(): samples [H][4], models [H][4][12]."""

    PREFIX, SHAPE = "pnp", (4, 4, 12)
    STATS = ("drawn", "scored", "best_index", "best_count", "refit_kept", "beta_case", "status", "inliers", "n")

    def stats(self):
        """Diagnostic of the last call: dict of STATS and Rt [12] f64, the final [R | t]."""
        s = np.zeros(9, np.int32)
        Rt = np.zeros(12, np.float64)
        self.ctx._check(self.ctx.lib.rs_pnp_estimator_stats(self.ctx.h, self.h, s.ctypes.data_as(C.c_void_p),
                                                            Rt.ctypes.data_as(C.c_void_p)), "rs_pnp_estimator_stats")
        d = {k: int(v) for k, v in zip(self.STATS, s)}
        d.update(Rt=Rt)
        return d


# ---- §8(f) rank 4: the resident map (rs_map / rs_frame) -----------------------------------------------------
class Vocabulary:
    """rs_vocabulary: the DBoW2 tree on the device (children contiguous, top levels first)."""

    def __init__(self, ctx, k=0, L=0, weighting=0, scoring=0, parent=None, desc=None, weight=None, path=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        if path is not None:
            ctx._check(ctx.lib.rs_vocabulary_load_text(ctx.h, os.fsencode(path), C.byref(self.h)), "rs_vocabulary_load_text")
        else:
            p = np.ascontiguousarray(parent, np.int32)
            d = np.ascontiguousarray(desc, np.uint8)
            w = np.ascontiguousarray(weight, np.float64)
            assert d.size == 32 * len(p) and len(w) == len(p)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)         # noqa: E731
            ctx._check(ctx.lib.rs_vocabulary_create(ctx.h, int(k), int(L), int(weighting), int(scoring), len(p), vp(p), vp(d), vp(w),
                                                    C.byref(self.h)), "rs_vocabulary_create")
        self.__dict__.update(self.info())

    def info(self):
        v = (C.c_int32 * 6)()
        self.ctx._check(self.ctx.lib.rs_vocabulary_info(self.h, v), "rs_vocabulary_info")
        return dict(zip(("k", "L", "weighting", "scoring", "n_nodes", "n_words"), list(v)))

    def arrays(self):
        """(parent [n] i32, desc [n][32] u8, weight [n] f64) as given or read, in node order."""
        n = self.n_nodes
        p, d, w = np.zeros(n, np.int32), np.zeros((n, 32), np.uint8), np.zeros(n, np.float64)
        self.ctx._check(self.ctx.lib.rs_vocabulary_arrays(self.h, p.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                                          w.ctypes.data_as(C.c_void_p)), "rs_vocabulary_arrays")
        return p, d, w

    def close(self):
        if self.h:
            self.ctx.lib.rs_vocabulary_destroy(self.h)
            self.h = C.c_void_p()


class Bow:
    """rs_bow: one bag-of-words vector on the device and the scratch that makes it."""

    def __init__(self, ctx, voc, max_points=8192):
        self.ctx, self.voc, self.max_points = ctx, voc, int(max_points)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.rs_bow_create(ctx.h, voc.h, self.max_points, C.byref(self.h)), "rs_bow_create")

    def transform(self, d_desc, d_count, max_n, words=True):
        """rs_bow_transform; d_count is a device [1] i32.  Returns d_word [max_n] i32 (device), or None with words=False."""
        d_word = self.ctx.empty((max(int(max_n), 1),), self.ctx.torch.int32) if words else None
        self.ctx._check(self.ctx.lib.rs_bow_transform(self.ctx.h, self.h, _dp(d_desc), _dp(d_count), int(max_n), _dp(d_word)),
                        "rs_bow_transform")
        return d_word

    def download(self):
        """Diagnostic (synchronises): dict(words [m] i32, counts [m] i32, values [m] f64, norm)."""
        m = self.max_points
        w, c, v = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.float64)
        n, norm = np.zeros(1, np.int32), np.zeros(1, np.float64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)             # noqa: E731
        self.ctx._check(self.ctx.lib.rs_bow_download(self.ctx.h, self.h, vp(w), vp(c), vp(v), vp(n), vp(norm)), "rs_bow_download")
        k = int(n[0])
        return dict(words=w[:k].copy(), counts=c[:k].copy(), values=v[:k].copy(), norm=float(norm[0]))

    def close(self):
        if self.h:
            self.ctx.lib.rs_bow_destroy(self.h)
            self.h = C.c_void_p()


class BowDatabase:
    """rs_bow_database: the key frames' vectors as a packed CSR on the device."""

    def __init__(self, ctx, voc, max_entries, max_total_words):
        self.ctx, self.voc = ctx, voc
        self.h = C.c_void_p()
        ctx._check(ctx.lib.rs_bow_database_create(ctx.h, voc.h, int(max_entries), int(max_total_words), C.byref(self.h)),
                   "rs_bow_database_create")

    def add(self, bow):
        """Appends bow's current vector; returns its entry index (one 4-byte read-back)."""
        e = C.c_int32(-1)
        self.ctx._check(self.ctx.lib.rs_bow_database_add(self.ctx.h, self.h, bow.h, C.byref(e)), "rs_bow_database_add")
        return e.value

    def score(self, bow, first=0, count=None, out=None):
        """rs_bow_database_score: device f64 [count] scores of bow's vector against entries first .. first + count - 1."""
        if count is None:
            count = self.counts()[0] - first
        if out is None:
            out = self.ctx.empty((max(int(count), 1),), self.ctx.torch.float64)
        self.ctx._check(self.ctx.lib.rs_bow_database_score(self.ctx.h, self.h, bow.h, int(first), int(count), _dp(out)),
                        "rs_bow_database_score")
        return out[:max(int(count), 0)]

    def counts(self):
        e, w = C.c_int32(0), C.c_int32(0)
        self.ctx._check(self.ctx.lib.rs_bow_database_counts(self.h, C.byref(e), C.byref(w)), "rs_bow_database_counts")
        return e.value, w.value

    def close(self):
        if self.h:
            self.ctx.lib.rs_bow_database_destroy(self.h)
            self.h = C.c_void_p()


class LoopVerifier:
    """rs_loop_verifier: verify_pnp of a query key frame against ranked candidates, all key frames of a ResidentMap."""

    def __init__(self, ctx, max_points=8192, max_candidates=3, max_hypotheses=200):
        self.ctx, self.max_points, self.max_candidates = ctx, int(max_points), int(max_candidates)
        self.max_hypotheses = int(max_hypotheses)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.rs_loop_verifier_create(ctx.h, self.max_points, self.max_candidates, self.max_hypotheses, C.byref(self.h)),
                   "rs_loop_verifier_create")
        n = max(self.max_candidates, 1)
        self._res = (LoopResult * n)()
        self._listed = [np.zeros((n, self.max_points), np.int32) for _ in range(3)]

    def verify(self, map_, query_kf, candidates, K, width, max_distance=64, threshold_px=4.0, confidence=0.99, max_hypotheses=200,
               seed=0):
        """rs_map_verify_loop: one dict per candidate — status, ok, correspondences, inliers, listed, spread, drift, gap
        (f32), pose [4][4] f32 and the listed correspondences query_kp / point / candidate_kp [listed] i32."""
        cand = np.ascontiguousarray(candidates, np.int32)
        n = len(cand)
        if n > self.max_candidates:                      # (the library refuses it: ask it with buffers that hold the answer)
            res, listed = (LoopResult * n)(), [np.zeros((n, self.max_points), np.int32) for _ in range(3)]
        else:
            res, listed = self._res, self._listed
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self.ctx._check(self.ctx.lib.rs_map_verify_loop(
            self.ctx.h, self.h, map_.h, int(query_kf), cand.ctypes.data_as(C.c_void_p), n, Kc, int(width), int(max_distance),
            C.c_double(threshold_px), C.c_double(confidence), int(max_hypotheses), C.c_uint64(int(seed) & (2 ** 64 - 1)), res,
            *[a.ctypes.data_as(C.c_void_p) for a in listed]), "rs_map_verify_loop")
        out = []
        for c in range(n):
            r, k = res[c], res[c].listed
            out.append(dict(status=r.status, ok=bool(r.ok), correspondences=r.correspondences, inliers=r.inliers, listed=k,
                            spread=np.float32(r.spread), drift=np.float32(r.drift), gap=np.float32(r.gap),
                            pose=np.array(r.pose, np.float32).reshape(4, 4), query_kp=listed[0][c, :k].copy(),
                            point=listed[1][c, :k].copy(), candidate_kp=listed[2][c, :k].copy()))
        return out

    def download(self, candidate):
        """rs_loop_verifier_download (synchronises): chain `candidate` of the last call — dict(nt, rows [nt][32] u8, slots,
        keypoints [nt] i32, positions [nt][3] f32, match_query, match_train [count] i32, inlier_index [inliers] i32)."""
        m = self.max_points
        rows, pos = np.zeros((m, 32), np.uint8), np.zeros((m, 3), np.float32)
        slots, kps, mq, mt, ii = (np.zeros(m, np.int32) for _ in range(5))
        nt, cnt, inl = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)         # noqa: E731
        self.ctx._check(self.ctx.lib.rs_loop_verifier_download(self.ctx.h, self.h, int(candidate), C.byref(nt), vp(rows), vp(slots),
                                                               vp(kps), vp(pos), vp(mq), vp(mt), C.byref(cnt), vp(ii), C.byref(inl)),
                        "rs_loop_verifier_download")
        return dict(nt=nt.value, rows=rows[:nt.value].copy(), slots=slots[:nt.value].copy(), keypoints=kps[:nt.value].copy(),
                    positions=pos[:nt.value].copy(), match_query=mq[:cnt.value].copy(), match_train=mt[:cnt.value].copy(),
                    inlier_index=ii[:inl.value].copy())

    def close(self):
        if self.h:
            self.ctx.lib.rs_loop_verifier_destroy(self.h)
            self.h = C.c_void_p()


class _FrameMatches:
    """The frame's match table (Frame::m_map_matches on the device), for both kinds of frame."""

    def matches_clear(self):
        self.ctx._check(self.ctx.lib.rs_frame_matches_clear(self.ctx.h, self.h), "rs_frame_matches_clear")

    def matches_add(self, d_kp, d_point, d_count=None, max_n=None):
        """Frame::add_map_match for a device list, in list order; the count is read on the device."""
        n = int(d_kp.shape[0]) if max_n is None else int(max_n)
        self.ctx._check(self.ctx.lib.rs_frame_matches_add(self.ctx.h, self.h, _dp(d_kp), _dp(d_point), _dp(d_count), n), "rs_frame_matches_add")

    def matches(self):
        """rs_frame_matches_download (synchronises): (table [n] i32, Frame::num_map_matches)."""
        tab, cnt = np.full(max(self.n, 1), -1, np.int32), C.c_int(0)
        self.ctx._check(self.ctx.lib.rs_frame_matches_download(self.ctx.h, self.h, tab.ctypes.data_as(C.c_void_p), C.byref(cnt)),
                        "rs_frame_matches_download")
        return tab[:self.n], cnt.value


class ResidentFrame(_FrameMatches):
    def __init__(self, ctx, keypoints, descriptors):
        self.ctx = ctx
        kp = np.ascontiguousarray(keypoints, np.float32)
        de = np.ascontiguousarray(descriptors, np.uint8)
        self.n = len(kp)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.rs_frame_create(ctx.h, kp.ctypes.data_as(C.c_void_p), de.ctypes.data_as(C.c_void_p), self.n, C.byref(self.h)), "rs_frame_create")

    def download(self):
        return frame_download(self.ctx, self)

    def close(self):
        if self.h:
            self.ctx.lib.rs_frame_destroy(self.h)
            self.h = C.c_void_p()


def frame_download(ctx, frame):
    """rs_frame_download of a ResidentFrame or a DeviceFrame (synchronises): dict(n, kp [n][2] f32, desc [n][32] u8,
    kd [3][n] i32 = node_kp | left | right, root, packed u8 [20 n])."""
    n = C.c_int(0)
    ctx._check(ctx.lib.rs_frame_download(ctx.h, frame.h, C.byref(n), None, None, None, None, None), "rs_frame_download")
    m = max(n.value, 1)
    kp, desc, kd = np.zeros((m, 2), np.float32), np.zeros((m, 32), np.uint8), np.zeros((3, m), np.int32)
    packed, root = np.zeros(20 * m, np.uint8), C.c_int32(0)
    ctx._check(ctx.lib.rs_frame_download(ctx.h, frame.h, C.byref(n), kp.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p),
                                         kd.ctypes.data_as(C.c_void_p), C.byref(root), packed.ctypes.data_as(C.c_void_p)),
               "rs_frame_download")
    k = n.value
    return dict(n=k, kp=kp[:k], desc=desc[:k], kd=kd[:, :k] if k else np.zeros((3, 0), np.int32), root=root.value,
                packed=packed[:20 * k])


class DeviceFrame(_FrameMatches):
    """rs_frame filled from device arrays (rs_frame_create_device / rs_frame_assign_device): allocated once for
    max_points keypoints, reassigned every video frame; usable wherever ResidentMap takes a frame."""

    def __init__(self, ctx, max_points=8192):
        self.ctx, self.max_points, self.n = ctx, int(max_points), 0
        self.h = C.c_void_p()
        ctx._check(ctx.lib.rs_frame_create_device(ctx.h, self.max_points, C.byref(self.h)), "rs_frame_create_device")

    def assign(self, d_desc, d_pt_a=None, d_count_a=None, d_pt_b=None, d_count_b=None):
        """List a (rs_track_features' pts / count) then list b (rs_detect_features' pts / counts[1:]) and the first n rows
        of d_desc (rs_describe_features' desc), all device tensors; one 4-byte read-back.  Returns n."""
        n = C.c_int(0)
        self.ctx._check(self.ctx.lib.rs_frame_assign_device(self.ctx.h, self.h, _dp(d_pt_a), _dp(d_count_a), _dp(d_pt_b),
                                                            _dp(d_count_b), _dp(d_desc), C.byref(n)), "rs_frame_assign_device")
        self.n = n.value
        return self.n

    def download(self):
        return frame_download(self.ctx, self)

    def close(self):
        if self.h:
            self.ctx.lib.rs_frame_destroy(self.h)
            self.h = C.c_void_p()


class TrackResults(C.Structure):
    _fields_ = [("capacity_tracks", C.c_int), ("capacity_pairs", C.c_int), ("counts", C.c_int32 * 3), ("out_of_range", C.c_int32),
                ("n_tracks", C.c_int32), ("n_pairs", C.c_int32), ("h_keypoint", C.c_void_p), ("h_xyz", C.c_void_p),
                ("h_sightings", C.c_void_p), ("h_kf_ptr", C.c_void_p), ("h_kf_pairs", C.c_void_p), ("h_track", C.c_void_p),
                ("h_parallax_cos", C.c_void_p), ("h_required_cos", C.c_void_p), ("h_inconsistent", C.c_void_p)]


QUERY_FIELDS = ("covisible", "num_map_matches", "waiting", "live", "first_frame", "next_id_low")


def needs_key_frame(query, frame_gap, last_key_frame_matches, max_key_frame_gap=20, new_tracks_threshold=200,
                    min_covisible_points=50, min_covisible_fraction=0.7):
    """Mapper::needs_key_frame's decision on TrackStore.query's six integers (host only: no context, no device)."""
    q = (C.c_int32 * 6)(*[int(query[k]) for k in QUERY_FIELDS] if isinstance(query, dict) else [int(v) for v in query])
    out = C.c_int(-1)
    rc = load().rs_needs_key_frame(q, int(frame_gap), int(last_key_frame_matches), int(max_key_frame_gap), int(new_tracks_threshold),
                                   int(min_covisible_points), C.c_float(min_covisible_fraction), C.byref(out))
    if rc:
        raise RsError(f"rs_needs_key_frame -> status {rc}")
    return bool(out.value)


class TrackStore:
    """rs_track_store: TrackStore and the key-frame decision's counts on the device; every method is one C-ABI call."""

    def __init__(self, ctx, max_points=8192, max_sightings=100):
        self.ctx, self.lib, self.max_points, self.max_sightings = ctx, ctx.lib, int(max_points), int(max_sightings)
        self.h, self._out = C.c_void_p(), None
        ctx._check(self.lib.rs_track_store_create(ctx.h, self.max_points, self.max_sightings, C.byref(self.h)), "rs_track_store_create")

    def close(self):
        if self.h:
            self.lib.rs_track_store_destroy(self.h)
            self.h = C.c_void_p()

    def clear(self):
        self.ctx._check(self.lib.rs_track_store_clear(self.ctx.h, self.h), "rs_track_store_clear")

    def carry(self, d_prev_index, d_inlier_index=None, d_count=None, max_n=None):
        """TrackStore::carry_forward on rs_track_features' kept-index list and rs_estimate_pose's inlier list; nothing comes back."""
        n = int(d_prev_index.shape[0]) if max_n is None else int(max_n)
        self.ctx._check(self.lib.rs_track_store_carry(self.ctx.h, self.h, _dp(d_prev_index), _dp(d_inlier_index), _dp(d_count), n),
                        "rs_track_store_carry")

    def extend(self, frame, frame_index, key_frame=-1):
        self.ctx._check(self.lib.rs_track_store_extend(self.ctx.h, self.h, frame.h, int(frame_index), int(key_frame)), "rs_track_store_extend")

    def query(self, frame, map_=None, last_key_frame=-1, min_sightings=3, min_travel=20.0):
        """The path's one read-back per frame: dict of QUERY_FIELDS."""
        out = (C.c_int32 * 6)()
        self.ctx._check(self.lib.rs_track_store_query(self.ctx.h, self.h, None if map_ is None else map_.h, frame.h, int(last_key_frame),
                                                      int(min_sightings), C.c_float(min_travel), out), "rs_track_store_query")
        return dict(zip(QUERY_FIELDS, [int(v) for v in out]))

    def triangulate(self, frame, d_poses, pose_base, kf_pose, K, map_=None, any_parallax_cosine=1.0, max_reproj=4.0,
                    min_parallax_cosine=0.999848, rotation_parallax_factor=0.20, min_new_points=100, d_required=None,
                    capacity_pairs=None):
        """Mapper::triangulate_tracks' loop from the store.  Returns dict(counts [3], out_of_range, n_tracks, n_pairs and, per
        accepted track, keypoint, xyz, sightings, kf_ptr, kf_pairs [n_pairs][2])."""
        T = self.max_points
        cp = 4 * T if capacity_pairs is None else int(capacity_pairs)
        if self._out is None or self._out[0] != cp:            # the host arrays are made once, not per key frame
            self._out = (cp, np.zeros(T, np.int32), np.zeros((T, 3), np.float32), np.zeros(T, np.int32), np.zeros(T + 1, np.int32),
                         np.zeros((max(cp, 1), 2), np.int32), np.zeros(T, np.int32), np.zeros(T, np.float32), np.zeros(T, np.float32),
                         np.zeros(T, np.int32))
        _, kp, xyz, ns, ptr, pairs, trk, pc, rc, inc = self._out
        r = TrackResults(capacity_tracks=T, capacity_pairs=cp, h_keypoint=kp.ctypes.data, h_xyz=xyz.ctypes.data, h_sightings=ns.ctypes.data,
                         h_kf_ptr=ptr.ctypes.data, h_kf_pairs=pairs.ctypes.data, h_track=trk.ctypes.data, h_parallax_cos=pc.ctypes.data,
                         h_required_cos=rc.ctypes.data, h_inconsistent=inc.ctypes.data)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self.ctx._check(self.lib.rs_track_store_triangulate(
            self.ctx.h, self.h, None if map_ is None else map_.h, frame.h, _dp(d_poses), int(d_poses.shape[0]), int(pose_base), int(kf_pose), Kc,
            C.c_float(any_parallax_cosine), C.c_float(max_reproj), C.c_float(min_parallax_cosine), C.c_float(rotation_parallax_factor),
            int(min_new_points), None if d_required is None else _dp(d_required), C.byref(r)), "rs_track_store_triangulate")
        na = max(min(int(r.counts[0]), int(r.n_tracks)), 0)
        return dict(counts=np.array(list(r.counts), np.int32), out_of_range=int(r.out_of_range), n_tracks=int(r.n_tracks), n_pairs=int(r.n_pairs),
                    keypoint=kp[:na].copy(), xyz=xyz[:na].copy(), sightings=ns[:na].copy(), kf_ptr=ptr[:na + 1].copy(),
                    kf_pairs=pairs[:min(int(r.n_pairs), cp)].copy(), track=trk[:na].copy(), parallax_cos=pc[:na].copy(),
                    required_cos=rc[:na].copy(), inconsistent=inc[:max(min(int(r.counts[2]), int(r.n_tracks)), 0)].copy())

    def erase_inconsistent(self):
        self.ctx._check(self.lib.rs_track_store_erase_inconsistent(self.ctx.h, self.h), "rs_track_store_erase_inconsistent")

    def download(self):
        """Diagnostic (synchronises): the live tracks in id order — dict(n, next_id, id [n] u64, keypoint [n], count [n],
        sightings [n][max_sightings] records (frame, x, y, kf, kp); entries past count[t] are zero)."""
        T, S = self.max_points, self.max_sightings
        n, nxt = C.c_int(0), C.c_uint64(0)
        ids, kp, cnt = np.zeros(T, np.uint64), np.zeros(T, np.int32), np.zeros(T, np.int32)
        sg = np.zeros((T, S), SIGHTING_DTYPE)
        self.ctx._check(self.lib.rs_track_store_download(self.ctx.h, self.h, C.byref(n), C.byref(nxt), ids.ctypes.data_as(C.c_void_p),
                                                         kp.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
                                                         sg.ctypes.data_as(C.c_void_p)), "rs_track_store_download")
        k = n.value
        return dict(n=k, next_id=int(nxt.value), id=ids[:k].copy(), keypoint=kp[:k].copy(), count=cnt[:k].copy(), sightings=sg[:k].copy())

    def packed(self):
        """Diagnostic (synchronises): rs_triangulate_tracks' inputs as the last triangulate call packed them."""
        nt, ns = C.c_int(0), C.c_int(0)
        T, S = self.max_points, self.max_points * self.max_sightings
        uv, skip, ptr = np.zeros((T, 2), np.float32), np.zeros(T, np.uint8), np.zeros(T + 1, np.int32)
        pose, suv = np.zeros(S, np.int32), np.zeros((S, 2), np.float32)
        self.ctx._check(self.lib.rs_track_store_download_packed(
            self.ctx.h, self.h, C.byref(nt), C.byref(ns), uv.ctypes.data_as(C.c_void_p), skip.ctypes.data_as(C.c_void_p),
            ptr.ctypes.data_as(C.c_void_p), pose.ctypes.data_as(C.c_void_p), suv.ctypes.data_as(C.c_void_p), S), "rs_track_store_download_packed")
        t, s = nt.value, ns.value
        return dict(track_uv=uv[:t].copy(), skip=skip[:t].copy(), sight_ptr=ptr[:t + 1].copy(), sight_pose=pose[:s].copy(), sight_uv=suv[:s].copy())


SIGHTING_DTYPE = np.dtype([("frame", np.int32), ("x", np.float32), ("y", np.float32), ("kf", np.int32), ("kp", np.int32)])


FUSE_MAX_COVISIBLE = 64


class FuseOptions(C.Structure):
    _fields_ = [("intrinsics", C.c_float * 4), ("width", C.c_int), ("height", C.c_int), ("max_distance", C.c_int),
                ("min_shared", C.c_int), ("max_covisible", C.c_int), ("check", C.c_int),
                ("h_sources", C.c_void_p), ("capacity_sources", C.c_int), ("h_removed", C.c_void_p), ("capacity_removed", C.c_int)]


class FuseReport(C.Structure):
    _fields_ = [("n_old_frames", C.c_int), ("old_frames", C.c_int32 * (FUSE_MAX_COVISIBLE + 1)), ("n_sources", C.c_int),
                ("outcomes", C.c_int * 6), ("n_removed", C.c_int), ("device_state_mismatches", C.c_int)]


class ResidentMap:
    """Thin wrapper of rs_map: every method is one C-ABI call."""

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        ctx._check(self.lib.rs_map_create(ctx.h, C.byref(self.h)), "rs_map_create")

    def close(self):
        if self.h:
            self.lib.rs_map_destroy(self.h)
            self.h = C.c_void_p()

    def _f3(self, v):
        return (C.c_float * 3)(*[float(x) for x in v])

    def add_keyframe(self, frame, pose):
        out = C.c_int(-1)
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        self.ctx._check(self.lib.rs_map_add_keyframe(self.h, frame.h, p.ctypes.data_as(C.c_void_p), C.byref(out)), "rs_map_add_keyframe")
        return out.value

    def set_keyframe_pose(self, kf, pose):
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        self.ctx._check(self.lib.rs_map_set_keyframe_pose(self.h, int(kf), p.ctypes.data_as(C.c_void_p)), "rs_map_set_keyframe_pose")

    def add_point(self, xyz):
        out = C.c_int(-1)
        self.ctx._check(self.lib.rs_map_add_point(self.h, self._f3(xyz), C.byref(out)), "rs_map_add_point")
        return out.value

    def set_position(self, point, xyz):
        self.ctx._check(self.lib.rs_map_set_position(self.h, int(point), self._f3(xyz)), "rs_map_set_position")

    def remove_point(self, point):
        self.ctx._check(self.lib.rs_map_remove_point(self.h, int(point)), "rs_map_remove_point")

    def add_observation(self, point, kf, keypoint):
        self.ctx._check(self.lib.rs_map_add_observation(self.h, int(point), int(kf), int(keypoint)), "rs_map_add_observation")

    def remove_observation(self, point, kf):
        self.ctx._check(self.lib.rs_map_remove_observation(self.h, int(point), int(kf)), "rs_map_remove_observation")

    def counts(self):
        buf = (C.c_int * 4)()
        self.ctx._check(self.lib.rs_map_counts(self.h, buf), "rs_map_counts")
        return dict(slots=buf[0], alive=buf[1], observations=buf[2], key_frames=buf[3])

    def positions(self):
        n = self.counts()["slots"]
        out = np.zeros((max(n, 1), 3), np.float32)
        self.ctx._check(self.lib.rs_map_get_positions(self.h, 0, n, out.ctypes.data_as(C.c_void_p)), "rs_map_get_positions")
        return out[:n]

    def match(self, frame, pose, K, width, height, kp_matched=None, matched_points=(), required_observer=-1, only_points=None,
              replace=0, max_distance=64):
        n = frame.n
        mk, mp = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        cnt = C.c_int(0)
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        km = None if kp_matched is None else np.ascontiguousarray(kp_matched, np.uint8)
        mpts = np.ascontiguousarray(matched_points, np.int32)
        only = None if only_points is None else np.ascontiguousarray(only_points, np.int32)
        self.ctx._check(self.lib.rs_map_match(
            self.ctx.h, self.h, frame.h, p.ctypes.data_as(C.c_void_p), Kc, int(width), int(height),
            None if km is None else km.ctypes.data_as(C.c_void_p), mpts.ctypes.data_as(C.c_void_p), len(mpts), int(required_observer),
            None if only is None else only.ctypes.data_as(C.c_void_p), -1 if only is None else len(only), int(replace), int(max_distance),
            mk.ctypes.data_as(C.c_void_p), mp.ctypes.data_as(C.c_void_p), C.byref(cnt)), "rs_map_match")
        return mk[:cnt.value].copy(), mp[:cnt.value].copy()

    # -- the tail of Tracker::track on the frame's device table
    def set_track_consistent(self, point):
        self.ctx._check(self.lib.rs_map_set_track_consistent(self.h, int(point)), "rs_map_set_track_consistent")

    def carry_matches(self, prev, nxt, d_prev_index, d_inlier_index=None, d_count=None, max_n=None, min_points=15, d_stats=None):
        """Tracker::track_from_last_frame on the two frames' tables; stream-ordered, nothing comes back."""
        n = int(d_prev_index.shape[0]) if max_n is None else int(max_n)
        self.ctx._check(self.lib.rs_map_carry_matches(self.ctx.h, self.h, prev.h, nxt.h, _dp(d_prev_index), _dp(d_inlier_index),
                                                      _dp(d_count), n, int(min_points), _dp(d_stats)), "rs_map_carry_matches")

    def refine_pose(self, frame, cam, K, min_matches=15, prior=None, delta=None, options=None):
        """Tracker::optimize_pose's refit from the frame's table; prior / delta as Context.refine_pose_inertial.
        Returns cam, velocity, summary, n_used."""
        cam = np.array(cam, np.float64, order="C")
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        s, used = BaSummary(), C.c_int(0)
        vel = np.zeros(3)
        kind, pred, sigma, keep, args = 0, None, 0.0, [], [None, None, None, None, None]
        if prior is not None:
            kind, sigma = 1, float(prior[1])
            keep.append(np.ascontiguousarray(prior[0], np.float64))
            pred = keep[-1].ctypes.data_as(C.c_void_p)
        if delta is not None:
            kind = 2
            farr, _ = imu_factor_array(delta["imu"])
            keep += [np.ascontiguousarray(delta[k], np.float64) for k in ("prev_pose", "prev_velocity", "prev_bias")]
            keep.append(np.ascontiguousarray(delta["imu"]["gravity"], np.float64))
            vel = np.array(delta["velocity"], np.float64)
            args = [keep[-4].ctypes.data_as(C.c_void_p), keep[-3].ctypes.data_as(C.c_void_p), keep[-2].ctypes.data_as(C.c_void_p),
                    farr, keep[-1].ctypes.data_as(C.c_void_p)]
        self.ctx._check(self.lib.rs_map_refine_pose(
            self.ctx.h, self.h, frame.h, cam.ctypes.data_as(C.c_void_p), Kc, int(min_matches), kind, pred, C.c_double(sigma),
            args[0], args[1], args[2], args[3], args[4], vel.ctypes.data_as(C.c_void_p),
            None if options is None else C.byref(options), C.byref(s), C.byref(used)), "rs_map_refine_pose")
        return cam, vel, s.as_dict(), used.value

    def match_frame(self, frame, pose, K, width, height, required_observer=-1, max_distance=64):
        """match_key_frame / match_map on the frame's table; returns the number of new matches."""
        cnt = C.c_int(0)
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        self.ctx._check(self.lib.rs_map_match_frame(self.ctx.h, self.h, frame.h, p.ctypes.data_as(C.c_void_p), Kc, int(width), int(height),
                                                    int(required_observer), int(max_distance), C.byref(cnt)), "rs_map_match_frame")
        return cnt.value

    def pose_graph(self, loops, four_dof=False, gravity=(0.0, 0.0, 0.0), options=None):
        n = self.counts()["key_frames"]
        poses, rot = np.zeros((max(n, 1), 16), np.float32), np.zeros((max(n, 1), 9), np.float32)
        g = (C.c_double * 3)(*[float(v) for v in gravity])
        s = BaSummary()
        self.ctx._check(self.lib.rs_map_pose_graph(self.ctx.h, self.h, pose_graph_edges(loops), len(loops), int(bool(four_dof)), g,
                                                   None if options is None else C.byref(options), poses.ctypes.data_as(C.c_void_p),
                                                   rot.ctypes.data_as(C.c_void_p), C.byref(s)), "rs_map_pose_graph")
        return s.as_dict(), poses[:n].reshape(-1, 4, 4), rot[:n].reshape(-1, 3, 3)

    def bundle_adjust(self, kfs, free, K, options=None, capacity=None):
        """Returns (summary, poses [n][16], free point slots, their positions).  `capacity` is the room given to the
        library for free points (default: every slot); summary["n_points"] is the full count it reports, the slots and
        positions returned are the first min(n_points, capacity)."""
        kfs = np.ascontiguousarray(kfs, np.int32)
        free = np.ascontiguousarray(free, np.uint8)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        s = BaSummary()
        cap = self.counts()["slots"] if capacity is None else int(capacity)
        poses = np.zeros((len(kfs), 16), np.float32)
        pts, xyz = np.zeros(max(cap, 1), np.int32), np.zeros((max(cap, 1), 3), np.float32)
        n = C.c_int(0)
        self.ctx._check(self.lib.rs_map_bundle_adjust(
            self.ctx.h, self.h, kfs.ctypes.data_as(C.c_void_p), free.ctypes.data_as(C.c_void_p), len(kfs), Kc,
            None if options is None else C.byref(options), C.byref(s), poses.ctypes.data_as(C.c_void_p),
            pts.ctypes.data_as(C.c_void_p), xyz.ctypes.data_as(C.c_void_p), cap, C.byref(n)), "rs_map_bundle_adjust")
        k = min(n.value, max(cap, 0))
        return dict(s.as_dict(), n_points=n.value), poses, pts[:k].copy(), xyz[:k].copy()

    # -- Mapper::insert on the resident map
    def insert_keyframe(self, frame, pose):
        """rs_map_add_keyframe + the adoption of the frame's device match table.  Returns (key-frame handle, adopted)."""
        kf, n = C.c_int(-1), C.c_int(0)
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        self.ctx._check(self.lib.rs_map_insert_keyframe(self.ctx.h, self.h, frame.h, p.ctypes.data_as(C.c_void_p), C.byref(kf), C.byref(n)),
                        "rs_map_insert_keyframe")
        return kf.value, n.value

    def add_track_points(self, kf, results, window_kfs, capacity_pairs=None):
        """Mapper::triangulate_tracks' creation loop for TrackStore.triangulate's dict (keypoint, xyz, sightings, kf_ptr,
        kf_pairs, n_pairs).  capacity_pairs: the room the pairs had (default: n_pairs).  Returns the new point slots."""
        na = len(results["keypoint"])
        kp = np.ascontiguousarray(results["keypoint"], np.int32)
        xyz = np.ascontiguousarray(results["xyz"], np.float32).reshape(-1, 3)
        ns = np.ascontiguousarray(results["sightings"], np.int32)
        ptr = np.ascontiguousarray(results["kf_ptr"], np.int32)
        pairs = np.ascontiguousarray(results["kf_pairs"], np.int32).reshape(-1, 2)
        n_pairs = int(results.get("n_pairs", len(pairs)))
        cp = n_pairs if capacity_pairs is None else int(capacity_pairs)
        r = TrackResults(capacity_tracks=max(na, 1), capacity_pairs=cp, h_keypoint=kp.ctypes.data, h_xyz=xyz.ctypes.data,
                         h_sightings=ns.ctypes.data, h_kf_ptr=ptr.ctypes.data, h_kf_pairs=pairs.ctypes.data)
        r.counts[0], r.n_tracks, r.n_pairs = na, na, n_pairs
        win = np.ascontiguousarray(window_kfs, np.int32)
        out = np.full(max(na, 1), -1, np.int32)
        self.ctx._check(self.lib.rs_map_add_track_points(self.h, int(kf), C.byref(r), win.ctypes.data_as(C.c_void_p), len(win),
                                                         out.ctypes.data_as(C.c_void_p)), "rs_map_add_track_points")
        return out[:na].copy()

    def reanchor(self, kfs, before, capacity=None):
        """rs_map_reanchor.  Returns (n_points, moved slots, their new positions); the arrays hold min(n_points, capacity)."""
        kfs = np.ascontiguousarray(kfs, np.int32)
        before = np.ascontiguousarray(before, np.float32).reshape(-1, 16)
        cap = self.counts()["slots"] if capacity is None else int(capacity)
        pts, xyz = np.zeros(max(cap, 1), np.int32), np.zeros((max(cap, 1), 3), np.float32)
        n = C.c_int(0)
        self.ctx._check(self.lib.rs_map_reanchor(self.ctx.h, self.h, kfs.ctypes.data_as(C.c_void_p), before.ctypes.data_as(C.c_void_p),
                                                 len(kfs), pts.ctypes.data_as(C.c_void_p), xyz.ctypes.data_as(C.c_void_p), cap, C.byref(n)),
                        "rs_map_reanchor")
        k = min(n.value, max(cap, 0))
        return n.value, pts[:k].copy(), xyz[:k].copy()

    def cull_points(self, kfs, K, max_mean_error=3.0, apply=True, capacity=None, check=True):
        """rs_map_cull_points.  Returns dict(status, n_removed, n_local, removed, xyz).  check=False returns the status of a
        refused call (capacity too small) instead of raising."""
        kfs = np.ascontiguousarray(kfs, np.int32)
        Kc = (C.c_float * 4)(*[float(v) for v in K])
        cap = self.counts()["slots"] if capacity is None else int(capacity)
        pts, xyz = np.zeros(max(cap, 1), np.int32), np.zeros((max(cap, 1), 3), np.float32)
        n, nl = C.c_int(0), C.c_int(0)
        rc = self.lib.rs_map_cull_points(self.ctx.h, self.h, kfs.ctypes.data_as(C.c_void_p), len(kfs), Kc, C.c_float(max_mean_error),
                                         int(bool(apply)), pts.ctypes.data_as(C.c_void_p), xyz.ctypes.data_as(C.c_void_p), cap,
                                         C.byref(n), C.byref(nl))
        if check:
            self.ctx._check(rc, "rs_map_cull_points")
        k = min(n.value, max(cap, 0)) if rc == 0 else 0
        return dict(status=rc, n_removed=n.value, n_local=nl.value, removed=pts[:k].copy(), xyz=xyz[:k].copy())

    def window(self, kfs, free):
        """rs_map_window: the problem bundle_adjust would solve, unsolved: dict(points, positions f64, obs_ptr, obs_cam,
        obs_uv).  Asks once for the sizes, then once more with room for them."""
        kfs = np.ascontiguousarray(kfs, np.int32)
        free = np.ascontiguousarray(free, np.uint8)
        n, m = C.c_int(0), C.c_int(0)
        cap_p, cap_o = 0, 0
        while True:
            pts, xyz = np.zeros(max(cap_p, 1), np.int32), np.zeros((max(cap_p, 1), 3))
            ptr, cam, uv = np.zeros(cap_p + 1, np.int32), np.zeros(max(cap_o, 1), np.int32), np.zeros((max(cap_o, 1), 2), np.float32)
            self.ctx._check(self.lib.rs_map_window(
                self.ctx.h, self.h, kfs.ctypes.data_as(C.c_void_p), free.ctypes.data_as(C.c_void_p), len(kfs),
                *[a.ctypes.data_as(C.c_void_p) for a in (pts, xyz, ptr, cam, uv)], cap_p, cap_o, C.byref(n), C.byref(m)), "rs_map_window")
            if n.value <= cap_p and m.value <= cap_o:
                return dict(points=pts[:n.value].copy(), positions=xyz[:n.value].copy(), obs_ptr=ptr[:n.value + 1].copy(),
                            obs_cam=cam[:m.value].copy(), obs_uv=uv[:m.value].copy())
            cap_p, cap_o = n.value, m.value

    # -- Mapper::fuse_loop on the resident map
    def fuse_points(self, kept, discarded):
        """rs_map_fuse_points (Map::fuse)"""
        self.ctx._check(self.lib.rs_map_fuse_points(self.h, int(kept), int(discarded)), "rs_map_fuse_points")

    def observations(self, point):
        """rs_map_get_observations: [(key frame, keypoint)] in insertion order"""
        n = C.c_int(0)
        self.ctx._check(self.lib.rs_map_get_observations(self.h, int(point), None, None, 0, C.byref(n)), "rs_map_get_observations")
        kf, kp = np.zeros(max(n.value, 1), np.int32), np.zeros(max(n.value, 1), np.int32)
        self.ctx._check(self.lib.rs_map_get_observations(self.h, int(point), kf.ctypes.data_as(C.c_void_p), kp.ctypes.data_as(C.c_void_p),
                                                         n.value, C.byref(n)), "rs_map_get_observations")
        return [(int(a), int(b)) for a, b in zip(kf[:n.value], kp[:n.value])]

    def keyframe_matches(self, kf):
        """rs_map_get_keyframe_matches: the key frame's keypoint -> point table"""
        n = C.c_int(0)
        self.ctx._check(self.lib.rs_map_get_keyframe_matches(self.h, int(kf), None, 0, C.byref(n)), "rs_map_get_keyframe_matches")
        tab = np.full(max(n.value, 1), -1, np.int32)
        self.ctx._check(self.lib.rs_map_get_keyframe_matches(self.h, int(kf), tab.ctypes.data_as(C.c_void_p), n.value, C.byref(n)),
                        "rs_map_get_keyframe_matches")
        return tab[:n.value].copy()

    def fuse_loop(self, query, candidate, inliers, window, K, width, height, max_distance=64, min_shared=15, max_covisible=20,
                  check=False, journal=True, capacity=None, raise_on_error=True):
        """rs_map_fuse_loop.  inliers: [(keypoint, point)].  Returns dict(status, old_frames, sources, sections (a list of
        [(keypoint, point, outcome)] per section; None with journal=False), n_entries, outcomes, removed,
        device_state_mismatches).  capacity: the room of the journal arrays (default: every possible entry)."""
        ik = np.ascontiguousarray([i[0] for i in inliers], np.int32)
        ip = np.ascontiguousarray([i[1] for i in inliers], np.int32)
        win = np.ascontiguousarray(window, np.int32)
        c = self.counts()
        opt = FuseOptions(width=int(width), height=int(height), max_distance=int(max_distance), min_shared=int(min_shared),
                          max_covisible=int(max_covisible), check=int(bool(check)))
        for i in range(4):
            opt.intrinsics[i] = float(K[i])
        src, rem = np.full(max(c["slots"], 1), -1, np.int32), np.full(max(c["slots"], 1), -1, np.int32)
        opt.h_sources, opt.capacity_sources, opt.h_removed, opt.capacity_removed = src.ctypes.data, len(src), rem.ctypes.data, len(rem)
        rep = FuseReport()
        # a section has at most min(sources, keypoints of the frame) entries: a source is accepted by at most one keypoint,
        # and a key frame inside the envelope has at most 8192
        cap = len(ik) + len(win) * min(c["slots"], 8192) if capacity is None else int(capacity)
        sec = np.zeros(len(win) + 2, np.int32)
        jk, jp, jo = (np.zeros(max(cap, 1), np.int32) for _ in range(3))
        n = C.c_int(0)
        ptr = (lambda a: a.ctypes.data_as(C.c_void_p)) if journal else (lambda a: None)
        rc = self.lib.rs_map_fuse_loop(self.ctx.h, self.h, int(query), int(candidate), ik.ctypes.data_as(C.c_void_p), ip.ctypes.data_as(C.c_void_p),
                                       len(ik), win.ctypes.data_as(C.c_void_p), len(win), C.byref(opt), C.byref(rep), ptr(sec), ptr(jk), ptr(jp),
                                       ptr(jo), cap if journal else 0, C.byref(n))
        if raise_on_error:
            self.ctx._check(rc, "rs_map_fuse_loop")
        if rc != 0:
            return dict(status=rc)
        sections = None
        if journal:
            k = min(n.value, max(cap, 0))
            sections = [[(int(jk[e]), int(jp[e]), int(jo[e])) for e in range(min(sec[i], k), min(sec[i + 1], k))] for i in range(len(sec) - 1)]
        return dict(status=rc, old_frames=[int(v) for v in rep.old_frames[:rep.n_old_frames]], sources=src[:rep.n_sources].copy(),
                    sections=sections, n_entries=n.value, outcomes=[int(v) for v in rep.outcomes], removed=rem[:rep.n_removed].copy(),
                    device_state_mismatches=rep.device_state_mismatches)
