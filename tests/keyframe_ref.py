"""Mapper::insert's four map stages (reference src/Mapper.cpp:152-174) restated on tests/map_model.MapModel: test
infrastructure only.  The arithmetic is the oracle's (oracle.reanchor_points, oracle.point_errors); this file decides WHICH
points take part and in which order, which is what the resident-map calls must reproduce:

  adopt             :157-159   the frame's match table, ascending keypoint, alive points only  (rs_map_insert_keyframe)
  add_track_points  :310-331   create_point + the window's key-frame sightings                 (rs_map_add_track_points)
  reanchor          :379-393   alive, exactly one observation, observer listed                 (rs_map_reanchor)
  cull              :396-431   alive and observed by a listed key frame; all observations      (rs_map_cull_points)

tests/test_keyframe_cpu.py pins every function against a literal object-graph walk; tests/test_gpu_keyframe.py holds the
library against them.  random_scene / build_model make the small maps both use.
"""
import numpy as np

from map_model import MapModel

MAX_POINT_REPROJECTION_ERROR = 3.0      # src/Mapper.cpp:20
CULL_MARGIN = 1e-3                      # px: a case is usable when no local mean is closer to the threshold than this


# ---------------------------------------------------------------------------------------------- the four stages
def adopt(model, kf, table, calls=None):
    """Associates every table entry (ascending keypoint) whose point is alive; returns how many.  `calls` (a list)
    collects the per-match C-ABI calls that make the same edits."""
    n = 0
    for i, p in enumerate(np.asarray(table)[:len(model.kf_kp[kf])]):
        p = int(p)
        if p < 0 or p >= model.n_slots() or not model.alive[p]:       # -1, or a dangling pointer in the reference
            continue
        c = model.associate(kf, p, i)
        if calls is not None:
            calls += c
        n += 1
    return n


def add_track_points(model, kf, res, window, calls=None, skipped=None):
    """res: TrackStore.triangulate's dict (keypoint, xyz, sightings, kf_ptr, kf_pairs; n_pairs / capacity_pairs optional).
    Returns (new slots, the slots set track-consistent).  Raises ValueError where the library refuses.  `calls` (a list)
    collects the per-point C-ABI calls that make the same edits; `skipped` (a dict) counts the sighting pairs each skip rule
    dropped: null (no handle), self, outside (the window), kp (keypoint taken), point (the observer already sees the point)."""
    calls = [] if calls is None else calls
    skipped = {} if skipped is None else skipped
    for k in ("null", "self", "outside", "kp", "point"):
        skipped.setdefault(k, 0)
    if int(res.get("n_pairs", len(res["kf_pairs"]))) > int(res.get("capacity_pairs", len(res["kf_pairs"]))):
        raise ValueError("the pairs are incomplete")
    window = {int(k) for k in window}
    slots, consistent = [], []
    for a in range(len(res["keypoint"])):
        p, c = model.create_point(res["xyz"][a], [(kf, int(res["keypoint"][a]))])                  # :312
        calls += c
        for s in range(int(res["kf_ptr"][a]), int(res["kf_ptr"][a + 1])):
            h, kp = int(res["kf_pairs"][s][0]), int(res["kf_pairs"][s][1])
            if h < 0 or h == kf or h not in window:                                                # :316-318
                skipped["null" if h < 0 else "self" if h == kf else "outside"] += 1
                continue
            if model.kp_point[h][kp] >= 0 or model.observer_kp(p, h) is not None:                  # :319-321
                skipped["kp" if model.kp_point[h][kp] >= 0 else "point"] += 1
                continue
            calls += model.associate(h, p, kp)                                                     # :322
        if int(res["sightings"][a]) >= 3:                                                          # :326-329
            consistent.append(p)
        slots.append(p)
    return slots, consistent


def reanchor_lists(model, kfs):
    """rs_reanchor_points' lists: the moved slots ascending and, per slot, its observer's index in kfs."""
    where = {int(k): c for c, k in enumerate(kfs)}
    pts = [p for p in range(model.n_slots())
           if model.alive[p] and len(model.obs[p]) == 1 and model.obs[p][0][0] in where]           # :387
    return np.array(pts, np.int32), np.array([where[model.obs[p][0][0]] for p in pts], np.int32)


def reanchor(model, kfs, before, oracle):
    """Moves the model's points; `after` is the model's current pose.  Returns (slots, their new positions)."""
    pts, fidx = reanchor_lists(model, kfs)
    if len(pts) == 0:
        return pts, np.zeros((0, 3), np.float32)
    after = np.stack([model.kf_pose[int(k)] for k in kfs]).astype(np.float32)
    pos = oracle.reanchor_points(pts, fidx, np.asarray(before, np.float32).reshape(-1, 16), after, model.positions())
    for p in pts:
        model.pos[int(p)] = pos[int(p)].copy()
    return pts, pos[pts]


def cull_problem(model, kfs):
    """rs_point_errors' flattened problem for the local set: dict(local slots ascending, positions, obs_ptr, obs_pose =
    key-frame handle, obs_uv, poses = every key frame's)."""
    listed = {int(k) for k in kfs}
    local = [p for p in range(model.n_slots()) if model.alive[p] and any(kf in listed for kf, _ in model.obs[p])]
    optr, opose, ouv = [0], [], []
    for p in local:
        for kf, kp in model.obs[p]:
            opose.append(kf)
            ouv.append(model.kf_kp[kf][kp])
        optr.append(len(opose))
    return dict(local=np.array(local, np.int32), positions=model.positions()[local].reshape(-1, 3),
                obs_ptr=np.array(optr, np.int32), obs_pose=np.array(opose, np.int32),
                obs_uv=np.array(ouv, np.float32).reshape(-1, 2),
                poses=np.stack(model.kf_pose).astype(np.float32) if model.n_kf() else np.zeros((0, 16), np.float32))


def cull(model, kfs, K, oracle, max_mean_error=MAX_POINT_REPROJECTION_ERROR, apply=True):
    """Returns dict(local, removed slots ascending, xyz, mean_err per local point); apply removes them from the model."""
    pr = cull_problem(model, kfs)
    if len(pr["local"]) == 0:
        return dict(local=pr["local"], removed=np.zeros(0, np.int32), xyz=np.zeros((0, 3), np.float32), mean_err=np.zeros(0, np.float32))
    r = oracle.point_errors(pr["positions"], pr["obs_ptr"], pr["obs_pose"], pr["obs_uv"], pr["poses"], K, max_mean_error)
    removed = pr["local"][r["cull_idx"]]
    xyz = model.positions()[removed].reshape(-1, 3)
    if apply:
        for p in removed:
            model.remove_point(int(p))
    return dict(local=pr["local"], removed=removed, xyz=xyz, mean_err=r["mean_err"])


def cull_margin(mean_err, max_mean_error=MAX_POINT_REPROJECTION_ERROR):
    """Distance of the closest mean to the threshold (inf for an empty set)."""
    return float(np.min(np.abs(np.asarray(mean_err, np.float64) - max_mean_error))) if len(mean_err) else float("inf")


# ---------------------------------------------------------------------------------------------- small maps
K = (500.0, 500.0, 320.0, 240.0)
WIDTH, HEIGHT = 640, 480


def pose_of(k, rng=None):
    """World -> camera, row-major f32: a small turn about y and a step along x per key frame."""
    a = 0.02 * k + (0.0 if rng is None else float(rng.normal(0, 0.004)))
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T[:3, 3] = [-0.15 * k, 0.01 * k, 0.0]
    if rng is not None:
        T[:3, 3] += rng.normal(0, 0.01, 3)
    return T.astype(np.float32).reshape(16)


def perturb_pose(T, rng, angle=0.004, step=0.01):
    """The pose after an adjustment: a small turn about y and a small step, in f32."""
    a = float(rng.normal(0, angle))
    D = np.eye(4)
    D[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    D[:3, 3] = rng.normal(0, step, 3)
    return (D @ np.asarray(T, np.float64).reshape(4, 4)).astype(np.float32).reshape(16)


def project(T, X):
    c = np.asarray(T, np.float64).reshape(4, 4)[:3] @ np.r_[np.asarray(X, np.float64), 1.0]
    return np.array([K[0] * c[0] / c[2] + K[2], K[1] * c[1] / c[2] + K[3]])


def random_scene(seed, n_kf, n_kp, P, max_obs=None, bad_frac=0.25, bad_px=(5.0, 12.0), noise_px=0.4, pose_scale=1.0):
    """n_kf key frames of n_kp keypoints and P point slots; a point is observed by 0 .. max_obs (default n_kf) key frames
    while they have keypoints left.  A `bad` point's pixels are off by bad_px (it is culled); the others by noise_px."""
    rng = np.random.default_rng(seed)
    max_obs = n_kf if max_obs is None else max_obs
    poses = [pose_of(k * pose_scale) for k in range(n_kf)]
    kf_kp = [[] for _ in range(n_kf)]
    pts = np.c_[rng.uniform(-2, 2, P), rng.uniform(-1.5, 1.5, P), rng.uniform(4, 8, P)].astype(np.float32).reshape(P, 3)
    obs = []
    for p in range(P):
        n = int(rng.integers(0, max_obs + 1)) if p % 7 else (1 if p == 0 else int(rng.integers(0, 2)))   # every 7th slot: none or one observer; slot 0: one
        bad = rng.random() < bad_frac
        sign = rng.choice([-1.0, 1.0], 2)
        for kf in rng.permutation(n_kf)[:n]:
            if len(kf_kp[kf]) >= n_kp:
                continue
            off = sign * rng.uniform(*bad_px, 2) if bad else rng.normal(0, noise_px, 2)
            kf_kp[kf].append(project(poses[kf], pts[p]) + off)
            obs.append((p, int(kf), len(kf_kp[kf]) - 1))
    for kf in range(n_kf):
        while len(kf_kp[kf]) < n_kp:
            kf_kp[kf].append(rng.uniform((0, 0), (WIDTH, HEIGHT)))
    kf_kp = [np.array(k, np.float32).reshape(-1, 2) for k in kf_kp]
    kf_desc = [rng.integers(0, 256, (n_kp, 32), dtype=np.uint8) for _ in range(n_kf)]
    return dict(seed=seed, poses=poses, kf_kp=kf_kp, kf_desc=kf_desc, points=pts, obs=obs, K=K)


def build_model(scene, replay=None):
    """The scene as a MapModel; replay(calls) (optional) drives the same edits on an rs_map."""
    model = MapModel()
    for kp, de, T in zip(scene["kf_kp"], scene["kf_desc"], scene["poses"]):
        _, calls = model.add_keyframe(kp, de, T)
        if replay:
            replay(calls)
    per = {}
    for p, kf, kp in scene["obs"]:
        per.setdefault(p, []).append((kf, kp))
    for p in range(len(scene["points"])):
        _, calls = model.create_point(scene["points"][p], per.get(p, []))
        if replay:
            replay(calls)
    return model


def match_frame_of(model, seed, n=120, extra=10, at=None):
    """A frame that sees some of the map: keypoints at the projections of observed alive points under a pose next to the
    last key frame's (or to pose_of(at)), each with the descriptor of its point's first observation; dict(pose, keypoints,
    descriptors)."""
    rng = np.random.default_rng(seed)
    T = pose_of(model.n_kf() if at is None else at, rng)
    cand = [p for p in model.alive_points() if model.obs[p]]
    pick = rng.permutation(len(cand))[:n]
    kp, de = [], []
    for i in pick:
        p = cand[int(i)]
        uv = project(T, model.pos[p]) + rng.normal(0, 0.3, 2)
        if 8 <= uv[0] < WIDTH - 8 and 8 <= uv[1] < HEIGHT - 8:
            kf, k = model.obs[p][0]
            kp.append(uv)
            de.append(model.kf_desc[kf][k])
    for _ in range(extra):                                           # keypoints that see no map point
        kp.append(rng.uniform((8, 8), (WIDTH - 8, HEIGHT - 8)))
        de.append(rng.integers(0, 256, 32, dtype=np.uint8))
    return dict(pose=T, keypoints=np.array(kp, np.float32).reshape(-1, 2), descriptors=np.array(de, np.uint8).reshape(-1, 32))


def random_results(model, kf, rng, n_acc=25):
    """An rs_track_results for key frame kf as a dict: n_acc accepted tracks at free keypoints, each with 0 .. 6 key-frame
    sighting pairs that exercise every skip rule — no handle, kf itself, any key frame (inside or outside a window), taken
    and free keypoints — and, every fifth track, one observer twice at two free keypoints."""
    free_kp = np.flatnonzero(model.kp_point[kf] < 0)
    kps = rng.choice(free_kp, n_acc, replace=False)
    ptr, pairs = [0], []
    for a in range(n_acc):
        for _ in range(int(rng.integers(0, 7))):
            r = rng.random()
            h = -1 if r < 0.15 else kf if r < 0.3 else int(rng.integers(model.n_kf()))
            hh = h if h >= 0 else 0
            taken = np.flatnonzero(model.kp_point[hh] >= 0)
            kp = int(rng.choice(taken)) if rng.random() < 0.3 and len(taken) else int(rng.integers(len(model.kf_kp[hh])))
            pairs.append((h, kp))
        if a % 5 == 0:                                               # the same observer twice, both keypoints free: the second is skipped
            h = 0 if kf != 0 else 2
            used = {k for hh, k in pairs if hh == h}
            two = [int(k) for k in np.flatnonzero(model.kp_point[h] < 0) if int(k) not in used][:2]
            pairs += [(h, two[0]), (h, two[1])]
        ptr.append(len(pairs))
    return dict(keypoint=kps.astype(np.int32), xyz=rng.normal(0, 1, (n_acc, 3)).astype(np.float32) + np.float32([0, 0, 6]),
                sightings=rng.integers(1, 6, n_acc).astype(np.int32), kf_ptr=np.array(ptr, np.int32),
                kf_pairs=np.array(pairs, np.int32).reshape(-1, 2), n_pairs=len(pairs))


# the maps of tests/test_gpu_keyframe.py: (seed, key frames, keypoints each, point slots); the slot counts cross the block
# size (256), k_kf_compact's 1024-slot chunks and the 4096-slot growth of the map buffers
GPU_CASES = [(11, 3, 40, 0), (12, 3, 40, 1), (13, 4, 120, 255), (14, 4, 120, 256), (15, 5, 150, 257), (16, 5, 300, 1023),
             (17, 6, 300, 1025), (18, 6, 300, 4097)]
# the other maps of that file, with random_scene's keyword arguments
GPU_OTHER_CASES = [((21, 5, 150, 700), {}), ((22, 4, 120, 300), {}), ((23, 40, 40, 60), dict(max_obs=40, pose_scale=0.1)),
                   ((24, 4, 150, 257), {}), ((25, 5, 200, 257), {}), ((26, 4, 200, 400), dict(bad_frac=0.1)), ((27, 4, 120, 256), {})]
