"""Synthetic inputs for the hot path, shaped as SURVEY.md §8(d) / BASELINE.json configs.

All inputs are generated on the host with numpy's PCG64 (seed 0x5EED0000 +
config id) and handed unchanged to the GPU library, the oracle and the CPU
baseline, so every leg sees bit-identical arrays.  There is no dataset: the
reference's inputs are video frames; here keypoints are projections of random
landmarks and descriptors are random 256-bit strings with 5 % bit flips per
observation (true-match Hamming ~13, impostor ~128).
"""
import numpy as np

SEED_BASE = 0x5EED0000


def rng_for(config_id, stream=0):
    return np.random.default_rng([SEED_BASE + int(config_id), int(stream)])


def yaw_matrix(deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def make_pose(R_wc, centre):
    """world->camera 4x4 (f32) from camera-to-world rotation and centre."""
    T = np.eye(4)
    T[:3, :3] = R_wc.T
    T[:3, 3] = -R_wc.T @ centre
    return T.astype(np.float32)


def rodrigues(aa):
    th = np.linalg.norm(aa)
    if th < 1e-12:
        return np.eye(3)
    k = aa / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def log_so3(R):
    c = np.clip((np.trace(R) - 1) / 2, -1, 1)
    th = np.arccos(c)
    if th < 1e-12:
        return np.zeros(3)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2 * np.sin(th))
    return w * th


def random_descriptors(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def flip_bits(rng, desc, p=0.05):
    bits = np.unpackbits(desc, axis=1)
    flips = rng.random(bits.shape) < p
    return np.packbits(bits ^ flips.astype(np.uint8), axis=1)


def project(T, K, X):
    Xc = X @ T[:3, :3].T.astype(np.float64) + T[:3, 3].astype(np.float64)
    u = K[0] * Xc[:, 0] / Xc[:, 2] + K[2]
    v = K[1] * Xc[:, 1] / Xc[:, 2] + K[3]
    return np.stack([u, v], 1), Xc[:, 2]


def pair_config(config_id):
    if config_id == 1:
        return dict(width=640, height=480, K=np.array([500, 500, 320, 240], np.float32), n=500, unmatched=0.0)
    return dict(width=1920, height=1080, K=np.array([1000, 1000, 960, 540], np.float32), n=2000, unmatched=0.10)


def make_pair(config_id=2, seed_stream=0, n=None, pose_jitter=0.0):
    """Two-frame scene of cfg 1 / cfg 2: returns a dict with
    desc1/kp1 (train, the keyframe), desc2/kp2 (query, the new frame), poses [2][16], K.
    pose_jitter > 0 (cfg 4 batches): the second pose varies with the seed stream."""
    cfg = pair_config(config_id)
    rng = rng_for(config_id, seed_stream)
    N = cfg["n"] if n is None else int(n)
    K, W, H = cfg["K"].astype(np.float64), cfg["width"], cfg["height"]
    T1 = make_pose(np.eye(3), np.zeros(3))
    if pose_jitter > 0.0:
        jr = np.random.default_rng(0xC4 + seed_stream)
        T2 = make_pose(yaw_matrix(2.0 + pose_jitter * jr.uniform(-1, 1)),
                       np.array([0.2, 0.0, 0.05]) + pose_jitter * 0.05 * jr.uniform(-1, 1, 3))
    else:
        T2 = make_pose(yaw_matrix(2.0), np.array([0.2, 0.0, 0.05]))
    n_shared = int(round(N * (1.0 - cfg["unmatched"])))
    # landmarks uniform in frame 1's frustum, depth U[4,20]
    z = rng.uniform(4, 20, n_shared)
    u = rng.uniform(0, W, n_shared)
    v = rng.uniform(0, H, n_shared)
    X = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)
    base = random_descriptors(rng, n_shared)
    kp1, _ = project(T1, K, X)
    kp2, _ = project(T2, K, X)
    kp1 = kp1 + rng.normal(0, 0.5, kp1.shape)
    kp2 = kp2 + rng.normal(0, 0.5, kp2.shape)
    d1 = flip_bits(rng, base)
    d2 = flip_bits(rng, base)
    n_extra = N - n_shared
    if n_extra > 0:
        for kp, d in ((kp1, d1), (kp2, d2)):
            pass
        e1 = np.stack([rng.uniform(0, W, n_extra), rng.uniform(0, H, n_extra)], 1)
        e2 = np.stack([rng.uniform(0, W, n_extra), rng.uniform(0, H, n_extra)], 1)
        kp1 = np.concatenate([kp1, e1]); kp2 = np.concatenate([kp2, e2])
        d1 = np.concatenate([d1, random_descriptors(rng, n_extra)])
        d2 = np.concatenate([d2, random_descriptors(rng, n_extra)])
    # independent shuffles so that index i in frame 1 is not index i in frame 2
    p1 = rng.permutation(N)
    p2 = rng.permutation(N)
    return dict(desc1=np.ascontiguousarray(d1[p1]), kp1=kp1[p1].astype(np.float32),
                desc2=np.ascontiguousarray(d2[p2]), kp2=kp2[p2].astype(np.float32),
                poses=np.stack([T1.reshape(16), T2.reshape(16)]).astype(np.float32),
                K=cfg["K"], width=W, height=H,
                truth12=(np.argsort(p1), np.argsort(p2), n_shared))


def make_pair_batch(batch=64, config_id=2, first_stream=0, n=None, pose_jitter=1.0):
    """cfg 4 (BASELINE.json configs[3]): `batch` independent instances of the cfg-2 pair, stacked:
    desc1/desc2 [B][N][32], kp1/kp2 [B][N][2], poses [B][2][16], K."""
    prs = [make_pair(config_id, seed_stream=first_stream + b, n=n, pose_jitter=pose_jitter) for b in range(batch)]
    out = {k: np.ascontiguousarray(np.stack([p[k] for p in prs])) for k in ("desc1", "kp1", "desc2", "kp2", "poses")}
    out.update(K=prs[0]["K"], width=prs[0]["width"], height=prs[0]["height"], pairs=prs)
    return out


def make_ba_window(n_kf=20, n_points=10000, config_id=3, seed_stream=0, n_fixed=2,
                   run_min=2, run_max=10, pixel_noise=0.5, outlier_frac=0.02,
                   rot_noise_deg=0.5, trans_noise=0.01, depth_noise=0.01):
    """cfg 3 / cfg 5 window: keyframes on a gently curving forward track, each landmark
    seen by a run of consecutive keyframes.  Returns the flat BA problem
    (cams [C][6] = angle-axis(R_cw) + centre, points [P][3], CSR observations) plus
    the ground truth and the keyframe poses."""
    rng = rng_for(config_id, seed_stream)
    K = np.array([1000, 1000, 960, 540], np.float32)
    Kd = K.astype(np.float64)
    W, H = 1920, 1080
    R = np.eye(3)
    c = np.zeros(3)
    Rs, cs = [], []
    for i in range(n_kf):
        Rs.append(R.copy()); cs.append(c.copy())
        R = R @ yaw_matrix(1.5)
        c = c + R @ np.array([0, 0, 0.5])
    poses_true = np.stack([make_pose(Rs[i], cs[i]) for i in range(n_kf)])
    run_max = min(run_max, n_kf)
    run_len = rng.integers(run_min, run_max + 1, n_points)
    start = (rng.random(n_points) * (n_kf - run_len + 1)).astype(np.int64)
    mid = start + run_len // 2
    z = rng.uniform(4, 20, n_points)
    u = rng.uniform(0.1 * W, 0.9 * W, n_points)
    v = rng.uniform(0.1 * H, 0.9 * H, n_points)
    Xc = np.stack([(u - Kd[2]) / Kd[0] * z, (v - Kd[3]) / Kd[1] * z, z], 1)
    Rm = np.stack([Rs[m] for m in mid]); cm = np.stack([cs[m] for m in mid])
    X = np.einsum("nij,nj->ni", Rm, Xc) + cm
    obs_ptr = np.zeros(n_points + 1, np.int32)
    obs_ptr[1:] = np.cumsum(run_len)
    M = int(obs_ptr[-1])
    obs_cam = np.concatenate([np.arange(s, s + l) for s, l in zip(start, run_len)]).astype(np.int32)
    obs_pt = np.repeat(np.arange(n_points), run_len)
    uv = np.zeros((M, 2))
    for k in range(n_kf):
        sel = obs_cam == k
        if sel.any():
            uv[sel], _ = project(poses_true[k], Kd, X[obs_pt[sel]])
    uv += rng.normal(0, pixel_noise, uv.shape)
    out = rng.random(M) < outlier_frac
    uv[out] += rng.uniform(-30, 30, (int(out.sum()), 2))
    # perturbed initial state
    cams = np.zeros((n_kf, 6))
    cams_true = np.zeros((n_kf, 6))
    for i in range(n_kf):
        Rcw = Rs[i].T
        cams_true[i, :3] = log_so3(Rcw); cams_true[i, 3:] = cs[i]
        if i < n_fixed:
            cams[i] = cams_true[i]
        else:
            dR = rodrigues(rng.normal(0, np.deg2rad(rot_noise_deg) / np.sqrt(3), 3))
            cams[i, :3] = log_so3(dR @ Rcw)
            cams[i, 3:] = cs[i] + rng.normal(0, trans_noise * 0.5, 3)
    cams = cams.astype(np.float32).astype(np.float64)   # pack_pose output is f32-valued
    cams_true = cams_true.astype(np.float32).astype(np.float64)
    depth_scale = 1.0 + rng.normal(0, depth_noise, n_points)
    pts = cm + (X - cm) * depth_scale[:, None]
    pts = pts.astype(np.float32).astype(np.float64)     # MapPoint::position is f32
    cam_free = np.ones(n_kf, np.uint8)
    cam_free[:n_fixed] = 0
    return dict(cams=cams, cam_free=cam_free, points=pts, obs_ptr=obs_ptr, obs_cam=obs_cam,
                obs_uv=uv.astype(np.float32), K=K, cams_true=cams_true, points_true=X,
                poses_true=poses_true, width=W, height=H, run_start=start.astype(np.int32),
                run_len=run_len.astype(np.int32))


def make_imu(window, seed=11, duration=0.5, sigma_rot=2e-3, sigma_vel=2e-2, sigma_pos=1e-2, skip=(), pairs=None,
             durations=None, shuffle=None, cov_scale=1.0, cov_cond=None, gyro_bias_sigma=2.78e-5, accel_bias_sigma=2.79e-3,
             zero_bias_jacobian=False):
    """Synthetic IMU factor pairs for a BA window (reference src/Optimization.cpp:317-346): one per pair of consecutive
    FREE cameras (pairs listed in `skip` are left out, like a gap with fewer than two samples), consistent with the
    ground-truth trajectory up to noise:
        delta R = R_i R_j^T,  delta v = R_i (v_j - v_i - g T),  delta p = R_i (c_j - c_i - v_i T - g T^2 / 2)
    (R = world -> camera; the residual of src/ImuFactor.cpp:66-69 vanishes on them).  Covariances are random SPD
    matrices of realistic scale, the bias Jacobians random, and the current bias estimates differ slightly from the
    biases used at preintegration so that the first-order bias correction (:49-61) is exercised.  Also returns the
    perturbed initial velocities / biases per camera (cam_velocity [C][3], cam_bias [C][6]) and gravity.
    Envelope knobs (the defaults reproduce the original output bit for bit):
      pairs               explicit (cam_i, cam_j) list instead of the consecutive free pairs: any two cameras, either
                          order, repeats allowed (`skip` is not applied)
      durations           per-factor preintegration time (one per factor; default `duration` for all)
      shuffle             seed of a permutation of the factor order (velocities / biases are those of the unshuffled list)
      cov_scale, cov_cond the covariance times cov_scale; cov_cond: its eigenvalues respread geometrically over that
                          condition number below the largest one (eigenvectors and their order kept)
      gyro_bias_sigma, accel_bias_sigma  the bias random-walk densities
      zero_bias_jacobian  all bias Jacobians zero (no first-order bias correction)"""
    rng = np.random.default_rng(0x1A2B0000 + seed)
    cams_true = window["cams_true"]
    C = len(cams_true)
    T = float(duration)
    g = np.array([0.0, 0.0, -9.80665])
    Rcw = np.stack([rodrigues(cams_true[c, :3]) for c in range(C)])
    ctr = cams_true[:, 3:]
    v_true = np.zeros((C, 3))
    for c in range(C):
        n = min(c + 1, C - 1)
        p = max(n - 1, 0)
        v_true[c] = (ctr[n] - ctr[p]) / T if n != p else 0.0
    free = np.flatnonzero(window["cam_free"])
    fac = dict(cam_i=[], cam_j=[], duration=[], rotation=[], velocity=[], position=[], covariance=[], bias_gyro=[],
               bias_accel=[], bias_jacobian=[])
    if pairs is None:
        pairs = [(int(a), int(b)) for a, b in zip(free[:-1], free[1:]) if b == a + 1 and (int(a), int(b)) not in skip]
    if durations is not None and len(durations) != len(pairs):
        raise ValueError("one duration per factor")
    for f, (a, b) in enumerate(pairs):
        T = float(duration) if durations is None else float(durations[f])
        dR = Rcw[a] @ Rcw[b].T @ rodrigues(rng.normal(0, sigma_rot, 3))
        dv = Rcw[a] @ (v_true[b] - v_true[a] - g * T) + rng.normal(0, sigma_vel, 3)
        dp = Rcw[a] @ (ctr[b] - ctr[a] - v_true[a] * T - 0.5 * g * T * T) + rng.normal(0, sigma_pos, 3)
        A = rng.normal(0, 1, (9, 9)) * np.array([sigma_rot] * 3 + [sigma_vel] * 3 + [sigma_pos] * 3)[:, None] * 0.3
        cov = A @ A.T + np.diag(np.array([sigma_rot] * 3 + [sigma_vel] * 3 + [sigma_pos] * 3) ** 2)
        if cov_scale != 1.0:
            cov = cov * cov_scale
        if cov_cond is not None:
            ev, Q = np.linalg.eigh(cov)
            spread = ev[-1] * np.geomspace(1.0 / float(cov_cond), 1.0, 9)      # ascending like eigh's eigenvalues
            cov = (Q * spread) @ Q.T
            cov = 0.5 * (cov + cov.T)
        bj = rng.normal(0, 1, (9, 6)) * np.array([T] * 3 + [T] * 3 + [T * T] * 3)[:, None] * 0.5
        if zero_bias_jacobian:
            bj = np.zeros_like(bj)
        fac["cam_i"].append(a); fac["cam_j"].append(b); fac["duration"].append(T)
        fac["rotation"].append(dR.reshape(9)); fac["velocity"].append(dv); fac["position"].append(dp)
        fac["covariance"].append(cov.reshape(81)); fac["bias_gyro"].append(rng.normal(0, 1e-3, 3))
        fac["bias_accel"].append(rng.normal(0, 1e-2, 3)); fac["bias_jacobian"].append(bj.reshape(54))
    out = {k: np.array(v, np.int32 if k.startswith("cam_") else np.float64) for k, v in fac.items()}
    nF = len(out["cam_i"])
    bias = np.zeros((C, 6))
    for f in range(nF):
        i = out["cam_i"][f]
        bias[i, :3] = out["bias_gyro"][f] + rng.normal(0, 2e-4, 3)
        bias[i, 3:] = out["bias_accel"][f] + rng.normal(0, 2e-3, 3)
    if nF:
        bias[out["cam_j"][-1]] = bias[out["cam_i"][-1]] + rng.normal(0, 1e-4, 6)
    out.update(cam_velocity=v_true + rng.normal(0, 0.05, (C, 3)), cam_bias=bias, gravity=g, cam_velocity_true=v_true,
               gyro_bias_sigma=gyro_bias_sigma, accel_bias_sigma=accel_bias_sigma)      # defaults: imu::NoiseDensity, src/Imu.h:42-49
    if shuffle is not None and nF:
        perm = np.random.default_rng(0x5EED0000 + int(shuffle)).permutation(nF)
        for k in fac:
            out[k] = out[k][perm]
    return out


def shard_ba_by_landmark(prob, n_shards, shard, bounds=None):
    """Landmark shard `shard` of `n_shards` (contiguous blocks of landmarks;
    cameras replicated) — SURVEY.md §8(e).  bounds: explicit split points [n_shards + 1]
    (equal bounds give an empty shard)."""
    P = len(prob["points"])
    lo = (P * shard) // n_shards if bounds is None else int(bounds[shard])
    hi = (P * (shard + 1)) // n_shards if bounds is None else int(bounds[shard + 1])
    o0, o1 = int(prob["obs_ptr"][lo]), int(prob["obs_ptr"][hi])
    out = dict(prob)
    out["points"] = prob["points"][lo:hi].copy()
    out["obs_ptr"] = (prob["obs_ptr"][lo:hi + 1] - o0).astype(np.int32)
    out["obs_cam"] = prob["obs_cam"][o0:o1].copy()
    out["obs_uv"] = prob["obs_uv"][o0:o1].copy()
    out["point_range"] = (lo, hi)
    return out


def make_match_scene(window=None, n_keypoints=2000, config_id=3, seed_stream=7, matched_frac=0.3,
                     kdtree_build=None):
    """Reprojection-gated matching scene (a2): the newest frame of a BA window
    against the window's landmarks.  Every landmark observation gets a
    descriptor row in the pool; the frame sees a subset of the landmarks plus
    clutter keypoints; `matched_frac` of its keypoints are already matched."""
    if window is None:
        window = make_ba_window(config_id=config_id)
    rng = rng_for(config_id, seed_stream)
    K = window["K"].astype(np.float64)
    W, H = window["width"], window["height"]
    P = len(window["points"])
    n_kf = len(window["cams"])
    X = window["points_true"]
    # the frame: one step beyond the last keyframe
    T_last = window["poses_true"][-1].astype(np.float64)
    R_wc = T_last[:3, :3].T @ yaw_matrix(1.5)
    centre = -T_last[:3, :3].T @ T_last[:3, 3] + R_wc @ np.array([0, 0, 0.5])
    pose = make_pose(R_wc, centre)
    uv, zc = project(pose, K, X)
    vis = (zc > 0.5) & (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)
    vis_idx = np.flatnonzero(vis)
    n_seen = min(len(vis_idx), int(n_keypoints * 0.8))
    seen = rng.choice(vis_idx, n_seen, replace=False) if n_seen > 0 else np.zeros(0, np.int64)
    base = random_descriptors(rng, P)
    kp = uv[seen] + rng.normal(0, 1.5, (n_seen, 2))
    desc = flip_bits(rng, base[seen])
    n_extra = n_keypoints - n_seen
    kp = np.concatenate([kp, np.stack([rng.uniform(0, W, n_extra), rng.uniform(0, H, n_extra)], 1)])
    desc = np.concatenate([desc, random_descriptors(rng, n_extra)])
    perm = rng.permutation(n_keypoints)
    kp = kp[perm].astype(np.float32)
    desc = np.ascontiguousarray(desc[perm])
    kp_matched = (rng.random(n_keypoints) < matched_frac).astype(np.uint8)
    # observation descriptors: one pool row per observation
    M = len(window["obs_cam"])
    obs_pt = np.repeat(np.arange(P), np.diff(window["obs_ptr"]))
    desc_pool = flip_bits(rng, base[obs_pt])
    obs_desc = rng.permutation(M).astype(np.int32)        # rows are not in observation order
    pool = np.zeros_like(desc_pool)
    pool[obs_desc] = desc_pool
    kf_centers = window["cams_true"][:, 3:].astype(np.float32)
    eligible = (rng.random(P) < 0.9).astype(np.uint8)
    frame = dict(pose=pose.reshape(16), K=window["K"], width=W, height=H, keypoints=kp,
                 descriptors=desc, kp_matched=kp_matched)
    if kdtree_build is not None:
        node_kp, left, right, root = kdtree_build(kp)
        frame.update(kd_node_kp=node_kp, kd_left=left, kd_right=right, kd_root=root)
    mp = dict(positions=window["points"].astype(np.float32), eligible=eligible,
              obs_ptr=window["obs_ptr"], obs_kf=window["obs_cam"], obs_desc=obs_desc,
              kf_centers=kf_centers, desc_pool=pool)
    return frame, mp


def make_tracks(n_tracks=2000, n_frames=12, config_id=6, outlier_frac=0.05, noise_px=0.5, far_frac=0.3,
                max_sightings=10, image=(1920, 1080), K=(1000.0, 1000.0, 960.0, 540.0)):
    """Synthetic input of Mapper::triangulate_tracks (reference src/Mapper.cpp:222-305): a forward-moving,
    gently turning camera (`n_frames` trajectory poses, the last one is the key frame), `n_tracks` feature
    tracks, each sighted in a run of consecutive frames ending at the key frame.  `far_frac` of the landmarks
    are far away (low parallax: they exercise the requirement / quota top-up), `outlier_frac` of the tracks
    get one corrupted sighting (inconsistent)."""
    rng = np.random.default_rng(0x5EED0000 + config_id)
    fx, fy, cx, cy = K
    W, H = image
    poses = np.zeros((n_frames, 16), np.float32)
    for f in range(n_frames):
        yaw = np.deg2rad(0.4 * f)
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        c = np.array([0.03 * f, 0.0, 0.12 * f])
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = -R @ c
        poses[f] = T.astype(np.float32).reshape(16)
    kf = n_frames - 1
    Tk = poses[kf].reshape(4, 4).astype(np.float64)
    # landmarks in the key frame's frustum
    depth = np.where(rng.random(n_tracks) < far_frac, rng.uniform(60, 400, n_tracks), rng.uniform(3, 25, n_tracks))
    u = rng.uniform(50, W - 50, n_tracks)
    v = rng.uniform(50, H - 50, n_tracks)
    Xc = np.stack([(u - cx) / fx * depth, (v - cy) / fy * depth, depth], 1)
    Xw = (Xc - Tk[:3, 3]) @ Tk[:3, :3]          # R^T (Xc - t)
    track_uv = np.zeros((n_tracks, 2), np.float32)
    sight_ptr = [0]
    sight_pose, sight_uv = [], []
    skip = (rng.random(n_tracks) < 0.03).astype(np.uint8)
    for t in range(n_tracks):
        ns = int(rng.integers(0, max_sightings + 1)) if rng.random() < 0.03 else int(rng.integers(2, max_sightings + 1))
        ns = min(ns, kf)
        frames = list(range(kf - ns, kf))           # sightings in the frames before the key frame
        bad = rng.random() < outlier_frac and ns >= 2
        bad_at = int(rng.integers(1, ns)) if bad else -1
        for j, f in enumerate(frames):
            T = poses[f].reshape(4, 4).astype(np.float64)
            pc = T[:3, :3] @ Xw[t] + T[:3, 3]
            px = np.array([fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy]) + rng.normal(0, noise_px, 2)
            if j == bad_at:
                px += rng.uniform(8, 30, 2) * rng.choice([-1, 1], 2)
            sight_pose.append(f)
            sight_uv.append(px)
        pk = Tk[:3, :3] @ Xw[t] + Tk[:3, 3]
        track_uv[t] = np.array([fx * pk[0] / pk[2] + cx, fy * pk[1] / pk[2] + cy]) + rng.normal(0, noise_px, 2)
        sight_ptr.append(len(sight_pose))
    return dict(track_uv=track_uv, skip=skip, sight_ptr=np.array(sight_ptr, np.int32),
                sight_pose=np.array(sight_pose, np.int32).reshape(-1),
                sight_uv=np.array(sight_uv, np.float32).reshape(-1, 2), poses=poses, kf_pose=kf,
                K=np.array(K, np.float32))


def make_pose_graph(n_kf=60, n_loops=3, laps=1.25, drift_rot=2e-3, drift_trans=2e-2, loop_noise=(2e-3, 1e-2),
                    outlier_loops=0, seed=0):
    """Key frames of a camera driving `laps` laps of an oval (y up, gravity = -y), odometry with accumulated drift, and
    loop constraints between key frames that see the same place one lap apart (reference LoopDetector -> pose_graph,
    src/Slam.cpp:258-268).  Returns dict(poses [n,4,4] f32 drifted world->camera, poses_true, loops [(from, to,
    relative 4x4 f64)], gravity): relative = T_from T_to^-1 measured on the TRUE trajectory plus noise, `from` the newer
    key frame as the detector emits them.  `outlier_loops` of them get a gross error (exercises the Huber loss)."""
    rng = np.random.default_rng(0x50600000 + seed)
    per_lap = int(round(n_kf / laps))
    T_true = []
    for i in range(n_kf):
        a = 2 * np.pi * i / per_lap
        centre = np.array([40.0 * np.cos(a), 0.3 * np.sin(3 * a), 25.0 * np.sin(a)])
        R_wc = yaw_matrix(-np.rad2deg(a)) @ rodrigues(np.array([0.02 * np.sin(2 * a), 0.0, 0.03 * np.cos(a)]))
        T_true.append(make_pose(R_wc, centre).astype(np.float64))
    T_true = np.stack(T_true)
    # odometry: true relative motion + noise, chained from the first true pose
    T = [T_true[0]]
    for i in range(1, n_kf):
        rel = T_true[i] @ np.linalg.inv(T_true[i - 1])               # T_i = rel T_{i-1}
        N = np.eye(4)
        N[:3, :3] = rodrigues(rng.normal(0, drift_rot, 3))
        N[:3, 3] = rng.normal(0, drift_trans, 3)
        T.append(N @ rel @ T[-1])
    poses = np.stack(T).astype(np.float32)
    loops = []
    cand = [i for i in range(per_lap, n_kf)]
    pick = rng.choice(cand, size=min(n_loops, len(cand)), replace=False) if cand else []
    for k, i in enumerate(sorted(int(v) for v in pick)):
        j = i - per_lap
        rel = T_true[i] @ np.linalg.inv(T_true[j])
        N = np.eye(4)
        N[:3, :3] = rodrigues(rng.normal(0, loop_noise[0], 3))
        N[:3, 3] = rng.normal(0, loop_noise[1], 3)
        if k < outlier_loops:
            N[:3, :3] = rodrigues(np.array([0.0, 0.4, 0.0]))
            N[:3, 3] = np.array([3.0, 0.0, -2.0])
        loops.append((i, j, N @ rel))
    return dict(poses=poses, poses_true=T_true, loops=loops, gravity=np.array([0.0, -9.80665, 0.0]))


def _value_noise(grid, x, y, scale):
    """C1 value noise: the lattice `grid` (spacing `scale` pixels) interpolated with smoothstep weights at (x, y)."""
    gx, gy = x / scale, y / scale
    x0, y0 = np.floor(gx).astype(np.int64), np.floor(gy).astype(np.int64)
    tx, ty = gx - x0, gy - y0
    tx, ty = tx * tx * (3 - 2 * tx), ty * ty * (3 - 2 * ty)
    h, w = grid.shape
    x0, y0 = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    g00, g01, g10, g11 = grid[y0, x0], grid[y0, x0 + 1], grid[y0 + 1, x0], grid[y0 + 1, x0 + 1]
    return (g00 * (1 - tx) + g01 * tx) * (1 - ty) + (g10 * (1 - tx) + g11 * tx) * ty


def make_klt_pair(config_id=2, seed=0, n_points=2000):
    """Two grey frames for the KLT stage (Tracker::track_features, src/Tracker.cpp:90-134) with a known motion.
    cfg 2: 1920x1080, cfg 1: 640x480.  Frame 1 is multi-scale value noise (periods 3 .. 48 px) over a flat rectangle;
    frame 2 is frame 1 warped by q = c + s R(theta) (p - c) + t (sub-pixel translation, a slight rotation and scale)
    with an occluding patch of independent texture pasted in.  Points, [n][2] f32, with `label`:
      0 textured (high gradient, away from the borders), 1 flat (minEig failures), 2 leaving the image (their motion
      target lies >= 3 px outside frame 2), 3 inside the occluded patch (forward-backward failures).
    `mask` is the static mask with a zeroed bottom band (the car's hood); `truth` = the motion target of every point;
    `bgr1` / `bgr2` are BGR frames whose grey conversion (BT.601, 8-bit) is `img1` / `img2`'s content source."""
    cfg = pair_config(config_id)
    W, H = cfg["width"], cfg["height"]
    rng = rng_for(config_id, 40 + int(seed))
    scales, amps = (3, 6, 12, 24, 48), (10.0, 18.0, 26.0, 30.0, 34.0)
    grids = [rng.normal(0, 1, (H // s + 8, W // s + 8)) for s in scales]
    occ_grid = rng.normal(0, 1, (H // 4 + 8, W // 4 + 8))
    flat = (int(0.10 * W), int(0.15 * H), int(0.10 * W) + max(W // 10, 90), int(0.15 * H) + max(H // 8, 70))   # x0 y0 x1 y1
    occ = (int(0.62 * W), int(0.30 * H), int(0.62 * W) + max(W // 8, 110), int(0.30 * H) + max(W // 8, 110))
    c = np.array([W / 2.0, H / 2.0])
    theta, s, t = np.deg2rad(0.25 + 0.1 * rng.uniform()), 1.0 + 0.003 * (1 + rng.uniform()), rng.uniform(1.2, 2.4, 2)
    R = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])

    def tex(x, y, chan=0):
        v = 128.0 + sum(a * _value_noise(g, x + 4 * sc + 7 * chan, y + 4 * sc + 3 * chan, sc)
                        for g, a, sc in zip(grids, amps, scales))
        inflat = (x >= flat[0] - 0.5) & (x < flat[2] - 0.5) & (y >= flat[1] - 0.5) & (y < flat[3] - 0.5)
        return np.where(inflat, 96.0, v)

    def warp_inv(x, y):      # frame-2 pixel -> frame-1 position
        q = np.stack([x - c[0] - t[0], y - c[1] - t[1]], -1) @ R / s     # R^T (q - c - t) / s, row vectors
        return q[..., 0] + c[0], q[..., 1] + c[1]

    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f1 = tex(xx, yy)
    u, v = warp_inv(xx, yy)
    f2 = tex(u, v)
    inocc = (xx >= occ[0]) & (xx < occ[2]) & (yy >= occ[1]) & (yy < occ[3])
    f2 = np.where(inocc, 128.0 + 45.0 * _value_noise(occ_grid, xx, yy, 4), f2)
    q8 = lambda f: np.clip(np.rint(f), 0, 255).astype(np.uint8)      # noqa: E731
    img1, img2 = q8(f1), q8(f2)

    # points: textured ones at the strongest gradient cells of a coarse grid, then the special sets
    gy_, gx_ = np.gradient(f1)
    mag = np.hypot(gx_, gy_)
    cell = 12
    n_flat, n_leave, n_occ = 60, 40, 80
    n_tex = n_points - n_flat - n_leave - n_occ
    bx, by = 30, 30
    cand = []
    for y0 in range(by, H - by - cell, cell):
        for x0 in range(bx, W - bx - cell, cell):
            blk = mag[y0:y0 + cell, x0:x0 + cell]
            k = int(np.argmax(blk))
            cand.append((blk.flat[k], x0 + k % cell, y0 + k // cell))
    cand = np.array(cand)
    px, py = cand[:, 1], cand[:, 2]
    far = lambda r, m: (px < r[0] - m) | (px >= r[2] + m) | (py < r[1] - m) | (py >= r[3] + m)     # noqa: E731
    cand = cand[far(flat, 24) & far(occ, 24)]
    cand = cand[np.argsort(-cand[:, 0], kind="stable")][:n_tex]
    tex_pts = cand[:, 1:3] + rng.uniform(-0.5, 0.5, (len(cand), 2))
    flat_pts = np.stack([rng.uniform(flat[0] + 16, flat[2] - 16, n_flat), rng.uniform(flat[1] + 16, flat[3] - 16, n_flat)], 1)
    occ_pts = np.stack([rng.uniform(occ[0] + 32, occ[2] - 32, n_occ), rng.uniform(occ[1] + 32, occ[3] - 32, n_occ)], 1)
    # leaving: the motion target lies 3 .. 12 px beyond the right / bottom border of frame 2
    leave = []
    while len(leave) < n_leave:
        side = len(leave) % 2
        p = np.array([W - 1.0 - rng.uniform(0, 3), rng.uniform(40, H - 40)]) if side == 0 else \
            np.array([rng.uniform(40, W - 40), H - 1.0 - rng.uniform(0, 3)])
        q = c + s * R @ (p - c) + t
        if (q[0] >= W + 2.5) or (q[1] >= H + 2.5):
            leave.append(p)
        else:
            p[side] += 1.0
            p[side] = min(p[side], (W, H)[side] - 0.01)
            q = c + s * R @ (p - c) + t
            if (q[0] >= W + 2.5) or (q[1] >= H + 2.5):
                leave.append(p)
    leave_pts = np.array(leave)
    pts = np.concatenate([tex_pts, flat_pts, leave_pts, occ_pts])
    label = np.concatenate([np.zeros(len(tex_pts)), np.ones(n_flat), np.full(n_leave, 2), np.full(n_occ, 3)]).astype(np.int8)
    order = rng.permutation(len(pts))
    pts, label = pts[order].astype(np.float32), label[order]
    truth = (pts.astype(np.float64) - c) @ (s * R).T + c + t
    mask = np.full((H, W), 255, np.uint8)
    mask[int(0.85 * H):] = 0
    # BGR frames: per-channel offsets around the grey content (their BT.601 grey is what the tracker sees)
    def bgr(img):
        g = img.astype(np.int64)
        b = np.clip(g + 20, 0, 255); r = np.clip(g - 15, 0, 255)
        return np.ascontiguousarray(np.stack([b, np.clip(g, 0, 255), r], -1).astype(np.uint8))
    return dict(img1=img1, img2=img2, bgr1=bgr(img1), bgr2=bgr(img2), pts=pts, label=label, truth=truth, mask=mask,
                width=W, height=H, motion=dict(theta=theta, scale=s, t=t, centre=c), flat=flat, occluder=occ)


def make_corner_scene(width=640, height=480, seed=0, side=16, spacing=48, band=(0.70, 0.80)):
    """A grey frame with known corners for the corner detector (Tracker::track_features' replenishment, GFTT): bright
    axis-aligned squares of `side` px on a grid of `spacing` px (each jittered by a few px) over a dark noise floor
    (0 .. 2 grey levels).  A square covering pixels [x0, x0 + side) x [y0, y0 + side) has its corners at the pixel
    boundaries (x0 - 0.5, y0 - 0.5) ... (x0 + side - 0.5, y0 + side - 0.5).  `mask` is all-255 except a zeroed
    horizontal band (rows band[0] .. band[1] of the height).  Returns dict(img, mask, corners [n][2] f64)."""
    rng = np.random.default_rng(1000 + int(seed))
    img = 60 + rng.integers(0, 3, (height, width))
    corners = []
    for gy in range(spacing // 2, height - side - spacing // 2, spacing):
        for gx in range(spacing // 2, width - side - spacing // 2, spacing):
            x0, y0 = gx + int(rng.integers(-4, 5)), gy + int(rng.integers(-4, 5))
            img[y0:y0 + side, x0:x0 + side] = 190 + int(rng.integers(0, 40))
            corners += [(x0 - 0.5, y0 - 0.5), (x0 + side - 0.5, y0 - 0.5), (x0 - 0.5, y0 + side - 0.5),
                        (x0 + side - 0.5, y0 + side - 0.5)]
    mask = np.full((height, width), 255, np.uint8)
    mask[int(band[0] * height):int(band[1] * height)] = 0
    return dict(img=img.astype(np.uint8), mask=mask, corners=np.array(corners), width=width, height=height)


def make_dot_chain(n=30, spacing=3, direction=(1, 0), width=320, height=240, base=250, step=2, background=40):
    """A grey frame that makes the corner detector's minimum-distance walk long (its rounds, csrc/gftt.hip): a chain of
    `n` bright 2x2 dots on a flat background, dot i at start + i * spacing * direction with grey level base - step * i,
    so the response falls along the chain.  With spacing 3 (4 along an axis, or 3 diagonally) and min_distance 5,
    consecutive dots lie closer than the distance and every second dot does not: each dot's fate waits for the one
    before it, and the synchronous rounds grow with n.  The chain is centred in the frame.  Returns dict(img, dots
    [n][2] int (x, y) of each dot's top-left pixel)."""
    dx, dy = direction
    assert base - step * (n - 1) > background + 16, "contrast must stay well above the background"
    ext_x, ext_y = (n - 1) * spacing * dx, (n - 1) * spacing * dy
    x0, y0 = (width - 2 - ext_x) // 2, (height - 2 - ext_y) // 2
    dots = np.array([(x0 + i * spacing * dx, y0 + i * spacing * dy) for i in range(n)], np.int64)
    assert (dots.min(0) >= 8).all() and (dots[:, 0].max() < width - 9) and (dots[:, 1].max() < height - 9), "chain leaves the frame"
    img = np.full((height, width), background, np.uint8)
    for i, (x, y) in enumerate(dots):
        img[y:y + 2, x:x + 2] = base - step * i
    return dict(img=img, dots=dots, width=width, height=height)


def make_refine_problem(n=600, seed=0, outlier_frac=0.0, noise_px=0.0, rot0=None, rot_err=0.02, offset=0.0,
                        trans_err=0.05, bad_depth_frac=0.0, imu=False, width=640, height=480):
    """One frame's pose solve (optimization::refine_pose, reference src/Optimization.cpp:194-267): n world points with
    their observations in the frame and a starting camera cam0 (angle-axis | centre, p = R(aa) (X - centre)).

    rot0: the starting angle-axis, used bit for bit (None: a random rotation of 0.3 rad); the true rotation is
    R(e) R(rot0) with |e| = rot_err, so a solve leaves rot0 on its first step.  offset: distance of the true centre from
    the origin along a random direction (the points travel with it); trans_err: distance of cam0's centre from the true
    one.  Observations are the true projections plus Gaussian noise of noise_px (f32); a fraction outlier_frac of them is
    moved by 20..120 px in a random direction.  A fraction bad_depth_frac of the points lies near or behind the true
    camera's image plane (camera-frame depth in [-2, 0.05], a few of them at |depth| <= 1e-4), observed at random
    pixels.  imu=True adds a one-factor InertialDelta built by make_imu on the (previous, this) pair of true cameras:
    delta = dict(imu, prev_pose, prev_velocity, prev_bias, velocity) as refine_pose_inertial takes it.
    Returns dict(cam0, points [n][3] f64, uv [n][2] f32, K (f32 fx, fy, cx, cy), cam_true, outlier [n] bool,
    bad_depth [n] bool, delta or None)."""
    rng = np.random.default_rng([0x5EED7E00, int(seed)])
    K = np.array([450.0, 445.0, width / 2.0, height / 2.0], np.float32)
    fx, fy, cx, cy = [float(k) for k in K]
    if rot0 is None:
        d = rng.normal(size=3)
        rot0 = 0.3 * d / np.linalg.norm(d)
    rot0 = np.asarray(rot0, np.float64)
    e = rng.normal(size=3)
    e *= rot_err / np.linalg.norm(e)
    R_true = rodrigues(e) @ rodrigues(rot0)
    u = rng.normal(size=3)
    c_true = float(offset) * u / np.linalg.norm(u)
    t = rng.normal(size=3)
    c0 = c_true + float(trans_err) * t / np.linalg.norm(t)
    cam_true = np.concatenate([log_so3(R_true), c_true])
    cam0 = np.concatenate([rot0, c0])
    # points in the true camera's frame: in front (depth 2..30) or, for the bad fraction, near / behind the image plane
    px = np.stack([rng.uniform(0, width, n), rng.uniform(0, height, n)], 1)
    depth = rng.uniform(2.0, 30.0, n)
    bad = rng.random(n) < bad_depth_frac
    depth[bad] = rng.uniform(-2.0, 0.05, int(bad.sum()))
    tiny = bad & (rng.random(n) < 0.2)
    depth[tiny] = rng.uniform(-1e-4, 1e-4, int(tiny.sum()))
    p = np.stack([(px[:, 0] - cx) / fx * depth, (px[:, 1] - cy) / fy * depth, depth], 1)
    points = p @ R_true + c_true                       # X = R^T p + c
    q = (points - c_true) @ R_true.T
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([fx * q[:, 0] / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy], 1)
    uv[bad] = np.stack([rng.uniform(0, width, int(bad.sum())), rng.uniform(0, height, int(bad.sum()))], 1)
    uv[~bad] += rng.normal(0.0, 1.0, (int((~bad).sum()), 2)) * noise_px
    out = ~bad & (rng.random(n) < outlier_frac)
    ang = rng.uniform(0, 2 * np.pi, int(out.sum()))
    mag = rng.uniform(20.0, 120.0, int(out.sum()))
    uv[out] += np.stack([np.cos(ang), np.sin(ang)], 1) * mag[:, None]
    delta = None
    if imu:
        T = 0.5
        prev_c = c_true - rng.normal(0.0, 0.5, 3)
        prev_aa = log_so3(rodrigues(rng.normal(0.0, 0.02, 3)) @ R_true)
        win = dict(cams_true=np.stack([np.concatenate([prev_aa, prev_c]), cam_true]), cam_free=np.ones(2, np.uint8))
        f = make_imu(win, seed=int(seed), duration=T)
        delta = dict(imu=f, prev_pose=win["cams_true"][0], prev_velocity=f["cam_velocity_true"][0],
                     prev_bias=f["cam_bias"][0], velocity=f["cam_velocity"][1])
    return dict(cam0=cam0, points=points, uv=uv.astype(np.float32), K=K, cam_true=cam_true, outlier=out,
                bad_depth=bad, delta=delta)


POSE_MOTIONS = ("forward", "sideways", "small", "rotation", "planar")


def make_pose_pair(seed=0, n=2000, outlier_frac=0.3, noise_px=0.5, motion="forward", width=1280, height=720, K=None,
                   rotvec=None, epipole_points=0):
    """Matched pixels of two views for the relative-pose stage (pose::estimate_pose, src/PoseEstimation.cpp:59-88) with a
    known motion X2 = R X1 + t.  motion: "forward" (the dash-cam case: t mostly along the optical axis, the epipole
    inside the image), "sideways", "small" (a baseline of 2 cm against depths of 4 .. 40 m), "rotation" (3 degrees with a
    baseline of 1 mm) or "planar" (every point on one tilted plane).  Inliers are the true projections plus Gaussian
    noise of noise_px; a fraction outlier_frac of the points is moved to a random pixel of the second image.
    Knobs (the defaults give the arrays of the plain call): K = (fx, fy, cx, cy) replaces the intrinsics (700, 700, centre);
    rotvec replaces the motion's axis-angle rotation (radians, before the same jitter); epipole_points > 0 puts the last
    epipole_points matches exactly on the epipoles (the other camera's centre seen from each view, noise-free, inliers),
    where E x1 = E^T x2 = 0 and the Sampson denominator vanishes.
    Returns dict(pts_from, pts_to [n][2] f32, K (f32 fx, fy, cx, cy), R [3][3], t [3] (unit), inlier [n] bool)."""
    rng = np.random.default_rng([0x905E, POSE_MOTIONS.index(motion), int(seed)])
    K = np.array([700.0, 700.0, width / 2.0, height / 2.0] if K is None else K, np.float32)
    fx, fy, cx, cy = (float(k) for k in K)
    aa = {"forward": (0.0, 0.02, 0.0), "sideways": (0.0, 0.035, 0.005), "small": (0.01, 0.01, 0.0),
          "rotation": (0.01, 0.05, 0.0), "planar": (0.01, -0.02, 0.005)}[motion]
    tv = {"forward": (0.05, 0.02, 1.0), "sideways": (1.0, 0.05, 0.1), "small": (0.3, 0.1, 1.0),
          "rotation": (0.6, 0.2, 0.4), "planar": (0.3, 0.05, 1.0)}[motion]
    scale = {"small": 0.02, "rotation": 0.001}.get(motion, 1.0)
    R = rodrigues(np.array(aa if rotvec is None else rotvec, np.float64) + rng.normal(0, 0.002, 3))
    t = np.array(tv) + rng.normal(0, 0.02, 3)
    t /= np.linalg.norm(t)
    pf, pt, X = [], [], 0
    while X < n:
        m = 2 * n
        u = np.stack([rng.uniform(0, width, m), rng.uniform(0, height, m)], 1)
        ray = np.stack([(u[:, 0] - cx) / fx, (u[:, 1] - cy) / fy, np.ones(m)], 1)
        if motion == "planar":                        # plane n . X = 12 with n tilted towards the camera
            nrm = np.array([0.1, -0.3, 1.0])
            depth = 12.0 / (ray @ nrm)
        else:
            depth = rng.uniform(4.0, 40.0, m)
        P1 = ray * depth[:, None]
        P2 = P1 @ R.T + scale * t
        ok = (depth > 0.5) & (P2[:, 2] > 0.5)
        u2 = np.stack([fx * P2[:, 0] / P2[:, 2] + cx, fy * P2[:, 1] / P2[:, 2] + cy], 1)
        ok &= (u2[:, 0] >= 0) & (u2[:, 0] < width) & (u2[:, 1] >= 0) & (u2[:, 1] < height)
        pf.append(u[ok])
        pt.append(u2[ok])
        X += int(ok.sum())
    pf, pt = np.concatenate(pf)[:n], np.concatenate(pt)[:n]
    pf = pf + rng.normal(0, noise_px, pf.shape)
    pt = pt + rng.normal(0, noise_px, pt.shape)
    inlier = rng.random(n) >= outlier_frac
    bad = ~inlier
    pt[bad] = np.stack([rng.uniform(0, width, bad.sum()), rng.uniform(0, height, bad.sum())], 1)
    if epipole_points:
        c1 = -R.T @ t                                 # camera 2's centre in camera 1, and camera 1's in camera 2 (= t)
        k = int(epipole_points)
        pf[-k:] = (fx * c1[0] / c1[2] + cx, fy * c1[1] / c1[2] + cy)
        pt[-k:] = (fx * t[0] / t[2] + cx, fy * t[1] / t[2] + cy)
        inlier[-k:] = True
    return dict(pts_from=pf.astype(np.float32), pts_to=pt.astype(np.float32), K=K, R=R, t=t, inlier=inlier,
                width=width, height=height)


PNP_LAYOUTS = ("volume", "far", "near_planar", "narrow")


def make_pnp_scene(seed=0, n=2000, outlier_frac=0.3, noise_px=0.5, layout="volume", width=1280, height=720,
                   descriptors=False, K=None, rotvec=None, t=None, world_offset=None, plane=None):
    """Object points and their pixels for the absolute-pose stage (the cv::solvePnPRansac calls of LoopDetector's
    verify_pnp and Initialization's third-view check) under a known world -> camera pose.  layout: "volume" (depths of
    4 .. 40 m over the whole image), "far" (60 .. 200 m), "near_planar" (a tilted plane 12 m away, 2 cm thick) or
    "narrow" (the central 15 % of the image, 10 .. 30 m).  Inlier pixels are the projections of the f32 points plus
    Gaussian noise of noise_px; a fraction outlier_frac of the pixels is displaced by 20 .. 200 px in a random direction,
    so the true inlier set is unambiguous at a 2 px gate.
    Returns dict(points [n][3] f32, pixels [n][2] f32, K (f32 fx, fy, cx, cy), pose [4][4] f64 world -> camera,
    inlier [n] bool).  With descriptors=True the pixels are permuted and the dict also holds desc_points [n][32] u8
    (random_descriptors), desc_pixels [n][32] u8 (flip_bits of the point's row; random rows for outliers) and
    pixel_point [n] (the object point of each pixel); inlier then follows the pixels' order.
    The knobs leave the default output as it is: K = (fx, fy, cx, cy) replaces the centred 700 px camera; rotvec and t
    replace the drawn world -> camera pose; world_offset [3] moves the world's origin away from the scene (the points
    become Xw + offset, t becomes t - R offset, and the pixels are the projections of the f32-rounded points, so the
    returned pose stays their exact truth); plane = "z3" puts every point exactly on Z = 3 and "tilted" on
    Z = X / 2 + Y / 4 + 1 with X, Y multiples of 1 / 64 (exact in f32) instead of the layout's depths."""
    rng = np.random.default_rng([0x9A9, PNP_LAYOUTS.index(layout), int(seed)])
    K = np.array([700.0, 700.0, width / 2.0, height / 2.0] if K is None else K, np.float32)
    fx, fy, cx, cy = (float(k) for k in K)
    R = rodrigues(np.array([0.2, -0.4, 0.1]) + rng.normal(0, 0.05, 3))
    t_drawn = np.array([0.5, -0.3, 2.0]) + rng.normal(0, 0.2, 3)
    R = R if rotvec is None else rodrigues(np.asarray(rotvec, np.float64))
    t = t_drawn if t is None else np.asarray(t, np.float64)
    span = 0.15 if layout == "narrow" else 1.0
    u = np.stack([cx + span * rng.uniform(-0.5, 0.5, n) * width, cy + span * rng.uniform(-0.5, 0.5, n) * height], 1)
    ray = np.stack([(u[:, 0] - cx) / fx, (u[:, 1] - cy) / fy, np.ones(n)], 1)
    if layout == "near_planar":
        depth = 12.0 / (ray @ np.array([0.1, -0.3, 1.0])) + rng.uniform(-0.01, 0.01, n)
    else:
        lo, hi = {"volume": (4.0, 40.0), "far": (60.0, 200.0), "narrow": (10.0, 30.0)}[layout]
        depth = rng.uniform(lo, hi, n)
    Xc = ray * depth[:, None]
    Xw = (Xc - t) @ R                                 # R^T (Xc - t)
    if plane == "z3":
        Xw = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n), np.full(n, 3.0)], 1)
    elif plane == "tilted":
        g = rng.integers(-128, 129, (n, 2)) / 64.0
        Xw = np.stack([g[:, 0], g[:, 1], g[:, 0] / 2.0 + g[:, 1] / 4.0 + 1.0], 1)
    elif plane is not None:
        raise ValueError(plane)
    if world_offset is not None:
        off = np.asarray(world_offset, np.float64)
        Xw, t = Xw + off, t - R @ off
    Xw = Xw.astype(np.float32)
    Xf = Xw.astype(np.float64) @ R.T + t
    pix = np.stack([fx * Xf[:, 0] / Xf[:, 2] + cx, fy * Xf[:, 1] / Xf[:, 2] + cy], 1)
    pix = pix + rng.normal(0, noise_px, pix.shape)
    inlier = rng.random(n) >= outlier_frac
    bad = np.flatnonzero(~inlier)
    ang, mag = rng.uniform(0, 2 * np.pi, len(bad)), rng.uniform(20.0, 200.0, len(bad))
    pix[bad] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R, t
    out = dict(points=Xw, pixels=pix.astype(np.float32), K=K, pose=pose, inlier=inlier, width=width, height=height)
    if descriptors:
        dp = random_descriptors(rng, n)
        dq = flip_bits(rng, dp)
        dq[bad] = random_descriptors(rng, len(bad))
        perm = rng.permutation(n)
        out.update(pixels=out["pixels"][perm], inlier=inlier[perm], desc_points=dp, desc_pixels=np.ascontiguousarray(dq[perm]),
                   pixel_point=perm.astype(np.int32))
    return out


def _sparse_flips(rng, n):
    """[n][32] u8 masks with every bit set with probability 1/8."""
    return random_descriptors(rng, n) & random_descriptors(rng, n) & random_descriptors(rng, n)


def make_vocabulary(k, L, seed=0, ragged=False, stopped_fraction=0.0, duplicate_children=False):
    """A DBoW2-style vocabulary tree for key-frame recognition (LoopDetector's "Loop retrieval"): k children per node, L
    levels below the root.  A child's descriptor is its parent's with 1/8 of the bits flipped (the children of the root
    are random rows); leaves carry idf-like weights in [0.5, 8), inner nodes 0.  Node ids are a random numbering with
    parent < child, so a node's children are neither contiguous nor in creation order.
      ragged               about 15 % of the inner candidates above depth L become early leaves and the others get
                           1 .. k children (one-child nodes among them)
      stopped_fraction     that fraction of the leaves gets weight 0 (stopped words); 1.0 stops every word
      duplicate_children   in about 30 % of the families two siblings carry identical descriptors (ties)
    Returns dict(k, L, n_nodes, parent [n] i32 (parent[0] = -1), desc [n][32] u8, weight [n] f64, leaf [n] bool)."""
    rng = np.random.default_rng([0xB0, int(k), int(L), int(seed), int(ragged), int(duplicate_children)])
    parent, desc, depth = [np.array([-1], np.int64)], [np.zeros((1, 32), np.uint8)], [np.zeros(1, np.int64)]
    key = [np.array([-1.0])]
    level_ids, level_desc, level_key, total = np.array([0], np.int64), desc[0], key[0], 1
    for d in range(1, L + 1):
        m = len(level_ids)
        cnt = np.full(m, k, np.int64)
        if ragged and d > 1:                                    # (the root keeps its k children)
            cnt = rng.integers(1, k + 1, m)
            cnt[rng.random(m) < 0.2] = 1
            if d > 1:
                cnt[rng.random(m) < 0.15] = 0                   # early leaves
            if not cnt.any():
                cnt[0] = 1
        owner = np.repeat(np.arange(m), cnt)
        nc = len(owner)
        if nc == 0:
            break
        cd = random_descriptors(rng, nc) if d == 1 else level_desc[owner] ^ _sparse_flips(rng, nc)
        if duplicate_children:
            first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            fam = np.flatnonzero((cnt >= 2) & (rng.random(m) < 0.3))
            a = first[fam] + rng.integers(0, cnt[fam])
            b = first[fam] + (a - first[fam] + 1 + rng.integers(0, cnt[fam] - 1)) % cnt[fam]
            cd[b] = cd[a]
        parent.append(level_ids[owner])
        desc.append(cd)
        depth.append(np.full(nc, d, np.int64))
        ck = level_key[owner] + rng.random(nc) + 1e-9
        key.append(ck)
        level_ids, level_desc, level_key = total + np.arange(nc), cd, ck
        total += nc
    parent, desc, key = np.concatenate(parent), np.concatenate(desc), np.concatenate(key)
    order = np.argsort(key, kind="stable")                      # new id -> creation id; the root stays 0
    new_id = np.empty(total, np.int64)
    new_id[order] = np.arange(total)
    p = parent[order]
    p[1:] = new_id[p[1:]]
    desc = np.ascontiguousarray(desc[order])
    leaf = np.bincount(p[1:], minlength=total) == 0
    weight = np.zeros(total, np.float64)
    nl = int(leaf.sum())
    w = rng.uniform(0.5, 8.0, nl)
    w[rng.random(nl) < stopped_fraction] = 0.0
    weight[leaf] = w
    return dict(k=int(k), L=int(L), n_nodes=total, parent=p.astype(np.int32), desc=desc, weight=weight, leaf=leaf)


def make_bow_descriptors(voc, n, seed=0, noise=0.04, equidistant_fraction=0.1):
    """n ORB rows for make_vocabulary's tree `voc`: noisy copies (bit flips with probability `noise`) of random leaves'
    descriptors; a fraction equidistant_fraction of the rows is instead built exactly equidistant from two sibling
    leaves (half of the bits in which the two differ are taken from each; identical siblings are equidistant from any
    row), which exercises the descent's tie rule.  Returns [n][32] u8."""
    rng = np.random.default_rng([0xB1, int(seed), int(n)])
    leaves = np.flatnonzero(voc["leaf"])
    rows = flip_bits(rng, voc["desc"][leaves[rng.integers(0, len(leaves), n)]], noise) if n else np.zeros((0, 32), np.uint8)
    parent = voc["parent"]
    for r in np.flatnonzero(rng.random(n) < equidistant_fraction):
        a = leaves[rng.integers(0, len(leaves))]
        sib = np.flatnonzero(parent == parent[a]) if voc["n_nodes"] <= 4096 else \
            parent[a] + 1 + np.flatnonzero(parent[parent[a] + 1:parent[a] + 200001] == parent[a])
        sib = sib[sib != a]
        if not len(sib):
            continue
        b = sib[rng.integers(0, len(sib))]
        bits_a, bits_b = np.unpackbits(voc["desc"][a]), np.unpackbits(voc["desc"][b])
        diff = np.flatnonzero(bits_a != bits_b)
        diff = diff[:len(diff) - len(diff) % 2]
        take = rng.permutation(diff)[:len(diff) // 2]
        bits_a[take] = bits_b[take]
        rows[r] = np.packbits(bits_a)
    return np.ascontiguousarray(rows)


def loop_scene(seed=0, nq=300, candidates=((400, 200, 80, 0.3, None),), width=1280, height=720, drift=(0.03, 0.3), flip=0.03):
    """A query key frame and candidate key frames of one map, for LoopDetector's "Loop verify" stage (verify_pnp).
    candidates: one (n, matched, shared, outlier_frac, strip) per candidate key frame — n keypoints, `matched` of them
    (a random subset, point slots in random order) observe a map point, `shared` of those points are also seen by the
    query: a query keypoint carries the candidate's row with a fraction `flip` of its bits flipped and lies at the point's
    projection under the query's TRUE pose plus 0.5 px noise, except a fraction outlier_frac of the shared ones, which lie
    anywhere in the image (wrong matches).  strip = (x0, x1) as fractions of the width confines the correctly placed ones
    to that band.  All other rows are random, so they match nothing.  The candidates' shared query keypoints are disjoint
    (their sum must not exceed nq).  The query's pose in the map is the true one turned by drift[0] rad and moved by
    drift[1] m; a candidate's pose is the true one moved by a few decimetres.
    Returns dict(K, width, height, points [P][3] f32, key_frames: list of dict(kp [n][2] f32, desc [n][32] u8, pose [4][4]
    f32, kp_point [n] i32) with the query LAST, observations [(point, key frame, keypoint)] in the order to add them,
    query = its index, true_pose [4][4] f64, shared: per candidate (query keypoints, candidate keypoints, placed bool))."""
    rng = np.random.default_rng([0x100B, int(seed)])
    K = np.array([700.0, 700.0, width / 2.0, height / 2.0], np.float32)
    fx, fy, cx, cy = (float(k) for k in K)
    R = rodrigues(np.array([0.1, -0.2, 0.05]) + rng.normal(0, 0.05, 3))
    t = np.array([0.4, -0.2, 1.5]) + rng.normal(0, 0.2, 3)
    true_pose = np.eye(4)
    true_pose[:3, :3], true_pose[:3, 3] = R, t

    def moved(rot, trans):
        axis = rng.normal(0, 1, 3)
        dR = rodrigues(rot * axis / np.linalg.norm(axis))
        step = rng.normal(0, 1, 3)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = dR @ R, dR @ t + trans * step / np.linalg.norm(step)
        return T.astype(np.float32)

    def world_points(u):
        ray = np.stack([(u[:, 0] - cx) / fx, (u[:, 1] - cy) / fy, np.ones(len(u))], 1)
        Xc = ray * rng.uniform(4.0, 40.0, len(u))[:, None]
        return ((Xc - t) @ R).astype(np.float32)

    def anywhere(n):
        return np.stack([rng.uniform(0, width, n), rng.uniform(0, height, n)], 1)

    assert sum(c[2] for c in candidates) <= nq
    q_kp, q_desc = anywhere(nq), random_descriptors(rng, nq)
    q_free = rng.permutation(nq)
    points, key_frames, observations, shared_out = [], [], [], []
    n_points = 0
    for kf, (n, matched, shared, outlier_frac, strip) in enumerate(candidates):
        assert shared <= matched <= n
        kp, desc = anywhere(n), random_descriptors(rng, n)
        kps = np.sort(rng.choice(n, matched, replace=False)) if matched else np.zeros(0, np.int64)
        x0, x1 = strip if strip is not None else (0.02, 0.98)
        u = np.stack([rng.uniform(x0 * width, x1 * width, matched), rng.uniform(0.02 * height, 0.98 * height, matched)], 1)
        X = world_points(u)
        slots = n_points + rng.permutation(matched)              # keypoint kps[i] observes point slots[i]
        xyz = np.zeros((matched, 3), np.float32)
        xyz[slots - n_points] = X
        points.append(xyz)
        kp_point = np.full(n, -1, np.int32)
        kp_point[kps] = slots
        for i in rng.permutation(matched):
            observations.append((int(slots[i]), kf, int(kps[i])))
        # the shared ones in the query
        sh = rng.permutation(matched)[:shared]
        qk, q_free = q_free[:shared], q_free[shared:]
        Xf = X[sh].astype(np.float64) @ R.T + t
        pix = np.stack([fx * Xf[:, 0] / Xf[:, 2] + cx, fy * Xf[:, 1] / Xf[:, 2] + cy], 1) + rng.normal(0, 0.5, (shared, 2))
        placed = rng.random(shared) >= outlier_frac
        pix[~placed] = anywhere(int((~placed).sum()))
        q_kp[qk] = pix
        q_desc[qk] = flip_bits(rng, desc[kps[sh]], flip)
        shared_out.append((qk.astype(np.int32), kps[sh].astype(np.int32), placed))
        key_frames.append(dict(kp=kp.astype(np.float32), desc=desc, pose=moved(0.02, 0.3), kp_point=kp_point))
        n_points += matched
    key_frames.append(dict(kp=q_kp.astype(np.float32), desc=q_desc, pose=moved(*drift), kp_point=np.full(nq, -1, np.int32)))
    pts = np.concatenate(points) if points else np.zeros((0, 3), np.float32)
    return dict(K=K, width=width, height=height, points=pts, key_frames=key_frames, observations=observations,
                query=len(key_frames) - 1, true_pose=true_pose, shared=shared_out)
