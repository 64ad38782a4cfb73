"""Deterministic case builders for the triangulation / track-selection / culling / rigid-move envelope, shared by
test_tri_cases_cpu.py (oracle against the float64 referee tri_ref.py) and test_gpu_triangulate_envelope.py (kernels
against both).  Every builder is a pure function of its arguments; results are cached and must not be written to."""
import functools

import numpy as np

K = np.array([1000.0, 1000.0, 960.0, 540.0], np.float32)
WIDTH, HEIGHT = 1920, 1080
GATES = ((0.9999, 2.0), (1.0, 4.0))          # (min_parallax_cosine, max_reprojection_error): the strict and the loose pair

# one and two elements per thread of the 1024-thread compactions, and the edges of their 8- and 16-wide load batches
COMPACTION_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384, 16385)
KEEP_PATTERNS = ("all", "none", "first", "last", "alternating", "random10", "random50", "random90")

# Far depths.  The band of the referee's cosine at the gate cos <= 1.0 is gamma(10) = 6.0e-7 wide (tri_ref.py): a point
# at depth d seen over a baseline b has 1 - cos = (b_perp / d)^2 / 2, so with b_perp = 0.3 m the band starts at d = 270 m,
# and half a pixel of noise (5e-4 rad against a parallax of 0.3 / d) spreads the triangulated depth by d / 600 of itself.
# 30 .. 60 m keeps the parallax at 5e-3 .. 1e-2 rad (0.2 m for the synthetic pair: 3.5e-3 and more), five noise sigmas
# and more from zero; at 40 .. 100 m the synthetic pair had 5 % of its points inside the band, and the 60 .. 400 m of
# synth.make_tracks puts a third of them there.  test_tri_cases_cpu.py asserts the resulting share.
FAR_DEPTH = (30.0, 60.0)
NEAR_DEPTH = (3.0, 25.0)
BASELINE, WIDE_BASELINE, WIDE_DEPTH = 0.32, 3.0, (10.0, 25.0)


def rodrigues(axis, deg):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    a = np.deg2rad(deg)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def pose(R_wc, centre):
    """world -> camera, row-major [16] f32, from the camera-to-world rotation and the centre."""
    T = np.eye(4)
    T[:3, :3] = R_wc.T
    T[:3, 3] = -R_wc.T @ np.asarray(centre, np.float64)
    return T.astype(np.float32).reshape(16)


def project(T, X):
    T = np.asarray(T, np.float64).reshape(4, 4)
    c = X @ T[:3, :3].T + T[:3, 3]
    with np.errstate(all="ignore"):
        return np.stack([K[0] * c[:, 0] / c[:, 2] + K[2], K[1] * c[:, 1] / c[:, 2] + K[3]], 1), c[:, 2]


# name: (rotation of view 1 about a general axis [deg] or None = the synthetic pair, relative turn [deg], world offset [m],
#        depth range, pixel noise, share of outliers, baseline [m])
# At 1000 m the referee's own SVD term decides what can be compared: the homogeneous system carries the offset in its last
# column, the relative gap falls to 1e-5 and below, and 1e-13 / gap on the unit null vector is 1e3 * 1e3 times that on the
# point (|X| / h_3).  Over 0.3 m of baseline that is more than two pixels of bound on the pixel error, above the gate itself.
# The f32 camera point R X + t itself is only good to gamma(3) * 2700 m = 5e-4 m there, f / depth times that in pixels.  The
# two 1000 m families therefore take WIDE_BASELINE and WIDE_DEPTH, where the bound on the pixel error is a third of a pixel.
PAIR_FAMILIES = {
    "synthetic_near": (None, 2.0, 0.0, NEAR_DEPTH, 0.5, 0.05, BASELINE),
    "synthetic_far": (None, 2.0, 0.0, FAR_DEPTH, 0.5, 0.0, BASELINE),
    "axis30_turn1_near": (30.0, 1.0, 0.0, NEAR_DEPTH, 0.5, 0.05, BASELINE),
    "axis90_turn5_off10_near": (90.0, 5.0, 10.0, NEAR_DEPTH, 0.5, 0.05, BASELINE),
    "axis180_turn20_off10_noise15": (180.0, 20.0, 10.0, NEAR_DEPTH, 1.5, 0.10, BASELINE),
    "axis120_turn1_off10_far": (120.0, 1.0, 10.0, FAR_DEPTH, 0.5, 0.0, BASELINE),
    "axis45_turn20_far": (45.0, 20.0, 0.0, FAR_DEPTH, 0.5, 0.05, BASELINE),
    "axis135_turn5_off1000_wide": (135.0, 5.0, 1000.0, WIDE_DEPTH, 0.5, 0.05, WIDE_BASELINE),
    "axis60_turn20_off1000_wide": (60.0, 20.0, 1000.0, WIDE_DEPTH, 0.5, 0.05, WIDE_BASELINE),
}
FAMILY_SIZE = 400


def _pair(seed, n, rot, turn, offset, depth, noise, outliers, baseline=BASELINE):
    """Two views of n landmarks in view 1's frustum, `outliers` of them with the view-2 pixel 8 .. 30 px off on both axes."""
    rng = np.random.default_rng(seed)
    if rot is None:
        R1, c1 = np.eye(3), np.zeros(3)
        R2, c2 = rodrigues([0, 1, 0], turn), np.array([0.2, 0.0, 0.05])
    else:
        axis = rng.normal(size=3)
        R1 = rodrigues(axis, rot)
        c1 = offset * np.array([0.6, -0.48, 0.64])
        R2 = R1 @ rodrigues(rng.normal(size=3), turn)
        c2 = c1 + R1 @ (baseline / 0.32 * np.array([0.3, 0.05, 0.08]))
    T1, T2 = pose(R1, c1), pose(R2, c2)
    z = rng.uniform(depth[0], depth[1], n)
    u, v = rng.uniform(100, WIDTH - 100, n), rng.uniform(100, HEIGHT - 100, n)
    Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)
    X = Xc @ R1.T + c1
    uv1, _ = project(T1, X)
    uv2, _ = project(T2, X)
    uv1 = uv1 + rng.normal(0, noise, uv1.shape)
    uv2 = uv2 + rng.normal(0, noise, uv2.shape)
    out = rng.random(n) < outliers
    uv2[out] += rng.uniform(8, 30, (int(out.sum()), 2)) * rng.choice([-1.0, 1.0], (int(out.sum()), 2))
    return dict(uv1=uv1.astype(np.float32), uv2=uv2.astype(np.float32), poses=np.stack([T1, T2]), X=X, outlier=out, K=K)


@functools.lru_cache(maxsize=None)
def pair_family(name, n=FAMILY_SIZE):
    rot, turn, offset, depth, noise, outliers, baseline = PAIR_FAMILIES[name]
    return _pair(1000 + sorted(PAIR_FAMILIES).index(name), n, rot, turn, offset, depth, noise, outliers, baseline)


# ----------------------------------------------------------------------------------- degenerate and non-finite rows
@functools.lru_cache(maxsize=None)
def edge_rows():
    """Rows for the per-item-pose form of K4: finite but degenerate inputs, then non-finite pixels.  Returns uv1, uv2 [m][2],
    poses [5][16], idx1, idx2 [m], names [m]."""
    rng = np.random.default_rng(77)
    R1 = rodrigues([0.3, 1.0, -0.2], 25.0)
    c1 = np.array([2.0, -1.0, 3.0])
    R2 = R1 @ rodrigues([0.1, 1.0, 0.0], 4.0)
    c2 = c1 + R1 @ np.array([0.3, 0.02, 0.06])
    # a third camera that looks along view 1's x axis from 6 m ahead: view 1's landmarks near its own z = 0 plane
    R3 = R1 @ rodrigues([0, 1, 0], 90.0)
    poses = [pose(R1, c1), pose(R2, c2), None, pose(np.eye(3), np.zeros(3))]
    z = rng.uniform(4, 12, 4)
    u, v = rng.uniform(300, 1600, 4), rng.uniform(200, 900, 4)
    X = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1) @ R1.T + c1
    p1, _ = project(poses[0], X)
    p2, _ = project(poses[1], X)
    rows = []

    def add(name, a, b, i1, i2):
        for x, y in zip(a, b):
            rows.append((name, x, y, i1, i2))

    add("identical_poses_identical_pixels", p1, p1, 0, 0)
    add("identical_poses_shifted_pixels", p1, p1 + np.array([5.0, 0.0]), 0, 0)
    add("swapped_views", p2, p1, 0, 1)
    # view 3's centre sits so that landmark 0 has depth +1e-3 / -1e-3 in it: a point on its z = 0 plane as nearly as a finite pixel allows
    axis3 = R3[:, 2]
    for slot, dz in ((2, 1e-3), (4, -1e-3)):
        T3 = pose(R3, X[0] - dz * axis3 - 0.4 * R3[:, 0])
        if slot == 2:
            poses[2] = T3
        else:
            poses.append(T3)
        p3, _ = project(T3, X[:1])
        add("on_view2_z0_plane", p1[:1], p3, 0, slot)
    # the landmark on view 1's optical axis: its pixel is the principal point exactly
    Xa = (np.array([[0.0, 0.0, 7.0]]) @ R1.T + c1)
    pa2, _ = project(poses[1], Xa)
    add("principal_point", np.array([[float(K[2]), float(K[3])]]), pa2, 0, 1)
    add("principal_point", pa2, np.array([[float(K[2]), float(K[3])]]), 1, 0)
    add("identity_pose_pair", p1[:1], p1[:1] + 3.0, 3, 3)
    n_finite = len(rows)
    for bad in (np.nan, np.inf, -np.inf):
        for view in (0, 1):
            for comp in (0, 1):
                a, b = p1[1].copy(), p2[1].copy()
                (a if view == 0 else b)[comp] = bad
                rows.append(("nonfinite_view%d" % (view + 1), a, b, 0, 1))
    # ordinary correspondences in between, so that the compaction has something to keep around the odd rows
    for i in range(4):
        rows.insert(3 * i, ("ordinary", p1[i], p2[i], 0, 1))
    return dict(names=[r[0] for r in rows], uv1=np.array([r[1] for r in rows], np.float32), uv2=np.array([r[2] for r in rows], np.float32),
                idx1=np.array([r[3] for r in rows], np.int32), idx2=np.array([r[4] for r in rows], np.int32),
                poses=np.stack(poses), n_finite=n_finite + 4, K=K)


# ------------------------------------------------------------------------------------------------- compactions
def keep_pattern(name, n):
    k = np.zeros(n, bool)
    if name == "all":
        k[:] = True
    elif name == "first":
        k[0] = True
    elif name == "last":
        k[-1] = True
    elif name == "alternating":
        k[::2] = True
    elif name.startswith("random"):
        k = np.random.default_rng([n, int(name[6:])]).random(n) < int(name[6:]) / 100.0
    else:
        assert name == "none"
    return k


@functools.lru_cache(maxsize=None)
def _compaction_base(n):
    return _pair(4242 + n, n, 30.0, 2.0, 0.0, (3.0, 6.0), 0.0, 0.0)


def compaction_case(pattern, n):
    """n correspondences whose keep flags under the strict gates are exactly keep_pattern(pattern, n): noise-free
    landmarks at 3 .. 6 m (parallax 0.025 rad and more even towards the baseline's side of the image: cos < 0.9997), the others with the view-2 pixel 200 px off."""
    base = _compaction_base(n)
    keep = keep_pattern(pattern, n)
    uv2 = base["uv2"].copy()
    uv2[~keep, 1] += np.float32(200.0)
    return dict(uv1=base["uv1"], uv2=uv2, poses=base["poses"], keep=keep, K=K)


# --------------------------------------------------------------------------------------------- selection tables
def trajectory(n_frames=12):
    """The camera path of synth.make_tracks: 0.4 degrees of yaw, 0.03 m sideways and 0.12 m forward per frame."""
    out = np.zeros((n_frames, 16), np.float32)
    for f in range(n_frames):
        out[f] = pose(rodrigues([0, 1, 0], 0.4 * f), np.array([0.03 * f, 0.0, 0.12 * f]))
    return out


def track_scene(kinds, seed, dups=(), low=()):
    """One track per character of `kinds`:  A accepted (3 .. 8 m, first sighted 11 frames back), R rejected (30 .. 70 m,
    first sighted 3 frames back: parallax under one degree), I inconsistent (A with one sighting 10 .. 30 px off),
    S skipped, E without sightings, N a candidate with a NaN cosine (R with a NaN key-frame pixel).  All landmarks lie
    left of the image centre, away from the epipole of the forward motion.  dups: (source, destination) pairs, the
    destination track becomes a byte-for-byte copy of the source; low: R tracks put at 25 m at the image's left edge, where the
    parallax of this motion is largest (0.0116 rad against 0.0103 and less for the others): the smallest cosines."""
    rng = np.random.default_rng(seed)
    poses = trajectory(12)
    kf = 11
    Tk = poses[kf].reshape(4, 4).astype(np.float64)
    n = len(kinds)
    tracks = []
    for t, kind in enumerate(kinds):
        far = kind in "RN"
        depth = rng.uniform(30, 70) if far else rng.uniform(3, 8)
        u, v = rng.uniform(200, 760), rng.uniform(200, 880)
        if t in low:
            depth, u, v = 25.0, 200.0, 540.0
        Xc = np.array([(u - K[2]) / K[0] * depth, (v - K[3]) / K[1] * depth, depth])
        Xw = (Xc - Tk[:3, 3]) @ Tk[:3, :3]
        frames = [] if kind == "E" else ([8, 9, 10] if far else [0, 4, 7, 10])
        suv = []
        for j, f in enumerate(frames):
            px = project(poses[f], Xw[None])[0][0] + rng.normal(0, 0.2, 2)
            if kind == "I" and j == 1 + t % 3:
                px = px + rng.uniform(10, 30, 2) * rng.choice([-1.0, 1.0], 2)
            suv.append(px)
        tuv = project(poses[kf], Xw[None])[0][0] + rng.normal(0, 0.2, 2)
        if kind == "N":
            tuv[t % 2] = np.nan
        tracks.append([tuv, frames, suv, 1 if kind == "S" else 0])
    for src, dst in dups:
        tracks[dst] = tracks[src]
    ptr = np.concatenate([[0], np.cumsum([len(t[1]) for t in tracks])]).astype(np.int32)
    sp = np.array([f for t in tracks for f in t[1]], np.int32).reshape(-1)
    suv = np.array([p for t in tracks for p in t[2]], np.float32).reshape(-1, 2)
    return dict(track_uv=np.array([t[0] for t in tracks], np.float32).reshape(n, 2), skip=np.array([t[3] for t in tracks], np.uint8),
                sight_ptr=ptr, sight_pose=sp, sight_uv=suv, poses=poses, kf_pose=kf, K=K, kinds=kinds)


def _mixed(n, seed, letters="ARIS", weights=(0.3, 0.4, 0.15, 0.15)):
    rng = np.random.default_rng(seed)
    return "".join(rng.choice(list(letters), n, p=weights))


def _quotas(kinds):
    na, nr = kinds.count("A"), kinds.count("R") + kinds.count("N")
    return {"q0": 0, "qacc": na, "qacc1": na + 1, "qall": na + nr, "qbeyond": na + nr + 7}


@functools.lru_cache(maxsize=None)
def selection_tables():
    """name -> (kinds, dups, low, quota).  The scene of a table is track_scene(kinds, seed_of(name), dups, low)."""
    T = {}
    for kind in "ARISE":
        T["one_" + kind] = (kind, (), (), 1)
    T["one_A_q0"] = ("A", (), (), 0)
    T["one_R_q0"] = ("R", (), (), 0)
    for n in (1023, 1024, 1025, 2049):
        kinds = _mixed(n, n)
        q = _quotas(kinds)
        names = q if n == 1025 else {"qacc1": q["qacc1"]} if n != 2049 else {"qacc1": q["qacc1"], "qall": q["qall"]}
        for qn in names:
            T["mixed_%d_%s" % (n, qn)] = (kinds, (), (), q[qn])
    T["all_accepted_1025"] = ("A" * 1025, (), (), 100)
    T["all_accepted_1025_qbeyond"] = ("A" * 1025, (), (), 2000)
    T["all_rejected_1025"] = ("R" * 1025, (), (), 100)
    T["all_rejected_1025_qall"] = ("R" * 1025, (), (), 1025)
    T["all_inconsistent_1025"] = ("I" * 1025, (), (), 100)
    T["all_skipped_1025"] = ("S" * 1025, (), (), 100)
    T["all_empty_65"] = ("E" * 65, (), (), 100)
    # equal cosines: with 2049 tracks a thread of the selection owns 3; 9..11 is one thread's chunk, 14 | 15 the border of two.
    # The copied tracks are the nearest of the rejected, so they head the order and a small quota cuts through a run.
    dups = ((9, 10), (9, 11), (14, 15), (300, 301), (300, 302), (300, 303), (300, 304))
    low = (9, 14, 300)
    for q in (1, 2, 4, 6, 9, 10, 2049):
        T["equal_runs_2049_q%d" % q] = ("R" * 2049, dups, low, q)
    kinds = list(_mixed(2049, 5))
    for t in (9, 10, 11, 14, 15, 300, 301, 302, 303, 304):
        kinds[t] = "R"
    kinds = "".join(kinds)
    T["equal_runs_mixed_2049"] = (kinds, dups, low, kinds.count("A") + 5)
    # NaN cosines among the rejected
    base = "R" * 64
    T["nan_first_q5"] = ("N" + base[1:], (), (), 5)
    T["nan_first_qall"] = ("N" + base[1:], (), (), 64)
    several = list(base)
    for t in (0, 7, 8, 31, 63):
        several[t] = "N"
    several = "".join(several)
    T["nan_several_q5"] = (several, (), (), 5)
    T["nan_several_q60"] = (several, (), (), 60)            # 59 numbers, then the first NaN in track order
    T["nan_several_qall"] = (several, (), (), 64)
    T["nan_only_q5"] = ("N" * 64, (), (), 5)
    T["nan_only_qbeyond"] = ("N" * 64, (), (), 100)
    mixed = list(_mixed(1025, 9))
    for t in range(3, 1025, 41):
        mixed[t] = "N"
    mixed = "".join(mixed)
    T["nan_mixed_1025"] = (mixed, (), (), mixed.count("A") + mixed.count("R") + 3)
    return T


@functools.lru_cache(maxsize=None)
def selection_scene(name):
    kinds, dups, low, quota = selection_tables()[name]
    sc = track_scene(kinds, 9000 + sorted(selection_tables()).index(name) % 7, dups, low)
    sc["quota"] = quota
    return sc


# ---------------------------------------------------------------------------------------------------------- K12
def _general_poses(n, seed, offset=10.0, spread=0.4, turn=6.0):
    """n poses around a base pose of general orientation: centres within `spread` m, turned by up to `turn` degrees."""
    rng = np.random.default_rng(seed)
    R0 = rodrigues(rng.normal(size=3), rng.uniform(20, 170))
    c0 = offset * np.array([0.6, -0.48, 0.64])
    Rs, cs = [], []
    for _ in range(n):
        Rs.append(R0 @ rodrigues(rng.normal(size=3), rng.uniform(0, turn)))
        cs.append(c0 + R0 @ rng.uniform(-spread, spread, 3))
    return R0, c0, Rs, cs


@functools.lru_cache(maxsize=None)
def k12_scene():
    """600 points (three blocks of 256 lanes) under 8 general poses and one that looks the other way (w < 0: the (-1, -1)
    rule).  Observation lists of 0, 1, 2, 17 and 128 entries; the points at 255, 256 and 257 have none."""
    rng = np.random.default_rng(1212)
    R0, c0, Rs, cs = _general_poses(8, 12)
    poses = [pose(R, c) for R, c in zip(Rs, cs)] + [pose(R0 @ rodrigues([0, 1, 0], 180.0), c0)]
    n = 600
    z = rng.uniform(4, 20, n)
    u, v = rng.uniform(300, 1600, n), rng.uniform(200, 900, n)
    X = (np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1) @ R0.T + c0).astype(np.float32)
    counts = np.array([(0, 1, 2, 17, 1, 2, 128, 1, 2, 2)[i % 10] for i in range(n)])
    counts[[255, 256, 257]] = 0
    counts[[0, 254, 258, n - 1]] = (128, 17, 2, 1)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    op = rng.integers(0, 8, ptr[-1]).astype(np.int32)
    op[rng.random(len(op)) < 0.02] = 8
    owner = np.repeat(np.arange(n), counts)
    uv = np.zeros((len(op), 2))
    for k in range(9):
        m = op == k
        uv[m] = project(poses[k], X[owner[m]].astype(np.float64))[0]
    uv[op == 8] = rng.uniform(-3, 3, (int((op == 8).sum()), 2))           # around (-1, -1): both sides of 3 px
    noisy = rng.random(n) < 0.35                                           # points whose observations are 2 .. 6 px off
    uv += np.where(noisy[owner, None], rng.normal(0, 3.0, uv.shape), rng.normal(0, 0.5, uv.shape))
    return dict(positions=X, obs_ptr=ptr, obs_pose=op, obs_uv=uv.astype(np.float32), poses=np.stack(poses), K=K)


@functools.lru_cache(maxsize=None)
def k12_exact():
    """Integer-valued pixels under the identity pose: the point (0, 0, 1) projects to (960, 540) exactly, every error and
    every sum below is exact in f32.  Returns the scene and `expect` [n] (the cull flag) with `mean` [n]."""
    e = 2.0 ** -14                                     # one ulp of f32 at 963
    lists = [([(963, 540)], 3.0, 0), ([(960, 537)], 3.0, 0), ([(965, 540), (960, 541)], 3.0, 0), ([(964, 543), (961, 540)], 3.0, 0),
             ([(962, 540), (963, 540), (964, 540)], 3.0, 0), ([(963, 540)] * 17, 3.0, 0), ([(963, 540)] * 128, 3.0, 0),
             ([(963 + e, 540)], 3.0 + e, 1), ([(963 - e, 540)], 3.0 - e, 0), ([(963, 540), (963 + e, 540)], None, 1),
             ([(963, 540), (963 - e, 540)], None, 0), ([(964, 540)], 4.0, 1), ([(962, 540)], 2.0, 0), ([], 0.0, 0),
             ([(963, 544), (960, 539)], 3.0, 0), ([(963, 544), (960, 538)], 3.5, 1)]
    ptr = np.concatenate([[0], np.cumsum([len(l[0]) for l in lists])]).astype(np.int32)
    uv = np.array([p for l in lists for p in l[0]], np.float32).reshape(-1, 2)
    n = len(lists)
    mean = np.array([np.nan if l[1] is None else l[1] for l in lists])
    return dict(positions=np.tile(np.array([[0, 0, 1]], np.float32), (n, 1)), obs_ptr=ptr, obs_pose=np.zeros(len(uv), np.int32), obs_uv=uv,
                poses=np.eye(4, dtype=np.float32).reshape(1, 16), K=K, expect=np.array([l[2] for l in lists], np.uint8), mean=mean)


@functools.lru_cache(maxsize=None)
def k12_plane():
    """Points on the identity camera's z = 0 plane: w = 0 is not < 0, so the division yields inf (culled: inf > 3) or NaN
    (kept: the comparison fails), as in the reference's arithmetic."""
    X = np.array([[1, 1, 0], [0, 0, 0], [0, 0, 1], [-1, 2, 0], [1, 0, 0]], np.float32)
    return dict(positions=X, obs_ptr=np.arange(6, dtype=np.int32), obs_pose=np.zeros(5, np.int32),
                obs_uv=np.tile(np.array([[960, 540]], np.float32), (5, 1)), poses=np.eye(4, dtype=np.float32).reshape(1, 16), K=K)


CULL_SIZES = tuple(s for s in COMPACTION_SIZES if s <= 2049)


def k12_cull_case(pattern, n):
    """n points with one exact observation each, 10 px off where keep_pattern says `cull`, exact otherwise."""
    cull = keep_pattern(pattern, n)
    uv = np.tile(np.array([[960, 540]], np.float32), (n, 1))
    uv[cull, 0] = 970
    return dict(positions=np.tile(np.array([[0, 0, 1]], np.float32), (n, 1)), obs_ptr=np.arange(n + 1, dtype=np.int32),
                obs_pose=np.zeros(n, np.int32), obs_uv=uv, poses=np.eye(4, dtype=np.float32).reshape(1, 16), K=K, cull=cull)


# ----------------------------------------------------------------------------------------------------- K13, K14
def _moved_poses(n, seed):
    _, _, Rs, cs = _general_poses(n, seed, offset=10.0, spread=3.0, turn=40.0)
    rng = np.random.default_rng(seed + 1)
    before = np.stack([pose(R, c) for R, c in zip(Rs, cs)])
    after = np.stack([pose(R @ rodrigues(rng.normal(size=3), rng.uniform(0, 3)), c + rng.uniform(-0.2, 0.2, 3)) for R, c in zip(Rs, cs)])
    return before, after


@functools.lru_cache(maxsize=None)
def k13_case(n_frames, n, permuted):
    """n listed points, frames drawn from [0, n_frames) with every 9th entry -1 and every 11th n_frames (the point
    stays); point_idx None or a permutation into a position array of n + 5 rows."""
    rng = np.random.default_rng([13, n_frames, n, int(permuted)])
    before, after = _moved_poses(n_frames, 130 + n_frames)
    f = rng.integers(0, n_frames, n).astype(np.int32)
    f[4::9] = -1
    f[6::11] = n_frames
    if n_frames > 1:
        f[0], f[n - 1] = n_frames - 1, 0
    pos = (10.0 * np.array([0.6, -0.48, 0.64]) + rng.uniform(-15, 15, (n + 5, 3))).astype(np.float32)
    idx = rng.permutation(n + 5)[:n].astype(np.int32) if permuted else None
    return dict(point_idx=idx, frame_idx=f, before=before, after=after, positions=pos)


@functools.lru_cache(maxsize=None)
def k14_case(n=600, n_kf=7):
    """Observation lists of 0 .. 6 key frames with the owner (the smallest index) first, last or in the middle; every 13th
    list holds a -1 (the point stays); lists are empty at 255 .. 257 and for every 10th point.  No owner >= n_kf."""
    rng = np.random.default_rng(14)
    before, after = _moved_poses(n_kf, 140)
    lists = []
    for p in range(n):
        m = 0 if (p % 10 == 3 or p in (255, 256, 257)) else int(rng.integers(1, 7))
        l = sorted(rng.choice(n_kf, m, replace=False).tolist())
        if m:
            where = (0, m - 1, m // 2)[p % 3]
            l = l[1:where + 1] + l[:1] + l[where + 1:]
            if p % 13 == 5:
                l[int(rng.integers(0, m))] = -1
        lists.append(l)
    lists[0], lists[n - 1] = [n_kf - 1], [0]
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    kf = np.array([k for l in lists for k in l], np.int32).reshape(-1)
    pos = (10.0 * np.array([0.6, -0.48, 0.64]) + rng.uniform(-15, 15, (n, 3))).astype(np.float32)
    return dict(obs_ptr=ptr, obs_kf=kf, before=before, after=after, positions=pos, lists=lists)


def oracle_reanchor(oracle, c):
    """pyoracle.reanchor_points over the entries of case c whose frame exists (orc_reanchor_points takes no n_frames and
    would read past its pose arrays): the other points keep their bytes."""
    f = c["frame_idx"]
    ok = (f >= 0) & (f < len(c["before"]))
    idx = (np.arange(len(f), dtype=np.int32) if c["point_idx"] is None else c["point_idx"])[ok]
    return oracle.reanchor_points(idx, f[ok], c["before"], c["after"], c["positions"])
