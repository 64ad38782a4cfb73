"""Scenes and descriptor sets for the matcher envelope tests (tests/test_match_ref_cpu.py on the CPU,
tests/test_gpu_match_envelope.py on the GPU).  Every builder is a pure function of its arguments.

A scene is (frame, mp) in the layout of synth.make_match_scene: a camera looking at map points spread over (and
around) its image, key frames around the camera so that most points pass the viewing-angle and distance gates, a few
"odd" points observed only from far away key frames so that they fail them, keypoints near the projections of the
visible points (descriptors a chosen number of bits away from the point's) and clutter."""
import numpy as np


def flip_bits(rng, rows, k):
    """rows [n][32] uint8 with k[i] (0..256) distinct random bits of row i flipped."""
    n = len(rows)
    k = np.broadcast_to(np.asarray(k, np.int64), (n,))
    r = rng.random((n, 256))
    rank = np.argsort(np.argsort(r, 1), 1)
    mask = rank < k[:, None]
    return rows ^ np.packbits(mask, axis=1)


def descriptors(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def pose_matrix(R, centre):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ centre
    return T


def rot(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return Ry @ Rx


def _mask(rng, n, mode, frac):
    if mode == "none":
        return np.zeros(n, np.uint8)
    if mode == "all":
        return np.ones(n, np.uint8)
    return (rng.random(n) < frac).astype(np.uint8)


def assemble(rng, T, K, W, H, Xw, obs, kp, kdesc, base, kf_centres, odd_kfs, odd, matched="mixed", eligible="mixed",
             kdtree_build=None, pool_flip=(0, 6)):
    """frame, mp from world points Xw [P][3], their observation counts `obs` [P], keypoints kp [N][2] with descriptors
    kdesc, the points' descriptors base [P][32], near key frame centres and far ones (odd points use only those)."""
    P = len(Xw)
    n_near = len(kf_centres)
    centres = np.concatenate([kf_centres, odd_kfs]).astype(np.float32)
    obs_ptr = np.zeros(P + 1, np.int32)
    obs_ptr[1:] = np.cumsum(obs)
    okf = np.zeros(int(obs_ptr[-1]), np.int32)
    for p in range(P):
        o0, o1 = obs_ptr[p], obs_ptr[p + 1]
        if odd[p]:
            okf[o0:o1] = n_near + rng.integers(0, len(odd_kfs), o1 - o0)
        else:
            okf[o0:o1] = rng.choice(n_near, o1 - o0, replace=o1 - o0 > n_near)
    M = int(obs_ptr[-1])
    obs_pt = np.repeat(np.arange(P), obs)
    rows = flip_bits(rng, base[obs_pt], rng.integers(pool_flip[0], pool_flip[1] + 1, M)) if M else np.zeros((0, 32), np.uint8)
    perm = rng.permutation(M).astype(np.int32)          # pool rows are not in observation order
    pool = np.zeros((max(M, 1), 32), np.uint8)
    pool[perm] = rows
    N = len(kp)
    frame = dict(pose=np.asarray(T, np.float32).reshape(16), K=np.asarray(K, np.float32), width=int(W), height=int(H),
                 keypoints=np.ascontiguousarray(kp, np.float32).reshape(N, 2),
                 descriptors=np.ascontiguousarray(kdesc, np.uint8).reshape(N, 32),
                 kp_matched=_mask(rng, N, matched, 0.3))
    if kdtree_build is not None:
        node_kp, left, right, root = kdtree_build(frame["keypoints"])
        frame.update(kd_node_kp=node_kp, kd_left=left, kd_right=right, kd_root=root)
    mp = dict(positions=np.ascontiguousarray(Xw, np.float32).reshape(P, 3), eligible=_mask(rng, P, eligible, 0.9),
              obs_ptr=obs_ptr, obs_kf=okf if M else np.zeros(1, np.int32), obs_desc=perm if M else np.zeros(1, np.int32),
              kf_centers=centres, desc_pool=pool)
    return frame, mp


def scene(N, P, obs=(3,), W=1920, H=1080, K=None, seed=0, matched="mixed", eligible="mixed", behind=0.05, odd=0.08,
          flip=(3, 40), integer=False, outside=False, dup=0, kdtree_build=None):
    """General scene: N keypoints, P points with obs[p % len(obs)] observations each."""
    rng = np.random.default_rng(0x4D41 + 7919 * seed)
    fx, fy, cx, cy = K if K is not None else (0.8 * W, 0.8 * W + 11.0, 0.5 * W + 7.25, 0.5 * H - 3.5)
    centre = np.array([0.3, -0.2, 1.0])
    R = rot(0.1, 0.05)
    T = pose_matrix(R, centre)
    pu = rng.uniform(-0.1 * W, 1.1 * W, P)
    pv = rng.uniform(-0.1 * H, 1.1 * H, P)
    z = rng.uniform(4.0, 30.0, P)
    z[rng.random(P) < behind] *= -1.0
    Xc = np.stack([(pu - cx) / fx * z, (pv - cy) / fy * z, z], 1)
    Xw = Xc @ R + centre                                     # R^T Xc + centre
    obs_n = np.array([obs[p % len(obs)] for p in range(P)], np.int64)
    base = descriptors(rng, P)
    if dup:
        base = base[rng.integers(0, dup, P)]
    vis = np.flatnonzero((z > 0) & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H))
    n_seen = min(len(vis), int(np.ceil(0.6 * N)))
    seen = rng.choice(vis, n_seen, replace=False) if n_seen else np.zeros(0, np.int64)
    kp_seen = np.stack([pu[seen], pv[seen]], 1) + rng.normal(0, 2.0, (n_seen, 2))
    d_seen = flip_bits(rng, base[seen], rng.integers(flip[0], flip[1] + 1, n_seen))
    n_extra = N - n_seen
    lo_u, hi_u, lo_v, hi_v = (-30.0, W + 30.0, -30.0, H + 30.0) if outside else (0.0, W, 0.0, H)
    kp_extra = np.stack([rng.uniform(lo_u, hi_u, n_extra), rng.uniform(lo_v, hi_v, n_extra)], 1)
    d_extra = descriptors(rng, n_extra) if not dup else flip_bits(rng, base[rng.integers(0, P, n_extra)] if P else descriptors(rng, n_extra), rng.integers(20, 60, n_extra))
    kp = np.concatenate([kp_seen, kp_extra])
    kd = np.concatenate([d_seen, d_extra])
    if integer:
        kp = np.round(kp)
    perm = rng.permutation(N)
    kf_centres = centre + rng.normal(0, 0.4, (max(obs) + 4, 3))
    odd_kfs = np.concatenate([centre + np.array([25.0, 0, 0]) + rng.normal(0, 1, (3, 3)),
                              centre + np.array([0, 0, -60.0]) @ R + rng.normal(0, 1, (3, 3))])
    odd_pts = rng.random(P) < odd
    return assemble(rng, T, (fx, fy, cx, cy), W, H, Xw, obs_n, kp[perm], kd[perm], base, kf_centres, odd_kfs, odd_pts,
                    matched, eligible, kdtree_build)


def disc_scene(counts, obs=(4,), seed=0, matched="none", W=1280, H=720, kdtree_build=None, pad_to=0):
    """One point per entry of `counts`, each with exactly that many integer-pixel keypoints inside its 20-px disc (equal
    coordinates allowed) and none of any other point's: discs 64 px apart.  The keypoints of a disc carry three
    descriptor variants at equal distance from the point's, so that queued and on-the-spot candidates tie.  pad_to adds
    far-away clutter up to that many keypoints (to push the tree out of LDS)."""
    rng = np.random.default_rng(0xD15C + seed)
    fx, fy, cx, cy = 900.0, 905.0, 0.5 * W + 3.5, 0.5 * H - 1.25
    centre = np.array([0.0, 0.0, 0.0])
    R = rot(0.0, 0.0)
    T = pose_matrix(R, centre)
    P = len(counts)
    cols = (W - 80) // 64
    pu = 40.0 + 64.0 * (np.arange(P) % cols) + 0.37
    pv = 40.0 + 64.0 * (np.arange(P) // cols) + 0.41
    assert pv.max() < H - 40, "too many discs for the image"
    z = rng.uniform(6.0, 12.0, P)
    Xw = np.stack([(pu - cx) / fx * z, (pv - cy) / fy * z, z], 1)
    base = descriptors(rng, P)
    kp, kd = [], []
    for p, c in enumerate(counts):
        ang = rng.uniform(0, 2 * np.pi, c)
        rad = rng.uniform(0, 13.0, c)
        pts = np.round(np.stack([pu[p] + rad * np.cos(ang), pv[p] + rad * np.sin(ang)], 1))
        if c > 4:
            pts[: c // 4] = pts[0]                                 # equal coordinates
        variants = flip_bits(rng, np.repeat(base[p:p + 1], 3, 0), [9, 9, 9])
        kp.append(pts)
        kd.append(variants[rng.integers(0, 3, c)])
    kp = np.concatenate(kp) if kp else np.zeros((0, 2))
    kd = np.concatenate(kd) if kd else np.zeros((0, 32), np.uint8)
    if pad_to > len(kp):
        n = pad_to - len(kp)
        # clutter in a band below the discs' rows, > 20 px from every disc
        band0 = pv.max() + 30.0 if P else 0.0
        kp = np.concatenate([kp, np.stack([rng.uniform(0, W, n), rng.uniform(band0, H, n)], 1)])
        kd = np.concatenate([kd, descriptors(rng, n)])
    perm = rng.permutation(len(kp))
    obs_n = np.array([obs[p % len(obs)] for p in range(P)], np.int64)
    kf_centres = centre + rng.normal(0, 0.3, (max(obs) + 4, 3))
    odd_kfs = np.array([[30.0, 0, 0]])
    return assemble(rng, T, (fx, fy, cx, cy), W, H, Xw, obs_n, kp[perm], kd[perm], base, kf_centres, odd_kfs,
                    np.zeros(P, bool), matched, "all", kdtree_build, pool_flip=(0, 0))


# Edge geometry: identity pose, dyadic intrinsics and depths so that float32 and float64 agree exactly on where a
# point projects: fx != fy, the principal point off centre.
EDGE_K = (512.0, 384.0, 256.0, 192.0)
EDGE_WH = (640, 480)
EDGE_Z = 2.0
# (u, v, accepted by is_in_image): u == 0 / v == 0 are inside, u == width / v == height outside
EDGE_UV = [(0.0, 240.0, True), (640.0, 240.0, False), (320.0, 0.0, True), (320.0, 480.0, False), (0.0, 0.0, True),
           (640.0, 480.0, False), (639.5, 479.5, True), (-0.5, 100.0, False), (100.0, -0.5, False)]


def edge_scene(seed=0, kdtree_build=None, behind=True):
    rng = np.random.default_rng(0xED6E + seed)
    fx, fy, cx, cy = EDGE_K
    W, H = EDGE_WH
    uv = np.array([(u, v) for u, v, _ in EDGE_UV])
    z = np.full(len(uv), EDGE_Z)
    Xw = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    if behind:            # the same points mirrored behind the camera (z < 0): they project inside the image but are rejected
        Xb = Xw.copy()
        Xb[:, :2] *= -1.0
        Xb[:, 2] *= -1.0
        Xw = np.concatenate([Xw, Xb])
        uv = np.concatenate([uv, uv])
    P = len(Xw)
    base = descriptors(rng, P)
    kp, kd = [], []
    for p in range(P):
        # a keypoint on the projection, one just outside the image (negative or past the edge) and one inside
        for off, nb in (((0.0, 0.0), 2), ((-3.0, -2.0), 4), ((2.0, 3.0), 6)):
            kp.append((uv[p, 0] + off[0], uv[p, 1] + off[1]))
            kd.append(flip_bits(rng, base[p:p + 1], [nb])[0])
    kp = np.array(kp)
    kd = np.array(kd)
    kf_centres = rng.normal(0, 0.2, (6, 3))
    obs = np.full(P, 3)
    return assemble(rng, np.eye(4), EDGE_K, W, H, Xw, obs, kp, kd, base, kf_centres, np.array([[30.0, 0, 0]]),
                    np.zeros(P, bool), "none", "all", kdtree_build, pool_flip=(0, 0))


def project_f32(frame, X):
    """The float32 projection in the operation order rs_reproj_match documents (K * pose[:3] first, then the point;
    (a0 b0 + a1 b1) + (a2 b2 + a3 b3)), to check where a constructed point really lands."""
    f = np.float32
    T = np.asarray(frame["pose"], f).reshape(4, 4)
    fx, fy, cx, cy = [f(k) for k in frame["K"]]
    KP = np.zeros((3, 4), f)
    for j in range(4):
        KP[0, j] = (fx * T[0, j] + f(0) * T[1, j]) + cx * T[2, j]
        KP[1, j] = (f(0) * T[0, j] + fy * T[1, j]) + cy * T[2, j]
        KP[2, j] = (f(0) * T[0, j] + f(0) * T[1, j]) + f(1) * T[2, j]
    X = np.asarray(X, f).reshape(-1, 3)
    uvw = np.stack([(KP[i, 0] * X[:, 0] + KP[i, 1] * X[:, 1]) + (KP[i, 2] * X[:, 2] + KP[i, 3] * f(1)) for i in range(3)], 1)
    return uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2], uvw[:, 2]


# ------------------------------------------------------------------ descriptor sets for K1 / K1b
def knn_set(nq, nt, batch=1, seed=0, near=0.5):
    """batch x (queries, train): a fraction `near` of the queries are a few bits from a train row, the rest random."""
    rng = np.random.default_rng(0x4B31 + 131 * seed + nq * 7 + nt * 3 + batch)
    t = descriptors(rng, batch * nt).reshape(batch, nt, 32)
    q = descriptors(rng, batch * nq).reshape(batch, nq, 32)
    for b in range(batch):
        k = rng.random(nq) < near
        src = rng.integers(0, nt, int(k.sum()))
        q[b, k] = flip_bits(rng, t[b, src], rng.integers(0, 70, len(src)))
    return q, t


def k1_launch(nq, nt, batch):
    """The launch arithmetic of rs_hamming_knn2 (csrc/hamming.hip, knn2_launch): (nsplit, regime, rows_per_wave,
    number of empty waves).  regime: "one" (nsplit == 1 from the wave target), "split" (1 < nsplit < max_split) or
    "capped" (the wave target asks for more splits than nt / 32 allows)."""
    nqb = (nq + 63) // 64
    want = -(-2048 // (4 * nqb * batch))
    max_split = (nt + 31) // 32
    nsplit = max(1, min(want, max_split))
    rows = -(-nt // (nsplit * 4))
    empty = sum(1 for w in range(nsplit * 4) if w * rows >= nt)
    regime = "capped" if want > max_split else ("one" if nsplit == 1 else "split")
    return nsplit, regime, rows, empty


# ------------------------------------------------------------------ the reprojection-match cases
# name -> (builder, kwargs, [(replace, max_distance), ...]).  N > 6144 (K2_MAX_LDS_NODES) walks the tree in global memory.
_R01 = [(0, 64), (1, 64)]
REPROJ = {}
for _n in (1, 2, 63, 64, 65, 2000, 4096, 6144, 6145, 8192, 16384):
    REPROJ[f"N{_n}"] = (scene, dict(N=_n, P=400 if _n < 100 else 3000, seed=_n), _R01)
for _p in (0, 1, 63, 64, 65, 127, 128, 129, 10000, 50000):
    REPROJ[f"P{_p}"] = (scene, dict(N=2000, P=_p, seed=100 + _p), _R01)
REPROJ["P10000-N8192"] = (scene, dict(N=8192, P=10000, seed=7), _R01)
_OBS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 40)
REPROJ["obs-all-N2000"] = (scene, dict(N=2000, P=1100, obs=_OBS, seed=11, odd=0.0), _R01)
REPROJ["obs-all-N8192"] = (scene, dict(N=8192, P=1100, obs=_OBS, seed=12, odd=0.0), _R01)
_DISCS = (0, 1, 15, 16, 17, 60)
REPROJ["discs-N-lds"] = (disc_scene, dict(counts=_DISCS * 20, obs=(1, 8, 9, 17), seed=1), _R01)
REPROJ["discs-N-global"] = (disc_scene, dict(counts=_DISCS * 20, obs=(1, 8, 9, 17), seed=2, pad_to=7000), _R01)
REPROJ["discs-matched-mixed"] = (disc_scene, dict(counts=_DISCS * 20, obs=(3, 16), seed=3, matched="mixed"), _R01)
REPROJ["discs-matched-mixed-N-global"] = (disc_scene, dict(counts=_DISCS * 20, obs=(3, 16), seed=4, matched="mixed", pad_to=6400), _R01)
REPROJ["int-dup-N2000"] = (scene, dict(N=2000, P=1500, obs=(2, 9, 17, 30), integer=True, dup=40, seed=21), _R01)
REPROJ["int-dup-N8192"] = (scene, dict(N=8192, P=3000, obs=(2, 9, 17, 30), integer=True, dup=40, seed=22), _R01)
for _m in ("none", "all", "mixed"):
    for _e in ("none", "all", "mixed"):
        for _n in (2000, 8192):
            REPROJ[f"kpm-{_m}-elig-{_e}-N{_n}"] = (scene, dict(N=_n, P=2000, matched=_m, eligible=_e, seed=31 + _n), _R01)
_MD = [(r, md) for md in (0, 1, 64, 65, 128, 256) for r in (0, 1)]
REPROJ["maxdist-N2000"] = (scene, dict(N=2000, P=3000, flip=(0, 120), seed=41), _MD)
REPROJ["maxdist-N8192"] = (scene, dict(N=8192, P=3000, flip=(0, 120), seed=42), _MD)
REPROJ["geom-640x480"] = (scene, dict(N=1500, P=2000, W=640, H=480, K=(500.0, 530.0, 300.5, 260.25), behind=0.2,
                                      outside=True, seed=51), _R01)
REPROJ["geom-3840x2160"] = (scene, dict(N=8192, P=6000, W=3840, H=2160, K=(2900.0, 2950.0, 2000.0, 1000.0), behind=0.2,
                                        outside=True, seed=52), _R01)
REPROJ["geom-edges"] = (edge_scene, dict(), [(0, 64), (1, 64), (0, 3)])


def reproj_case(name, kdtree_build):
    builder, kw, runs = REPROJ[name]
    frame, mp = builder(kdtree_build=kdtree_build, **kw)
    return frame, mp, runs
