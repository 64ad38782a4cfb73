"""Loop-fusion scenes for tests/test_fuse_cpu.py and tests/test_gpu_fuse.py: plain numpy, test infrastructure only.

Geometry as racing-slam_amd/synth.py builds it (pinhole camera, world -> camera poses, 640 x 480): all key frames look
along +z at one cloud of points 5 .. 7 units away from centres a few tenths apart — a closed loop, where old and new key
frames see the same place.  Old points are observed by the old key frames.  The "new" copy D of an old point P sits a
few hundredths away (a pixel or two of reprojection), is observed by new key frames only, and its observations carry P's
base descriptor with a few bits flipped, well within 64 bits of P's own observations; descriptors of different points
are random, ~128 bits apart.

A case is dict(name, model, query, candidate, inliers, window, camera, options) and, per case, `expect`: the branches the
case is there for, which tests/test_fuse_cpu.py asserts on the restatement alone.
"""
import numpy as np

from map_model import MapModel

K = (400.0, 400.0, 320.0, 240.0)
CAMERA = dict(K=K, width=640, height=480)


def flip(desc, n, rng, taken=None):
    """desc with n bits flipped, none of them in `taken` (a set that receives the flipped bits)"""
    out = np.array(desc, np.uint8).copy()
    free = [b for b in range(256) if taken is None or b not in taken]
    for b in rng.choice(free, n, replace=False):
        out[b // 8] ^= np.uint8(1 << (b % 8))
        if taken is not None:
            taken.add(int(b))
    return out


class Builder:
    def __init__(self, seed, n_kf, spread=0.3):
        self.rng = np.random.default_rng(seed)
        self.centres = np.concatenate([self.rng.uniform(-spread, spread, (n_kf, 2)), np.zeros((n_kf, 1))], 1).astype(np.float32)
        self.kp = [[] for _ in range(n_kf)]
        self.desc = [[] for _ in range(n_kf)]
        self.points = []                      # (xyz, [(kf, kp)])
        self.base = []

    def pose(self, kf):
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = -self.centres[kf]
        return T.reshape(16)

    def project(self, kf, xyz):
        x = np.asarray(xyz, np.float64) - self.centres[kf].astype(np.float64)
        return np.array([K[0] * x[0] / x[2] + K[2], K[1] * x[1] / x[2] + K[3]])

    def new_xyz(self):
        return np.array([self.rng.uniform(-2, 2), self.rng.uniform(-1.5, 1.5), self.rng.uniform(5, 7)], np.float32)

    def new_base(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def add_kp(self, kf, uv, desc):
        self.kp[kf].append(np.asarray(uv, np.float32))
        self.desc[kf].append(np.asarray(desc, np.uint8))
        return len(self.kp[kf]) - 1

    def seen_kp(self, kf, xyz, base, flips=6, noise=0.3, desc=None):
        uv = self.project(kf, xyz) + self.rng.uniform(-noise, noise, 2)
        return self.add_kp(kf, uv, flip(base, flips, self.rng) if desc is None else desc)

    def add_point(self, xyz, base, observers, flips=6, noise=0.3):
        """a point observed by `observers` in that order, each at a new keypoint; returns the slot"""
        obs = [(kf, self.seen_kp(kf, xyz, base, flips, noise)) for kf in observers]
        self.points.append((np.asarray(xyz, np.float32), obs))
        self.base.append(np.asarray(base, np.uint8))
        return len(self.points) - 1

    def observe(self, p, kf, kp=None, flips=6):
        """one more observation of point p, by kf (at a new keypoint unless one is given)"""
        if kp is None:
            kp = self.seen_kp(kf, self.points[p][0], self.base[p], flips)
        self.points[p][1].append((kf, kp))
        return kp

    def pad(self, kf, n):
        """random unmatched keypoints with random descriptors until the key frame has n"""
        while len(self.kp[kf]) < n:
            self.add_kp(kf, [self.rng.uniform(5, 635), self.rng.uniform(5, 475)], self.new_base())

    def model(self):
        m = MapModel()
        for kf in range(len(self.kp)):
            m.add_keyframe(np.array(self.kp[kf], np.float32).reshape(-1, 2), np.array(self.desc[kf], np.uint8).reshape(-1, 32), self.pose(kf))
        for xyz, obs in self.points:
            m.create_point(xyz, obs)
        return m


def case(name, b, query, candidate, inliers, window, expect=(), **options):
    return dict(name=name, model=b.model(), query=query, candidate=candidate, inliers=list(inliers), window=list(window),
                camera=CAMERA, options=dict(dict(max_distance=64, min_shared=15, max_covisible=20), **options), expect=set(expect))


def loop_scene(seed, n_old_kf=5, n_new_kf=5, n_old=120, dup_frac=0.25, n_kp=128, pairs=4, free_frac=0.15, p_cand=1.0, p_old=0.6,
               inlier_frac=0.5, n_new_only=0, both_frac=0.3):
    """The general scene.  Key frame 0 is the candidate, 1 .. n_old_kf-1 the other old frames, then the new frames; the query
    is the last.  Returns (builder, query, inliers, window, info)."""
    n_kf = n_old_kf + n_new_kf
    b = Builder(seed, n_kf)
    rng = b.rng
    old_kfs, new_kfs = list(range(n_old_kf)), list(range(n_old_kf, n_kf))
    query = n_kf - 1
    olds = []
    for _ in range(n_old):
        seers = [kf for kf in old_kfs if rng.random() < (p_cand if kf == 0 else p_old)]
        olds.append(b.add_point(b.new_xyz(), b.new_base(), seers or [0 if p_cand > 0 else 1]))
    # pairs for RS_FUSE_OLD: Q, a near copy of P, both old; a new frame observes Q, not P
    plain = list(olds)
    for _ in range(pairs):
        P = plain.pop(int(rng.integers(len(plain))))
        Q = b.add_point(b.points[P][0] + np.array([0.015, 0.01, 0], np.float32), flip(b.base[P], 20, rng), [0, 1])
        b.observe(Q, int(rng.choice(new_kfs)))
        olds.append(Q)
    dups, inliers = [], []
    n_dup = int(round(dup_frac * len(plain)))
    for P in [plain.pop(int(rng.integers(len(plain)))) for _ in range(n_dup)]:
        seers = [kf for kf in new_kfs if rng.random() < 0.5] or [int(rng.choice(new_kfs))]
        off = np.array([rng.uniform(0.01, 0.03), rng.uniform(0.01, 0.03), 0], np.float32)
        D = b.add_point(b.points[P][0] + off, b.base[P], seers)
        dups.append((P, D))
        others = [kf for kf in seers if kf != query]
        if others and rng.random() < both_frac:        # a new frame that sees BOTH: kept_observed inside the fuse
            b.observe(P, others[-1])
        if query in seers and b.points[P][1][0][0] == 0 and rng.random() < inlier_frac:
            inliers.append((dict(b.points[D][1])[query], P))
    for P in plain:                                    # free keypoints where an old point projects
        for kf in new_kfs:
            if rng.random() < free_frac:
                b.seen_kp(kf, b.points[P][0], b.base[P])
    for _ in range(n_new_only):                        # points of the new frames alone: they never take part
        b.add_point(b.new_xyz(), b.new_base(), [kf for kf in new_kfs if rng.random() < 0.2] or [query])
    for kf in range(n_kf):
        b.pad(kf, n_kp)
    return b, query, inliers, new_kfs, dict(olds=olds, dups=dups, old_kfs=old_kfs, new_kfs=new_kfs)


# ---------------------------------------------------------------------------------------------- named cases
def general(seed=11, **kw):
    b, query, inliers, window, info = loop_scene(seed, **kw)
    return case(f"general{seed}", b, query, 0, inliers, window, expect={"o1", "o4", "o5", "kept_observed", "blocked_by_fuse"})


def inlier_branches(seed=12):
    """every inlier outcome: out-of-range keypoint, dead point, unknown point, the same point twice (second keypoint once
    free, once holding a D), D in the old set, the keypoint already holding the point"""
    b, query, inliers, window, info = loop_scene(seed, inlier_frac=0.0)
    m_obs = {p: dict(b.points[p][1]) for p in range(len(b.points))}
    fused = {P for P, _ in info["dups"]}
    held = next(p for p in info["olds"] if p not in fused and query not in m_obs[p])
    held_kp = b.observe(held, query)                              # an old point the query observes
    in_query = [(P, D) for P, D in info["dups"] if query in m_obs[D] and query not in m_obs[P]]
    assert len(in_query) >= 4
    (P0, D0), (P1, D1), (P2, D2), (P3, D3) = in_query[:4]
    free = b.add_kp(query, [600.0, 20.0], b.new_base())
    free2 = b.add_kp(query, [610.0, 30.0], b.new_base())
    dead = b.add_point(b.new_xyz(), b.new_base(), [1])           # removed below
    inl = [(len(b.kp[query]) + 5, P0), (-1, P0),                  # 0: keypoint out of range
           (free, dead), (free, len(b.points) + 7), (free, -3),   # 0: dead / unknown point
           (m_obs[D0][query], P0),                                # 5
           (free, P0),                                            # 2: free keypoint, but the query now matches P0
           (m_obs[D1][query], P1), (m_obs[D2][query], P1),        # 5 then 5: the same point again at a keypoint holding another D
           (free2, P3),                                           # 1
           (free2, P3),                                           # 3: the keypoint already holds the point
           (held_kp, P2)]                              # 4: the keypoint's point is old
    c = case("inlier_branches", b, query, 0, inl, window, expect={"o0", "o1", "o2", "o3", "o4", "o5"})
    c["model"].remove_point(dead)
    return c


def covisibility(seed=13):
    """26 key frames qualify against a cut of 20, counts 13 .. 16 around the threshold of 15, two equal counts across the cut"""
    n_cov = 28
    b = Builder(seed, 1 + n_cov + 2)
    counts = [13, 14, 15, 16] + [40 - i for i in range(18)] + [22, 22, 22] + [17, 18, 19]      # 28 covisibles, 26 of them qualify
    # sorted descending: 40 .. 23 (18 frames), then 22 x3: the cut of 20 takes two of the three — the lower handles stay
    pts = [b.add_point(b.new_xyz(), b.new_base(), [0]) for _ in range(40)]
    for j, c in enumerate(counts):
        for p in pts[:c]:
            b.observe(p, 1 + j)
    new_kfs = [1 + n_cov, 2 + n_cov]
    for p in pts[:10]:
        b.add_point(b.points[p][0] + np.array([0.02, 0.01, 0], np.float32), b.base[p], new_kfs)
    for kf in range(len(b.kp)):
        b.pad(kf, 64)
    return case("covisibility", b, new_kfs[-1], 0, [], new_kfs, expect={"cut", "o5"}), counts


def empty_candidate(seed=14):
    """a candidate with no matches: old = [candidate], S = 0; the inliers are still applied; the window matches nothing"""
    b, query, inliers, window, info = loop_scene(seed, p_cand=0.0, pairs=0)
    free = b.add_kp(query, [600.0, 20.0], b.new_base())
    c = case("empty_candidate", b, query, 0, [(free, info["olds"][0])], window, expect={"o1", "s0"})
    assert not np.any(c["model"].kp_point[0] >= 0)
    return c


def source_count(S, seed=15):
    """exactly S sources: every old point is observed by the candidate, max_covisible = 0"""
    n_kp = max(128, S + 40)
    b, query, inliers, window, info = loop_scene(seed + S, n_old_kf=3, n_new_kf=3, n_old=S, dup_frac=0.5, n_kp=n_kp, pairs=0)
    return case(f"sources{S}", b, query, 0, inliers, window, expect={f"s{S}"}, max_covisible=0)


def dependence(seed=16):
    """the four dependences between window frames, each on a point of its own:
       a  P fused with D in frame i; frame j > i observed D too: P must be absent from j's section
       b  P's own descriptors are > 64 bits from keypoint k of frame j, D's (gained in frame i) within 64: (k, P) is matched
       c  P's row grows from 8 to 9 observations in frame i; frame j matches P at a free keypoint from the longer row
       d  D's observers partly observe P already: fewer observations are appended than D has"""
    n_old_kf = 9
    b = Builder(seed, n_old_kf + 3, spread=0.15)
    i, j, q = n_old_kf, n_old_kf + 1, n_old_kf + 2
    filler = [b.add_point(b.new_xyz(), b.new_base(), list(range(n_old_kf))) for _ in range(20)]      # makes every old frame covisible
    Pa = b.add_point(b.new_xyz(), b.new_base(), [0, 1, 2])
    Da = b.add_point(b.points[Pa][0] + np.array([0.02, 0.01, 0], np.float32), b.base[Pa], [i, j])
    Pb = b.add_point(b.new_xyz(), b.new_base(), [0, 1])
    used = set()
    mid = flip(b.base[Pb], 45, b.rng, used)                       # 45 bits from P's base
    far = flip(mid, 45, b.rng, used)                              # 45 OTHER bits: 90 from P's base, 45 from mid
    Db = len(b.points)
    kpD = b.seen_kp(i, b.points[Pb][0], b.base[Pb], desc=mid)
    b.points.append((b.points[Pb][0] + np.array([0.01, 0.01, 0], np.float32), [(i, kpD)]))
    b.base.append(mid)
    kb = b.seen_kp(j, b.points[Pb][0], b.base[Pb], desc=far)      # free keypoint of frame j
    Pc = b.add_point(b.new_xyz(), b.new_base(), list(range(8)))   # exactly 8 observations
    Dc = b.add_point(b.points[Pc][0] + np.array([0.02, 0.02, 0], np.float32), b.base[Pc], [i])
    kc = b.seen_kp(j, b.points[Pc][0], b.base[Pc])                # free keypoint of frame j
    Pd = b.add_point(b.new_xyz(), b.new_base(), [0, 2])
    Dd = b.add_point(b.points[Pd][0] + np.array([0.02, 0.01, 0], np.float32), b.base[Pd], [i, j, q])
    b.observe(Pd, j)
    b.observe(Pd, q)
    for kf in range(len(b.kp)):
        b.pad(kf, 96)
    c = case("dependence", b, q, 0, [], [i, j, q], expect={"blocked_by_fuse", "gained_descriptor", "kept_observed", "row8to9"})
    c["marks"] = dict(i=i, j=j, Pa=Pa, Da=Da, Pb=Pb, Db=Db, kb=kb, Pc=Pc, Dc=Dc, kc=kc, Pd=Pd, Dd=Dd)
    return c


def many_matches(seed=17):
    """at least 300 accepted matches in a 512-keypoint frame, outcomes 1, 4 and 5 mixed (3 cannot come from a window
    frame: a point the frame observes is not eligible)"""
    b, query, inliers, window, info = loop_scene(seed, n_old_kf=3, n_new_kf=1, n_old=440, dup_frac=0.6, n_kp=512, pairs=12, free_frac=0.45,
                                                 p_old=0.8)
    return case("many_matches", b, query, 0, [], window, expect={"o1", "o4", "o5", "m300"})


def window_sizes(seed=18, big=513):
    """key frames of 1, 2 and `big` keypoints in the window, and old frames listed in it"""
    b, query, inliers, window, info = loop_scene(seed, n_old_kf=4, n_new_kf=3, n_old=80, n_kp=100)
    n = len(b.kp)
    one, two, large = n, n + 1, n + 2
    for _ in range(3):
        b.kp.append([]); b.desc.append([])
    b.centres = np.concatenate([b.centres, b.rng.uniform(-0.3, 0.3, (3, 3)).astype(np.float32) * [1, 1, 0]]).astype(np.float32)
    olds = info["olds"]
    b.seen_kp(one, b.points[olds[0]][0], b.base[olds[0]])
    b.seen_kp(two, b.points[olds[1]][0], b.base[olds[1]])
    b.seen_kp(two, b.points[olds[2]][0], b.base[olds[2]])
    for p in olds[:40]:
        b.seen_kp(large, b.points[p][0], b.base[p])
    b.pad(large, big)
    return case(f"window{big}", b, query, 0, inliers, [1, one, window[0], two, 2, large] + window[1:], expect={"o1", "o5"})


def soak(seed):
    """a seeded random map: 30 key frames of 128 keypoints, about 600 points, 25 % duplicated"""
    b, query, inliers, window, info = loop_scene(1000 + seed, n_old_kf=12, n_new_kf=18, n_old=480, dup_frac=0.25, n_kp=128, pairs=6,
                                                 free_frac=0.03, p_cand=0.22, p_old=0.22)
    return case(f"soak{seed}", b, query, 0, inliers, window[-20:], expect=set())
