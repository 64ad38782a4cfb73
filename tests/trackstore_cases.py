"""Cases of rs_track_store (racing-slam_amd/csrc/track_store.hip), shared by tests/test_trackstore_cases_cpu.py (the
specification tests/trackstore_ref.py against the object model and the oracle, and the condition each case exists for) and
tests/test_gpu_trackstore_envelope.py (the device against the specification and the oracle).  No GPU import.

A case is a dict:
  cap, max_sightings   the store
  steps                the calls in order: ("carry", prev, inlier, count, max_n) and ("extend", pixels, frame_index, key_frame),
                       every list as the arrays the call gets; replay() applies them to anything with those two methods
  tri                  the key frame that follows (None where the case has none): table, pixels, poses, pose_base, kf_pose, K,
                       min_new_points
Every kernel of the store is one 1024-thread workgroup in which thread t owns ceil(cap / 1024) rows or ceil(T / 1024)
tracks; the sizes below sit where that chunking, the sort width n2, the copy's 64-lane trip count or the read-back's split
changes."""
import functools

import numpy as np

import trackstore_ref as R

THREADS = 1024                          # TS_THREADS
RAGGED_CAPS = (1, 63, 1025, 4097, 8191)
PACK_SHAPES = ((1, 1, 0.0), (2, 2, 0.0), (3, 3, 0.0), (1023, 1023, 0.1), (1024, 1024, 0.1), (1025, 1025, 0.1), (2049, 2049, 0.06),
               (2049, 2500, 0.7))       # T, cap, share of tracks given a bad sighting


def scene(rng, n, frames):
    """static points in front of a camera moving along x: pixels per frame, poses, intrinsics"""
    K = (500.0, 500.0, 320.0, 240.0)
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 9, n)], axis=1)
    poses = np.tile(np.eye(4, dtype=np.float32), (frames, 1, 1))
    pix = np.zeros((frames, n, 2), np.float32)
    for f in range(frames):
        poses[f, 0, 3] = -0.15 * f
        pix[f, :, 0] = K[0] * (X[:, 0] - 0.15 * f) / X[:, 2] + K[2]
        pix[f, :, 1] = K[1] * X[:, 1] / X[:, 2] + K[3]
    return pix, poses.reshape(frames, 16), K


def monotone_lists(rng, n_prev, n_next, keep=0.8, inliers=0.7):
    """rs_track_features' kept-index list (ascending previous keypoints) and an ascending inlier list into it"""
    m = min(n_next, int(rng.binomial(n_prev, keep)))
    prev = np.sort(rng.choice(n_prev, m, replace=False)).astype(np.int32)
    return prev, np.flatnonzero(rng.random(m) < inliers).astype(np.int32)


def replay(case, store, after=None):
    for step in case["steps"]:
        getattr(store, step[0])(*step[1:])
        if after is not None:
            after(step)
    return store


class Script:
    """records the calls of a sequence while the specification runs along, so that a frame's pixels can follow its tracks:
    the track with id i watches scene point i % pool"""

    def __init__(self, cap, max_sightings, seed, pool=0, frames=0):
        self.cap, self.max_sightings, self.rng = cap, max_sightings, np.random.default_rng(seed)
        self.ref, self.steps, self.tri, self.pool = R.Store(cap, max_sightings), [], None, pool
        if pool:
            self.pix, self.poses, self.K = scene(self.rng, pool, frames)

    def carry(self, prev, inlier=None, count=None, max_n=None):
        prev = np.asarray(prev, np.int32)
        inlier = None if inlier is None else np.asarray(inlier, np.int32)
        max_n = len(prev) if max_n is None else int(max_n)
        self.steps.append(("carry", prev, inlier, count, max_n))
        self.ref.carry(prev, inlier, count, max_n)

    def extend(self, pixels, frame_index, key_frame=-1):
        pixels = np.ascontiguousarray(pixels, np.float32).reshape(-1, 2)
        self.steps.append(("extend", pixels, int(frame_index), int(key_frame)))
        self.ref.extend(pixels, frame_index, key_frame)

    def ids(self, n):
        """per keypoint of the next frame of n keypoints: the id its track has or will be given"""
        ids = np.full(n, -1, np.int64)
        has = self.ref.keypoint < n
        ids[self.ref.keypoint[has]] = self.ref.id[has].astype(np.int64)
        new = np.flatnonzero(ids < 0)
        ids[new] = self.ref.next_id + np.arange(len(new))
        return ids

    def pixels(self, scene_frame, n):
        return self.pix[scene_frame, self.ids(n) % self.pool].copy()

    def key_frame(self, table, pixels, pose_base, n_poses, kf_pose, min_new_points=100):
        self.tri = dict(table=np.asarray(table, np.int32), pixels=np.ascontiguousarray(pixels, np.float32), pose_base=int(pose_base),
                        poses=np.ascontiguousarray(self.poses[pose_base:pose_base + n_poses]), kf_pose=int(kf_pose), K=self.K,
                        min_new_points=int(min_new_points))

    def case(self, **more):
        return dict(cap=self.cap, max_sightings=self.max_sightings, steps=self.steps, tri=self.tri, **more)


def expected(ref, tri, oracle):
    """what a triangulate call on the specification's store must give: ref.pack's arrays, and the oracle's selection on
    them with the accepted tracks' keypoints, counts, positions and key-frame pairs"""
    pack = ref.pack(tri["table"], tri["pixels"], tri["pose_base"], len(tri["poses"]))
    o = oracle.triangulate_tracks(pack["track_uv"], pack["sight_ptr"], pack["sight_pose"], pack["sight_uv"], tri["poses"], tri["kf_pose"],
                                  tri["K"], skip=pack["skip"], min_new_points=tri["min_new_points"])
    acc, inc = o["accepted"], o["inconsistent"]
    pairs = [ref.key_frame_pairs(t) for t in acc]
    kf_ptr = np.concatenate([[0], np.cumsum([len(x) for x in pairs])]).astype(np.int32)
    return dict(pack=pack, status=o["status"], counts=np.array([len(acc), o["n_topped_up"], len(inc)], np.int32), track=acc.astype(np.int32),
                inconsistent=inc.astype(np.int32), keypoint=ref.keypoint[acc], sightings=ref.count[acc], xyz=o["xyz"][acc],
                parallax_cos=o["parallax_cos"][acc], required_cos=o["required_cos"][acc], kf_ptr=kf_ptr,
                kf_pairs=np.concatenate(pairs + [np.zeros((0, 2), np.int32)]).astype(np.int32), n_pairs=int(kf_ptr[-1]))


# ------------------------------------------------------------------------------------------------ 1: ragged ownership
@functools.lru_cache(maxsize=None)
def ragged(cap, repeats=False):
    """max_sightings 2, six frames hugging cap; the carries before frames 1 .. 5 take the forms of
    test_gpu_trackstore.py's sequence test: a list and its count, a count above max_n over junk entries, both null, a
    negative count, a zero count"""
    s = Script(cap, 2, [1, cap, int(repeats)])
    rng, forms = s.rng, (None, 1, 3, 2, 4, 5)
    n_prev = 0
    for frame, n in enumerate([cap, cap - 1, cap, (cap + 1) // 2, 1, cap]):
        if frame:
            prev, inl = monotone_lists(rng, n_prev, n)
            m = len(prev)
            if repeats:                                    # repeated previous keypoints and repeated current keypoints
                prev = rng.integers(0, max(1, n_prev // 2), m).astype(np.int32)
                inl = rng.integers(0, max(1, m), m + 7).astype(np.int32)
            form = forms[frame]
            if form == 1:
                s.carry(prev, inl, len(inl), m)
            elif form == 2:
                s.carry(prev, None, None, m)
            elif form == 3:
                prev[rng.random(m) < 0.1] = rng.choice([-1, n_prev, 8192, 2 ** 30, -2 ** 31])
                full = np.concatenate([inl, rng.choice([-1, m, m + 3, 8192, 2 ** 30], max(m - len(inl), 0) + 1)])[:max(m, 1)].astype(np.int32)
                rng.shuffle(full)
                s.carry(prev, full if m else None, m + 50, m)
            elif form == 4:
                s.carry(prev, inl, -7, m)
            else:
                s.carry(prev, inl[:0] if m == 0 else inl, 0, m)
        s.extend(rng.uniform(0, 700, (n, 2)).astype(np.float32), 10 + frame, frame // 3 if frame % 3 == 0 else -1)
        n_prev = n
    return s.case()


# ------------------------------------------------------------------------------------------------ 2, 3: the pack's chunks
@functools.lru_cache(maxsize=None)
def pack_case(T, cap, bad, frames=5, max_sightings=6):
    """T live tracks by a static-scene sequence of `frames` frames of T keypoints; every carry but the last drops some
    tracks, so rows are reused and id order leaves keypoint and row order; a share `bad` of the tracks gets one sighting
    25 px off (inconsistent), a tenth of the key frame's keypoints is matched in the table (skipped)"""
    s = Script(cap, max_sightings, [2, T, cap], pool=2 * T + 64, frames=frames + 1)
    rng, ident = s.rng, np.arange(T, dtype=np.int32)
    for f in range(frames):
        if f:
            inl = np.flatnonzero(rng.random(T) < 0.93).astype(np.int32)
            s.carry(ident, inl, len(inl), T)
        pix = s.pixels(f, T)
        if f == frames - 2:
            pix[rng.random(T) < bad] += np.float32(25.0)
        s.extend(pix, f, {0: 0, 2: 1}.get(f, -1))
    s.carry(ident)                                         # the frame in between: every track is found again
    table = np.full(T, -1, np.int32)
    hit = np.flatnonzero(rng.random(T) < 0.1)
    table[hit] = np.arange(len(hit))
    s.key_frame(table, s.pixels(frames, T), 0, frames + 1, frames)
    assert len(s.ref.id) == T
    return s.case()


@functools.lru_cache(maxsize=None)
def full_size():
    """T = cap = 8192, max_sightings 2: n2 = 8192 (a 64 KB sort), 8 rows and 8 tracks per thread.  Frame 1 is reached
    through a shuffled kept-index list that loses a quarter of the tracks, so the sort's input is far from sorted"""
    n = 8192
    s = Script(n, 2, [3], pool=2 * n, frames=3)
    rng = s.rng
    s.extend(s.pixels(0, n), 0, 0)
    inl = np.flatnonzero(rng.random(n) < 0.75).astype(np.int32)
    s.carry(rng.permutation(n).astype(np.int32), inl, len(inl), n)
    pix = s.pixels(1, n)
    pix[rng.random(n) < 0.05] += np.float32(25.0)
    s.extend(pix, 1, -1)
    s.carry(np.arange(n, dtype=np.int32))
    table = np.full(n, -1, np.int32)
    hit = np.flatnonzero(rng.random(n) < 0.1)
    table[hit] = np.arange(len(hit))
    s.key_frame(table, s.pixels(2, n), 0, 3, 2)
    assert len(s.ref.id) == n
    return s.case()


# ------------------------------------------------------------------------------------------------ 4: sighting counts
LONG_BIRTHS = {1: 1, 2: 2, 4: 2, 5: 64, 6: 65, 7: 66, 8: 128, 10: 100, 11: 120}      # keypoint -> the frame its last track is born in
LONG_ROLES = dict(first=0, kept=1, late=2, ends=3)       # keypoints: out of range at index 0; 128 sightings in range and the
#                                                          key-frame sighting of frame 129 dropped; at index 127 only; at both ends


@functools.lru_cache(maxsize=None)
def long_tracks():
    """cap 96, max_sightings 128, frames 0 .. 129 of 12 keypoints (frame 129: 4), poses for frames 1 .. 128.
    A track born in frame b and seen up to frame 128 holds 129 - b sightings: 1, 63, 64, 65 and 127 are there, the
    tracks of frames 0 and 1 hit 128 and lose what follows.  Keypoint 3's track hides at keypoint 40 during frames 60
    and 61, so it holds frame 0 at index 0 and frame 129 at index 127: out of range at both ends, counted once.
    Every tenth frame is a key frame, and so is frame 129, whose sighting the track of keypoint 1 has no room for"""
    n, F = 12, 130
    s = Script(96, 128, [4], pool=64, frames=F)
    ident = np.arange(n, dtype=np.int32)
    for f in range(F):
        if f in (60, 61):                                  # a list of 41 entries for a frame of 12 keypoints
            prev = np.full(41, -1, np.int32)
            prev[:n] = ident
            prev[3], prev[40] = (-1, 3) if f == 60 else (3, 40)
            s.carry(prev)
        elif f == 62:
            prev = ident.copy()
            prev[3] = 40
            s.carry(prev)
        elif f:
            inl = np.array([j for j in range(n) if LONG_BIRTHS.get(j) != f], np.int32)
            s.carry(ident, inl, len(inl), n)
        m = 4 if f == F - 1 else n
        s.extend(s.pixels(f, m), f, 13 if f == F - 1 else (f // 10 if f % 10 == 0 else -1))
    s.carry(ident)
    table = np.full(n, -1, np.int32)
    table[10] = 7
    s.key_frame(table, s.pixels(128, n), 1, 128, 127, min_new_points=3)
    return s.case()


# ------------------------------------------------------------------------------------------------ 5: more than 2 T pairs
@functools.lru_cache(maxsize=None)
def many_pairs():
    """50 keypoints, cap 64, max_sightings 6: frames 0 .. 5 are key frames 0 .. 5, frames 6 .. 8 are none.  A track of
    frame 0 holds six key-frame sightings and nothing else; the 15 tracks born in frame 6 hold none"""
    n = 50
    s = Script(64, 6, [5], pool=256, frames=10)
    rng, ident = s.rng, np.arange(n, dtype=np.int32)
    for f in range(9):
        if f:
            keep = rng.random(n) < 0.95
            if f == 6:
                keep[30:45] = False
            inl = np.flatnonzero(keep).astype(np.int32)
            s.carry(ident, inl, len(inl), n)
        s.extend(s.pixels(f, n), f, f if f < 6 else -1)
    s.carry(ident)
    s.key_frame(np.full(n, -1, np.int32), s.pixels(9, n), 0, 10, 9, min_new_points=45)
    return s.case()


# ------------------------------------------------------------------------------------------------ 6: ids beyond 2^19
ID_FRAMES = 66


@functools.lru_cache(maxsize=None)
def id_spread():
    """cap 8192, max_sightings 2, 66 frames of 8192 keypoints.  Two tracks of frame 0 live on through two-entry inlier
    lists — id 0 in row 0, which ends at keypoint 8000, and id 8191 in row 8191, which ends at keypoint 5 — and every
    other keypoint is new in every frame: 8192 + 65 * 8190 = 540 542 ids >= 2^19, where (id - min id) << 13 | row
    leaves 32 bits."""
    n = 8192
    s = Script(n, 2, [6], pool=2 * n, frames=ID_FRAMES + 1)
    rng = s.rng
    a, b = 0, n - 1
    s.extend(s.pixels(0, n), 0, 0)
    for f in range(1, ID_FRAMES):
        a2, b2 = (8000, 5) if f == ID_FRAMES - 1 else (int(x) for x in rng.choice(n, 2, replace=False))
        prev = np.arange(n, dtype=np.int32)
        prev[a2], prev[b2] = a, b
        s.carry(prev, np.array([a2, b2], np.int32), 2, n)
        s.extend(s.pixels(f, n), f, f // 10 if f % 10 == 0 else -1)
        a, b = a2, b2
    s.key_frame(np.full(n, -1, np.int32), s.pixels(ID_FRAMES, n), 0, ID_FRAMES + 1, ID_FRAMES)
    return s.case()


# ------------------------------------------------------------------------------------------------ 8: the query at size
@functools.lru_cache(maxsize=None)
def query_at_size():
    """8192 keypoints against a map of 2000 slots with 0 .. 6 observations (key frames 0 .. n_obs - 1, in order) and 60 dead
    slots; `single` is a max_sightings 1 store (travel 0), `moving` a max_sightings 3 store whose tracks travel 0 .. 40 px,
    one of them to a NaN pixel and one to an infinite pixel"""
    n, P = 8192, 2000
    rng = np.random.default_rng(8)
    n_obs = rng.integers(0, 7, P)
    dead = np.sort(rng.choice(P, 60, replace=False))
    table = np.full(n, -1, np.int32)
    hit = rng.choice(n, 2010, replace=False)
    table[hit] = rng.choice(P + 20, 2010, replace=False)                 # some beyond the map: matches, never covisible
    single = Script(n, 1, [8, 1])
    single.extend(rng.uniform(0, 700, (n, 2)), 4)
    moving = Script(n, 3, [8, 3])
    ident = np.arange(n, dtype=np.int32)
    pix = rng.uniform(0, 700, (n, 2)).astype(np.float32)
    moving.extend(pix, 0)
    for f in (1, 2):
        inl = np.flatnonzero(rng.random(n) < 0.9).astype(np.int32)
        moving.carry(ident, inl, len(inl), n)
        ang = rng.uniform(0, 6.28, n)
        pix = (pix + rng.uniform(0, 20, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)).astype(np.float32)
        if f == 2:
            whole = np.flatnonzero((moving.ref.count == 2) & (table[moving.ref.keypoint] < 0))      # unmatched tracks that will hold 3 sightings
            pix[moving.ref.keypoint[whole[0]], 0] = np.nan
            pix[moving.ref.keypoint[whole[1]]] = np.inf
        moving.extend(pix, f)
    return dict(n=n, P=P, n_obs=n_obs, dead=dead, table=table, single=single.case(pixels=single.steps[-1][1]),
                moving=moving.case(pixels=pix))


def covisible(n_obs, dead, last_kf):
    """SimpleMap's point p is observed by key frames 0 .. n_obs[p] - 1 unless it is dead"""
    cov = np.asarray(n_obs) > last_kf if last_kf >= 0 else np.zeros(len(n_obs), bool)
    cov[np.asarray(dead, np.int64)] = False
    return cov
