"""Host model of the reference's map (Map / MapPoint / Frame::map_matches, reference src/Map.cpp:44-124) and of the
problems the library builds from it: plain Python / numpy, test infrastructure only — the product package never imports
it.

The model keeps both directions of the graph, as the reference does:

  per point      position (f32), alive flag, observations [(key frame, keypoint)] in insertion order
                 (MapPoint::add_observation; the library keeps insertion order where the reference's unordered_map has
                 none).  A removed slot keeps its last position (rs_map_get_positions documents this) and is never reused.
  per key frame  pose [16] f32, keypoints, descriptors, keypoint -> point table (Frame::map_matches, -1 = unmatched).

Every edit returns the C-ABI calls that drive the same edit on an rs_map ("The resident map"), so a test
replays exactly what the model did:

  ("add_point", xyz) ("remove_point", p) ("add_observation", p, kf, kp) ("remove_observation", p, kf)
  ("set_position", p, xyz) ("set_keyframe_pose", kf, pose) ("add_keyframe", kf)

The flatteners build what the library must solve: the matching arrays of the flat path (rs_reproj_match), the list-ordered
view of match_for_fuse, the local-BA window walked frame-side as src/Optimization.cpp:287-315 walks it (and point-side, as
a second formulation), and the observation CSR of the loop-closure point transform (src/Optimization.cpp:512-536).
"""
import numpy as np


def centre_f32(T):
    """Frame::camera_center in f32 with the library's operation order: (-R0i*t0 + -R1i*t1) + -R2i*t2"""
    T = np.asarray(T, np.float32).reshape(16)
    return np.array([(-T[i] * T[3] + -T[4 + i] * T[7]) + -T[8 + i] * T[11] for i in range(3)], np.float32)


class MapModel:
    def __init__(self):
        self.pos, self.alive, self.obs = [], [], []
        self.kf_pose, self.kf_kp, self.kf_desc, self.kp_point = [], [], [], []

    # ------------------------------------------------------------------------------------------ queries
    def n_slots(self):
        return len(self.alive)

    def n_kf(self):
        return len(self.kf_pose)

    def observer_kp(self, p, kf):
        """MapPoint::observations().find(kf): the keypoint, or None"""
        for k, i in self.obs[p]:
            if k == kf:
                return i
        return None

    def alive_points(self):
        return [p for p in range(len(self.alive)) if self.alive[p]]

    def counts(self):
        return dict(slots=len(self.alive), alive=int(sum(self.alive)), observations=sum(len(o) for o in self.obs),
                    key_frames=len(self.kf_pose))

    def positions(self):
        return np.array(self.pos, np.float32).reshape(-1, 3)

    def consistent(self):
        """The two directions agree: every observation is in its key frame's table and every table entry is an
        observation of an alive point; at most one observation per (point, key frame)."""
        n_tab = 0
        for kf, tab in enumerate(self.kp_point):
            for kp in np.flatnonzero(tab >= 0):
                p = int(tab[kp])
                if not self.alive[p] or self.observer_kp(p, kf) != kp:
                    return False
                n_tab += 1
        for p, ol in enumerate(self.obs):
            if len({k for k, _ in ol}) != len(ol) or (ol and not self.alive[p]):
                return False
            if any(self.kp_point[k][i] != p for k, i in ol):
                return False
        return n_tab == sum(len(o) for o in self.obs)

    # ------------------------------------------------------------------------------------------ edits
    def add_keyframe(self, keypoints, descriptors, pose):
        """Mapper::insert: a key frame with its own keypoints / descriptors and an empty match table"""
        kp = np.asarray(keypoints, np.float32).reshape(-1, 2)
        self.kf_kp.append(kp)
        self.kf_desc.append(np.asarray(descriptors, np.uint8).reshape(-1, 32))
        self.kf_pose.append(np.asarray(pose, np.float32).reshape(16).copy())
        self.kp_point.append(np.full(len(kp), -1, np.int64))
        kf = len(self.kf_pose) - 1
        return kf, [("add_keyframe", kf)]

    def add_point(self, xyz):
        """Map::add_point: a new slot at the end (slots are never reused: ascending slot = map order)"""
        self.pos.append(np.asarray(xyz, np.float32).reshape(3).copy())
        self.alive.append(1)
        self.obs.append([])
        return len(self.alive) - 1, [("add_point", self.pos[-1].copy())]

    def create_point(self, xyz, observations):
        """Map::create_point (:21-61): add the point, then associate it with each (key frame, keypoint) in turn"""
        p, calls = self.add_point(xyz)
        for kf, kp in observations:
            calls += self.associate(kf, p, kp)
        return p, calls

    def _remove_map_match(self, kf, p):
        """Frame::remove_map_match (reference src/Frame.cpp:104-116): every table entry equal to the point is cleared"""
        tab = self.kp_point[kf]
        tab[tab == p] = -1

    def disassociate(self, kf, p):
        """Map::disassociate (:115-124): a key frame the point is not observed by is a no-op"""
        kp = self.observer_kp(p, kf)
        if kp is None:
            return [("remove_observation", p, kf)]
        self._remove_map_match(kf, p)
        self.obs[p] = [o for o in self.obs[p] if o[0] != kf]
        return [("remove_observation", p, kf)]

    def associate(self, kf, p, kp):
        """Map::associate (:95-113)"""
        tab = self.kp_point[kf]
        call = [("add_observation", p, kf, kp)]
        if tab[kp] == p and self.observer_kp(p, kf) is not None:          # :97-100 the same pair again
            return call
        if tab[kp] >= 0 and tab[kp] != p:                                  # :101-106 the keypoint is taken from its point
            self.disassociate(kf, int(tab[kp]))
        if self.observer_kp(p, kf) is not None:                            # :107-109 the point leaves its old keypoint
            self.disassociate(kf, p)
        self.obs[p].append((kf, kp))                                       # :110-111
        tab[kp] = p
        return call

    def remove_point(self, p):
        """Map::remove_point (:63-76): the observers' tables forget the point; the slot keeps its position"""
        for kf, _ in self.obs[p]:
            self._remove_map_match(kf, p)
        self.obs[p] = []
        self.alive[p] = 0
        return [("remove_point", p)]

    def fuse(self, kept, discarded):
        """Map::fuse (:78-93), built from the other edits.  Returns (outcomes, calls): one outcome per observation of
        `discarded` — 'moved', or the first skip condition that held: 'kept_observed' (kept.is_observed_by(frame)),
        'kp_matched' (frame->is_matched(index)), 'kept_matched' (frame->is_matched(kept)) — or ['same'] for kept ==
        discarded."""
        if kept == discarded:                                              # :80-82
            return ["same"], []
        calls, outcomes = [], []
        for kf, kp in list(self.obs[discarded]):                           # a copy: the loop edits the point (:83)
            calls += self.disassociate(kf, discarded)                      # :85
            if self.observer_kp(kept, kf) is not None:                     # :86
                outcomes.append("kept_observed")
            elif self.kp_point[kf][kp] >= 0:
                outcomes.append("kp_matched")
            elif np.any(self.kp_point[kf] == kept):
                outcomes.append("kept_matched")
            else:
                calls += self.associate(kf, kept, kp)                      # :89
                outcomes.append("moved")
        calls += self.remove_point(discarded)                              # :92
        return outcomes, calls

    def set_position(self, p, xyz):
        """MapPoint::set_position"""
        self.pos[p] = np.asarray(xyz, np.float32).reshape(3).copy()
        return [("set_position", p, self.pos[p].copy())]

    def set_pose(self, kf, pose):
        """Frame::set_pose on a key frame"""
        self.kf_pose[kf] = np.asarray(pose, np.float32).reshape(16).copy()
        return [("set_keyframe_pose", kf, self.kf_pose[kf].copy())]

    # ------------------------------------------------------------------------------------------ flatteners
    def match_arrays(self, matched_points=(), required=-1):
        """The flat map of rs_reproj_match: every slot in map order, eligible = alive, not already matched by the frame
        (src/MapMatcher.cpp:53) and, for match_key_frame, observed by `required` (:169); observation CSR by point with
        descriptor rows of the key frames' concatenated descriptor matrices."""
        P = len(self.alive)
        rows = np.cumsum([0] + [len(d) for d in self.kf_desc])
        elig = np.array(self.alive, np.uint8).reshape(P)
        elig[np.asarray(list(matched_points), np.int64)] = 0
        optr, okf, odesc = [0], [], []
        for p in range(P):
            if required >= 0 and self.observer_kp(p, required) is None:
                elig[p] = 0
            for kf, kp in self.obs[p]:
                okf.append(kf)
                odesc.append(rows[kf] + kp)
            optr.append(len(okf))
        return dict(positions=self.positions(), eligible=elig, obs_ptr=np.array(optr, np.int32),
                    obs_kf=np.array(okf, np.int32), obs_desc=np.array(odesc, np.int32),
                    kf_centers=np.stack([centre_f32(T) for T in self.kf_pose]),
                    desc_pool=np.concatenate(self.kf_desc + [np.zeros((1, 32), np.uint8)]))

    def fuse_view(self, only, matched_points=(), required=-1):
        """match_for_fuse (src/MapMatcher.cpp:117-127): the listed slots as arrays of their own IN LIST ORDER (what the
        shim builds from the caller's vector); point i of the view is only[i].  Dead slots are never eligible."""
        full = self.match_arrays(matched_points, required)
        optr, okf, odesc = [0], [], []
        for p in only:
            a, b = full["obs_ptr"][p], full["obs_ptr"][p + 1]
            okf += list(full["obs_kf"][a:b])
            odesc += list(full["obs_desc"][a:b])
            optr.append(len(okf))
        idx = np.asarray(only, np.int64)
        return dict(full, positions=full["positions"][idx], eligible=full["eligible"][idx], obs_ptr=np.array(optr, np.int32),
                    obs_kf=np.array(okf, np.int32), obs_desc=np.array(odesc, np.int32))

    def _window(self, kfs, free, per_point):
        """Convert {point: [(list index, keypoint uv)]} to the order map.hip documents: free points in ascending slot
        order, CSR by point, frames in list order within a point."""
        order = sorted(per_point)
        per = [sorted(per_point[p], key=lambda x: x[0]) for p in order]
        return dict(points=np.array(order, np.int32), obs_ptr=np.cumsum([0] + [len(x) for x in per]).astype(np.int32),
                    obs_cam=np.array([c for x in per for c, _ in x], np.int32),
                    obs_uv=np.array([uv for x in per for _, uv in x], np.float32).reshape(-1, 2),
                    positions=np.array([self.pos[p] for p in order], np.float64).reshape(-1, 3),
                    kfs=np.asarray(kfs, np.int32), cam_free=np.asarray(free, np.uint8))

    def ba_window(self, kfs, free):
        """optimization::bundle_adjust's problem, walked frame-side (src/Optimization.cpp:287-315).  Free points: matched
        by a free listed frame (Frame::map_matches, ascending keypoint) and observed >= 2 times in the whole map
        (MIN_OBSERVATIONS_TO_OPTIMIZE, :296).  Residuals: every listed frame, in list order, x each free point it
        matches (:304-315) — fixed frames included."""
        free_set = set()
        for c, kf in enumerate(kfs):
            if not free[c]:
                continue
            for kp in np.flatnonzero(self.kp_point[kf] >= 0):
                p = int(self.kp_point[kf][kp])
                if len(self.obs[p]) >= 2:
                    free_set.add(p)
        per_point = {p: [] for p in free_set}
        for c, kf in enumerate(kfs):
            for kp in np.flatnonzero(self.kp_point[kf] >= 0):
                p = int(self.kp_point[kf][kp])
                if p in per_point:
                    per_point[p].append((c, self.kf_kp[kf][kp]))
        return self._window(kfs, free, per_point)

    def ba_window_pointside(self, kfs, free):
        """The same window walked point-side, like the library's device build: a slot is free when it is alive, has >= 2
        observations and one of them is by a free listed frame; its residuals are its observations by listed frames."""
        where = {int(kf): c for c, kf in enumerate(kfs)}
        per_point = {}
        for p in range(len(self.alive)):
            listed = [(where[kf], kp) for kf, kp in self.obs[p] if kf in where]
            if self.alive[p] and len(self.obs[p]) >= 2 and any(free[c] for c, _ in listed):
                per_point[p] = [(c, self.kf_kp[kfs[c]][kp]) for c, kp in listed]
        return self._window(kfs, free, per_point)

    def transform_csr(self):
        """The observation CSR (key frames only) that the loop-closure point transform reads: every slot in map order,
        observations in insertion order (the owner is the lowest-index observer, src/Optimization.cpp:512-536)."""
        optr, okf = [0], []
        for ol in self.obs:
            okf += [kf for kf, _ in ol]
            optr.append(len(okf))
        return np.array(optr, np.int32), np.array(okf, np.int32)


# ---------------------------------------------------------------------------------------------- random edits
EDIT_WEIGHTS = dict(associate=6, disassociate=3, create_point=2, remove_point=1, fuse=1, set_position=2, set_pose=1)


def random_edit(model, rng, weights=EDIT_WEIGHTS, kinds=None):
    """Draw one edit of the kinds in `weights`, apply it to the model and return (kind, calls).  Targets are biased
    towards the interesting branches: occupied keypoints, keypoints of a key frame the point is already observed by,
    and points that share observers."""
    names = sorted(weights) if kinds is None else kinds
    w = np.array([weights[k] for k in names], np.float64)
    kind = names[int(rng.choice(len(names), p=w / w.sum()))]
    alive = model.alive_points()
    kfs = [k for k in range(model.n_kf()) if len(model.kf_kp[k])]
    if not alive or not kfs:
        kind = "create_point"
    if kind == "create_point":
        base = model.pos[int(rng.choice(alive))] if alive else np.zeros(3, np.float32)
        xyz = base + rng.normal(0, 0.05, 3).astype(np.float32)
        obs = []
        for kf in rng.choice(kfs, min(len(kfs), int(rng.integers(0, 4))), replace=False) if kfs else []:
            obs.append((int(kf), int(rng.integers(len(model.kf_kp[kf])))))
        return kind, model.create_point(xyz, obs)[1]
    p = int(rng.choice(alive))
    if kind == "associate":
        r = rng.random()
        if r < 0.3 and model.obs[p]:                                   # same key frame: the same pair or another keypoint
            kf, kp = model.obs[p][int(rng.integers(len(model.obs[p])))]
            if rng.random() < 0.5:
                kp = int(rng.integers(len(model.kf_kp[kf])))
        else:
            kf = int(rng.choice(kfs))
            taken = np.flatnonzero(model.kp_point[kf] >= 0)
            kp = int(rng.choice(taken)) if r < 0.6 and len(taken) else int(rng.integers(len(model.kf_kp[kf])))
        return kind, model.associate(int(kf), p, int(kp))
    if kind == "disassociate":
        if model.obs[p] and rng.random() < 0.8:
            kf = model.obs[p][int(rng.integers(len(model.obs[p])))][0]
        else:
            kf = int(rng.integers(model.n_kf()))
        return kind, model.disassociate(int(kf), p)
    if kind == "remove_point":
        return kind, model.remove_point(p)
    if kind == "fuse":
        q = p
        for kf, kp in model.obs[p]:                                    # prefer a point sharing an observer
            near = [int(x) for x in model.kp_point[kf] if x >= 0 and x != p]
            if near:
                q = near[int(rng.integers(len(near)))]
                break
        if q == p and len(alive) > 1:
            q = int(rng.choice(alive))
        return kind, model.fuse(q, p)[1]
    if kind == "set_position":
        return kind, model.set_position(p, model.pos[p] + rng.normal(0, 0.01, 3).astype(np.float32))
    kf = int(rng.integers(model.n_kf()))                               # set_pose: a small move of a key frame
    T = model.kf_pose[kf].reshape(4, 4).copy()
    T[:3, 3] += rng.normal(0, 0.005, 3).astype(np.float32)
    return "set_pose", model.set_pose(kf, T)
