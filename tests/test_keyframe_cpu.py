"""tests/keyframe_ref.py (the specification of rs_map_insert_keyframe, rs_map_add_track_points, rs_map_reanchor and
rs_map_cull_points on tests/map_model.MapModel) against a literal walk of an object graph written the way the reference
writes Mapper::insert (src/Mapper.cpp:152-174, :310-331, :379-393, :396-431; Map::associate, src/Map.cpp:97-124): sets of
frames, per-point dicts, pointers compared by identity.  Maps are random scenes after random_edit sequences, so they hold
removed slots, points without observations and key frames outside the list.  No GPU."""
import numpy as np
import pytest

import keyframe_ref as R
from map_model import random_edit


# ------------------------------------------------------------------------------------------ the object graph
class Pt:
    def __init__(self, slot, position):
        self.slot, self.position, self.observations, self.alive, self.consistent = slot, np.array(position, np.float32), {}, True, False


class Fr:
    def __init__(self, index, pose, keypoints):
        self.index, self.pose, self.keypoints, self.matches = index, np.array(pose, np.float32), keypoints, {}      # keypoint -> Pt

    def is_matched_kp(self, kp):
        return kp in self.matches

    def is_matched_point(self, pt):
        return any(q is pt for q in self.matches.values())

    def remove_map_match(self, pt):                          # src/Frame.cpp:104-116
        for kp in [k for k, q in self.matches.items() if q is pt]:
            del self.matches[kp]


class Graph:
    def __init__(self, model):
        self.frames = [Fr(k, model.kf_pose[k], model.kf_kp[k]) for k in range(model.n_kf())]
        self.points = [Pt(p, model.pos[p]) for p in range(model.n_slots())]
        for p, pt in enumerate(self.points):
            pt.alive = bool(model.alive[p])
            for kf, kp in model.obs[p]:
                pt.observations[self.frames[kf]] = kp
                self.frames[kf].matches[kp] = pt

    def disassociate(self, frame, pt):                       # src/Map.cpp:116-124
        if frame not in pt.observations:
            return
        frame.remove_map_match(pt)
        del pt.observations[frame]

    def associate(self, frame, pt, kp):                      # src/Map.cpp:97-114
        if frame.is_matched_kp(kp) and frame.matches[kp] is pt and frame in pt.observations:
            return
        if frame.is_matched_kp(kp):
            existing = frame.matches[kp]
            if existing is not pt:
                self.disassociate(frame, existing)
        if frame in pt.observations:
            self.disassociate(frame, pt)
        pt.observations[frame] = kp
        frame.matches[kp] = pt

    def create_point(self, position, frame, kp):             # src/Map.cpp:44-61
        pt = Pt(len(self.points), position)
        self.points.append(pt)
        self.associate(frame, pt, kp)
        return pt

    def remove_point(self, pt):                              # src/Map.cpp:63-76
        for frame in list(pt.observations):
            frame.remove_map_match(pt)
        pt.observations, pt.alive = {}, False

    def same_as(self, model):
        assert len(self.points) == model.n_slots() and len(self.frames) == model.n_kf()
        for p, pt in enumerate(self.points):
            assert pt.alive == bool(model.alive[p]), p
            assert [(f.index, kp) for f, kp in pt.observations.items()] == [tuple(o) for o in model.obs[p]], p
            assert pt.position.tobytes() == np.asarray(model.pos[p], np.float32).tobytes(), p
        for k, fr in enumerate(self.frames):
            tab = np.full(len(model.kf_kp[k]), -1, np.int64)
            for kp, pt in fr.matches.items():
                tab[kp] = pt.slot
            assert np.array_equal(tab, model.kp_point[k]), k


def edited_model(seed, n_kf=5, n_kp=110, P=150, n_edits=120):
    model = R.build_model(R.random_scene(seed, n_kf, n_kp, P))
    rng = np.random.default_rng(500 + seed)
    for _ in range(n_edits):
        random_edit(model, rng)
    assert model.consistent()
    assert any(not a for a in model.alive) and any(a and not o for a, o in zip(model.alive, model.obs))
    return model, rng


SEEDS = [1, 2, 3, 4]


# ------------------------------------------------------------------------------------------ adopt
@pytest.mark.parametrize("seed", SEEDS)
def test_adopt_equals_the_loop_over_the_frames_matches(seed):
    model, rng = edited_model(seed)
    g = Graph(model)
    n_kp = 70
    kp, de = rng.uniform(0, 600, (n_kp, 2)).astype(np.float32), rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
    table = np.full(n_kp, -1, np.int64)
    dead = [p for p in range(model.n_slots()) if not model.alive[p]]
    live = model.alive_points()
    sel = rng.permutation(n_kp)[:45]
    table[sel[:35]] = rng.choice(live, 35, replace=False)
    table[sel[35:40]] = dead[:5]                                     # removed slots left in the frame's table
    table[sel[40:43]] = model.n_slots() + np.arange(3)               # slots the map never had
    table[sel[43:45]] = table[sel[0]]                                # one point named by three keypoints
    kf, _ = model.add_keyframe(kp, de, R.pose_of(model.n_kf()))
    n = R.adopt(model, kf, table)
    # the reference: a KeyFrame made from the frame; for (match : map_matches()) associate(*key_frame, point, index)
    fr = Fr(kf, model.kf_pose[kf], kp)
    g.frames.append(fr)
    made = 0
    for i in range(n_kp):
        if table[i] < 0 or table[i] >= len(g.points) or not g.points[table[i]].alive:
            continue
        g.associate(fr, g.points[table[i]], i)
        made += 1
    assert n == made == 35 + 2 and model.consistent()
    g.same_as(model)
    assert model.observer_kp(int(table[sel[0]]), kf) == int(max(sel[0], sel[43], sel[44]))     # the latest keypoint holds it


# ------------------------------------------------------------------------------------------ add_track_points
@pytest.mark.parametrize("seed", SEEDS)
def test_add_track_points_equals_the_creation_loop(seed):
    model, rng = edited_model(seed)
    kf = model.n_kf() - 1
    window = [k for k in range(model.n_kf()) if k != 1]               # key frame 1 is outside the BA window
    res = R.random_results(model, kf, rng)
    g = Graph(model)
    counted = {}
    slots, consistent = R.add_track_points(model, kf, res, window, skipped=counted)
    ba_window = {g.frames[k] for k in window}
    key_frame, made, cons = g.frames[kf], [], []
    skipped = dict(null=0, self=0, outside=0, kp=0, point=0)
    for a in range(len(res["keypoint"])):
        pt = g.create_point(res["xyz"][a], key_frame, int(res["keypoint"][a]))
        for h, kp in res["kf_pairs"][res["kf_ptr"][a]:res["kf_ptr"][a + 1]]:
            observer = g.frames[h] if h >= 0 else None
            if observer is None or observer is key_frame or observer not in ba_window:
                skipped["null" if observer is None else "self" if observer is key_frame else "outside"] += 1
                continue
            if observer.is_matched_kp(int(kp)) or observer.is_matched_point(pt):
                skipped["kp" if observer.is_matched_kp(int(kp)) else "point"] += 1
                continue
            g.associate(observer, pt, int(kp))
        if res["sightings"][a] >= 3:
            pt.consistent = True
            cons.append(pt.slot)
        made.append(pt.slot)
    assert slots == made and consistent == cons and model.consistent()
    assert min(skipped.values()) > 0, skipped                        # every skip rule was exercised
    assert counted == skipped                                        # (the restatement counts them the same way)
    g.same_as(model)
    with pytest.raises(ValueError):
        R.add_track_points(model, kf, dict(res, capacity_pairs=res["n_pairs"] - 1), window)


# ------------------------------------------------------------------------------------------ reanchor
@pytest.mark.parametrize("seed", SEEDS)
def test_reanchor_equals_the_walk_over_the_anchors(seed, oracle):
    model, rng = edited_model(seed)
    kfs = [3, 0, 4]                                                  # key frames 1 and 2 are not optimised
    before = np.stack([model.kf_pose[k] for k in kfs])
    for k in kfs:                                                    # the adjustment moved them
        T = model.kf_pose[k].reshape(4, 4).copy()
        T[:3, 3] += rng.normal(0, 0.02, 3).astype(np.float32)
        model.set_pose(k, T)
    g = Graph(model)
    pos0 = model.positions().copy()
    pts, xyz = R.reanchor(model, kfs, before, oracle)
    moved = set()
    for frame, bef in [(g.frames[k], before[c]) for c, k in enumerate(kfs)]:
        for kp, pt in frame.matches.items():
            if len(pt.observations) > 1:
                continue
            pt.position = oracle.reanchor_points(None, [0], bef[None], frame.pose[None], pt.position[None])[0]
            assert pt.slot not in moved
            moved.add(pt.slot)
    assert sorted(moved) == list(pts) and len(moved) > 3
    g.same_as(model)
    assert xyz.tobytes() == model.positions()[pts].tobytes()
    rest = np.setdiff1d(np.arange(model.n_slots()), pts)
    assert model.positions()[rest].tobytes() == pos0[rest].tobytes()
    # the untouched kinds are all present: two observers, dead, observer unlisted, no observer
    kinds = dict(two=0, dead=0, unlisted=0, none=0)
    for p in rest:
        o = model.obs[p]
        kinds["dead" if not model.alive[p] else "none" if not o else "two" if len(o) > 1 else "unlisted"] += 1
    assert min(kinds.values()) > 0, kinds


# ------------------------------------------------------------------------------------------ cull
@pytest.mark.parametrize("seed", SEEDS)
def test_cull_equals_the_walk_over_the_local_set(seed, oracle):
    model, rng = edited_model(seed)
    kfs = [2, 3, 4]
    g = Graph(model)
    poses = np.stack(model.kf_pose)
    dry = R.cull(model, kfs, R.K, oracle, apply=False)
    g.same_as(model)                                                 # apply = False changes nothing
    local = set()
    for k in kfs:
        for kp, pt in g.frames[k].matches.items():
            local.add(pt)
    to_remove = []
    for pt in local:
        obs = list(pt.observations.items())
        r = oracle.point_errors(pt.position[None], [0, len(obs)], [f.index for f, _ in obs],
                                np.array([f.keypoints[kp] for f, kp in obs], np.float32), poses, R.K, 3.0)
        if r["cull"][0]:
            to_remove.append(pt)
    assert sorted(pt.slot for pt in local) == list(dry["local"])
    assert sorted(pt.slot for pt in to_remove) == list(dry["removed"]) and 0 < len(to_remove) < len(local)
    assert dry["xyz"].tobytes() == np.stack([g.points[p].position for p in dry["removed"]]).tobytes()
    outside = [p for p in model.alive_points() if model.obs[p] and p not in set(dry["local"])]
    assert outside                                                   # observed only by unlisted key frames: never local
    wet = R.cull(model, kfs, R.K, oracle, apply=True)
    assert np.array_equal(wet["removed"], dry["removed"])
    for pt in sorted(to_remove, key=lambda q: q.slot):
        g.remove_point(pt)
    g.same_as(model)
    assert model.consistent()


def test_the_gpu_cases_keep_their_means_away_from_the_threshold(oracle):
    """tests/test_gpu_keyframe.py compares culled SETS on these maps: no mean may sit where float noise could flip it."""
    for seed, n_kf, n_kp, P in R.GPU_CASES:
        model = R.build_model(R.random_scene(seed, n_kf, n_kp, P))
        r = R.cull(model, range(n_kf), R.K, oracle, apply=False)
        assert R.cull_margin(r["mean_err"]) >= R.CULL_MARGIN, (seed, R.cull_margin(r["mean_err"]))
        if P >= 255:
            assert 0 < len(r["removed"]) < len(r["local"]) < P
            assert len(R.reanchor_lists(model, range(1, n_kf))[0]) > 5
    for (seed, n_kf, n_kp, P), kw in R.GPU_OTHER_CASES:
        model = R.build_model(R.random_scene(seed, n_kf, n_kp, P, **kw))
        r = R.cull(model, range(n_kf), R.K, oracle, apply=False)
        assert R.cull_margin(r["mean_err"]) >= R.CULL_MARGIN, (seed, R.cull_margin(r["mean_err"]))
    assert max(len(o) for o in model.obs) <= 6 and max(len(o) for o in R.build_model(R.random_scene(23, 40, 40, 60, max_obs=40, pose_scale=0.1)).obs) == 40
