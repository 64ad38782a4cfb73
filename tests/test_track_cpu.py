"""tests/track_ref.py (the CPU specification of racing-slam_amd/csrc/frame_matches.hip) against an independent object
model written from the reference: plain Python objects, Frame::add_map_match as the loop of src/Frame.cpp:80-102,
Tracker::track_from_last_frame as the two loops of src/Tracker.cpp:197-230.  No GPU."""
import numpy as np
import pytest

import refine_cases
import track_ref


class Point:
    def __init__(self, slot, n_obs=2, consistent=False):
        self.slot, self.n_obs, self.consistent = slot, n_obs, consistent


class Frame:
    """Frame's match bookkeeping (src/Frame.cpp:80-102, :123-151)."""

    def __init__(self, n):
        self.map_matches = [None] * n
        self.num_map_matches = 0
        self.matched_points = set()

    def add_map_match(self, point, keypoint_index):
        previous = self.map_matches[keypoint_index]
        if previous is point:
            return
        if previous is None:
            self.num_map_matches += 1
        else:
            self.matched_points.discard(previous)
        for i in range(len(self.map_matches)):
            if self.map_matches[i] is not point or i == keypoint_index:
                continue
            self.map_matches[i] = None
            if self.num_map_matches > 0:
                self.num_map_matches -= 1
        self.map_matches[keypoint_index] = point
        self.matched_points.add(point)

    def is_matched_kp(self, k):
        return self.map_matches[k] is not None

    def is_matched_point(self, p):
        return p in self.matched_points

    def table(self):
        return np.array([-1 if p is None else p.slot for p in self.map_matches], np.int32)


def frame_from(table, points):
    f = Frame(len(table))
    for k, p in enumerate(table):
        if p >= 0:
            f.add_map_match(points[p], k)
    return f


def random_table(rng, n, P, fill):
    t = np.full(n, -1, np.int32)
    k = rng.choice(n, min(int(fill * n), P), replace=False)
    t[k] = rng.choice(P, len(k), replace=False)
    return t


@pytest.mark.parametrize("seed", range(12))
def test_matches_add_equals_the_sequential_rule(seed):
    """Random edit sequences: lists with repeated keypoints, repeated points, both, out-of-range entries and clamped
    counts, applied one list after the other to one table."""
    rng = np.random.default_rng(seed)
    n, P = int(rng.integers(1, 70)), int(rng.integers(1, 90))
    points = [Point(p) for p in range(P)]
    table = random_table(rng, n, P, rng.uniform(0, 0.8))
    frame = frame_from(table, points)
    for _ in range(6):
        m = int(rng.integers(0, 3 * n + 2))
        kp = rng.integers(0, max(1, n // int(rng.integers(1, 4))), m)          # a narrow range repeats keypoints
        pt = rng.integers(0, max(1, P // int(rng.integers(1, 4))), m)
        bad = rng.random(m) < 0.1
        kp = np.where(bad & (rng.random(m) < 0.5), rng.choice([-1, n, n + 7], m), kp)
        pt = np.where(bad & (kp >= 0) & (kp < n), -1 - rng.integers(0, 3, m), pt)
        count = [None, m, m + 5, -3, m // 2][int(rng.integers(0, 5))]
        for i in range(track_ref.clamp_count(count, m)):
            if 0 <= kp[i] < n and pt[i] >= 0:
                frame.add_map_match(points[pt[i]], int(kp[i]))
        table = track_ref.matches_add(table, kp, pt, count)
        assert np.array_equal(table, frame.table())
        assert track_ref.num_matches(table) == frame.num_map_matches
        live = table[table >= 0]
        assert len(np.unique(live)) == len(live)


def model_carry(points, prev, nxt, prev_index, inliers, min_points):
    """src/Tracker.cpp:197-230 on the object model; inliers = the (query = next, train = prev) index pairs."""
    cand = []
    for q, t in inliers:
        if not prev.is_matched_kp(t):
            continue
        p = prev.map_matches[t]
        if p.n_obs < 2 and not p.consistent:
            continue
        cand.append((p, q))
    if len(cand) < min_points:
        return len(cand), 0
    acc = 0
    for p, q in cand:
        if nxt.is_matched_kp(q) or nxt.is_matched_point(p):
            continue
        nxt.add_map_match(p, q)
        acc += 1
    return len(cand), acc


@pytest.mark.parametrize("seed", range(10))
def test_carry_equals_the_reference_loops(seed):
    rng = np.random.default_rng(100 + seed)
    P, n_prev, n_next = 120, 90, 100
    points = [Point(p, n_obs=int(rng.integers(1, 4)), consistent=bool(rng.random() < 0.3)) for p in range(P)]
    alive = np.ones(P, np.uint8)
    n_obs = np.array([p.n_obs for p in points])
    cons = np.array([p.consistent for p in points], np.uint8)
    prev_t = random_table(rng, n_prev, P, 0.7)
    next_t = random_table(rng, n_next, P, rng.choice([0.0, 0.2]))
    n_list = 60
    prev_index = np.sort(rng.choice(n_prev, n_list, replace=False)).astype(np.int32)       # d_kept_index: ascending
    inl = None if seed % 3 == 0 else np.sort(rng.choice(n_list, int(rng.integers(5, n_list)), replace=False)).astype(np.int32)
    if seed % 4 == 3:                                    # a list no tracker produces: repeated positions
        inl = rng.integers(0, n_list, 50).astype(np.int32)
    count = n_list if inl is None else len(inl)
    min_points = [15, 1, 40][seed % 3]
    prev, nxt = frame_from(prev_t, points), frame_from(next_t, points)
    pairs = [(int(j), int(prev_index[j])) for j in (range(count) if inl is None else inl)]
    want = model_carry(points, prev, nxt, prev_index, pairs, min_points)
    got_t, c, a = track_ref.carry(alive, n_obs, cons, prev_t, next_t, prev_index, inl, count, n_list, min_points)
    assert (c, a) == want and np.array_equal(got_t, nxt.table())


def test_carry_skips_dead_slots_and_bad_indices():
    alive = np.array([1, 0, 1], np.uint8)
    n_obs, cons = np.array([2, 2, 2]), np.zeros(3, np.uint8)
    prev_t, next_t = np.array([0, 1, 2, -1], np.int32), np.full(4, -1, np.int32)
    t, c, a = track_ref.carry(alive, n_obs, cons, prev_t, next_t, np.array([0, 1, 2, 9], np.int32), np.array([0, 1, 2, 3, -1, 7], np.int32),
                              6, 4, 1)
    assert (c, a) == (2, 2) and t.tolist() == [0, -1, 2, -1]


def test_gather_order_gates_and_filter():
    rng = np.random.default_rng(5)
    P, n = 60, 50
    table = random_table(rng, n, P, 0.8)
    kp = rng.uniform(0, 500, (n, 2)).astype(np.float32)
    alive = (rng.random(P) < 0.9).astype(np.uint8)
    n_obs = rng.integers(1, 4, P)
    pos = rng.normal(0, 5, (P, 3)).astype(np.float32)
    pts, uv, m = track_ref.gather(table, kp, alive, n_obs, pos)
    ks = [k for k in range(n) if table[k] >= 0 and alive[table[k]] and n_obs[table[k]] >= 2]
    assert m == len(ks) > 10 and pts.dtype == np.float64
    assert np.array_equal(uv, kp[ks]) and np.array_equal(pts, pos[table[ks]].astype(np.float64))
    few = table.copy()
    few[np.flatnonzero(few >= 0)[14:]] = -1
    assert track_ref.gather(few, kp, alive, n_obs, pos)[2] == -1                       # 14 matches: the :307 gate
    assert track_ref.gather(table, kp, alive, np.ones(P, int), pos)[2] == 0            # enough matches, none with 2 observations


def test_refine_is_the_oracle_on_the_gathered_arrays_and_agrees_with_dense_lm(oracle, synth):
    import dense_lm
    case = refine_cases.CASES["n63"]
    p = refine_cases.problem(synth, case)
    n = len(p["points"])
    pos = p["points"].astype(np.float32)
    table = np.full(2 * n, -1, np.int32)
    table[::2] = np.arange(n)[::-1]                     # keypoint 2 i holds point n - 1 - i
    kp = np.zeros((2 * n, 2), np.float32)
    kp[::2] = p["uv"][::-1]
    alive, n_obs = np.ones(n, np.uint8), np.full(n, 2)
    cam, _, s, used = track_ref.refine(oracle, p["cam0"], table, kp, alive, n_obs, pos, p["K"])
    assert used == n and s["usable"] == 1
    q = dict(p, points=pos[::-1].astype(np.float64), uv=p["uv"][::-1].copy())
    dcam, _, ds = refine_cases.solve_dense(dense_lm, oracle, q, case)
    assert ds["iterations"] == s["iterations"] and np.allclose(cam, dcam, rtol=1e-7, atol=1e-9)
    cam2, _, s2, used2 = track_ref.refine(oracle, p["cam0"], table, kp, alive, np.ones(n, int), pos, p["K"])
    assert used2 == 0 and s2 is None and np.array_equal(cam2, p["cam0"])


def test_match_through_the_oracle_folds_into_the_table(oracle, synth, rs):
    w = synth.make_ba_window(n_kf=5, n_points=200, run_max=4, config_id=81)
    frame, mp = synth.make_match_scene(w, n_keypoints=150, kdtree_build=rs.kdtree_build, config_id=81)
    mp = dict(mp, eligible=np.ones(len(mp["positions"]), np.uint8))
    t0 = np.full(150, -1, np.int32)
    t1, c1 = track_ref.match(oracle, frame, mp, t0, required_kf=4)
    t2, c2 = track_ref.match(oracle, frame, mp, t1, required_kf=-1)
    assert c1 > 0 and c2 > 0 and track_ref.num_matches(t2) == c1 + c2
    assert np.array_equal(t2[t1 >= 0], t1[t1 >= 0])                  # the second match leaves the first one's alone
    live = t2[t2 >= 0]
    assert len(np.unique(live)) == len(live)


def test_the_shim_fragment_makes_the_four_calls_and_has_a_harness():
    """What needs only this repository of integration/reference_shim/Tracker_track_tail.inc (type-checking it needs the
    upstream headers: integration/check_shim_syntax.py)."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "integration", "reference_shim", "Tracker_track_tail.inc")).read()
    order = [text.index(c) for c in ("ok(rs_map_carry_matches(", "ok(rs_map_refine_pose(", "ok(rs_map_match_frame(", "rs_frame_matches_download(")]
    assert order == sorted(order) and text.count("ok(rs_map_match_frame(") == 2
    assert "is_rotation_plausible" in text
    checker = open(os.path.join(root, "integration", "check_shim_syntax.py")).read()
    assert '#include "Tracker_track_tail.inc"' in checker and "Tracker::track(" in checker
