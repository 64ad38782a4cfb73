"""The tail of Tracker::track on the device (racing-slam_amd/csrc/frame_matches.hip): a frame's match table, the
carry-over from the previous frame, the pose refit from the map and the two matches, against tests/track_ref.py
(integers byte for byte), against rs_refine_pose_inertial on the arrays track_ref gathers (bit for bit: it is the same
kernel body on the same numbers in the same order) and against rs_map_match fed the table's host lists."""
import numpy as np
import pytest

import refine_cases
import track_ref
from conftest import to_np
from test_resident_map import Scene

pytestmark = pytest.mark.gpu


def i32(ctx, a):
    return ctx.dev(np.asarray(a, np.int32))


def make_frame(ctx, rs, n, seed=0):
    rng = np.random.default_rng([77, seed, n])
    return rs.ResidentFrame(ctx, rng.uniform(0, 600, (n, 2)).astype(np.float32), rng.integers(0, 256, (n, 32), dtype=np.uint8))


def random_table(rng, n, P, fill):
    t = np.full(n, -1, np.int32)
    k = rng.choice(n, min(int(fill * n), P), replace=False)
    t[k] = rng.choice(P, len(k), replace=False)
    return t


def set_table(ctx, frame, table):
    frame.matches_clear()
    k = np.flatnonzero(table >= 0)
    if len(k):
        frame.matches_add(i32(ctx, k), i32(ctx, table[k]))
    got, cnt = frame.matches()
    assert np.array_equal(got, table) and cnt == len(k)


class SimpleMap:
    """A resident map whose point p has n_obs[p] observations (key frame o, keypoint p), for the stages that read only
    alive / observation count / track_consistent / position."""

    def __init__(self, ctx, rs, positions, n_obs, consistent=(), dead=()):
        P = len(positions)
        self.map = rs.ResidentMap(ctx)
        for k in range(int(max(n_obs, default=0))):
            f = make_frame(ctx, rs, max(P, 1), seed=1000 + k)
            self.map.add_keyframe(f, np.eye(4, dtype=np.float32))
            f.close()
        for p in range(P):
            assert self.map.add_point(positions[p]) == p
            for o in range(int(n_obs[p])):
                self.map.add_observation(p, o, p)
        self.alive, self.n_obs = np.ones(P, np.uint8), np.array(n_obs).copy()
        self.consistent = np.zeros(P, np.uint8)
        self.positions = np.asarray(positions, np.float32).reshape(-1, 3)
        for p in consistent:
            self.map.set_track_consistent(int(p))
            self.consistent[p] = 1
        for p in dead:
            self.map.remove_point(int(p))
            self.alive[p], self.n_obs[p] = 0, 0

    def close(self):
        self.map.close()


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 8192])
def test_table_add_equals_the_sequential_rule(ctx, rs, n):
    rng = np.random.default_rng(n)
    fr = make_frame(ctx, rs, n)
    table, cnt = fr.matches()
    assert np.array_equal(table, np.full(n, -1, np.int32)) and cnt == 0
    P = 3 * n + 5
    for rep_kp, rep_pt in ((1, 1), (3, 1), (1, 3), (3, 3)):          # plain, repeated keypoints, repeated points, both
        m = min(8192, 2 * n + 3)
        kp = rng.integers(0, max(1, n // rep_kp), m).astype(np.int32)
        pt = rng.integers(0, max(1, P // (rep_pt * 3 if rep_pt > 1 else 1)), m).astype(np.int32)
        bad = rng.random(m) < 0.05
        kp[bad] = rng.choice([-1, n, n + 100, 2 ** 30], int(bad.sum()))
        pt[rng.random(m) < 0.03] = -2
        for count in (None, m + 9, -4, m // 2):
            dc = None if count is None else i32(ctx, [count])
            fr.matches_add(i32(ctx, kp), i32(ctx, pt), dc, m)
            table = track_ref.matches_add(table, kp, pt, count, m)
            got, cnt = fr.matches()
            assert np.array_equal(got, table) and cnt == track_ref.num_matches(table)
    assert track_ref.num_matches(table) > 0
    fr.matches_clear()
    assert fr.matches()[1] == 0
    fr.close()


def test_table_is_cleared_by_reassign_and_refuses_long_lists(ctx, rs):
    rng = np.random.default_rng(3)
    fr = rs.DeviceFrame(ctx, 300)
    pts = ctx.dev(rng.uniform(0, 500, (300, 2)).astype(np.float32))
    desc = ctx.dev(rng.integers(0, 256, (300, 32), dtype=np.uint8))
    assert fr.assign(desc, pts, i32(ctx, [200])) == 200
    fr.matches_add(i32(ctx, np.arange(0, 200, 2)), i32(ctx, np.arange(100)))
    got, cnt = fr.matches()
    assert cnt == 100 and np.array_equal(got[::2], np.arange(100)) and np.all(got[1::2] == -1)
    assert fr.assign(desc, pts, i32(ctx, [260])) == 260                 # nothing of the previous frame shows through
    got, cnt = fr.matches()
    assert cnt == 0 and np.all(got == -1) and len(got) == 260
    with pytest.raises(rs.RsError):
        fr.matches_add(i32(ctx, np.zeros(8193)), i32(ctx, np.zeros(8193)))
    fr.close()


# ------------------------------------------------------------------------------------------------ carry-over
def carry_case(ctx, rs, n_cand, with_inliers=True, prepopulate=False, repeats=False):
    """prev holds 40 points: points 0 .. n_cand-1 pass the :209 gate (2 observations, or 1 and track-consistent), the
    others fail it (1 observation) or are dead.  The dead one was track-consistent when it was removed (the flag survives
    removal), so only the dead-slot rule keeps it out."""
    rng = np.random.default_rng([9, n_cand, int(with_inliers), int(prepopulate), int(repeats)])
    P = 60
    n_obs = np.ones(P, int)
    n_obs[:n_cand:2] = 2
    cons = list(range(1, n_cand, 2))
    sm = SimpleMap(ctx, rs, rng.normal(0, 5, (P, 3)).astype(np.float32), n_obs, consistent=cons + [n_cand + 1], dead=[n_cand + 1])
    assert sm.consistent[n_cand + 1] and not sm.alive[n_cand + 1]
    n_prev, n_next, n_list = 80, 90, 50
    prev, nxt = make_frame(ctx, rs, n_prev, 1), make_frame(ctx, rs, n_next, 2)
    prev_t = np.full(n_prev, -1, np.int32)
    prev_t[rng.choice(n_prev, 40, replace=False)] = np.arange(40)
    # every matched keypoint of prev is tracked, so the candidates are exactly the gate's
    kept = np.sort(np.concatenate([np.flatnonzero(prev_t >= 0), rng.choice(np.flatnonzero(prev_t < 0), n_list - 40, replace=False)]))
    inl = np.arange(n_list) if with_inliers else None
    if repeats:
        inl = np.concatenate([inl, inl[::3]])
        rng.shuffle(inl)
    next_t = np.full(n_next, -1, np.int32)
    if prepopulate:                      # keypoint-taken and point-taken both fire
        cand_pos = [j for j in range(n_list) if 0 <= prev_t[kept[j]] < n_cand]
        next_t[cand_pos[0]] = 55                                  # the keypoint of the first candidate is taken
        next_t[n_list + 3] = prev_t[kept[cand_pos[1]]]            # the point of the second one is matched elsewhere
    set_table(ctx, prev, prev_t)
    set_table(ctx, nxt, next_t)
    stats = ctx.dev(np.full(2, -7, np.int32))
    max_n = 2 * n_list
    d_kept = i32(ctx, np.concatenate([kept, np.full(max_n - n_list, -1)]))
    count = n_list if inl is None else len(inl)
    d_inl = None if inl is None else i32(ctx, np.concatenate([inl, np.zeros(max_n - len(inl))]))
    sm.map.carry_matches(prev, nxt, d_kept, d_inl, i32(ctx, [count]), max_n, 15, stats)
    want_t, c, a = track_ref.carry(sm.alive, sm.n_obs, sm.consistent, prev_t, next_t, np.concatenate([kept, np.full(max_n - n_list, -1)]),
                                   None if inl is None else inl, count, max_n, 15)
    got, _ = nxt.matches()
    assert np.array_equal(got, want_t) and to_np(stats).tolist() == [c, a]
    assert np.array_equal(prev.matches()[0], prev_t)
    # the mark array is clean: the same call on a cleared frame gives the same answer
    set_table(ctx, nxt, next_t)
    sm.map.carry_matches(prev, nxt, d_kept, d_inl, i32(ctx, [count]), max_n, 15, stats)
    assert np.array_equal(nxt.matches()[0], want_t)
    prev.close(); nxt.close(); sm.close()
    return c, a


@pytest.mark.parametrize("n_cand", [14, 15, 16])
def test_carry_around_min_points(ctx, rs, n_cand):
    c, a = carry_case(ctx, rs, n_cand)
    assert c == n_cand and a == (0 if n_cand < 15 else n_cand)


def test_carry_without_inlier_list_prepopulated_and_repeated(ctx, rs):
    assert carry_case(ctx, rs, 20, with_inliers=False) == (20, 20)
    assert carry_case(ctx, rs, 20, prepopulate=True) == (20, 18)
    c, a = carry_case(ctx, rs, 20, repeats=True)
    assert c > 20 and a == 20
    assert carry_case(ctx, rs, 20, prepopulate=True, repeats=True)[1] == 18


def test_carry_sees_points_added_after_an_earlier_carry(ctx, rs):
    """A tracker adds points at every key frame: the device's track-consistent flags must follow the map as it grows, not
    only the map as it was at the first call."""
    rng = np.random.default_rng(21)
    P0, n_new = 45, 10
    n_obs = np.ones(P0, int)
    n_obs[:30] = 2
    sm = SimpleMap(ctx, rs, rng.normal(0, 5, (P0, 3)).astype(np.float32), n_obs)
    n_prev, n_next = 80, 90
    prev, nxt = make_frame(ctx, rs, n_prev, 3), make_frame(ctx, rs, n_next, 4)
    kept = np.arange(n_prev, dtype=np.int32)
    d_kept, stats = i32(ctx, kept), ctx.dev(np.zeros(2, np.int32))

    def run(prev_t):
        set_table(ctx, prev, prev_t)
        nxt.matches_clear()
        sm.map.carry_matches(prev, nxt, d_kept, None, None, n_prev, 15, stats)
        want, c, a = track_ref.carry(sm.alive, sm.n_obs, sm.consistent, prev_t, np.full(n_next, -1, np.int32), kept, None, None, n_prev, 15)
        assert np.array_equal(nxt.matches()[0], want) and to_np(stats).tolist() == [c, a]
        return c

    prev_t = np.full(n_prev, -1, np.int32)
    prev_t[rng.choice(n_prev, P0, replace=False)] = np.arange(P0)
    assert run(prev_t) == 30
    # a key frame's worth of new points with one observation each (key frame 1 has keypoints 30 .. 44 free)
    for i in range(n_new):
        p = sm.map.add_point(rng.normal(0, 5, 3).astype(np.float32))
        assert p == P0 + i
        sm.map.add_observation(p, 1, 30 + i)
    sm.alive, sm.n_obs = np.concatenate([sm.alive, np.ones(n_new, np.uint8)]), np.concatenate([sm.n_obs, np.ones(n_new, int)])
    sm.consistent = np.concatenate([sm.consistent, np.zeros(n_new, np.uint8)])
    prev_t[rng.choice(np.flatnonzero(prev_t < 0), n_new, replace=False)] = np.arange(P0, P0 + n_new)
    assert run(prev_t) == 30                              # one observation, not track-consistent: none of them is carried
    for p in (P0 + 2, P0 + 7):
        sm.map.set_track_consistent(p)
        sm.consistent[p] = 1
    assert run(prev_t) == 32
    # past the first capacity of the device image (4096 slots): the arrays are reallocated, the flags with them
    for i in range(4100):
        sm.map.add_point(np.zeros(3, np.float32))
    grown = 4100
    sm.alive, sm.n_obs = np.concatenate([sm.alive, np.ones(grown, np.uint8)]), np.concatenate([sm.n_obs, np.zeros(grown, int)])
    sm.consistent = np.concatenate([sm.consistent, np.zeros(grown, np.uint8)])
    last = P0 + n_new + grown - 1
    prev_t[np.flatnonzero(prev_t < 0)[:3]] = [last, last - 1, last - 2000]
    assert run(prev_t) == 32
    sm.map.set_track_consistent(last)
    sm.consistent[last] = 1
    assert run(prev_t) == 33
    prev.close(); nxt.close(); sm.close()


# ------------------------------------------------------------------------------------------------ refit
class GpuSolver:
    """rs_refine_pose_inertial on uploaded arrays, with track_ref.refine's solver interface."""

    def __init__(self, ctx):
        self.ctx = ctx

    def refine_pose_inertial(self, cam, pts, uv, K, prior=None, delta=None, options=None):
        return self.ctx.refine_pose_inertial(cam, self.ctx.dev(pts), self.ctx.dev(uv), K, prior=prior, delta=delta, options=options)


def refine_scene(ctx, rs, synth, n, kind, seed=0):
    """n points with two observations spread over a frame's table among 20 points with one observation and a dead one."""
    case = dict(scene=dict(refine_cases.DEFAULT_SCENE, n=n, seed=300 + n + seed, imu=kind == 2), opt={},
                prior=(1e-3, 0.01) if kind == 1 else None, delta=kind == 2)
    p = refine_cases.problem(synth, case)
    rng = np.random.default_rng([5, n, kind])
    extra = 21
    pos = np.concatenate([p["points"].astype(np.float32), rng.normal(0, 5, (extra, 3)).astype(np.float32)])
    n_obs = np.concatenate([np.full(n, 2), np.ones(extra, int)])
    sm = SimpleMap(ctx, rs, pos, n_obs, dead=[n + extra - 1])
    N = n + extra + 13
    keys = rng.permutation(N)[:n + extra]
    kp = rng.uniform(0, 600, (N, 2)).astype(np.float32)
    kp[keys[:n]] = p["uv"]
    table = np.full(N, -1, np.int32)
    table[keys] = np.arange(n + extra)
    fr = rs.ResidentFrame(ctx, kp, rng.integers(0, 256, (N, 32), dtype=np.uint8))
    set_table(ctx, fr, table)
    return p, sm, fr, table, kp


def same_solve(a, b):
    cam_a, vel_a, s_a, n_a = a
    cam_b, vel_b, s_b, n_b = b
    assert n_a == n_b
    assert cam_a.tobytes() == cam_b.tobytes() and vel_a.tobytes() == vel_b.tobytes()
    if s_b is None:
        assert s_a == dict(rs_zero_summary())
    else:
        assert s_a.keys() == s_b.keys()
        for k in s_a:
            assert np.array([s_a[k]]).tobytes() == np.array([s_b[k]]).tobytes(), k


def rs_zero_summary():
    return dict(termination=0, iterations=0, successful_steps=0, usable=0, initial_cost=0.0, final_cost=0.0, final_radius=0.0)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 511, 512, 513, 2000])
def test_refine_is_bit_identical_to_the_solve_on_gathered_arrays(ctx, rs, synth, n, kind):
    p, sm, fr, table, kp = refine_scene(ctx, rs, synth, n, kind)
    want = track_ref.refine(GpuSolver(ctx), p["cam0"], table, kp, sm.alive, sm.n_obs, sm.positions, p["K"], prior=p["prior"], delta=p["delta"])
    assert want[3] == n and want[2] is not None
    got = sm.map.refine_pose(fr, p["cam0"], p["K"], prior=p["prior"], delta=p["delta"])
    same_solve(got, want)
    if n > 1:
        assert got[2]["usable"] == 1 and got[2]["iterations"] > 0 and not np.array_equal(got[0], p["cam0"])
    again = sm.map.refine_pose(fr, p["cam0"], p["K"], prior=p["prior"], delta=p["delta"])       # two calls in a row repeat byte for byte
    same_solve(again, got)
    fr.close(); sm.close()


def test_refine_gates(ctx, rs, synth):
    p, sm, fr, table, kp = refine_scene(ctx, rs, synth, 40, 2, seed=1)
    zero = rs_zero_summary()
    vel0 = np.array(p["delta"]["velocity"], np.float64)
    few = table.copy()
    few[np.flatnonzero(few >= 0)[14:]] = -1                            # 14 table entries: :307
    set_table(ctx, fr, few)
    cam, vel, s, used = sm.map.refine_pose(fr, p["cam0"], p["K"], delta=p["delta"])
    assert used == -1 and s == zero and np.array_equal(cam, p["cam0"]) and np.array_equal(vel, vel0)
    ones = np.full(len(table), -1, np.int32)                           # 15 entries, every point with one observation
    ones[:15] = np.arange(40, 55)
    set_table(ctx, fr, ones)
    cam, vel, s, used = sm.map.refine_pose(fr, p["cam0"], p["K"], delta=p["delta"])
    assert used == 0 and s == zero and np.array_equal(cam, p["cam0"]) and np.array_equal(vel, vel0)
    same_solve((cam, vel, s, used), track_ref.refine(GpuSolver(ctx), p["cam0"], ones, kp, sm.alive, sm.n_obs, sm.positions, p["K"], delta=p["delta"]))
    # a dead point in the table: it counts as a match, it is not an observation
    set_table(ctx, fr, table)
    for dead in (3, 17):
        sm.map.remove_point(dead)
        sm.alive[dead], sm.n_obs[dead] = 0, 0
    want = track_ref.refine(GpuSolver(ctx), p["cam0"], table, kp, sm.alive, sm.n_obs, sm.positions, p["K"], delta=p["delta"])
    got = sm.map.refine_pose(fr, p["cam0"], p["K"], delta=p["delta"])
    assert got[3] == 38
    same_solve(got, want)
    fr.close(); sm.close()


# ------------------------------------------------------------------------------------------------ the two matches
def host_match(sc, frame, fdict, table, required):
    """rs_map_match fed the table's host lists, then the host fold."""
    matched, pts = track_ref.match_inputs(table)
    mk, mp = sc.map.match(frame, fdict["pose"], sc.K, fdict["width"], fdict["height"], kp_matched=matched, matched_points=pts,
                          required_observer=required)
    return track_ref.match_fold(table, mk, mp), len(mk)


def device_match(sc, frame, fdict, required):
    return sc.map.match_frame(frame, fdict["pose"], sc.K, fdict["width"], fdict["height"], required_observer=required)


@pytest.fixture(scope="module")
def scene(ctx, rs, synth):
    sc = Scene(ctx, rs, synth, n_kf=6, n_points=300, seed=4)
    yield sc
    sc.map.close()


@pytest.mark.parametrize("n_kp", [64, 6500])
def test_match_frame_equals_map_match_and_fold(ctx, rs, synth, scene, n_kp):
    sc = scene
    # the scene's own frame (its rows belong to the map's pool): its first 64 keypoints, or all 500 among 6000 of clutter
    rng = np.random.default_rng(n_kp)
    kp, rows = sc.frame["keypoints"][:n_kp], sc.frame["descriptors"][:n_kp]
    if n_kp > len(kp):
        extra = n_kp - len(kp)
        kp = np.concatenate([kp, np.stack([rng.uniform(0, sc.frame["width"], extra), rng.uniform(0, sc.frame["height"], extra)], 1).astype(np.float32)])
        rows = np.concatenate([rows, rng.integers(0, 256, (extra, 32), dtype=np.uint8)])
    fd = dict(pose=sc.frame["pose"], width=sc.frame["width"], height=sc.frame["height"])
    fr = rs.ResidentFrame(ctx, kp, rows)
    fresh = sc.map.match(sc.rframe, sc.frame["pose"], sc.K, sc.frame["width"], sc.frame["height"])
    total = 0
    # on an empty table: the tracker's sequence, the last key frame and then the whole map
    table = np.full(n_kp, -1, np.int32)
    for required in (5, -1):
        table, c = host_match(sc, fr, fd, table, required)
        assert device_match(sc, fr, fd, required) == c
        assert np.array_equal(fr.matches()[0], table)
        total += c
    assert total > (0 if n_kp == 64 else 10)
    # after a carry-over: a table that already holds matches (some of them of points the matcher would have taken)
    keep = np.flatnonzero(table >= 0)[::2]
    start = np.full(n_kp, -1, np.int32)
    start[keep] = table[keep]
    free_kp = np.flatnonzero(table < 0)
    unused = np.setdiff1d(np.arange(300), table[table >= 0])
    m = min(len(free_kp), len(unused), 20)
    start[rng.choice(free_kp, m, replace=False)] = rng.choice(unused, m, replace=False)
    prev = make_frame(ctx, rs, n_kp, 5)                  # the previous frame holds them at the same keypoints, all track-consistent
    set_table(ctx, prev, start)
    consistent = np.zeros(300, np.uint8)
    for p in start[start >= 0]:
        sc.map.set_track_consistent(int(p))
        consistent[p] = 1
    fr.matches_clear()
    d_same = i32(ctx, np.arange(n_kp))
    sc.map.carry_matches(prev, fr, d_same, None, None, n_kp, 1)
    table, _, carried = track_ref.carry(np.array(sc.alive, np.uint8), np.array([len(o) for o in sc.obs]), consistent, start,
                                        np.full(n_kp, -1, np.int32), np.arange(n_kp), None, None, n_kp, 1)
    assert carried == track_ref.num_matches(start) > 0 and np.array_equal(table, start)
    assert np.array_equal(fr.matches()[0], table)
    prev.close()
    for required in (4, -1):
        table, c = host_match(sc, fr, fd, table, required)
        assert device_match(sc, fr, fd, required) == c
        assert np.array_equal(fr.matches()[0], table)
    live = table[table >= 0]
    assert len(np.unique(live)) == len(live)
    # the flag table is clean: a plain rs_map_match matches as on a fresh map
    again = sc.map.match(sc.rframe, sc.frame["pose"], sc.K, sc.frame["width"], sc.frame["height"])
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1]) and len(fresh[0]) > 10
    fr.close()


# ------------------------------------------------------------------------------------------------ the chain
def test_chain_from_tracked_lists_to_matches_with_no_host_list(ctx, rs, synth):
    """rs_track_features' outputs (synthetic) -> rs_estimate_pose -> rs_frame_assign_device -> carry -> refine -> match x2
    at 256 keypoints, against the step-by-step host form on downloaded lists."""
    sc = Scene(ctx, rs, synth)
    rng = np.random.default_rng(11)
    K = np.asarray(sc.K, np.float64)
    W, H = sc.frame["width"], sc.frame["height"]
    T1 = np.asarray(sc.frame["pose"], np.float64).reshape(4, 4)
    T0 = T1.copy()
    T0[:3, 3] += np.array([0.3, 0.05, 0.6])                       # the previous frame: a step back and to the side
    X = np.array(sc.pos, np.float64)
    uv0, z0 = synth.project(T0, K, X)
    uv1, z1 = synth.project(T1, K, X)
    inside = lambda uv, z: (z > 0.5) & (uv[:, 0] > 40) & (uv[:, 0] < W - 40) & (uv[:, 1] > 40) & (uv[:, 1] < H - 40)   # noqa: E731
    vis = np.flatnonzero(inside(uv0, z0) & inside(uv1, z1))
    assert len(vis) >= 60
    n_tr = min(100, int(0.6 * len(vis)))
    tracked, fresh = vis[:n_tr], vis[n_tr:n_tr + 60]              # points prev sees and tracks / points only the matcher can find
    desc_of = lambda p: sc.kf_desc[sc.obs[p][0][0]][sc.obs[p][0][1]]      # noqa: E731
    n_prev = n_tr + 40
    # prev: the tracked points, then clutter; its table holds the first 60 % of them
    kp_prev = np.concatenate([uv0[tracked], rng.uniform(50, 1000, (40, 2))]).astype(np.float32)
    prev = rs.ResidentFrame(ctx, kp_prev, rng.integers(0, 256, (n_prev, 32), dtype=np.uint8))
    prev_t = np.full(n_prev, -1, np.int32)
    n_held = int(0.6 * n_tr)
    prev_t[:n_held] = tracked[:n_held]
    set_table(ctx, prev, prev_t)
    # the tracked list: prev's tracked keypoints without every 9th, then 10 of the clutter that "tracked" somewhere wrong
    kept = np.concatenate([np.setdiff1d(np.arange(n_tr), np.arange(4, n_tr, 9)), np.arange(n_tr, n_tr + 10)]).astype(np.int32)
    n_t = len(kept)
    good = kept < n_tr
    kept_pt = np.where(good[:, None], uv1[tracked[np.minimum(kept, n_tr - 1)]] + rng.normal(0, 0.2, (n_t, 2)),
                       rng.uniform(50, 1000, (n_t, 2))).astype(np.float32)
    n_b = 256 - n_t
    pt_b = np.concatenate([uv1[fresh] + rng.normal(0, 0.5, (len(fresh), 2)), rng.uniform(50, 1000, (n_b - len(fresh), 2))]).astype(np.float32)
    rows = rng.integers(0, 256, (256, 32), dtype=np.uint8)
    for i in np.flatnonzero(good):
        rows[i] = desc_of(int(tracked[kept[i]]))
    for i, p in enumerate(fresh):
        rows[n_t + i] = desc_of(int(p))
    cap = 300
    kept_full = np.concatenate([kept, np.full(cap - n_t, -1)]).astype(np.int32)
    d_kept = i32(ctx, kept_full)
    d_kept_pt = ctx.dev(np.concatenate([kept_pt, np.zeros((cap - n_t, 2), np.float32)]))
    d_count = i32(ctx, [n_t])
    d_desc = ctx.dev(np.concatenate([rows, np.zeros((cap - 256, 32), np.uint8)]))
    est = ctx.pose_estimator(cap, 256)
    po = ctx.estimate_pose(est, ctx.dev(kp_prev), d_kept_pt, d_count, cap, sc.K, d_from_index=d_kept, max_hypotheses=256)
    nxt = rs.DeviceFrame(ctx, cap)
    assert nxt.assign(d_desc, d_kept_pt, d_count, ctx.dev(pt_b), i32(ctx, [n_b])) == 256
    stats = ctx.dev(np.zeros(2, np.int32))
    sc.map.carry_matches(prev, nxt, d_kept, po["inlier_index"], po["inlier_count"], cap, 15, stats)
    Tn = T1.copy()
    Tn[:3, 3] += np.array([0.01, -0.008, 0.012])
    cam0 = rs.pack_pose(Tn.astype(np.float32))
    cam, _, s, used = sc.map.refine_pose(nxt, cam0, sc.K)
    pose = rs.unpack_pose(cam)
    c1 = sc.map.match_frame(nxt, pose, sc.K, W, H, required_observer=5)
    c2 = sc.map.match_frame(nxt, pose, sc.K, W, H, required_observer=-1)
    got_table, got_n = nxt.matches()
    # the host form, step by step
    n_in = int(to_np(po["inlier_count"])[0])
    inl = to_np(po["inlier_index"])[:n_in]
    assert int(to_np(po["status"])[0]) == 0 and n_in >= n_t // 2
    alive, n_obs = np.array(sc.alive, np.uint8), np.array([len(o) for o in sc.obs])
    table, c, a = track_ref.carry(alive, n_obs, np.zeros(len(alive), np.uint8), prev_t, np.full(256, -1, np.int32), kept_full, inl, n_in,
                                  cap, 15)
    assert to_np(stats).tolist() == [c, a] and a >= 15
    kp_next = np.concatenate([kept_pt, pt_b])
    want = track_ref.refine(GpuSolver(ctx), cam0, table, kp_next, alive, n_obs, np.array(sc.pos, np.float32), sc.K)
    same_solve((cam, np.zeros(3), s, used), want)
    assert s["usable"] == 1 and used == a
    host = rs.ResidentFrame(ctx, kp_next, rows)
    fd = dict(pose=pose, width=W, height=H)
    table, h1 = host_match(sc, host, fd, table, 5)
    table, h2 = host_match(sc, host, fd, table, -1)
    assert (c1, c2) == (h1, h2) and h1 + h2 > 0
    assert np.array_equal(got_table, table) and got_n == track_ref.num_matches(table)
    for o in (host, nxt, prev, est):
        o.close()
    sc.map.close()
