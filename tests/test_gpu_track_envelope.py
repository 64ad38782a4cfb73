"""The frame match table's kernels (racing-slam_amd/csrc/frame_matches.hip) on the cases of tests/track_cases.py, where
lists cross the 1024-thread stride, tables cross every `per` of the gather, marks land past the map's first device
capacities and hash chains run long and wrap.  Every comparison is an equality: integers against the case (which is
tests/track_ref.py's answer), the refit bit for bit against rs_refine_pose_inertial on the arrays track_ref gathers, the
match against rs_map_match fed the table's host lists and then track_ref.match_fold."""
import numpy as np
import pytest

import track_cases as TC
import track_ref
from conftest import to_np
from test_gpu_track import GpuSolver, SimpleMap, make_frame, rs_zero_summary, same_solve, set_table
from test_resident_map import Scene

pytestmark = pytest.mark.gpu

RAN = {"carry": set(), "add": set(), "gather": set(), "match": set()}


def i32(ctx, a):
    return ctx.dev(np.array(a, np.int32))              # (a copy: the cases' arrays are read-only)


class SlotMap(SimpleMap):
    """SimpleMap for more slots than a key frame has keypoints: observation o of point p is keypoint p % 8192 of key frame
    2 (p // 8192) + o.  `dead` slots are removed after they were observed (and flagged), as a tracker's map removes them."""

    def __init__(self, ctx, rs, positions, n_obs_built, consistent, dead):
        P = len(positions)
        self.map = rs.ResidentMap(ctx)
        with_obs = np.flatnonzero(np.asarray(n_obs_built) > 0)
        n_kf = 0 if not len(with_obs) else 2 * (int(with_obs.max()) // TC.FM_MAX) + 2
        for k in range(n_kf):
            f = make_frame(ctx, rs, min(P, TC.FM_MAX), seed=2000 + k)
            self.map.add_keyframe(f, np.eye(4, dtype=np.float32))
            f.close()
        for p in range(P):
            assert self.map.add_point(positions[p]) == p
            for o in range(int(n_obs_built[p])):
                self.map.add_observation(p, 2 * (p // TC.FM_MAX) + o, p % TC.FM_MAX)
        for p in np.flatnonzero(consistent):
            self.map.set_track_consistent(int(p))
        for p in dead:
            self.map.remove_point(int(p))
        self.positions = np.asarray(positions, np.float32).reshape(-1, 3)


@pytest.fixture(scope="module")
def carry_maps(ctx, rs):
    maps = {}

    def get(P):
        if P not in maps:
            m = TC.carry_map(P)
            maps[P] = SlotMap(ctx, rs, np.random.default_rng(P).normal(0, 5, (P, 3)).astype(np.float32), m["n_obs_built"], m["consistent"], m["dead"])
            assert maps[P].map.counts()["slots"] == P and maps[P].map.counts()["alive"] == int(m["alive"].sum())
        return maps[P]

    yield get
    for m in maps.values():
        m.close()


# ------------------------------------------------------------------------------------------------ carry
def run_carry(ctx, sm, prev, nxt, c, stats):
    """one rs_map_carry_matches of the case on freshly set tables; returns next's table and the stats (None without)"""
    set_table(ctx, prev, c["prev_table"])
    set_table(ctx, nxt, c["next_table"])
    d_stats = ctx.dev(np.full(2, -7, np.int32)) if stats else None
    sm.map.carry_matches(prev, nxt, i32(ctx, c["prev_index"]), None if c["inlier"] is None else i32(ctx, c["inlier"]),
                         None if c["count"] is None else i32(ctx, [c["count"]]), c["max_n"], c["min_points"], d_stats)
    got = nxt.matches()[0]
    assert np.array_equal(prev.matches()[0], c["prev_table"])          # prev is read only
    return got, None if d_stats is None else to_np(d_stats).tolist()


@pytest.mark.parametrize("case", TC.carry_cases(), ids=lambda c: c["name"])
def test_carry_case(ctx, rs, carry_maps, case):
    c, e = case, case["expect"]
    sm = carry_maps(c["P"])
    prev, nxt = make_frame(ctx, rs, c["n_prev"], 1), make_frame(ctx, rs, c["n_next"], 2)
    got, stats = run_carry(ctx, sm, prev, nxt, c, c["stats"])
    assert np.array_equal(got, e["table"])
    assert stats == ([e["candidates"], e["accepted"]] if c["stats"] else None)
    # the marks are clean: the same call on re-set tables gives the same bytes, with the other kind of stats pointer too
    again, stats = run_carry(ctx, sm, prev, nxt, c, not c["stats"])
    assert again.tobytes() == got.tobytes()
    assert stats == (None if c["stats"] else [e["candidates"], e["accepted"]])
    prev.close(); nxt.close()
    # ... and a small list without repeats on the same map still comes out right
    p = TC.carry_probe(c["P"])
    prev, nxt = make_frame(ctx, rs, p["n_prev"], 3), make_frame(ctx, rs, p["n_next"], 4)
    got, stats = run_carry(ctx, sm, prev, nxt, p, True)
    assert np.array_equal(got, p["expect"]["table"]) and stats == [p["expect"]["candidates"], p["expect"]["accepted"]]
    assert p["expect"]["accepted"] > 0
    prev.close(); nxt.close()
    RAN["carry"].add(c["name"])


# ------------------------------------------------------------------------------------------------ add
@pytest.mark.parametrize("case", TC.add_cases(), ids=lambda c: c["name"])
def test_add_case(ctx, rs, case):
    fr = make_frame(ctx, rs, case["n_kp"], 5)
    for with_count in (False, True):                   # a list taken whole: no count pointer, then a device count of max_n
        set_table(ctx, fr, case["start"])
        for li in case["lists"]:
            count = li["count"] if li["count"] is not None else (li["max_n"] if with_count else None)
            fr.matches_add(i32(ctx, li["kp"]), i32(ctx, li["point"]), None if count is None else i32(ctx, [count]), li["max_n"])
            got, cnt = fr.matches()
            assert np.array_equal(got, li["expect"]) and cnt == track_ref.num_matches(li["expect"])
    fr.close()
    RAN["add"].add(case["name"])


# ------------------------------------------------------------------------------------------------ gather and refit
@pytest.fixture(scope="module")
def gather_world(ctx, rs, synth):
    geom, m = TC.gather_geometry(synth), TC.gather_map()
    sm = SlotMap(ctx, rs, geom["positions"], m["n_obs"], np.zeros(m["P"], np.uint8), np.flatnonzero(m["alive"] == 0))
    assert sm.map.counts()["slots"] == m["P"]
    yield geom, m, sm
    sm.close()


def gather_kinds(n_kp):
    return (0, 1, 2) if n_kp in (3000, TC.FM_MAX) else (0,)


@pytest.mark.parametrize("n_kp", TC.GATHER_SIZES)
def test_gather_cases_refit_bit_for_bit(ctx, rs, gather_world, n_kp):
    geom, m, sm = gather_world
    p = geom["problem"]
    kp = TC.gather_keypoints(geom, n_kp)
    fr = rs.ResidentFrame(ctx, kp, np.random.default_rng(n_kp).integers(0, 256, (n_kp, 32), dtype=np.uint8))
    vel0 = np.array(p["delta"]["velocity"], np.float64)
    for c in [c for c in TC.gather_cases() if c["n_kp"] == n_kp]:
        set_table(ctx, fr, c["table"])
        for kind in gather_kinds(n_kp):
            kw = dict(prior=p["prior"] if kind == 1 else None, delta=p["delta"] if kind == 2 else None)
            want = track_ref.refine(GpuSolver(ctx), p["cam0"], c["table"], kp, m["alive"], m["n_obs"], geom["positions"], p["K"],
                                    min_matches=c["min_matches"], **kw)
            got = sm.map.refine_pose(fr, p["cam0"], p["K"], min_matches=c["min_matches"], **kw)
            assert got[3] == c["expect"]["n_used"] == want[3], c["name"]
            same_solve(got, want)
            if got[3] <= 0:                            # a gate refused: nothing moved, the summary is zero
                assert got[2] == rs_zero_summary() and np.array_equal(got[0], p["cam0"])
                assert np.array_equal(got[1], vel0 if kind == 2 else np.zeros(3))
            elif got[3] >= 100:
                assert got[2]["usable"] == 1 and got[2]["iterations"] > 0 and not np.array_equal(got[0], p["cam0"])
            RAN["gather"].add((c["name"], kind))
    fr.close()


# ------------------------------------------------------------------------------------------------ match
@pytest.fixture(scope="module")
def match_scene(ctx, rs, synth):
    sc = Scene(ctx, rs, synth, **TC.MATCH_SCENE)
    sc.remove_point(TC.MATCH_DEAD)
    yield sc
    sc.map.close()


def match_frame_of(ctx, rs, sc, n_kp):
    """the scene's own frame: its first keypoints, or all of them among clutter (as tests/test_gpu_track.py builds it)"""
    rng = np.random.default_rng(n_kp)
    kp, rows = sc.frame["keypoints"][:n_kp], sc.frame["descriptors"][:n_kp]
    if n_kp > len(kp):
        extra = n_kp - len(kp)
        kp = np.concatenate([kp, np.stack([rng.uniform(0, sc.frame["width"], extra), rng.uniform(0, sc.frame["height"], extra)], 1).astype(np.float32)])
        rows = np.concatenate([rows, rng.integers(0, 256, (extra, 32), dtype=np.uint8)])
    return rs.ResidentFrame(ctx, kp, rows)


def host_match(sc, frame, table, required, max_distance):
    """tests/test_gpu_track.py's host_match with a distance: rs_map_match fed the table's host lists (it refuses a slot
    past the map, which Frame::is_matched still counts: the keypoint's byte says so), then the host fold"""
    matched, pts = track_ref.match_inputs(table)
    f = sc.frame
    mk, mp = sc.map.match(frame, f["pose"], sc.K, f["width"], f["height"], kp_matched=matched, matched_points=pts[pts < len(sc.pos)],
                          required_observer=required, max_distance=max_distance)
    return track_ref.match_fold(table, mk, mp), len(mk)


@pytest.mark.parametrize("n_kp", [64, TC.FM_MAX])
def test_match_cases(ctx, rs, match_scene, n_kp):
    sc, f = match_scene, match_scene.frame
    cases = [c for c in TC.match_cases() if c["n_kp"] == n_kp]
    req = cases[0]["requires"]
    P = len(sc.pos)
    assert P == req["P"] and P % 4 != 0 and not sc.alive[req["dead"]] and sc.alive[P - 1] and len(sc.kf_pose) == req["n_kf"]
    assert sc.map.counts()["slots"] == P and all(sc.alive[p] for p in range(40, 44))
    fresh = sc.map.match(sc.rframe, f["pose"], sc.K, f["width"], f["height"])
    fr = match_frame_of(ctx, rs, sc, n_kp)
    new = 0
    for c in cases:
        start = TC.start_table(c)
        assert start[c["start_kp"][0]] == P - 1
        set_table(ctx, fr, start)
        want, n = host_match(sc, fr, start, c["required_observer"], c["max_distance"])
        got_n = sc.map.match_frame(fr, f["pose"], sc.K, f["width"], f["height"], required_observer=c["required_observer"],
                                   max_distance=c["max_distance"])
        got = fr.matches()[0]
        assert got_n == n and np.array_equal(got, want), c["name"]
        assert np.array_equal(got[start >= 0], start[start >= 0])          # what the table held stays, dead and past-the-map slots too
        new += n
        # a second pass over the table the first one left: the flags of its new matches are set and cleared too
        want, n = host_match(sc, fr, got, -1, c["max_distance"])
        assert sc.map.match_frame(fr, f["pose"], sc.K, f["width"], f["height"], max_distance=c["max_distance"]) == n
        assert np.array_equal(fr.matches()[0], want)
        RAN["match"].add(c["name"])
    assert new > 0
    with pytest.raises(rs.RsError):
        sc.map.match_frame(fr, f["pose"], sc.K, f["width"], f["height"], required_observer=req["n_kf"])
    # the flag table is clean: a plain rs_map_match of the scene's own frame matches as before any of it
    again = sc.map.match(sc.rframe, f["pose"], sc.K, f["width"], f["height"])
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1]) and len(fresh[0]) > 10
    fr.close()


def test_match_on_an_empty_map_and_an_empty_frame(ctx, rs, match_scene):
    sc, f = match_scene, match_scene.frame
    fresh = sc.map.match(sc.rframe, f["pose"], sc.K, f["width"], f["height"])
    empty = rs.ResidentMap(ctx)
    kf = make_frame(ctx, rs, 64, 6)
    assert empty.add_keyframe(kf, np.eye(4, dtype=np.float32)) == 0
    fr = match_frame_of(ctx, rs, sc, 64)
    start = TC.start_table(TC.match_cases()[0])
    set_table(ctx, fr, start)
    for required in (-1, 0):
        assert empty.match_frame(fr, f["pose"], sc.K, f["width"], f["height"], required_observer=required) == 0
        assert np.array_equal(fr.matches()[0], start)
    with pytest.raises(rs.RsError):
        empty.match_frame(fr, f["pose"], sc.K, f["width"], f["height"], required_observer=1)
    none = rs.ResidentFrame(ctx, np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8))
    for required in (-1, TC.MATCH_SCENE["n_kf"] - 1):
        assert sc.map.match_frame(none, f["pose"], sc.K, f["width"], f["height"], required_observer=required) == 0
    table, cnt = none.matches()
    assert len(table) == 0 and cnt == 0
    again = sc.map.match(sc.rframe, f["pose"], sc.K, f["width"], f["height"])
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1])
    none.close(); fr.close(); kf.close(); empty.close()


# ------------------------------------------------------------------------------------------------ nothing was skipped
def test_every_case_of_every_generator_ran():
    """Last in the file: a parametrisation that was deselected or lost would otherwise go unseen."""
    assert RAN["carry"] == {c["name"] for c in TC.carry_cases()} and len(RAN["carry"]) == len(TC.carry_cases())
    assert RAN["add"] == {c["name"] for c in TC.add_cases()} and len(RAN["add"]) == len(TC.add_cases())
    assert RAN["gather"] == {(c["name"], kind) for c in TC.gather_cases() for kind in gather_kinds(c["n_kp"])}
    assert RAN["match"] == {c["name"] for c in TC.match_cases()} and len(RAN["match"]) == len(TC.match_cases())
