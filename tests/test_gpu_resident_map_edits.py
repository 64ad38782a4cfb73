"""The device-resident map (rs_map, csrc/map.hip) under the edits the reference makes between uses (src/Map.cpp:44-124),
checked against the host model tests/map_model.py.  Every edit is applied to the model, which returns the C-ABI calls
that drive the same edit on the rs_map; at checkpoints the map's counts and positions must equal the model's exactly and
every match mode must equal the oracle and the flat path on the model's flattening.  Local-BA windows on edited maps
(subsets, permutations, fixed frames, dead slots, more than one k_win_scan chunk) must give the model's free set and the
flat solve of the model-built problem; the loop-closure point transform must follow the edited observers.

What reaches what:
  rs_map_remove_observation through the ABI      every test (Mirror.replay), test_a_disassociated_keypoint_is_free_...
  remove_observation alone, then a use           test_edit_sequences_match_the_model (checkpoints)
  k_win_scan carry across chunks, dead slots     test_ba_windows_on_an_edited_map_of_3000_slots, ..._scan_chunk_boundary
  subset / permutation / fixed frames in a list  test_ba_windows_on_an_edited_map_of_3000_slots
  >= 2 observations only through other frames,
  only listed observer fixed                     the same windows (the model's free set and rs_map_window, exactly)
  Pf == 0, all frames fixed, capacity < n        test_ba_windows_on_an_edited_map_of_3000_slots
  pool growth after matches and a BA, promoted
  rframe, a key frame with zero keypoints        test_edit_sequences_match_the_model
  pose graph after the owners were edited        test_pose_graph_after_edits
  refusals                                       test_invalid_edits_are_refused_and_leave_the_map_unchanged"""
import numpy as np
import pytest

from conftest import to_np
from map_model import EDIT_WEIGHTS, MapModel, random_edit

pytestmark = pytest.mark.gpu

BA_FAILURE = 5                     # RS_BA_FAILURE, include/rsgpu.h


def bits(a):
    return np.ascontiguousarray(a, np.float32).tobytes()


class Mirror:
    """A MapModel and an rs_map driven by the same edits.  The initial map is the scene of test_resident_map.Scene: key
    frames of synth.make_ba_window with their observations' descriptors plus a few unmatched keypoints, and the newest
    frame of synth.make_match_scene as the frame that is matched (rframe)."""

    def __init__(self, ctx, rs, synth, n_kf=6, n_points=600, seed=3, n_keypoints=500):
        self.ctx, self.rs = ctx, rs
        w = synth.make_ba_window(n_kf=n_kf, n_points=n_points, run_max=5, config_id=70 + seed)
        frame, mp = synth.make_match_scene(w, n_keypoints=n_keypoints, kdtree_build=rs.kdtree_build, config_id=70 + seed)
        self.w, self.frame, self.K = w, frame, w["K"]
        self.model, self.map = MapModel(), rs.ResidentMap(ctx)
        self.touched = []                        # key frames of the latest observation edits, newest last
        pool_of_obs = mp["desc_pool"][mp["obs_desc"]]
        kp_index = np.zeros(len(w["obs_cam"]), np.int64)
        for k in range(n_kf):
            sel = np.flatnonzero(w["obs_cam"] == k)
            kp_index[sel] = np.arange(len(sel))
            rng = np.random.default_rng(100 + k)
            desc = np.concatenate([pool_of_obs[sel], rng.integers(0, 256, (7, 32), dtype=np.uint8)])
            kp = np.concatenate([w["obs_uv"][sel], rng.uniform(0, 500, (7, 2)).astype(np.float32)])
            self.add_keyframe(kp, desc, w["poses_true"][k])
        for p in range(n_points):
            o = range(w["obs_ptr"][p], w["obs_ptr"][p + 1])
            self.replay(self.model.create_point(mp["positions"][p], [(int(w["obs_cam"][i]), int(kp_index[i])) for i in o])[1])
        self.rframe = rs.ResidentFrame(ctx, frame["keypoints"], frame["descriptors"])

    def close(self):
        self.map.close()
        self.rframe.close()

    def add_keyframe(self, kp, desc, pose, frame=None):
        kf, _ = self.model.add_keyframe(kp, desc, pose)
        fr = frame if frame is not None else self.rs.ResidentFrame(self.ctx, np.asarray(kp, np.float32).reshape(-1, 2),
                                                                    np.asarray(desc, np.uint8).reshape(-1, 32))
        assert self.map.add_keyframe(fr, self.model.kf_pose[kf]) == kf
        if frame is None:
            fr.close()
        return kf

    def replay(self, calls):
        m = self.map
        for c in calls:
            op, a = c[0], c[1:]
            if op == "add_point":
                assert m.add_point(a[0]) == self.model.n_slots() - 1      # the model has just appended the slot
            elif op == "add_observation":
                m.add_observation(*a)
                self.touched.append(a[1])
            elif op == "remove_observation":
                m.remove_observation(*a)
                self.touched.append(a[1])
            elif op == "remove_point":
                m.remove_point(a[0])
            elif op == "set_position":
                m.set_position(*a)
            elif op == "set_keyframe_pose":
                m.set_keyframe_pose(*a)
            else:
                raise AssertionError(op)

    def edit(self, rng, weights=EDIT_WEIGHTS):
        kind, calls = random_edit(self.model, rng, weights)
        self.replay(calls)
        return kind

    # -- checks
    def check_state(self):
        assert self.map.counts() == self.model.counts()
        assert bits(self.map.positions()) == bits(self.model.positions())           # dead slots included

    def check_match(self, oracle, kp_matched=None, matched_points=(), required=-1, only=None, replace=0):
        """rs_map_match == oracle.reproj_match == ctx.reproj_match on the model's flattening, in index and point"""
        fr = dict(self.frame)
        fr["kp_matched"] = np.zeros(len(fr["keypoints"]), np.uint8) if kp_matched is None else kp_matched
        if only is None:
            mp = self.model.match_arrays(matched_points, required)
        else:
            mp = self.model.fuse_view(only, matched_points, required)
        ref = oracle.reproj_match(fr, mp, replace=replace)
        fv, k1 = self.ctx.make_frame_view(fr)
        mv, k2 = self.ctx.make_map_view(mp)
        flat = self.ctx.reproj_match(fv, mv, replace=replace)
        n = int(to_np(flat["count"])[0])
        assert np.array_equal(to_np(flat["match_kp"])[:n], ref["match_kp"])
        assert np.array_equal(to_np(flat["match_point"])[:n], ref["match_point"])
        want_pt = ref["match_point"] if only is None else np.asarray(only, np.int32)[ref["match_point"]]
        mk, mpt = self.map.match(self.rframe, fr["pose"], self.K, fr["width"], fr["height"], kp_matched=kp_matched,
                                 matched_points=matched_points, required_observer=required, only_points=only, replace=replace)
        assert np.array_equal(mk, ref["match_kp"]) and np.array_equal(mpt, want_pt)
        return mk, mpt

    def check_all_modes(self, oracle, rng):
        """match_map; match_key_frame for the key frame whose observations changed last; kp_matched + matched points;
        an unsorted match_for_fuse list holding dead slots; then a plain match_map: the flag table was left clean."""
        n_all = len(self.check_match(oracle)[0])
        assert n_all > 20
        self.check_match(oracle, required=self.touched[-1] if self.touched else 0)
        P = self.model.n_slots()
        kpm = (rng.random(len(self.frame["keypoints"])) < 0.3).astype(np.uint8)
        pts = rng.choice(P, min(P, 80), replace=False)
        self.check_match(oracle, kp_matched=kpm, matched_points=pts)
        dead = np.flatnonzero(np.array(self.model.alive) == 0)
        only = np.concatenate([rng.choice(P, min(P, 200), replace=False), dead[:20]])
        rng.shuffle(only)
        assert len(dead) == 0 or np.any(np.isin(only, dead))
        self.check_match(oracle, kp_matched=kpm, only=only.astype(np.int32), replace=1)
        assert len(self.check_match(oracle)[0]) == n_all


def check_ba(mi, ctx, rs, oracle, kfs, free, capacity=None):
    """rs_map_bundle_adjust on the window (kfs, free) against the model's frame-side window: the free set exactly, the flat
    solve of the model-built problem (same LM schedule, cost to 1e-9), the oracle on that problem; fixed poses and
    non-free slots bit-unchanged.  The model then takes the map's result, and a match checks that the map holds it."""
    model = mi.model
    kfs, free = np.asarray(kfs, np.int32), np.asarray(free, np.uint8)
    win = model.ba_window(kfs, free)
    n = len(win["points"])
    dev = mi.map.window(kfs, free)                                  # the device-built problem, unsolved: exactly the model's
    for key in ("points", "obs_ptr", "obs_cam"):
        assert np.array_equal(dev[key], win[key]), key
    assert dev["obs_uv"].tobytes() == win["obs_uv"].tobytes() and dev["positions"].tobytes() == win["positions"].tobytes()
    pos0 = mi.map.positions().copy()
    poses0 = [model.kf_pose[k].copy() for k in kfs]
    s, poses, out_pts, out_xyz = mi.map.bundle_adjust(kfs, free, mi.K, capacity=capacity)
    assert len(poses) == len(kfs)
    if n == 0:                                                       # the empty-window path: nothing to solve
        assert s["usable"] == 0 and s["termination"] == BA_FAILURE and s["n_points"] == 0 and len(out_pts) == 0
        assert all(bits(poses[c]) == bits(poses0[c]) for c in range(len(kfs)))
        assert bits(mi.map.positions()) == bits(pos0)
        return s
    cams = np.stack([rs.pack_pose(model.kf_pose[k].reshape(4, 4)) for k in kfs])
    dc, dp = ctx.dev(cams), ctx.dev(win["positions"])
    args = (ctx.dev(win["obs_ptr"]), ctx.dev(win["obs_cam"]), ctx.dev(win["obs_uv"]))
    s_flat = ctx.bundle_adjust(dc, free, dp, *args, mi.K)
    assert s["usable"] == 1 and (s["iterations"], s["successful_steps"]) == (s_flat["iterations"], s_flat["successful_steps"])
    assert np.isclose(s["final_cost"], s_flat["final_cost"], rtol=1e-9)
    k = n if capacity is None else min(n, capacity)
    assert s["n_points"] == n and np.array_equal(out_pts, win["points"][:k])
    after = mi.map.positions()
    assert bits(out_xyz) == bits(after[win["points"][:k]])
    assert np.allclose(after[win["points"]], to_np(dp).astype(np.float32), rtol=1e-6, atol=1e-6)
    fc = to_np(dc)
    for c in range(len(kfs)):
        if free[c]:
            assert np.allclose(poses[c], rs.unpack_pose(fc[c]).reshape(16), rtol=1e-6, atol=1e-6)
        else:
            assert bits(poses[c]) == bits(poses0[c])
    rc, rp, rs_ = oracle.bundle_adjust(cams, free, win["positions"], win["obs_ptr"], win["obs_cam"], win["obs_uv"], mi.K)
    assert (rs_["iterations"], rs_["successful_steps"]) == (s_flat["iterations"], s_flat["successful_steps"])
    assert np.allclose(fc, rc, rtol=1e-7, atol=1e-9)
    rest = np.ones(len(pos0), bool)
    rest[win["points"]] = False
    assert bits(after[rest]) == bits(pos0[rest])
    # the model takes the map's result (poses of free frames, positions of free points)
    for c in np.flatnonzero(free):
        model.set_pose(int(kfs[c]), poses[c])
    for p in win["points"]:
        model.pos[p] = after[p].copy()
    mi.check_state()
    return s


# ------------------------------------------------------------------------------------------ edit sequences
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_edit_sequences_match_the_model(ctx, rs, oracle, synth, seed):
    mi = Mirror(ctx, rs, synth, n_kf=6, n_points=600, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    mi.check_state()
    mi.check_all_modes(oracle, rng)
    kinds = {}
    for i in range(1, 241):
        k = mi.edit(rng)
        kinds[k] = kinds.get(k, 0) + 1
        if i == 50:                                      # a key frame with zero keypoints, then more edits around it
            kf0 = mi.add_keyframe(np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8), mi.model.kf_pose[-1])
            mi.check_match(oracle, required=kf0)
        if i == 100:                                     # the frame just matched becomes a key frame; its matches associate
            mk, mpt = mi.check_match(oracle)
            kf = mi.add_keyframe(mi.frame["keypoints"], mi.frame["descriptors"], mi.frame["pose"], frame=mi.rframe)
            for kp, p in zip(mk, mpt):
                mi.replay(mi.model.associate(kf, int(p), int(kp)))
            assert len(mi.check_match(oracle, required=kf)[0]) > 0
        if i == 150:                                     # a BA, then a key frame larger than the whole pool: it must grow
            check_ba(mi, ctx, rs, oracle, np.arange(mi.model.n_kf()), [0, 0] + [1] * (mi.model.n_kf() - 2))
            mk, mpt = mi.check_match(oracle)
            # the pools at least double when they grow, so a key frame with as many rows as the pool holds always outgrows it;
            # its first rows are the matched frame's, so the matches below are observations at the end of the grown pools
            rows = sum(len(k) for k in mi.model.kf_kp)
            big = np.random.default_rng(seed)
            kp = np.concatenate([mi.frame["keypoints"], big.uniform(0, 1920, (rows, 2)).astype(np.float32)])
            desc = np.concatenate([mi.frame["descriptors"], big.integers(0, 256, (rows, 32), dtype=np.uint8)])
            kf = mi.add_keyframe(kp, desc, mi.frame["pose"])
            for q, p in zip(mk, mpt):
                mi.replay(mi.model.associate(kf, int(p), int(q)))
        if i % 40 == 0:
            mi.check_state()
            mi.check_all_modes(oracle, rng)
            # observations removed with nothing else in between: the next use must still see them gone
            kf = int(np.argmax([int((t >= 0).sum()) for t in mi.model.kp_point]))
            for p in [int(x) for x in mi.model.kp_point[kf] if x >= 0][:6]:
                mi.replay(mi.model.disassociate(kf, p))
            mi.check_match(oracle, required=kf)
            mi.check_match(oracle)
    assert min(kinds.values()) >= 5 and len(kinds) == len(EDIT_WEIGHTS)
    # the old rows of both pools survived the growth: a BA over every key frame, then every match mode
    check_ba(mi, ctx, rs, oracle, np.arange(mi.model.n_kf()), [0, 0] + [1] * (mi.model.n_kf() - 2))
    mi.check_all_modes(oracle, rng)
    mi.close()


def test_a_disassociated_keypoint_is_free_for_another_point(ctx, rs, oracle, synth):
    """Map::disassociate frees the key frame's keypoint (Frame::remove_map_match): a later associate of another point to
    it must not reach back to the point that left, wherever that point is observed in the key frame now."""
    mi = Mirror(ctx, rs, synth, n_kf=4, n_points=200, seed=15)
    model = mi.model
    kf = 2
    p, q = [int(x) for x in model.kp_point[kf] if x >= 0][:2]
    kp_p = model.observer_kp(p, kf)
    free_kp = int(np.flatnonzero(model.kp_point[kf] < 0)[0])
    mi.replay(model.disassociate(kf, p))
    mi.replay(model.associate(kf, p, free_kp))             # p is back in the key frame at another keypoint
    mi.replay(model.associate(kf, q, kp_p))                # q takes p's old keypoint
    assert model.observer_kp(p, kf) == free_kp and model.observer_kp(q, kf) == kp_p
    mi.check_state()
    mi.check_match(oracle, required=kf)
    mi.close()


# ------------------------------------------------------------------------------------------ BA windows
def edited_window_map(ctx, rs, synth, n_points, seed, n_kf=8, dead_frac=0.4, n_edits=150, weights=EDIT_WEIGHTS):
    mi = Mirror(ctx, rs, synth, n_kf=n_kf, n_points=n_points, seed=seed)
    rng = np.random.default_rng(2000 + seed)
    for p in rng.choice(n_points - 1, int(dead_frac * n_points), replace=False):
        mi.replay(mi.model.remove_point(int(p)))
    for _ in range(n_edits):
        mi.edit(rng, weights)
    for k in range(2, n_kf):                             # perturb the poses: the solves have something to do
        T = mi.model.kf_pose[k].reshape(4, 4).copy()
        T[:3, 3] += rng.normal(0, 0.01, 3).astype(np.float32)
        mi.replay(mi.model.set_pose(k, T))
    mi.check_state()
    return mi, rng


def test_ba_windows_on_an_edited_map_of_3000_slots(ctx, rs, oracle, synth):
    """3300 slots (k_win_scan: four 1024-slot chunks), 40% of them dead"""
    mi, rng = edited_window_map(ctx, rs, synth, n_points=3300, seed=11)
    assert mi.model.n_slots() >= 3300 and mi.model.counts()["alive"] < 0.65 * mi.model.n_slots()
    # a free frame whose points were all removed
    gone = [int(p) for p in mi.model.kp_point[6] if p >= 0]
    for p in gone:
        mi.replay(mi.model.remove_point(p))
    assert gone and not np.any(mi.model.kp_point[6] >= 0)
    windows = [
        ([1, 2, 4, 5, 7], [0, 1, 1, 1, 1], None),          # ascending subset
        (rng.permutation(8), [0, 0, 1, 1, 1, 1, 1, 1], 37),  # permutation, output truncated to 37 slots
        ([7, 2, 5, 0, 3], [1, 0, 1, 0, 1], None),          # fixed frames interleaved with free ones
        ([4], [1], None),                                  # a single free frame
        ([5, 6, 7], [0, 1, 1], None),                      # a free frame without points, next to one with points
        ([6, 3], [1, 0], None),                            # the only free frame has no points: empty window
        ([0, 1, 2], [0, 0, 0], None),                      # all frames fixed: FAILURE
        ([], [], None),                                    # no frames
    ]
    solved = 0
    for kfs, free, cap in windows:
        s = check_ba(mi, ctx, rs, oracle, kfs, free, capacity=cap)
        solved += s["usable"]
        if cap is not None:
            assert s["n_points"] > cap
        mi.check_match(oracle)
    assert solved == 5
    # the window's last free point lies in the last chunk
    w = mi.model.ba_window(np.arange(8, dtype=np.int32), np.r_[0, 0, np.ones(6)].astype(np.uint8))
    assert w["points"][-1] >= 3072
    mi.close()


@pytest.mark.parametrize("n_points", [1024, 1025])
def test_ba_window_at_the_scan_chunk_boundary(ctx, rs, oracle, synth, n_points):
    """k_win_scan scans 1024 slots per step: exactly one full chunk, and one more slot that is a free point"""
    no_new_slots = {k: v for k, v in EDIT_WEIGHTS.items() if k not in ("create_point", "remove_point", "fuse")}
    mi, rng = edited_window_map(ctx, rs, synth, n_points=n_points, seed=12, n_kf=6, dead_frac=0.2, n_edits=60, weights=no_new_slots)
    assert mi.model.n_slots() == n_points
    kfs, free = np.arange(6, dtype=np.int32), np.array([0, 0, 1, 1, 1, 1], np.uint8)
    w = mi.model.ba_window(kfs, free)
    assert w["points"][-1] == n_points - 1                 # the last slot is free: the carry reaches it
    check_ba(mi, ctx, rs, oracle, kfs, free)
    mi.check_match(oracle)
    mi.close()


# ------------------------------------------------------------------------------------------ loop closure after edits
def test_pose_graph_after_edits(ctx, rs, oracle, synth):
    """Disassociating a point's lowest-index observer moves its anchor (src/Optimization.cpp:512-536); the resident
    transform must follow the edited observers, and the map then keeps matching and optimising from the result."""
    mi = Mirror(ctx, rs, synth, n_kf=8, n_points=800, seed=13)
    rng = np.random.default_rng(13)
    model = mi.model
    moved = 0
    for p in rng.choice(800, 300, replace=False):
        p = int(p)
        if len(model.obs[p]) >= 2:
            owner = min(kf for kf, _ in model.obs[p])
            mi.replay(model.disassociate(owner, p))
            moved += 1
    for p in rng.choice(800, 100, replace=False):
        if model.alive[p]:
            mi.replay(model.remove_point(int(p)))
    assert moved > 150
    # drift the newer key frames, then close the loop 7 -> 0 on the true trajectory
    Tt = mi.w["poses_true"].astype(np.float64)
    for k in range(1, 8):
        T = model.kf_pose[k].reshape(4, 4).copy()
        T[:3, 3] += np.float32(0.004 * k)
        mi.replay(model.set_pose(k, T))
    loops = [(7, 0, Tt[7] @ np.linalg.inv(Tt[0])), (6, 1, Tt[6] @ np.linalg.inv(Tt[1]))]
    before = np.stack(model.kf_pose)
    want_poses, want_rot, s0, _ = rs.pose_graph(before, loops)
    optr, okf = model.transform_csr()
    want_pos = oracle.transform_points(optr, okf, before, want_poses.reshape(-1, 16), model.positions())
    s, poses, rot = mi.map.pose_graph(loops)
    assert s == s0 and s["usable"] == 1
    assert bits(poses) == bits(want_poses) and bits(rot) == bits(want_rot)
    got = mi.map.positions()
    assert bits(got) == bits(want_pos)
    assert np.any(got != model.positions())
    for k in range(8):
        model.kf_pose[k] = poses[k].reshape(16).copy()
    model.pos = [x.copy() for x in got]
    mi.check_state()
    mi.check_all_modes(oracle, rng)
    check_ba(mi, ctx, rs, oracle, [3, 4, 5, 6, 7], [0, 1, 1, 1, 1])
    mi.check_match(oracle)
    mi.close()


# ------------------------------------------------------------------------------------------ refusals
def test_invalid_edits_are_refused_and_leave_the_map_unchanged(ctx, rs, oracle, synth):
    mi = Mirror(ctx, rs, synth, n_kf=4, n_points=200, seed=14)
    model, m = mi.model, mi.map
    dead = 5
    mi.replay(model.remove_point(dead))
    n_kp = len(model.kf_kp[1])
    refused = [
        lambda: m.add_observation(dead, 1, 0),             # edits of a removed point
        lambda: m.remove_observation(dead, 1),
        lambda: m.set_position(dead, [1, 2, 3]),
        lambda: m.remove_point(dead),
        lambda: m.add_observation(200, 1, 0),              # a slot that does not exist
        lambda: m.add_observation(-1, 1, 0),
        lambda: m.add_observation(3, 4, 0),                # out-of-range key frame
        lambda: m.add_observation(3, -1, 0),
        lambda: m.remove_observation(3, 4),
        lambda: m.set_keyframe_pose(4, np.eye(4)),
        lambda: m.add_observation(3, 1, n_kp),             # out-of-range keypoint
        lambda: m.add_observation(3, 1, -1),
        lambda: m.bundle_adjust([0, 2, 1, 2], [0, 1, 1, 1], mi.K),     # a key frame listed twice
        lambda: m.bundle_adjust([0, 4], [0, 1], mi.K),                 # a key frame that does not exist
        lambda: m.match(mi.rframe, mi.frame["pose"], mi.K, 1920, 1080, required_observer=4),
        lambda: m.match(mi.rframe, mi.frame["pose"], mi.K, 1920, 1080, only_points=[3, 200]),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(rs.RsError):
            call()
        mi.check_state()
    mi.check_all_modes(oracle, np.random.default_rng(14))
    mi.close()
