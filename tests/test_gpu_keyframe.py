"""Mapper::insert on the resident map (csrc/map.hip, csrc/map_keyframe.hip): rs_map_insert_keyframe,
rs_map_add_track_points, rs_map_reanchor and rs_map_cull_points against tests/keyframe_ref.py, the flattened forms
(rs_reanchor_points, rs_point_errors) and the oracle, on small maps built through the public calls.

The maps (keyframe_ref.GPU_CASES) have 3 - 6 key frames of 40 - 300 keypoints and 0, 1, 255, 256, 257, 1023, 1025 and 4097
point slots: across the block size, k_kf_compact's 1024-slot chunks and the 4096-slot growth of the map buffers.  A point
has at most one observation per key frame, so these maps reach 6 observations per point; the 40-observation lists are in
test_long_observation_lists on a map of 40 small key frames.  tests/test_keyframe_cpu.py checks on the CPU that no mean
error of these maps lies within 1e-3 px of the culling threshold, so the set comparisons test the kernel and not float noise.
The whole chain through the C++ host form (slam::insert_key_frame) runs in tests/test_keyframe_host.py.
test_every_buffer_of_the_map_is_outgrown_in_use grows one map of 64-keypoint key frames past every first capacity of the
device image (GROW_STEPS), with the calls above and the other readers of the image in between."""
import numpy as np
import pytest

import keyframe_ref as R
from conftest import to_np

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).tobytes()


def replay_on(m):
    def replay(calls):
        for c in calls:
            op, a = c[0], c[1:]
            if op == "add_point":
                m.add_point(a[0])
            elif op == "add_observation":
                m.add_observation(*a)
            elif op == "remove_observation":
                m.remove_observation(*a)
            elif op == "remove_point":
                m.remove_point(a[0])
            elif op == "set_position":
                m.set_position(*a)
            elif op == "set_keyframe_pose":
                m.set_keyframe_pose(*a)
            else:
                raise AssertionError(op)
    return replay


def map_of(ctx, rs, model):
    """An rs_map rebuilt from scratch from a model's state: key frames, every slot in order (dead ones added and removed),
    observations in the model's order."""
    m = rs.ResidentMap(ctx)
    for k in range(model.n_kf()):
        f = rs.ResidentFrame(ctx, model.kf_kp[k], model.kf_desc[k])
        assert m.add_keyframe(f, model.kf_pose[k]) == k
        f.close()
    for p in range(model.n_slots()):
        assert m.add_point(model.pos[p]) == p
    order = sorted((i, p, kf, kp) for p in range(model.n_slots()) for i, (kf, kp) in enumerate(model.obs[p]))
    for _, p, kf, kp in order:
        m.add_observation(p, kf, kp)
    for p in range(model.n_slots()):
        if not model.alive[p]:
            m.remove_point(p)
    return m


class Case:
    def __init__(self, ctx, rs, case, extra=10, **kw):
        seed, n_kf, n_kp, P = case
        self.ctx, self.rs, self.n_kf, self.P = ctx, rs, n_kf, P
        self.scene = R.random_scene(seed, n_kf, n_kp, P, **kw)
        self.model = R.build_model(self.scene)
        self.map = map_of(ctx, rs, self.model)
        fr = self.fr = R.match_frame_of(self.model, seed, extra=extra)
        self.fpose = fr["pose"]
        self.frame = rs.ResidentFrame(ctx, fr["keypoints"], fr["descriptors"])
        self.replay = replay_on(self.map)

    def close(self):
        self.frame.close()
        self.map.close()

    def match(self, m=None, required=-1):
        mk, mp = (m or self.map).match(self.frame, self.fpose, R.K, R.WIDTH, R.HEIGHT, required_observer=required)
        return mk.tolist(), mp.tolist()

    def same_as_rebuilt(self, kfs):
        """counts, positions, match results and the BA window equal those of a map rebuilt from the model"""
        ref = map_of(self.ctx, self.rs, self.model)
        try:
            assert self.map.counts() == ref.counts() == self.model.counts()
            assert bits(self.map.positions()) == bits(self.model.positions())
            assert self.match() == self.match(ref)
            assert self.match(required=self.n_kf - 1) == self.match(ref, required=self.n_kf - 1)
            free = np.r_[0, np.ones(len(kfs) - 1)].astype(np.uint8)
            a, b = self.map.window(kfs, free), ref.window(kfs, free)
            assert all(np.array_equal(a[k], b[k]) for k in a)
        finally:
            ref.close()

    def move_poses(self, kfs, seed):
        """the adjustment moved the listed key frames: returns their poses before"""
        rng = np.random.default_rng(seed)
        before = np.stack([self.model.kf_pose[k] for k in kfs]).astype(np.float32)
        for k in kfs:
            self.replay(self.model.set_pose(k, R.perturb_pose(self.model.kf_pose[k], rng)))
        return before


# ------------------------------------------------------------------------------------------ rs_map_reanchor
@pytest.mark.parametrize("case", R.GPU_CASES, ids=lambda c: f"P{c[3]}")
def test_reanchor(ctx, rs, oracle, case):
    c = Case(ctx, rs, case)
    model = c.model
    kfs = list(range(1, c.n_kf))                           # key frame 0 is not optimised
    before = c.move_poses(kfs, case[0])
    after = np.stack([model.kf_pose[k] for k in kfs]).astype(np.float32)
    pos0 = model.positions().copy()
    pts, fidx = R.reanchor_lists(model, kfs)
    n, slots, xyz = c.map.reanchor(kfs, before)
    assert n == len(pts) and np.array_equal(slots, pts)
    if len(pts):                                           # the flattened K13 on the lists the restatement builds: bit for bit
        d_pos = ctx.dev(pos0)
        ctx.reanchor_points(ctx.dev(pts), ctx.dev(fidx), ctx.dev(before), ctx.dev(after), d_pos)
        assert bits(xyz) == bits(to_np(d_pos)[pts])
    want_pts, want_xyz = R.reanchor(model, kfs, before, oracle)          # the oracle (and the model takes the result)
    assert np.array_equal(xyz.view(np.uint32), want_xyz.view(np.uint32))
    got = c.map.positions()
    rest = np.setdiff1d(np.arange(c.P), pts).astype(np.int64)
    assert bits(got[rest]) == bits(pos0[rest])             # two observers, dead, observer unlisted, no observer: byte for byte
    if c.P >= 255:
        kinds = dict(two=0, unlisted=0, none=0)
        for p in rest:
            o = model.obs[p]
            kinds["none" if not o else "two" if len(o) > 1 else "unlisted"] += 1
        assert min(kinds.values()) > 0 and len(pts) > 5 and np.any(got[pts] != pos0[pts]), kinds
    if c.P:
        c.same_as_rebuilt(kfs)                             # the mirror and the device image both hold the new positions
    c.close()


def test_reanchor_with_dead_slots_capacity_and_a_second_call(ctx, rs, oracle):
    c = Case(ctx, rs, (21, 5, 150, 700))
    model = c.model
    rng = np.random.default_rng(21)
    single = [p for p in model.alive_points() if len(model.obs[p]) == 1]
    for p in rng.choice(single, 30, replace=False):        # removed points that HAD one listed observer
        c.replay(model.remove_point(int(p)))
    kfs = [4, 2, 1]                                        # a permuted subset
    before = c.move_poses(kfs, 5)
    pts, _ = R.reanchor_lists(model, kfs)
    pos0 = model.positions().copy()
    n, slots, xyz = c.map.reanchor(kfs, before, capacity=7)
    assert n == len(pts) > 7 and np.array_equal(slots, pts[:7])
    _, want_xyz = R.reanchor(model, kfs, before, oracle)
    assert bits(xyz) == bits(want_xyz[:7])
    dead = np.flatnonzero(np.array(model.alive) == 0)
    assert len(dead) == 30 and bits(c.map.positions()[dead]) == bits(pos0[dead])
    c.same_as_rebuilt(kfs)
    # again with before == after: every listed point is reported and none moves more than rounding
    same = np.stack([model.kf_pose[k] for k in kfs])
    n2, slots2, xyz2 = c.map.reanchor(kfs, same)
    assert n2 == n and np.array_equal(slots2, pts)
    _, want2 = R.reanchor(model, kfs, same, oracle)
    assert bits(xyz2) == bits(want2)
    c.same_as_rebuilt(kfs)
    c.close()


# ------------------------------------------------------------------------------------------ rs_map_cull_points
def flat_cull(ctx, model, kfs, max_mean_error=3.0):
    """rs_point_errors on the flattened local set, its d_cull_idx mapped back to slots"""
    pr = R.cull_problem(model, kfs)
    if len(pr["local"]) == 0:
        return np.zeros(0, np.int32)
    out = ctx.point_errors(ctx.dev(pr["positions"]), ctx.dev(pr["obs_ptr"]), ctx.dev(pr["obs_pose"]), ctx.dev(pr["obs_uv"]),
                           ctx.dev(pr["poses"]), R.K, max_mean_error)
    k = int(to_np(out["cull_count"])[0])
    return pr["local"][to_np(out["cull_idx"])[:k]]


@pytest.mark.parametrize("case", R.GPU_CASES, ids=lambda c: f"P{c[3]}")
def test_cull_points(ctx, rs, oracle, case):
    c = Case(ctx, rs, case)
    model = c.model
    kfs = list(range(1, c.n_kf))                           # points seen only by key frame 0 are not local
    want = R.cull(model, kfs, R.K, oracle, apply=False)
    assert R.cull_margin(want["mean_err"]) >= R.CULL_MARGIN
    counts0, match0 = c.map.counts(), c.match()
    dry = c.map.cull_points(kfs, R.K, apply=False)
    assert np.array_equal(dry["removed"], flat_cull(ctx, model, kfs))          # the flattened K12, bit for bit
    assert np.array_equal(dry["removed"], want["removed"]) and dry["n_removed"] == len(want["removed"])
    assert dry["n_local"] == len(want["local"]) and bits(dry["xyz"]) == bits(want["xyz"])
    assert c.map.counts() == counts0 == model.counts() and c.match() == match0      # apply = 0 changed nothing
    if c.P >= 255:
        only0 = [p for p in model.alive_points() if model.obs[p] and all(kf == 0 for kf, _ in model.obs[p])]
        bad0 = R.cull(model, [0], R.K, oracle, apply=False)["removed"]
        assert set(only0) & set(bad0.tolist()) and not set(only0) & set(dry["removed"].tolist())
        assert 0 < dry["n_removed"] < dry["n_local"]
    wet = c.map.cull_points(kfs, R.K, apply=True)
    assert np.array_equal(wet["removed"], want["removed"]) and bits(wet["xyz"]) == bits(want["xyz"])
    R.cull(model, kfs, R.K, oracle, apply=True)
    if c.P:
        c.same_as_rebuilt(kfs)
    again = c.map.cull_points(kfs, R.K, apply=True)        # nothing left above the threshold
    assert again["n_removed"] == 0 and again["n_local"] == len(want["local"]) - len(want["removed"])
    c.close()


def test_cull_points_special_sets(ctx, rs, oracle):
    c = Case(ctx, rs, (22, 4, 120, 300))
    model = c.model
    kfs = [1, 2, 3]
    local = R.cull_problem(model, kfs)["local"]
    counts0 = c.map.counts()
    none = c.map.cull_points(kfs, R.K, max_mean_error=1e9, apply=True)            # none culled
    assert none["n_removed"] == 0 and none["n_local"] == len(local) and c.map.counts() == counts0
    # the local set is empty: a key frame nothing observes
    f = rs.ResidentFrame(ctx, model.kf_kp[0][:5], model.kf_desc[0][:5])
    kf_new, _ = model.add_keyframe(model.kf_kp[0][:5], model.kf_desc[0][:5], R.pose_of(4))
    assert c.map.add_keyframe(f, model.kf_pose[kf_new]) == kf_new
    f.close()
    empty = c.map.cull_points([kf_new], R.K, max_mean_error=-1.0, apply=True)
    assert (empty["n_removed"], empty["n_local"]) == (0, 0)
    assert c.map.cull_points([], R.K, apply=True)["n_local"] == 0
    # capacity too small: the count is reported, the call is refused, the map is unchanged
    small = c.map.cull_points(kfs, R.K, max_mean_error=-1.0, apply=True, capacity=len(local) - 1, check=False)
    assert small["status"] == 1 and small["n_removed"] == len(local) and c.map.counts() == counts0 | dict(key_frames=5)
    with pytest.raises(rs.RsError):
        c.map.cull_points(kfs, R.K, max_mean_error=-1.0, apply=True, capacity=0)
    c.same_as_rebuilt(kfs)
    # all local points culled (every mean is > -1); points observed only outside the list stay, whatever their error
    outside = [p for p in model.alive_points() if p not in set(local.tolist())]
    assert any(model.obs[p] for p in outside)
    everything = c.map.cull_points(kfs, R.K, max_mean_error=-1.0, apply=True, capacity=len(local))
    assert np.array_equal(everything["removed"], local) and everything["n_local"] == len(local)
    want = R.cull(model, kfs, R.K, oracle, max_mean_error=-1.0, apply=True)
    assert np.array_equal(want["removed"], local) and bits(everything["xyz"]) == bits(want["xyz"])
    assert model.alive_points() == outside
    c.same_as_rebuilt(kfs)
    c.close()


def test_cull_threshold_is_strict(ctx, rs):
    """A one-observation point at (0, 0, 1) under the identity pose projects onto the principal point — put at the origin
    here, so that the pixel's distance from it IS the pixel's coordinate: at exactly 3 px the point is kept (:420 is >),
    at the next float above 3 px it is removed."""
    K0 = (500.0, 500.0, 0.0, 0.0)
    up = np.nextafter(np.float32(3.0), np.float32(4.0))
    kp = np.array([[3.0, 0.0], [up, 0.0], [0.0, -3.0], [0.0, -up]], np.float32)
    m = rs.ResidentMap(ctx)
    f = rs.ResidentFrame(ctx, kp, np.zeros((4, 32), np.uint8))
    kf = m.add_keyframe(f, np.eye(4, dtype=np.float32))
    f.close()
    for i in range(4):
        m.add_observation(m.add_point([0.0, 0.0, 1.0]), kf, i)
    r = m.cull_points([kf], K0, max_mean_error=3.0, apply=True)
    assert r["removed"].tolist() == [1, 3] and r["n_local"] == 4
    assert m.counts() == dict(slots=4, alive=2, observations=2, key_frames=1)
    m.close()


def test_long_observation_lists(ctx, rs, oracle):
    """40 key frames of 40 keypoints: points with up to 40 observations, summed in the CSR's insertion order"""
    c = Case(ctx, rs, (23, 40, 40, 60), max_obs=40, pose_scale=0.1)
    model = c.model
    assert max(len(o) for o in model.obs) == 40
    kfs = list(range(5, 40))
    want = R.cull(model, kfs, R.K, oracle, apply=False)
    assert R.cull_margin(want["mean_err"]) >= R.CULL_MARGIN and 0 < len(want["removed"]) < len(want["local"])
    got = c.map.cull_points(kfs, R.K, apply=True)
    assert np.array_equal(got["removed"], want["removed"]) and np.array_equal(got["removed"], flat_cull(ctx, model, kfs))
    R.cull(model, kfs, R.K, oracle, apply=True)
    before = c.move_poses(kfs, 9)
    n, slots, xyz = c.map.reanchor(kfs, before)
    pts, want_xyz = R.reanchor(model, kfs, before, oracle)
    assert np.array_equal(slots, pts) and bits(xyz) == bits(want_xyz)
    c.same_as_rebuilt(kfs[:6])
    c.close()


# ------------------------------------------------------------------------------------------ the two host halves
def test_insert_keyframe_adopts_the_frames_table(ctx, rs):
    c = Case(ctx, rs, (24, 4, 150, 257))
    model = c.model
    rng = np.random.default_rng(24)
    n_kp = c.frame.n
    live = [p for p in model.alive_points()]
    kps = rng.permutation(n_kp)[:60]
    pts = rng.choice(live, 60, replace=False)
    gone = [int(p) for p in pts[:6]]
    pts = np.r_[pts[:58], 257 + 5, 257 + 900]               # two slots the map never had
    c.frame.matches_add(ctx.dev(kps.astype(np.int32)), ctx.dev(pts.astype(np.int32)))
    for p in gone:                                          # removed after the tracker matched them: stale entries
        c.replay(model.remove_point(p))
    table, cnt = c.frame.matches()
    assert cnt == 60
    kf, _ = model.add_keyframe(c.fr["keypoints"], c.fr["descriptors"], c.fpose)
    kf_got, adopted = c.map.insert_keyframe(c.frame, c.fpose)
    calls = []
    assert kf_got == kf and adopted == R.adopt(model, kf, table, calls) == 52
    # the map built by the per-match calls in the same order
    ref = map_of(ctx, rs, R.build_model(c.scene))
    for p in gone:
        ref.remove_point(p)
    assert ref.add_keyframe(c.frame, c.fpose) == kf
    replay_on(ref)(calls)
    kfs = [1, 2, 3, kf]
    free = np.array([0, 1, 1, 1], np.uint8)
    assert c.map.counts() == ref.counts() == model.counts()
    a, b = c.map.window(kfs, free), ref.window(kfs, free)
    assert all(np.array_equal(a[k], b[k]) for k in a) and len(a["points"]) > 10
    assert c.match(required=kf) == c.match(ref, required=kf) and len(c.match(required=kf)[0]) > 0
    ref.close()
    c.same_as_rebuilt(kfs)
    c.close()


def test_add_track_points_creates_and_associates(ctx, rs):
    c = Case(ctx, rs, (25, 5, 200, 257))
    model = c.model
    rng = np.random.default_rng(25)
    kf, window = 4, [0, 2, 3, 4]                            # key frame 1 is outside the window
    res = R.random_results(model, kf, rng)
    counts0 = c.map.counts()
    with pytest.raises(rs.RsError):                         # n_pairs > capacity_pairs: the pairs are incomplete
        c.map.add_track_points(kf, res, window, capacity_pairs=res["n_pairs"] - 1)
    with pytest.raises(rs.RsError):                         # a window key frame the map does not have
        c.map.add_track_points(kf, res, [0, 2, 9], None)
    assert c.map.counts() == counts0
    ref = map_of(ctx, rs, model)
    calls = []
    skipped = {}
    want_slots, _ = R.add_track_points(model, kf, res, window, calls, skipped)
    assert min(skipped.values()) > 0 and len(skipped) == 5, skipped     # every skip rule of :316-321 is exercised
    got = c.map.add_track_points(kf, res, window)
    assert got.tolist() == want_slots
    replay_on(ref)(calls)                                   # rs_map_add_point / rs_map_add_observation, one by one
    kfs = [1, 0, 2, 3, 4]
    free = np.array([0, 1, 1, 1, 1], np.uint8)
    assert c.map.counts() == ref.counts() == model.counts() and c.map.counts()["slots"] == 257 + 25
    a, b = c.map.window(kfs, free), ref.window(kfs, free)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert c.match(required=kf) == c.match(ref, required=kf)
    ref.close()
    c.same_as_rebuilt(kfs)
    c.close()


# ------------------------------------------------------------------------------------------ the chain
def test_the_calls_in_mapper_insert_order(ctx, rs, oracle):
    """insert -> add_track_points -> bundle_adjust -> reanchor -> cull through the binding, against keyframe_ref fed with
    the poses and points rs_map_bundle_adjust returned (the solver's noise does not enter)."""
    c = Case(ctx, rs, (26, 4, 200, 400), extra=60, bad_frac=0.1)        # 60 keypoints without a map match: room for the new tracks
    model = c.model
    rng = np.random.default_rng(26)
    table = np.full(c.frame.n, -1, np.int32)
    mk, mp = c.match()
    c.frame.matches_add(ctx.dev(np.array(mk, np.int32)), ctx.dev(np.array(mp, np.int32)))
    table[mk] = mp
    assert len(mk) > 20
    kf, _ = model.add_keyframe(c.fr["keypoints"], c.fr["descriptors"], c.fpose)
    assert c.map.insert_keyframe(c.frame, c.fpose) == (kf, R.adopt(model, kf, table))
    window = [1, 2, 3]
    res = R.random_results(model, kf, rng, n_acc=15)
    assert c.map.add_track_points(kf, res, window).tolist() == R.add_track_points(model, kf, res, window)[0]
    kfs, free = np.array(window + [kf], np.int32), np.array([0, 1, 1, 1], np.uint8)
    opt = [int(k) for k, f in zip(kfs, free) if f]
    before = np.stack([model.kf_pose[k] for k in opt])
    s, poses, ba_pts, ba_xyz = c.map.bundle_adjust(kfs, free, R.K)
    assert s["usable"] == 1 and len(ba_pts) > 50
    for k, T in zip(kfs, poses):                            # the model takes the solve
        model.set_pose(int(k), T)
    for p, x in zip(ba_pts, ba_xyz):
        model.set_position(int(p), x)
    n, slots, xyz = c.map.reanchor(opt, before)
    want_slots, want_xyz = R.reanchor(model, opt, before, oracle)
    assert n == len(want_slots) > 10 and np.array_equal(slots, want_slots) and bits(xyz) == bits(want_xyz)
    want = R.cull(model, kfs, R.K, oracle, apply=True)
    assert R.cull_margin(want["mean_err"]) >= R.CULL_MARGIN
    got = c.map.cull_points(kfs, R.K, apply=True)
    assert np.array_equal(got["removed"], want["removed"]) and bits(got["xyz"]) == bits(want["xyz"]) and got["n_removed"] > 0
    c.same_as_rebuilt(kfs)
    c.close()


# ------------------------------------------------------------------------------------------ growth
GROW_KP = 64                            # keypoints per key frame of the growing map
# (key frames, point slots) after each step, and what the step outgrows of what the uses before it allocated.  First
# capacities (csrc/map.hip): 1024 entries for the centres [KF][3], the poses [KF][16], d_win [2 P + 2], d_out
# [2 P + 4 N + 1], d_kp_point [rows] and the two pools (32 bytes, 2 floats a row); 4096 point slots; 16384 observations.
# Crossed elsewhere on a live map: 4096 slots (test_gpu_track.py), the pools with kept rows and d_kp_point
# (test_gpu_resident_map_edits.py, test_gpu_loop_envelope.py), the two 4096-entry tables of the context
# (test_gpu_match_envelope.py's two reuse tests).  Crossed only here: the 65th pose, the 342nd centre, d_win and d_out past
# 1024 after a use, 16384 observations, and the second doubling of the slots; the fuse scratch in test_gpu_fuse.py.
GROW_STEPS = [(64, 700),                # the poses fill their 1024 floats and d_kp_point its 4096 rows exactly
              (65, 700),                # the 65th pose; 4160 rows in d_kp_point; both pools, which keep their rows
              (65, 1100),               # d_win (2202 words after 2048) and d_out
              (342, 1100),              # the 342nd centre; the pools and d_kp_point again
              (342, 4096),              # 4096 slots and 16384 observations: both fit exactly, d_win grows
              (342, 4097),              # the 4097th slot: the seven per-point arrays; its observations: the two per-observation arrays
              (342, 8193),              # the slots double again (d_obs_ptr, one entry longer than the rest, must double with them) ...
              (342, 8194)]              # ... and the next slot fits every one of the seven


def growing_scene(seed=31):
    """342 key frames and 8194 points laid out so that the map can be built in GROW_STEPS' order: a point's observers are
    the least-filled key frames among those its step already has.  Slots below 1100 have 1 - 3 observers (the single ones
    are what rs_map_reanchor moves); the later ones 5, then 4, so that slot 4095 brings the count to 16384 exactly; from
    slot 4097 on one."""
    rng = np.random.default_rng(seed)
    n_kf, P = GROW_STEPS[-1]
    poses = [R.pose_of(0.02 * k) for k in range(n_kf)]
    pts = np.c_[rng.uniform(-2, 2, P), rng.uniform(-1.5, 1.5, P), rng.uniform(4, 8, P)].astype(np.float32)
    kf_kp = [[] for _ in range(n_kf)]
    fill = np.zeros(n_kf, np.int64)
    obs = [[] for _ in range(P)]
    for p in range(P):
        have = next(kf for kf, slots in GROW_STEPS if p < slots)
        n = 1 + p % 3 if p < 1100 else (5 if p < 3301 else 4 if p < 4097 else 1)
        bad = rng.random() < 0.25
        sign = rng.choice([-1.0, 1.0], 2)
        for kf in sorted(np.argsort(fill[:have], kind="stable")[:n].tolist()):
            off = sign * rng.uniform(5.0, 12.0, 2) if bad else rng.normal(0, 0.4, 2)
            kf_kp[kf].append(R.project(poses[kf], pts[p]) + off)
            obs[p].append((kf, int(fill[kf])))
            fill[kf] += 1
    assert fill.max() <= GROW_KP and sum(len(o) for o in obs[:4096]) == 16384
    for kf in range(n_kf):
        while len(kf_kp[kf]) < GROW_KP:
            kf_kp[kf].append(rng.uniform((0, 0), (R.WIDTH, R.HEIGHT)))
    return dict(poses=poses, points=pts, obs=obs, kf_kp=[np.array(k, np.float32).reshape(-1, 2) for k in kf_kp],
                kf_desc=[rng.integers(0, 256, (GROW_KP, 32), dtype=np.uint8) for _ in range(n_kf)])


def test_every_buffer_of_the_map_is_outgrown_in_use(ctx, rs, oracle):
    """One map built in GROW_STEPS' order and used after every step, so that each grow-only buffer of the device image is
    reallocated while the map is live.  A use: counts, positions, two plain matches (the second equal to the first: the flag
    table came back all zero), a match by observer, match_frame's table (d_mark, the track-consistent flags), the BA window
    against the model's, a loop verification's gathered rows, slots and positions (the pools' old rows, d_kp_point) against
    the model, a dry cull and a re-anchor against the oracle; the matches and the window also against a map rebuilt from the
    model in one go, which never reallocates."""
    import types
    from loop_checks import _check
    from map_model import MapModel
    s = growing_scene()
    model, m = MapModel(), rs.ResidentMap(ctx)
    replay = replay_on(m)
    ver = ctx.loop_verifier(256, 2, 200)
    rng = np.random.default_rng(32)
    probe = None

    def match_frame_table(mm):
        f = rs.ResidentFrame(ctx, probe["keypoints"], probe["descriptors"])
        n = mm.match_frame(f, probe["pose"], R.K, R.WIDTH, R.HEIGHT)
        tab = f.matches()[0].tolist()
        f.close()
        return n, tab

    def use(step):
        n_kf = model.n_kf()
        assert m.counts() == model.counts() and bits(m.positions()) == bits(model.positions()), step
        ref = map_of(ctx, rs, model)
        f = rs.ResidentFrame(ctx, probe["keypoints"], probe["descriptors"])
        try:
            first = m.match(f, probe["pose"], R.K, R.WIDTH, R.HEIGHT)
            again = m.match(f, probe["pose"], R.K, R.WIDTH, R.HEIGHT)
            want = ref.match(f, probe["pose"], R.K, R.WIDTH, R.HEIGHT)
            assert len(first[0]) > 20 and all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(first, again, want)), step
            for kf in (0, n_kf - 1):
                got, want = (mm.match(f, probe["pose"], R.K, R.WIDTH, R.HEIGHT, required_observer=kf) for mm in (m, ref))
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), (step, kf)
            assert match_frame_table(m) == match_frame_table(ref), step
            kfs = np.array([0, 1, n_kf // 2, n_kf - 2, n_kf - 1], np.int32)
            free = np.array([0, 1, 1, 1, 1], np.uint8)
            a, b, w = m.window(kfs, free), ref.window(kfs, free), model.ba_window(kfs, free)
            assert all(np.array_equal(a[k], b[k]) for k in a) and len(a["points"]) > 10, step
            assert all(np.array_equal(a[k], w[k]) for k in ("points", "obs_ptr", "obs_cam")) and a["obs_uv"].tobytes() == w["obs_uv"].tobytes(), step
        finally:
            f.close()
            ref.close()
        # the loop view: the oldest and the newest key frame's rows gathered for a query in the middle
        key_frames = [dict(kp=model.kf_kp[k], desc=model.kf_desc[k], pose=model.kf_pose[k].reshape(4, 4)) for k in range(n_kf)]
        b = types.SimpleNamespace(s=dict(key_frames=key_frames, query=n_kf // 2, width=R.WIDTH), map=m, pos=model.positions(),
                                  kp_point=[np.asarray(t, np.int32) for t in model.kp_point])
        cands = [0, n_kf - 1]
        _check(ver, b, cands, ver.verify(m, n_kf // 2, cands, R.K, R.WIDTH))
        assert ver.download(0)["nt"] > 0, step
        # a dry cull, then a re-anchor after a small move of the listed poses (the image's poses and centres follow)
        kfs = [int(k) for k in kfs[1:]]
        want = R.cull(model, kfs, R.K, oracle, apply=False)
        assert R.cull_margin(want["mean_err"]) >= R.CULL_MARGIN and 0 < len(want["removed"]) < len(want["local"]), step
        got = m.cull_points(kfs, R.K, apply=False)
        assert np.array_equal(got["removed"], want["removed"]) and bits(got["xyz"]) == bits(want["xyz"]), step
        before = np.stack([model.kf_pose[k] for k in kfs]).astype(np.float32)
        for k in kfs:
            replay(model.set_pose(k, R.perturb_pose(model.kf_pose[k], rng, angle=2e-4, step=5e-4)))
        n, slots, xyz = m.reanchor(kfs, before)
        want_slots, want_xyz = R.reanchor(model, kfs, before, oracle)
        assert n == len(want_slots) > 0 and np.array_equal(slots, want_slots) and bits(xyz) == bits(want_xyz), step
        assert bits(m.positions()) == bits(model.positions()), step

    try:
        for step, (n_kf, P) in enumerate(GROW_STEPS):
            for k in range(model.n_kf(), n_kf):
                model.add_keyframe(s["kf_kp"][k], s["kf_desc"][k], s["poses"][k])
                f = rs.ResidentFrame(ctx, s["kf_kp"][k], s["kf_desc"][k])
                assert m.add_keyframe(f, model.kf_pose[k]) == k
                f.close()
            for p in range(model.n_slots(), P):
                replay(model.create_point(s["points"][p], s["obs"][p])[1])
            if probe is None:
                probe = R.match_frame_of(model, 31, at=0.02 * n_kf)
            use(step)
        assert model.counts()["observations"] > 16384 and model.consistent()
        # the cull applied on the grown map, and a last use of what is left
        kfs = list(range(300, 342))
        want = R.cull(model, kfs, R.K, oracle, apply=True)
        assert R.cull_margin(want["mean_err"]) >= R.CULL_MARGIN and len(want["removed"]) > 100
        got = m.cull_points(kfs, R.K, apply=True)
        assert np.array_equal(got["removed"], want["removed"]) and bits(got["xyz"]) == bits(want["xyz"])
        use("after the cull")
    finally:
        ver.close()
        m.close()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_map_usable(ctx, rs, oracle):
    c = Case(ctx, rs, (27, 4, 120, 256))
    model = c.model
    other = rs.Context(0)
    foreign = rs.ResidentFrame(other, model.kf_kp[0], model.kf_desc[0])
    counts0 = c.map.counts()
    I4 = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (4, 1))
    lib, h = ctx.lib, c.map.h
    import ctypes as C
    n = C.c_int(-5)
    kfs = (C.c_int32 * 2)(1, 2)
    Kc = (C.c_float * 4)(*R.K)
    refused = [
        lambda: c.map.reanchor([1, 4], I4[:2]),                                   # unknown key frame
        lambda: c.map.reanchor([1, 2, 1], I4[:3]),                                # repeated key frame
        lambda: c.map.reanchor([-1], I4[:1]),
        lambda: c.map.cull_points([0, 7], R.K),
        lambda: c.map.cull_points([2, 2], R.K),
        lambda: c.map.insert_keyframe(foreign, c.fpose),                          # a frame of another context
        lambda: c.map.add_track_points(9, R.random_results(model, 3, np.random.default_rng(1), n_acc=5), [1, 2]),
    ]
    for call in refused:
        with pytest.raises(rs.RsError):
            call()
        assert c.map.counts() == counts0
    # a foreign context, and null outputs, through the raw ABI: RS_ERR_INVALID (1)
    assert lib.rs_map_reanchor(other.h, h, kfs, I4.ctypes.data_as(C.c_void_p), 2, None, None, 0, C.byref(n)) == 1
    assert lib.rs_map_cull_points(other.h, h, kfs, 2, Kc, C.c_float(3.0), 0, None, None, 0, C.byref(n), None) == 1
    assert lib.rs_map_reanchor(ctx.h, h, kfs, I4.ctypes.data_as(C.c_void_p), 2, None, None, 0, None) == 1
    assert lib.rs_map_cull_points(ctx.h, h, kfs, 2, Kc, C.c_float(3.0), 0, None, None, 0, None, None) == 1
    assert lib.rs_map_cull_points(ctx.h, h, kfs, 2, Kc, C.c_float(3.0), 0, None, None, 5, C.byref(n), None) == 1     # room announced, no array
    assert lib.rs_map_insert_keyframe(ctx.h, h, c.frame.h, c.fpose.ctypes.data_as(C.c_void_p), None, C.byref(n)) == 1
    assert lib.rs_map_add_track_points(h, 1, None, kfs, 2, None) == 1
    assert c.map.counts() == counts0
    foreign.close()
    other.close()
    # null output arrays with capacity 0 are a count query; the map works as before
    assert lib.rs_map_reanchor(ctx.h, h, kfs, I4.ctypes.data_as(C.c_void_p), 2, None, None, 0, C.byref(n)) == 0
    assert n.value == len(R.reanchor_lists(model, [1, 2])[0])
    R.reanchor(model, [1, 2], I4[:2], oracle)               # (the count query above did move the points)
    want = R.cull(model, [1, 2, 3], R.K, oracle, apply=True)
    assert R.cull_margin(want["mean_err"]) >= R.CULL_MARGIN and 0 < len(want["removed"]) < len(want["local"])
    got = c.map.cull_points([1, 2, 3], R.K, apply=True)
    assert np.array_equal(got["removed"], want["removed"])
    c.same_as_rebuilt([1, 2, 3])
    c.close()
