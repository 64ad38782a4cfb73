"""The kernels whose hand-off-independent work was moved (K8's held Jacobians, K5's operand prefetch from every state
buffer, K6's table of projection rows) at the smallest shapes at which that code takes another path.

Bundle adjustment: every case against pyoracle.bundle_adjust with the contract of bench.py's check_pass_parity —
identical (iterations, successful_steps, termination, usable), final cost to 1e-7 relative, cameras rtol 1e-6 / atol
1e-8, points rtol 1e-6 / atol 1e-7 — as the fused launch (ba_fuse_mode 2) and as separate launches (ba_fuse_mode 1),
and the two forms against each other at the same tolerances.

Track stage: status, xyz bits, parallax bits, the requirement (host table), accepted, inconsistent and the counts
bit for bit against pyoracle.triangulate_tracks."""
import numpy as np
import pytest

from conftest import to_np

pytestmark = pytest.mark.gpu

SCHEDULE = ("iterations", "successful_steps", "termination", "usable")


# ------------------------------------------------------------------------------------------ bundle adjustment
def _from_camera_zero(w):
    """The landmarks of window w whose run starts at camera 0: with two fixed cameras every one of them has
    observations of fixed cameras in its first rounds, and those of run length 3 are seen by the two fixed cameras
    and ONE free camera."""
    keep = np.flatnonzero(w["run_start"] == 0)
    ptr = w["obs_ptr"]
    sel = np.concatenate([np.arange(ptr[p], ptr[p + 1]) for p in keep])
    out = dict(w)
    out["points"] = w["points"][keep]
    out["obs_cam"], out["obs_uv"] = w["obs_cam"][sel], w["obs_uv"][sel]
    out["obs_ptr"] = np.concatenate([[0], np.cumsum(w["run_len"][keep])]).astype(np.int32)
    out["run_len"], out["run_start"] = w["run_len"][keep], w["run_start"][keep]
    return out


# name -> (make_ba_window arguments, landmark filter, ba_speculative_sets (0 = the library's default))
BA_CASES = {
    "few_obs_300": (dict(n_kf=6, n_points=300, run_max=6), None, 0),                  # every observation held; 300 % 64, 300 % 128 != 0
    "few_obs_129": (dict(n_kf=6, n_points=129, run_max=6), None, 0),                  # one landmark in the last block
    "more_than_12_obs": (dict(n_kf=20, n_points=200, run_min=13, run_max=20), None, 0),   # held rounds + the on-demand path
    "fixed_cameras": (dict(n_kf=6, n_points=900, run_max=6, n_fixed=2), _from_camera_zero, 0),
    "sets_1": (dict(n_kf=20, n_points=1000), None, 1),
    "sets_3": (dict(n_kf=20, n_points=1000), None, 3),
    "sets_5": (dict(n_kf=20, n_points=1000), None, 5),                               # second pass of a K8 workgroup; every state buffer
    "large_11000": (dict(n_kf=20, n_points=11000), None, 0),                          # fewer sets resident: the pass > 1 reload
}
_BA = {}


def _ba_case(synth, oracle, name):
    """(window, oracle cameras, oracle points, oracle summary): built once per session, never written to."""
    if name not in _BA:
        kw, filt, _ = BA_CASES[name]
        w = synth.make_ba_window(**kw)
        if filt:
            w = filt(w)
        rc, rp, rsum = oracle.bundle_adjust(w["cams"], w["cam_free"], w["points"], w["obs_ptr"], w["obs_cam"], w["obs_uv"], w["K"])
        _BA[name] = (w, rc, rp, rsum)
    return _BA[name]


def _solve(ctx, w, fuse_mode, sets):
    dc, dp = ctx.dev(w["cams"]), ctx.dev(w["points"])
    try:
        ctx.set_int("ba_fuse_mode", fuse_mode)
        ctx.set_int("ba_speculative_sets", sets)
        s = ctx.bundle_adjust(dc, w["cam_free"], dp, ctx.dev(w["obs_ptr"]), ctx.dev(w["obs_cam"]), ctx.dev(w["obs_uv"]), w["K"])
    finally:
        ctx.set_int("ba_fuse_mode", 0)
        ctx.set_int("ba_speculative_sets", 0)
    return to_np(dc), to_np(dp), s


def _same_solve(tag, got, ref):
    (gc, gp, gs), (rc, rp, rs_) = got, ref
    rel = abs(gs["final_cost"] - rs_["final_cost"]) / max(abs(rs_["final_cost"]), 1e-300)
    print(tag, [gs[k] for k in SCHEDULE], [rs_[k] for k in SCHEDULE], "cost rel", rel, "cams", float(np.abs(gc - rc).max()),
          "points", float(np.abs(gp - rp).max()))
    assert tuple(gs[k] for k in SCHEDULE) == tuple(rs_[k] for k in SCHEDULE), tag
    assert rel <= 1e-7, tag
    assert np.allclose(gc, rc, rtol=1e-6, atol=1e-8), tag
    assert np.allclose(gp, rp, rtol=1e-6, atol=1e-7), tag


@pytest.mark.parametrize("name", list(BA_CASES))
def test_ba_against_the_oracle_fused_and_separate(ctx, synth, oracle, name):
    w, rc, rp, rsum = _ba_case(synth, oracle, name)
    assert rsum["usable"] == 1
    if name == "fixed_cameras":
        assert (w["run_len"] == 3).any() and (w["obs_cam"] < 2).any()
    if name == "more_than_12_obs":
        assert int(np.diff(w["obs_ptr"]).min()) > 12
    sets = BA_CASES[name][2]
    fused = _solve(ctx, w, 2, sets)
    separate = _solve(ctx, w, 1, sets)
    _same_solve(name + " fused vs oracle", fused, (rc, rp, rsum))
    _same_solve(name + " separate vs oracle", separate, (rc, rp, rsum))
    _same_solve(name + " fused vs separate", fused, separate)


# ------------------------------------------------------------------------------------------------- track stage
K = np.array([1000.0, 1000.0, 960.0, 540.0], np.float32)
K6_TABLE_POSES = 512          # csrc/tracks.hip


def _trajectory(n):
    """n world -> camera poses of a forward-moving, gently turning camera, 2.4 m and 12 degrees in all."""
    poses = np.zeros((n, 16), np.float32)
    for f in range(n):
        a = f / max(n - 1, 1)
        yaw = np.deg2rad(12.0 * a)
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        c = np.array([0.6 * a, 0.0, 2.4 * a])
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = -R @ c
        poses[f] = T.astype(np.float32).reshape(16)
    return poses


def _tracks(frames_per_track, poses, kf, seed, bad=None, skip=None):
    """Tracks sighted in the listed frames (any order of poses) and in key frame kf.  bad: {track: position of the sighting
    that is moved by 10 .. 30 px}."""
    rng = np.random.default_rng(seed)
    n = len(frames_per_track)
    Tk = poses[kf].reshape(4, 4).astype(np.float64)
    depth = rng.uniform(5, 25, n)
    u, v = rng.uniform(300, 1620, n), rng.uniform(200, 880, n)
    Xc = np.stack([(u - K[2]) / K[0] * depth, (v - K[3]) / K[1] * depth, depth], 1)
    Xw = (Xc - Tk[:3, 3]) @ Tk[:3, :3]

    def pix(T, X):
        pc = T[:3, :3] @ X + T[:3, 3]
        return np.array([K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]])

    ptr, sp, suv = [0], [], []
    track_uv = np.zeros((n, 2), np.float32)
    for t, frames in enumerate(frames_per_track):
        for j, f in enumerate(frames):
            px = pix(poses[f].reshape(4, 4).astype(np.float64), Xw[t]) + rng.normal(0, 0.3, 2)
            if bad and bad.get(t) == j:
                px += rng.uniform(10, 30, 2) * rng.choice([-1, 1], 2)
            sp.append(f)
            suv.append(px)
        track_uv[t] = pix(Tk, Xw[t]) + rng.normal(0, 0.3, 2)
        ptr.append(len(sp))
    return dict(track_uv=track_uv, sight_ptr=np.array(ptr, np.int32), sight_pose=np.array(sp, np.int32).reshape(-1),
                sight_uv=np.array(suv, np.float32).reshape(-1, 2), poses=poses, kf_pose=kf,
                skip=np.zeros(n, np.uint8) if skip is None else np.asarray(skip, np.uint8))


def _check_tracks(ctx, rs, oracle, sc, quota=5):
    n = len(sc["track_uv"])
    ref = oracle.triangulate_tracks(sc["track_uv"], sc["sight_ptr"], sc["sight_pose"], sc["sight_uv"], sc["poses"], sc["kf_pose"], K,
                                    skip=sc["skip"], min_new_points=quota)
    req = rs.parallax_requirements(sc["poses"], sc["kf_pose"])
    got = ctx.triangulate_tracks(ctx.dev(sc["track_uv"]), ctx.dev(sc["sight_ptr"]), ctx.dev(sc["sight_pose"]), ctx.dev(sc["sight_uv"]),
                                 ctx.dev(sc["poses"]), sc["kf_pose"], K, d_skip=ctx.dev(sc["skip"]), min_new_points=quota,
                                 d_required=ctx.dev(req))
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)       # noqa: E731
    assert np.array_equal(to_np(got["status"])[:n], ref["status"])
    assert np.array_equal(bits(to_np(got["xyz"])[:n]), bits(ref["xyz"]))
    assert np.array_equal(bits(to_np(got["parallax_cos"])[:n]), bits(ref["parallax_cos"]))
    assert np.array_equal(bits(to_np(got["required_cos"])[:n]), bits(ref["required_cos"]))
    cnt = to_np(got["counts"])
    assert (int(cnt[0]), int(cnt[1]), int(cnt[2])) == (len(ref["accepted"]), ref["n_topped_up"], len(ref["inconsistent"]))
    assert np.array_equal(to_np(got["accepted"])[:cnt[0]], ref["accepted"])
    assert np.array_equal(to_np(got["inconsistent"])[:cnt[2]], ref["inconsistent"])
    return ref


@pytest.mark.parametrize("n_tracks", [1, 63, 64, 65, 130])
def test_tracks_block_edges_and_skip_flags(ctx, rs, oracle, n_tracks):
    poses = _trajectory(12)
    counts = [2 + (3 * t) % 9 for t in range(n_tracks)]
    skip = [1 if t % 7 == 3 else 0 for t in range(n_tracks)]
    sc = _tracks([list(range(11 - c, 11)) for c in counts], poses, 11, 100 + n_tracks, bad={t: 1 for t in range(2, n_tracks, 11)}, skip=skip)
    ref = _check_tracks(ctx, rs, oracle, sc)
    if n_tracks > 1:
        assert (ref["status"][np.asarray(skip) == 1] == 0).all() and (ref["status"] == 1).any()


def test_tracks_sighting_counts_and_the_failing_sighting(ctx, rs, oracle):
    """0, 1, 4, 5, 9 and 100 sightings (batches of four: none, a part, exactly one, one and a part, two and a part,
    25), and tracks of 9 sightings made inconsistent by the first, a middle and the last of them (the first sighting
    is also the one the point is triangulated from)."""
    poses = _trajectory(101)
    frames = [list(range(100 - c, 100)) for c in (0, 1, 4, 5, 9, 100)] * 3
    base = len(frames)
    frames += [list(range(91, 100))] * 6
    bad = {base + 0: 0, base + 1: 4, base + 2: 8, base + 3: 3, base + 4: 7}
    sc = _tracks(frames, poses, 100, 7, bad=bad)
    ref = _check_tracks(ctx, rs, oracle, sc)
    st = ref["status"]
    assert (st[0:base:6] == 0).all()                                  # no sighting: no candidate
    assert (st[[base + 1, base + 2, base + 3, base + 4]] == 2).all() and st[base + 5] == 1
    assert st[base + 0] != 1                                          # (moving the first sighting moves the point)
    assert (st[:base] == 1).sum() >= 10


@pytest.mark.parametrize("n_poses", [1, 2, K6_TABLE_POSES, K6_TABLE_POSES + 1])
def test_tracks_pose_table_sizes(ctx, rs, oracle, n_poses):
    """One pose (every sighting in the key frame's own pose), two, as many as the table holds, and one more (the
    kernel gathers the poses as before)."""
    poses = _trajectory(n_poses)
    kf = n_poses - 1
    if n_poses <= 2:
        frames = [[0] * (1 + t % 5) for t in range(70)]
    else:
        # sightings over the whole pose array, the first and the last table rows included
        frames = [sorted({0, (37 * t) % kf, (91 * t + 5) % kf, kf - 1 - t % 3, kf - 1}) for t in range(70)]
    sc = _tracks(frames, poses, kf, 1000 + n_poses, bad={t: 1 for t in range(4, 70, 9)})
    ref = _check_tracks(ctx, rs, oracle, sc)
    if n_poses > 2:
        assert (ref["status"] == 1).any() and (ref["status"] == 2).any()
