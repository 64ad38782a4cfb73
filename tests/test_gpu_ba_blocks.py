"""What the per-call blocks of the bundle-adjustment driver and of refine_pose carry (csrc/ba_blocks.h), at the sizes where
their layout changes: the windows of tests/ba_block_cases.py (which tests/test_ba_blocks_cpu.py pins on the oracle), the
smallest inertial window under both inertial solves, a grid batch of three different windows, refine_pose plain and in its
two inertial kinds, and the two-piece workspaces of rs_reanchor_points_host_poses and rs_track_features.  Every solve is
held to the oracle by the contract of tests/ba_compare.py (refine_pose: by test_gpu_refine_pose.assert_matches); on top of
that the record has exactly `iterations` entries with the oracle's outcomes, and the camera mirror in pinned memory equals
d_cameras read back.  Every case is carried by the oracle; none needs another reference."""
import numpy as np
import pytest

import ba_block_cases as BB
import ba_cases as B
import ba_compare as CMP
import inertial_cases as IC
import klt_ref as K
import refine_cases as RC
import test_gpu_klt_envelope as KE
import test_gpu_refine_pose as RP
import tri_cases as TC
from conftest import to_np

pytestmark = pytest.mark.gpu


def _device(ctx, w):
    dc, dp = ctx.dev(w["cams"]), ctx.dev(w["points"])
    return dc, dp, (dc, w["cam_free"], dp, ctx.dev(w["obs_ptr"]), ctx.dev(w["obs_cam"]), ctx.dev(w["obs_uv"]), w["K"])


def _assert_record_and_mirror(ctx, g, ref_trace):
    """rs_ba_get_trace: exactly `iterations` entries, the oracle's outcomes; rs_ba_get_cameras: d_cameras as read back."""
    assert len(g["tr"]) == g["s"]["iterations"] == len(ref_trace)
    assert [t["outcome"] for t in g["tr"]] == [t["outcome"] for t in ref_trace]
    assert g["s"]["usable"] == 1
    mirror = ctx.ba_cameras(np.zeros_like(g["c"]))
    assert mirror.tobytes() == g["c"].tobytes()


@pytest.mark.parametrize("name", list(BB.SINGLE))
def test_single_window(ctx, rs, oracle, synth, name):
    kw, opt, expect = BB.SINGLE[name]
    w = synth.make_ba_window(**kw)
    rc, rp, rs_, rtr = B.solve_oracle(oracle, w, opt)
    dc, dp, args = _device(ctx, w)
    s = ctx.bundle_adjust(*args, options=B.options(rs, opt))
    ctx.synchronize()
    g = dict(s=s, tr=ctx.ba_trace(), c=to_np(dc), p=to_np(dp))
    print(name, B.outcomes(rtr), B.outcomes(g["tr"]), {k: s[k] for k in CMP.SCHEDULE}, rs_["final_cost"], s["final_cost"])
    if expect is not None:
        assert s["termination"] == expect
    CMP.assert_same_solve(g, (rc, rp, None, None, rs_, rtr))
    _assert_record_and_mirror(ctx, g, rtr)
    fixed = np.asarray(w["cam_free"]) == 0
    assert g["c"][fixed].tobytes() == w["cams"][fixed].tobytes()


@pytest.mark.parametrize("mode", [0, 1])
def test_inertial_window(ctx, rs, oracle, synth, mode):
    """The velocity | bias block of the pinned layout and the workspace tail behind the window, in both inertial solves."""
    case = IC.CASES[BB.INERTIAL]
    w = IC.window(synth, case)
    m = IC.imu(synth, w, case)
    ref = IC.solve_oracle(oracle, w, m, case)
    ctx.set_int("ba_imu_mode", mode)
    try:
        dc, dp, args = _device(ctx, w)
        s, v, b = ctx.bundle_adjust_inertial(*args, m, options=IC.options(rs, case))
    finally:
        ctx.set_int("ba_imu_mode", 0)
    ctx.synchronize()
    g = dict(s=s, tr=ctx.ba_trace(), c=to_np(dc), p=to_np(dp), v=v, b=b)
    print(mode, B.outcomes(ref[5]), B.outcomes(g["tr"]), {k: s[k] for k in CMP.SCHEDULE}, ref[4]["final_cost"], s["final_cost"])
    CMP.assert_same_solve(g, ref)
    _assert_record_and_mirror(ctx, g, ref[5])


def test_grid_batch_of_different_windows(ctx, rs, oracle, synth):
    """Per-window placement in the workspace and the pinned block, and the table of windows behind the pinned parts."""
    ws = [synth.make_ba_window(**kw) for kw in BB.BATCH]
    refs = [B.solve_oracle(oracle, w, {}) for w in ws]
    dev = [_device(ctx, w) for w in ws]
    ctx.prof_begin()
    try:
        out = ctx.bundle_adjust_batch([d[2] for d in dev])
    finally:
        prof = ctx.prof_end()
    ctx.synchronize()
    print([tuple(s[k] for k in CMP.SCHEDULE) for s in out], [tuple(r[2][k] for k in CMP.SCHEDULE) for r in refs], sorted(prof))
    assert "K7_ba_reduced_solve" in prof and int(prof["K0_ba_init"][0]) == 1           # the grid form ran, once for all windows
    for s, (dc, dp, _), w, ref in zip(out, dev, ws, refs):
        CMP.assert_same_summary(s, to_np(dc), to_np(dp), (ref[0], ref[1], ref[2]))
        assert s["usable"] == 1
        fixed = np.asarray(w["cam_free"]) == 0
        assert to_np(dc)[fixed].tobytes() == w["cams"][fixed].tobytes()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_refine_pose_kinds_at_20_points(ctx, rs, oracle, synth, kind):
    case = RC._c(dict(n=20, seed=70 + kind, imu=kind == 2), prior=(1e-3, 0.01) if kind == 1 else None, delta=kind == 2)
    p = RC.problem(synth, case)
    ref_cam, ref_vel, ref_s = RC.solve_oracle(oracle, p, case)
    cam, vel, s = RP.gpu_solve(ctx, rs, p, case)
    print(kind, s, ref_s)
    assert ref_s["usable"] == 1
    RP.assert_matches(s, ref_s, cam, ref_cam, vel, ref_vel)


@pytest.mark.parametrize("n_frames", [3, 33])
def test_reanchor_host_poses_at_10_points(ctx, oracle, n_frames):
    """3 key frames travel as kernel arguments; 33 is the smallest set that goes through the two-piece workspace."""
    c = TC.k13_case(n_frames, 10, False)
    ref = TC.oracle_reanchor(oracle, c)
    d_idx = None if c["point_idx"] is None else ctx.dev(c["point_idx"])
    pos = ctx.dev(c["positions"])
    ctx.reanchor_points_host_poses(d_idx, ctx.dev(c["frame_idx"]), c["before"], c["after"], pos)
    assert np.array_equal(to_np(pos).view(np.uint32), np.ascontiguousarray(ref, np.float32).view(np.uint32))


def test_track_features_at_50_points(ctx):
    a, b = KE._images(ctx, 21, 4)
    try:
        pts = KE._pair()["pts"][:50]
        ref = K.track_features(KE._pyr("img1", 21, 4), KE._pyr("img2", 21, 4), pts, win=21, max_level=4)
        assert ref["index"].size > 25
        KE._check_features(ctx, a, b, pts, ref)
    finally:
        a.close(); b.close()
