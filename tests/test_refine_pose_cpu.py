"""refine_pose and its RotationPrior / InertialDelta forms: the oracle (oracle/ba.c, jets + normal equations) against the
independent dense restatement (tests/dense_lm.py: complex-step Jacobians, dense f64) over the cases of
tests/refine_cases.py, which tests/test_gpu_refine_pose.py then holds the GPU to.  Also pins the scene generator."""

import numpy as np
import pytest

import dense_lm as D
import refine_cases as RC

SCHEDULE = ("termination", "iterations", "successful_steps", "usable")
DENSE_CASES = [k for k, c in RC.CASES.items() if RC.dense_ok(c)]



@pytest.mark.parametrize("name", DENSE_CASES)
def test_oracle_refine_pose_matches_dense_lm(name, oracle, synth):
    case = RC.CASES[name]
    p = RC.problem(synth, case)
    cam, vel, s = RC.solve_oracle(oracle, p, case)
    dcam, dvel, ds = RC.solve_dense(D, oracle, p, case)
    assert tuple(s[k] for k in SCHEDULE) == tuple(ds[k] for k in SCHEDULE)
    if "expect" in case:
        assert s["termination"] == case["expect"]
    if case.get("moved"):
        assert s["successful_steps"] >= 1 and s["usable"] == 0
    assert np.allclose(cam, dcam, rtol=1e-8, atol=1e-10)
    if vel is not None:
        assert np.allclose(vel, dvel, rtol=1e-8, atol=1e-10)
    if np.isfinite(s["initial_cost"]):
        assert np.isclose(s["initial_cost"], ds["initial_cost"], rtol=1e-9)
        assert np.isclose(s["final_cost"], ds["final_cost"], rtol=1e-9)
        assert np.isclose(s["final_radius"], ds["final_radius"], rtol=1e-12)
    else:
        assert not np.isfinite(ds["initial_cost"])
    if not s["usable"]:
        assert np.array_equal(cam, p["cam0"])
        if vel is not None:
            assert np.array_equal(vel, p["delta"]["velocity"])


@pytest.mark.parametrize("name", [k for k, c in RC.CASES.items() if not RC.dense_ok(c)])
def test_large_cases_reach_their_schedule(name, oracle, synth):
    """The cases too large for dense_lm: the oracle converges and its result is one of the dense-checked solves'."""
    case = RC.CASES[name]
    p = RC.problem(synth, case)
    cam, _, s = RC.solve_oracle(oracle, p, case)
    assert s["usable"] == 1 and s["termination"] in (RC.FUNCTION, RC.PARAMETER, RC.GRADIENT)
    assert np.abs(cam - p["cam_true"]).max() < 1e-2


def test_zero_depth_point_really_is_at_depth_zero(oracle, synth):
    p = RC.problem(synth, RC.CASES["zero_depth"])
    k = p["poke_index"]
    with np.errstate(all="ignore"):
        r, _, _ = oracle.reprojection(p["cam0"], p["points"][k], p["uv"][k], p["K"])
    assert not np.all(np.isfinite(r))
    assert p["points"][k, 2] - p["cam0"][5] == 0.0


def test_make_refine_problem(synth):
    p = synth.make_refine_problem(n=500, seed=4, outlier_frac=0.2, noise_px=0.0, bad_depth_frac=0.1)
    q = synth.make_refine_problem(n=500, seed=4, outlier_frac=0.2, noise_px=0.0, bad_depth_frac=0.1)
    for k in ("cam0", "points", "uv", "K", "cam_true", "outlier", "bad_depth"):
        assert np.array_equal(p[k], q[k]), k
    assert p["points"].dtype == np.float64 and p["points"].shape == (500, 3)
    assert p["uv"].dtype == np.float32 and p["uv"].shape == (500, 2) and p["K"].dtype == np.float32
    assert p["delta"] is None
    assert not np.any(p["outlier"] & p["bad_depth"])
    assert 0.1 < p["outlier"].mean() < 0.3 and 0.04 < p["bad_depth"].mean() < 0.16
    # depths in the true camera: bad points near / behind the image plane, the others in front
    R = synth.rodrigues(p["cam_true"][:3])
    z = ((p["points"] - p["cam_true"][3:]) @ R.T)[:, 2]
    assert np.all(z[~p["bad_depth"]] >= 2.0) and np.all(z[p["bad_depth"]] <= 0.05)
    assert np.any(np.abs(z[p["bad_depth"]]) <= 1e-4) and np.any(z[p["bad_depth"]] < 0)
    # noise-free inliers project onto their observation (f32 rounding), outliers are 20..120 px off
    K = p["K"].astype(np.float64)
    Q = (p["points"] - p["cam_true"][3:]) @ R.T
    with np.errstate(all="ignore"):
        e = np.hypot(K[0] * Q[:, 0] / Q[:, 2] + K[2] - p["uv"][:, 0], K[1] * Q[:, 1] / Q[:, 2] + K[3] - p["uv"][:, 1])
    good = ~p["outlier"] & ~p["bad_depth"]
    assert e[good].max() < 1e-3
    assert e[p["outlier"]].min() > 19.9 and e[p["outlier"]].max() < 120.1
    # the starting rotation is used bit for bit; the start is off the truth by rot_err / trans_err
    for rot0 in ([0.0, 0.0, 0.0], [1e-9, 0.0, 0.0], [0.0, 2e-8, 0.0], [0.0, 0.0, np.pi - 1e-3]):
        r = synth.make_refine_problem(n=10, rot0=rot0, rot_err=0.02, trans_err=0.05, offset=1e3)
        assert np.array_equal(r["cam0"][:3], np.asarray(rot0))
        assert abs(np.linalg.norm(r["cam0"][3:] - r["cam_true"][3:]) - 0.05) < 1e-9
        assert abs(np.linalg.norm(r["cam_true"][3:]) - 1e3) < 1e-9
        dR = synth.rodrigues(r["cam_true"][:3]) @ synth.rodrigues(np.asarray(rot0)).T
        assert abs(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)) - 0.02) < 1e-6
    # the one-factor InertialDelta: consistent with the true pair up to the synthetic noise
    d = synth.make_refine_problem(n=10, imu=True, seed=2)["delta"]
    assert len(d["imu"]["cam_i"]) == 1 and d["imu"]["cam_i"][0] == 0 and d["imu"]["cam_j"][0] == 1
    assert d["imu"]["duration"][0] > 0 and d["prev_pose"].shape == (6,) and d["velocity"].shape == (3,)
