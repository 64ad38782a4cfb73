"""The oracle's inertial bundle adjustment (orc_bundle_adjust_inertial) across the case table of tests/inertial_cases.py,
pinned to the independent dense restatement (tests/dense_lm.py: complex-step Jacobians, no Schur complement) on every
case small enough for it, with the tolerances of test_golden.py::test_independent_dense_lm_reproduces_the_inertial_solves.
Also: the table keeps reaching what it was written for, the oracle does not depend on the order of the factors, and
synth.make_imu's knobs build factors that stay consistent with the ground truth."""
import numpy as np
import pytest

import dense_lm as D
import inertial_cases as IC

DENSE = [k for k, c in IC.CASES.items() if c.get("dense")]
EXPECT = [k for k, c in IC.CASES.items() if "expect" in c or c.get("moved")]


@pytest.mark.parametrize("name", DENSE)
def test_oracle_matches_dense_lm(oracle, synth, name):
    case = IC.CASES[name]
    w = IC.window(synth, case)
    m = IC.imu(synth, w, case)
    c, p, v, b, s, tr = IC.solve_oracle(oracle, w, m, case)
    dc, dv, db, ds, dtr, prob = IC.solve_dense(D, oracle, w, m, case)
    assert [s["termination"], s["iterations"], s["successful_steps"], s["usable"]] == \
           [ds["termination"], ds["iterations"], ds["successful_steps"], ds["usable"]]
    assert [t["outcome"] for t in tr] == [t["outcome"] for t in dtr]
    for k, tol in (("radius", 1e-8), ("cost", 1e-10), ("candidate_cost", 1e-9), ("model_cost_change", 1e-7)):
        assert np.allclose([t[k] for t in tr], [t[k] for t in dtr], rtol=tol), k
    if not s["usable"]:            # nothing moves: the inputs come back bit for bit
        assert np.array_equal(c, w["cams"]) and np.array_equal(p, w["points"])
        assert np.array_equal(v, m["cam_velocity"]) and np.array_equal(b, m["cam_bias"])
        return
    assert np.isclose(s["final_cost"], ds["final_cost"], rtol=1e-10)
    assert np.allclose(c, dc, rtol=1e-8, atol=1e-10)
    inert = prob.inert
    assert np.allclose(v[inert], dv[inert], rtol=1e-7, atol=1e-9)
    assert np.allclose(b[inert], db[inert], rtol=1e-6, atol=1e-9)
    # frames without an inertial block keep their velocity / bias
    other = np.setdiff1d(np.arange(len(w["cams"])), inert)
    assert np.array_equal(v[other], m["cam_velocity"][other]) and np.array_equal(b[other], m["cam_bias"][other])


def _gate_path0(w, m):
    """ba_solve_impl's choice for imu mode 0, restated: the local-window path needs 6 <= n = 6 Cf <= 126, 2 <= Ci <= 21
    and every factor joining consecutive inertial slots (slots in camera order of the frames the factors touch)."""
    Cf = int(np.count_nonzero(w["cam_free"]))
    inert = np.unique(np.concatenate([m["cam_i"], m["cam_j"]]))
    slot = {int(c): q for q, c in enumerate(inert)}
    ok = 6 <= 6 * Cf <= 126 and 2 <= len(inert) <= 21
    return "lds" if ok and all(slot[int(j)] == slot[int(i)] + 1 for i, j in zip(m["cam_i"], m["cam_j"])) else "big"


@pytest.mark.parametrize("name", list(IC.CASES))
def test_case_table_is_what_it_says(synth, name):
    """The path each case claims for imu mode 0 is the one the gate's rule gives; the Cf / Ci a case is named for hold."""
    case = IC.CASES[name]
    w = IC.window(synth, case)
    m = IC.imu(synth, w, case)
    if m is None:
        assert case["path0"] is None
        return
    assert case["path0"] == _gate_path0(w, m)
    assert len(m["cam_i"]) >= 1 and np.all(w["cam_free"][m["cam_i"]]) and np.all(w["cam_free"][m["cam_j"]])
    Cf, Ci = int(np.count_nonzero(w["cam_free"])), len(np.unique(np.concatenate([m["cam_i"], m["cam_j"]])))
    if name.startswith("chain_cf"):
        assert Cf == Ci == int(name[8:])
    if name.startswith("ci") and name[2].isdigit():
        assert Ci == int(name[2:].split("_")[0])
    for c in case.get("fix", ()):
        assert not w["cam_free"][c] and 0 < c < len(w["cams"]) - 1


@pytest.mark.parametrize("name", EXPECT)
def test_cases_reach_their_termination(oracle, synth, name):
    case = IC.CASES[name]
    w = IC.window(synth, case)
    m = IC.imu(synth, w, case)
    c, p, v, b, s, tr = IC.solve_oracle(oracle, w, m, case)
    if "expect" in case:
        assert s["termination"] == case["expect"]
    if case.get("moved"):
        assert s["successful_steps"] >= 1 and not s["usable"]
        assert np.array_equal(c, w["cams"]) and np.array_equal(v, m["cam_velocity"]) and np.array_equal(b, m["cam_bias"])


@pytest.mark.parametrize("name", ["chain_cf20", "duplicate_pairs", "backwards_factor", "fixed_middle", "durations_1ms_2s"])
def test_oracle_does_not_depend_on_the_factor_order(oracle, synth, name):
    case = IC.CASES[name]
    w = IC.window(synth, case)
    m = IC.imu(synth, w, case)
    ref = IC.solve_oracle(oracle, w, m, case)
    keys = ("cam_i", "cam_j", "duration", "rotation", "velocity", "position", "covariance", "bias_gyro", "bias_accel",
            "bias_jacobian")
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(len(m["cam_i"]))
        if seed == 0:
            perm = perm[::-1].copy()
        mp = dict(m, **{k: m[k][perm] for k in keys})
        c, p, v, b, s, tr = IC.solve_oracle(oracle, w, mp, case)
        assert [s[k] for k in ("termination", "iterations", "successful_steps", "usable")] == \
               [ref[4][k] for k in ("termination", "iterations", "successful_steps", "usable")]
        assert [t["outcome"] for t in tr] == [t["outcome"] for t in ref[5]]
        # only the summation order of the inertial blocks differs
        assert np.allclose([t["cost"] for t in tr], [t["cost"] for t in ref[5]], rtol=1e-12)
        assert np.allclose([t["radius"] for t in tr], [t["radius"] for t in ref[5]], rtol=1e-10)
        assert np.allclose(c, ref[0], rtol=1e-10, atol=1e-12) and np.allclose(p, ref[1], rtol=1e-9, atol=1e-11)
        assert np.allclose(v, ref[2], rtol=1e-9, atol=1e-11) and np.allclose(b, ref[3], rtol=1e-8, atol=1e-11)


def test_make_imu_knobs_stay_consistent_with_the_truth(synth):
    w = synth.make_ba_window(n_kf=10, n_points=50, run_max=4, config_id=97)
    pairs = [(2, 3), (5, 3), (3, 7), (3, 7), (9, 2)]
    durs = [1e-3, 2.0, 0.5, 0.25, 1.0]
    m = synth.make_imu(w, pairs=pairs, durations=durs, cov_scale=1e-2, cov_cond=1e6, gyro_bias_sigma=1e-3,
                       accel_bias_sigma=1e-1, zero_bias_jacobian=True, sigma_rot=1e-9, sigma_vel=1e-9, sigma_pos=1e-9)
    assert [tuple(map(int, p)) for p in zip(m["cam_i"], m["cam_j"])] == pairs
    assert np.array_equal(m["duration"], durs)
    assert (m["gyro_bias_sigma"], m["accel_bias_sigma"]) == (1e-3, 1e-1) and not np.any(m["bias_jacobian"])
    g = m["gravity"]
    R = [synth.rodrigues(w["cams_true"][c, :3]) for c in range(len(w["cams"]))]
    ctr, vt = w["cams_true"][:, 3:], m["cam_velocity_true"]
    for f, (i, j) in enumerate(pairs):
        T = durs[f]
        # the ground truth satisfies every factor up to its (here 1e-9) noise
        assert np.allclose(m["rotation"][f].reshape(3, 3), R[i] @ R[j].T, atol=1e-8)
        assert np.allclose(m["velocity"][f], R[i] @ (vt[j] - vt[i] - g * T), atol=1e-8)
        assert np.allclose(m["position"][f], R[i] @ (ctr[j] - ctr[i] - vt[i] * T - 0.5 * g * T * T), atol=1e-8)
        ev = np.linalg.eigvalsh(m["covariance"][f].reshape(9, 9))
        assert ev[0] > 0 and np.isclose(ev[-1] / ev[0], 1e6, rtol=1e-6)
    # the defaults are unchanged by the knobs' existence; a shuffle only permutes the factors
    base = synth.make_imu(w)
    sh = synth.make_imu(w, shuffle=3)
    perm = [list(zip(base["cam_i"], base["cam_j"])).index(p) for p in zip(sh["cam_i"], sh["cam_j"])]
    assert sorted(perm) == list(range(len(base["cam_i"]))) and perm != sorted(perm)
    for k in ("cam_i", "cam_j", "duration", "rotation", "velocity", "position", "covariance", "bias_gyro", "bias_accel",
              "bias_jacobian"):
        assert np.array_equal(sh[k], base[k][perm]), k
    for k in ("cam_velocity", "cam_bias", "cam_velocity_true"):
        assert np.array_equal(sh[k], base[k]), k
    scaled = synth.make_imu(w, cov_scale=4.0)
    assert np.allclose(scaled["covariance"], 4.0 * base["covariance"], rtol=1e-15, atol=0)
    assert np.array_equal(scaled["velocity"], base["velocity"])
