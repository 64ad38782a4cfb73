"""Which kernels a bundle adjustment launches, per shape and knob: the host driver of csrc/ba.hip chooses among nine
kernel paths (ba_choose_path, ba_choose_fusion, ba_choose_band), and a change to one condition would silently move a
window onto another kernel.  Every case is one solve of max_num_iterations 4 inside prof_begin / prof_end on the smallest
window that reaches its path, and pins
  the set of profile scope names (with the case's own number of speculative sets),
  the per-scope launch counts with ba_speculative_sets 1 (rounds are then enqueued exactly max_iter times, whatever the
  host-to-GPU timing; with more sets the number of rounds the host enqueues depends on that timing by design),
  iterations, successful_steps, termination and usable of both runs, and final_cost to relative 1e-9 (the repeatability
  bound of test_repeatability_of_a_pass).
EXPECT was recorded once, on an MI355X, from a build of the commit BEFORE the driver was split into named steps; it is
never regenerated from the code under test (run_case below is all a recorder needs)."""
import numpy as np
import pytest

import inertial_cases as IC

pytestmark = pytest.mark.gpu

MAX_ITER = 4
SCHEDULE = ("iterations", "successful_steps", "termination", "usable")
KNOBS = ("ba_fuse_mode", "ba_speculative_sets", "ba_band_mode", "ba_imu_mode", "ba_batch_mode")      # all default to 0

PLAIN = dict(n_kf=8, n_points=300)
BLOCKED = dict(n_kf=24, run_max=6, n_points=600)                       # 22 free cameras: n = 132 > 126
WIDE = dict(n_kf=30, run_min=12, run_max=20, n_points=600)             # camera spans beyond the band
GENERIC = dict(n_kf=131, run_max=6, n_points=400)                      # 129 free cameras > 128
NO_FREE = dict(n_kf=3, n_points=60)
INERTIAL = "ci2_one_factor"                                            # the smallest consecutive-factor window

# name -> (kind, window, knobs)
CASES = {
    "plain": ("single", PLAIN, {}),
    "plain_fuse1": ("single", PLAIN, dict(ba_fuse_mode=1)),
    "plain_fuse3_sets3": ("single", PLAIN, dict(ba_fuse_mode=3, ba_speculative_sets=3)),
    "one_rank_comm": ("comm", PLAIN, {}),
    "blocked_banded": ("single", BLOCKED, {}),
    "blocked_band2": ("single", BLOCKED, dict(ba_band_mode=2)),
    "blocked_band1": ("single", BLOCKED, dict(ba_band_mode=1)),
    "blocked_wide_span": ("single", WIDE, {}),
    "generic_k5": ("single", GENERIC, {}),
    "no_free_camera": ("nofree", NO_FREE, {}),
    "inertial_lds": ("inertial", INERTIAL, {}),
    "inertial_imu1": ("inertial", INERTIAL, dict(ba_imu_mode=1)),
    "batch_grid": ("batch", PLAIN, {}),
    "batch_lanes": ("batch", PLAIN, dict(ba_batch_mode=1)),
}

# name -> (scope names, {scope: launches with one set}, schedule with the case's sets, final_cost(s), schedule with
# one set, final_cost(s) with one set); batches hold one schedule / cost per window
EXPECT = {
    "plain": (["K0_ba_init", "K10_ba_finalize", "K5_ba_schur_mfma", "K5s_group_landmarks", "K78_ba_solve_backsub"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_schur_mfma": 4, "K5s_group_landmarks": 1, "K78_ba_solve_backsub": 4},
        [(4, 4, 0, 1)], [1523.4899802894204], [(4, 4, 0, 1)], [1523.4899802894188]),
    "plain_fuse1": (["K0_ba_init", "K10_ba_finalize", "K5_ba_schur_mfma", "K5s_group_landmarks", "K7_ba_reduced_solve", "K8_ba_backsub_cost"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_schur_mfma": 4, "K5s_group_landmarks": 1, "K7_ba_reduced_solve": 4, "K8_ba_backsub_cost": 4},
        [(4, 4, 0, 1)], [1523.4899802894201], [(4, 4, 0, 1)], [1523.489980289421]),
    "plain_fuse3_sets3": (["K0_ba_init", "K10_ba_finalize", "K578_ba_round", "K5s_group_landmarks"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K578_ba_round": 4, "K5s_group_landmarks": 1},
        [(4, 4, 0, 1)], [1523.4899802894215], [(4, 4, 0, 1)], [1523.489980289421]),
    "one_rank_comm": (["C1_allreduce_system", "C2_allreduce_cost", "K0_ba_init", "K10_ba_finalize", "K5_ba_schur_mfma", "K5s_group_landmarks", "K78_ba_solve_backsub"],
        {"C1_allreduce_system": 4, "C2_allreduce_cost": 4, "K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_schur_mfma": 4, "K5s_group_landmarks": 1, "K78_ba_solve_backsub": 4},
        [(4, 4, 0, 1)], [1523.4899802894201], [(4, 4, 0, 1)], [1523.489980289421]),
    "blocked_banded": (["K0_ba_init", "K10_ba_finalize", "K5_ba_schur_mfma", "K5s_group_landmarks", "K7_ba_reduced_solve_blocked", "K7b_band_factor", "K7c_band_separator", "K8_ba_backsub_cost"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_schur_mfma": 4, "K5s_group_landmarks": 1, "K7_ba_reduced_solve_blocked": 4, "K7b_band_factor": 4, "K7c_band_separator": 4, "K8_ba_backsub_cost": 4},
        [(4, 4, 0, 1)], [2960.277979581623], [(4, 4, 0, 1)], [2960.277979581582]),
    "blocked_band2": (["K0_ba_init", "K10_ba_finalize", "K5_ba_schur_mfma", "K5s_group_landmarks", "K7_ba_reduced_solve_blocked", "K7b_band_factor", "K8_ba_backsub_cost"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_schur_mfma": 4, "K5s_group_landmarks": 1, "K7_ba_reduced_solve_blocked": 4, "K7b_band_factor": 4, "K8_ba_backsub_cost": 4},
        [(4, 4, 0, 1)], [2960.277979581603], [(4, 4, 0, 1)], [2960.2779795816023]),
    "blocked_band1": (["K0_ba_init", "K10_ba_finalize", "K5_ba_schur_mfma", "K5s_group_landmarks", "K7_ba_reduced_solve_blocked", "K8_ba_backsub_cost"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_schur_mfma": 4, "K5s_group_landmarks": 1, "K7_ba_reduced_solve_blocked": 4, "K8_ba_backsub_cost": 4},
        [(4, 4, 0, 1)], [2960.2779795815954], [(4, 4, 0, 1)], [2960.27797958159]),
    "blocked_wide_span": (["K0_ba_init", "K10_ba_finalize", "K5_ba_schur_mfma", "K5s_group_landmarks", "K7_ba_reduced_solve_blocked", "K8_ba_backsub_cost"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_schur_mfma": 4, "K5s_group_landmarks": 1, "K7_ba_reduced_solve_blocked": 4, "K8_ba_backsub_cost": 4},
        [(4, 0, 0, 1)], [2317918.317784622], [(4, 0, 0, 1)], [2317918.3177846223]),
    "generic_k5": (["K0_ba_init", "K10_ba_finalize", "K5_ba_linearize_schur", "K7_ba_reduced_solve_blocked", "K8_ba_backsub_cost_global"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_linearize_schur": 4, "K7_ba_reduced_solve_blocked": 4, "K8_ba_backsub_cost_global": 4},
        [(4, 4, 0, 1)], [1543.5173645738828], [(4, 4, 0, 1)], [1543.5173645745149]),
    "no_free_camera": (["K0_ba_init", "K10_ba_finalize", "K5_ba_linearize_schur", "K7_ba_reduced_solve_global", "K8_ba_backsub_cost"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_linearize_schur": 4, "K7_ba_reduced_solve_global": 4, "K8_ba_backsub_cost": 4},
        [(4, 4, 0, 1)], [1026.364613324837], [(4, 4, 0, 1)], [1026.364613324837]),
    "inertial_lds": (["K0_ba_init", "K10_ba_finalize", "K5_ba_schur_mfma", "K5s_group_landmarks", "K6i_imu_eliminate", "K7_ba_reduced_solve", "K7i_imu_expand", "K8_ba_backsub_cost"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_schur_mfma": 4, "K5s_group_landmarks": 1, "K6i_imu_eliminate": 4, "K7_ba_reduced_solve": 4, "K7i_imu_expand": 4, "K8_ba_backsub_cost": 4},
        [(4, 4, 0, 1)], [934.7417344866442], [(4, 4, 0, 1)], [934.7417344866451]),
    "inertial_imu1": (["K0_ba_init", "K10_ba_finalize", "K5_ba_schur_mfma", "K5s_group_landmarks", "K7_ba_reduced_solve_inertial", "K8_ba_backsub_cost"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_schur_mfma": 4, "K5s_group_landmarks": 1, "K7_ba_reduced_solve_inertial": 4, "K8_ba_backsub_cost": 4},
        [(4, 4, 0, 1)], [934.7417344866461], [(4, 4, 0, 1)], [934.7417344866449]),
    "batch_grid": (["K0_ba_init", "K10_ba_finalize", "K5_ba_schur_mfma", "K5s_group_landmarks", "K7_ba_reduced_solve", "K8_ba_backsub_cost"],
        {"K0_ba_init": 1, "K10_ba_finalize": 1, "K5_ba_schur_mfma": 4, "K5s_group_landmarks": 1, "K7_ba_reduced_solve": 4, "K8_ba_backsub_cost": 4},
        [(4, 4, 0, 1), (4, 4, 0, 1), (4, 4, 0, 1)], [1523.489980289417, 1813.623949196019, 1765.8263875663383], [(4, 4, 0, 1), (4, 4, 0, 1), (4, 4, 0, 1)], [1523.4899802894179, 1813.6239491960173, 1765.8263875664013]),
    "batch_lanes": ([],
        {},
        [(4, 4, 0, 1), (4, 4, 0, 1), (4, 4, 0, 1)], [1523.4899802894192, 1813.6239491960173, 1765.8263875663613], [(4, 4, 0, 1), (4, 4, 0, 1), (4, 4, 0, 1)], [1523.4899802894215, 1813.6239491960187, 1765.8263875663338]),
}

_PROBLEMS = {}


def _problem(synth, name):
    """The host-side inputs of a case, built once per session and never written to."""
    if name not in _PROBLEMS:
        kind, win, _ = CASES[name]
        if kind == "inertial":
            w = IC.window(synth, IC.CASES[win])
            _PROBLEMS[name] = [(w, IC.imu(synth, w, IC.CASES[win]))]
        elif kind == "batch":
            _PROBLEMS[name] = [(synth.make_ba_window(seed_stream=i, **win), None) for i in range(3)]
        else:
            w = synth.make_ba_window(**win)
            if kind == "nofree":
                w["cam_free"] = np.zeros_like(w["cam_free"])
            _PROBLEMS[name] = [(w, None)]
    return _PROBLEMS[name]


def _solve(c, rs, kind, probs, knobs):
    """One profiled solve on context c under `knobs`; returns (profile, [summary per window])."""
    opt = rs.default_options()
    opt.max_num_iterations = MAX_ITER
    args = [(c.dev(w["cams"]), w["cam_free"], c.dev(w["points"]), c.dev(w["obs_ptr"]), c.dev(w["obs_cam"]), c.dev(w["obs_uv"]), w["K"])
            for w, _ in probs]
    try:
        for k, v in knobs.items():
            c.set_int(k, v)
        c.prof_begin()
        try:
            if kind == "batch":
                out = c.bundle_adjust_batch(args, options=opt)
            elif kind == "inertial":
                out = [c.bundle_adjust_inertial(*args[0], probs[0][1], options=opt)[0]]
            else:
                out = [c.bundle_adjust(*args[0], options=opt)]
        finally:
            prof = c.prof_end()
    finally:
        for k in KNOBS:
            c.set_int(k, 0)
    return prof, out


def run_case(ctx, rs, synth, name):
    """(scope names, launch counts with one set, schedules, costs, schedules with one set, costs with one set)."""
    kind, _, knobs = CASES[name]
    probs = _problem(synth, name)
    c = ctx
    if kind == "comm":                      # a communicator of one rank, on a context of its own
        c = rs.Context(0)
        rs.Context.comm_init_local([c])
    try:
        prof, out = _solve(c, rs, kind, probs, knobs)
        prof1, out1 = _solve(c, rs, kind, probs, dict(knobs, ba_speculative_sets=1))
    finally:
        if c is not ctx:
            c.comm_destroy()
            c.close()
    sched = lambda o: [tuple(int(s[k]) for k in SCHEDULE) for s in o]      # noqa: E731
    cost = lambda o: [float(s["final_cost"]) for s in o]                   # noqa: E731
    return sorted(prof), {k: int(v[0]) for k, v in sorted(prof1.items())}, sched(out), cost(out), sched(out1), cost(out1)


@pytest.mark.parametrize("name", list(CASES))
def test_ba_path(ctx, rs, synth, name):
    names, counts, sched, cost, sched1, cost1 = run_case(ctx, rs, synth, name)
    print(name, names, counts, sched, cost, sched1, cost1)
    e_names, e_counts, e_sched, e_cost, e_sched1, e_cost1 = EXPECT[name]
    assert set(names) == set(e_names)
    assert counts == e_counts
    assert sched == e_sched and sched1 == e_sched1
    assert np.allclose(cost, e_cost, rtol=1e-9, atol=0.0) and np.allclose(cost1, e_cost1, rtol=1e-9, atol=0.0)


def test_no_free_camera_against_the_oracle(ctx, synth, oracle):
    """The values of the path without a free camera (n = 0: only the landmarks move), against the CPU oracle; the case
    above pins its kernels and its cost alone.  A clean, well-conditioned window: the oracle ends on termination 1 after
    5 iterations with 4 successful steps (an accepted step, a rejected step and a convergence exit, 47.666137 ->
    17.646648), and 1e-13 relative on its input points moves its result by 6e-13 at most, 3e-8 of the tolerance below —
    which is the plain-window parity tolerance (test_gpu_parity.py)."""
    w = synth.make_ba_window(n_kf=3, n_points=60, outlier_frac=0.0, pixel_noise=0.3, rot_noise_deg=0.2, config_id=23)
    free = np.zeros_like(w["cam_free"])
    dc, dp = ctx.dev(w["cams"]), ctx.dev(w["points"])
    s = ctx.bundle_adjust(dc, free, dp, ctx.dev(w["obs_ptr"]), ctx.dev(w["obs_cam"]), ctx.dev(w["obs_uv"]), w["K"])
    _, rp, r = oracle.bundle_adjust(w["cams"], free, w["points"], w["obs_ptr"], w["obs_cam"], w["obs_uv"], w["K"])
    print({k: s[k] for k in ("termination", "iterations", "successful_steps", "initial_cost", "final_cost")}, r,
          float(np.abs(dp.cpu().numpy() - rp).max()))
    for k in ("termination", "iterations", "successful_steps"):
        assert s[k] == r[k], k
    assert np.array_equal(dc.cpu().numpy(), np.asarray(w["cams"], np.float64))
    assert np.allclose(dp.cpu().numpy(), rp, rtol=1e-6, atol=1e-7)
    assert np.isclose(s["final_cost"], r["final_cost"], rtol=1e-7, atol=0.0)
