"""Cases of the inertial bundle adjustment (rs_bundle_adjust_inertial) shared by tests/test_inertial_ba_cpu.py (oracle
against dense_lm) and tests/test_gpu_inertial_ba_envelope.py (GPU against the oracle, imu modes 0 and 1).

A case is a dict:
  window  keyword arguments of synth.make_ba_window
  fix     cameras fixed in the middle of the window (besides the first two): their pose slots and inertial slots differ
  imu     keyword arguments of synth.make_imu; None: a vision-only control (rs_bundle_adjust)
  opt     rs_ba_options fields that differ from the defaults
  poke    "nan_uv": one observation made non-finite
  path0   the solve that imu mode 0 must take: "lds" (K6a / K6b / K7i around the LDS reduced solve) or "big" (the N x N
          blocked solve); imu mode 1 always takes "big".  None for the vision-only controls.  Derived from the rule of
          ba_solve_impl by hand, so that a change to that gate cannot quietly move a case to the other path
  sets    True: the GPU file also runs ba_speculative_sets 1, 2 and 3
  expect  the termination the case exists to reach (checked against the oracle)
  moved   True: the case must end unusable after at least one successful step
  dense   True: small enough for the dense restatement (tests/dense_lm.py)
"""
import numpy as np

NO_CONVERGENCE, FUNCTION, PARAMETER, GRADIENT, RADIUS, FAILURE = 0, 1, 2, 3, 4, 5

# option field -> dense_lm.solve keyword
DENSE_KW = dict(max_num_iterations="max_iter", initial_trust_region_radius="r0", max_trust_region_radius="rmax",
                min_trust_region_radius="rmin", min_relative_decrease="min_rel", min_lm_diagonal="dmin",
                max_lm_diagonal="dmax", function_tolerance="ftol", gradient_tolerance="gtol",
                parameter_tolerance="ptol", max_num_consecutive_invalid_steps="max_invalid", jacobi_scaling="jacobi")


def _c(window, imu=None, path0="lds", **kw):
    return dict(window=window, imu=imu, path0=path0, opt=kw.pop("opt", {}), **kw)


def _w(n_kf, n_points, config_id, run_max=6, run_min=3):
    """Every landmark seen at least three times, so that none drifts along its ray and the comparisons stay well posed."""
    return dict(n_kf=n_kf, n_points=n_points, run_min=run_min, run_max=run_max, config_id=config_id)


def _chain(cams):
    return [(int(a), int(b)) for a, b in zip(cams[:-1], cams[1:])]


# the small window of the dense comparisons (8 key frames, 6 optimised, 200 landmarks: like the golden inertial window)
W8 = _w(8, 200, 61)

CASES = {}
# ---- size boundary of the local-window path: n = 6 Cf <= 126 (Cf <= 21); Cf = 22 goes to the blocked path by itself.
# K6b's Schur update works on 16 x 16 tiles of the (n + 1) x (n + 1) upper triangle: 7 tiles per side up to n = 108,
# 8 (36 tiles) from Cf = 19 on
for _cf in range(17, 23):
    CASES[f"chain_cf{_cf}"] = _c(_w(_cf + 2, 600, 70 + _cf), {}, path0="lds" if _cf <= 21 else "big", sets=19 <= _cf <= 21)
# ---- the minimum: two inertial cameras, one factor
CASES["ci2_one_factor"] = _c(_w(6, 150, 81), dict(pairs=[(3, 4)]), dense=True)
# ---- K6b stages the z rows 84 at a time: Ci = 9 one pass, 10 and 18 two, 19 and 21 three (chain_cf21)
CASES["ci9_chain"] = _c(_w(11, 150, 82, run_max=5), {}, dense=True)
CASES["ci10_chain"] = _c(_w(12, 150, 83, run_max=5), {})
CASES["ci18_of_cf21_tail"] = _c(_w(23, 600, 84), dict(pairs=_chain(range(5, 23))), sets=True)
CASES["ci19_of_cf21_head"] = _c(_w(23, 600, 85), dict(pairs=_chain(range(2, 21))), sets=True)
# ---- part of the window inertial (Ci < Cf): the last cameras (their pose columns are those of the last tiles), the first,
# a chain with gaps (the inertial slots stay consecutive: a zero block in H_zz)
CASES["tail6_of_cf20"] = _c(_w(22, 600, 86), dict(pairs=_chain(range(16, 22))), sets=True)
CASES["head6_of_cf20"] = _c(_w(22, 600, 87), dict(pairs=_chain(range(2, 8))))
CASES["gaps_of_cf20"] = _c(_w(22, 600, 88), dict(skip={(6, 7), (12, 13), (13, 14)}), sets=True)
CASES["tail2_of_6"] = _c(W8, dict(pairs=[(5, 6), (6, 7)]), dense=True)
CASES["head3_of_6"] = _c(W8, dict(pairs=[(2, 3), (3, 4)]), dense=True)
CASES["gaps_of_6"] = _c(W8, dict(skip={(4, 5)}), dense=True)
# ---- order and form of the factors
CASES["shuffled"] = _c(W8, dict(shuffle=1), dense=True)
CASES["shuffled_cf19"] = _c(_w(21, 600, 89), dict(shuffle=2), sets=True)
CASES["duplicate_pairs"] = _c(W8, dict(pairs=[(2, 3), (3, 4), (3, 4), (4, 5), (5, 6), (5, 6), (6, 7), (2, 3)]), dense=True)
# a factor over a camera without an inertial block: the inertial slots stay consecutive
CASES["skips_noninertial_camera"] = _c(W8, dict(pairs=[(2, 3), (3, 5), (5, 6), (6, 7)]), dense=True)
# a factor over an inertial camera, or one that runs backwards: H_zz is no longer block tridiagonal -> blocked path
CASES["skips_inertial_camera"] = _c(W8, dict(pairs=[(2, 3), (3, 4), (4, 5), (3, 5), (5, 6)]), path0="big", dense=True)
CASES["backwards_factor"] = _c(W8, dict(pairs=[(2, 3), (4, 3), (4, 5), (5, 6)]), path0="big", dense=True)
CASES["backwards_chain"] = _c(W8, dict(pairs=[(7, 6), (6, 5), (5, 4), (4, 3), (3, 2)]), path0="big", dense=True)
# ---- a fixed camera in the middle: pose slot != inertial slot != camera index; one factor spans the fixed camera
CASES["fixed_middle"] = _c(_w(10, 150, 90, run_max=5), dict(pairs=_chain([2, 3, 4, 6, 7, 8, 9])), fix=[5], dense=True)
CASES["fixed_middle_cf20"] = _c(_w(23, 600, 91), dict(pairs=_chain([c for c in range(2, 23) if c != 12])), fix=[12], sets=True)
# ---- the factors themselves: durations, covariance scale / condition, bias densities, no bias correction
CASES["durations_1ms_2s"] = _c(W8, dict(durations=[1e-3, 2.0, 1e-3, 2.0, 0.5]), dense=True)
CASES["cov_scale_1e-3"] = _c(W8, dict(cov_scale=1e-3), dense=True)
CASES["cov_scale_1e3"] = _c(W8, dict(cov_scale=1e3), dense=True)
CASES["cov_cond_1e8"] = _c(W8, dict(cov_cond=1e8), dense=True)
CASES["bias_sigmas_large"] = _c(W8, dict(gyro_bias_sigma=1e-2, accel_bias_sigma=1.0), dense=True)
CASES["bias_sigmas_small"] = _c(W8, dict(gyro_bias_sigma=1e-7, accel_bias_sigma=1e-5), dense=True)
CASES["zero_bias_jacobian"] = _c(W8, dict(zero_bias_jacobian=True), dense=True)
# ---- options
CASES["no_jacobi"] = _c(W8, {}, opt=dict(jacobi_scaling=0), dense=True)
CASES["no_jacobi_cf20"] = _c(_w(22, 600, 92), {}, opt=dict(jacobi_scaling=0), sets=True)
CASES["min_diagonal_0"] = _c(W8, {}, opt=dict(min_lm_diagonal=0.0), dense=True)
# a capped LM diagonal from a small radius: the damping is max_lm_diagonal / (radius s^2)
CASES["lm_diagonal_cap"] = _c(W8, {}, opt=dict(initial_trust_region_radius=1.0, max_lm_diagonal=0.5), dense=True)
CASES["lm_diagonal_cap_cf21"] = _c(_w(23, 600, 93), {}, opt=dict(initial_trust_region_radius=1.0, max_lm_diagonal=0.5), sets=True)
CASES["max_iter_1"] = _c(W8, {}, opt=dict(max_num_iterations=1), expect=NO_CONVERGENCE, dense=True)
CASES["max_iter_2"] = _c(W8, {}, opt=dict(max_num_iterations=2), expect=NO_CONVERGENCE, dense=True)
CASES["max_iter_1_cf20"] = _c(_w(22, 600, 94), {}, opt=dict(max_num_iterations=1), expect=NO_CONVERGENCE, sets=True)
CASES["max_iter_2_cf20"] = _c(_w(22, 600, 94), {}, opt=dict(max_num_iterations=2), expect=NO_CONVERGENCE, sets=True)
CASES["radius_tiny"] = _c(W8, {}, opt=dict(initial_trust_region_radius=1e-4), dense=True)
CASES["radius_huge"] = _c(W8, {}, opt=dict(initial_trust_region_radius=1e14), dense=True)
CASES["function"] = _c(W8, {}, opt=dict(function_tolerance=0.5), expect=FUNCTION, dense=True)
CASES["parameter"] = _c(W8, {}, opt=dict(parameter_tolerance=1e-2), expect=PARAMETER, dense=True)
CASES["gradient"] = _c(W8, {}, opt=dict(gradient_tolerance=1e9), expect=GRADIENT, dense=True)
# every step rejected (rho never exceeds 1.5) and the first rejection takes the radius below the minimum
CASES["radius_min"] = _c(W8, {}, opt=dict(min_relative_decrease=1.5, min_trust_region_radius=9e3), expect=RADIUS, dense=True)
CASES["nan_uv"] = _c(W8, {}, poke="nan_uv", expect=FAILURE, dense=True)
# unusable after the state has moved: a negative LM diagonal at a fixed radius, without Jacobi scaling, anti-damps the
# step; the first step is accepted, then the damped system stops being positive definite and one invalid step ends the
# solve in FAILURE (the margin: every diagonal in [-0.0040, -0.0020] gives this schedule)
_UNUSABLE = dict(min_lm_diagonal=-0.0028, max_lm_diagonal=-0.0028, initial_trust_region_radius=1.0, max_trust_region_radius=1.0,
                 max_num_consecutive_invalid_steps=1, max_num_iterations=20, jacobi_scaling=0)
CASES["unusable_after_steps"] = _c(W8, {}, opt=_UNUSABLE, expect=FAILURE, moved=True, dense=True)
# ---- the blocked path at size: N = 240 + 360 (a partial 48-block) and a window of 100 key frames (N = 588 + 882)
CASES["big_cf40"] = _c(_w(42, 1500, 95), {}, path0="big")
CASES["big_kf100"] = _c(_w(100, 1500, 96, run_max=8), {}, path0="big")
# ---- vision-only controls at the sizes of the last tiles (K5 / K7 without K6)
for _cf in (19, 20, 21):
    CASES[f"vision_cf{_cf}"] = _c(_w(_cf + 2, 600, 70 + _cf), None, path0=None)


def window(synth, case):
    """The BA window of a case, with its extra fixed cameras and its poke applied."""
    w = synth.make_ba_window(**case["window"])
    for c in case.get("fix", ()):
        w["cam_free"][c] = 0
        w["cams"][c] = w["cams_true"][c]
    if case.get("poke") == "nan_uv":
        w["obs_uv"] = w["obs_uv"].copy()
        w["obs_uv"][len(w["obs_uv"]) // 2, 0] = np.nan
    return w


def imu(synth, w, case):
    return None if case["imu"] is None else synth.make_imu(w, **case["imu"])


def ba_args(w):
    return (w["cams"], w["cam_free"], w["points"], w["obs_ptr"], w["obs_cam"], w["obs_uv"], w["K"])


def options(mod, case):
    """rs_ba_options of a case from mod.default_options() (mod = the oracle or the GPU bindings: same fields)."""
    o = mod.default_options()
    for k, v in case["opt"].items():
        setattr(o, k, v)
    return o


def solve_oracle(O, w, m, case):
    """Returns cams, points, velocity, bias, summary, trace (velocity / bias None for a vision-only control)."""
    o = options(O, case)
    if m is None:
        c, p, s, tr = O.bundle_adjust_trace(*ba_args(w), options=o)
        return c, p, None, None, s, tr
    return O.bundle_adjust_inertial(*ba_args(w), m, options=o, trace=True)


def solve_dense(D, O, w, m, case):
    """dense_lm on the same problem; returns cams, velocity, bias, summary, trace (the input state when unusable)."""
    o = options(O, case)
    kw = {name: getattr(o, k) for k, name in DENSE_KW.items() if k in case["opt"]}
    prob = D.Problem(*ba_args(w), huber_a=o.huber_delta, imu=m)
    with np.errstate(all="ignore"):
        x, s, tr = D.solve(prob, **kw)
    if not s["usable"]:
        x = prob.pack(prob.cams0, prob.pts0)
    cams, _ = prob.unpack(x)
    vel, bias = prob.unpack_inertial(x)
    return cams, vel, bias, s, tr, prob
