"""Cases of the per-frame pose solve (refine_pose and its RotationPrior / InertialDelta forms) shared by
tests/test_refine_pose_cpu.py (oracle against dense_lm) and tests/test_gpu_refine_pose.py (GPU against the oracle).

A case is a dict:
  scene  keyword arguments of synth.make_refine_problem (n, seed, outlier_frac, noise_px, rot0, offset, ...)
  opt    rs_ba_options fields that differ from the defaults
  prior  (sigma, perturbation of the predicted rotation in rad) for a RotationPrior (kind 1)
  delta  True for an InertialDelta (kind 2); "not_pd" replaces its covariance by one that is not positive definite
  poke   "nan_point" / "nan_uv" / "zero_depth": one input made non-finite, or one point at camera-frame depth exactly 0
  expect the termination the case exists to reach (checked against the oracle, so that the case keeps reaching it)
  moved  True: the case must end unusable after at least one successful step (checked against the oracle)
  dense  False: too large for the dense restatement (the GPU file still compares it with the oracle)
"""
import numpy as np

NO_CONVERGENCE, FUNCTION, PARAMETER, GRADIENT, RADIUS, FAILURE = 0, 1, 2, 3, 4, 5

DEFAULT_SCENE = dict(n=300, seed=1, noise_px=0.5, outlier_frac=0.1)
DENSE_MAX_N = 2047          # dense_lm loops over observations in Python

# option field -> dense_lm.solve keyword
DENSE_KW = dict(max_num_iterations="max_iter", initial_trust_region_radius="r0", max_trust_region_radius="rmax",
                min_trust_region_radius="rmin", min_relative_decrease="min_rel", min_lm_diagonal="dmin",
                max_lm_diagonal="dmax", function_tolerance="ftol", gradient_tolerance="gtol",
                parameter_tolerance="ptol", max_num_consecutive_invalid_steps="max_invalid", jacobi_scaling="jacobi")


def _c(scene=None, **kw):
    return dict(scene=dict(DEFAULT_SCENE, **(scene or {})), opt=kw.pop("opt", {}), **kw)


CASES = {}
# observation counts: a single partial wave, wave edges, 512-thread stride edges, several strides
for _n in (1, 2, 63, 64, 65, 511, 512, 513, 2000, 2047, 4097, 50000):
    CASES[f"n{_n}"] = _c(dict(n=_n, seed=_n), dense=_n <= DENSE_MAX_N)
# loss: outlier fractions, Huber's linear region everywhere, pure L2
for _f in (0.0, 0.3, 0.6):
    CASES[f"outliers{_f}"] = _c(dict(outlier_frac=_f, noise_px=1.0, seed=7))
CASES["huber_tiny"] = _c(dict(outlier_frac=0.3, noise_px=1.0), opt=dict(huber_delta=1e-4))
CASES["huber_huge"] = _c(dict(outlier_frac=0.3, noise_px=1.0), opt=dict(huber_delta=1e6))
# starting pose: zero rotation, inside / just outside the first-order branch (theta^2 <= DBL_EPSILON), near pi, far away
CASES["rot_zero"] = _c(dict(rot0=[0.0, 0.0, 0.0]))
CASES["rot_1e-9"] = _c(dict(rot0=[6e-10, -8e-10, 0.0]))
CASES["rot_2e-8"] = _c(dict(rot0=[0.0, 1.2e-8, 1.6e-8]))
CASES["rot_near_pi"] = _c(dict(rot0=[0.0, 0.0, np.pi - 1e-3]))
CASES["rot_near_pi_axis"] = _c(dict(rot0=list((np.pi - 1e-6) * np.array([2.0, -1.0, 2.0]) / 3.0), rot_err=0.05))
CASES["offset_1e3"] = _c(dict(offset=1e3, trans_err=0.5))
CASES["offset_1e3_rot_zero"] = _c(dict(offset=1e3, rot0=[0.0, 0.0, 0.0]))
CASES["big_start_error"] = _c(dict(rot_err=0.3, trans_err=2.0, seed=5))
CASES["bad_depth"] = _c(dict(bad_depth_frac=0.2, seed=3))
CASES["bad_depth_rot_1e-9"] = _c(dict(bad_depth_frac=0.4, rot0=[1e-9, 0.0, 0.0], seed=4))
# the first-order branch seen by the whole solve: a rank-poor scene (few points, far away) whose first step is large
CASES["rot_1e-9_one_step"] = _c(dict(n=6, rot0=[0.0, 1e-9, 0.0], rot_err=0.2, trans_err=1.0, noise_px=0.0, outlier_frac=0.0),
                                opt=dict(max_num_iterations=1), expect=NO_CONVERGENCE)
# each termination, forced through the options
CASES["max_iter_0"] = _c(opt=dict(max_num_iterations=0), expect=NO_CONVERGENCE)
CASES["max_iter_1"] = _c(opt=dict(max_num_iterations=1), expect=NO_CONVERGENCE)
CASES["gradient"] = _c(opt=dict(gradient_tolerance=1e3), expect=GRADIENT)
CASES["gradient_late"] = _c(opt=dict(gradient_tolerance=1e-2, function_tolerance=0.0, parameter_tolerance=0.0), expect=GRADIENT)
CASES["function"] = _c(opt=dict(function_tolerance=0.5), expect=FUNCTION)
CASES["parameter"] = _c(opt=dict(parameter_tolerance=1e-2), expect=PARAMETER)
# (a natural rejection on a scene with points behind the camera / every step rejected from a small radius)
CASES["radius_min"] = _c(dict(bad_depth_frac=0.2, seed=3), opt=dict(min_trust_region_radius=9e3), expect=RADIUS)
CASES["radius_tiny_initial"] = _c(opt=dict(initial_trust_region_radius=1e-3, min_trust_region_radius=1e-4, min_relative_decrease=1.5),
                                  expect=RADIUS)
CASES["nan_point"] = _c(poke="nan_point", expect=FAILURE)
CASES["nan_uv"] = _c(poke="nan_uv", expect=FAILURE)
CASES["zero_depth"] = _c(dict(rot0=[0.0, 0.0, 0.0]), poke="zero_depth", expect=FAILURE)
CASES["no_jacobi"] = _c(dict(rot_err=0.1, trans_err=0.5), opt=dict(jacobi_scaling=0))
# a capped LM diagonal from a small radius: the damping is max_lm_diagonal / (radius s^2), so the step depends on the
# Jacobi scale s itself — which is fixed at the first Jacobian
CASES["lm_diagonal_cap"] = _c(dict(rot_err=0.3, trans_err=2.0, seed=5), opt=dict(initial_trust_region_radius=1.0, max_lm_diagonal=0.5))
CASES["max_iter_2_no_jacobi"] = _c(opt=dict(max_num_iterations=2, jacobi_scaling=0), expect=NO_CONVERGENCE)
# RotationPrior (kind 1)
for _s in (1e-6, 1e-3, 1.0, 1e3):
    for _p in (0.0, 0.01):
        CASES[f"prior_s{_s:g}_p{_p:g}"] = _c(prior=(_s, _p))
CASES["prior_n1"] = _c(dict(n=1, seed=11), prior=(1e-3, 0.01))
CASES["prior_n513"] = _c(dict(n=513, seed=12), prior=(1e-3, 0.01))
CASES["prior_max_iter_1"] = _c(prior=(1e-3, 0.01), opt=dict(max_num_iterations=1), expect=NO_CONVERGENCE)
CASES["prior_nan_uv"] = _c(prior=(1e-3, 0.01), poke="nan_uv", expect=FAILURE)
# InertialDelta (kind 2)
for _s in range(4):
    CASES[f"delta_seed{_s}"] = _c(dict(seed=20 + _s, imu=True), delta=True)
CASES["delta_n1"] = _c(dict(n=1, seed=30, imu=True), delta=True)
CASES["delta_n513"] = _c(dict(n=513, seed=31, imu=True), delta=True)
CASES["delta_not_pd"] = _c(dict(seed=32, imu=True), delta="not_pd")
CASES["delta_no_jacobi"] = _c(dict(seed=33, imu=True), delta=True, opt=dict(jacobi_scaling=0))
CASES["delta_lm_diagonal_cap"] = _c(dict(rot_err=0.3, trans_err=2.0, seed=5, imu=True), delta=True,
                                    opt=dict(initial_trust_region_radius=1.0, max_lm_diagonal=0.5))
# unusable after the state has moved: a negative LM diagonal at a fixed radius anti-damps the step; the first steps are
# accepted, then the damped system stops being positive definite and one invalid step ends the solve in FAILURE — camera
# and velocity must come back as they went in although x had moved (the margin: every diagonal in [-0.40, -0.325] gives
# this schedule)
_UNUSABLE = dict(min_lm_diagonal=-0.35, max_lm_diagonal=-0.35, initial_trust_region_radius=1.0, max_trust_region_radius=1.0,
                 max_num_consecutive_invalid_steps=1, max_num_iterations=20)
CASES["delta_unusable_after_steps"] = _c(dict(n=10, seed=3, rot_err=0.3, trans_err=1.5, imu=True), delta=True, opt=_UNUSABLE,
                                         expect=FAILURE, moved=True)
CASES["delta_unusable_after_steps_n6"] = _c(dict(n=6, seed=4, rot_err=0.2, trans_err=1.0, imu=True), delta=True,
                                            opt=dict(_UNUSABLE, min_lm_diagonal=-0.36, max_lm_diagonal=-0.36), expect=FAILURE, moved=True)
# min_lm_diagonal = 0: the damping is the bare column norm / radius, so a parameter block without residuals (the bias of an
# InertialDelta, which is not part of this problem) would make the system singular
CASES["min_diagonal_0"] = _c(opt=dict(min_lm_diagonal=0.0))
CASES["delta_min_diagonal_0"] = _c(dict(seed=20, imu=True), delta=True, opt=dict(min_lm_diagonal=0.0))
CASES["delta_nan_uv"] = _c(dict(seed=34, imu=True), delta=True, poke="nan_uv", expect=FAILURE)
CASES["delta_max_iter_0"] = _c(dict(seed=35, imu=True), delta=True, opt=dict(max_num_iterations=0), expect=NO_CONVERGENCE)


def dense_ok(case):
    return case.get("dense", True) and case["scene"]["n"] <= DENSE_MAX_N


def problem(synth, case):
    """The scene of a case with its poke applied: dict of synth.make_refine_problem + prior / delta arguments."""
    p = synth.make_refine_problem(**case["scene"])
    pts, uv = p["points"].copy(), p["uv"].copy()
    poke = case.get("poke")
    k = len(pts) // 2
    if poke == "nan_point":
        pts[k, 1] = np.nan
    elif poke == "nan_uv":
        uv[k, 0] = np.nan
    elif poke == "zero_depth":
        # with a zero rotation both the oracle's and the kernel's rotation are exactly the identity, so the camera-frame
        # depth of this point is X_z - c_z = 0 in floating point
        assert not np.any(p["cam0"][:3])
        pts[k, 2] = p["cam0"][5]
    p.update(points=pts, uv=uv, prior=None, poke_index=k if poke else None)
    if case.get("prior"):
        sigma, pert = case["prior"]
        R = synth.rodrigues(p["cam_true"][:3])
        if pert:
            R = synth.rodrigues(np.array([0.6, -0.48, 0.64]) * pert) @ R
        p["prior"] = (R, sigma)
    if case.get("delta") == "not_pd":
        f = dict(p["delta"]["imu"])
        cov = np.diag([4e-6] * 3 + [4e-4] * 3 + [1e-4] * 3)
        cov[4, 4] = -4e-4
        f["covariance"] = cov.reshape(1, 81)
        p["delta"] = dict(p["delta"], imu=f)
    elif not case.get("delta"):
        p["delta"] = None
    return p


def options(mod, case):
    """rs_ba_options of a case from mod.default_options() (mod = the oracle or the GPU bindings: same fields)."""
    o = mod.default_options()
    for k, v in case["opt"].items():
        setattr(o, k, v)
    return o


def solve_oracle(O, p, case):
    """Returns cam, velocity (None unless kind 2), summary."""
    o = options(O, case)
    if p["prior"] is None and p["delta"] is None:
        cam, s = O.refine_pose(p["cam0"], p["points"], p["uv"], p["K"], options=o)
        return cam, None, s
    cam, vel, s = O.refine_pose_inertial(p["cam0"], p["points"], p["uv"], p["K"], prior=p["prior"], delta=p["delta"], options=o)
    return cam, (vel if p["delta"] is not None else None), s


def solve_dense(D, O, p, case):
    """dense_lm on the same problem; returns cam, velocity (None unless kind 2), summary."""
    n = len(p["points"])
    kw = {}
    o = options(O, case)
    for k, name in DENSE_KW.items():
        if k in case["opt"]:
            kw[name] = getattr(o, k)
    delta = None
    if p["delta"] is not None:
        delta = dict(p["delta"], prev_pose=np.asarray(p["delta"]["prev_pose"], np.float64))
    prob = D.Problem(p["cam0"][None], np.ones(1, np.uint8), p["points"], np.arange(n + 1), np.zeros(n, np.int64), p["uv"], p["K"],
                     huber_a=o.huber_delta, points_constant=True, prior=p["prior"], delta=delta)
    with np.errstate(all="ignore"):
        x, s, _ = D.solve(prob, **kw)
    if not s["usable"]:
        x = prob.pack(prob.cams0, prob.pts0)
    return x[:6], (x[6:9] if p["delta"] is not None else None), s
