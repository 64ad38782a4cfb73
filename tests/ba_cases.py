"""Cases of the vision-only bundle adjustment (rs_bundle_adjust, rs_bundle_adjust_batch) shared by
tests/test_ba_cases_cpu.py (oracle against dense_lm, every case reaches what it is for, stability of every schedule) and
tests/test_gpu_ba_envelope.py (every kernel path of the host driver against the oracle under every option case).

  WINDOWS    one window per path class of test_gpu_ba_paths.py (its make_ba_window arguments, with every landmark seen at
             least three times where the class allows it) and a "hard" twin of each (10 % outliers, 2 degrees of
             rotation noise) whose default solve rejects at least one step
  PATHS      the vision-only entries of test_gpu_ba_paths.CASES: name -> (kind, window class, knobs)
  OPTIONS    option cases: dict(opt = rs_ba_options fields that differ from the defaults (a callable takes the window's
             name: values tuned per window), poke = an input made non-finite, expect = the termination the case exists to
             reach, moved = it must end unusable after at least one successful step, not_pd = its first factorisation
             must fail, tuned = the per-window value it needs: it applies where TUNED has one)
  STRUCTURE  edits of a window's structure, solved with default options
  BATCHES    lists of windows solved by one rs_bundle_adjust_batch call under one option set
"""
import numpy as np

import test_gpu_ba_paths as P
from inertial_cases import DENSE_KW, FAILURE, FUNCTION, GRADIENT, NO_CONVERGENCE, PARAMETER, RADIUS, ba_args  # noqa: F401

ACCEPTED, REJECTED, INVALID, CONVERGED = 1, 0, -1, 2
LETTER = {ACCEPTED: "A", REJECTED: "R", INVALID: "I", CONVERGED: "C"}

HARD = dict(outlier_frac=0.1, rot_noise_deg=2.0)
# window class -> (make_ba_window arguments of test_gpu_ba_paths.py, config_id of the hard twin).  run_min = 3 wherever the
# class does not set it (WIDE asks for 12; NO_FREE has three key frames, so every landmark is seen by all three)
_CLASSES = {"plain": (P.PLAIN, 210), "blocked": (P.BLOCKED, 230), "wide": (P.WIDE, 230), "generic": (P.GENERIC, 201),
            "no_free": (P.NO_FREE, 222)}
WINDOWS = {}
for _name, (_args, _cfg) in _CLASSES.items():
    WINDOWS[_name] = dict(dict(run_min=3), **_args)
    WINDOWS[_name + "_hard"] = dict(WINDOWS[_name], config_id=_cfg, **HARD)
CLASS_OF = {id(a): n for n, (a, _) in _CLASSES.items()}

# the vision-only kernel paths: (kind, window class, knobs) of test_gpu_ba_paths.CASES, the gates are not restated here
PATHS = {k: (kind, CLASS_OF[id(win)], knobs) for k, (kind, win, knobs) in P.CASES.items() if kind != "inertial"}
SINGLE_PATHS = [k for k, (kind, _, _) in PATHS.items() if kind != "batch"]
BATCH_PATHS = [k for k, (kind, _, _) in PATHS.items() if kind == "batch"]


def is_no_free(window_name):
    return window_name.startswith("no_free")


# ---------------------------------------------------------------------------------------------------------------- options
# Values tuned per window on the CPU oracle; beside each the interval of values that gives the same schedule (outcome
# string and termination), found by bisection on the oracle.
#   ptol      parameter_tolerance of "parameter": the solve must end PARAMETER after at least one accepted step
#   not_pd    the constant LM diagonal (< 0) of "not_pd": the first factorisation fails
#   unusable  the constant LM diagonal (< 0) of "unusable_after_steps": accepted steps, then a failed factorisation
# (the negative diagonals were scanned down to -33: "<= x" means every value from there up to x)
TUNED = {
    "plain": dict(ptol=8e-3,            # AAAAC over [5.5e-3, 1.1e-2]
                  not_pd=-0.1,          # I over <= -0.016
                  unusable=-2.5e-3),    # AAI over [-3.6e-3, -1.6e-3]
    "blocked": dict(ptol=1.22e-2,       # AAC over [1.16e-2, 1.28e-2]
                    not_pd=-0.1,        # I over <= -2.7e-3
                    unusable=-3e-4),    # AAI over [-7.9e-4, -5.2e-5]
    "wide": dict(ptol=8e-3,             # RRRC over [7.0e-3, 9.2e-3]
                 not_pd=-0.1),          # I over <= -0.013; (no diagonal gives an accepted step before the failure)
    "generic": dict(ptol=8.5e-3,        # AAAC over [7.4e-3, 9.3e-3]
                    not_pd=-0.1),       # I over <= -3.1e-4; (accepted steps before the failure exist only over
                                        # [-1.0e-5, -7.9e-6], and there 1e-13 on the input moves the costs by 3e-5)
    "no_free": dict(ptol=0.17,          # C over >= 0.162 (the relative step grows from 0.159 on: no later exit exists)
                    not_pd=-1.0,        # I over <= -0.035
                    unusable=-5e-4),    # AAI over [-2.2e-3, -2.1e-4]
    "plain_hard": dict(ptol=3.5e-2,     # AAC over [2.5e-2, 4.4e-2]
                       not_pd=-0.1,     # I over <= -6.0e-4
                       unusable=-1e-4),   # AAI over [-3.2e-4, -1.7e-6]
    "blocked_hard": dict(not_pd=-0.1,   # I over <= -3.2e-3
                         unusable=-3e-4),   # AI over [-2.7e-3, -3.1e-5]
    "wide_hard": dict(not_pd=-0.1,      # I over <= -0.018
                      unusable=-7e-4),  # ARRRI over [-1.8e-3, -2.8e-4]
    "generic_hard": dict(not_pd=-0.1),  # I over <= -3.1e-4; (no accepted step before the failure)
    "no_free_hard": dict(not_pd=-0.1),  # I over <= -4.2e-3; (no accepted step before the failure)
}


def _negative_diagonal(key, max_invalid):
    def opt(window_name):
        v = TUNED[window_name][key]
        return dict(min_lm_diagonal=v, max_lm_diagonal=v, initial_trust_region_radius=1.0, max_trust_region_radius=1.0,
                    max_num_consecutive_invalid_steps=max_invalid, max_num_iterations=20, jacobi_scaling=0)
    return opt


def _o(opt=None, **kw):
    return dict(opt=opt or {}, **kw)


OPTIONS = {
    "default": _o(),
    "no_jacobi": _o(dict(jacobi_scaling=0)),
    "min_diagonal_0": _o(dict(min_lm_diagonal=0.0)),
    # a capped LM diagonal from a small radius: the damping is max_lm_diagonal / (radius s^2)
    "lm_diagonal_cap": _o(dict(initial_trust_region_radius=1.0, max_lm_diagonal=0.5)),
    # Without a clamp the damping clamp(s^2 h) / (radius s^2) is h / radius whatever the Jacobi scale s: "no_jacobi" alone
    # cannot tell a solve that ignores jacobi_scaling from one that honours it.  Under the cap it is 0.5 / (radius s^2), and
    # a floor above s^2 h ~ 1 is the only thing that makes min_lm_diagonal matter
    "no_jacobi_cap": _o(dict(jacobi_scaling=0, initial_trust_region_radius=1.0, max_lm_diagonal=0.5)),
    "lm_diagonal_floor": _o(dict(min_lm_diagonal=10.0)),
    "max_iter_0": _o(dict(max_num_iterations=0), expect=NO_CONVERGENCE),
    "max_iter_1": _o(dict(max_num_iterations=1), expect=NO_CONVERGENCE),
    "max_iter_2": _o(dict(max_num_iterations=2), expect=NO_CONVERGENCE),
    "radius_tiny": _o(dict(initial_trust_region_radius=1e-4)),
    "radius_huge": _o(dict(initial_trust_region_radius=1e14)),
    # (every residual in Huber's linear part: the weights a / |r| leave a badly conditioned system, and each iteration
    # amplifies the rounding of the one before: three iterations keep every window within a tenth of the tolerances)
    "huber_tiny": _o(dict(huber_delta=1e-4, max_num_iterations=3)),
    "huber_huge": _o(dict(huber_delta=1e6, max_num_iterations=8)),
    "function": _o(dict(function_tolerance=0.5), expect=FUNCTION),
    "parameter": _o(lambda w: dict(parameter_tolerance=TUNED[w]["ptol"]), expect=PARAMETER, tuned="ptol"),
    "gradient": _o(dict(gradient_tolerance=1e9), expect=GRADIENT),
    # every step rejected (rho never exceeds 1.5) until the radius falls below the minimum
    "radius_min": _o(dict(min_relative_decrease=1.5, min_trust_region_radius=9e3), expect=RADIUS),
    "nan_uv": _o(poke="nan_uv", expect=FAILURE),
    "nan_point": _o(poke="nan_point", expect=FAILURE),
    "nan_camera": _o(poke="nan_camera", expect=FAILURE),
    # a negative LM diagonal at a fixed radius, without Jacobi scaling, anti-damps the system: strong, and the very first
    # factorisation fails; weaker, and steps are accepted until the damped system stops being positive definite
    "not_pd": _o(_negative_diagonal("not_pd", 1), expect=FAILURE, not_pd=True, tuned="not_pd"),
    "unusable_after_steps": _o(_negative_diagonal("unusable", 1), expect=FAILURE, moved=True, tuned="unusable"),
    # the same two where an invalid step is followed by another round (at a halved, here clamped, radius) before the exit
    "not_pd_3": _o(_negative_diagonal("not_pd", 3), expect=FAILURE, not_pd=True, tuned="not_pd"),
    "unusable_after_steps_3": _o(_negative_diagonal("unusable", 3), expect=FAILURE, moved=True, tuned="unusable"),
}
# the hard twins run these on every path (the exits and failures that can fall inside a speculated set, and the default
# solve with its rejected steps); SETS is what the local-window paths repeat with 1, 2, 3 and the maximum of radii
SETS = ("function", "radius_min", "max_iter_1", "max_iter_2", "not_pd", "unusable_after_steps")
HARD_OPTIONS = ("default",) + SETS


def applies(window_name, option_name):
    tuned = OPTIONS[option_name].get("tuned")
    return (tuned is None or tuned in TUNED[window_name]) and (window_name, option_name) not in EXCLUDED


# (window, option) pairs left out because the oracle itself is ill posed there (test_ba_cases_cpu.py: the schedule
# changes under a relative perturbation of 1e-13 of the input points), with the reason
_HUGE = "an initial radius of 1e14 leaves the first system undamped: 1e-13 on the input moves its step by more than the tolerances"
EXCLUDED = {(w, "radius_huge"): _HUGE for w in ("blocked", "generic", "no_free", "plain_hard")}
# (without a robust loss the outliers of the hard window make its rejected candidates cost 1e3 times the state's: the oracle
# and the dense restatement, both right, differ by 1e-8 on such a candidate's cost)
EXCLUDED["plain_hard", "huber_huge"] = "rejected candidates of cost 5e7 are evaluated to 1e-8 only"


# options every case of a class starts from (a case's own fields win).  GENERIC is a chain of 129 free cameras behind two
# fixed ones: its far end is held by products of relative poses, 1e-13 on the input moves the cameras by the whole
# tolerance of the GPU comparison after ten iterations, by less than a tenth of it after four
CLASS_OPT = {"generic": dict(max_num_iterations=4)}


def opt_of(window_name, option_name):
    o = OPTIONS[option_name]["opt"]
    return dict(CLASS_OPT.get(window_name.replace("_hard", ""), {}), **(o(window_name) if callable(o) else o))


def pairs(window_names, option_names=None):
    return [(w, o) for w in window_names for o in (option_names or OPTIONS) if applies(w, o)]


# ---------------------------------------------------------------------------------------------------------------- windows
def poke(w, kind):
    """One input value made non-finite (in a copy): an observation, a landmark or a camera that has observations."""
    w = dict(w)
    mid = len(w["obs_cam"]) // 2
    if kind == "nan_uv":
        w["obs_uv"] = w["obs_uv"].copy()
        w["obs_uv"][mid, 0] = np.nan
    elif kind == "nan_point":
        w["points"] = w["points"].copy()
        w["points"][len(w["points"]) // 2, 1] = np.nan
    elif kind == "nan_camera":
        w["cams"] = w["cams"].copy()
        w["cams"][int(w["obs_cam"][mid]), 4] = np.nan
    else:
        raise KeyError(kind)
    return w


def window(synth, window_name, option_name="default", seed_stream=0, **over):
    """The window of a (window, option) pair: built, without a free camera for the NO_FREE class, poked for the NaN cases."""
    w = synth.make_ba_window(**dict(WINDOWS[window_name], seed_stream=seed_stream, **over))
    if is_no_free(window_name):
        w["cam_free"] = np.zeros_like(w["cam_free"])
    kind = OPTIONS[option_name].get("poke")
    return poke(w, kind) if kind else w


def options(mod, opt):
    """rs_ba_options from mod.default_options() (mod = the oracle or the GPU bindings: same fields)."""
    o = mod.default_options()
    for k, v in opt.items():
        setattr(o, k, v)
    return o


def solve_oracle(O, w, opt):
    """cams, points, summary, trace of the oracle."""
    return O.bundle_adjust_trace(*ba_args(w), options=options(O, opt))


def solve_dense(D, O, w, opt):
    """dense_lm on the same problem: cams, points, summary, trace (the input state when unusable)."""
    o = options(O, opt)
    kw = {name: getattr(o, k) for k, name in DENSE_KW.items() if k in opt}
    prob = D.Problem(*ba_args(w), huber_a=o.huber_delta, imu=None)
    with np.errstate(all="ignore"):
        x, s, tr = D.solve(prob, **kw)
    if not s["usable"]:
        x = prob.pack(prob.cams0, prob.pts0)
    cams, pts = prob.unpack(x)
    return cams, pts, s, tr


def outcomes(trace):
    return "".join(LETTER[t["outcome"]] for t in trace)


# -------------------------------------------------------------------------------------------------------------- structure
def _drop_observations(w, keep):
    """The window with only the observations keep[o] (landmarks stay, possibly without any)."""
    pt = np.repeat(np.arange(len(w["points"])), np.diff(w["obs_ptr"]))
    ptr = np.zeros(len(w["points"]) + 1, np.int32)
    ptr[1:] = np.cumsum(np.bincount(pt[keep], minlength=len(w["points"])))
    return dict(w, obs_ptr=ptr, obs_cam=w["obs_cam"][keep].copy(), obs_uv=w["obs_uv"][keep].copy())


def _landmark_on_free_cameras(w):
    """A landmark all of whose observations are by free cameras, from the middle of the window."""
    pt = np.repeat(np.arange(len(w["points"])), np.diff(w["obs_ptr"]))
    fixed_seen = np.bincount(pt, weights=(w["cam_free"][w["obs_cam"]] == 0), minlength=len(w["points"]))
    cand = np.flatnonzero(fixed_seen == 0)
    return int(cand[len(cand) // 2])


def single_observation(w):
    """One landmark cut to its first observation."""
    p = _landmark_on_free_cameras(w)
    keep = np.ones(len(w["obs_cam"]), bool)
    keep[w["obs_ptr"][p] + 1:w["obs_ptr"][p + 1]] = False
    return _drop_observations(w, keep)


def fixed_cameras_only(w):
    """One landmark seen by the two fixed cameras only (it still moves: its own 3 x 3 block is all it takes part in)."""
    fixed = np.flatnonzero(w["cam_free"] == 0)[:2]
    pt = np.repeat(np.arange(len(w["points"])), np.diff(w["obs_ptr"]))
    seen_by_both = np.flatnonzero(np.bincount(pt, weights=np.isin(w["obs_cam"], fixed), minlength=len(w["points"])) == 2)
    p = int(seen_by_both[0])
    keep = ~((pt == p) & ~np.isin(w["obs_cam"], fixed))
    return _drop_observations(w, keep)


def far_behind(w):
    """One landmark far behind the cameras that see it (its projection flips sign; the depth is -1000 or so)."""
    p = _landmark_on_free_cameras(w)
    pts = w["points"].copy()
    c = int(w["obs_cam"][w["obs_ptr"][p]])
    centre = w["cams"][c, 3:]
    pts[p] = centre - 100.0 * (pts[p] - centre)
    return dict(w, points=pts)


def free_camera_unobserved(w):
    """The last free camera loses every observation (landmarks it alone kept above two sightings keep the others)."""
    c = int(np.flatnonzero(w["cam_free"])[-1])
    return _drop_observations(w, w["obs_cam"] != c)


STRUCTURE = {"single_observation": single_observation, "fixed_cameras_only": fixed_cameras_only, "far_behind": far_behind,
             "free_camera_unobserved": free_camera_unobserved}
STRUCTURE_WINDOWS = ("plain", "blocked")
# the header: non-free points "are not passed" — for these the library may equal the oracle or refuse with RS_ERR_INVALID
MAY_REFUSE = ("single_observation", "fixed_cameras_only")


def structure_window(synth, window_name, edit):
    return STRUCTURE[edit](window(synth, window_name))


# ---------------------------------------------------------------------------------------------------------------- batches
# A batch window: dict(base = a name of WINDOWS, make_ba_window arguments that differ, poke, at_optimum = the window
# starts where the oracle's solve (default options, 50 iterations) ended, empty = a problem of the window's cameras and
# no landmark)
def _plain(n_points, seed_stream, **kw):
    return dict(base="plain", n_points=n_points, seed_stream=seed_stream, **kw)


_PLAINS = [_plain(300, 0), _plain(260, 1), _plain(220, 2), _plain(180, 3), _plain(140, 4)]
_MIXED = _PLAINS + [dict(base="plain_hard"), _plain(200, 5, poke="nan_uv"), _plain(240, 6, at_optimum=True)]
# the diagonal of mixed_exits_not_pd: inside the "unusable" interval of both plain and plain_hard (TUNED), so some windows
# fail after accepted steps and some at once, and every invalid step is followed by two more rounds
_MIXED_NOT_PD = dict(min_lm_diagonal=-2.5e-4, max_lm_diagonal=-2.5e-4, initial_trust_region_radius=1.0, max_trust_region_radius=1.0,
                     max_num_consecutive_invalid_steps=3, max_num_iterations=20, jacobi_scaling=0)
# grid: whether rs_bundle_adjust_batch's grid form (ba_batch_mode 0) runs the batch or declines it to the lanes
BATCHES = {
    "mixed_exits": dict(windows=_MIXED, opt=dict(function_tolerance=1e-3), grid=True),
    "mixed_exits_not_pd": dict(windows=_MIXED, opt=_MIXED_NOT_PD, grid=True),
    "with_big_window": dict(windows=_PLAINS[:3] + [dict(base="blocked")], opt={}, grid=False),
    "max_iter_0": dict(windows=_PLAINS[:3], opt=dict(max_num_iterations=0), grid=False),
    "with_empty_window": dict(windows=_PLAINS[:2] + [_plain(0, 0, empty=True)] + _PLAINS[2:3], opt={}, grid=False),
}


def batch_window(synth, O, spec):
    spec = dict(spec)
    base, kind, at_optimum, empty = spec.pop("base"), spec.pop("poke", None), spec.pop("at_optimum", False), spec.pop("empty", False)
    if empty:
        w = window(synth, base)
        return dict(w, points=np.zeros((0, 3)), obs_ptr=np.zeros(1, np.int32), obs_cam=np.zeros(0, np.int32),
                    obs_uv=np.zeros((0, 2), np.float32))
    w = window(synth, base, **spec)
    if at_optimum:
        c, p, s, _ = solve_oracle(O, w, dict(max_num_iterations=50))
        assert s["usable"] and s["termination"] in (FUNCTION, PARAMETER, GRADIENT)
        w = dict(w, cams=c, points=p)
    return poke(w, kind) if kind else w
