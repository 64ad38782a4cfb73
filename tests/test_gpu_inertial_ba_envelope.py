"""rs_bundle_adjust_inertial on the GPU against the oracle over the cases of tests/inertial_cases.py (which
tests/test_inertial_ba_cpu.py pins the oracle on against dense_lm), in both solve paths:
  imu mode 0  the velocity / bias blocks eliminated around the LDS reduced solve (csrc/ba_imu.hip: K6a, K6b, K7i) where
              ba_solve_impl's gate allows it, the N x N blocked solve elsewhere
  imu mode 1  always the N x N blocked solve (ba_launch_reduced_solve_inertial, csrc/ba_solve_big.hip)
The path a solve takes is read from the launch profile, so that a change to the gate cannot quietly skip a case.  Also:
1 .. 3 speculative radii on the windows of 19 .. 21 optimised cameras, vision-only controls at those sizes, and factors the
library refuses."""
import ctypes as C

import numpy as np
import pytest

import inertial_cases as IC
from ba_compare import assert_same_solve as _assert_same_solve      # (the contract shared with test_gpu_ba_envelope.py)
from conftest import to_np

pytestmark = pytest.mark.gpu

LDS, BIG = "K6i_imu_eliminate", "K7_ba_reduced_solve_inertial"
INERTIAL = [k for k, c in IC.CASES.items() if c["imu"] is not None]
VISION = [k for k, c in IC.CASES.items() if c["imu"] is None]
SETS = [(k, ns) for k, c in IC.CASES.items() if c.get("sets") for ns in (1, 2, 3)]

_ORACLE = {}


def _problem(synth, oracle, name):
    """window, imu, oracle result of a case (the oracle runs once per case and session)."""
    if name not in _ORACLE:
        case = IC.CASES[name]
        w = IC.window(synth, case)
        m = IC.imu(synth, w, case)
        _ORACLE[name] = (w, m, IC.solve_oracle(oracle, w, m, case))
    return _ORACLE[name]


def _gpu(ctx, rs, w, m, case, mode=0, sets=0):
    ctx.set_int("ba_imu_mode", mode)
    ctx.set_int("ba_speculative_sets", sets)
    try:
        dc, dp = ctx.dev(w["cams"]), ctx.dev(w["points"])
        args = (dc, w["cam_free"], dp, ctx.dev(w["obs_ptr"]), ctx.dev(w["obs_cam"]), ctx.dev(w["obs_uv"]), w["K"])
        o = IC.options(rs, case)
        ctx.prof_begin()
        try:
            if m is None:
                s, v, b = ctx.bundle_adjust(*args, options=o), None, None
            else:
                s, v, b = ctx.bundle_adjust_inertial(*args, m, options=o)
        finally:
            prof = ctx.prof_end()
        return dict(s=s, tr=ctx.ba_trace(), c=to_np(dc), p=to_np(dp), v=v, b=b, prof=prof, stats=ctx.ba_stats())
    finally:
        ctx.set_int("ba_imu_mode", 0)
        ctx.set_int("ba_speculative_sets", 0)


def _assert_path(g, want):
    """want: "lds", "big" or None (vision-only: neither inertial solve).  The first round is always enqueued, so even a
    solve that ends before its first iteration (gradient, non-finite cost) shows the path it took."""
    lds, big = LDS in g["prof"], BIG in g["prof"]
    if want is None:
        assert not lds and not big, g["prof"]
    elif want == "lds":
        assert lds and not big, g["prof"]
    else:
        assert big and not lds, g["prof"]


def _assert_untouched_where_due(g, w, m):
    """Fixed frames and frames without an inertial block keep velocity / bias bit for bit; an unusable solve leaves
    cameras, points, velocities and biases as they went in."""
    keep = np.ones(len(w["cams"]), bool)
    keep[m["cam_i"]] = False
    keep[m["cam_j"]] = False
    assert g["v"][keep].tobytes() == m["cam_velocity"][keep].tobytes()
    assert g["b"][keep].tobytes() == m["cam_bias"][keep].tobytes()
    fixed = np.asarray(w["cam_free"]) == 0
    assert g["c"][fixed].tobytes() == w["cams"][fixed].tobytes()
    if not g["s"]["usable"]:
        assert g["c"].tobytes() == w["cams"].tobytes() and g["p"].tobytes() == w["points"].tobytes()
        assert g["v"].tobytes() == np.asarray(m["cam_velocity"], np.float64).tobytes()
        assert g["b"].tobytes() == np.asarray(m["cam_bias"], np.float64).tobytes()


@pytest.mark.parametrize("name", INERTIAL)
def test_inertial_case_in_both_modes(ctx, rs, oracle, synth, name):
    case = IC.CASES[name]
    w, m, ref = _problem(synth, oracle, name)
    if "expect" in case:
        assert ref[4]["termination"] == case["expect"]
    if case.get("moved"):
        assert ref[4]["successful_steps"] >= 1 and not ref[4]["usable"]
    runs = {}
    for mode in (0, 1):
        g = runs[mode] = _gpu(ctx, rs, w, m, case, mode)
        _assert_path(g, case["path0"] if mode == 0 else "big")
        _assert_same_solve(g, ref)
        _assert_untouched_where_due(g, w, m)
    # the two solve paths agree with each other as closely as each agrees with the oracle
    g0, g1 = runs[0], runs[1]
    _assert_same_solve(g1, (g0["c"], g0["p"], g0["v"], g0["b"], g0["s"], g0["tr"]))


@pytest.mark.parametrize("name", VISION)
def test_vision_control(ctx, rs, oracle, synth, name):
    """The windows of 19 .. 21 optimised cameras without factors (K5 / K7 / K8 only): a mismatch in the inertial cases of
    the same size that shows here too is not K6's."""
    case = IC.CASES[name]
    w, m, ref = _problem(synth, oracle, name)
    g = _gpu(ctx, rs, w, m, case)
    _assert_path(g, None)
    _assert_same_solve(g, ref)


@pytest.mark.parametrize("name,ns", SETS)
def test_speculative_sets(ctx, rs, oracle, synth, name, ns):
    """1 .. 3 trust-region radii per round on the local-window path (one K6b / K7i workgroup per radius): the per-iteration
    record is the oracle's whatever the number; max_num_iterations clamps the number of sets."""
    case = IC.CASES[name]
    w, m, ref = _problem(synth, oracle, name)
    g = _gpu(ctx, rs, w, m, case, 0, ns)
    _assert_path(g, case["path0"])
    _assert_same_solve(g, ref)
    _assert_untouched_where_due(g, w, m)
    st = g["stats"]
    max_iter = case["opt"].get("max_num_iterations", 10)
    assert st["set_evaluations"] <= min(ns, max_iter) * st["rounds"]
    # the first round evaluates one radius, the second min(sets, iterations left) of them (s.nact, ba_common.h)
    second = min(ns, max_iter - 1)
    if second <= 1:
        assert st["rounds"] == st["set_evaluations"] == g["s"]["iterations"], st
    else:       # K6b / K7i ran more than one workgroup (one per radius) in at least one round
        assert g["s"]["iterations"] >= 2 and st["set_evaluations"] > st["rounds"], st


def _raw_inertial(ctx, rs, w, m, dc, dp, vel, bias):
    cam_free = np.ascontiguousarray(w["cam_free"], np.uint8)
    Kc = (C.c_float * 4)(*[float(v) for v in w["K"]])
    g = np.ascontiguousarray(m["gravity"], np.float64)
    arr, nf = rs.imu_factor_array(m)
    s = rs.BaSummary()
    keep = [ctx.dev(w["obs_ptr"]), ctx.dev(w["obs_cam"]), ctx.dev(w["obs_uv"])]
    return ctx.lib.rs_bundle_adjust_inertial(
        ctx.h, len(w["cams"]), len(w["points"]), len(w["obs_cam"]), C.c_void_p(dc.data_ptr()),
        cam_free.ctypes.data_as(C.c_void_p), C.c_void_p(dp.data_ptr()), *[C.c_void_p(t.data_ptr()) for t in keep], Kc,
        vel.ctypes.data_as(C.c_void_p), bias.ctypes.data_as(C.c_void_p), arr, nf, g.ctypes.data_as(C.c_void_p), None,
        C.byref(s))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bad", ["fixed_i", "fixed_j", "same", "out_of_range", "negative"])
def test_refused_factors_leave_everything_untouched(ctx, rs, synth, bad, mode):
    """A factor must join two distinct optimised cameras of the window: anything else is refused before any work, and
    cameras, points, velocities and biases come back bit for bit."""
    w = IC.window(synth, IC.CASES["fixed_middle"])
    m = synth.make_imu(w, pairs=[(2, 3), (3, 4), (6, 7)])
    f = dict(m, cam_i=m["cam_i"].copy(), cam_j=m["cam_j"].copy())
    if bad == "fixed_i":
        f["cam_i"][1] = 5                   # the fixed camera in the middle
    elif bad == "fixed_j":
        f["cam_j"][2] = 1
    elif bad == "same":
        f["cam_j"][1] = f["cam_i"][1]
    elif bad == "out_of_range":
        f["cam_j"][2] = len(w["cams"])
    else:
        f["cam_i"][0] = -1
    vel, bias = np.array(m["cam_velocity"], np.float64), np.array(m["cam_bias"], np.float64)
    dc, dp = ctx.dev(w["cams"]), ctx.dev(w["points"])
    ctx.set_int("ba_imu_mode", mode)
    try:
        rc = _raw_inertial(ctx, rs, w, f, dc, dp, vel, bias)
    finally:
        ctx.set_int("ba_imu_mode", 0)
    assert rc != 0
    assert to_np(dc).tobytes() == w["cams"].tobytes() and to_np(dp).tobytes() == w["points"].tobytes()
    assert vel.tobytes() == m["cam_velocity"].tobytes() and bias.tobytes() == m["cam_bias"].tobytes()
    # the same window with its valid factors still solves (the refusal left no state behind)
    g = _gpu(ctx, rs, w, m, dict(opt={}), mode)
    assert g["s"]["usable"] == 1
