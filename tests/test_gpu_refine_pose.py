"""refine_pose on the GPU (K11: ba_refine_pose / ba_refine_pose_inertial, csrc/refine_pose.hip) against the oracle over the cases of
tests/refine_cases.py — which tests/test_refine_pose_cpu.py pins the oracle on against dense_lm — plus the ABI's
disabled-constraint, argument and context-state contracts."""
import ctypes as C

import numpy as np
import pytest

import refine_cases as RC

pytestmark = pytest.mark.gpu

SCHEDULE = ("termination", "iterations", "successful_steps", "usable")



def gpu_solve(ctx, rs, p, case):
    o = RC.options(rs, case)
    dp, duv = ctx.dev(p["points"]), ctx.dev(p["uv"])
    if p["prior"] is None and p["delta"] is None:
        cam, s = ctx.refine_pose(p["cam0"], dp, duv, p["K"], options=o)
        return cam, None, s
    cam, vel, s = ctx.refine_pose_inertial(p["cam0"], dp, duv, p["K"], prior=p["prior"], delta=p["delta"], options=o)
    return cam, (vel if p["delta"] is not None else None), s


def assert_matches(s, ref_s, cam, ref_cam, vel=None, ref_vel=None):
    assert tuple(s[k] for k in SCHEDULE) == tuple(ref_s[k] for k in SCHEDULE)
    for k in ("initial_cost", "final_cost"):
        if np.isfinite(ref_s[k]):
            # atol: exactly determined scenes (n = 1, 2) end at a cost of rounding noise (1e-22 .. 1e-15), where no relative
            # tolerance holds; the largest gap measured there is 4e-25 x the initial cost
            assert np.isclose(s[k], ref_s[k], rtol=1e-9, atol=1e-20 * ref_s["initial_cost"]), k
        else:       # a point at depth 0: the kernel's reciprocal gives NaN where the oracle's division gives inf
            assert not np.isfinite(s[k]), k
    assert np.isclose(s["final_radius"], ref_s["final_radius"], rtol=1e-7, atol=0)
    assert np.allclose(cam, ref_cam, rtol=1e-7, atol=1e-9)
    if ref_vel is not None:
        assert np.allclose(vel, ref_vel, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_refine_pose_matches_oracle(name, ctx, rs, oracle, synth):
    case = RC.CASES[name]
    p = RC.problem(synth, case)
    ref_cam, ref_vel, ref_s = RC.solve_oracle(oracle, p, case)
    if case.get("moved"):
        assert ref_s["successful_steps"] >= 1 and ref_s["usable"] == 0
    if "expect" in case:
        assert ref_s["termination"] == case["expect"]
    cam, vel, s = gpu_solve(ctx, rs, p, case)
    assert_matches(s, ref_s, cam, ref_cam, vel, ref_vel)
    if not s["usable"]:         # not usable: the inputs come back untouched, bit for bit
        assert cam.tobytes() == np.asarray(p["cam0"], np.float64).tobytes()
        if vel is not None:
            assert vel.tobytes() == np.asarray(p["delta"]["velocity"], np.float64).tobytes()


# ---------------------------------------------------------------- raw ABI calls
def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw_refine(ctx, rs, cam, dp, duv, n, K, options=None, summary=None):
    s = summary if summary is not None else rs.BaSummary()
    Kc = None if K is None else (C.c_float * 4)(*[float(v) for v in K])
    rc = ctx.lib.rs_refine_pose(ctx.h, _vp(cam), None if dp is None else C.c_void_p(dp.data_ptr()),
                                None if duv is None else C.c_void_p(duv.data_ptr()), int(n), Kc,
                                None if options is None else C.byref(options), C.byref(s))
    return rc, s


def raw_inertial(ctx, rs, cam, dp, duv, n, K, kind, pred=None, sigma=0.0, delta=None, vel=None, options=None, summary=None,
                 drop=()):
    """rs_refine_pose_inertial with every pointer explicit; `drop` names pointers passed as null."""
    s = summary if summary is not None else rs.BaSummary()
    Kc = (C.c_float * 4)(*[float(v) for v in K])
    keep = {}
    if delta is not None:
        keep["farr"], _ = rs.imu_factor_array(delta["imu"])
        for k in ("prev_pose", "prev_velocity", "prev_bias"):
            keep[k] = np.ascontiguousarray(delta[k], np.float64)
        keep["gravity"] = np.ascontiguousarray(delta["imu"]["gravity"], np.float64)
    ptr = lambda k: None if (k in drop or k not in keep) else (keep[k] if k == "farr" else _vp(keep[k]))   # noqa: E731
    if pred is not None:
        keep["pred"] = np.ascontiguousarray(pred, np.float64)
    pr = None if (pred is None or "predicted" in drop) else _vp(keep["pred"])
    rc = ctx.lib.rs_refine_pose_inertial(ctx.h, _vp(cam), C.c_void_p(dp.data_ptr()), C.c_void_p(duv.data_ptr()), int(n), Kc,
                                         int(kind), pr, C.c_double(sigma), ptr("prev_pose"), ptr("prev_velocity"),
                                         ptr("prev_bias"), ptr("farr"), ptr("gravity"),
                                         None if (vel is None or "velocity" in drop) else _vp(vel),
                                         None if options is None else C.byref(options), C.byref(s))
    return rc, s


def _bytes(s):
    return bytes(memoryview(s))


def test_disabled_constraints_equal_plain_refine(ctx, rs, synth):
    """RotationPrior::enabled / InertialDelta::enabled: a null predicted rotation, sigma <= 0 (or NaN), a null delta and a
    delta of duration <= 0 are no constraint — camera, velocity and summary byte-equal to rs_refine_pose."""
    p = synth.make_refine_problem(n=700, seed=40, noise_px=0.5, outlier_frac=0.1, imu=True)
    n = len(p["points"])
    dp, duv = ctx.dev(p["points"]), ctx.dev(p["uv"])
    cam_ref = p["cam0"].copy()
    rc, s_ref = raw_refine(ctx, rs, cam_ref, dp, duv, n, p["K"])
    assert rc == 0 and s_ref.usable == 1 and not np.array_equal(cam_ref, p["cam0"])
    R = synth.rodrigues(p["cam_true"][:3])
    d = p["delta"]
    variants = [dict(kind=1, pred=None, sigma=1e-3), dict(kind=1, pred=R, sigma=0.0), dict(kind=1, pred=R, sigma=-1.0),
                dict(kind=1, pred=R, sigma=float("nan")),
                dict(kind=2, delta=d, drop=("farr",))]
    for dur in (0.0, -0.5):
        f = dict(d["imu"], duration=np.array([dur]))
        variants.append(dict(kind=2, delta=dict(d, imu=f)))
    for kw in variants:
        cam = p["cam0"].copy()
        vel = np.array(d["velocity"], np.float64)
        rc, s = raw_inertial(ctx, rs, cam, dp, duv, n, p["K"], vel=vel, **kw)
        assert rc == 0, kw
        assert cam.tobytes() == cam_ref.tobytes(), kw
        assert _bytes(s) == _bytes(s_ref), kw
        assert vel.tobytes() == np.asarray(d["velocity"], np.float64).tobytes(), kw     # a disabled delta frees no velocity


def test_refused_arguments_leave_a_zeroed_summary(ctx, rs, synth):
    p = synth.make_refine_problem(n=100, seed=41, imu=True)
    n = len(p["points"])
    dp, duv = ctx.dev(p["points"]), ctx.dev(p["uv"])
    zero = _bytes(rs.BaSummary())

    def garbage():
        s = rs.BaSummary()
        s.termination, s.iterations, s.successful_steps, s.usable = 7, 9, 9, 1
        s.initial_cost, s.final_cost, s.final_radius = 1.0, 2.0, 3.0
        return s

    R = synth.rodrigues(p["cam_true"][:3])
    cases = [("n<0", lambda cam, s: raw_refine(ctx, rs, cam, dp, duv, -1, p["K"], summary=s)),
             ("null camera", lambda cam, s: raw_refine(ctx, rs, None, dp, duv, n, p["K"], summary=s)),
             ("null points", lambda cam, s: raw_refine(ctx, rs, cam, None, duv, n, p["K"], summary=s)),
             ("null uv", lambda cam, s: raw_refine(ctx, rs, cam, dp, None, n, p["K"], summary=s)),
             ("null intrinsics", lambda cam, s: raw_refine(ctx, rs, cam, dp, duv, n, None, summary=s)),
             ("kind 1, n<0", lambda cam, s: raw_inertial(ctx, rs, cam, dp, duv, -1, p["K"], 1, pred=R, sigma=1e-3, summary=s)),
             ("kind 2, n<0", lambda cam, s: raw_inertial(ctx, rs, cam, dp, duv, -1, p["K"], 2, delta=p["delta"],
                                                        vel=np.zeros(3), summary=s)),
             ("kind 3", lambda cam, s: raw_inertial(ctx, rs, cam, dp, duv, n, p["K"], 3, summary=s)),
             ("kind -1", lambda cam, s: raw_inertial(ctx, rs, cam, dp, duv, n, p["K"], -1, summary=s))]
    for k in ("prev_pose", "prev_velocity", "prev_bias", "gravity", "velocity"):
        cases.append((f"kind 2, null {k}", lambda cam, s, k=k: raw_inertial(ctx, rs, cam, dp, duv, n, p["K"], 2, delta=p["delta"],
                                                                          vel=np.zeros(3), drop=(k,), summary=s)))
    for what, call in cases:
        cam = p["cam0"].copy()
        s = garbage()
        rc, s = call(cam, s)
        assert rc != 0, what
        assert _bytes(s) == zero, what
        assert cam.tobytes() == p["cam0"].tobytes(), what
    # n == 0 is not an error: "nothing to constrain"
    cam = p["cam0"].copy()
    rc, s = raw_refine(ctx, rs, cam, dp, duv, 0, p["K"], summary=garbage())
    assert rc == 0 and _bytes(s) == zero and cam.tobytes() == p["cam0"].tobytes()


@pytest.fixture
def own_ctx(rs):
    c = rs.Context(0)
    yield c
    c.close()


def test_refine_after_bundle_adjust_clears_its_record(own_ctx, rs, oracle, synth):
    """rs_ba_get_cameras / rs_ba_get_trace are valid until the next optimisation call: a refine_pose ends them, and the
    next bundle adjustment on the same context (the pinned block reused) still equals the oracle."""
    ctx = own_ctx
    w = synth.make_ba_window(n_kf=5, n_points=150, run_max=4, config_id=5)
    C_ = len(w["cams"])

    def ba():
        dc = ctx.dev(w["cams"])
        s = ctx.bundle_adjust(dc, w["cam_free"], ctx.dev(w["points"]), ctx.dev(w["obs_ptr"]), ctx.dev(w["obs_cam"]),
                              ctx.dev(w["obs_uv"]), w["K"])
        return dc.cpu().numpy(), s

    rc_, rp_, rs_ = oracle.bundle_adjust(w["cams"], w["cam_free"], w["points"], w["obs_ptr"], w["obs_cam"], w["obs_uv"], w["K"])
    cams, s = ba()
    assert s["usable"] == rs_["usable"] == 1 and np.allclose(cams, rc_, rtol=1e-7, atol=1e-9)
    out = np.zeros((C_, 6))
    ctx.ba_cameras(out)
    assert np.array_equal(out, cams)
    assert len(ctx.ba_trace()) == s["iterations"] > 0
    for kind in (0, 1, 2):
        case = RC._c(dict(n=300, seed=50 + kind, imu=kind == 2), prior=(1e-3, 0.01) if kind == 1 else None, delta=kind == 2)
        p = RC.problem(synth, case)
        ref = RC.solve_oracle(oracle, p, case)
        cam, vel, s2 = gpu_solve(ctx, rs, p, case)
        assert_matches(s2, ref[2], cam, ref[0], vel, ref[1])
        with pytest.raises(rs.RsError):
            ctx.ba_cameras(out)
        assert ctx.ba_trace() == []
        cams2, s3 = ba()
        assert tuple(s3[k] for k in SCHEDULE) == tuple(rs_[k] for k in SCHEDULE)
        assert np.isclose(s3["final_cost"], rs_["final_cost"], rtol=1e-9)
        assert np.allclose(cams2, rc_, rtol=1e-7, atol=1e-9)
        ctx.ba_cameras(out)
        assert np.array_equal(out, cams2) and len(ctx.ba_trace()) == s3["iterations"]


def test_refine_on_a_non_default_stream(own_ctx, rs, oracle, synth):
    """A context moved to a stream of its own, inputs written on that stream: the same bytes as on the default stream."""
    import torch
    ctx = own_ctx
    for kind in (0, 2):
        case = RC._c(dict(n=1500, seed=60 + kind, noise_px=0.5, outlier_frac=0.2, imu=kind == 2), delta=kind == 2)
        p = RC.problem(synth, case)
        ctx.use_stream(torch.cuda.current_stream())
        cam0, vel0, s0 = gpu_solve(ctx, rs, p, case)
        st = torch.cuda.Stream()
        try:
            with torch.cuda.stream(st):
                ctx.use_stream(st)
                cam1, vel1, s1 = gpu_solve(ctx, rs, p, case)
        finally:
            ctx.use_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert s0 == s1
        assert cam0.tobytes() == cam1.tobytes()
        if kind == 2:
            assert vel0.tobytes() == vel1.tobytes()
        ref = RC.solve_oracle(oracle, p, case)
        assert_matches(s1, ref[2], cam1, ref[0], vel1, ref[1])
