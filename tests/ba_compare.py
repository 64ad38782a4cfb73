"""The contract between a GPU bundle adjustment and the oracle's solve of the same problem, shared by the envelope files
(tests/test_gpu_inertial_ba_envelope.py, tests/test_gpu_ba_envelope.py): the schedule exactly, values within the tolerances
of test_gpu_parity.py::test_bundle_adjust_inertial.  TOL names every tolerance once; `scale` tightens all of them together
(tests/test_ba_cases_cpu.py asks the oracle to reproduce itself within a tenth of them under a perturbed input)."""
import numpy as np

SCHEDULE = ("iterations", "successful_steps", "termination", "usable")
TRACE = (("radius", 1e-7), ("cost", 1e-9), ("candidate_cost", 1e-6), ("model_cost_change", 1e-6), ("x_norm", 1e-6))
TOL = dict(initial_cost=1e-12, final_cost=1e-8, cams=(1e-7, 1e-9), points=(1e-6, 1e-7), velocity=(1e-7, 1e-9), bias=(1e-6, 1e-9))


def close(a, b, rtol, atol=0.0):
    return np.allclose(a, b, rtol=rtol, atol=atol, equal_nan=True)


def assert_same_summary(s, cams, points, ref, scale=1.0, initial=True):
    """Summary and state against ref = (cams, points, summary): what a solve without a trace (a batch) can be held to.
    initial=False leaves the initial cost out (for two solves whose inputs differ on purpose)."""
    rc, rp, rs_ = ref
    assert tuple(s[k] for k in SCHEDULE) == tuple(rs_[k] for k in SCHEDULE)
    assert not initial or close(s["initial_cost"], rs_["initial_cost"], scale * TOL["initial_cost"])
    assert close(s["final_cost"], rs_["final_cost"], scale * TOL["final_cost"])
    assert close(cams, rc, scale * TOL["cams"][0], scale * TOL["cams"][1])
    assert close(points, rp, scale * TOL["points"][0], scale * TOL["points"][1])


def assert_same_trace(tr, otr, scale=1.0):
    assert [t["outcome"] for t in tr] == [t["outcome"] for t in otr]
    for k, tol in TRACE:
        assert close([t[k] for t in tr], [t[k] for t in otr], scale * tol), k


def assert_same_solve(g, ref, scale=1.0, initial=True):
    """g = dict(s summary, tr trace, c cameras, p points[, v velocity, b bias]) against ref = (cams, points, velocity, bias,
    summary, trace); velocity / bias None for a vision-only solve."""
    rc, rp, rv, rb, rs_, otr = ref
    assert tuple(g["s"][k] for k in SCHEDULE) == tuple(rs_[k] for k in SCHEDULE)
    assert_same_trace(g["tr"], otr, scale)
    assert_same_summary(g["s"], g["c"], g["p"], (rc, rp, rs_), scale, initial)
    if rv is not None:
        assert close(g["v"], rv, scale * TOL["velocity"][0], scale * TOL["velocity"][1])
        assert close(g["b"], rb, scale * TOL["bias"][0], scale * TOL["bias"][1])
