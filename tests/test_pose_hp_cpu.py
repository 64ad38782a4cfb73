"""The relative-pose restatement tests/essential_ref.py against the independent high-precision checks of
tests/pose_hp.py, on the scenes of tests/pose_cases.py.  No GPU.

Root level: the real roots of each sample's f64 degree-10 determinant against mpmath at 50 digits, on every motion.
Model level: every emitted model is an essential matrix that satisfies its own sample, and a noise-free, outlier-free
sample yields the true E.  Scores: the integer count equals a literal f64 Sampson count.  Known rotation: the refit t
against the f64 SVD of the inlier constraint stack and against ground truth at a 30 degree rotation."""
import functools

import numpy as np
import pytest

import essential_ref as R
import pose_cases as PC
import pose_hp as HP

S = 100                  # random 5-point samples per scene


@functools.lru_cache(maxsize=None)
def _samples(motion, K=None):
    d = PC.synth().make_pose_pair(3, 1000, 0.0, 0.0, motion, K=K)
    x1, y1 = R.normalise(d["pts_from"], d["K"])
    x2, y2 = R.normalise(d["pts_to"], d["K"])
    rng = np.random.default_rng(0)
    idx = np.array([rng.choice(1000, 5, replace=False) for _ in range(S)])
    return d, [a[idx] for a in (x1, y1, x2, y2)]


@functools.lru_cache(maxsize=None)
def _solve(motion, K=None):
    d, smp = _samples(motion, K)
    N, _ = R.null_basis(*smp)
    C, _ = R._gauss_jordan(R.constraint_matrix(N), 10)
    poly = R.det_poly(*R.b_matrix(C))
    z, nr = R.real_roots(poly)
    models, cnt = R.five_point(*smp)
    return poly, z, nr, models, cnt


_SCENES = [(m, None) for m in PC.MOTIONS] + [("forward", (650.0, 760.0, 590.0, 410.0)), ("forward", (150.0, 152.0, 640.0, 360.0)),
                                             ("sideways", (3000.0, 2990.0, 600.0, 380.0))]


@pytest.mark.parametrize("motion,K", _SCENES)
def test_real_roots_match_mpmath(motion, K):
    """No spurious root, no missed root (outside clusters closer than pose_hp.CLUSTER_GAP; none occur on these
    scenes), each within 1e-6 relative of mpmath's.  Before the derivative cascade the Sturm finder had, on 300
    samples: forward 11 spurious / 19 missed, small 97 / 270, planar 291 / 476."""
    poly, z, nr, _, _ = _solve(motion, K)
    spurious = missed = 0
    for s in range(S):
        sp, mi = HP.match_roots(list(z[s, :nr[s]]), poly[s])
        spurious += sp
        missed += mi
    assert (spurious, missed) == (0, 0)
    assert np.isnan(z[np.arange(10)[None, :] >= nr[:, None]]).all()
    assert (np.diff(z, axis=1)[np.arange(9)[None, :] < nr[:, None] - 1] > 0).all()      # ascending, distinct


def test_real_roots_of_constructed_polynomials():
    """Roots of large magnitude and of both signs, a trimmed leading coefficient, no real root at all."""
    cases = [[-270.0, -38.1, -12.2, 22.2, 38.0, 46.9], [1e-3, 2e-3, 5.0, 300.0, -1e4], [-0.5, 0.25, 7.0]]
    for rts in cases:
        c = np.polynomial.polynomial.polyfromroots(rts)
        c = np.r_[c, np.zeros(11 - len(c))] if len(c) < 11 else c
        z, nr = R.real_roots(c[None])
        assert nr[0] == len(rts)
        assert np.allclose(z[0, :nr[0]], np.sort(rts), rtol=1e-9, atol=1e-12)
    c = np.polynomial.polynomial.polyfromroots([1.0, 2.0, 3.0])
    z, nr = R.real_roots(np.r_[c, np.zeros(7)][None] * np.r_[np.ones(4), np.zeros(7)][None])
    assert nr[0] == 3
    z, nr = R.real_roots(np.array([[1.0, 0, 2.0, 0, 1.0, 0, 0, 0, 0, 0, 0]]))     # (z^2 + 1)^2
    assert nr[0] == 0
    z, nr = R.real_roots(np.zeros((1, 11)))
    assert nr[0] == 0


# samples without the true E among their models, on S = 100 samples per scene (noise-free, outlier-free).  Before the
# fix, on the issue's 300 samples: forward 4, sideways 2, small 96, rotation 234, planar 98.
#   sideways   the true z is a near-double root that the f64 coefficients turn into a complex pair (97.0 +- 1.2 i)
#   small      a 2 cm baseline against 4 .. 40 m depths: the 10 x 10 elimination is ill-conditioned (cond ~1e9)
#   rotation   a 1 mm baseline: nearly every E = [t]x R fits, the true one is not singled out
#   planar     3 of 100: the plane's second solution is found, the true E is lost in the ill-conditioned elimination
# (the sideways sample above is one of the issue's 300, not of these 100).  Recorded, held as ceilings:
NO_TRUE_E = {"forward": 0, "sideways": 0, "small": 16, "rotation": 73, "planar": 3}
# models dropped by the identity check (ESS_EPS) on those samples, recorded, held as ceilings
DROPPED = {"forward": 3, "sideways": 0, "small": 34, "rotation": 98, "planar": 6}


@pytest.mark.parametrize("motion", PC.MOTIONS)
def test_models_are_essential_and_contain_the_true_E(motion, monkeypatch):
    d, smp = _samples(motion)
    _, _, _, models, cnt = _solve(motion)
    Et = HP.true_E(d["R"], d["t"])
    worst = [0.0, 0.0, 0.0]
    nohit = 0
    for s in range(S):
        for m in range(cnt[s]):
            c = HP.essential_checks(models[s, m], *(a[s] for a in smp))
            worst = [max(w, v) for w, v in zip(worst, c)]
        nohit += not any(HP.dist_up_to_sign(models[s, m], Et) < 1e-3 for m in range(cnt[s]))
    # recorded maxima over the five motions: det 4.6e-7, cubic 9.7e-7 (the filter's bound is 1e-6), epipolar 7.9e-14
    assert worst[0] < 1e-6 and worst[1] <= 1.01e-6 and worst[2] < 1e-12, worst
    assert nohit <= NO_TRUE_E[motion], nohit
    monkeypatch.setattr(R, "ESS_EPS", np.inf)
    _, cnt_all = R.five_point(*smp)
    assert int((cnt_all - cnt).sum()) <= DROPPED[motion]


@pytest.mark.parametrize("name", ["forward", "sideways", "planar", "fx_ne_fy", "focal150", "focal3000", "epipole", "thr0.25",
                                  "thr20.0", "n8", "n65"])
def test_scores_are_literal_sampson_counts(name):
    case = PC.CASES[name]
    d = PC.scene(case)
    pf, pt, K, count, max_n, kw = PC.call_args(case, d)
    n = min(count, max_n)
    ref = R.estimate_pose(pf[:n], pt[:n], K, threshold_px=kw["threshold_px"], confidence=kw["confidence"],
                          max_hypotheses=kw["max_hypotheses"], seed=kw["seed"], stages=True)
    for h in range(ref["drawn"]):
        for m in range(ref["nmodels"][h]):
            c, near = HP.sampson_count(ref["models"][h, m], pf[:n], pt[:n], K, kw["threshold_px"])
            assert abs(int(ref["scores"][h, m]) - c) <= near, (h, m)
    if ref["status"] == 0:
        c, near = HP.sampson_count(ref["E"], pf[:n], pt[:n], K, kw["threshold_px"])
        assert abs(ref["count"] - c) <= near
        assert ref["count"] >= int(ref["scores"].max())                          # LO never lowers the count
        assert HP.essential_checks(ref["E"])[1] < 1e-12
    if case["scene"].get("epipole_points"):
        # true matches on the epipoles: the estimated E leaves a denominator of ~1e-8 there, not 0, and keeps them
        assert ref["inlier"][-case["scene"]["epipole_points"]:].all()


@pytest.mark.parametrize("name", ["forward", "sideways", "fx_ne_fy", "focal3000", "epipole"])
def test_noisy_scenes_recover_the_motion(name):
    case = PC.CASES[name]
    d = PC.scene(case)
    pf, pt, K, _, _, kw = PC.call_args(case, d)
    ref = R.estimate_pose(pf, pt, K, **kw)
    assert ref["status"] == 0
    assert HP.dist_up_to_sign(ref["E"], HP.true_E(d["R"], d["t"])) < 0.02


@pytest.mark.parametrize("name", ["kr_rot30", "kr_fx_ne_fy", "kr_iter200"])
def test_known_rotation_refit_against_the_svd(name):
    case = PC.KR_CASES[name]
    d = PC.scene(case)
    n = len(d["pts_from"])
    Rm = d["R"].astype(np.float32)
    ref = R.estimate_pose_known_rotation(d["pts_from"], d["pts_to"], d["K"], Rm, PC.kr_pairs(case, n))
    assert ref["status"] == 0
    t_svd = HP.refit_translation(d["pts_from"], d["pts_to"], d["K"], Rm, ref["inlier"])
    # the f32 smallest eigenvector of the f64 normal matrix against the f64 SVD: recorded <= 2e-7
    assert HP.dist_up_to_sign(ref["t_refit"], t_svd) < 1e-5
    t = ref["pose"][:3, 3].astype(np.float64)
    ang = np.degrees(np.arccos(np.clip(t @ d["t"] / np.linalg.norm(t), -1, 1)))
    assert ang < 1.0, ang
    if name == "kr_rot30":
        # a transposed R must not fit: with R^T the best support collapses
        bad = R.estimate_pose_known_rotation(d["pts_from"], d["pts_to"], d["K"], Rm.T.copy(), PC.kr_pairs(case, n))
        assert bad["count"] < ref["count"] // 4
