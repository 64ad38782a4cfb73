"""The relative-pose stage on the GPU (csrc/pose.hip: rs_pose_estimator_*, rs_estimate_pose,
rs_estimate_pose_known_rotation) against the CPU restatement tests/essential_ref.py, stage by stage and as a whole.

Sample indices, model counts and cheirality counts are integers and compared for equality.  Models agree to 1e-9
relative (up to sign).  A score may differ from the restatement only by the points whose squared Sampson error lies
within 1e-9 relative of t^2 (the slack is counted from the restatement).  The restatement sums the LO normal matrix in
the kernel's fixed order, so the final E agrees to 1e-9 and the final mask up to the same near-threshold points.
"""
import functools
import importlib

import numpy as np
import pytest

import essential_ref as R
from conftest import to_np

pytestmark = pytest.mark.gpu


def _synth():
    return importlib.import_module("racing-slam_amd").synth


@functools.lru_cache(maxsize=None)
def _scene(seed=0, n=2000, outlier_frac=0.3, noise_px=0.5, motion="forward"):
    return _synth().make_pose_pair(seed, n, outlier_frac, noise_px, motion)


@functools.lru_cache(maxsize=None)
def _ref(seed=0, n=2000, outlier_frac=0.3, noise_px=0.5, motion="forward", max_hyp=1000, rseed=0):
    d = _scene(seed, n, outlier_frac, noise_px, motion)
    return R.estimate_pose(d["pts_from"], d["pts_to"], d["K"], max_hypotheses=max_hyp, seed=rseed, stages=True)


def _run(ctx, est, pf, pt, K, count=None, max_n=None, idx=None, **kw):
    pf = np.ascontiguousarray(pf, np.float32).reshape(-1, 2)
    pt = np.ascontiguousarray(pt, np.float32).reshape(-1, 2)
    n = len(pt) if count is None else count
    max_n = len(pt) if max_n is None else max_n
    dev = lambda a: ctx.dev(a) if len(a) else ctx.empty((1, 2), ctx.torch.float32)     # noqa: E731
    di = None if idx is None else ctx.dev(np.asarray(idx, np.int32))
    r = ctx.estimate_pose(est, dev(pf), dev(pt), ctx.dev(np.array([n], np.int32)), max_n, K, d_from_index=di, **kw)
    o = {k: to_np(v) for k, v in r.items()}
    o["status"], o["inlier_count"] = int(o["status"][0]), int(o["inlier_count"][0])
    return o


@pytest.fixture(scope="module")
def est(ctx):
    e = ctx.pose_estimator(8192, 4096)
    yield e
    e.close()


def _same_up_to_sign(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return min(np.abs(a - b).max(), np.abs(a + b).max()) <= tol * max(np.abs(b).max(), 1e-300)


def _slack(E, d, thr2):
    x1, y1 = R.normalise(d["pts_from"], d["K"])
    x2, y2 = R.normalise(d["pts_to"], d["K"])
    err = R.sampson(E, x1, y1, x2, y2)
    return np.abs(err - thr2) <= 1e-9 * thr2


def test_stages_match_the_restatement(ctx, est):
    d, ref = _scene(), _ref()
    o = _run(ctx, est, d["pts_from"], d["pts_to"], d["K"])
    st, hy = est.stats(), est.hypotheses()
    H = ref["drawn"]
    assert st["drawn"] == H
    assert np.array_equal(hy["samples"][:H], ref["samples"])
    assert np.array_equal(hy["nmodels"][:H], ref["nmodels"])
    assert (hy["nmodels"][H:] == -1).all()
    for h in range(H):
        for m in range(ref["nmodels"][h]):
            assert _same_up_to_sign(hy["models"][h, m], ref["models"][h, m], 1e-9), (h, m)
            diff = abs(int(hy["scores"][h, m]) - int(ref["scores"][h, m]))
            assert diff <= int(_slack(ref["models"][h, m], d, ref["thr2"]).sum()), (h, m)
    assert st["scored"] == int(ref["nmodels"].sum())
    h, m = ref["best"]
    assert st["best_index"] == 10 * h + m
    assert st["lo_kept"] == ref["lo_kept"]
    assert _same_up_to_sign(st["E"], ref["E"], 1e-9)             # the LO normal matrix is summed in the kernel's order
    assert o["status"] == 0
    near = _slack(ref["E"], d, ref["thr2"])
    assert np.array_equal(o["inlier"][~near], ref["inlier"][~near])
    # the four f32 candidates: counts equal the oracle's DLT on exactly these poses; the first strict maximum wins
    fin = np.ones(len(d["pts_from"]), bool)
    assert st["cheir"] == R.cheirality_counts(st["candidates"], d["pts_from"], d["pts_to"], d["K"], fin)
    assert st["chosen"] == R.first_strict_max(st["cheir"])
    assert np.array_equal(o["pose"], st["candidates"][st["chosen"]])
    assert np.allclose(o["pose"], ref["pose"], atol=1e-5)
    # the compacted inlier list: ascending, exactly the mask
    assert o["inlier_count"] == int(o["inlier"].sum()) == st["inliers"]
    assert np.array_equal(o["inlier_index"][:o["inlier_count"]], np.flatnonzero(o["inlier"]))


@pytest.mark.parametrize("motion", ["forward", "sideways", "small", "rotation", "planar"])
def test_every_motion_matches_the_restatement(ctx, est, motion):
    """Agreement with the restatement only: for "small", "rotation" and "planar" the restatement's pose is itself not
    the true motion (tests/test_essential_cpu.py DEGENERATE records by how much)."""
    d, ref = _scene(1, 1500, 0.4, 0.5, motion), _ref(1, 1500, 0.4, 0.5, motion)
    o = _run(ctx, est, d["pts_from"], d["pts_to"], d["K"])
    st = est.stats()
    assert o["status"] == ref["status"] == 0
    assert st["drawn"] == ref["drawn"] and st["best_index"] == 10 * ref["best"][0] + ref["best"][1]
    assert _same_up_to_sign(st["E"], ref["E"], 1e-9)
    assert abs(o["inlier_count"] - ref["count"]) <= 3
    assert st["chosen"] == R.first_strict_max(st["cheir"])
    if max(ref["cheir"]) > 50:                                  # a decisive vote: the same pose
        assert np.allclose(o["pose"], ref["pose"], atol=1e-5)


def test_deterministic_and_seeded(ctx, est):
    d = _scene()
    a = _run(ctx, est, d["pts_from"], d["pts_to"], d["K"], seed=7)
    ha = est.hypotheses()
    b = _run(ctx, est, d["pts_from"], d["pts_to"], d["K"], seed=7)
    hb = est.hypotheses()
    for k in ("pose", "inlier", "inlier_index"):
        assert a[k].tobytes() == b[k].tobytes()
    for k in ha:
        assert ha[k].tobytes() == hb[k].tobytes()
    _run(ctx, est, d["pts_from"], d["pts_to"], d["K"], seed=8)
    hc = est.hypotheses()
    assert not np.array_equal(ha["samples"][:256], hc["samples"][:256])
    # a later call with fewer hypotheses leaves nothing of the earlier one in the table
    _run(ctx, est, d["pts_from"], d["pts_to"], d["K"], seed=8, max_hypotheses=3000, confidence=1 - 1e-12)
    _run(ctx, est, d["pts_from"], d["pts_to"], d["K"], seed=8, max_hypotheses=10)
    hd = est.hypotheses()
    assert (hd["nmodels"][10:] == -1).all() and (hd["samples"][10:] == -1).all() and (hd["scores"][10:] == 0).all()


def test_real_chain_from_track_features(ctx, est):
    """Points and count straight from rs_track_features: the "from" points gathered through d_kept_index."""
    fr = _synth().make_klt_pair(1)
    W, H = fr["width"], fr["height"]
    i1, i2 = ctx.image(W, H, frame=fr["img1"]), ctx.image(W, H, frame=fr["img2"])
    d_prev = ctx.dev(fr["pts"])
    n = len(fr["pts"])
    tr = ctx.track_features(i1, i2, d_prev, n)
    K = np.array([500.0, 500.0, W / 2.0, H / 2.0], np.float32)
    r = ctx.estimate_pose(est, d_prev, tr["pts"], tr["count"], n, K, d_from_index=tr["index"])
    cnt = int(to_np(tr["count"])[0])
    idx = to_np(tr["index"])[:cnt]
    ref = R.estimate_pose(fr["pts"][idx], to_np(tr["pts"])[:cnt], K)
    st = est.stats()
    assert cnt > 100 and st["n"] == cnt
    assert int(to_np(r["status"])[0]) == ref["status"]
    assert st["drawn"] == ref["drawn"] and st["best_index"] == 10 * ref["best"][0] + ref["best"][1]
    assert _same_up_to_sign(st["E"], ref["E"], 1e-9)
    i1.close(); i2.close()


def test_envelope(ctx, est):
    rs = importlib.import_module("racing-slam_amd").rsgpu
    d = _scene()
    pf, pt, K = d["pts_from"], d["pts_to"], d["K"]
    for n in (0, 4):                                             # too few points: identity, no inliers
        o = _run(ctx, est, pf[:n], pt[:n], K, count=n, max_n=max(n, 1)) if n else _run(ctx, est, pf[:1], pt[:1], K, count=0)
        assert o["status"] == 1 and o["inlier_count"] == 0 and np.array_equal(o["pose"], np.eye(4, dtype=np.float32))
        assert not o["inlier"].any()
    o = _run(ctx, est, pf[:5], pt[:5], K)
    ref = R.estimate_pose(pf[:5], pt[:5], K)
    assert o["status"] == ref["status"] and o["inlier_count"] == ref["count"]
    # max_n below the device count: the first max_n points
    o = _run(ctx, est, pf, pt, K, count=2000, max_n=700)
    ref = R.estimate_pose(pf[:700], pt[:700], K)
    assert est.stats()["n"] == 700 and est.stats()["best_index"] == 10 * ref["best"][0] + ref["best"][1]
    assert o["inlier"].shape == (700,)
    # max_points: 8192 points
    big = _scene(3, 8192, 0.3, 0.5, "forward")
    o = _run(ctx, est, big["pts_from"], big["pts_to"], big["K"], max_hypotheses=256)
    ref = R.estimate_pose(big["pts_from"], big["pts_to"], big["K"], max_hypotheses=256)
    assert o["status"] == 0 and est.stats()["best_index"] == 10 * ref["best"][0] + ref["best"][1]
    # one hypothesis; the cap of 4096 hypotheses on pure outliers (no early stop)
    o = _run(ctx, est, pf, pt, K, max_hypotheses=1)
    ref = R.estimate_pose(pf, pt, K, max_hypotheses=1)
    assert est.stats()["drawn"] == 1 and o["status"] == ref["status"]
    rng = np.random.default_rng(5)
    junk = rng.uniform(0, 1000, (2, 300, 2)).astype(np.float32)
    o = _run(ctx, est, junk[0], junk[1], K, max_hypotheses=4096)
    ref = R.estimate_pose(junk[0], junk[1], K, max_hypotheses=4096, stages=True)
    st, hy = est.stats(), est.hypotheses()
    assert st["drawn"] == ref["drawn"] and np.array_equal(hy["samples"][:ref["drawn"]], ref["samples"])
    assert o["status"] == ref["status"] and st["best_index"] == 10 * ref["best"][0] + ref["best"][1]
    # duplicates: one point repeated; no 5 distinct points, no model
    o = _run(ctx, est, np.repeat(pf[:1], 50, 0), np.repeat(pt[:1], 50, 0), K)
    assert o["status"] == 2 and o["inlier_count"] == 0
    # non-finite points are never sampled, never inliers
    pfn, ptn = pf[:1000].copy(), pt[:1000].copy()
    pfn[::7, 0] = np.nan
    ptn[3::11, 1] = np.inf
    o = _run(ctx, est, pfn, ptn, K)
    ref = R.estimate_pose(pfn, ptn, K, stages=True)
    bad = ~np.isfinite(pfn).all(1) | ~np.isfinite(ptn).all(1)
    hy = est.hypotheses()
    assert not bad[hy["samples"][:ref["drawn"]].ravel()].any()
    assert not o["inlier"][bad].any() and o["status"] == 0
    assert np.array_equal(hy["samples"][:ref["drawn"]], ref["samples"])
    # a near-pure rotation
    rot = _scene(2, 1000, 0.2, 0.3, "rotation")
    o = _run(ctx, est, rot["pts_from"], rot["pts_to"], rot["K"])
    ref = R.estimate_pose(rot["pts_from"], rot["pts_to"], rot["K"])
    assert o["status"] == ref["status"] and est.stats()["best_index"] == 10 * ref["best"][0] + ref["best"][1]
    # outside the envelope
    for mp, mh in ((0, 10), (8193, 10), (100, 0), (100, 4097)):
        with pytest.raises(rs.RsError, match="status 4"):
            ctx.pose_estimator(mp, mh)
    small = ctx.pose_estimator(100, 10)
    with pytest.raises(rs.RsError, match="status 4"):
        _run(ctx, small, pf[:200], pt[:200], K)
    with pytest.raises(rs.RsError, match="status 4"):
        _run(ctx, small, pf[:50], pt[:50], K, max_hypotheses=11)
    small.close()


def test_known_rotation_matches_the_restatement(ctx, est):
    d = _scene(4, 1500, 0.3, 0.5, "forward")
    rng = np.random.default_rng(11)
    pairs = rng.integers(0, 1500, (200, 2)).astype(np.int32)
    pairs[5] = (3, 3)                                            # i == j: skipped
    Rm = d["R"].astype(np.float32)
    ref = R.estimate_pose_known_rotation(d["pts_from"], d["pts_to"], d["K"], Rm, pairs)
    r = ctx.estimate_pose_known_rotation(est, ctx.dev(d["pts_from"]), ctx.dev(d["pts_to"]), 1500, d["K"], Rm,
                                         ctx.dev(pairs), 200)
    o = {k: to_np(v) for k, v in r.items()}
    st, hy = est.stats(), est.hypotheses()
    assert np.array_equal(hy["scores"][:200, 0], ref["support"])
    assert np.array_equal(hy["samples"][:200, :2], pairs)
    assert (hy["samples"][:200, 2:] == -1).all() and (hy["nmodels"][200:] == -1).all() and st["drawn"] == 200
    assert np.array_equal(hy["nmodels"][:200], (ref["support"] >= 0).astype(np.int32))
    assert st["best_index"] == ref["best_iter"] and int(o["status"][0]) == 0 == ref["status"]
    assert np.array_equal(o["inlier"], ref["inlier"]) and int(o["inlier_count"][0]) == ref["count"]
    assert (st["cheir0"], st["cheir1"]) == ref["front"]
    assert np.allclose(o["pose"], ref["pose"], atol=2e-6)
    assert np.array_equal(o["pose"][:3, :3], Rm)
    t = o["pose"][:3, 3].astype(np.float64)
    assert np.degrees(np.arccos(np.clip(t @ d["t"] / np.linalg.norm(t), -1, 1))) < 1.0
    # fewer than 8 points: [R | 0]
    r = ctx.estimate_pose_known_rotation(est, ctx.dev(d["pts_from"][:7]), ctx.dev(d["pts_to"][:7]), 7, d["K"], Rm,
                                         ctx.dev(np.zeros((200, 2), np.int32)), 200)
    assert int(to_np(r["status"])[0]) == 1 and np.array_equal(to_np(r["pose"])[:3, 3], np.zeros(3, np.float32))
