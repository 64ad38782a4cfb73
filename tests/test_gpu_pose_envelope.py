"""rs_estimate_pose and rs_estimate_pose_known_rotation across their envelope (tests/pose_cases.py): the GPU against the
restatement tests/essential_ref.py at the strength of tests/test_gpu_essential.py, then the GPU's own hypothesis table
against the independent checks of tests/pose_hp.py, so that a table that is wrong in the same way as the restatement
still fails.  Then the C-ABI contract: sentinel-filled outputs, d_from_index, refused calls, alternating forms."""
import functools

import numpy as np
import pytest

import essential_ref as R
import pose_cases as PC
import pose_hp as HP
from conftest import to_np

pytestmark = pytest.mark.gpu

SENT = 0x5A


@functools.lru_cache(maxsize=None)
def _scene(name):
    return PC.scene(PC.CASES[name] if name in PC.CASES else PC.KR_CASES[name])


@functools.lru_cache(maxsize=None)
def _ref(name):
    case = PC.CASES[name]
    pf, pt, K, count, max_n, kw = PC.call_args(case, _scene(name))
    n = min(count, max_n)
    return R.estimate_pose(pf[:n], pt[:n], K, stages=True, **kw)


@pytest.fixture(scope="module")
def est(ctx):
    e = ctx.pose_estimator(8192, 4096)
    yield e
    e.close()


def _out(ctx, m):
    t = ctx.torch
    o = dict(pose=ctx.empty((4, 4), t.float32), inlier=ctx.empty((m,), t.uint8), inlier_index=ctx.empty((m,), t.int32),
             inlier_count=ctx.empty((1,), t.int32), status=ctx.empty((1,), t.int32))
    for v in o.values():
        v.view(t.uint8).fill_(SENT)
    return o


def _np(o):
    r = {k: to_np(v) for k, v in o.items()}
    r["status"], r["inlier_count"] = int(r["status"][0]), int(r["inlier_count"][0])
    return r


def _run(ctx, est, pf, pt, K, count, max_n, idx=None, **kw):
    pf = np.ascontiguousarray(pf, np.float32).reshape(-1, 2)
    pt = np.ascontiguousarray(pt, np.float32).reshape(-1, 2)
    out = _out(ctx, max(max_n, 1))
    di = None if idx is None else ctx.dev(np.asarray(idx, np.int32))
    ctx.estimate_pose(est, ctx.dev(pf), ctx.dev(pt), ctx.dev(np.array([count], np.int32)), max_n, K, d_from_index=di,
                      out=out, **kw)
    return _np(out)


def _check_outputs(o, n, max_n):
    """Every output written: the mask zero past n, the first count indices exact, pose and status set."""
    assert o["status"] in (0, 1, 2)
    assert set(np.unique(o["inlier"][:max_n])) <= {0, 1} and not o["inlier"][n:max_n].any()
    c = o["inlier_count"]
    assert c == int(o["inlier"].sum())
    assert np.array_equal(o["inlier_index"][:c], np.flatnonzero(o["inlier"]))
    assert not (o["pose"].view(np.uint8) == SENT).all()
    if o["status"] != 0:
        assert c == 0 and np.array_equal(o["pose"], np.eye(4, dtype=np.float32))


def _independent(st, hy, pf, pt, K, thr, drawn, exact_scene=None):
    """The GPU's own table against pose_hp: every model essential and fitting its sample, every score a literal f64
    Sampson count (up to the points within 1e-9 of the bound), LO never lowering the count, the table -1 / 0 past the
    stop, scored = the models drawn."""
    x1, y1 = HP.normalised(pf, K)
    x2, y2 = HP.normalised(pt, K)
    nm = hy["nmodels"]
    assert (nm[:drawn] >= 0).all() and (nm[:drawn] <= 10).all()
    assert (nm[drawn:] == -1).all() and (hy["samples"][drawn:] == -1).all() and (hy["scores"][drawn:] == 0).all()
    assert st["scored"] == int(nm[:drawn].sum())
    hit = 0
    for h in range(drawn):
        s = hy["samples"][h]
        if nm[h] == 0:
            continue
        assert len(set(s.tolist())) == 5 and (s >= 0).all()
        for m in range(nm[h]):
            E = hy["models"][h, m]
            det, cubic, epi = HP.essential_checks(E, x1[s], y1[s], x2[s], y2[s])
            assert det < 1e-6 and cubic <= 1.01e-6 and epi < 1e-9, (h, m, det, cubic, epi)
            c, near = HP.sampson_count(E, pf, pt, K, thr)
            assert abs(int(hy["scores"][h, m]) - c) <= near, (h, m)
        if exact_scene is not None:
            hit += any(HP.dist_up_to_sign(hy["models"][h, m], exact_scene) < 1e-3 for m in range(nm[h]))
    assert (hy["scores"][:drawn][np.arange(10)[None, :] >= nm[:drawn, None]] == 0).all()
    if st["status"] == 0:
        assert st["inliers"] >= st["best_count"] == int(hy["scores"].max())
    return hit


@pytest.mark.parametrize("name", list(PC.CASES))
def test_case_against_restatement_and_independent_checks(ctx, est, name):
    case = PC.CASES[name]
    d = _scene(name)
    pf, pt, K, count, max_n, kw = PC.call_args(case, d)
    n = min(count, max_n)
    o = _run(ctx, est, pf[:max_n], pt[:max_n], K, count, max_n, **kw)
    st, hy, ref = est.stats(), est.hypotheses(), _ref(name)
    H = ref["drawn"]
    assert st["n"] == n and st["drawn"] == H
    if case["stop"] is None:
        assert H == kw["max_hypotheses"] or n < 5
    else:
        assert H == min(256 * case["stop"], kw["max_hypotheses"])
    assert np.array_equal(hy["samples"][:H], ref["samples"])
    assert np.array_equal(hy["nmodels"][:H], ref["nmodels"])
    x1, y1 = R.normalise(pf[:n], K)
    x2, y2 = R.normalise(pt[:n], K)
    for h in range(H):
        for m in range(ref["nmodels"][h]):
            assert HP.dist_up_to_sign(hy["models"][h, m], ref["models"][h, m]) <= 1e-9, (h, m)
            near = np.abs(R.sampson(ref["models"][h, m], x1, y1, x2, y2) - ref["thr2"]) <= 1e-9 * ref["thr2"]
            assert abs(int(hy["scores"][h, m]) - int(ref["scores"][h, m])) <= int(near.sum()), (h, m)
    assert st["best_index"] == (10 * ref["best"][0] + ref["best"][1] if ref["best"][0] >= 0 else -1)
    assert o["status"] == ref["status"] == st["status"]
    _check_outputs(o, n, max_n)
    if o["status"] == 0:
        near = np.abs(R.sampson(ref["E"], x1, y1, x2, y2) - ref["thr2"]) <= 1e-9 * ref["thr2"]
        assert HP.dist_up_to_sign(st["E"], ref["E"]) <= 1e-9
        assert np.array_equal(o["inlier"][:n][~near], ref["inlier"][~near])
        c, nr = HP.sampson_count(st["E"], pf[:n], pt[:n], K, kw["threshold_px"])
        assert abs(o["inlier_count"] - c) <= nr
    exact = case["scene"]["noise_px"] == 0 and case["scene"]["outlier_frac"] == 0
    Et = HP.true_E(d["R"], d["t"]) if exact else None
    hit = _independent(st, hy, pf[:n], pt[:n], K, kw["threshold_px"], H, Et)
    if exact and case["scene"]["motion"] in ("forward", "sideways"):
        # noise-free samples hold the true E (within 1e-3), but for samples too close to degenerate for the f32 pixels:
        # recorded 2 of 256 on forward (nearest models 0.015 and 0.32 away), 0 on sideways
        assert hit >= int((hy["nmodels"][:H] > 0).sum()) - {"forward": 2, "sideways": 0}[case["scene"]["motion"]]


def test_from_index_permutation_repeats_and_negatives(ctx, est):
    d = _scene("forward")
    pf, pt, K = d["pts_from"], d["pts_to"], d["K"]
    n = 600
    rng = np.random.default_rng(1)
    big = rng.uniform(0, 1000, (2000, 2)).astype(np.float32)
    idx = rng.permutation(2000)[:n].astype(np.int32)
    big[idx] = pf[:n]
    idx[50:60] = idx[40]                                          # repeated "from" points
    idx[100:130] = -1                                             # negative: a non-finite point
    idx[200] = -(1 << 30)
    gathered = np.where((idx >= 0)[:, None], big[np.maximum(idx, 0)], np.float32(np.nan))
    o = _run(ctx, est, big, pt[:n], K, n, n, idx=idx)
    ref = R.estimate_pose(gathered, pt[:n], K, stages=True)
    st, hy = est.stats(), est.hypotheses()
    assert np.array_equal(hy["samples"][:ref["drawn"]], ref["samples"])
    assert not np.isin(hy["samples"][:ref["drawn"]], np.flatnonzero(idx < 0)).any()
    assert st["best_index"] == 10 * ref["best"][0] + ref["best"][1] and o["status"] == 0
    assert not o["inlier"][idx < 0].any()
    # the known-rotation form through the same index
    pairs = PC.kr_pairs(PC.KR_CASES["kr_iter200"], n)
    Rm = d["R"].astype(np.float32)
    out = _out(ctx, n)
    ctx.estimate_pose_known_rotation(est, ctx.dev(big), ctx.dev(pt[:n]), n, K, Rm, ctx.dev(pairs), 200,
                                     d_from_index=ctx.dev(idx), out=out)
    o = _np(out)
    kr = R.estimate_pose_known_rotation(gathered, pt[:n], K, Rm, pairs)
    hy = est.hypotheses()
    assert np.array_equal(hy["scores"][:200, 0], kr["support"])
    assert o["status"] == kr["status"] == 0 and np.array_equal(o["inlier"], kr["inlier"])
    assert not o["inlier"][idx < 0].any()
    _check_outputs(o, n, n)


def test_status_1_and_2_write_every_output(ctx, est):
    d = _scene("forward")
    pf, pt, K = d["pts_from"], d["pts_to"], d["K"]
    o = _run(ctx, est, pf[:64], pt[:64], K, 4, 64)                # 4 of 64: too few points
    assert o["status"] == 1
    _check_outputs(o, 4, 64)
    o = _run(ctx, est, np.repeat(pf[:1], 64, 0), np.repeat(pt[:1], 64, 0), K, 64, 64)   # no 5 distinct points
    assert o["status"] == 2 and est.stats()["drawn"] == 1000            # no model: no early stop
    _check_outputs(o, 64, 64)
    Rm = d["R"].astype(np.float32)
    for n, status in ((7, 1), (64, 2)):
        out = _out(ctx, 64)
        p = np.zeros((200, 2), np.int32)                          # every pair i == j: skipped, [R | 0]
        ctx.estimate_pose_known_rotation(est, ctx.dev(pf[:64]), ctx.dev(pt[:64]), n, K, Rm, ctx.dev(p), 200, out=out)
        o = _np(out)
        assert o["status"] == status and o["inlier_count"] == 0 and not o["inlier"][:n].any()     # d_inlier is [n] here
        want = np.eye(4, dtype=np.float32)
        want[:3, :3] = Rm
        assert np.array_equal(o["pose"], want)
        st, hy = est.stats(), est.hypotheses()
        if n < 8:                                                 # fewer than 8 points: nothing drawn, the table empty
            assert st["drawn"] == 0 and (hy["nmodels"] == -1).all() and (hy["samples"] == -1).all()
        else:
            assert st["drawn"] == 200 and (hy["scores"][:200, 0] == -1).all() and (hy["nmodels"][:200] == 0).all()


def _snapshot(ctx, est, out):
    ctx.synchronize()
    st = est.stats()
    return ({k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in st.items()},
            {k: v.tobytes() for k, v in est.hypotheses().items()}, {k: to_np(v).tobytes() for k, v in out.items()})


def test_refused_calls_leave_everything_untouched(ctx, est):
    rs = __import__("importlib").import_module("racing-slam_amd").rsgpu
    d = _scene("forward")
    pf, pt, K = ctx.dev(d["pts_from"]), ctx.dev(d["pts_to"]), d["K"]
    cnt = ctx.dev(np.array([1000], np.int32))
    out = _out(ctx, 1000)
    ctx.estimate_pose(est, pf, pt, cnt, 1000, K, out=out)
    before = _snapshot(ctx, est, out)
    Kbad = [(0.0, 700, 640, 360), (700, -1, 640, 360), (700, 700, np.nan, 360), (700, 700, 640, np.inf)]
    calls = [dict(K=k) for k in Kbad] + [dict(threshold_px=0.0), dict(threshold_px=-1.0), dict(threshold_px=np.nan),
                                         dict(confidence=0.0), dict(confidence=1.0), dict(confidence=np.nan),
                                         dict(max_hypotheses=0), dict(max_hypotheses=4097)]
    for c in calls:
        kw = dict(c)
        k = kw.pop("K", K)
        with pytest.raises(rs.RsError):
            ctx.estimate_pose(est, pf, pt, cnt, 1000, k, out=out, **kw)
        assert _snapshot(ctx, est, out) == before, c
    with pytest.raises(rs.RsError):
        ctx.estimate_pose(est, pf, pt, None, 1000, K, out=out)    # a null count
    assert _snapshot(ctx, est, out) == before
    Rm = _scene("forward")["R"].astype(np.float32)
    pairs = ctx.dev(np.zeros((4096, 2), np.int32))
    for c in [dict(K=k) for k in Kbad] + [dict(max_epipolar_px=0.0), dict(max_epipolar_px=-2.0),
                                          dict(max_epipolar_px=np.nan), dict(n_iter=0), dict(n_iter=4097)]:
        kw = dict(c)
        k, it = kw.pop("K", K), kw.pop("n_iter", 200)
        with pytest.raises(rs.RsError):
            ctx.estimate_pose_known_rotation(est, pf, pt, 1000, k, Rm, pairs, it, out=out, **kw)
        assert _snapshot(ctx, est, out) == before, c


def test_alternating_forms_leave_nothing_stale(ctx, est):
    d = _scene("forward")
    pf, pt, K = d["pts_from"], d["pts_to"], d["K"]
    Rm = d["R"].astype(np.float32)
    pairs = PC.kr_pairs(PC.KR_CASES["kr_iter4096"], 1000)
    for _ in range(2):
        out = _out(ctx, 1000)
        ctx.estimate_pose_known_rotation(est, ctx.dev(pf), ctx.dev(pt), 1000, K, Rm, ctx.dev(pairs), 4096, out=out)
        st, hy = est.stats(), est.hypotheses()
        assert st["known"] == 1 and st["drawn"] == 4096 and (hy["samples"][:, 2:] == -1).all()
        o = _run(ctx, est, pf, pt, K, 1000, 1000, max_hypotheses=300)
        st, hy, ref = est.stats(), est.hypotheses(), R.estimate_pose(pf, pt, K, max_hypotheses=300, stages=True)
        H = ref["drawn"]
        assert st["known"] == 0 and st["drawn"] == H
        assert np.array_equal(hy["samples"][:H], ref["samples"]) and np.array_equal(hy["nmodels"][:H], ref["nmodels"])
        assert (hy["nmodels"][H:] == -1).all() and (hy["samples"][H:] == -1).all() and (hy["scores"][H:] == 0).all()
        assert o["status"] == 0


@pytest.mark.parametrize("name", list(PC.KR_CASES))
def test_known_rotation_case(ctx, est, name):
    case = PC.KR_CASES[name]
    d = _scene(name)
    n = len(d["pts_from"])
    Rm = d["R"].astype(np.float32)
    pairs = PC.kr_pairs(case, n)
    it = case["n_iter"]
    ref = R.estimate_pose_known_rotation(d["pts_from"], d["pts_to"], d["K"], Rm, pairs, case["max_epipolar_px"])
    out = _out(ctx, n)
    ctx.estimate_pose_known_rotation(est, ctx.dev(d["pts_from"]), ctx.dev(d["pts_to"]), n, d["K"], Rm, ctx.dev(pairs), it,
                                     max_epipolar_px=case["max_epipolar_px"], out=out)
    o = _np(out)
    st, hy = est.stats(), est.hypotheses()
    assert o["status"] == ref["status"] == st["status"] and st["known"] == 1
    _check_outputs_kr(o, n, Rm)
    if n < 8:
        assert st["drawn"] == 0 and (hy["nmodels"] == -1).all() and (hy["samples"] == -1).all()
        return
    assert st["drawn"] == it
    assert np.array_equal(hy["samples"][:it, :2], pairs)
    assert np.array_equal(hy["scores"][:it, 0], ref["support"])
    assert np.array_equal(hy["nmodels"][:it], (ref["support"] >= 0).astype(np.int32))
    assert (hy["nmodels"][it:] == -1).all()
    ok = ref["support"] >= 0
    assert np.array_equal(hy["models"][:it, 0, :3][ok].astype(np.float32), ref["trans"][ok])
    assert st["best_index"] == ref["best_iter"] or ref["status"] != 0
    assert np.array_equal(o["inlier"], ref["inlier"]) and o["inlier_count"] == ref["count"]
    if ref["status"] == 0:
        assert (st["cheir0"], st["cheir1"]) == ref["front"]
        assert np.allclose(o["pose"], ref["pose"], atol=2e-6)
        t = o["pose"][:3, 3].astype(np.float64)
        t_svd = HP.refit_translation(d["pts_from"], d["pts_to"], d["K"], Rm, o["inlier"])
        assert HP.dist_up_to_sign(t, t_svd) < 1e-5
        if case["pairs"] in ("random", "out_of_range") and it >= 200 and n >= 257:
            assert np.degrees(np.arccos(np.clip(t @ d["t"] / np.linalg.norm(t), -1, 1))) < 1.0
    if case["pairs"] == "tie":
        assert st["best_index"] == 0
    if case["pairs"] == "diagonal":
        assert o["status"] == 2 and (hy["scores"][:it, 0] == -1).all()


def _check_outputs_kr(o, n, Rm):
    _c = o["inlier_count"]
    assert _c == int(o["inlier"].sum()) and np.array_equal(o["inlier_index"][:_c], np.flatnonzero(o["inlier"]))
    assert np.array_equal(o["pose"][:3, :3], Rm) and np.array_equal(o["pose"][3], [0, 0, 0, 1])
    if o["status"] != 0:
        assert _c == 0 and np.array_equal(o["pose"][:3, 3], np.zeros(3, np.float32))


def test_known_rotation_support_8_against_7_and_the_sign_flip(ctx, est):
    """Best support of exactly 8 is accepted, 7 is not; the (i, j) order flips best t, and the cheirality vote must
    flip it back (fm > fp taken for one order and not the other)."""
    d = PC.synth().make_pose_pair(30, 9, 0.0, 0.0, "forward")
    Rm = d["R"].astype(np.float32)
    pf, pt, K = d["pts_from"].copy(), d["pts_to"].copy(), d["K"]
    flips = set()
    for order in ((0, 1), (1, 0)):
        pairs = np.array([order] * 4, np.int32)
        for bad, want in ((0, 0), (2, 2)):                        # 9 inliers, or 7 after moving two
            q = pt.copy()
            q[7:7 + bad] += np.float32(300.0)
            ref = R.estimate_pose_known_rotation(pf, q, K, Rm, pairs)
            out = _out(ctx, 9)
            ctx.estimate_pose_known_rotation(est, ctx.dev(pf), ctx.dev(q), 9, K, Rm, ctx.dev(pairs), 4, out=out)
            o = _np(out)
            assert o["status"] == ref["status"] == want and o["inlier_count"] == ref["count"]
            if want == 0:
                assert np.allclose(o["pose"], ref["pose"], atol=2e-6)
                flips.add(ref["front"][1] > ref["front"][0])
    q = pt.copy()
    q[8] += np.float32(300.0)                                     # exactly 8 inliers
    ref = R.estimate_pose_known_rotation(pf, q, K, Rm, np.array([(0, 1)] * 4, np.int32))
    out = _out(ctx, 9)
    ctx.estimate_pose_known_rotation(est, ctx.dev(pf), ctx.dev(q), 9, K, Rm, ctx.dev(np.array([(0, 1)] * 4, np.int32)), 4,
                                     out=out)
    o = _np(out)
    assert ref["count"] == 8 and o["status"] == ref["status"] == 0 and o["inlier_count"] == 8
    assert flips == {True, False}
