"""tests/loop_ref.py — the restatement of LoopDetector's "Loop verify" stage, best_candidate, publish_result and
update_streak — pinned by independent formulations, and the condition the GPU tests rest on, checked for every scene
they use with the restatement alone.  No GPU."""
import numpy as np
import pytest

import loop_cases as S
import loop_ref as L


def test_candidate_rows_is_the_mask_of_matched_keypoints():
    rng = np.random.default_rng(0)
    for n in (0, 1, 7, 300, 2500):
        kp = np.where(rng.random(n) < 0.4, rng.integers(0, 10 ** 6, n), -1).astype(np.int32)
        assert np.array_equal(L.candidate_rows(kp), np.flatnonzero(kp >= 0))
    assert len(L.candidate_rows(np.full(5, -1))) == 0 and L.candidate_rows(np.zeros(3, np.int32)).tolist() == [0, 1, 2]


def _pose(rng):
    A = np.linalg.qr(rng.normal(0, 1, (3, 3)))[0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = A * np.sign(np.linalg.det(A)), rng.normal(0, 3, 3)
    return T.astype(np.float32)


def test_verdict_against_f64():
    rng = np.random.default_rng(1)
    for k in range(50):
        T, qc, cc = _pose(rng), rng.normal(0, 3, 3).astype(np.float32), rng.normal(0, 3, 3).astype(np.float32)
        x = rng.uniform(0, 1280, int(rng.integers(0, 40))).astype(np.float32)
        corr = int(rng.integers(len(x), len(x) + 60))
        v = L.verdict(T, x, 1280, qc, cc, corr, len(x))
        T64 = T.astype(np.float64)
        c = -T64[:3, :3].T @ T64[:3, 3]
        assert abs(float(v["drift"]) - np.linalg.norm(c - qc)) <= 1e-6 * max(1.0, np.linalg.norm(c - qc))
        assert abs(float(v["gap"]) - np.linalg.norm(c - cc)) <= 1e-6 * max(1.0, np.linalg.norm(c - cc))
        spread = 0.0 if len(x) < 2 else (float(x.max()) - float(x.min())) / 1280.0
        assert abs(float(v["spread"]) - spread) <= 1e-6
        ratio = 0.0 if corr == 0 else len(x) / corr
        if abs(ratio - 0.35) > 1e-6 and abs(spread - 0.25) > 1e-6:
            assert v["ok"] == (len(x) >= 20 and ratio >= 0.35 and spread >= 0.25)
        assert all(v[k].dtype == np.float32 for k in ("spread", "drift", "gap"))
    assert L.verdict(np.eye(4), [5.0], 1280, np.zeros(3), np.zeros(3), 1, 1)["spread"] == 0
    assert L.verdict(np.eye(4), [5.0, 900.0], 0, np.zeros(3), np.zeros(3), 2, 2)["spread"] == 0
    # exactly on the three bounds: inclusive, as the reference's >=
    assert L.verdict(np.eye(4), [0.0, 320.0] + [10.0] * 18, 1280, np.zeros(3), np.zeros(3), 20, 20)["ok"]
    assert not L.verdict(np.eye(4), [0.0, 319.0] + [10.0] * 18, 1280, np.zeros(3), np.zeros(3), 20, 20)["ok"]
    assert not L.verdict(np.eye(4), [0.0, 320.0] + [10.0] * 17, 1280, np.zeros(3), np.zeros(3), 19, 19)["ok"]
    assert L.verdict(np.eye(4), [0.0, 640.0] + [10.0] * 33, 1280, np.zeros(3), np.zeros(3), 100, 35)["ok"]
    assert not L.verdict(np.eye(4), [0.0, 640.0] + [10.0] * 32, 1280, np.zeros(3), np.zeros(3), 100, 34)["ok"]


def V(ok, inliers, pose=None):
    return dict(ok=ok, inliers=inliers, pose=np.eye(4, dtype=np.float32) if pose is None else pose,
                query_kp=np.arange(inliers, dtype=np.int32), point=np.arange(inliers, dtype=np.int32) + 100)


def test_best_candidate():
    assert L.best_candidate([V(False, 5)]) == 0
    assert L.best_candidate([V(False, 50), V(True, 20), V(True, 30), V(True, 30)]) == 2          # verified first, most inliers, first of equals
    assert L.best_candidate([V(False, 5), V(False, 9), V(False, 9)]) == 1
    assert L.best_candidate([V(False, 9), V(False, 9)]) == 0


EYE = [np.eye(4, dtype=np.float32)] * 3


def test_streak_of_three_yields_one_constraint():
    st = L.LoopState()
    rng = np.random.default_rng(2)
    pose, cand = _pose(rng), _pose(rng)
    for k, q in enumerate((60, 61, 62)):
        chosen = L.update_streak(st, q, [3 + k, 30], [V(True, 40, pose), V(False, 90)], [cand, cand])
        assert chosen == 0 and len(st.streak) == k + 1
        assert st.consume_new_loop() == (k == 2)
    assert len(st.constraints) == 1
    c = st.constraints[0]
    assert (c["from"], c["to"]) == (62, 5) and c["pairs"].shape == (40, 2)
    R, t = cand[:3, :3].astype(np.float64), cand[:3, 3].astype(np.float64)
    inv = np.eye(4)
    inv[:3, :3], inv[:3, 3] = R.T, -R.T @ t
    assert np.allclose(c["relative"], pose.astype(np.float64) @ inv, atol=1e-5)
    assert not st.consume_new_loop()


def test_candidate_gap_resets_the_streak():
    st = L.LoopState()
    L.update_streak(st, 60, [3], [V(True, 40)], EYE)
    L.update_streak(st, 61, [4], [V(True, 40)], EYE)
    assert len(st.streak) == 2
    L.update_streak(st, 62, [4 + 16], [V(True, 40)], EYE)               # 16 > CONSISTENCY_WINDOW: a new streak of one
    assert len(st.streak) == 1 and not st.constraints
    L.update_streak(st, 63, [20 + 15, 2], [V(True, 40), V(True, 90)], EYE)      # 15 is inside; the better one is too far
    assert len(st.streak) == 2 and st.streak[-1]["candidate_index"] == 35


def test_second_loop_near_a_constraint_is_suppressed():
    st = L.LoopState()
    for q in range(60, 66):
        L.update_streak(st, q, [q - 57], [V(True, 40)], EYE)
    assert [(c["from"], c["to"]) for c in st.constraints] == [(62, 5)] and len(st.streak) == 6
    st2 = L.LoopState()
    st2.constraints = [{"from": 62, "to": 5}]
    for q in (77, 78, 79):                                              # from-gap 15: not suppressed
        L.update_streak(st2, q, [10], [V(True, 40)], EYE)
    assert [(c["from"], c["to"]) for c in st2.constraints] == [(62, 5), (79, 10)]
    st3 = L.LoopState()
    st3.constraints = [{"from": 62, "to": 5}]
    for q in (74, 75, 76):                                              # from-gap 14 and to-gap 14: suppressed
        L.update_streak(st3, q, [19], [V(True, 40)], EYE)
    assert len(st3.constraints) == 1 and not st3.new_loop
    for q in (77,):                                                     # to-gap 15 from then on
        L.update_streak(st3, q, [20], [V(True, 40)], EYE)
    assert [(c["from"], c["to"]) for c in st3.constraints] == [(62, 5), (77, 20)]


def test_unverified_query_clears_and_gap_in_queries_restarts():
    st = L.LoopState()
    L.update_streak(st, 60, [3], [V(True, 40)], EYE)
    L.update_streak(st, 61, [3], [V(True, 40)], EYE)
    assert L.update_streak(st, 62, [3, 4], [V(False, 90), V(False, 10)], EYE) == -1 and st.streak == []
    L.update_streak(st, 63, [3], [V(True, 40)], EYE)
    L.update_streak(st, 64, [3], [V(True, 40)], EYE)
    L.update_streak(st, 66, [3], [V(True, 40)], EYE)                    # 65 was skipped: the streak restarts
    assert len(st.streak) == 1 and not st.constraints
    L.update_streak(st, 67, [], [], [])                                 # nothing ranked
    assert st.streak == []


def test_publish_shows_the_best_candidate():
    p = L.publish([7, 9, 12], [0.3, 0.2, 0.1], [V(False, 80), V(True, 30), V(True, 25)])
    assert p == dict(candidate_index=9, score=0.2, matches=30, verified=True, edges=[False, True, True], display=1)


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_scenes_are_far_from_every_bound(name):
    """What lets the GPU tests demand equal status, correspondences and ok: per candidate at most 3 correspondences lie
    in test_gpu_pnp.py's near-threshold band of the final model, and no bound of the verdict is within that of flipping."""
    s, refs = S.scene(name), S.reference(name)
    assert [(r["status"], r["ok"]) for r in refs] == S.EXPECT[name]
    for c, r in enumerate(refs):
        slack = int(S.near_threshold(s, r).sum())
        assert slack <= 3, (c, slack)
        n, k = r["correspondences"], r["inliers"]
        if r["status"] != 0:
            continue
        assert k - slack >= L.MIN_PNP_INLIERS or k + slack < L.MIN_PNP_INLIERS, (c, k)
        assert (k - slack) / n >= 0.35 + 1e-6 or (k + slack) / n < 0.35 - 1e-6, (c, k, n)
        assert abs(float(r["spread"]) - 0.25) > 1.0 / s["width"], (c, r["spread"])
    if name == "paths":
        assert [r["correspondences"] for r in refs[1:4]] == [0, 1, 11]
        assert refs[4]["correspondences"] >= 12 and refs[5]["inliers"] < 20 <= refs[6]["inliers"] and refs[7]["inliers"] >= 20
        assert refs[6]["inliers"] / refs[6]["correspondences"] < 0.35 <= refs[7]["inliers"] / refs[7]["correspondences"]
        assert float(refs[6]["spread"]) >= 0.25 > float(refs[7]["spread"])
    else:
        assert len(refs[0]["rows"]) == 1100
