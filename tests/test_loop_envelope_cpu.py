"""The scenes of tests/test_gpu_loop_envelope.py (loop_cases.ENVELOPE, loop_cases.PARAMETERS) are what their names say, and
the condition that file rests on, with the restatements alone.  No GPU.

Condition, not a measurement: wherever the GPU test demands the restatement's ok, loop_cases.decided holds — at most 3
correspondences in test_gpu_pnp.py's near-threshold band (the cap of tests/test_loop_cpu.py) and no bound of the verdict
within that slack of flipping; in `bounds`, which sits ON the bounds, the band is empty."""
import numpy as np

import loop_cases as S
import loop_ref as L
import match_ref

f32 = np.float32


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _consistent(s):
    """kp_point and the observations are one fact, and a shared pair's rows are near copies of each other."""
    seen = [np.full(len(k["kp"]), -1, np.int64) for k in s["key_frames"]]
    for p, kf, i in s["observations"]:
        assert seen[kf][i] == -1
        seen[kf][i] = p
    for k, t in zip(s["key_frames"], seen):
        assert np.array_equal(k["kp_point"], t)
    q = s["key_frames"][s["query"]]
    for c, (qk, ck, _) in enumerate(s["shared"]):
        if len(qk):
            d = match_ref.hamming(q["desc"][qk], s["key_frames"][c]["desc"][ck])
            assert d.diagonal().max() <= 30 and (s["key_frames"][c]["kp_point"][ck] >= 0).all()


def test_relabel_moves_everything_together():
    s = S.scene("paths")
    rng = np.random.default_rng(0)
    for kf in (0, s["query"]):
        perm = rng.permutation(len(s["key_frames"][kf]["kp"]))
        t = S.relabel(s, kf, perm)
        _consistent(t)
        a, b = s["key_frames"][kf], t["key_frames"][kf]
        for n in ("kp", "desc", "kp_point"):
            assert np.array_equal(b[n], a[n][perm])
        assert t["points"] is s["points"] and all(t["key_frames"][o] is s["key_frames"][o] for o in range(len(s["key_frames"])) if o != kf)
        back = S.relabel(t, kf, np.argsort(perm))
        assert all(np.array_equal(back["key_frames"][kf][n], a[n]) for n in ("kp", "desc", "kp_point")) and back["observations"] == s["observations"]
    _consistent(s)                                                      # the original is untouched


def test_chunk_edges_has_every_pattern():
    s = S.envelope_scene("chunk_edges")
    _consistent(s)
    assert len(s["shared"]) == 9 and len(s["key_frames"][s["query"]]["kp"]) == 50
    for c, (n, at) in enumerate(zip(S.CHUNK_EDGES_N, S.CHUNK_EDGES_AT)):
        k = s["key_frames"][c]
        assert len(k["kp"]) == n and np.array_equal(L.candidate_rows(k["kp_point"]), at), c
    assert sorted(set(S.CHUNK_EDGES_N)) == [1, 255, 256, 257, 511, 512, 513, 768]
    refs = S.envelope_reference("chunk_edges")                          # the two with shared rows reach PnP across the chunks
    assert [r["correspondences"] for r in refs] == [0, 20, 0, 0, 0, 20, 0, 0, 0]
    assert refs[1]["rows"][refs[1]["mt"]].max() >= 256 and refs[5]["rows"][refs[5]["mt"]].max() >= 512


def test_gather_scenes_fill_their_verifiers():
    s = S.envelope_scene("tight")
    _consistent(s)
    assert [len(k["kp"]) for k in s["key_frames"]] == [300, 300, 300]
    assert [len(L.candidate_rows(s["key_frames"][c]["kp_point"])) for c in (0, 1)] == [300, 299]
    s = S.envelope_scene("one")
    assert [len(k["kp"]) for k in s["key_frames"]] == [1, 1] and L.candidate_rows(s["key_frames"][0]["kp_point"]).tolist() == [0]
    r = S.envelope_reference("one")[0]
    assert (r["status"], r["correspondences"], r["listed"]) == (1, 1, 1)
    s = S.envelope_scene("wide")
    _consistent(s)
    assert [len(k["kp"]) for k in s["key_frames"]] == [8192, 400, 300, 8192] and s["query"] == 2
    assert [len(L.candidate_rows(s["key_frames"][c]["kp_point"])) for c in (0, 1)] == [8192, 200]
    t = S.envelope_scene("wide", "q8192")
    assert t["query"] == 3 and t["key_frames"] is s["key_frames"]
    # the second query's own 300 rows match as the first's do, its 7892 random rows match nothing
    for a, b in zip(S.envelope_reference("wide"), S.envelope_reference("wide", "q8192")):
        assert a["status"] == b["status"] == 0 and np.array_equal(a["mq"], b["mq"]) and np.array_equal(a["mt"], b["mt"])


def test_gate_has_eleven_and_twelve_matches_of_many_rows():
    s, refs = S.envelope_scene("gate"), S.envelope_reference("gate")
    assert all(len(r["rows"]) == 400 for r in refs)
    assert [r["correspondences"] for r in refs] == [11, 12, 12, 12]
    assert [r["status"] for r in refs] == [1, 0, 2, 0] and not any(r["ok"] for r in refs)
    assert 0 < refs[1]["inliers"] <= 12 and 0 < refs[3]["inliers"] <= 12 and float(refs[3]["spread"]) < 0.25 <= float(refs[1]["spread"])
    assert (refs[0]["listed"], refs[2]["listed"]) == (11, 12)
    assert all(S.decided(s, r) for r in refs)


def test_bounds_sit_on_the_inclusive_bounds():
    s, refs = S.envelope_scene("bounds"), S.envelope_reference("bounds")
    assert [(r["inliers"], r["correspondences"], r["ok"]) for r in refs] == S.EXPECT_BOUNDS
    assert all(r["status"] == 0 and int(S.near_threshold(s, r).sum()) == 0 and S.decided(s, r, cap=0) for r in refs)
    assert all(float(r["spread"]) > 0.5 for r in refs)                  # the spread decides nothing here
    assert [r["inliers"] for r in refs[:3]] == [L.MIN_PNP_INLIERS - 1, L.MIN_PNP_INLIERS, L.MIN_PNP_INLIERS + 1]
    ratio = [f32(f32(r["inliers"]) / f32(r["correspondences"])) for r in refs[3:]]
    assert ratio[0] < L.MIN_PNP_INLIER_RATIO and _bits(ratio[1]) == _bits(L.MIN_PNP_INLIER_RATIO) and ratio[2] > L.MIN_PNP_INLIER_RATIO
    assert all(r["inliers"] >= L.MIN_PNP_INLIERS for r in refs[3:])     # there the ratio alone decides


def test_listing_goes_beyond_one_stride_and_relabelling_is_verdict_neutral():
    s, refs = S.envelope_scene("listing"), S.envelope_reference("listing")
    assert refs[0]["status"] == 0 and refs[0]["listed"] > 512 and refs[0]["listed"] % 64 != 0
    assert refs[1]["status"] == 2 and refs[1]["listed"] == refs[1]["correspondences"] > 256
    assert all(S.decided(s, r) for r in refs)
    triples = lambda r, perm: {(int(perm[q]), int(p), int(c)) for q, p, c in zip(r["query_kp"], r["point"], r["candidate_kp"])}      # noqa: E731
    base = [triples(r, np.arange(1000)) for r in refs]
    x = s["key_frames"][s["query"]]["kp"][refs[0]["query_kp"], 0]
    where = {}
    for form in S.LISTING_FORMS:
        t, got, perm = S.envelope_scene("listing", form), S.envelope_reference("listing", form), S.listing_perm(form)
        _consistent(t)
        for r, g, b in zip(refs, got, base):
            assert (g["status"], g["correspondences"], g["inliers"], g["listed"], g["ok"]) == (r["status"], r["correspondences"], r["inliers"], r["listed"], r["ok"])
            assert _bits(g["spread"]) == _bits(r["spread"]) and triples(g, perm) == b
            assert S.decided(t, g)
        gx = t["key_frames"][t["query"]]["kp"][got[0]["query_kp"], 0]
        assert gx.min() == x.min() and gx.max() == x.max()
        where[form] = sorted((int(np.argmin(gx)), int(np.argmax(gx))))
    n = refs[0]["listed"]
    assert where["last"] == [n - 2, n - 1] and n - 2 >= 512             # the tail stride, which not every thread takes
    assert where["first"] == [0, 1]
    assert all(k >= 256 and k % 256 >= 192 for k in where["wave3"])     # wave 3 of the second stride


def test_the_parameter_table_keeps_what_is_decided():
    s = S.scene("paths")
    assert len(S.PARAMETERS) == 11
    for i, (kw, kept) in enumerate(S.PARAMETERS):
        refs = S.parameter_reference(i)
        assert kept == tuple(c for c in (0, 6) if S.decided(s, refs[c])), (kw, kept)
        if kw.get("max_distance") == 0:
            assert [refs[c]["status"] for c in (0, 6)] == [1, 1]
    by = {tuple(kw.items()): S.parameter_reference(i) for i, (kw, _) in enumerate(S.PARAMETERS)}
    # every parameter changes something the verifier returns, so an argument that did not reach its stage would show
    assert by[(("max_distance", 8),)][0]["correspondences"] < by[(("max_distance", 64),)][0]["correspondences"]
    assert by[(("threshold_px", 0.5),)][0]["inliers"] < by[(("threshold_px", 4.0),)][0]["inliers"]
    assert by[(("threshold_px", 50.0),)][6]["inliers"] > by[(("threshold_px", 4.0),)][6]["inliers"]
    assert by[(("max_hypotheses", 1),)][0]["status"] == 2 and by[(("max_hypotheses", 200),)][0]["status"] == 0


def test_the_chain_sequence_is_what_it_says():
    """test_a_chain_forgets_its_last_candidate: 700 inliers, then status 2, status 1 with 11 matches, nt = 0, verified."""
    refs = S.reference("paths")
    assert S.envelope_reference("listing")[0]["inliers"] == 700
    assert [(refs[c]["status"], refs[c]["correspondences"] if c == 3 else len(refs[c]["rows"]) if c == 1 else None) for c in (4, 3, 1, 0)] == \
        [(2, None), (1, 11), (1, 0), (0, None)]
    assert refs[0]["ok"]
