"""tests/match_ref.py (the independent numpy restatement of the matchers) against the CPU oracle, over the shapes of
tests/test_gpu_match_envelope.py: a wrong reference is caught here, before it judges the GPU.  The kNN cases use smaller
stand-ins where numpy would be slow; the reprojection cases are the GPU file's own scenes."""
import numpy as np
import pytest

import match_cases as MC
import match_ref as MR


def _knn_equal(oracle, q, t):
    got = MR.knn2(q, t)
    ref = oracle.hamming_knn2(q, t)
    for g, r, name in zip(got, ref, ("idx0", "dist0", "idx1", "dist1")):
        assert np.array_equal(g, r), name


@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 2), (63, 31), (64, 32), (65, 33), (4097, 64), (9000, 33), (5, 65536),
                                   (2, (1 << 20) - 1)])
def test_knn2_matches_oracle(oracle, nq, nt):
    q, t = MC.knn_set(nq, nt)
    _knn_equal(oracle, q[0], t[0])


def test_knn2_ties_and_complements(oracle):
    rng = np.random.default_rng(5)
    t = MC.descriptors(rng, 300)
    t[200] = t[17]                   # rank-1 tie
    t[250] = t[17]
    q = np.stack([t[17], ~t[40], t[3]])
    t[120] = MC.flip_bits(rng, t[3:4], [5])[0]      # rank-2 tie at distance 5
    t[260] = t[120]
    _knn_equal(oracle, q, t)
    i0, d0, i1, d1 = MR.knn2(q, t)
    assert (i0[0], d0[0], i1[0], d1[0]) == (17, 0, 200, 0)
    assert d0[1] <= 256 and MR.knn2(q[1:2], t[40:41])[1][0] == 256
    assert (i0[2], i1[2], d1[2]) == (3, 120, 5)


@pytest.mark.parametrize("max_distance", [-1, 0, 1, 63, 64, 65, 255, 256])
def test_match_descriptors_matches_oracle(oracle, max_distance):
    q, t = MC.knn_set(700, 500, seed=3)
    gq, gt = MR.match_descriptors(q[0], t[0], max_distance)
    rq, rt = oracle.match_descriptors(q[0], t[0], max_distance)
    assert np.array_equal(gq, rq) and np.array_equal(gt, rt)
    if max_distance >= 64:
        assert len(gq) > 50


def test_match_descriptors_filter_edges(oracle):
    """d0 == max_distance (kept), 4 d0 == 3 d1 (kept), 4 d0 == 3 d1 + 1 (dropped), one train row (no ratio test)."""
    rng = np.random.default_rng(8)
    base = MC.descriptors(rng, 1)
    t = np.concatenate([MC.flip_bits(rng, base, [30]), MC.flip_bits(rng, base, [40])])
    q = np.concatenate([base, base])
    for md, want in ((30, 2), (29, 0)):
        gq, _ = MR.match_descriptors(q, t, md)
        assert len(gq) == want
        assert np.array_equal(gq, oracle.match_descriptors(q, t, md)[0])
    _, d0, _, d1 = MR.knn2(q, t)
    assert 4 * d0[0] == 3 * d1[0]


@pytest.mark.parametrize("name", list(MC.REPROJ))
def test_reproj_reference_matches_oracle(oracle, name):
    frame, mp, runs = MC.reproj_case(name, oracle.kdtree_build)
    P, N = len(mp["positions"]), len(frame["keypoints"])
    for replace, md in runs:
        ref = MR.reproj_match(frame, mp, replace, md)
        got = oracle.reproj_match(frame, mp, replace=replace, max_distance=md)
        MR.assert_reproj_equal(got, ref, f"{name} replace={replace} max_distance={md}: ")
        if name == "geom-edges":            # built on the edges on purpose: test_reproj_reference_edges_and_empty_points
            continue
        # the boundary set is a few points, not a fraction of the map: otherwise the comparison checks nothing
        assert len(ref["boundary_points"]) <= 0.01 * P + 8, len(ref["boundary_points"])
        assert len(ref["boundary_kps"]) <= 0.1 * N + 32, len(ref["boundary_kps"])


def test_reproj_reference_edges_and_empty_points(oracle):
    """u == 0 / v == 0 accepted, u == width / v == height rejected (float32 lands exactly there), points behind the
    camera rejected, eligible points with no observations rejected without a NaN."""
    frame, mp, _ = MC.reproj_case("geom-edges", oracle.kdtree_build)
    u, v, z = MC.project_f32(frame, mp["positions"])
    n = len(MC.EDGE_UV)
    for i, (eu, ev, _) in enumerate(MC.EDGE_UV):
        assert u[i] == np.float32(eu) and v[i] == np.float32(ev) and z[i] > 0
        assert u[n + i] == np.float32(eu) and v[n + i] == np.float32(ev) and z[n + i] < 0
    ref = oracle.reproj_match(frame, mp, replace=0)
    accepted = np.array([a for _, _, a in MC.EDGE_UV])
    assert np.array_equal(ref["point_kp"][:n] >= 0, accepted)
    assert np.all(ref["point_kp"][n:] == -1)
    # eligible, in view, no observations
    mp2 = dict(mp, obs_ptr=np.zeros(len(mp["positions"]) + 1, np.int32))
    with np.errstate(all="raise"):
        r2 = MR.reproj_match(frame, mp2, 1, 64)
    assert np.all(r2["point_kp"] == -1) and len(r2["boundary_points"]) == 0
    assert np.all(oracle.reproj_match(frame, mp2, replace=1)["point_kp"] == -1)
