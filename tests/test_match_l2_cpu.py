"""The float-descriptor (L2) matchers without a GPU: the restatement's exact float32 fma against libm, its two distance
forms against a float64 referee within bounds that are derived (tests/match_l2_ref.py: dot_bound, diff_bound), its tie and
filter rules on constructed rows, and the boundary: the new entry points are exported and refuse a NULL context."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import match_cases as MC
import match_l2_cases as LC
import match_l2_ref as LR

F = np.float32
NEW = ("rs_l2_knn2", "rs_match_descriptors_f32", "rs_reproj_match_l2")


def _libm_fmaf():
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = C.c_float
    m.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
    return m.fmaf


def _triples():
    rng = np.random.default_rng(11)
    n = 20000
    a = (rng.normal(0, 1, n) * 2.0 ** rng.integers(-20, 20, n)).astype(F)
    b = (rng.normal(0, 1, n) * 2.0 ** rng.integers(-20, 20, n)).astype(F)
    c = (rng.normal(0, 1, n) * 2.0 ** rng.integers(-40, 40, n)).astype(F)
    sets = [(a, b, c)]
    # near-cancelling: c = -(a b) rounded, and its neighbours
    ab = (a.astype(np.float64) * b.astype(np.float64)).astype(F)
    for step in (0, 1, -1):
        sets.append((a, b, np.nextafter(-ab, F(np.inf) * step) if step else -ab))
    # midpoint-near: a b = 2^-24-ish against c = 1, so that a b + c sits at or next to a float32 rounding midpoint
    x = (1.0 + rng.integers(0, 1 << 23, n) * 2.0 ** -23).astype(F)
    half = np.full(n, 2.0 ** -24, F)
    for y in (half, np.nextafter(half, F(1)), np.nextafter(half, F(0)), F(3) * half):
        sets.append((np.ones(n, F), y, x))
        sets.append((x, y, x))
    return sets


def test_fma32_equals_libm_fmaf_bitwise():
    fmaf = _libm_fmaf()
    for a, b, c in _triples():
        got = LR.fma32(a, b, c)
        ref = np.array([fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("dim", [4, 8, 64, 128, 256, 260, 1024])
@pytest.mark.parametrize("kind", ["unit", "raw"])
def test_d_dot_within_the_derived_bound(dim, kind):
    q, t = LC.knn_set(24, 40, dim, seed=dim, kind=kind)
    d2 = LR.dot_d2(q[0], t[0]).astype(np.float64)
    err = np.abs(d2 - LR.d2_f64(q[0], t[0]))
    bound = LR.dot_bound(q[0], t[0])
    assert (err <= bound).all(), float((err / bound).max())
    assert (d2 >= 0).all()


@pytest.mark.parametrize("dim", [4, 8, 64, 128, 256, 260, 1024])
@pytest.mark.parametrize("kind", ["unit", "raw"])
def test_d_diff_within_the_derived_bound(dim, kind):
    q, t = LC.knn_set(24, 40, dim, seed=1000 + dim, kind=kind)
    d2 = LR.diff_d2(q[0], t[0]).astype(np.float64)
    exact = LR.d2_f64(q[0], t[0])
    assert (np.abs(d2 - exact) <= LR.diff_bound(q[0], t[0])).all()
    same = np.all(q[0][:, None, :] == t[0][None, :, :], axis=-1)
    assert same.any() and (d2[same] == 0).all()                     # a query that is a train row: exactly 0


def test_knn2_tie_goes_to_the_lower_index_and_filters():
    rng = np.random.default_rng(3)
    t = LC.unit_rows(rng, 10, 64)
    t[7] = t[2]
    q = t[[7, 4]]
    i0, d0, i1, d1 = LR.knn2_l2(q, t)
    assert list(i0) == [2, 4] and i1[0] == 7 and d0[0] == d1[0]
    # q = 0, t0 = 3 e0, t1 = 4 e0: dist0 == 0.75f * dist1 exactly, accepted; max_distance == dist0 accepted, one ulp below rejected
    e = np.zeros((3, 8), F)
    e[0, 0], e[1, 0] = 3, 4
    i0, d0, i1, d1 = LR.knn2_l2(e[2:], e[:2])
    assert (i0[0], d0[0], i1[0], d1[0]) == (0, 3.0, 1, 4.0)
    assert len(LR.match_descriptors_l2(e[2:], e[:2], 3.0)[0]) == 1
    assert len(LR.match_descriptors_l2(e[2:], e[:2], np.nextafter(F(3), F(0)))[0]) == 0
    e[1, 0] = np.nextafter(F(4), F(0))
    assert len(LR.match_descriptors_l2(e[2:], e[:2], 3.0)[0]) == 0
    one = LR.knn2_l2(e[2:], e[:1])
    assert one[2][0] == -1 and one[3][0] == -1.0 and len(LR.match_descriptors_l2(e[2:], e[:1], 3.0)[0]) == 1


@pytest.mark.parametrize("dim", [8, 260, 1024])
def test_restatement_is_exact_on_integer_rows(dim):
    """On rows of small integers nothing rounds: the restatement must give the integer arithmetic's answer."""
    q, t, d2 = LC.integer_set(20, 70, dim, seed=dim)
    assert np.array_equal(LR.dot_d2(q[0], t[0]).astype(np.int64), d2[0])
    assert np.array_equal(LR.diff_d2(q[0], t[0]).astype(np.int64), d2[0])
    for g, r in zip(LR.knn2_l2(q[0], t[0]), LC.integer_knn2(d2[0])):
        assert np.array_equal(LR.bits(g), LR.bits(r))


def test_reproj_restatement_on_a_disc_scene(rs):
    """Equal rows inside a disc tie and the walk order decides; a duplicated point loses to its original."""
    frame, mp, fdesc, pool, dim, _ = LC.reproj_case("discs-d128", rs.kdtree_build)
    ref = LR.reproj_match_l2(frame, mp, fdesc, pool, 0, 1.0)
    assert ref["tied_points"] > 0 and len(ref["match_kp"]) > 0
    won = ref["prop_point"][ref["match_kp"]]
    mp2 = LC.duplicate_points(mp, won[:5])
    ref2 = LR.reproj_match_l2(frame, mp2, fdesc, pool, 0, 1.0)
    P = len(mp["positions"])
    assert np.array_equal(ref2["point_kp"][P:], ref2["point_kp"][won[:5]]) and (ref2["point_kp"][P:] >= 0).all()
    assert np.array_equal(ref2["prop_point"], ref["prop_point"])
    assert len(LR.reproj_match_l2(frame, mp, fdesc, pool, 0, 0.0)["match_kp"]) == 0
    # without noise the float rows reproduce the bit rows' ordering: d2 = 4 c^2 x Hamming distance, exactly
    h = MC.descriptors(np.random.default_rng(1), 6)
    d2 = LR.diff_d2(LC.float_rows(h, 128), LC.float_rows(h, 128))
    ham = np.unpackbits(h[:, None, :16] ^ h[None, :, :16], axis=-1).sum(-1)
    c = 2.0 ** np.round(-0.5 * np.log2(128))
    assert np.array_equal(d2, (4.0 * c * c * ham).astype(F))


def test_new_symbols_are_exported_and_refuse_a_null_context(rs):
    lib = rs.load()
    for name in NEW:
        assert name in rs.EXPORTS and hasattr(lib, name), name
    z = [None] * 4
    assert lib.rs_l2_knn2(None, None, 4, None, 4, 128, 1, *z) == 1
    assert lib.rs_match_descriptors_f32(None, None, 4, None, 4, 128, 1, 0.5, None, None, None, *z) == 1
    assert lib.rs_reproj_match_l2(None, None, None, None, None, 128, 0, 0.5, *([None] * 7)) == 1
