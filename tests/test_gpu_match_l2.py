"""K12 (rs_l2_knn2, rs_match_descriptors_f32) and K13 (rs_reproj_match_l2) on the GPU: indices, distance BITS, counts and
compacted lists against the numpy restatement (tests/match_l2_ref.py, pinned on the CPU by tests/test_match_l2_cpu.py);
the reprojection matcher outside the restatement's boundary set (its gates are match_ref's float64 ones).

K12: sizes on both sides of the 32-row MFMA tile, the 128-row pass and the train splits; every k-chunk shape (dim below,
at, and not a multiple of 32, up to 1024); batches; equal train rows across every tile boundary; queries that are train
rows (the clamp); the filter edges; sentinel-filled outputs; two runs; the float64 referee.
K13: workgroup-edge point counts, 1 .. 9 observations, discs with more candidates than the queue holds, equal rows inside
a disc, equally distant points, matched keypoints, ineligible points, replace, max_distance <= 0 and huge."""
import ctypes as C

import numpy as np
import pytest

import match_l2_cases as LC
import match_l2_ref as LR
from conftest import to_np

pytestmark = pytest.mark.gpu
F = np.float32
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _bits_equal(a, b):
    return np.array_equal(LR.bits(np.asarray(a)), LR.bits(np.asarray(b)))


# ------------------------------------------------------------------------------------------------------------ K12
def _knn_check(ctx, q, t, max_distance, key):
    """q [B][nq][dim], t [B][nt][dim]: raw 2-NN, the filtered lists with and without the raw outputs, twice."""
    B, nq, dim = q.shape
    nt = t.shape[1]
    refs = _cached(("knn", key), lambda: [LR.knn2_l2(q[b], t[b]) for b in range(B)])
    dq, dt = ctx.dev(q), ctx.dev(t)
    raw = [to_np(x) for x in ctx.l2_knn2(dq, dt, nq, nt, dim, batch=B)]
    m = ctx.match_descriptors_f32(dq, dt, nq, nt, dim, batch=B, max_distance=max_distance, raw=True)
    m2 = ctx.match_descriptors_f32(dq, dt, nq, nt, dim, batch=B, max_distance=max_distance)
    raw2 = [to_np(x) for x in m["raw"]]
    cnt, mq, mt = to_np(m["cnt"]), to_np(m["mq"]), to_np(m["mt"])
    cnt2, mq2, mt2 = to_np(m2["cnt"]), to_np(m2["mq"]), to_np(m2["mt"])
    for b in range(B):
        for g, g2, r, name in zip(raw, raw2, refs[b], ("idx0", "dist0", "idx1", "dist1")):
            assert _bits_equal(g[b, :nq], r), f"item {b} {name} vs the restatement"
            assert _bits_equal(g2[b, :nq], r), f"item {b} {name} (second run) vs the restatement"
        rq, rt = LR.match_descriptors_l2(q[b], t[b], max_distance, knn=refs[b])
        for c, lq, lt in ((cnt, mq, mt), (cnt2, mq2, mt2)):
            assert c[b] == len(rq), f"item {b}: {c[b]} matches, the restatement has {len(rq)}"
            assert np.array_equal(lq[b, :c[b]], rq) and np.array_equal(lt[b, :c[b]], rt), f"item {b} match list"
    return refs


@pytest.mark.parametrize("nq,nt,dim", [(70, 300, 8), (33, 257, 260), (70, 300, 1024), (257, 33, 64)])
def test_fragment_maps_on_exact_integer_rows(ctx, nq, nt, dim):
    """The MFMA lane and register maps, the zero padding and the masks, apart from rounding: rows of small integers, every
    row different and the two operands unrelated, so float32 is exact in any order and the expected answer is integer
    arithmetic (match_l2_cases.integer_knn2), not the fma restatement.  A transposed operand, a wrong row formula of the
    accumulator or an unmasked padding row reports another index or distance here."""
    B = 2
    q, t, d2 = LC.integer_set(nq, nt, dim, batch=B, seed=1)
    got = [to_np(x) for x in ctx.l2_knn2(ctx.dev(q), ctx.dev(t), nq, nt, dim, batch=B)]
    for b in range(B):
        for g, r, name in zip(got, LC.integer_knn2(d2[b]), ("idx0", "dist0", "idx1", "dist1")):
            assert _bits_equal(g[b, :nq], r), f"item {b} {name} vs integer arithmetic"


_EDGE = (1, 2, 31, 32, 33, 63, 64, 65, 257)
@pytest.mark.parametrize("nt", _EDGE)
@pytest.mark.parametrize("nq", _EDGE)
def test_knn_tile_edges(ctx, nq, nt):
    q, t = LC.knn_set(nq, nt, 64)
    _knn_check(ctx, q, t, 0.6, ("shape", nq, nt))


@pytest.mark.parametrize("dim", [4, 8, 64, 128, 256, 260, 1024])
@pytest.mark.parametrize("kind", ["unit", "raw"])
def test_knn_dims(ctx, dim, kind):
    q, t = LC.knn_set(65, 257, dim, seed=1, kind=kind)
    refs = _knn_check(ctx, q, t, 0.6 if kind == "unit" else 3.0, ("dim", dim, kind))
    i0, d0 = refs[0][0], refs[0][1]
    assert (d0 == 0).any(), "no query is a train row: the clamp is not exercised"
    # the float64 referee: d2 within the derived bound; dist = sqrt(d2) rounded once, so dist^2 adds 3 u d2 at most
    exact = LR.d2_f64(q[0], t[0])[np.arange(65), i0]
    got = to_np(ctx.l2_knn2(ctx.dev(q), ctx.dev(t), 65, 257, dim)[1])[0].astype(np.float64) ** 2
    bound = LR.dot_bound(q[0], t[0])[np.arange(65), i0] + 3 * LR.U * exact
    assert (np.abs(got - exact) <= bound).all()


@pytest.mark.parametrize("dim", [0, 3, 1028, -4, 6])
def test_unsupported_dim_is_refused_and_the_context_stays_usable(ctx, rs, dim):
    q, t = LC.knn_set(5, 7, 8)
    dq, dt = ctx.dev(q), ctx.dev(t)
    o = [ctx.empty((1, 5), d) for d in (ctx.torch.int32, ctx.torch.float32, ctx.torch.int32, ctx.torch.float32)]
    p = [C.c_void_p(x.data_ptr()) for x in o]
    lib = ctx.lib
    assert lib.rs_l2_knn2(ctx.h, C.c_void_p(dq.data_ptr()), 5, C.c_void_p(dt.data_ptr()), 7, dim, 1, *p) == 4
    assert lib.rs_match_descriptors_f32(ctx.h, C.c_void_p(dq.data_ptr()), 5, C.c_void_p(dt.data_ptr()), 7, dim, 1, 0.5, p[0], p[0], p[0], *p) == 4
    with pytest.raises(rs.RsError):
        ctx.l2_knn2(dq, dt, 5, 7, dim)
    # row counts whose rounding up to a 128-row pass would leave int: refused before anything is read
    for nq, nt in ((5, 2 ** 31 - 1), (5, 2 ** 31 - 128), (2 ** 31 - 1, 7)):
        assert lib.rs_l2_knn2(ctx.h, C.c_void_p(dq.data_ptr()), nq, C.c_void_p(dt.data_ptr()), nt, 8, 1, *p) == 4
    _knn_check(ctx, q, t, 0.6, "after-refusal")


@pytest.mark.parametrize("batch,nq,nt,dim", [(1, 40, 300, 8), (3, 40, 300, 8), (8, 40, 300, 8), (3, 33, 130, 128), (8, 2100, 700, 4)])
def test_knn_batches_and_splits(ctx, batch, nq, nt, dim):
    """(8, 2100, 700): 528 query blocks leave two train splits of three 128-row passes each."""
    q, t = LC.knn_set(nq, nt, dim, batch=batch, seed=batch)
    _knn_check(ctx, q, t, 0.6, ("batch", batch, nq, nt, dim))


@pytest.mark.parametrize("batch,nq,nt", [(1, 70, 700), (8, 2100, 700)])
def test_equal_train_rows_across_every_boundary(ctx, batch, nq, nt):
    """Rows B - 1 and B are equal for every multiple B of 32 (tiles, the four waves, 128-row passes, the splits), and rows 3
    and nt - 1: each pair is the exact best of a query, the lower index must be reported first and the higher second."""
    dim = 4
    q, t = LC.knn_set(nq, nt, dim, batch=batch, seed=9)
    bounds = list(range(32, nt, 32))
    for b in range(batch):
        for j, B in enumerate(bounds):
            t[b, B] = t[b, B - 1]
            q[b, j] = t[b, B]
        t[b, nt - 1] = t[b, 3]
        q[b, len(bounds)] = t[b, 3]
    refs = _knn_check(ctx, q, t, 0.6, ("ties", batch, nq, nt))
    for b in range(batch):
        i0, d0, i1, d1 = refs[b]
        assert list(i0[:len(bounds)]) == [B - 1 for B in bounds] and list(i1[:len(bounds)]) == bounds
        assert (i0[len(bounds)], i1[len(bounds)]) == (3, nt - 1) and (d0[:len(bounds) + 1] == d1[:len(bounds) + 1]).all()


def test_filter_edges(ctx):
    e = np.zeros((1, 3, 8), F)
    e[0, 0, 0], e[0, 1, 0] = 3, 4
    q, t = e[:, 2:], e[:, :2]
    dq, dt = ctx.dev(q), ctx.dev(t)

    def count(md, tt=dt, nt=2):
        return int(to_np(ctx.match_descriptors_f32(dq, tt, 1, nt, 8, max_distance=md)["cnt"])[0])
    raw = [to_np(x)[0, 0] for x in ctx.l2_knn2(dq, dt, 1, 2, 8)]
    assert raw == [0, 3.0, 1, 4.0]
    assert count(3.0) == 1                                   # dist0 == max_distance and dist0 == 0.75f * dist1: accepted
    assert count(float(np.nextafter(F(3), F(0)))) == 0       # max_distance one ulp below dist0
    assert count(float("nan")) == 0
    t2 = t.copy()
    t2[0, 1, 0] = np.nextafter(F(4), F(0))                   # dist0 > 0.75f * dist1 by one ulp of dist1
    assert count(3.0, ctx.dev(t2)) == 0
    one = [to_np(x)[0, 0] for x in ctx.l2_knn2(dq, dt, 1, 1, 8)]
    assert one == [0, 3.0, -1, -1.0] and count(3.0, dt, 1) == 1      # nt == 1: no ratio test


def test_outputs_are_written_inside_their_contract_only(ctx):
    T = ctx.torch
    B, nq, nt, dim, pad = 3, 37, 50, 8, 64
    q, t = LC.knn_set(nq, nt, dim, batch=B, seed=4)
    dq, dt = ctx.dev(q), ctx.dev(t)

    def sentinel(n, dtype):
        return T.full((n,), -7, dtype=dtype, device=ctx.device)
    kinds = (T.int32, T.float32, T.int32, T.float32)
    for a, b in ((0, nt), (nq, 0)):                          # nothing is written; the filtered call zeroes the counts
        raw = [sentinel(B * nq + pad, k) for k in kinds]
        out = dict(mq=sentinel(B * nq + pad, T.int32), mt=sentinel(B * nq + pad, T.int32), cnt=sentinel(B + pad, T.int32), raw=raw)
        ctx._check(ctx.lib.rs_l2_knn2(ctx.h, C.c_void_p(dq.data_ptr()), a, C.c_void_p(dt.data_ptr()), b, dim, B,
                                      *[C.c_void_p(x.data_ptr()) for x in raw]), "rs_l2_knn2")
        assert all((to_np(x) == -7).all() for x in raw)
        ctx.match_descriptors_f32(dq, dt, a, b, dim, batch=B, max_distance=0.6, out=out)
        assert all((to_np(x) == -7).all() for x in raw + [out["mq"], out["mt"]])
        assert (to_np(out["cnt"])[:B] == 0).all() and (to_np(out["cnt"])[B:] == -7).all()
    raw = [sentinel(B * nq + pad, k) for k in kinds]
    out = dict(mq=sentinel(B * nq + pad, T.int32), mt=sentinel(B * nq + pad, T.int32), cnt=sentinel(B + pad, T.int32), raw=raw)
    ctx.match_descriptors_f32(dq, dt, nq, nt, dim, batch=B, max_distance=0.6, out=out)
    cnt = to_np(out["cnt"])
    assert (cnt[B:] == -7).all()
    for x in raw + [out["mq"], out["mt"]]:
        assert (to_np(x)[B * nq:] == -7).all()
    for b in range(B):
        r = LR.knn2_l2(q[b], t[b])
        for g, rr in zip(raw, r):
            assert _bits_equal(to_np(g)[b * nq:(b + 1) * nq], rr)
        rq, _ = LR.match_descriptors_l2(q[b], t[b], 0.6, knn=r)
        assert cnt[b] == len(rq) and np.array_equal(to_np(out["mq"])[b * nq:b * nq + cnt[b]], rq)


# ------------------------------------------------------------------------------------------------------------ K13
def _reproj_gpu(ctx, frame, mp, fdesc, pool, dim, replace, md):
    fv, k1 = ctx.make_frame_view(frame)
    mv, k2 = ctx.make_map_view(mp)
    fv.d_descriptors = None                     # the u8 pointers, the packed tree and the grid are not read
    mv.d_desc_pool = None
    o = ctx.reproj_match_l2(fv, mv, ctx.dev(fdesc), ctx.dev(pool), dim, replace=replace, max_distance=md)
    P, N = len(mp["positions"]), len(frame["keypoints"])
    n = int(to_np(o["count"])[0])
    return dict(point_kp=to_np(o["point_kp"])[:P], point_dist=to_np(o["point_dist"])[:P], prop_point=to_np(o["prop_point"])[:N],
                prop_dist=to_np(o["prop_dist"])[:N], match_kp=to_np(o["match_kp"])[:n], match_point=to_np(o["match_point"])[:n])


@pytest.mark.parametrize("name", sorted(LC.REPROJ))
def test_reproj_cases(ctx, rs, name):
    frame, mp, fdesc, pool, dim, runs = _cached(("scene", name), lambda: LC.reproj_case(name, rs.kdtree_build))
    P, N = len(mp["positions"]), len(frame["keypoints"])
    checked = 0
    for replace, md in runs:
        ref = _cached(("reproj", name, replace, md), lambda: LR.reproj_match_l2(frame, mp, fdesc, pool, replace, md))
        got = _reproj_gpu(ctx, frame, mp, fdesc, pool, dim, replace, md)
        LR.assert_reproj_equal(got, ref, f"{name} replace {replace} max_distance {md}: ")
        again = _reproj_gpu(ctx, frame, mp, fdesc, pool, dim, replace, md)
        assert all(_bits_equal(got[k], again[k]) for k in got), "two runs differ"
        if md <= 0:
            assert len(got["match_kp"]) == 0 and (got["point_kp"] == -1).all() and (got["prop_point"] == -1).all()
            assert _bits_equal(got["point_dist"], np.full(P, md, F)) and _bits_equal(got["prop_dist"], np.full(N, md, F))
        checked += len(ref["match_kp"])
        # the restatement vouches for most of the scene (the edge scene puts its points ON the image border)
        assert name.startswith("edges") or len(ref["boundary_points"]) <= max(2, P // 10), len(ref["boundary_points"])
    if name.startswith("discs"):
        assert _CACHE[("reproj", name, 0, 1.0)]["tied_points"] > 0 or dim == 256
    if not name.startswith(("elig-none", "matched-all", "P1-", "P200-N1-", "edges")):
        assert checked > 0, "the case matches nothing: it checks nothing"


def test_equally_distant_points_go_to_the_lower_map_index(ctx, rs):
    frame, mp, fdesc, pool, dim, _ = _cached(("scene", "discs-d128"), lambda: LC.reproj_case("discs-d128", rs.kdtree_build))
    base = _reproj_gpu(ctx, frame, mp, fdesc, pool, dim, 0, 1.0)
    won = base["match_point"][:8]
    mp2 = LC.duplicate_points(mp, won)
    got = _reproj_gpu(ctx, frame, mp2, fdesc, pool, dim, 0, 1.0)
    P = len(mp["positions"])
    assert np.array_equal(got["point_kp"][P:], got["point_kp"][won]) and (got["point_kp"][P:] >= 0).all()
    assert _bits_equal(got["point_dist"][P:], got["point_dist"][won])
    assert np.array_equal(got["prop_point"], base["prop_point"]) and np.array_equal(got["match_point"], base["match_point"])
    LR.assert_reproj_equal(got, LR.reproj_match_l2(frame, mp2, fdesc, pool, 0, 1.0), "duplicated points: ")


def test_reproj_refuses_unsupported_dim_and_handles_empty_sides(ctx, rs):
    frame, mp, fdesc, pool, dim, _ = _cached(("scene", "P63-N300-d128"), lambda: LC.reproj_case("P63-N300-d128", rs.kdtree_build))
    fv, k1 = ctx.make_frame_view(frame)
    mv, k2 = ctx.make_map_view(mp)
    df, dp = ctx.dev(fdesc), ctx.dev(pool)
    for bad in (0, 3, 1028):
        with pytest.raises(rs.RsError, match="status 4"):
            ctx.reproj_match_l2(fv, mv, df, dp, bad)
    mv.n_points = 0
    o = ctx.reproj_match_l2(fv, mv, df, dp, dim)
    assert int(to_np(o["count"])[0]) == 0 and (to_np(o["prop_point"])[:300] == -1).all()
    mv.n_points = 63
    fv.n_keypoints = 0
    o = ctx.reproj_match_l2(fv, mv, df, dp, dim, max_distance=0.625)
    assert int(to_np(o["count"])[0]) == 0 and (to_np(o["point_kp"])[:63] == -1).all()
    assert (to_np(o["point_dist"])[:63] == F(0.625)).all()          # no keypoint: every point reports max_distance
    fv.n_keypoints = 300
    got = _reproj_gpu(ctx, frame, mp, fdesc, pool, dim, 0, 1.0)
    LR.assert_reproj_equal(got, LR.reproj_match_l2(frame, mp, fdesc, pool, 0, 1.0), "after the refusals: ")
