"""Numpy restatement of the float-descriptor (L2) matchers, for tests only: rs_l2_knn2, rs_match_descriptors_f32 and
rs_reproj_match_l2 as include/rsgpu.h specifies them, bit for bit in float32.

  fma32(a, b, c)          exact float32 fused multiply-add: the product of two float32 is exact in float64 (48 bits); c is
                          added with round-to-odd (TwoSum tells whether the float64 sum was inexact and in which direction),
                          and a round-to-odd float64 rounds to float32 as the exact sum would (53 >= 2 * 24 + 2)
  dot_d2(q, t)            "D-dot": s = fmaf chain over ascending k, d2 = max(fma(-2, s, nq2 + nt2), 0)      [nq][nt] float32
  diff_d2(a, b)           "D-diff": r[k & 3] = fmaf(e, e, r[k & 3]), e = a[k] - b[k]; d2 = (r0 + r1) + (r2 + r3)
  knn2_l2, match_descriptors_l2, reproj_match_l2      the three entry points
  d2_f64(q, t), dot_bound(q, t), diff_bound(q, t)     the float64 referee and the derived error bounds

Vectorised over pairs with a Python loop over k.  The gates and the walk order of reproj_match_l2 are match_ref's
(float64 with a boundary set the restatement does not vouch for)."""
import numpy as np

import match_ref as MR

F = np.float32
U = 2.0 ** -24


def fma32(a, b, c):
    a, b, c = np.asarray(a, F), np.asarray(b, F), np.asarray(c, F)
    with np.errstate(over="ignore", invalid="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(F)


def _chain(a, b):
    """fmaf chain over ascending k of a[..., k] * b[..., k] (broadcast over the leading axes), from 0."""
    s = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), F)
    for k in range(a.shape[-1]):
        s = fma32(a[..., k], b[..., k], s)
    return s


def row_norms(x):
    x = np.asarray(x, F)
    return _chain(x, x)


def dot_d2(q, t):
    q, t = np.asarray(q, F), np.asarray(t, F)
    s = _chain(q[:, None, :], t[None, :, :])
    with np.errstate(over="ignore", invalid="ignore"):
        n = row_norms(q)[:, None] + row_norms(t)[None, :]
        d2 = fma32(F(-2.0), s, n)
        return np.where(d2 > 0, d2, F(0.0)).astype(F)          # fmaxf(d2, 0): a NaN gives 0 as well


def diff_d2(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    r = [np.zeros((len(a), len(b)), F) for _ in range(4)]
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(a.shape[1]):
            e = a[:, None, k] - b[None, :, k]
            r[k & 3] = fma32(e, e, r[k & 3])
        return (r[0] + r[1]) + (r[2] + r[3])


def knn2_l2(q, t):
    """idx0, dist0, idx1, dist1 (float32 distances, pre-clamp order by (d2, index)); idx1 = -1, dist1 = -1 for one train row."""
    q, t = np.asarray(q, F), np.asarray(t, F)
    nq, nt = len(q), len(t)
    i0, i1 = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
    d0, d1 = np.full(nq, -1, F), np.full(nq, -1, F)
    if nq == 0 or nt == 0:
        return i0, d0, i1, d1
    d2 = dot_d2(q, t)
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(nt, dtype=np.uint64)[None, :]
    rows = np.arange(nq)
    i0[:] = np.argmin(key, axis=1)                    # keys are unique: d2 >= 0 orders as its bits do, then the index
    d0[:] = np.sqrt(d2[rows, i0])
    if nt >= 2:
        key[rows, i0] = np.uint64(0xFFFFFFFFFFFFFFFF)
        i1[:] = np.argmin(key, axis=1)
        d1[:] = np.sqrt(d2[rows, i1])
    return i0, d0, i1, d1


def match_descriptors_l2(q, t, max_distance, knn=None):
    """Kept queries ascending: dist0 <= max_distance and (nt < 2 or dist0 <= 0.75f * dist1), one float32 product."""
    nq, nt = len(q), len(t)
    if nq == 0 or nt == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    i0, d0, _, d1 = knn if knn is not None else knn2_l2(q, t)
    with np.errstate(invalid="ignore"):
        keep = d0 <= F(max_distance)
        if nt >= 2:
            keep &= d0 <= F(0.75) * d1
    qi = np.flatnonzero(keep).astype(np.int32)
    return qi, i0[qi].astype(np.int32)


def d2_f64(q, t):
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    return ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1)


def gamma(n):
    return n * U / (1.0 - n * U)


def dot_bound(q, t):
    """|d2 - exact| <= gamma_(dim+2) (sum q^2 + sum t^2 + 2 sum |q t|): the dot products' standard bound (gamma_dim each),
    one more rounding for nq2 + nt2 and one for the final fma.  (The clamp at 0 only moves d2 towards the exact value.)"""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    scale = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] + 2.0 * (np.abs(q)[:, None, :] * np.abs(t)[None, :, :]).sum(-1)
    return gamma(q.shape[1] + 2) * scale


def diff_bound(q, t):
    """|d2 - exact| <= gamma_(dim/4+5) sum (q - t)^2: e carries one rounding (squared: two), each accumulator's chain
    dim / 4, the two levels of the final sum two more."""
    return gamma(np.asarray(q).shape[1] // 4 + 5) * d2_f64(q, t)


def reproj_match_l2(frame, mp, fdesc, pool, replace=0, max_distance=1.0):
    """rs_reproj_match_l2 restated: match_ref's gates and radius search, per point the minimum D-diff distance over
    (candidate x observation) with a strict '<' from max_distance (the first candidate in visiting order wins a tie), then per
    keypoint the strict-'<' minimum over points in map order.  Distances are float32."""
    kp = np.asarray(frame["keypoints"], np.float32).astype(np.float64).reshape(-1, 2)
    N, P = len(kp), len(mp["positions"])
    fdesc, pool = np.asarray(fdesc, F), np.asarray(pool, F)
    md = F(max_distance)
    open_kp = np.ones(N, bool) if replace else ~np.asarray(frame["kp_matched"]).astype(bool)
    ptr = np.asarray(mp["obs_ptr"], np.int64)
    odesc = np.asarray(mp["obs_desc"], np.int64)
    point_kp = np.full(P, -1, np.int32)
    point_dist = np.full(P, md, F)
    bpts, bkps = np.zeros(P, bool), np.zeros(N, bool)
    ties = 0
    if N > 0 and P > 0:
        passed, boundary, u, v, duv = MR._gates(frame, mp)
        bpts[:] = boundary
        order = np.argsort(kp[:, 0], kind="stable")
        xs = kp[order, 0]
        r = MR.SEARCH_RADIUS
        for p in np.flatnonzero(passed | boundary):
            tol = np.sqrt(2.0) * duv[p] + MR.MARGIN * r
            lo = np.searchsorted(xs, u[p] - r - tol, "left")
            hi = np.searchsorted(xs, u[p] + r + tol, "right")
            near = order[lo:hi]
            d = np.hypot(kp[near, 0] - u[p], kp[near, 1] - v[p])
            maybe = near[d <= r + tol]
            if boundary[p]:
                bkps[maybe] = True
                continue
            dm = d[d <= r + tol]
            sure = maybe[dm + tol <= r]
            undecided = maybe[(dm + tol > r) & open_kp[maybe]]
            if len(undecided):
                bpts[p] = True
                bkps[maybe] = True
                continue
            cand = sure[open_kp[sure]]
            o0, o1 = ptr[p], ptr[p + 1]
            if len(cand) == 0 or o1 == o0:
                continue
            with np.errstate(invalid="ignore"):
                dist = np.sqrt(diff_d2(fdesc[cand], pool[odesc[o0:o1]]))
                dist = np.where(dist < md, dist, F(np.inf))            # only a pair strictly below max_distance can win
            dmin = dist.min(1)
            best = dmin.min()
            if not best < md:
                continue
            tied = cand[dmin == best]
            winner = int(tied[0])
            if len(tied) > 1:
                ties += 1
                visit, vorder, close = MR._walk_order(frame, u[p], v[p], tied)
                visit(int(frame["kd_root"]), 0, tol)
                assert sorted(vorder) == sorted(int(t) for t in tied), "the walk missed a candidate"
                if close[0]:
                    bpts[p] = True
                    bkps[maybe] = True
                    continue
                winner = vorder[0]
            point_kp[p], point_dist[p] = winner, best
    prop_point = np.full(N, -1, np.int32)
    prop_dist = np.full(N, md, F)
    has = np.flatnonzero(point_kp >= 0)
    srt = has[np.lexsort((has, point_dist[has], point_kp[has]))]
    first = np.ones(len(srt), bool)
    first[1:] = point_kp[srt][1:] != point_kp[srt][:-1]
    win = srt[first]
    prop_point[point_kp[win]] = win
    prop_dist[point_kp[win]] = point_dist[win]
    match_kp = np.flatnonzero(prop_point >= 0).astype(np.int32)
    return dict(point_kp=point_kp, point_dist=point_dist, prop_point=prop_point, prop_dist=prop_dist,
                match_kp=match_kp, match_point=prop_point[match_kp].copy(),
                boundary_points=np.flatnonzero(bpts), boundary_kps=np.flatnonzero(bkps), tied_points=ties)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def assert_reproj_equal(got, ref, what=""):
    """got: the library's outputs (numpy); ref: reproj_match_l2's.  Equal bit for bit outside the boundary set."""
    P, N = len(ref["point_kp"]), len(ref["prop_point"])
    okp, okk = np.ones(P, bool), np.ones(N, bool)
    okp[ref["boundary_points"]] = False
    okk[ref["boundary_kps"]] = False
    for k, mask in (("point_kp", okp), ("point_dist", okp), ("prop_point", okk), ("prop_dist", okk)):
        g, r = bits(np.asarray(got[k])[: len(mask)]), bits(ref[k])
        bad = np.flatnonzero((g != r) & mask)
        assert len(bad) == 0, f"{what}{k} differs from the restatement at {bad[:8]}: {np.asarray(got[k])[bad[:8]]} vs {ref[k][bad[:8]]}"
    gk, gp = np.asarray(got["match_kp"]), np.asarray(got["match_point"])
    keep, rk = okk[gk], okk[ref["match_kp"]]
    assert np.array_equal(gk[keep], ref["match_kp"][rk]), f"{what}match_kp differs from the restatement"
    assert np.array_equal(gp[keep], ref["match_point"][rk]), f"{what}match_point differs from the restatement"
