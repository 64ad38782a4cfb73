"""Independent numpy restatement of the two matchers, for tests only.

Written from the contracts in include/rsgpu.h (rs_hamming_knn2, rs_match_descriptors, rs_reproj_match) and the
reference behaviour they cite, not from oracle/*.c or the kernels; it does not call either.  Integer work is exact.
The reprojection gates are evaluated in float64, so where the library's float32 arithmetic may honestly decide
otherwise the reference says so: reproj_match returns a BOUNDARY set of points and keypoints whose outputs it does not
vouch for.  Everything outside that set must agree exactly.

  knn2(q, t)                            -> idx0, dist0, idx1, dist1     (OpenCV's tie rule: the lower train index wins)
  match_descriptors(q, t, max_distance) -> match_query, match_train     (src/MapMatcher.cpp:150-161)
  reproj_match(frame, mp, replace, max_distance) -> dict of the outputs + "boundary_points" / "boundary_kps"
"""
import numpy as np

SEARCH_RADIUS = 20.0            # src/MapMatcher.cpp:12
MIN_VIEWING_COSINE = 0.5        # :13
NEARER, FURTHER = 2.0, 1.25     # :16-17
# Relative margin of the boundary set.  float32 rounds to 2^-24 ~ 6e-8 of the value; each gate quantity takes at most
# ~12 roundings, each on a term no larger than the sum of absolute terms that the margin is scaled by (the
# computation's condition number), so the float32 value lies within 12 * 6e-8 ~ 7e-7 of that scale from the exact one
# in the worst case.  3e-6 leaves four times that worst case.  Larger margins only cost coverage: on a 16k-keypoint
# frame every 1e-5 of margin puts ~2 % of the map points in the boundary set (a keypoint within 0.04 px of a disc).
MARGIN = 3e-6


def _u64(d):
    d = np.ascontiguousarray(d, np.uint8).reshape(-1, 32)
    return d.view(np.uint64)


def hamming(a, b):
    """All-pairs 256-bit Hamming distances of two descriptor sets ([n][32] uint8) as an int64 [na][nb] matrix."""
    A, B = _u64(a), _u64(b)
    d = np.zeros((len(A), len(B)), np.int64)
    for w in range(4):
        d += np.bitwise_count(A[:, None, w] ^ B[None, :, w])
    return d


def knn2(q, t, chunk_pairs=1 << 24):
    """Nearest and second nearest train rows of every query; ties go to the lower train index.  idx1 = dist1 = -1 when
    there is one train row.  Chunked over queries so that 8192 x 8192 (or a few x 2^20) fits in memory."""
    Q, T = _u64(q), _u64(t)
    nq, nt = len(Q), len(T)
    out = [np.full(nq, -1, np.int32) for _ in range(4)]
    if nq == 0 or nt == 0:
        return out
    step = max(1, chunk_pairs // nt)
    for a in range(0, nq, step):
        b = min(nq, a + step)
        d = np.zeros((b - a, nt), np.int32)
        for w in range(4):
            d += np.bitwise_count(Q[a:b, None, w] ^ T[None, :, w]).astype(np.int32)
        rows = np.arange(b - a)
        i0 = np.argmin(d, axis=1)                     # argmin returns the FIRST minimum: the lower index on a tie
        out[0][a:b], out[1][a:b] = i0, d[rows, i0]
        if nt >= 2:
            d[rows, i0] = 1 << 30
            i1 = np.argmin(d, axis=1)
            out[2][a:b], out[3][a:b] = i1, d[rows, i1]
    return out


def match_descriptors(q, t, max_distance=64):
    """Kept queries in ascending order: d0 <= max_distance and (nt < 2 or 4 d0 <= 3 d1)."""
    nq, nt = len(q), len(t)
    if nq == 0 or nt == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    i0, d0, _, d1 = knn2(q, t)
    keep = d0.astype(np.int64) <= max_distance
    if nt >= 2:
        keep &= 4 * d0.astype(np.int64) <= 3 * d1.astype(np.int64)
    qi = np.flatnonzero(keep).astype(np.int32)
    return qi, i0[qi].astype(np.int32)


def _gates(frame, mp):
    """Per point, in float64: (pass, boundary, u, v, delta_uv) of projection, in-image, viewing-angle and distance gates.
    `boundary` marks points whose float32 decision may differ; delta_uv bounds the float32 error of (u, v)."""
    T = np.asarray(frame["pose"], np.float32).astype(np.float64).reshape(4, 4)
    fx, fy, cx, cy = [float(np.float32(k)) for k in frame["K"]]
    W, H = float(frame["width"]), float(frame["height"])
    X = np.asarray(mp["positions"], np.float32).astype(np.float64).reshape(-1, 3)
    P = len(X)
    Kc = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    KP = Kc @ T[:3, :]
    Xh = np.concatenate([X, np.ones((P, 1))], 1)
    uvw = Xh @ KP.T
    scale = np.abs(Xh) @ (np.abs(Kc) @ np.abs(T[:3, :])).T        # sum of |terms| per row: the projection's condition
    z = uvw[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = uvw[:, 0] / z, uvw[:, 1] / z
        du = MARGIN * (scale[:, 0] + np.abs(u) * scale[:, 2]) / np.abs(z)
        dv = MARGIN * (scale[:, 1] + np.abs(v) * scale[:, 2]) / np.abs(z)
    z_boundary = np.abs(z) <= MARGIN * scale[:, 2]
    front = z > 0           # z < 0: behind the camera, rejected; z == 0 only on the boundary
    with np.errstate(invalid="ignore"):
        in_sure = front & (u - du >= 0) & (u + du < W) & (v - dv >= 0) & (v + dv < H)
        out_sure = ~front | (u + du < 0) | (u - du >= W) | (v + dv < 0) | (v - dv >= H)
    boundary = z_boundary | ~(in_sure | out_sure)
    passed = in_sure.copy()

    # viewing angle and distance range over the observing key frames' centres (src/MapPoint.cpp:24-45)
    center = -T[:3, :3].T @ T[:3, 3]
    C = np.asarray(mp["kf_centers"], np.float32).astype(np.float64).reshape(-1, 3)
    ptr = np.asarray(mp["obs_ptr"], np.int64)
    okf = np.asarray(mp["obs_kf"], np.int64)
    elig = np.asarray(mp["eligible"]).astype(bool)
    ray = X - center
    dist = np.linalg.norm(ray, axis=1)
    for p in np.flatnonzero(elig & (in_sure | boundary)):
        o0, o1 = ptr[p], ptr[p + 1]
        if o1 == o0:
            # no observation: the normal is the zero vector (a zero vector stays zero when normalized), its cosine
            # with the ray is 0 < 0.5 whatever the ray is, so the point is rejected for certain
            passed[p] = False
            boundary[p] = False
            continue
        d = X[p] - C[okf[o0:o1]]
        dn = np.linalg.norm(d, axis=1)
        unit = np.divide(d, dn[:, None], out=np.zeros_like(d), where=dn[:, None] > 0)
        normal = unit.sum(0)
        nn = np.linalg.norm(normal)
        if nn > 0 and dist[p] > 0:
            cosang = float(normal @ ray[p]) / (nn * dist[p])
        else:
            cosang = 0.0
        nearest, furthest = dn.min(), dn.max()
        mag = np.abs(X[p]).sum() + np.abs(C[okf[o0:o1]]).sum(1).max() + np.abs(center).sum()
        small = min(dn.min(), dist[p])
        kappa = np.inf if small == 0 else 1.0 + mag / small
        k_angle = kappa * (1.0 + (o1 - o0) / nn) if nn > 0 else np.inf
        m_ang = MARGIN * k_angle
        ang_pass = cosang - m_ang >= MIN_VIEWING_COSINE
        ang_fail = cosang + m_ang < MIN_VIEWING_COSINE
        lo, hi = nearest / NEARER, furthest * FURTHER
        m_d = MARGIN * kappa * dist[p]
        rng_pass = (dist[p] - m_d >= lo * (1 + MARGIN * kappa)) and (dist[p] + m_d <= hi * (1 - MARGIN * kappa))
        rng_fail = (dist[p] + m_d < lo * (1 - MARGIN * kappa)) or (dist[p] - m_d > hi * (1 + MARGIN * kappa))
        sure_pass = ang_pass and rng_pass
        sure_fail = ang_fail or rng_fail
        if sure_fail and not in_sure[p] and not boundary[p]:
            continue
        if in_sure[p]:
            boundary[p] = z_boundary[p] or not (sure_pass or sure_fail)
            passed[p] = sure_pass and not boundary[p]
        else:                       # the projection gate itself is undecided
            passed[p] = False
            boundary[p] = not sure_fail
    passed &= elig
    boundary &= elig
    return passed, boundary, u, v, np.maximum(du, dv)


def _walk_order(frame, u, v, cand):
    """The radius search's visiting order (src/KDTree.cpp:52-82: node, then the near child, then the far child if the
    splitting line is within the radius; x splits at even depth, y at odd) restricted to `cand`, in float64, and
    whether any near/far choice on the way was too close to call."""
    kp = np.asarray(frame["keypoints"], np.float32).astype(np.float64).reshape(-1, 2)
    node_kp, left, right = frame["kd_node_kp"], frame["kd_left"], frame["kd_right"]
    want = set(int(c) for c in cand)
    r2 = SEARCH_RADIUS * SEARCH_RADIUS
    order, close = [], [False]

    def visit(node, depth, tol):
        if node < 0:
            return
        k = int(node_kp[node])
        dx, dy = kp[k, 0] - u, kp[k, 1] - v
        if k in want:
            order.append(k)
        delta = dx if depth % 2 == 0 else dy
        if abs(delta) <= tol:
            close[0] = True
        near, far = (left[node], right[node]) if delta > 0 else (right[node], left[node])
        visit(int(near), depth + 1, tol)
        if delta * delta <= r2:
            visit(int(far), depth + 1, tol)

    return visit, order, close


def reproj_match(frame, mp, replace=0, max_distance=64):
    """rs_reproj_match restated: gates, brute-force radius search (r = 20 px, inclusive), per-point minimum Hamming
    distance over (candidate x observation) with a strict '<' from max_distance (the first candidate in visiting order
    wins a tie), then per keypoint the strict-'<' minimum over points in map order."""
    kp = np.asarray(frame["keypoints"], np.float32).astype(np.float64).reshape(-1, 2)
    N = len(kp)
    P = len(mp["positions"])
    desc = np.ascontiguousarray(frame["descriptors"], np.uint8).reshape(-1, 32)
    pool = np.ascontiguousarray(mp["desc_pool"], np.uint8).reshape(-1, 32)
    open_kp = np.ones(N, bool) if replace else ~np.asarray(frame["kp_matched"]).astype(bool)
    ptr = np.asarray(mp["obs_ptr"], np.int64)
    odesc = np.asarray(mp["obs_desc"], np.int64)
    point_kp = np.full(P, -1, np.int32)
    point_dist = np.full(P, max_distance, np.int32)
    bpts = np.zeros(P, bool)
    bkps = np.zeros(N, bool)
    if N > 0 and P > 0:
        passed, boundary, u, v, duv = _gates(frame, mp)
        bpts[:] = boundary
        order = np.argsort(kp[:, 0], kind="stable")
        xs = kp[order, 0]
        r = SEARCH_RADIUS
        for p in np.flatnonzero(passed | boundary):
            tol = np.sqrt(2.0) * duv[p] + MARGIN * r
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
            dmin = hamming(desc[cand], pool[odesc[o0:o1]]).min(1)
            best = int(dmin.min())
            if best >= max_distance:
                continue
            tied = cand[dmin == best]
            winner = int(tied[0])
            if len(tied) > 1:
                visit, vorder, close = _walk_order(frame, u[p], v[p], tied)
                visit(int(frame["kd_root"]), 0, tol)
                assert sorted(vorder) == sorted(int(t) for t in tied), "the walk missed a candidate"
                if close[0]:
                    bpts[p] = True
                    bkps[maybe] = True
                    continue
                winner = vorder[0]
            point_kp[p], point_dist[p] = winner, best
    prop_point = np.full(N, -1, np.int32)
    prop_dist = np.full(N, max_distance, np.int32)
    has = np.flatnonzero(point_kp >= 0)
    # per keypoint: the smallest distance, then the earliest point in map order (sequential strict '<')
    srt = has[np.lexsort((has, point_dist[has], point_kp[has]))]
    first = np.ones(len(srt), bool)
    first[1:] = point_kp[srt][1:] != point_kp[srt][:-1]
    win = srt[first]
    prop_point[point_kp[win]] = win
    prop_dist[point_kp[win]] = point_dist[win]
    match_kp = np.flatnonzero(prop_point >= 0).astype(np.int32)
    return dict(point_kp=point_kp, point_dist=point_dist, prop_point=prop_point, prop_dist=prop_dist,
                match_kp=match_kp, match_point=prop_point[match_kp].copy(),
                boundary_points=np.flatnonzero(bpts), boundary_kps=np.flatnonzero(bkps))


def assert_reproj_equal(got, ref, what=""):
    """got: outputs of the library or the oracle (point_kp .. match_point, numpy); ref: reproj_match's result.  Equal
    outside the boundary set."""
    P, N = len(ref["point_kp"]), len(ref["prop_point"])
    okp = np.ones(P, bool)
    okp[ref["boundary_points"]] = False
    okk = np.ones(N, bool)
    okk[ref["boundary_kps"]] = False
    for k, mask in (("point_kp", okp), ("point_dist", okp), ("prop_point", okk), ("prop_dist", okk)):
        g = np.asarray(got[k])[: len(mask)]
        bad = np.flatnonzero((g != ref[k]) & mask)
        assert len(bad) == 0, f"{what}{k} differs from the reference at {bad[:8]}: {g[bad[:8]]} vs {ref[k][bad[:8]]}"
    gk, gp = np.asarray(got["match_kp"]), np.asarray(got["match_point"])
    keep = okk[gk]
    rk = okk[ref["match_kp"]]
    assert np.array_equal(gk[keep], ref["match_kp"][rk]), f"{what}match_kp differs from the reference"
    assert np.array_equal(gp[keep], ref["match_point"][rk]), f"{what}match_point differs from the reference"
