"""K2 through the frame's cell grid (rs_kdtree_grid_build, k2_reproj_match_grid) against the oracle's walk on the same
arrays, bit for bit, and against the two walk kernels (k2_grid 0, k2_mode 1).

The grid has no visiting order, the reference keeps the FIRST candidate in visiting order among those at the minimal
distance: the tie cases give several keypoints of one disc the point's own descriptor (distance 0 for each of them) and
say, from a model of the recursion order on node ids, which configurations they contain.  Every scene is a camera at the
origin with dyadic intrinsics and points at depth 2, so that a point projects exactly where it is put."""
import threading

import numpy as np
import pytest

import match_cases as MC
from conftest import to_np

pytestmark = pytest.mark.gpu

K = (512.0, 256.0, 256.0, 192.0)
Z = 2.0
CELL = 40
KEYS = ("point_kp", "point_dist", "prop_point", "prop_dist", "match_kp", "match_point")


# ------------------------------------------------------------------------------------------------------------ scenes
def make(rs, W, H, uv, kp, kdesc, base, obs=3, seed=0, matched=None, tree=None):
    """Points projecting at uv [P][2] with descriptors base [P][32] (every observation row equals it), keypoints kp
    [N][2] with descriptors kdesc; tree: None = rs.kdtree_build, or a function keypoints -> (node_kp, left, right, root)."""
    rng = np.random.default_rng(0x6B1D + seed)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    P = len(uv)
    fx, fy, cx, cy = K
    Xw = np.stack([(uv[:, 0] - cx) / fx * Z, (uv[:, 1] - cy) / fy * Z, np.full(P, Z)], 1)
    obs = np.broadcast_to(np.asarray(obs, np.int64), (P,))
    frame, mp = MC.assemble(rng, np.eye(4), K, W, H, Xw, obs, np.asarray(kp, np.float64).reshape(-1, 2), kdesc, base,
                            rng.normal(0, 0.05, (int(obs.max()) + 4, 3)), np.array([[30.0, 0, 0]]), np.zeros(P, bool),
                            "none", "all", tree or rs.kdtree_build, pool_flip=(0, 0))
    if matched is not None:
        frame["kp_matched"] = np.asarray(matched, np.uint8)
    u, v, _ = MC.project_f32(frame, mp["positions"])
    assert np.array_equal(u, uv[:, 0].astype(np.float32)) and np.array_equal(v, uv[:, 1].astype(np.float32))
    return frame, mp


def outs(o, P, N):
    cnt = int(to_np(o["count"])[0])
    return dict(point_kp=to_np(o["point_kp"])[:P].copy(), point_dist=to_np(o["point_dist"])[:P].copy(),
                prop_point=to_np(o["prop_point"])[:N].copy(), prop_dist=to_np(o["prop_dist"])[:N].copy(),
                match_kp=to_np(o["match_kp"])[:cnt].copy(), match_point=to_np(o["match_point"])[:cnt].copy())


def same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"


def grid_header(keep):
    """nx, ny, cell, n, usable of the grid make_frame_view(pack=True) built."""
    return [int(x) for x in to_np(keep["d_kd_grid"])[:5]]


def check(ctx, oracle, frame, mp, replace=0, md=64, usable=True, walks=True):
    """grid == oracle (== k2_grid 0 == k2_mode 1); returns the oracle's result."""
    P, N = len(mp["positions"]), len(frame["keypoints"])
    orc = oracle.reproj_match(frame, mp, replace=replace, max_distance=md)
    fv, k1 = ctx.make_frame_view(frame, pack=True)
    mv, k2 = ctx.make_map_view(mp)
    h = grid_header(k1)
    assert h[2] == CELL and h[3] == N and h[4] == (1 if usable else 0), h
    same(outs(ctx.reproj_match(fv, mv, replace=replace, max_distance=md), P, N), orc, "grid vs oracle")
    if walks:
        for name, value in (("k2_grid", 0), ("k2_mode", 1)):
            ctx.set_int(name, value)
            try:
                same(outs(ctx.reproj_match(fv, mv, replace=replace, max_distance=md), P, N), orc, f"{name} {value} vs oracle")
            finally:
                ctx.set_int(name, 1 if name == "k2_grid" else 0)
    return orc


# ------------------------------------------------------------------------------------------------------------ the order model
def node_of_kp(frame):
    inv = np.zeros(len(frame["kd_node_kp"]), np.int64)
    inv[frame["kd_node_kp"]] = np.arange(len(inv))
    return inv


def lca(a, b, n):
    """(L, depth) of the lowest common ancestor of nodes a, b in the implicit tree over n nodes."""
    s, e, d = 0, n, 0
    while True:
        m = (s + e) // 2
        if a == m or b == m or (a < m) != (b < m):
            return m, d
        if a < m:
            e = m
        else:
            s = m + 1
        d += 1


def tie_kind(frame, q, ka, kb):
    """How the recursion orders keypoints ka, kb for the query q: ("anc",) or ("lca", depth parity, query left of L)."""
    inv = node_of_kp(frame)
    a, b = int(inv[ka]), int(inv[kb])
    L, d = lca(a, b, len(inv))
    if L in (a, b):
        return ("anc",)
    c = frame["keypoints"][frame["kd_node_kp"][L]][d % 2]
    return ("lca", d % 2, bool(np.float32(c) - np.float32(q[d % 2]) > 0))


def tie_scene(rs, n, group, seed, W=640, H=480, reach=13.0, crowd=0):
    """n random keypoints; disjoint groups of `group` keypoints within `reach` px of their first one get one point each,
    projecting at the group's centroid (a multiple of 1/4 px), and every keypoint of the group carries the point's
    descriptor: a `group`-way tie at distance 0.  crowd: that many further keypoints (random descriptors) dropped within
    15 px of every query.  Returns frame, mp, [(query, [keypoints of the group])]."""
    rng = np.random.default_rng(0x71E5 + seed)
    kp = np.round(np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1) * 4) / 4
    used, groups = np.zeros(n, bool), []
    for i in range(n):
        if used[i]:
            continue
        near = [j for j in np.flatnonzero(~used) if j != i and np.hypot(*(kp[j] - kp[i])) <= reach][:group - 1]
        if len(near) < group - 1:
            continue
        g = [i] + near
        q = np.round(kp[g].mean(0) * 4) / 4
        if not (0 <= q[0] < W and 0 <= q[1] < H) or max(np.hypot(*(kp[j] - q)) for j in g) > 19.0:
            continue
        used[g] = True
        groups.append((q, g))
    assert groups
    kdesc = MC.descriptors(rng, n)
    base = MC.descriptors(rng, len(groups))
    for p, (_, g) in enumerate(groups):
        kdesc[g] = base[p]
    if crowd:
        extra = np.concatenate([q + np.round(rng.uniform(-10, 10, (crowd, 2)) * 4) / 4 for q, _ in groups])
        kp = np.concatenate([kp, extra])
        kdesc = np.concatenate([kdesc, MC.descriptors(rng, len(extra))])
    frame, mp = make(rs, W, H, [q for q, _ in groups], kp, kdesc, base, seed=seed)
    return frame, mp, groups


# ------------------------------------------------------------------------------------------------------------ ties
def test_pairs_tied_across_every_kind_of_common_ancestor(ctx, oracle, rs):
    """Two keypoints at distance 0: their lowest common ancestor is one of them, or a third node at an even and at an odd
    depth with the query on either side of its coordinate.  The oracle's winner is the second keypoint of the pair in
    some cases and the first in others, so that no fixed preference passes."""
    kinds, first, second = set(), 0, 0
    for n, seed, W, H in ((16, 1, 100, 80), (64, 2, 200, 160), (300, 3, 640, 480), (300, 4, 640, 480)):
        frame, mp, groups = tie_scene(rs, n, 2, seed, W, H)
        orc = check(ctx, oracle, frame, mp)
        for p, (q, g) in enumerate(groups):
            assert orc["point_dist"][p] == 0 and orc["point_kp"][p] in g
            kinds.add(tie_kind(frame, q, g[0], g[1]))
            first += orc["point_kp"][p] == min(g)
            second += orc["point_kp"][p] == max(g)
    assert kinds == {("anc",)} | {("lca", d, s) for d in (0, 1) for s in (False, True)}, kinds
    assert first > 5 and second > 5


@pytest.mark.parametrize("group", [3, 5])
def test_ties_of_several_keypoints(ctx, oracle, rs, group):
    W, H = (640, 480) if group == 3 else (300, 220)            # five within 15 px need a denser frame
    frame, mp, groups = tie_scene(rs, 300, group, 10 + group, W, H, reach=15.0)
    assert len(groups) >= 3
    orc = check(ctx, oracle, frame, mp)
    assert all(orc["point_dist"][p] == 0 for p in range(len(groups)))
    assert len({sorted(g).index(orc["point_kp"][p]) for p, (_, g) in enumerate(groups)}) > 1      # not always the lowest index


def test_tied_pair_among_more_than_sixteen_candidates(ctx, oracle, rs):
    """24 further keypoints inside every disc: more candidates than the walk kernels queue (K2_MAXC 16), the tie among them."""
    frame, mp, groups = tie_scene(rs, 60, 2, 21, crowd=24)
    orc = check(ctx, oracle, frame, mp)
    assert all(orc["point_kp"][p] in g and orc["point_dist"][p] == 0 for p, (_, g) in enumerate(groups))


def test_ties_between_cell_rows_and_columns(ctx, oracle, rs):
    """Tied keypoints in different cell rows (and columns) of the query's range.  Two keypoints within 20 px of one query
    are less than 40 px apart, so they lie in the same or in adjacent rows: the first and the last row of a two-row
    range, and rows 1 and 2 or 0 and 1 of a three-row range."""
    rng = np.random.default_rng(5)
    uv, kp, own = [], [], []
    for i, (qx, qy, dxa, dya, dxb, dyb) in enumerate([
            (100.0, 80.0, 0.0, -19.0, 0.0, 19.0),        # rows 1 | 2 of the range 1 .. 2
            (300.0, 60.0, 3.0, -20.0, -3.0, 19.75),      # rows 1 | 1..: v - 20.5 = 39.5 -> rows 0 .. 2, entries in rows 1 and 1
            (500.0, 59.75, 0.0, -20.0, 0.0, 20.0),       # 39.75 (row 0) | 79.75 (row 1), the range is rows 0 .. 2
            (120.0, 300.0, -19.0, 0.0, 19.0, 0.0),       # columns 2 | 3
            (200.0, 200.25, -1.0, -0.5, 1.0, 0.0),       # 199.75 (row 4) | 200.25 (row 5), columns 4 | 5
            (40.0, 40.0, -15.0, -12.0, 12.0, 15.0)]):    # diagonal: cell (0, 0) | cell (1, 1)
        uv.append((qx, qy))
        kp += [(qx + dxa, qy + dya), (qx + dxb, qy + dyb)]
        own += [i, i]
    clutter = np.round(np.stack([rng.uniform(0, 640, 200), rng.uniform(0, 480, 200)], 1))
    kp = np.concatenate([np.array(kp), clutter])
    base = MC.descriptors(rng, len(uv))
    kdesc = np.concatenate([base[own], MC.descriptors(rng, len(clutter))])
    perm = rng.permutation(len(kp))                                 # the pairs anywhere in the tree
    frame, mp = make(rs, 640, 480, uv, kp[perm], kdesc[perm], base)
    orc = check(ctx, oracle, frame, mp)
    assert np.all(orc["point_dist"] == 0)


# ------------------------------------------------------------------------------------------------------------ geometry
def _alike(rng, P, N):
    """Descriptors of P points and N keypoints, all within a few bits of one row: every keypoint in a point's disc is a
    candidate below max_distance, at one of a few distances, so that which keypoints are IN the disc decides the result."""
    d = MC.descriptors(rng, 1)
    return MC.flip_bits(rng, np.repeat(d, P, 0), rng.integers(0, 6, P)), MC.flip_bits(rng, np.repeat(d, N, 0), rng.integers(0, 12, N))


def test_keypoints_on_cell_borders_and_at_distance_twenty(ctx, oracle, rs):
    """Keypoints on every cell border of a 200 x 200 corner; queries on borders, beside them, and 20 px (inclusive) and
    20.25 px from integer keypoints along both axes and on the 12-16-20 triangle."""
    rng = np.random.default_rng(6)
    kp = np.array([(x, y) for x in (0, 40, 80, 120, 160, 39.75, 40.25) for y in (0, 40, 80, 120, 160, 79.75)], np.float64)
    uv = [(x, y) for x in (20.0, 40.0, 59.75, 60.0, 60.25, 100.0, 19.75) for y in (20.0, 60.0, 80.0, 100.25, 139.75)]
    uv += [(52.0, 56.0), (28.0, 24.0), (92.0, 96.0), (52.25, 56.0)]                      # 12-16-20 from (40, 40) / (80, 80)
    base, kdesc = _alike(rng, len(uv), len(kp))
    frame, mp = make(rs, 200, 200, uv, kp, kdesc, base)
    orc = check(ctx, oracle, frame, mp)
    assert (orc["point_kp"] >= 0).sum() > 10
    # the point 20 px along x from its only keypoint is matched, the one 20.25 px away is not
    for q, hit in (((60.0, 300.0), True), ((60.25, 300.0), False), ((40.0, 320.0), True), ((40.0, 279.75), False)):
        b = MC.descriptors(rng, 1)
        f1, m1 = make(rs, 640, 480, [q], [(40.0, 300.0)], b, b)
        assert (check(ctx, oracle, f1, m1)["point_kp"][0] == 0) == hit, q


@pytest.mark.parametrize("W,H", [(640, 480), (650, 490), (1, 1), (39, 41), (80, 40)])
def test_image_borders_corners_and_keypoints_outside(ctx, oracle, rs, W, H):
    """Projections within 20 px of every border and corner; keypoints at (0, 0), negative, at and beyond width / height
    (they sit in border cells); sizes that are no multiple of the cell; a 1 x 1 image."""
    rng = np.random.default_rng(W * 1000 + H)
    xs = sorted({0.0, 0.25, 5.0, 19.75, min(20.0, W - 0.25), W / 2 - (W / 2) % 0.25, max(W - 20.0, 0.0), max(W - 5.0, 0.0), W - 0.25})
    ys = sorted({0.0, 7.5, min(20.25, H - 0.25), H / 2 - (H / 2) % 0.25, max(H - 19.75, 0.0), H - 0.25})
    uv = [(x, y) for x in xs for y in ys]
    kp = [(0.0, 0.0), (-0.25, 3.0), (-15.0, -15.0), (-19.0, H / 2), (W, 0.0), (W + 10.0, H + 10.0), (W - 0.25, H), (W / 2, H + 19.0),
          (W / 2, -12.0), (W + 19.75, H / 2), (-300.0, -300.0), (W + 5000.0, 1.0), (3.0, H + 1e6)]
    kp += [tuple(p) for p in np.round(np.stack([rng.uniform(-20, W + 20, 150), rng.uniform(-20, H + 20, 150)], 1) * 4) / 4]
    base, kdesc = _alike(rng, len(uv), len(kp))
    frame, mp = make(rs, W, H, uv, kp, kdesc, base)
    orc = check(ctx, oracle, frame, mp)
    assert (orc["point_kp"] >= 0).any()


def test_forty_keypoints_in_one_disc(ctx, oracle, rs):
    rng = np.random.default_rng(8)
    uv = [(100.0, 100.0), (300.25, 200.5), (621.0, 470.0)]
    kp = np.concatenate([np.array(q) + np.round(rng.uniform(-13, 13, (40, 2)) * 4) / 4 for q in uv])
    base = MC.descriptors(rng, len(uv))
    kdesc = MC.flip_bits(rng, np.repeat(base, 40, 0), rng.integers(3, 12, len(kp)))      # many equal minima among the forty
    frame, mp = make(rs, 640, 480, uv, kp, kdesc, base, obs=[1, 9, 17])
    orc = check(ctx, oracle, frame, mp)
    assert np.all(orc["point_kp"] >= 0)
    check(ctx, oracle, dict(frame, kp_matched=(rng.random(len(kp)) < 0.5).astype(np.uint8)), mp)


# ------------------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65])
def test_keypoint_counts(ctx, oracle, rs, n):
    frame, mp = MC.scene(N=n, P=300, seed=900 + n, W=320, H=240, kdtree_build=rs.kdtree_build)
    for replace in (0, 1):
        check(ctx, oracle, frame, mp, replace=replace)


@pytest.mark.parametrize("P", [1, 63, 65])
def test_point_counts(ctx, oracle, rs, P):
    frame, mp = MC.scene(N=400, P=P, seed=950 + P, W=320, H=240, eligible="all", behind=0.0, odd=0.0, kdtree_build=rs.kdtree_build)
    assert (check(ctx, oracle, frame, mp)["point_kp"] >= 0).any() or P == 1


def test_seven_thousand_keypoints_against_the_global_walk(ctx, oracle, rs):
    """Beyond the 6144 nodes that fit in LDS both walk kernels run over global memory; the grid does not care."""
    frame, mp = MC.scene(N=7000, P=2000, seed=7000, obs=(1, 3, 9, 17), kdtree_build=rs.kdtree_build)
    assert len(check(ctx, oracle, frame, mp)["match_kp"]) > 200


# ------------------------------------------------------------------------------------------------------------ unusable grids
def _tree_mid_up(kp):
    """A valid KD-tree of another shape: the node of [s, e) sits at (s + e + 1) / 2 where that is inside the range."""
    kp = np.asarray(kp, np.float32)
    n = len(kp)
    node_kp, left, right = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    order = np.arange(n)

    def build(s, e, depth):
        if s >= e:
            return -1
        seg = order[s:e]
        order[s:e] = seg[np.lexsort((seg, kp[seg, depth % 2]))]
        mid = min((s + e + 1) // 2, e - 1)
        node_kp[mid] = order[mid]
        left[mid] = build(s, mid, depth + 1)
        right[mid] = build(mid + 1, e, depth + 1)
        return mid

    root = build(0, n, 0)
    return node_kp, left, right, np.int32(root)


@pytest.mark.parametrize("n", [100, 101])
def test_tree_of_another_shape_is_walked(ctx, oracle, rs, n):
    """n = 101: the root itself differs (51, not 50), no grid is built at all; n = 100: the root agrees, children do not."""
    frame, mp = MC.scene(N=n, P=300, seed=n, W=320, H=240, kdtree_build=_tree_mid_up)
    assert not np.array_equal(frame["kd_left"], rs.kdtree_build(frame["keypoints"])[1])
    P = len(mp["positions"])
    orc = oracle.reproj_match(frame, mp, replace=0, max_distance=64)
    fv, keep = ctx.make_frame_view(frame, pack=True)
    mv, k2 = ctx.make_map_view(mp)
    if n == 100:
        assert grid_header(keep)[3:5] == [n, 0]
    same(outs(ctx.reproj_match(fv, mv), P, n), orc, "walk of the other tree vs oracle")
    assert (orc["point_kp"] >= 0).any()


def _broken(rs, how):
    frame, mp = MC.scene(N=200, P=400, seed=77, W=320, H=240, eligible="all", matched="none", kdtree_build=rs.kdtree_build)
    frame = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in frame.items()}
    node_kp = frame["kd_node_kp"]
    if how == "order":            # a leaf of the root's left subtree and one of its right subtree change places
        root = int(frame["kd_root"])
        a = next(i for i in range(root) if frame["kd_left"][i] < 0 and frame["kd_right"][i] < 0)
        b = next(i for i in range(len(node_kp) - 1, root, -1) if frame["kd_left"][i] < 0 and frame["kd_right"][i] < 0)
        assert frame["keypoints"][node_kp[a]][0] < frame["keypoints"][node_kp[b]][0]
        node_kp[a], node_kp[b] = node_kp[b], node_kp[a]
    else:                         # the coordinate changes under the finished tree, as the oracle's walk sees it too
        k = int(node_kp[int(frame["kd_left"][int(frame["kd_root"])])])          # an inner node high in the tree
        frame["keypoints"][k, 1 if how == "nan-y" else 0] = np.nan if how.startswith("nan") else np.inf
    return frame, mp


@pytest.mark.parametrize("how", ["order", "nan-x", "nan-y", "inf"])
def test_unusable_trees_are_walked(ctx, oracle, rs, how):
    frame, mp = _broken(rs, how)
    orc = check(ctx, oracle, frame, mp, usable=False)
    assert (orc["point_kp"] >= 0).sum() > 20


# ------------------------------------------------------------------------------------------------------------ state
def test_one_grid_two_calls_with_different_kp_matched_and_replace(ctx, oracle, rs):
    """The benchmark's pattern: the frame's view, tree and grid made once, kp_matched rewritten between the calls."""
    frame, mp = MC.scene(N=900, P=1500, seed=31, W=640, H=480, matched="none", kdtree_build=rs.kdtree_build)
    P, N = len(mp["positions"]), len(frame["keypoints"])
    rng = np.random.default_rng(31)
    fv, keep = ctx.make_frame_view(frame, pack=True)
    mv, k2 = ctx.make_map_view(mp)
    assert grid_header(keep)[4] == 1
    seen = []
    for frac, replace in ((0.0, 0), (0.4, 0), (0.8, 0), (0.8, 1), (1.0, 0), (0.1, 0)):
        kpm = (rng.random(N) < frac).astype(np.uint8)
        keep["d_kp_matched"].copy_(ctx.dev(kpm))
        orc = oracle.reproj_match(dict(frame, kp_matched=kpm), mp, replace=replace, max_distance=64)
        same(outs(ctx.reproj_match(fv, mv, replace=replace), P, N), orc, f"kp_matched {frac} replace {replace}")
        seen.append(len(orc["match_kp"]))
    assert seen[0] > seen[1] > seen[2] and seen[3] == seen[0] and seen[4] == 0


def test_view_matched_on_a_forked_child_context(ctx, oracle, rs):
    """The benchmark's front end: the view, tree and grid are made on the library's context, the match runs on a child
    context with a stream of its own between a fork and a join."""
    import torch
    frame, mp = MC.scene(N=900, P=1500, seed=32, W=640, H=480, dup=25, kdtree_build=rs.kdtree_build)
    P, N = len(mp["positions"]), len(frame["keypoints"])
    orc = oracle.reproj_match(frame, mp, replace=0, max_distance=64)
    fv, keep = ctx.make_frame_view(frame, pack=True)
    mv, k2 = ctx.make_map_view(mp)
    child = rs.Context(0)
    try:
        child.use_stream(torch.cuda.Stream(device=ctx.device))
        for _ in range(2):
            ctx.fork(child)
            o = child.reproj_match(fv, mv)
            ctx.wait_for(child)
            ctx.synchronize()
            same(outs(o, P, N), orc, "child context vs oracle")
    finally:
        child.close()
    assert len(orc["match_kp"]) > 100


def test_sharded_with_a_point_base(oracle, rs):
    """rs_reproj_match_sharded on the grid: three shards (one empty) with their point_base, every rank the unsharded result."""
    import torch
    frame, mp = MC.scene(N=700, P=1200, seed=41, W=640, H=480, dup=30, kdtree_build=rs.kdtree_build)
    orc = oracle.reproj_match(frame, mp, replace=0, max_distance=64)
    P = len(mp["positions"])
    bounds = (0, 517, 517, P)
    n = len(bounds) - 1
    ctxs = [rs.Context(0) for _ in range(n)]
    streams = [torch.cuda.Stream(device=ctxs[0].device) for _ in range(n)]
    for c, st in zip(ctxs, streams):
        c.use_stream(st)
    rs.Context.comm_init_local(ctxs)
    out = [None] * n

    def shard(lo, hi):
        o0, o1 = int(mp["obs_ptr"][lo]), int(mp["obs_ptr"][hi])
        sh = dict(mp, positions=mp["positions"][lo:hi], eligible=mp["eligible"][lo:hi],
                  obs_ptr=(mp["obs_ptr"][lo:hi + 1] - o0).astype(np.int32),
                  obs_kf=mp["obs_kf"][o0:o1] if o1 > o0 else np.zeros(1, np.int32),
                  obs_desc=mp["obs_desc"][o0:o1] if o1 > o0 else np.zeros(1, np.int32))
        if hi == lo:
            sh.update(positions=np.zeros((1, 3), np.float32), eligible=np.zeros(1, np.uint8), obs_ptr=np.zeros(2, np.int32))
        return sh

    def work(r):
        try:
            c = ctxs[r]
            with torch.cuda.stream(streams[r]):
                lo, hi = bounds[r], bounds[r + 1]
                fv, k1 = c.make_frame_view(frame, pack=True)
                assert grid_header(k1)[4] == 1
                mv, k2 = c.make_map_view(shard(lo, hi))
                mv.n_points = hi - lo
                streams[r].synchronize()
                o = c.reproj_match_sharded(fv, mv, lo)
                streams[r].synchronize()
                out[r] = outs(o, hi - lo, len(frame["keypoints"]))
        except BaseException as ex:      # noqa: BLE001
            out[r] = ex

    threads = [threading.Thread(target=work, args=(r,)) for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank is stuck in the exchange step"
    for c in ctxs:
        c.comm_destroy()
        c.close()
    for r in range(n):
        assert not isinstance(out[r], BaseException), out[r]
        lo, hi = bounds[r], bounds[r + 1]
        for k in ("prop_point", "prop_dist", "match_kp", "match_point"):
            assert np.array_equal(out[r][k], orc[k]), (r, k)
        assert np.array_equal(out[r]["point_kp"], orc["point_kp"][lo:hi]), r
    assert (orc["prop_point"] >= 517).any() and len(orc["match_kp"]) > 50


def test_resident_frame_reassigned_larger_and_smaller(ctx, rs, oracle, synth):
    """rs_map_match on a device-assigned rs_frame: its grid is rebuilt after every assign (500 -> 2500 -> 200 keypoints in
    one rs_frame) and shared by the calls in between, with another kp_matched and another image size."""
    from test_resident_map import Scene
    sc = Scene(ctx, rs, synth)
    sc.rframe.close()
    df = rs.DeviceFrame(ctx, 4096)
    sc.rframe = df
    base = dict(sc.frame)
    rng = np.random.default_rng(12)
    try:
        for n in (500, 2500, 200):
            kp, desc = base["keypoints"][:min(n, 500)], base["descriptors"][:min(n, 500)]
            if n > 500:
                kp = np.concatenate([kp, np.stack([rng.uniform(0, base["width"], n - 500), rng.uniform(0, base["height"], n - 500)], 1).astype(np.float32)])
                desc = np.concatenate([desc, MC.flip_bits(rng, base["descriptors"][rng.integers(0, 500, n - 500)], rng.integers(5, 60, n - 500))])
            node_kp, left, right, root = rs.kdtree_build(kp)
            sc.frame = dict(base, keypoints=kp, descriptors=desc, kp_matched=np.zeros(n, np.uint8), kd_node_kp=node_kp, kd_left=left,
                            kd_right=right, kd_root=root)
            assert df.assign(ctx.dev(desc), ctx.dev(kp), ctx.dev(np.array([n], np.int32))) == n
            assert sc.check(oracle) > (50 if n >= 500 else 0)
            kpm = (rng.random(n) < 0.3).astype(np.uint8)
            sc.check(oracle, kp_matched=kpm)
            sc.check(oracle, kp_matched=kpm, replace=1)
            sc.frame = dict(sc.frame, width=base["width"] - 37)          # the grid follows the image size of the call
            sc.check(oracle)
    finally:
        df.close()
        sc.map.close()
