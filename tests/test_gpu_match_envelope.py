"""K1 / K1b (rs_hamming_knn2, rs_match_descriptors) and K2 / K3 (rs_reproj_match, rs_reproj_match_sharded,
rs_map_match) across their envelope.  Every case is compared with the oracle bit for bit and with tests/match_ref.py
(the independent restatement, pinned on the CPU by tests/test_match_ref_cpu.py) outside its boundary set.

K1: the three nsplit regimes of knn2_launch (named in the ids from the launch arithmetic, match_cases.k1_launch), the
XCD-grouped block order (batch % 8 == 0) with the split merge, K1b's multi-pass compaction (nq > 4096), exact ties
across splits and waves, the filter edges, and the top-2 table reused across sizes.
K2: keypoint counts on both sides of the 6144-node LDS tree (the global-memory walk beyond), both kernels (k2_mode 0 /
1), the tree packed and not, workgroup-edge point counts, observation counts at the preload / batch edges, candidate
counts at the queue edge, max_distance, geometry edges, and the proposal table reused across sizes."""
import threading

import numpy as np
import pytest

import match_cases as MC
import match_ref as MR
from conftest import to_np

pytestmark = pytest.mark.gpu

_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ K1
def _knn_gpu(ctx, q, t, max_distance=64, raw=True, match=True):
    """q [batch][nq][32], t [batch][nt][32] -> per item (idx0, dist0, idx1, dist1) or None, (mq, mt) or None."""
    B, nq, nt = q.shape[0], q.shape[1], t.shape[1]
    dq, dt = ctx.dev(q), ctx.dev(t)
    if not match:
        o = [to_np(x) for x in ctx.hamming_knn2(dq, dt, nq, nt, batch=B)]
        return [tuple(x[b, :nq] for x in o) for b in range(B)], None
    m = ctx.match_descriptors(dq, dt, nq, nt, batch=B, max_distance=max_distance, raw=raw)
    cnt = to_np(m["cnt"])
    mq, mt = to_np(m["mq"]), to_np(m["mt"])
    lists = [(mq[b, :cnt[b]], mt[b, :cnt[b]]) for b in range(B)]
    rawo = [tuple(to_np(x)[b, :nq] for x in m["raw"]) for b in range(B)] if raw else None
    return rawo, lists


def _knn_check(ctx, oracle, q, t, max_distances=(64,), key=None):
    B = q.shape[0]
    refs = _cached(("knn", key), lambda: [(MR.knn2(q[b], t[b]), oracle.hamming_knn2(q[b], t[b])) for b in range(B)])
    raw, _ = _knn_gpu(ctx, q, t, match=False)
    for b in range(B):
        for g, r, o, name in zip(raw[b], refs[b][0], refs[b][1], ("idx0", "dist0", "idx1", "dist1")):
            assert np.array_equal(g, o), f"item {b} {name} vs oracle"
            assert np.array_equal(g, r), f"item {b} {name} vs reference"
    for md in max_distances:
        raw2, lists = _knn_gpu(ctx, q, t, max_distance=md, raw=True)
        _, lists_noraw = _knn_gpu(ctx, q, t, max_distance=md, raw=False)
        for b in range(B):
            for g, r in zip(raw2[b], raw[b]):
                assert np.array_equal(g, r)
            oq, ot = oracle.match_descriptors(q[b], t[b], md)
            rq, rt = MR.match_descriptors(q[b], t[b], md)
            for lq, lt in (lists[b], lists_noraw[b]):
                assert np.array_equal(lq, oq) and np.array_equal(lt, ot), f"item {b} max_distance {md} vs oracle"
                assert np.array_equal(lq, rq) and np.array_equal(lt, rt), f"item {b} max_distance {md} vs reference"


def _knn_id(nq, nt, batch):
    ns, regime, rows, empty = MC.k1_launch(nq, nt, batch)
    return f"nq{nq}-nt{nt}-b{batch}-nsplit{ns}-{regime}" + ("-emptywaves" if empty else "")


_NQ = [(nq, nt) for nq in (1, 63, 64, 65, 4095, 4096, 4097, 8192, 9000) for nt in (33, 500)]
_NT = [(5, 1), (5, 2), (64, 31), (64, 32), (64, 33), (64, 4096), (40, 65536), (3, (1 << 20) - 1)]


@pytest.mark.parametrize("nq,nt", _NQ + _NT, ids=[_knn_id(nq, nt, 1) for nq, nt in _NQ + _NT])
def test_knn_shapes(ctx, oracle, nq, nt):
    q, t = MC.knn_set(nq, nt)
    _knn_check(ctx, oracle, q, t, max_distances=(64,), key=(nq, nt, 1))


_BATCH = [(b, nq, nt) for b in (1, 3, 7, 8, 9, 16) for nq, nt in ((100, 700), (2000, 2000))]


@pytest.mark.parametrize("batch,nq,nt", _BATCH, ids=[_knn_id(nq, nt, b) for b, nq, nt in _BATCH])
def test_knn_batches(ctx, oracle, batch, nq, nt):
    q, t = MC.knn_set(nq, nt, batch=batch, seed=batch)
    if batch in (8, 16) and nq == 100:
        assert MC.k1_launch(nq, nt, batch)[0] > 1          # the XCD-grouped order together with the split merge
    _knn_check(ctx, oracle, q, t, key=(nq, nt, batch))


@pytest.mark.parametrize("max_distance", [0, 1, 63, 64, 65, 255, 256])
def test_knn_max_distance(ctx, oracle, max_distance):
    q, t = MC.knn_set(700, 900, seed=5, near=0.8)
    _knn_check(ctx, oracle, q, t, max_distances=(max_distance,), key="md")


def _tie_set(nt, batch=1):
    """Ties at rank 1 and rank 2 whose rows lie in different splits and different waves, d0 == max_distance,
    4 d0 == 3 d1 and complementary rows (distance 256)."""
    rng = np.random.default_rng(77 + nt + batch)
    q = MC.descriptors(rng, batch * 64).reshape(batch, 64, 32)
    t = MC.descriptors(rng, batch * nt).reshape(batch, nt, 32)
    _, _, rows, _ = MC.k1_launch(64, nt, batch)
    far = [nt - 1, nt // 2 + rows, rows + 1, 3]                 # several splits and waves apart
    for b in range(batch):
        for i in range(0, 16):                                   # rank-1 ties: the same row at two far indices
            t[b, far[i % 4]] = q[b, i]
            t[b, far[(i + 1) % 4] - (i % 2)] = q[b, i]
            q[b, i] = MC.flip_bits(rng, q[b, i:i + 1], [i])[0]
        for i in range(16, 32):                                  # rank-2 ties: best near, two equal seconds far apart
            t[b, 5 + i] = MC.flip_bits(rng, q[b, i:i + 1], [10])[0]
            t[b, far[i % 4] - 1] = MC.flip_bits(rng, q[b, i:i + 1], [20])[0]
            t[b, far[(i + 2) % 4] - 2] = t[b, far[i % 4] - 1]
        for i in range(32, 40):                                  # 4 d0 == 3 d1 with d0 == 64 (== max_distance)
            t[b, 60 + i] = MC.flip_bits(rng, q[b, i:i + 1], [48 if i % 2 else 64])[0]
            t[b, far[i % 4] - 3] = MC.flip_bits(rng, q[b, i:i + 1], [64 if i % 2 else 86])[0]
        for i in range(40, 44):                                  # complement of a train row: distance 256
            q[b, i] = ~t[b, far[i % 4]]
    return q, t


_TIES = [(4096, 1), (4096, 8), (1000, 16), (128, 1), (300, 1)]


@pytest.mark.parametrize("nt,batch", _TIES, ids=[_knn_id(64, nt, b) for nt, b in _TIES])
def test_knn_ties_across_splits_and_filter_edges(ctx, oracle, nt, batch):
    q, t = _tie_set(nt, batch)
    _knn_check(ctx, oracle, q, t, max_distances=(64, 63, 48, 256), key=("ties", nt, batch))
    raw, _ = _knn_gpu(ctx, q, t, match=False)
    assert any((raw[b][1] == raw[b][3]).any() for b in range(batch))          # ties present
    if nt >= 300:
        assert any((4 * raw[b][1] == 3 * raw[b][3]).any() for b in range(batch))


@pytest.mark.parametrize("nt", [1, 2, 40])
def test_knn_complementary_rows(ctx, oracle, nt):
    """distance 256: every query the complement of a train row, max_distance 256 keeps them where the ratio allows."""
    rng = np.random.default_rng(nt)
    t = MC.descriptors(rng, nt)[None]
    q = ~t[:, rng.integers(0, nt, 70)]
    _knn_check(ctx, oracle, q, t, max_distances=(255, 256), key=("compl", nt))
    raw, _ = _knn_gpu(ctx, q, t, match=False)
    if nt == 1:
        assert np.all(raw[0][1] == 256) and np.all(raw[0][2] == -1) and np.all(raw[0][3] == -1)


def test_knn_regimes_are_covered():
    regimes = {MC.k1_launch(nq, nt, 1)[1] for nq, nt in _NQ + _NT} | {MC.k1_launch(nq, nt, b)[1] for b, nq, nt in _BATCH}
    assert regimes == {"one", "split", "capped"}
    assert any(MC.k1_launch(nq, nt, 1)[3] for nq, nt in _NQ + _NT)           # some waves get no train rows


def test_knn_refuses_2_20_train_rows_and_stays_usable(ctx, oracle, rs):
    q = np.zeros((1, 4, 32), np.uint8)
    dq, dt = ctx.dev(q), ctx.empty((1 << 20, 32), ctx.torch.uint8)
    with pytest.raises(rs.RsError, match="status 4: nt must be < 2\\^20"):
        ctx.hamming_knn2(dq, dt, 4, 1 << 20)
    with pytest.raises(rs.RsError, match="status 4: nt must be < 2\\^20"):
        ctx.match_descriptors(dq, dt, 4, 1 << 20)
    q, t = MC.knn_set(100, 300, seed=9)
    _knn_check(ctx, oracle, q, t, key="after-refusal")


def test_knn_table_reuse(ctx, oracle):
    """batch x nq grows, shrinks and grows again on one context: every call equals a fresh one (the top-2 table is
    grow-only and must be left all-ones)."""
    seq = [(1, 100, 500), (4, 3000, 500), (1, 7, 64), (2, 9000, 200), (3, 50, 2000), (16, 700, 300), (1, 4097, 900)]
    for batch, nq, nt in seq:
        q, t = MC.knn_set(nq, nt, batch=batch, seed=nq)
        _knn_check(ctx, oracle, q, t, key=("reuse", batch, nq, nt))


# ------------------------------------------------------------------------------------------------------------ K2
def _outs(o, P, N):
    cnt = int(to_np(o["count"])[0])
    return dict(point_kp=to_np(o["point_kp"])[:P], point_dist=to_np(o["point_dist"])[:P],
                prop_point=to_np(o["prop_point"])[:N], prop_dist=to_np(o["prop_dist"])[:N],
                match_kp=to_np(o["match_kp"])[:cnt].copy(), match_point=to_np(o["match_point"])[:cnt].copy())


def _same(a, b, what):
    for k in ("point_kp", "point_dist", "prop_point", "prop_dist", "match_kp", "match_point"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k}"


def _reproj_refs(oracle, name, frame, mp, runs):
    return _cached(("reproj", name), lambda: {(r, md): (oracle.reproj_match(frame, mp, replace=r, max_distance=md),
                                                        MR.reproj_match(frame, mp, r, md)) for r, md in runs})


def _scene(rs, name):
    return _cached(("scene", name), lambda: MC.reproj_case(name, rs.kdtree_build))


def _reproj_all_paths(ctx, frame, mp, replace, md):
    """k2_mode 0 / 1 x tree packed / not: four results that must be identical bytes."""
    P, N = len(mp["positions"]), len(frame["keypoints"])
    fv, k1 = ctx.make_frame_view(frame)
    fvp, k3 = ctx.make_frame_view(frame, pack=True)
    mv, k2 = ctx.make_map_view(mp)
    res = {}
    for mode in (0, 1):
        ctx.set_int("k2_mode", mode)
        try:
            for packed, f in ((0, fv), (1, fvp)):
                res[(mode, packed)] = _outs(ctx.reproj_match(f, mv, replace=replace, max_distance=md), P, N)
        finally:
            ctx.set_int("k2_mode", 0)
    return res


@pytest.mark.parametrize("name", list(MC.REPROJ))
def test_reproj_envelope(ctx, oracle, rs, name):
    frame, mp, runs = _scene(rs, name)
    refs = _reproj_refs(oracle, name, frame, mp, runs)
    for (replace, md), (orc, ref) in refs.items():
        what = f"{name} replace={replace} max_distance={md}"
        res = _reproj_all_paths(ctx, frame, mp, replace, md)
        for path, got in res.items():
            _same(got, orc, f"{what} k2_mode/packed={path} vs oracle")
            MR.assert_reproj_equal(got, ref, f"{what} k2_mode/packed={path} vs reference: ")


def test_reproj_edges_decided_as_documented(ctx, rs):
    """u == 0 / v == 0 accepted, u == width / v == height rejected, behind the camera rejected, on the GPU."""
    frame, mp, _ = _scene(rs, "geom-edges")
    u, v, z = MC.project_f32(frame, mp["positions"])
    n = len(MC.EDGE_UV)
    for i, (eu, ev, _) in enumerate(MC.EDGE_UV):
        assert u[i] == np.float32(eu) and v[i] == np.float32(ev) and z[i] > 0
    accepted = np.array([a for _, _, a in MC.EDGE_UV])
    for path, got in _reproj_all_paths(ctx, frame, mp, 0, 64).items():
        assert np.array_equal(got["point_kp"][:n] >= 0, accepted), path
        assert np.all(got["point_kp"][n:] == -1), path


def test_reproj_proposal_table_reuse(ctx, oracle, rs):
    """N = 2000 -> 8192 -> 100 -> 8192 on one context (both kernels): each equals a fresh call, i.e. the oracle."""
    seq = [("N2000", 2000), ("N8192", 8192), ("N65", 65), ("N8192", 8192)]
    for mode in (0, 1):
        ctx.set_int("k2_mode", mode)
        try:
            for name, _ in seq:
                frame, mp, runs = _scene(rs, name)
                orc = _reproj_refs(oracle, name, frame, mp, runs)[(0, 64)][0]
                fv, k1 = ctx.make_frame_view(frame)
                mv, k2 = ctx.make_map_view(mp)
                _same(_outs(ctx.reproj_match(fv, mv, replace=0), len(mp["positions"]), len(frame["keypoints"])), orc,
                      f"{name} k2_mode {mode}")
        finally:
            ctx.set_int("k2_mode", 0)


def test_reproj_sharded_global_walk(oracle, rs):
    """N = 8192 (global-memory walk), the map in three shards, one empty, through the in-process group: every rank
    returns the unsharded result."""
    import torch
    frame, mp, runs = _scene(rs, "N8192")
    orc = _reproj_refs(oracle, "N8192", frame, mp, runs)[(0, 64)][0]
    P = len(mp["positions"])
    bounds = (0, 1234, 1234, P)
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
                mv, k2 = c.make_map_view(shard(lo, hi))
                mv.n_points = hi - lo
                streams[r].synchronize()
                o = c.reproj_match_sharded(fv, mv, lo)
                streams[r].synchronize()
                out[r] = _outs(o, hi - lo, len(frame["keypoints"]))
        except Exception as ex:      # noqa: BLE001
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
        assert not isinstance(out[r], Exception), out[r]
        lo, hi = bounds[r], bounds[r + 1]
        for k in ("prop_point", "prop_dist", "match_kp", "match_point"):
            assert np.array_equal(out[r][k], orc[k]), (r, k)
        assert np.array_equal(out[r]["point_kp"], orc["point_kp"][lo:hi]), r


def test_resident_map_match_beyond_lds_tree(ctx, rs, oracle, synth):
    """rs_map_match with a frame of 8192 keypoints (> 6144: the global-memory walk) equals the flat path."""
    from test_resident_map import Scene
    sc = Scene(ctx, rs, synth)
    rng = np.random.default_rng(44)
    n_extra = 8192 - len(sc.frame["keypoints"])
    kp = np.concatenate([sc.frame["keypoints"], rng.uniform(0, 500, (n_extra, 2)).astype(np.float32)])
    desc = np.concatenate([sc.frame["descriptors"], MC.flip_bits(rng, sc.frame["descriptors"][rng.integers(0, 500, n_extra)],
                                                                  rng.integers(10, 50, n_extra))])
    node_kp, left, right, root = rs.kdtree_build(kp)
    sc.frame = dict(sc.frame, keypoints=kp, descriptors=desc, kd_node_kp=node_kp, kd_left=left, kd_right=right, kd_root=root)
    sc.rframe.close()
    sc.rframe = rs.ResidentFrame(ctx, kp, desc)
    kpm = (rng.random(len(kp)) < 0.3).astype(np.uint8)
    assert sc.check(oracle) > 50
    assert sc.check(oracle, kp_matched=kpm) > 20
    sc.check(oracle, kp_matched=kpm, replace=1)
    sc.map.close()
