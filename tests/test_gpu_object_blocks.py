"""Every fixed-capacity object keeps its device arrays as adjoining pieces of one block (csrc/carve.h, csrc/dev_array.h), so a
kernel that wrote one entry past an array would land in its neighbour, not in an allocator's slack.  Each stage therefore
runs twice on the same small input — once on an object whose capacity is exactly the input's size, once on one of four times
that capacity (where the pieces lie elsewhere and tails are padding) — and everything the Python wrapper returns or downloads
must hold the same bytes.  Sizes: n = 65 and 257 (a piece's tail is padding, the last workgroup partial), images of 67 x 35,
33 hypotheses, a database of 3 entries and exactly the words added.  Output arrays are handed in zeroed, so that rows a stage
does not write compare equal; an array whose shape follows the capacity is compared over the input's rows.

rs_image has no capacity beyond its size: its two forms are a pyramid of exactly the levels and padding the tracking call
uses (max_level 1, window 5) and one with more of both (max_level 4, window 7; 67 x 35 gives it three levels)."""
import functools

import numpy as np
import pytest

import loop_cases
from conftest import to_np
from loop_checks import Built
from trackstore_cases import monotone_lists

pytestmark = pytest.mark.gpu

SIZES = (65, 257)
W, H = 67, 35
HYP = 33


def _same(a, b, what=""):
    """The same bytes, through dicts, lists and tuples."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), what


def _np(d):
    return {k: to_np(v).copy() for k, v in d.items()}


def _zeros(ctx, shape, dtype):
    return ctx.dev(np.zeros(shape, dtype))


def _count(ctx, n):
    return ctx.dev(np.array([n], np.int32))


@functools.lru_cache(maxsize=None)
def _frames():
    """Two 67 x 35 crops of synth.make_klt_pair's 640 x 480 pair (textured ground, away from its flat and occluded patches)."""
    pair = loop_cases.synth().make_klt_pair(config_id=1, seed=0, n_points=400)
    y0, x0 = 300, 200
    return pair["img1"][y0:y0 + H, x0:x0 + W].copy(), pair["img2"][y0:y0 + H, x0:x0 + W].copy()


def _points(n, lo, hi, seed):
    rng = np.random.default_rng([0xB10C, n, seed])
    return np.stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n)], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ rs_image + rs_klt_track
def _klt(ctx, n, max_level, win):
    img1, img2 = _frames()
    a, b = ctx.image(W, H, max_level, win, img1), ctx.image(W, H, max_level, win, img2)
    try:
        assert len(a.levels()) >= 2
        out = dict(next=_zeros(ctx, (n, 2), np.float32), status=_zeros(ctx, (n,), np.uint8))
        ctx.klt_track(a, b, ctx.dev(_points(n, (0, 0), (W - 1, H - 1), 1)), n, win=5, max_level=1, out=out)
        got = _np(out)
        for im, name in ((a, "from"), (b, "to")):
            for level in (0, 1):                        # the levels the call reads, without their padding
                got[f"{name}{level}"] = [p[win:-win, win:-win].copy() for p in im.download(level)]
        return got
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("n", SIZES)
def test_image_and_klt_track(ctx, n):
    exact = _klt(ctx, n, 1, 5)
    assert exact["status"].any()
    _same(exact, _klt(ctx, n, 4, 7), "klt")


# ------------------------------------------------------------------------------------------------ rs_detector
def _detect(ctx, img, n, capacity):
    det = ctx.detector(W, H, capacity)
    try:
        out = dict(pts=_zeros(ctx, (n, 2), np.float32), response=_zeros(ctx, (n,), np.float32), counts=_zeros(ctx, (2,), np.int32))
        ctx.detect_features(det, img, max_corners=n, quality=0.005, min_distance=1.0, border=1, out=out)
        got = _np(out)
        got["stats"] = det.stats()
        got["eig"] = to_np(ctx.corner_response(det, img)).copy()
        return got
    finally:
        det.close()


@pytest.mark.parametrize("n", SIZES)
def test_detector(ctx, n):
    img = ctx.image(W, H, 1, 5, _frames()[0])
    try:
        exact = _detect(ctx, img, n, n)
        assert exact["counts"][0] > 0
        _same(exact, _detect(ctx, img, n, 4 * n), "detect")
    finally:
        img.close()


# ------------------------------------------------------------------------------------------------ rs_describer
def _describe(ctx, img, n, capacity):
    d = ctx.describer(W, H, capacity)
    try:
        out = dict(desc=_zeros(ctx, (capacity, 32), np.uint8), fresh=_zeros(ctx, (capacity,), np.uint8), n=_zeros(ctx, (1,), np.int32))
        # border 16 keeps centres in [16, 50] x [16, 18]: points on both sides of the filter
        ctx.describe_features(d, img, ctx.dev(_points(n, (10, 12), (56, 22), 2)), _count(ctx, n), border=16, out=out)
        got = _np(out)
        got["desc"], got["fresh"] = got["desc"][:n], got["fresh"][:n]
        got["blur"] = to_np(ctx.orb_blur(d, img)).copy()
        return got
    finally:
        d.close()


@pytest.mark.parametrize("n", SIZES)
def test_describer(ctx, n):
    img = ctx.image(W, H, 1, 5, _frames()[0])
    try:
        exact = _describe(ctx, img, n, n)
        assert exact["n"][0] == n and exact["fresh"].any() and not exact["fresh"].all()
        _same(exact, _describe(ctx, img, n, 4 * n), "describe")
    finally:
        img.close()


# ------------------------------------------------------------------------------------------------ the two pose RANSACs
def _pose_out(ctx, n):
    return dict(pose=_zeros(ctx, (4, 4), np.float32), inlier=_zeros(ctx, (n,), np.uint8), inlier_index=_zeros(ctx, (n,), np.int32),
                inlier_count=_zeros(ctx, (1,), np.int32), status=_zeros(ctx, (1,), np.int32))


def _estimator_outputs(est, out):
    got = _np(out)
    got["stats"] = est.stats()
    got["hypotheses"] = {k: v[:HYP].copy() for k, v in est.hypotheses().items()}
    return got


def _pose(ctx, n, scale):
    s = loop_cases.synth().make_pose_pair(seed=3, n=n, outlier_frac=0.2)
    est = ctx.pose_estimator(scale * n, scale * HYP)
    try:
        out = ctx.estimate_pose(est, ctx.dev(s["pts_from"]), ctx.dev(s["pts_to"]), _count(ctx, n), n, s["K"], max_hypotheses=HYP, seed=7,
                                out=_pose_out(ctx, n))
        return _estimator_outputs(est, out)
    finally:
        est.close()


@pytest.mark.parametrize("n", SIZES)
def test_pose_estimator(ctx, n):
    exact = _pose(ctx, n, 1)
    assert exact["status"][0] == 0 and exact["inlier_count"][0] > 0
    _same(exact, _pose(ctx, n, 4), "pose")


def _pnp(ctx, n, scale):
    s = loop_cases.synth().make_pnp_scene(seed=3, n=n, outlier_frac=0.2)
    est = ctx.pnp_estimator(scale * n, scale * HYP)
    try:
        out = ctx.estimate_pose_pnp(est, ctx.dev(s["points"]), ctx.dev(s["pixels"]), _count(ctx, n), n, s["K"], max_hypotheses=HYP, seed=7,
                                    out=_pose_out(ctx, n))
        return _estimator_outputs(est, out)
    finally:
        est.close()


@pytest.mark.parametrize("n", SIZES)
def test_pnp_estimator(ctx, n):
    exact = _pnp(ctx, n, 1)
    assert exact["status"][0] == 0 and exact["inlier_count"][0] > 0
    _same(exact, _pnp(ctx, n, 4), "pnp")


# ------------------------------------------------------------------------------------------------ rs_bow, rs_bow_database
@functools.lru_cache(maxsize=None)
def _voc():
    return loop_cases.synth().make_vocabulary(4, 3, seed=1)


def _bow(ctx, voc, n, scale, db_words):
    """Three frames of n rows transformed, added to a database of (3, db_words) entries and words times `scale`, and scored
    against the last one.  db_words None: no database, the words the three vectors hold are counted instead."""
    rows = [loop_cases.synth().make_bow_descriptors(_voc(), n, seed=k) for k in range(3)]
    bow = ctx.bow(voc, scale * n)
    db = None if db_words is None else ctx.bow_database(voc, scale * 3, scale * db_words)
    try:
        got = dict(words=[], vectors=[], entries=[])
        for r in rows:
            got["words"].append(to_np(bow.transform(ctx.dev(r), _count(ctx, n), n)).copy())
            got["vectors"].append(bow.download())
            if db is not None:
                got["entries"].append(db.add(bow))
        if db is not None:
            got["counts"] = list(db.counts())
            got["scores"] = to_np(db.score(bow)).copy()
        return got
    finally:
        bow.close()
        if db is not None:
            db.close()


@pytest.mark.parametrize("n", SIZES)
def test_bow_and_database(ctx, n):
    v = _voc()
    voc = ctx.vocabulary(v["k"], v["L"], 0, 0, v["parent"], v["desc"], v["weight"])
    try:
        total = sum(len(x["words"]) for x in _bow(ctx, voc, n, 1, None)["vectors"])
        exact = _bow(ctx, voc, n, 1, total)
        assert exact["counts"] == [3, total] and exact["entries"] == [0, 1, 2]
        _same(exact, _bow(ctx, voc, n, 4, total), "bow")
    finally:
        voc.close()


# ------------------------------------------------------------------------------------------------ the scenes with a map
@functools.lru_cache(maxsize=None)
def _loop_scene(n, candidates):
    shared = (n - 2) // 3                               # the candidates' shared query keypoints are disjoint
    return loop_cases.synth().loop_scene(40 + n, n, tuple((n, (3 * n) // 4, shared, 0.1, None) for _ in range(candidates)))


# ------------------------------------------------------------------------------------------------ rs_frame
@pytest.mark.parametrize("n", SIZES)
def test_device_frame_assign_then_match(ctx, rs, n):
    b = Built(ctx, rs, _loop_scene(n, 1))
    try:
        s = b.s
        q = s["key_frames"][s["query"]]
        split = n // 3
        d_desc, d_a, d_b = ctx.dev(q["desc"]), ctx.dev(q["kp"][:split]), ctx.dev(q["kp"][split:])

        def run(capacity):
            f = rs.DeviceFrame(ctx, capacity)
            try:
                assert f.assign(d_desc, d_a, _count(ctx, split), d_b, _count(ctx, n - split)) == n
                got = dict(frame=f.download(), empty_table=f.matches())
                got["match"] = b.map.match(f, s["true_pose"].astype(np.float32), s["K"], s["width"], s["height"])
                got["new"] = b.map.match_frame(f, s["true_pose"].astype(np.float32), s["K"], s["width"], s["height"])
                got["table"] = f.matches()
                return got
            finally:
                f.close()

        exact = run(n)
        assert len(exact["match"][0]) > 0 and exact["new"] > 0
        _same(exact, run(4 * n), "frame")
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ rs_track_store
def _track_store(ctx, rs, n, capacity):
    rng = np.random.default_rng([0x75, n])
    ts = rs.TrackStore(ctx, capacity, 3)
    frames = []
    try:
        got, n_prev = dict(query=[], store=[]), 0
        for k in range(5):
            if k:
                prev, inl = monotone_lists(rng, n_prev, n)
                ts.carry(ctx.dev(prev), ctx.dev(inl) if len(inl) else None, _count(ctx, len(inl)) if len(inl) else None, len(prev))
            pix = rng.uniform(0, 700, (n, 2)).astype(np.float32)
            frames.append(rs.ResidentFrame(ctx, pix, np.zeros((n, 32), np.uint8)))
            ts.extend(frames[-1], 10 + k, k // 2 if k % 2 == 0 else -1)
            got["query"].append(ts.query(frames[-1], min_sightings=2, min_travel=5.0))
            got["store"].append(ts.download())
            n_prev = n
        return got
    finally:
        ts.close()
        for f in frames:
            f.close()


@pytest.mark.parametrize("n", SIZES)
def test_track_store(ctx, rs, n):
    exact = _track_store(ctx, rs, n, n)
    assert exact["store"][-1]["n"] >= n and (exact["store"][-1]["count"] == 3).any()
    _same(exact, _track_store(ctx, rs, n, 4 * n), "track store")


# ------------------------------------------------------------------------------------------------ rs_loop_verifier
def _verify(ctx, b, n, candidates, max_points, max_candidates, max_hyp):
    s = b.s
    ver = ctx.loop_verifier(max_points, max_candidates, max_hyp)
    try:
        got = dict(verdict=ver.verify(b.map, s["query"], list(range(candidates)), s["K"], s["width"], max_hypotheses=HYP))
        got["chains"] = [ver.download(c) for c in range(candidates)]
        return got
    finally:
        ver.close()


@pytest.mark.parametrize("candidates", (1, 3))
@pytest.mark.parametrize("n", SIZES)
def test_loop_verifier(ctx, rs, n, candidates):
    b = Built(ctx, rs, _loop_scene(n, candidates))
    try:
        exact = _verify(ctx, b, n, candidates, n, candidates, HYP)
        assert all(v["status"] == 0 for v in exact["verdict"])
        _same(exact, _verify(ctx, b, n, candidates, 4 * n, min(4 * candidates, 8), 4 * HYP), "loop")
    finally:
        b.close()
