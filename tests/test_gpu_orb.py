"""The description stage on the GPU (csrc/orb.hip: rs_describer_*, rs_describe_features, rs_orb_blur) against the CPU
restatement tests/orb_ref.py (OrbFeatureExtractor::refresh_descriptors).  The blur is the restatement's f32 sequence
of operations and the tests are integer compares, so the plane, the rows, the fresh flags and the count are compared
for equality, byte for byte.
"""
import functools
import importlib

import numpy as np
import pytest

import orb_ref as O
from conftest import to_np

pytestmark = pytest.mark.gpu


def _synth():
    return importlib.import_module("racing-slam_amd").synth


@functools.lru_cache(maxsize=None)
def _random(w, h, seed=0):
    return np.random.default_rng(seed * 7919 + w * 13 + h).integers(0, 256, (h, w), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _pair():
    return _synth().make_klt_pair(2)


def _i32(v):
    return np.array([v], np.int32)


def _run(ctx, d, im, pa=None, ca=None, idx=None, carry=None, pb=None, cb=None, border=31):
    """describe_features with host arrays; returns (desc [n][32], fresh [n], n) read back."""
    dev = lambda a, t=None: None if a is None else ctx.dev(a, t)       # noqa: E731
    n_carry = 0 if carry is None else len(carry)
    r = ctx.describe_features(d, im, dev(pa, np.float32), dev(ca, np.int32), dev(idx, np.int32), dev(carry, np.uint8), n_carry,
                              dev(pb, np.float32), dev(cb, np.int32), border)
    n = int(to_np(r["n"])[0])
    return to_np(r["desc"])[:n].copy(), to_np(r["fresh"])[:n].copy(), n


def _check(got, want):
    desc, fresh, n = got
    assert n == want["n"]
    assert np.array_equal(fresh, want["fresh"]), "fresh flags"
    assert np.array_equal(desc, want["desc"]), f"rows differ: {np.flatnonzero((desc != want['desc']).any(1))[:10]}"


@pytest.mark.parametrize("size", [(1, 1), (7, 3), (3, 7), (63, 63), (101, 77), (129, 65), (640, 480), (1920, 1080)])
def test_blur_plane_bit_equal(ctx, size):
    w, h = size
    img = _random(w, h)
    im = ctx.image(w, h, 0, 5, img)
    d = ctx.describer(w, h, 16)
    try:
        assert np.array_equal(to_np(ctx.orb_blur(d, im)), O.blur(img))
    finally:
        im.close(); d.close()


def test_track_detect_describe_chain_bit_equal(ctx):
    """track_features -> detect_features -> describe_features on one stream, device counts, no host read between;
    then against refresh() on what the first two produced."""
    p = _pair()
    W, H, n = p["width"], p["height"], len(p["pts"])
    im1, im2 = ctx.image(W, H, frame=p["img1"]), ctx.image(W, H, frame=p["img2"])
    det, d = ctx.detector(W, H, 3000), ctx.describer(W, H, 8192)
    try:
        d_pts, d_mask = ctx.dev(p["pts"]), ctx.dev(p["mask"])
        prev = ctx.describe_features(d, im1, None, None, None, None, 0, d_pts, ctx.dev(_i32(n)))    # frame 1's rows
        prev_desc = to_np(prev["desc"])[:n].copy()
        assert int(to_np(prev["n"])[0]) == n
        _check((prev_desc, to_np(prev["fresh"])[:n], n), O.refresh(p["img1"], pts_b=p["pts"]))
        tr = ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask)
        g = ctx.detect_features(det, im2, d_mask, tr["pts"], tr["count"], max_total=2000)
        r = ctx.describe_features(d, im2, tr["pts"], tr["count"], tr["index"], prev["desc"], n, g["pts"], g["counts"][1:])
        m = int(to_np(tr["count"])[0])
        appended = int(to_np(g["counts"])[1])
        kept_idx, kept_pt = to_np(tr["index"])[:m].copy(), to_np(tr["pts"])[:m].copy()
        want = O.refresh(p["img2"], kept_pt, kept_idx, prev_desc, to_np(g["pts"])[:appended])
        total = int(to_np(r["n"])[0])
        assert total == m + appended and m > 1500 and appended > 0
        got = (to_np(r["desc"])[:total].copy(), to_np(r["fresh"])[:total].copy(), total)
        _check(got, want)
        # every corner is inside GFTT's 31-px border: all described
        assert got[1][m:].all()
        # a tracked row that is not fresh is exactly the previous frame's row at its kept index
        stale = np.flatnonzero(got[1][:m] == 0)
        assert np.array_equal(got[0][stale], prev_desc[kept_idx[stale]])
    finally:
        for x in (im1, im2, det, d):
            x.close()


def test_edge_points_carry_their_rows(ctx):
    W, H = 320, 240
    img = _random(W, H, 1)
    im, d = ctx.image(W, H, 0, 5, img), ctx.describer(W, H, 64)
    try:
        carry = _random(32, 20, 2)
        pa = np.array([[5, 100], [30.4, 100], [160, 3], [160, 208.6], [W - 1, H - 1], [100, 100], [288.4, 120], [0, 0]], np.float32)
        idx = np.array([19, 4, 0, 7, 3, 11, 2, 25], np.int32)                 # 25: outside carry -> zeros
        got = _run(ctx, d, im, pa, _i32(len(pa)), idx, carry)
        want = O.refresh(img, pa, idx, carry)
        _check(got, want)
        assert got[1].tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
        assert np.array_equal(got[0][[0, 1, 2, 3, 4]], carry[[19, 4, 0, 7, 3]]) and not got[0][7].any()
        # without an index: row i; without carried rows: zeros
        _check(_run(ctx, d, im, pa, _i32(len(pa)), None, carry), O.refresh(img, pa, None, carry))
        _check(_run(ctx, d, im, pa, _i32(len(pa))), O.refresh(img, pa))
    finally:
        im.close(); d.close()


def test_half_pixel_border_cases(ctx):
    W, H = 200, 151
    img = _random(W, H, 3)
    im, d = ctx.image(W, H, 0, 5, img), ctx.describer(W, H, 64)
    try:
        v = [30.5, 31.5, W - 32.5, W - 31.5, 30.49, 30.51, W - 31.51, W - 31.0, 31.0]
        vy = [30.5, 31.5, H - 32.5, H - 31.5, 30.49, 30.51, H - 31.51, H - 31.0, 31.0]
        pts = np.array([[x, 75.0] for x in v] + [[100.0, y] for y in vy] + [[np.nan, 75], [75, np.inf], [-3e9, 75]], np.float32)
        got = _run(ctx, d, im, pts, _i32(len(pts)))
        want = O.refresh(img, pts)
        _check(got, want)
        assert got[1][:9].tolist() == [0, 1, 1, 1, 0, 1, 1, 0, 1]
        assert got[1][9:18].tolist() == [0, 1, 1, 0, 0, 1, 1, 0, 1]         # H odd: 119.5 -> 120 = H-31, dropped
    finally:
        im.close(); d.close()


def test_list_shapes_and_capacity(ctx):
    W, H = 640, 480
    img = _random(W, H, 4)
    rng = np.random.default_rng(9)
    im, d = ctx.image(W, H, 0, 5, img), ctx.describer(W, H, 8192)
    try:
        pa = rng.uniform(-10, [W + 10, H + 10], (8192, 2)).astype(np.float32)
        pb = rng.uniform(20, [W - 20, H - 20], (8192, 2)).astype(np.float32)
        carry = rng.integers(0, 256, (8192, 32), dtype=np.uint8)
        idx = rng.integers(-5, 8200, 8192).astype(np.int32)
        # empty lists, and both lists absent
        assert _run(ctx, d, im, pa, _i32(0), idx, carry, pb, _i32(0))[2] == 0
        assert _run(ctx, d, im)[2] == 0
        # only a, only b
        _check(_run(ctx, d, im, pa[:300], _i32(300), idx, carry), O.refresh(img, pa[:300], idx, carry))
        _check(_run(ctx, d, im, None, None, None, None, pb[:500], _i32(500)), O.refresh(img, pts_b=pb[:500]))
        # 8192 points in all
        _check(_run(ctx, d, im, pa[:5000], _i32(5000), idx, carry, pb, _i32(3192)),
               O.refresh(img, pa[:5000], idx, carry, pb[:3192]))
        _check(_run(ctx, d, im, pa, _i32(8192), idx, carry), O.refresh(img, pa, idx, carry))
        # device counts above capacity: list a first, b gets what is left; negative counts are 0
        _check(_run(ctx, d, im, pa[:6000], _i32(6000), idx, carry, pb, _i32(99999)),
               O.refresh(img, pa[:6000], idx, carry, pb, max_points=8192))
        _check(_run(ctx, d, im, pa, _i32(10 ** 6), idx, carry, pb, _i32(5)), O.refresh(img, pa, idx, carry, pb[:5]))
        _check(_run(ctx, d, im, pa, _i32(-7), idx, carry, pb[:40], _i32(40)), O.refresh(img, None, None, None, pb[:40]))
        small = ctx.describer(W, H, 100)
        try:
            _check(_run(ctx, small, im, pa[:100], _i32(250), idx, carry, pb[:100], _i32(100)),
                   O.refresh(img, pa[:100], idx, carry, pb[:100], max_points=100))
        finally:
            small.close()
    finally:
        im.close(); d.close()


def test_two_calls_give_the_same_bytes(ctx):
    p = _pair()
    W, H = p["width"], p["height"]
    im, d = ctx.image(W, H, frame=p["img2"]), ctx.describer(W, H, 4096)
    try:
        pts, cnt = ctx.dev(p["truth"]), ctx.dev(_i32(len(p["truth"])))
        a = ctx.describe_features(d, im, pts, cnt)
        first = (to_np(a["desc"]).copy(), to_np(a["fresh"]).copy(), to_np(a["n"]).copy())
        ctx.describe_features(d, im, pts, cnt, out=a)
        assert np.array_equal(first[0], to_np(a["desc"])) and np.array_equal(first[1], to_np(a["fresh"]))
        assert first[2][0] == len(p["truth"])
    finally:
        im.close(); d.close()


def test_descriptors_recover_the_klt_correspondence(ctx):
    """End to end: frame-1 rows and the chain's frame-2 rows through the existing rs_match_descriptors; the match of a
    tracked textured point is, for most of them, the point it was tracked from."""
    p = _pair()
    W, H, n = p["width"], p["height"], len(p["pts"])
    im1, im2 = ctx.image(W, H, frame=p["img1"]), ctx.image(W, H, frame=p["img2"])
    det, d1, d2 = ctx.detector(W, H, 3000), ctx.describer(W, H, 4096), ctx.describer(W, H, 4096)
    try:
        d_pts, d_mask = ctx.dev(p["pts"]), ctx.dev(p["mask"])
        r1 = ctx.describe_features(d1, im1, d_pts, ctx.dev(_i32(n)))
        tr = ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask)
        g = ctx.detect_features(det, im2, d_mask, tr["pts"], tr["count"], max_total=2000)
        r2 = ctx.describe_features(d2, im2, tr["pts"], tr["count"], tr["index"], r1["desc"], n, g["pts"], g["counts"][1:])
        m = int(to_np(tr["count"])[0])
        kept_idx = to_np(tr["index"])[:m]
        textured = p["label"][kept_idx] == 0
        mt = ctx.match_descriptors(r2["desc"][:m].contiguous(), r1["desc"][:n].contiguous(), m, n)
        cnt = int(to_np(mt["cnt"])[0])
        q, t = to_np(mt["mq"])[0, :cnt], to_np(mt["mt"])[0, :cnt]
        right = np.zeros(m, bool)
        right[q[t == kept_idx[q]]] = True
        frac = right[textured].mean()
        print(f"{m} tracked, {cnt} matches, correspondence recovered for {100 * frac:.1f} % of textured points")
        assert frac > 0.8
    finally:
        for x in (im1, im2, det, d1, d2):
            x.close()


def test_envelope(ctx, rs):
    with pytest.raises(rs.RsError):
        ctx.describer(4097, 16)
    with pytest.raises(rs.RsError):
        ctx.describer(64, 64, 8193)
    with pytest.raises(rs.RsError):
        ctx.describer(64, 64, 0)
    img = _random(64, 64, 5)
    im, d = ctx.image(64, 64, 0, 5, img), ctx.describer(64, 64, 8)
    other = ctx.image(65, 64, 0, 5, _random(65, 64, 5))
    try:
        pts, cnt = ctx.dev(np.zeros((8, 2), np.float32)), ctx.dev(_i32(8))
        with pytest.raises(rs.RsError):
            ctx.describe_features(d, im, pts, cnt, border=15)
        with pytest.raises(rs.RsError):
            ctx.describe_features(d, im, pts, None)
        with pytest.raises(rs.RsError):
            ctx.describe_features(d, other, pts, cnt)
        with pytest.raises(rs.RsError):
            ctx.orb_blur(d, other)
        got = _run(ctx, d, im, np.full((8, 2), 32, np.float32), _i32(8), border=16)
        _check(got, O.refresh(img, np.full((8, 2), 32, np.float32), border=16))
        assert got[1].all()
    finally:
        im.close(); d.close(); other.close()
