"""The replenishment stage on the GPU (csrc/gftt.hip: rs_detector_*, rs_detect_features, rs_corner_response) against
the CPU restatement tests/gftt_ref.py (goodFeaturesToTrack + Tracker.cpp:127-146).  Tensor sums are exact integers on
both sides and the f32 min-eigenvalue is the same sequence of IEEE operations, so the eig map, the corner list
(positions, responses, order) and both counts are compared for equality, bit for bit.
"""
import functools
import importlib

import numpy as np
import pytest

import gftt_ref as G
import klt_ref as K
from conftest import to_np

pytestmark = pytest.mark.gpu


def _synth():
    return importlib.import_module("racing-slam_amd").synth


@functools.lru_cache(maxsize=None)
def _random(w, h, seed=0):
    return np.random.default_rng(seed * 7919 + w).integers(0, 256, (h, w), dtype=np.uint8)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _band_mask(w, h):
    m = np.full((h, w), 255, np.uint8)
    m[int(0.85 * h):] = 0
    m[:, : w // 7] = 0
    return m


def _detect(ctx, img, mask=None, ex=None, radius=5, max_corners=3000, quality=0.005, md=5.0, border=31, max_total=-1,
            det=None, im=None):
    h, w = img.shape
    own_im, own_det = im is None, det is None
    im = im or ctx.image(w, h, 0, 5, img)
    det = det or ctx.detector(w, h, max(max_corners, 1))
    try:
        d_ex = d_cnt = None
        if ex is not None:
            d_ex = ctx.dev(np.asarray(ex, np.float32).reshape(-1, 2) if len(ex) else np.zeros((1, 2), np.float32))
            d_cnt = ctx.dev(np.array([len(ex)], np.int32))
        r = ctx.detect_features(det, im, None if mask is None else ctx.dev(mask), d_ex, d_cnt, radius, max_corners, quality,
                                md, border, max_total)
        c = to_np(r["counts"]).copy()
        n = int(c[0])
        return dict(pts=to_np(r["pts"])[:n].copy(), response=to_np(r["response"])[:n].copy(), detected=n,
                    appended=int(c[1]), stats=det.stats())
    finally:
        if own_im:
            im.close()
        if own_det:
            det.close()


def _check(got, want):
    assert got["detected"] == want["detected"], (got["detected"], want["detected"])
    assert got["appended"] == want["appended"]
    assert np.array_equal(_bits(got["pts"]), _bits(want["pts"])), "positions / order"
    assert np.array_equal(_bits(got["response"]), _bits(want["response"])), "responses"


@pytest.mark.parametrize("size", [(1920, 1080), (640, 480), (1001, 777), (64, 48), (7, 5), (2, 3), (1, 1)])
def test_eig_map_bit_equal(ctx, size):
    w, h = size
    img = _random(w, h)
    im = ctx.image(w, h, 0, 5, img)
    det = ctx.detector(w, h)
    try:
        eig = to_np(ctx.corner_response(det, im))
        assert np.array_equal(_bits(eig), _bits(G.corner_response(img)))
    finally:
        im.close(); det.close()


@pytest.mark.parametrize("size", [(1920, 1080), (640, 480), (1001, 777)])
@pytest.mark.parametrize("masked", [False, True])
def test_random_frames_bit_equal(ctx, size, masked):
    w, h = size
    img = _random(w, h, 1)
    mask = _band_mask(w, h) if masked else None
    got = _detect(ctx, img, mask)
    want = G.detect_features(img, mask)
    _check(got, want)
    assert got["stats"]["capped"] == min(3000, got["stats"]["accepted"])
    if size == (1920, 1080):
        assert got["stats"]["candidates"] == len(G.candidates(want["eig"], want["mask"], 0.005)[1])
        assert 1 <= got["stats"]["rounds"] and got["detected"] > 2500


def test_klt_frames_with_exclusion_discs(ctx):
    d = _synth().make_klt_pair(1)
    ex = d["pts"][d["label"] == 0][:600]
    for img in (d["img1"], d["img2"]):
        got = _detect(ctx, img, d["mask"], ex, max_total=2000)
        want = G.detect_features(img, d["mask"], ex, max_total=2000)
        _check(got, want)
        assert want["detected"] > 100 and want["appended"] == min(want["detected"], 1400)


def test_all_zero_mask_and_empty_exclusion(ctx):
    img = _random(320, 240, 2)
    z = np.zeros((240, 320), np.uint8)
    got = _detect(ctx, img, z)
    assert got["detected"] == 0 and got["appended"] == 0
    got = _detect(ctx, img, None, np.zeros((0, 2), np.float32), max_total=100)
    _check(got, G.detect_features(img, None, np.zeros((0, 2), np.float32), max_total=100))


def test_exclusion_discs_touching_the_border(ctx):
    w, h = 400, 300
    img = _random(w, h, 3)
    ex = np.array([[0, 0], [w - 1, h - 1], [2.5, 100], [w - 0.5, 3], [200.5, 0.4], [-3.0, 150], [w + 4.0, 150],
                   [np.nan, 5], [1e9, 7], [150.5, 150.5], [151.5, 151.5]], np.float32)
    for radius in (0, 5, 16):
        got = _detect(ctx, img, None, ex, radius=radius, border=0, max_corners=5000, md=1.5)
        _check(got, G.detect_features(img, None, ex, radius, 5000, 0.005, 1.5, 0))


@pytest.mark.parametrize("max_corners,md,max_total,n_ex", [(50, 5.0, -1, 0), (8192, 5.0, -1, 0), (3000, 0.0, -1, 0),
                                                          (3000, 16.0, -1, 0), (2000, 3.0, 500, 500), (2000, 3.0, 300, 500),
                                                          (1, 1.0, 10, 3)])
def test_cap_distance_and_budget(ctx, max_corners, md, max_total, n_ex):
    img = _random(1001, 777, 4)
    ex = np.random.default_rng(5).uniform(0, 1000, (n_ex, 2)).astype(np.float32) if n_ex else None
    got = _detect(ctx, img, None, ex, max_corners=max_corners, md=md, max_total=max_total)
    want = G.detect_features(img, None, ex, 5, max_corners, 0.005, md, 31, max_total)
    _check(got, want)
    if max_total >= 0 and max_total <= n_ex:
        assert got["appended"] == 0 and got["detected"] > 0


def test_cap_not_hit_on_the_corner_scene(ctx):
    d = _synth().make_corner_scene()
    got = _detect(ctx, d["img"], d["mask"])
    want = G.detect_features(d["img"], d["mask"])
    _check(got, want)
    assert got["stats"]["capped"] < 3000 and 250 < got["detected"] < 3000


@pytest.mark.parametrize("period", [4, 8, 16])
def test_plateaus_and_exact_ties(ctx, period):
    """A periodic image: every period the same responses, so many candidates tie exactly (order by offset)."""
    tile = np.random.default_rng(period).integers(0, 256, (period, period), dtype=np.uint8)
    img = np.ascontiguousarray(np.tile(tile, (480 // period + 1, 640 // period + 1))[:480, :640])
    for md in (0.0, 2.0, 5.0):
        got = _detect(ctx, img, md=md, max_corners=4000)
        want = G.detect_features(img, None, None, 5, 4000, 0.005, md)
        _check(got, want)
        assert len(np.unique(want["response"])) < want["detected"] // 4
    flat = np.full((100, 120), 77, np.uint8)
    flat[40:60, 50:70] = 200                                    # a square on a flat plateau
    got = _detect(ctx, flat, border=0)
    _check(got, G.detect_features(flat, border=0))
    assert got["detected"] >= 4


def test_upload_track_detect_chain_without_host_sync(ctx):
    """Tracker::track_features on one stream: upload -> pyramid -> KLT -> replenishment, one read-back at the end."""
    d = _synth().make_klt_pair(2)
    W, H, n = d["width"], d["height"], len(d["pts"])
    a, b = ctx.image(W, H), ctx.image(W, H)
    det = ctx.detector(W, H)
    try:
        a.upload(d["img1"])
        b.upload(d["img2"])
        d_mask = ctx.dev(d["mask"])
        t = ctx.track_features(a, b, ctx.dev(d["pts"]), n, d_mask=d_mask)
        r = ctx.detect_features(det, b, d_mask, t["pts"], t["count"], 5, 3000, 0.005, 5.0, 31, 2000)
        counts = to_np(r["counts"])                             # the one synchronisation
        m = int(to_np(t["count"])[0])
        ref_t = K.track_features(K.build_pyramid(d["img1"]), K.build_pyramid(d["img2"]), d["pts"], d["mask"])
        assert m == len(ref_t["index"]) and np.array_equal(_bits(to_np(t["pts"])[:m]), _bits(ref_t["pts"]))
        want = G.detect_features(d["img2"], d["mask"], ref_t["pts"], 5, 3000, 0.005, 5.0, 31, 2000)
        got = dict(pts=to_np(r["pts"])[:int(counts[0])], response=to_np(r["response"])[:int(counts[0])],
                   detected=int(counts[0]), appended=int(counts[1]))
        _check(got, want)
        assert want["appended"] == min(want["detected"], max(0, 2000 - m))
    finally:
        a.close(); b.close(); det.close()


def test_detector_reuse_across_frames(ctx):
    synth = _synth()
    frames = [synth.make_klt_pair(1, seed=s) for s in range(3)]
    W, H = frames[0]["width"], frames[0]["height"]
    im, det = ctx.image(W, H), ctx.detector(W, H)
    try:
        for k, fr in enumerate(frames):
            im.upload(fr["img2"])
            ex = fr["pts"][: 200 * (k + 1)]
            got = _detect(ctx, fr["img2"], fr["mask"], ex, max_total=1000, det=det, im=im)
            _check(got, G.detect_features(fr["img2"], fr["mask"], ex, max_total=1000))
            # a different call shape on the same detector in between
            got = _detect(ctx, fr["img2"], None, None, md=0.0, max_corners=100, det=det, im=im)
            _check(got, G.detect_features(fr["img2"], None, None, 5, 100, 0.005, 0.0))
    finally:
        im.close(); det.close()


def test_requests_outside_the_envelope_are_refused(ctx, rs):
    import ctypes as C
    for args in [(4097, 100, 3000), (100, 4097, 3000), (640, 480, 8193), (640, 480, 0), (0, 480, 3000)]:
        with pytest.raises(rs.RsError):
            ctx.detector(*args)
    h = C.c_void_p()
    assert ctx.lib.rs_detector_create(ctx.h, 640, 480, 3000, 5, 3, C.byref(h)) == 4      # block size 5: unsupported
    assert ctx.lib.rs_detector_create(ctx.h, 640, 480, 3000, 3, 5, C.byref(h)) == 4      # Sobel 5: unsupported
    img = _random(640, 480)
    im, det = ctx.image(640, 480, 0, 5, img), ctx.detector(640, 480, 1000)
    other = ctx.image(320, 240, 0, 5, _random(320, 240))
    empty = ctx.image(640, 480, 0, 5)
    try:
        ex, cnt = ctx.dev(np.zeros((4, 2), np.float32)), ctx.dev(np.array([4], np.int32))
        bad = [dict(max_corners=1001), dict(max_corners=0), dict(min_distance=16.5), dict(min_distance=-1.0),
               dict(exclude_radius=17), dict(exclude_radius=-1), dict(quality=0.0), dict(quality=1.5), dict(border=-1)]
        for kw in bad:
            a = dict(max_corners=1000)
            a.update(kw)
            with pytest.raises(rs.RsError):
                ctx.detect_features(det, im, d_exclude_pt=ex, d_exclude_count=cnt, **a)
        with pytest.raises(rs.RsError):
            ctx.detect_features(det, im, d_exclude_pt=ex, max_corners=1000)              # points without a count
        with pytest.raises(rs.RsError):
            ctx.detect_features(det, other, max_corners=1000)                            # size differs
        with pytest.raises(rs.RsError):
            ctx.detect_features(det, empty, max_corners=1000)                            # no frame uploaded
        with pytest.raises(rs.RsError):
            ctx.corner_response(det, other)
        # still usable after refusals
        got = _detect(ctx, img, max_corners=1000, det=det, im=im)
        _check(got, G.detect_features(img, max_corners=1000))
    finally:
        im.close(); det.close(); other.close(); empty.close()
