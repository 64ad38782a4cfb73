"""rs_frame from device arrays (csrc/frame.hip: rs_frame_create_device, rs_frame_assign_device, rs_frame_download).

The yardstick is rs_frame_create on the same data downloaded to the host: rs_kdtree_build is deterministic (ties by
(coordinate, keypoint index), node id = position), so the device-built frame must hold the SAME BYTES — keypoints,
descriptor rows, node_kp | left | right, root, packed tree, n.  Every comparison here is equality, with one exception
that is not this feature's: rs_map_bundle_adjust sums f64 with atomics in varying order and reproduces itself to 1e-9
relative with the same LM schedule (test_gpu_parity.test_repeatability_of_a_pass), so two BA runs on byte-equal problems
(the problems ARE compared byte for byte, through rs_map_window) are compared at that, the solver's own noise, plus one
rounding of its f64 results to the f32 outputs.
"""
import ctypes as C

import numpy as np
import pytest

import frame_ref
from conftest import to_np

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1000, 2000, 2001, 4095, 4096, 6144, 6145, 8191, 8192]
KEYS = ("n", "kp", "desc", "kd", "root", "packed")


def _desc(n, seed=0):
    return np.random.default_rng(77 + seed + n).integers(0, 256, (n, 32), dtype=np.uint8)


def _i32(v):
    return np.array([v], np.int32)


def _same(a, b, what=""):
    """Two rs_frame_download results hold the same bytes."""
    for k in KEYS:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)
        else:
            assert x == y, (what, k, x, y)


def _host(ctx, rs, kp, desc):
    f = rs.ResidentFrame(ctx, kp, desc)
    out = f.download()
    f.close()
    return out


def _pad(a, rows):
    """At least `rows` (>= 1) rows: the device arrays a caller hands over are never empty."""
    out = np.zeros((max(rows, 1),) + a.shape[1:], a.dtype)
    out[:len(a)] = a
    return out


def _assign(ctx, frame, kp, desc, split=None):
    """kp[:split] as list a, kp[split:] as list b; returns the download."""
    n = len(kp)
    split = n // 3 if split is None else split
    got = frame.assign(ctx.dev(_pad(desc, n)), ctx.dev(_pad(kp[:split], split)), ctx.dev(_i32(split)),
                       ctx.dev(_pad(kp[split:], n - split)), ctx.dev(_i32(n - split)))
    assert got == n == frame.n
    return frame.download()


@pytest.mark.parametrize("family", frame_ref.FAMILIES)
def test_tree_and_packed_bytes_equal_the_host_frame(ctx, rs, family):
    big = rs.DeviceFrame(ctx, 8192)
    try:
        for n in SIZES:
            kp, desc = frame_ref.keypoints(family, n), _desc(n)
            ref = _host(ctx, rs, kp, desc)
            assert ref["n"] == n and ref["root"] == (n // 2 if n else -1)
            _same(_assign(ctx, big, kp, desc), ref, (family, n, "capacity 8192"))
            tight = rs.DeviceFrame(ctx, max(n, 1))         # capacity == n
            try:
                _same(_assign(ctx, tight, kp, desc, split=n), ref, (family, n, "capacity n"))
            finally:
                tight.close()
            if n in (5, 257, 2000):                        # and against the numpy restatement of the device algorithm
                node_kp, left, right, root = frame_ref.build(kp)
                assert np.array_equal(ref["kd"], np.stack([node_kp, left, right])) and ref["root"] == root
                assert ref["packed"].tobytes() == frame_ref.pack(kp, node_kp, left, right).tobytes()
    finally:
        big.close()


def test_list_rules_follow_the_describer_clamp(ctx, rs):
    cap = 100
    pa, pb = frame_ref.keypoints("uniform", 150, 1), frame_ref.keypoints("uniform", 150, 2)
    desc = _desc(150)
    d_pa, d_pb, d_desc = ctx.dev(pa), ctx.dev(pb), ctx.dev(desc)
    f = rs.DeviceFrame(ctx, cap)
    try:
        cases = [(40, None), (None, 30), (40, 30), (None, None), (150, 30), (1000, 1000), (-5, 30), (40, -1), (-1, -1),
                 (100, 30), (99, 30), (0, 0), (70, 70), (40, 2 ** 31 - 1), (-2 ** 31, 30)]
        for ca, cb in cases:
            na, nb = frame_ref.gather_counts(ca, cb, cap)
            n = f.assign(d_desc, None if ca is None else d_pa, None if ca is None else ctx.dev(_i32(ca)),
                         None if cb is None else d_pb, None if cb is None else ctx.dev(_i32(cb)))
            assert n == na + nb, (ca, cb)
            kp = np.concatenate([pa[:na], pb[:nb]])
            _same(f.download(), _host(ctx, rs, kp, desc[:n]), (ca, cb))
        # neither list and no descriptors at all
        assert f.assign(None) == 0 and f.download()["n"] == 0
        with pytest.raises(rs.RsError):                    # points without their count
            f.assign(d_desc, d_pa, None)
    finally:
        f.close()


def _scene(ctx, rs, synth, n_keypoints, seed=3):
    """A scene of tests/test_resident_map.py with a frame of n_keypoints (its own is 500)."""
    from test_resident_map import Scene
    sc = Scene(ctx, rs, synth, seed=seed)
    if n_keypoints != 500:         # its 500 keypoints (the ones that see the map) followed by clutter
        sc.rframe.close()
        rng = np.random.default_rng(seed)
        fr, extra = dict(sc.frame), n_keypoints - 500
        clutter = np.stack([rng.uniform(0, fr["width"], extra), rng.uniform(0, fr["height"], extra)], 1).astype(np.float32)
        fr["keypoints"] = np.concatenate([fr["keypoints"], clutter])
        fr["descriptors"] = np.concatenate([fr["descriptors"], rng.integers(0, 256, (extra, 32), dtype=np.uint8)])
        fr["kp_matched"] = np.zeros(n_keypoints, np.uint8)
        node_kp, left, right, root = rs.kdtree_build(fr["keypoints"])
        fr.update(kd_node_kp=node_kp, kd_left=left, kd_right=right, kd_root=root)
        sc.frame = fr
        sc.rframe = rs.ResidentFrame(ctx, fr["keypoints"], fr["descriptors"])
    return sc


def _match_all(sc, frame, kpm, pts, only):
    fr = sc.frame
    args = (frame, fr["pose"], sc.K, fr["width"], fr["height"])
    return [sc.map.match(*args),                                                             # match_map
            sc.map.match(*args, required_observer=5),                                        # match_key_frame
            sc.map.match(*args, kp_matched=kpm, matched_points=pts),
            sc.map.match(*args, kp_matched=kpm, matched_points=pts, required_observer=4),
            sc.map.match(*args, kp_matched=kpm, only_points=only, replace=1)]                # match_for_fuse


@pytest.mark.parametrize("n_keypoints", [500, 7000])
def test_matching_equals_the_host_built_frame(ctx, rs, oracle, synth, n_keypoints):
    sc = _scene(ctx, rs, synth, n_keypoints)
    df = rs.DeviceFrame(ctx, 8192)
    try:
        kp, desc = sc.frame["keypoints"], sc.frame["descriptors"]
        assert len(kp) == n_keypoints
        _same(_assign(ctx, df, kp, desc), sc.rframe.download())
        rng = np.random.default_rng(1)
        kpm = (rng.random(n_keypoints) < 0.3).astype(np.uint8)
        pts = rng.choice(600, 80, replace=False)
        only = np.sort(rng.choice(600, 200, replace=False))
        sc.check(oracle)                                    # the host-built frame is right to begin with
        host, dev = _match_all(sc, sc.rframe, kpm, pts, only), _match_all(sc, df, kpm, pts, only)
        for (hk, hp), (dk, dp) in zip(host, dev):
            assert np.array_equal(hk, dk) and np.array_equal(hp, dp)
        assert len(host[0][0]) > 50 and len(host[1][0]) > 0 and len(host[4][0]) > 0
    finally:
        df.close()
        sc.map.close()


def test_key_frame_from_a_device_frame(ctx, rs, synth):
    """Two identical maps; the newest key frame comes from a host-built frame in one and from a device-built frame in the
    other, is given observations, and the device frame is then reassigned.  A later frame matches identically against
    both, the BA problems are byte-equal, and the BA results agree to the solver's own run-to-run noise."""
    a, b = _scene(ctx, rs, synth, 500, seed=7), _scene(ctx, rs, synth, 500, seed=7)
    df = rs.DeviceFrame(ctx, 2048)
    try:
        fr = a.frame
        kp, desc = fr["keypoints"], fr["descriptors"]
        _assign(ctx, df, kp, desc)
        first = a.map.match(a.rframe, fr["pose"], a.K, fr["width"], fr["height"])
        again = b.map.match(df, fr["pose"], b.K, fr["width"], fr["height"])
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and len(first[0]) > 50
        pose = np.asarray(fr["pose"], np.float32).reshape(4, 4)
        ka, kb = a.map.add_keyframe(a.rframe, pose), b.map.add_keyframe(df, pose)
        assert ka == kb == 6
        for k, p in zip(*first):
            a.map.add_observation(int(p), ka, int(k))
            b.map.add_observation(int(p), kb, int(k))
        # the device frame moves on to other contents: the key frame keeps its own rows
        # the later frame: the same view, keypoints moved by a pixel or so, a few descriptor bits flipped, clutter added
        rng = np.random.default_rng(9)
        later = dict(fr)
        later["keypoints"] = np.concatenate([kp + rng.normal(0, 0.7, kp.shape).astype(np.float32),
                                             rng.uniform(0, [fr["width"], fr["height"]], (400, 2)).astype(np.float32)])
        later["descriptors"] = np.concatenate([synth.flip_bits(rng, desc, 0.02), rng.integers(0, 256, (400, 32), dtype=np.uint8)])
        lh = rs.ResidentFrame(ctx, later["keypoints"], later["descriptors"])
        _same(_assign(ctx, df, later["keypoints"], later["descriptors"]), lh.download())
        args = (later["pose"], a.K, later["width"], later["height"])
        for req in (-1, ka, 5):
            ma, mb = a.map.match(lh, *args, required_observer=req), b.map.match(df, *args, required_observer=req)
            assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
            assert len(ma[0]) > 0
        rng = np.random.default_rng(4)                         # BA gets something to do, the same in both maps
        for k in range(2, 7):
            T = (pose if k == 6 else np.array(a.kf_pose[k]).reshape(4, 4)).copy()
            T[:3, 3] += rng.normal(0, 0.01, 3).astype(np.float32)
            a.map.set_keyframe_pose(k, T)
            b.map.set_keyframe_pose(k, T)
        kfs, free = np.arange(7, dtype=np.int32), np.array([0, 0, 1, 1, 1, 1, 1], np.uint8)
        wa, wb = a.map.window(kfs, free), b.map.window(kfs, free)
        for k in wa:
            assert wa[k].tobytes() == wb[k].tobytes(), k
        assert (wa["obs_cam"] == 6).sum() > 50                 # the new key frame's keypoints are in the problem
        sa, pa, ia, xa = a.map.bundle_adjust(kfs, free, a.K)
        sb, pb, ib, xb = b.map.bundle_adjust(kfs, free, b.K)
        assert sa["usable"] == 1 and (sa["iterations"], sa["successful_steps"]) == (sb["iterations"], sb["successful_steps"])
        assert np.array_equal(ia, ib) and np.isclose(sa["final_cost"], sb["final_cost"], rtol=1e-9)
        # f32 outputs of f64 solves that agree to 1e-9 relative: one rounding to f32 apart (2^-23 relative), and for entries
        # near zero 1e-9 of the scene's scale (coordinates up to ~100) = 1e-7 absolute
        assert np.allclose(pa, pb, rtol=2.0 ** -23, atol=1e-7) and np.allclose(xa, xb, rtol=2.0 ** -23, atol=1e-7)
        lh.close()
    finally:
        df.close()
        a.map.close()
        b.map.close()


def test_chain_track_detect_describe_assign_match(ctx, rs, synth):
    """track_features -> detect_features -> describe_features -> DeviceFrame.assign -> map.match with no host read before
    the assign, against the host path fed with the downloaded lists."""
    p = synth.make_klt_pair(2)
    W, H, n = p["width"], p["height"], len(p["pts"])
    im1, im2 = ctx.image(W, H, frame=p["img1"]), ctx.image(W, H, frame=p["img2"])
    det, d = ctx.detector(W, H, 3000), ctx.describer(W, H, 8192)
    df, mp = rs.DeviceFrame(ctx, 8192), rs.ResidentMap(ctx)
    try:
        d_pts, d_mask = ctx.dev(p["pts"]), ctx.dev(p["mask"])
        prev = ctx.describe_features(d, im1, None, None, None, None, 0, d_pts, ctx.dev(_i32(n)))
        tr = ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask)
        g = ctx.detect_features(det, im2, d_mask, tr["pts"], tr["count"], max_total=2000)
        r = ctx.describe_features(d, im2, tr["pts"], tr["count"], tr["index"], prev["desc"], n, g["pts"], g["counts"][1:])
        nf = df.assign(r["desc"], tr["pts"], tr["count"], g["pts"], g["counts"][1:])
        # only now the host looks
        m, app = int(to_np(tr["count"])[0]), int(to_np(g["counts"])[1])
        assert nf == m + app == int(to_np(r["n"])[0]) and m > 500 and app > 0
        kp = np.concatenate([to_np(tr["pts"])[:m], to_np(g["pts"])[:app]])
        desc = to_np(r["desc"])[:nf]
        hf = rs.ResidentFrame(ctx, kp, desc)
        _same(df.download(), hf.download())
        # a map seen from the frame's own pose: every third keypoint is a point 5 m down its ray, observed by a key frame
        # that holds the same keypoints
        K = (1000.0, 1000.0, W / 2.0, H / 2.0)
        T = np.eye(4, dtype=np.float32)
        kf = mp.add_keyframe(hf, T)
        sel = np.arange(0, nf, 3)
        for i in sel:
            z = 5.0
            pt = mp.add_point([(kp[i, 0] - K[2]) / K[0] * z, (kp[i, 1] - K[3]) / K[1] * z, z])
            mp.add_observation(pt, kf, int(i))
        T2 = T.copy()
        T2[0, 3] = 0.01                                      # a small step sideways: ~2 px
        mh, md = mp.match(hf, T2, K, W, H), mp.match(df, T2, K, W, H)
        assert np.array_equal(mh[0], md[0]) and np.array_equal(mh[1], md[1])
        assert len(mh[0]) > len(sel) // 2
        hf.close()
    finally:
        for o in (df, mp, im1, im2, det, d):
            o.close()


def test_descriptor_rows_at_any_byte_offset(ctx, rs):
    """d_desc need not be 16-byte aligned (a view into a larger buffer): the rows are then copied byte by byte."""
    import torch
    f = rs.DeviceFrame(ctx, 1024)
    try:
        for n, off in ((1000, 1), (257, 3), (64, 8), (5, 13)):
            kp, desc = frame_ref.keypoints("uniform", n, 6), _desc(n, 6)
            buf = torch.zeros(32 * n + 16, dtype=torch.uint8, device=ctx.device)
            view = buf[off:off + 32 * n].view(n, 32)
            view.copy_(ctx.dev(desc))
            assert view.data_ptr() % 16 == off
            assert f.assign(view, ctx.dev(kp), ctx.dev(_i32(n))) == n
            _same(f.download(), _host(ctx, rs, kp, desc), (n, off))
    finally:
        f.close()


def test_reuse_of_one_frame(ctx, rs):
    f = rs.DeviceFrame(ctx, 8192)
    try:
        for n, family in ((8192, "uniform"), (5, "grid"), (0, "uniform"), (2000, "uniform"), (8192, "grid"), (1, "zeros")):
            kp, desc = frame_ref.keypoints(family, n, 3), _desc(n, 3)
            _same(_assign(ctx, f, kp, desc), _host(ctx, rs, kp, desc), (n, family))
    finally:
        f.close()


def test_the_same_assign_twice_gives_the_same_bytes(ctx, rs):
    f = rs.DeviceFrame(ctx, 8192)
    try:
        for n in (2000, 8192):
            kp, desc = frame_ref.keypoints("grid", n, 4), _desc(n, 4)
            d = (ctx.dev(desc), ctx.dev(kp[:77]), ctx.dev(_i32(77)), ctx.dev(kp[77:]), ctx.dev(_i32(n - 77)))
            assert f.assign(*d) == n
            first = f.download()
            for _ in range(3):
                assert f.assign(*d) == n
                _same(f.download(), first)
    finally:
        f.close()


def test_refusals(ctx, rs):
    lib = ctx.lib
    h = C.c_void_p()
    for bad in (0, 8193, -1):
        assert lib.rs_frame_create_device(ctx.h, bad, C.byref(h)) == 4          # RS_ERR_UNSUPPORTED
    assert lib.rs_frame_create_device(ctx.h, 16, None) == 1                     # RS_ERR_INVALID
    kp, desc = frame_ref.keypoints("uniform", 16), _desc(16)
    d_kp, d_cnt, d_desc = ctx.dev(kp), ctx.dev(_i32(16)), ctx.dev(desc)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                    # noqa: E731
    n = C.c_int(-1)
    assert lib.rs_frame_assign_device(ctx.h, None, ptr(d_kp), ptr(d_cnt), None, None, ptr(d_desc), C.byref(n)) == 1      # NULL frame
    hf = rs.ResidentFrame(ctx, kp, desc)                                        # a host-created frame has no capacity
    assert lib.rs_frame_assign_device(ctx.h, hf.h, ptr(d_kp), ptr(d_cnt), None, None, ptr(d_desc), C.byref(n)) == 1
    _same(hf.download(), _host(ctx, rs, kp, desc))                              # and is untouched
    other = rs.Context(0)
    try:
        of = rs.DeviceFrame(other, 16)
        assert lib.rs_frame_assign_device(ctx.h, of.h, ptr(d_kp), ptr(d_cnt), None, None, ptr(d_desc), C.byref(n)) == 1  # another context's
        assert lib.rs_frame_download(ctx.h, of.h, C.byref(n), None, None, None, None, None) == 1
        of.close()
    finally:
        other.close()
    assert lib.rs_frame_download(ctx.h, None, C.byref(n), None, None, None, None, None) == 1
    assert n.value == -1
    # the context still works
    f = rs.DeviceFrame(ctx, 16)
    try:
        _same(_assign(ctx, f, kp, desc), hf.download())
        assert f.assign(d_desc, d_kp, d_cnt, None, None) == 16                  # h_n may be NULL too
        assert lib.rs_frame_assign_device(ctx.h, f.h, ptr(d_kp), ptr(d_cnt), None, None, ptr(d_desc), None) == 0
    finally:
        f.close()
        hf.close()


def test_non_finite_coordinates_still_give_a_permutation(ctx, rs):
    """NaN is outside rs_kdtree_build's contract (its comparator is no ordering then): only RS_OK and a permutation."""
    f = rs.DeviceFrame(ctx, 8192)
    try:
        for n in (7, 300, 4097):
            kp = frame_ref.keypoints("uniform", n, 5)
            kp[::7, 0] = np.nan
            kp[3::11, 1] = -np.nan
            kp[5::13] = np.inf
            kp[6::17, 0] = -np.inf
            out = _assign(ctx, f, kp, _desc(n))
            assert np.array_equal(np.sort(out["kd"][0]), np.arange(n))
            left, right, root = frame_ref.closed_form(n)
            assert np.array_equal(out["kd"][1], left) and np.array_equal(out["kd"][2], right) and out["root"] == root
            assert out["kp"].tobytes() == kp.tobytes()
    finally:
        f.close()
