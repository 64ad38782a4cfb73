"""The one-workgroup tails and heads of a key-frame pass — K3 (k3_accept), K4's head and K4b (k4_compact, single and
batched), K6b (k6_select) and the bundle adjustment's finalize — at the sizes where each takes another path: one chunk
of a thread held in registers (1024 threads x 8 entries) against the two-pass fallback, a device count below the launch
bound, a rejected list inside K6b's LDS table (2048 entries) and beyond it.

K3, K4 / K4b and K6 / K6b are held against the oracle bit for bit (finite floats equal in every bit, non-finite ones
non-finite in the same places).  Of a bundle adjustment the schedule (termination, iterations, successful steps, usable,
the outcome of every iteration) equals the oracle's exactly; its f64 sums are accumulated by atomics in another order
than the oracle's loops, so costs, radii and cameras are held to the bounds the suite already uses for them
(test_golden.py::test_gpu_lm_trace_golden); what finalize itself decides — that the pinned camera mirror is the device
array — is checked bit for bit."""
import numpy as np
import pytest

import match_cases as MC
import tri_cases as C
from conftest import to_np

pytestmark = pytest.mark.gpu

PAD = 16
SENT_I, SENT_B = -0x01234567, 0xA5
K3_REGISTER_BOUND = 8 * 1024          # entries one workgroup of K3 / K4b / K6b holds in registers
K6B_REJ_LDS = 2048                    # rejected candidates K6b ranks out of LDS


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_floats(got, ref, tag=""):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), tag
    assert np.array_equal(bits(got)[fin], bits(ref)[fin]), tag


def _untouched(a, tag=""):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        assert (a == SENT_B).all(), tag
    else:
        assert (a.view(np.int32) == SENT_I).all(), tag


def _sentinel(ctx, shape, dtype):
    t = ctx.torch
    if dtype == t.uint8:
        return t.full(shape, SENT_B, dtype=t.uint8, device=ctx.device)
    return t.full(shape, SENT_I, dtype=t.int32, device=ctx.device).view(dtype)


def _np(out):
    return {k: to_np(v) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------- K3
def _k3_outs(o, P, N):
    cnt = int(to_np(o["count"])[0])
    return dict(point_kp=to_np(o["point_kp"])[:P], point_dist=to_np(o["point_dist"])[:P], prop_point=to_np(o["prop_point"])[:N],
                prop_dist=to_np(o["prop_dist"])[:N], match_kp=to_np(o["match_kp"])[:cnt].copy(), match_point=to_np(o["match_point"])[:cnt].copy())


@pytest.mark.parametrize("n", [1, 2, 1023, 1025, 2049, K3_REGISTER_BOUND + 8])
def test_k3_accept_sizes_twice_on_one_context(ctx, oracle, rs, n):
    """Frames of n keypoints against a map of 300 points, twice in a row on the same context (the second call sees the
    proposal table as the first one's K3 left it), then once through the sharded entry point, which shares K3's body."""
    frame, mp = MC.scene(N=n, P=300, seed=500 + n, kdtree_build=rs.kdtree_build)
    ref = oracle.reproj_match(frame, mp, replace=0, max_distance=64)
    fv, k1 = ctx.make_frame_view(frame)
    mv, k2 = ctx.make_map_view(mp)
    runs = [ctx.reproj_match(fv, mv), ctx.reproj_match(fv, mv), ctx.reproj_match_sharded(fv, mv, 0)]
    for call, o in enumerate(runs):
        got = _k3_outs(o, 300, n)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (n, call, k)
    if n >= 1023:
        assert len(ref["match_kp"]) > 0


# ----------------------------------------------------------------------------------------------------- K4 head and K4b
K4_SIZES = (1, 63, 64, 65, 1025, K3_REGISTER_BOUND + 8)
GARBAGE = np.array([0x7FFFFFFF, -1, -0x40000000, 0x12345678], np.int32)


def _k4_out(ctx, rows, counts=1):
    t = ctx.torch
    return dict(xyz=_sentinel(ctx, (rows + PAD, 3), t.float32), keep=_sentinel(ctx, (rows + PAD,), t.uint8),
                out_index=_sentinel(ctx, (rows + PAD,), t.int32), out_xyz=_sentinel(ctx, (rows + PAD, 3), t.float32),
                count=_sentinel(ctx, (counts + PAD,), t.int32))


def _check_k4(got, ref, base, rows, count_at, tag):
    """The pair's slice starts at row `base` and is `rows` long; ref covers the m rows below the device count.  Rows from m
    on are as they were before the call, and so are the compacted rows from the count on."""
    m, k = len(ref["keep"]), len(ref["out_index"])
    _same_floats(got["xyz"][base:base + m], ref["xyz"], tag)
    assert np.array_equal(got["keep"][base:base + m], ref["keep"]), tag
    assert int(got["count"][count_at]) == k, tag
    assert np.array_equal(got["out_index"][base:base + k], ref["out_index"]), tag
    _same_floats(got["out_xyz"][base:base + k], ref["out_xyz"], tag)
    for name, lo in (("xyz", m), ("keep", m), ("out_index", k), ("out_xyz", k)):
        _untouched(got[name][base + lo:base + rows], tag + " " + name)


_K4_REF = {}


def _k4_case(oracle, n):
    """n correspondences (half of them kept), their keypoints shuffled and gathered back, and the oracle over all of them:
    the oracle's rows are independent, so the first m of them are the oracle of a call with a device count of m."""
    if n not in _K4_REF:
        c = C.compaction_case("random50", n)
        rng = np.random.default_rng(n)
        p1, p2 = rng.permutation(n), rng.permutation(n)
        ref = oracle.triangulate(c["uv1"], c["uv2"], c["poses"], C.K)
        _K4_REF[n] = (c, c["uv1"][p1], c["uv2"][p2], np.argsort(p1).astype(np.int32), np.argsort(p2).astype(np.int32), ref)
    return _K4_REF[n]


def _k4_ref_prefix(ref, m):
    kept = np.flatnonzero(ref["keep"][:m] != 0).astype(np.int32)
    return dict(xyz=ref["xyz"][:m], keep=ref["keep"][:m], out_index=kept, out_xyz=ref["xyz"][kept])


def _with_garbage(g, m):
    g = g.copy()
    g[m:] = np.resize(GARBAGE, len(g) - m)
    return g


@pytest.mark.parametrize("n", K4_SIZES)
def test_k4_matches_device_counts_and_garbage_beyond(ctx, oracle, n):
    """rs_triangulate_matches with max_matches = n and *d_n at 0, 1, n - 1 and n; the gather lists hold garbage from the
    count on (indices far outside the keypoint arrays): no row at or beyond the count may be computed, kept or written."""
    c, kp1, kp2, g1, g2, ref = _k4_case(oracle, n)
    full = _k4_ref_prefix(ref, n)
    assert np.array_equal(full["out_index"], ref["out_index"]) and np.array_equal(bits(full["out_xyz"]), bits(ref["out_xyz"]))
    d_kp1, d_kp2, d_poses = ctx.dev(kp1), ctx.dev(kp2), ctx.dev(c["poses"])
    for count in sorted({0, 1, n - 1, n}):
        got = _np(ctx.triangulate_matches(d_kp1, d_kp2, ctx.dev(_with_garbage(g1, count)), ctx.dev(_with_garbage(g2, count)),
                                          ctx.dev(np.array([count], np.int32)), n, d_poses, C.K, out=_k4_out(ctx, n)))
        _check_k4(got, _k4_ref_prefix(ref, count), 0, n + PAD, 0, "count %d of %d" % (count, n))
        _untouched(got["count"][1:], "count")


@pytest.mark.parametrize("n", K4_SIZES)
def test_k4_batch_with_different_counts(ctx, oracle, n):
    """rs_triangulate_matches_batch, four pairs of stride n with the counts n, 0, n - 1 and 1 and garbage beyond each."""
    c, kp1, kp2, g1, g2, ref = _k4_case(oracle, n)
    counts = np.array([n, 0, n - 1, 1], np.int32)
    B = len(counts)
    mt = np.stack([_with_garbage(g1, int(m)) for m in counts])
    mq = np.stack([_with_garbage(g2, int(m)) for m in counts])
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))        # noqa: E731
    got = _np(ctx.triangulate_matches_batch(ctx.dev(tile(kp1)), ctx.dev(tile(kp2)), ctx.dev(mt), ctx.dev(mq), ctx.dev(counts),
                                            ctx.dev(tile(c["poses"])), C.K, out=_k4_out(ctx, B * n, counts=B)))
    for b in range(B):
        _check_k4(got, _k4_ref_prefix(ref, int(counts[b])), b * n, n, b, "pair %d, stride %d" % (b, n))
    for k in ("xyz", "keep", "out_index", "out_xyz"):
        _untouched(got[k][B * n:], k)
    _untouched(got["count"][B:], "count")


# --------------------------------------------------------------------------------------------------------------- K6b
def _k6_kinds(n, seed, nan_every=0):
    rng = np.random.default_rng(seed)
    kinds = list(rng.choice(list("ARIS"), n, p=(0.2, 0.5, 0.15, 0.15)))
    if nan_every:
        for t in range(3, n, nan_every):
            kinds[t] = "N"
    return kinds


def _k6_tables():
    """name -> (kinds, dups, low, quotas).  Every quota lies above the accepted count, so the top-up runs.  A dup is a
    byte-for-byte copy of a track (equal cosines), `low` puts the copied tracks at the head of the order, N is a
    candidate with a NaN cosine."""
    T = {"n1_R": (["R"], (), (), (1, 5)), "n1_N": (["N"], (), (), (1,))}
    for n in (1023, 1025, 2049):
        kinds = _k6_kinds(n, n, nan_every=37)
        for t in (9, 10, 11, 14, 15, 300, 301, 302):
            kinds[t] = "R"
        na, nr = kinds.count("A"), kinds.count("R") + kinds.count("N")
        assert nr <= K6B_REJ_LDS
        T["mixed_%d" % n] = (kinds, ((9, 10), (9, 11), (14, 15), (300, 301), (300, 302)), (9, 14, 300), (na + 1, na + 4, na + nr - 2, na + nr + 7))
    kinds = ["R"] * 2049                                   # 2049 rejected candidates: one more than the LDS table holds
    for t in range(5, 2049, 101):
        kinds[t] = "N"
    T["all_rejected_2049"] = (kinds, ((9, 10), (9, 11), (14, 15), (300, 301), (300, 302), (300, 303)), (9, 14, 300), (1, 2, 5, 2040, 2049, 3000))
    return T


K6_TABLES = _k6_tables()
_K6_SCENES = {}


def _k6_scene(name):
    if name not in _K6_SCENES:
        kinds, dups, low, _ = K6_TABLES[name]
        _K6_SCENES[name] = C.track_scene("".join(kinds), 77 + len(kinds), dups, low)
    return _K6_SCENES[name]


@pytest.mark.parametrize("name", list(K6_TABLES))
def test_k6_select_quota_top_up(ctx, rs, oracle, name):
    sc = _k6_scene(name)
    n = len(sc["track_uv"])
    t = ctx.torch
    req = rs.parallax_requirements(sc["poses"], sc["kf_pose"])
    dev = [ctx.dev(sc[k]) for k in ("track_uv", "sight_ptr", "sight_pose", "sight_uv", "poses")]
    d_skip, d_req = ctx.dev(sc["skip"]), ctx.dev(req)
    for quota in K6_TABLES[name][3]:
        ref = oracle.triangulate_tracks(sc["track_uv"], sc["sight_ptr"], sc["sight_pose"], sc["sight_uv"], sc["poses"], sc["kf_pose"], C.K,
                                        skip=sc["skip"], min_new_points=quota)
        out = dict(status=_sentinel(ctx, (n + PAD,), t.uint8), xyz=_sentinel(ctx, (n + PAD, 3), t.float32),
                   parallax_cos=_sentinel(ctx, (n + PAD,), t.float32), required_cos=_sentinel(ctx, (n + PAD,), t.float32),
                   accepted=_sentinel(ctx, (n + PAD,), t.int32), inconsistent=_sentinel(ctx, (n + PAD,), t.int32),
                   counts=_sentinel(ctx, (3 + PAD,), t.int32))
        got = _np(ctx.triangulate_tracks(*dev, sc["kf_pose"], C.K, d_skip=d_skip, min_new_points=quota, d_required=d_req, out=out))
        tag = "%s quota %d" % (name, quota)
        assert np.array_equal(got["status"][:n], ref["status"]), tag
        _same_floats(got["parallax_cos"][:n], ref["parallax_cos"], tag)
        assert np.array_equal(bits(got["required_cos"][:n]), bits(ref["required_cos"])), tag
        na, top, ni = (int(v) for v in got["counts"][:3])
        assert (na, top, ni) == (len(ref["accepted"]), ref["n_topped_up"], len(ref["inconsistent"])), tag
        assert np.array_equal(got["accepted"][:na], ref["accepted"]), tag
        assert np.array_equal(got["inconsistent"][:ni], ref["inconsistent"]), tag
        _untouched(got["accepted"][na:], tag)
        _untouched(got["inconsistent"][ni:], tag)
        _untouched(got["counts"][3:], tag)
        cand = got["status"][:n] == 1
        rejected = cand & ~(got["parallax_cos"][:n] <= got["required_cos"][:n])
        assert top == min(quota - (na - top), int(rejected.sum())) and top > 0, tag
        if name == "all_rejected_2049":
            assert int(rejected.sum()) > K6B_REJ_LDS
        if len(sc["track_uv"]) > 1:
            assert np.isnan(got["parallax_cos"][:n][rejected]).any(), tag


# ---------------------------------------------------------------------------------------------------------- finalize
SCHEDULE = ("termination", "iterations", "successful_steps", "usable")
TRACE_TOL = (("radius", 1e-7), ("cost", 1e-9), ("candidate_cost", 1e-8), ("model_cost_change", 1e-6), ("step_norm", 1e-4), ("x_norm", 1e-4))
_BA = {}


def _window(synth):
    if "w" not in _BA:
        _BA["w"] = synth.make_ba_window(n_kf=3, n_points=50, run_min=2, run_max=3, n_fixed=1, config_id=41)
    return _BA["w"]


def _options(mod, **kw):
    o = mod.default_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _ba_args(w):
    return w["cams"], w["cam_free"], w["points"], w["obs_ptr"], w["obs_cam"], w["obs_uv"], w["K"]


def _check_finalize(ctx, w, s, dc, dp, ref):
    """Summary, trace and the camera mirror against the oracle's (rc, rp, summary, trace) and against the device arrays."""
    rc, rp, rs_, otr = ref
    tr = ctx.ba_trace()
    assert tuple(s[k] for k in SCHEDULE) == tuple(rs_[k] for k in SCHEDULE)
    assert len(tr) == s["iterations"] == len(otr)
    assert [t["outcome"] for t in tr] == [t["outcome"] for t in otr]
    for k, tol in TRACE_TOL:
        assert np.allclose([t[k] for t in tr], [t[k] for t in otr], rtol=tol, atol=1e-9, equal_nan=True), k
    assert np.allclose([s["initial_cost"], s["final_cost"]], [rs_["initial_cost"], rs_["final_cost"]], rtol=1e-9, equal_nan=True)
    cams, pts = to_np(dc), to_np(dp)
    mirror = ctx.ba_cameras(np.full_like(w["cams"], -7.0))
    assert mirror.tobytes() == cams.tobytes()                                 # the pinned mirror IS the device array
    assert np.allclose(cams, rc, rtol=1e-7, atol=1e-9) and np.allclose(pts, rp, rtol=1e-6, atol=1e-7)
    fixed = np.asarray(w["cam_free"]) == 0
    assert cams[fixed].tobytes() == w["cams"][fixed].tobytes()
    if not s["usable"]:
        assert cams.tobytes() == w["cams"].tobytes() and pts.tobytes() == w["points"].tobytes()


@pytest.mark.parametrize("case", ["cap1", "default", "nan_pixel"])
def test_finalize_summary_trace_and_camera_mirror(ctx, rs, oracle, synth, case):
    """A window of 3 key frames and 50 landmarks: a solve that ends after a single iteration, the default solve (ten
    accepted steps), and one that ends unusable.  The trust-region loop never accepts a rising cost and an iteration cap
    of 0 is a usable solve in the oracle, so neither ends unusable; a non-finite pixel does (the cost at the start is not
    finite, the solve fails before its first step, cameras and points stay as they went in).  (With a cap of 0 no round
    runs at all and the library reports both costs as 0 where the oracle evaluates the cost once: that is the host
    driver's, not finalize's, and is not held against the oracle here.)"""
    w = dict(_window(synth))
    kw = {"cap1": dict(max_num_iterations=1)}.get(case, {})
    if case == "nan_pixel":
        w["obs_uv"] = w["obs_uv"].copy()
        w["obs_uv"][7, 0] = np.nan
    ref = oracle.bundle_adjust_trace(*_ba_args(w), options=_options(oracle, **kw))
    if case == "cap1":
        assert ref[2]["iterations"] == 1
    elif case == "nan_pixel":
        assert ref[2]["usable"] == 0
    else:
        assert ref[2]["usable"] == 1 and ref[2]["successful_steps"] >= 2
    for _ in range(2):                                     # twice: the second solve finds the first one's trace and state
        dc, dp = ctx.dev(w["cams"]), ctx.dev(w["points"])
        s = ctx.bundle_adjust(dc, w["cam_free"], dp, ctx.dev(w["obs_ptr"]), ctx.dev(w["obs_cam"]), ctx.dev(w["obs_uv"]), w["K"],
                              _options(rs, **kw))
        _check_finalize(ctx, w, s, dc, dp, ref)


@pytest.mark.parametrize("cap", [1, None])
def test_finalize_inertial(ctx, rs, oracle, synth, cap):
    """The inertial form of the same window: the mirror, the trace and the velocity / bias hand-back behind finalize."""
    w = _window(synth)
    m = synth.make_imu(w, pairs=[(1, 2)])
    kw = {} if cap is None else dict(max_num_iterations=cap)
    rc, rp, rv, rb, rs_, otr = oracle.bundle_adjust_inertial(*_ba_args(w), m, options=_options(oracle, **kw), trace=True)
    dc, dp = ctx.dev(w["cams"]), ctx.dev(w["points"])
    s, v, b = ctx.bundle_adjust_inertial(dc, w["cam_free"], dp, ctx.dev(w["obs_ptr"]), ctx.dev(w["obs_cam"]), ctx.dev(w["obs_uv"]), w["K"], m,
                                         _options(rs, **kw))
    _check_finalize(ctx, w, s, dc, dp, (rc, rp, rs_, otr))
    assert np.allclose(v, rv, rtol=1e-7, atol=1e-9) and np.allclose(b, rb, rtol=1e-6, atol=1e-9)
