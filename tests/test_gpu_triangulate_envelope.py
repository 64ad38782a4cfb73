"""K4 (two-view DLT and its compaction, through all five entry points), K6/K6b (per-track triangulation and the quota
selection), K12/K12b (point errors and the cull list) and K13/K14 (rigid point moves) across their envelope: the case
families, degenerate and non-finite rows, keep patterns, compaction sizes, device counts, batches, selection tables and
observation lists of tri_cases.py.

Every result is held against the oracle bit for bit (finite floats equal in every bit, non-finite ones non-finite in the
same places: NaN payload and sign differ between x86 and the GPU) and against the float64 referee tri_ref.py with the
bounds, bands and the 2 % cap of test_tri_cases_cpu.py.  Outputs are prefilled with a sentinel and allocated with spare
rows: nothing may be written at or past n in the per-item arrays, nor at or past the count in the compacted ones."""
import numpy as np
import pytest

import tri_cases as C
import tri_ref as R
from conftest import to_np

pytestmark = pytest.mark.gpu

PAD = 16
SENT_I, SENT_B = -0x01234567, 0xA5
BAND_CAP = 0.02


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


def _k4_out(ctx, rows, counts=1):
    t = ctx.torch
    return dict(xyz=_sentinel(ctx, (rows + PAD, 3), t.float32), keep=_sentinel(ctx, (rows + PAD,), t.uint8),
                out_index=_sentinel(ctx, (rows + PAD,), t.int32), out_xyz=_sentinel(ctx, (rows + PAD, 3), t.float32),
                count=_sentinel(ctx, (counts + PAD,), t.int32))


def _check_k4(got, ref, rows, tag="", base=0, count_at=0, checked_to=None):
    """got: the numpy copies of a _k4_out; ref: the oracle over the `m` rows the call had to compute; the pair's slice
    starts at row `base` and is `rows` long: rows m .. rows of it must be untouched, the compacted ones from the count on."""
    m = len(ref["keep"])
    sl = slice(base, base + m)
    _same_floats(got["xyz"][sl], ref["xyz"], tag)
    assert np.array_equal(got["keep"][sl], ref["keep"]), tag
    end = base + rows if checked_to is None else checked_to
    _untouched(got["xyz"][base + m:end], tag)
    _untouched(got["keep"][base + m:end], tag)
    k = len(ref["out_index"])
    assert int(got["count"][count_at]) == k, tag
    assert np.array_equal(got["out_index"][base:base + k], ref["out_index"]), tag
    _same_floats(got["out_xyz"][base:base + k], ref["out_xyz"], tag)
    _untouched(got["out_index"][base + k:end], tag)
    _untouched(got["out_xyz"][base + k:end], tag)


def _np(out):
    return {k: to_np(v) for k, v in out.items()}


def _against_referee(xyz, keep, r, gates, tag):
    ok = r["finite"]
    assert (np.abs(xyz[ok].astype(np.float64) - r["X"][ok]) <= r["bX"][ok]).all(), tag
    want, decided = R.gates(r, *gates)
    assert 1.0 - decided.mean() <= BAND_CAP, tag
    assert np.array_equal(want[decided], keep[decided] != 0), tag


# ------------------------------------------------------------------------------------------ K4: the five entry points
_REF = {}


def _family(oracle, name, gates):
    key = (name, gates)
    if key not in _REF:
        f = C.pair_family(name)
        _REF[key] = (f, oracle.triangulate(f["uv1"], f["uv2"], f["poses"], C.K, min_parallax_cosine=gates[0], max_reproj=gates[1]),
                     R.two_view(f["uv1"], f["uv2"], f["poses"][0], f["poses"][1], C.K))
    return _REF[key]


def _shuffled(uv1, uv2, seed):
    """Keypoint arrays in shuffled order and the gather lists that put the correspondences back."""
    rng = np.random.default_rng(seed)
    p1, p2 = rng.permutation(len(uv1)), rng.permutation(len(uv2))
    return uv1[p1], uv2[p2], np.argsort(p1).astype(np.int32), np.argsort(p2).astype(np.int32)


@pytest.mark.parametrize("gates", C.GATES, ids=["strict", "loose"])
@pytest.mark.parametrize("name", list(C.PAIR_FAMILIES))
def test_k4_families_through_every_entry_point(ctx, oracle, name, gates):
    f, ref, r = _family(oracle, name, gates)
    n = len(f["uv1"])
    kw = dict(min_parallax_cosine=gates[0], max_reproj=gates[1])
    d_poses = ctx.dev(f["poses"])
    # rs_triangulate, without and with per-item pose indices
    got = _np(ctx.triangulate(ctx.dev(f["uv1"]), ctx.dev(f["uv2"]), n, d_poses, 2, C.K, out=_k4_out(ctx, n), **kw))
    _check_k4(got, ref, n + PAD, name + " rs_triangulate")
    _against_referee(got["xyz"][:n], got["keep"][:n], r, gates, name)
    poses4 = np.concatenate([f["poses"][::-1], f["poses"]])
    got = _np(ctx.triangulate(ctx.dev(f["uv1"]), ctx.dev(f["uv2"]), n, ctx.dev(poses4), 4, C.K, d_idx1=ctx.dev(np.full(n, 2, np.int32)),
                              d_idx2=ctx.dev(np.where(np.arange(n) % 2, 3, 0).astype(np.int32)), out=_k4_out(ctx, n), **kw))
    _check_k4(got, ref, n + PAD, name + " rs_triangulate, pose indices")
    # rs_triangulate_matches and the batch form with one pair: shuffled keypoints, gathered back
    kp1, kp2, g1, g2 = _shuffled(f["uv1"], f["uv2"], 5)
    cnt = ctx.dev(np.array([n], np.int32))
    got = _np(ctx.triangulate_matches(ctx.dev(kp1), ctx.dev(kp2), ctx.dev(g1), ctx.dev(g2), cnt, n, d_poses, C.K, out=_k4_out(ctx, n), **kw))
    _check_k4(got, ref, n + PAD, name + " rs_triangulate_matches")
    got = _np(ctx.triangulate_matches_batch(ctx.dev(kp1[None]), ctx.dev(kp2[None]), ctx.dev(g1[None]), ctx.dev(g2[None]), cnt, ctx.dev(f["poses"][None]),
                                            C.K, out=_k4_out(ctx, n), **kw))
    _check_k4(got, ref, n + PAD, name + " rs_triangulate_matches_batch")
    # rs_triangulate_host: the grid kernels above 256, one workgroup up to it
    idx, xyz = ctx.triangulate_host(f["uv1"], f["uv2"], f["poses"][0], f["poses"][1], C.K, **kw)
    assert np.array_equal(idx, ref["out_index"])
    _same_floats(xyz, ref["out_xyz"], name + " rs_triangulate_host")
    small = oracle.triangulate(f["uv1"][:200], f["uv2"][:200], f["poses"], C.K, **kw)
    idx, xyz = ctx.triangulate_host(f["uv1"][:200], f["uv2"][:200], f["poses"][0], f["poses"][1], C.K, **kw)
    assert np.array_equal(idx, small["out_index"])
    _same_floats(xyz, small["out_xyz"], name + " rs_triangulate_host, one workgroup")


@pytest.mark.parametrize("gates", C.GATES, ids=["strict", "loose"])
def test_k4_degenerate_and_non_finite_rows(ctx, oracle, gates):
    e = C.edge_rows()
    n = len(e["uv1"])
    kw = dict(min_parallax_cosine=gates[0], max_reproj=gates[1])
    ref = oracle.triangulate(e["uv1"], e["uv2"], e["poses"], C.K, idx1=e["idx1"], idx2=e["idx2"], **kw)
    got = _np(ctx.triangulate(ctx.dev(e["uv1"]), ctx.dev(e["uv2"]), n, ctx.dev(e["poses"]), len(e["poses"]), C.K, d_idx1=ctx.dev(e["idx1"]),
                              d_idx2=ctx.dev(e["idx2"]), out=_k4_out(ctx, n), **kw))
    _check_k4(got, ref, n + PAD, "edge rows")
    assert (~np.isfinite(ref["xyz"])).any() and ref["keep"][np.isnan(ref["xyz"]).any(1)].all()
    # the rows of the first pose pair also through the one-workgroup host form (NaN rows kept, in order)
    rows = np.flatnonzero((e["idx1"] == 0) & (e["idx2"] == 1))
    two = oracle.triangulate(e["uv1"][rows], e["uv2"][rows], e["poses"][:2], C.K, **kw)
    idx, xyz = ctx.triangulate_host(e["uv1"][rows], e["uv2"][rows], e["poses"][0], e["poses"][1], C.K, **kw)
    assert np.array_equal(idx, two["out_index"])
    _same_floats(xyz, two["out_xyz"], "edge rows, host form")


@pytest.mark.parametrize("n", C.COMPACTION_SIZES)
def test_k4_compaction_patterns_and_sizes(ctx, oracle, n):
    for pattern in C.KEEP_PATTERNS:
        c = C.compaction_case(pattern, n)
        ref = oracle.triangulate(c["uv1"], c["uv2"], c["poses"], C.K)
        assert np.array_equal(ref["keep"] != 0, c["keep"]), pattern
        got = _np(ctx.triangulate(ctx.dev(c["uv1"]), ctx.dev(c["uv2"]), n, ctx.dev(c["poses"]), 2, C.K, out=_k4_out(ctx, n)))
        _check_k4(got, ref, n + PAD, "%s %d" % (pattern, n))


@pytest.mark.parametrize("n", [2, 65, 1025, 2049])
def test_k4_device_count(ctx, oracle, n):
    """*d_n at 0, 1, n - 1, n, n + 1 and 10 n: rows from the count on stay as they were, in all four outputs."""
    c = C.compaction_case("random50", n)
    kp1, kp2, g1, g2 = _shuffled(c["uv1"], c["uv2"], n)
    d = [ctx.dev(a) for a in (kp1, kp2, g1, g2)]
    d_poses = ctx.dev(c["poses"])
    for count in (0, 1, n - 1, n, n + 1, 10 * n):
        m = min(count, n)
        ref = oracle.triangulate(c["uv1"][:m], c["uv2"][:m], c["poses"], C.K)
        got = _np(ctx.triangulate_matches(d[0], d[1], d[2], d[3], ctx.dev(np.array([count], np.int32)), n, d_poses, C.K, out=_k4_out(ctx, n)))
        _check_k4(got, ref, n + PAD, "count %d of %d" % (count, n))


@pytest.mark.parametrize("batch,stride", [(1, 1), (1, 1025), (3, 63), (3, 64), (3, 65), (3, 1025), (65, 1), (65, 65)])
def test_k4_batch_against_the_single_pair_call(ctx, oracle, batch, stride):
    """n1 != n2; per-pair counts of 0, the stride, above it and in between in one call; gather lists that are permutations
    (even pairs) or hold repeats (odd pairs).  Each pair equals the oracle and rs_triangulate_matches on its slice."""
    rng = np.random.default_rng([batch, stride])
    n1, n2 = stride + 3, stride + 7
    counts = np.array([(0, stride, stride + 5, 1, max(stride - 1, 0), 10 * stride)[b % 6] for b in range(batch)], np.int32)
    if batch == 1:
        counts[0] = stride
    kp1, kp2, mt, mq, poses = [], [], [], [], []
    for b in range(batch):
        f = C._pair(7000 + b, n2, 40.0 + b, 1.0 + (b % 5), 0.0, (3.0, 12.0), 0.5, 0.2)
        p2 = rng.permutation(n2)
        kp1.append(f["uv1"][:n1])
        kp2.append(f["uv2"][p2])
        pick = rng.permutation(n1)[:stride] if b % 2 == 0 else rng.integers(0, n1, stride)
        mt.append(pick.astype(np.int32))
        mq.append(np.argsort(p2)[pick].astype(np.int32))
        poses.append(f["poses"])
    kp1, kp2, mt, mq, poses = (np.ascontiguousarray(np.stack(a)) for a in (kp1, kp2, mt, mq, poses))
    out = _k4_out(ctx, batch * stride, counts=batch)
    got = _np(ctx.triangulate_matches_batch(ctx.dev(kp1), ctx.dev(kp2), ctx.dev(mt), ctx.dev(mq), ctx.dev(counts), ctx.dev(poses), C.K, out=out))
    for b in range(batch):
        m = min(int(counts[b]), stride)
        ref = oracle.triangulate(kp1[b][mt[b][:m]], kp2[b][mq[b][:m]], poses[b], C.K)
        _check_k4(got, ref, stride, "pair %d of %d, stride %d" % (b, batch, stride), base=b * stride, count_at=b)
        if b < 6:
            one = _np(ctx.triangulate_matches(ctx.dev(kp1[b]), ctx.dev(kp2[b]), ctx.dev(mt[b]), ctx.dev(mq[b]), ctx.dev(counts[b:b + 1]), stride,
                                              ctx.dev(poses[b]), C.K, out=_k4_out(ctx, stride)))
            _check_k4(one, ref, stride + PAD, "single pair %d" % b)
    for k in ("xyz", "keep", "out_index", "out_xyz"):
        _untouched(got[k][batch * stride:], k)
    _untouched(got["count"][batch:], "count")
    if batch >= 3 and stride > 1:
        assert got["count"][:batch].max() > 0 and got["count"][0] == 0


def test_k4_host_form_call_sequence(ctx, oracle):
    """256, 3, 1, 257 and 2 correspondences on one context: a row of the pinned block or a ticket left over from the call
    before would show.  Then all kept and none kept at 1 and at 256."""
    f = C.pair_family("axis30_turn1_near")
    for n in (256, 3, 1, 257, 2):
        lo = 300 - n
        ref = oracle.triangulate(f["uv1"][lo:lo + n], f["uv2"][lo:lo + n], f["poses"], C.K)
        idx, xyz = ctx.triangulate_host(f["uv1"][lo:lo + n], f["uv2"][lo:lo + n], f["poses"][0], f["poses"][1], C.K)
        assert np.array_equal(idx, ref["out_index"]), n
        _same_floats(xyz, ref["out_xyz"], "host form, n = %d" % n)
    for n in (1, 256):
        for pattern in ("all", "none", "all"):
            c = C.compaction_case(pattern, n)
            ref = oracle.triangulate(c["uv1"], c["uv2"], c["poses"], C.K)
            idx, xyz = ctx.triangulate_host(c["uv1"], c["uv2"], c["poses"][0], c["poses"][1], C.K)
            assert len(idx) == (n if pattern == "all" else 0) and np.array_equal(idx, ref["out_index"])
            _same_floats(xyz, ref["out_xyz"], "host form, %s of %d" % (pattern, n))


# ---------------------------------------------------------------------------------------------------- K6 and K6b
def _nonempty(a, shape, dtype):
    """A CSR payload without entries still needs an address."""
    return a if len(a) else np.zeros(shape, dtype)


def _run_tracks(ctx, rs, sc, quota):
    t = ctx.torch
    n = len(sc["track_uv"])
    out = dict(status=_sentinel(ctx, (n + PAD,), t.uint8), xyz=_sentinel(ctx, (n + PAD, 3), t.float32),
               parallax_cos=_sentinel(ctx, (n + PAD,), t.float32), required_cos=_sentinel(ctx, (n + PAD,), t.float32),
               accepted=_sentinel(ctx, (n + PAD,), t.int32), inconsistent=_sentinel(ctx, (n + PAD,), t.int32), counts=_sentinel(ctx, (3 + PAD,), t.int32))
    req = rs.parallax_requirements(sc["poses"], sc["kf_pose"])
    return _np(ctx.triangulate_tracks(ctx.dev(sc["track_uv"]), ctx.dev(sc["sight_ptr"]), ctx.dev(_nonempty(sc["sight_pose"], (1,), np.int32)),
                                      ctx.dev(_nonempty(sc["sight_uv"], (1, 2), np.float32)), ctx.dev(sc["poses"]), sc["kf_pose"], C.K,
                                      d_skip=ctx.dev(sc["skip"]), min_new_points=quota, d_required=ctx.dev(req), out=out))


@pytest.mark.parametrize("name", list(C.selection_tables()))
def test_k6_selection_tables(ctx, rs, oracle, name):
    sc = C.selection_scene(name)
    quota = sc["quota"]
    n = len(sc["track_uv"])
    ref = oracle.triangulate_tracks(sc["track_uv"], sc["sight_ptr"], sc["sight_pose"], sc["sight_uv"], sc["poses"], sc["kf_pose"], C.K,
                                    skip=sc["skip"], min_new_points=quota)
    got = _run_tracks(ctx, rs, sc, quota)
    assert np.array_equal(got["status"][:n], ref["status"])
    _same_floats(got["xyz"][:n], ref["xyz"], name)
    _same_floats(got["parallax_cos"][:n], ref["parallax_cos"], name)
    assert np.array_equal(bits(got["required_cos"][:n]), bits(ref["required_cos"]))
    na, top, ni = (int(v) for v in got["counts"][:3])
    assert (na, top, ni) == (len(ref["accepted"]), ref["n_topped_up"], len(ref["inconsistent"]))
    assert np.array_equal(got["accepted"][:na], ref["accepted"]) and np.array_equal(got["inconsistent"][:ni], ref["inconsistent"])
    # the specification, on the kernel's own per-track values
    acc, stop, inc = R.select(got["status"][:n], got["parallax_cos"][:n], got["required_cos"][:n], quota)
    assert np.array_equal(got["accepted"][:na], acc) and top == stop and np.array_equal(got["inconsistent"][:ni], inc)
    for k in ("status", "xyz", "parallax_cos", "required_cos"):
        _untouched(got[k][n:], k)
    _untouched(got["accepted"][na:], "accepted")
    _untouched(got["inconsistent"][ni:], "inconsistent")
    _untouched(got["counts"][3:], "counts")
    # the referee: statuses outside the band, the point and the cosine within their bounds
    r = R.track_body(sc["track_uv"], sc["skip"], sc["sight_ptr"], sc["sight_pose"], sc["sight_uv"], sc["poses"], sc["kf_pose"], C.K)
    d = r["decided"]
    assert 1.0 - d.mean() <= BAND_CAP and np.array_equal(r["status"][d], got["status"][:n][d])
    c = (got["status"][:n] == 1) & r["finite"]
    assert (np.abs(got["xyz"][:n][c] - r["X"][c]) <= r["bX"][c]).all()
    assert (np.abs(got["parallax_cos"][:n][c] - r["parallax_cos"][c]) <= r["b_parallax"][c]).all()
    # two runs give the same bytes
    again = _run_tracks(ctx, rs, sc, quota)
    for k in got:
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(again[k]).view(np.uint8)), k


# -------------------------------------------------------------------------------------------------------------- K12
def _run_errors(ctx, sc):
    t = ctx.torch
    n = len(sc["positions"])
    out = dict(mean_err=_sentinel(ctx, (n + PAD,), t.float32), cull=_sentinel(ctx, (n + PAD,), t.uint8), cull_idx=_sentinel(ctx, (n + PAD,), t.int32),
               cull_count=_sentinel(ctx, (1 + PAD,), t.int32), sums=ctx.torch.zeros((2,), dtype=t.float64, device=ctx.device))
    return _np(ctx.point_errors(ctx.dev(sc["positions"]), ctx.dev(sc["obs_ptr"]), ctx.dev(sc["obs_pose"]), ctx.dev(sc["obs_uv"]), ctx.dev(sc["poses"]),
                                C.K, out=out))


def _check_errors(got, ref, n, tag="", sums=True):
    _same_floats(got["mean_err"][:n], ref["mean_err"], tag)
    assert np.array_equal(got["cull"][:n], ref["cull"]), tag
    k = int(got["cull_count"][0])
    assert k == len(ref["cull_idx"]) and np.array_equal(got["cull_idx"][:k], ref["cull_idx"]), tag
    _untouched(got["mean_err"][n:], tag)
    _untouched(got["cull"][n:], tag)
    _untouched(got["cull_idx"][k:], tag)
    _untouched(got["cull_count"][1:], tag)
    if sums:
        assert got["sums"][1] == float(ref["n_obs"]), tag
        assert abs(got["sums"][0] - ref["err_sum"]) <= 1e-12 * max(abs(ref["err_sum"]), 1.0), tag


def test_k12_observation_lists_and_block_edges(ctx, oracle):
    sc = C.k12_scene()
    n = len(sc["positions"])
    ref = oracle.point_errors(sc["positions"], sc["obs_ptr"], sc["obs_pose"], sc["obs_uv"], sc["poses"], C.K)
    got = _run_errors(ctx, sc)
    _check_errors(got, ref, n)
    r = R.point_errors(sc["positions"], sc["obs_ptr"], sc["obs_pose"], sc["obs_uv"], sc["poses"], C.K)
    assert (np.abs(got["mean_err"][:n] - r["mean"]) <= r["b_mean"]).all()
    d = r["decided"]
    assert 1.0 - d.mean() <= BAND_CAP and np.array_equal(r["cull"][d], got["cull"][:n][d] != 0)


def test_k12_threshold_on_exact_values_and_the_camera_plane(ctx, oracle):
    sc = C.k12_exact()
    n = len(sc["positions"])
    got = _run_errors(ctx, sc)
    _check_errors(got, oracle.point_errors(sc["positions"], sc["obs_ptr"], sc["obs_pose"], sc["obs_uv"], sc["poses"], C.K), n)
    assert np.array_equal(got["cull"][:n], sc["expect"])
    known = ~np.isnan(sc["mean"])
    assert np.array_equal(got["mean_err"][:n][known].astype(np.float64), sc["mean"][known])
    sc = C.k12_plane()
    n = len(sc["positions"])
    got = _run_errors(ctx, sc)
    _check_errors(got, oracle.point_errors(sc["positions"], sc["obs_ptr"], sc["obs_pose"], sc["obs_uv"], sc["poses"], C.K), n, sums=False)
    assert list(got["cull"][:n]) == [1, 0, 0, 1, 0] and got["sums"][1] == 5.0 and np.isnan(got["sums"][0])


@pytest.mark.parametrize("n", C.CULL_SIZES)
def test_k12_cull_list_patterns_and_sizes(ctx, oracle, n):
    for pattern in C.KEEP_PATTERNS:
        sc = C.k12_cull_case(pattern, n)
        ref = oracle.point_errors(sc["positions"], sc["obs_ptr"], sc["obs_pose"], sc["obs_uv"], sc["poses"], C.K)
        got = _run_errors(ctx, sc)
        _check_errors(got, ref, n, "%s %d" % (pattern, n))
        assert np.array_equal(got["cull"][:n] != 0, sc["cull"]) and got["sums"][0] == 10.0 * sc["cull"].sum()


# ---------------------------------------------------------------------------------------------------- K13 and K14
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("n_frames", [1, 32, 33])
def test_k13_forms(ctx, oracle, n_frames, n, permuted):
    """rs_reanchor_points and rs_reanchor_points_host_poses (the argument block up to 32 frames, the workspace above)."""
    c = C.k13_case(n_frames, n, permuted)
    ref = C.oracle_reanchor(oracle, c)
    d_idx = None if c["point_idx"] is None else ctx.dev(c["point_idx"])
    d_f = ctx.dev(c["frame_idx"])
    rows = len(c["positions"])

    def positions():
        p = _sentinel(ctx, (rows + PAD, 3), ctx.torch.float32)
        p[:rows] = ctx.dev(c["positions"])
        return p

    a = positions()
    ctx.reanchor_points(d_idx, d_f, ctx.dev(c["before"]), ctx.dev(c["after"]), a)
    b = positions()
    ctx.reanchor_points_host_poses(d_idx, d_f, c["before"], c["after"], b)
    a, b = to_np(a), to_np(b)
    for got in (a, b):
        assert np.array_equal(bits(got[:rows]), bits(ref))
        _untouched(got[rows:])
    want, bound = R.reanchor_points(c["point_idx"], c["frame_idx"], c["before"], c["after"], c["positions"])
    assert (np.abs(a[:rows] - want) <= bound).all()
    stays = ~bound.any(1)
    assert stays.any() and np.array_equal(bits(a[:rows][stays]), bits(c["positions"][stays]))


@pytest.mark.parametrize("n_kf", [7, 5, 1])
def test_k14_owners(ctx, oracle, n_kf):
    """n_kf = 7: every owner exists, bit for bit against the oracle.  n_kf = 5 and 1: points owned by a key frame at or past
    n_kf stay (the oracle has no n_kf; the rule is the referee's and the bytes of those points)."""
    c = C.k14_case()
    n = len(c["positions"])
    p = _sentinel(ctx, (n + PAD, 3), ctx.torch.float32)
    p[:n] = ctx.dev(c["positions"])
    # (the binding takes the number of points from the position rows it is handed: the first n, not the spare ones)
    ctx.transform_points(ctx.dev(c["obs_ptr"]), ctx.dev(c["obs_kf"]), ctx.dev(c["before"][:n_kf]), ctx.dev(c["after"][:n_kf]), p[:n])
    got = to_np(p)
    _untouched(got[n:])
    want, bound, owner = R.transform_points(c["obs_ptr"], c["obs_kf"], c["before"], c["after"], c["positions"], n_kf=n_kf)
    moves = (owner >= 0) & (owner < n_kf)
    assert np.array_equal(moves, bound.any(1)) and moves.any() and (~moves).any()
    assert (np.abs(got[:n] - want) <= bound).all()
    assert np.array_equal(bits(got[:n][~moves]), bits(c["positions"][~moves]))
    ref = oracle.transform_points(c["obs_ptr"], c["obs_kf"], c["before"], c["after"], c["positions"])
    assert np.array_equal(bits(got[:n][moves]), bits(ref[moves]))
    if n_kf < 7:
        assert (owner >= n_kf).any()
