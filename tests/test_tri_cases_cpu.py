"""The oracle's triangulation, track body, selection, cull rule and rigid moves held against the float64 referee
(tri_ref.py) on every case family of tri_cases.py.  Runs without a GPU.

Positions must lie within the referee's bound; a gate decision, a status or a cull flag must equal the referee's
wherever the referee's quantity lies outside its derived band; the share of cases inside a band is capped at 2 % per
family and gate pair (a condition on the case builders: tri_cases.py chooses depths and baselines to meet it).  The
selection is held against its specification (tri_ref.select) on every table, NaN cosines included.

Before oracle/tracks.c sorted by the kernel's total order, the NaN tables failed here: with synth.make_tracks(n_tracks=64,
far_frac=1.0, outlier_frac=0, config_id=7), quota 5 and track_uv[0, 0] = NaN the oracle accepted [0 55 31 51 16] (its
insertion sort on `>` left the NaN track where it stood), the specification and k6_select give [55 31 51 16 44]."""
import numpy as np
import pytest

import tri_cases as C
import tri_ref as R

BAND_CAP = 0.02


# ------------------------------------------------------------------------------------------------------- two views
_PAIRS = {}


def _pair_ref(name):
    if name not in _PAIRS:
        f = C.pair_family(name)
        _PAIRS[name] = (f, R.two_view(f["uv1"], f["uv2"], f["poses"][0], f["poses"][1], C.K))
    return _PAIRS[name]


@pytest.mark.parametrize("name", list(C.PAIR_FAMILIES))
def test_positions_within_the_bound(oracle, name):
    f, r = _pair_ref(name)
    o = oracle.triangulate(f["uv1"], f["uv2"], f["poses"], C.K)
    d = np.abs(o["xyz"].astype(np.float64) - r["X"])
    lead = (d.max(1) / np.abs(r["X"]).max(1)).max() / R.U
    print(name, "max |oracle - referee| / bound", (d / r["bX"]).max(), "; in units of 2^-24 of the largest component", lead,
          "; smallest relative gap", r["gap"].min())
    assert r["finite"].all() and (d <= r["bX"]).all()
    # the issue's probe figure (2.3 * 2^-24 of the largest component over its four families; 2.31 here); three roundings allow 3
    assert lead <= 3.0
    assert r["gap"].min() > 5e-7


@pytest.mark.parametrize("gates", C.GATES, ids=["strict", "loose"])
@pytest.mark.parametrize("name", list(C.PAIR_FAMILIES))
def test_gate_decisions_outside_the_band_and_the_band_share(oracle, name, gates):
    f, r = _pair_ref(name)
    o = oracle.triangulate(f["uv1"], f["uv2"], f["poses"], C.K, min_parallax_cosine=gates[0], max_reproj=gates[1])
    keep, decided = R.gates(r, *gates)
    share = 1.0 - decided.mean()
    print(name, gates, "kept", int(o["keep"].sum()), "of", len(keep), "band share", share)
    assert share <= BAND_CAP
    assert np.array_equal(keep[decided], o["keep"][decided] != 0)
    assert np.array_equal(o["out_index"], np.flatnonzero(o["keep"])) and np.array_equal(o["out_xyz"], o["xyz"][o["keep"] != 0])
    if f["outlier"].any():
        assert not o["keep"][f["outlier"]].all()


def test_loose_gate_loses_far_points_to_f32_rounding(oracle):
    """Finding 2 of the issue, as its record: at 60 .. 400 m over a 0.3 m baseline the f32 cosine rounds above 1.0 for points a
    float64 evaluation keeps.  Every such point lies inside the referee's band; the behaviour restates the reference and stays."""
    f = C._pair(60400, 2000, 30.0, 1.0, 0.0, (60.0, 400.0), 0.5, 0.0)
    r = R.two_view(f["uv1"], f["uv2"], f["poses"][0], f["poses"][1], C.K)
    o = oracle.triangulate(f["uv1"], f["uv2"], f["poses"], C.K, min_parallax_cosine=1.0, max_reproj=4.0)
    keep, decided = R.gates(r, 1.0, 4.0)
    lost = keep & (o["keep"] == 0)
    print("lost", int(lost.sum()), "of 2000; farthest from the threshold", (1.0 - r["cos"][lost]).max() if lost.any() else None,
          "band", R.gamma(10), "band share", 1.0 - decided.mean())
    assert lost.any() and not decided[lost].any()
    assert ((1.0 - r["cos"][lost]) <= R.gamma(10) * 1.01).all()
    assert np.array_equal(keep[decided], o["keep"][decided] != 0)


def test_degenerate_and_non_finite_rows(oracle):
    e = C.edge_rows()
    P = e["poses"]
    r = R.two_view(e["uv1"], e["uv2"], P[e["idx1"]], P[e["idx2"]], C.K)
    names = np.array(e["names"])
    for gates in C.GATES:
        o = oracle.triangulate(e["uv1"], e["uv2"], P, C.K, idx1=e["idx1"], idx2=e["idx2"], min_parallax_cosine=gates[0], max_reproj=gates[1])
        keep, decided = R.gates(r, *gates)
        sure = decided & (r["gap"] > 1e-6)
        assert np.array_equal(keep[sure], o["keep"][sure] != 0)
        assert (o["keep"][names == "ordinary"] == 1).all() and (o["keep"][names == "swapped_views"] == 0).all()
        assert sure[names == "ordinary"].all() and sure[names == "swapped_views"].all() and sure[names == "principal_point"].all()
        ok = r["gap"] > 1e-6
        assert (np.abs(o["xyz"][ok] - r["X"][ok]) <= r["bX"][ok]).all()
        # pinned, as the reference computes them: a NaN point fails every comparison and is kept; so is the point at a shared centre
        nan = np.isnan(o["xyz"]).any(1)
        assert nan.any() and (o["keep"][nan] == 1).all()
        i = int(np.flatnonzero(names == "identity_pose_pair")[0])
        assert o["keep"][i] == 1 and not o["xyz"][i].any()
        assert not r["finite"][names == "nonfinite_view1"].any() and not r["finite"][names == "nonfinite_view2"].any()


@pytest.mark.parametrize("n", C.COMPACTION_SIZES)
def test_keep_patterns_are_exact_under_the_oracle(oracle, n):
    for pattern in C.KEEP_PATTERNS:
        c = C.compaction_case(pattern, n)
        o = oracle.triangulate(c["uv1"], c["uv2"], c["poses"], C.K)
        assert np.array_equal(o["keep"] != 0, c["keep"]), pattern
        assert np.array_equal(o["out_index"], np.flatnonzero(c["keep"])), pattern


# ---------------------------------------------------------------------------------------------------------- tracks
def _oracle_tracks(oracle, sc, quota):
    return oracle.triangulate_tracks(sc["track_uv"], sc["sight_ptr"], sc["sight_pose"], sc["sight_uv"], sc["poses"], sc["kf_pose"], C.K,
                                     skip=sc["skip"], min_new_points=quota)


def _same_selection(o, quota, tag=""):
    acc, top, inc = R.select(o["status"], o["parallax_cos"], o["required_cos"], quota)
    assert np.array_equal(o["accepted"], acc), (tag, o["accepted"][:12], acc[:12])
    assert o["n_topped_up"] == top and np.array_equal(o["inconsistent"], inc), tag
    return acc, top


@pytest.mark.parametrize("name", list(C.selection_tables()))
def test_selection_tables(oracle, name):
    sc = C.selection_scene(name)
    kinds = np.array(list(sc["kinds"]))
    o = _oracle_tracks(oracle, sc, sc["quota"])
    acc, top = _same_selection(o, sc["quota"], name)
    # the table is what its name says: every track falls where it was built to fall
    meets = o["parallax_cos"] <= o["required_cos"]
    want = {"A": (1, True), "R": (1, False), "N": (1, False), "I": (2, None), "S": (0, None), "E": (0, None)}
    for k, (st, m) in want.items():
        sel = kinds == k
        assert (o["status"][sel] == st).all(), k
        if m is not None:
            assert (meets[sel] == m).all(), k
    assert np.isnan(o["parallax_cos"][kinds == "N"]).all() and np.isnan(o["xyz"][kinds == "N"]).all()
    na, nr = int(((kinds == "A")).sum()), int(((kinds == "R") | (kinds == "N")).sum())
    assert top == min(max(sc["quota"] - na, 0), nr) and len(acc) == na + top
    # against the referee: statuses where decided, the point, the cosine and the requirement within their bounds
    r = R.track_body(sc["track_uv"], sc["skip"], sc["sight_ptr"], sc["sight_pose"], sc["sight_uv"], sc["poses"], sc["kf_pose"], C.K)
    d = r["decided"]
    print(name, "tracks", len(kinds), "accepted", na, "topped up", top, "band share", 1.0 - d.mean())
    assert 1.0 - d.mean() <= BAND_CAP
    assert np.array_equal(r["status"][d], o["status"][d])
    c = (o["status"] == 1) & r["finite"]
    assert (np.abs(o["xyz"][c] - r["X"][c]) <= r["bX"][c]).all()
    assert (np.abs(o["parallax_cos"][c] - r["parallax_cos"][c]) <= r["b_parallax"][c]).all()
    assert (np.abs(o["required_cos"][c] - r["required_cos"][c]) <= r["b_required"][c]).all()
    with np.errstate(invalid="ignore"):
        clear = c & (np.abs(r["parallax_cos"] - r["required_cos"]) > r["b_parallax"] + r["b_required"])
    assert np.array_equal(meets[clear], (r["parallax_cos"] <= r["required_cos"])[clear])
    assert clear.sum() >= 0.98 * c.sum()


def test_equal_cosines_keep_track_order(oracle):
    sc = C.selection_scene("equal_runs_2049_q2049")
    o = _oracle_tracks(oracle, sc, 2049)
    pc = o["parallax_cos"].view(np.uint32)
    assert pc[9] == pc[10] == pc[11] and pc[14] == pc[15] and len({int(pc[t]) for t in range(300, 305)}) == 1
    order = list(o["accepted"])
    # the copies are the smallest cosines of the table and stand in track order
    assert sorted(order[:10]) == [9, 10, 11, 14, 15, 300, 301, 302, 303, 304]
    for run in ((9, 10, 11), (14, 15), (300, 301, 302, 303, 304)):
        at = [order.index(t) for t in run]
        assert at == list(range(at[0], at[0] + len(run)))


def test_nan_cosine_sorts_after_every_number(oracle, synth):
    """Finding 1 of the issue, on its own input."""
    tk = synth.make_tracks(n_tracks=64, far_frac=1.0, outlier_frac=0, config_id=7)
    uv = tk["track_uv"].copy()
    uv[0, 0] = np.nan
    o = oracle.triangulate_tracks(uv, tk["sight_ptr"], tk["sight_pose"], tk["sight_uv"], tk["poses"], tk["kf_pose"], tk["K"], skip=tk["skip"],
                                  min_new_points=5)
    assert o["status"][0] == 1 and np.isnan(o["parallax_cos"][0])
    print("accepted", o["accepted"])
    _same_selection(o, 5)
    assert 0 not in o["accepted"]


def test_select_specification_on_hand_made_keys():
    nan = np.float32(np.nan)
    st = np.array([1, 1, 2, 1, 0, 1, 1, 1], np.uint8)
    pc = np.array([0.5, nan, 0.1, 0.5, 0.0, -0.0, 0.0, nan], np.float32)
    rc = np.array([0.4, 0.4, 0.4, 0.4, 0.4, -1.0, -1.0, 0.4], np.float32)
    acc, top, inc = R.select(st, pc, rc, 10)
    assert list(acc) == [5, 6, 0, 3, 1, 7] and top == 6 and list(inc) == [2]
    assert list(R.select(st, pc, rc, 3)[0]) == [5, 6, 0] and list(R.select(st, pc, rc, 0)[0]) == []


# ------------------------------------------------------------------------------------------------------------- K12
def _oracle_errors(oracle, sc):
    return oracle.point_errors(sc["positions"], sc["obs_ptr"], sc["obs_pose"], sc["obs_uv"], sc["poses"], C.K)


def test_point_errors_against_the_referee(oracle):
    sc = C.k12_scene()
    o = _oracle_errors(oracle, sc)
    r = R.point_errors(sc["positions"], sc["obs_ptr"], sc["obs_pose"], sc["obs_uv"], sc["poses"], C.K)
    cnt = np.diff(sc["obs_ptr"])
    print("culled", int(o["cull"].sum()), "of", len(cnt), "band share", 1.0 - r["decided"].mean(), "max err / bound",
          np.nanmax(np.abs(o["mean_err"] - r["mean"])[cnt > 0] / r["b_mean"][cnt > 0]))
    assert set(cnt.tolist()) >= {0, 1, 2, 17, 128} and (cnt[[255, 256, 257]] == 0).all()
    assert (np.abs(o["mean_err"] - r["mean"]) <= r["b_mean"]).all()
    assert 1.0 - r["decided"].mean() <= BAND_CAP
    assert np.array_equal(r["cull"][r["decided"]], o["cull"][r["decided"]] != 0)
    assert 0.1 < o["cull"].mean() < 0.9 and (o["cull"][cnt == 0] == 0).all() and (o["mean_err"][cnt == 0] == 0).all()
    assert np.array_equal(o["cull_idx"], np.flatnonzero(o["cull"])) and o["n_obs"] == cnt.sum()
    assert (sc["obs_pose"] == 8).any()                       # the (-1, -1) rule is in play


def test_cull_threshold_on_exact_values(oracle):
    sc = C.k12_exact()
    o = _oracle_errors(oracle, sc)
    known = ~np.isnan(sc["mean"])
    assert np.array_equal(o["mean_err"][known].astype(np.float64), sc["mean"][known])
    assert np.array_equal(o["cull"], sc["expect"])
    assert (o["cull"][sc["mean"] == 3.0] == 0).all() and (sc["mean"] == 3.0).sum() >= 7
    r = R.point_errors(sc["positions"], sc["obs_ptr"], sc["obs_pose"], sc["obs_uv"], sc["poses"], C.K)
    assert (np.abs(o["mean_err"] - r["mean"]) <= r["b_mean"]).all()


def test_points_on_the_camera_plane(oracle):
    sc = C.k12_plane()
    o = _oracle_errors(oracle, sc)
    m = o["mean_err"]
    assert np.isinf(m[0]) and np.isnan(m[1]) and m[2] == 0.0 and np.isinf(m[3]) and np.isnan(m[4])      # (1000 / 0, 0 / 0) is (inf, NaN)
    assert list(o["cull"]) == [1, 0, 0, 1, 0]


@pytest.mark.parametrize("n", C.CULL_SIZES)
def test_cull_patterns_are_exact_under_the_oracle(oracle, n):
    for pattern in C.KEEP_PATTERNS:
        sc = C.k12_cull_case(pattern, n)
        o = _oracle_errors(oracle, sc)
        assert np.array_equal(o["cull"] != 0, sc["cull"]) and np.array_equal(o["cull_idx"], np.flatnonzero(sc["cull"]))
        assert o["err_sum"] == 10.0 * sc["cull"].sum()


# -------------------------------------------------------------------------------------------------------- K13, K14
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("n_frames", [1, 32, 33])
def test_reanchor_against_the_referee(oracle, n_frames, n, permuted):
    c = C.k13_case(n_frames, n, permuted)
    got = C.oracle_reanchor(oracle, c)
    ref, bound = R.reanchor_points(c["point_idx"], c["frame_idx"], c["before"], c["after"], c["positions"])
    moved = bound.any(1)
    print("moved", int(moved.sum()), "max err / bound", (np.abs(got - ref)[moved] / bound[moved]).max())
    assert (np.abs(got - ref) <= bound).all()
    assert np.array_equal(got[~moved], c["positions"][~moved])
    f = c["frame_idx"]
    assert moved.sum() == ((f >= 0) & (f < n_frames)).sum() and (f == -1).any() and (f == n_frames).any()
    assert (np.abs(got - c["positions"])[moved].max(1) > 1e-3).all()


def test_transform_points_against_the_referee(oracle):
    c = C.k14_case()
    got = oracle.transform_points(c["obs_ptr"], c["obs_kf"], c["before"], c["after"], c["positions"])
    ref, bound, owner = R.transform_points(c["obs_ptr"], c["obs_kf"], c["before"], c["after"], c["positions"])
    moved = bound.any(1)
    assert (np.abs(got - ref) <= bound).all() and np.array_equal(got[~moved], c["positions"][~moved])
    assert np.array_equal(moved, owner >= 0) and (owner == -1).any() and (owner == -2).any() and owner.max() == len(c["before"]) - 1
    # the owner stands first, last and in the middle of its list
    where = {l.index(min(l)) - (len(l) - 1) / 2.0 for l in c["lists"] if len(l) >= 3 and min(l) >= 0}
    assert min(where) < 0 < max(where) and 0.0 in where
