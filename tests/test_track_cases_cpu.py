"""tests/track_cases.py without a GPU: every case's expectation recomputed from tests/track_ref.py, and every tag of its
`reaches` derived again from the arrays by the predicates below, which use tests/track_ref.py and the restated hash alone.
The union of the tags over all cases must be every tag the module declares, so a generator cannot lose a path quietly.

Every carry and add case with at most 2049 entries and keypoints is also held against the independent object model of
tests/test_track_cpu.py (Frame.add_map_match entry by entry, model_carry's two loops).  The model walks a whole table per
entry, so the 8192-sized cases rest on tests/track_ref.py alone, which tests/test_track_cpu.py holds against the same
model on random small inputs."""
import numpy as np
import pytest

import track_cases as TC
import track_ref as R
from test_track_cpu import Frame, Point, model_carry

MODEL_MAX = 2049


# ------------------------------------------------------------------------------------------------ carry
def carry_reached(c):
    """every carry tag that holds of the case's arrays"""
    m = TC.carry_map(c["P"])
    P, nxt, prev_t, prev_index, inl = c["P"], c["next_table"], c["prev_table"], c["prev_index"].astype(np.int64), c["inlier"]
    n = R.clamp_count(c["count"], c["max_n"])
    usable = min(c["n_next"], c["max_n"])
    cand = R.carry_candidates(m["alive"], m["n_obs"], m["consistent"], prev_t, c["n_next"], prev_index, inl, c["count"], c["max_n"])
    table, n_c, acc = R.carry(m["alive"], m["n_obs"], m["consistent"], prev_t, nxt, prev_index, inl, c["count"], c["max_n"], c["min_points"])
    assert n_c == len(cand)
    existing = set(int(p) for p in nxt if 0 <= p < P)
    live = [(i, j, p) for i, j, p in cand if nxt[j] < 0 and p not in existing]
    is_open = len(cand) >= c["min_points"]
    cut = c["count"] is not None and c["count"] <= 0   # a count of nothing goes by the length of the list it cuts
    got = {"long" if (c["max_n"] if cut else n) > TC.THREADS else "small"}
    by_kp, by_pt = {}, {}
    for i, j, p in live:
        by_kp.setdefault(j, []).append(i)
        by_pt.setdefault(p, []).append(i)
    kp_rep = any(len(v) > 1 for v in by_kp.values())
    pt_rep = any(len({j for i, j, q in live if q == p}) > 1 for p, v in by_pt.items() if len(v) > 1)
    repeats = kp_rep or any(len(v) > 1 for v in by_pt.values())
    if not is_open:
        got.add("gated")
    else:
        got.add("serial" if repeats else "parallel" if acc > 0 else "nothing_accepted")
        if any(nxt[j] >= 0 for _, j, _ in cand):
            got.add("refused_kp")
        if any(p in existing for _, _, p in cand):
            got.add("refused_point")
        at = {i: (j, p) for i, j, p in live}
        for d in (1, 64, 1024):
            if any(i + d in at and (at[i + d][0] == j or at[i + d][1] == p) for i, (j, p) in at.items()):
                got.add(f"repeat_{d}")
        if kp_rep:
            got.add("kp_repeat")
        if pt_rep:
            got.add("point_repeat")
        if kp_rep and pt_rep:
            got.add("both_repeats")
        if repeats and n == TC.FM_MAX and live[-1][0] == n - 1:
            rest = live[:-1]
            if len({j for _, j, _ in rest}) == len(rest) == len({p for _, _, p in rest}):
                got.add("fallback_full_walk")          # the one repeat is the last entry: the lane walks all 8192
        marks = [p for _, _, p in live] + list(existing)
        if any(p >= 4096 for p in marks):
            got.add("mark_past_4096")
        if any(p >= 8192 for p in marks):
            got.add("mark_past_8192")
    if len({(j, p) for _, j, p in cand}) < c["min_points"] <= len(cand):
        got.add("gate_by_multiplicity")
    if any(p == P - 1 for _, _, p in cand):
        got.add("slot_last")
    if c["n_next"] < c["max_n"]:
        got.add("n_next_lt_max_n")
    if c["n_next"] > c["max_n"]:
        got.add("n_next_gt_max_n")
    cnt = c["count"]
    got.add("count_none" if cnt is None else "count_zero" if cnt == 0 else "count_negative" if cnt < 0 else
            "count_over" if cnt > c["max_n"] else "count_half" if cnt == c["max_n"] // 2 else "count_other")
    got.add({0: "min_at", -1: "min_below", 1: "min_above"}.get(c["min_points"] - len(cand), "min_other"))
    if not c["stats"]:
        got.add("null_stats")
    got.add("no_inlier" if inl is None else "inlier_ascending" if np.all(np.diff(inl[:n]) > 0) else "inlier_other")
    special = {-1, c["n_prev"], c["max_n"], TC.I32_MAX}
    if inl is not None and special <= set(int(v) for v in inl[:n]) and special <= set(int(v) for v in prev_index[:usable]):
        got.add("bad_index")
    for i in range(n):                                 # what the entries find in prev's table
        j = int(inl[i]) if inl is not None else i
        if 0 <= j < usable and 0 <= prev_index[j] < c["n_prev"]:
            p = int(prev_t[prev_index[j]])
            if p >= P:
                got.add("prev_oob")
            elif p >= 0 and not m["alive"][p]:
                got.add("prev_dead")
            elif p >= 0 and m["n_obs"][p] < 2 and not m["consistent"][p]:
                got.add("prev_gate_fail")
    if any(0 <= p < P and not m["alive"][p] for p in nxt):
        got.add("next_dead")
    if any(p >= P for p in nxt):
        got.add("next_oob")
    return got, (table, n_c, acc)


@pytest.mark.parametrize("case", TC.carry_cases(), ids=lambda c: c["name"])
def test_carry_case_reaches_what_it_says(case):
    got, (table, n_c, acc) = carry_reached(case)
    e = case["expect"]
    assert np.array_equal(table, e["table"]) and (n_c, acc) == (e["candidates"], e["accepted"])
    assert case["reaches"] <= TC.CARRY_TAGS and case["reaches"] <= got, case["reaches"] - got
    live = e["table"][(e["table"] >= 0)]
    assert len(np.unique(live)) == len(live)
    assert len(case["prev_index"]) == case["max_n"] and (case["inlier"] is None or len(case["inlier"]) == case["max_n"])


def test_carry_cases_cover_every_path_at_both_lengths():
    cases = TC.carry_cases()
    assert set().union(*[c["reaches"] for c in cases]) == TC.CARRY_TAGS
    for tag in TC.CARRY_BOTH_LENGTHS:
        for length in ("small", "long"):
            assert any({tag, length} <= c["reaches"] for c in cases), (tag, length)
    # the sizes the cases must mix
    assert {1, 64, 1023, 1025, 8192} <= {c["n_prev"] for c in cases} and {1, 64, 1023, 1025, 8192} <= {c["n_next"] for c in cases}
    assert {1, 1024, 1025, 2049, 8192} == {c["max_n"] for c in cases} and {1, 61, 4097, 9001} == {c["P"] for c in cases}
    for P in (1, 61, 4097, 9001):
        assert "parallel" in carry_reached(TC.carry_probe(P))[0]


def model_points(P, m, *tables):
    """the object model's points by slot; a dead slot or one past the map is a match that no gate lets through"""
    pts = {p: Point(p, int(m["n_obs"][p]) if m["alive"][p] else 0, bool(m["consistent"][p]) and bool(m["alive"][p])) for p in range(P)}
    for t in tables:
        for p in t:
            if p >= P:
                pts.setdefault(int(p), Point(int(p), 0, False))
    return pts


def model_frame(table, pts):
    f = Frame(len(table))
    for k, p in enumerate(table):
        if p >= 0:
            f.add_map_match(pts[int(p)], k)
    return f


@pytest.mark.parametrize("case", [c for c in TC.carry_cases() if max(c["n_prev"], c["n_next"], c["max_n"]) <= MODEL_MAX], ids=lambda c: c["name"])
def test_carry_case_equals_the_object_model(case):
    c, m = case, TC.carry_map(case["P"])
    pts = model_points(c["P"], m, c["prev_table"], c["next_table"])
    prev, nxt = model_frame(c["prev_table"], pts), model_frame(c["next_table"], pts)
    n, usable = R.clamp_count(c["count"], c["max_n"]), min(c["n_next"], c["max_n"])
    pairs = []
    for i in range(n):                                 # the (query, train) pairs a tracker could have produced
        j = int(c["inlier"][i]) if c["inlier"] is not None else i
        if 0 <= j < usable and 0 <= c["prev_index"][j] < c["n_prev"]:
            pairs.append((j, int(c["prev_index"][j])))
    want = model_carry(pts, prev, nxt, c["prev_index"], pairs, c["min_points"])
    assert want == (c["expect"]["candidates"], c["expect"]["accepted"]) and np.array_equal(nxt.table(), c["expect"]["table"])


# ------------------------------------------------------------------------------------------------ add
def add_reached(c):
    got, table = {f"table_{c['n_kp']}"}, np.array(c["start"])
    assert R.num_matches(table) > 0
    tables = []
    for li in c["lists"]:
        kp, pt, n = li["kp"].astype(np.int64), li["point"].astype(np.int64), R.clamp_count(li["count"], li["max_n"])
        hmask = TC.add_hmask(li["max_n"])
        ok = (kp[:n] >= 0) & (kp[:n] < c["n_kp"]) & (pt[:n] >= 0)
        k, p = kp[:n][ok], pt[:n][ok]
        _, first = np.unique(p, return_index=True)
        distinct = p[np.sort(first)]                   # in list order
        assert 2 * len(distinct) <= hmask + 1          # the kernel's probe loop ends only below full
        homes = (TC.fm_hash(distinct) & np.uint64(hmask)).astype(np.int64)
        if hmask == 63 and np.bincount(homes).max() >= 32:
            got.add("chain32")
        if 2 * len(distinct) == hmask + 1:
            got.add(f"load_half_{hmask + 1}")
        # more keys at home in the last four slots than those hold: whatever order the threads insert in, one probe goes on to slot 0
        if np.count_nonzero(homes >= hmask - 3) >= 200 and any(hmask in w and w[-1] < w[0] for w in TC.probe_slots(hmask, distinct.tolist())):
            got.add("wraps")
        if len(distinct) == 1 and len(np.unique(k)) == n == TC.FM_MAX:
            got.add("one_point_many_kp")
        if len(np.unique(k)) == 1 and len(distinct) == n == TC.FM_MAX:
            got.add("one_kp_many_points")
        if TC.I32_MAX in distinct:
            got.add("point_max")
        for stride in (1, 128, 2 ** 16, 2 ** 25):
            if n == li["max_n"] in (32, TC.FM_MAX) and np.array_equal(p, TC.progression(stride, n)):
                got.add(f"ap_{stride}")
        if li["count"] is not None:
            got.add("device_count")
        if len(np.unique(k)) < len(k):
            got.add("kp_repeat")
        if len(distinct) < len(p):
            got.add("point_repeat")
            crowded = set(distinct[(homes >= hmask - 3) | (homes == np.bincount(homes).argmax())].tolist())
            if (hmask == 63 or np.count_nonzero(homes >= hmask - 3) >= 200) and any(np.count_nonzero(p == q) > 1 for q in crowded):
                got.add("cluster_repeat")
        after = R.matches_add(table, kp, pt, li["count"], li["max_n"])
        unnamed = np.setdiff1d(np.arange(c["n_kp"]), k)
        if np.any((table[unnamed] >= 0) & (after[unnamed] < 0)):
            got.add("clears_unnamed")
        table = after
        tables.append(after)
    return got, tables


@pytest.mark.parametrize("case", TC.add_cases(), ids=lambda c: c["name"])
def test_add_case_reaches_what_it_says(case):
    got, tables = add_reached(case)
    for li, t in zip(case["lists"], tables):
        assert np.array_equal(t, li["expect"])
        live = t[t >= 0]
        assert len(np.unique(live)) == len(live)
    assert case["reaches"] <= TC.ADD_TAGS and case["reaches"] <= got, case["reaches"] - got


def test_add_cases_cover_every_path():
    assert set().union(*[c["reaches"] for c in TC.add_cases()]) == TC.ADD_TAGS
    # the restated hash: Knuth's multiplier in 32 bits, bits 7 and up
    assert int(TC.fm_hash(1)) == 2654435761 >> 7 and int(TC.fm_hash(3)) == (3 * 2654435761 % 2 ** 32) >> 7
    assert int(TC.fm_hash(TC.I32_MAX)) == (TC.I32_MAX * 2654435761 % 2 ** 32) >> 7
    assert (TC.add_hmask(1), TC.add_hmask(32), TC.add_hmask(33), TC.add_hmask(8192)) == (63, 63, 127, 16383)


@pytest.mark.parametrize("case", [c for c in TC.add_cases() if c["n_kp"] <= MODEL_MAX and all(li["max_n"] <= MODEL_MAX for li in c["lists"])],
                         ids=lambda c: c["name"])
def test_add_case_equals_the_object_model(case):
    pts = {}
    point = lambda p: pts.setdefault(int(p), Point(int(p)))      # noqa: E731
    frame = Frame(case["n_kp"])
    for k, p in enumerate(case["start"]):
        if p >= 0:
            frame.add_map_match(point(p), k)
    for li in case["lists"]:
        for i in range(R.clamp_count(li["count"], li["max_n"])):
            if 0 <= li["kp"][i] < case["n_kp"] and li["point"][i] >= 0:
                frame.add_map_match(point(li["point"][i]), int(li["kp"][i]))
        assert np.array_equal(frame.table(), li["expect"]) and frame.num_map_matches == R.num_matches(li["expect"])


# ------------------------------------------------------------------------------------------------ gather
@pytest.fixture(scope="module")
def geometry(synth):
    return TC.gather_geometry(synth)


@pytest.mark.parametrize("n_kp", TC.GATHER_SIZES)
def test_gather_cases_reach_what_they_say(geometry, n_kp):
    m, kp = TC.gather_map(), TC.gather_keypoints(geometry, n_kp)
    per = (n_kp + TC.THREADS - 1) // TC.THREADS
    cases = [c for c in TC.gather_cases() if c["n_kp"] == n_kp]
    assert len(cases) == 8
    for c in cases:
        t, e = c["table"], c["expect"]
        pts, uv, n_used = R.gather(t, kp, m["alive"], m["n_obs"], geometry["positions"], c["min_matches"])
        matched = R.num_matches(t)
        assert n_used == e["n_used"] and matched == e["matched"]
        got = {f"per_{per}"}
        if n_used >= 0:
            assert np.array_equal(uv, kp[e["kept"]]) and np.array_equal(pts, geometry["positions"][t[e["kept"]]].astype(np.float64))
            assert n_used == len(e["kept"]) and np.all(np.diff(e["kept"]) > 0)
            if n_used > 0:                             # a kept keypoint sees its point where the problem observed it
                assert np.array_equal(uv, geometry["problem"]["uv"][t[e["kept"]]])
        else:
            got.add("gate_refuses")
        if matched == 0:
            got.add("empty")
        if n_used == 0:
            got.add("none_kept")
        if n_used == TC.FM_MAX:
            got.add("all_kept_8192")
        if matched >= 4096 and (n_used >= 4096 or n_used == 0):
            got.add("packed_high")                     # the scan's upper half carries thousands while the lower one is full or empty
        if n_used > 0 and np.array_equal(e["kept"], np.arange(0, n_kp, 2)) and matched == n_kp:
            got.add("alternating")
        if n_used > 0 and matched == n_kp and e["kept"][0] == (n_kp - 1) // per * per and e["kept"][0] // per == (n_kp - 1) // per:
            got.add("last_run_only")
        if any(0 <= p < m["P"] and not m["alive"][p] for p in t) and any(p >= m["P"] for p in t) and TC.I32_MAX in t:
            got.add("dead_and_oob")
        got.add({0: "min_at", 1: "min_above"}.get(c["min_matches"] - matched, "min_other"))
        assert c["reaches"] <= TC.GATHER_TAGS and c["reaches"] <= got, (c["name"], c["reaches"] - got)


def test_gather_cases_cover_every_per_and_gate():
    cases = TC.gather_cases()
    assert set().union(*[c["reaches"] for c in cases]) == TC.GATHER_TAGS
    assert {1, 1024, 1025, 2049, 3000, 4097, 5000, 6145, 7000, 7169, 8192} <= set(TC.GATHER_SIZES)
    m = TC.gather_map()
    assert m["P"] > 2 * TC.FM_MAX and len(m["alive"]) == len(m["n_obs"]) == m["P"]


# ------------------------------------------------------------------------------------------------ match
def test_match_cases_state_their_table():
    cases = TC.match_cases()
    assert set().union(*[c["reaches"] for c in cases]) == TC.MATCH_TAGS and len(cases) == 12
    for c in cases:
        P, t = c["requires"]["P"], TC.start_table(c)
        pts = set(int(p) for p in t if p >= 0)
        got = {f"kp_{c['n_kp']}", f"distance_{c['max_distance']}", "required_last" if c["required_observer"] == c["requires"]["n_kf"] - 1 else
               "required_none" if c["required_observer"] == -1 else "required_other"}
        assert P % 4 != 0 and len(pts) == R.num_matches(t) == len(c["start_kp"])
        if P - 1 in pts:
            got.add("last_slot")
        if any({4 * q, 4 * q + 1, 4 * q + 2, 4 * q + 3} <= pts for q in range(P // 4)):
            got.add("four_in_word")
        if c["requires"]["dead"] in pts:
            got.add("dead")
        if any(p >= P for p in pts):
            got.add("oob")
        if sum(p < P and p != c["requires"]["dead"] for p in pts) >= 20:
            got.add("live")
        assert c["reaches"] <= got
