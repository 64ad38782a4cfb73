"""The cases of tests/bow_cases.py without a GPU: each is held, on the restatement tests/bow_ref.py alone, to the
condition it exists for — so that the GPU test of the same case (tests/test_gpu_bow_envelope.py) cannot pass on a case
that missed its target.  If a seed misses a condition, another seed is chosen; the condition stays."""
import numpy as np
import pytest

import bow_cases as BC
import bow_ref as B


def words_of(t, rows, weighting=B.TF_IDF):
    return B.transform(BC.voc_of(t, weighting), rows)


# ------------------------------------------------------------------------------------------------ trees and aimed rows
@pytest.mark.parametrize("n,k", BC.HEAP_TREES)
def test_heap_trees(n, k):
    case = BC.heap_case(n, k)
    t = case["tree"]
    voc = BC.voc_of(t)
    assert voc.n_nodes == n and t["L"] == (7 if k == 3 else 3) and t["k"] == k
    assert np.array_equal(BC.bfs_order(voc), np.arange(n))      # breadth-first position == node id
    assert np.array_equal(t["parent"][1:], (np.arange(1, n) - 1) // k)
    assert BC.depth_of(voc)[-1] == t["L"] and np.all(t["weight"][t["leaf"]] > 0) and np.all(t["weight"][~t["leaf"]] == 0)
    # the staged prefix: all of the tree up to LDS_NODES nodes, a partial last trip of the staging loop at 1279
    assert (min(n, BC.LDS_NODES) == n) == (n <= BC.LDS_NODES)
    assert case["targets"] == tuple(range(n - 4, n)) and all(t["leaf"][list(case["targets"])])
    assert 200 <= len(case["rows"]) <= 400
    wid = B.descend(voc, case["rows"])
    for node in case["targets"]:
        assert (wid == voc.word_of[node]).sum() >= 8, node
    last = np.flatnonzero(t["parent"] == t["parent"][-1])
    if (n, k) == (1281, 20):                                    # nineteen children in LDS, the twentieth in global memory
        assert last.tolist() == list(range(1261, 1281)) and (last < BC.LDS_NODES).sum() == 19
    if (n, k) == (1281, 3):
        assert last.tolist() == [1279, 1280]
    if (n, k) == (1282, 3):
        assert last.tolist() == [1279, 1280, 1281]


def test_bfs_order_is_a_layout_of_the_tree():
    """on a tree whose node ids are shuffled: a permutation, the root first, every family contiguous and ascending"""
    voc = BC.ref_voc(BC.K46)
    order = BC.bfs_order(voc)
    assert order[0] == 0 and np.array_equal(np.sort(order), np.arange(voc.n_nodes)) and not np.array_equal(order, np.arange(voc.n_nodes))
    at = np.empty(voc.n_nodes, np.int64)
    at[order] = np.arange(voc.n_nodes)
    depth = BC.depth_of(voc)
    assert np.all(np.diff(depth[order]) >= 0)
    for node in (0, int(order[5]), int(order[300]), int(order[1279])):
        c = voc.children(node)
        assert np.all(np.diff(c) > 0) and np.array_equal(at[c], at[c[0]] + np.arange(len(c)))


def test_straddling_leaves():
    case = BC.straddle_case()
    voc = BC.ref_voc(BC.K104)
    assert voc.n_nodes == 11111 and voc.n_words == 10000
    order = BC.bfs_order(voc)
    lo, hi = case["targets"]
    assert order[BC.LDS_NODES - 1] == lo and order[BC.LDS_NODES] == hi      # on opposite sides of the prefix's end
    assert voc.parent[lo] == voc.parent[hi] and voc.leaf[lo] and voc.leaf[hi]
    wid = B.descend(voc, case["rows"])
    assert (wid == voc.word_of[lo]).sum() >= 8 and (wid == voc.word_of[hi]).sum() >= 8
    assert 200 <= len(case["rows"]) <= 400


def test_straddling_inner_nodes():
    case = BC.inner_straddle_case()
    voc = BC.ref_voc(BC.K46)
    assert voc.n_nodes == 5461
    order = BC.bfs_order(voc)
    depth = BC.depth_of(voc)
    assert np.all(depth[order[341:1365]] == 5) and depth[order[340]] == 4 and depth[order[1365]] == 6
    lo, hi = case["targets"]
    assert order[BC.LDS_NODES - 1] == lo and order[BC.LDS_NODES] == hi
    assert voc.parent[lo] == voc.parent[hi] and not voc.leaf[lo] and not voc.leaf[hi]
    wid = B.descend(voc, case["rows"])
    for fam in case["families"]:
        assert len(fam) == 4 and all(voc.leaf[list(fam)])
        assert np.isin(wid, voc.word_of[list(fam)]).sum() >= 8
    assert 200 <= len(case["rows"]) <= 400


def test_ties():
    case = BC.tie_case()
    t, pairs = case["tree"], case["pairs"]
    voc = BC.voc_of(t)
    assert (t["k"], t["L"], t["n_nodes"]) == (20, 2, 421)
    assert [(lo - t["parent"][lo] * 20 - 1, hi - t["parent"][hi] * 20 - 1) for lo, hi in pairs] == [(2, 18), (16, 17)]
    wid = B.descend(voc, case["rows"])
    tied = case["rows"][:case["n_tied"]]
    hits = 0
    for lo, hi in pairs:
        assert t["parent"][lo] == t["parent"][hi] and np.array_equal(t["desc"][lo], t["desc"][hi]) and t["leaf"][lo] and t["leaf"][hi]
        assert not np.any(wid == voc.word_of[hi])               # the lower sibling wins, always
        mine = np.flatnonzero(wid[:case["n_tied"]] == voc.word_of[lo])
        assert len(mine) >= 100
        hits += len(mine)
        fam = voc.children(t["parent"][lo])
        d = B.hamming(tied[mine][:, None, :], t["desc"][fam][None, :, :])
        assert np.all(d.min(1) == d[:, list(fam).index(lo)]) and np.all(d[:, list(fam).index(lo)] == d[:, list(fam).index(hi)])
        assert np.any(d.min(1) == 0) and np.any(d.min(1) > 0)   # the shared row itself, and rows near it
    assert hits == case["n_tied"]


def test_chain():
    case = BC.chain_case()
    t = case["tree"]
    voc = BC.voc_of(t)
    assert (t["k"], t["L"], t["n_nodes"], voc.n_words) == (1, 10, 11, 1)
    assert np.array_equal(t["parent"], np.arange(-1, 10))
    assert B.hamming(case["rows"], t["desc"][-1]).max() == 256
    assert np.all(B.descend(voc, case["rows"]) == 0)


# ------------------------------------------------------------------------------------------------ wide sets
def test_every_leaf_of_the_wide_trees_returns_to_itself():
    assert len(BC.own_words(BC.K104)) == 10000
    assert len(BC.own_words(BC.K114)) >= 3 * BC.MAX_POINTS // 2


@pytest.mark.parametrize("m", BC.WIDE_SIZES)
def test_wide_sets(m):
    ref = B.transform(BC.ref_voc(BC.K104), BC.wide_rows(m))
    assert len(ref["words"]) == m and np.all(ref["counts"] == 1)
    if m > 1:
        assert np.any(np.diff(ref["word_of_feature"]) < 0)      # not handed over in order


def test_wide_stopped_sets():
    voc = BC.ref_voc(BC.K104_STOPPED)
    assert np.array_equal(BC.tree(BC.K104_STOPPED)["desc"], BC.tree(BC.K104)["desc"])
    for m in BC.WIDE_VARIANT_SIZES:
        rows = BC.wide_rows(m)
        ref = B.transform(voc, rows)
        unique = np.unique(ref["word_of_feature"])
        assert len(unique) == m and 0 < len(ref["words"]) < m
        if m == 8192:
            assert 3000 <= len(ref["words"]) <= 5200
            kept = np.isin(unique, ref["words"])
            for at in range(0, m, 512):                         # holes in every wave's 512 runs
                assert kept[at:at + 512].any() and not kept[at:at + 512].all()


def test_wide_repeated_sets():
    for m in BC.WIDE_VARIANT_SIZES:
        rows, u = BC.repeated_rows(m)
        ref = B.transform(BC.ref_voc(BC.K104), rows)
        assert len(rows) == m and len(ref["words"]) == u and u > 0.7 * m and ref["counts"].sum() == m
        assert set(ref["counts"].tolist()) >= {1, 2, 3, 4, 5}
        assert np.any(np.diff(ref["word_of_feature"]) < 0)
    assert u > 7 * 1024                                         # the last of the 16 waves holds runs too


# ------------------------------------------------------------------------------------------------ score pairs
def pair_words(name):
    voc = BC.ref_voc(BC.K114)
    q, e = BC.score_pair(name)
    return B.transform(voc, q), B.transform(voc, e)


def test_score_pairs():
    seen = set()
    for name in BC.SCORE_PAIRS:
        rq, re_ = pair_words(name)
        q, e = set(rq["words"].tolist()), set(re_["words"].tolist())
        lo, hi = min(q), max(q)
        if name == "e_in_q":
            assert e < q and len(e) > 1
        elif name == "q_in_e":
            assert q < e and len(q) > 1
        elif name == "share_lowest":
            assert q & e == {lo} and min(e) < lo and max(e) > hi
        elif name == "share_highest":
            assert q & e == {hi} and min(e) < lo and max(e) > hi
        elif name == "e_below":
            assert max(e) < lo and len(e) > 64
        elif name == "e_above":
            assert min(e) > hi and len(e) > 64
        elif name == "same_words_other_counts":
            assert q == e and not np.array_equal(rq["counts"], re_["counts"]) and rq["counts"].max() > 1 and re_["counts"].max() > 1
            assert 0 < B.score(rq, re_) < 1 - 1e-3
        elif name == "q_single":
            assert len(q) == 1 and q < e
        elif name == "both_8192":
            assert len(q) == len(e) == 8192 and 3500 <= len(q & e) <= 4700
        assert (B.score(rq, re_) > 0) == bool(q & e)
        seen.add(name)
    assert seen == set(BC.SCORE_PAIRS)


def test_score_entry_sizes():
    voc = BC.ref_voc(BC.K114)
    assert BC.SCORE_ENTRY_SIZES == (0, 1, 63, 64, 65, 127, 128, 129, 8192)
    for size in BC.SCORE_ENTRY_SIZES:
        assert len(B.transform(voc, BC.score_entry_rows(size))["words"]) == size


# ------------------------------------------------------------------------------------------------ the sequence
def test_sequence_sets():
    t, stopped = BC.sequence_tree()
    voc = BC.voc_of(t)
    assert len(stopped) == 400 and np.all(voc.word_weight[stopped] == 0) and (voc.word_weight == 0).sum() == 400
    r = {name: B.transform(voc, rows) for name, rows in BC.sequence_sets().items()}
    w = {name: set(v["words"].tolist()) for name, v in r.items()}
    assert len(w["A"]) == 8192 and len(w["B"]) == 100 and not w["A"] & w["B"]
    assert len(BC.sequence_sets()["empty"]) == 0 and not w["empty"] and r["empty"]["norm"] == 0
    assert len(BC.sequence_sets()["stopped"]) == 300 and not w["stopped"] and r["stopped"]["norm"] == 0
    assert len(np.unique(r["stopped"]["word_of_feature"])) == 300
    assert len(w["C"]) == 100 and len(w["C"] & w["A"]) == 1
    assert len(w["A2"]) == 4097 and w["A2"] < w["A"] and r["A2"]["counts"].max() > 1
    assert len(w["D"]) == 1500 and len(w["D"] & w["A"]) == 750
    # a second trip of the loop that clears the previous vector from the table, with something to get wrong: words of A
    # beyond its first 1024 that B's entry, C and D would find
    late = set(r["A"]["words"][1024:].tolist())
    assert late & w["A2"] and late & w["D"] and (w["C"] & w["A"]) <= late
    assert BC.SEQUENCE == ("A", "B", "empty", "stopped", "A", "C", "A") and set(BC.SEQUENCE_DATABASE) <= set(r)
    assert B.score(r["A"], r["B"]) == 0 and B.score(r["A"], r["A2"]) > 0


# ------------------------------------------------------------------------------------------------ text files
def parse(tmp_path, name, text):
    path = tmp_path / f"{name}.txt"
    path.write_bytes(text.encode())
    return B.parse_text(path)


def test_text_files(tmp_path):
    R = BC.ref_voc(BC.TEXT_TREE, B.IDF)
    assert len(set(np.bincount(R.parent[1:]).tolist())) > 2     # ragged
    texts = BC.well_formed_texts(R)
    assert set(texts) >= {"crlf", "tabs_and_runs_of_spaces", "no_final_newline", "three_trailing_blank_lines", "exponent_weights",
                          "one_extra_trailing_field"}
    assert "\r\n" in texts["crlf"] and "\t" in texts["tabs_and_runs_of_spaces"] and "   " in texts["tabs_and_runs_of_spaces"]
    assert not texts["no_final_newline"].endswith("\n") and texts["three_trailing_blank_lines"].count("\n") == R.n_nodes + 3
    assert "e+00" in texts["exponent_weights"] and len(texts["one_extra_trailing_field"].split("\n")[4].split()) == 36
    for name, text in texts.items():
        v = parse(tmp_path, name, text)
        assert (v.k, v.L, v.weighting, v.scoring, v.n_nodes, v.n_words) == (R.k, R.L, R.weighting, R.scoring, R.n_nodes, R.n_words), name
        assert np.array_equal(v.parent, R.parent) and np.array_equal(v.desc, R.desc) and np.array_equal(v.weight, R.weight), name


def test_malformed_text_files(tmp_path):
    R = BC.ref_voc(BC.TEXT_TREE, B.IDF)
    texts = BC.malformed_texts(R)
    assert len(texts) >= 12
    changed = {name: text.split("\n")[5].split() for name, (text, status) in texts.items() if not name.startswith(("header", "only"))}
    assert len(changed["34_fields_a_byte_missing"]) == 34 and "." in changed["34_fields_a_byte_missing"][-1]
    assert len(changed["no_weight"]) == 34 and "." not in changed["no_weight"][-1]
    assert changed["blank_line_in_the_middle"] == []
    for name, (text, status) in texts.items():
        with pytest.raises((ValueError, OverflowError)):
            parse(tmp_path, name, text)
        assert status == (4 if name in ("header_k_21", "header_L_11") else 1)
