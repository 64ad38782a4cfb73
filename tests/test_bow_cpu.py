"""tests/bow_ref.py (the specification of csrc/bow.hip and rs_rank_loop_candidates) pinned by formulations that share
no code with it, the vocabulary text format, the synthetic vocabularies, and the host-only ranking entry point."""
import importlib

import numpy as np
import pytest

import bow_ref as B

synth = importlib.import_module("racing-slam_amd").synth


def _voc(k, L, weighting=B.TF_IDF, **kw):
    v = synth.make_vocabulary(k, L, **kw)
    return v, B.Vocabulary(k, L, weighting, B.L1_NORM, v["parent"], v["desc"], v["weight"])


TREES = [dict(k=2, L=1), dict(k=3, L=4), dict(k=10, L=3), dict(k=17, L=2), dict(k=20, L=2), dict(k=4, L=4, ragged=True),
         dict(k=5, L=3, duplicate_children=True), dict(k=6, L=3, ragged=True, duplicate_children=True, stopped_fraction=0.3)]


def _bits(rows):
    return np.unpackbits(np.ascontiguousarray(rows, np.uint8), axis=-1).astype(np.int32)


def _descend_loop(V, rows):
    """One feature at a time; np.argmin takes the first minimum.  Also counts the levels at which the minimum is shared."""
    kids = [[] for _ in range(V.n_nodes)]
    for i in range(1, V.n_nodes):
        kids[V.parent[i]].append(i)                             # ascending id
    leaves = [i for i in range(V.n_nodes) if not kids[i]]
    word = {node: w for w, node in enumerate(leaves)}
    nb, out, ties = _bits(V.desc), [], 0
    for fb in _bits(rows):
        node = 0
        while kids[node]:
            d = np.array([(fb != nb[c]).sum() for c in kids[node]])
            ties += int((d == d.min()).sum() > 1)
            node = kids[node][int(np.argmin(d))]
        out.append(word[node])
    return np.array(out, np.int32), ties


@pytest.mark.parametrize("tree", TREES, ids=lambda t: "-".join(f"{k}{v}" for k, v in t.items()))
def test_descent_transform_and_score_against_independent_forms(tree):
    v, V = _voc(**tree)
    rows = synth.make_bow_descriptors(v, 150, seed=1)
    wid, ties = _descend_loop(V, rows)
    assert np.array_equal(B.descend(V, rows), wid)
    if tree.get("duplicate_children"):
        assert ties > 0                                         # the tie rule is exercised
    # children and words as the loader numbers them
    n_children = np.bincount(V.parent[1:], minlength=V.n_nodes)
    assert n_children.max() <= V.k and V.n_words == int((n_children == 0).sum())
    assert np.array_equal(V.node_of_word, np.flatnonzero(n_children == 0))
    for weighting in (B.TF_IDF, B.TF, B.IDF, B.BINARY):
        W = B.Vocabulary(V.k, V.L, weighting, B.L1_NORM, V.parent, V.desc, V.weight)
        r = B.transform(W, rows)
        assert np.array_equal(r["word_of_feature"], wid)
        occ = np.bincount(wid, minlength=W.n_words)
        live = W.word_weight > 0
        dense = np.where(live, (occ if weighting in (B.TF_IDF, B.TF) else (occ > 0)) * W.word_weight, 0.0)
        total = dense.sum()
        dense = dense / total if total > 0 else dense
        assert np.array_equal(r["words"], np.flatnonzero((occ > 0) & live))
        assert np.array_equal(r["counts"], occ[r["words"]])
        assert np.allclose(r["values"], dense[r["words"]], rtol=1e-13, atol=0)
        assert np.isclose(r["norm"], total, rtol=1e-13)
        # score: 1 - |v - w|_1 / 2 on dense vectors
        other = B.transform(W, synth.make_bow_descriptors(v, 90, seed=2))
        d2 = np.zeros(W.n_words)
        d2[other["words"]] = other["values"]
        if len(r["words"]) and len(other["words"]):
            assert abs(B.score(r, other) - (1.0 - 0.5 * np.abs(dense - d2).sum())) < 1e-12
            assert abs(B.score(r, r) - 1.0) < 1e-12
        else:
            assert B.score(r, other) == 0


def test_empty_and_stopped_vectors():
    v, V = _voc(3, 3, stopped_fraction=1.0)
    r = B.transform(V, synth.make_bow_descriptors(v, 40))
    assert len(r["words"]) == 0 and r["norm"] == 0.0 and len(r["word_of_feature"]) == 40 and (r["word_of_feature"] >= 0).all()
    v, V = _voc(3, 3)
    e = B.transform(V, np.zeros((0, 32), np.uint8))
    assert len(e["words"]) == 0 and B.score(e, e) == 0
    full = B.transform(V, synth.make_bow_descriptors(v, 40))
    assert B.score(e, full) == 0 and B.score(full, e) == 0


def test_synthetic_vocabularies_have_the_promised_shapes():
    v = synth.make_vocabulary(10, 3)
    assert v["n_nodes"] == 1111 and int(v["leaf"].sum()) == 1000
    assert np.all(v["parent"][1:] < np.arange(1, v["n_nodes"])) and np.all(v["parent"][1:] >= 0)
    assert np.any(np.diff(np.flatnonzero(v["parent"] == 0)) > 1)                # children are not contiguous ids
    r = synth.make_vocabulary(6, 4, ragged=True)
    nc = np.bincount(r["parent"][1:], minlength=r["n_nodes"])
    assert nc.max() <= 6 and (nc == 1).any() and len(set(nc.tolist())) > 3
    depth = np.zeros(r["n_nodes"], np.int64)
    for i in range(1, r["n_nodes"]):
        depth[i] = depth[r["parent"][i]] + 1
    assert depth.max() == 4 and (depth[r["leaf"]] < 4).any()                    # early leaves
    d = synth.make_vocabulary(5, 3, duplicate_children=True)
    twins = 0
    for p in range(d["n_nodes"]):
        rows = d["desc"][d["parent"] == p]
        twins += len(rows) - len(np.unique(rows, axis=0)) if len(rows) else 0
    assert twins > 0
    s = synth.make_vocabulary(4, 3, stopped_fraction=0.5)
    w = s["weight"][s["leaf"]]
    assert (w == 0).any() and (w > 0).any() and np.all(s["weight"][~s["leaf"]] == 0)
    a, b = synth.make_vocabulary(3, 4, seed=1), synth.make_vocabulary(3, 4, seed=1)
    assert all(np.array_equal(a[k], b[k]) for k in ("parent", "desc", "weight"))


def test_text_round_trip(tmp_path):
    v, V = _voc(4, 3, weighting=B.IDF, ragged=True, stopped_fraction=0.2)
    path = tmp_path / "voc.txt"
    B.write_text(V, path)
    R = B.parse_text(path)
    assert (R.k, R.L, R.weighting, R.scoring, R.n_nodes) == (V.k, V.L, V.weighting, V.scoring, V.n_nodes)
    assert np.array_equal(R.parent, V.parent) and np.array_equal(R.desc, V.desc) and np.array_equal(R.weight, V.weight)
    text = path.read_text()
    assert text.endswith("\n") and len(text.split("\n")) == V.n_nodes + 1       # the trailing blank line makes no node
    path.write_text(text + "\n")
    assert B.parse_text(path).n_nodes == V.n_nodes


def test_malformed_trees_are_refused(tmp_path):
    v, V = _voc(3, 2)
    ok = dict(k=3, L=2, weighting=0, scoring=0, parent=v["parent"].copy(), desc=v["desc"], weight=v["weight"])
    B.Vocabulary(**ok)
    bad = dict(ok, k=2)
    with pytest.raises(ValueError):
        B.Vocabulary(**bad)                                     # more than k children
    p = ok["parent"].copy()
    p[3] = 3
    with pytest.raises(ValueError):
        B.Vocabulary(**dict(ok, parent=p))                      # parent not below the node
    with pytest.raises(ValueError):
        B.Vocabulary(**dict(ok, scoring=1))
    for env in (dict(k=21), dict(L=11), dict(k=0), dict(L=0)):
        with pytest.raises(ValueError):
            B.Vocabulary(**dict(ok, **env))
    path = tmp_path / "voc.txt"
    B.write_text(V, path)
    lines = path.read_text().split("\n")
    t = lines[1].split()
    t[1] = "0" if t[1] == "1" else "1"
    lines[1] = " ".join(t)
    path.write_text("\n".join(lines))
    with pytest.raises(ValueError):
        B.parse_text(path)                                      # leaf flag against the children


# ------------------------------------------------------------------------------------------------ ranking
def _rank_direct(scores, top=3, min_score=np.float32(0.02), ratio=np.float32(1.25)):
    """rank_candidates transcribed on plain lists of f32: positions in the considered list."""
    s = [np.float32(x) for x in scores]
    if s:
        srt = sorted(s)
        median = srt[min(len(s) - 1, int(np.float32(0.5) * np.float32(len(s) - 1)))]
    else:
        median = np.float32(0)
    thresh = max(min_score, np.float32(median * ratio))
    peaks = []
    for i, x in enumerate(s):
        left = s[i - 1] if i > 0 else np.float32(0)
        right = s[i + 1] if i + 1 < len(s) else np.float32(0)
        if x >= thresh and x >= left and x >= right:
            peaks.append(i)
    out = []
    while peaks and len(out) < top:                             # repeated first-maximum selection = a stable descending sort
        best = max(range(len(peaks)), key=lambda j: (s[peaks[j]], -j))
        out.append(peaks.pop(best))
    return out


RANK_CASES = {
    "plateau": [0.05, 0.06, 0.30, 0.30, 0.30, 0.05, 0.04, 0.05, 0.20, 0.05, 0.06, 0.05],
    "peak_at_the_start": [0.40, 0.10, 0.05, 0.05, 0.06, 0.05, 0.05, 0.04],
    "peak_at_the_end": [0.05, 0.05, 0.06, 0.05, 0.05, 0.04, 0.10, 0.40],
    "both_ends_and_middle": [0.5, 0.1, 0.1, 0.1, 0.6, 0.1, 0.1, 0.1, 0.1, 0.1, 0.7],
    "four_peaks_keep_three": [0.1, 0.5, 0.1, 0.1, 0.4, 0.1, 0.1, 0.6, 0.1, 0.1, 0.45, 0.1, 0.1],
    "equal_peaks_keep_their_order": [0.1, 0.5, 0.1, 0.1, 0.5, 0.1, 0.1, 0.5, 0.1, 0.1, 0.5, 0.1, 0.1],
    "one_peak": [0.05, 0.05, 0.30, 0.05, 0.05, 0.05, 0.05],
    "all_below_the_floor": [0.010, 0.015, 0.019, 0.012, 0.011, 0.0199],
    "flat": [0.2] * 7,
    "single": [0.3],
    "below_the_median_rule": [0.30, 0.31, 0.30, 0.31, 0.30, 0.31, 0.30],
    "empty": [],
}


@pytest.mark.parametrize("name", sorted(RANK_CASES))
def test_rank_candidates_against_a_direct_transcription(name, rs):
    scores = RANK_CASES[name]
    entries = np.arange(len(scores), dtype=np.int32) * 2 + 1
    got = B.rank_candidates(entries, np.array(scores, np.float32))
    want = _rank_direct(scores)
    assert got["entries"].tolist() == [int(entries[i]) for i in want]
    assert got["scores"].tolist() == [np.float32(scores[i]) for i in want]
    if want or not scores:
        assert got["rejected"] is None
    else:                                                       # nothing passes: the first entry of greatest score is reported
        b = max(range(len(scores)), key=lambda i: (np.float32(scores[i]), -i))
        assert got["rejected"] == (int(entries[b]), np.float32(scores[b]))
    assert bool(want) == (name not in ("all_below_the_floor", "flat", "below_the_median_rule", "single", "empty"))
    if name == "equal_peaks_keep_their_order":
        assert want == [1, 4, 7]
    if name == "plateau":
        assert want == [2, 3, 4]
    # the C entry point, through the gates: 49 later entries are too close to the query
    f64 = np.concatenate([np.array(scores, np.float32).astype(np.float64) + 1e-12, np.full(49, 0.9)])
    frames = np.arange(len(f64), dtype=np.int64) * 10
    c = rs.rank_loop_candidates(f64, frames, 10 * len(f64), 1.0 / 30.0)
    r = B.retrieve(f64, frames, 10 * len(f64), 1.0 / 30.0)
    assert c["entries"].tolist() == r["entries"].tolist() == want
    assert c["scores"].tobytes() == r["scores"].tobytes()
    assert c["rejected"] == r["rejected"]


def test_gates(rs):
    scores = np.array(RANK_CASES["four_peaks_keep_three"] + [0.9] * 60, np.float64)
    n = len(scores)
    frames = np.arange(n, dtype=np.int64) * 3
    # every entry gated out: by the key-frame gap, then by time
    for kw, spf in ((dict(min_keyframe_gap=n + 1), 1.0), (dict(), 1e-3)):
        e, s = B.score_candidates(scores, frames, 3 * n, spf, **kw)
        assert len(e) == 0
        r = B.retrieve(scores, frames, 3 * n, spf, **kw)
        c = rs.rank_loop_candidates(scores, frames, 3 * n, spf, **kw)
        assert not len(r["entries"]) and r["rejected"] is None and not len(c["entries"]) and c["rejected"] is None
    # the time gate cuts inside the list: dt = 3 (n - i) / 30 >= 10 only for i <= n - 100
    e, s = B.score_candidates(scores, frames, 3 * n, 1.0 / 30.0)
    want = [i for i in range(n) if n - i >= 50 and float(3 * n - 3 * i) * (1.0 / 30.0) >= 10.0]
    assert e.tolist() == want
    e, s = B.score_candidates(scores, frames, 3 * n, 1.0)
    assert e.tolist() == list(range(n - 49)) and s.dtype == np.float32
    for spf, top in ((1.0, 3), (1.0, 1), (1.0, 5), (0.2, 3)):
        r = B.retrieve(scores, frames, 3 * n, spf, top=top)
        c = rs.rank_loop_candidates(scores, frames, 3 * n, spf, top=top)
        assert c["entries"].tolist() == r["entries"].tolist() and c["scores"].tobytes() == r["scores"].tobytes()
        assert c["rejected"] == r["rejected"]
    assert B.percentile([], 0.5) == 0 and B.percentile([3.0, 1.0, 2.0, 4.0], 0.5) == 2.0
