"""slam::LoopRetrieval (racing-slam_amd/host/slam_host.cpp) — the C++ host-side form of LoopDetector::query's "Loop
retrieval" stage — built against librsgpu and checked against the restatement tests/bow_ref.py; the vocabulary's text
loader round trip; and the new symbols of the C ABI without a GPU."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import bow_ref as B

from host_build import build_host_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rs_vocabulary_create", "rs_vocabulary_load_text", "rs_vocabulary_info", "rs_vocabulary_arrays", "rs_vocabulary_destroy",
           "rs_bow_create", "rs_bow_destroy", "rs_bow_transform", "rs_bow_download", "rs_bow_database_create",
           "rs_bow_database_destroy", "rs_bow_database_add", "rs_bow_database_score", "rs_bow_database_counts",
           "rs_rank_loop_candidates")


def build_bow_host(rs):
    return build_host_binary(rs, "test_bow_host")


def test_library_exports_the_bow_symbols(rs):
    lib = rs.load()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert set(SYMBOLS) <= set(rs.EXPORTS)
    assert all(hasattr(rs.Context, m) for m in ("vocabulary", "vocabulary_from_text", "bow", "bow_database"))
    assert hasattr(rs.Bow, "transform") and hasattr(rs.BowDatabase, "score") and hasattr(rs, "rank_loop_candidates")


def test_nothing_without_a_context(rs):
    lib = rs.load()
    h = C.c_void_p()
    assert lib.rs_vocabulary_create(None, 3, 2, 0, 0, 13, None, None, None, C.byref(h)) == 1 and not h.value   # RS_ERR_INVALID
    assert lib.rs_vocabulary_load_text(None, b"nowhere", C.byref(h)) == 1 and not h.value
    assert lib.rs_bow_create(None, None, 100, C.byref(h)) == 1 and not h.value
    assert lib.rs_bow_database_create(None, None, 10, 10, C.byref(h)) == 1 and not h.value
    assert lib.rs_bow_transform(None, None, None, None, 0, None) == 1
    assert lib.rs_vocabulary_destroy(None) == 0 and lib.rs_bow_destroy(None) == 0 and lib.rs_bow_database_destroy(None) == 0


def test_bow_host_mirror_compiles(rs):
    assert os.path.exists(build_bow_host(rs))


def make_sequence(synth, n_kf=120, revisit_from=100, rows=160, seed=0):
    """Key frames along a path of places: place p sees leaves seq[12 p .. 12 p + rows), so neighbours share most of their
    words; key frames revisit_from .. n_kf-1 see places 0, 1, ... again.  Rows are noisy copies of those leaves."""
    voc = synth.make_vocabulary(10, 3, seed=3, stopped_fraction=0.05)
    rng = np.random.default_rng([0xB2, seed])
    leaves = np.flatnonzero(voc["leaf"])
    seq = leaves[rng.integers(0, len(leaves), 12 * n_kf + rows)]
    desc = np.zeros((n_kf, rows, 32), np.uint8)
    counts = np.zeros(n_kf, np.int32)
    for q in range(n_kf):
        place = q if q < revisit_from else q - revisit_from
        desc[q] = synth.flip_bits(rng, voc["desc"][seq[12 * place:12 * place + rows]], 0.03)
        counts[q] = rows - int(rng.integers(0, 20))
    frames = np.cumsum(rng.integers(4, 15, n_kf)).astype(np.int64)
    return voc, desc, counts, frames


@pytest.mark.gpu
def test_loop_retrieval_matches_the_restatement(rs, tmp_path):
    exe = build_bow_host(rs)
    synth = importlib.import_module("racing-slam_amd").synth
    voc, desc, counts, frames = make_sequence(synth)
    n_kf, rows, spf = len(desc), desc.shape[1], 1.0 / 30.0
    V = B.Vocabulary(voc["k"], voc["L"], B.TF_IDF, B.L1_NORM, voc["parent"], voc["desc"], voc["weight"])
    B.write_text(V, tmp_path / "voc.txt")
    (tmp_path / "meta.txt").write_text(f"{n_kf} {rows} {float(np.float32(spf))!r}\n")
    frames.tofile(str(tmp_path / "frames.i64"))
    counts.tofile(str(tmp_path / "counts.i32"))
    desc.tofile(str(tmp_path / "desc.u8"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    # the text file read back: the arrays exactly
    assert [int(v) for v in (tmp_path / "info.txt").read_text().split()] == [V.k, V.L, V.weighting, V.scoring, V.n_nodes, V.n_words]
    assert np.array_equal(np.fromfile(str(tmp_path / "parent.i32"), np.int32), V.parent)
    assert np.array_equal(np.fromfile(str(tmp_path / "nodes.u8"), np.uint8).reshape(-1, 32), V.desc)
    assert np.array_equal(np.fromfile(str(tmp_path / "weight.f64"), np.float64), V.weight)
    # every query against score_candidates + rank_candidates
    vec = [B.transform(V, desc[q, :counts[q]]) for q in range(n_kf)]
    lines = (tmp_path / "out.txt").read_text().strip().split("\n")
    assert len(lines) == n_kf
    ranked_total = 0
    for q, line in enumerate(lines):
        t = line.split()
        assert int(t[0]) == q
        ent = [int(v) for v in t[2::2]]
        sc = np.array([int(v, 16) for v in t[3::2]], np.uint32).view(np.float32)
        assert len(ent) == int(t[1])
        scores = np.array([B.score(vec[q], vec[i]) for i in range(q)]) if q >= B.MIN_KEYFRAME_GAP else np.zeros(q)
        ref = B.retrieve(scores, frames[:q], frames[q], np.float32(spf))
        assert ent == ref["entries"].tolist(), (q, ent, ref)
        assert np.allclose(sc, ref["scores"], rtol=0, atol=1e-6)
        ranked_total += len(ent)
    # the revisit is found: the key frames that see places 0 .. 19 again rank their first visit on top
    assert ranked_total >= 15
    hits = [int(line.split()[2]) for line in lines[100:] if int(line.split()[1])]
    assert len(hits) >= 15 and all(abs(h - k) <= 2 for h, k in zip(hits, range(20)))
