"""Loop verification on the GPU (csrc/loop.hip: rs_loop_verifier_*, rs_map_verify_loop) against the CPU restatement
tests/loop_ref.py.

Exact layer: the gathered rows, slots, keypoints and their number equal loop_ref.candidate_rows applied to the mirror;
the match lists equal match_ref; the verdict record and the three listed arrays equal loop_ref.finish applied to the
GPU's own pose and inlier list — integers exactly, spread / drift / gap bit for bit.
End to end against loop_ref.verify_pnp on the same scene, by test_gpu_pnp.py's rules: status, correspondences and ok are
equal, the pose agrees to atol 1e-5 and the inlier lists are equal outside the near-threshold band (|e^2 - thr^2| <= 1e-9
thr^2 of the restatement's final model; tests/test_loop_cpu.py checks without a GPU that at most 3 correspondences lie in
it and that no bound of the verdict is that close to flipping).
"""
import numpy as np
import pytest

import bow_ref as B
import loop_cases as S
import loop_ref as L
from loop_checks import Built, _check, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built(ctx, rs):
    b = {name: Built(ctx, rs, S.scene(name)) for name in S.SCENES}
    yield b
    for v in b.values():
        v.close()


@pytest.fixture(scope="module")
def ver(ctx):
    v = ctx.loop_verifier(2500, 8, 200)
    yield v
    v.close()


def test_every_status_and_verdict(ctx, ver, built):
    """Eight candidates in one call: verified, nt = 0 / 1 / 11 (status 1), all matches wrong (status 2) and the three ways
    ok is false with a pose."""
    b = built["paths"]
    got = ver.verify(b.map, b.s["query"], list(range(8)), b.s["K"], b.s["width"])
    assert [(g["status"], g["ok"]) for g in got] == S.EXPECT["paths"]
    _check(ver, b, list(range(8)), got, S.reference("paths"))
    assert [ver.download(c)["nt"] for c in (1, 2, 3)] == [0, 1, 11]


def test_compaction_across_chunks(ctx, ver, built):
    b = built["big"]
    got = ver.verify(b.map, b.s["query"], [0, 1], b.s["K"], b.s["width"])
    assert ver.download(0)["nt"] == 1100 and got[0]["ok"] and got[1]["ok"]
    _check(ver, b, [0, 1], got, S.reference("big"))


def test_call_forms_are_deterministic(ctx, ver, built):
    """1 and 3 candidates, a duplicated candidate, both issue forms and a repeated call: the same bytes per candidate."""
    b = built["paths"]
    args = (b.s["K"], b.s["width"])
    eight = ver.verify(b.map, b.s["query"], list(range(8)), *args)
    one = ver.verify(b.map, b.s["query"], [6], *args)
    _check(ver, b, [6], one, S.reference("paths"))
    _same(one, [eight[6]])
    three = ver.verify(b.map, b.s["query"], [5, 0, 5], *args)
    _check(ver, b, [5, 0, 5], three, S.reference("paths"))
    _same(three, [eight[5], eight[0], eight[5]])
    ctx.set_int("loop_verify_streams", 1)
    try:
        other_form = ver.verify(b.map, b.s["query"], list(range(8)), *args)
        _check(ver, b, list(range(8)), other_form, S.reference("paths"))
        other3 = ver.verify(b.map, b.s["query"], [5, 0, 5], *args)
    finally:
        ctx.set_int("loop_verify_streams", 0)
    _same(other_form, eight)
    _same(other3, three)
    _same(ver.verify(b.map, b.s["query"], list(range(8)), *args), eight)
    other = ver.verify(b.map, b.s["query"], [0], *args, seed=5)             # the seed reaches PnP
    assert other[0]["status"] == 0 and other[0]["correspondences"] == eight[0]["correspondences"]


def test_a_map_edit_is_seen(ctx, rs, ver):
    b = Built(ctx, rs, S.synth().loop_scene(7, 300, ((300, 150, 60, 0.2, None),)))
    try:
        args = (b.map, 1, [0], b.s["K"], b.s["width"])
        before = ver.verify(*args)
        _check(ver, b, [0], before)
        rows = L.candidate_rows(b.kp_point[0])
        gone = int(b.kp_point[0][rows[3]])
        b.map.remove_point(gone)
        b.kp_point[0][rows[3]] = -1
        _check(ver, b, [0], ver.verify(*args))
        assert ver.download(0)["nt"] == len(rows) - 1
        free = np.flatnonzero(b.kp_point[0] < 0)
        new = b.map.add_point([1.0, 2.0, 30.0])
        b.pos = np.concatenate([b.pos, np.array([[1.0, 2.0, 30.0]], np.float32)])
        for kp in free[:2]:
            b.map.add_observation(new, 0, int(kp))                          # the second moves the observation: one per key frame
        b.kp_point[0][free[1]] = new
        _check(ver, b, [0], ver.verify(*args))
        d = ver.download(0)
        assert d["nt"] == len(rows) and new in d["slots"] and gone not in d["slots"]
        b.map.set_position(new, [2.0, 2.0, 31.0])                           # positions alone
        b.pos[new] = (2.0, 2.0, 31.0)
        _check(ver, b, [0], ver.verify(*args))
    finally:
        b.close()


def test_errors_leave_the_context_usable(ctx, rs, ver, built):
    b = built["paths"]
    K, w, q = b.s["K"], b.s["width"], b.s["query"]
    assert ver.verify(b.map, q, [], K, w) == []
    # n_candidates == 0 writes nothing: sentinel-filled outputs stay as they are, and null outputs are accepted
    import ctypes as C
    res = (rs.LoopResult * 2)()
    C.memset(res, 0x5A, C.sizeof(res))
    listed = [np.full((2, ver.max_points), 0x5A5A5A5A, np.int32) for _ in range(3)]
    Kc = (C.c_float * 4)(*[float(v) for v in K])
    call = lambda *out: ctx.lib.rs_map_verify_loop(ctx.h, ver.h, b.map.h, int(q), None, 0, Kc, int(w), 64, C.c_double(4.0),       # noqa: E731
                                                   C.c_double(0.99), 200, C.c_uint64(0), *out)
    assert call(res, *[a.ctypes.data_as(C.c_void_p) for a in listed]) == 0
    assert bytes(res) == b"\x5a" * C.sizeof(res) and all((a == 0x5A5A5A5A).all() for a in listed)
    assert call(None, None, None, None) == 0
    good = ver.verify(b.map, q, [0], K, w)
    for cands in ([q], [0, q], [99], [-1], list(range(8)) + [0]):
        with pytest.raises(rs.RsError, match="status 1"):
            ver.verify(b.map, q, cands, K, w)
    with pytest.raises(rs.RsError, match="status 1"):
        ver.verify(b.map, 99, [0], K, w)
    with pytest.raises(rs.RsError, match="status 4"):
        ver.verify(b.map, q, [0], K, w, max_hypotheses=201)
    small = ctx.loop_verifier(299, 2, 50)                                   # the query has 300 keypoints, candidate 0 has 400
    with pytest.raises(rs.RsError, match="status 1"):
        small.verify(b.map, q, [1], K, w, max_hypotheses=50)
    small.close()
    for mp, mc, mh in ((0, 1, 1), (8193, 1, 1), (10, 0, 1), (10, 9, 1), (10, 1, 0), (10, 1, 4097)):
        with pytest.raises(rs.RsError, match="status 4"):
            ctx.loop_verifier(mp, mc, mh)
    _same(ver.verify(b.map, q, [0], K, w), good)
    with pytest.raises(rs.RsError, match="status 1"):
        ver.download(1)


def test_retrieval_verification_streak_chain(ctx, rs, synth):
    """A synthetic lap: key frames 0 .. 52 see places 0 .. 52, key frames 53, 54, 55 see places 1, 2, 3 again.  Retrieval
    ranks the first visit, the verifier verifies it, and the third consecutive verified query yields ONE constraint."""
    voc = synth.make_vocabulary(10, 3, seed=3)
    rng = np.random.default_rng(11)
    leaves = np.flatnonzero(voc["leaf"])
    n_rows, n_kf = 160, 56
    scenes = {53 + i: synth.loop_scene(20 + i, n_rows, ((n_rows, 120, 100, 0.2, None),), flip=0.01) for i in range(3)}
    rows_of = []
    for kf in range(53):
        rows_of.append(synth.flip_bits(rng, voc["desc"][leaves[rng.integers(0, len(leaves), n_rows)]], 0.02))
    for i in range(3):                                                      # place 1 + i carries its scene's candidate rows
        sc = scenes[53 + i]
        sh_q, sh_c, _ = sc["shared"][0]
        sc["key_frames"][0]["desc"] = rows_of[1 + i]
        qd = synth.flip_bits(rng, voc["desc"][leaves[rng.integers(0, len(leaves), n_rows)]], 0.02)
        qd[sh_q] = synth.flip_bits(rng, rows_of[1 + i][sh_c], 0.01)
        sc["key_frames"][1]["desc"] = qd
        rows_of.append(qd)
    gvoc = ctx.vocabulary(voc["k"], voc["L"], B.TF_IDF, B.L1_NORM, voc["parent"], voc["desc"], voc["weight"])
    bow, db = ctx.bow(gvoc, 256), ctx.bow_database(gvoc, n_kf, 256 * n_kf)
    m, ver, streak, ref = rs.ResidentMap(ctx), ctx.loop_verifier(256, 3, 200), rs.LoopStreak(), L.LoopState()
    frames, poses, kps, kp_point, pos = [], [], [], [], np.zeros((0, 3), np.float32)
    frame_index = 10 * np.arange(n_kf, dtype=np.int64)
    K = scenes[53]["K"]
    try:
        for kf in range(n_kf):
            sc = scenes.get(kf)
            src = sc["key_frames"][1] if sc else (scenes[52 + kf]["key_frames"][0] if 1 <= kf <= 3 else None)
            kp = src["kp"] if src else rng.uniform(0, 700, (n_rows, 2)).astype(np.float32)
            pose = src["pose"] if src else np.eye(4, dtype=np.float32)
            frames.append(rs.ResidentFrame(ctx, kp, rows_of[kf]))
            assert m.add_keyframe(frames[-1], pose) == kf
            poses.append(pose)
            kps.append(kp)
            kp_point.append(np.full(n_rows, -1, np.int32))
            if 1 <= kf <= 3:                                                # the candidate's points and observations
                sc, base = scenes[52 + kf], len(pos)
                for xyz in sc["points"]:
                    m.add_point(xyz)
                pos = np.concatenate([pos, sc["points"]])
                for p, _, i in sc["observations"]:
                    m.add_observation(base + p, kf, i)
                    kp_point[kf][i] = base + p
            bow.transform(ctx.dev(rows_of[kf]), ctx.dev(np.array([n_rows], np.int32)), n_rows, words=False)
            assert db.add(bow) == kf
            if kf < 53:
                continue
            scores = db.score(bow, 0, kf).cpu().numpy()
            ranked = rs.rank_loop_candidates(scores, frame_index[:kf], frame_index[kf], 1.0 / 30.0)
            ent = ranked["entries"].tolist()
            assert ent and ent[0] == kf - 52, (kf, ranked)
            got = ver.verify(m, kf, ent, K, 1280)
            mirror = lambda i: dict(desc=rows_of[i], kp=kps[i], kp_point=kp_point[i], pose=poses[i])      # noqa: E731
            want = [L.verify_pnp(mirror(kf), mirror(e), pos, K, 1280) for e in ent]
            assert [(g["status"], g["ok"], g["correspondences"]) for g in got] == [(r["status"], r["ok"], r["correspondences"]) for r in want]
            assert got[0]["ok"]
            chosen = streak.update(kf, ent, got, [poses[e] for e in ent])
            assert chosen == L.update_streak(ref, kf, ent, want, [poses[e] for e in ent]) == 0
            assert streak.consume_new_loop() == ref.consume_new_loop() == (kf == 55)
        assert len(streak.constraints) == len(ref.constraints) == 1
        c, r = streak.constraints[0], ref.constraints[0]
        assert (c["from"], c["to"]) == (r["from"], r["to"]) == (55, 3)
        assert np.allclose(c["relative"], r["relative"], rtol=0, atol=1e-5)
        assert len(c["pairs"]) == got[0]["inliers"] and set(c["pairs"][:, 1]) <= set(kp_point[3][kp_point[3] >= 0])
    finally:
        ver.close(); m.close(); bow.close(); db.close(); gvoc.close()
        for f in frames:
            f.close()
