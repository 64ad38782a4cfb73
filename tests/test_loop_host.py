"""slam::LoopStreak (racing-slam_amd/host/slam_host.cpp) and the host-only C functions rs_loop_best_candidate /
rs_loop_update_streak against the restatement tests/loop_ref.py, over scripted query sequences.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import loop_ref as L

from host_build import build_host_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rs_loop_verifier_create", "rs_loop_verifier_destroy", "rs_map_verify_loop", "rs_loop_verifier_download",
           "rs_loop_best_candidate", "rs_loop_update_streak")


def build_loop_host(rs):
    return build_host_binary(rs, "test_loop_host")


def V(ok, inliers, pose=None):
    return dict(ok=bool(ok), inliers=inliers, pose=np.eye(4, dtype=np.float32) if pose is None else pose,
                query_kp=np.arange(inliers, dtype=np.int32), point=np.arange(inliers, dtype=np.int32) + 100)


# (from, [(candidate index, ok, inliers)]): a streak of three and its constraint; a loop too near it suppressed; an
# unverified query; a skipped query; a jump in the candidate index; nothing ranked; a second constraint far enough away
SEQUENCE = [(60, [(3, 1, 40), (30, 0, 90)]), (61, [(4, 1, 40)]), (62, [(5, 1, 40), (6, 1, 30)]), (63, [(6, 1, 40)]),
            (64, [(7, 0, 80), (8, 0, 10)]), (65, [(7, 1, 40)]), (66, [(8, 1, 40)]), (68, [(9, 1, 40)]), (69, [(10, 1, 40)]),
            (70, [(27, 1, 40)]), (71, [(28, 1, 25), (50, 1, 60)]), (72, []), (80, [(20, 1, 40)]), (81, [(21, 1, 40)]),
            (82, [(22, 1, 40), (23, 1, 40)]), (83, [(38, 1, 99), (24, 1, 20)])]


def _poses():
    rng = np.random.default_rng(3)
    out = []
    for _ in range(2):
        A = np.linalg.qr(rng.normal(0, 1, (3, 3)))[0]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = A * np.sign(np.linalg.det(A)), rng.normal(0, 3, 3)
        out.append(T.astype(np.float32))
    return out


def _reference():
    pose, cand = _poses()
    st, lines = L.LoopState(), []
    for frm, cs in SEQUENCE:
        chosen = L.update_streak(st, frm, [c[0] for c in cs], [V(c[1], c[2], pose) for c in cs], [cand] * len(cs))
        lines.append((chosen, int(st.consume_new_loop()), len(st.streak)))
    return st, lines


def test_library_exports_the_loop_symbols(rs):
    lib = rs.load()
    assert not [s for s in SYMBOLS if not hasattr(lib, s)] and set(SYMBOLS) <= set(rs.EXPORTS)
    assert hasattr(rs.Context, "loop_verifier") and hasattr(rs.LoopVerifier, "verify") and hasattr(rs.LoopVerifier, "download")
    h = C.c_void_p()
    assert lib.rs_loop_verifier_create(None, 100, 3, 200, C.byref(h)) == 1 and not h.value       # RS_ERR_INVALID: nothing without a context
    assert lib.rs_loop_verifier_destroy(None) == 0
    assert lib.rs_map_verify_loop(None, None, None, 0, None, 0, None, 0, 64, C.c_double(4.0), C.c_double(0.99), 200, C.c_uint64(0),
                                  None, None, None, None) == 1


def test_c_functions_follow_the_restatement(rs):
    st, lines = _reference()
    assert [c["from"] for c in st.constraints] == [62, 82] and [c["to"] for c in st.constraints] == [5, 22]
    state, constraints = rs.LoopStreakState(0, 0, 0), []
    for (frm, cs), want in zip(SEQUENCE, lines):
        ver = [V(c[1], c[2]) for c in cs]
        if cs:
            assert rs.loop_best_candidate(ver) == L.best_candidate(ver)
        chosen, new = rs.loop_update_streak(state, frm, [c[0] for c in cs], ver, constraints)
        if new:
            constraints.append((frm, cs[chosen][0]))
        assert (chosen, int(new), state.length) == want, (frm, chosen, new, state.length, want)
    assert constraints == [(62, 5), (82, 22)]
    assert rs.loop_best_candidate([V(0, 50), V(1, 20), V(1, 30), V(1, 30)]) == 2 and rs.loop_best_candidate([V(0, 9), V(0, 9)]) == 0
    assert rs.load().rs_loop_best_candidate(None, 0, None) == 1


def test_python_streak_follows_the_restatement(rs):
    pose, cand = _poses()
    st, lines = _reference()
    mine = rs.LoopStreak()
    for (frm, cs), want in zip(SEQUENCE, lines):
        chosen = mine.update(frm, [c[0] for c in cs], [V(c[1], c[2], pose) for c in cs], [cand] * len(cs))
        assert (chosen, int(mine.consume_new_loop()), mine.state.length) == want
    for c, r in zip(mine.constraints, st.constraints):
        assert (c["from"], c["to"]) == (r["from"], r["to"]) and np.array_equal(c["pairs"], r["pairs"])
        assert np.allclose(c["relative"], r["relative"], rtol=0, atol=1e-5)


def test_cpp_streak_follows_the_restatement(rs, tmp_path):
    exe = build_loop_host(rs)
    pose, cand = _poses()
    st, lines = _reference()
    text = " ".join(repr(float(v)) for v in pose.ravel()) + "\n" + " ".join(repr(float(v)) for v in cand.ravel()) + "\n"
    for frm, cs in SEQUENCE:
        text += f"{frm} {len(cs)} " + " ".join(f"{c[0]} {c[1]} {c[2]}" for c in cs) + "\n"
    (tmp_path / "script.txt").write_text(text)
    r = subprocess.run([exe, str(tmp_path / "script.txt"), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    got = (tmp_path / "out.txt").read_text().strip().split("\n")
    assert len(got) == len(SEQUENCE) + len(st.constraints)
    for line, want in zip(got, lines):
        assert tuple(int(v) for v in line.split()) == want
    for line, c in zip(got[len(SEQUENCE):], st.constraints):
        t = line.split()
        assert (int(t[0]), int(t[1]), int(t[2])) == (c["from"], c["to"], len(c["pairs"]))
        assert np.allclose(np.array([float(v) for v in t[3:]]).reshape(4, 4), c["relative"], rtol=0, atol=1e-5)
