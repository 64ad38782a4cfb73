"""CPU tests of the loop-fusion restatement (tests/fuse_ref.py) and of the cases (tests/fuse_cases.py).

fuse_ref is held against an independent brute-force formulation: its own graph (dicts and sets, no flags, none of
MapModel's edits), re-flattened from scratch before every frame, matched by the f32 oracle (oracle/reproj_match.c) where
fuse_ref uses the float64 numpy matcher.  Then every case is asserted to reach the branch it is named for, on the
restatement alone: a case that misses its branch fails here, not silently on the GPU.
"""
import copy
from collections import Counter

import numpy as np
import pytest

import fuse_cases
import fuse_ref
from map_model import centre_f32


def brute_fuse_loop(oracle, c):
    m = c["model"]
    obs = {p: list(m.obs[p]) for p in range(m.n_slots()) if m.alive[p]}          # point -> [(kf, kp)]; a dead point has no entry
    table = {(kf, int(kp)): int(p) for kf in range(m.n_kf()) for kp, p in enumerate(m.kp_point[kf]) if p >= 0}
    n_kp = [len(k) for k in m.kf_kp]
    rows = np.cumsum([0] + n_kp)
    pool = np.concatenate(m.kf_desc + [np.zeros((1, 32), np.uint8)])
    centres = np.stack([centre_f32(T) for T in m.kf_pose])
    o = c["options"]
    cand = c["candidate"]
    shared = Counter(kf for (k, _), p in table.items() if k == cand for kf, _ in obs[p] if kf != cand)
    ranked = sorted((kf for kf in shared if shared[kf] >= o["min_shared"]), key=lambda kf: (-shared[kf], kf))
    old_frames = [cand] + ranked[:o["max_covisible"]]
    old_points = {p for (k, _), p in table.items() if k in set(old_frames)}
    removed = []

    def seen_by(p, kf):
        return any(k == kf for k, _ in obs[p])

    def drop(p, kf):
        for k, i in obs[p]:
            if k == kf:
                del table[(k, i)]
        obs[p] = [x for x in obs[p] if x[0] != kf]

    def fuse_match(kf, kp, kept):
        if not (0 <= kp < n_kp[kf]) or kept not in obs:
            return 0
        d = table.get((kf, kp))
        if d is None:
            if seen_by(kept, kf):
                return 2
            obs[kept].append((kf, kp)); table[(kf, kp)] = kept
            return 1
        if d == kept:
            return 3
        if d in old_points:
            return 4
        for k, i in list(obs[d]):
            drop(d, k)
            if not seen_by(kept, k) and (k, i) not in table:
                obs[kept].append((k, i)); table[(k, i)] = kept
        del obs[d]
        removed.append(d)
        return 5

    journal = [[(kp, pt, fuse_match(c["query"], kp, pt)) for kp, pt in c["inliers"]]]
    sources = sorted(old_points)
    for kf in c["window"]:
        journal.append([])
        if kf in old_frames or n_kp[kf] == 0 or not sources:
            continue
        ptr, okf, odesc = [0], [], []
        for p in sources:
            okf += [k for k, _ in obs[p]]
            odesc += [rows[k] + i for k, i in obs[p]]
            ptr.append(len(okf))
        mp = dict(positions=np.array([m.pos[p] for p in sources], np.float32), eligible=np.array([0 if seen_by(p, kf) else 1 for p in sources], np.uint8),
                  obs_ptr=np.array(ptr, np.int32), obs_kf=np.array(okf, np.int32), obs_desc=np.array(odesc, np.int32), kf_centers=centres,
                  desc_pool=pool)
        fr = fuse_ref.frame_dict(m, kf, c["camera"])
        fr["kd_node_kp"], fr["kd_left"], fr["kd_right"], fr["kd_root"] = oracle.kdtree_build(m.kf_kp[kf])
        r = oracle.reproj_match(fr, mp, replace=1, max_distance=o["max_distance"])
        for kp, s in zip(r["match_kp"], r["match_point"]):
            journal[-1].append((int(kp), sources[int(s)], fuse_match(kf, int(kp), sources[int(s)])))
    return dict(old_frames=old_frames, sources=sources, journal=journal, removed=removed, obs=obs, table=table)


def run_ref(c, **kw):
    args = dict(window=c["window"], inliers=c["inliers"])
    args.update(kw)
    return fuse_ref.fuse_loop(c["model"], c["query"], c["candidate"], args["inliers"], args["window"], c["camera"], **c["options"])


def check_against_brute(oracle, c):
    ref, bf = run_ref(c), brute_fuse_loop(oracle, c)
    for k in ("old_frames", "sources", "journal", "removed"):
        assert ref[k] == bf[k], (c["name"], k)
    m = ref["model"]
    assert m.consistent()
    assert {p: m.obs[p] for p in m.alive_points()} == bf["obs"]
    assert {(kf, int(kp)): int(p) for kf in range(m.n_kf()) for kp, p in enumerate(m.kp_point[kf]) if p >= 0} == bf["table"]
    return ref


def outcomes(ref):
    return Counter(oc for sec in ref["journal"] for _, _, oc in sec)


def check_expect(c, ref):
    """the branches the case is named for"""
    oc, want = outcomes(ref), c["expect"]
    for k in range(6):
        if f"o{k}" in want:
            assert oc[k] > 0, (c["name"], f"no entry with outcome {k}", dict(oc))
    if "kept_observed" in want:
        assert any("kept_observed" in t[2] for t in ref["trace"]), c["name"]
    if "blocked_by_fuse" in want:
        after_inliers = run_ref(c, window=[])["model"]
        hit = 0
        for w, kf in enumerate(c["window"]):
            if ref["eligible"][w] is None:
                continue
            for s, p in enumerate(ref["sources"]):
                hit += int(not ref["eligible"][w][s] and after_inliers.observer_kp(p, kf) is None)
        assert hit > 0, (c["name"], "no source made ineligible by an earlier frame's fuse")
    for w in want:
        if w[0] == "s" and w[1:].isdigit():
            assert len(ref["sources"]) == int(w[1:]), (c["name"], len(ref["sources"]))
    if "m300" in want:
        big = [sec for sec, kf in zip(ref["journal"][1:], c["window"]) if len(c["model"].kf_kp[kf]) == 512 and len(sec) >= 300]
        assert big and {1, 4, 5} <= {o for _, _, o in big[0]}, (c["name"], [len(s) for s in ref["journal"]])


CASES = {
    "general": fuse_cases.general,
    "inlier_branches": fuse_cases.inlier_branches,
    "empty_candidate": fuse_cases.empty_candidate,
    "many_matches": fuse_cases.many_matches,
    "window513": fuse_cases.window_sizes,
    "soak0": lambda: fuse_cases.soak(0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_brute_force_and_reaches_its_branches(oracle, name):
    c = CASES[name]()
    check_expect(c, check_against_brute(oracle, c))


@pytest.mark.parametrize("S", [0, 1, 63, 64, 65, 257])
def test_source_counts(oracle, S):
    c = fuse_cases.source_count(S)
    ref = check_against_brute(oracle, c)
    check_expect(c, ref)
    assert ref["old_frames"] == [0]
    if S >= 63:
        assert outcomes(ref)[5] > 0


def test_covisibility_threshold_cut_and_tie(oracle):
    c, counts = fuse_cases.covisibility()
    ref = check_against_brute(oracle, c)
    check_expect(c, ref)
    want = sorted((1 + j for j, n in enumerate(counts) if n >= 15), key=lambda kf: (-counts[kf - 1], kf))
    assert len(want) == 26 and counts[want[19] - 1] == counts[want[20] - 1] == 22 and want[19] < want[20]
    assert ref["old_frames"] == [0] + want[:20]
    for n, kf in ((13, 1), (14, 2)):
        assert counts[kf - 1] == n and kf not in ref["old_frames"]
    # max_covisible = 0: the candidate alone
    c["options"]["max_covisible"] = 0
    assert run_ref(c)["old_frames"] == [0]


def test_dependence_between_window_frames(oracle):
    c = fuse_cases.dependence()
    ref = check_against_brute(oracle, c)
    check_expect(c, ref)
    k, m0, m1 = c["marks"], c["model"], ref["model"]
    sec = {kf: s for kf, s in zip(c["window"], ref["journal"][1:])}
    # a: fused in frame i, absent from frame j, which observed D
    assert any(pt == k["Pa"] and oc == 5 for _, pt, oc in sec[k["i"]]) and all(pt != k["Pa"] for _, pt, _ in sec[k["j"]])
    assert m0.observer_kp(k["Da"], k["j"]) is not None and any(pt == k["Pa"] for _, pt in fuse_ref.frame_matches(m0, k["j"], ref["sources"], c["camera"])[0])
    # b: the match of frame j exists only because of the descriptor gained in frame i
    assert (k["kb"], k["Pb"], 1) in sec[k["j"]]
    assert all(pt != k["Pb"] for _, pt in fuse_ref.frame_matches(m0, k["j"], ref["sources"], c["camera"])[0])
    # c: the row grows from 8 to 9 in frame i and is matched again in frame j
    assert len(m0.obs[k["Pc"]]) == 8 and (k["kc"], k["Pc"], 1) in sec[k["j"]] and len(m1.obs[k["Pc"]]) == 10
    assert m1.obs[k["Pc"]][8][0] == k["i"]
    # d: fewer observations appended than D had
    t = [x for x in ref["trace"] if x[0] == k["Pd"]]
    assert len(t) == 1 and t[0][2] == ["moved", "kept_observed", "kept_observed"]
    assert len(m1.obs[k["Pd"]]) == len(m0.obs[k["Pd"]]) + 1


def test_window_forms(oracle):
    c = fuse_cases.general(21)
    old = run_ref(c)["old_frames"]
    for window in ([], old[1:3], [c["query"]]):
        ref = check_against_brute(oracle, dict(c, window=window))
        assert len(ref["journal"]) == len(window) + 1
        if window and window[0] in old:
            assert all(s == [] for s in ref["journal"][1:])
