"""rs_map_fuse_loop on the GPU against the restatement (tests/fuse_ref.py), with the call's self-check on.

Everything is compared for exact equality: the old frames, the sources, every journal section with its outcomes, the
removed points, device_state_mismatches == 0, rs_map_counts, the observations of every slot in insertion order and every
key frame's table.  Afterwards rs_map_match and rs_map_match_frame on the fused map equal the same calls on a second
rs_map built from the restatement's edited model: the flag tables came back clean and the image follows the edits.
The cases and the branches they reach are asserted on the CPU in tests/test_fuse_cpu.py.
"""
import numpy as np
import pytest

import fuse_cases
import fuse_ref

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = 4, 1


def build_map(ctx, rs, model):
    """an rs_map holding the model's state: key frames, every slot (dead ones added and removed), observations in order"""
    m = rs.ResidentMap(ctx)
    for kf in range(model.n_kf()):
        f = rs.ResidentFrame(ctx, model.kf_kp[kf].reshape(-1, 2), model.kf_desc[kf].reshape(-1, 32))
        assert m.add_keyframe(f, model.kf_pose[kf]) == kf
        f.close()
    for p in range(model.n_slots()):
        assert m.add_point(model.pos[p]) == p
        for kf, kp in model.obs[p]:
            m.add_observation(p, kf, kp)
        if not model.alive[p]:
            m.remove_point(p)
    return m


def assert_state(m, model, what=""):
    assert m.counts() == model.counts(), what
    for p in range(model.n_slots()):
        assert m.observations(p) == [(int(a), int(b)) for a, b in model.obs[p]], (what, "observations of slot", p)
    for kf in range(model.n_kf()):
        assert np.array_equal(m.keyframe_matches(kf), model.kp_point[kf]), (what, "table of key frame", kf)


def probe(ctx, rs, m, model, c, kf):
    """match_map of a fresh frame with key frame kf's keypoints against map m: (matches, table after match_frame)"""
    cam = c["camera"]
    f = rs.ResidentFrame(ctx, model.kf_kp[kf].reshape(-1, 2), model.kf_desc[kf].reshape(-1, 32))
    mk, mp = m.match(f, model.kf_pose[kf], cam["K"], cam["width"], cam["height"])
    n = m.match_frame(f, model.kf_pose[kf], cam["K"], cam["width"], cam["height"])
    tab = f.matches()[0].copy()
    f.close()
    return mk.tolist(), mp.tolist(), n, tab.tolist()


def call(m, c, **kw):
    cam, o = c["camera"], c["options"]
    args = dict(max_distance=o["max_distance"], min_shared=o["min_shared"], max_covisible=o["max_covisible"], check=True)
    args.update(kw)
    return m.fuse_loop(c["query"], c["candidate"], c["inliers"], c["window"], cam["K"], cam["width"], cam["height"], **args)


def run_ref(c):
    return fuse_ref.fuse_loop(c["model"], c["query"], c["candidate"], c["inliers"], c["window"], c["camera"], **c["options"])


def check_case(ctx, rs, c, keep=False, ref=None, **kw):
    ref = run_ref(c) if ref is None else ref
    m = build_map(ctx, rs, c["model"])
    got = call(m, c, **kw)
    what = c["name"]
    assert got["old_frames"] == ref["old_frames"], what
    assert got["sources"].tolist() == ref["sources"], what
    if kw.get("journal", True) and kw.get("capacity") is None:
        assert got["sections"] == ref["journal"], what
    total = sum(len(s) for s in ref["journal"])
    assert got["n_entries"] == total, what
    assert got["removed"].tolist() == ref["removed"], what
    assert got["outcomes"] == [sum(oc == k for s in ref["journal"] for _, _, oc in s) for k in range(6)], what
    assert got["device_state_mismatches"] == 0, what
    assert_state(m, ref["model"], what)
    m2 = build_map(ctx, rs, ref["model"])
    for kf in (c["query"], c["candidate"]):
        assert probe(ctx, rs, m, ref["model"], c, kf) == probe(ctx, rs, m2, ref["model"], c, kf), (what, "later matches", kf)
    m2.close()
    if keep:
        return m, ref, got
    m.close()
    return None, ref, got


@pytest.mark.parametrize("make", [fuse_cases.general, fuse_cases.inlier_branches, fuse_cases.empty_candidate, fuse_cases.dependence,
                                  fuse_cases.many_matches, fuse_cases.window_sizes], ids=lambda f: f.__name__)
def test_fuse_loop_equals_the_restatement(ctx, rs, make):
    check_case(ctx, rs, make())


def test_covisibility_threshold_cut_and_tie(ctx, rs):
    c, _ = fuse_cases.covisibility()
    _, ref, _ = check_case(ctx, rs, c)
    assert len(ref["old_frames"]) == 21
    c["options"]["max_covisible"] = 0
    _, ref, _ = check_case(ctx, rs, c)
    assert ref["old_frames"] == [0]


@pytest.mark.parametrize("S", [0, 1, 63, 64, 65, 257])
def test_source_counts(ctx, rs, S):
    _, ref, _ = check_case(ctx, rs, fuse_cases.source_count(S))
    assert len(ref["sources"]) == S


def test_a_key_frame_beyond_the_lds_tree(ctx, rs):
    """6145 keypoints: K2 walks the tree in global memory"""
    check_case(ctx, rs, fuse_cases.window_sizes(big=6145))


def test_window_forms(ctx, rs):
    c = fuse_cases.general(21)
    old = run_ref(c)["old_frames"]
    for window in ([], old[1:3], [c["query"]]):
        check_case(ctx, rs, dict(c, window=window, name=f"window {window}"))


def test_journal_arrays_too_small_or_absent_edit_the_map_identically(ctx, rs):
    c = fuse_cases.general(11)
    ref = run_ref(c)
    total = sum(len(s) for s in ref["journal"])
    _, _, got = check_case(ctx, rs, c, ref=ref, capacity=total - 1)
    flat = [e for s in ref["journal"] for e in s]
    assert [e for s in got["sections"] for e in s] == flat[:total - 1]
    _, _, got = check_case(ctx, rs, c, ref=ref, journal=False)
    assert got["sections"] is None and got["n_entries"] == total


def test_refusals_leave_the_map_unchanged(ctx, rs):
    c = fuse_cases.general(11)
    model = c["model"]
    big = model.add_keyframe(np.random.default_rng(0).uniform(0, 400, (8193, 2)).astype(np.float32), np.zeros((8193, 32), np.uint8),
                             model.kf_pose[0])[0]
    m = build_map(ctx, rs, model)
    before = probe(ctx, rs, m, model, c, c["query"])
    n_kf = model.n_kf()
    bad = [(dict(c, query=-1), INVALID), (dict(c, query=n_kf), INVALID), (dict(c, candidate=n_kf), INVALID),
           (dict(c, window=c["window"] + [n_kf + 3]), INVALID), (dict(c, window=c["window"] + c["window"][:1]), INVALID),
           (dict(c, window=list(range(n_kf)) * 3), INVALID),                      # listed twice comes before the envelope
           (dict(c, window=c["window"] + [big]), UNSUPPORTED), (dict(c, query=big), UNSUPPORTED),
           (dict(c, inliers=[(0, 0)] * 8193), UNSUPPORTED),
           (dict(c, options=dict(c["options"], max_covisible=65)), UNSUPPORTED), (dict(c, options=dict(c["options"], max_covisible=-1)), UNSUPPORTED)]
    for cc, status in bad:
        assert call(m, cc, raise_on_error=False)["status"] == status
        assert_state(m, model, "after a refusal")
    # a null argument on the live map, through the library itself (the binding always supplies these)
    import ctypes as C
    lib, ptr = rs.load(), lambda x: x.ctypes.data_as(C.c_void_p)
    cam, o = c["camera"], c["options"]
    opt = rs.FuseOptions(width=cam["width"], height=cam["height"], max_distance=o["max_distance"], min_shared=o["min_shared"],
                         max_covisible=o["max_covisible"], check=1)
    for i in range(4):
        opt.intrinsics[i] = cam["K"][i]
    rep, n = rs.FuseReport(), C.c_int(0)
    ik, ip = (np.ascontiguousarray([e[k] for e in c["inliers"]], np.int32) for k in (0, 1))
    win = np.ascontiguousarray(c["window"], np.int32)
    assert len(ik) > 0 and len(win) > 0
    good = [ctx.h, m.h, c["query"], c["candidate"], ptr(ik), ptr(ip), len(ik), ptr(win), len(win), C.byref(opt), C.byref(rep),
            None, None, None, None, 0, C.byref(n)]
    for null in (0, 1, 4, 5, 7, 9, 10):             # context, map, inlier keypoints, inlier points, window, options, report
        args = list(good)
        args[null] = None
        assert lib.rs_map_fuse_loop(*args) == INVALID, null
        assert_state(m, model, "after a null argument")
    assert probe(ctx, rs, m, model, c, c["query"]) == before
    other = rs.Context(0)
    mine, m.ctx = m.ctx, other                      # a map of another context
    assert call(m, c, raise_on_error=False)["status"] == INVALID
    m.ctx = mine
    other.close()
    assert_state(m, model, "after a refusal")
    assert probe(ctx, rs, m, model, c, c["query"]) == before
    m.close()


def test_window_envelope(ctx, rs):
    """65 distinct window key frames are outside the envelope, 64 are inside"""
    b = fuse_cases.Builder(5, 66)
    for kf in range(66):
        b.pad(kf, 4)
    c = fuse_cases.case("envelope", b, 65, 0, [], list(range(1, 66)))
    m = build_map(ctx, rs, c["model"])
    assert call(m, c, raise_on_error=False)["status"] == UNSUPPORTED
    assert call(m, dict(c, window=list(range(2, 66))))["n_entries"] == 0
    m.close()


def test_reuse_after_an_insertion_chain(ctx, rs):
    """a second fuse on the same map with another candidate, then Mapper::insert's chain on the fused map (match_frame,
    rs_map_insert_keyframe, rs_map_add_track_points, rs_map_reanchor, rs_map_cull_points: the users of d_flag and of the
    image the fuse left dirty) held against the same chain on a map rebuilt from the restatement, then a third fuse: the
    scratch is reused after edits and the tables came back clean"""
    import keyframe_ref as R
    c = fuse_cases.general(23)
    cam = c["camera"]
    m, ref, _ = check_case(ctx, rs, c, keep=True)
    c2 = dict(c, model=ref["model"], candidate=1, inliers=[], name="second fuse")
    ref2 = run_ref(c2)
    got = call(m, c2)
    assert got["sections"] == ref2["journal"] and got["old_frames"] == ref2["old_frames"] and got["device_state_mismatches"] == 0
    model = ref2["model"]
    assert_state(m, model, "second fuse")
    m2 = build_map(ctx, rs, model)
    # the new frame: the query's keypoints a quarter pixel on, under the query's pose
    q = c["query"]
    kp, desc, pose = model.kf_kp[q] + np.float32(0.25), model.kf_desc[q], model.kf_pose[q]
    rng = np.random.default_rng(9)
    window = list(c["window"])
    before = np.stack([R.perturb_pose(model.kf_pose[k], rng) for k in window] + [R.perturb_pose(pose, rng)])
    kf_model = model.add_keyframe(kp, desc, pose)[0]
    chain, res = [], None
    for mm in (m, m2):
        f = rs.ResidentFrame(ctx, kp, desc)
        matched = mm.match_frame(f, pose, cam["K"], cam["width"], cam["height"])
        table = f.matches()[0].copy()
        kf, adopted = mm.insert_keyframe(f, pose)
        f.close()
        if res is None:                                 # the model follows the first map; the second must repeat it
            assert kf == kf_model and matched > 20 and R.adopt(model, kf, table) == adopted
            # twelve accepted tracks at free keypoints; sighting pairs in and outside the window, at free and taken keypoints,
            # without a handle and of the key frame itself
            acc = rng.choice(np.flatnonzero(model.kp_point[kf] < 0), 12, replace=False).astype(np.int32)
            ptr, pairs = [0], []
            for _ in acc:
                for _ in range(int(rng.integers(0, 5))):
                    h = int(rng.choice([-1, kf] + list(range(model.n_kf()))))
                    pairs.append((h, int(rng.integers(len(model.kf_kp[max(h, 0)])))))
                ptr.append(len(pairs))
            res = dict(keypoint=acc, xyz=(rng.normal(0, 0.5, (12, 3)) + [0, 0, 6]).astype(np.float32), sightings=rng.integers(1, 6, 12).astype(np.int32),
                       kf_ptr=np.array(ptr, np.int32), kf_pairs=np.array(pairs, np.int32).reshape(-1, 2), n_pairs=len(pairs))
            created = R.add_track_points(model, kf, res, window)[0]
        new = mm.add_track_points(kf, res, window)
        moved = mm.reanchor(window + [kf], before)
        culled = mm.cull_points(window + [kf], cam["K"], apply=True)
        chain.append((matched, table.tolist(), kf, adopted, new.tolist(), moved[0], moved[1].tolist(), moved[2].tobytes(),
                      culled["n_removed"], culled["n_local"], culled["removed"].tolist(), culled["xyz"].tobytes()))
    assert chain[0] == chain[1], "the chain on the fused map differs from the chain on the rebuilt map"
    # the chain did work: something moved, and the cull saw at least what the new key frame alone observes
    assert chain[0][4] == list(created) and chain[0][5] > 0 and chain[0][9] >= chain[0][3] + len(created) > 30
    for p, x in zip(chain[0][6], np.frombuffer(chain[0][7], np.float32).reshape(-1, 3)):
        model.set_position(p, x)
    for p in chain[0][10]:
        model.remove_point(p)
    for mm in (m, m2):
        assert_state(mm, model, "after the insertion chain")
        assert mm.positions().tobytes() == model.positions().tobytes()
    c3 = dict(c2, model=model, candidate=2, window=window + [kf_model], name="third fuse")
    ref3 = run_ref(c3)
    got = call(m, c3)
    assert got["sections"] == ref3["journal"] and got["old_frames"] == ref3["old_frames"] and got["device_state_mismatches"] == 0
    assert_state(m, ref3["model"], "third fuse")
    m3 = build_map(ctx, rs, ref3["model"])
    assert probe(ctx, rs, m, ref3["model"], c3, kf_model) == probe(ctx, rs, m3, ref3["model"], c3, kf_model)
    for mm in (m, m2, m3):
        mm.close()


def grown_between_fuses(c, model):
    """The edits between the two fuses of the test below, on the model: a key frame of 1000 keypoints that alone observes 900
    new points, then 4100 slots nothing observes.  Returns the calls that make them on an rs_map: (op, arguments)."""
    rng = np.random.default_rng(5)
    kp = np.stack([rng.uniform(5, 635, 1000), rng.uniform(5, 475, 1000)], 1).astype(np.float32)
    desc = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    kf = model.add_keyframe(kp, desc, model.kf_pose[c["query"]])[0]
    calls = [("add_keyframe", kp, desc, model.kf_pose[kf])]
    for i in range(5000):
        xyz = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(5, 7)], np.float32)
        p = model.create_point(xyz, [(kf, i)] if i < 900 else [])[0]
        calls.append(("add_point", xyz, [(p, kf, i)] if i < 900 else []))
    return calls


def test_the_scratch_is_outgrown_between_two_fuses(ctx, rs):
    """The first fuse, with one window frame on a map of 153 slots, makes the three scratch arrays at their first sizes: the
    prologue's KF + 68 + P = 231 words in 4096, the 3 P + 8192 = 8651 bytes in 16384 and stage 3's 4135 words in 8192.  The
    map then grows (grown_between_fuses) and a second fuse, with another candidate and the whole window, needs each of them
    larger: 5232 words, 23651 bytes, and through the 900 new observations more than 10000 words in stage 3."""
    c = fuse_cases.general(23)
    m, ref, _ = check_case(ctx, rs, dict(c, window=c["window"][:1], name="first fuse"), keep=True)
    model = ref["model"]
    for call_ in grown_between_fuses(c, model):
        if call_[0] == "add_keyframe":
            f = rs.ResidentFrame(ctx, call_[1], call_[2])
            m.add_keyframe(f, call_[3])
            f.close()
        else:
            m.add_point(call_[1])
            for p, kf, kp in call_[2]:
                m.add_observation(p, kf, kp)
    assert_state(m, model, "grown")
    c2 = dict(c, model=model, candidate=1, inliers=[], name="second fuse")
    ref2 = run_ref(c2)
    got = call(m, c2)
    assert got["sections"] == ref2["journal"] and got["old_frames"] == ref2["old_frames"] and got["sources"].tolist() == ref2["sources"]
    assert got["device_state_mismatches"] == 0 and got["n_entries"] > 0
    assert_state(m, ref2["model"], "second fuse")
    m2 = build_map(ctx, rs, ref2["model"])
    for kf in (c["query"], 1):
        assert probe(ctx, rs, m, ref2["model"], c, kf) == probe(ctx, rs, m2, ref2["model"], c, kf)
    m2.close()
    m.close()


def test_fuse_points_equals_the_model(ctx, rs):
    """rs_map_fuse_points is Map::fuse: pairs that share observers, pairs that do not, a point with itself, dead slots"""
    c = fuse_cases.general(11)
    model = c["model"]
    m = build_map(ctx, rs, model)
    rng = np.random.default_rng(4)
    for it in range(60):
        alive = model.alive_points()
        kept = int(rng.choice(alive))
        near = [int(p) for kf, _ in model.obs[kept] for p in model.kp_point[kf] if p >= 0 and p != kept]
        gone = int(rng.choice(near)) if near and it % 3 else int(rng.choice(alive))
        model.fuse(kept, gone)
        m.fuse_points(kept, gone)
    assert model.consistent() and model.counts()["alive"] < model.counts()["slots"] - 40
    assert_state(m, model, "after 60 fuses")
    dead = next(p for p in range(model.n_slots()) if not model.alive[p])
    for kept, gone in ((dead, model.alive_points()[0]), (model.alive_points()[0], dead), (model.n_slots(), 0), (0, -1)):
        with pytest.raises(rs.RsError):
            m.fuse_points(kept, gone)
    assert_state(m, model, "after refused fuses")
    m2 = build_map(ctx, rs, model)
    assert probe(ctx, rs, m, model, c, c["query"]) == probe(ctx, rs, m2, model, c, c["query"])
    m2.close()
    m.close()


@pytest.mark.parametrize("seed", range(20))
def test_soak(ctx, rs, seed):
    check_case(ctx, rs, fuse_cases.soak(seed))
