"""Loop verification across its envelope (csrc/loop.hip: loop_gather, loop_gate, loop_verdict, the chains' state, the pinned
result block; csrc/map.hip: rs_map_loop_sync, rs_map_loop_keyframe), by tests/test_gpu_loop.py's two layers unchanged
(tests/loop_checks.py).  K1 and PnP have envelopes of their own; this file is about what loop.hip adds around them.

The scenes are loop_cases.ENVELOPE; tests/test_loop_envelope_cpu.py checks without a GPU that each is what its name says and
that loop_cases.decided holds wherever the restatement's ok is demanded here.

What cannot be reached through the public calls: a status 0 with fewer than two listed correspondences (PnP needs four
inliers), so spread's `listed < 2` branch is only taken with status 1 and 2, where spread is not computed at all."""
import types

import numpy as np
import pytest

import keyframe_ref as R
import loop_cases as S
import loop_ref as L
from loop_checks import Built, _bits, _check, _same

pytestmark = pytest.mark.gpu

RECORD = ("status", "ok", "correspondences", "inliers", "listed", "spread", "drift", "gap", "pose", "query_kp", "point", "candidate_kp")


def _view(b, **changes):
    """The same map and mirror, the scene read with other values (its query, its width)."""
    return types.SimpleNamespace(s=dict(b.s, **changes), map=b.map, kp_point=b.kp_point, pos=b.pos)


def _same_download(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert np.asarray(a[n]).tobytes() == np.asarray(b[n]).tobytes(), n


@pytest.fixture(scope="module")
def maps(ctx, rs):
    """Built maps, made on first use and shared: maps(name, form) for loop_cases.ENVELOPE, maps("paths") for SCENES."""
    made = {}

    def get(name, form=None):
        if name == "wide" and form is not None:
            return _view(get("wide"), query=S.envelope_scene("wide", form)["query"])
        if (name, form) not in made:
            made[name, form] = Built(ctx, rs, S.scene(name) if name in S.SCENES else S.envelope_scene(name, form))
        return made[name, form]

    yield get
    for b in made.values():
        b.close()


@pytest.fixture(scope="module")
def vers(ctx):
    """Verifiers by size, made on first use and shared."""
    made = {}

    def get(*size):
        if size not in made:
            made[size] = ctx.loop_verifier(*size)
        return made[size]

    yield get
    for v in made.values():
        v.close()


@pytest.fixture(scope="module")
def ver(vers):
    return vers(2500, 8, 200)


def _call(v, b, cands, **kw):
    return v.verify(b.map, b.s["query"], cands, b.s["K"], b.s["width"], **kw)


def test_gather_chunk_edges(ver, maps):
    """n = 256, 513, 512, 513, 257, 768, 1 and 255 in one call of eight: n on a chunk edge, nt = n, the first lane alone, the
    single lane of a third chunk alone, the last and the first lane of two chunks, a chunk with no matched keypoint, nt = 0.
    The ninth candidate (n = 511: the last lane of chunk 0 and the last keypoint) runs in a second call."""
    b = maps("chunk_edges")
    got = _call(ver, b, list(range(8)))
    _check(ver, b, list(range(8)), got)
    for c in range(8):
        d = ver.download(c)
        assert d["nt"] == len(S.CHUNK_EDGES_AT[c]) and np.array_equal(d["keypoints"], S.CHUNK_EDGES_AT[c]), c
    assert [g["correspondences"] for g in got] == [0, 20, 0, 0, 0, 20, 0, 0]
    assert got[1]["candidate_kp"].max() >= 256 and got[5]["candidate_kp"].max() >= 512         # listed from beyond a chunk edge
    again = _call(ver, b, [8, 3, 1])                                        # each chain after a candidate of another size
    _check(ver, b, [8, 3, 1], again)
    assert np.array_equal(ver.download(0)["keypoints"], S.CHUNK_EDGES_AT[8])
    _same(again[1:], [got[3], got[1]])


@pytest.mark.parametrize("name,form,size,cands", [("tight", None, (300, 2, 200), [0, 1]), ("one", None, (1, 1, 1), [0]),
                                                  ("wide", None, (8192, 2, 200), [0, 1]), ("wide", "q8192", (8192, 2, 200), [0, 1]),
                                                  ("paths", None, (401, 1, 37), [0])],
                         ids=["tight", "one", "wide", "wide-q8192", "paths-401"])
def test_verifier_sizes(ver, vers, maps, name, form, size, cands):
    """max_points = n = nt = nq (tight: the guard o < max_points and the up256 slab layout at a size that is no multiple of
    64), (1, 1, 1), RANSAC_MAX_POINTS with every row gathered and with a query as large, and sizes one above the largest
    key frame.  The same bytes as the module's (2500, 8, 200) verifier gives wherever that one can hold the scene.
    wide-q8192 takes 0.51 s on the MI355X box, of which the restatement's 8192 x 8192 Hamming table is nearly all (the
    slowest test of tests/test_gpu_loop.py takes 0.18 s there); the size is the envelope's edge and stays."""
    b, v, mh = maps(name, form), vers(*size), min(200, size[2])
    got = _call(v, b, cands, max_hypotheses=mh)
    _check(v, b, cands, got)
    nts = [v.download(c)["nt"] for c in range(len(cands))]
    if name == "tight":
        assert nts == [300, 299] and got[0]["status"] == 0
    if name == "one":
        assert nts == [1] and (got[0]["status"], got[0]["correspondences"], got[0]["listed"]) == (1, 1, 1)
    if name == "wide":
        assert nts == [8192, 200] and [g["status"] for g in got] == [0, 0]
        if form is not None:                                                # the 7892 rows more of the query change nothing
            _same(got, _call(v, maps("wide"), cands))
    if max(size[0], max(len(k["kp"]) for k in b.s["key_frames"])) <= ver.max_points:
        big = _call(ver, b, cands, max_hypotheses=mh)
        _same(got, big)
        for c in range(len(cands)):
            _same_download(v.download(c), ver.download(c))


def test_gate_at_eleven_and_twelve(ver, maps):
    """400 gathered rows and exactly 11 or 12 matches: K1's count decides, not nt."""
    b, refs = maps("gate"), S.envelope_reference("gate")
    got = _call(ver, b, [0, 1, 2, 3])
    _check(ver, b, [0, 1, 2, 3], got, refs)
    assert [ver.download(c)["nt"] for c in range(4)] == [400] * 4
    assert [(g["status"], g["correspondences"]) for g in got] == [(1, 11), (0, 12), (2, 12), (0, 12)]
    g = got[0]
    assert np.array_equal(g["pose"], np.eye(4, dtype=np.float32)) and g["inliers"] == 0 and g["listed"] == g["correspondences"] == 11
    assert not g["ok"] and _bits(g["spread"]) == _bits(g["drift"]) == _bits(g["gap"]) == 0
    assert all(0 < got[c]["inliers"] <= 12 and not got[c]["ok"] for c in (1, 3)) and got[2]["listed"] == 12
    # the chain that has just fed 12 correspondences to PnP gets the candidate of 11: PnP must be told of none, so no
    # inlier is left on the chain (the exact layer's "status != 0: no inliers")
    order = [1, 0, 3, 2]
    again = _call(ver, b, order)
    _check(ver, b, order, again, refs)
    _same(again, [got[c] for c in order])


@pytest.mark.parametrize("cands", [[0, 1, 2], [3, 4, 5]], ids=["inliers", "ratio"])
def test_verdict_on_its_bounds(ver, maps, cands):
    """19 / 20 / 21 inliers, and 20/58, 21/60, 22/60 against 0.35f: the near-threshold band is empty for these candidates
    (tests/test_loop_envelope_cpu.py), so ok is demanded as the restatement's."""
    b, refs = maps("bounds"), S.envelope_reference("bounds", only=tuple(cands))
    got = _call(ver, b, cands)
    _check(ver, b, cands, got, refs)
    assert [(g["inliers"], g["correspondences"], g["ok"]) for g in got] == [S.EXPECT_BOUNDS[c] for c in cands]
    assert [g["ok"] for g in got] == [False, True, True]                    # ok differs across the bound, which is inclusive


def test_width_decides_spread_alone(ver, maps):
    """width <= 0, 1, the two widths either side of spread == 0.25f (from the GPU's own listed x), the image's and 2^31 - 1:
    spread and ok are loop_ref.finish's bit for bit, ok flips between the two, and nothing else in the record moves."""
    b = maps("paths")
    base = _call(ver, b, [0])
    assert base[0]["ok"] and base[0]["listed"] >= 2
    x = b.s["key_frames"][b.s["query"]]["kp"][base[0]["query_kp"], 0]
    d = np.float32(x.max() - x.min())
    frac = lambda w: np.float32(d / np.float32(w))                          # noqa: E731
    w_lo = int(4 * float(d)) + 2
    while frac(w_lo) < L.MIN_SPREAD_FRAC:
        w_lo -= 1
    w_hi = w_lo + 1
    assert frac(w_lo) >= L.MIN_SPREAD_FRAC > frac(w_hi) and w_lo > 1
    by = {}
    for w in (-5, 0, 1, w_lo, w_hi, 1280, 2 ** 31 - 1):
        got = ver.verify(b.map, b.s["query"], [0], b.s["K"], w)
        _check(ver, _view(b, width=w), [0], got)                            # spread and ok equal loop_ref.finish bit for bit
        by[w] = got[0]
        for n in RECORD:
            if n not in ("spread", "ok"):
                assert np.asarray(got[0][n]).tobytes() == np.asarray(base[0][n]).tobytes(), (w, n)
    assert [by[w]["ok"] for w in (-5, 0, 1, w_lo, w_hi, 1280, 2 ** 31 - 1)] == [False, False, True, True, False, True, False]
    assert _bits(by[-5]["spread"]) == _bits(by[0]["spread"]) == 0 and _bits(by[1]["spread"]) == _bits(d)
    assert _bits(by[1280]["spread"]) == _bits(base[0]["spread"])


@pytest.mark.parametrize("form", S.LISTING_FORMS)
def test_listing_beyond_one_stride(ver, maps, form):
    """700 listed correspondences (two full strides and a tail of 188: not every thread, not every lane of the last wave),
    the two query keypoints of extreme x listed last, first, or by wave 3 in the second stride; 300 listed with status 2.
    Spread and the listed triples (mapped back) are those of the scene before relabelling, so equal across the forms."""
    b, refs, perm = maps("listing", form), S.envelope_reference("listing", form), S.listing_perm(form)
    got = _call(ver, b, [0, 1])
    _check(ver, b, [0, 1], got, refs)
    assert (got[0]["status"], got[0]["listed"], got[1]["status"], got[1]["listed"]) == (0, 700, 2, 300)
    x = b.s["key_frames"][b.s["query"]]["kp"][got[0]["query_kp"], 0]
    assert sorted((int(np.argmin(x)), int(np.argmax(x)))) == {"last": [698, 699], "first": [0, 1], "wave3": [456, 457]}[form]
    for g, r in zip(got, S.envelope_reference("listing")):
        assert _bits(g["spread"]) == _bits(r["spread"]) and g["ok"] == r["ok"]
        assert {(int(perm[q]), int(p), int(c)) for q, p, c in zip(g["query_kp"], g["point"], g["candidate_kp"])} == \
            {(int(q), int(p), int(c)) for q, p, c in zip(r["query_kp"], r["point"], r["candidate_kp"])}


def test_a_chain_forgets_its_last_candidate(ctx, ver, maps):
    """Chain 0 sees 700 inliers, then status 2, status 1 with 11 matches, nt = 0 and a verified candidate: after each call the
    record and the chain's buffers are those of a chain that has never run.  The never-run chain is chain i of ONE fresh
    verifier at step i (a call of i + 1 candidates touches chains 0 .. i; chains share no buffer, which
    test_call_forms_are_deterministic pins), so the test makes one verifier, not five.  Then 8 -> 1 -> 8 candidates.  Both
    issue forms; the one-stream form is held against the forked form's bytes."""
    lst, p = maps("listing", "last"), maps("paths")
    steps = [(lst, 0, (0, 700)), (p, 4, (2, 0)), (p, 3, (1, 0)), (p, 1, (1, 0)), (p, 0, (0, None))]
    fresh = ctx.loop_verifier(2500, 8, 200)
    kept = []
    try:
        for form in (0, 1):
            ctx.set_int("loop_verify_streams", form)
            for i, (b, c, (status, inliers)) in enumerate(steps):
                got = _call(ver, b, [c])
                d = ver.download(0)
                assert got[0]["status"] == status and inliers in (None, got[0]["inliers"])
                _check(ver, b, [c], got)
                if form == 0:
                    want = _call(fresh, b, [c] * (i + 1))
                    kept.append((want[i:], fresh.download(i)))
                _same(got, kept[i][0])
                _same_download(d, kept[i][1])
            assert ver.download(0)["nt"] == 200 and _call(ver, p, [1])[0]["listed"] == 0 and ver.download(0)["nt"] == 0
            eight = _call(ver, p, list(range(8)))
            one = _call(ver, p, [6])
            _same(one, [eight[6]])
            _same(_call(ver, p, list(range(8))), eight)
            if form == 0:
                kept.append(_call(fresh, p, list(range(8))))
            _same(eight, kept[len(steps)])
            assert [(g["status"], g["ok"]) for g in eight] == S.EXPECT["paths"]
    finally:
        ctx.set_int("loop_verify_streams", 0)
        fresh.close()


@pytest.mark.parametrize("index", range(len(S.PARAMETERS)), ids=lambda i: "-".join(f"{k}={v}" for k, v in S.PARAMETERS[i][0].items()))
def test_parameters_reach_both_stages(ver, maps, index):
    """max_distance reaches K1 and threshold_px, confidence and max_hypotheses reach PnP: one argument off its default per
    case (loop_cases.PARAMETERS), the exact layer always and end to end for the candidates the table keeps."""
    kw, kept = S.PARAMETERS[index]
    b, refs = maps("paths"), S.parameter_reference(index)
    got = _call(ver, b, [0, 6], **kw)
    _check(ver, b, [0, 6], got, {c: refs[c] for c in kept}, max_distance=kw.get("max_distance", 64))
    for g, c in zip(got, (0, 6)):                                           # (whatever is kept: the gate is exact)
        assert (g["status"] == 1) == (refs[c]["status"] == 1) and g["correspondences"] == refs[c]["correspondences"]
    if kw.get("max_distance") == 0:
        assert [g["status"] for g in got] == [1, 1]


def test_map_states_the_lap_never_reaches(ctx, rs, synth, vers):
    """The exact layer after each map edit that loop.hip reads through rs_map_loop_sync: a candidate's and the query's pose
    (the centres behind gap and drift), a key frame of 6000 rows added after the first call (the pool and d_kp_point grow;
    it is then a candidate with nt = 0), remove_observation of three gathered points, map matches of the query's own, and
    the roles swapped so that the candidate's index is above the query's."""
    v = vers(8192, 2, 200)
    s = synth.loop_scene(9, 300, ((400, 200, 70, 0.2, None), (300, 150, 60, 0.2, None)))
    b = Built(ctx, rs, s)
    q = s["query"]
    rng = np.random.default_rng(9)

    def moved(T):
        out = np.array(T, np.float32)
        out[:3, 3] += rng.normal(0, 0.5, 3).astype(np.float32)
        return out

    try:
        first = _call(v, b, [0, 1])
        _check(v, b, [0, 1], first)
        assert first[0]["status"] == first[1]["status"] == 0
        # the candidate's pose moves its centre: gap follows, nothing else; then the query's: drift follows
        s["key_frames"][0] = dict(s["key_frames"][0], pose=moved(s["key_frames"][0]["pose"]))
        b.map.set_keyframe_pose(0, s["key_frames"][0]["pose"])
        got = _call(v, b, [0, 1])
        _check(v, b, [0, 1], got)
        assert _bits(got[0]["gap"]) != _bits(first[0]["gap"]) and _bits(got[0]["drift"]) == _bits(first[0]["drift"])
        _same(got[1:], first[1:])
        s["key_frames"][q] = dict(s["key_frames"][q], pose=moved(s["key_frames"][q]["pose"]))
        b.map.set_keyframe_pose(q, s["key_frames"][q]["pose"])
        got2 = _call(v, b, [0, 1])
        _check(v, b, [0, 1], got2)
        for a, c in zip(got2, got):
            assert _bits(a["drift"]) != _bits(c["drift"]) and _bits(a["gap"]) == _bits(c["gap"])
        # a key frame of 6000 rows after the first verification: the pool and d_kp_point grow
        kp = np.stack([rng.uniform(0, 1280, 6000), rng.uniform(0, 720, 6000)], 1).astype(np.float32)
        desc = rng.integers(0, 256, (6000, 32), dtype=np.uint8)
        b.frames.append(rs.ResidentFrame(ctx, kp, desc))
        new = b.map.add_keyframe(b.frames[-1], np.eye(4, dtype=np.float32))
        assert new == 3
        s["key_frames"].append(dict(kp=kp, desc=desc, pose=np.eye(4, dtype=np.float32), kp_point=np.full(6000, -1, np.int32)))
        b.kp_point.append(np.full(6000, -1, np.int32))
        got3 = _call(v, b, [0, 1])
        _check(v, b, [0, 1], got3)
        _same(got3, got2)
        got4 = _call(v, b, [new, 0])
        _check(v, b, [new, 0], got4)
        assert v.download(0)["nt"] == 0 and got4[0]["status"] == 1
        _same(got4[1:], got2[:1])
        # three gathered points lose their observation in the candidate
        rows = L.candidate_rows(b.kp_point[0])
        gone = [int(b.kp_point[0][r]) for r in rows[[0, 5, -1]]]
        for r, pnt in zip(rows[[0, 5, -1]], gone):
            b.map.remove_observation(pnt, 0)
            b.kp_point[0][r] = -1
        got5 = _call(v, b, [0, 1])
        _check(v, b, [0, 1], got5)
        d = v.download(0)
        assert d["nt"] == len(rows) - 3 and not set(gone) & set(d["slots"].tolist())
        _same(got5[1:], got2[1:])
        # the query gets map matches of its own: 40 of its shared keypoints observe the points they show
        qk, ck, _ = s["shared"][0]
        pairs = [(int(a), int(b.kp_point[0][c])) for a, c in zip(qk, ck) if b.kp_point[0][c] >= 0][:40]
        assert len(pairs) == 40
        b.kp_point[q] = b.kp_point[q].copy()
        for a, pnt in pairs:
            b.map.add_observation(pnt, q, a)
            b.kp_point[q][a] = pnt
        got6 = _call(v, b, [0, 1])
        _check(v, b, [0, 1], got6)
        _same(got6, got5)
        # the roles swapped: the candidate's index is above the query's
        sw = _view(b, query=0)
        got7 = _call(v, sw, [q, 1])
        _check(v, sw, [q, 1], got7)
        assert v.download(0)["nt"] == 40 and got7[0]["correspondences"] >= 12
    finally:
        b.close()


def test_after_the_key_frame_stages(ctx, rs, oracle, ver):
    """insert_keyframe from a DeviceFrame, reanchor and cull_points(apply=True) in Mapper::insert's order on
    test_gpu_keyframe.py's map of 4 key frames and 400 slots, then a verification of the new key frame against the old ones;
    the mirror is the model keyframe_ref keeps, the positions are map.positions().  Exact layer only.
    A key frame without keypoints can be made (rs_frame_create takes n = 0): as a query it gives status 1 with no
    correspondences, and as a candidate nt = 0."""
    import test_gpu_keyframe as KF
    c = KF.Case(ctx, rs, (26, 4, 200, 400), extra=60, bad_frac=0.1)
    model, fr = c.model, c.fr
    n = len(fr["keypoints"])
    df = rs.DeviceFrame(ctx, 512)
    empty = rs.ResidentFrame(ctx, np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8))
    try:
        assert df.assign(ctx.dev(fr["descriptors"]), ctx.dev(fr["keypoints"]), ctx.dev(np.array([n], np.int32))) == n
        mk, mp = c.map.match(df, c.fpose, R.K, R.WIDTH, R.HEIGHT)
        assert (mk.tolist(), mp.tolist()) == c.match() and len(mk) > 20
        df.matches_add(ctx.dev(mk.astype(np.int32)), ctx.dev(mp.astype(np.int32)))
        table = np.full(n, -1, np.int32)
        table[mk] = mp
        kf, _ = model.add_keyframe(fr["keypoints"], fr["descriptors"], c.fpose)
        assert c.map.insert_keyframe(df, c.fpose) == (kf, R.adopt(model, kf, table))
        opt = [1, 2, 3]
        before = c.move_poses(opt, 26)
        cnt, slots, xyz = c.map.reanchor(opt, before)
        want_slots, want_xyz = R.reanchor(model, opt, before, oracle)
        assert cnt == len(want_slots) > 10 and np.array_equal(slots, want_slots) and KF.bits(xyz) == KF.bits(want_xyz)
        kfs = np.array(opt + [kf], np.int32)
        want = R.cull(model, kfs, R.K, oracle, apply=True)
        assert R.cull_margin(want["mean_err"]) >= R.CULL_MARGIN
        got = c.map.cull_points(kfs, R.K, apply=True)
        assert np.array_equal(got["removed"], want["removed"]) and got["n_removed"] > 0
        assert c.map.add_keyframe(empty, np.eye(4, dtype=np.float32)) == kf + 1
        model.add_keyframe(np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8), np.eye(4, dtype=np.float32))
        assert model.consistent()
        key_frames = [dict(kp=model.kf_kp[k], desc=model.kf_desc[k], pose=model.kf_pose[k].reshape(4, 4)) for k in range(model.n_kf())]
        pos = c.map.positions()
        assert KF.bits(pos) == KF.bits(model.positions())
        b = types.SimpleNamespace(s=dict(key_frames=key_frames, query=kf, width=R.WIDTH), map=c.map, pos=pos,
                                  kp_point=[np.asarray(t, np.int32) for t in model.kp_point])
        cands = [0, 1, 2, 3]
        res = ver.verify(c.map, kf, cands, R.K, R.WIDTH)
        _check(ver, b, cands, res)
        assert max(g["correspondences"] for g in res) >= 12 and all(ver.download(i)["nt"] > 0 for i in range(4))
        assert not set(want["removed"].tolist()) & set(np.concatenate([ver.download(i)["slots"] for i in range(4)]).tolist())
        nq0 = _view(b, query=kf + 1)
        res = ver.verify(c.map, kf + 1, [kf, 0], R.K, R.WIDTH)
        _check(ver, nq0, [kf, 0], res)
        assert [(g["status"], g["correspondences"], g["listed"]) for g in res] == [(1, 0, 0)] * 2
        res = ver.verify(c.map, kf, [kf + 1, 1], R.K, R.WIDTH)
        _check(ver, b, [kf + 1, 1], res)
        assert ver.download(0)["nt"] == 0 and res[0]["status"] == 1
    finally:
        empty.close()
        df.close()
        c.close()
