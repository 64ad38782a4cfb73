"""The scenes of tests/test_loop_cpu.py and tests/test_gpu_loop.py (synth.loop_scene) and their restatement results,
computed once per process."""
import functools
import importlib

import numpy as np

import loop_ref as L
import pnp_ref as P

# name -> (seed, nq, candidates (n, matched, shared, outlier_frac, strip)); what each candidate is there for
SCENES = {
    "paths": (1, 300, ((400, 200, 70, 0.3, None),           # 0 verified
                       (60, 0, 0, 0.0, None),               # 1 nt = 0                      -> status 1
                       (60, 1, 1, 0.0, None),               # 2 nt = 1 (K1's no-ratio path) -> status 1
                       (100, 11, 11, 0.0, None),            # 3 11 matched                  -> status 1
                       (200, 100, 40, 1.0, None),           # 4 every match wrong           -> status 2
                       (300, 100, 16, 0.0, None),           # 5 fewer than 20 inliers
                       (300, 150, 90, 0.7, None),           # 6 inlier ratio below 0.35
                       (300, 120, 50, 0.0, (0.40, 0.55)))), # 7 all inliers in a narrow strip
    "big": (2, 300, ((2500, 1100, 120, 0.3, None),          # the compaction crosses chunk boundaries, nt > one block
                     (400, 200, 60, 0.2, None))),
}
EXPECT = {"paths": [(0, True), (1, False), (1, False), (1, False), (2, False), (0, False), (0, False), (0, False)],
          "big": [(0, True), (0, True)]}


def synth():
    return importlib.import_module("racing-slam_amd").synth


@functools.lru_cache(maxsize=None)
def scene(name):
    seed, nq, cands = SCENES[name]
    return synth().loop_scene(seed, nq, cands)


@functools.lru_cache(maxsize=None)
def reference(name):
    """loop_ref.verify_pnp of every candidate of the scene against its query (the reference's constants, seed 0)."""
    s = scene(name)
    q = s["key_frames"][s["query"]]
    return [L.verify_pnp(q, s["key_frames"][c], s["points"], s["K"], s["width"]) for c in range(s["query"])]


def near_threshold(s, r):
    """The correspondences of a verification within test_gpu_pnp.py's band of the final model: |e^2 - thr^2| <= 1e-9 thr^2."""
    if r["pnp"] is None:
        return np.zeros(len(r["mq"]), bool)
    q = s["key_frames"][s["query"]]
    X, Y, Z, x, y, fin = P.prepare(r["obj"], q["kp"], s["K"], r["mt"], r["mq"])
    zc, e2 = P.reproj2(r["pnp"]["Rt"], X, Y, Z, x, y, float(s["K"][0]), float(s["K"][1]))
    thr2 = r["pnp"]["thr2"]
    return fin & (np.abs(e2 - thr2) <= 1e-9 * thr2)


# ---------------------------------------------------------------------------------------------- the envelope
# tests/test_loop_envelope_cpu.py and tests/test_gpu_loop_envelope.py: scenes that put loop.hip's gather, gate and verdict
# on their edges.  Kept apart from SCENES, which tests/test_gpu_loop.py builds in full.
def relabel(scene, kf, perm):
    """The scene with the keypoints of key frame kf permuted: new keypoint j is old keypoint perm[j].  kp, desc, kp_point,
    the keypoint index inside the observations and the shared entries move together, so the scene is the same
    geometrically; only the order of the keypoints changes, and with it the gather and the listing order."""
    perm = np.asarray(perm, np.int64)
    k = scene["key_frames"][kf]
    assert np.array_equal(np.sort(perm), np.arange(len(k["kp"])))
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    out = dict(scene)
    out["key_frames"] = list(scene["key_frames"])
    out["key_frames"][kf] = dict(kp=k["kp"][perm].copy(), desc=k["desc"][perm].copy(), pose=k["pose"], kp_point=k["kp_point"][perm].copy())
    out["observations"] = [(p, f, int(inv[i]) if f == kf else i) for p, f, i in scene["observations"]]
    out["shared"] = [(inv[qk].astype(np.int32) if kf == scene["query"] else qk, inv[ck].astype(np.int32) if kf == c else ck, placed)
                     for c, (qk, ck, placed) in enumerate(scene["shared"])]
    return out


def matched_at(scene, kf, positions):
    """relabel so that the keypoints of key frame kf that have a map match are exactly `positions` (as many as matched)."""
    kpp = scene["key_frames"][kf]["kp_point"]
    want = np.zeros(len(kpp), bool)
    want[np.asarray(positions, np.int64)] = True
    assert want.sum() == (kpp >= 0).sum(), (kf, int(want.sum()), int((kpp >= 0).sum()))
    perm = np.empty(len(kpp), np.int64)
    perm[want], perm[~want] = np.flatnonzero(kpp >= 0), np.flatnonzero(kpp < 0)
    return relabel(scene, kf, perm)


# gather scenes (exact layer only).  chunk_edges: per candidate the keypoints that carry a map match, in chunks of LOOP_BLOCK
# = 256.  Nine candidates: the eight of one call, and a ninth so that every size 1, 255 .. 513, 768 occurs (both "all
# matched" and "only the last keypoint" want n = 513).
CHUNK_EDGES_AT = (np.arange(256),                                     # a  n = 256: one full chunk, n on the chunk edge
                  np.arange(513),                                     # b  n = 513: two full chunks and one lane, nt = n
                  np.array([0]),                                      # c  n = 512: the first lane only
                  np.array([512]),                                    # d  n = 513: the single lane of a third chunk only
                  np.array([255, 256]),                               # e  n = 257: the last lane of chunk 0, the first of chunk 1
                  np.r_[np.arange(256), np.arange(512, 768)],         # f  n = 768: chunk 1 has no matched keypoint at all
                  np.array([0]),                                      # g  n = 1
                  np.zeros(0, np.int64),                              # h  n = 255: none matched
                  np.array([255, 510]))                               # i  n = 511: the last lane of chunk 0, the last keypoint
CHUNK_EDGES_N = (256, 513, 512, 513, 257, 768, 1, 255, 511)
# seeds and outlier fractions found by search with the restatement alone; tests/test_loop_envelope_cpu.py asserts what they give
GATE_SEED, BOUNDS_SEED, LISTING_SEED = 1, 1, 8
BOUNDS_FRAC = (0.605, 0.5825, 0.6125)
# name -> (seed, nq, candidates (n, matched, shared, outlier_frac, strip))
ENVELOPE = {
    "chunk_edges": (3, 50, tuple((n, len(at), sh, 0.0, None) for n, at, sh in zip(CHUNK_EDGES_N, CHUNK_EDGES_AT, (0, 20, 0, 0, 0, 20, 0, 0, 0)))),
    "tight": (4, 300, ((300, 300, 80, 0.0, None),                     # n = nt = nq = max_points
                       (300, 299, 80, 0.0, None))),
    "one": (5, 1, ((1, 1, 1, 0.0, None),)),
    "wide": (6, 300, ((8192, 8192, 120, 0.2, None),                   # RANSAC_MAX_POINTS rows, all gathered
                      (400, 200, 60, 0.0, None))),                    # and a second query of 8192 keypoints (envelope_scene)
    # gate and verdict scenes (exact layer and end to end)
    "gate": (GATE_SEED, 100, ((600, 400, 11, 0.0, None),              # 0 11 matches of 400 gathered rows -> status 1
                              (600, 400, 12, 0.0, None),              # 1 12, all placed                   -> status 0, ok false
                              (600, 400, 12, 1.0, None),              # 2 12, all wrong                    -> status 2
                              (600, 400, 12, 0.0, (0.40, 0.55)))),    # 3 12, all placed in a strip
    # the inliers are the placed ones: BOUNDS_FRAC places exactly 20, 21 and 22 of candidates 3, 4 and 5
    "bounds": (BOUNDS_SEED, 300, ((300, 150, 19, 0.0, None),          # 0 19 inliers                        ok false
                                  (300, 150, 20, 0.0, None),          # 1 20                                ok
                                  (300, 150, 21, 0.0, None),          # 2 21                                ok
                                  (300, 150, 58, BOUNDS_FRAC[0], None),   # 3 20 / 58 < 0.35f               ok false
                                  (300, 150, 60, BOUNDS_FRAC[1], None),   # 4 21 / 60 == 0.35f              ok
                                  (300, 150, 60, BOUNDS_FRAC[2], None))), # 5 22 / 60 > 0.35f               ok
    # nq = 1000, not 800: the two candidates' shared query keypoints are disjoint, 700 + 300 of them
    "listing": (LISTING_SEED, 1000, ((900, 800, 700, 0.0, None),      # 0 status 0, listed > 512 and no multiple of 64
                                     (500, 400, 300, 1.0, None))),    # 1 status 2, listed = correspondences > 256
}
EXPECT_BOUNDS = [(19, 19, False), (20, 20, True), (21, 21, True), (20, 58, False), (21, 60, True), (22, 60, True)]   # inliers, correspondences, ok
LISTING_FORMS = ("last", "first", "wave3")      # where the two listed query keypoints of extreme x sit in the listing
WIDE_QUERY = 8192


@functools.lru_cache(maxsize=None)
def listing_perm(form):
    """The query relabelling `form` of `listing` (new keypoint j is old keypoint perm[j]), from the restatement's result for
    candidate 0 of the unrelabelled scene."""
    s, r = envelope_scene("listing"), envelope_reference("listing", only=(0,))[0]
    q = s["key_frames"][s["query"]]
    listed = r["query_kp"].astype(np.int64)
    x = q["kp"][listed, 0]
    ends = [int(listed[np.argmin(x)]), int(listed[np.argmax(x)])]
    inl = [int(i) for i in listed if int(i) not in ends]
    rest = [i for i in range(len(q["kp"])) if i not in set(listed.tolist())]
    if form == "last":                          # the highest query indices: listed last, in the tail stride
        return np.array(inl + rest + ends)
    if form == "first":
        return np.array(ends + inl + rest)
    assert form == "wave3"                      # listing positions 456 and 457: k >= 256 and k % 256 >= 192
    return np.array(inl[:456] + ends + inl[456:] + rest)


@functools.lru_cache(maxsize=None)
def envelope_scene(name, form=None):
    """The scene `name` of ENVELOPE.  form: for "listing" one of LISTING_FORMS (the query relabelled), for "wide" "q8192"
    (the same map, the query is its second query key frame of 8192 keypoints)."""
    seed, nq, cands = ENVELOPE[name]
    if form is not None and name == "listing":
        s = envelope_scene(name)
        return relabel(s, s["query"], listing_perm(form))
    if form is not None:
        assert (name, form) == ("wide", "q8192")
        return dict(envelope_scene(name), query=len(cands) + 1)
    s = synth().loop_scene(seed, nq, cands)
    if name == "chunk_edges":
        for kf, at in enumerate(CHUNK_EDGES_AT):
            s = matched_at(s, kf, at)
    if name == "wide":                          # a second query after the first: its rows, then random rows that match nothing
        q, rng = s["key_frames"][s["query"]], np.random.default_rng(seed)
        extra = WIDE_QUERY - nq
        kp = np.concatenate([q["kp"], np.stack([rng.uniform(0, s["width"], extra), rng.uniform(0, s["height"], extra)], 1).astype(np.float32)])
        desc = np.concatenate([q["desc"], rng.integers(0, 256, (extra, 32), dtype=np.uint8)])
        s["key_frames"].append(dict(kp=kp, desc=desc, pose=q["pose"], kp_point=np.full(WIDE_QUERY, -1, np.int32)))
    return s


def envelope_reference(name, form=None, only=None):
    """loop_ref.verify_pnp of every candidate of envelope_scene(name, form) against its query: a list, or for the
    candidates `only` a dict.  Computed once per candidate."""
    if only is not None:
        return {c: _candidate_reference(name, form, c) for c in only}
    return [_candidate_reference(name, form, c) for c in range(len(envelope_scene(name, form)["shared"]))]


@functools.lru_cache(maxsize=None)
def _candidate_reference(name, form, c):
    s = envelope_scene(name, form)
    q = s["key_frames"][s["query"]]
    return L.verify_pnp(q, s["key_frames"][c], s["points"], s["K"], s["width"])


def decided(s, r, cap=3):
    """The condition under which a device may be asked for the restatement's ok: at most `cap` correspondences in the
    near-threshold band, and no bound of the verdict within that many inliers (or, for the spread, a pixel) of flipping."""
    slack = int(near_threshold(s, r).sum())
    if slack > cap:
        return False
    if r["status"] != 0:
        return True
    n, k = r["correspondences"], r["inliers"]
    return bool((k - slack >= L.MIN_PNP_INLIERS or k + slack < L.MIN_PNP_INLIERS) and
                (slack == 0 or (k - slack) / n >= 0.35 + 1e-6 or (k + slack) / n < 0.35 - 1e-6) and
                abs(float(r["spread"]) - 0.25) > 1.0 / s["width"])


# test_parameters_reach_both_stages: on `paths`, the arguments of one call and the candidates of (0, 6) for which end to
# end equality is demanded (decided() holds for them; tests/test_loop_envelope_cpu.py asserts exactly that)
PARAMETERS = tuple((kw, (0, 6)) for kw in (
    [dict(max_distance=v) for v in (0, 8, 64, 256)] + [dict(threshold_px=v) for v in (0.5, 4.0, 50.0)] +
    [dict(confidence=v) for v in (0.5, 0.999)] + [dict(max_hypotheses=v) for v in (1, 200)]))


@functools.lru_cache(maxsize=None)
def parameter_reference(index):
    """loop_ref.verify_pnp of candidates 0 and 6 of `paths` with the arguments PARAMETERS[index]: {candidate: result}."""
    s = scene("paths")
    q = s["key_frames"][s["query"]]
    return {c: L.verify_pnp(q, s["key_frames"][c], s["points"], s["K"], s["width"], **PARAMETERS[index][0]) for c in (0, 6)}
