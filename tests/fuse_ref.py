"""Python restatement of Mapper::fuse_loop (reference src/Mapper.cpp:41-77,176-220) on the test model of the map: plain
Python / numpy, test infrastructure only.

Built from what the tests already have: map_model.MapModel (fuse, associate, fuse_view), match_ref.reproj_match (with the
KD-tree walk order) and frame_ref.build (the KD-tree).  Where the reference leaves an order unspecified the project's
rules apply (include/rsgpu.h): sources in ascending point slot, covisibles by shared count descending, key-frame handle
ascending.

match_ref evaluates the gates in float64 and names a BOUNDARY set it does not vouch for.  A fuse case must not depend on
such a decision — later frames depend on earlier ones.  frame_matches therefore first closes every keypoint that cannot win
a proposal (an exact transformation, see closed_for), which takes the rims of the search discs out of the question, and
refuses (AssertionError) a case in which a source is still in that set: the case is then not a valid case and is changed,
not tolerated.

Outcome codes: include/rsgpu.h, RS_FUSE_*.
"""
import copy

import numpy as np

import frame_ref
import match_ref

SKIPPED, ASSOCIATED, POINT_MATCHED, SAME, OLD, FUSED = range(6)


def loop_old_frames(model, candidate, min_shared=15, max_covisible=20):
    """loop_covisibles (:41-66): [candidate] + the ranked covisibles"""
    shared = {}
    for p in model.kp_point[candidate]:
        if p < 0:
            continue
        for kf, _ in model.obs[int(p)]:
            if kf != candidate:
                shared[kf] = shared.get(kf, 0) + 1
    ranked = sorted((kf for kf, c in shared.items() if c >= min_shared), key=lambda kf: (-shared[kf], kf))
    return [candidate] + ranked[:max(max_covisible, 0)]


def loop_points(model, old_frames):
    """loop_points (:68-77): the set of point slots the old frames match"""
    return {int(p) for kf in old_frames for p in model.kp_point[kf] if p >= 0}


def fuse_match(model, kf, kp, kept, old_points, trace=None):
    """Mapper::fuse_match (:176-196).  Returns the outcome; trace (a list) receives Map::fuse's per-observation outcomes."""
    if kf < 0 or kf >= model.n_kf() or kp < 0 or kp >= len(model.kp_point[kf]):
        return SKIPPED
    if kept < 0 or kept >= model.n_slots() or not model.alive[kept]:
        return SKIPPED
    existing = int(model.kp_point[kf][kp])
    if existing < 0:
        if np.any(model.kp_point[kf] == kept):
            return POINT_MATCHED
        model.associate(kf, kept, kp)
        return ASSOCIATED
    if existing == kept:
        return SAME
    if existing in old_points:
        return OLD
    outcomes, _ = model.fuse(kept, existing)
    if trace is not None:
        trace.append((kept, existing, outcomes))
    return FUSED


def frame_dict(model, kf, camera):
    kp = model.kf_kp[kf]
    node_kp, left, right, root = frame_ref.build(kp)
    return dict(pose=model.kf_pose[kf], K=camera["K"], width=camera["width"], height=camera["height"], keypoints=kp,
                descriptors=model.kf_desc[kf], kp_matched=np.zeros(len(kp), np.uint8), kd_node_kp=node_kp, kd_left=left,
                kd_right=right, kd_root=root)


def frame_matches(model, kf, sources, camera, max_distance=64):
    """MapMatcher::match_for_fuse (src/MapMatcher.cpp:117-127) of key frame kf against the ascending source list on the
    model's CURRENT state: [(keypoint, point)] in ascending keypoint order, and the sources' eligibility."""
    if len(model.kf_kp[kf]) == 0 or len(sources) == 0:
        return [], np.zeros(len(sources), np.uint8)
    observed = [p for p in sources if model.observer_kp(p, kf) is not None]
    mp = model.fuse_view(list(sources), matched_points=observed)
    fr = frame_dict(model, kf, camera)

    def closed_for(view):
        """A keypoint whose descriptor is max_distance or more from every observation of every eligible point of `view` can
        never win a proposal there (strict '<' from max_distance, src/MapMatcher.cpp:78,88): closing it (replace = 0 with
        kp_matched set) changes no output, and keeps match_ref from calling a point undecided because such a keypoint
        sits on the rim of its search disc.  The tree keeps every keypoint, so the walk order of the others is untouched."""
        rows = [r for s in np.flatnonzero(view["eligible"]) for r in view["obs_desc"][view["obs_ptr"][s]:view["obs_ptr"][s + 1]]]
        if not rows:
            return np.ones(len(fr["keypoints"]), np.uint8)
        return (match_ref.hamming(fr["descriptors"], view["desc_pool"][sorted(set(rows))]).min(1) >= max_distance).astype(np.uint8)

    ref = match_ref.reproj_match(dict(fr, kp_matched=closed_for(mp)), mp, replace=0, max_distance=max_distance)
    point_kp, point_dist = ref["point_kp"].copy(), ref["point_dist"].copy()
    for s in ref["boundary_points"]:         # once more, alone: only the keypoints that can win THIS point stay open
        one = model.fuse_view([sources[int(s)]], matched_points=observed)
        r1 = match_ref.reproj_match(dict(fr, kp_matched=closed_for(one)), one, replace=0, max_distance=max_distance)
        assert len(r1["boundary_points"]) == 0, f"key frame {kf}, point {sources[int(s)]}: a float32 gate is too close to call for this case"
        point_kp[s], point_dist[s] = r1["point_kp"][0], r1["point_dist"][0]
    best = {}                                # per keypoint: the smallest distance, then the earliest source (sequential strict '<')
    for s in np.flatnonzero(point_kp >= 0):
        k = int(point_kp[s])
        if k not in best or point_dist[s] < point_dist[best[k]]:
            best[k] = int(s)
    return [(k, int(sources[best[k]])) for k in sorted(best)], mp["eligible"].copy()


def fuse_loop(model, query, candidate, inliers, window, camera, max_distance=64, min_shared=15, max_covisible=20):
    """Mapper::fuse_loop (:198-220) on a COPY of the model.  Returns dict(old_frames, sources (ascending), journal (section
    0 = the inliers, section 1 + w = window entry w; entries (keypoint, point, outcome)), removed (discarded slots in
    order), model (edited), trace (Map::fuse's per-observation outcomes), eligible (per window entry: the sources'
    eligibility when the frame ran, None for a skipped frame))."""
    m = copy.deepcopy(model)
    old_frames = loop_old_frames(m, candidate, min_shared, max_covisible)
    old_points = loop_points(m, old_frames)
    sources = sorted(old_points)
    journal, removed, trace, eligible = [[]], [], [], []

    def run(kf, kp, pt, section):
        before = len(trace)
        oc = fuse_match(m, kf, kp, pt, old_points, trace)
        section.append((int(kp), int(pt), oc))
        if len(trace) > before:
            removed.append(trace[-1][1])

    for kp, pt in inliers:
        run(query, int(kp), int(pt), journal[0])
    for kf in window:
        section = []
        journal.append(section)
        if kf in old_frames:
            eligible.append(None)
            continue
        matches, elig = frame_matches(m, kf, sources, camera, max_distance)
        eligible.append(elig)
        for kp, pt in matches:
            run(kf, kp, pt, section)
    return dict(old_frames=old_frames, sources=sources, journal=journal, removed=removed, model=m, trace=trace, eligible=eligible)
