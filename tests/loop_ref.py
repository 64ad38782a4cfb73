"""CPU restatement of LoopDetector::query's "Loop verify" stage and what follows it (reference src/LoopDetector.cpp):
verify_pnp (:176-229) with set_correspondences (:117-144), keypoint_spread (:146-158) and finish_verification (:160-174);
best_candidate (:267-285), publish_result (:287-308) and Impl::update_streak (:375-442).

The two calls inside verify_pnp are the project's own restatements: match_ref.match_descriptors (MapMatcher's
match_descriptors) and pnp_ref.estimate_pose_pnp (the cv::solvePnPRansac call).  This module adds what surrounds them,
over a map given as plain arrays (the mirror of an rs_map): per key frame its descriptor rows desc [n][32], keypoints
kp [n][2] f32, kp_point [n] (point slot of keypoint i or -1) and pose [4][4] f32; the points' positions pos [P][3] f32.
"""
import numpy as np

import match_ref
import pnp_ref

MIN_PNP_CORRESPONDENCES = 12        # :34
MIN_PNP_INLIERS = 20                # :35
MIN_PNP_INLIER_RATIO = np.float32(0.35)     # :36
MIN_SPREAD_FRAC = np.float32(0.25)          # :37
PNP_REPROJ_ERROR = 4.0              # :38
MIN_LOOP_SEPARATION = 15            # :47
MIN_CONSISTENT = 3                  # :48
CONSISTENCY_WINDOW = 15             # :49

f32 = np.float32


def candidate_rows(kp_point):
    """The candidate's keypoints with a map match, ascending: Frame::map_matches() walks m_map_matches, a vector indexed
    by keypoint (src/Frame.cpp:14, :100)."""
    out = []
    for i, p in enumerate(np.asarray(kp_point)):
        if p >= 0:
            out.append(i)
    return np.array(out, np.int32)


def centre_of(pose):
    """Frame::camera_center = -R^T t in f32, in the operation order of map.hip's centre_of."""
    T = np.asarray(pose, f32).reshape(16)
    return np.array([f32(f32(f32(-T[i]) * T[3]) + f32(f32(-T[4 + i]) * T[7])) + f32(f32(-T[8 + i]) * T[11]) for i in range(3)], f32)


def _distance(a, b):
    d = [f32(a[k]) - f32(b[k]) for k in range(3)]
    return np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])))


def verdict(pose, listed_x, width, query_centre, candidate_centre, correspondences, inliers):
    """finish_verification in f32: dict(spread, drift, gap, ok).  listed_x: the x of the listed query keypoints."""
    x = np.asarray(listed_x, f32)
    if len(x) < 2 or width <= 0:
        spread = f32(0.0)
    else:
        lo = hi = x[0]
        for v in x:
            lo, hi = min(lo, v), max(hi, v)
        spread = f32(f32(hi - lo) / f32(width))
    rc = centre_of(pose)
    drift, gap = _distance(rc, query_centre), _distance(rc, candidate_centre)
    ratio = f32(0.0) if correspondences == 0 else f32(f32(inliers) / f32(correspondences))
    ok = bool(inliers >= MIN_PNP_INLIERS and ratio >= MIN_PNP_INLIER_RATIO and spread >= MIN_SPREAD_FRAC)
    return dict(spread=f32(spread), drift=f32(drift), gap=f32(gap), ok=ok)


def finish(status, pose, inlier_index, mq, mt, rows, kp_point_c, kp_q, width, query_centre, candidate_centre):
    """The record and the listed correspondences from a status, a pose and an inlier index list (the restatement's own
    or a device's): what verify_pnp returns once solvePnPRansac has answered."""
    cnt = len(mq)
    out = dict(status=int(status), correspondences=cnt, inliers=0, ok=False, spread=f32(0), drift=f32(0), gap=f32(0),
               pose=np.eye(4, dtype=f32))
    listed = np.asarray(inlier_index, np.int64) if status == 0 else np.arange(cnt)
    q, t = np.asarray(mq, np.int64)[listed], np.asarray(mt, np.int64)[listed]
    # correspondence j = (query keypoint, point of train row, candidate keypoint of that row).  In rs_map kp_point and the
    # observation list are one fact, so set_correspondences' search of observations() for the candidate (:129-138) always
    # finds the keypoint the row came from: nothing is ever skipped.
    out.update(listed=len(listed), query_kp=q.astype(np.int32), point=np.asarray(kp_point_c)[rows[t]].astype(np.int32),
               candidate_kp=rows[t].astype(np.int32))
    if status == 0:
        out.update(inliers=len(listed), pose=np.asarray(pose, f32).reshape(4, 4))
        out.update(verdict(pose, np.asarray(kp_q, f32)[q, 0], width, query_centre, candidate_centre, cnt, len(listed)))
    return out


def verify_pnp(query, candidate, pos, K, width, max_distance=64, threshold_px=PNP_REPROJ_ERROR, confidence=0.99,
               max_hypotheses=200, seed=0):
    """query / candidate: dict(desc, kp, kp_point, pose).  Returns finish()'s dict plus rows, mq, mt and pnp (the
    restatement's full result, None when PnP was not run)."""
    rows = candidate_rows(candidate["kp_point"])
    train = np.asarray(candidate["desc"], np.uint8).reshape(-1, 32)[rows]
    mq, mt = match_ref.match_descriptors(np.asarray(query["desc"], np.uint8).reshape(-1, 32), train, max_distance)
    obj = np.asarray(pos, f32).reshape(-1, 3)[np.asarray(candidate["kp_point"])[rows]]
    qc, cc = centre_of(query["pose"]), centre_of(candidate["pose"])
    pnp = None
    if len(mq) < MIN_PNP_CORRESPONDENCES:                                         # :183-186
        status, pose, inl = 1, None, []
    else:
        pnp = pnp_ref.estimate_pose_pnp(obj, query["kp"], K, threshold_px, confidence, max_hypotheses, seed, object_index=mt,
                                        pixel_index=mq)
        inl = np.flatnonzero(pnp["mask"])
        status, pose = (2, None) if (pnp["status"] != 0 or len(inl) == 0) else (0, pnp["pose"])       # :215-218
    out = finish(status, pose, inl, mq, mt, rows, candidate["kp_point"], query["kp"], width, qc, cc)
    out.update(rows=rows, mq=mq, mt=mt, pnp=pnp, obj=obj)
    return out


def best_candidate(verifications):
    """:267-285 over dicts with ok and inliers."""
    best, found = 0, False
    for i, v in enumerate(verifications):
        if v["ok"] and (not found or v["inliers"] > verifications[best]["inliers"]):
            best, found = i, True
    if not found:
        for i in range(1, len(verifications)):
            if verifications[i]["inliers"] > verifications[best]["inliers"]:
                best = i
    return best


class LoopState:
    """What Impl keeps between queries: the streak (:336), the constraints (:324) and new_loop (:325)."""

    def __init__(self):
        self.streak, self.constraints, self.new_loop, self.last = [], [], False, None

    def consume_new_loop(self):
        added, self.new_loop = self.new_loop, False
        return added


def publish(ranked_index, ranked_score, verifications):
    """publish_result (:287-308): what last() shows of the displayed candidate."""
    d = best_candidate(verifications)
    return dict(candidate_index=int(ranked_index[d]), score=float(ranked_score[d]), matches=int(verifications[d]["inliers"]),
                verified=bool(verifications[d]["ok"]), edges=[bool(v["ok"]) for v in verifications], display=d)


def update_streak(state, frm, ranked_index, verifications, candidate_poses):
    """:375-442.  ranked_index [n]: the candidates' key-frame indices; candidate_poses [n][4][4] f32 their poses.  Returns
    the chosen candidate or -1.  Nothing ranked (LoopDetector::query :495-499) clears the streak."""
    if len(ranked_index) == 0:
        state.streak = []
        return -1
    seed = best_candidate(verifications)
    if not verifications[seed]["ok"]:
        state.streak = []
        return -1
    chosen = seed
    consecutive = bool(state.streak) and frm == state.streak[-1]["query_index"] + 1
    if consecutive:
        continued = len(ranked_index)
        for i in range(len(ranked_index)):
            gap = abs(int(ranked_index[i]) - state.streak[-1]["candidate_index"])
            if not verifications[i]["ok"] or gap > CONSISTENCY_WINDOW:
                continue
            if continued == len(ranked_index) or verifications[i]["inliers"] > verifications[continued]["inliers"]:
                continued = i
        if continued < len(ranked_index):
            chosen = continued
        else:
            state.streak = []
    else:
        state.streak = []
    v = verifications[chosen]
    state.streak.append(dict(query_index=int(frm), candidate_index=int(ranked_index[chosen]), pose=np.array(v["pose"], f32),
                             inliers=int(v["inliers"]), drift=v.get("drift", f32(0)),
                             pairs=np.stack([v.get("query_kp", np.zeros(0, np.int32)), v.get("point", np.zeros(0, np.int32))], 1)))
    if len(state.streak) < MIN_CONSISTENT:
        return chosen
    hit = state.streak[-1]
    for c in state.constraints:
        if abs(int(frm) - c["from"]) < MIN_LOOP_SEPARATION and abs(hit["candidate_index"] - c["to"]) < MIN_LOOP_SEPARATION:
            return chosen
    relative = hit["pose"].astype(np.float64) @ np.linalg.inv(np.asarray(candidate_poses[chosen], np.float64).reshape(4, 4))
    state.constraints.append({"from": int(frm), "to": hit["candidate_index"], "relative": relative, "pairs": hit["pairs"]})
    state.new_loop = True
    return chosen
