"""CPU specification of the tail of Tracker::track on a frame's match table (racing-slam_amd/csrc/frame_matches.hip;
reference src/Tracker.cpp:83-86, :197-248, :302-320, src/Frame.cpp:80-102).

A table is an int32 array, keypoint -> point slot or -1, whose points are unique.  The map is what the stages read of
it: alive [P] u8, n_obs [P] (observations per point), consistent [P] u8, positions [P][3] f32.

matches_add is written as the closed form the kernel uses, not as the loop of Frame::add_map_match:
tests/test_track_cpu.py holds it against that loop on an independent object model.
"""
import numpy as np

MIN_TRACKED_MAP_POINTS = 15
MIN_OBSERVATIONS_TO_OPTIMIZE = 2


def clamp_count(count, max_n):
    return max_n if count is None else min(max(int(count), 0), max_n)


def matches_add(table, kp, point, count=None, max_n=None):
    """Frame::add_map_match for the first n list entries in list order, n = clamp(count, 0, max_n).  Keypoint k ends with
    the point of the LAST entry naming k if that entry is also the last one naming its point, else with -1; a keypoint no
    entry names keeps its point unless an entry names that point.  Entries with a keypoint outside the table or a
    negative point are skipped."""
    table = np.array(table, np.int32)
    kp, point = np.asarray(kp, np.int64), np.asarray(point, np.int64)
    n = clamp_count(count, len(kp) if max_n is None else max_n)
    idx = np.arange(n)
    ok = (kp[:n] >= 0) & (kp[:n] < len(table)) & (point[:n] >= 0)
    idx, k, p = idx[ok], kp[:n][ok], point[:n][ok]
    last_of_kp, last_of_point = {}, {}
    for i, kk, pp in zip(idx, k, p):
        last_of_kp[int(kk)] = int(i)
        last_of_point[int(pp)] = int(i)
    for kk in range(len(table)):
        t = last_of_kp.get(kk)
        if t is not None:
            table[kk] = point[t] if last_of_point[int(point[t])] == t else -1
        elif table[kk] >= 0 and int(table[kk]) in last_of_point:
            table[kk] = -1
    return table


def num_matches(table):
    return int(np.count_nonzero(np.asarray(table) >= 0))


def carry_candidates(alive, n_obs, consistent, prev_table, n_next, prev_index, inlier_index=None, count=None, max_n=None):
    """The first loop of Tracker::track_from_last_frame (:204-214): (list position, next's keypoint, point) of every
    candidate, in list order."""
    prev_index = np.asarray(prev_index, np.int64)
    max_n = len(prev_index) if max_n is None else max_n
    n = clamp_count(count, max_n)
    P = len(alive)
    cand = []
    for i in range(n):
        j = int(inlier_index[i]) if inlier_index is not None else i
        if j < 0 or j >= min(max_n, n_next):
            continue
        kq = int(prev_index[j])
        if kq < 0 or kq >= len(prev_table):
            continue
        p = int(prev_table[kq])
        if p < 0 or p >= P or not alive[p]:
            continue
        if n_obs[p] < 2 and not consistent[p]:            # :209
            continue
        cand.append((i, j, p))
    return cand


def carry(alive, n_obs, consistent, prev_table, next_table, prev_index, inlier_index=None, count=None, max_n=None,
          min_points=MIN_TRACKED_MAP_POINTS):
    """Tracker::track_from_last_frame (:197-230).  Returns (next's table, candidates, accepted).  A dead slot in prev's
    table (undefined behaviour in the reference) is no candidate."""
    nxt = np.array(next_table, np.int32)
    cand = [(j, p) for _, j, p in carry_candidates(alive, n_obs, consistent, prev_table, len(nxt), prev_index, inlier_index, count, max_n)]
    if len(cand) < min_points:                            # :216-219
        return nxt, len(cand), 0
    accepted = 0
    taken = set(int(p) for p in nxt if p >= 0)
    for j, p in cand:                                     # :222-228
        if nxt[j] >= 0 or p in taken:
            continue
        nxt[j] = p
        taken.add(p)
        accepted += 1
    return nxt, len(cand), accepted


def gather(table, keypoints, alive, n_obs, positions, min_matches=MIN_TRACKED_MAP_POINTS):
    """optimization::refine_pose's walk over Frame::map_matches() (ascending keypoint): (points [n][3] f64, uv [n][2] f32,
    n_used) with n_used = -1 when the table holds fewer than min_matches matches (:307; points and uv are empty then)."""
    table = np.asarray(table)
    P = len(alive)
    if num_matches(table) < min_matches:
        return np.zeros((0, 3)), np.zeros((0, 2), np.float32), -1
    keep = [k for k in range(len(table))
            if 0 <= table[k] < P and alive[table[k]] and n_obs[table[k]] >= MIN_OBSERVATIONS_TO_OPTIMIZE]
    pts = np.asarray(positions, np.float32)[table[keep]].astype(np.float64).reshape(-1, 3)
    uv = np.asarray(keypoints, np.float32)[keep].reshape(-1, 2)
    return pts, uv, len(keep)


def refine(solver, cam, table, keypoints, alive, n_obs, positions, K, min_matches=MIN_TRACKED_MAP_POINTS, prior=None, delta=None,
           options=None):
    """Tracker::optimize_pose's refit.  `solver` is anything with refine_pose_inertial(cam, points, uv, K, prior=, delta=,
    options=) -> cam, velocity, summary: the oracle, or a GPU context fed device copies by the caller.  Returns cam,
    velocity, summary (None when a gate refused the solve), n_used."""
    pts, uv, n = gather(table, keypoints, alive, n_obs, positions, min_matches)
    if n <= 0:
        vel = np.zeros(3) if delta is None else np.array(delta["velocity"], np.float64)
        return np.array(cam, np.float64), vel, None, n
    cam, vel, s = solver.refine_pose_inertial(cam, pts, uv, K, prior=prior, delta=delta, options=options)
    return cam, vel, s, n


def match_inputs(table):
    """What MapMatcher::match reads of the frame: Frame::is_matched per keypoint (:81) and the matched points (:53)."""
    table = np.asarray(table)
    return (table >= 0).astype(np.uint8), table[table >= 0].astype(np.int32)


def match_fold(table, match_kp, match_point):
    """Tracker::match_with_last_key_frame / match_with_map's loop of add_map_match (:235-237, :244-246)."""
    return matches_add(table, match_kp, match_point)


def match(oracle, frame, mp, table, required_kf=-1, max_distance=64):
    """match_key_frame / match_map through the oracle on flat arrays (frame, mp: synth.make_match_scene's dicts; mp's
    `eligible` = alive), folded into the table.  Returns (table, count)."""
    matched, pts = match_inputs(table)
    elig = np.array(mp["eligible"], np.uint8)
    elig[pts[pts < len(elig)]] = 0
    if required_kf >= 0:
        ptr = np.asarray(mp["obs_ptr"])
        for p in range(len(elig)):
            if not np.any(np.asarray(mp["obs_kf"])[ptr[p]:ptr[p + 1]] == required_kf):
                elig[p] = 0
    r = oracle.reproj_match(dict(frame, kp_matched=matched), dict(mp, eligible=elig), replace=0, max_distance=max_distance)
    return match_fold(table, r["match_kp"], r["match_point"]), len(r["match_kp"])
