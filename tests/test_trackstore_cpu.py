"""tests/trackstore_ref.py (closed forms over whole lists) against an object model of the same rules — a dict of
id -> Track stepped entry by entry as src/TrackStore.cpp and src/Mapper.cpp:91-120 read — on random sequences, and
rs_needs_key_frame (host only: no device) through the library against hand-computed cases."""
import numpy as np
import pytest

import trackstore_ref as R


class Track:
    def __init__(self, keypoint):
        self.sightings, self.keypoint = [], keypoint


class Model:
    def __init__(self, max_points, max_sightings):
        self.cap, self.max_sightings, self.tracks, self.by_keypoint, self.next_id = max_points, max_sightings, {}, {}, 0

    def carry_forward(self, prev_index, inlier_index, count, max_n):
        n = max_n if count is None else min(max(count, 0), max_n)
        carried, by_keypoint, named = {}, {}, set()
        for i in range(n):
            j = i if inlier_index is None else int(inlier_index[i])
            if j < 0 or j >= min(max_n, self.cap):
                continue
            q = int(prev_index[j])
            if q not in self.by_keypoint:
                continue
            if q in named:
                continue
            named.add(q)
            if j in by_keypoint:
                continue
            tid = self.by_keypoint[q]
            self.tracks[tid].keypoint = j
            by_keypoint[j] = tid
            carried[tid] = self.tracks[tid]
        self.tracks, self.by_keypoint = carried, by_keypoint

    def extend(self, pixels, frame_index, key_frame):
        for i in range(len(pixels)):
            if i not in self.by_keypoint:
                self.by_keypoint[i] = self.next_id
                self.tracks[self.next_id] = Track(i)
                self.next_id += 1
            s = self.tracks[self.by_keypoint[i]].sightings
            if len(s) < self.max_sightings:
                s.append((frame_index, np.float32(pixels[i][0]), np.float32(pixels[i][1]), key_frame, i))

    def erase(self, tid):
        if tid in self.tracks:
            del self.by_keypoint[self.tracks[tid].keypoint]
            del self.tracks[tid]

    def unmapped_tracks(self, table, min_sightings, min_travel):
        count = 0
        for tid in sorted(self.tracks):
            t = self.tracks[tid]
            if len(t.sightings) < min_sightings:
                continue
            if t.keypoint < len(table) and table[t.keypoint] >= 0:
                continue
            dx, dy = np.float32(t.sightings[-1][1] - t.sightings[0][1]), np.float32(t.sightings[-1][2] - t.sightings[0][2])
            if np.sqrt(np.float32(np.float32(dx * dx) + np.float32(dy * dy))) < np.float32(min_travel):
                continue
            count += 1
        return count


def same(ref, model):
    ids = sorted(model.tracks)
    assert ref.id.tolist() == ids and ref.next_id == model.next_id
    assert ref.keypoint.tolist() == [model.tracks[t].keypoint for t in ids]
    assert ref.count.tolist() == [len(model.tracks[t].sightings) for t in ids]
    for a, t in enumerate(ids):
        got = [tuple(r) for r in ref.sightings[a, :ref.count[a]].tolist()]
        assert got == [(f, float(x), float(y), kf, kp) for f, x, y, kf, kp in model.tracks[t].sightings]
    assert {int(k): int(ref.id[a]) for a, k in enumerate(ref.keypoint)} == model.by_keypoint


def random_lists(rng, n_prev, n_next, repeats, junk):
    """a kept-index list (current keypoint -> previous keypoint) and an inlier list over it"""
    m = int(rng.integers(0, n_next + 1))
    prev = np.sort(rng.choice(n_prev, min(m, n_prev), replace=False)).astype(np.int32) if not repeats else rng.integers(0, max(1, n_prev // 2), m).astype(np.int32)
    m = len(prev)
    inl = np.flatnonzero(rng.random(m) < 0.7).astype(np.int32)
    if repeats and len(inl):
        inl = rng.choice(inl, len(inl) + 3).astype(np.int32)
    if junk and m:
        prev[rng.random(m) < 0.1] = rng.choice([-1, n_prev + 7, 2 ** 30, -2 ** 31])
        inl = np.concatenate([inl, np.array([-1, m, m + 5, 2 ** 30], np.int32)])
        rng.shuffle(inl)
    return prev, inl


@pytest.mark.parametrize("seed,max_sightings,repeats,junk", [(0, 100, False, False), (1, 3, False, True), (2, 2, True, False), (3, 1, True, True),
                                                             (4, 5, False, False)])
def test_specification_equals_the_object_model(seed, max_sightings, repeats, junk):
    rng = np.random.default_rng(seed)
    cap = 96
    ref, model = R.Store(cap, max_sightings), Model(cap, max_sightings)
    n_prev = 0
    for frame in range(25):
        n = int(rng.integers(1, cap + 1))
        pixels = rng.uniform(0, 40, (n, 2)).astype(np.float32)
        if frame:
            prev, inl = random_lists(rng, n_prev, n, repeats, junk)
            form = frame % 4
            inlier, count, max_n = (None, None, len(prev)) if form == 0 else (inl, len(inl), len(prev))
            if form == 2:
                count = len(inl) + 5                       # clamped to max_n: the list must hold max_n entries
                inlier = np.concatenate([inl, np.zeros(max(0, len(prev) - len(inl)), np.int32)])[:max(len(prev), 1)]
                count = min(count, len(inlier))
            if form == 3 and frame % 8 == 3:
                count = -3
            if inlier is not None and len(inlier) < max(count or 0, 0):
                count = len(inlier)
            ref.carry(prev, inlier, count, max_n)
            model.carry_forward(prev, inlier, count, max_n)
            same(ref, model)
        table = np.where(rng.random(n) < 0.3, rng.integers(0, 50, n), -1).astype(np.int32)
        q = ref.query(table, rng.random(50) < 0.5, 3, 20.0)
        assert q["waiting"] == model.unmapped_tracks(table, 3, 20.0) and q["live"] == len(model.tracks)
        if frame % 6 == 5 and len(ref.id):
            gone = rng.choice(len(ref.id), max(1, len(ref.id) // 4), replace=False)
            for tid in ref.id[gone].tolist():
                model.erase(tid)
            ref.erase(gone)
            same(ref, model)
        kf = frame // 5 if frame % 5 == 0 else -1
        ref.extend(pixels, frame, kf)
        model.extend(pixels, frame, kf)
        same(ref, model)
        n_prev = n
        p = ref.pack(table, pixels, max(0, frame - 10), 11)          # pack order = id order = the model's sorted ids
        ids = sorted(model.tracks)
        assert p["sight_ptr"].tolist() == np.concatenate([[0], np.cumsum([len(model.tracks[t].sightings) for t in ids])]).tolist()
        flat = [s for t in ids for s in model.tracks[t].sightings]
        assert p["sight_pose"].tolist() == [s[0] - max(0, frame - 10) for s in flat]
        want_skip = [int(table[model.tracks[t].keypoint] >= 0 or any(s[0] < frame - 10 for s in model.tracks[t].sightings)) for t in ids]
        assert p["skip"].tolist() == want_skip
    assert ref.next_id > cap


def test_query_counts_covisible_points_and_first_frame():
    ref = R.Store(8, 4)
    ref.extend(np.zeros((3, 2), np.float32), 7)
    table = np.array([2, -1, 0, 5, 9], np.int32)              # 9 is outside the map: a match, never covisible
    q = ref.query(table, np.array([True, True, False, False, False, True]), 1, 0.0)
    assert (q["covisible"], q["num_map_matches"], q["live"], q["first_frame"], q["waiting"]) == (2, 4, 3, 7, 1)
    assert R.Store(4, 1).query(np.zeros(0, np.int32), np.zeros(0, bool))["first_frame"] == -1


# (covisible, waiting, gap, last key frame's matches, constants or None) -> decision, each worked by hand
CASES = [
    ((1000, 0, 20, 100, None), True),        # the gap of exactly 20
    ((1000, 0, 19, 100, None), False),
    ((1000, 0, -1, 100, None), True),        # an unsigned gap that wrapped
    ((1000, 200, 3, 100, None), True),       # waiting of exactly 200
    ((1000, 199, 3, 100, None), False),
    ((50, 0, 3, 50, None), False),           # covisible of exactly 50: 50 < 50 no, 50 < 35 no
    ((49, 0, 3, 50, None), True),
    ((63, 0, 3, 90, None), False),           # 0.7f * 90 = 62.99999893 rounds to 63.0f: 63 < 63 no
    ((62, 0, 3, 90, None), True),
    ((100, 0, 3, 143, None), True),          # 0.7f * 143 = 100.1: 100 < 100.1
    ((101, 0, 3, 143, None), False),
    ((10, 0, 3, 100, (20, 200, 5, 0.1)), False),   # 0.1f * 100 = 10.00000015 rounds to 10.0f in f32 (f64 would say 10 < 10.00000015)
    ((9, 0, 3, 100, (20, 200, 5, 0.1)), True),
    ((4, 0, 3, 0, (20, 200, 5, 0.1)), True),       # below min_covisible_points
    ((75, 0, 5, 100, (5, 200, 50, 0.75)), True),   # other constants: the gap bound 5
    ((75, 0, 4, 100, (5, 200, 50, 0.75)), False),  # 75 < 75 no
]


@pytest.mark.parametrize("case,want", CASES)
def test_needs_key_frame_decision(rs, case, want):
    cov, waiting, gap, last, consts = case
    q = dict(covisible=cov, num_map_matches=cov + 5, waiting=waiting, live=2000, first_frame=0, next_id_low=0)
    args = () if consts is None else consts
    assert rs.needs_key_frame(q, gap, last, *args) is want
    assert R.needs_key_frame(q, gap, last, *args) is want
