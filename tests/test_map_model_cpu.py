"""Pins the host model of the map (tests/map_model.py: Map::associate / disassociate / remove_point / fuse, reference
src/Map.cpp:44-124, and the local-BA window of src/Optimization.cpp:287-315) independently of the device: hand-worked
cases for each branch of the edits, agreement of the two directions of the graph after long random edit sequences, and a
second, point-side formulation of the BA window."""
import numpy as np
import pytest

from map_model import EDIT_WEIGHTS, MapModel, random_edit


def small_map(n_kf=3, n_kp=5, n_points=4):
    m = MapModel()
    for k in range(n_kf):
        m.add_keyframe(np.arange(2 * n_kp, dtype=np.float32).reshape(-1, 2) + 100 * k, np.full((n_kp, 32), k, np.uint8),
                       np.eye(4, dtype=np.float32))
    for p in range(n_points):
        m.add_point([p, 0, 1])
    return m


def tables(m):
    return [t.tolist() for t in m.kp_point]


# ------------------------------------------------------------------------------------------ associate (:95-113)
def test_associate_same_pair_is_a_no_op():
    m = small_map()
    m.associate(0, 1, 2)
    m.associate(1, 1, 0)
    before = (list(map(list, m.obs)), tables(m))
    assert m.associate(0, 1, 2) == [("add_observation", 1, 0, 2)]      # :97-100
    assert (list(map(list, m.obs)), tables(m)) == before
    assert m.obs[1] == [(0, 2), (1, 0)]                                 # insertion order kept: no re-append


def test_associate_steals_an_occupied_keypoint():
    m = small_map()
    m.associate(0, 1, 2)
    m.associate(1, 1, 4)
    m.associate(0, 3, 2)                                                # :101-106 point 1 loses keypoint 2 of kf 0
    assert m.obs[1] == [(1, 4)] and m.obs[3] == [(0, 2)]
    assert tables(m)[0] == [-1, -1, 3, -1, -1] and tables(m)[1] == [-1, -1, -1, -1, 1]
    assert m.consistent()


def test_associate_moves_the_point_to_another_keypoint_of_the_same_key_frame():
    m = small_map()
    m.associate(2, 0, 1)
    m.associate(0, 0, 3)
    m.associate(2, 0, 4)                                                # :107-109 the old keypoint is freed
    assert m.obs[0] == [(0, 3), (2, 4)]                                 # the re-associated observation goes last
    assert tables(m)[2] == [-1, -1, -1, -1, 0]
    # both branches at once: the point moves onto a keypoint that another point holds
    m.associate(2, 1, 2)
    m.associate(2, 0, 2)
    assert m.obs[1] == [] and m.obs[0] == [(0, 3), (2, 2)] and tables(m)[2] == [-1, -1, 0, -1, -1]
    assert m.consistent()


# ------------------------------------------------------------------------------------------ the other edits
def test_disassociate_of_an_absent_key_frame_is_a_no_op():
    m = small_map()
    m.associate(0, 2, 1)
    before = (list(map(list, m.obs)), tables(m))
    assert m.disassociate(1, 2) == [("remove_observation", 2, 1)]      # :118-120
    assert (list(map(list, m.obs)), tables(m)) == before
    m.disassociate(0, 2)
    assert m.obs[2] == [] and tables(m)[0] == [-1] * 5


def test_remove_point_clears_its_observers_tables_and_keeps_the_slot():
    m = small_map()
    for kf, kp in [(0, 1), (1, 3), (2, 0)]:
        m.associate(kf, 2, kp)
    m.associate(1, 0, 0)
    m.set_position(2, [7, 8, 9])
    assert m.remove_point(2) == [("remove_point", 2)]
    assert tables(m) == [[-1] * 5, [0, -1, -1, -1, -1], [-1] * 5]
    assert m.obs[2] == [] and m.alive == [1, 1, 0, 1]
    assert m.counts() == dict(slots=4, alive=3, observations=1, key_frames=3)
    assert np.array_equal(m.positions()[2], np.float32([7, 8, 9]))    # a dead slot keeps its last position
    assert m.add_point([0, 0, 0])[0] == 4                               # slots are never reused


def test_fuse_branches():
    m = small_map()
    assert m.fuse(1, 1) == (["same"], [])                               # :80-82
    # discarded 0 seen by kf 0, 1, 2; kept 1 already seen by kf 1
    for kf, kp in [(0, 0), (1, 1), (2, 2)]:
        m.associate(kf, 0, kp)
    m.associate(1, 1, 4)
    outcomes, calls = m.fuse(1, 0)
    assert outcomes == ["moved", "kept_observed", "moved"]             # :86 first condition
    assert m.obs[1] == [(1, 4), (0, 0), (2, 2)] and m.alive[0] == 0 and m.obs[0] == []
    assert tables(m) == [[1, -1, -1, -1, -1], [-1, -1, -1, -1, 1], [-1, -1, 1, -1, -1]]
    assert calls == [("remove_observation", 0, 0), ("add_observation", 1, 0, 0), ("remove_observation", 0, 1),
                     ("remove_observation", 0, 2), ("add_observation", 1, 2, 2), ("remove_point", 0)]
    assert m.consistent()


def test_fuse_second_and_third_skip_conditions_follow_from_the_first():
    """frame->is_matched(index) and frame->is_matched(kept) (:86) are evaluated after disassociate(frame, discarded)
    has freed `index`: in a consistent map the first can never hold and the second holds exactly when
    kept.is_observed_by(frame) does.  So on every reachable map a fuse only ever moves or skips as 'kept_observed'."""
    rng = np.random.default_rng(11)
    m = small_map(n_kf=4, n_kp=6, n_points=30)
    seen = set()
    for _ in range(3000):
        kind, _ = random_edit(m, rng, dict(EDIT_WEIGHTS, fuse=4))
        alive = m.alive_points()
        if len(alive) > 1:
            a, b = rng.choice(alive, 2, replace=False)
            seen.update(m.fuse(int(a), int(b))[0])
        if len(m.alive_points()) < 10:
            m.create_point([0, 0, 1], [])
    assert seen == {"moved", "kept_observed"}


# ------------------------------------------------------------------------------------------ long random sequences
@pytest.mark.parametrize("seed", [0, 1])
def test_two_directions_agree_after_random_edits(seed):
    rng = np.random.default_rng(seed)
    m = small_map(n_kf=6, n_kp=40, n_points=150)
    kinds = {k: 0 for k in EDIT_WEIGHTS}
    n_obs_calls = 0
    for i in range(10_000):
        kind, calls = random_edit(m, rng)
        kinds[kind] += 1
        n_obs_calls += sum(c[0] == "remove_observation" for c in calls)
        if i % 2500 == 2499:
            n_kp = int(rng.integers(0, 3)) * 20                       # key frames added mid-sequence, some empty
            m.add_keyframe(rng.uniform(0, 500, (n_kp, 2)), np.zeros((n_kp, 32), np.uint8), np.eye(4))
            assert m.consistent()
    assert m.consistent()
    assert min(kinds.values()) > 100 and n_obs_calls > 1000
    c = m.counts()
    assert c["observations"] == sum(int((t >= 0).sum()) for t in m.kp_point) > 100
    assert 0 < c["alive"] < c["slots"]


# ------------------------------------------------------------------------------------------ the BA window
def random_edited_map(seed, n_kf=8, n_kp=30, n_points=120, n_edits=1500):
    rng = np.random.default_rng(seed)
    m = small_map(n_kf=n_kf, n_kp=n_kp, n_points=n_points)
    for p in range(n_points):
        for kf in rng.choice(n_kf, int(rng.integers(0, 4)), replace=False):
            m.associate(int(kf), p, int(rng.integers(n_kp)))
    for _ in range(n_edits):
        random_edit(m, rng)
    return m, rng


def residual_multiset(w, kfs):
    return sorted((int(w["points"][i]), int(w["obs_cam"][o]), *w["obs_uv"][o].tolist())
                  for i in range(len(w["points"])) for o in range(w["obs_ptr"][i], w["obs_ptr"][i + 1]))


@pytest.mark.parametrize("seed", range(6))
def test_ba_window_frame_side_equals_point_side(seed):
    m, rng = random_edited_map(seed)
    n = m.n_kf()
    windows = [(np.arange(n), np.r_[np.zeros(2), np.ones(n - 2)]),                                  # identity
               (np.sort(rng.choice(n, 4, replace=False)), np.ones(4)),                                # ascending subset
               (rng.permutation(n), rng.integers(0, 2, n)),                                           # permutation
               (rng.permutation(n)[:5], np.array([0, 1, 0, 1, 0])),                                   # fixed interleaved
               (rng.permutation(n)[:1], np.ones(1)),                                                  # single free frame
               (rng.permutation(n)[:3], np.zeros(3))]                                                 # all fixed
    for kfs, free in windows:
        kfs, free = np.asarray(kfs, np.int32), np.asarray(free, np.uint8)
        a, b = m.ba_window(kfs, free), m.ba_window_pointside(kfs, free)
        assert np.array_equal(a["points"], b["points"])
        assert np.array_equal(a["obs_ptr"], b["obs_ptr"]) and np.array_equal(a["obs_cam"], b["obs_cam"])
        assert np.array_equal(a["obs_uv"], b["obs_uv"])
        assert residual_multiset(a, kfs) == residual_multiset(b, kfs)
        if not free.any():
            assert len(a["points"]) == 0
        for i, p in enumerate(a["points"]):
            cams = a["obs_cam"][a["obs_ptr"][i]:a["obs_ptr"][i + 1]]
            assert len(m.obs[p]) >= 2 and any(free[c] for c in cams) and np.all(np.diff(cams) > 0)


def test_ba_window_hand_worked():
    """Points that are free only through observers outside the window, whose only listed observer is fixed, and
    residuals of fixed frames."""
    m = small_map(n_kf=4, n_kp=4, n_points=6)
    m.associate(0, 0, 0); m.associate(1, 0, 0)            # p0: kf0 (fixed) + kf1 (free)
    m.associate(1, 1, 1); m.associate(3, 1, 1)            # p1: kf1 (free) + kf3 (outside): >= 2 only through kf3
    m.associate(0, 2, 2); m.associate(2, 2, 2)            # p2: kf0 (fixed) + kf2 (fixed): no free observer
    m.associate(1, 3, 3)                                  # p3: one observation
    m.associate(0, 4, 3); m.associate(3, 4, 3)            # p4: only listed observer fixed
    m.associate(2, 5, 1); m.associate(1, 5, 2); m.remove_point(5)
    kfs, free = np.array([2, 1, 0], np.int32), np.array([0, 1, 0], np.uint8)
    for w in (m.ba_window(kfs, free), m.ba_window_pointside(kfs, free)):
        assert w["points"].tolist() == [0, 1]
        assert w["obs_ptr"].tolist() == [0, 2, 3]
        assert w["obs_cam"].tolist() == [1, 2, 1]          # list order: kf1 is list index 1, kf0 is 2
        assert np.array_equal(w["obs_uv"], np.float32([m.kf_kp[1][0], m.kf_kp[0][0], m.kf_kp[1][1]]))
