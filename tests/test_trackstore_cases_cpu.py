"""The cases of tests/trackstore_cases.py without a GPU: every sequence is stepped through the specification
(tests/trackstore_ref.py) and through the entry-by-entry object model of tests/test_trackstore_cpu.py, the key frame that
follows goes through ref.pack and the oracle, and each case is held to the condition it exists for — so that the GPU test
of the same case (tests/test_gpu_trackstore_envelope.py) cannot pass on a case that silently degenerated."""
import numpy as np
import pytest

import trackstore_cases as TC
import trackstore_ref as R
from test_trackstore_cpu import Model


class Stepped(Model):
    carry = Model.carry_forward


def light(ref, model):
    ids = sorted(model.tracks)
    assert ref.id.tolist() == ids and ref.next_id == model.next_id
    assert ref.keypoint.tolist() == [model.tracks[t].keypoint for t in ids]
    assert ref.count.tolist() == [len(model.tracks[t].sightings) for t in ids]
    return ids


def full(ref, model):
    """test_trackstore_cpu.same with the sightings as bytes (a NaN pixel equals itself)"""
    for a, t in enumerate(light(ref, model)):
        assert ref.sightings[a, :ref.count[a]].tobytes() == np.array(model.tracks[t].sightings, R.SIGHTING).tobytes()
    assert {int(k): int(ref.id[a]) for a, k in enumerate(ref.keypoint)} == model.by_keypoint


def run(case):
    """both forms through the case's calls: compared in full after every call where the store is small, else ids,
    keypoints and counts after every call and in full at the end"""
    ref, model = R.Store(case["cap"], case["max_sightings"]), Stepped(case["cap"], case["max_sightings"])
    small = case["cap"] * case["max_sightings"] <= 2048
    seen = dict(disorder=False, emptied=False)
    for step in case["steps"]:
        getattr(ref, step[0])(*step[1:])
        getattr(model, step[0])(*step[1:])
        (full if small else light)(ref, model)
        seen["disorder"] |= bool(np.any(np.diff(ref.keypoint) < 0))
        seen["emptied"] |= step[0] == "carry" and len(ref.id) == 0
    full(ref, model)
    return ref, seen


def pose_index(ref, tri, t):
    return ref.sightings[t, :ref.count[t]]["frame"].astype(np.int64) - tri["pose_base"]


@pytest.mark.parametrize("cap", TC.RAGGED_CAPS)
def test_ragged_capacities(cap):
    case = TC.ragged(cap, repeats=cap == 1025)
    assert cap == 1 or cap % TC.THREADS                       # the last owning thread's run of rows is short
    ref, seen = run(case)
    forms = [(s[2] is None, s[3]) for s in case["steps"] if s[0] == "carry"]
    assert [f[0] for f in forms] == [False, cap == 1, True, False, False]      # (one keypoint: the junk form has no list)
    assert forms[1][1] > case["steps"][3][4] and forms[2][1] is None and forms[3][1] < 0 and forms[4][1] == 0
    assert seen["emptied"] and len(ref.id) == cap and (cap < 63 or seen["disorder"])
    sizes = [len(s[1]) for s in case["steps"] if s[0] == "extend"]
    assert sizes == [cap, cap - 1, cap, (cap + 1) // 2, 1, cap]
    if cap == 1025:                                           # repeats on both sides of the list
        prev, inl = case["steps"][1][1:3]
        assert len(np.unique(prev)) < len(prev) and len(np.unique(inl)) < len(inl)


@pytest.mark.parametrize("T,cap,bad", TC.PACK_SHAPES)
def test_pack_shapes(oracle, T, cap, bad):
    case = TC.pack_case(T, cap, bad)
    ref, seen = run(case)
    e = TC.expected(ref, case["tri"], oracle)
    assert len(ref.id) == T and (T <= 1024 or T % 4) and len(e["pack"]["skip"]) == T
    if T > 3:
        assert seen["disorder"] and e["counts"][0] > T // 4 and e["counts"][2] > 0 and e["pack"]["skip"].sum() > 0
        assert len(set(ref.count.tolist())) > 2 and e["n_pairs"] > 0
    if (T, cap) == (2049, 2049):
        assert e["counts"][0] > 1024                          # k_ts_results: two accepted tracks per thread
    if (T, cap) == (2049, 2500):
        assert e["counts"][2] > 1024                          # k_ts_results' and k_ts_erase's second trip over the inconsistent list


def test_full_size(oracle):
    case = TC.full_size()
    ref, seen = run(case)
    e = TC.expected(ref, case["tri"], oracle)
    assert len(ref.id) == case["cap"] == 8192 and seen["disorder"]
    assert e["counts"][0] > 1024 and e["counts"][2] > 0 and e["pack"]["skip"].sum() > 0


def test_long_tracks(oracle):
    case = TC.long_tracks()
    ref, _ = run(case)
    tri = case["tri"]
    e = TC.expected(ref, tri, oracle)
    assert {1, 63, 64, 65, 127, 128} <= set(ref.count.tolist()) and len(case["steps"]) == 2 * 130
    by_kp = {int(k): t for t, k in enumerate(ref.keypoint)}
    n_poses = len(tri["poses"])
    out = {name: (lambda p: np.flatnonzero((p < 0) | (p >= n_poses)))(pose_index(ref, tri, by_kp[kp])) for name, kp in TC.LONG_ROLES.items()}
    assert out["first"].tolist() == [0] and out["late"].tolist() == [127] and out["ends"].tolist() == [0, 127] and len(out["kept"]) == 0
    assert e["pack"]["out_of_range"] == 4 >= 3
    # the track of keypoint 1 holds 128 sightings, lost the key-frame sighting of frame 129 and is accepted without it
    t = by_kp[TC.LONG_ROLES["kept"]]
    a = e["track"].tolist().index(t)
    assert ref.count[t] == 128 and ref.sightings[t, 127]["frame"] == 128
    pairs = e["kf_pairs"][e["kf_ptr"][a]:e["kf_ptr"][a + 1]]
    assert pairs[:, 0].tolist() == list(range(1, 13)) and 13 not in e["kf_pairs"][:, 0]
    assert ("extend", 129, 13) == (case["steps"][-2][0],) + case["steps"][-2][2:]
    # accepted tracks on both sides of the copy's 64-lane trip
    assert {63, 64, 65, 127, 128} <= set(e["sightings"].tolist())


def test_many_pairs(oracle):
    case = TC.many_pairs()
    ref, _ = run(case)
    e = TC.expected(ref, case["tri"], oracle)
    T = len(ref.id)
    assert e["n_pairs"] > 2 * T + 5 and T == 50
    per = np.diff(e["kf_ptr"])
    assert np.any((per == e["sightings"]) & (per == 6)) and np.count_nonzero(per == 0) >= 3


def test_id_spread(oracle):
    case = TC.id_spread()
    ref, seen = run(case)
    assert ref.next_id >= 2 ** 19 and int(ref.id.max() - ref.id.min()) >= 2 ** 19 and len(ref.id) == 8192
    assert ref.id[:2].tolist() == [0, 8191] and ref.keypoint[:2].tolist() == [8000, 5] and seen["disorder"]
    # as 32-bit words the keys (id - min id) << 13 | row of the young tracks fall below that of id 8191
    assert ((int(ref.id[2]) << 13) & 0xFFFFFFFF) < (8191 << 13)
    e = TC.expected(ref, case["tri"], oracle)
    assert e["pack"]["sight_ptr"][:3].tolist() == [0, 2, 4] and e["status"][0] == 1


def test_query_at_size():
    q = TC.query_at_size()
    assert set(q["n_obs"].tolist()) == set(range(7)) and np.any(q["table"] >= q["P"])
    for name, min_sightings in (("single", 1), ("moving", 3)):
        case = q[name]
        ref, _ = run(case)
        counts = {}
        for last_kf in (-1, 0, 3, 5):
            for min_travel in (0.0, 20.0):
                got = ref.query(q["table"], TC.covisible(q["n_obs"], q["dead"], last_kf), min_sightings, min_travel)
                counts[last_kf, min_travel] = (got["covisible"], got["waiting"])
        cov = [counts[k, 0.0][0] for k in (-1, 0, 3, 5)]
        assert cov[0] == 0 and cov[1] > cov[2] > cov[3] > 0
        if name == "single":
            assert counts[0, 0.0][1] == int(np.count_nonzero(q["table"] < 0)) and counts[0, 20.0][1] == 0
        else:
            with np.errstate(invalid="ignore"):
                travel = ref.travel()
            odd = np.flatnonzero(~np.isfinite(travel))         # NaN and +inf: neither is below min_travel, both wait
            assert np.isnan(travel[odd]).tolist() == [True, False] and np.all(ref.count[odd] == 3) and np.all(q["table"][ref.keypoint[odd]] < 0)
            assert 2 < counts[0, 20.0][1] < counts[0, 0.0][1]
