"""rs_track_store (racing-slam_amd/csrc/track_store.hip) on the cases of tests/trackstore_cases.py: the shapes at which a
thread's run of rows or tracks is ragged or longer than one, the sort is wider than the workgroup, the copy kernel takes
a second trip, the read-back splits, and the sort key needs more than 32 bits.  tests/test_trackstore_cases_cpu.py holds
every case to the condition it exists for.

All comparisons are exact.  After every call the downloaded store equals the specification (tests/trackstore_ref.py);
after every triangulate call the packed arrays equal ref.pack byte for byte and the results equal the CPU oracle
(pyoracle.triangulate_tracks) run on ref.pack's arrays — so a wrong pack cannot cancel against the device's own
rs_triangulate_tracks — with the parallax requirement as one table (rs.parallax_requirements) and the key-frame pairs
from ref.key_frame_pairs."""
import ctypes as C

import numpy as np
import pytest

import trackstore_cases as TC
from conftest import to_np
from test_gpu_track import SimpleMap, set_table
from test_gpu_trackstore import Pair, make_frame

pytestmark = pytest.mark.gpu
PACK_ARRAYS = ("track_uv", "skip", "sight_ptr", "sight_pose", "sight_uv")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stepped(ctx, rs, case):
    """the device store and the specification through the case's calls, compared after every one"""
    p = Pair(ctx, rs, case["cap"], case["max_sightings"])
    TC.replay(case, p, after=lambda step: p.check())
    return p


def key_frame_of(ctx, rs, tri):
    fr = make_frame(ctx, rs, tri["pixels"])
    set_table(ctx, fr, tri["table"])
    return fr


def triangulate(ctx, rs, p, fr, tri, capacity_pairs=None):
    return p.dev.triangulate(fr, ctx.dev(tri["poses"]), tri["pose_base"], tri["kf_pose"], tri["K"], min_new_points=tri["min_new_points"],
                             d_required=ctx.dev(rs.parallax_requirements(tri["poses"], tri["kf_pose"])), capacity_pairs=capacity_pairs)


def compare(p, got, e, capacity_pairs=None):
    pk = p.dev.packed()
    for name in PACK_ARRAYS:
        assert pk[name].tobytes() == e["pack"][name].tobytes(), name
    assert got["out_of_range"] == e["pack"]["out_of_range"] and got["n_tracks"] == len(p.ref.id)
    assert got["counts"].tolist() == e["counts"].tolist()
    for name in ("track", "inconsistent", "keypoint", "sightings", "kf_ptr"):
        assert got[name].tobytes() == e[name].tobytes(), name
    for name in ("xyz", "parallax_cos", "required_cos"):
        assert np.array_equal(bits(got[name]), bits(e[name])), name
    assert got["n_pairs"] == e["n_pairs"] == got["kf_ptr"][-1]
    room = e["n_pairs"] if capacity_pairs is None else min(capacity_pairs, e["n_pairs"])
    assert got["kf_pairs"].tobytes() == e["kf_pairs"][:room].tobytes()


def against_the_device_kernel(ctx, rs, got, e, tri):
    """the second check: rs_triangulate_tracks on the host-built arrays, as tests/test_gpu_trackstore.py compares"""
    pack = e["pack"]
    host = ctx.triangulate_tracks(ctx.dev(pack["track_uv"]), ctx.dev(pack["sight_ptr"]), ctx.dev(pack["sight_pose"]), ctx.dev(pack["sight_uv"]),
                                  ctx.dev(tri["poses"]), tri["kf_pose"], tri["K"], d_skip=ctx.dev(pack["skip"]), min_new_points=tri["min_new_points"],
                                  d_required=ctx.dev(rs.parallax_requirements(tri["poses"], tri["kf_pose"])))
    counts = to_np(host["counts"])
    acc = to_np(host["accepted"])[:counts[0]]
    assert got["counts"].tobytes() == counts.tobytes() and got["track"].tobytes() == acc.tobytes()
    assert got["inconsistent"].tobytes() == to_np(host["inconsistent"])[:counts[2]].tobytes()
    assert got["xyz"].tobytes() == to_np(host["xyz"])[acc].tobytes()


def key_frame(ctx, rs, oracle, p, tri, second=True):
    """query, triangulate and every comparison; returns (results, expectation, the frame: the caller closes it)"""
    fr = key_frame_of(ctx, rs, tri)
    assert p.dev.query(fr)["live"] == len(p.ref.id)
    got, e = triangulate(ctx, rs, p, fr, tri), TC.expected(p.ref, tri, oracle)
    compare(p, got, e)
    if second:
        against_the_device_kernel(ctx, rs, got, e, tri)
    return got, e, fr


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("cap", TC.RAGGED_CAPS)
def test_ragged_capacities(ctx, rs, cap):
    """carry, extend and download where the last owning thread's run of rows is short (or, at cap 1 and 63, where one
    thread or one wave owns everything): every carry form, repeats at 1025"""
    p = stepped(ctx, rs, TC.ragged(cap, repeats=cap == 1025))
    fr = make_frame(ctx, rs, np.zeros((cap, 2), np.float32))
    assert p.dev.query(fr) == p.ref.query(np.full(cap, -1), np.zeros(0, bool))
    fr.close(); p.close()


# ------------------------------------------------------------------------------------------------ 2, 3
def pack_and_erase(ctx, rs, oracle, case):
    p = stepped(ctx, rs, case)
    got, e, fr = key_frame(ctx, rs, oracle, p, case["tri"])
    p.dev.erase_inconsistent()
    p.ref.erase(e["inconsistent"])
    p.check()
    assert p.dev.query(fr)["live"] == len(p.ref.id) == got["n_tracks"] - got["counts"][2]
    fr.close(); p.close()


@pytest.mark.parametrize("T,cap,bad", TC.PACK_SHAPES)
def test_pack_results_and_erase_at_the_chunk_edges(ctx, rs, oracle, T, cap, bad):
    """T on both sides of one and of two tracks per thread (n2 = 2 .. 4096), cap == T and with headroom; in the 2049
    cases more than 1024 tracks are accepted, or more than 1024 inconsistent and erased"""
    pack_and_erase(ctx, rs, oracle, TC.pack_case(T, cap, bad))


def test_full_size(ctx, rs, oracle):
    """T = cap = 8192: a 64 KB sort, eight rows and eight tracks per thread"""
    pack_and_erase(ctx, rs, oracle, TC.full_size())


# ------------------------------------------------------------------------------------------------ 4
def test_long_tracks_and_the_pose_range(ctx, rs, oracle):
    """tracks of 1, 63, 64, 65, 127 and 128 sightings and tracks that hit max_sightings; out-of-range sightings at index
    0, at index 127 only and at both ends of one track.  The copy kernel's second trip is pinned by the packed arrays:
    sight_pose and sight_uv beyond a track's 64th sighting equal ref.pack's."""
    case = TC.long_tracks()
    p = stepped(ctx, rs, case)
    got, e, fr = key_frame(ctx, rs, oracle, p, case["tri"])
    assert got["out_of_range"] == 4 and {63, 64, 65, 127, 128} <= set(got["sightings"].tolist())
    pk, want = p.dev.packed(), e["pack"]
    for t in np.flatnonzero(p.ref.count > 64):
        tail = slice(want["sight_ptr"][t] + 64, want["sight_ptr"][t + 1])
        assert pk["sight_pose"][tail].tobytes() == want["sight_pose"][tail].tobytes() and len(want["sight_pose"][tail]) == p.ref.count[t] - 64
        assert pk["sight_uv"][tail].tobytes() == want["sight_uv"][tail].tobytes() and np.all(want["sight_uv"][tail] != 0)
    assert not np.any(got["kf_pairs"][:, 0] == 13)         # the key-frame sighting of frame 129 that found no room
    fr.close(); p.close()


# ------------------------------------------------------------------------------------------------ 5
def test_more_pairs_than_the_first_read_back(ctx, rs, oracle):
    """n_pairs > 2 T: the rest comes by the second copy; capacity_pairs on both sides of every bound"""
    case = TC.many_pairs()
    p = stepped(ctx, rs, case)
    got, e, fr = key_frame(ctx, rs, oracle, p, case["tri"])
    T, n_pairs = got["n_tracks"], got["n_pairs"]
    assert n_pairs > 2 * T + 1
    for room in (n_pairs, n_pairs + 5, 2 * T, 2 * T + 1, 3, 0):
        few = triangulate(ctx, rs, p, fr, case["tri"], capacity_pairs=room)
        assert few["n_pairs"] == n_pairs and len(few["kf_pairs"]) == min(room, n_pairs)
        compare(p, few, e, room)
    fr.close(); p.close()


# ------------------------------------------------------------------------------------------------ 6
def test_ids_spread_beyond_2_to_the_19(ctx, rs, oracle):
    """(id - min id) << 13 | row beyond 32 bits: the packed order must still be the id order, the two tracks of frame 0
    first.  (2^32 ids, where next_id_low wraps, would take half a million frames: out of reach of a test.)"""
    case = TC.id_spread()
    p = stepped(ctx, rs, case)
    got, e, fr = key_frame(ctx, rs, oracle, p, case["tri"], second=False)
    q = p.dev.query(fr)
    assert q == p.ref.query(case["tri"]["table"], np.zeros(0, bool)) and q["next_id_low"] == p.ref.next_id >= 2 ** 19
    pk = p.dev.packed()
    assert pk["track_uv"][:2].tobytes() == case["tri"]["pixels"][[8000, 5]].tobytes() and pk["sight_ptr"][:3].tolist() == [0, 2, 4]
    fr.close(); p.close()


# ------------------------------------------------------------------------------------------------ 7
def test_bookkeeping_without_a_query(ctx, rs, oracle):
    case = TC.pack_case(200, 256, 0.15)
    tri = case["tri"]
    p = stepped(ctx, rs, case)
    got, e, fr = key_frame(ctx, rs, oracle, p, tri)
    T, gone = got["n_tracks"], int(got["counts"][2])
    assert gone > 0
    p.dev.erase_inconsistent()
    p.ref.erase(e["inconsistent"])
    again = triangulate(ctx, rs, p, fr, tri)               # no query in between: the host subtracted what it erased
    assert again["n_tracks"] == T - gone
    compare(p, again, TC.expected(p.ref, tri, oracle))
    assert p.dev.query(fr)["live"] == T - gone
    p.check()
    p.dev.erase_inconsistent()                             # nothing is inconsistent any more ...
    p.dev.erase_inconsistent()                             # ... and a second call has no pack to apply
    p.check()
    assert p.dev.query(fr)["live"] == T - gone
    # an empty store
    p.dev.clear()
    p.ref.clear()
    assert p.dev.query(fr)["live"] == 0
    none = triangulate(ctx, rs, p, fr, tri)
    assert none["counts"].tolist() == [0, 0, 0] and none["n_tracks"] == none["n_pairs"] == none["out_of_range"] == 0 and none["kf_ptr"].tolist() == [0]
    compare(p, none, TC.expected(p.ref, tri, oracle))
    p.dev.erase_inconsistent()
    p.check()
    # a frame with fewer keypoints than the carried indices reach: those tracks are skipped and keep living
    TC.replay(case, p)
    short = dict(tri, pixels=tri["pixels"][:120], table=tri["table"][:120])
    fs = key_frame_of(ctx, rs, short)
    assert p.dev.query(fs) == p.ref.query(short["table"], np.zeros(0, bool)) and len(p.ref.id) == T
    part, es = triangulate(ctx, rs, p, fs, short), TC.expected(p.ref, short, oracle)
    compare(p, part, es)
    assert np.all(es["pack"]["skip"][p.ref.keypoint >= 120] == 1) and part["n_tracks"] == T and part["counts"][0] > 0
    p.check()
    assert p.dev.query(fr)["live"] == T
    fs.close(); fr.close(); p.close()


# ------------------------------------------------------------------------------------------------ 8
def test_query_at_size(ctx, rs):
    """8192 keypoints and 8192 rows (eight per thread) against a map of 2000 slots: last_key_frame absent, first, in the
    middle or last in the observation lists; min_sightings 1 on a max_sightings 1 store; min_travel 0; a NaN and an
    infinite pixel, which are not below min_travel and wait"""
    q = TC.query_at_size()
    rng = np.random.default_rng(88)
    sm = SimpleMap(ctx, rs, rng.uniform(-1, 1, (q["P"], 3)).astype(np.float32), q["n_obs"], dead=q["dead"])
    for name, min_sightings in (("single", 1), ("moving", 3)):
        case = q[name]
        p = stepped(ctx, rs, case)
        fr = make_frame(ctx, rs, case["pixels"])
        set_table(ctx, fr, q["table"])
        for last_kf in (-1, 0, 3, 5):
            for min_travel in (0.0, 20.0):
                want = p.ref.query(q["table"], TC.covisible(q["n_obs"], q["dead"], last_kf), min_sightings, min_travel)
                assert p.dev.query(fr, sm.map, last_kf, min_sightings, min_travel) == want, (name, last_kf, min_travel)
        fr.close(); p.close()
    sm.close()


# ------------------------------------------------------------------------------------------------ 9
def raw_triangulate(ctx, rs, p, fr, d_poses, n_poses, kf_pose, K, capacity_tracks):
    """the C call with arguments TrackStore.triangulate always derives: the capacity of the result arrays and the pose count"""
    cap = p.dev.max_points
    i32s, f32s, pairs = [np.zeros(cap + 1, np.int32) for _ in range(5)], [np.zeros((cap, 3), np.float32) for _ in range(3)], np.zeros((4, 2), np.int32)
    r = rs.TrackResults(capacity_tracks=capacity_tracks, capacity_pairs=4, h_keypoint=i32s[0].ctypes.data, h_xyz=f32s[0].ctypes.data,
                        h_sightings=i32s[1].ctypes.data, h_kf_ptr=i32s[2].ctypes.data, h_kf_pairs=pairs.ctypes.data,
                        h_track=i32s[3].ctypes.data, h_parallax_cos=f32s[1].ctypes.data, h_required_cos=f32s[2].ctypes.data,
                        h_inconsistent=i32s[4].ctypes.data)
    return ctx.lib.rs_track_store_triangulate(ctx.h, p.dev.h, None, fr.h, None if d_poses is None else C.c_void_p(d_poses.data_ptr()), int(n_poses), 0,
                                              int(kf_pose), (C.c_float * 4)(*K), C.c_float(1.0), C.c_float(4.0), C.c_float(0.999848), C.c_float(0.20),
                                              100, None, C.byref(r))


def test_refusals_of_triangulate(ctx, rs, oracle):
    """each refusal leaves the store as it was and the next valid call correct: status 1 = RS_ERR_INVALID, 4 = RS_ERR_UNSUPPORTED"""
    case = TC.pack_case(200, 256, 0.15)
    tri = case["tri"]
    p = stepped(ctx, rs, case)
    got, e, fr = key_frame(ctx, rs, oracle, p, tri, second=False)
    T, K, n_poses, d_poses = got["n_tracks"], tri["K"], len(tri["poses"]), ctx.dev(tri["poses"])
    other = rs.Context(0)
    foreign = rs.ResidentMap(other)
    big = make_frame(ctx, rs, np.zeros((case["cap"] + 1, 2), np.float32))

    def wrapped(frame=fr, kf_pose=tri["kf_pose"], map_=None, poses=d_poses):
        return lambda: p.dev.triangulate(frame, poses, 0, kf_pose, K, map_=map_)

    refusals = [
        ("capacity_tracks < T", 1, lambda: raw_triangulate(ctx, rs, p, fr, d_poses, n_poses, tri["kf_pose"], K, T - 1)),
        ("n_poses < 1", 1, lambda: raw_triangulate(ctx, rs, p, fr, d_poses, 0, 0, K, case["cap"])),
        ("kf_pose beyond the poses", 1, wrapped(kf_pose=n_poses)),
        ("kf_pose negative", 1, wrapped(kf_pose=-1)),
        ("null poses", 1, lambda: raw_triangulate(ctx, rs, p, fr, None, n_poses, tri["kf_pose"], K, case["cap"])),
        ("a map of another context", 1, wrapped(map_=foreign)),
        ("a frame above cap", 4, wrapped(frame=big)),
    ]
    assert raw_triangulate(ctx, rs, p, fr, d_poses, n_poses, tri["kf_pose"], K, T) == 0         # the raw form itself is accepted at capacity T
    for what, status, call in refusals:
        try:
            rc = call()
        except rs.RsError as err:
            rc = int(str(err).split("status ")[1].split(":")[0])
        assert rc == status, what
        p.check()
        compare(p, triangulate(ctx, rs, p, fr, tri), e)
    big.close(); foreign.close(); other.close(); fr.close(); p.close()
