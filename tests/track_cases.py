"""Cases of the frame match table's kernels (racing-slam_amd/csrc/frame_matches.hip), shared by
tests/test_track_cases_cpu.py (every case recomputed from tests/track_ref.py, the kernel path each case exists for, and
the small ones against the object model of tests/test_track_cpu.py) and tests/test_gpu_track_envelope.py (the device
against the case).  No GPU import; every generator is seeded and cached, and its arrays are read-only.

A case is a dict: the plain arrays the stage reads, `expect` (what tests/track_ref.py gives) and `reaches`, the set of
kernel paths the case was written to reach.  tests/test_track_cases_cpu.py derives each tag again from the arrays, so a
generator that loses a path fails there, without a GPU.

Every kernel here is one 1024-thread workgroup whose thread t takes entries t, t + 1024, ... (k_fm_add, k_fm_carry) or
the ceil(n_kp / 1024) keypoints from t * per (k_fm_gather).  The sizes sit where that chunking, the hash table's size
(64 slots up to 32 entries, 16384 at 8192) and the map's device capacity (4096 slots, doubled) change."""
import functools

import numpy as np

import track_ref as R

THREADS = 1024                      # FM_THREADS
FM_MAX = 8192
I32_MAX = 2 ** 31 - 1
BAD_INDEX = (-1, "n_prev", "max_n", I32_MAX)

CARRY_TAGS = frozenset("""parallel serial gated gate_by_multiplicity refused_kp refused_point repeat_1 repeat_64 repeat_1024
kp_repeat point_repeat both_repeats fallback_full_walk mark_past_4096 mark_past_8192 slot_last n_next_lt_max_n n_next_gt_max_n
count_none count_zero count_negative count_over count_half min_at min_below min_above null_stats bad_index prev_dead prev_oob
prev_gate_fail next_dead next_oob no_inlier inlier_ascending long small""".split())
# what must be reached by a list of more than 1024 entries and by one of at most 1024 (repeat_1024 needs 1025)
CARRY_BOTH_LENGTHS = frozenset("""parallel serial gated gate_by_multiplicity refused_kp refused_point repeat_1 repeat_64 kp_repeat
point_repeat both_repeats count_zero count_negative count_over count_half min_at min_below min_above null_stats bad_index prev_dead
prev_oob prev_gate_fail next_dead next_oob no_inlier inlier_ascending""".split())
ADD_TAGS = frozenset("""chain32 wraps load_half_64 load_half_16384 one_point_many_kp one_kp_many_points point_max ap_1 ap_128
ap_65536 ap_33554432 device_count table_33 table_1025 table_8192 clears_unnamed kp_repeat point_repeat cluster_repeat""".split())
GATHER_TAGS = frozenset([f"per_{k}" for k in range(1, 9)] + """empty all_kept_8192 none_kept alternating last_run_only dead_and_oob
min_at min_above gate_refuses packed_high""".split())
MATCH_TAGS = frozenset("live dead oob four_in_word last_slot required_last required_none distance_0 distance_64 distance_256 kp_64 kp_8192".split())


def _ro(a):
    a.setflags(write=False)
    return a


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            _ro(v)
        elif isinstance(v, dict):
            _freeze(v)
        elif isinstance(v, (list, tuple)):
            for w in v:
                if isinstance(w, dict):
                    _freeze(w)
    return case


# ------------------------------------------------------------------------------------------------ carry
@functools.lru_cache(maxsize=None)
def carry_map(P):
    """What k_fm_carry reads of a map of P slots.  Slot s: s % 4 == 0 or 3 two observations, 1 one observation and
    track-consistent, 2 one observation (fails the :209 gate); s % 16 == 7 was removed (two observations before that, and
    every other one of them track-consistent: the flag survives removal).  Slot P - 1 passes the gate at every P used."""
    s = np.arange(P)
    n_obs_built = np.where((s % 4 == 0) | (s % 4 == 3), 2, 1)
    consistent = (s % 4 == 1).astype(np.uint8)
    dead = s % 16 == 7
    consistent[dead & (s % 32 == 7)] = 1
    return dict(P=P, alive=_ro((~dead).astype(np.uint8)), n_obs=_ro(np.where(dead, 0, n_obs_built)), n_obs_built=_ro(n_obs_built),
                consistent=_ro(consistent), dead=_ro(np.flatnonzero(dead)))


def _bad_values(n_prev, max_n):
    return np.array([-1, n_prev, max_n, I32_MAX], np.int64)


def _carry(name, P, n_prev, n_next, max_n, seed, reaches, inlier=None, count=None, min_points=15, stats=True, kp_repeats=(),
           point_repeats=(), prefill=False, bad=False, n_cand=None, twice=0, last_repeat=False):
    rng = np.random.default_rng([41, seed, P, n_prev, n_next, max_n])
    m = carry_map(P)
    usable = min(n_next, max_n)                        # list positions that name a keypoint of next
    passes = (m["alive"] != 0) & ((m["n_obs"] >= 2) | (m["consistent"] != 0))
    good, fail, dead = np.flatnonzero(passes), np.flatnonzero((m["alive"] != 0) & ~passes), m["dead"]
    nc = min(len(good), n_prev, usable)
    nc = nc if nc <= 2 else int(0.7 * nc)
    if n_cand:
        nc = min(nc, n_cand)
    # candidate points over the whole slot range, slot P - 1 among them
    pts = good[np.unique(np.round(np.linspace(0, len(good) - 1, nc)).astype(int))]
    nc = len(pts)
    pts = rng.permutation(pts)
    prev_table = np.full(n_prev, -1, np.int32)
    kqs = rng.permutation(n_prev)
    prev_table[kqs[:nc]] = pts
    rest = kqs[nc:]
    q = len(rest) // 4
    noise = np.concatenate([dead[:q], fail[:q], P + np.arange(min(q, 50), dtype=np.int64)])
    if len(noise) and noise[-1] >= P:
        noise[-1] = I32_MAX
    prev_table[rest[:len(noise)]] = noise
    # the kept-index list: prev's keypoints, each once; the candidates' at positions next has a keypoint for
    prev_index = np.full(max_n, -1, np.int64)
    pos_c = rng.permutation(usable)[:nc]
    if nc and 0 not in pos_c:                          # (position 0 is one: a list of 1025 has its pair 0, 1024)
        pos_c[0] = 0
    prev_index[pos_c] = kqs[:nc]
    free = rng.permutation(np.setdiff1d(np.arange(max_n), pos_c))
    others = kqs[nc:][:len(free)]
    prev_index[free[:len(others)]] = others
    touched = set()

    def pairs(d, k=3):
        """up to k candidate positions j with j + d usable and neither end used by another pair"""
        out = []
        for j in np.sort(pos_c):
            if j + d < usable and j not in touched and j + d not in touched:
                out.append(int(j))
                touched.update((int(j), int(j) + d))
                if len(out) == k:
                    break
        assert out, (name, d)
        return out

    for d in point_repeats:                            # the same previous keypoint at two positions: one point, two keypoints
        for j in pairs(d):
            prev_index[j + d] = prev_index[j]
    inl = None
    if inlier == "ascending":
        inl = np.sort(rng.choice(usable, max(1, int(0.8 * usable)), replace=False)).astype(np.int64)
    elif inlier == "identity" or kp_repeats or last_repeat or bad:
        inl = np.arange(max_n, dtype=np.int64)
    for d in kp_repeats:                               # one position twice: the keypoint and the point repeat
        for j in pairs(d):
            inl[j + d] = inl[j]
    if twice:                                          # `twice` distinct candidates, the whole run listed two times
        first = np.sort(pos_c)[:twice]
        inl = np.concatenate([first, first])
    if last_repeat:
        assert max_n == FM_MAX and count is None
        inl[max_n - 1] = np.sort(pos_c)[0]
    if bad:
        spots = rng.permutation(np.setdiff1d(np.arange(usable), np.concatenate([pos_c, pos_c + 1])))[:8]
        prev_index[spots[:4]] = _bad_values(n_prev, max_n)
        inl[spots[4:]] = _bad_values(n_prev, max_n)
    if inl is not None and count is None and len(inl) < max_n:
        count = len(inl)
    if inl is not None:
        inl = np.concatenate([inl, np.zeros(max(0, max_n - len(inl)), np.int64)])
    next_table = np.full(n_next, -1, np.int32)
    if prefill:
        c = np.sort(pos_c)[::-1]                       # (the repeats above sit at the other end of the list)
        taken_by = [fail[0], dead[0], P + 3]           # a live point, a dead slot, a slot past the map: all "matched"
        for j, p in zip(c[:3], taken_by):
            next_table[j] = p
        elsewhere = np.setdiff1d(np.arange(n_next), pos_c)[-5:]
        for k, j in zip(elsewhere[:3], c[3:6]):        # these candidates' points are matched at another keypoint
            next_table[k] = prev_table[prev_index[j]]
        next_table[elsewhere[3]], next_table[elsewhere[4]] = dead[1], I32_MAX
        live = next_table[next_table >= 0]
        assert len(np.unique(live)) == len(live)
    args = (m["alive"], m["n_obs"], m["consistent"], prev_table)
    n_c = len(R.carry_candidates(*args, n_next, prev_index, inl, count, max_n))
    if isinstance(min_points, tuple):
        min_points = n_c + min_points[1]
    table, cands, accepted = R.carry(*args, next_table, prev_index, inl, count, max_n, min_points)
    n = max_n if count is not None and count <= 0 else R.clamp_count(count, max_n)     # (a count of nothing: by the list it cuts)
    return _freeze(dict(name=name, P=P, n_prev=n_prev, n_next=n_next, max_n=max_n, prev_table=prev_table, next_table=next_table,
                        prev_index=prev_index.astype(np.int32), inlier=None if inl is None else inl.astype(np.int32), count=count,
                        min_points=int(min_points), stats=stats, expect=dict(table=table, candidates=cands, accepted=accepted),
                        reaches=frozenset(reaches) | {"long" if n > THREADS else "small"}))


SMALL = (61, 64, 1023, 1024)            # P, n_prev, n_next, max_n: n_next < max_n
SMALL_1025 = (61, 64, 1025, 1025)       # the shortest list with entries i and i + 1024
MID = (4097, 1025, 8192, 2049)          # n_next > max_n; marks past the map's first device capacity
MID_WIDE = (4097, 1023, 1025, 8192)     # a full-length list of which next has keypoints for 1025 positions
LONG = (9001, 8192, 8192, 8192)         # marks past 8192


@functools.lru_cache(maxsize=None)
def carry_cases():
    c, seed = [], iter(range(1000))

    def add(name, cfg, reaches, **kw):
        c.append(_carry(name, *cfg, next(seed), reaches.split(), **kw))

    add("tiny", (1, 1, 1, 1), "parallel slot_last", min_points=1)
    add("tiny_gated", (1, 1, 1, 1), "gated", min_points=15)
    add("one_point_map", (1, 64, 1, 1025), "parallel n_next_lt_max_n", min_points=1)
    add("one_entry_list", (9001, 1, 8192, 1), "parallel n_next_gt_max_n", min_points=1)
    add("narrow_next", (61, 1023, 64, 1024), "parallel n_next_lt_max_n no_inlier")
    add("wide_list", MID_WIDE, "parallel n_next_lt_max_n no_inlier")
    for tag, cfg in (("small", SMALL), ("mid", MID), ("long", LONG)):
        past = {"small": "", "mid": " mark_past_4096", "long": " mark_past_4096 mark_past_8192"}[tag]
        add(f"plain_{tag}", cfg, "parallel no_inlier count_none slot_last prev_dead prev_oob prev_gate_fail" + past)
        add(f"ascending_{tag}", cfg, "parallel inlier_ascending", inlier="ascending")
    for tag, cfg, ds in (("small", SMALL, (1, 64)), ("long", LONG, (1, 64, 1024))):
        for d in ds:
            add(f"kp_repeat_{d}_{tag}", cfg, f"serial kp_repeat repeat_{d}", kp_repeats=(d,))
            add(f"point_repeat_{d}_{tag}", cfg, f"serial point_repeat repeat_{d}", point_repeats=(d,))
        add(f"both_repeats_{tag}", cfg, "serial both_repeats kp_repeat point_repeat", kp_repeats=ds, point_repeats=ds)
    add("kp_repeat_1024_1025", SMALL_1025, "serial kp_repeat repeat_1024", kp_repeats=(1024,))
    add("point_repeat_1024_1025", SMALL_1025, "serial point_repeat repeat_1024", point_repeats=(1024,))
    add("repeats_mid", MID, "serial both_repeats repeat_1 repeat_64 repeat_1024 mark_past_4096", kp_repeats=(1, 1024), point_repeats=(64, 1024))
    add("last_entry_repeats", LONG, "serial fallback_full_walk kp_repeat", last_repeat=True)
    for tag, cfg in (("small", SMALL), ("long", LONG)):
        add(f"prefilled_{tag}", cfg, "parallel refused_kp refused_point next_dead next_oob", prefill=True)
        add(f"bad_index_{tag}", cfg, "bad_index", bad=True)
        for what, count in (("zero", 0), ("negative", -5), ("over", cfg[3] + 9), ("half", cfg[3] // 2)):
            add(f"count_{what}_{tag}", cfg, f"count_{what}", count=count, inlier="identity" if what == "half" else None, min_points=1)
        for what, rel in (("at", 0), ("below", -1), ("above", 1)):
            add(f"min_{what}_{tag}", cfg, f"min_{what} " + ("gated" if rel > 0 else "parallel"), min_points=("candidates", rel))
    add("prefilled_repeats_small", SMALL, "serial refused_kp refused_point", prefill=True, kp_repeats=(1,), point_repeats=(64,))
    add("prefilled_repeats_mid", MID, "serial refused_kp refused_point", prefill=True, kp_repeats=(1024,), point_repeats=(1,))
    add("eight_twice", SMALL, "serial gate_by_multiplicity kp_repeat", twice=8, min_points=15)
    add("six_hundred_twice", MID, "serial gate_by_multiplicity kp_repeat", twice=600, min_points=1199)
    add("null_stats_small", SMALL, "null_stats serial", stats=False, kp_repeats=(1,))
    add("null_stats_long", LONG, "null_stats parallel", stats=False)
    assert len({k["name"] for k in c}) == len(c)
    return tuple(c)


@functools.lru_cache(maxsize=None)
def carry_probe(P):
    """A small list without repeats on the map of P slots: what must still come out right after any other case."""
    n = min(64, max(P, 1))
    return _carry(f"probe_{P}", P, n, n, n, 999, ["parallel"], min_points=1)


# ------------------------------------------------------------------------------------------------ add
def fm_hash(p):
    """fm_hash of frame_matches.hip in uint32 arithmetic: (uint32) p * 2654435761 >> 7"""
    return ((np.asarray(p, np.int64).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(7)


def add_hmask(max_n):
    slots = 64
    while slots < 2 * max_n:
        slots *= 2
    return slots - 1


def probe_slots(hmask, points):
    """The slots a sequential insertion of the distinct `points`, in this order, visits: one list of slots per point,
    the last one being where it rests."""
    used, out = {}, []
    for p in points:
        h, walk = int(fm_hash(p)) & hmask, []
        while True:
            walk.append(h)
            if h not in used or used[h] == p:
                used[h] = p
                break
            h = (h + 1) & hmask
        out.append(walk)
    return out


@functools.lru_cache(maxsize=None)
def hash_cluster(hmask, first_slot, need):
    """The `need` smallest points whose home slot is first_slot .. hmask."""
    p = np.arange(1, 1 << 22, dtype=np.int64)
    hit = p[(fm_hash(p) & np.uint64(hmask)) >= np.uint64(first_slot)][:need]
    assert len(hit) == need
    return _ro(hit)


def progression(stride, n, base=3):
    """n distinct non-negative int32 points base + i * stride; past 2^31 the progression starts again one higher."""
    i = np.arange(n, dtype=np.int64)
    return (base + i * stride) % 2 ** 31 + (base + i * stride) // 2 ** 31


def _add(name, n_kp, lists, seed, reaches):
    rng = np.random.default_rng([43, seed, n_kp])
    named = np.unique(np.concatenate([np.asarray(pt, np.int64)[np.asarray(pt) >= 0] for _, pt, _, _ in lists]))
    # a table that is not empty: half of its points are points the lists will name, half are not
    k = max(1, n_kp // 2)
    a = rng.permutation(named)[:k // 2]
    b = np.setdiff1d(rng.integers(0, I32_MAX, k - len(a) + 8), named)[:k - len(a)]
    start = np.full(n_kp, -1, np.int32)
    pts = rng.permutation(np.concatenate([a, b]))
    start[rng.permutation(n_kp)[:len(pts)]] = pts
    out, table = [], start
    for kp, pt, count, max_n in lists:
        kp, pt = np.asarray(kp, np.int32), np.asarray(pt, np.int32)
        assert len(kp) == len(pt) == max_n <= FM_MAX
        table = R.matches_add(table, kp, pt, count, max_n)
        out.append(dict(kp=kp, point=pt, count=count, max_n=max_n, expect=table))
    return _freeze(dict(name=name, n_kp=n_kp, start=start, lists=out, reaches=frozenset(reaches.split()) | {f"table_{n_kp}"}))


def _interleave(rng, *parts):
    return rng.permutation(np.concatenate([np.asarray(p, np.int64) for p in parts]))


@functools.lru_cache(maxsize=None)
def add_cases():
    c = []
    rng = np.random.default_rng(47)
    for max_n, sizes in ((32, (33, 33, 33, 33)), (FM_MAX, (FM_MAX, 1025, FM_MAX, 1025))):
        for stride, n_kp in zip((1, 128, 2 ** 16, 2 ** 25), sizes):
            pt = progression(stride, max_n)
            kp = rng.permutation(n_kp)[:max_n] if n_kp >= max_n else rng.integers(0, n_kp, max_n)
            again = (rng.permutation(n_kp)[:max_n] if n_kp >= max_n else rng.integers(0, n_kp, max_n), pt[::-1].copy(), max_n // 2, max_n)
            c.append(_add(f"progression_{stride}_x{max_n}", n_kp, [(kp, pt, None, max_n), again], len(c),
                          f"ap_{stride} device_count load_half_{64 if max_n == 32 else 16384}" + (" kp_repeat" if n_kp < max_n else "")))
    c.append(_add("one_point_everywhere", FM_MAX, [(rng.permutation(FM_MAX), np.full(FM_MAX, 77), None, FM_MAX)], len(c),
                  "one_point_many_kp point_repeat"))
    many = np.concatenate([rng.choice(I32_MAX, FM_MAX - 1, replace=False), [I32_MAX]])
    for n_kp in (1025, FM_MAX):
        c.append(_add(f"one_keypoint_{n_kp}", n_kp, [(np.full(FM_MAX, 5), rng.permutation(many), None, FM_MAX)], len(c),
                      "one_kp_many_points kp_repeat point_max clears_unnamed"))
    # 32 points whose home is one slot of the 64: a probe chain of 32, then half of them among others and their own repeats
    home = int(np.bincount((fm_hash(np.arange(1, 4096)) & np.uint64(63)).astype(int)).argmax())
    one_slot = np.array([p for p in range(1, 8192) if int(fm_hash(p)) & 63 == home][:32])
    assert len(one_slot) == 32
    mixed = _interleave(rng, one_slot[:16], one_slot[:8], rng.integers(0, I32_MAX, 8))
    c.append(_add("one_slot_of_64", 33, [(rng.permutation(33)[:32], rng.permutation(one_slot), None, 32),
                                         (rng.integers(0, 33, 32), mixed, None, 32), (rng.permutation(33)[:32], mixed[::-1].copy(), 20, 32)], len(c),
                  "chain32 load_half_64 cluster_repeat kp_repeat point_repeat device_count"))
    # 240 points whose home is one of the last four slots of the 16384: the chain runs on through slot 0
    tail = hash_cluster(16383, 16380, 240)
    for n_kp in (FM_MAX, 1025):
        pt = _interleave(rng, tail, tail[::2], rng.integers(0, I32_MAX, FM_MAX - 360))
        kp = rng.permutation(n_kp)[:FM_MAX] if n_kp >= FM_MAX else rng.integers(0, n_kp, FM_MAX)
        c.append(_add(f"last_slots_of_16384_{n_kp}", n_kp, [(kp, pt, None, FM_MAX), (kp[::-1].copy(), pt, FM_MAX // 2, FM_MAX)], len(c),
                      "wraps cluster_repeat point_repeat device_count"))
    assert len({k["name"] for k in c}) == len(c)
    return tuple(c)


# ------------------------------------------------------------------------------------------------ gather
GATHER_TWO, GATHER_ONE, GATHER_DEAD = 8192, 8192, 1700     # slots with two observations, then with one, then removed ones
# per = ceil(n_kp / 1024):  1  1     2     3     3     4     5     5     6     7     7     8     8
GATHER_SIZES = (1, 1024, 1025, 2049, 3000, 3073, 4097, 5000, 5121, 6145, 7000, 7169, 8192)


@functools.lru_cache(maxsize=None)
def gather_map():
    P = GATHER_TWO + GATHER_ONE + GATHER_DEAD
    s = np.arange(P)
    return dict(P=P, alive=_ro((s < GATHER_TWO + GATHER_ONE).astype(np.uint8)),
                n_obs=_ro(np.where(s < GATHER_TWO, 2, np.where(s < GATHER_TWO + GATHER_ONE, 1, 0))))


def gather_slots(n_kp):
    """keypoint k's point with two observations; its one-observation point is GATHER_TWO higher"""
    return np.random.default_rng([53, n_kp]).permutation(GATHER_TWO)[:n_kp]


@functools.lru_cache(maxsize=None)
def gather_geometry(synth):
    """One well-posed pose problem of 8192 points (refine_cases.problem) behind every gather case: the positions of the
    map's slots and, with a rotation prior and an inertial delta, what kinds 1 and 2 need."""
    import refine_cases
    p = refine_cases.problem(synth, dict(scene=dict(refine_cases.DEFAULT_SCENE, n=GATHER_TWO, seed=77, imu=True), opt={}, prior=(1e-3, 0.01),
                                         delta=True))
    m = gather_map()
    rng = np.random.default_rng(59)
    pos = np.concatenate([p["points"].astype(np.float32), rng.normal(0, 5, (m["P"] - GATHER_TWO, 3)).astype(np.float32)])
    return dict(problem=p, positions=_ro(pos))


def gather_keypoints(geom, n_kp):
    """keypoint k sees its two-observation point where the problem observes it"""
    return geom["problem"]["uv"][gather_slots(n_kp)].astype(np.float32)


def _gather(name, n_kp, table, min_matches, reaches):
    m = gather_map()
    table = np.asarray(table, np.int32)
    live = table[table >= 0]
    assert len(np.unique(live)) == len(live)
    keep = [k for k in range(n_kp) if 0 <= table[k] < m["P"] and m["alive"][table[k]] and m["n_obs"][table[k]] >= 2]
    matched = R.num_matches(table)
    _, _, n_used = R.gather(table, np.zeros((n_kp, 2), np.float32), m["alive"], m["n_obs"], np.zeros((m["P"], 3), np.float32), min_matches)
    assert n_used == (-1 if matched < min_matches else len(keep))
    per = (n_kp + THREADS - 1) // THREADS
    return _freeze(dict(name=f"{name}_{n_kp}", n_kp=n_kp, table=table, min_matches=min_matches,
                        expect=dict(n_used=n_used, kept=np.array(keep, np.int32), matched=matched),
                        reaches=frozenset(reaches.split()) | {f"per_{per}"}))


@functools.lru_cache(maxsize=None)
def gather_cases():
    c, P = [], gather_map()["P"]
    for n_kp in GATHER_SIZES:
        two = gather_slots(n_kp).astype(np.int64)
        one = two + GATHER_TWO
        k = np.arange(n_kp)
        per = (n_kp + THREADS - 1) // THREADS
        c.append(_gather("empty", n_kp, np.full(n_kp, -1), 15, "empty gate_refuses"))
        c.append(_gather("empty_no_minimum", n_kp, np.full(n_kp, -1), 0, "empty none_kept"))
        c.append(_gather("all_kept", n_kp, two, 15 if n_kp >= 15 else 1, "all_kept_8192 packed_high" if n_kp == FM_MAX else ""))
        c.append(_gather("one_observation", n_kp, one, n_kp, "none_kept min_at" + (" packed_high" if n_kp == FM_MAX else "")))
        c.append(_gather("alternating", n_kp, np.where(k % 2 == 0, two, one), 1, "alternating"))
        last = (n_kp - 1) // per * per                 # the first keypoint of the last thread that has any
        c.append(_gather("last_run", n_kp, np.where(k >= last, two, one), n_kp, "last_run_only min_at"))
        mixed = np.select([k % 5 == 0, k % 5 == 1, k % 5 == 2, k % 5 == 3], [two, one, GATHER_TWO + GATHER_ONE + k // 5, P + k], -1)
        if n_kp > 3:
            mixed[3] = I32_MAX
        n = int(np.count_nonzero(mixed >= 0))
        c.append(_gather("dead_and_past_at", n_kp, mixed, n, "min_at" + (" dead_and_oob" if n_kp > 3 else "")))
        c.append(_gather("dead_and_past_above", n_kp, mixed, n + 1, "min_above gate_refuses" + (" dead_and_oob" if n_kp > 3 else "")))
    return tuple(c)


# ------------------------------------------------------------------------------------------------ match
MATCH_SCENE = dict(n_kf=6, n_points=302, seed=4)      # a test_resident_map.Scene; 302 slots: the last flag word is half used
MATCH_DEAD = 17                                       # the slot the test removes from the scene before anything else
MATCH_WORD = 10                                       # slots 40 .. 43 share flag word 10


@functools.lru_cache(maxsize=None)
def match_cases():
    """The start table as index lists (keypoints all below 64) on the scene above.  There is no expectation here: the
    yardstick is rs_map_match fed the table's host lists, then track_ref.match_fold.  `requires` states what the scene
    must offer; the GPU test asserts it."""
    P = MATCH_SCENE["n_points"]
    pts = [P - 1, 4 * MATCH_WORD, 4 * MATCH_WORD + 1, 4 * MATCH_WORD + 2, 4 * MATCH_WORD + 3, MATCH_DEAD, P + 5, I32_MAX] + list(range(60, 260, 10))
    kps = [63, 0, 1, 2, 3, 9, 11, 13] + list(range(20, 60, 2))
    assert len(pts) == len(kps) == len(set(pts)) == len(set(kps))
    c = []
    for n_kp in (64, FM_MAX):
        for dist in (0, 64, 256):
            for required in ("none", "last"):
                c.append(_freeze(dict(name=f"kp{n_kp}_d{dist}_{required}", n_kp=n_kp, start_kp=np.array(kps, np.int32), start_point=np.array(pts, np.int32),
                                      required_observer=-1 if required == "none" else MATCH_SCENE["n_kf"] - 1, max_distance=dist,
                                      requires=dict(P=P, dead=MATCH_DEAD, n_kf=MATCH_SCENE["n_kf"]),
                                      reaches=frozenset(["live", "dead", "oob", "four_in_word", "last_slot", f"required_{required}",
                                                         f"distance_{dist}", f"kp_{n_kp}"]))))
    return tuple(c)


def start_table(case):
    t = np.full(case["n_kp"], -1, np.int32)
    t[case["start_kp"]] = case["start_point"]
    return t
