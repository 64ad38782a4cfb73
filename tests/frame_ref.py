"""numpy restatement of the DEVICE algorithm of rs_frame_assign_device (racing-slam_amd/csrc/frame.hip), step for step,
so that the algorithm is checked against rs_kdtree_build on the CPU before a GPU sees it.

rs_kdtree_build (csrc/host.cpp) orders keypoints by the total order (coordinate, keypoint index) and makes the node of a
segment [s, e) at depth d the element of rank mid = (s + e) / 2 of that segment under axis d % 2; node id = mid.  So root,
left[] and right[] depend on n alone (closed_form) and only node_kp[] depends on the data.

The device form:
  ordered_key   f32 bits -> u32 whose unsigned order is the float order: -0 canonicalised to +0 (they compare equal and
                are then ordered by index), negative values bit-inverted, the others get the top bit;
  ranks         rank_x[i] = #{j : (key_x[j], j) < (key_x[i], i)}, likewise y: two permutations of 0 .. n-1
                (k_frame_rank: one thread per i, the j range cut into chunks that are summed with integer atomics);
  build         integer only.  Per position p two lists: `cur`, sorted by the level's axis inside every segment, and
                `oth`, sorted by the other axis.  Per level every segment takes cur[mid] as its node, then its part of
                `oth` is stably partitioned by rank_cur < rank_cur(node) (one prefix sum over all positions, segment counts
                by difference); the halves of `cur` are already sorted and become the children's `oth`.
"""
import numpy as np


def ordered_key(v):
    """u32 keys of f32 values: key(a) < key(b) <=> a < b and key(a) == key(b) <=> a == b for every non-NaN a, b."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32).copy()
    b[(b << np.uint32(1)) == 0] = 0                       # -0.0 -> +0.0
    neg = (b & np.uint32(0x80000000)) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def ranks(kp):
    """(rank_x, rank_y) int32 [n]: position of keypoint i under (ordered_key(coordinate), i)."""
    kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 2)
    n = len(kp)
    out = []
    for axis in range(2):
        key = (ordered_key(kp[:, axis]).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        r = np.empty(n, np.int32)
        r[np.argsort(key, kind="stable")] = np.arange(n, dtype=np.int32)
        out.append(r)
    return out[0], out[1]


def closed_form(n):
    """(left, right, root) of rs_kdtree_build for n keypoints: they do not depend on the data."""
    left, right = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    work = [(0, n)] if n > 0 else []
    while work:
        s, e = work.pop()
        m = (s + e) // 2
        if s < m:
            left[m] = (s + m) // 2
            work.append((s, m))
        if m + 1 < e:
            right[m] = (m + 1 + e) // 2
            work.append((m + 1, e))
    return left, right, (n // 2 if n > 0 else -1)


def levels(n):
    """Levels of the tree = levels the device loop runs: floor(log2 n) + 1."""
    return int(n).bit_length()


def build(kp):
    """(node_kp, left, right, root) by the device algorithm, vectorised over positions like the kernel's threads."""
    kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 2)
    n = len(kp)
    left, right, root = closed_form(n)
    node_kp = np.zeros(n, np.int32)
    if n == 0:
        return node_kp, left, right, root
    rank = ranks(kp)
    cur, oth = np.empty(n, np.int32), np.empty(n, np.int32)
    cur[rank[0]] = np.arange(n, dtype=np.int32)            # sorted by x
    oth[rank[1]] = np.arange(n, dtype=np.int32)            # sorted by y
    s, e = np.zeros(n, np.int64), np.full(n, n, np.int64)  # segment of every position; done = already a node
    done = np.zeros(n, bool)
    p = np.arange(n, dtype=np.int64)
    for depth in range(levels(n)):
        rk = rank[depth % 2]
        act = ~done
        m = (s + e) // 2
        pivot = cur[np.where(act, m, 0)]
        v = oth
        is_piv = act & (v == pivot)
        less = act & (rk[v] < rk[pivot])
        packed = less.astype(np.int64) + (is_piv.astype(np.int64) << 16)
        F = np.concatenate([[0], np.cumsum(packed)[:-1]])  # exclusive prefix over ALL positions
        d = F - F[np.where(act, s, 0)]
        lb, pb = d & 0xFFFF, d >> 16
        dest = np.where(is_piv, m, np.where(less, s + lb, m + 1 + (p - s - lb - pb)))
        new = np.empty(n, np.int32)
        new[:] = -1
        new[dest[act]] = v[act]
        fin = act & (p == m)
        node_kp[fin] = cur[fin]
        s = np.where(act & (p > m), m + 1, s)
        e = np.where(act & (p < m), m, e)
        done |= fin
        cur, oth = new, cur
    assert done.all()
    return node_kp, left, right, root


def pack(kp, node_kp, left, right):
    """rs_kdtree_pack's layout: {x, y, left, right}[n] then keypoint[n], 20 n bytes."""
    kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 2)
    n = len(node_kp)
    out = np.zeros(5 * n, np.int32)
    q = out[:4 * n].reshape(n, 4)
    q[:, :2] = kp[node_kp].view(np.int32)
    q[:, 2], q[:, 3] = left, right
    out[4 * n:] = node_kp
    return out.view(np.uint8)


def gather_counts(count_a, count_b, cap):
    """rs_describe_features' clamp: n_a = clamp(count_a, 0, cap), n_b = clamp(count_b, 0, cap - n_a); None = no list."""
    na = 0 if count_a is None else min(max(int(count_a), 0), cap)
    nb = 0 if count_b is None else min(max(int(count_b), 0), cap - na)
    return na, nb


# coordinate families of the tests (CPU and GPU)
FAMILIES = ["uniform", "grid", "identical", "same_x", "same_y", "zeros", "wide", "subnormal", "inf"]


def keypoints(family, n, seed=0):
    """[n][2] f32 of one coordinate family: a 1920x1080 image, an integer grid (many equal x and equal y), one point, one
    column, one row, a mix of -0.0 and +0.0, negative and > 1e6 magnitudes, subnormals, N(0, 1e6), +-inf / +-FLT_MAX."""
    rng = np.random.default_rng(1000 * seed + n)
    if family == "uniform":
        kp = rng.uniform(0, 1, (n, 2)) * [1920, 1080]
    elif family == "grid":
        kp = np.stack([rng.integers(0, 12, n), rng.integers(0, 9, n)], 1)
    elif family == "identical":
        kp = np.full((n, 2), 17.25)
    elif family == "same_x":
        kp = np.stack([np.full(n, 960.0), rng.uniform(0, 1080, n)], 1)
    elif family == "same_y":
        kp = np.stack([rng.uniform(0, 1920, n), np.full(n, 540.5)], 1)
    elif family == "zeros":
        kp = np.where(rng.random((n, 2)) < 0.5, -0.0, 0.0)
    elif family == "wide":
        kp = rng.uniform(-1, 1, (n, 2)) * 10.0 ** rng.integers(0, 9, (n, 2))
    elif family == "subnormal":
        kp = (rng.integers(-40, 40, (n, 2)).astype(np.float64)) * 1.401298464324817e-45
    elif family == "normal1e6":
        kp = rng.normal(0, 1e6, (n, 2))
    elif family == "inf":
        kp = rng.choice(np.array([-np.inf, np.inf, 0.0, -0.0, 1.0, -1.0, 3.4028234663852886e38, -3.4028234663852886e38]), (n, 2))
    else:
        raise ValueError(family)
    return np.ascontiguousarray(kp, np.float32).reshape(n, 2)
