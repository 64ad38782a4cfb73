"""Float descriptor sets and scenes for the L2 matcher tests (tests/test_match_l2_cpu.py, tests/test_gpu_match_l2.py).
Every builder is a pure function of its arguments.  All values are zero or at least 2^-40 in magnitude, so that no product
and no squared difference is subnormal."""
import numpy as np

import match_cases as MC

F = np.float32
TINY = 2.0 ** -40


def _clean(x):
    x = np.ascontiguousarray(x, F)
    x[np.abs(x) < TINY] = 0
    return x


def unit_rows(rng, n, dim):
    x = rng.normal(0, 1, (n, dim))
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    return _clean(x)


def raw_rows(rng, n, dim):
    return _clean(rng.uniform(-4.0, 4.0, (n, dim)))


def knn_set(nq, nt, dim, batch=1, seed=0, kind="unit", near=0.5, exact=0.1):
    """batch x (queries [nq][dim], train [nt][dim]): a fraction `near` of the queries are a train row plus noise, a
    fraction `exact` of those ARE a train row (distance 0: the clamp), the rest unrelated."""
    rng = np.random.default_rng(0x4C32 + 131 * seed + 7 * nq + 3 * nt + 1009 * dim + batch)
    make = unit_rows if kind == "unit" else raw_rows
    t = make(rng, batch * nt, dim).reshape(batch, nt, dim)
    q = make(rng, batch * nq, dim).reshape(batch, nq, dim)
    scale = 0.05 if kind == "unit" else 0.3
    for b in range(batch):
        k = np.flatnonzero(rng.random(nq) < near)
        src = rng.integers(0, nt, len(k))
        noise = rng.normal(0, scale / np.sqrt(dim), (len(k), dim))
        noise[rng.random(len(k)) < exact] = 0
        noise[:1] = 0                                    # at least one wherever a query is near at all
        q[b, k] = _clean(t[b, src] + noise)
    return q, t


def integer_set(nq, nt, dim, batch=1, seed=0):
    """Exact data for the fragment maps: independent random integers in -3 .. 3, every row different, queries unrelated to the
    train rows (an asymmetric pair of operands).  Every product, partial sum, norm and d2 is an integer below 2^24, so float32
    computes them exactly in ANY order: a wrong index or distance on such data is a layout or masking fault, never rounding.
    -> q [batch][nq][dim], t [batch][nt][dim] float32 and the exact d2 [batch][nq][nt] int64."""
    assert 4 * 36 * dim < 1 << 24
    rng = np.random.default_rng(0x1D7 + 17 * seed + 3 * nq + 5 * nt + 7 * dim)
    q = rng.integers(-3, 4, (batch, nq, dim))
    t = rng.integers(-3, 4, (batch, nt, dim))
    d2 = np.stack([(q[b] ** 2).sum(1)[:, None] + (t[b] ** 2).sum(1)[None, :] - 2 * (q[b] @ t[b].T) for b in range(batch)])   # int64
    return q.astype(F), t.astype(F), d2.astype(np.int64)


def integer_knn2(d2):
    """idx0, dist0, idx1, dist1 from one item's exact d2 [nq][nt]: ordered by (d2, train index), dist = sqrt rounded to float32."""
    nq, nt = d2.shape
    key = d2 * (1 << 32) + np.arange(nt, dtype=np.int64)[None, :]
    order = np.argsort(key, axis=1, kind="stable")
    rows = np.arange(nq)
    i0 = order[:, 0].astype(np.int32)
    d0 = np.sqrt(d2[rows, i0].astype(F))
    if nt < 2:
        return i0, d0, np.full(nq, -1, np.int32), np.full(nq, -1, F)
    i1 = order[:, 1].astype(np.int32)
    return i0, d0, i1, np.sqrt(d2[rows, i1].astype(F))


def float_rows(desc_u8, dim, seed=None, noise=0.02):
    """Float rows from 256-bit rows: bit k -> +-c with c the power of two nearest 1 / sqrt(dim) (bits repeat past 256), so
    that equal bit rows give equal float rows and, without noise, every squared distance is 4 c^2 x (a Hamming distance),
    exact in float32: ties abound.  seed: add N(0, noise) to every value."""
    d = np.ascontiguousarray(desc_u8, np.uint8).reshape(-1, 32)
    bits = np.unpackbits(d, axis=1)
    bits = np.tile(bits, (1, -(-dim // 256)))[:, :dim]
    c = 2.0 ** np.round(-0.5 * np.log2(dim))
    x = (2.0 * bits - 1.0) * c
    if seed is not None:
        x = x + np.random.default_rng(0xF10A + seed).normal(0, noise, x.shape)
    return _clean(x)


def attach(frame, mp, dim, seed=None):
    """(frame rows [N][dim], pool rows [rows][dim]) for a scene of match_cases."""
    return float_rows(frame["descriptors"], dim, seed), float_rows(mp["desc_pool"], dim, None if seed is None else seed + 1)


def select_points(mp, idx):
    """mp made of points `idx` of mp, in that order (a point may be listed more than once)."""
    idx = np.asarray(idx, np.int64)
    ptr = np.asarray(mp["obs_ptr"], np.int64)
    okf, od, new_ptr = [], [], [0]
    for i in idx:
        okf += list(mp["obs_kf"][ptr[i]:ptr[i + 1]])
        od += list(mp["obs_desc"][ptr[i]:ptr[i + 1]])
        new_ptr.append(len(okf))
    out = dict(mp)
    out.update(positions=np.asarray(mp["positions"])[idx], eligible=np.asarray(mp["eligible"])[idx], obs_ptr=np.asarray(new_ptr, np.int32),
               obs_kf=np.asarray(okf if okf else [0], np.int32), obs_desc=np.asarray(od if od else [0], np.int32))
    return out


def duplicate_points(mp, idx):
    """mp with copies of points `idx` appended (same position, eligibility and observations): each copy is exactly as far
    from every keypoint as its original, so the original (lower map index) must keep the keypoint."""
    return select_points(mp, np.concatenate([np.arange(len(mp["positions"])), np.asarray(idx, np.int64)]))


# name -> (builder, kwargs, dim, noise seed or None, [(replace, max_distance), ...])
_R01 = [(0, 1.0), (1, 1.0)]
_OBS = (1, 2, 3, 4, 5, 6, 7, 8, 9)
REPROJ = {}
for _p in (1, 63, 64, 65, 200):
    REPROJ[f"P{_p}-N300-d128"] = (MC.scene, dict(N=300, P=_p, obs=_OBS, W=640, H=480, seed=200 + _p), 128, _p, _R01)
for _n in (1, 50):
    REPROJ[f"P200-N{_n}-d128"] = (MC.scene, dict(N=_n, P=200, obs=_OBS, W=640, H=480, seed=300 + _n), 128, _n, _R01)
for _d in (4, 256):
    REPROJ[f"P200-N300-d{_d}"] = (MC.scene, dict(N=300, P=200, obs=_OBS, W=640, H=480, seed=400 + _d), _d, _d, _R01)
REPROJ["P200-N300-d128-ties"] = (MC.scene, dict(N=300, P=200, obs=_OBS, W=640, H=480, seed=77, dup=12, integer=True), 128, None, _R01)
REPROJ["elig-none"] = (MC.scene, dict(N=300, P=65, obs=(3,), W=640, H=480, seed=78, eligible="none"), 128, 1, _R01)
REPROJ["matched-all"] = (MC.scene, dict(N=300, P=65, obs=(3,), W=640, H=480, seed=79, matched="all"), 128, 1, _R01)
# discs holding more than sixteen candidates (the queue is flushed and refilled), equal rows inside a disc
_DISCS = (0, 1, 15, 16, 17, 33, 60)
REPROJ["discs-d128"] = (MC.disc_scene, dict(counts=_DISCS * 6, obs=(1, 8, 9), seed=5), 128, None, _R01)
REPROJ["discs-d4-matched"] = (MC.disc_scene, dict(counts=_DISCS * 6, obs=(2, 5), seed=6, matched="mixed"), 4, None, _R01)
REPROJ["discs-d256-noise"] = (MC.disc_scene, dict(counts=_DISCS * 3, obs=(1, 9), seed=7), 256, 9, _R01)
REPROJ["edges-d128"] = (MC.edge_scene, dict(), 128, None, [(0, 1.0), (1, 1.0), (0, 0.25)])
REPROJ["maxdist"] = (MC.scene, dict(N=300, P=200, obs=_OBS, W=640, H=480, seed=91, flip=(0, 120)), 128, 3,
                     [(0, 0.0), (1, 0.0), (0, -1.0), (0, 0.5), (1, 1e30), (0, 1e30)])


def reproj_case(name, kdtree_build):
    builder, kw, dim, seed, runs = REPROJ[name]
    frame, mp = builder(kdtree_build=kdtree_build, **kw)
    fdesc, pool = attach(frame, mp, dim, seed)
    return frame, mp, fdesc, pool, dim, runs
