"""The device algorithm of rs_frame_assign_device, restated in numpy (frame_ref.py), against rs_kdtree_build — a host
function of librsgpu.so that needs no GPU.  Every comparison is equality; there is no tolerance in this feature."""
import numpy as np
import pytest

import frame_ref

SIZES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 255, 256, 257, 1000, 2001]
FAMILIES = frame_ref.FAMILIES + ["normal1e6"]
keypoints = frame_ref.keypoints


@pytest.mark.parametrize("family", FAMILIES)
def test_build_equals_rs_kdtree_build(rs, family):
    for n in SIZES:
        kp = keypoints(family, n)
        node_kp, left, right, root = rs.kdtree_build(kp)
        g_kp, g_left, g_right, g_root = frame_ref.build(kp)
        assert root == g_root, (family, n)
        assert np.array_equal(node_kp, g_kp), (family, n)
        assert np.array_equal(left, g_left) and np.array_equal(right, g_right), (family, n)
        c_left, c_right, c_root = frame_ref.closed_form(n)
        assert root == c_root and np.array_equal(left, c_left) and np.array_equal(right, c_right), (family, n)
        if n:
            assert np.array_equal(np.sort(node_kp), np.arange(n))


def test_levels_is_the_height_of_the_tree():
    for n in range(1, 600):
        left, right, root = frame_ref.closed_form(n)
        depth, front = 0, [root]
        while front:
            depth += 1
            front = [c for v in front for c in (left[v], right[v]) if c >= 0]
        assert depth == frame_ref.levels(n), n


def test_ordered_key_agrees_with_float_compare():
    tiny = np.float32(1.401298464324817e-45)
    fmax = np.finfo(np.float32).max
    t = np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, -3 * tiny, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny,
                  1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), 1919.5, 1e6, -1e6, fmax, -fmax, np.inf, -np.inf,
                  0.5, -0.5, 17.25], np.float32)
    k = frame_ref.ordered_key(t)
    lt, eq = t[:, None] < t[None, :], t[:, None] == t[None, :]
    assert np.array_equal(k[:, None] < k[None, :], lt)
    assert np.array_equal(k[:, None] == k[None, :], eq)
    rng = np.random.default_rng(5)
    r = rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[np.isfinite(r)]
    k = frame_ref.ordered_key(r)
    assert np.array_equal(k[:, None] < k[None, :], r[:, None] < r[None, :])
    assert np.array_equal(k[:, None] == k[None, :], r[:, None] == r[None, :])


def test_ranks_are_permutations_even_with_nan():
    kp = keypoints("uniform", 300)
    kp[::7, 0] = np.nan
    kp[3::11, 1] = -np.nan
    kp[5::13] = np.inf
    rx, ry = frame_ref.ranks(kp)
    assert np.array_equal(np.sort(rx), np.arange(300)) and np.array_equal(np.sort(ry), np.arange(300))
    node_kp = frame_ref.build(kp)[0]
    assert np.array_equal(np.sort(node_kp), np.arange(300))


def test_pack_layout():
    kp = keypoints("uniform", 65)
    node_kp, left, right, _ = frame_ref.build(kp)
    b = frame_ref.pack(kp, node_kp, left, right)
    assert b.nbytes == 20 * 65
    q = b[:16 * 65].view(np.int32).reshape(65, 4)
    assert np.array_equal(q[:, :2].view(np.float32), kp[node_kp]) and np.array_equal(q[:, 2], left) and np.array_equal(q[:, 3], right)
    assert np.array_equal(b[16 * 65:].view(np.int32), node_kp)


def test_gather_counts_follow_the_describer_clamp():
    assert frame_ref.gather_counts(5, 7, 100) == (5, 7)
    assert frame_ref.gather_counts(500, 7, 100) == (100, 0)
    assert frame_ref.gather_counts(-3, 700, 100) == (0, 100)
    assert frame_ref.gather_counts(None, -1, 100) == (0, 0)
    assert frame_ref.gather_counts(60, 60, 100) == (60, 40)
