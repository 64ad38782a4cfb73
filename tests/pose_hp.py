"""Independent high-precision checks of the relative-pose stage.  Shares no code with tests/essential_ref.py (the
restatement that csrc/pose.hip follows operation by operation), so a bug the two have in common still fails here.

  real_roots_hp      the real roots of a degree-10 polynomial of f64 coefficients, by mpmath.polyroots at 50 digits
  essential_checks   scale-free det E, the cubic 2 E E^T E - tr(E E^T) E and the epipolar residuals of given points, f64
  sampson_count      a literal f64 inlier count of E over pixels, threshold and K
  refit_translation  the known-rotation refit t: the last right singular vector of np.linalg.svd of the inlier
                     constraint stack (what the reference's JacobiSVD computes; the kernel takes the smallest eigenvector
                     of the normal matrix instead)
  true_E             [t]x R of a ground-truth motion, unit norm
"""
import mpmath
import numpy as np

DPS = 50
IMAG_TOL = 1e-9          # a root with |Im z| <= IMAG_TOL (1 + |z|) is real
CLUSTER_GAP = 1e-6       # roots closer than this relative gap form a cluster (f64 coefficients cannot separate them)


def real_roots_hp(coeffs_asc):
    """[(root, in_cluster)] ascending: the real roots of sum c_k z^k (the f64 values taken exactly).  in_cluster: another
    root of the polynomial, real or complex, lies within CLUSTER_GAP (1 + |z|)."""
    c = [float(v) for v in coeffs_asc]
    while c and c[-1] == 0.0:
        c.pop()
    if len(c) < 2:
        return []
    with mpmath.workdps(DPS):
        allr = [complex(r) for r in mpmath.polyroots([mpmath.mpf(v) for v in c[::-1]], maxsteps=800, extraprec=400)]
    out = []
    for i, r in enumerate(allr):
        if abs(r.imag) <= IMAG_TOL * (1.0 + abs(r)):
            near = any(j != i and abs(allr[j] - r) <= CLUSTER_GAP * (1.0 + abs(r)) for j in range(len(allr)))
            out.append((r.real, near))
    return sorted(out)


def match_roots(found, coeffs_asc, rel=1e-6):
    """(spurious, missed) of found real roots against real_roots_hp: a found root with no true real root within rel,
    and a true real root outside a cluster with no found root within rel."""
    hp = real_roots_hp(coeffs_asc)
    close = lambda a, b: abs(a - b) <= rel * (1.0 + abs(b))      # noqa: E731
    spurious = sum(not any(close(f, r) for r, _ in hp) for f in found)
    missed = sum(not any(close(f, r) for f in found) for r, cl in hp if not cl)
    return spurious, missed


def essential_checks(E, x1=None, y1=None, x2=None, y2=None):
    """(|det E| / |E|^3, max |2 E E^T E - tr(E E^T) E| / |E|^3, max |x2^T E x1| / |E| over the given points)."""
    M = np.asarray(E, np.float64).reshape(3, 3)
    n = np.linalg.norm(M)
    det = abs(np.linalg.det(M)) / n ** 3
    cubic = np.abs(2.0 * M @ M.T @ M - np.trace(M @ M.T) * M).max() / n ** 3
    epi = 0.0
    if x1 is not None:
        a = np.stack([x1, y1, np.ones_like(x1)], -1)
        b = np.stack([x2, y2, np.ones_like(x2)], -1)
        epi = np.abs(np.einsum("ki,ij,kj->k", b, M, a)).max() / n
    return det, cubic, epi


def normalised(pix, K):
    fx, fy, cx, cy = (float(k) for k in K)
    p = np.asarray(pix, np.float32).astype(np.float64)
    return (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy


def sampson_sq(E, pix_from, pix_to, K):
    """Squared Sampson distance of every match in normalised coordinates (NaN for a non-finite point or a vanishing
    denominator)."""
    M = np.asarray(E, np.float64).reshape(3, 3)
    x1, y1 = normalised(pix_from, K)
    x2, y2 = normalised(pix_to, K)
    a = np.stack([x1, y1, np.ones_like(x1)], -1)
    b = np.stack([x2, y2, np.ones_like(x2)], -1)
    Ea, Etb = a @ M.T, b @ M
    num = np.einsum("ki,ki->k", b, Ea) ** 2
    den = Ea[:, 0] ** 2 + Ea[:, 1] ** 2 + Etb[:, 0] ** 2 + Etb[:, 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return num / den


def sampson_count(E, pix_from, pix_to, K, threshold_px):
    """(count, near): matches with squared Sampson distance < (threshold / mean focal)^2, and how many lie within 1e-9
    relative of that bound (where rounding may decide either way)."""
    t = threshold_px / ((float(K[0]) + float(K[1])) / 2.0)
    err = sampson_sq(E, pix_from, pix_to, K)
    return int(np.sum(err < t * t)), int(np.sum(np.abs(err - t * t) <= 1e-9 * t * t))


def refit_translation(pix_from, pix_to, K, R, inlier):
    """Unit t minimising |C t| for the stack C of the inliers' constraints (R f) x g, f64, by np.linalg.svd."""
    fx, fy, cx, cy = (float(k) for k in K)
    pf = np.asarray(pix_from, np.float64)[np.asarray(inlier, bool)]
    pt = np.asarray(pix_to, np.float64)[np.asarray(inlier, bool)]
    f = np.stack([(pf[:, 0] - cx) / fx, (pf[:, 1] - cy) / fy, np.ones(len(pf))], -1)
    g = np.stack([(pt[:, 0] - cx) / fx, (pt[:, 1] - cy) / fy, np.ones(len(pt))], -1)
    C = np.cross(f @ np.asarray(R, np.float64).T, g)
    return np.linalg.svd(C)[2][-1]


def true_E(R, t):
    t = np.asarray(t, np.float64)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    E = (tx @ np.asarray(R, np.float64)).ravel()
    return E / np.linalg.norm(E)


def dist_up_to_sign(a, b):
    """max |a - b| or max |a + b| of a, b scaled to unit norm, the smaller."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return min(np.abs(a - b).max(), np.abs(a + b).max())
