"""Independent high-precision checks of the absolute-pose stage.  Shares no code with tests/pnp_ref.py (the restatement
that csrc/pnp.hip follows operation by operation) and none with essential_ref.real_roots, so a bug the two have in common
still fails here.

  p3p_hp           every P3P pose of one triple's f64 inputs, by mpmath at 50 digits: the two quadrics in
                   (u, v) = (s2 / s1, s3 / s1) that the cosine laws give, u eliminated by their Sylvester resultant (not
                   by the substitution u = N(v) / D(v) of the restatement), u from the quadratic itself, the pose by
                   Kabsch / SVD over the two triangles and their normals
  rotation_checks  max |R R^T - I| and det R - 1 of a model, f64
  reproj_count     a literal f64 inlier count of a model over f32 points and pixels, K and a threshold
  lsq_optimum      the RMS reprojection error at scipy's least-squares optimum over a given set of points
"""
import functools
import math

import mpmath
import numpy as np

DPS = 50
IMAG_TOL = 1e-7          # a root with |Im v| <= IMAG_TOL (1 + |v|) counts as real: a double root of exact data that the
                         # f64 inputs split into a complex pair sqrt(1e-16) apart.  Such a root is never "isolated".
ISOLATED = 1e-3          # a model is isolated when its root's gap to every other root is >= ISOLATED (1 + |v|)


def _mp(v):
    return mpmath.mpf(float(v))


def _pmul(a, b):
    out = [mpmath.mpf(0)] * (len(a) + len(b) - 1)
    for i, p in enumerate(a):
        for j, q in enumerate(b):
            out[i + j] = out[i + j] + p * q
    return out


def _padd(a, b, sb=1):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else 0) + sb * (b[i] if i < len(b) else 0) for i in range(n)]


def _kabsch(W, C):
    """R, t with C_i = R W_i + t for the two triangles W, C ([3] of mp 3-vectors): SVD of the correlation of the centred
    points and of the unit normals (three points span a plane; the normals fix the out-of-plane sign)."""
    cw = [sum(W[i][k] for i in range(3)) / 3 for k in range(3)]
    cc = [sum(C[i][k] for i in range(3)) / 3 for k in range(3)]

    def normal(T):
        a = [T[1][k] - T[0][k] for k in range(3)]
        b = [T[2][k] - T[0][k] for k in range(3)]
        n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        ln = mpmath.sqrt(sum(q * q for q in n))
        return [q / ln for q in n]

    A = [[W[i][k] - cw[k] for k in range(3)] for i in range(3)] + [normal(W)]
    B = [[C[i][k] - cc[k] for k in range(3)] for i in range(3)] + [normal(C)]
    H = mpmath.matrix(3, 3)
    for a in range(3):
        for b in range(3):
            H[a, b] = sum(B[i][a] * A[i][b] for i in range(4))
    U, _, Vt = mpmath.svd_r(H)
    D = mpmath.diag([1, 1, mpmath.det(U * Vt)])
    R = U * D * Vt
    t = [cc[i] - sum(R[i, k] * cw[k] for k in range(3)) for i in range(3)]
    return [float(R[i, k]) for i in range(3) for k in range(3)], [float(q) for q in t]


def p3p_hp(P, x, y):
    """One triple: P [3][3] world points, x, y [3] normalised image coordinates (the f64 values taken exactly).  Returns
    [(model [12] f64 row-major [R | t], gap, v)] in ascending v: every pose with positive depths, gap = the distance of
    its root v to the nearest other root of the quartic, real or complex, over (1 + |v|).  [] for a degenerate triple."""
    return _p3p_hp(np.asarray(P, np.float64).tobytes(), np.asarray(x, np.float64).tobytes(),
                   np.asarray(y, np.float64).tobytes())


@functools.lru_cache(maxsize=1 << 16)
def _p3p_hp(Pb, xb, yb):
    P = np.frombuffer(Pb, np.float64).reshape(3, 3)
    x, y = np.frombuffer(xb, np.float64), np.frombuffer(yb, np.float64)
    with mpmath.workdps(DPS):
        W = [[_mp(q) for q in p] for p in P]
        jv = []
        for k in range(3):
            v = [_mp(x[k]), _mp(y[k]), mpmath.mpf(1)]
            ln = mpmath.sqrt(v[0] * v[0] + v[1] * v[1] + 1)
            jv.append([q / ln for q in v])
        dist2 = lambda a, b: sum((W[a][k] - W[b][k]) ** 2 for k in range(3))       # noqa: E731
        cosv = lambda a, b: sum(jv[a][k] * jv[b][k] for k in range(3))             # noqa: E731
        a2, b2, c2 = dist2(1, 2), dist2(0, 2), dist2(0, 1)
        ca, cb, cg = cosv(1, 2), cosv(0, 2), cosv(0, 1)
        if a2 == 0 or b2 == 0 or c2 == 0:
            return []
        d21, d31 = [W[1][k] - W[0][k] for k in range(3)], [W[2][k] - W[0][k] for k in range(3)]
        cr = [d21[1] * d31[2] - d21[2] * d31[1], d21[2] * d31[0] - d21[0] * d31[2], d21[0] * d31[1] - d21[1] * d31[0]]
        if sum(q * q for q in cr) <= mpmath.mpf(10) ** (-12) * b2 * c2:       # collinear to 1e-6: no pose is defined
            return []
        den = [mpmath.mpf(1), -2 * cb, mpmath.mpf(1)]                    # 1 - 2 cos(beta) v + v^2 = b2 / s1^2
        # E1: b2 (u^2 + v^2 - 2 u v ca) = a2 den        E2: b2 (1 + u^2 - 2 u cg) = c2 den      (both A u^2 + B u + C)
        B1, C1 = [mpmath.mpf(0), -2 * b2 * ca], _padd([0, 0, b2], [a2 * q for q in den], -1)
        B2, C2 = [-2 * b2 * cg], _padd([b2], [c2 * q for q in den], -1)
        ac = [b2 * q for q in _padd(C2, C1, -1)]                         # A C' - A' C
        ab = [b2 * q for q in _padd(B2, B1, -1)]                         # A B' - A' B
        bc = _padd(_pmul(B1, C2), _pmul(B2, C1), -1)                     # B C' - B' C
        res = _padd(_pmul(ac, ac), _pmul(ab, bc), -1)                    # the resultant: a quartic in v
        while res and res[-1] == 0:
            res.pop()
        if len(res) < 2:
            return []
        roots = mpmath.polyroots(res[::-1], maxsteps=2000, extraprec=4 * DPS)
        out = []
        for i, z in enumerate(roots):
            im = abs(mpmath.im(z)) / (1 + abs(z))
            if im > IMAG_TOL:
                continue
            v = mpmath.re(z)
            if not v > 0:
                continue
            gap = min([abs(z - w) for j, w in enumerate(roots) if j != i] or [mpmath.inf]) / (1 + abs(v))
            dv = (v * v - 2 * cb * v) + 1
            if not dv > 0:
                continue
            # u from E2, kept when it also satisfies E1 (to the precision that the root itself has)
            c0 = 1 - c2 * dv / b2
            disc = cg * cg - c0
            tol = mpmath.mpf(10) ** (-25) + 100 * im + (mpmath.mpf(10) ** (-20) if gap < mpmath.mpf(10) ** (-10) else 0)
            if disc < 0:
                if disc < -1e-12:
                    continue
                disc = mpmath.mpf(0)
            sq = mpmath.sqrt(disc)
            for u in ((cg - sq, cg + sq) if sq > 0 else (cg,)):
                if not u > 0:
                    continue
                e1 = b2 * ((u * u + v * v) - 2 * u * v * ca) - a2 * dv
                if abs(e1) > tol * (b2 * ((u * u + v * v) + 2 * abs(u * v * ca)) + a2 * dv):
                    continue
                s1 = mpmath.sqrt(b2 / dv)
                s = (s1, u * s1, v * s1)
                C = [[s[k] * q for q in jv[k]] for k in range(3)]
                R, t = _kabsch(W, C)
                m = np.array([R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]])
                out.append((m, float(gap), float(v)))
        out.sort(key=lambda q: q[2])
        return out


def model_dist(a, b):
    """max |a - b| / max(1, max |b|) of two models [12]."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def rotation_checks(m):
    """(max |R R^T - I|, det R - 1) of model m [12]."""
    R = np.asarray(m, np.float64).reshape(3, 4)[:, :3]
    return float(np.abs(R @ R.T - np.eye(3)).max()), float(np.linalg.det(R) - 1.0)


def reproj_sq(m, obj, pix, K):
    """(depth [n], squared reprojection error in pixels [n]) of model m [12] over f32 points and pixels, f64."""
    M = np.asarray(m, np.float64).reshape(3, 4)
    fx, fy, cx, cy = (float(k) for k in K)
    W = np.asarray(obj, np.float32).reshape(-1, 3).astype(np.float64)
    p = np.asarray(pix, np.float32).reshape(-1, 2).astype(np.float64)
    Xc = W @ M[:, :3].T + M[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        du = (fx * Xc[:, 0] / Xc[:, 2] + cx) - p[:, 0]
        dv = (fy * Xc[:, 1] / Xc[:, 2] + cy) - p[:, 1]
    return Xc[:, 2], du * du + dv * dv


def reproj_count(m, obj, pix, K, thr):
    """(count, near): the points with positive depth whose squared reprojection error is < thr^2, and how many points lie
    within 1e-9 relative of thr^2 (where rounding may decide either way).  A non-finite point never counts."""
    z, e2 = reproj_sq(m, obj, pix, K)
    t2 = float(thr) * float(thr)
    with np.errstate(invalid="ignore"):
        return int(np.sum((z > 0.0) & (e2 < t2))), int(np.sum(np.abs(e2 - t2) <= 1e-9 * t2))


def lsq_optimum(obj, pix, K, pose, select=None):
    """The RMS reprojection error (pixels, over both coordinates of each point) at scipy's least-squares optimum over the
    points `select` (a mask; default all), started at pose [4][4] or [12].  f32 inputs taken exactly, f64 arithmetic."""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    fx, fy, cx, cy = (float(k) for k in K)
    W = np.asarray(obj, np.float32).reshape(-1, 3).astype(np.float64)
    p = np.asarray(pix, np.float32).reshape(-1, 2).astype(np.float64)
    if select is not None:
        W, p = W[np.asarray(select, bool)], p[np.asarray(select, bool)]
    x, y = (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy
    M = np.asarray(pose, np.float64).ravel()[:12].reshape(3, 4)

    def f(q):
        Xc = W @ Rotation.from_rotvec(q[:3]).as_matrix().T + q[3:]
        return np.concatenate([fx * (Xc[:, 0] / Xc[:, 2] - x), fy * (Xc[:, 1] / Xc[:, 2] - y)])

    q0 = np.concatenate([Rotation.from_matrix(M[:, :3]).as_rotvec(), M[:, 3]])
    r = least_squares(f, q0, xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return math.sqrt(float((r.fun ** 2).sum() / len(x)))
